"""StreamTable -- which stream lives in which slot (addition; no reference counterpart).

The device keeps per-slot state (mi355_dt.Context.stream_open); callers think in
stream keys such as camera names.  This is the bookkeeping between the two, pure
Python: open a key, look its slot up, release it (the slot is reset and handed
to the next key that opens).

    table = StreamTable(tracker, n_slots=8)
    table.open("gate-3")
    res = tracker.track_stream(frames, table.slots(["gate-3"]))
    table.release("gate-3")

`tracker` is anything with open_streams(n_slots, cap) and reset_streams(slots)
-- a MultiObjDetTracker, a TinyTracker or a TinyHeatmapTracker (their slots hold
the per-object LSTM state; `cap` means nothing to them and is ignored) -- or
None for bookkeeping alone.
"""


class StreamTableError(KeyError):
    def __str__(self):      # KeyError would show the repr of the message
        return str(self.args[0]) if self.args else ""


class StreamTable(object):
    def __init__(self, tracker=None, n_slots=1, cap=None):
        if n_slots <= 0:
            raise ValueError("n_slots must be positive, got %r" % (n_slots,))
        self.tracker = tracker
        self.n_slots = int(n_slots)
        self._slot = {}                                   # key -> slot
        self._free = list(range(self.n_slots - 1, -1, -1))   # popped from the end: lowest number first
        if tracker is not None:
            tracker.open_streams(self.n_slots, cap=cap)

    def __len__(self):
        return len(self._slot)

    def __contains__(self, key):
        return key in self._slot

    def keys(self):
        return sorted(self._slot, key=self._slot.get)

    def open(self, key):
        """Give `key` a fresh slot and return its number."""
        if key in self._slot:
            raise StreamTableError("stream %r is already open (slot %d)" % (key, self._slot[key]))
        if not self._free:
            raise StreamTableError("no free slot for stream %r: all %d are in use (%s)" % (
                key, self.n_slots, ", ".join(repr(k) for k in self.keys())))
        s = self._free.pop()
        self._slot[key] = s
        return s

    def slot(self, key):
        try:
            return self._slot[key]
        except KeyError:
            raise StreamTableError("unknown stream %r (open: %s)" % (key, ", ".join(repr(k) for k in self.keys()) or "none"))

    def slots(self, keys):
        """Slot numbers of `keys`, in order: the `slots` argument of track_stream."""
        out = [self.slot(k) for k in keys]
        if len(set(out)) != len(out):
            raise StreamTableError("a stream is named twice in %r" % (list(keys),))
        return out

    def release(self, key):
        """Close `key`: its slot is reset on the device and becomes free (lowest free number is reused first)."""
        s = self.slot(key)
        if self.tracker is not None:
            self.tracker.reset_streams([s])
        del self._slot[key]
        self._free.append(s)
        self._free.sort(reverse=True)
        return s
