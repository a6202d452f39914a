"""Plain restatement of the track read-out (track read-out), for the tests.

The match, the velocity update, the rebuild and the capacity cut are tests/track_motion_ref.py's TrackMotion, reused as it
stands, so ids, nids and gaps cannot drift from it.  On top of it:

  * HITS.  Every table entry carries `hits`, the frames in which its track had a box: a box that opens a new id starts at 1, a
    box that claims entry j carries hits_j + 1, an unclaimed survivor keeps its hits.  The hits are kept here by track id (an id
    is in the table at most once) and dropped with the entries that leave the table.
  * READ-OUT.  After the frame's rebuild and cut the table is walked in its order -- the frame's boxes in decode order (age 0),
    then the surviving lost tracks -- and every entry with hits >= min_hits becomes one row:
      floats  x, y, w, h, label, vx, vy, 0     age 0: the stored x, y bits; age a >= 1: x + float32(a)*vx, y + float32(a)*vy
                                               (a multiply, then an add, each rounded to float32)
      ints    id, age, hits, box               box = the entry's index among the frame's boxes for age 0, -1 for a coasting entry
    Rows behind the count are zero / -1.

Everything is a Python list walked one element at a time, with np.float32 around every single operation.  Test infrastructure only.
"""
import numpy as np

from track_motion_ref import CASES, TrackMotion, moving_boxes      # noqa: F401  (the cases and the generator are shared)

f32 = np.float32
TRACK_FLOATS, TRACK_INTS = 8, 4
KEYS = ("ids", "nids", "gaps", "hits", "tracks", "track_info", "track_counts")


class TrackReadout(object):
    """the state a stream carries: TrackMotion's, and the hits of the tracks in its table"""

    def __init__(self, tcap, thr, gain, min_hits):
        self.tm = TrackMotion(tcap, thr, gain)
        self.tcap, self.min_hits = int(tcap), int(min_hits)
        assert self.min_hits >= 1
        self.hits = {}           # track id -> hits, for the ids in tm.table

    @property
    def next_id(self):
        return self.tm.next_id

    @property
    def dropped(self):
        return self.tm.dropped

    def forget_hits(self):
        """what a call of dt_associate_stream_motion does to the slot's tracks: every track reads as hits = 1"""
        for e in self.tm.table:
            self.hits[e[2]] = 1

    def forget_velocities(self):
        """what dt_associate_stream / dt_associate_stream_mem do: velocities and hits both forgotten"""
        self.tm.forget_velocities()
        self.forget_hits()

    def frame(self, rows, max_age, gain=None):
        """rows: the frame's boxes [n, 8] in decode order -> (ids, gaps, hits: lists of n; the table after the frame as read-out
        rows, confirmed or not: list of (floats8, ints4))"""
        ids, gaps = self.tm.frame(rows, max_age, gain)
        bh = []
        for i, g in zip(ids, gaps):
            h = 1 if g < 0 else self.hits[i] + 1
            self.hits[i] = h
            bh.append(h)
        self.hits = {e[2]: self.hits[e[2]] for e in self.tm.table}      # entries that left the table take their hits along
        out = []
        for j, (box, lab, tid, age, vx, vy) in enumerate(self.tm.table):
            if age == 0:
                x, y = f32(box[0]), f32(box[1])
            else:
                a = f32(age)
                x = f32(f32(box[0]) + f32(a * f32(vx)))
                y = f32(f32(box[1]) + f32(a * f32(vy)))
            out.append(([x, y, f32(box[2]), f32(box[3]), f32(lab), f32(vx), f32(vy), f32(0)],
                        [tid, age, self.hits[tid], j if age == 0 else -1]))
        return ids, gaps, bh, out

    def clip(self, boxes, counts, max_age, gain=None):
        """boxes [T, cap, 8], counts [T]; max_age an int or one per frame -> dict of the per-frame outputs (KEYS without nids), and
        under `table` the whole table of every frame as rows, confirmed or not (with_min_hits filters it again)"""
        T, cap, _ = boxes.shape
        ages = [int(max_age)] * T if np.isscalar(max_age) else [int(a) for a in max_age]
        assert len(ages) == T
        r = dict(ids=np.full((T, cap), -1, dtype=np.int32), gaps=np.full((T, cap), -1, dtype=np.int32),
                 hits=np.full((T, cap), -1, dtype=np.int32), table=[])
        for t in range(T):
            n = min(int(counts[t]), cap)
            i, g, h, rows = self.frame(boxes[t, :n], ages[t], gain)
            r["ids"][t, :n] = i
            r["gaps"][t, :n] = g
            r["hits"][t, :n] = h
            r["table"].append(rows)
        r.update(read_out(r["table"], self.min_hits, self.tcap))
        return r


def read_out(table, min_hits, tcap):
    """the rows of every frame's table with hits >= min_hits, compacted in table order; zero / -1 behind the count"""
    T = len(table)
    tracks = np.zeros((T, tcap, TRACK_FLOATS), dtype=np.float32)
    info = np.full((T, tcap, TRACK_INTS), -1, dtype=np.int32)
    tcounts = np.zeros(T, dtype=np.int32)
    for t, rows in enumerate(table):
        assert len(rows) <= tcap
        k = 0
        for fl, it in rows:
            if it[2] >= min_hits:
                tracks[t, k] = fl
                info[t, k] = it
                k += 1
        tcounts[t] = k
    return dict(tracks=tracks, track_info=info, track_counts=tcounts)


def with_min_hits(res, min_hits):
    """a stateless result for another min_hits: the match does not depend on it, only the read-out is filtered again"""
    r = dict(res)
    r.update(read_out(res["table"], min_hits, res["tracks"].shape[1]))
    return r


def _join(parts, tr):
    r = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "table"}
    r["table"] = [rows for p in parts for rows in p["table"]]
    r["nids"] = tr.next_id
    r["dropped"] = tr.dropped
    return r


def associate_tracks(boxes, counts, thr, max_age, gain, min_hits, tcap=None):
    """the stateless call on one clip -> dict of KEYS (arrays without the clip axis, nids an int) and `dropped`"""
    tr = TrackReadout(boxes.shape[1] if tcap is None else tcap, thr, gain, min_hits)
    return _join([tr.clip(boxes, counts, max_age)], tr)


def associate_tracks_chunked(boxes, counts, thr, max_age, gain, min_hits, tcap, chunks, motion_at=(), plain_at=()):
    """the same through one carried state fed in chunks along T.  A chunk whose index is in motion_at stands for a call of
    dt_associate_stream_motion: the match goes on as it is and afterwards the tracks have forgotten their hits.  One in plain_at
    stands for dt_associate_stream_mem (or, with max_age an array holding 0 there, dt_associate_stream): velocities forgotten,
    the chunk runs with gain 0, hits forgotten afterwards.  Those chunks have no hits and no read-out: -1 / 0 in the result."""
    tr = TrackReadout(tcap, thr, gain, min_hits)
    parts, t0 = [], 0
    for c, L in enumerate(chunks):
        a = max_age if np.isscalar(max_age) else max_age[t0:t0 + L]
        b, n = boxes[t0:t0 + L], counts[t0:t0 + L]
        if c in plain_at or c in motion_at:
            if c in plain_at:
                tr.forget_velocities()
            p = tr.clip(b, n, a, gain=0.0 if c in plain_at else None)
            tr.forget_hits()
            p["hits"][:] = -1; p["tracks"][:] = 0; p["track_info"][:] = -1; p["track_counts"][:] = 0
            p["table"] = [[] for _ in p["table"]]
        else:
            p = tr.clip(b, n, a)
        parts.append(p)
        t0 += L
    assert t0 == boxes.shape[0]
    return _join(parts, tr)
