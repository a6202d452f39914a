"""Plain restatement of the track match policy (track match policy), for the tests.

Everything that is not the match is tests/track_readout_ref.py's and tests/track_motion_ref.py's, reused as it stands: the
prediction, the velocity update on the stored box, hits, gaps, the rebuild, the capacity cut and the read-out.  The match
of a frame is restated here in two steps.

  * CANDIDATES.  Pairs (i, j): box i of the frame in decode order, table entry j with age <= max_age; without ANY_LABEL
    the labels must be equal, with it they are not compared.  The pair's value is bbox_iou(box i, predicted box of entry
    j) as float32, and only pairs with value >= thr are candidates.
  * ORDER.  Without BEST_FIRST the boxes are visited in decode order and each takes its unclaimed candidate entry with the
    largest value, ties to the lowest j.  With BEST_FIRST the candidate pair with the largest value is taken repeatedly,
    ties to the lowest i, then the lowest j; box i claims entry j and every candidate of box i and of entry j leaves the set.
  * IDS.  After the match the boxes that claimed nothing open new ids in decode order.

Everything is a Python list walked one element at a time, with np.float32 around every single operation; the IoU is
orc.bbox_iou, so its float32 bits are the oracle's.  Test infrastructure only.
"""
import numpy as np

from oracle import oracle as orc

from track_readout_ref import CASES, KEYS, TrackMotion, TrackReadout, _join, moving_boxes      # noqa: F401

f32 = np.float32
MATCH_BEST_FIRST, MATCH_ANY_LABEL = 1, 2


class TrackMatch(TrackMotion):
    """TrackMotion with the match of a frame chosen by `match` (an attribute: it belongs to the call, not to the table)"""

    def __init__(self, tcap, thr, gain, match=0):
        TrackMotion.__init__(self, tcap, thr, gain)
        assert 0 <= int(match) <= 3
        self.match = int(match)
        self.ties = 0            # frames so far in which two candidates sharing a box or an entry had equal IoU

    def candidates(self, rows, max_age):
        """{(i, j): IoU as float32} of the frame"""
        thr32 = f32(self.thr)
        cand = {}
        for i, r in enumerate(rows):
            for j, (box, lab, _, age, vx, vy) in enumerate(self.table):
                if age > max_age:
                    continue
                if not (self.match & MATCH_ANY_LABEL) and f32(lab) != f32(r[5]):
                    continue
                k = f32(age + 1)
                px = f32(f32(box[0]) + f32(k * f32(vx)))
                py = f32(f32(box[1]) + f32(k * f32(vy)))
                pred = np.array([px, py, box[2], box[3]], dtype=np.float32)
                iou = f32(orc.bbox_iou(r[:4], pred))
                if iou >= thr32:
                    cand[(i, j)] = iou
        return cand

    def frame(self, rows, max_age, gain=None):
        """rows: the frame's boxes [n, 8] in decode order -> (ids, gaps), lists of n"""
        g = f32(self.gain if gain is None else gain)
        cand = self.candidates(rows, max_age)
        if shared_tie(cand):
            self.ties += 1
        pair = {}                # box -> entry
        if self.match & MATCH_BEST_FIRST:
            left = dict(cand)
            while left:
                best = None
                for (i, j) in sorted(left):                 # ascending i, then j: a strict comparison keeps the first
                    if best is None or left[(i, j)] > left[best]:
                        best = (i, j)
                pair[best[0]] = best[1]
                left = {p: v for p, v in left.items() if p[0] != best[0] and p[1] != best[1]}
        else:
            claimed = set()
            for i in range(len(rows)):
                best = None
                for j in range(len(self.table)):
                    if (i, j) in cand and j not in claimed and (best is None or cand[(i, j)] > cand[(i, best)]):
                        best = j
                if best is not None:
                    pair[i] = best
                    claimed.add(best)
        ids, gaps, vels = [], [], []
        for i, r in enumerate(rows):
            if i in pair:
                box, _, tid, age, vx, vy = self.table[pair[i]]
                k = f32(age + 1)
                ox = f32(f32(f32(r[0]) - f32(box[0])) / k)
                oy = f32(f32(f32(r[1]) - f32(box[1])) / k)
                nvx = f32(f32(vx) + f32(g * f32(ox - f32(vx))))
                nvy = f32(f32(vy) + f32(g * f32(oy - f32(vy))))
                ids.append(tid); gaps.append(age); vels.append((nvx, nvy))
            else:
                ids.append(self.next_id); gaps.append(-1); vels.append((f32(0), f32(0)))
                self.next_id += 1
        claimed = set(pair.values())
        new = [[np.array(r[:4], dtype=np.float32), f32(r[5]), i, 0, v[0], v[1]] for r, i, v in zip(rows, ids, vels)]
        for j, (box, lab, tid, age, vx, vy) in enumerate(self.table):
            if j not in claimed and age + 1 <= max_age:
                new.append([box, lab, tid, age + 1, vx, vy])
        self.dropped += max(0, len(new) - self.tcap)
        self.table = new[:self.tcap]
        return ids, gaps


def shared_tie(cand):
    """whether two candidate pairs that share a box or an entry have equal IoU"""
    by_box, by_entry = {}, {}
    for (i, j), v in cand.items():
        by_box.setdefault(i, []).append(v)
        by_entry.setdefault(j, []).append(v)
    for vals in list(by_box.values()) + list(by_entry.values()):
        bits = [int(np.array(v, dtype=np.float32).view(np.uint32)) for v in vals]
        if len(set(bits)) != len(bits):
            return True
    return False


class TrackMatchReadout(TrackReadout):
    """TrackReadout over a TrackMatch table"""

    def __init__(self, tcap, thr, gain, min_hits, match=0):
        TrackReadout.__init__(self, tcap, thr, gain, min_hits)
        self.tm = TrackMatch(tcap, thr, gain, match)


def associate_tracks_match(boxes, counts, thr, max_age, gain, min_hits, match, tcap=None):
    """the stateless call on one clip -> dict of KEYS (arrays without the clip axis, nids an int), `dropped`, and `ties`: the
    frames in which two candidates sharing a box or an entry had equal IoU"""
    tr = TrackMatchReadout(boxes.shape[1] if tcap is None else tcap, thr, gain, min_hits, match)
    r = _join([tr.clip(boxes, counts, max_age)], tr)
    r["ties"] = tr.tm.ties
    return r


def associate_tracks_match_chunked(boxes, counts, thr, max_age, gain, min_hits, match, tcap, chunks, motion_at=()):
    """the same through one carried state fed in chunks along T; match an int, or one per chunk: the policy switches at the
    chunk boundaries and nothing else does.  A chunk whose index is in motion_at stands for a call of dt_associate_stream_motion
    (track_readout_ref.associate_tracks_chunked's): today's match whatever `match` says there, the hits forgotten afterwards,
    no hits and no read-out from it: -1 / 0 in the result."""
    ms = [int(match)] * len(chunks) if np.isscalar(match) else [int(m) for m in match]
    assert len(ms) == len(chunks)
    tr = TrackMatchReadout(tcap, thr, gain, min_hits, ms[0])
    parts, t0 = [], 0
    for c, (L, m) in enumerate(zip(chunks, ms)):
        tr.tm.match = 0 if c in motion_at else m
        p = tr.clip(boxes[t0:t0 + L], counts[t0:t0 + L], max_age)
        if c in motion_at:
            tr.forget_hits()
            p["hits"][:] = -1; p["tracks"][:] = 0; p["track_info"][:] = -1; p["track_counts"][:] = 0
            p["table"] = [[] for _ in p["table"]]
        parts.append(p)
        t0 += L
    assert t0 == boxes.shape[0]
    r = _join(parts, tr)
    r["ties"] = tr.tm.ties
    return r


def moving_boxes_gt(T, cap, n_obj_t, seed, duplicates=True):
    """moving_boxes with the same draws -> (boxes, counts, obj [T, cap]: the generator's object index of every box, -1 in
    unused entries).  duplicates=False leaves out the generator's exact-duplicate line (the draws stay the same)."""
    rs = np.random.RandomState(seed)
    n_max = max(n_obj_t(t) for t in range(T))
    pos = rs.rand(n_max, 2); vel = (rs.rand(n_max, 2) - .5) * .06; wh = rs.rand(n_max, 2) * .2 + .05
    lab = rs.randint(0, 3, n_max)
    boxes = np.zeros((T, cap, 8), dtype=np.float32)
    counts = np.zeros(T, dtype=np.int32)
    obj = np.full((T, cap), -1, dtype=np.int32)
    for t in range(T):
        alive = [k for k in range(n_obj_t(t)) if rs.rand() > 0.15]
        rs.shuffle(alive)
        for i, k in enumerate(alive[:cap]):
            p = pos[k] + vel[k] * t
            boxes[t, i] = [p[0], p[1], wh[k, 0], wh[k, 1], .9, lab[k] if rs.rand() > .05 else (lab[k] + 1) % 3, .8, i]
            obj[t, i] = k
        counts[t] = min(len(alive), cap)
        if duplicates and t % 5 == 3 and counts[t] >= 2:
            boxes[t, 1, :4] = boxes[t, 0, :4]      # exact duplicate -> tie on IoU
    return boxes, counts, obj


def identity_switches(ids, counts, obj):
    """frames in which an object of the generator appears under another id than at its previous appearance"""
    last, n = {}, 0
    for t in range(ids.shape[0]):
        for i in range(min(int(counts[t]), ids.shape[1])):
            k, tid = int(obj[t, i]), int(ids[t, i])
            if k in last and last[k] != tid:
                n += 1
            last[k] = tid
    return n


def permute_frames(boxes, counts, seed):
    """every frame's boxes shuffled among themselves (the rows as they are, field 7 included)"""
    rs = np.random.RandomState(seed)
    out = boxes.copy()
    for t in range(boxes.shape[0]):
        n = min(int(counts[t]), boxes.shape[1])
        out[t, :n] = boxes[t, rs.permutation(n)]
    return out


def partition(ids, boxes, counts):
    """the tracks of a run as a set of sets of (frame, box row bytes): what must not depend on the order of a frame's boxes"""
    tracks = {}
    for t in range(ids.shape[0]):
        for i in range(min(int(counts[t]), ids.shape[1])):
            tracks.setdefault(int(ids[t, i]), set()).add((t, boxes[t, i].tobytes()))
    return set(frozenset(v) for v in tracks.values())


# the scenes of the permutation tests: (T, cap, objects per frame, tcap) at seed 7 -- both kernel forms, no drop at these tcap
PERMUTATION_SCENES = {
    "general_form": (40, 64, 30, 128),
    "general_form_dense": (8, 128, 140, 512),
    "register_form": (40, 32, 12, 64),
}
