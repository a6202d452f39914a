"""Plain restatement of the track assignment (track assignment), for the tests.

Everything that is not the match is tests/track_match_ref.py's and the files it reuses: the candidates, the prediction, the
velocity update on the stored box, hits, gaps, the rebuild, the capacity cut and the read-out.  The match of a frame:

  * CANDIDATES.  TrackMatch.candidates(rows, max_age) as it stands: {(i, j): IoU as float32}.
  * WEIGHTS.  W [n][nt] of integers over all n boxes and all nt table entries: a candidate weighs
    1 + int(float32(iou * float32(1048576))) (the product is exact, the conversion truncates), every other pair 0.
  * MATCH.  The pairs are row_to_col of identity_score_ref.assign_max(W): the solver's restatement, step for step.
  * IDS.  The tail is TrackMatch.frame's: a claiming box inherits id, gap and the velocity update, the others open ids in
    decode order at rest.

Everything is a Python list walked one element at a time, with np.float32 around every single operation.  Test
infrastructure only.
"""
import numpy as np

import identity_score_ref as isr
import track_match_ref as tmr
from track_readout_ref import CASES, KEYS, TrackReadout, _join, moving_boxes, with_min_hits      # noqa: F401

f32 = np.float32
MATCH_BEST_FIRST, MATCH_ANY_LABEL = tmr.MATCH_BEST_FIRST, tmr.MATCH_ANY_LABEL
ASSIGN_IOU_SCALE = 1048576


def weight(iou):
    """the integer weight of a candidate of IoU `iou` (float32)"""
    return 1 + int(f32(f32(iou) * f32(ASSIGN_IOU_SCALE)))


def weights(cand, n, nt):
    """{(i, j): IoU} -> W [n, nt] int64, 0 where the pair is no candidate"""
    w = np.zeros((n, nt), dtype=np.int64)
    for (i, j), v in cand.items():
        w[i, j] = weight(v)
    return w


def best_first_pairs(cand):
    """the pairs DT_MATCH_BEST_FIRST takes from a frame's candidates (track_match_ref.TrackMatch.frame's loop)"""
    pair, left = {}, dict(cand)
    while left:
        best = None
        for (i, j) in sorted(left):
            if best is None or left[(i, j)] > left[best]:
                best = (i, j)
        pair[best[0]] = best[1]
        left = {p: v for p, v in left.items() if p[0] != best[0] and p[1] != best[1]}
    return pair


class TrackAssign(tmr.TrackMatch):
    """TrackMatch whose frames are matched by the optimal assignment while `assign` is set (an attribute: it belongs to the call).
    `match` holds the label bit only.  log: per assigned frame (n, nt, the optimal pairs' summed weight, best-first's on the same
    table, whether the two sets of pairs differ)."""

    def __init__(self, tcap, thr, gain, match=0, assign=True):
        tmr.TrackMatch.__init__(self, tcap, thr, gain, match)
        self.assign = bool(assign)
        self.log = []

    def frame(self, rows, max_age, gain=None):
        if not self.assign:
            return tmr.TrackMatch.frame(self, rows, max_age, gain)
        assert not (self.match & MATCH_BEST_FIRST)
        g = f32(self.gain if gain is None else gain)
        n, nt = len(rows), len(self.table)
        cand = self.candidates(rows, max_age)
        w = weights(cand, n, nt)
        pair = {}                # box -> entry
        if n and nt:
            r2c, _, total = isr.assign_max(w)
            pair = {i: int(r2c[i]) for i in range(n) if r2c[i] >= 0}
            assert all(p in cand for p in pair.items()) and total == sum(int(w[i, j]) for i, j in pair.items())
        bf = best_first_pairs(cand)
        self.log.append((n, nt, sum(int(w[i, j]) for i, j in pair.items()), sum(int(w[i, j]) for i, j in bf.items()), pair != bf))
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


class TrackAssignReadout(TrackReadout):
    """TrackReadout over a TrackAssign table"""

    def __init__(self, tcap, thr, gain, min_hits, match=0, assign=True):
        TrackReadout.__init__(self, tcap, thr, gain, min_hits)
        self.tm = TrackAssign(tcap, thr, gain, match, assign)


def _finish(r, tr):
    r["log"] = list(tr.tm.log)
    return r


def associate_tracks_assign(boxes, counts, thr, max_age, gain, min_hits, match, tcap=None):
    """the stateless call on one clip -> dict of KEYS (arrays without the clip axis, nids an int), `dropped` and `log`"""
    assert match in (0, MATCH_ANY_LABEL)
    tr = TrackAssignReadout(boxes.shape[1] if tcap is None else tcap, thr, gain, min_hits, match)
    return _finish(_join([tr.clip(boxes, counts, max_age)], tr), tr)


def associate_tracks_assign_chunked(boxes, counts, thr, max_age, gain, min_hits, match, tcap, chunks, match_at=None, motion_at=()):
    """the same through one carried state fed in chunks along T.  A chunk whose index is a key of match_at stands for a call of
    dt_associate_stream_tracks_match with that match; one in motion_at for dt_associate_stream_motion (decode order within a
    label, the hits forgotten afterwards, no hits and no read-out from it: -1 / 0 in the result); every other chunk is the
    assignment with `match`."""
    assert match in (0, MATCH_ANY_LABEL)
    match_at = dict(match_at or {})
    tr = TrackAssignReadout(tcap, thr, gain, min_hits, match)
    parts, t0 = [], 0
    for c, L in enumerate(chunks):
        if c in motion_at:
            tr.tm.assign, tr.tm.match = False, 0
        elif c in match_at:
            tr.tm.assign, tr.tm.match = False, int(match_at[c])
        else:
            tr.tm.assign, tr.tm.match = True, int(match)
        p = tr.clip(boxes[t0:t0 + L], counts[t0:t0 + L], max_age)
        if c in motion_at:
            tr.forget_hits()
            p["hits"][:] = -1; p["tracks"][:] = 0; p["track_info"][:] = -1; p["track_counts"][:] = 0
            p["table"] = [[] for _ in p["table"]]
        parts.append(p)
        t0 += L
    assert t0 == boxes.shape[0]
    return _finish(_join(parts, tr), tr)


# ---------------------------------------------------------------------------------------------------------------- scenes
def crowd_boxes_gt(T, cap, n_obj_t, seed, span):
    """a crowded scene: objects of similar size packed into `span` of the image, two labels -> (boxes, counts, obj [T, cap]: the
    generator's object index of every box, -1 in unused entries)"""
    rs = np.random.RandomState(seed)
    n_max = max(n_obj_t(t) for t in range(T))
    pos = 0.5 + (rs.rand(n_max, 2) - .5) * span; vel = (rs.rand(n_max, 2) - .5) * .04; wh = rs.rand(n_max, 2) * .06 + .18
    boxes = np.zeros((T, cap, 8), dtype=np.float32); counts = np.zeros(T, dtype=np.int32)
    obj = np.full((T, cap), -1, dtype=np.int32)
    for t in range(T):
        alive = [k for k in range(n_obj_t(t)) if rs.rand() > 0.1]
        rs.shuffle(alive)
        for i, k in enumerate(alive[:cap]):
            p = pos[k] + vel[k] * t
            boxes[t, i] = [p[0], p[1], wh[k, 0], wh[k, 1], .9, k % 2, .8, i]
            obj[t, i] = k
        counts[t] = min(len(alive), cap)
    return boxes, counts, obj


def crowd_boxes(T, cap, n_obj_t, seed, span):
    return crowd_boxes_gt(T, cap, n_obj_t, seed, span)[:2]


THR, GAIN, SEED = 0.3, 0.5, 7
# name -> (T, cap, objects(t), tcap, max_age, span, the match its differences from best-first are stated at, kernel form)
SCENES = {
    "crowd_reg_grow": (12, 32, lambda t: 10 + 2 * t, 64, 0, .35, 0, "register"),
    "crowd_reg": (12, 32, lambda t: 24, 64, 2, .35, MATCH_ANY_LABEL, "register"),
    "crowd_lds": (6, 96, lambda t: 60 + 6 * t, 160, 2, .6, 0, "general"),
    "crowd_long": (66, 24, lambda t: 14 + (t % 8), 48, 1, .3, 0, "general"),
}
_BOXES, _REFS = {}, {}


def form_of(tcap, T):
    """the kernel form the launcher takes"""
    return "register" if tcap <= 64 and T <= 64 else "general"


def scene(name):
    """-> (boxes, counts), computed once"""
    if name not in _BOXES:
        T, cap, nobj, _, _, span, _, _ = SCENES[name]
        _BOXES[name] = crowd_boxes(T, cap, nobj, SEED, span)
    return _BOXES[name]


def case_boxes(k):
    """the boxes of track_readout_ref.CASES[k], computed once -> (boxes, counts)"""
    key = ("case", k)
    if key not in _BOXES:
        _BOXES[key] = moving_boxes(*CASES[k][:3], seed=SEED)
    return _BOXES[key]


def ref(key, boxes, counts, max_age, min_hits, match, tcap):
    """the stateless restatement at THR and GAIN, computed once per key and shared: callers must leave it unchanged"""
    key = (key, int(max_age), int(match), int(tcap))
    if key not in _REFS:
        _REFS[key] = associate_tracks_assign(boxes, counts, THR, max_age, GAIN, 1, match, tcap)
    return with_min_hits(_REFS[key], min_hits)


def scene_ref(name, match, min_hits=1, max_age=None, tcap=None):
    b, c = scene(name)
    s = SCENES[name]
    return ref(name, b, c, s[4] if max_age is None else max_age, min_hits, match, s[3] if tcap is None else tcap)


def worked_example():
    """the issue's smallest case: two boxes compete for one track -> (boxes [2, 2, 8], counts [2])"""
    boxes = np.zeros((2, 2, 8), dtype=np.float32)
    for t, xs in enumerate(((0.40, 0.52), (0.44, 0.33))):
        for i, x in enumerate(xs):
            boxes[t, i] = [x, 0.5, 0.2, 0.2, .9, 0, .8, i]
    return boxes, np.array([2, 2], dtype=np.int32)
