"""Plain restatement of track scoring ("Track scoring"), for the tests.

The CLEAR-MOT frame step with the optimal assignment replaced by the best-IoU-first order:

  * VALID PAIRS.  (g, i): ground-truth row g and hypothesis row i of the frame with bbox_iou >= thr as float32, and equal labels
    as floats unless any_label.
  * CARRY-OVER.  g ascending: if g's id has a table row whose last track id tau is >= 0, the lowest unclaimed i with hypothesis
    id tau is looked up; if (g, i) is valid, g is matched to i.
  * THE REST.  Among unmatched g and unclaimed i the valid pair of the largest IoU is taken repeatedly, ties to the lowest g, then
    the lowest i.
  * COUNTS and TABLE UPDATE in g order, every read of the table seeing it as the previous frame left it.  The update is a plain
    walk over the rows: when an id occurs in several rows of a frame the counters add, the highest row decides "last appearance
    matched", and the last track id is that of the highest MATCHED row (an unmatched row keeps the id, whoever set it).

Everything is a Python list walked one element at a time, with np.float32 around each operation; the IoU is orc.bbox_iou, so its
float32 bits are the oracle's.  Test infrastructure only.
"""
import numpy as np

from oracle import oracle as orc

import track_match_ref as tmr

f32 = np.float32
SCORE_INTS, OBJ_INTS = 8, 8
KEYS = ("totals", "objs", "nobjs", "frame_counts", "match", "miou")


class TrackScore(object):
    """the state a resumed run carries: the totals and the object table"""

    def __init__(self, thr, any_label, ocap):
        self.thr, self.any_label, self.ocap = f32(thr), bool(any_label), int(ocap)
        self.objs = []           # rows [gt id, last track id, present, matched, switches, fragments, last appearance matched, 0]
        self.totals = [0] * SCORE_INTS
        self.ties = 0            # frames so far in which two valid pairs sharing a row had equal IoU

    def frame(self, gt_rows, gt_ids, hyp_rows, hyp_ids, label_at):
        """one frame -> (match: list of hypothesis rows or -1 per g, miou: list of float32, (gt, hyp, matches, switches))"""
        ng, nh = len(gt_rows), len(hyp_rows)
        valid = {}
        for g in range(ng):
            for i in range(nh):
                if not self.any_label and f32(gt_rows[g][5]) != f32(hyp_rows[i][label_at]):
                    continue
                iou = f32(orc.bbox_iou(gt_rows[g][:4], hyp_rows[i][:4]))
                if iou >= self.thr:
                    valid[(g, i)] = iou
        if tmr.shared_tie(valid):
            self.ties += 1
        before = [list(r) for r in self.objs]      # the table as the previous frame left it
        entry = []
        for g in range(ng):
            e = -1
            if int(gt_ids[g]) >= 0:
                for k, r in enumerate(before):
                    if r[0] == int(gt_ids[g]):
                        e = k
            entry.append(e)
        match, claimed = [-1] * ng, set()
        for g in range(ng):                        # carry-over
            if entry[g] < 0 or before[entry[g]][1] < 0:
                continue
            tau = before[entry[g]][1]
            for i in range(nh):
                if i not in claimed and int(hyp_ids[i]) == tau:
                    if (g, i) in valid:
                        match[g] = i
                        claimed.add(i)
                    break                          # the lowest such i only
        while True:                                # the rest, best IoU first
            best = None
            for (g, i) in sorted(valid):           # ascending g, then i: a strict comparison keeps the first
                if match[g] >= 0 or i in claimed:
                    continue
                if best is None or valid[(g, i)] > valid[best]:
                    best = (g, i)
            if best is None:
                break
            match[best[0]] = best[1]
            claimed.add(best[1])
        miou = [valid[(g, match[g])] if match[g] >= 0 else f32(0) for g in range(ng)]
        switch, fragment = [], []
        for g in range(ng):
            r = before[entry[g]] if entry[g] >= 0 else None
            hit = match[g] >= 0 and r is not None
            switch.append(bool(hit and r[1] >= 0 and r[1] != int(hyp_ids[match[g]])))
            fragment.append(bool(hit and r[3] > 0 and r[6] == 0))
        n_match = sum(1 for m in match if m >= 0)
        for g in range(ng):                        # the update, in g order
            gid = int(gt_ids[g])
            if gid < 0:
                continue
            e = -1
            for k, r in enumerate(self.objs):
                if r[0] == gid:
                    e = k
            if e < 0:
                if len(self.objs) >= self.ocap:
                    self.totals[6] += 1
                    continue
                self.objs.append([gid, -1, 0, 0, 0, 0, 0, 0])
                e = len(self.objs) - 1
            r = self.objs[e]
            r[2] += 1
            if match[g] >= 0:
                r[3] += 1
                r[4] += int(switch[g])
                r[5] += int(fragment[g])
                r[1] = int(hyp_ids[match[g]])
                r[6] = 1
            else:
                r[6] = 0
        fc = (ng, nh, n_match, sum(switch))
        self.totals[0] += 1
        self.totals[1] += ng
        self.totals[2] += nh
        self.totals[3] += n_match
        self.totals[4] += sum(switch)
        self.totals[5] += sum(fragment)
        return match, miou, fc

    def clip(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, label_at=5):
        """gt_boxes [T, gcap, 8], gt_counts [T], gt_ids [T, gcap]; hyp_boxes [T, hcap, 8], hyp_counts [T], hyp_ids [T, hcap] (or
        [T, hcap, k]: the id in word 0) -> dict of the per-frame outputs"""
        T, gcap, _ = gt_boxes.shape
        hcap = hyp_boxes.shape[1]
        if hyp_ids.ndim == 3:
            hyp_ids = hyp_ids[:, :, 0]
        r = dict(frame_counts=np.zeros((T, 4), dtype=np.int32), match=np.full((T, gcap), -1, dtype=np.int32),
                 miou=np.zeros((T, gcap), dtype=np.float32))
        for t in range(T):
            ng, nh = min(max(int(gt_counts[t]), 0), gcap), min(max(int(hyp_counts[t]), 0), hcap)
            m, u, fc = self.frame(gt_boxes[t, :ng], gt_ids[t, :ng], hyp_boxes[t, :nh], hyp_ids[t, :nh], label_at)
            r["match"][t, :ng] = m
            r["miou"][t, :ng] = u
            r["frame_counts"][t] = fc
        return r

    def state(self):
        objs = np.zeros((self.ocap, OBJ_INTS), dtype=np.int32)
        objs[:, :2] = -1
        for k, row in enumerate(self.objs):
            objs[k] = row
        return dict(totals=np.array(self.totals, dtype=np.int32), objs=objs, nobjs=len(self.objs))


def track_score(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, thr=0.5, any_label=False, ocap=64, label_at=5, chunks=None):
    """one clip -> dict of KEYS (arrays without the clip axis, nobjs an int) and `ties`; chunks: the same through one carried
    state fed in chunks along T"""
    T = gt_boxes.shape[0]
    ts = TrackScore(thr, any_label, ocap)
    parts, t0 = [], 0
    for L in (chunks or [T]):
        s = slice(t0, t0 + L)
        parts.append(ts.clip(gt_boxes[s], gt_counts[s], gt_ids[s], hyp_boxes[s], hyp_counts[s], hyp_ids[s], label_at))
        t0 += L
    assert t0 == T
    r = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    r.update(ts.state())
    r["ties"] = ts.ties
    return r


def misses_fps_switches(r):
    t = r["totals"]
    return int(t[1] - t[3]), int(t[2] - t[3]), int(t[4])


# ---------------------------------------------------------------------------------------------------------------- scenes
TRACKER = dict(thr=0.3, max_age=1, gain=0.5, min_hits=1, match=tmr.MATCH_BEST_FIRST)      # the tracker whose ids the scenes score


def make_scene(T, gcap, hcap, n_obj, seed, empty=False, over_cap=False, duplicates=False, repeats=False):
    """ground truth = track_match_ref.moving_boxes_gt (ids = the generator's object index); hypotheses = the same boxes with seeded
    jitter, about 10 % dropped, about 5 % mislabelled, up to two spurious boxes per frame, in shuffled order; hypothesis ids from the restatement of the
    tracker (track_match_ref.associate_tracks_match).
    empty: frames 2, 3, 4 have no ground truth, no hypotheses, neither.  over_cap: the counts of full frames exceed the capacity.
    duplicates: the generator's exact-duplicate boxes stay in the ground truth, so pairs tie on IoU.
    repeats: in every frame four ground-truth rows take the id of another row of the frame (an id then occurs twice or more, in any
    order of matched and unmatched rows), two rows get the id -1 (they take part, without memory), and two hypotheses take the id of
    another hypothesis of the frame (so the lowest unclaimed one of an id is not the only one).
    -> dict(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids)"""
    n_of = n_obj if callable(n_obj) else (lambda t: n_obj)
    gt_boxes, gt_counts, obj = tmr.moving_boxes_gt(T, gcap, n_of, seed, duplicates=duplicates)
    rs = np.random.RandomState(seed + 1000)
    hyp_boxes = np.zeros((T, hcap, 8), dtype=np.float32)
    hyp_counts = np.zeros(T, dtype=np.int32)
    source = gt_counts.copy()                      # the hypotheses of a frame without ground truth still come from its boxes
    if empty:
        gt_counts[2] = 0
        gt_counts[4] = 0
    for t in range(T):
        rows = []
        for g in range(min(int(source[t]), gcap)):
            if rs.rand() < 0.1:
                continue
            r = gt_boxes[t, g].copy()
            r[:2] += ((rs.rand(2) - .5) * .02).astype(np.float32)
            r[2:4] *= (1 + (rs.rand(2) - .5) * .1).astype(np.float32)
            if rs.rand() < 0.05:
                r[5] = (r[5] + 1) % 3              # a wrong label: a miss and a false positive unless labels are not compared
            rows.append(r)
        for _ in range(rs.randint(0, 3)):
            rows.append(np.array([rs.rand(), rs.rand(), .05 + .2 * rs.rand(), .05 + .2 * rs.rand(), .9, rs.randint(0, 3), .8, 0], dtype=np.float32))
        order = rs.permutation(len(rows))
        rows = [rows[k] for k in order][:hcap]
        if empty and t in (3, 4):
            rows = []
        for i, r in enumerate(rows):
            hyp_boxes[t, i] = r
        hyp_counts[t] = len(rows)
    if empty:
        obj[2] = -1
        obj[4] = -1
    a = tmr.associate_tracks_match(hyp_boxes, hyp_counts, TRACKER["thr"], TRACKER["max_age"], TRACKER["gain"], TRACKER["min_hits"],
                                   TRACKER["match"], None)
    if over_cap:
        gt_counts = np.where(gt_counts >= gcap, gt_counts + 3, gt_counts).astype(np.int32)
        hyp_counts = np.where(hyp_counts >= hcap, hyp_counts + 5, hyp_counts).astype(np.int32)
    gt_ids, hyp_ids = obj.astype(np.int32), a["ids"].astype(np.int32)
    if repeats:
        rr = np.random.RandomState(seed + 2000)
        for t in range(T):
            ng, nh = min(int(gt_counts[t]), gcap), min(int(hyp_counts[t]), hcap)
            if ng < 4 or nh < 2:
                continue
            for _ in range(4):
                src, dst = rr.choice(ng, 2, replace=False)
                gt_ids[t, dst] = gt_ids[t, src]
            for g in rr.choice(ng, 2, replace=False):
                gt_ids[t, g] = -1
            for _ in range(2):
                src, dst = rr.choice(nh, 2, replace=False)
                hyp_ids[t, dst] = hyp_ids[t, src]
    return dict(gt_boxes=gt_boxes, gt_counts=gt_counts, gt_ids=gt_ids, hyp_boxes=hyp_boxes, hyp_counts=hyp_counts, hyp_ids=hyp_ids)


def repeated_id_cases(s, ref):
    """what a scene with repeated ids exercises, counted on the restatement's match: frames x ids in which an id occurs in several
    rows and (a) a lower row is matched while the highest is not, (b) the highest is matched while a lower one is not, (c) the rows
    lie in different 64-row passes; (d) rows with id < 0 that are matched; (e) frames in which two hypotheses share an id"""
    a = b = c = d = e = 0
    for t in range(s["gt_boxes"].shape[0]):
        ng = min(max(int(s["gt_counts"][t]), 0), s["gt_boxes"].shape[1])
        nh = min(max(int(s["hyp_counts"][t]), 0), s["hyp_boxes"].shape[1])
        rows = {}
        for g in range(ng):
            if s["gt_ids"][t, g] < 0:
                d += int(ref["match"][t, g] >= 0)
            else:
                rows.setdefault(int(s["gt_ids"][t, g]), []).append(g)
        for gs in rows.values():
            if len(gs) < 2:
                continue
            hit = [ref["match"][t, g] >= 0 for g in gs]
            a += int(any(hit[:-1]) and not hit[-1])
            b += int(hit[-1] and not all(hit[:-1]))
            c += int(gs[0] // 64 != gs[-1] // 64)
        e += int(len(set(s["hyp_ids"][t, :nh].tolist())) < nh)
    return a, b, c, d, e


# name -> (T, gcap, hcap, objects, ocap, kwargs of make_scene); seed 7 everywhere
SCENES = {
    "small": (40, 32, 32, 12, 64, dict(duplicates=True)),   # ... with IoU ties
    "wide": (8, 128, 160, 140, 256, {}),                    # several 64-lane passes on every axis, gcap != hcap
    "long": (130, 32, 32, 20, 64, {}),
    "empty": (20, 32, 32, 12, 64, dict(empty=True)),
    "counts_above_cap": (12, 16, 12, 24, 64, dict(over_cap=True)),
    "repeated_ids": (12, 96, 96, 100, 160, dict(repeats=True)),      # an id in several rows of a frame, rows with id -1, shared hypothesis ids
}

_SCENES = {}


def scene(name):
    """the scene, built once"""
    if name not in _SCENES:
        T, gcap, hcap, n_obj, ocap, kw = SCENES[name]
        _SCENES[name] = (make_scene(T, gcap, hcap, n_obj, 7, **kw), ocap)
    return _SCENES[name]


_REFS = {}


def scene_ref(name, any_label, ocap=None):
    """the restatement on a scene, computed once per (scene, any_label, ocap)"""
    s, oc = scene(name)
    key = (name, bool(any_label), ocap or oc)
    if key not in _REFS:
        _REFS[key] = track_score(s["gt_boxes"], s["gt_counts"], s["gt_ids"], s["hyp_boxes"], s["hyp_counts"], s["hyp_ids"], 0.5, any_label,
                                 ocap or oc)
    return _REFS[key]


def worked_example():
    """DESIGN.md's five frames: one object, gt id 7, box (0.30, 0.5, 0.2, 0.2), label 0 -> the scene dict"""
    hyps = [[(0, 0.30)], [(0, 0.35), (1, 0.30)], [(1, 0.30)], [(1, 0.60)], [(1, 0.30)]]
    T, cap = 5, 2
    gt_boxes = np.zeros((T, cap, 8), dtype=np.float32)
    gt_boxes[:, 0] = [0.30, 0.5, 0.2, 0.2, 1.0, 0, 1.0, 0]
    hyp_boxes = np.zeros((T, cap, 8), dtype=np.float32)
    hyp_ids = np.full((T, cap), -1, dtype=np.int32)
    hyp_counts = np.zeros(T, dtype=np.int32)
    for t, rows in enumerate(hyps):
        for i, (tid, x) in enumerate(rows):
            hyp_boxes[t, i] = [x, 0.5, 0.2, 0.2, 0.9, 0, 0.8, i]
            hyp_ids[t, i] = tid
        hyp_counts[t] = len(rows)
    gt_ids = np.full((T, cap), -1, dtype=np.int32)
    gt_ids[:, 0] = 7
    return dict(gt_boxes=gt_boxes, gt_counts=np.ones(T, dtype=np.int32), gt_ids=gt_ids, hyp_boxes=hyp_boxes, hyp_counts=hyp_counts,
                hyp_ids=hyp_ids)


WORKED_TOTALS = [5, 5, 6, 4, 1, 1, 0, 0]
WORKED_OBJ = [7, 1, 5, 4, 1, 1, 1, 0]
WORKED_MATCH = [0, 0, 0, -1, 0]
WORKED_FRAME_COUNTS = [[1, 1, 1, 0], [1, 2, 1, 0], [1, 1, 1, 1], [1, 1, 0, 0], [1, 1, 1, 0]]


def two_rows(matched_row):
    """one frame, gt id 9 in rows 0 and 1 at different places, one hypothesis (id 5) on row `matched_row`; then a second frame with
    the object once, under hypothesis id 6"""
    gt_boxes = np.zeros((2, 2, 8), dtype=np.float32)
    gt_boxes[0, 0] = [0.2, 0.5, 0.1, 0.1, 1, 0, 1, 0]
    gt_boxes[0, 1] = [0.7, 0.5, 0.1, 0.1, 1, 0, 1, 0]
    gt_boxes[1, 0] = gt_boxes[0, matched_row]
    hyp_boxes = np.zeros((2, 2, 8), dtype=np.float32)
    hyp_boxes[:, 0] = gt_boxes[0, matched_row]
    return dict(gt_boxes=gt_boxes, gt_counts=np.array([2, 1], dtype=np.int32), gt_ids=np.array([[9, 9], [9, -1]], dtype=np.int32),
                hyp_boxes=hyp_boxes, hyp_counts=np.array([1, 1], dtype=np.int32), hyp_ids=np.array([[5, -1], [6, -1]], dtype=np.int32))
