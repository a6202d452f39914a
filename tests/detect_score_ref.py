"""Plain restatement of detection scoring ("Detection scoring"), for the tests.

  * MATCH, per frame (the VOC devkit's rule).  The candidates of detection i are all ground-truth rows of equal label, claimed and
    ignored ones too; best[i] is the candidate of the largest bbox_iou(gt g, det i) as float32, ties to the lowest g; without a
    candidate best = -1 and iou = 0.  Per threshold the frame's detections are walked by descending score, ties to the lower row:
    best < 0 or iou < thr -> FP (0); best is an ignore row -> ignored (2), nothing claimed; best unclaimed -> TP (1), claimed;
    otherwise FP (a duplicate).  Rows whose label is not an integer value in 0..NC-1 take no part (-1).
  * RANK, over all frames, per threshold and label: the detections of state 0 / 1 by descending score, ties to the lower flat
    index; rank = the position, ctp = the TPs up to and including it.
  * AP from the integers, in Python floats: "area", "voc11", "coco101".

Everything is a Python list walked one element at a time, with np.float32 around each comparison; the IoU is orc.bbox_iou, so its
float32 bits are the oracle's.  Test infrastructure only.
"""
import numpy as np

from oracle import oracle as orc

f32 = np.float32
COCO = tuple(0.5 + 0.05 * i for i in range(10))
METHODS = ("area", "voc11", "coco101")


def label_of(v, NC):
    """the class of a row, or -1 when its label float takes no part"""
    v = float(f32(v))
    return int(v) if v == int(v) and 0 <= v < NC else -1


def _clamp(n, cap):
    return min(max(int(n), 0), cap)


def match_frame(det, nd, gt, ng, flags, NC, thresholds, score_at):
    """one frame -> (state [n_thr][nd], best [nd], iou [nd], IoU ties)"""
    best, iou, ties = [], [], 0
    for i in range(nd):
        bj, bi, tie = -1, f32(0), False
        if label_of(det[i][5], NC) >= 0:
            for g in range(ng):
                if f32(gt[g][5]) != f32(det[i][5]):
                    continue
                v = f32(orc.bbox_iou(gt[g][:4], det[i][:4]))
                if bj < 0 or v > bi:
                    bj, bi, tie = g, v, False
                elif v == bi and v > 0:
                    tie = True
        best.append(bj)
        iou.append(bi)
        ties += int(tie)
    order = sorted(range(nd), key=lambda i: (-float(f32(det[i][score_at])), i))
    state = []
    for thr in thresholds:
        thr = f32(thr)
        claimed, st = set(), [-1] * nd
        for i in order:
            if label_of(det[i][5], NC) < 0:
                continue
            if best[i] < 0 or iou[i] < thr:
                st[i] = 0
            elif flags is not None and int(flags[best[i]]) & 1:
                st[i] = 2
            elif best[i] not in claimed:
                st[i] = 1
                claimed.add(best[i])
            else:
                st[i] = 0
        state.append(st)
    return state, best, iou, ties


def detect_match(det_boxes, det_counts, gt_boxes, gt_counts, gt_flags, NC, thresholds, score_at=6, chunks=None):
    """-> dict(state [n_thr,B,cap], best [B,cap], iou [B,cap], ties).  chunks: frame counts; every chunk is matched by a call of its
    own and the parts are concatenated along B (the chunk contract)."""
    B, cap, _ = det_boxes.shape
    gcap = gt_boxes.shape[1]
    n_thr = len(thresholds)
    parts, b0 = [], 0
    for L in (chunks or [B]):
        state = np.full((n_thr, L, cap), -1, dtype=np.int32)
        best = np.full((L, cap), -1, dtype=np.int32)
        iou = np.zeros((L, cap), dtype=np.float32)
        ties = 0
        for b in range(b0, b0 + L):
            nd, ng = _clamp(det_counts[b], cap), _clamp(gt_counts[b], gcap)
            st, bj, bi, t = match_frame(det_boxes[b], nd, gt_boxes[b], ng, None if gt_flags is None else gt_flags[b], NC, thresholds, score_at)
            for k in range(n_thr):
                state[k, b - b0, :nd] = st[k]
            best[b - b0, :nd] = bj
            iou[b - b0, :nd] = bi
            ties += t
        parts.append((state, best, iou, ties))
        b0 += L
    assert b0 == B
    return dict(state=np.concatenate([p[0] for p in parts], axis=1), best=np.concatenate([p[1] for p in parts]),
                iou=np.concatenate([p[2] for p in parts]), ties=sum(p[3] for p in parts))


def detect_rank(det_boxes, det_counts, state, gt_boxes, gt_counts, gt_flags, NC, score_at=6):
    """-> dict(rank, ctp [n_thr,B,cap], ngt [NC], ndet, ntp [n_thr,NC])"""
    B, cap, _ = det_boxes.shape
    gcap = gt_boxes.shape[1]
    n_thr = state.shape[0]
    rank = np.full((n_thr, B, cap), -1, dtype=np.int32)
    ctp = np.full((n_thr, B, cap), -1, dtype=np.int32)
    ngt = np.zeros(NC, dtype=np.int32)
    ndet = np.zeros((n_thr, NC), dtype=np.int32)
    ntp = np.zeros((n_thr, NC), dtype=np.int32)
    for b in range(B):
        for g in range(_clamp(gt_counts[b], gcap)):
            c = label_of(gt_boxes[b, g, 5], NC)
            if c >= 0 and not (gt_flags is not None and int(gt_flags[b, g]) & 1):
                ngt[c] += 1
    rows = []                                      # (class, score, flat index) of the rows in use
    for b in range(B):
        for i in range(_clamp(det_counts[b], cap)):
            c = label_of(det_boxes[b, i, 5], NC)
            if c >= 0:
                rows.append((c, f32(det_boxes[b, i, score_at]), b * cap + i))
    for k in range(n_thr):
        for c in range(NC):
            mine = [r for r in rows if r[0] == c and int(state[k, r[2] // cap, r[2] % cap]) in (0, 1)]
            mine = sorted(mine, key=lambda r: (-float(r[1]), r[2]))
            tps = 0
            for pos, r in enumerate(mine):
                b, i = r[2] // cap, r[2] % cap
                tps += int(state[k, b, i] == 1)
                rank[k, b, i] = pos
                ctp[k, b, i] = tps
            ndet[k, c] = len(mine)
            ntp[k, c] = tps
    return dict(rank=rank, ctp=ctp, ngt=ngt, ndet=ndet, ntp=ntp)


INT_KEYS = ("state", "best", "rank", "ctp", "ngt", "ndet", "ntp")


def detect_score(s, NC, thresholds, score_at=6, flags=True, chunks=None):
    """a scene dict -> the union of match and rank, plus what evaluate.average_precision wants beside them"""
    fl = s["gt_flags"] if flags else None
    r = detect_match(s["det_boxes"], s["det_counts"], s["gt_boxes"], s["gt_counts"], fl, NC, thresholds, score_at, chunks)
    r.update(detect_rank(s["det_boxes"], s["det_counts"], r["state"], s["gt_boxes"], s["gt_counts"], fl, NC, score_at))
    r.update(thresholds=np.asarray(thresholds, dtype=np.float32), nb_class=NC, scores=s["det_boxes"][:, :, score_at],
             labels=s["det_boxes"][:, :, 5])
    return r


# ---------------------------------------------------------------------------------------------------------------- AP, loop form
def curve(r, k, c):
    """ctp in rank order for threshold k, class c, as a list"""
    NC = int(r["nb_class"])
    n = int(r["ndet"][k][c])
    out = [None] * n
    B, cap = r["rank"].shape[1:]
    for b in range(B):
        for i in range(cap):
            if r["rank"][k, b, i] >= 0 and label_of(r["labels"][b, i], NC) == c:
                assert out[int(r["rank"][k, b, i])] is None
                out[int(r["rank"][k, b, i])] = int(r["ctp"][k, b, i])
    assert None not in out
    return out


def ap_from_curve(ctps, ngt, method):
    if ngt == 0:
        return float("nan")
    n = len(ctps)
    if n == 0:
        return 0.0
    p = [ctps[j] / float(j + 1) for j in range(n)]
    rc = [ctps[j] / float(ngt) for j in range(n)]
    if method == "area":
        env = list(p)
        for j in range(n - 2, -1, -1):
            env[j] = max(env[j], env[j + 1])
        ap, prev = 0.0, 0.0
        for j in range(n):
            ap += (rc[j] - prev) * env[j]
            prev = rc[j]
        return ap
    steps = {"voc11": 10, "coco101": 100}[method]
    total = 0.0
    for i in range(steps + 1):
        t = i / float(steps)
        best = 0.0
        for j in range(n):
            if rc[j] >= t and p[j] > best:
                best = p[j]
        total += best
    return total / float(steps + 1)


def average_precision(r, method="area"):
    """-> (ap [n_thr][NC] with nan, map [n_thr], map_all)"""
    n_thr, NC = len(r["thresholds"]), int(r["nb_class"])
    ap = [[ap_from_curve(curve(r, k, c) if r["ngt"][c] > 0 else [], int(r["ngt"][c]), method) for c in range(NC)] for k in range(n_thr)]
    maps = []
    for k in range(n_thr):
        vals = [ap[k][c] for c in range(NC) if r["ngt"][c] > 0]
        maps.append(sum(vals) / len(vals) if vals else float("nan"))
    return ap, maps, (sum(maps) / len(maps) if maps and maps[0] == maps[0] else float("nan"))


# ---------------------------------------------------------------------------------------------------------------- scenes
def row(x, y, w, h, label, score=1.0, conf=1.0):
    return np.array([x, y, w, h, conf, label, score, 0], dtype=np.float32)


def make_scene(B, cap, gcap, NC, n_obj, seed, classes=None, heavy=None, empty=False, over_cap=False):
    """Seeded frames.  Ground truth: n_obj random boxes per frame (+- a fifth), labels from `classes` (default: all NC; `heavy` = (class,
    share) gives one class that share of the rows), about one in seven duplicated exactly (IoU ties between candidates), about 5 %
    with a label outside 0..NC-1 (NC, -1, or c + 0.5), about 12 % flagged ignore (flag words 1 and 3; 2 has bit 0 clear and is not).
    Detections: per ground-truth row, with probability 0.9, a copy jittered by 1 %, 5 % or 12 % (so some pass 0.5 and fail 0.75), a
    second copy for a quarter of them (duplicates), 5 % mislabelled, 3 % with a label outside the range; up to two spurious boxes of any
    class (often without a candidate).  Half the scores lie on a grid of 0.05 (ties within and across frames).  Rows are shuffled.
    In frame 0 the ground-truth rows of the first detection's class get the label NC, so that class has detections without a candidate.
    empty: frame 1 has no detections, frame 2 no ground truth, frame 3 neither.  over_cap: the counts of full frames exceed the capacity."""
    rs = np.random.RandomState(seed)
    classes = list(range(NC)) if classes is None else list(classes)
    det_boxes = np.zeros((B, cap, 8), dtype=np.float32)
    gt_boxes = np.zeros((B, gcap, 8), dtype=np.float32)
    det_counts = np.zeros(B, dtype=np.int32)
    gt_counts = np.zeros(B, dtype=np.int32)
    gt_flags = np.zeros((B, gcap), dtype=np.int32)

    def bad(c):
        return [NC, -1, c + 0.5][rs.randint(3)]

    for b in range(B):
        n = n_obj + rs.randint(-(n_obj // 5), n_obj // 5 + 1) if n_obj >= 5 else n_obj
        gts, fl = [], []
        for _ in range(n):
            c = heavy[0] if heavy is not None and rs.rand() < heavy[1] else classes[rs.randint(len(classes))]
            g = row(.1 + .8 * rs.rand(), .1 + .8 * rs.rand(), .05 + .2 * rs.rand(), .05 + .2 * rs.rand(), c)
            gts.append(g)
            fl.append([1, 3][rs.randint(2)] if rs.rand() < 0.12 else [0, 0, 2][rs.randint(3)])
            if rs.rand() < 0.15:
                gts.append(g.copy())
                fl.append(0)
        dets = []
        for g in gts:
            if rs.rand() >= 0.9:
                continue
            for _ in range(2 if rs.rand() < 0.25 else 1):
                j = [.01, .01, .05, .12][rs.randint(4)]
                d = g.copy()
                d[:2] += ((rs.rand(2) - .5) * 2 * j).astype(np.float32)
                d[2:4] *= (1 + (rs.rand(2) - .5) * 2 * j).astype(np.float32)
                if rs.rand() < 0.05:
                    d[5] = classes[rs.randint(len(classes))]
                if rs.rand() < 0.03:
                    d[5] = bad(d[5])
                dets.append(d)
        for _ in range(rs.randint(0, 3)):
            dets.append(row(rs.rand(), rs.rand(), .05 + .2 * rs.rand(), .05 + .2 * rs.rand(), rs.randint(NC)))
        for k in range(len(gts)):
            if rs.rand() < 0.05:
                gts[k][5] = bad(gts[k][5])
        for d in dets:
            d[6] = np.round(rs.rand() * 20) / 20 if rs.rand() < 0.5 else rs.rand()
            d[4] = rs.rand()
        order = rs.permutation(len(dets))
        dets = [dets[k] for k in order]
        if b == 0 and dets:                         # frame 0: the class of its first detection loses its ground truth -> no candidate
            for g in gts:
                if g[5] == dets[0][5]:
                    g[5] = NC
        order = rs.permutation(len(gts))
        gts, fl = [gts[k] for k in order], [fl[k] for k in order]
        if empty and b in (1, 3):
            dets = []
        if empty and b in (2, 3):
            gts, fl = [], []
        nd, ng = min(len(dets), cap), min(len(gts), gcap)
        for i in range(nd):
            det_boxes[b, i] = dets[i]
        for g in range(ng):
            gt_boxes[b, g] = gts[g]
            gt_flags[b, g] = fl[g]
        det_counts[b] = len(dets) + 5 if over_cap and len(dets) >= cap else nd
        gt_counts[b] = len(gts) + 3 if over_cap and len(gts) >= gcap else ng
    return dict(det_boxes=det_boxes, det_counts=det_counts, gt_boxes=gt_boxes, gt_counts=gt_counts, gt_flags=gt_flags)


# name -> (B, cap, gcap, NC, objects per frame, seed, thresholds of the GPU case, kwargs of make_scene)
SCENES = {
    "registers": (5, 16, 8, 3, 6, 11, (0.5,), {}),
    "passes": (7, 96, 80, 12, 60, 12, COCO, {}),                                     # several 64-lane passes on both sides
    "thr16": (6, 40, 32, 1, 20, 13, tuple(0.2 + 0.05 * i for i in range(16)), {}),
    "nc80": (6, 48, 40, 80, 24, 14, (0.5, 0.75), dict(classes=(0, 3, 7, 41, 79))),    # most classes empty
    "edges": (10, 20, 16, 4, 24, 15, (0.5, 0.6), dict(empty=True, over_cap=True)),
    "rank_tiles": (64, 96, 80, 12, 68, 16, (0.5, 0.75), dict(heavy=(3, 0.97))),       # > 5000 rows in use, one class with > 90 %
    "odd_grid": (9, 37, 21, 5, 18, 17, (0.5,), {}),                                   # B * cap = 333: no multiple of a workgroup
}

_SCENES, _REFS, _COVER = {}, {}, {}


def scene(name):
    """the scene, built once -> (dict, NC, thresholds)"""
    if name not in _SCENES:
        B, cap, gcap, NC, n_obj, seed, thr, kw = SCENES[name]
        _SCENES[name] = (make_scene(B, cap, gcap, NC, n_obj, seed, **kw), NC, thr)
    return _SCENES[name]


def scene_ref(name, thresholds=None, flags=True, score_at=6):
    """the restatement on a scene, computed once per argument set (the result is shared: do not write to it)"""
    s, NC, thr = scene(name)
    thr = tuple(thr if thresholds is None else thresholds)
    key = (name, thr, bool(flags), score_at)
    if key not in _REFS:
        _REFS[key] = detect_score(s, NC, thr, score_at, flags)
    return _REFS[key]


def all_empty(B=3, cap=8, gcap=4):
    """a set without a detection or a ground-truth row (the boxes hold garbage that must not be read as rows)"""
    rs = np.random.RandomState(5)
    return dict(det_boxes=rs.rand(B, cap, 8).astype(np.float32), det_counts=np.zeros(B, dtype=np.int32),
                gt_boxes=rs.rand(B, gcap, 8).astype(np.float32), gt_counts=np.array([0, -2, 0][:B], dtype=np.int32),
                gt_flags=np.ones((B, gcap), dtype=np.int32))


def coverage(name):
    """what a scene exercises, counted on the restatement at the COCO thresholds: the keys of the returned dict are the cases the
    tests require of every scene"""
    if name in _COVER:
        return _COVER[name]
    s, NC, _ = scene(name)
    r = scene_ref(name, COCO)
    B, cap, _ = s["det_boxes"].shape
    gcap = s["gt_boxes"].shape[1]
    c = dict(tp=0, duplicate_fp=0, low_iou_fp=0, ignored=0, no_candidate=0, score_tie_in_frame=0, score_tie_across_frames=0,
             iou_tie=int(r["ties"]), state_differs=0, label_outside=0)
    seen = {}
    for b in range(B):
        nd = _clamp(s["det_counts"][b], cap)
        here = {}
        for i in range(nd):
            cl = label_of(s["det_boxes"][b, i, 5], NC)
            if cl < 0:
                c["label_outside"] += 1
                assert (r["state"][:, b, i] == -1).all()
                continue
            sc = (cl, float(s["det_boxes"][b, i, 6]))
            c["score_tie_in_frame"] += int(sc in here)
            c["score_tie_across_frames"] += int(sc in seen and seen[sc] != b)
            here[sc] = b
            st = [int(v) for v in r["state"][:, b, i]]
            c["tp"] += int(1 in st)
            c["ignored"] += int(2 in st)
            c["no_candidate"] += int(r["best"][b, i] < 0)
            c["state_differs"] += int(len(set(st)) > 1)
            for k, thr in enumerate(COCO):
                if st[k] == 0 and r["best"][b, i] >= 0:
                    if r["iou"][b, i] >= f32(thr):
                        c["duplicate_fp"] += 1
                    elif r["iou"][b, i] > 0:
                        c["low_iou_fp"] += 1
        seen.update(here)
        for g in range(_clamp(s["gt_counts"][b], gcap)):
            c["label_outside"] += int(label_of(s["gt_boxes"][b, g, 5], NC) < 0)
    _COVER[name] = c
    return c


# ---------------------------------------------------------------------------------------------------------------- the worked example
def worked_example():
    """DESIGN.md's two frames: one class, threshold 0.5 -> the scene dict"""
    A, Bx, C = (0.25, 0.25, 0.25, 0.25), (0.75, 0.75, 0.25, 0.25), (0.5, 0.5, 0.25, 0.25)      # exact in float32: IoU 1 with itself
    s = dict(det_boxes=np.zeros((2, 4, 8), dtype=np.float32), det_counts=np.array([4, 1], dtype=np.int32),
             gt_boxes=np.zeros((2, 2, 8), dtype=np.float32), gt_counts=np.array([2, 1], dtype=np.int32),
             gt_flags=np.array([[0, 1], [0, 0]], dtype=np.int32))
    s["gt_boxes"][0, 0], s["gt_boxes"][0, 1], s["gt_boxes"][1, 0] = row(*A, label=0), row(*Bx, label=0), row(*C, label=0)
    s["det_boxes"][0, 0] = row(*A, label=0, score=0.9)
    s["det_boxes"][0, 1] = row(0.28125, 0.25, 0.25, 0.25, label=0, score=0.8)       # A shifted by 1/32: IoU 7/9
    s["det_boxes"][0, 2] = row(*Bx, label=0, score=0.7)
    s["det_boxes"][0, 3] = row(0.125, 0.875, 0.125, 0.125, label=0, score=0.95)    # overlaps nothing
    s["det_boxes"][1, 0] = row(*C, label=0, score=0.85)
    return s


def zero_area():
    """one frame, one class: a ground-truth row without area and two detections equal to it.  Their IoU is 0 / 0 = NaN, which is below
    no threshold: the higher score is a TP, the other its duplicate; a third detection, elsewhere, has IoU 0 with the row"""
    s = dict(det_boxes=np.zeros((1, 4, 8), dtype=np.float32), det_counts=np.array([3], dtype=np.int32),
             gt_boxes=np.zeros((1, 2, 8), dtype=np.float32), gt_counts=np.array([1], dtype=np.int32), gt_flags=np.zeros((1, 2), dtype=np.int32))
    s["gt_boxes"][0, 0] = row(0.5, 0.5, 0, 0, label=0)
    s["det_boxes"][0, 0] = row(0.5, 0.5, 0, 0, label=0, score=0.8)
    s["det_boxes"][0, 1] = row(0.5, 0.5, 0, 0, label=0, score=0.9)
    s["det_boxes"][0, 2] = row(0.25, 0.25, 0.125, 0.125, label=0, score=0.7)
    return s


WORKED_STATE = [[1, 0, 2, 0], [1, -1, -1, -1]]
WORKED_RANK = [[1, 3, -1, 0], [2, -1, -1, -1]]
WORKED_CTP = [[1, 2, -1, 0], [2, -1, -1, -1]]
WORKED_NGT, WORKED_NDET, WORKED_NTP = 2, 4, 2
WORKED_AP = 2.0 / 3.0
