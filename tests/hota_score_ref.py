"""Plain restatement of HOTA scoring ("HOTA scoring"), for the tests.

  * TABLES.  identity_score_ref's: a ground-truth and a hypothesis table per clip, ids >= 0 in order of first appearance.
  * SIMILARITY.  q[g][i] = int(f32(iou) * 2^20), 0 where the labels differ (unless any_label), the IoU is NaN or <= 0, or a row has no
    trajectory.
  * PASS 1.  Per frame R[g] = sum_i q, C[i] = sum_g q; a pair with q > 0 adds (q << 20) // (R[g] + C[i] - q) to P[a][b].
  * PASS 2.  From the finished P and tables: W[g][i] = 1 + (P[a][b] * q) // (2^20 * (n_a + n_b) - P[a][b]) where q > 0, else 0; the
    frame's match is identity_score_ref.assign_max's row_to_col on W.
  * COUNTS.  A matched pair's level L = the thresholds its float32 IoU reaches; L >= 1 adds 1 to tp[L-1], q to loc[L-1], 1 to
    pairs[L-1][a][b].
Everything is a Python int walked one element at a time; the IoU is orc.bbox_iou, so its float32 bits are the oracle's.

trackeval_rule is the measure as TrackEval computes it, in float64 (float sums, scipy's assignment on the alignment score times the
similarity), with this build's validity rule and float32 threshold compare.
Test infrastructure only.
"""
import numpy as np

from oracle import oracle as orc

import identity_score_ref as isr

f32 = np.float32
S = 1 << 20
INPUTS = isr.INPUTS
ALIGN_KEYS = ("sizes", "gt_tab", "hyp_tab", "align")
FRAME_KEYS = ("w", "dims", "gt_ent", "hyp_ent", "row_to_col")
COUNT_KEYS = ("tp", "loc", "pairs")
ALL_KEYS = ALIGN_KEYS + FRAME_KEYS + COUNT_KEYS
THRESHOLDS = np.array([0.05 * k for k in range(1, 20)], dtype=np.float32)


def quantise(iou):
    """float32 IoU -> q"""
    iou = f32(iou)
    if not iou > 0:                                              # NaN too
        return 0
    v = float(iou) * float(S)                                    # exact: a power of two
    return (1 << 31) - 1 if v >= float(1 << 31) else int(v)      # (the device's conversion saturates; no test reaches it)


def similarity(gt_rows, hyp_rows, a, b, any_label, label_at):
    """-> (q [ng][nh] ints, iou [ng][nh] float32 or None where it was not computed)"""
    q = [[0] * len(hyp_rows) for _ in gt_rows]
    iou = [[None] * len(hyp_rows) for _ in gt_rows]
    for g in range(len(gt_rows)):
        for i in range(len(hyp_rows)):
            if a[g] < 0 or b[i] < 0:
                continue
            if not any_label and f32(gt_rows[g][5]) != f32(hyp_rows[i][label_at]):
                continue
            iou[g][i] = f32(orc.bbox_iou(gt_rows[g][:4], hyp_rows[i][:4]))
            q[g][i] = quantise(iou[g][i])
    return q, iou


def counts_of(counts, t, cap):
    return min(max(int(counts[t]), 0), cap)


class Align(object):
    """pass 1 and the state a resumed run carries: sizes, both tables, P"""

    def __init__(self, any_label, acap, bcap):
        self.any_label, self.acap, self.bcap = bool(any_label), int(acap), int(bcap)
        self.sizes = [0] * isr.IDENT_INTS
        self.gt_tab, self.hyp_tab = [], []
        self.P = [[0] * self.bcap for _ in range(self.acap)]

    def clip(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, label_at=5):
        T, gcap, _ = gt_boxes.shape
        hcap = hyp_boxes.shape[1]
        if hyp_ids.ndim == 3:
            hyp_ids = hyp_ids[:, :, 0]
        for t in range(T):
            ng, nh = counts_of(gt_counts, t, gcap), counts_of(hyp_counts, t, hcap)
            a, oa = isr.Identity.rows_of(gt_ids[t, :ng], self.gt_tab, self.acap)
            b, ob = isr.Identity.rows_of(hyp_ids[t, :nh], self.hyp_tab, self.bcap)
            q, _ = similarity(gt_boxes[t, :ng], hyp_boxes[t, :nh], a, b, self.any_label, label_at)
            R = [sum(q[g]) for g in range(ng)]
            C = [sum(q[g][i] for g in range(ng)) for i in range(nh)]
            pairs = 0
            for g in range(ng):
                for i in range(nh):
                    if q[g][i] > 0:
                        self.P[a[g]][b[i]] += (q[g][i] << 20) // (R[g] + C[i] - q[g][i])
                        pairs += 1
            s = self.sizes
            s[0] += 1
            s[1] += ng
            s[2] += nh
            s[5] += oa
            s[6] += ob
            s[7] += pairs

    def state(self):
        def tab(rows, cap):
            out = np.zeros((cap, 2), dtype=np.int32)
            out[:, 0] = -1
            for k, r in enumerate(rows):
                out[k] = r
            return out
        sizes = list(self.sizes)
        sizes[3], sizes[4] = len(self.gt_tab), len(self.hyp_tab)
        return dict(sizes=np.array(sizes, dtype=np.int32), gt_tab=tab(self.gt_tab, self.acap), hyp_tab=tab(self.hyp_tab, self.bcap),
                    align=np.array(self.P, dtype=np.int64).reshape(self.acap, self.bcap))


def hota_align(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, any_label=False, acap=64, bcap=64, label_at=5, chunks=None):
    """one clip -> dict of ALIGN_KEYS; chunks: the same through one carried state fed in chunks along T"""
    T = gt_boxes.shape[0]
    st = Align(any_label, acap, bcap)
    t0 = 0
    for L in (chunks or [T]):
        s = slice(t0, t0 + L)
        st.clip(gt_boxes[s], gt_counts[s], gt_ids[s], hyp_boxes[s], hyp_counts[s], hyp_ids[s], label_at)
        t0 += L
    assert t0 == T
    return st.state()


def lookup(ids, tab):
    """the row of every id in a finished table [cap][2] (ids distinct), -1 for ids < 0 and ids not in it"""
    rows = {int(r[0]): k for k, r in enumerate(tab)}
    return [rows.get(int(v), -1) if int(v) >= 0 else -1 for v in ids]


def hota_frames(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, al, thresholds=THRESHOLDS, any_label=False, label_at=5,
                state=None):
    """pass 2, the match and the counts of the frames given, from the finished alignment `al` -> dict of FRAME_KEYS + COUNT_KEYS;
    state: a dict with tp, loc, pairs that the counts continue"""
    T, gcap, _ = gt_boxes.shape
    hcap = hyp_boxes.shape[1]
    if hyp_ids.ndim == 3:
        hyp_ids = hyp_ids[:, :, 0]
    acap, bcap = al["gt_tab"].shape[0], al["hyp_tab"].shape[0]
    na, nb = min(max(int(al["sizes"][3]), 0), acap), min(max(int(al["sizes"][4]), 0), bcap)
    thr = [f32(v) for v in thresholds]
    out = dict(w=np.zeros((T, gcap, hcap), dtype=np.int32), dims=np.zeros((T, 2), dtype=np.int32),
               gt_ent=np.full((T, gcap), -1, dtype=np.int32), hyp_ent=np.full((T, hcap), -1, dtype=np.int32),
               row_to_col=np.full((T, gcap), -1, dtype=np.int32))
    tp = [0] * len(thr) if state is None else [int(v) for v in state["tp"]]
    loc = [0] * len(thr) if state is None else [int(v) for v in state["loc"]]
    pairs = np.zeros((len(thr), acap, bcap), dtype=np.int32) if state is None else state["pairs"].copy()
    for t in range(T):
        ng, nh = counts_of(gt_counts, t, gcap), counts_of(hyp_counts, t, hcap)
        a, b = lookup(gt_ids[t, :ng], al["gt_tab"][:na]), lookup(hyp_ids[t, :nh], al["hyp_tab"][:nb])
        q, iou = similarity(gt_boxes[t, :ng], hyp_boxes[t, :nh], a, b, any_label, label_at)
        out["dims"][t] = [ng, nh]
        out["gt_ent"][t, :ng], out["hyp_ent"][t, :nh] = a, b
        W = [[0] * hcap for _ in range(gcap)]
        for g in range(ng):
            for i in range(nh):
                if q[g][i] > 0:
                    P = int(al["align"][a[g], b[i]])
                    n = int(al["gt_tab"][a[g], 1]) + int(al["hyp_tab"][b[i], 1])
                    W[g][i] = 1 + (P * q[g][i]) // (S * n - P)
        out["w"][t] = W
        r2c, _, _ = isr.assign_max(out["w"][t], ng, nh)
        out["row_to_col"][t] = r2c
        for g in range(ng):
            i = int(r2c[g])
            if i < 0:
                continue
            level = sum(1 for v in thr if iou[g][i] >= v)
            if level >= 1:
                tp[level - 1] += 1
                loc[level - 1] += q[g][i]
                pairs[level - 1, a[g], b[i]] += 1
    out.update(tp=np.array(tp, dtype=np.int32), loc=np.array(loc, dtype=np.int64), pairs=pairs)
    return out


def hota_score(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, thresholds=THRESHOLDS, any_label=False, acap=64, bcap=64,
               label_at=5, chunks=None):
    """one clip -> dict of ALL_KEYS (+ thresholds); chunks: both passes fed in chunks along T, the frame arrays concatenated"""
    x = (gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids)
    T = gt_boxes.shape[0]
    al = hota_align(*x, any_label=any_label, acap=acap, bcap=bcap, label_at=label_at, chunks=chunks)
    parts, state, t0 = [], None, 0
    for L in (chunks or [T]):
        state = hota_frames(*[v[t0:t0 + L] for v in x], al, thresholds, any_label, label_at, state)
        parts.append(state)
        t0 += L
    out = dict(al, thresholds=np.asarray(thresholds, dtype=np.float32).copy())
    for k in FRAME_KEYS:
        out[k] = np.concatenate([p[k] for p in parts])
    for k in COUNT_KEYS:
        out[k] = parts[-1][k]
    return out


# ---------------------------------------------------------------------------------------------------------------- the float rule
def trackeval_rule(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, thresholds=THRESHOLDS, any_label=False, label_at=5):
    """TrackEval's HOTA on one clip in float64 -> dict(TP [n_thr] ints, HOTA, DetA, AssA, LocA [n_thr] float64).  The similarity is the
    float32 IoU under this build's validity rule (labels, ids >= 0); a matched pair is a TP at threshold k when its float32 IoU >= thr[k]."""
    from scipy.optimize import linear_sum_assignment
    T, gcap, _ = gt_boxes.shape
    hcap = hyp_boxes.shape[1]
    gids = sorted({int(v) for t in range(T) for v in gt_ids[t, :counts_of(gt_counts, t, gcap)] if v >= 0})
    hids = sorted({int(v) for t in range(T) for v in hyp_ids[t, :counts_of(hyp_counts, t, hcap)] if v >= 0})
    ga, hb = {v: k for k, v in enumerate(gids)}, {v: k for k, v in enumerate(hids)}
    thr = [f32(v) for v in thresholds]
    pot = np.zeros((len(gids), len(hids)))
    n_a, n_b = np.zeros(len(gids)), np.zeros(len(hids))
    frames = []
    for t in range(T):
        ng, nh = counts_of(gt_counts, t, gcap), counts_of(hyp_counts, t, hcap)
        a = [ga.get(int(v), -1) for v in gt_ids[t, :ng]]
        b = [hb.get(int(v), -1) for v in hyp_ids[t, :nh]]
        _, iou = similarity(gt_boxes[t, :ng], hyp_boxes[t, :nh], a, b, any_label, label_at)
        sim = np.array([[float(v) if v is not None and v > 0 else 0.0 for v in row] for row in iou], dtype=np.float64).reshape(ng, nh)
        for g in a:
            if g >= 0:
                n_a[g] += 1
        for i in b:
            if i >= 0:
                n_b[i] += 1
        den = sim.sum(axis=0)[None, :] + sim.sum(axis=1)[:, None] - sim
        share = np.where(den > 0, sim / np.where(den > 0, den, 1.0), 0.0)
        for g in range(ng):
            for i in range(nh):
                if sim[g, i] > 0:
                    pot[a[g], b[i]] += share[g, i]
        frames.append((a, b, sim, iou))
    score = pot / np.maximum(1e-300, n_a[:, None] + n_b[None, :] - pot)
    TP = np.zeros(len(thr), dtype=np.int64)
    loc = np.zeros(len(thr))
    m = np.zeros((len(thr), len(gids), len(hids)))
    for a, b, sim, iou in frames:
        if not sim.size:
            continue
        A = np.array([[score[a[g], b[i]] if a[g] >= 0 and b[i] >= 0 else 0.0 for i in range(len(b))] for g in range(len(a))]).reshape(sim.shape)
        rows, cols = linear_sum_assignment(-(A * sim))
        for g, i in zip(rows, cols):
            if not sim[g, i] > 0:
                continue
            for k, v in enumerate(thr):
                if iou[g][i] >= v:
                    TP[k] += 1
                    loc[k] += sim[g, i]
                    m[k, a[g], b[i]] += 1
    gt = sum(counts_of(gt_counts, t, gcap) for t in range(T))
    hyp = sum(counts_of(hyp_counts, t, hcap) for t in range(T))
    A = m / np.maximum(1.0, n_a[None, :, None] + n_b[None, None, :] - m)
    AssA = (m * A).sum(axis=(1, 2)) / np.maximum(1.0, TP)
    DetA = TP / np.maximum(1.0, gt + hyp - TP)
    return dict(TP=TP, HOTA=np.sqrt(DetA * AssA), DetA=DetA, AssA=AssA, LocA=np.where(TP > 0, loc / np.maximum(1.0, TP), 1.0))


# ---------------------------------------------------------------------------------------------------------------- scenes
def separated_clip(seed, T=12, slots=5, gcap=8, hcap=8):
    """objects in slots 0.18 apart, boxes 0.1 wide with jitter <= 0.04: a ground-truth box overlaps the hypothesis of its own slot only.
    Hypotheses miss frames, change ids and appear without ground truth."""
    rs = np.random.RandomState(seed)
    s = dict(gt_boxes=np.zeros((T, gcap, 8), dtype=np.float32), gt_counts=np.zeros(T, dtype=np.int32),
             gt_ids=np.full((T, gcap), -1, dtype=np.int32), hyp_boxes=np.zeros((T, hcap, 8), dtype=np.float32),
             hyp_counts=np.zeros(T, dtype=np.int32), hyp_ids=np.full((T, hcap), -1, dtype=np.int32))
    hid = list(range(100, 100 + slots))
    nxt = 100 + slots
    for t in range(T):
        g = h = 0
        for k in range(slots):
            x = 0.1 + 0.18 * k
            if rs.rand() < 0.1:
                hid[k], nxt = nxt, nxt + 1                       # an identity switch
            if rs.rand() < 0.85:
                s["gt_boxes"][t, g] = [x, 0.5, 0.1, 0.1, 1.0, k % 2, 1.0, 0]
                s["gt_ids"][t, g] = k
                g += 1
            if rs.rand() < 0.85:
                j = (rs.rand(2) - 0.5) * 0.08
                s["hyp_boxes"][t, h] = [x + j[0], 0.5 + j[1], 0.1, 0.1, 0.9, k % 2, 0.8, 0]
                s["hyp_ids"][t, h] = hid[k]
                h += 1
        s["gt_counts"][t], s["hyp_counts"][t] = g, h
    return s


def hand_example():
    """two far-apart objects, T = 4, hypotheses equal to the ground truth, ids swapped after frame 2"""
    T = 4
    boxes = np.zeros((T, 2, 8), dtype=np.float32)
    boxes[:, 0] = [0.2, 0.5, 0.1, 0.1, 1.0, 0, 1.0, 0]
    boxes[:, 1] = [0.7, 0.5, 0.1, 0.1, 1.0, 0, 1.0, 0]
    ids = np.array([[0, 1]] * T, dtype=np.int32)
    hyp_ids = np.array([[0, 1], [0, 1], [1, 0], [1, 0]], dtype=np.int32)
    two = np.full(T, 2, dtype=np.int32)
    return dict(gt_boxes=boxes, gt_counts=two, gt_ids=ids, hyp_boxes=boxes.copy(), hyp_counts=two.copy(), hyp_ids=hyp_ids)


_REFS = {}


def scene_ref(name, any_label, acap=None, bcap=None):
    """the restatement on an identity_score_ref scene, computed once per (scene, any_label, acap, bcap)"""
    s, ac, bc = isr.scene(name)
    key = (name, bool(any_label), acap or ac, bcap or bc)
    if key not in _REFS:
        _REFS[key] = hota_score(*[s[k] for k in INPUTS], any_label=any_label, acap=key[2], bcap=key[3])
    return _REFS[key]


def edge_clip():
    """T = 5, gcap 6, hcap 7: an empty frame on either side, ids < 0, an id twice in a frame on either side, a NaN box on either side,
    a pair whose boxes are equal (IoU 1) and a pair of IoU exactly 0.5 -> the scene dict"""
    T, gcap, hcap = 5, 6, 7
    s = dict(gt_boxes=np.zeros((T, gcap, 8), dtype=np.float32), gt_counts=np.array([4, 0, 5, 4, 3], dtype=np.int32),
             gt_ids=np.full((T, gcap), -1, dtype=np.int32), hyp_boxes=np.zeros((T, hcap, 8), dtype=np.float32),
             hyp_counts=np.array([5, 3, 0, 4, 4], dtype=np.int32), hyp_ids=np.full((T, hcap), -1, dtype=np.int32))
    rs = np.random.RandomState(4)
    for t in range(T):
        for g in range(gcap):
            s["gt_boxes"][t, g] = [0.1 + 0.16 * g, 0.5, 0.22, 0.2, 1.0, 0, 1.0, 0]        # wider than the spacing: neighbours overlap
            s["gt_ids"][t, g] = 10 + g
        for i in range(hcap):
            j = (rs.rand(2) - 0.5) * 0.06
            s["hyp_boxes"][t, i] = [0.1 + 0.16 * (i % gcap) + j[0], 0.5 + j[1], 0.22, 0.2, 0.9, 0, 0.8, 0]
            s["hyp_ids"][t, i] = 50 + (i + t // 3) % hcap
    s["gt_ids"][0, 1] = -1                                       # ids < 0 on either side
    s["hyp_ids"][0, 2] = -3
    s["gt_ids"][3, 2] = s["gt_ids"][3, 0]                        # an id twice in a frame, on either side
    s["hyp_ids"][3, 3] = s["hyp_ids"][3, 1]
    s["gt_boxes"][4, 1, 2] = np.nan                              # NaN boxes
    s["hyp_boxes"][4, 2, 0] = np.nan
    s["hyp_boxes"][0, 0] = s["gt_boxes"][0, 0]                   # IoU 1
    s["hyp_boxes"][0, 3, :4] = [s["gt_boxes"][0, 3, 0], 0.45, 0.22, 0.1]     # the upper half: IoU 0.5
    return s
