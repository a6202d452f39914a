"""Plain restatement of identity scoring ("Identity scoring"), for the tests.

  * TRAJECTORIES.  Per clip a ground-truth table of at most acap rows [id, boxes], one per distinct gt id >= 0 in order of first
    appearance (within a frame: row order), and a hypothesis table of at most bcap rows built the same way.  A box whose id is < 0, or
    whose id finds its table full (counted as that side's overflow), has no trajectory.
  * OVERLAP.  n[a][b] = the valid pairs (g, i) over all frames with g of gt trajectory a and i of hypothesis trajectory b; valid is
    track scoring's: bbox_iou >= thr as float32, equal labels as floats unless any_label.  Nothing is claimed.
  * ASSIGNMENT.  The shortest-augmenting-path Hungarian method with integer potentials on c = -w, step for step as DESIGN.md states
    it (the lowest column on ties), on the orientation whose row count is the smaller; and a brute force over permutations.

Everything is a Python list walked one element at a time; the IoU is orc.bbox_iou, so its float32 bits are the oracle's.  Test
infrastructure only.
"""
import itertools

import numpy as np

from oracle import oracle as orc

import track_score_ref as tsr

f32 = np.float32
IDENT_INTS = 8
KEYS = ("sizes", "gt_tab", "hyp_tab", "overlap")
ALL_KEYS = KEYS + ("gt_to_hyp", "hyp_to_gt", "idtp")
INPUTS = ("gt_boxes", "gt_counts", "gt_ids", "hyp_boxes", "hyp_counts", "hyp_ids")
INF = 0x7fffffff


class Identity(object):
    """the state a resumed run carries: the sizes, both tables and the overlap"""

    def __init__(self, thr, any_label, acap, bcap):
        self.thr, self.any_label, self.acap, self.bcap = f32(thr), bool(any_label), int(acap), int(bcap)
        self.sizes = [0] * IDENT_INTS
        self.gt_tab, self.hyp_tab = [], []                       # rows [id, boxes]
        self.overlap = np.zeros((self.acap, self.bcap), dtype=np.int64)

    @staticmethod
    def rows_of(ids, table, cap):
        """the table row of every box in row order, opened where the id is new and the table has room -> (rows, overflow boxes)"""
        rows, over = [], 0
        for v in ids:
            v, e = int(v), -1
            if v >= 0:
                for k, r in enumerate(table):
                    if r[0] == v:
                        e = k
                if e < 0:
                    if len(table) < cap:
                        table.append([v, 0])
                        e = len(table) - 1
                    else:
                        over += 1
            if e >= 0:
                table[e][1] += 1
            rows.append(e)
        return rows, over

    def frame(self, gt_rows, gt_ids, hyp_rows, hyp_ids, label_at):
        a, oa = self.rows_of(gt_ids, self.gt_tab, self.acap)
        b, ob = self.rows_of(hyp_ids, self.hyp_tab, self.bcap)
        pairs = 0
        for g in range(len(gt_rows)):
            for i in range(len(hyp_rows)):
                if a[g] < 0 or b[i] < 0:
                    continue
                if not self.any_label and f32(gt_rows[g][5]) != f32(hyp_rows[i][label_at]):
                    continue
                if f32(orc.bbox_iou(gt_rows[g][:4], hyp_rows[i][:4])) >= self.thr:
                    self.overlap[a[g], b[i]] += 1
                    pairs += 1
        s = self.sizes
        s[0] += 1
        s[1] += len(gt_rows)
        s[2] += len(hyp_rows)
        s[5] += oa
        s[6] += ob
        s[7] += pairs

    def clip(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, label_at=5):
        T, gcap, _ = gt_boxes.shape
        hcap = hyp_boxes.shape[1]
        if hyp_ids.ndim == 3:
            hyp_ids = hyp_ids[:, :, 0]
        for t in range(T):
            ng, nh = min(max(int(gt_counts[t]), 0), gcap), min(max(int(hyp_counts[t]), 0), hcap)
            self.frame(gt_boxes[t, :ng], gt_ids[t, :ng], hyp_boxes[t, :nh], hyp_ids[t, :nh], label_at)

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
                    overlap=self.overlap.astype(np.int32))


def identity_overlap(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, thr=0.5, any_label=False, acap=64, bcap=64, label_at=5,
                     chunks=None):
    """one clip -> dict of KEYS (arrays without the clip axis); chunks: the same through one carried state fed in chunks along T"""
    T = gt_boxes.shape[0]
    st = Identity(thr, any_label, acap, bcap)
    t0 = 0
    for L in (chunks or [T]):
        s = slice(t0, t0 + L)
        st.clip(gt_boxes[s], gt_counts[s], gt_ids[s], hyp_boxes[s], hyp_counts[s], hyp_ids[s], label_at)
        t0 += L
    assert t0 == T
    return st.state()


def assign_max(w, rows=None, cols=None):
    """w [rcap, ccap] integers, the rows x cols block in use -> (row_to_col [rcap], col_to_row [ccap], total): DESIGN.md's steps"""
    w = np.asarray(w)
    rcap, ccap = w.shape
    rows = rcap if rows is None else min(max(int(rows), 0), rcap)
    cols = ccap if cols is None else min(max(int(cols), 0), ccap)
    tr = cols < rows                                             # the solve's rows are the matrix's columns
    N, M = (cols, rows) if tr else (rows, cols)
    cost = (lambda i, j: -int(w[j - 1, i - 1])) if tr else (lambda i, j: -int(w[i - 1, j - 1]))
    u, v, p, way = [0] * (N + 1), [0] * (M + 1), [0] * (M + 1), [0] * (M + 1)
    for i in range(1, N + 1):
        p[0] = i
        j0 = 0
        minv, used = [INF] * (M + 1), [False] * (M + 1)
        for _ in range(M + 1):
            used[j0] = True
            i0 = p[j0]
            delta, j1 = None, -1
            for j in range(1, M + 1):
                if used[j]:
                    continue
                cur = cost(i0, j) - u[i0] - v[j]
                if cur < minv[j]:
                    minv[j] = cur
                    way[j] = j0
                if delta is None or minv[j] < delta:             # strict: the lowest column on ties
                    delta, j1 = minv[j], j
            for j in range(M + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        else:
            raise AssertionError("more than M + 1 steps")
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    r2c, c2r, total = [-1] * rcap, [-1] * ccap, 0
    for j in range(1, M + 1):
        i = p[j]
        if i == 0:
            continue
        r, c = (j - 1, i - 1) if tr else (i - 1, j - 1)
        if int(w[r, c]) == 0:                                    # a pair without weight is reported as unassigned
            continue
        r2c[r], c2r[c] = c, r
        total += int(w[r, c])
    return np.array(r2c, dtype=np.int32), np.array(c2r, dtype=np.int32), total


def brute_force(w):
    """the largest total over all one-to-one assignments of a small matrix"""
    w = np.asarray(w)
    if w.shape[0] > w.shape[1]:
        w = w.T
    n, m = w.shape
    best = 0
    for perm in itertools.permutations(range(m), n):
        best = max(best, sum(int(w[r, c]) for r, c in enumerate(perm)))
    return best


def check_assignment(w, rows, cols, r2c, c2r, total):
    """one-to-one, consistent both ways, inside the block, no zero-weight pair, and the total is the sum of the chosen weights"""
    w = np.asarray(w)
    rcap, ccap = w.shape
    assert len(r2c) == rcap and len(c2r) == ccap
    s = 0
    for r in range(rcap):
        c = int(r2c[r])
        if c < 0:
            assert c == -1
            continue
        assert r < rows and 0 <= c < cols and int(c2r[c]) == r and int(w[r, c]) != 0
        s += int(w[r, c])
    for c in range(ccap):
        r = int(c2r[c])
        assert r == -1 or (0 <= r < rows and c < cols and int(r2c[r]) == c)
    assert s == int(total)


def identity_score(*args, **kw):
    """identity_overlap, then assign_max on its overlap and trajectory counts -> dict of ALL_KEYS"""
    r = identity_overlap(*args, **kw)
    r["gt_to_hyp"], r["hyp_to_gt"], idtp = assign_max(r["overlap"], r["sizes"][3], r["sizes"][4])
    r["idtp"] = np.int64(idtp)
    return r


def counts(r):
    """-> (IDTP, IDFN, IDFP)"""
    return int(r["idtp"]), int(r["sizes"][1]) - int(r["idtp"]), int(r["sizes"][2]) - int(r["idtp"])


def splits(r):
    """ground-truth trajectories that overlap two or more hypothesis trajectories"""
    return int(((r["overlap"] > 0).sum(axis=1) >= 2).sum())


# ---------------------------------------------------------------------------------------------------------------- scenes
def hyp_ids_of(s):
    """the distinct hypothesis ids >= 0 of the rows in use"""
    ids = s["hyp_ids"] if s["hyp_ids"].ndim == 2 else s["hyp_ids"][:, :, 0]
    out = set()
    for t in range(ids.shape[0]):
        out.update(int(v) for v in ids[t, :min(max(int(s["hyp_counts"][t]), 0), ids.shape[1])] if v >= 0)
    return out


_WIDE = {}


def wide_scene():
    """T = 12, gcap 96, hcap 160, 80 objects: more than 64 gt trajectories, more than 128 hypothesis trajectories -> (scene, acap, bcap)"""
    if "s" not in _WIDE:
        s = tsr.make_scene(12, 96, 160, 80, 11)
        _WIDE["s"] = (s, 128, 64 * ((len(hyp_ids_of(s)) + 63) // 64) + 64)
    return _WIDE["s"]


_SCENES, _REFS = {}, {}


def scene(name):
    """a track_score_ref scene (or "ident_wide") with table sizes that hold every trajectory -> (scene, acap, bcap)"""
    if name not in _SCENES:
        if name == "ident_wide":
            _SCENES[name] = wide_scene()
        else:
            s, ocap = tsr.scene(name)
            _SCENES[name] = (s, ocap, len(hyp_ids_of(s)) + 3)
    return _SCENES[name]


def scene_ref(name, any_label, acap=None, bcap=None):
    """the restatement on a scene, computed once per (scene, any_label, acap, bcap)"""
    s, ac, bc = scene(name)
    key = (name, bool(any_label), acap or ac, bcap or bc)
    if key not in _REFS:
        _REFS[key] = identity_score(*[s[k] for k in INPUTS], thr=0.5, any_label=any_label, acap=key[2], bcap=key[3])
    return _REFS[key]


# DESIGN.md's first example: track scoring's five frames.  n = [[2, 3]], gt 5, hyp 6
WORKED_SIZES = [5, 5, 6, 1, 2, 0, 0, 5]
WORKED_GT_TAB = [[7, 5]]
WORKED_HYP_TAB = [[0, 2], [1, 4]]
WORKED_OVERLAP = [[2, 3]]
WORKED_IDTP, WORKED_IDFN, WORKED_IDFP = 3, 2, 3
# ... and its second: best-first greedy takes 5 + 0, the optimum is 4 + 4
ANTI_GREEDY = [[5, 4], [4, 0]]
