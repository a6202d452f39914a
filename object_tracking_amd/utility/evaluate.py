"""Scoring on the host side ("Track scoring", "Identity scoring", "HOTA scoring" and "Detection scoring"): MOT ground truth in,
CLEAR-MOT, identity and HOTA figures out; annotation records in, per-class average precision out.

The counting itself runs on the device (mi355_dt.Context.track_score / dt_track_score; Context.identity_score /
dt_identity_overlap, dt_assign_max; Context.hota_score / dt_hota_align, dt_hota_weights, dt_hota_count; Context.detect_score / dt_detect_match, dt_detect_rank).  This module only prepares its input and turns its integer output into the usual figures, in float64; nothing
here touches the GPU.
"""
import numpy as np

DT_BOX_FLOATS = 8
TOTAL_FIELDS = ("frames", "gt", "hyp", "matches", "switches", "fragments", "overflow")
MOSTLY_TRACKED, MOSTLY_LOST = 0.8, 0.2
HOTA_THRESHOLDS = np.array([0.05 * k for k in range(1, 20)], dtype=np.float32)      # 0.05 .. 0.95, the measure's own
HOTA_SCALE = 1048576                                                                # DT_ASSIGN_IOU_SCALE: loc sums trunc(IoU * 2^20)
HOTA_ARRAYS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")


def _host(a):
    """a device tensor or an array -> numpy"""
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _figures(totals, miou_sum, objs):
    frames, gt, hyp, matches, switches, fragments, overflow = (int(v) for v in totals[:7])
    misses, fps = gt - matches, hyp - matches
    ratios = [float(o[3]) / float(o[2]) for o in objs if o[2] > 0]
    return dict(frames=frames, gt=gt, hyp=hyp, matches=matches, misses=misses, false_positives=fps, switches=switches,
                fragments=fragments, overflow=overflow, objects=len(objs),
                mota=1.0 - float(misses + fps + switches) / float(gt) if gt > 0 else float("nan"),
                motp=None if miou_sum is None else (miou_sum / matches if matches > 0 else float("nan")),
                mostly_tracked=sum(1 for r in ratios if r >= MOSTLY_TRACKED), mostly_lost=sum(1 for r in ratios if r <= MOSTLY_LOST))


def summarize(result):
    """A Context.track_score result (or the results of the chunks of one run, in order, as a list) -> dict(clips=[...], pooled=...).
    Every entry has frames, gt, hyp, matches, misses, false_positives, switches, fragments, overflow, objects and
      mota            1 - (misses + false_positives + switches) / gt; nan when gt is 0
      motp            the mean IoU of the matches, summed in float64 (nan without a match; None when the result has no `miou`)
      mostly_tracked  objects with matched / present >= 0.8;  mostly_lost: <= 0.2
    `pooled` adds the counts of all clips before the ratios are taken (objects of different clips are different objects).  Objects
    scored without memory (`overflow`) are in the counts but in neither of the last two."""
    parts = list(result) if isinstance(result, (list, tuple)) else [result]
    last = parts[-1]                                   # totals and objects accumulate along a resumed run
    totals, objs, nobjs = _host(last["totals"]), _host(last["objs"]), _host(last["nobjs"])
    n = totals.shape[0]
    have_iou = all(p.get("miou") is not None for p in parts)
    sums = np.zeros(n, dtype=np.float64)
    if have_iou:
        for p in parts:
            sums += _host(p["miou"]).astype(np.float64).reshape(n, -1).sum(axis=1)
    clips, rows = [], []
    for k in range(n):
        o = [tuple(int(v) for v in r) for r in objs[k, :int(nobjs[k])]]
        rows += o
        clips.append(_figures(totals[k], float(sums[k]) if have_iou else None, o))
    pooled = _figures(totals.astype(np.int64).sum(axis=0) if n else np.zeros(8, dtype=np.int64), float(sums.sum()) if have_iou else None, rows)
    return dict(clips=clips, pooled=pooled)


def _identity_figures(idtp, gt, hyp, gt_tracks, hyp_tracks, overflow):
    nan = float("nan")
    return dict(idtp=idtp, idfn=gt - idtp, idfp=hyp - idtp, gt=gt, hyp=hyp, gt_tracks=gt_tracks, hyp_tracks=hyp_tracks, overflow=overflow,
                idp=float(idtp) / float(hyp) if hyp > 0 else nan, idr=float(idtp) / float(gt) if gt > 0 else nan,
                idf1=2.0 * float(idtp) / float(gt + hyp) if gt + hyp > 0 else nan)


def identity(result):
    """A Context.identity_score result (of a resumed run: its last one; a list's last entry is taken) -> dict(clips=[...], pooled=...).
    Every entry has idtp, idfn = gt - idtp, idfp = hyp - idtp, gt, hyp (boxes), gt_tracks, hyp_tracks (trajectories), overflow (boxes
    of either side whose id found its table full: they count in gt / hyp and can never be identity true positives) and
      idp = idtp / hyp, idr = idtp / gt, idf1 = 2 idtp / (gt + hyp)       in float64; nan where the denominator is 0
    `pooled` adds the counts of all clips before the ratios are taken."""
    last = result[-1] if isinstance(result, (list, tuple)) else result
    sizes, idtp = _host(last["sizes"]).astype(np.int64), _host(last["idtp"]).astype(np.int64)
    clips = [_identity_figures(int(idtp[k]), int(s[1]), int(s[2]), int(s[3]), int(s[4]), int(s[5] + s[6])) for k, s in enumerate(sizes)]
    tot = sizes.sum(axis=0) if len(sizes) else np.zeros(8, dtype=np.int64)
    pooled = _identity_figures(int(idtp.sum()), int(tot[1]), int(tot[2]), int(tot[3]), int(tot[4]), int(tot[5] + tot[6]))
    return dict(clips=clips, pooled=pooled)


def _hota_sums(sizes, gt_tab, hyp_tab, tp, loc, pairs):
    """one clip's buckets -> what pools over clips: per threshold TP, L, sum m A, sum m m / n_a, sum m m / n_b; and gt, hyp"""
    n_a = gt_tab[:, 1].astype(np.float64)[None, :, None]
    n_b = hyp_tab[:, 1].astype(np.float64)[None, None, :]
    suffix = lambda x: np.cumsum(x[::-1], axis=0)[::-1]          # a pair that passes threshold k passes every lower one
    TP, L, m = suffix(tp.astype(np.int64)), suffix(loc.astype(np.int64)), suffix(pairs.astype(np.int64)).astype(np.float64)
    ass = (m * (m / np.maximum(1.0, n_a + n_b - m))).sum(axis=(1, 2))
    re = (m * (m / np.maximum(1.0, n_a))).sum(axis=(1, 2))
    pr = (m * (m / np.maximum(1.0, n_b))).sum(axis=(1, 2))
    return dict(TP=TP, L=L, ass=ass, re=re, pr=pr, gt=int(sizes[1]), hyp=int(sizes[2]))


def _hota_figures(s, gt_tracks, hyp_tracks, overflow):
    TP = s["TP"].astype(np.float64)
    FN, FP = s["gt"] - TP, s["hyp"] - TP
    one = np.maximum(1.0, TP)
    out = dict(TP=s["TP"].copy(), FN=s["gt"] - s["TP"], FP=s["hyp"] - s["TP"], gt=s["gt"], hyp=s["hyp"], gt_tracks=gt_tracks,
               hyp_tracks=hyp_tracks, overflow=overflow)
    out["DetA"], out["DetRe"], out["DetPr"] = TP / np.maximum(1.0, TP + FN + FP), TP / np.maximum(1.0, TP + FN), TP / np.maximum(1.0, TP + FP)
    out["AssA"], out["AssRe"], out["AssPr"] = s["ass"] / one, s["re"] / one, s["pr"] / one
    out["HOTA"] = np.sqrt(out["DetA"] * out["AssA"])
    out["LocA"] = np.where(s["TP"] > 0, s["L"].astype(np.float64) / (float(HOTA_SCALE) * one), 1.0)
    for k in HOTA_ARRAYS:
        out[k.lower()] = float(out[k].mean())
    out["hota0"], out["loca0"] = float(out["HOTA"][0]), float(out["LocA"][0])
    return out


def hota(result):
    """A Context.hota_score result (of a resumed run: its last one; a list's last entry is taken) -> dict(clips=[...], pooled=...).
    Every entry has, per threshold (arrays of len(thresholds), float64 but for the counts):
      TP, FN = gt - TP, FP = hyp - TP         TP at threshold k: the matched pairs whose IoU reaches it (the buckets k and above)
      DetA = TP / (TP + FN + FP), DetRe = TP / (TP + FN), DetPr = TP / (TP + FP)
      AssA = sum m A / TP with A(a, b) = m / (n_a + n_b - m), m[a][b] the pairs of the trajectories a, b among the TP and n their boxes;
      AssRe = sum m (m / n_a) / TP, AssPr = sum m (m / n_b) / TP
      HOTA = sqrt(DetA AssA);  LocA = loc / (2^20 TP), the mean truncated IoU of the TP
    their means over the thresholds (hota, deta, assa, detre, detpr, assre, asspr, loca), the first threshold's hota0 and loca0, and
    gt, hyp (boxes), gt_tracks, hyp_tracks (trajectories), overflow (boxes whose id found its table full).
    Every denominator is max(1, .) and LocA is 1.0 where TP = 0 -- TrackEval's conventions, so that figures compare with published ones
    (summarize and identity return nan there instead).  `pooled` adds TP, gt, hyp, loc and the sums over m of all clips before the ratios
    are taken (objects of different clips are different objects)."""
    last = result[-1] if isinstance(result, (list, tuple)) else result
    sizes, gt_tab, hyp_tab = _host(last["sizes"]).astype(np.int64), _host(last["gt_tab"]), _host(last["hyp_tab"])
    tp, loc, pairs = _host(last["tp"]), _host(last["loc"]), _host(last["pairs"])
    n_thr = tp.shape[1]
    sums = [_hota_sums(sizes[k], gt_tab[k], hyp_tab[k], tp[k], loc[k], pairs[k]) for k in range(len(sizes))]
    clips = [_hota_figures(s, int(sizes[k][3]), int(sizes[k][4]), int(sizes[k][5] + sizes[k][6])) for k, s in enumerate(sums)]
    tot = sizes.sum(axis=0) if len(sizes) else np.zeros(8, dtype=np.int64)
    pool = dict(TP=np.zeros(n_thr, dtype=np.int64), L=np.zeros(n_thr, dtype=np.int64), ass=np.zeros(n_thr), re=np.zeros(n_thr),
                pr=np.zeros(n_thr), gt=0, hyp=0)
    for s in sums:
        for k in pool:
            pool[k] = pool[k] + s[k]
    return dict(clips=clips, pooled=_hota_figures(pool, int(tot[3]), int(tot[4]), int(tot[5] + tot[6])),
                thresholds=np.asarray(last["thresholds"], dtype=np.float32).copy())


def gt_from_mot(lines, width, height, T, gcap, classes=None):
    """MOT `gt.txt` text -> (gt_boxes [T, gcap, 8] float32, gt_counts [T] int32, gt_ids [T, gcap] int32) of one sequence, the
    arrays Context.track_score takes once a clip axis is put in front.
    lines: the file's text or its lines; 9 comma-separated fields each: frame (from 1), identity, box left, top, width, height (pixels),
    the consider flag (rows with 0 are dropped), class, visibility.  width, height: the sequence's frame size.
    A box becomes x, y = its centre and w, h, each divided by the frame size (nothing is clipped: a box may leave the frame);
    float 4 is 1, float 5 the label, float 6 the visibility.  classes: {MOT class: label}; rows of other classes are dropped
    (None: every class c, as label c - 1 -- the index in MultiObjDetTracker.LABELS_MOT17).  Frames beyond T are dropped;
    more than gcap boxes in a frame is an error.  Rows keep the file's order within a frame; ids in unused entries are -1."""
    if isinstance(lines, str):
        lines = lines.splitlines()
    boxes = np.zeros((T, gcap, DT_BOX_FLOATS), dtype=np.float32)
    counts = np.zeros(T, dtype=np.int32)
    ids = np.full((T, gcap), -1, dtype=np.int32)
    for ln in lines:
        ln = ln.strip()
        if not ln:
            continue
        f = ln.split(",")
        if len(f) != 9:
            raise ValueError("a gt.txt line has 9 comma-separated fields, got %d: %r" % (len(f), ln))
        t, ident = int(f[0]) - 1, int(f[1])
        left, top, w, h = (float(v) for v in f[2:6])
        flag, cls, vis = int(float(f[6])), int(f[7]), float(f[8])
        if flag == 0 or t < 0 or t >= T:
            continue
        if classes is None:
            label = cls - 1
        elif cls in classes:
            label = classes[cls]
        else:
            continue
        k = int(counts[t])
        if k >= gcap:
            raise ValueError("frame %d holds more than gcap = %d boxes" % (t + 1, gcap))
        boxes[t, k] = [(left + w / 2.0) / width, (top + h / 2.0) / height, w / width, h / height, 1.0, label, vis, 0.0]
        ids[t, k] = ident
        counts[t] = k + 1
    return boxes, counts, ids


# ---------------------------------------------------------------------------------------------------------------- detection scoring
COCO_THRESHOLDS = tuple(0.5 + 0.05 * i for i in range(10))      # .50:.05:.95
AP_METHODS = ("area", "voc11", "coco101")


def _curves(result):
    """-> (rank, ctp [n_thr, M], class per flat row [M] with -1 where the label takes no part, ngt [NC], ndet [n_thr, NC])"""
    rank, ctp = _host(result["rank"]), _host(result["ctp"])
    n_thr = rank.shape[0]
    ngt, ndet = _host(result["ngt"]).astype(np.int64), _host(result["ndet"]).astype(np.int64)
    lab = _host(result["labels"]).astype(np.float64).reshape(-1)
    ok = (lab >= 0) & (lab < ngt.shape[0]) & (lab == np.floor(lab))
    cls = np.where(ok, lab, -1).astype(np.int64)
    return rank.reshape(n_thr, -1), ctp.reshape(n_thr, -1), cls, ngt, ndet


def _curve(rank_k, ctp_k, cls, c, n):
    """the cumulative TP counts of class c in rank order"""
    sel = (rank_k >= 0) & (cls == c)
    out = np.zeros(n, dtype=np.float64)
    out[rank_k[sel]] = ctp_k[sel]
    return out, sel


def _ap(ctp, ngt, method):
    if ngt == 0:
        return float("nan")
    n = ctp.shape[0]
    if n == 0:
        return 0.0
    p = ctp / np.arange(1, n + 1, dtype=np.float64)
    r = ctp / float(ngt)
    if method == "area":
        env = np.maximum.accumulate(p[::-1])[::-1]
        return float(np.sum((r - np.concatenate([[0.0], r[:-1]])) * env))
    steps = {"voc11": 10, "coco101": 100}[method]
    env = np.maximum.accumulate(p[::-1])[::-1]                 # r does not decrease along the curve: max{p_j : r_j >= t} = env at the first such j
    t = np.arange(steps + 1, dtype=np.float64) / float(steps)
    first = np.searchsorted(r, t, side="left")
    vals = np.where(first < n, env[np.minimum(first, n - 1)], 0.0)
    return float(np.sum(vals) / float(steps + 1))


def average_precision(result, method="area"):
    """A Context.detect_score result (device tensors or arrays: rank, ctp, ngt, ndet, ntp, labels, thresholds) -> dict:
      ap          [n_thr, NC] float64: the AP of class c at threshold k; nan where the class has no ground truth (ngt = 0), 0 where
                  it has ground truth and no ranked detection
      map         [n_thr]: the mean over the classes with ground truth (nan without one);  map_all: the mean of map over the
                  thresholds -- COCO's mAP when the thresholds are COCO_THRESHOLDS
      ngt [NC], ndet, ntp [n_thr, NC], thresholds
    For threshold k and class c the curve has n = ndet points, p_j = ctp_j / (j + 1), r_j = ctp_j / ngt, j in rank order.
    method: "area" (VOC2010+): sum_j (r_j - r_{j-1}) * max_{j' >= j} p_j';  "voc11": the mean over t = i / 10, i = 0..10, of
    max{p_j : r_j >= t} (0 where there is none);  "coco101": the same over t = i / 100, i = 0..100."""
    if method not in AP_METHODS:
        raise ValueError("method must be one of %s" % (AP_METHODS,))
    rank, ctp, cls, ngt, ndet = _curves(result)
    n_thr, NC = rank.shape[0], ngt.shape[0]
    ap = np.full((n_thr, NC), np.nan, dtype=np.float64)
    for k in range(n_thr):
        for c in range(NC):
            if ngt[c] > 0:
                ap[k, c] = _ap(_curve(rank[k], ctp[k], cls, c, int(ndet[k, c]))[0], int(ngt[c]), method)
    have = ngt > 0
    m = ap[:, have].mean(axis=1) if have.any() else np.full(n_thr, np.nan)
    return dict(ap=ap, map=m, map_all=float(m.mean()) if have.any() else float("nan"), ngt=ngt, ndet=ndet,
                ntp=_host(result["ntp"]).astype(np.int64), thresholds=np.asarray(_host(result["thresholds"]), dtype=np.float64))


def precision_recall(result, k, c):
    """The curve of class c at threshold index k, in rank order -> dict(precision, recall [n] float64 (recall nan when the class has no
    ground truth), scores [n] float32 (the ranking score of the detection at each rank), tp [n] int64 (cumulative))."""
    rank, ctp, cls, ngt, ndet = _curves(result)
    n = int(ndet[k, c])
    cum, sel = _curve(rank[k], ctp[k], cls, c, n)
    scores = np.zeros(n, dtype=np.float32)
    scores[rank[k][sel]] = _host(result["scores"]).reshape(-1)[sel]
    with np.errstate(divide="ignore", invalid="ignore"):
        recall = cum / float(ngt[c]) if ngt[c] > 0 else np.full(n, np.nan)
    return dict(precision=cum / np.arange(1, n + 1, dtype=np.float64), recall=recall, scores=scores, tp=cum.astype(np.int64))


def gt_from_annotations(records, labels, gcap):
    """utility.preprocessing.parse_annotation records -> (gt_boxes [B, gcap, 8] float32, gt_counts [B] int32, gt_flags [B, gcap] int32),
    one frame per record, for Context.detect_score / KerasYOLO.score.
    A record: dict(width, height, object=[dict(name, xmin, ymin, xmax, ymax[, difficult])]).  A box becomes x, y = its centre and
    w, h, each divided by the record's width / height; float 4 is 1, float 5 the index of `name` in `labels`, float 6 is 1.
    Objects whose name is not in `labels` are dropped; a true 'difficult' key sets bit 0 of the flag (the row is ignored in scoring).
    More than gcap objects in a record is an error."""
    B = len(records)
    boxes = np.zeros((B, gcap, DT_BOX_FLOATS), dtype=np.float32)
    counts = np.zeros(B, dtype=np.int32)
    flags = np.zeros((B, gcap), dtype=np.int32)
    index = {name: i for i, name in enumerate(labels)}
    for b, rec in enumerate(records):
        W, H = float(rec["width"]), float(rec["height"])
        for o in rec["object"]:
            if o["name"] not in index:
                continue
            k = int(counts[b])
            if k >= gcap:
                raise ValueError("record %d holds more than gcap = %d objects" % (b, gcap))
            x0, y0, x1, y1 = float(o["xmin"]), float(o["ymin"]), float(o["xmax"]), float(o["ymax"])
            boxes[b, k] = [(x0 + x1) / 2.0 / W, (y0 + y1) / 2.0 / H, (x1 - x0) / W, (y1 - y0) / H, 1.0, index[o["name"]], 1.0, 0.0]
            flags[b, k] = 1 if int(o.get("difficult", 0)) else 0
            counts[b] = k + 1
    return boxes, counts, flags
