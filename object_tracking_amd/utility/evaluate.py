"""Track scoring on the host side: MOT ground truth in, CLEAR-MOT figures out ("Track scoring").

The counting itself runs on the device (mi355_dt.Context.track_score / dt_track_score).  This module only prepares its input
from MOT `gt.txt` text and turns its integer output into the usual figures; nothing here touches the GPU.
"""
import numpy as np

DT_BOX_FLOATS = 8
TOTAL_FIELDS = ("frames", "gt", "hyp", "matches", "switches", "fragments", "overflow")
MOSTLY_TRACKED, MOSTLY_LOST = 0.8, 0.2


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
