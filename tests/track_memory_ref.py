"""Plain restatement of the track-memory identity rule (`max_age`), for the tests.

The rule, as the kernel's documents state it.  Per clip (or stream) a TABLE of at most `tcap` entries, each
(box x y w h, label, id, age); age = frames since the track last had a box.  Frames in order, boxes in decode order:

  * box i takes the id of the entry j that is not yet claimed in this frame, has age <= max_age and the same label, and
    has the largest bbox_iou(box i, entry j's box) >= thr; ties go to the lowest j.  Otherwise it opens a new id.
  * gap = the claimed entry's age (-1 for a new id).
  * after the frame the table is: the frame's boxes in decode order (age 0), then the unclaimed entries with
    age + 1 <= max_age in their previous order (age + 1, box unchanged); entries beyond tcap are dropped.

Everything is a Python list walked one element at a time; the IoU is orc.bbox_iou, so its float32 bits are the oracle's.
`max_age` may differ from frame to frame (it belongs to the call, not to the table).  Test infrastructure only.
"""
import numpy as np

from oracle import oracle as orc


class TrackMemory(object):
    """the state a stream carries: the table and the next free id"""

    def __init__(self, tcap, thr):
        self.tcap, self.thr = int(tcap), float(thr)
        self.table = []          # entries [box4, label, id, age]
        self.next_id = 0
        self.dropped = 0         # entries the tcap cut has removed so far

    def frame(self, rows, max_age):
        """rows: the frame's boxes [n, 8] in decode order -> (ids, gaps), lists of n"""
        thr32 = np.float32(self.thr)
        claimed = [False] * len(self.table)
        ids, gaps = [], []
        for r in rows:
            best, bj = None, -1
            for j, (box, lab, _, age) in enumerate(self.table):
                if claimed[j] or age > max_age or np.float32(lab) != np.float32(r[5]):
                    continue
                iou = np.float32(orc.bbox_iou(r[:4], box))
                if iou >= thr32 and (best is None or iou > best):      # strictly better: ties stay with the lowest j
                    best, bj = iou, j
            if bj >= 0:
                claimed[bj] = True
                ids.append(self.table[bj][2]); gaps.append(self.table[bj][3])
            else:
                ids.append(self.next_id); gaps.append(-1)
                self.next_id += 1
        new = [[np.array(r[:4], dtype=np.float32), np.float32(r[5]), i, 0] for r, i in zip(rows, ids)]
        for j, (box, lab, tid, age) in enumerate(self.table):
            if not claimed[j] and age + 1 <= max_age:
                new.append([box, lab, tid, age + 1])
        self.dropped += max(0, len(new) - self.tcap)
        self.table = new[:self.tcap]
        return ids, gaps

    def clip(self, boxes, counts, max_age):
        """boxes [T, cap, 8], counts [T]; max_age an int or one per frame -> ids [T, cap], gaps [T, cap] (-1 in unused entries)"""
        T, cap, _ = boxes.shape
        ages = [int(max_age)] * T if np.isscalar(max_age) else [int(a) for a in max_age]
        assert len(ages) == T
        ids = np.full((T, cap), -1, dtype=np.int32)
        gaps = np.full((T, cap), -1, dtype=np.int32)
        for t in range(T):
            n = min(int(counts[t]), cap)
            i, g = self.frame(boxes[t, :n], ages[t])
            ids[t, :n] = i
            gaps[t, :n] = g
        return ids, gaps


def associate_memory(boxes, counts, thr, max_age, tcap=None):
    """the stateless call on one clip -> (ids [T, cap], nids, gaps [T, cap], entries dropped by the tcap cut)"""
    tm = TrackMemory(boxes.shape[1] if tcap is None else tcap, thr)
    ids, gaps = tm.clip(boxes, counts, max_age)
    return ids, tm.next_id, gaps, tm.dropped


def associate_memory_chunked(boxes, counts, thr, max_age, tcap, chunks):
    """the same through one carried state fed in chunks along T"""
    tm = TrackMemory(tcap, thr)
    ids, gaps, t0 = [], [], 0
    for L in chunks:
        i, g = tm.clip(boxes[t0:t0 + L], counts[t0:t0 + L], max_age if np.isscalar(max_age) else max_age[t0:t0 + L])
        ids.append(i); gaps.append(g)
        t0 += L
    assert t0 == boxes.shape[0]
    return np.concatenate(ids), tm.next_id, np.concatenate(gaps), tm.dropped


def moving_boxes(T, cap, n_obj_t, seed):
    """the generator of tests/test_gpu_stream.py, restated: moving boxes with births, deaths, label changes and ties;
    n_obj_t(t) = objects that may be alive in frame t (0: an empty frame); 15 % of detections are dropped per frame"""
    rs = np.random.RandomState(seed)
    n_max = max(n_obj_t(t) for t in range(T))
    pos = rs.rand(n_max, 2); vel = (rs.rand(n_max, 2) - .5) * .06; wh = rs.rand(n_max, 2) * .2 + .05
    lab = rs.randint(0, 3, n_max)
    boxes = np.zeros((T, cap, 8), dtype=np.float32)
    counts = np.zeros(T, dtype=np.int32)
    for t in range(T):
        alive = [k for k in range(n_obj_t(t)) if rs.rand() > 0.15]
        rs.shuffle(alive)
        for i, k in enumerate(alive[:cap]):
            p = pos[k] + vel[k] * t
            boxes[t, i] = [p[0], p[1], wh[k, 0], wh[k, 1], .9, lab[k] if rs.rand() > .05 else (lab[k] + 1) % 3, .8, i]
        counts[t] = min(len(alive), cap)
        if t % 5 == 3 and counts[t] >= 2:
            boxes[t, 1, :4] = boxes[t, 0, :4]      # exact duplicate -> tie on IoU
    return boxes, counts


# the parity cases: name -> (T, cap, objects alive in frame t, tcap, chunkings for the stream tests -- those of
# tests/test_gpu_stream.py:ASSOC_CASES for the shapes taken from there)
CASES = {
    "register_form": (40, 32, lambda t: 12, 64, [[1] * 40, [7, 33]]),
    "register_form_edge": (40, 64, lambda t: 30, 64, [[1] * 40, [7, 33]]),
    "lds_form": (8, 128, lambda t: 140, 256, [[8], [5, 3], [1] * 8]),
    "table_over_64_then_small": (12, 128, lambda t: 120 if t < 6 else 20, 160, [[6, 6], [5, 1, 6]]),
    "table_small_then_over_64": (12, 128, lambda t: 20 if t < 6 else 120, 160, [[6, 6], [6, 1, 5]]),
    "empty_frames": (14, 64, lambda t: 0 if t in (6, 7) else 25, 64, [[7, 7], [6, 1, 1, 6], [8, 6]]),
    "longer_than_64_frames": (70, 32, lambda t: 12, 64, [[40, 30], [64, 6]]),
}
