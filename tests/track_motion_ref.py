"""Plain restatement of the track-motion identity rule (motion gain), for the tests.

The rule is the track-memory rule of tests/track_memory_ref.py with one change and one addition.  A table entry is
(box x y w h, label, id, age, velocity vx vy); the velocity is that of the box's x, y per frame.

  * PREDICTION.  For an entry of age a, k = float32(a + 1), px = x + k*vx, py = y + k*vy (a multiply, then an add, each
    rounded to float32).  Box i is matched against the entry's predicted box (px, py, w, h); the rest of the match is the
    memory rule's: unclaimed entries with age <= max_age and the same label, the largest IoU >= thr, ties to the lowest
    table index, otherwise a new id; gap = the claimed entry's age, -1 for a new id.
  * UPDATE.  When box i claims entry j: ox = (x_i - x_j) / k on the entry's STORED x_j (not the prediction), oy likewise;
    vx_i = vx_j + gain*(ox - vx_j) (subtract, multiply, add), vy_i likewise.  A box that opens a new id gets v = (0, 0).
  * REBUILD.  The frame's boxes first (age 0, the velocity just computed), then the unclaimed entries with
    age + 1 <= max_age in their previous order, box and velocity unchanged; cut at tcap.

Everything is a Python list walked one element at a time, with np.float32 around every single operation; the IoU is
orc.bbox_iou, so its float32 bits are the oracle's.  Test infrastructure only.
"""
import numpy as np

from oracle import oracle as orc

from track_memory_ref import CASES, moving_boxes      # noqa: F401  (the cases and the generator are shared)

f32 = np.float32


class TrackMotion(object):
    """the state a stream carries: the table with its velocities and the next free id (interface of track_memory_ref.TrackMemory)"""

    def __init__(self, tcap, thr, gain):
        self.tcap, self.thr, self.gain = int(tcap), float(thr), float(gain)
        self.table = []          # entries [box4, label, id, age, vx, vy]
        self.next_id = 0
        self.dropped = 0         # entries the tcap cut has removed so far

    def forget_velocities(self):
        """what a call of dt_associate_stream / dt_associate_stream_mem does to the slot's tracks: every track at rest"""
        for e in self.table:
            e[4], e[5] = f32(0), f32(0)

    def frame(self, rows, max_age, gain=None):
        """rows: the frame's boxes [n, 8] in decode order -> (ids, gaps), lists of n"""
        thr32 = f32(self.thr)
        g = f32(self.gain if gain is None else gain)
        claimed = [False] * len(self.table)
        ids, gaps, vels = [], [], []
        for r in rows:
            best, bj = None, -1
            for j, (box, lab, _, age, vx, vy) in enumerate(self.table):
                if claimed[j] or age > max_age or f32(lab) != f32(r[5]):
                    continue
                k = f32(age + 1)
                px = f32(f32(box[0]) + f32(k * f32(vx)))
                py = f32(f32(box[1]) + f32(k * f32(vy)))
                pred = np.array([px, py, box[2], box[3]], dtype=np.float32)
                iou = f32(orc.bbox_iou(r[:4], pred))
                if iou >= thr32 and (best is None or iou > best):      # strictly better: ties stay with the lowest j
                    best, bj = iou, j
            if bj >= 0:
                claimed[bj] = True
                box, _, tid, age, vx, vy = self.table[bj]
                k = f32(age + 1)
                ox = f32(f32(f32(r[0]) - f32(box[0])) / k)
                oy = f32(f32(f32(r[1]) - f32(box[1])) / k)
                nvx = f32(f32(vx) + f32(g * f32(ox - f32(vx))))
                nvy = f32(f32(vy) + f32(g * f32(oy - f32(vy))))
                ids.append(tid); gaps.append(age); vels.append((nvx, nvy))
            else:
                ids.append(self.next_id); gaps.append(-1); vels.append((f32(0), f32(0)))
                self.next_id += 1
        new = [[np.array(r[:4], dtype=np.float32), f32(r[5]), i, 0, v[0], v[1]] for r, i, v in zip(rows, ids, vels)]
        for j, (box, lab, tid, age, vx, vy) in enumerate(self.table):
            if not claimed[j] and age + 1 <= max_age:
                new.append([box, lab, tid, age + 1, vx, vy])
        self.dropped += max(0, len(new) - self.tcap)
        self.table = new[:self.tcap]
        return ids, gaps

    def clip(self, boxes, counts, max_age, gain=None):
        """boxes [T, cap, 8], counts [T]; max_age an int or one per frame -> ids [T, cap], gaps [T, cap] (-1 in unused entries)"""
        T, cap, _ = boxes.shape
        ages = [int(max_age)] * T if np.isscalar(max_age) else [int(a) for a in max_age]
        assert len(ages) == T
        ids = np.full((T, cap), -1, dtype=np.int32)
        gaps = np.full((T, cap), -1, dtype=np.int32)
        for t in range(T):
            n = min(int(counts[t]), cap)
            i, g = self.frame(boxes[t, :n], ages[t], gain)
            ids[t, :n] = i
            gaps[t, :n] = g
        return ids, gaps


def associate_motion(boxes, counts, thr, max_age, gain, tcap=None):
    """the stateless call on one clip -> (ids [T, cap], nids, gaps [T, cap], entries dropped by the tcap cut)"""
    tm = TrackMotion(boxes.shape[1] if tcap is None else tcap, thr, gain)
    ids, gaps = tm.clip(boxes, counts, max_age)
    return ids, tm.next_id, gaps, tm.dropped


def associate_motion_chunked(boxes, counts, thr, max_age, gain, tcap, chunks, plain_at=()):
    """the same through one carried state fed in chunks along T.  Chunks whose index is in plain_at stand for a call of
    dt_associate_stream_mem (or, with max_age an array holding 0 there, dt_associate_stream): the tracks forget their
    velocities and the chunk runs with gain 0, which is the memory rule."""
    tm = TrackMotion(tcap, thr, gain)
    ids, gaps, t0 = [], [], 0
    for c, L in enumerate(chunks):
        a = max_age if np.isscalar(max_age) else max_age[t0:t0 + L]
        if c in plain_at:
            tm.forget_velocities()
            i, g = tm.clip(boxes[t0:t0 + L], counts[t0:t0 + L], a, gain=0.0)
        else:
            i, g = tm.clip(boxes[t0:t0 + L], counts[t0:t0 + L], a)
        ids.append(i); gaps.append(g)
        t0 += L
    assert t0 == boxes.shape[0]
    return np.concatenate(ids), tm.next_id, np.concatenate(gaps), tm.dropped
