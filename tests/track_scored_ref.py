"""Plain restatement of the scored two-pass track association (track scores), for the tests.

Everything that is not named here is tests/track_assign_ref.py's and the files it reuses: the prediction, the weights, the
solver (identity_score_ref.assign_max), the velocity update on the stored box, hits, gaps, the rebuild order, the capacity cut
and the read-out.  The step of a frame with n boxes, a table of nt entries and s_i = box i's float `score_at`:

  * CLASSES.  Box i is HIGH when s_i >= score_high as float32, else LOW (a NaN score is LOW).
  * PASS 1.  The assignment's candidates, restricted to HIGH boxes: W1 [n][nt] with every LOW row zero, solved by assign_max
    on the full shape, so that the solver's orientation and tie rules do not depend on how many boxes are HIGH.
  * PASS 2 (skipped when max_age_low == -1).  Candidates: LOW box i, entry j not claimed in pass 1, age_j <= min(max_age,
    max_age_low), labels equal unless ANY_LABEL, IoU against the predicted box >= thr_low.  W2 on the full shape, solved alike.
  * IDS.  A box that claimed an entry in either pass inherits as in the assignment.  An unclaimed box with s_i >= score_new
    opens an id in decode order.  Every other unclaimed box is DROPPED: id -1, gap -1, hits 0.
  * TABLE.  A dropped box still takes its row among the frame's leading rows: id -1, hits 0, age 0, at rest, box and label
    stored.  Such a DEAD row is never a candidate of any entry, is never read out (hits 0) and never survives a rebuild; it
    counts in the capacity cut of the frame that made it.

A chunk of a chunked run may stand for a call of another stream entry (the plain assignment, a match policy, the motion
entry): those skip dead rows too -- TrackMatch.candidates and TrackAssign's rebuild know nothing of them, so both are
restated here with the test `id >= 0`.

Counts per run (`stats`): pass-1 pairs, pass-2 pairs, dropped boxes, and the pairs that would have been candidates had their
entry not been dead.  Everything is a Python list walked one element at a time, with np.float32 around every single
operation.  Test infrastructure only.
"""
import numpy as np

from oracle import oracle as orc

import identity_score_ref as isr
import track_assign_ref as tar
from track_readout_ref import KEYS, _join, with_min_hits      # noqa: F401

f32 = np.float32
MATCH_BEST_FIRST, MATCH_ANY_LABEL = tar.MATCH_BEST_FIRST, tar.MATCH_ANY_LABEL
THR, GAIN = tar.THR, tar.GAIN
# the parameters the scenes are stated at
SCORE_HIGH, SCORE_NEW, THR_LOW, MAX_AGE_LOW, SCORE_AT = 0.5, 0.6, THR, 0, 6
DEAD = -1                # the id of a dead row


class TrackScored(tar.TrackAssign):
    """TrackAssign whose frames take the two passes while `scored` is set (an attribute: it belongs to the call).  With it
    unset a frame is TrackAssign's or TrackMatch's (by `assign`) on a table whose dead rows are skipped."""

    def __init__(self, tcap, thr, gain, match=0, score_at=SCORE_AT, score_high=SCORE_HIGH, score_new=SCORE_NEW, thr_low=THR_LOW,
                 max_age_low=MAX_AGE_LOW):
        tar.TrackAssign.__init__(self, tcap, thr, gain, match, True)
        self.scored = True
        self.score_at, self.score_high, self.score_new = int(score_at), f32(score_high), f32(score_new)
        self.thr_low, self.max_age_low = f32(thr_low), int(max_age_low)
        assert 0 <= self.score_at <= 7 and self.max_age_low >= -1
        self.stats = dict(pass1=0, pass2=0, dropped_boxes=0, dead_candidates=0)

    def ious(self, rows, max_age):
        """{(i, j): IoU as float32 of box i and the predicted box of entry j} over the live entries with age <= max_age whose
        label is the box's (ANY_LABEL: any); TrackMatch.candidates' walk without its threshold.  A dead entry gives no pair; where it
        would have been a candidate at `thr` it is counted."""
        thr32 = f32(self.thr)
        out = {}
        for i, r in enumerate(rows):
            for j, (box, lab, tid, age, vx, vy) in enumerate(self.table):
                if age > max_age:
                    continue
                if not (self.match & MATCH_ANY_LABEL) and f32(lab) != f32(r[5]):
                    continue
                k = f32(age + 1)
                px = f32(f32(box[0]) + f32(k * f32(vx)))
                py = f32(f32(box[1]) + f32(k * f32(vy)))
                iou = f32(orc.bbox_iou(r[:4], np.array([px, py, box[2], box[3]], dtype=np.float32)))
                if tid < 0:
                    self.stats["dead_candidates"] += int(iou >= thr32)
                    continue
                out[(i, j)] = iou
        return out

    def candidates(self, rows, max_age):
        """TrackMatch.candidates on the live entries"""
        thr32 = f32(self.thr)
        return {p: v for p, v in self.ious(rows, max_age).items() if v >= thr32}

    def frame(self, rows, max_age, gain=None):
        if not self.scored:
            # another entry's frame.  Its rebuild would keep a dead row of age + 1 <= max_age; the kernel's survivor test is
            # `id >= 0`, so the dead rows leave here: counted on their own, then put beyond every max_age for this frame.
            table = self.table
            if any(e[2] < 0 for e in table):
                self.table = [e for e in table if e[2] < 0]
                self.ious(rows, max_age)
                self.table = [e if e[2] >= 0 else e[:3] + [1 << 30] + e[4:] for e in table]
            return tar.TrackAssign.frame(self, rows, max_age, gain)
        assert not (self.match & MATCH_BEST_FIRST)
        g = f32(self.gain if gain is None else gain)
        n, nt = len(rows), len(self.table)
        score = [f32(r[self.score_at]) for r in rows]
        high = [bool(s >= self.score_high) for s in score]      # (a NaN compares false: LOW)
        iou = self.ious(rows, max_age)
        thr32 = f32(self.thr)
        pair = {}                # box -> entry

        def solve(cand):
            if not (n and nt):
                return {}
            w = tar.weights(cand, n, nt)
            r2c, _, total = isr.assign_max(w)
            got = {i: int(r2c[i]) for i in range(n) if r2c[i] >= 0}
            assert all(p in cand for p in got.items()) and total == sum(int(w[i, j]) for i, j in got.items())
            return got

        first = solve({p: v for p, v in iou.items() if high[p[0]] and v >= thr32})
        pair.update(first)
        self.stats["pass1"] += len(first)
        if self.max_age_low != -1:
            claimed = set(first.values())
            low_age = min(max_age, self.max_age_low)
            second = solve({p: v for p, v in iou.items()
                            if not high[p[0]] and p[1] not in claimed and self.table[p[1]][3] <= low_age and v >= self.thr_low})
            assert not (set(second) & set(first)) and not (set(second.values()) & claimed)
            pair.update(second)
            self.stats["pass2"] += len(second)
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
            elif score[i] >= self.score_new:
                ids.append(self.next_id); gaps.append(-1); vels.append((f32(0), f32(0)))
                self.next_id += 1
            else:
                ids.append(DEAD); gaps.append(-1); vels.append((f32(0), f32(0)))
                self.stats["dropped_boxes"] += 1
        claimed = set(pair.values())
        new = [[np.array(r[:4], dtype=np.float32), f32(r[5]), i, 0, v[0], v[1]] for r, i, v in zip(rows, ids, vels)]
        for j, (box, lab, tid, age, vx, vy) in enumerate(self.table):
            if j not in claimed and tid >= 0 and age + 1 <= max_age:
                new.append([box, lab, tid, age + 1, vx, vy])
        self.dropped += max(0, len(new) - self.tcap)
        self.table = new[:self.tcap]
        return ids, gaps


class TrackScoredReadout(tar.TrackReadout):
    """TrackReadout over a TrackScored table: a dropped box and its dead row have hits 0"""

    def __init__(self, tcap, thr, gain, min_hits, match=0, **score):
        tar.TrackReadout.__init__(self, tcap, thr, gain, min_hits)
        self.tm = TrackScored(tcap, thr, gain, match, **score)

    def frame(self, rows, max_age, gain=None):
        """TrackReadout.frame with the dropped boxes' hits"""
        ids, gaps = self.tm.frame(rows, max_age, gain)
        bh = []
        for i, g in zip(ids, gaps):
            h = 0 if i < 0 else 1 if g < 0 else self.hits[i] + 1
            self.hits[i] = h
            bh.append(h)
        self.hits = {e[2]: self.hits[e[2]] for e in self.tm.table}
        out = []
        for j, (box, lab, tid, age, vx, vy) in enumerate(self.tm.table):
            if age == 0:
                x, y = f32(box[0]), f32(box[1])
            else:
                a = f32(age)
                x = f32(f32(box[0]) + f32(a * f32(vx)))
                y = f32(f32(box[1]) + f32(a * f32(vy)))
            out.append(([x, y, f32(box[2]), f32(box[3]), f32(lab), f32(vx), f32(vy), f32(0)],
                        [tid, age, self.hits[tid], j if age == 0 else -1]))
        return ids, gaps, bh, out


def _finish(r, tr):
    r["log"] = list(tr.tm.log)
    r["stats"] = dict(tr.tm.stats)
    return r


def associate_tracks_scored(boxes, counts, thr, max_age, gain, min_hits, match, tcap=None, **score):
    """the stateless call on one clip -> dict of KEYS (arrays without the clip axis, nids an int), `dropped` (entries the capacity
    cut took) and `stats`.  score: score_at, score_high, score_new, thr_low, max_age_low (the scenes' values where left out)"""
    assert match in (0, MATCH_ANY_LABEL)
    tr = TrackScoredReadout(boxes.shape[1] if tcap is None else tcap, thr, gain, min_hits, match, **score)
    return _finish(_join([tr.clip(boxes, counts, max_age)], tr), tr)


def associate_tracks_scored_chunked(boxes, counts, thr, max_age, gain, min_hits, match, tcap, chunks, assign_at=(), match_at=None,
                                    motion_at=(), **score):
    """the same through one carried state fed in chunks along T.  A chunk whose index is in assign_at stands for a call of
    dt_associate_stream_tracks_assign with `match`; a key of match_at for dt_associate_stream_tracks_match with that match; one in
    motion_at for dt_associate_stream_motion (decode order within a label, the hits forgotten afterwards, no hits and no read-out
    from it: -1 / 0 in the result); every other chunk is the scored entry with `match`."""
    assert match in (0, MATCH_ANY_LABEL)
    match_at = dict(match_at or {})
    tr = TrackScoredReadout(tcap, thr, gain, min_hits, match, **score)
    parts, t0 = [], 0
    for c, L in enumerate(chunks):
        if c in motion_at:
            tr.tm.scored, tr.tm.assign, tr.tm.match = False, False, 0
        elif c in match_at:
            tr.tm.scored, tr.tm.assign, tr.tm.match = False, False, int(match_at[c])
        elif c in assign_at:
            tr.tm.scored, tr.tm.assign, tr.tm.match = False, True, int(match)
        else:
            tr.tm.scored, tr.tm.assign, tr.tm.match = True, True, int(match)
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
SCENES = tar.SCENES
SCORE_SEEDS = (11, 12, 13)
_BOXES, _REFS = {}, {}


def with_scores(boxes, counts, obj, span, seed):
    """the scene's boxes with scores, and clutter: frames in order, boxes in order; a box of object k in frame t is weak when
    (t + 3k) % 7 is 3 or 4 and draws its score from [.15, .45), any other from [.55, .95) (float 6; float 4 = min(1, score + .05));
    then per frame three clutter boxes (centre in `span`, w = h = .2, a random label, score in [.12, .3)) while count < cap"""
    rs = np.random.RandomState(seed)
    boxes, counts = boxes.copy(), counts.copy()
    T, cap = boxes.shape[:2]
    for t in range(T):
        for i in range(int(counts[t])):
            weak = (t + 3 * int(obj[t, i])) % 7 in (3, 4)
            s = rs.uniform(.15, .45) if weak else rs.uniform(.55, .95)
            boxes[t, i, 6] = s
            boxes[t, i, 4] = min(1.0, s + .05)
        for _ in range(3):
            if counts[t] < cap:
                c = 0.5 + (rs.rand(2) - .5) * span
                lab = rs.randint(2)
                s = rs.uniform(.12, .3)
                i = int(counts[t])
                boxes[t, i] = [c[0], c[1], .2, .2, min(1.0, s + .05), lab, s, i]
                counts[t] += 1
    return boxes, counts


def scene(name, seed=SCORE_SEEDS[0]):
    """-> (boxes, counts) of the scene with the scores of `seed`, computed once"""
    key = (name, seed)
    if key not in _BOXES:
        T, cap, nobj, _, _, span, _, _ = SCENES[name]
        _BOXES[key] = with_scores(*tar.crowd_boxes_gt(T, cap, nobj, tar.SEED, span), span=span, seed=seed)
    return _BOXES[key]


def ref(key, boxes, counts, max_age, min_hits, match, tcap, **score):
    """the stateless restatement at THR and GAIN, computed once per key and shared: callers must leave it unchanged"""
    key = (key, int(max_age), int(match), int(tcap), tuple(sorted(score.items())))
    if key not in _REFS:
        _REFS[key] = associate_tracks_scored(boxes, counts, THR, max_age, GAIN, 1, match, tcap, **score)
    return with_min_hits(_REFS[key], min_hits)


def scene_ref(name, match, min_hits=1, seed=SCORE_SEEDS[0], **score):
    b, c = scene(name, seed)
    s = SCENES[name]
    return ref((name, seed), b, c, s[4], min_hits, match, s[3], **score)


def swap_floats(boxes, a, b):
    out = boxes.copy()
    out[..., a], out[..., b] = boxes[..., b], boxes[..., a]
    return out


def compact_high(boxes, counts, score_high, score_at=SCORE_AT):
    """the frames with the LOW boxes removed and the rest moved up -> (boxes, counts, index [T, cap]: where box i of the input went,
    -1 for a LOW or unused one)"""
    T, cap = boxes.shape[:2]
    out = np.zeros_like(boxes); cnt = np.zeros_like(counts); index = np.full((T, cap), -1, dtype=np.int32)
    for t in range(T):
        k = 0
        for i in range(min(int(counts[t]), cap)):
            if f32(boxes[t, i, score_at]) >= f32(score_high):
                out[t, k] = boxes[t, i]
                index[t, i] = k
                k += 1
        cnt[t] = k
    return out, cnt, index


def worked_example():
    """the issue's smallest case: a track's box turns weak for one frame beside a weak clutter box -> (boxes [3, 2, 8], counts [3])"""
    boxes = np.zeros((3, 2, 8), dtype=np.float32)
    rows = (((.40, .9),), ((.80, .2), (.42, .3)), ((.44, .9),))
    for t, fr in enumerate(rows):
        for i, (x, s) in enumerate(fr):
            boxes[t, i] = [x, .5, .2, .2, min(1.0, s + .05), 0, s, i]
    return boxes, np.array([1, 2, 1], dtype=np.int32)
