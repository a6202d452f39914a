"""Plain restatement of "a tiny-tracker stream carries its LSTM state", for the tests.

A slot holds (h, c), both [U] float32; a slot that is not in the table is fresh (h = c = 0).  A call names one slot per
sequence and feeds T frames: per frame pool (+) det -> orc.lstm_step from the slots' rows -> orc.dense_sigmoid, and after
frame T - 1 the rows go back to the slots.  The steps are the oracle's own, one frame at a time, so a stream fed in chunks
is by construction the oracle's recurrence with the loop cut in pieces.  Test infrastructure only.
"""
import numpy as np

from oracle import oracle as orc


class TinyStreams(object):
    def __init__(self, weights, pool="Global"):
        self.w, self.pool = weights, pool
        self.U = weights["recurrent"].shape[0]
        self.state = {}          # slot -> (h [U], c [U])

    def reset(self, slots=None):
        if slots is None:
            self.state.clear()
        for s in slots or ():
            self.state.pop(int(s), None)

    def forward(self, feat, det, slots):
        """feat [n,T,fh,fw,fc], det [n,T,4 | hs*hs], slots: n distinct numbers -> [n,T,O]"""
        n, T = feat.shape[:2]
        slots = [int(s) for s in slots]
        assert len(slots) == n and len(set(slots)) == n
        zero = np.zeros(self.U, dtype=np.float32)
        h = np.stack([self.state.get(s, (zero, zero))[0] for s in slots])
        c = np.stack([self.state.get(s, (zero, zero))[1] for s in slots])
        out = np.zeros((n, T, self.w["dense_kernel"].shape[1]), dtype=np.float32)
        for t in range(T):
            f = feat[:, t]
            v = orc.global_maxpool(f) if self.pool == "Global" else orc.maxpool4_flatten(f)
            x = np.concatenate([v, np.ascontiguousarray(det[:, t], dtype=np.float32)], axis=1)
            h, c = orc.lstm_step(x, h, c, self.w["kernel"], self.w["recurrent"], self.w["bias"])
            out[:, t] = orc.dense_sigmoid(h, self.w["dense_kernel"], self.w["dense_bias"])
        for i, s in enumerate(slots):
            self.state[s] = (h[i].copy(), c[i].copy())
        return out


def run_chunks(streams, feat, det, chunks, slots):
    """feed feat / det [n, sum(chunks), ...] chunk by chunk; the outputs concatenated along T"""
    outs, t0 = [], 0
    for k in chunks:
        outs.append(streams.forward(feat[:, t0:t0 + k], det[:, t0:t0 + k], slots))
        t0 += k
    assert t0 == feat.shape[1]
    return np.concatenate(outs, axis=1)
