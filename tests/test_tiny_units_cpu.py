"""The tiny-tracker unit tests' own test, without a GPU: the tolerance tests/test_gpu_tiny_units.py computes rejects every named defect
of tests/tiny_units_ref.py, the head-level tolerance of the older tests accepts one of them, the float32 restatement agrees with the
oracle's step, every case's inputs meet their conditions, and the heatmap restatements equal the reference functions' recorded results.

Measured here (float64 numpy reference; float32 numpy; tol = 8 gap + 4 floor; case by case in tests/test_gpu_tiny_units.py):
  gap max|H32 - H64| 1.05e-7 (13 x 1) .. 2.04e-7 (64 x 3), round-trip floor 2.84e-7 .. 3.48e-7, tol 2.04e-6 .. 2.96e-6; the oracle's
  float32 step is within 4.9e-7 of H64 on 13 x 3.
  Smallest defect: unit 511's output gate without lane 63's k-slice moves h by 9.0e-4 (n = 8) .. 3.5e-3 (n = 63), 360 to 1300 times
  the tolerance of its case; every unit's cell gate without that slice by 0.03; the other three by 0.002 (f and o swapped for unit 0
  at n = 1) to 0.23.
  Through synth_tiny_weights(512)'s Dense(4, sigmoid) head (n = 13, T = 6, pooled randn features, D = 516): the smallest defect moves h by
  1.38e-3 (unit-level tolerance there: 8.7e-6) and the head's output by 2.7e-5, inside rtol = 1e-4, atol = 2e-5 of the head-level tests
  (outputs near 0.5: 7e-5).
"""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from utility import synth

import tiny_units_ref as tur

U = tur.U
MUTATION_CASES = [(name, n, T) for name, (_, applies) in tur.MUTATIONS.items() for (n, T) in tur.LSTM_CASES if T == 3 and applies(n)]


def test_every_mutation_has_its_case():
    names = {m for m, _, _ in MUTATION_CASES}
    assert names == set(tur.MUTATIONS) and len(names) == 5
    assert ("ragged_tail_takes_its_neighbour", 13, 3) in MUTATION_CASES and ("tracks_8_9_swap_high_units", 13, 3) in MUTATION_CASES
    assert set(tur.LSTM_NS) == {1, 7, 8, 9, 13, 63, 64, 65, 72, 129} and {(13, 1), (13, 2), (13, 3)} <= set(tur.LSTM_CASES)


@pytest.mark.parametrize("n,T", tur.LSTM_CASES)
def test_case_conditions(n, T):
    """gates mostly unsaturated, tracks far apart, a tolerance from the references alone -- and the identity read-out of the float32
    restatement passes the tolerance it is going to be held to"""
    case = tur.lstm_case(n, T)
    print("n=%d T=%d scale %.1f: inside %.3f, gap %.3g, floor %.3g, tol %.3g, min track distance %.3g"
          % (n, T, case.scale, tur.inside_fraction(case.Z), case.gap, case.floor, case.tol, tur.min_track_distance(case.H64) if n > 1 else np.nan))
    tur.check_conditions(case)
    assert case.x.shape == (n, T, tur.D_ROWS) and case.x.dtype == np.float32
    s = np.float32(1) / (np.float32(1) + np.exp(-case.H32))      # what the identity head would return for the float32 run
    tur.assert_all_close(tur.logit64(s), case, "float32 restatement through the identity head")


@pytest.mark.parametrize("name,n,T", MUTATION_CASES)
def test_mutation_is_rejected(name, n, T):
    case = tur.lstm_case(n, T)
    Hm = tur.mutated(case, name)
    moved = float(np.abs(Hm - case.H64).max())
    print("%s n=%d: moves h by %.3g, %.1f x tol %.3g" % (name, n, moved, moved / case.tol, case.tol))
    assert moved > 2.0 * case.tol, "%s at n=%d moves h by %.3g only: the tolerance %.3g would let it pass" % (name, n, moved, case.tol)
    with pytest.raises(AssertionError):
        tur.assert_all_close(Hm, case, name)
    # ... with the read-out's own error on top
    s = (1.0 / (1.0 + np.exp(-Hm))).astype(np.float32)
    with pytest.raises(AssertionError):
        tur.assert_all_close(tur.logit64(s), case, name + " through the identity head")


def test_old_head_tolerance_accepts_the_smallest_mutation():
    """the gap this suite closes: Dense(4, sigmoid) at rtol = 1e-4, atol = 2e-5 does not see unit 511's output gate lose eight of its
    512 terms"""
    tw = synth.synth_tiny_weights(512)
    n, T = 13, 6
    rs = np.random.RandomState(11)
    feat = rs.randn(n, T, 4, 4, 512).astype(np.float32)
    det = rs.rand(n, T, 4).astype(np.float32)
    x = np.concatenate([tur.global_maxpool(feat.reshape(n * T, 4, 4, 512)).reshape(n, T, 512), det], axis=2)
    H = tur.lstm_sequence(x, tw["kernel"], tw["recurrent"], tw["bias"])
    Hm = tur.lstm_sequence(x, tw["kernel"], tw["recurrent"], tw["bias"], mutate=tur.MUTATIONS["unit511_o_loses_lane63"][0])
    out = tur.dense_sigmoid64(H, tw["dense_kernel"], tw["dense_bias"])
    outm = tur.dense_sigmoid64(Hm, tw["dense_kernel"], tw["dense_bias"])
    dh, dout = float(np.abs(Hm - H).max()), float(np.abs(outm - out).max())
    H32 = tur.lstm_sequence(x, tw["kernel"], tw["recurrent"], tw["bias"], np.float32)
    tol = 8.0 * float(np.abs(H32 - H).max()) + 4.0 * tur.roundtrip_floor(H)
    msg = "h moves by %.3g (unit-level tolerance %.3g), the head's output by %.3g (head-level rtol 1e-4, atol 2e-5)" % (dh, tol, dout)
    print(msg)
    assert np.all(np.abs(outm - out) <= 2e-5 + 1e-4 * np.abs(out)), "the head-level tolerance sees it after all: " + msg
    assert dh > 8.0 * tol, "the unit-level tolerance would not see it: " + msg


def test_float32_restatement_matches_the_oracle_step():
    """ties the numpy restatement to the existing reference: orc.lstm_step, step by step, on one case"""
    case, tw = tur.lstm_case(13, 3), tur.weights()
    h = np.zeros((13, U), dtype=np.float32)
    c = np.zeros_like(h)
    for t in range(3):
        h, c = orc.lstm_step(case.x[:, t], h, c, tw["kernel"], tw["recurrent"], tw["bias"])
        err = float(np.abs(h.astype(np.float64) - case.H64[:, t]).max())
        print("step %d: oracle vs H64 %.3g, vs H32 %.3g, tol %.3g" % (t, err, float(np.abs(h - case.H32[:, t]).max()), case.tol))
        assert err <= case.tol
        assert float(np.abs(h - case.H32[:, t]).max()) <= case.tol


def test_head_tolerance_is_small_and_pools_restate_the_oracle():
    case = tur.lstm_case(3, 3)
    for O in (1, 3, 8, 9, 257):
        Wd, bd = tur.head_weights(O)
        tol, gap = tur.head_tolerance(case, Wd, bd, orc.dense_sigmoid)
        print("O=%d: float32 head vs float64 %.3g, tolerance %.3g .. %.3g" % (O, gap, tol.min(), tol.max()))
        assert tol.shape == (O,) and 0 < tol.max() < 1e-4
    rs = np.random.RandomState(3)
    f = rs.randn(2, 13, 13, 8).astype(np.float32)
    assert np.array_equal(tur.global_maxpool(f), orc.global_maxpool(f))
    assert np.array_equal(tur.maxpool4_flatten(f), orc.maxpool4_flatten(f))
    for fh, fw, C, _ in tur.GLOBAL_CASES:
        neg, peak = tur.global_inputs(3, fh, fw, C, 1)
        assert neg.max() < 0
        assert np.array_equal(peak.reshape(3, fh * fw, C).argmax(axis=1), np.tile(np.arange(C) % (fh * fw), (3, 1)))
    for H, W, C, _ in tur.MAX_CASES:
        f = tur.max_inputs(2, H, W, C, 2)
        assert tur.maxpool4_flatten(f).max() < 50.0 and (f.max() > 50.0) == bool(H % 4 or W % 4)


def test_heatmap_restatements_equal_the_recorded_reference(golden_dir):
    """tests/golden/tiny_units_heatmap.npz holds what the reference's generate_heatmap_feat / generate_rectangle_from_heatmap gave on
    these boxes and maps"""
    d = np.load(os.path.join(golden_dir, "tiny_units_heatmap.npz"))
    boxes = tur.heat_boxes()
    c4, corners = tur.centre_boxes()
    assert np.array_equal(d["boxes"], boxes) and np.array_equal(d["centre4"], c4)
    for hs in tur.HEAT_SIZES:
        mine = np.stack([tur.heatmap_feat(*b, hs=hs) for b in boxes])
        assert np.array_equal(mine, d["heat_%d" % hs].astype(np.float32)), hs
        mine_c = np.stack([tur.heatmap_feat(*b, hs=hs) for b in corners])
        assert np.array_equal(mine_c, d["heat_c_%d" % hs].astype(np.float32)), hs
        assert np.array_equal(orc.heatmap_from_boxes(c4, hs), mine_c), hs
        if hs > 1:      # the cases are what they claim: some empty, some full, some in between
            sums = mine.sum(axis=1)
            assert sums.min() == 0 and sums.max() == hs * hs and len(set(sums.tolist())) >= 6
    for hs in tur.RECT_SIZES:
        maps = tur.rect_maps(hs)
        assert np.array_equal(d["maps_%d" % hs], maps)
        mine = np.array([tur.rect_of_heatmap(m, tur.THRESH, hs) for m in maps], dtype=np.int32)
        assert np.array_equal(mine, d["rects_%d" % hs]), hs
        assert np.array_equal(orc.rect_from_heatmap(maps, hs, tur.THRESH), mine), hs
        assert mine[0].tolist() == [hs, hs, -1, -1] and mine[4].tolist() == [hs, hs, -1, -1]
        assert mine[1].tolist() == [hs - 1] * 4 and mine[2].tolist() == [0] * 4 and mine[3, 0] == mine[3, 2] >= 0
