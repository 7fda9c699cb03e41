"""The per-update stream audit (tests/stream_audit.py) without a GPU: each check accepts what is right and rejects the fault it
is there to find, so that it cannot pass by construction (for example by comparing the truth with itself)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle.edges_py import EdgesPy
from tests import stream_audit as A

PAD = (12, 16)      # ops.FMAP_PADY, ops.FMAP_PADX


def _corr_case(seed=3, E=40, level1_scale=1.0):
    rng = np.random.default_rng(seed)
    mem, C, h, w, Ng = 3, 24, 24, 32, 10
    f1 = (rng.standard_normal((mem, C, h, w)) / 4).astype(np.float16)
    f2 = (rng.standard_normal((mem, C, h // 4, w // 4)) / 4 * level1_scale).astype(np.float16)
    gmap = (rng.standard_normal((Ng, C, 3, 3)) / 4).astype(np.float16)
    off = np.arange(3.0) - 1
    cx, cy = rng.uniform(2, w - 2, E), rng.uniform(2, h - 2, E)
    coords = np.empty((E, 2, 3, 3), np.float32)
    coords[:, 0] = cx[:, None, None] + off[None, None, :]
    coords[:, 1] = cy[:, None, None] + off[None, :, None]
    kk, jj = rng.integers(0, Ng, E), rng.integers(0, mem, E)
    return O.slam_corr(gmap, f1, f2, coords, kk, jj, 3, "truth")


def test_the_correlation_check_accepts_the_truth_and_rejects_a_moved_level1_element():
    truth = _corr_case()
    got = truth.astype(np.float16)                 # what a correct kernel stores: the truth rounded to half
    errs = A.check_corr(got, truth)
    assert 0 < errs["all"][0] <= 1.0
    tol = A.corr_tol(truth)
    bad = got.copy()
    bad[17, 2 * 100 + 1] = np.float16(truth[17, 2 * 100 + 1] + 3 * tol)      # one level-1 element (odd channel)
    with pytest.raises(AssertionError):
        A.check_corr(bad, truth)
    # level 1 much smaller than level 0: an error inside the overall bound but three times level 1's own bound is still caught
    truth = _corr_case(level1_scale=1.0 / 64)
    got = truth.astype(np.float16)
    A.check_corr(got, truth)
    t1 = A.corr_tol(truth[:, 1::2])
    assert 3 * t1 < A.corr_tol(truth)
    bad = got.astype(np.float64)
    bad[5, 2 * 220 + 1] = truth[5, 2 * 220 + 1] + 3 * t1
    assert np.abs(bad - truth).max() <= A.corr_tol(truth)               # the overall maximum alone would let it through
    with pytest.raises(AssertionError, match="level1"):
        A.check_corr(bad, truth)
    # a systematically biased result passes the max bound but not the mean
    biased = truth + 0.5 * A.corr_tol(truth)
    with pytest.raises(AssertionError, match="mean"):
        A.check_corr(biased, truth)


def _rings(seed=4, mem=5, pmem=5, M=3, C=8, h=16, w=24):
    rng = np.random.default_rng(seed)
    o1 = (rng.standard_normal((mem, C, h, w)) / 4).astype(np.float16)
    o2 = (rng.standard_normal((mem, C, h // 4, w // 4)) / 4).astype(np.float16)
    og = (rng.standard_normal((pmem * M, C, 3, 3)) / 4).astype(np.float16)
    py, px = PAD
    r1 = torch.zeros((mem, h + 2 * py, w + 2 * px, C), dtype=torch.float16)
    r2 = torch.zeros((mem, h // 4 + 2 * py, w // 4 + 2 * px, C), dtype=torch.float16)
    r1[:, py:-py, px:-px] = torch.as_tensor(o1).permute(0, 2, 3, 1)
    r2[:, py:-py, px:-px] = torch.as_tensor(o2).permute(0, 2, 3, 1)
    g = torch.as_tensor(og).clone()
    pm = g.reshape(-1, C, 9).transpose(1, 2).contiguous()
    return r1, r2, g, pm, o1, o2, og, M


def test_the_ring_check_rejects_swapped_slots():
    r1, r2, g, pm, o1, o2, og, M = _rings()
    n = 12            # five-slot rings, twelve keyframes: four live slots each
    assert A.compare_rings(r1, r2, g, pm, o1, o2, og, n, M, PAD) == {"fmap2_ulps": 0, "gmap_ulps": 0}
    # one ulp in fmap2 is allowed, two are not
    b2 = r2.clone()
    b2.view(torch.int16)[1, PAD[0] + 1, PAD[1] + 2, 3] += 1
    assert A.compare_rings(r1, b2, g, pm, o1, o2, og, n, M, PAD)["fmap2_ulps"] == 1
    b2.view(torch.int16)[1, PAD[0] + 1, PAD[1] + 2, 3] += 1
    with pytest.raises(AssertionError, match="fmap2"):
        A.compare_rings(r1, b2, g, pm, o1, o2, og, n, M, PAD)
    live = [f % 5 for f in A.live_frames(n, 5)]
    s, t = live[0], live[2]
    for which in ("fmap1", "fmap2"):
        b1, b2 = r1.clone(), r2.clone()
        b = b1 if which == "fmap1" else b2
        b[[s, t]] = b[[t, s]]
        with pytest.raises(AssertionError, match=which):
            A.compare_rings(b1, b2, g, pm, o1, o2, og, n, M, PAD)
    # two frames' tiles swapped in both tile arrays (consistent with each other, not with the oracle)
    bg, bpm = g.clone(), pm.clone()
    for x in (bg, bpm):
        a, c = x[s * M:(s + 1) * M].clone(), x[t * M:(t + 1) * M].clone()
        x[s * M:(s + 1) * M], x[t * M:(t + 1) * M] = c, a
    with pytest.raises(AssertionError, match="gmap"):
        A.compare_rings(r1, r2, bg, bpm, o1, o2, og, n, M, PAD)
    # ... or in the pixel-major copy only: caught without an oracle too
    with pytest.raises(AssertionError, match="gmap_pm"):
        A.compare_rings(r1, r2, g, bpm, None, None, None, n, M, PAD)
    # a margin element that is not zero
    b1 = r1.clone()
    b1[2, PAD[0] - 1, PAD[1] + 3, 0] = 1.0
    with pytest.raises(AssertionError, match="margin"):
        A.compare_rings(b1, r2, g, pm, o1, o2, og, n, M, PAD)
    # the slot the next frame overwrites is not live: a difference there is not a finding
    b1 = r1.clone()
    b1[n % 5] = 0
    A.compare_rings(b1, r2, g, pm, o1, o2, og, n, M, PAD)


def test_f16_ulps_counts_across_zero_and_subnormals():
    a = torch.tensor([0.0, -0.0, 6e-8, 1.0, -1.0], dtype=torch.float16)
    b = torch.tensor([-0.0, 6e-8, -6e-8, 1.0009765625, -1.0], dtype=torch.float16)
    assert A.f16_ulps(a, b).tolist() == [0, 1, 2, 1, 0]


@pytest.mark.parametrize("dropped", [False, True])
def test_the_pruned_rows_follow_the_oracle_keyframe(dropped):
    """pruned_rows (the audit's model of keyframe()) against oracle/edges_py.py on a stream of frames"""
    M, r, rw, ki = 4, 5, 6, 4
    ix = np.repeat(np.arange(64), M)
    e = EdgesPy()
    n = 0
    for f in range(20):
        n += 1
        e.append_factors(*e.edges_forw(n, M, r), ix)
        e.append_factors(*e.edges_back(n, M, r), ix)
        if n < 8:
            continue
        e.target = np.arange(2 * len(e.ii), dtype=np.float32).reshape(-1, 2)
        ii, jj, kk, tg = e.ii.copy(), e.jj.copy(), e.kk.copy(), e.target.copy()
        n_inac = len(e.ii_inac)
        drop = dropped and f % 3 == 2
        old, kept, ii2, jj2, kk2 = A.pruned_rows(ii, jj, kk, n, M, ki, rw, drop)
        n = e.keyframe(n - ki, n, M, ix, rw, drop=drop)
        assert np.array_equal(ii2[kept], e.ii) and np.array_equal(jj2[kept], e.jj) and np.array_equal(kk2[kept], e.kk)
        assert np.array_equal(tg[kept], e.target)
        assert np.array_equal(ii2[old], e.ii_inac[n_inac:]) and np.array_equal(kk2[old], e.kk_inac[n_inac:])
        assert np.array_equal(jj2[old], e.jj_inac[n_inac:]) and np.array_equal(tg[old], e.target_inac[n_inac:])
    assert len(e.ii_inac) > 0


def test_the_stub_recompute_is_the_oracle_runners_stub():
    """stub_recompute is StreamOracle._update's operator stub, and the ulp measure sees a one-ulp change"""
    rng = np.random.default_rng(8)
    E = 500
    coords = rng.uniform(0, 120, (E, 2, 3, 3)).astype(np.float32)
    corr = rng.standard_normal((E, 882)).astype(np.float16).astype(np.float32)
    t, w = A.stub_recompute(coords, corr[:, :4], 0.25)
    assert np.array_equal(t, (coords[:, :, 1, 1] + np.float32(0.25) * np.tanh(corr[:, :2])).astype(np.float32))
    assert np.array_equal(w, (1.0 / (1.0 + np.exp(-corr[:, 2:4]))).astype(np.float32))
    assert A.ulps32(t, t) == 0.0
    assert A.ulps32(np.nextafter(t, np.float32(np.inf)), t) == pytest.approx(1.0)
