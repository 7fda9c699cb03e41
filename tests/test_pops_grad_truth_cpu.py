"""The truth of the projective_ops backward (tests/pops_grad_truth.py) checks itself, and the inputs of the GPU tests are what
they are meant to be.

The closed-form VJP (composed from lie_grad_truth.vjp: act4, mul, inv, plus the two pinhole maps) against central differences
of the same module's forward (h = 2^-16, poses moved as Exp(eps) X, lie_truth's long double where the platform has it).
Required: finer than 1e-7 max(1, |want|), as for the Lie ops -- a truth coarser than float32's u could not judge a float32
kernel.  The worst deviation is printed."""
import numpy as np
import pytest

import pops_grad_truth as PT

TOL = 1e-7


@pytest.mark.parametrize("P", [3, 1])
def test_closed_form_against_differences(P):
    """13 edges over 4 frames and 5 patches, with edges on both sides of the clamp, a self edge and a repeated patch"""
    case = PT.make_case(13, 4, P=P, m=5, seed=3, structure=P == 3)
    gap, above, below, behind = PT.clamp_report(case)
    assert above > 0 and below > 0 and behind > 0 and gap >= PT.CLAMP_MARGIN
    args = (case["poses"], case["patches"], case["intr"], case["ii"], case["jj"], case["kk"], case["grad"])
    want, fd = PT.vjp(*args), PT.fd_vjp(*args)
    for k in ("dposes", "dpatches"):
        w = np.asarray(want[k], np.float64)
        dev = np.abs(w - np.asarray(fd[k], np.float64)) / np.maximum(1, np.abs(w))
        print("P=%d %-8s worst |closed - difference| / max(1, |want|) = %.3e (largest |want| %.3e)" % (P, k, dev.max(), np.abs(w).max()))
        assert np.isfinite(dev).all() and dev.max() < TOL, k
    assert not np.asarray(want["dposes"])[:, 6].any()


def test_clamp_passes_no_gradient_below():
    """an edge whose pixels all lie below the clamp: its coords do not move with Z, so q_z = 0 and D = 10"""
    case = PT.make_case(3, 2, P=1, m=4, seed=1)
    case["patches"][:, 2] = 1.5                                                    # Z = 1 - 1.2 * 1.5 < 0 over 0 -> 1
    case["ii"][:], case["jj"][:] = 0, 1
    assert PT.clamp_report(case)[1] == 0
    args = (case["poses"], case["patches"], case["intr"], case["ii"], case["jj"], case["kk"], case["grad"])
    want, fd = PT.vjp(*args), PT.fd_vjp(*args)
    for k in ("dposes", "dpatches"):
        w = np.asarray(want[k], np.float64)
        assert (np.abs(w - np.asarray(fd[k], np.float64)) / np.maximum(1, np.abs(w))).max() < TOL


def _cases():
    for E, n, P in PT.TRUTH_CASES:
        yield "truth E=%d n=%d P=%d" % (E, n, P), PT.make_case(E, n, P=P), True
    for E in PT.SIZES_E:
        for n in PT.SIZES_N:
            yield "sizes E=%d n=%d" % (E, n), PT.make_case(E, n, structure=True), False


def test_gpu_inputs_meet_their_conditions():
    """every case of tests/test_transform_backward.py: |Z - 0.1| >= 1e-3 at every pixel (float64), so that float32 takes the
    truth's branch; the truth cases have pixels on each side of the clamp and behind the camera; intrinsics differ between
    frames and within a frame; inverse depths in [0.1, 2]; grids inside the 47 x 30 map; the size cases have their duplicate
    patch, their empty patch, a frame that is never a source, one that is never a target and a self edge"""
    for name, c, both_sides in _cases():
        gap, above, below, behind = PT.clamp_report(c)
        assert gap >= PT.CLAMP_MARGIN, (name, gap)
        if both_sides or (c["n"] >= 2 and c["E"] >= 255):
            assert above > 0 and below > 0 and behind > 0, name
        K = c["intr"]
        assert all(len(set(row.tolist())) == 4 for row in K), name
        assert all(len(set(K[:, col].tolist())) == len(K) for col in range(4)), name
        d = c["patches"][:, 2]
        assert d.min() >= 0.1 and d.max() <= 2.0, name
        x, y = c["patches"][:, 0], c["patches"][:, 1]
        assert x.min() >= 0 and x.max() <= PT.MAP_W - 1 and y.min() >= 0 and y.max() <= PT.MAP_H - 1, name
        nq = np.linalg.norm(c["poses"][:, 3:].astype(np.float64), axis=1)
        assert (np.abs(nq - 1) > 5e-4).all() and (np.abs(nq - 1) < 2e-3).all(), name
        if not both_sides:
            E, n, m = c["E"], c["n"], c["m"]
            assert (c["kk"] == 0).sum() == min(300, E // 2) and not (c["kk"] == m - 1).any(), name
            assert (c["ii"] == c["jj"]).any(), name
            if n >= 4:
                assert not (c["ii"] == 1).any() and not (c["jj"] == 2).any(), name
