"""The truth of the Lie-op backward (tests/lie_grad_truth.py) checks itself, and the CPU side of cdv_lie_bwd.

Closed forms against central differences (h = 2^-16, lie_truth.lie in 80-bit long double where the platform has it) on the
whole input set of tests/lie_cases.py, every op, SO3 and SE3.  Required: finer than 1e-7 max(1, |want|) -- a truth coarser
than float32's u could not judge a float32 kernel.  Measured worst case over all ops and rows: 8.5e-9 (Jinv, SE3, theta in
[1, pi), |tau| = 100); log 2.3e-9, exp 2.1e-10, adj / adjT / act / act4 / projector 4e-11, mul 4.6e-12, inv 9.8e-13
(printed by test_closed_forms_against_differences).

Left out for log and Jinv only: the band `pi` and the |w| ~ 0 elements (lie_cases.W_SPECIAL), where phi and -phi are one
rotation and Jl^-1 has two values; both facts are asserted."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lie_cases as LC
import lie_grad_truth as GT
import lie_truth as LT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = [(LC.SO3, "SO3"), (LC.SE3, "SE3")]
TOL = 1e-7


def _differences(group, op, grad, inputs):
    n = len(inputs[0])
    if op == "projector":
        return {"P": GT.fd_projector(group, inputs[0]).reshape(n, -1)}
    if op == "Jinv":
        return {"Jinv": GT.fd_jinv(group, *inputs)}
    dx, dy = GT.fd_vjp(group, op, grad, *inputs)
    return {"dx": dx} if dy is None else {"dx": dx, "dy": dy}


@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_closed_forms_against_differences(group, gname):
    cases = LC.Cases(group, np.float64)
    unique = GT.log_is_unique(cases)
    assert 0 < (~unique).sum() < len(unique) // 10
    for op in GT.BWD_OPS + GT.EXTRA_OPS:
        grad, inputs, band, theta = GT.case_args(cases, op)
        rows = unique if op in ("log", "Jinv") else np.ones(len(band), bool)
        if op not in ("log", "Jinv"):
            assert rows.all()                                     # nothing is left out for any other op
        want, fd = GT.truth_outputs(group, op, grad, inputs), _differences(group, op, grad, inputs)
        for k in want:
            dev = np.abs(want[k] - fd[k])[rows] / np.maximum(1, np.abs(want[k][rows]))
            i = int(np.argmax(dev.max(1)))
            print("%s %-9s %-4s worst |closed - difference| / max(1, |want|) = %.3e  [%s]"
                  % (gname, op, k, float(dev.max()), cases.band_name(band[rows][i])))
            assert np.isfinite(dev).all() and dev.max() < TOL, (op, k)


def test_log_is_two_valued_at_pi():
    """what is left out is left out for a reason: at a rotation by pi, X and X with q -> -q are one element, Log gives phi
    or -phi, and Jl^-1 differs between them"""
    phi = np.array([[np.pi, 0, 0]])
    Jp, Jm = GT.left_jacobian_inverse(LC.SO3, phi), GT.left_jacobian_inverse(LC.SO3, -phi)
    assert np.abs(LT.rotation_matrix(LT.so3_exp(phi)) - LT.rotation_matrix(LT.so3_exp(-phi))).max() < 1e-15
    assert np.abs(Jp - Jm).max() > 1.0


def test_series_and_closed_forms_agree_where_they_overlap():
    """theta in [0.3, 0.7]: Q's coefficients by series (switch above) and by closed form (switch at 0), float64, each
    weighted with the power of theta it multiplies in Q, to 1e-15.  The SE3 left Jacobian and its inverse for |tau| = 1 add
    the three coefficients' errors: the closed forms subtract numbers of size theta, 1 and theta and divide by theta^3,
    theta^4, theta^5, i.e. up to 2 u / theta each once weighted, so 3 * 2 u / 0.3 + 4 u = 2.7e-15 for the matrices"""
    rng = np.random.default_rng(0)
    theta = rng.uniform(0.3, 0.7, 2000)
    s, c = GT.q_coeffs(theta, 10.0), GT.q_coeffs(theta, 0.0)
    for k, power in enumerate((1, 2, 3)):
        assert np.abs((s[k] - c[k]) * theta ** power).max() <= 1e-15
    xi = np.concatenate([LC._axes(rng, 2000), theta[:, None] * LC._axes(rng, 2000)], 1)
    for fn in (GT.left_jacobian, GT.left_jacobian_inverse):
        assert np.abs(fn(LC.SE3, xi, np.float64, 10.0) - fn(LC.SE3, xi, np.float64, 0.0)).max() <= (3 * 2 / 0.3 + 4) * 2.0 ** -53


# ---- the C ABI of the backward, without a GPU ---------------------------------------------------------------------------

def test_header_ctypes_and_library_agree_on_cdv_lie_bwd(tmp_path):
    from cdv_slam_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(ROOT, "include", "cdvslam_hip.h")).read()
    assert re.search(r"int\s+cdv_lie_bwd\s*\(\s*const\s+cdv_lie_bwd_args\s*\*\s*args\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert hasattr(lib, "cdv_lie_bwd") and _lib.SIGNATURES["cdv_lie_bwd"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    fields = [f[0] for f in _lib.LieBwdArgs._fields_]
    assert fields == ["group", "op", "dtype", "need", "n", "rep_x", "rep_y", "grad", "x", "y", "dx", "dy"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu", sizeof(cdv_lie_bwd_args));\n%s\nreturn 0;}\n'
                    % (os.path.join(ROOT, "include", "cdvslam_hip.h"),
                       "\n".join('printf(" %%zu", offsetof(cdv_lie_bwd_args, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = _lib.LieBwdArgs
    assert got == [ctypes.sizeof(A)] + [getattr(A, f).offset for f in fields]


def test_backward_argument_errors_are_codes():
    from cdv_slam_amd import _lib
    lib = _lib.load()
    a = 0x10000                                   # never dereferenced: every check sits in front of the launch

    def call(group=3, op=7, dtype=1, need=3, n=18, rx=1, ry=1, dx=a, dy=a):
        rec = _lib.LieBwdArgs(group, op, dtype, need, n, rx, ry, a, a, a, dx, dy)
        return lib.cdv_lie_bwd(ctypes.byref(rec), None)

    assert call(group=2) == -4 and b"SO3" in lib.cdv_last_error()
    assert call(group=4) == -4
    assert call(dtype=0) == -4 and b"dtype" in lib.cdv_last_error()
    assert call(op=8) == -2 and b"no backward" in lib.cdv_last_error()
    assert call(op=11) == -2
    assert call(n=19, rx=9) == -2 and b"multiple" in lib.cdv_last_error()
    assert call(rx=9, ry=2) == -2 and b"one grouped" in lib.cdv_last_error()
    assert call(n=130, rx=65) == -2
    assert call(dx=None) == -2 and b"dx" in lib.cdv_last_error()
    assert call(dy=None) == -2 and b"dy" in lib.cdv_last_error()
    assert call(dy=None, need=1, n=0) == 0        # an output that is not needed may be NULL
    assert call(op=1, dy=None, n=0) == 0          # a unary op has no second gradient to ask for
    assert call(n=0) == 0 and call(n=0, rx=9) == 0
    assert lib.cdv_lie_bwd(None, None) == -2


def test_backends_backward_refuses_cpu_tensors():
    """the HIP-only refusal (RuntimeError), not a missing backward (NotImplementedError, itself a RuntimeError)"""
    import cdv_slam_amd
    _, _, lb = cdv_slam_amd.install_dropin()
    X, a, p3, p4 = torch.zeros(2, 7), torch.zeros(2, 6), torch.zeros(2, 3), torch.zeros(2, 4)
    X[:, 6] = 1
    calls = [("expm_backward", (X, a)), ("logm_backward", (a, X)), ("inv_backward", (X, X)), ("mul_backward", (X, X, X)),
             ("adj_backward", (a, X, a)), ("adjT_backward", (a, X, a)), ("act_backward", (p3, X, p3)),
             ("act4_backward", (p4, X, p4)), ("projector", (X,)), ("Jinv", (X, a))]
    for name, args in calls:
        with pytest.raises(RuntimeError) as e:
            getattr(lb, name)(3, *args)
        assert not isinstance(e.value, NotImplementedError), name
    from cdv_slam_amd.lietorch import SE3
    with pytest.raises(RuntimeError) as e:
        SE3.exp(a.requires_grad_()).log().sum().backward()
    assert not isinstance(e.value, NotImplementedError)
