"""The Lie-op backward (csrc/lie_bwd.hip, cdv_lie_bwd) and the forward-shaped `projector` / `Jinv` against the closed-form
truth of tests/lie_grad_truth.py, on the input set of tests/lie_cases.py: every rotation angle from 1e-9 to pi, q and -q,
stored quaternions that are not unit length, translations of 1e-3, 1 and 100.

No bound is a fixed number or looks at the kernel: per op, output, band and dtype it is 4 x what the number format costs the
truth's own closed forms on the same rows plus 4 u max(1, |want|) (lie_grad_truth.bounds), printed next to the error.  For
log and Jinv the band `pi` and the |w| ~ 0 elements are left out (Jl^-1 has two values there, test_lie_grad_truth_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import lie_cases as LC
import lie_grad_truth as GT
import lie_truth as LT
from cdv_slam_amd import _lib, ops
from tests import guard_arena as GA

pytestmark = pytest.mark.gpu

DEV = "cuda"
GROUPS = [(LC.SO3, "SO3"), (LC.SE3, "SE3")]
DTYPES = [np.float32, np.float64]
TD = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
GROUPED = [("act", 0), ("act4", 0), ("mul", 0), ("mul", 1)]           # (op, which operand is grouped)
REPS = [1, 2, 9, 64]
GROUP_ROWS = [1, 255, 256, 257]


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _run(group, op, grad, inputs):
    """{name: rows} of the package for one op of the truth's table"""
    if op in GT.EXTRA_OPS:
        out = ops.lie_op(group, op, *[T(x) for x in inputs])
        return {"P" if op == "projector" else "Jinv": _np(out).reshape(len(inputs[0]), -1)}
    dx, dy = ops.lie_backward(group, op, T(grad), *[T(x) for x in inputs])
    return {"dx": _np(dx)} if dy is None else {"dx": _np(dx), "dy": _np(dy)}


_CASES = {}


def _cases(group, dtype):
    key = (group, np.dtype(dtype))
    if key not in _CASES:
        _CASES[key] = LC.Cases(group, dtype)
    return _CASES[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_ops_against_truth(group, gname, dtype):
    """the eight backward ops, projector and Jinv: every row of the set, every band, within the band's bound"""
    cases = _cases(group, dtype)
    unique = GT.log_is_unique(cases)
    K, N = GT.dims(group)
    bad = []
    for op in GT.BWD_OPS + GT.EXTRA_OPS:
        grad, inputs, band, theta = GT.case_args(cases, op)
        rows = unique if op in ("log", "Jinv") else np.ones(len(band), bool)
        want, bnd = GT.bounds(group, op, grad, inputs, band, dtype, rows)
        got = _run(group, op, grad, inputs)
        assert got.keys() == want.keys()
        for k in want:
            assert got[k].dtype == cases.dtype and got[k].shape == want[k].shape, (op, k)
            err = LC.band_max((got[k].astype(LC.REF) - want[k])[rows], band[rows])
            bad += [(op,) + b for b in LC.report(cases, op, {k: err}, {k: bnd[k]})]
        if op in ("log", "inv", "mul", "adj", "adjT", "act", "act4"):      # a group element's gradient: K words and a zero
            assert not got["dx"][:, K:].any(), op
        if op == "mul":
            assert not got["dy"][:, K:].any()
    assert not bad, "\n".join(LC.FAILURE % b for b in bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_batch_sizes(group, gname, dtype):
    """1, 255, 256 and 257 rows (256 lanes per workgroup): bit for bit the rows of the full batch"""
    cases = _cases(group, dtype)
    rng = np.random.default_rng(5)
    for op in GT.BWD_OPS + GT.EXTRA_OPS:
        grad, inputs, _, _ = GT.case_args(cases, op)
        full = _run(group, op, grad, inputs)
        for n in LC.BATCHES:
            rows = np.sort(rng.permutation(len(inputs[0]))[:n])
            part = _run(group, op, grad[rows], [x[rows] for x in inputs])
            for k in full:
                assert len(part[k]) == n and GA.same_bits(part[k], full[k][rows]), (op, k, n)


# ---------------------------------------------------------------------------------------------------
# one operand grouped: [n / m] rows, each used by m consecutive rows of the call
# ---------------------------------------------------------------------------------------------------

def _grouped_case(group, dtype, op, which, m, n_groups, seed=0):
    """(grad, [x, y] with operand `which` holding n_groups rows and the other n_groups * m) from the input set"""
    cases = _cases(group, dtype)
    grad, inputs, _, _ = GT.case_args(cases, op)
    rng = np.random.default_rng(seed + 131 * m + n_groups)
    n = n_groups * m
    rows = rng.integers(0, len(grad), n)
    short = rng.integers(0, len(grad), n_groups)
    ins = [inputs[i][short] if i == which else inputs[i][rows] for i in range(2)]
    return grad[rows], ins


def _sequential_sum(rows, m, dtype):
    """[n / m, w]: the m rows of each group added in ascending order, every partial sum rounded to `dtype`"""
    r = np.asarray(rows, dtype).reshape(-1, m, rows.shape[1])
    acc = r[:, 0].copy()
    for j in range(1, m):
        acc = acc + r[:, j]
    return acc


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("op,which", GROUPED, ids=["%s-%s" % (o, "xy"[w]) for o, w in GROUPED])
def test_grouped_operand(op, which, dtype):
    """m in {1, 2, 9, 64} x {1, 255, 256, 257} groups (SE3): the other operand's gradient is, bit for bit, the ungrouped call's
    on expanded rows; the grouped operand's is that call's rows summed, within 4 x what adding them in ascending order costs
    in `dtype` (against the sum in lie_truth.REF, float64 or wider) + 4 u max(1, |sum|); two runs give the same bits"""
    group, u = LC.SE3, LC.U[np.dtype(dtype)]
    for m in REPS:
        for n_groups in GROUP_ROWS:
            grad, ins = _grouped_case(group, dtype, op, which, m, n_groups)
            rep = (m, 1) if which == 0 else (1, m)
            g, a = T(grad), [T(x) for x in ins]
            got = ops.lie_backward(group, op, g, *a, rep=rep)
            again = ops.lie_backward(group, op, g, *a, rep=rep)
            expanded = [x.repeat_interleave(m, 0) if i == which else x for i, x in enumerate(a)]
            flat = ops.lie_backward(group, op, g, *expanded)
            assert got[which].shape == a[which].shape
            assert GA.same_bits(got[0], again[0]) and GA.same_bits(got[1], again[1]), (m, n_groups)
            assert GA.same_bits(got[1 - which], flat[1 - which]), (m, n_groups)
            rows = _np(flat[which]).astype(LC.REF)
            want = rows.reshape(n_groups, m, -1).sum(1)
            bound = float(4 * np.abs(_sequential_sum(rows, m, dtype).astype(LC.REF) - want).max() + 4 * u * max(1.0, np.abs(want).max()))
            err = float(np.abs(_np(got[which]).astype(LC.REF) - want).max())
            print("  %s grouped %s m=%d groups=%d: err %.3e bound %.3e" % (op, "xy"[which], m, n_groups, err, bound))
            assert err <= bound, (m, n_groups, err, bound)


def test_grouped_need_and_empty():
    """`need` leaves the buffer that is not asked for untouched (grouped and not), and n = 0 is served"""
    group, dtype, m, n_groups = LC.SE3, np.float32, 9, 257
    grad, ins = _grouped_case(group, dtype, "act4", 0, m, n_groups)
    g, x, y = T(grad), T(ins[0]), T(ins[1])
    full = ops.lie_backward(group, "act4", g, x, y, rep=(m, 1))
    lib = _lib.load()
    for rep_x, xs in ((m, x), (1, x.repeat_interleave(m, 0).contiguous())):
        ref = ops.lie_backward(group, "act4", g, xs, y, rep=(rep_x, 1))
        for need in (1, 2):
            dx, dy = torch.full_like(xs, 7.0), torch.full_like(y, 7.0)
            rec = _lib.LieBwdArgs(group, ops.LIE_OPS["act4"], ops.F32, need, len(g), rep_x, 1, g.data_ptr(), xs.data_ptr(),
                                  y.data_ptr(), dx.data_ptr(), dy.data_ptr())
            _lib.check(lib.cdv_lie_bwd(ctypes.byref(rec), torch.cuda.current_stream().cuda_stream), "cdv_lie_bwd")
            kept, written, want = (dy, dx, ref[0]) if need == 1 else (dx, dy, ref[1])
            assert bool((kept == 7.0).all()) and GA.same_bits(written, want), (rep_x, need)
        only_x = ops.lie_backward(group, "act4", g, xs, y, need=(True, False), rep=(rep_x, 1))
        assert only_x[1] is None and GA.same_bits(only_x[0], ref[0])
    assert GA.same_bits(full[0], ops.lie_backward(group, "act4", g, x, y, rep=(m, 1))[0])
    e = ops.lie_backward(group, "act4", g[:0], x[:0], y[:0], rep=(m, 1))
    assert e[0].shape == (0, 7) and e[1].shape == (0, 4)
    e = ops.lie_backward(group, "log", g[:0, :0].reshape(0, 6), x[:0])
    assert e[0].shape == (0, 7) and e[1] is None


def test_rep_65_falls_back_in_the_classes():
    """65 points per pose is beyond the grouped kernel: groups.py expands and torch sums; the gradients agree with the m = 64
    style evaluation of the truth"""
    from cdv_slam_amd.lietorch import SE3
    rng = np.random.default_rng(3)
    a = rng.standard_normal((5, 6)) * 0.3
    p = rng.standard_normal((5, 65, 4))
    w = rng.standard_normal((5, 65, 4))
    X = LT.se3_exp(a)
    xt = T(np.asarray(X, np.float64)).requires_grad_()
    pt = T(p).requires_grad_()
    ((SE3(xt)[:, None] * pt) * T(w)).sum().backward()
    Xe = np.repeat(np.asarray(X, np.float64), 65, 0)
    dx, dp = GT.vjp(LC.SE3, "act4", w.reshape(-1, 4), Xe, p.reshape(-1, 4))
    assert np.abs(_np(xt.grad) - np.asarray(dx, np.float64).reshape(5, 65, 7).sum(1)).max() <= 1e-12 * 65
    assert np.abs(_np(pt.grad).reshape(-1, 4) - np.asarray(dp, np.float64)).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------
# capture and replay; guard bands
# ---------------------------------------------------------------------------------------------------

def _captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def test_backward_replays():
    grad, ins = _grouped_case(LC.SE3, np.float32, "act4", 0, 9, 257)
    g, x, y = T(grad), T(ins[0]), T(ins[1])
    eager = ops.lie_backward(LC.SE3, "act4", g, x, y, rep=(9, 1))
    graph, out = _captured(lambda: ops.lie_backward(LC.SE3, "act4", g, x, y, rep=(9, 1)))
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert GA.same_bits(out[0], eager[0]) and GA.same_bits(out[1], eager[1])


N256 = [1, 255, 256, 257, 1009]      # one lane per row, 256 lanes per workgroup; grouped: floor(256 / m) groups per workgroup


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_guard_bands(group, gname, dtype):
    """the four conditions of tests/test_bounds_audit.py for cdv_lie_bwd: (a) every guard byte intact, (b) NaN-guarded and
    zero-guarded runs bit-identical, (c) the result meets the truth within the bound of test_ops_against_truth's style, (d)
    bit for bit the ops.lie_backward call.  Sizes 1, 255, 256, 257, 1009 rows (ungrouped) or groups (m = 9: 28 groups per
    workgroup, the last one partly filled)."""
    td, u = TD[np.dtype(dtype)], LC.U[np.dtype(dtype)]
    K, N = GT.dims(group)
    lib = _lib.load()
    for n_rows in N256:
        for op, which, m in [(o, None, 1) for o in GT.BWD_OPS] + [("act4", 0, 9), ("mul", 1, 9)]:
            rng = np.random.default_rng(n_rows)
            n = n_rows * m
            a = (0.5 * rng.standard_normal((n, K))).astype(dtype)
            X = np.asarray(LT.lie(group, "exp", a), dtype)
            second = {"mul": np.asarray(LT.lie(group, "exp", a[::-1].copy()), dtype), "adj": a, "adjT": a,
                      "act": rng.standard_normal((n, 3)).astype(dtype), "act4": rng.standard_normal((n, 4)).astype(dtype)}.get(op)
            ins = [a] if op == "exp" else [X] if second is None else [X, second]
            if which is not None:
                ins[which] = np.ascontiguousarray(ins[which][:n_rows])
            width = {"exp": N, "log": K, "inv": N, "mul": N, "adj": K, "adjT": K, "act": 3, "act4": 4}[op]
            grad = rng.standard_normal((n, width)).astype(dtype)
            rep = [1, 1]
            if which is not None:
                rep[which] = m

            def fn(ar):
                gt = ar.tensor("grad", grad)
                ts = [ar.tensor("xy"[i], v) for i, v in enumerate(ins)]
                outs = [ar.tensor("d" + "xy"[i], v.shape, td) for i, v in enumerate(ins)]
                rec = _lib.LieBwdArgs(group, ops.LIE_OPS[op], ops._DT[td], 3, n, rep[0], rep[1], gt.data_ptr(), ts[0].data_ptr(),
                                      ts[1].data_ptr() if len(ts) > 1 else None, outs[0].data_ptr(),
                                      outs[1].data_ptr() if len(outs) > 1 else None)
                _lib.check(lib.cdv_lie_bwd(ctypes.byref(rec), torch.cuda.current_stream().cuda_stream), "cdv_lie_bwd")
                return {"d" + "xy"[i]: o for i, o in enumerate(outs)}

            what = "cdv_lie_bwd %s n=%d m=%d" % (op, n, m)
            got = GA.run_twice(fn, DEV, row_bytes=N * np.dtype(dtype).itemsize, capacity=1 << 22, what=what)
            direct = ops.lie_backward(group, op, T(grad), *[T(v) for v in ins], rep=tuple(rep))
            expanded = [np.repeat(v, m, 0) if i == which else v for i, v in enumerate(ins)]
            want = GT.vjp(group, op, grad.astype(LC.REF), *[v.astype(LC.REF) for v in expanded])
            low = GT.vjp(group, op, grad.astype(LC.REF), *[v.astype(LC.REF) for v in expanded], dtype=dtype)
            for i in range(len(ins)):
                name = "d" + "xy"[i]
                assert GA.same_bits(got[name], direct[i]), (what, name)
                w, l = np.asarray(want[i], np.float64), np.asarray(low[i], np.float64)
                if i == which:
                    l = _sequential_sum(l, m, dtype).astype(np.float64)
                    w = w.reshape(n_rows, m, -1).sum(1)
                bound = 4 * np.abs(l - w).max() + 4 * u * max(1.0, np.abs(w).max())
                assert np.abs(got[name].numpy().astype(np.float64) - w).max() <= bound, (what, name)


# ---------------------------------------------------------------------------------------------------
# autograd through the classes
# ---------------------------------------------------------------------------------------------------

def _chains(cls):
    rng = np.random.default_rng(11)
    K = cls.manifold_dim
    b = T(rng.standard_normal((3, K)))
    p3, p4, p94 = T(rng.standard_normal((3, 3))), T(rng.standard_normal((3, 4))), T(rng.standard_normal((3, 9, 4)))
    X0 = cls.exp(T(0.4 * rng.standard_normal((3, K))))
    return {
        "exp-log": (lambda a: cls.exp(a).log(), 1),
        "exp-exp-mul-log": (lambda a, c: (cls.exp(a) * cls.exp(c)).log(), 2),
        "exp-inv-log": (lambda a: cls.exp(a).inv().log(), 1),
        "exp-adj": (lambda a, v: cls.exp(a).adj(v), (1, b)),
        "exp-adjT": (lambda a, v: cls.exp(a).adjT(v), (1, b)),
        "exp-act": (lambda a, p: cls.exp(a) * p, (1, p3)),
        "exp-act4": (lambda a, p: cls.exp(a) * p, (1, p4)),
        "exp-act4-grouped": (lambda a, p: cls.exp(a)[:, None] * p, (1, p94)),
        "retr": (lambda a: X0.retr(a).log(), 1),
    }


@pytest.mark.parametrize("chain", ["exp-log", "exp-exp-mul-log", "exp-inv-log", "exp-adj", "exp-adjT", "exp-act", "exp-act4",
                                   "exp-act4-grouped", "retr"])
@pytest.mark.parametrize("gname", ["SO3", "SE3"])
def test_gradcheck(gname, chain):
    """torch.autograd.gradcheck, float64, default tolerances, 3 rows: Euclidean-to-Euclidean chains that together cross all
    eight ops"""
    from cdv_slam_amd import lietorch
    cls = getattr(lietorch, gname)
    fn, spec = _chains(cls)[chain]
    rng = np.random.default_rng(12)
    n_tangent, extra = (spec, ()) if isinstance(spec, int) else (spec[0], spec[1:])
    args = [T(0.5 * rng.standard_normal((3, cls.manifold_dim))).requires_grad_() for _ in range(n_tangent)]
    args += [e.clone().requires_grad_() for e in extra]
    assert torch.autograd.gradcheck(fn, args)


def _training_case():
    rng = np.random.default_rng(21)
    poses = np.asarray(LT.se3_exp(0.3 * rng.standard_normal((1, 4, 6))), np.float64)
    poses[..., 3:] *= 1.0 + 1e-3 * rng.standard_normal((1, 4, 1))
    ii, jj = np.repeat(np.arange(4), 3), np.array([1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2])
    X0 = rng.standard_normal((1, 12, 3, 3, 4))
    X0[..., 2] = 1.0
    W = rng.standard_normal((1, 12, 3, 3, 4))
    return poses, ii, jj, X0, W


def test_training_chain():
    """4 poses, 12 edges, 3 x 3 points, as projective_ops.transform composes them: Gij = P[:, jj] * P[:, ii].inv(),
    X1 = Gij[:, :, None, None] * X0, a weighted sum.  The gradients by pose data and X0 against the truth's composition of
    its own closed forms (the scatter of the two gathers added in float64); float64, 1e-12 max(1, |want|)"""
    from cdv_slam_amd.lietorch import SE3
    poses, ii, jj, X0, W = _training_case()
    pt, xt = T(poses).requires_grad_(), T(X0).requires_grad_()
    P = SE3(pt)
    Gij = P[:, T(jj)] * P[:, T(ii)].inv()
    X1 = Gij[:, :, None, None] * xt
    (X1 * T(W)).sum().backward()
    # the truth, backwards: act4 (summed over the 9 points of an edge), mul, inv, then the two gathers
    Pj, Pi = poses[0, jj], poses[0, ii]
    Pinv = LT.se3_inv(Pi)
    G = LT.se3_mul(Pj, Pinv)
    dG9, dX0 = GT.vjp(LC.SE3, "act4", W.reshape(-1, 4), np.repeat(G, 9, 0), X0.reshape(-1, 4))
    dG = dG9.reshape(12, 9, 7).sum(1)
    dPj, dPinv = GT.vjp(LC.SE3, "mul", dG, Pj, Pinv)
    dPi, _ = GT.vjp(LC.SE3, "inv", dPinv, Pi)
    want = np.zeros((4, 7), LC.REF)
    np.add.at(want, jj, dPj)
    np.add.at(want, ii, dPi)
    want = np.asarray(want, np.float64)
    assert np.abs(_np(pt.grad)[0] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    dX0 = np.asarray(dX0, np.float64).reshape(X0.shape)
    assert np.abs(_np(xt.grad) - dX0).max() <= 1e-12 * max(1.0, np.abs(dX0).max())


def test_pose_loss_chain():
    """(dP * dG.inv()).log() of the training loss, weighted and summed: gradients by both operands' data against the truth"""
    from cdv_slam_amd.lietorch import SE3
    rng = np.random.default_rng(22)
    A = np.asarray(LT.se3_exp(0.3 * rng.standard_normal((1, 6, 6))), np.float64)
    B = np.asarray(LT.se3_exp(0.3 * rng.standard_normal((1, 6, 6))), np.float64)
    W = rng.standard_normal((1, 6, 6))
    at, bt = T(A).requires_grad_(), T(B).requires_grad_()
    ((SE3(at) * SE3(bt).inv()).log() * T(W)).sum().backward()
    Binv = LT.se3_inv(B[0])
    dZ, _ = GT.vjp(LC.SE3, "log", W[0], LT.se3_mul(A[0], Binv))
    dA, dBinv = GT.vjp(LC.SE3, "mul", dZ, A[0], Binv)
    dB, _ = GT.vjp(LC.SE3, "inv", dBinv, B[0])
    for got, want in ((at.grad, dA), (bt.grad, dB)):
        want = np.asarray(want, np.float64)
        assert np.abs(_np(got)[0] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_vec_and_initfromvec_go_through_the_projector():
    from cdv_slam_amd.lietorch import SE3
    rng = np.random.default_rng(23)
    X = T(np.asarray(LT.se3_exp(0.3 * rng.standard_normal((5, 6))), np.float64))
    w = T(rng.standard_normal((5, 7)))
    a = T(0.1 * rng.standard_normal((5, 6))).requires_grad_()
    (SE3(X).retr(a).vec() * w).sum().backward()                      # d(stored row of Exp(a) X) / da at a: (w P) Jl(a)
    Z = LT.se3_mul(LT.se3_exp(_np(a.detach())), _np(X))
    g = GT._pad(GT._vm(_np(w).astype(LC.REF), GT.projector(LC.SE3, Z))[:, :6])
    want = np.asarray(GT.vjp(LC.SE3, "exp", g, _np(a.detach()))[0], np.float64)
    assert np.abs(_np(a.grad) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    d = X.clone().requires_grad_()
    (SE3.InitFromVec(d).log() * w[:, :6]).sum().backward()           # back out through pinv(P)
    dX = np.asarray(GT.vjp(LC.SE3, "log", _np(w)[:, :6], _np(X))[0], np.float64)
    Pm = np.asarray(GT.projector(LC.SE3, _np(X)), np.float64)
    want = np.einsum("ni,nij->nj", dX, np.linalg.pinv(Pm))
    assert np.abs(_np(d.grad) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_group_op_pattern_over_the_installed_backends():
    """the reference's GroupOp pattern (forward op, grad.contiguous(), backward op) restated over the installed
    lietorch_backends: the same gradients as the classes"""
    import cdv_slam_amd
    from cdv_slam_amd.lietorch import SE3
    _, _, lb = cdv_slam_amd.install_dropin()

    def group_op(fwd, bwd):
        class Op(torch.autograd.Function):
            @staticmethod
            def forward(ctx, group_id, *inputs):
                ctx.group_id = group_id
                ctx.save_for_backward(*inputs)
                return fwd(group_id, *inputs)

            @staticmethod
            def backward(ctx, grad):
                return (None,) + tuple(bwd(ctx.group_id, grad.contiguous(), *ctx.saved_tensors))
        return Op

    Exp, Log, Inv, Mul, Act4 = (group_op(getattr(lb, f), getattr(lb, b)) for f, b in
                                (("expm", "expm_backward"), ("logm", "logm_backward"), ("inv", "inv_backward"),
                                 ("mul", "mul_backward"), ("act4", "act4_backward")))
    rng = np.random.default_rng(31)
    a0, c0, p0 = (T(rng.standard_normal(s)) for s in ((7, 6), (7, 6), (7, 4)))
    w6, w4 = T(rng.standard_normal((7, 6))), T(rng.standard_normal((7, 4)))
    grads = []
    for style in ("backends", "classes"):
        a, c, p = (t.clone().requires_grad_() for t in (a0, c0, p0))
        if style == "backends":
            X, Y = Exp.apply(3, a), Exp.apply(3, c)
            Z = Mul.apply(3, X, Inv.apply(3, Y))
            loss = (Log.apply(3, Z) * w6).sum() + (Act4.apply(3, Z, p) * w4).sum()
        else:
            Z = SE3.exp(a) * SE3.exp(c).inv()
            loss = (Z.log() * w6).sum() + ((Z * p) * w4).sum()
        loss.backward()
        grads.append((a.grad, c.grad, p.grad))
    for u, v in zip(*grads):
        assert GA.same_bits(u, v)
    with pytest.raises(NotImplementedError):
        lb.expm_backward(2, w6, a0)
    with pytest.raises(NotImplementedError):
        lb.act4_backward(4, w4, a0, p0)
