"""The Lie-op kernels (lie.hip, cdv_se3.h lt_*) and the BA pose retraction (se3_retract_raw) against the plain truth of
tests/lie_truth.py, at every rotation angle from 1e-9 to pi, on both sides of every series threshold, for q and -q, for
stored quaternions that are not unit length and for translations of 1e-3, 1 and 100.

Inputs, compared quantities and bounds: tests/lie_cases.py.  No bound is a fixed number: each is 4 x what the number format
costs the truth's own formulas on the same rows, plus 4 u scale, and is printed next to the kernel's error."""
import numpy as np
import pytest
import torch

import lie_cases as LC
import lie_truth as LT
from cdv_slam_amd import ops, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
GROUPS = [(LC.SO3, "SO3"), (LC.SE3, "SE3")]
DTYPES = [np.float32, np.float64]


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _run(group, op, args):
    return ops.lie_op(group, op, *[T(x) for x in args]).cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_ops_against_truth(group, gname, dtype):
    """every op, every row of the set, every band: the kernel's error within the band's bound"""
    cases = LC.Cases(group, dtype)
    print("\n%s %s: %d tangents, %d group elements" % (gname, np.dtype(dtype).name, len(cases.a), len(cases.X)))
    bad = LC.op_failures(cases, _run)
    assert not bad, "\n".join(LC.FAILURE % b for b in bad)
    # w >= 0 up to a rotation by pi.  The kernel forms theta in `dtype` (three squares, two sums, a square root: within 2 u
    # of the row's angle), and w = cos(theta / 2) is negative as soon as that theta is above pi.  So: strictly for every
    # angle that is still at most pi after 4 u, and down to -4 u (the rounding of a result of size 1) for the rows that are
    # pi to the last bits.
    w = _run(group, "exp", (cases.a,))[:, -1]
    u = LC.U[np.dtype(dtype)]
    assert np.all(w[cases.a_theta <= np.pi * (1 - 4 * u)] >= 0)
    assert np.all(w[cases.a_theta <= np.pi] >= -4 * u)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_batch_sizes(group, gname, dtype):
    """1, 255, 256 and 257 rows (the launch is 256 lanes per workgroup): each row of a short batch is, bit for bit, the row
    the full batch of a few thousand gave, which test_ops_against_truth holds to its bound"""
    cases = LC.Cases(group, dtype)
    rng = np.random.default_rng(5)
    for op in LC.OPS:
        args, _, _ = cases.args(op)
        full = ops.lie_op(group, op, *[T(x) for x in args])
        for n in LC.BATCHES:
            rows = np.sort(rng.permutation(len(args[0]))[:n])
            part = ops.lie_op(group, op, *[T(x[rows]) for x in args])
            assert part.shape[0] == n
            assert torch.equal(part.view(torch.uint8), full[torch.as_tensor(rows, device=DEV)].view(torch.uint8)), (op, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_round_trips(group, gname, dtype):
    """log(exp(a)) and exp(log(X)) through the kernel alone"""
    bad = LC.round_trip_failures(LC.Cases(group, dtype), _run)
    assert not bad, "\n".join(LC.FAILURE % b for b in bad)


def test_se3_class_is_the_kernel():
    """the lietorch.SE3 / SO3 classes hand the same rows to the same kernel: bit for bit what ops.lie_op returns"""
    from cdv_slam_amd.lietorch import SE3, SO3
    for cls, group in ((SO3, LC.SO3), (SE3, LC.SE3)):
        for dtype in DTYPES:
            c = LC.Cases(group, dtype)
            a, X, Y, b, p3, p4 = (T(x) for x in (c.a, c.X, c.Y, c.b, c.p3, c.p4))
            G = cls(X)
            eq = lambda u, v: torch.equal(u.reshape(-1), v.reshape(-1))
            assert eq(cls.exp(a).data, ops.lie_op(group, "exp", a))
            assert eq(G.log(), ops.lie_op(group, "log", X))
            assert eq(G.inv().data, ops.lie_op(group, "inv", X))
            assert eq((G * cls(Y)).data, ops.lie_op(group, "mul", X, Y))
            assert eq(G * p3, ops.lie_op(group, "act", X, p3))
            assert eq(G * p4, ops.lie_op(group, "act4", X, p4))
            assert eq(G.adj(b), ops.lie_op(group, "adj", X, b))
            assert eq(G.adjT(b), ops.lie_op(group, "adjT", X, b))
            assert eq(G.matrix(), ops.lie_op(group, "matrix", X))
            n = len(c.a)
            assert eq(cls(X[:n]).retr(a).data, ops.lie_op(group, "mul", ops.lie_op(group, "exp", a), X[:n].contiguous()))


# ---------------------------------------------------------------------------------------------------
# the retraction of the three BA paths
# ---------------------------------------------------------------------------------------------------

def reference_retraction_f32(xi, P):
    """the float32 evaluation of the reference's retraction (fastba: series of the quaternion below theta^2 = 1e-8, the
    translation's rotation coupling only above theta = 1e-4, (1 - cos theta) / theta^2), every intermediate in float32"""
    f = np.float32
    xi, P = np.asarray(xi, f), np.asarray(P, f)
    tau, phi = xi[:, :3], xi[:, 3:]
    th2 = (phi * phi).sum(1)
    th = np.sqrt(th2)
    th4 = th2 * th2
    tiny = th2 < f(1e-8)
    safe = np.where(th > 0, th, f(1))
    sv = np.where(tiny, f(0.5) - th2 * f(1 / 48) + th4 * f(1 / 3840), np.sin(f(0.5) * safe) / safe)
    cw = np.where(tiny, f(1) - th2 * f(1 / 8) + th4 * f(1 / 384), np.cos(f(0.5) * th))
    dq = np.concatenate([sv[:, None] * phi, cw[:, None]], 1)
    w1 = LT.cross(phi, tau)
    w2 = LT.cross(phi, w1)
    a = (f(1) - np.cos(safe)) / (safe * safe)
    b = (safe - np.sin(safe)) / (safe * safe * safe)
    dt = tau + np.where((th > f(1e-4))[:, None], a[:, None] * w1 + b[:, None] * w2, f(0))
    t = LT.rotate(dq, P[:, :3], dtype=f, load=False) + dt
    return np.concatenate([t, LT.quat_mul(dq, P[:, 3:], dtype=f)], 1)


NOISE = [1e-2, 1.0, 30.0]
RETRACT_GRAPHS = [("default", "window"), ("stress", "mid"), ("global", "global")]


@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("name,path", RETRACT_GRAPHS, ids=[g[0] for g in RETRACT_GRAPHS])
def test_ba_retraction(name, path, noise):
    """one BA iteration: the poses written are the truth's retraction Exp(dX) P of the kernel's own dX (the iteration's
    dump, promoted exactly) applied to the input poses, within 4 x the error the float32 evaluation of the reference's own
    retraction formula makes on the same dX.  The targets' perturbation is scaled by `noise`, which moves the rotation
    increments across 1e-5 ... 1e-2 (asserted over the three scales by test_ba_retraction_angles_covered)."""
    st = _scaled_state(name, noise)
    N = st.n - st.t0
    assert {"window": N <= 10, "mid": 10 < N <= 32, "global": N > 32}[path]
    poses, dX = _one_iteration(st)
    P0 = st.poses[st.t0:st.n]
    want = LT.retract(dX, P0)
    ref = reference_retraction_f32(dX, P0)
    theta = np.linalg.norm(dX[:, 3:].astype(np.float64), axis=1)
    hist, edges = np.histogram(np.log10(np.maximum(theta, 1e-12)), bins=np.arange(-12, 2))
    print("\n%s x%g: N = %d, |phi| of dX in [%.2e, %.2e], |tau| up to %.2e; decades %s" %
          (name, noise, N, theta.min(), theta.max(), np.abs(dX[:, :3]).max(),
           {int(e): int(h) for e, h in zip(edges[:-1], hist) if h}))
    for part, sl in (("t", slice(0, 3)), ("q", slice(3, 7))):
        e_ref = float(np.abs(ref[:, sl] - want[:, sl]).max())
        e_got = float(np.abs(poses[st.t0:st.n, sl] - want[:, sl]).max())
        e_half = float(np.abs(LT.retract(dX, P0, dtype=np.float32)[:, sl] - want[:, sl]).max())
        print("  %s: kernel err %.3e, reference formula in float32 err %.3e (bound %.3e), the truth's formulas (half-angle c1, "
              "coupling at every angle) in float32 err %.3e" % (part, e_got, e_ref, 4 * e_ref, e_half))
        assert e_got <= 4 * e_ref, (part, e_got, e_ref)
    # the poses that are not free are not touched
    assert np.array_equal(poses[:st.t0], st.poses[:st.t0]) and np.array_equal(poses[st.n:], st.poses[st.n:])


def test_ba_retraction_angles_covered():
    """the three noise scales together put rotation increments of each path into every decade between 1e-5 and 1e-2:
    [1e-5, 1e-4), [1e-4, 1e-3) and [1e-3, 1e-2) are all populated"""
    for name, _ in RETRACT_GRAPHS:
        theta = np.concatenate([np.linalg.norm(_one_iteration(_scaled_state(name, noise))[1][:, 3:].astype(np.float64), axis=1)
                                for noise in NOISE])
        decades = np.floor(np.log10(theta[theta > 0])).astype(int)
        hist = {int(d): int((decades == d).sum()) for d in np.unique(decades)}
        print("%s: |phi| of dX from %.2e to %.2e, poses per decade %s" % (name, theta.min(), theta.max(), hist))
        assert {-5, -4, -3}.issubset(hist), (name, hist)


def _scaled_state(name, noise):
    """the named graph with the perturbation of its targets (N(0, 1) px around the exact reprojection) scaled by `noise`"""
    st = synth.make_state(name, features=False)
    exact = _exact_targets(st)
    st.target = (exact + noise * (st.target.astype(np.float64) - exact)).astype(np.float32)
    return st


def _exact_targets(st):
    """the reprojection of the patch centres at the state's own poses, in float64 (the truth's act on (x, y, 1, d))"""
    poses = st.poses.astype(np.float64)
    fx, fy, cx, cy = st.intrinsics[0].astype(np.float64)
    Gij = LT.se3_mul(poses[st.jj], LT.se3_inv(poses[st.ii], dtype=np.float64), dtype=np.float64)
    c = st.patches[st.kk, :, 1, 1].astype(np.float64)
    ray = np.stack([(c[:, 0] - cx) / fx, (c[:, 1] - cy) / fy, np.ones(len(c)), c[:, 2]], 1)
    Y = LT.se3_act4(Gij, ray, dtype=np.float64)
    z = np.maximum(Y[:, 2], 0.1)
    return np.stack([fx * Y[:, 0] / z + cx, fy * Y[:, 1] / z + cy], 1)


_RUNS = {}


def _one_iteration(st):
    key = (st.cfg.name, float(np.abs(st.target).sum()))
    if key not in _RUNS:
        _RUNS[key] = _run_one_iteration(st)
    return _RUNS[key]


def _run_one_iteration(st):
    poses, patches = T(st.poses).clone(), T(st.patches).clone()
    dbg = ops.ba_forward(poses, patches, T(st.intrinsics), T(st.target), T(st.weight),
                         torch.tensor([st.lmbda], device=DEV), T(st.ii), T(st.jj), T(st.kk), st.cfg.M, st.t0, st.n, 1, False,
                         debug=True)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), dbg["dX"].cpu().numpy()
