"""The backward of the fused projective_ops.transform (csrc/transform_bwd.hip, cdv_transform_bwd) against the closed-form truth
of tests/pops_grad_truth.py, on the inputs that module fixes (tests/test_pops_grad_truth_cpu.py asserts their conditions).

No bound is a fixed number or looks at the kernel: per output word it is 4 |truth evaluated in float32 - truth| + 4 u max(1, S)
with S the sum of the absolute values of the word's per-edge contributions (pops_grad_truth.bounds).  The worst error / bound
ratio of every test goes to profiles/transform_bwd_pytest_gpu.log."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pops_grad_truth as PT
from cdv_slam_amd import _lib, ops
from cdv_slam_amd import projective_ops as pops
from tests import guard_arena as GA

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "transform_bwd_pytest_gpu.log")


def _log(line):
    print(line)
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")


def _call(lib, *fields):
    """cdv_transform_bwd on a record of raw addresses and sizes, on the current stream -> the return code"""
    return lib.cdv_transform_bwd(ctypes.byref(_lib.TransformBwdArgs(*fields)), torch.cuda.current_stream().cuda_stream)


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _tensors(c):
    """(poses [1,n,7], patches [1,m,3,P,P], intr [1,n,4], ii, jj, kk, grad [1,E,P,P,2]) of a case on the device"""
    return (T(c["poses"])[None], T(c["patches"])[None], T(c["intr"])[None], T(c["ii"]), T(c["jj"]), T(c["kk"]), T(c["grad"])[None])


_TRUTH = {}


def _truth(key, case):
    """(want, bounds) of a case, computed once"""
    if key not in _TRUTH:
        _TRUTH[key] = PT.bounds(case)
    return _TRUTH[key]


def _ratio(got, want, bound):
    err = np.abs(got.detach().cpu().numpy().astype(np.float64).reshape(want.shape) - np.asarray(want, np.float64))
    return float((err / bound.reshape(want.shape)).max())


def _check(what, got, want, bnd):
    worst = {}
    for k, g in zip(("dposes", "dpatches"), got):
        if g is not None:
            worst[k] = _ratio(g, want[k], bnd[k])
    _log("%s: worst error / bound %s" % (what, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert all(np.isfinite(v) and v <= 1.0 for v in worst.values()), (what, worst)


@pytest.mark.parametrize("E,n,P", PT.TRUTH_CASES, ids=["P%d" % c[2] for c in PT.TRUTH_CASES])
def test_truth(E, n, P):
    """both layouts of grad, every `need`: within the bound of the truth; a single-output call gives the bits of its half of
    the two-output call"""
    case = PT.make_case(E, n, P=P)
    want, bnd = _truth(("truth", E, n, P), case)
    poses, patches, intr, ii, jj, kk, grad = _tensors(case)
    e2pp = grad.permute(0, 1, 4, 2, 3).contiguous()
    variants = {"EPP2": dict(grad=grad), "E2PP view": dict(grad=e2pp.permute(0, 1, 3, 4, 2)),
                "E2PP flag": dict(grad=e2pp, layout_e2pp=True)}
    strided = torch.empty((1, E, P, P, 4), device=DEV)[..., ::2]
    strided.copy_(grad)
    variants["strided"] = dict(grad=strided)
    assert ops._grad_layout(e2pp.permute(0, 1, 3, 4, 2), E, P)[1] or P == 1
    assert ops._grad_layout(e2pp.permute(0, 1, 3, 4, 2), E, P)[0].data_ptr() == e2pp.data_ptr()
    both = None
    for name, kw in variants.items():
        full = ops.transform_backward(poses, patches, intr, ii, jj, kk, **kw)
        assert full[0].shape == poses.shape and full[1].shape == patches.shape
        _check("truth P=%d %s" % (P, name), full, want, bnd)
        both = both or full
        assert GA.same_bits(full[0], both[0]) and GA.same_bits(full[1], both[1]), name
        only_p = ops.transform_backward(poses, patches, intr, ii, jj, kk, need=(True, False), **kw)
        only_x = ops.transform_backward(poses, patches, intr, ii, jj, kk, need=(False, True), **kw)
        assert only_p[1] is None and only_x[0] is None
        assert GA.same_bits(only_p[0], full[0]) and GA.same_bits(only_x[1], full[1]), name
    assert not full[0][..., 6].any()
    assert ops.transform_backward(poses, patches, intr, ii, jj, kk, grad, need=(False, False)) == (None, None)
    with pytest.raises(TypeError):
        ops.transform_backward(poses.double(), patches, intr, ii, jj, kk, grad)
    with pytest.raises(TypeError):
        ops.transform_backward(poses, patches, intr, ii, jj, kk, grad.double())
    with pytest.raises(RuntimeError):
        ops.transform_backward(poses.cpu(), patches, intr, ii, jj, kk, grad)


@pytest.mark.parametrize("n", PT.SIZES_N)
@pytest.mark.parametrize("E", PT.SIZES_E)
def test_sizes(E, n):
    """E around the tile and workgroup sizes x n from all self edges to more frames than lanes; a patch with (up to) 300
    duplicate edges, a patch with none, a frame that is never a source, one that is never a target, a self edge"""
    case = PT.make_case(E, n, structure=True)
    want, bnd = _truth(("sizes", E, n), case)
    poses, patches, intr, ii, jj, kk, grad = _tensors(case)
    got = ops.transform_backward(poses, patches, intr, ii, jj, kk, grad)
    _check("sizes E=%d n=%d" % (E, n), got, want, bnd)
    dposes, dpatches = got[0][0].cpu().numpy(), got[1][0].cpu().numpy()
    assert not dposes[:, 6].any()
    used = np.zeros(case["m"], bool)
    used[case["kk"]] = True
    assert not used[case["m"] - 1] and not dpatches[~used].any() and np.isfinite(dpatches).all()
    seen = np.zeros(n, bool)
    seen[case["ii"]] = True
    seen[case["jj"]] = True
    assert not dposes[~seen].any() and np.isfinite(dposes).all()


def test_no_edges_gives_zeros():
    case = PT.make_case(5, 4)
    poses, patches, intr, ii, jj, kk, grad = _tensors(case)
    dposes, dpatches = ops.transform_backward(poses, patches, intr, ii[:0], jj[:0], kk[:0], grad[:, :0])
    assert dposes.shape == poses.shape and dpatches.shape == patches.shape
    assert not dposes.any() and not dpatches.any()
    lib = _lib.load()
    args = [p.data_ptr() for p in (poses, patches, intr, ii, jj, kk)]
    out = [torch.empty_like(poses), torch.empty_like(patches)]
    assert _call(lib, *args, 5, 4, case["m"], 3, 0, grad.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), None) == -2
    ws = torch.empty(int(lib.cdv_transform_bwd_workspace_bytes(5, 4, case["m"], 3)), dtype=torch.uint8, device=DEV)
    assert _call(lib, *args, 5, 4, case["m"], 2, 0, grad.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr()) == -4
    assert _call(lib, *args, 5, 4, case["m"], 3, 2, grad.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr()) == -4
    assert lib.cdv_transform_bwd(None, None) == -2


def test_bitwise_reproducible():
    """two runs into NaN-filled outputs (and a NaN-filled workspace): the same bits, nothing left unwritten"""
    case = PT.make_case(1000, 33, structure=True)
    poses, patches, intr, ii, jj, kk, grad = _tensors(case)
    lib = _lib.load()
    E, n, m = case["E"], case["n"], case["m"]
    outs = []
    for fill in (float("nan"), float("nan"), 0.0):
        ws = torch.full((int(lib.cdv_transform_bwd_workspace_bytes(E, n, m, 3)) // 4 + 1,), fill, device=DEV)
        dposes, dpatches = torch.full_like(poses, float("nan")), torch.full_like(patches, float("nan"))
        rc = _call(lib, poses.data_ptr(), patches.data_ptr(), intr.data_ptr(), ii.data_ptr(), jj.data_ptr(), kk.data_ptr(), E, n, m, 3, 0,
                   grad.data_ptr(), dposes.data_ptr(), dpatches.data_ptr(), ws.data_ptr())
        _lib.check(rc, "cdv_transform_bwd")
        outs.append((dposes, dpatches))
    assert not torch.isnan(outs[0][0]).any() and not torch.isnan(outs[0][1]).any()
    for o in outs[1:]:
        assert GA.same_bits(o[0], outs[0][0]) and GA.same_bits(o[1], outs[0][1])
    direct = ops.transform_backward(poses, patches, intr, ii, jj, kk, grad)
    assert GA.same_bits(direct[0], outs[0][0]) and GA.same_bits(direct[1], outs[0][1])


def test_captured_and_replayed():
    case = PT.make_case(257, 5)
    poses, patches, intr, ii, jj, kk, grad = _tensors(case)
    fn = lambda: ops.transform_backward(poses, patches, intr, ii, jj, kk, grad)
    eager = fn()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    for _ in range(2):
        for o in out:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert GA.same_bits(out[0], eager[0]) and GA.same_bits(out[1], eager[1])


@pytest.mark.parametrize("E", [1, 257])
def test_guard_bands(E):
    """every tensor of cdv_transform_bwd, the workspace included, flush between guards; indices on the last frame and patch;
    guards intact, the result independent of what they hold, within the bound of the truth and the bits of the ops call"""
    case = PT.make_case(E, 5)
    n, m, P = case["n"], case["m"], 3
    case["ii"][-1], case["jj"][-1], case["kk"][-1] = n - 1, n - 1, m - 1
    if E > 1:
        case["ii"][0], case["jj"][0], case["kk"][0] = 0, n - 1, m - 1
    assert PT.clamp_report(case)[0] >= PT.CLAMP_MARGIN
    lib = _lib.load()
    nbytes = int(lib.cdv_transform_bwd_workspace_bytes(E, n, m, P))

    def fn(ar):
        t = {k: ar.tensor(k, case[k]) for k in ("poses", "patches", "intr", "grad")}
        ix = {k: ar.tensor(k, case[k], index_max=(m - 1 if k == "kk" else n - 1)) for k in ("ii", "jj", "kk")}
        dposes, dpatches = ar.tensor("dposes", (n, 7), torch.float32), ar.tensor("dpatches", (m, 3, P, P), torch.float32)
        ws = ar.tensor("workspace", (nbytes,), torch.uint8, fill=0xCD)
        rc = _call(lib, t["poses"].data_ptr(), t["patches"].data_ptr(), t["intr"].data_ptr(), ix["ii"].data_ptr(), ix["jj"].data_ptr(),
                   ix["kk"].data_ptr(), E, n, m, P, 0, t["grad"].data_ptr(), dposes.data_ptr(), dpatches.data_ptr(), ws.data_ptr())
        _lib.check(rc, "cdv_transform_bwd")
        return {"dposes": dposes, "dpatches": dpatches}

    got = GA.run_twice(fn, DEV, row_bytes=3 * P * P * 4, capacity=1 << 22, what="cdv_transform_bwd E=%d" % E)
    want, bnd = PT.bounds(case)
    _check("guard bands E=%d" % E, (got["dposes"], got["dpatches"]), want, bnd)
    poses, patches, intr, ii, jj, kk, grad = _tensors(case)
    direct = ops.transform_backward(poses, patches, intr, ii, jj, kk, grad)
    assert GA.same_bits(direct[0], got["dposes"]) and GA.same_bits(direct[1], got["dpatches"])


# ---------------------------------------------------------------------------------------------------
# autograd through projective_ops.transform
# ---------------------------------------------------------------------------------------------------

def _loss(coords, w1, w2):
    """the net_cdv.py pattern: the [1,E,2,P,P] copy feeds one term, the centre pixel another"""
    c = coords.shape[2] // 2
    return (coords.permute(0, 1, 4, 2, 3).contiguous() * w1).sum() + (coords[..., c, c, :] * w2).sum()


def _composed_f64(case, w1, w2):
    """the reference's formula over this package's iproj / proj and Lie classes, float64"""
    from cdv_slam_amd.lietorch import SE3
    p = T(case["poses"].astype(np.float64))[None].requires_grad_()
    x = T(case["patches"].astype(np.float64))[None].requires_grad_()
    K = T(case["intr"].astype(np.float64))[None]
    ii, jj, kk = T(case["ii"]), T(case["jj"]), T(case["kk"])
    G = SE3(p)
    Gij = G[:, jj] * G[:, ii].inv()
    X1 = Gij[:, :, None, None] * pops.iproj(x[:, kk], K[:, ii])
    coords = pops.proj(X1, K[:, jj])
    _loss(coords, w1.double(), w2.double()).backward()
    return p.grad, x.grad


def test_autograd_training_pattern(monkeypatch):
    from cdv_slam_amd.lietorch import SE3
    E, n, P = 257, 5, 3
    case = PT.make_case(E, n, P=P)
    poses, patches, intr, ii, jj, kk, _ = _tensors(case)
    rng = np.random.default_rng(5)
    w1, w2 = T(rng.standard_normal((1, E, 2, P, P)).astype(np.float32)), T(rng.standard_normal((1, E, 2)).astype(np.float32))
    with torch.no_grad():
        plain = pops.transform(SE3(poses), patches, intr, ii, jj, kk)
    p, x = poses.clone().requires_grad_(), patches.clone().requires_grad_()
    coords = pops.transform(SE3(p), x, intr, ii, jj, kk)
    assert coords.shape == plain.shape and coords.stride() == plain.stride() and GA.same_bits(coords, plain)
    _loss(coords, w1, w2).backward()
    assert p.grad is not None and x.grad is not None
    # the gradient the loss sends back, as the truth takes it
    g = w1.permute(0, 1, 3, 4, 2).clone()
    g[:, :, P // 2, P // 2, :] += w2
    case = dict(case, grad=g[0].cpu().numpy())
    want, bnd = PT.bounds(case)
    _check("autograd (SE3 poses and patches)", (p.grad, x.grad), want, bnd)
    cp, cx = _composed_f64(case, w1, w2)
    for name, got, ref in (("dposes", p.grad, cp), ("dpatches", x.grad, cx)):
        r = _ratio(got, ref.cpu().numpy().reshape(want[name].shape), bnd[name])
        _log("autograd against the composed float64 path: %s worst error / bound %.3f" % (name, r))
        assert r <= 1.0, name
    # one input at a time, and a plain pose tensor
    p2 = poses.clone().requires_grad_()
    _loss(pops.transform(p2, patches, intr, ii, jj, kk), w1, w2).backward()
    assert GA.same_bits(p2.grad, p.grad)
    x2 = patches.clone().requires_grad_()
    _loss(pops.transform(poses, x2, intr, ii, jj, kk), w1, w2).backward()
    assert GA.same_bits(x2.grad, x.grad)
    # valid=True: the mask carries no graph, the coords the same gradient
    p3 = poses.clone().requires_grad_()
    c3, mask = pops.transform(SE3(p3), patches, intr, ii, jj, kk, valid=True)
    with torch.no_grad():
        c0, mask0 = pops.transform(SE3(poses), patches, intr, ii, jj, kk, valid=True)
    assert not mask.requires_grad and GA.same_bits(mask, mask0) and GA.same_bits(c3, c0)
    _loss(c3, w1, w2).backward()
    assert GA.same_bits(p3.grad, p.grad)
    # without grad: the compiled lane and the launches of today -- counted at the two doors a call can leave through
    calls = {"fast": 0, "ops": 0, "bwd": 0}
    fast = ops._fast_mod()
    assert fast

    class Counting:
        def __getattr__(self, name):
            return getattr(fast, name)

        def transform(self, *a):
            calls["fast"] += 1
            return fast.transform(*a)

    real_transform, real_bwd = ops.transform, ops.transform_backward
    monkeypatch.setattr(ops, "_fast", Counting())
    monkeypatch.setattr(ops, "transform", lambda *a, **k: (calls.__setitem__("ops", calls["ops"] + 1), real_transform(*a, **k))[1])
    monkeypatch.setattr(ops, "transform_backward", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), real_bwd(*a, **k))[1])
    monkeypatch.delenv("CDV_DROPIN_FAST", raising=False)
    with torch.no_grad():
        out = pops.transform(SE3(p), x, intr, ii, jj, kk)
    assert calls == {"fast": 1, "ops": 0, "bwd": 0} and not out.requires_grad and GA.same_bits(out, plain)
    out = pops.transform(SE3(poses), patches, intr, ii, jj, kk)                    # grad mode on, nothing requires grad
    assert calls == {"fast": 2, "ops": 0, "bwd": 0} and not out.requires_grad
    out = pops.transform(SE3(p), x, intr, ii, jj, kk)
    assert calls == {"fast": 2, "ops": 1, "bwd": 0} and out.requires_grad


def test_jacobian_under_grad():
    from cdv_slam_amd.lietorch import SE3
    E, n, P = 257, 5, 3
    case = PT.make_case(E, n, P=P)
    poses, patches, intr, ii, jj, kk, _ = _tensors(case)
    with torch.no_grad():
        c0, v0, (Ji0, Jj0, Jz0) = pops.transform(SE3(poses), patches, intr, ii, jj, kk, jacobian=True)
    p, x = poses.clone().requires_grad_(), patches.clone().requires_grad_()
    c1, v1, (Ji, Jj, Jz) = pops.transform(SE3(p), x, intr, ii, jj, kk, jacobian=True)
    assert GA.same_bits(c1, c0) and GA.same_bits(v1, v0) and not v1.requires_grad and c1.requires_grad
    assert Ji.shape == Ji0.shape and Jj.shape == Jj0.shape and Jz.shape == Jz0.shape
    # float32 rounding, by the rule of lie_grad_truth.bounds: the fused Jacobians lie within 4 x what float32 costs the composed
    # formulas (the composed float32 run against its own float64 run, largest over the tensor) + 4 u max(1, largest |J|) of the
    # float64 run
    p64, x64 = poses.double().requires_grad_(), patches.double().requires_grad_()
    J64 = pops._jacobians_composed(SE3(p64), x64, intr.double(), ii, jj, kk)
    rng = np.random.default_rng(9)
    ws = [T(rng.standard_normal(tuple(J.shape))) for J in J64]
    for name, a, b, r in zip(("Ji", "Jj", "Jz"), (Ji, Jj, Jz), (Ji0, Jj0, Jz0), J64):
        a, r = a.detach(), r.detach()
        bound = 4 * float((a.double() - r).abs().max()) + 4 * PT.U32 * max(1.0, float(r.abs().max()))
        ratio = float((b.double() - r).abs().max()) / bound
        _log("jacobian=True under grad: fused %s against the composed float64 run, worst error / bound %.3f" % (name, ratio))
        assert ratio <= 1.0, name
    # gradients of the composed Jacobians: float32 run against the float64 run of the same function.  A Jacobian entry carries
    # d = 1 / Z up to the second power and its derivative the third (|d| <= 5 where it is not zero: 125), and a pose row sums the
    # entries of every edge that names it: 1e-4 of the largest gradient word is ~13 u per unit of that factor
    sum(((J * w.float()).sum() for J, w in zip((Ji, Jj, Jz), ws))).backward()
    sum(((J * w).sum() for J, w in zip(J64, ws))).backward()
    for name, g32, g64 in (("poses", p.grad, p64.grad), ("patches", x.grad, x64.grad)):
        scale = float(g64.abs().max())
        err = float((g32.double() - g64).abs().max())
        _log("jacobian=True under grad: d(Ji, Jj, Jz)/d%s float32 against float64, worst |difference| %.3e of largest %.3e" % (name, err, scale))
        assert err <= 1e-4 * max(1.0, scale), name
    # what is not built says so
    k = intr.clone().requires_grad_()
    with pytest.raises(NotImplementedError):
        pops.transform(SE3(p), x, k, ii, jj, kk)
    with pytest.raises(NotImplementedError):
        pops.transform(SE3(p), x, intr, ii, jj, kk, tonly=True)
    with pytest.raises(NotImplementedError):
        pops.transform(SE3(p), x, intr, ii, jj, kk, depth=True)


def test_dropin_pose_object_receives_its_gradient(tmp_path, monkeypatch):
    """install_dropin(package=...) on a stand-in package: its projective_ops is ours, and a pose object that carries its rows in
    `.data` with group_id 3 (the reference's lietorch.SE3) gets the gradient on `.data`"""
    import importlib
    import sys
    import cdv_slam_amd
    pkg = tmp_path / "standin_train"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "slam.py").write_text("from . import projective_ops as pops\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    cdv_slam_amd.install_dropin(package="standin_train")
    try:
        slam = importlib.import_module("standin_train.slam")
        assert slam.pops is pops

        class TheirSE3:
            group_id = 3

            def __init__(self, data):
                self.data = data

        case = PT.make_case(257, 5)
        want, bnd = _truth(("truth", 257, 5, 3), case)
        poses, patches, intr, ii, jj, kk, grad = _tensors(case)
        G = TheirSE3(poses.clone().requires_grad_())
        coords = slam.pops.transform(G, patches, intr, ii, jj, kk)
        (coords * grad).sum().backward()
        assert G.data.grad is not None
        _check("drop-in pose object", (G.data.grad, None), want, bnd)
    finally:
        for name in ("standin_train", "standin_train.slam", "standin_train.projective_ops"):
            sys.modules.pop(name, None)
