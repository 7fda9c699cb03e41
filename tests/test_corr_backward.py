"""The altcorr backward (training) on the GPU: cdv_corr_bwd / cdv_patchify_bwd against float64 torch autograd on the
CPU, determinism (eager and graph replay), the autograd surface of altcorr.corr / patchify and the drop-in names.

Tolerance, elementwise: |g - g64| <= 2e-5 m64 + 1e-30, where m64 is the same autograd run on the absolute values of
the inputs and of the incoming gradient (the sum of absolute terms); float16 outputs add one final rounding
(2^-11 |g64|)."""
import sys

import pytest
import torch
import torch.nn.functional as F

from cdv_slam_amd import altcorr, ops
from tests.corr_torch_ref import corr_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(g, g64, m64, f16=False):
    g = g.detach().double().cpu()
    tol = 2e-5 * m64 + 1e-30
    if f16:
        tol = tol + 2.0 ** -11 * g64.abs()
    err = (g - g64).abs()
    assert bool((err <= tol).all()), "max err %.3e (tol there %.3e)" % (float(err.max()), float(tol.flatten()[err.argmax()]))


# ---------------------------------------------------------------------------------------------------
# correlation
# ---------------------------------------------------------------------------------------------------

def _corr_case(seed, B, N1, N2, C, P, H2, W2, M, radius, far=False, invalid=False, repeat=False, same=False):
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(B, N1, C, P, P, generator=g)
    f2 = torch.randn(B, N2, C, H2, W2, generator=g)
    # centres over the map and a margin of a window beyond it: windows partly and wholly off the map
    x = torch.rand(B, M, 1, 1, 1, generator=g) * (W2 + 4 * radius + 8) - (2 * radius + 4)
    y = torch.rand(B, M, 1, 1, 1, generator=g) * (H2 + 4 * radius + 8) - (2 * radius + 4)
    d = torch.randn(B, M, 2, P, P, generator=g) * 1.5
    coords = torch.cat([x, y], 2) + d
    ii = torch.randint(0, N1, (M,), generator=g)
    jj = torch.randint(0, N2, (M,), generator=g)
    if far:
        coords[:, ::7, 0] = 1e6
        coords[:, 3::7, 1] = -1e6
        coords[:, 5::11] = -1e6
    if invalid:
        ii[::9] = N1 + 3
        jj[4::9] = -1
        ii[6::13] = -2
    if repeat:
        ii[M // 2:] = ii[:M - M // 2]
        jj[M // 2:] = jj[:M - M // 2]
    if same:
        coords[:] = torch.tensor([W2 * 0.37, H2 * 0.61]).view(1, 1, 2, 1, 1)
        ii[:], jj[:] = ii[0], jj[0]
    D1 = 2 * radius + 1
    grad = torch.randn(B, M, D1, D1, P, P, generator=g)
    return f1, f2, coords, ii, jj, grad


def _corr_truth(f1, f2, coords, ii, jj, grad, radius):
    """float64 autograd through tests/corr_torch_ref.corr_torch(mode='truth'), batch by batch; edges with an index
    off the maps give zero in the forward and are left out"""
    B, N1 = f1.shape[:2]
    N2 = f2.shape[1]
    ok = (ii >= 0) & (ii < N1) & (jj >= 0) & (jj < N2)

    def run(a, b, gr):
        a, b = a.double().requires_grad_(), b.double().requires_grad_()
        for k in range(B):
            if int(ok.sum()) == 0:
                break
            out = corr_torch(a[k], b[k], coords[k][ok], ii[ok], jj[ok], radius, "truth")
            out.backward(gr[k][ok].double())
        z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
        return z(a), z(b)

    g1, g2 = run(f1, f2, grad)
    m1, m2 = run(f1.abs(), f2.abs(), grad.abs())
    return g1, g2, m1, m2


def _gpu(*ts):
    return [t.to(DEV) for t in ts]


CORR_CASES = {
    # name: (seed, B, N1, N2, C, P, H2, W2, M, radius, flags)
    "tiny_p1_r0_c8": (1, 1, 5, 3, 8, 1, 9, 11, 23, 0, {}),
    "tiny_p1_r1_c8": (2, 1, 5, 3, 8, 1, 9, 11, 23, 1, {}),
    "tiny_p3_r1_c24": (3, 1, 6, 4, 24, 3, 12, 14, 40, 1, {}),
    "p3_r3_c24": (4, 1, 20, 5, 24, 3, 30, 40, 300, 3, {}),
    "p3_r3_c128": (5, 1, 20, 5, 128, 3, 30, 40, 200, 3, {}),
    "p1_r3_c128": (6, 1, 20, 5, 128, 1, 30, 40, 200, 3, {}),
    "euroc_odd_width": (7, 1, 30, 6, 24, 3, 30, 47, 400, 3, {}),
    "batch2": (8, 2, 10, 4, 24, 3, 30, 40, 150, 3, {}),
    "off_map_invalid_repeated": (9, 1, 20, 5, 24, 3, 30, 40, 300, 3, {"far": True, "invalid": True, "repeat": True}),
    "all_coords_equal": (10, 1, 8, 3, 24, 3, 30, 40, 64, 3, {"same": True}),
    "sparse_level0": (11, 1, 360, 15, 24, 3, 120, 160, 5000, 3, {}),
    "sparse_level1": (12, 1, 360, 15, 24, 3, 30, 40, 5000, 3, {}),
}


@pytest.mark.parametrize("name", list(CORR_CASES))
def test_corr_backward_matches_float64_truth(name):
    seed, B, N1, N2, C, P, H2, W2, M, radius, flags = CORR_CASES[name]
    f1, f2, coords, ii, jj, grad = _corr_case(seed, B, N1, N2, C, P, H2, W2, M, radius, **flags)
    if name.startswith("sparse_level1"):
        coords = coords / 4
    g1, g2 = ops.corr_backward(*_gpu(f1, f2, coords, ii, jj, grad), radius)
    assert g1.shape == f1.shape and g2.shape == f2.shape and g1.dtype == g2.dtype == torch.float32
    t1, t2, m1, m2 = _corr_truth(f1, f2, coords, ii, jj, grad, radius)
    _close(g1, t1, m1)
    _close(g2, t2, m2)
    if name == "off_map_invalid_repeated":
        assert float(t2.abs().sum()) > 0 and float(t1.abs().sum()) > 0


def test_corr_backward_honours_need_and_empty_edges():
    f1, f2, coords, ii, jj, grad = _gpu(*_corr_case(20, 1, 6, 3, 8, 3, 12, 14, 30, 1))
    a1, a2 = ops.corr_backward(f1, f2, coords, ii, jj, grad, 1)
    n1, n2 = ops.corr_backward(f1, f2, coords, ii, jj, grad, 1, need=(True, False))
    assert n2 is None and torch.equal(n1, a1)
    n1, n2 = ops.corr_backward(f1, f2, coords, ii, jj, grad, 1, need=(False, True))
    assert n1 is None and torch.equal(n2, a2)
    e1, e2 = ops.corr_backward(f1, f2, coords[:, :0], ii[:0], jj[:0], grad[:, :0], 1)
    assert not e1.any() and not e2.any()
    # a permuted (non-contiguous) grad, as autograd hands it over
    gp = grad.permute(0, 1, 3, 2, 4, 5).contiguous().permute(0, 1, 3, 2, 4, 5)
    assert not gp.is_contiguous()
    p1, p2 = ops.corr_backward(f1, f2, coords, ii, jj, gp, 1)
    assert torch.equal(p1, a1) and torch.equal(p2, a2)


# ---------------------------------------------------------------------------------------------------
# patchify
# ---------------------------------------------------------------------------------------------------

def _patch_gather64(net, coords, radius):
    """the raw (2r+2)^2 gather of patchify_forward as float64 torch indexing (its adjoint is index_put_ with
    accumulate): net [B,C,H,W], coords [B,M,2] -> [B,M,C,D,D], zero off the map"""
    B, C, H, W = net.shape
    D = 2 * radius + 2
    off = torch.arange(D) - radius
    rows = coords[..., 1].floor().long()[:, :, None, None] + off[None, None, :, None]    # [B,M,D,1]
    cols = coords[..., 0].floor().long()[:, :, None, None] + off[None, None, None, :]    # [B,M,1,D]
    inside = (rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)                         # [B,M,D,D]
    bi = torch.arange(B)[:, None, None, None]
    vals = net[bi, :, rows.clamp(0, H - 1), cols.clamp(0, W - 1)]                        # [B,M,D,D,C]
    vals = torch.where(inside[..., None], vals, torch.zeros((), dtype=vals.dtype))
    return vals.permute(0, 1, 4, 2, 3)


def _patch_truth(net, coords, pg, radius):
    def run(n, g):
        n = n.double().requires_grad_()
        _patch_gather64(n, coords, radius).backward(g.double())
        return n.grad
    return run(net, pg), run(net.abs(), pg.abs())


def _patch_case(seed, B, C, H, W, M, radius, dtype, same=False):
    g = torch.Generator().manual_seed(seed)
    net = torch.randn(B, C, H, W, generator=g).to(dtype)
    # centres across every border and beyond it
    x = torch.rand(B, M, generator=g) * (W + 2 * radius + 6) - (radius + 3)
    y = torch.rand(B, M, generator=g) * (H + 2 * radius + 6) - (radius + 3)
    coords = torch.stack([x, y], -1)
    coords[:, ::17] = 1e6
    if same:
        coords[:] = torch.tensor([W * 0.5 + 0.25, H * 0.5 + 0.75])
    D = 2 * radius + 2
    pg = torch.randn(B, M, C, D, D, generator=g).to(dtype)
    return net, coords, pg


PATCH_CASES = {
    "r0_c384": (30, 1, 384, 30, 40, 200, 0, {}),
    "r1_c24": (31, 2, 24, 30, 40, 200, 1, {}),
    "r3_c3": (32, 1, 3, 20, 27, 150, 3, {}),
    "r1_c24_full": (33, 1, 24, 120, 160, 1200, 1, {}),
    "one_pixel": (34, 1, 24, 30, 40, 300, 1, {"same": True}),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("name", list(PATCH_CASES))
def test_patchify_backward_matches_float64_truth(name, dtype):
    seed, B, C, H, W, M, radius, flags = PATCH_CASES[name]
    net, coords, pg = _patch_case(seed, B, C, H, W, M, radius, dtype, **flags)
    out = ops.patchify_backward(*_gpu(net, coords, pg), radius)
    assert out.shape == net.shape and out.dtype == dtype
    t, m = _patch_truth(net, coords, pg, radius)
    _close(out, t, m, f16=dtype == torch.float16)


# ---------------------------------------------------------------------------------------------------
# determinism: eager and graph replay
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


def test_backward_is_deterministic_and_replays():
    f1, f2, coords, ii, jj, grad = _gpu(*_corr_case(40, 1, 8, 3, 24, 3, 30, 40, 400, 3, same=False))
    coords[:, :100] = coords[:, :1]        # a hot spot: many windows on one place
    a = ops.corr_backward(f1, f2, coords, ii, jj, grad, 3)
    b = ops.corr_backward(f1, f2, coords, ii, jj, grad, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    graph, out = _captured(lambda: ops.corr_backward(f1, f2, coords, ii, jj, grad, 3))
    for _ in range(2):
        out[0].fill_(float("nan"))
        out[1].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], a[0]) and torch.equal(out[1], a[1])

    for dtype in (torch.float32, torch.float16):
        net, pc, pg = _gpu(*_patch_case(41, 1, 24, 30, 40, 300, 1, dtype))
        pc[:, :100] = pc[:, :1]
        a = ops.patchify_backward(net, pc, pg, 1)
        assert torch.equal(a, ops.patchify_backward(net, pc, pg, 1))
        graph, out = _captured(lambda: ops.patchify_backward(net, pc, pg, 1))
        for _ in range(2):
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


# ---------------------------------------------------------------------------------------------------
# the autograd surface: altcorr.corr / altcorr.patchify
# ---------------------------------------------------------------------------------------------------

def _leaf_case(seed=50, M=300, radius=3):
    f1, f2, coords, ii, jj, grad = _gpu(*_corr_case(seed, 1, 20, 5, 24, 3, 30, 40, M, radius))
    return f1.requires_grad_(), f2.requires_grad_(), coords, ii, jj, grad


def test_altcorr_corr_autograd_equals_the_op():
    f1, f2, coords, ii, jj, grad = _leaf_case()
    out = altcorr.corr(f1, f2, coords, ii, jj, 3)
    with torch.no_grad():
        plain = altcorr.corr(f1, f2, coords, ii, jj, 3)
    assert out.requires_grad and torch.equal(out.detach(), plain)
    g1, g2 = torch.autograd.grad(out, (f1, f2), grad)
    r1, r2 = ops.corr_backward(f1.detach(), f2.detach(), coords, ii, jj, grad, 3)
    assert torch.equal(g1, r1) and torch.equal(g2, r2)
    # only fmap2 differentiable: fmap1 gets nothing and needs nothing
    f1d = f1.detach()
    out = altcorr.corr(f1d, f2, coords, ii, jj, 3)
    (g2b,) = torch.autograd.grad(out, (f2,), grad)
    assert torch.equal(g2b, r2)


def test_altcorr_corr_dropout_draws_like_the_reference():
    f1, f2, coords, ii, jj, grad = _leaf_case(seed=51)
    M = coords.shape[1]
    torch.manual_seed(123)
    out = altcorr.corr(f1, f2, coords, ii, jj, 3, dropout=0.2)
    g1, g2 = torch.autograd.grad(out, (f1, f2), grad)
    torch.manual_seed(123)
    keep = torch.rand(M, device=DEV) < 0.2
    assert 0 < int(keep.sum()) < M
    r1, r2 = ops.corr_backward(f1.detach(), f2.detach(), coords[:, keep], ii[keep], jj[keep], grad[:, keep], 3)
    assert torch.equal(g1, r1) and torch.equal(g2, r2)
    # dropout >= 1: no draw at all
    state = torch.cuda.get_rng_state()
    out = altcorr.corr(f1, f2, coords, ii, jj, 3, dropout=1)
    torch.autograd.grad(out, (f1, f2), grad)
    assert torch.equal(torch.cuda.get_rng_state(), state)


@pytest.mark.parametrize("mode", ["bilinear", "upperleft", "raw"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_altcorr_patchify_autograd(mode, dtype):
    net, coords, _ = _gpu(*_patch_case(60, 1, 24, 30, 40, 200, 1, dtype))
    with torch.no_grad():
        plain = altcorr.patchify(net, coords, 1, mode)
    leaf = net.clone().requires_grad_()
    out = altcorr.patchify(leaf, coords, 1, mode)
    assert out.requires_grad and out.dtype == plain.dtype and out.shape == plain.shape
    if mode == "bilinear":
        assert torch.allclose(out.detach(), plain, atol=1e-6, rtol=0)
    else:
        assert torch.equal(out.detach(), plain)
    go = torch.randn(out.shape, device=DEV, dtype=out.dtype)
    (g,) = torch.autograd.grad(out, (leaf,), go)
    # the chain rule through the mode's expression, then the raw gather's adjoint
    raw = ops.patchify_forward(net, coords, 1).requires_grad_()
    if mode == "bilinear":
        offset = coords - coords.floor()
        dx, dy = offset[:, :, None, None, None].unbind(dim=-1)
        o = ((1 - dy) * (1 - dx) * raw[..., :3, :3] + (1 - dy) * dx * raw[..., :3, 1:] + dy * (1 - dx) * raw[..., 1:, :3]
             + dy * dx * raw[..., 1:, 1:])
    elif mode == "upperleft":
        o = raw[..., :1, :1]
    else:
        o = raw
    (graw,) = torch.autograd.grad(o, (raw,), go)
    assert torch.equal(g, ops.patchify_backward(net, coords, graw, 1))
    if mode == "bilinear":       # coords are differentiable through the blend
        c = coords.clone().requires_grad_()
        out = altcorr.patchify(net, c, 1, mode)
        (gc,) = torch.autograd.grad(out.sum(), (c,))
        assert gc.shape == c.shape and bool(torch.isfinite(gc).all())


# ---------------------------------------------------------------------------------------------------
# a CorrBlock-shaped graph (net_cdv.py:390-403): both gradient routes into fmap
# ---------------------------------------------------------------------------------------------------

def _corr_block_loss(fmap, pcoords, coords, ii, jj, w, corr_fn, patchify_fn):
    N, C, H, W = fmap.shape[1:]
    gmap = patchify_fn(fmap[0], pcoords, 1).view(1, -1, C, 3, 3)
    pyramid = [fmap, F.avg_pool2d(fmap[0], 4, stride=4).view(1, N, C, H // 4, W // 4)]
    corrs = [corr_fn(gmap, pyramid[i], coords / (1, 4)[i], ii, jj, 3) for i in range(2)]
    return (torch.stack(corrs, -1).view(1, len(ii), -1) * w).sum()


def test_corr_block_graph_matches_float64_truth():
    g = torch.Generator().manual_seed(70)
    N, C, H, W, PPI, M = 4, 24, 48, 64, 12, 300
    fmap = torch.randn(1, N, C, H, W, generator=g)
    px = torch.rand(N, PPI, 1, generator=g) * (W - 6) + 3
    py = torch.rand(N, PPI, 1, generator=g) * (H - 6) + 3
    pcoords = torch.cat([px, py], -1)
    ii = torch.randint(0, N * PPI, (M,), generator=g)
    jj = torch.randint(0, N, (M,), generator=g)
    coords = torch.cat([torch.rand(1, M, 1, 3, 3, generator=g) * W, torch.rand(1, M, 1, 3, 3, generator=g) * H], 2)
    w = torch.randn(1, M, 7 * 7 * 9 * 2, generator=g)

    leaf = fmap.to(DEV).requires_grad_()
    loss = _corr_block_loss(leaf, pcoords.to(DEV), coords.to(DEV), ii.to(DEV), jj.to(DEV), w.to(DEV), altcorr.corr,
                            altcorr.patchify)
    loss.backward()

    def patchify64(net, c, r):          # the reference's bilinear expression over the float64 gather
        p = _patch_gather64(net, c, r)
        off = c - c.floor()
        dx, dy = off.double()[:, :, None, None, None].unbind(dim=-1)
        d = 2 * r + 1
        return ((1 - dy) * (1 - dx) * p[..., :d, :d] + (1 - dy) * dx * p[..., :d, 1:] + dy * (1 - dx) * p[..., 1:, :d]
                + dy * dx * p[..., 1:, 1:])

    def corr64(f1, f2, c, a, b, r):
        return corr_torch(f1[0], f2[0], c[0], a, b, r, "truth")[None]

    def truth(fm, ww):
        x = fm.double().requires_grad_()
        _corr_block_loss(x, pcoords, coords, ii, jj, ww.double(), corr64, patchify64).backward()
        return x.grad

    t, m = truth(fmap, w), truth(fmap.abs(), w.abs())
    _close(leaf.grad, t, m)


# ---------------------------------------------------------------------------------------------------
# the drop-in names, called the way the reference's CorrLayer / PatchLayer call them
# ---------------------------------------------------------------------------------------------------

def test_dropin_layers_train_like_altcorr():
    import cdv_slam_amd
    cdv_slam_amd.install_dropin()
    cc = sys.modules["cuda_corr"]

    class CorrLayer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fmap1, fmap2, coords, ii, jj, radius):
            ctx.save_for_backward(fmap1, fmap2, coords, ii, jj)
            ctx.radius = radius
            (corr,) = cc.forward(fmap1, fmap2, coords, ii, jj, radius)
            return corr

        @staticmethod
        def backward(ctx, grad):
            fmap1, fmap2, coords, ii, jj = ctx.saved_tensors
            g1, g2 = cc.backward(fmap1, fmap2, coords, ii, jj, grad, ctx.radius)
            return g1, g2, None, None, None, None

    class PatchLayer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, net, coords, radius):
            ctx.radius = radius
            ctx.save_for_backward(net, coords)
            (patches,) = cc.patchify_forward(net, coords, radius)
            return patches

        @staticmethod
        def backward(ctx, grad):
            net, coords = ctx.saved_tensors
            (g,) = cc.patchify_backward(net, coords, grad, ctx.radius)
            return g, None, None

    f1, f2, coords, ii, jj, grad = _leaf_case(seed=80)
    # the reference's forward returns the permuted view of its (y, x) volume: a non-contiguous grad comes back
    gperm = grad.permute(0, 1, 3, 2, 4, 5).contiguous().permute(0, 1, 3, 2, 4, 5)
    out = CorrLayer.apply(f1, f2, coords, ii, jj, 3)
    assert type(out) is torch.Tensor
    d1, d2 = torch.autograd.grad(out, (f1, f2), gperm)
    out = altcorr.corr(f1, f2, coords, ii, jj, 3)
    a1, a2 = torch.autograd.grad(out, (f1, f2), grad)
    assert torch.equal(d1, a1) and torch.equal(d2, a2)
    assert d1.dtype == f1.dtype and d1.shape == f1.shape and d1.device == f1.device
    assert d2.dtype == f2.dtype and d2.shape == f2.shape and d2.device == f2.device

    for dtype in (torch.float32, torch.float16):
        net, pc, _ = _gpu(*_patch_case(81, 1, 24, 30, 40, 200, 1, dtype))
        leaf = net.clone().requires_grad_()
        out = PatchLayer.apply(leaf, pc, 1)
        go = torch.randn(out.shape, device=DEV, dtype=out.dtype)
        (dg,) = torch.autograd.grad(out, (leaf,), go)
        out = altcorr.patchify(leaf, pc, 1, mode="raw")
        (ag,) = torch.autograd.grad(out, (leaf,), go)
        assert torch.equal(dg, ag) and dg.dtype == dtype and dg.shape == net.shape
