"""GPU parity tests: every HIP entry point (through the C ABI) against the CPU oracle on the same
seeded inputs, plus the golden fixtures captured from the reference's Python files.

Tolerances: reprojected coords atol 1e-3 px; corr f16 path
|d| <= 2^-8 max|corr| + 2^-10 vs the float64 truth; S/y/C/u/E rtol 1e-4 (of the matrix scale);
poses after 2 GN iterations atol 1e-5 (t) / 1e-6 (q) and inverse depth rtol 1e-4 vs the float64
oracle on the window graphs (small, default, stress); explicit per-config numbers plus gauge-free bounds for the
weak-gauge graphs (init, pr1, global): tests/ba_checks.py; BIT-EXACT for kx, ku, neighbors.
"""
import os

import numpy as np
import pytest
import torch

from cdv_slam_amd import ops, synth
from oracle import oracle as O
from tests import ba_checks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _check_mode():
    os.environ["CDV_CHECK"] = "1"
    yield
    os.environ["CDV_CHECK"] = "0"


def T(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV) if dtype is None else \
        torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------------
# lietorch ops
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", [O.SO3, O.SE3])
@pytest.mark.parametrize("dtype,tol", [(np.float32, 2e-6), (np.float64, 1e-13)])
def test_lie_ops(group, dtype, tol):
    rng = np.random.default_rng(7)
    K, N = (6, 7) if group == O.SE3 else (3, 4)
    n = 1000
    a = (0.5 * rng.standard_normal((n, K))).astype(dtype)
    a[0] = 0
    a[1, -3:] = 1e-8  # Taylor branches
    b = rng.standard_normal((n, K)).astype(dtype)
    p3 = rng.standard_normal((n, 3)).astype(dtype)
    p4 = rng.standard_normal((n, 4)).astype(dtype)
    X = O.lie(group, "exp", a, dtype=dtype)
    Y = O.lie(group, "exp", b, dtype=dtype)
    Xg = ops.lie_op(group, "exp", T(a))
    assert np.allclose(Xg.cpu().numpy(), X, atol=tol)
    Xt, Yt = T(X), T(Y)
    cases = [("log", (Xt,), (X,)), ("inv", (Xt,), (X,)), ("mul", (Xt, Yt), (X, Y)), ("adj", (Xt, T(b)), (X, b)),
             ("adjT", (Xt, T(b)), (X, b)), ("act", (Xt, T(p3)), (X, p3)), ("act4", (Xt, T(p4)), (X, p4)),
             ("matrix", (Xt,), (X,))]
    for op, gargs, oargs in cases:
        got = ops.lie_op(group, op, *gargs).cpu().numpy()
        want = O.lie(group, op, *oargs, dtype=dtype)
        scale = max(1.0, np.abs(want).max())
        assert np.allclose(got, want, atol=tol * scale * 8), op


def test_lietorch_classes_golden(golden_dir):
    """the SE3 class surface reproduces the reference Python layer's outputs (groups.py broadcasting)"""
    from cdv_slam_amd.lietorch import SE3
    g = np.load(os.path.join(golden_dir, "lietorch_py.npz"))
    a, b, p4 = T(g["a"]), T(g["b"]), T(g["p4"])
    X, Y = SE3.exp(a), SE3.exp(b)
    tol = 1e-12
    assert np.allclose(X.data.cpu().numpy(), g["X"], atol=tol)
    assert np.allclose((X * Y).data.cpu().numpy(), g["XY"], atol=tol)
    assert np.allclose(X.inv().data.cpu().numpy(), g["Xinv"], atol=tol)
    assert np.allclose(X.log().cpu().numpy(), g["logX"], atol=tol)
    assert np.allclose((X[:, :, None] * p4).cpu().numpy(), g["act4"], atol=tol)
    assert np.allclose(X.matrix().cpu().numpy(), g["matrix"], atol=tol)
    assert np.allclose(X.adjT(a).cpu().numpy(), g["adjT"], atol=tol)
    assert np.allclose(X.adj(a).cpu().numpy(), g["adj"], atol=tol)
    assert np.allclose(X.retr(a).data.cpu().numpy(), g["retr"], atol=tol)


# ---------------------------------------------------------------------------------------------------
# projective ops
# ---------------------------------------------------------------------------------------------------

def test_transform_golden(golden_dir):
    """fused cdv_transform vs outputs of the reference's own projective_ops.py"""
    _transform_vs_pops_fixture(os.path.join(golden_dir, "pops_transform_f32.npz"))


def test_transform_golden_euroc(golden_dir):
    """the same at 480x752 with per-frame EuRoC intrinsics, no two of fx, fy, cx, cy equal (tests/golden/pops_euroc_f64.npz,
    the reference's projective_ops.py in float64): the roles of fx / fy / cx / cy in tf_pixel and point_cloud are pinned"""
    g = np.load(os.path.join(golden_dir, "pops_euroc_f64.npz"))
    assert all(len(set(row)) == 4 for row in g["intrinsics"].tolist())
    _transform_vs_pops_fixture(os.path.join(golden_dir, "pops_euroc_f64.npz"))


def _transform_vs_pops_fixture(path):
    from cdv_slam_amd import projective_ops as pops
    from cdv_slam_amd.lietorch import SE3
    g = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in np.load(path).items()}
    poses, patches, intr = T(g["poses"])[None], T(g["patches"])[None], T(g["intrinsics"])[None]
    ii, jj, kk = T(g["ii"]), T(g["jj"]), T(g["kk"])
    x1 = pops.transform(SE3(poses), patches, intr, ii, jj, kk)
    assert x1.shape == (1,) + g["coords"].shape
    assert np.abs(x1[0].cpu().numpy() - g["coords"]).max() < 1e-3
    x1j, v, (Ji, Jj, Jz) = pops.transform(SE3(poses), patches, intr, ii, jj, kk, jacobian=True)
    assert np.array_equal(v[0].cpu().numpy(), g["valid"])
    for a, b in ((Ji, g["Ji"]), (Jj, g["Jj"]), (Jz, g["Jz"])):
        assert a.shape == (1,) + b.shape
        assert np.allclose(a[0].cpu().numpy(), b, rtol=1e-4, atol=1e-4 * np.abs(b).max())
    x1v, val = pops.transform(SE3(poses), patches, intr, ii, jj, kk, valid=True)
    assert np.array_equal(val[0].cpu().numpy(), g["validpx"])
    x1t = pops.transform(SE3(poses), patches, intr, ii, jj, kk, tonly=True)
    assert np.abs(x1t[0].cpu().numpy() - g["coords_tonly"]).max() < 1e-3
    fm, fv = pops.flow_mag(SE3(poses), patches, intr, ii, jj, kk, beta=0.5)
    assert np.allclose(fm[0].cpu().numpy(), g["flow_mag"], atol=2e-3)
    assert np.array_equal(fv[0].cpu().numpy(), g["flow_valid"])
    ix = T(g["point_cloud_ix"])
    pc = pops.point_cloud(SE3(poses), patches[:, :len(ix)], intr, ix)
    assert np.allclose(pc[0].cpu().numpy(), g["point_cloud"], rtol=1e-4, atol=1e-4)
    # SLAM.reproject layout
    rp = pops.reproject(SE3(poses), patches, intr, ii, jj, kk)
    assert torch.equal(rp, x1.permute(0, 1, 4, 2, 3).contiguous())


@pytest.mark.parametrize("name", ["small", "default", "euroc"])
def test_transform_vs_oracle(name):
    st = synth.make_state(name, features=False)
    coords = ops.transform(T(st.poses)[None], T(st.patches)[None], T(st.intrinsics)[None], T(st.ii), T(st.jj),
                           T(st.kk), layout_e2pp=True)
    want = O.transform(st.poses, st.patches, st.intrinsics, st.ii, st.jj, st.kk, dtype=np.float64)
    assert np.abs(coords[0].cpu().numpy() - want.transpose(0, 3, 1, 2)).max() < 1e-3
    fr = ops.fastba_reproject(T(st.poses), T(st.patches), T(st.intrinsics), T(st.ii), T(st.jj), T(st.kk))
    want = O.fastba_reproject(st.poses, st.patches, st.intrinsics[0], st.ii, st.jj, st.kk, dtype=np.float64)
    assert np.abs(fr[0].cpu().numpy() - want).max() < 1e-3


# ---------------------------------------------------------------------------------------------------
# patch-graph index: bit-exact
# ---------------------------------------------------------------------------------------------------

def _check_graph(kk, jj, k_range):
    g = ops.GraphIndex(torch.device(DEV), E_cap=len(kk), k_range=k_range)
    g.build(T(jj), T(kk))
    kx, ku = g.unique()
    kx_o, ku_o = O.unique(kk)
    assert np.array_equal(kx.cpu().numpy(), kx_o)
    assert np.array_equal(ku.cpu().numpy(), ku_o)
    ix, jx = g.neighbors()
    ix_o, jx_o = O.neighbors(kk, jj)
    assert np.array_equal(ix.cpu().numpy(), ix_o)
    assert np.array_equal(jx.cpu().numpy(), jx_o)
    m = g.meta()
    assert m[0] == len(kx_o) and m[7] == len(kk)
    # a rebuild on the same workspace (stale histogram range re-zeroed in-kernel) gives the same answer
    g.build(T(jj), T(kk), force=True)
    ix2, jx2 = g.neighbors()
    assert torch.equal(ix, ix2) and torch.equal(jx, jx2)
    kx2, ku2 = g.unique()
    assert torch.equal(kx, kx2) and torch.equal(ku, ku2)


@pytest.mark.parametrize("name", ["tiny", "small", "pr1", "default", "stress"])
def test_graph_index_bit_exact(name):
    cfg = synth.CONFIGS[name]
    ii, jj, kk = synth.replay_edges(cfg)
    _check_graph(kk, jj, cfg.buffer_size * cfg.M)


def test_graph_index_irregular():
    """random multigraph: duplicate (k, j) edges, gaps in the id ranges, shuffled order"""
    rng = np.random.default_rng(11)
    E = 20000
    kk = rng.choice(np.arange(100, 9000, 3), size=E).astype(np.int64)
    jj = rng.integers(5, 300, size=E).astype(np.int64)
    _check_graph(kk, jj, 9000)
    # single edge / single patch
    _check_graph(np.array([7], np.int64), np.array([3], np.int64), 64)
    _check_graph(np.full(500, 42, np.int64), rng.integers(0, 20, 500).astype(np.int64), 64)
    # one workspace re-used for graphs with different id ranges (shrinking and growing)
    g = ops.GraphIndex(torch.device(DEV), E_cap=4096, k_range=5000)
    for lo, hi, E in ((100, 4000, 3000), (2000, 2100, 500), (0, 4999, 4096), (4500, 4600, 50)):
        kk = rng.integers(lo, hi, E).astype(np.int64)
        jj = rng.integers(0, 40, E).astype(np.int64)
        g.build(T(jj), T(kk))
        ix, jx = g.neighbors()
        ix_o, jx_o = O.neighbors(kk, jj)
        assert np.array_equal(ix.cpu().numpy(), ix_o) and np.array_equal(jx.cpu().numpy(), jx_o)
        kx, ku = g.unique()
        kx_o, ku_o = O.unique(kk)
        assert np.array_equal(kx.cpu().numpy(), kx_o) and np.array_equal(ku.cpu().numpy(), ku_o)


def test_graph_index_wrapping_ids_and_many_edges():
    """the histogram is indexed by id mod R: id ranges that straddle a multiple of the workspace capacity R (a patch
    ring that has wrapped many times), and more edges than one pass of the per-edge grids (1024 workgroups x 256)"""
    rng = np.random.default_rng(21)
    R = 6144
    for lo, span in ((7 * R + R - 50, 250), (123 * R - 3000, 6000), (5 * R, R)):
        kk = rng.integers(lo, lo + span, 30000).astype(np.int64)
        jj = rng.integers(0, 36, 30000).astype(np.int64)
        _check_graph(kk, jj, R)
    E = 300000
    kk = rng.integers(10 * R + 100, 10 * R + 100 + 5000, E).astype(np.int64)
    jj = rng.integers(0, 64, E).astype(np.int64)
    _check_graph(kk, jj, R)
    # a WIDE build (more than 200 k edges: one atomic per distinct id of a wave, the histogram's scan on 64 workgroups) over an id
    # range like a global bundle adjustment's frame-pair keys -- 90 k bins, ids without runs, the range wrapping around R
    R2 = 100000
    kk = rng.integers(3 * R2 - 40000, 3 * R2 + 50000, 250000).astype(np.int64)
    jj = rng.integers(0, 300, 250000).astype(np.int64)
    _check_graph(kk, jj, R2)


def test_graph_range_overflow_is_reported():
    g = ops.GraphIndex(torch.device(DEV), E_cap=16, k_range=8)
    os.environ["CDV_CHECK"] = "0"
    try:
        g.build(T(np.array([0, 100, 5], np.int64)), T(np.array([0, 100, 5], np.int64)))
        with pytest.raises(Exception):
            g.meta()
        # and the workspace recovers on the next in-range build
        g.build(T(np.array([3, 1, 2], np.int64)), T(np.array([4, 4, 6], np.int64)))
        assert g.meta()[0] == 2
    finally:
        os.environ["CDV_CHECK"] = "1"


def test_neighbors_dropin_signature():
    import cdv_slam_amd
    _, cuda_ba, _ = cdv_slam_amd.install_dropin()
    st = synth.make_state("small", features=False)
    ix, jx = cuda_ba.neighbors(T(st.kk), T(st.jj))
    ix_o, jx_o = O.neighbors(st.kk, st.jj)
    assert ix.dtype == torch.int64 and ix.is_cuda
    assert np.array_equal(ix.cpu().numpy(), ix_o) and np.array_equal(jx.cpu().numpy(), jx_o)


# ---------------------------------------------------------------------------------------------------
# altcorr
# ---------------------------------------------------------------------------------------------------

def _corr_tol(truth):
    return 2.0 ** -8 * np.abs(truth).max() + 2.0 ** -10


def _gpu_coords(st):
    return ops.transform(T(st.poses)[None], T(st.patches)[None], T(st.intrinsics)[None], T(st.ii), T(st.jj),
                         T(st.kk), layout_e2pp=True)


@pytest.mark.parametrize("name", ["tiny", "small", "default", "stress", "tartan", "euroc"])
def test_corr_fused_vs_oracle(name):
    """the fused two-level correlation against the float64 oracle -- on the benchmark workload too (default: E = 47,712,
    stress: E = 97,412), both as a direct call (planar tiles) and as the launch bench.py times: UpdatePath.step() with
    pixel-major tiles, the prologue's coordinates and the XCD dealing of the edge list"""
    from cdv_slam_amd.update import UpdatePath
    st = synth.make_state(name)
    up = UpdatePath(st, torch.device(DEV))
    big = st.E > 20000
    # the channels-last rings hold exactly the reference-layout maps
    assert torch.equal(ops.fmap_interior(up.fmap1).permute(0, 3, 1, 2).cpu(), torch.as_tensor(st.fmap1))
    # the zero margins stay zero (every element outside the interior, exactly)
    margin = up.fmap1.clone()
    ops.fmap_interior(margin).zero_()
    assert not margin.any()
    f2 = ops.fmap_interior(up.fmap2).permute(0, 3, 1, 2).float().cpu().numpy()
    assert np.abs(f2 - st.fmap2.astype(np.float32)).max() <= 2.0 ** -11 * np.abs(f2).max() + 1e-7
    coords = _gpu_coords(st)
    import ctypes
    perm = torch.randperm(st.E, device=DEV).to(torch.int32)
    fmap2 = ops.fmap_interior(up.fmap2).permute(0, 3, 1, 2).contiguous().cpu().numpy()  # what the kernel reads
    c = coords[0].cpu().numpy()
    truth = O.slam_corr(st.gmap, st.fmap1, fmap2, c, st.ii1, st.jj1, 3, "truth")
    tol = _corr_tol(truth)
    for order in (None, perm):
        optr = None if order is None else ctypes.c_void_p(order.data_ptr())
        out = ops.corr_fused(up.gmap, up.fmap1, up.fmap2, coords, up.kk, up.jj, kmod=up.kmod, jmod=up.jmod,
                             order_ptr=optr)
        got = out[0].float().cpu().numpy()
        assert got.shape == truth.shape == (st.E, 882)
        assert np.abs(got - truth).max() <= tol
        if not big:
            # and the reference-faithful half-precision emulation sits inside the same envelope
            ref = O.slam_corr(st.gmap, st.fmap1, fmap2, c, st.ii1, st.jj1, 3, "ref").astype(np.float64)
            assert np.abs(ref - truth).max() <= 4 * tol
            assert np.abs(got - ref).max() <= 4 * tol
    direct = out
    # the launch bench.py times
    res = up.step(iterations=0)
    torch.cuda.synchronize()
    assert torch.equal(res["coords"], coords)          # the prologue's reprojection is the same code
    got = res["corr"][0].float().cpu().numpy()
    assert np.abs(got - truth).max() <= tol
    assert torch.equal(res["corr"], direct)            # layouts, dealing and fusion change loads, not results
    # mean error well inside the bound: the bound is not met by luck at one element
    assert np.abs(got - truth).mean() <= 0.1 * tol


def test_corr_vs_reference_run_pin(golden_dir):
    """Rows a1 / a2 on the GPU against `corr_pin.npz` (the reference's own patchify blend executed in this repository's
    container, contracted with the patch features: tests/golden/make_golden.py corr-pin): cuda_corr.forward per level on
    half and on float32 maps, and the fused two-level launch of the update path on channels-last rings with pixel-major
    and planar tiles.  Half storage: |d| <= 2^-8 max|corr| + 2^-10; float32: 1e-5 relative."""
    _corr_vs_pin(np.load(os.path.join(golden_dir, "corr_pin.npz")), far=(8, 9))


def test_corr_vs_reference_run_pin_euroc():
    """the same against `corr_pin_euroc.npz`: 120x188 level-0 and 30x47 level-1 maps (the odd level-1 width of EuRoC's
    480x752 frames), edges on the right / bottom border of level 1 (x in {46, 46.5, 47.25, 49.75}) and wide footprints"""
    from tests import golden_util
    z = golden_util.load_corr_pin_euroc()
    assert z["fmap2"].shape[-2:] == (30, 47)
    _corr_vs_pin(z, far=())


def _corr_vs_pin(z, far):
    E = len(z["ii"])
    gmap, f1, f2 = T(z["gmap"]), T(z["fmap1"]), T(z["fmap2"])
    coords, ii, jj = T(z["coords"])[None], T(z["ii"]), T(z["jj"])
    saved, ops._pairing = ops._pairing, ops._LevelPairing()
    try:
        for lvl, (fm, s) in enumerate(((f1, 1.0), (f2, 4.0))):
            want = z["corr%d" % lvl]
            top = np.abs(want).max()
            got = ops.corr_forward(gmap[None], fm[None], coords / s, ii, jj, 3)
            assert got.dtype == torch.float16 and tuple(got.shape) == (1, E, 7, 7, 3, 3)
            assert np.abs(got[0].float().cpu().numpy() - want).max() <= 2.0 ** -8 * top + 2.0 ** -10
            got32 = ops.corr_forward(gmap[None].float(), fm[None].float(), coords / s, ii, jj, 3)
            assert got32.dtype == torch.float32
            assert np.abs(got32[0].cpu().numpy() - want).max() <= 1e-5 * top
            assert all(not got[0, e].any() for e in far)                # far outside the map
    finally:
        ops._pairing = saved
    mem, C, H, W = z["fmap1"].shape
    r1, r2 = ops.alloc_fmap_ring(mem, C, H, W, DEV), ops.alloc_fmap_ring(mem, C, H // 4, W // 4, DEV)
    ops.fmap_interior(r1).copy_(f1.permute(0, 2, 3, 1))
    ops.fmap_interior(r2).copy_(f2.permute(0, 2, 3, 1))       # the fixture's own level-1 map (torch's pooling, slam.py:682)
    want = np.stack([z["corr0"], z["corr1"]], -1).reshape(E, -1)
    tol = _corr_tol(want)
    for tiles, pm in ((gmap, False), (ops.gmap_to_pixel_major(gmap), True)):
        out = ops.corr_fused(tiles, r1, r2, coords, ii, jj, pixel_major=pm)
        assert np.abs(out[0].float().cpu().numpy() - want).max() <= tol
        assert np.abs(out[0].float().cpu().numpy() - want).mean() <= 0.1 * tol


def test_corr_processing_order_beyond_one_trip():
    """the same order on a graph whose per-edge launches loop (E = 705,024 > 1,024 workgroups x 256 edges): still a
    permutation grouped by target bin"""
    import ctypes
    st = synth.make_state("global_xl", features=False)
    g = ops.GraphIndex(torch.device(DEV), E_cap=st.E, k_range=len(st.patches))
    g.build(T(st.jj), T(st.kk), force=True, with_neighbors=True, ii=T(st.ii))
    torch.cuda.synchronize()
    order = torch.empty(st.E, dtype=torch.int32, device=DEV)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(ctypes.c_void_p(order.data_ptr()), g.corr_order_ptr(), 4 * st.E, 3) == 0
    o = order.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(o), np.arange(st.E))
    assert (np.diff(st.jj[o] & 31) >= 0).all()


def test_dropin_corr_pairs_the_two_level_calls():
    """cuda_corr.forward called the way slam.py:321-322 calls it (pyramid[0] with coords, pyramid[1] with coords / 4): from
    the second update on the first call computes both levels and the second only checks its coords on the device
    (ops._LevelPairing).  Results equal the unpaired calls bit for bit -- also when the second call's coords are NOT the
    first's divided by four for some edges (those are recomputed)."""
    st = synth.make_state("small")
    dev = torch.device(DEV)
    gmap = torch.as_tensor(st.gmap, device=dev)[None].contiguous()             # [1, Ng, C, 3, 3]
    f1 = torch.as_tensor(st.fmap1, device=dev)[None].contiguous()              # [1, mem, C, H, W]
    f2 = torch.as_tensor(st.fmap2, device=dev)[None].contiguous()
    ii1 = torch.as_tensor(st.kk % (st.cfg.M * st.cfg.pmem), device=dev)
    jj1 = torch.as_tensor(st.jj % st.cfg.mem, device=dev)
    rng = np.random.default_rng(5)
    h, w = f1.shape[-2], f1.shape[-1]
    base = torch.as_tensor(np.stack([rng.uniform(4, w - 4, (st.E, 3, 3)), rng.uniform(4, h - 4, (st.E, 3, 3))], 1)[None]
                           .astype(np.float32), device=dev)

    def plain(ring, c, ii=None, jj=None):      # an unpaired call: a fresh pairing state sees one call only
        saved, ops._pairing = ops._pairing, ops._LevelPairing()
        try:
            return ops.corr_forward(gmap, ring, c, ii1 if ii is None else ii, jj1 if jj is None else jj, 3).clone()
        finally:
            ops._pairing = saved

    ops._pairing = ops._LevelPairing()
    for it in range(3):
        coords = base + 0.37 * it
        c0, c1 = coords / 1, coords / 4
        if it == 2:          # a caller that does something else on some edges
            c1 = c1.clone()
            c1[0, ::7] += 0.125
        a = ops.corr_forward(gmap, f1, c0, ii1, jj1, 3)
        b = ops.corr_forward(gmap, f2, c1, ii1, jj1, 3)
        stacked = torch.stack([a, b], -1).view(1, st.E, -1)
        assert torch.equal(a, plain(f1, c0)), it
        assert torch.equal(b, plain(f2, c1)), it
        assert stacked.shape[-1] == 882 and type(stacked) is torch.Tensor
        assert torch.equal(stacked, torch.stack([plain(f1, c0), plain(f2, c1)], -1).view(1, st.E, -1)), it
        if it > 0:      # the two views of one buffer: the stack IS that buffer (no copy), any other stack is a real one
            assert stacked.data_ptr() == a.data_ptr() and isinstance(a, ops.PairedLevel)
            assert torch.stack([b, a], -1).data_ptr() != a.data_ptr() and torch.stack([a, b], 0).shape[0] == 2
            assert torch.equal(torch.stack([a, b], 0)[1], b) and type(a + 0) is torch.Tensor
    assert ops._pairing.n_fused == 2 and ops._pairing.n_stacked == 2      # updates 1 and 2; update 0 taught the pattern
    # a third caller between the two calls of a pair: the speculative level is dropped, nothing is mis-paired
    other = base[:, : st.E // 2].contiguous() + 1.5
    io, jo = ii1[: st.E // 2].contiguous(), jj1[: st.E // 2].contiguous()
    coords = base + 2.11
    a = ops.corr_forward(gmap, f1, coords / 1, ii1, jj1, 3)
    x = ops.corr_forward(gmap, f2, other / 4, io, jo, 3)              # somebody else, other tensors, the partner ring
    b = ops.corr_forward(gmap, f2, coords / 4, ii1, jj1, 3)
    assert ops._pairing.n_fused == 2
    assert torch.equal(a, plain(f1, coords / 1)) and torch.equal(b, plain(f2, coords / 4)) and torch.equal(x, plain(f2, other / 4, io, jo))
    # index tensors modified in place between the two calls (same objects, same addresses): not served from the pair
    jj_mut = jj1.clone()
    a = ops.corr_forward(gmap, f1, coords / 1, ii1, jj_mut, 3)
    jj_mut[::3] = (jj_mut[::3] + 1) % st.cfg.mem
    b = ops.corr_forward(gmap, f2, coords / 4, ii1, jj_mut, 3)
    assert ops._pairing.n_fused == 2 and torch.equal(b, ops.corr_forward(gmap, f2, coords / 4, ii1, jj_mut.clone(), 3))
    # the documented switch: CDV_PAIR_LEVELS=0 computes every call on its own
    os.environ["CDV_PAIR_LEVELS"] = "0"
    try:
        n0 = ops._pairing.n_fused
        for it in range(2):
            a = ops.corr_forward(gmap, f1, coords / 1, ii1, jj1, 3)
            b = ops.corr_forward(gmap, f2, coords / 4, ii1, jj1, 3)
        assert ops._pairing.n_fused == n0 and ops._pairing.pending is None
    finally:
        del os.environ["CDV_PAIR_LEVELS"]
    ops._pairing = ops._LevelPairing()


def test_ba_rebuilds_the_index_when_only_ii_changes():
    """the per-patch edge records carry the source frames (the N <= 32 kernels read them instead of ii): a second BA on
    the SAME jj / kk tensors with another ii, or with ii modified in place, must not reuse the index built for the first"""
    st = synth.make_state("small", features=False)
    dev = torch.device(DEV)
    jj, kk = T(st.jj), T(st.kk)
    g = ops.GraphIndex(dev, E_cap=st.E, k_range=st.cfg.buffer_size * st.cfg.M)
    ii_a = T(st.ii)
    ii_b = ii_a.clone()
    sel = torch.arange(0, st.E, 5, device=dev)
    ii_b[sel] = torch.clamp(ii_b[sel] - 1, min=0)                  # some edges claim another source frame

    def run(ii, graph):
        poses, patches = T(st.poses).clone(), T(st.patches).clone()
        ops.ba_forward(poses, patches, T(st.intrinsics), T(st.target), T(st.weight), torch.tensor([st.lmbda], device=dev), ii,
                       jj, kk, st.cfg.M, st.t0, st.n, 2, False, graph=graph)
        torch.cuda.synchronize()
        return poses.cpu().numpy()

    fresh = lambda: ops.GraphIndex(dev, E_cap=st.E, k_range=st.cfg.buffer_size * st.cfg.M)
    want_a, want_b = run(ii_a, fresh()), run(ii_b, fresh())
    # (a patch with two source frames sums part of its E column with LDS atomics: ii_b's result is reproducible to
    # rounding, not bit for bit -- hence a tolerance far below the difference between the two)
    same = lambda x, y: np.abs(x - y).max() < 1e-6
    assert np.abs(want_a - want_b).max() > 1e-4
    assert np.array_equal(run(ii_a, g), want_a)
    assert same(run(ii_b, g), want_b)                              # same jj / kk objects, another ii
    ii_c = ii_a.clone()
    assert np.array_equal(run(ii_c, g), want_a)
    ii_c.copy_(ii_b)                                               # modified in place: the version counter moved
    assert same(run(ii_c, g), want_b)
    # an index built without ii (neighbors) serves a BA that brings ii: nothing of ii is baked in, the kernels read it per edge
    g.build(jj, kk, force=True)
    assert same(run(ii_b, g), want_b)


@pytest.mark.parametrize("name", ["small", "default"])
def test_corr_processing_order_from_the_index_build(name):
    """the edge order the fused correlation works through (cdv_graph_corr_order, a counting sort by target frame riding
    the index build): a permutation of the edges, grouped by jj mod 32; the correlation output does not depend on it"""
    from cdv_slam_amd.update import UpdatePath
    st = synth.make_state(name, buffer_size=64 if name == "default" else None) if name == "default" else synth.make_state(name)
    up = UpdatePath(st, torch.device(DEV), sorted_corr=True)
    res = up.step(iterations=0)
    torch.cuda.synchronize()
    ptr = up.graph.corr_order_ptr()
    assert ptr is not None
    order = torch.empty(st.E, dtype=torch.int32, device=DEV)
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(ctypes.c_void_p(order.data_ptr()), ptr, 4 * st.E, 3) == 0     # device to device
    o = order.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(o), np.arange(st.E))
    bins = (st.jj[o] & 31)
    # grouped: the bin sequence along the order is non-decreasing
    assert (np.diff(bins) >= 0).all()
    sorted_out = res["corr"].clone()
    up2 = UpdatePath(st, torch.device(DEV), sorted_corr=False)
    res2 = up2.step(iterations=0)
    assert torch.equal(sorted_out, res2["corr"])



def test_reference_call_sequence_through_the_dropin_names():
    """The reference's own sequence for one update -- SLAM.reproject / SLAM.corr (slam.py:316-329), the ring writes
    (slam.py:679-682), Update's fastba.neighbors (net_cdv.py:102), fastba.BA (slam.py:512-515, fastba/ba.py:8) -- written
    against the module names it imports (cuda_corr, cuda_ba, lietorch_backends, registered by install_dropin()) and the
    reference's state layouts (cdv_slam_amd.update.DropinPath), on the benchmark workload; equal to UpdatePath.step():
    coordinates, correlation and neighbors bit for bit, the state after the bundle adjustment to the last bits (nothing on
    the path sums in an order that depends on timing)."""
    _dropin_call_sequence("default")


def test_reference_call_sequence_through_the_dropin_names_euroc():
    """the same at `euroc`: the NHWC shadows of 120x188 / 30x47 maps, the 1000-frame patch ring, the EuRoC intrinsics"""
    _dropin_call_sequence("euroc")


def _dropin_call_sequence(name):
    from cdv_slam_amd.update import DropinPath, UpdatePath
    st = synth.make_state(name)
    dev = torch.device(DEV)
    up = UpdatePath(st, dev)
    want = up.step()
    dp = DropinPath(st, dev)
    level1 = lambda: ops.fmap_interior(up.fmap2).permute(0, 3, 1, 2).contiguous()   # the 4x4 averages as the ingest rounds them
    assert float((dp.fmap2_[0].float() - level1().float()).abs().max()) <= 2.0 ** -10  # torch's pooling: same up to f16 rounding
    dp.fmap2_.copy_(level1()[None])
    got = dp.step(pooled=level1()[up.new_slot])
    torch.cuda.synchronize()
    assert got["ba"] == []
    assert torch.equal(got["coords"], want["coords"])
    assert got["corr"].shape == want["corr"].shape and torch.equal(got["corr"], want["corr"])
    assert torch.equal(got["ix"], want["ix"]) and torch.equal(got["jx"], want["jx"])
    # the bundle adjustment: the same sums in the same order, but through other instantiations of the kernels (the drop-in's
    # index carries no source frames, its workspace is sized for every patch of the buffer and so takes the four-launch
    # sequence): equal up to the compiler's multiply-add contractions
    same_state = lambda: (float((dp.poses_ - up.poses).abs().max()) < 1e-6 and float((dp.patches_.view_as(up.patches) - up.patches).abs().max()) < 1e-5)
    assert same_state()
    assert not torch.equal(dp.poses_, T(st.poses))
    # a second frame: only the ring slot that was written is converted again (fingerprint-gated shadow sync)
    before = ops._nhwc.converted_slots(dp.fmap1_)
    assert before == st.cfg.mem                       # the first sync converted every slot
    dp.new_frame = (dp.new_frame.float() * 0.5 + 0.125).half()
    up.new_frame = dp.new_frame.clone()
    want = up.step()
    got = dp.step(pooled=level1()[up.new_slot])
    torch.cuda.synchronize()
    assert ops._nhwc.converted_slots(dp.fmap1_) == before + 1
    assert torch.equal(got["coords"], want["coords"]) or float((got["coords"] - want["coords"]).abs().max()) < 1e-4
    assert float((got["corr"].float() - want["corr"].float()).abs().max()) <= 2.0 ** -8 * float(want["corr"].float().abs().max()) + 2.0 ** -10
    assert same_state()


def test_dropin_fast_path_under_the_unchanged_caller():
    """What the round-3 review found missing: the reference's SLAM object hands over a FRESH view of gmap_ at every access
    (slam.py:249-251; SLAM.corr reads it twice, :321-322), fresh views of poses / patches / intrinsics, NEW edge tensors
    every frame (torch.cat, slam.py:331-337), and calls the extension through an autograd.Function under autocast
    (altcorr/correlation.py:4-13, slam.py:486).  DropinPath now does all of that; the caches are keyed on memory + version,
    not on Python identity.  Per update, from the second on: the two per-level calls are served by ONE fused launch
    (n_fused + 1), the stack of the two results is the shared buffer (n_stacked + 1), the tile shadow is converted exactly
    once, the patch-graph index is built exactly once (neighbors + BA share it), and everything equals UpdatePath.step()
    from the same state: coordinates, correlation, neighbors bit for bit, the state after the BA to rounding."""
    from cdv_slam_amd.update import DropinPath, UpdatePath
    st = synth.make_state("default")
    dev = torch.device(DEV)
    up = UpdatePath(st, dev)
    dp = DropinPath(st, dev)
    assert dp.gmap is not dp.gmap and dp.poses is not dp.poses and dp.patches is not dp.patches     # property-style views
    level1 = lambda: ops.fmap_interior(up.fmap2).permute(0, 3, 1, 2).contiguous()
    dp.fmap2_.copy_(level1()[None])
    ops._pairing, ops._tiles = ops._LevelPairing(), ops.TileCache()
    g = ops._device_graph(dev)
    for it in range(4):
        # a new frame every step: other features, other tiles
        up.new_frame = (up.new_frame.float() * 0.75 + 0.03125 * it).half()
        dp.new_frame = up.new_frame.clone()
        tiles = (dp.new_tiles.float() * 0.5 + 0.0625 * it).half()
        dp.new_tiles = tiles
        up.gmap[up.new_tiles:up.new_tiles + up.M] = tiles
        dp.poses_.copy_(up.poses)                      # both paths start the step from the same state
        dp.patches_.copy_(up.patches.view_as(dp.patches_))
        want = up.step()
        f0, s0, c0, b0 = ops._pairing.n_fused, ops._pairing.n_stacked, ops._tiles.n_converted, g.n_builds
        old = (dp.ii, dp.jj, dp.kk)
        got = dp.step(pooled=level1()[up.new_slot])
        torch.cuda.synchronize()
        assert dp.ii is not old[0] and dp.jj is not old[1] and dp.kk is not old[2]      # fresh edge tensors, as torch.cat leaves
        assert dp.ii.data_ptr() != old[0].data_ptr() and torch.equal(dp.ii, old[0])
        if it > 0:      # step 0 taught the pairing
            assert ops._pairing.n_fused == f0 + 1 and ops._pairing.n_stacked == s0 + 1, it
            assert ops._tiles.n_converted == c0 + 1, it
        assert g.n_builds == b0 + 1, it
        assert type(got["corr"]) is torch.Tensor and got["corr"].shape == want["corr"].shape
        assert torch.equal(got["coords"], want["coords"]), it
        assert torch.equal(got["corr"], want["corr"]), it
        assert torch.equal(got["ix"], want["ix"]) and torch.equal(got["jx"], want["jx"]), it
        assert float((dp.poses_ - up.poses).abs().max()) < 1e-6, it
        assert float((dp.patches_.view_as(up.patches) - up.patches).abs().max()) < 1e-5, it
    # the same tensors once more, nothing written in between: the index is not rebuilt, the tiles not reconverted
    b0, c0 = g.n_builds, ops._tiles.n_converted
    dp.step(ingest=False)
    assert g.n_builds == b0 and ops._tiles.n_converted == c0
    # gmap_ written through ANOTHER view between the two calls of a pair: the second call must not be served from the pair
    coords = dp.reproject()
    ii1, jj1 = dp.kk % (dp.M * dp.pmem), dp.jj % dp.mem
    f0 = ops._pairing.n_fused
    a, = dp.cuda_corr.forward(dp.gmap, dp.pyramid[0], coords / 1, ii1, jj1, 3)
    dp.gmap_[3] = dp.gmap_[4]
    b, = dp.cuda_corr.forward(dp.gmap, dp.pyramid[1], coords / 4, ii1, jj1, 3)
    assert ops._pairing.n_fused == f0 and not isinstance(b, ops.PairedLevel)
    saved, ops._pairing = ops._pairing, ops._LevelPairing()
    try:
        assert torch.equal(b, ops.corr_forward(dp.gmap, dp.pyramid[1], coords / 4, ii1, jj1, 3))
    finally:
        ops._pairing = saved
    ops._pairing, ops._tiles = ops._LevelPairing(), ops.TileCache()


def test_shadows_sync_equals_the_single_ring_calls():
    """cdv_shadows_sync (both pyramid levels' shadows and the tile shadow brought in step in two launches) against
    2 x cdv_fmap_sync_nhwc + cdv_gmap_to_pixel_major on the same planar rings: the same shadows byte for byte, the same slots
    converted (first sync: all; then only the slots somebody wrote), for two rings, one ring, tiles only."""
    import ctypes
    from cdv_slam_amd import _lib
    lib = _lib.load()
    dev = torch.device(DEV)
    g = torch.Generator(device="cpu").manual_seed(11)
    mem, C, H, W, Ng = 12, 24, 32, 48, 300
    ra = torch.randn((1, mem, C, H, W), generator=g).half().to(dev)
    rb = torch.randn((1, mem, C, H // 4, W // 4), generator=g).half().to(dev)
    tiles = torch.randn((Ng, C, 3, 3), generator=g).half().to(dev)
    stream = ops._stream()

    def fresh(r):
        return {"shadow": torch.zeros((mem, r.shape[3] + 2 * ops.FMAP_PADY, r.shape[4] + 2 * ops.FMAP_PADX, C), dtype=torch.float16, device=dev),
                "ws": torch.zeros(lib.cdv_fmap_sync_workspace_bytes(mem), dtype=torch.uint8, device=dev), "parity": 0}

    def single(r, e):
        _lib.check(lib.cdv_fmap_sync_nhwc(r.data_ptr(), e["shadow"].data_ptr(), mem, C, r.shape[3], r.shape[4], e["ws"].data_ptr(),
                                          e["parity"], stream), "cdv_fmap_sync_nhwc")
        e["parity"] ^= 1

    def fused(pairs, tiles_in, pm):
        jobs = (_lib.ShadowRing * 2)()
        for q, (r, e) in enumerate(pairs):
            jobs[q] = _lib.ShadowRing(r.data_ptr(), e["shadow"].data_ptr(), e["ws"].data_ptr(), mem, C, r.shape[3], r.shape[4], e["parity"])
        _lib.check(lib.cdv_shadows_sync(ctypes.cast(jobs, ctypes.c_void_p), len(pairs), None if tiles_in is None else tiles_in.data_ptr(),
                                        None if pm is None else pm.data_ptr(), Ng, C, stream), "cdv_shadows_sync")
        for _, e in pairs:
            e["parity"] ^= 1

    dirty = lambda e: int(e["ws"][-64:-60].view(torch.int32).item())
    sa, sb, fa, fb = fresh(ra), fresh(rb), fresh(ra), fresh(rb)
    pm_f = torch.zeros((Ng, 9, C), dtype=torch.float16, device=dev)
    for step in range(4):
        if step == 1:                      # one slot of each ring written, as a frame does; tiles too
            ra[0, 5] += 0.5; rb[0, 5] -= 0.25; tiles[17] *= 2
        if step == 2:                      # nothing written
            pass
        if step == 3:                      # two slots of A, none of B
            ra[0, 0, 3, 2, 1] += 1.0; ra[0, 11] *= 0.5
        single(ra, sa); single(rb, sb)
        pm_s = ops.gmap_to_pixel_major(tiles)
        fused([(ra, fa), (rb, fb)], tiles, pm_f)
        torch.cuda.synchronize()
        assert torch.equal(sa["shadow"], fa["shadow"]) and torch.equal(sb["shadow"], fb["shadow"]) and torch.equal(pm_s, pm_f), step
        assert dirty(sa) == dirty(fa) == (mem, mem + 1, mem + 1, mem + 3)[step] and dirty(sb) == dirty(fb) == (mem, mem + 1, mem + 1, mem + 1)[step]
    # one ring only / tiles only / nothing at all
    rb[0, 2] += 1.0
    single(rb, sb); fused([(rb, fb)], None, None)
    tiles[3] += 1.0
    pm_f2 = pm_f.clone()
    fused([], tiles, pm_f2)
    fused([], None, None)
    torch.cuda.synchronize()
    assert torch.equal(sb["shadow"], fb["shadow"]) and dirty(fb) == mem + 2 and torch.equal(pm_f2, ops.gmap_to_pixel_major(tiles))
    assert lib.cdv_shadows_sync(None, 3, None, None, 0, C, stream) == -2


def test_dropin_compiled_bookkeeping_equals_the_python_bookkeeping():
    """The steady state of the drop-in modules runs compiled (csrc/dropin_fast.cpp, armed by ops.py after it has served a
    complete pair and a complete neighbors + BA itself).  The same updates with the lane on and off (CDV_DROPIN_FAST) from
    the same state: correlation, coordinates and neighbors bit for bit, the state after the bundle adjustment bit for bit
    (the same launches with the same arguments).  The lane is really the one that runs: armed after the second update, the
    counters the Python side keeps (pairs served, tiles converted, index builds) move as they do without it; what it does
    not recognise it hands back -- rings written through a batch view, another E, a call in between -- and is armed again
    by the next complete update."""
    from cdv_slam_amd.update import DropinPath
    st = synth.make_state("default")
    dev = torch.device(DEV)
    assert ops.fast_lane_enabled()

    def run(fast, n=5):
        os.environ["CDV_DROPIN_FAST"] = "1" if fast else "0"
        ops._disarm_pair(); ops._disarm_graph()
        ops._pairing, ops._tiles, ops._nhwc = ops._LevelPairing(), ops.TileCache(), ops.NhwcCache()
        dp = DropinPath(st, dev)
        g = ops._device_graph(dev)
        outs, used = [], []
        for it in range(n):
            dp.new_frame = (dp.new_frame.float() * 0.75 + 0.03125 * it).half()
            dp.new_tiles = (dp.new_tiles.float() * 0.5 + 0.0625 * it).half()
            c0, b0, f0 = ops._tiles.n_converted, g.n_builds, ops._pairing.n_fused
            o = dp.step()
            torch.cuda.synchronize()
            paired = 1 if it > 0 else 0          # update 0: two ordinary calls on planar tiles, which teach the pairing
            assert ops._tiles.n_converted == c0 + paired and g.n_builds == b0 + 1 and ops._pairing.n_fused == f0 + paired, it
            outs.append([o["corr"].clone(), o["coords"].clone(), o["ix"].clone(), o["jx"].clone(), dp.poses_.clone(), dp.patches_.clone()])
            used.append((ops._armed_pair is not None, ops._armed_graph is not None))
        return dp, outs, used

    try:
        _, want, used0 = run(False)
        assert not any(a or b for a, b in used0)
        dp, got, used1 = run(True)
        assert used1[0] == (False, True) and all(u == (True, True) for u in used1[1:])     # update 0 taught the pairing
        for it, (w, g_) in enumerate(zip(want, got)):
            for a, b in zip(w, g_):
                assert torch.equal(a, b), it
        # ---- what the lane does not recognise goes back to Python, which serves it and arms the lane again
        g = ops._device_graph(dev)
        # (a) shorter edge lists: another E is fine for the lane (buffers are per call) -- still armed, same results as Python
        keep = dp.ii.numel() - 96
        dp.ii, dp.jj, dp.kk = dp.ii[:keep].clone(), dp.jj[:keep].clone(), dp.kk[:keep].clone()
        dp.target, dp.weight = dp.target[:, :keep].contiguous(), dp.weight[:, :keep].contiguous()
        dp.n_new = min(dp.n_new, keep // 2)
        o = dp.step()
        assert ops._armed_pair is not None and ops._armed_graph is not None and o["corr"].shape[1] == keep
        # (b) the level-0 ring written through ANOTHER tensor on the same memory: the version counter moves, the lane re-syncs
        before = ops._nhwc.converted_slots(dp.fmap1_)
        dp.fmap1_.view(-1)[:8] += 1.0
        dp.step(ingest=False)
        assert ops._armed_pair is not None and ops._nhwc.converted_slots(dp.fmap1_) == before + 1
        # (c) a float32 BA state is not the lane's: Python serves (and raises what it raises)
        with pytest.raises(TypeError):
            ops.ba_forward(dp.poses.data.double(), dp.patches, dp.intrinsics, dp.target, dp.weight, torch.as_tensor([1e-4], device=dev),
                           dp.ii, dp.jj, dp.kk, dp.M, dp.t0, dp.n, 2)
        assert ops._armed_graph is None              # the Python path took the workspace back ...
        dp.step()
        assert ops._armed_graph is not None          # ... and the next complete update hands it over again
        # (d) the documented switch, read at every call
        os.environ["CDV_DROPIN_FAST"] = "0"
        b0 = g.n_builds
        o2 = dp.step(ingest=False)
        assert ops._armed_pair is None and ops._armed_graph is None and g.n_builds == b0      # same tensors: the index is kept
        os.environ["CDV_DROPIN_FAST"] = "1"
        dp.reset()
        a = dp.step(ingest=False)
        dp.reset()
        os.environ["CDV_DROPIN_FAST"] = "0"
        b = dp.step(ingest=False)
        assert torch.equal(a["corr"], b["corr"]) and torch.equal(a["ix"], b["ix"])
    finally:
        os.environ.pop("CDV_DROPIN_FAST", None)
        ops._disarm_pair(); ops._disarm_graph()
        ops._pairing, ops._tiles, ops._nhwc = ops._LevelPairing(), ops.TileCache(), ops.NhwcCache()


def test_dropin_compiled_bookkeeping_randomised_against_the_python_bookkeeping():
    """A seeded random walk of what a caller can do between and inside updates -- plain updates, updates without a new
    frame, a ring slot or the tiles written through another view, edge lists that shrink and grow, neighbors asked twice, a
    BA with another iteration count, a third caller's correlation between the two calls of a pair, the pairing switched off
    for an update, another path's bundle adjustment on the shared workspace -- run once with the compiled lane and once with
    the Python bookkeeping: every output of every step bit for bit the same, and the lane is the one that ran most steps."""
    from cdv_slam_amd.update import DropinPath, UpdatePath
    st = synth.make_state("small")
    dev = torch.device(DEV)
    other = UpdatePath(st, dev)                      # another path: its own index, the SHARED per-device BA workspace

    def walk(fast, steps=70):
        os.environ["CDV_DROPIN_FAST"] = "1" if fast else "0"
        ops._disarm_pair(); ops._disarm_graph()
        ops._pairing, ops._tiles, ops._nhwc = ops._LevelPairing(), ops.TileCache(), ops.NhwcCache()
        rng = np.random.default_rng(77)
        dp = DropinPath(st, dev)
        full = (dp.ii.clone(), dp.jj.clone(), dp.kk.clone(), dp.target.clone(), dp.weight.clone())
        outs, armed = [], 0
        for it in range(steps):
            act = int(rng.integers(0, 10)) if it >= 3 else 0
            dp.reset()
            if act == 1:                             # a ring slot and a tile written through other views of the same memory
                dp.fmap1_.view(-1, dp.fmap1_.shape[-1])[int(rng.integers(0, 50))] += 0.25
                dp.gmap_.view(-1)[int(rng.integers(0, 1000))] += 0.5
            if act == 2:                             # other edge lists: a random prefix
                keep = int(rng.integers(full[0].numel() // 2, full[0].numel()))
                dp.ii, dp.jj, dp.kk = full[0][:keep].clone(), full[1][:keep].clone(), full[2][:keep].clone()
                dp.target, dp.weight = full[3][:, :keep].contiguous(), full[4][:, :keep].contiguous()
                dp.n_new = min(dp.n_new, keep // 2)
            if act == 3:                             # all of them again
                dp.ii, dp.jj, dp.kk, dp.target, dp.weight = (t.clone() for t in full)
            if act == 4:
                os.environ["CDV_PAIR_LEVELS"] = "0"
            if act == 5:                             # somebody else's bundle adjustment on the shared workspace
                other.step()
            if act == 6:                             # a third caller between the two calls of a pair
                coords = dp.reproject()
                ii1, jj1 = dp.kk % (dp.M * dp.pmem), dp.jj % dp.mem
                a, = dp.cuda_corr.forward(dp.gmap, dp.pyramid[0], coords / 1, ii1, jj1, 3)
                x, = dp.cuda_corr.forward(dp.gmap, dp.pyramid[0], coords[:, :64].contiguous() + 0.5, ii1[:64].contiguous(), jj1[:64].contiguous(), 3)
                b, = dp.cuda_corr.forward(dp.gmap, dp.pyramid[1], coords / 4, ii1, jj1, 3)
                outs.append([a.clone(), x.clone(), b.clone()])
            o = dp.step(ingest=act != 7, iterations=3 if act == 8 else 2)
            rec = [o["corr"].clone(), o["coords"].clone(), o["ix"].clone(), o["jx"].clone(), dp.poses_.clone(), dp.patches_.clone()]
            if act == 9:                             # neighbors asked again, of the same and of other tensors
                ix2, jx2 = dp.cuda_ba.neighbors(dp.kk, dp.jj)
                ix3, jx3 = dp.cuda_ba.neighbors(dp.kk.clone(), dp.jj.clone())
                rec += [ix2.clone(), jx2.clone(), ix3.clone(), jx3.clone()]
            os.environ.pop("CDV_PAIR_LEVELS", None)
            outs.append(rec)
            armed += int(ops._armed_pair is not None and ops._armed_graph is not None)
        torch.cuda.synchronize()
        return outs, armed

    try:
        want, a0 = walk(False)
        got, a1 = walk(True)
        assert a0 == 0 and a1 >= 35, (a0, a1)
        assert len(want) == len(got)
        for it, (w, g_) in enumerate(zip(want, got)):
            assert len(w) == len(g_)
            for q, (x, y) in enumerate(zip(w, g_)):
                assert x.shape == y.shape and torch.equal(x, y), (it, q)
    finally:
        os.environ.pop("CDV_DROPIN_FAST", None)
        os.environ.pop("CDV_PAIR_LEVELS", None)
        ops._disarm_pair(); ops._disarm_graph()
        ops._pairing, ops._tiles, ops._nhwc = ops._LevelPairing(), ops.TileCache(), ops.NhwcCache()


def test_corr_pixel_major_tiles_bit_identical():
    """the [Ng,9,C] operand layout (cdv_gmap_to_pixel_major / cdv_frame_ingest) changes loads, not results"""
    from cdv_slam_amd.update import UpdatePath
    st = synth.make_state("small")
    up = UpdatePath(st, torch.device(DEV))
    pm = ops.gmap_to_pixel_major(up.gmap)
    assert torch.equal(pm, up.gmap.reshape(up.gmap.shape[0], up.gmap.shape[1], 9).permute(0, 2, 1).contiguous())
    coords = _gpu_coords(st)
    a = ops.corr_fused(up.gmap, up.fmap1, up.fmap2, coords, up.kk, up.jj, kmod=up.kmod, jmod=up.jmod)
    b = ops.corr_fused(pm, up.fmap1, up.fmap2, coords, up.kk, up.jj, kmod=up.kmod, jmod=up.jmod, pixel_major=True)
    assert torch.equal(a, b)
    # the per-frame ingest converts exactly the new frame's tiles and nothing else
    pm2 = torch.full_like(pm, 7.0)
    ops.fmap_ingest(up.new_frame, up.fmap1, up.fmap2, up.new_slot, gmap=up.gmap, gmap_pm=pm2, gmap_first=up.new_tiles,
                    gmap_count=up.M)
    torch.cuda.synchronize()
    sl = slice(up.new_tiles, up.new_tiles + up.M)
    assert torch.equal(pm2[sl], pm[sl])
    rest = torch.ones(pm.shape[0], dtype=torch.bool)
    rest[sl] = False
    assert bool((pm2[rest.to(pm2.device)] == 7.0).all())


def test_update_prologue_equals_separate_launches():
    """cdv_update_prologue (ingest + reproject + index histogram in one launch, then the rest of the index build) gives
    bit-identical rings, tiles, coordinates, index and neighbors to the three separate entry points"""
    _prologue_vs_separate_launches("small")


def test_update_prologue_equals_separate_launches_euroc():
    """the same at `euroc`: the pooled 30x47 level-1 ring (an odd width), the 1000-frame patch ring, EuRoC intrinsics"""
    _prologue_vs_separate_launches("euroc")


def _prologue_vs_separate_launches(name):
    from cdv_slam_amd.update import UpdatePath
    st = synth.make_state(name)
    dev = torch.device(DEV)
    a, b = UpdatePath(st, dev), UpdatePath(st, dev)
    a.fused_prologue, b.fused_prologue = True, False
    for up in (a, b):   # make the ingest visible: a new frame that differs from what the rings hold
        up.new_frame = (up.new_frame.float() * 0.5 + 0.125).half()
        up.gmap[up.new_tiles:up.new_tiles + up.M] += 0.25
    oa, ob = a.step(iterations=0), b.step(iterations=0)
    torch.cuda.synchronize()
    for k in ("coords", "ix", "jx", "corr"):
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(a.fmap1, b.fmap1) and torch.equal(a.fmap2, b.fmap2) and torch.equal(a.gmap_pm, b.gmap_pm)
    kxa, kua = a.graph.unique()
    kxb, kub = b.graph.unique()
    assert torch.equal(kxa, kxb) and torch.equal(kua, kub)
    ix_o, jx_o = O.neighbors(st.kk, st.jj)
    assert np.array_equal(oa["ix"].cpu().numpy(), ix_o) and np.array_equal(oa["jx"].cpu().numpy(), jx_o)


def test_corr_edge_cases():
    """out-of-bounds windows, windows straddling the border, wide footprints (per-pixel path), exact
    integer coordinates, and the per-level drop-in signature (planar inputs, f16 and f32)."""
    from cdv_slam_amd import altcorr
    rng = np.random.default_rng(5)
    N2, C, H, W, Ng = 3, 24, 20, 28, 10
    fmap2 = (rng.standard_normal((1, N2, C, H, W)) / 4).astype(np.float16)
    gmap = (rng.standard_normal((1, Ng, C, 3, 3)) / 4).astype(np.float16)
    cases = []
    base = np.stack(np.meshgrid(np.arange(3.0), np.arange(3.0), indexing="xy"))  # [2,3,3] x then y offsets
    # (centre, x / y stretch of the 3x3 patch): windows of 11x11 (one round of 9 register groups), 13x13 = 169 and
    # 16x12 = 192 pixels (second round through the registers), wider ones (per-pixel path), off-image ones
    for cx, cy, sx, sy in [(10.3, 8.7, 1.0, 1.0), (-20.0, 5.0, 1.0, 1.0), (0.2, 0.4, 1.0, 1.0), (27.9, 19.9, 1.0, 1.0),
                           (40.0, 40.0, 1.0, 1.0), (12.0, 9.0, 1.0, 1.0), (12.5, 9.5, 6.0, 6.0), (5.0, 5.0, 12.0, 12.0),
                           (-1.0, -1.0, 3.3, 3.3), (13.999, 7.001, 0.2, 0.2), (11.2, 9.4, 2.0, 2.0),
                           (14.6, 10.1, 2.4, 1.2), (12.1, 8.2, 3.5, 1.5), (3.3, 15.8, 1.5, 1.9), (25.7, 2.2, 2.2, 2.2)]:
        cases.append(np.stack([cx + sx * (base[0] - 1), cy + sy * (base[1] - 1)]))
    coords = np.stack(cases)[None].astype(np.float32)  # [1,M,2,3,3]
    M = coords.shape[1]
    us = rng.integers(0, Ng, M).astype(np.int64)
    vs = rng.integers(0, N2, M).astype(np.int64)
    truth = O.corr(gmap[0], fmap2[0], coords[0], us, vs, 3, "truth")
    got = altcorr.corr(T(gmap), T(fmap2), T(coords), T(us), T(vs), 3)  # fast MFMA path via the NHWC shadow
    assert got.shape == (1, M, 7, 7, 3, 3) and got.dtype == torch.float16
    assert np.abs(got[0].float().cpu().numpy() - truth).max() <= _corr_tol(truth)
    # fully out-of-bounds edges are exactly zero
    assert float(got[0, 1].abs().max()) == 0.0 and float(got[0, 4].abs().max()) == 0.0
    # generic kernel: f32 maps, radius 1 and 3
    f2_32, g_32 = fmap2.astype(np.float32), gmap.astype(np.float32)
    for r in (1, 3):
        got32 = altcorr.corr(T(g_32), T(f2_32), T(coords), T(us), T(vs), r)
        want = O.corr(g_32[0], f2_32[0], coords[0], us, vs, r, "truth")
        assert got32.dtype == torch.float32
        assert np.allclose(got32[0].cpu().numpy(), want, rtol=1e-5, atol=1e-5)
        ref32 = O.corr(g_32[0], f2_32[0], coords[0], us, vs, r, "f32")
        assert np.allclose(got32[0].cpu().numpy(), ref32, rtol=1e-5, atol=2e-5)
    # generic kernel, f16, radius 1 (not the MFMA shape)
    got16 = altcorr.corr(T(gmap), T(fmap2), T(coords), T(us), T(vs), 1)
    want = O.corr(gmap[0], fmap2[0], coords[0], us, vs, 1, "truth")
    assert np.abs(got16[0].float().cpu().numpy() - want).max() <= _corr_tol(want)


@pytest.mark.parametrize("C,H,W", [pytest.param(8, 24, 32, id="8"), pytest.param(16, 24, 32, id="16"),
                                   pytest.param(32, 24, 32, id="32"), pytest.param(24, 44, 60, id="24-44x60"),
                                   pytest.param(24, 120, 188, id="24-120x188")])
def test_corr_two_levels_other_widths(C, H, W):
    """the two-level kernel with a run-time feature width (the build for DIMF = 24 is specialised), planar and
    pixel-major tiles, ring indices that wrap (kk % kmod, jj % jmod, slam.py:319-320) and indices out of range (zeros);
    and maps with odd level-1 sides (11x15, and EuRoC's 30x47) with edges aimed at the right and bottom border of level 1"""
    rng = np.random.default_rng(20 + C if (H, W) == (24, 32) else 20 + C + H)
    N2, Ng, M = 5, 12, 300
    f1 = (rng.standard_normal((N2, C, H, W)) / 4).astype(np.float16)
    f2 = f1.reshape(N2, C, H // 4, 4, W // 4, 4).astype(np.float32).mean((3, 5)).astype(np.float16)
    gmap = (rng.standard_normal((Ng, C, 3, 3)) / 4).astype(np.float16)
    coords = np.empty((M, 2, 3, 3), np.float32)
    cx, cy = rng.uniform(-6, W + 6, M), rng.uniform(-6, H + 6, M)
    sc = rng.uniform(0.3, 2.5, M)
    off = np.arange(3.0) - 1
    coords[:, 0] = cx[:, None, None] + sc[:, None, None] * off[None, None, :]
    coords[:, 1] = cy[:, None, None] + sc[:, None, None] * off[None, :, None]
    if (H // 4) % 2 or (W // 4) % 2:
        # level-1 centres on, half a pixel past and beyond the last row / column of an odd-sided level-1 map
        h1, w1 = H // 4, W // 4
        edge = np.array([w1 - 1.0, w1 - 0.5, w1 + 0.25, w1 + 2.75])
        coords[:64, 0] = 4 * np.repeat(edge, 16)[:, None, None] + sc[:64, None, None] * off[None, None, :]
        coords[64:128, 1] = 4 * np.repeat(edge - w1 + h1, 16)[:, None, None] + sc[64:128, None, None] * off[None, :, None]
    kk = rng.integers(0, 5 * Ng, M).astype(np.int64)     # wraps: kk % Ng
    jj = rng.integers(0, 7 * N2, M).astype(np.int64)     # wraps: jj % N2
    dev = torch.device(DEV)
    r1, r2 = ops.alloc_fmap_ring(N2, C, H, W, dev), ops.alloc_fmap_ring(N2, C, H // 4, W // 4, dev)
    ops.fmap_interior(r1).copy_(T(f1).permute(0, 2, 3, 1))
    ops.fmap_interior(r2).copy_(T(f2).permute(0, 2, 3, 1))
    truth = O.slam_corr(gmap, f1, f2, coords, kk % Ng, jj % N2, 3, "truth")
    tol = _corr_tol(truth)
    pm = ops.gmap_to_pixel_major(T(gmap))
    a = ops.corr_fused(T(gmap), r1, r2, T(coords)[None], T(kk), T(jj), kmod=Ng, jmod=N2)
    b = ops.corr_fused(pm, r1, r2, T(coords)[None], T(kk), T(jj), kmod=Ng, jmod=N2, pixel_major=True)
    assert torch.equal(a, b)
    assert np.abs(a[0].float().cpu().numpy() - truth).max() <= tol
    # without the modulus the indices beyond the rings are invalid: those rows are zero, the others unchanged
    c = ops.corr_fused(pm, r1, r2, T(coords)[None], T(kk), T(jj), pixel_major=True)[0].float().cpu().numpy()
    ok = (kk < Ng) & (jj < N2)
    assert ok.any() and (~ok).any()
    assert np.all(c[~ok] == 0) and np.array_equal(c[ok], b[0].float().cpu().numpy()[ok])
    neg = kk.copy(); neg[::3] = -1 - neg[::3]
    d = ops.corr_fused(pm, r1, r2, T(coords)[None], T(neg), T(jj), kmod=Ng, jmod=N2, pixel_major=True)[0].float().cpu().numpy()
    assert np.all(d[::3] == 0) and np.array_equal(d[1::3], b[0].float().cpu().numpy()[1::3])


def test_corr_c128():
    """DPVO feature width (DIMF = 128, net_dpv.py:99): four MFMA k-steps"""
    rng = np.random.default_rng(9)
    N2, C, H, W, Ng, M = 2, 128, 16, 20, 6, 40
    fmap2 = (rng.standard_normal((1, N2, C, H, W)) / 8).astype(np.float16)
    gmap = (rng.standard_normal((1, Ng, C, 3, 3)) / 8).astype(np.float16)
    coords = np.empty((1, M, 2, 3, 3), np.float32)
    cx, cy = rng.uniform(-2, W + 2, M), rng.uniform(-2, H + 2, M)
    off = np.arange(3.0) - 1
    coords[0, :, 0] = cx[:, None, None] + off[None, None, :]
    coords[0, :, 1] = cy[:, None, None] + off[None, :, None]
    us, vs = rng.integers(0, Ng, M).astype(np.int64), rng.integers(0, N2, M).astype(np.int64)
    from cdv_slam_amd import altcorr
    got = altcorr.corr(T(gmap), T(fmap2), T(coords), T(us), T(vs), 3)
    truth = O.corr(gmap[0], fmap2[0], coords[0], us, vs, 3, "truth")
    assert np.abs(got[0].float().cpu().numpy() - truth).max() <= _corr_tol(truth)


def test_patchify_vs_oracle():
    from cdv_slam_amd import altcorr
    rng = np.random.default_rng(3)
    C, H, W, M = 24, 24, 32, 50
    net = rng.standard_normal((1, C, H, W)).astype(np.float16)
    coords = np.stack([rng.uniform(-3, W + 3, M), rng.uniform(-3, H + 3, M)], -1)[None].astype(np.float32)
    for r in (0, 1, 3):
        raw = altcorr.patchify(T(net), T(coords), r, mode="raw")
        assert torch.equal(raw[0].cpu(), torch.as_tensor(O.patchify_raw(net[0], coords[0], r)))
    bl = altcorr.patchify(T(net), T(coords), 1)
    want = O.patchify(net[0], coords[0], 1)
    assert bl.dtype == torch.float32 and np.allclose(bl[0].cpu().numpy(), want, atol=1e-6)
    ul = altcorr.patchify(T(net), T(coords), 0, mode="upperleft")
    assert ul.shape == (1, M, C, 1, 1)


# ---------------------------------------------------------------------------------------------------
# fastba
# ---------------------------------------------------------------------------------------------------

def _run_ba_on(st, graph, iterations=2):
    poses, patches = T(st.poses).clone(), T(st.patches).clone()
    ops.ba_forward(poses, patches, T(st.intrinsics), T(st.target), T(st.weight), torch.tensor([st.lmbda], device=DEV), T(st.ii),
                   T(st.jj), T(st.kk), st.cfg.M, st.t0, st.n, iterations, False, graph=graph)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), patches.cpu().numpy(), None


def _run_ba(st, iterations=2, debug=False, t0=None, t1=None):
    poses, patches = T(st.poses).clone(), T(st.patches).clone()
    t0 = st.t0 if t0 is None else t0
    t1 = st.n if t1 is None else t1
    res = ops.ba_forward(poses, patches, T(st.intrinsics), T(st.target), T(st.weight),
                         torch.tensor([st.lmbda], device=DEV), T(st.ii), T(st.jj), T(st.kk), st.cfg.M, t0, t1,
                         iterations, False, debug=debug)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), patches.cpu().numpy(), res


# graphs of the 10 < N <= 32 path (ba_mid.hip): `stress` (N = 21, M = 196), and two variants of `small`: N = 15 (an odd
# number of poses: the solver's last block is 6 wide) and N = 19 with 5 patches per frame (a chunk of 16 consecutive
# patches spans four source frames: two passes over the chunk)
MID_VARIANTS = {"mid15": dict(opt_window=15), "mid19_m5": dict(opt_window=19, M=5),
                # the ends of the path's range: 11 and 32 free poses (the latter: the largest system the solver's LDS holds)
                "mid11": dict(opt_window=11), "mid32": dict(frames=34, opt_window=32, removal_window=34, buffer_size=40)}


# tolerance class (tests/ba_checks.py) of a variant: mid32 frees all poses but two, the weak-scale-gauge class of pr1
MID_TOL = {"mid32": "pr1"}


# the window (N = 10) and mid (N = 21) graphs at EuRoC's 480x752 frames and calibration, in which no two of fx, fy, cx, cy
# are equal: each keeps the tolerance class of its graph
EUROC = dict(ht=480, wd=752, intr=synth.EUROC_INTR)
EUROC_VARIANTS = {"default_euroc": "default", "stress_euroc": "stress"}


def _make(name):
    if name in MID_VARIANTS:
        return synth.make_state("small", features=False, **MID_VARIANTS[name]), MID_TOL.get(name, "small")
    if name in EUROC_VARIANTS:
        return synth.make_state(EUROC_VARIANTS[name], features=False, **EUROC), EUROC_VARIANTS[name]
    return synth.make_state(name, features=False), name


@pytest.mark.parametrize("name", ["small", "init", "pr1", "default", "stress", "mid15", "mid19_m5", "mid11", "mid32",
                                  "default_euroc", "stress_euroc"])
def test_ba_intermediates_vs_oracle(name):
    """iteration-0 S, y, C, u, E, dX, dZ against the float64 oracle"""
    st, name = _make(name)
    _, _, dbg = _run_ba(st, iterations=1, debug=True)
    _, _, info, o = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                             st.kk, st.t0, st.n, 1, np.float64, debug=True)
    assert info == 0
    U = len(o["kx"])
    for key, got, want in (("S", dbg["S"], o["S"]), ("y", dbg["y"], o["y"]), ("C", dbg["C"][:U], o["C"]),
                           ("u", dbg["u"][:U], o["u"]), ("E", dbg["E"][:, :U], o["E"])):
        got = got.cpu().numpy()
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), key
    # dX, dZ: stated bounds (tests/ba_checks.py) -- the error of dX inside the well-determined
    # eigen-subspace of S, along the weak (scale) directions, the backward error of the kernel's own solve, dZ
    ba_checks.check_iteration0(name, {k: v.cpu().numpy() for k, v in dbg.items()}, o)


@pytest.mark.parametrize("name", ["small", "init", "pr1", "default", "stress", "mid15", "mid19_m5", "mid11", "mid32",
                                  "default_euroc", "stress_euroc"])
def test_ba_two_iterations_vs_oracle(name):
    st, name = _make(name)
    poses, patches, _ = _run_ba(st, iterations=2)
    p64, x64, info = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                              st.kk, st.t0, st.n, 2, np.float64)
    assert info == 0
    # explicit per-config bounds (tests/ba_checks.py = BASELINE.md section 5): raw poses / depths, and the gauge-free
    # quantities (Sim(3)-aligned ATE, reprojection cost) that carry the claim on the weak-gauge graphs init / pr1
    ba_checks.check_end_state(name, st, poses, patches, p64, x64)
    # fixed poses and untouched patches are bit-identical to the input
    assert np.array_equal(poses[:st.t0], st.poses[:st.t0])
    untouched = np.setdiff1d(np.arange(len(st.patches)), np.unique(st.kk))
    assert np.array_equal(patches[untouched], st.patches[untouched])
    # all P*P depth pixels of an updated patch are equal (ba_cuda.cu:223-227)
    k0 = np.unique(st.kk)
    assert np.all(patches[k0, 2] == patches[k0, 2, :1, :1])


@pytest.mark.parametrize("name", ["global", "global_l", "global_euroc"])
def test_global_ba_vs_oracle(name):
    """more than 32 free poses (slam.py:460-478, eff_impl=True in the reference): panel-sparse Schur products + blocked
    multi-workgroup Cholesky.  Same numbers as the dense path (ba_cuda.cu:567-580 == :583-592), checked against the
    float64 oracle: intermediates of iteration 0, then the state after two iterations.  global_euroc: the `global` graph
    at EuRoC's frames and calibration (tolerance class of `global`)."""
    if name == "global_euroc":
        st, name = synth.make_state("global", features=False, **EUROC), "global"
    else:
        st = synth.make_state(name, features=False)
    N = st.n - st.t0
    assert N > 32
    _, _, dbg = _run_ba(st, iterations=1, debug=True)
    _, _, info, o = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                             st.kk, st.t0, st.n, 1, np.float64, debug=True)
    assert info == 0
    U = len(o["kx"])
    S = np.tril(dbg["S"].cpu().numpy())     # this path accumulates and factors the lower triangle only
    assert np.abs(S - np.tril(o["S"])).max() <= 1e-4 * np.abs(o["S"]).max()
    for key, got, want in (("y", dbg["y"], o["y"]), ("C", dbg["C"][:U], o["C"]), ("u", dbg["u"][:U], o["u"]),
                           ("E", dbg["E"][:, :U], o["E"])):
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max(), key
    ba_checks.check_iteration0(name, {k: v.cpu().numpy() for k, v in dbg.items()}, o)
    # two iterations, end state; the dense-path call signature with eff_impl=True goes the same way
    poses, patches, _ = _run_ba(st, iterations=2)
    p64, x64, info = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                              st.kk, st.t0, st.n, 2, np.float64)
    ba_checks.check_end_state(name, st, poses, patches, p64, x64)
    assert np.array_equal(poses[:st.t0], st.poses[:st.t0])
    # a second call on the same workspace (accumulators re-zeroed by their consumers) gives the same answer
    poses2, patches2, _ = _run_ba(st, iterations=2)
    ba_checks.check_end_state(name, st, poses2, patches2, p64, x64)


def test_global_ba_at_the_reference_scale():
    """the global bundle adjustment at the size slam.py:460-478 runs it with MAX_EDGE_AGE = 1000 (slam.py:66-71): 299 free
    poses, 28,800 patches, 0.7 M edges (a 1794 x 1794 reduced system, a 1794 x 28,800 E) against the float64 oracle --
    intermediates of iteration 0, dX split by the eigen-subspaces of S, the state after two iterations"""
    st = synth.make_state("global_xl", features=False)
    assert st.n - st.t0 == 299 and st.E > 700000
    _, _, dbg = _run_ba(st, iterations=1, debug=True)
    _, _, info, o = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                             st.kk, st.t0, st.n, 1, np.float64, debug=True)
    assert info == 0
    U = len(o["kx"])
    assert U == 28800
    S = np.tril(dbg["S"].cpu().numpy())
    assert np.abs(S - np.tril(o["S"])).max() <= 1e-4 * np.abs(o["S"]).max()
    # y = v - E Q u sums ~2,400 signed terms of size 1e2 per entry into |y| ~ 1e3: float32 itself (the reference's
    # arithmetic restated in float32, sequential sums) is off by 1.6e-4 of max |y| here, so the bound for y is 5e-4 at
    # this scale; everything else keeps 1e-4
    for key, got, want, tol in (("y", dbg["y"], o["y"], 5e-4), ("C", dbg["C"][:U], o["C"], 1e-4),
                                ("u", dbg["u"][:U], o["u"], 1e-4), ("E", dbg["E"][:, :U], o["E"], 1e-4)):
        assert np.abs(got.cpu().numpy() - want).max() <= tol * np.abs(want).max(), key
    ba_checks.check_iteration0("global_xl", {k: v.cpu().numpy() for k, v in dbg.items() if k != "E"}, o)
    del dbg
    poses, patches, _ = _run_ba(st, iterations=2)
    p64, x64, info = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                              st.kk, st.t0, st.n, 2, np.float64)
    ba_checks.check_end_state("global_xl", st, poses, patches, p64, x64)
    assert ops.ba_status(torch.device(DEV)) == (0, 0, 0, 0)


def test_global_ba_more_work_items_than_workgroups():
    """the one-launch factorisation (ba_factor.hip) at 479 free poses: 45 block columns, ~1,000 block work items for the 256
    workgroups of the launch -- items queue behind the ticket counter and wait on flags of items that other workgroups are
    still holding.  Without an oracle run at this size: the solve's backward error || S dX - y || / || y || from the
    iteration-0 dump (the same bound as everywhere), the factor flagged positive definite, and two calls bit for bit equal."""
    st = synth.make_state("global", features=False, frames=480, M=24, buffer_size=496, ht=384, wd=512)
    assert st.n - st.t0 == 479
    _, _, dbg = _run_ba(st, iterations=1, debug=True)
    S = np.tril(dbg["S"].cpu().numpy().astype(np.float64))
    S = S + np.tril(S, -1).T
    y = dbg["y"].cpu().numpy().astype(np.float64)
    dX = dbg["dX"].cpu().numpy().astype(np.float64).reshape(-1)
    # (the working copy carries the damping of ba_cuda.cu:589 on its diagonal: the dump is that copy)
    res = np.linalg.norm(S @ dX - y) / np.linalg.norm(y)
    print("solve residual at N = 479: %.2e (<= %.0e)" % (res, ba_checks.SOLVE_RESIDUAL_TOL))
    assert res <= ba_checks.SOLVE_RESIDUAL_TOL, res
    del dbg
    assert ops.ba_status(torch.device(DEV)) == (0, 0, 0, 0)
    p1, x1, _ = _run_ba(st, iterations=2)
    p2, x2, _ = _run_ba(st, iterations=2)
    assert np.isfinite(p1).all() and not np.array_equal(p1, st.poses)
    assert np.array_equal(p1, p2) and np.array_equal(x1, x2)
    assert ops.ba_status(torch.device(DEV)) == (0, 0, 0, 0)


def _circle_pose(t, period=60.0, radius=0.5):
    """camera t of a closed path: world-to-camera pose (t, q) of a camera at radius * (cos a, sin a, 0) looking along +z"""
    a = 2 * np.pi * t / period
    return [-radius * np.cos(a), -radius * np.sin(a), 0.0, 0.0, 0.0, 0.0, 1.0]


def test_loop_closure_stream_runs_the_global_ba():
    """configs[2]'s mechanics on a synthetic stream (no images: stub networks): LOOP_CLOSURE keeps the patch ring at
    MAX_EDGE_AGE = 1000 frames (slam.py:66-71; the correlation indexes it with kk % (M * 1000)), edges_loop adds proximity
    edges when the camera comes back to where it was (patchgraph.py:71-97, slam.py:699-705), those edges survive the
    removal window (slam.py:453-457), and an update that sees long-range edges runs the GLOBAL bundle adjustment over
    inactive + active edges (slam.py:460-478,507).  Checked: the edge bookkeeping -- active and inactive lists -- against
    the numpy restatement of slam.py, bit for bit, after every frame; the global BA against the float64 oracle on the
    very state it ran on."""
    from cdv_slam_amd.stream import StreamRunner
    from oracle.edges_py import EdgesPy
    dev = torch.device(DEV)
    M = 16
    run = StreamRunner(dev, M=M, ht=192, wd=256, buffer_size=160, loop_closure=True, max_edge_age=1000, global_opt_freq=15,
                       backend_thresh=64.0, pose_init=_circle_pose, record_global=True)
    assert run.pmem == 1000 and run.gmap.shape[0] == 1000 * M and run.gmap_pm.shape[0] == 1000 * M
    g = EdgesPy()
    ix_np = np.repeat(np.arange(run.N), M)
    checked_global = False
    for f in range(110):
        n_globals = run.n_global
        run.frame(drop=False)
        n = run.n
        # the same frame through the numpy restatement (slam.py:699-709, then keyframe() without a drop)
        if run.last_loop_edges is not None:
            lk, lj = (t.cpu().numpy() for t in run.last_loop_edges)
            assert len(lk) % M == 0 and ((lj - ix_np[lk]) >= 30).all()
            g.append_factors(lk, lj, ix_np)
        g.append_factors(*g.edges_forw(n, M, run.r), ix_np)
        g.append_factors(*g.edges_back(n, M, run.r), ix_np)
        if n >= 8:
            g.keyframe(-1, n, M, ix_np, run.rw, drop=False, loop_closure=True, opt_window=run.ow)
        e = run.edges
        assert e.E == len(g.ii) and e.E_inac == len(g.ii_inac), (f, e.E, len(g.ii))
        assert np.array_equal(e.ii.cpu().numpy(), g.ii) and np.array_equal(e.jj.cpu().numpy(), g.jj) \
            and np.array_equal(e.kk.cpu().numpy(), g.kk)
        assert np.array_equal(e.ii_inac[:e.E_inac].cpu().numpy(), g.ii_inac) and \
            np.array_equal(e.kk_inac[:e.E_inac].cpu().numpy(), g.kk_inac)
        if run.n_global > n_globals and not checked_global:
            checked_global = True
            rec = run.last_global
            ii, jj, kk = (rec[k].cpu().numpy() for k in ("ii", "jj", "kk"))
            assert rec["E_inactive"] > 0 and len(ii) == rec["E_inactive"] + rec["E_active"]
            assert ((jj - ii) >= 30).any()                              # loop edges took part (reduce_edges admits j - i >= 30)
            assert (ii < rec["n"] - run.rw - 1).any()                   # what triggered the global BA (slam.py:507)
            assert rec["n"] - rec["t0"] > 32                            # the multi-workgroup solver path
            p0, x0 = rec["poses"].cpu().numpy(), rec["patches"].cpu().numpy()
            tg, wg = rec["target"].cpu().numpy(), rec["weight"].cpu().numpy()
            intr = run.intrinsics.cpu().numpy()
            p64, x64, info = O.fastba(p0, x0, intr[0], tg, wg, 1e-4, ii, jj, kk, rec["t0"], rec["n"], 2, np.float64)
            assert info == 0

            class _State:      # what ba_checks reads of a synthetic state
                pass
            s = _State()
            s.intrinsics, s.ii, s.jj, s.kk, s.target, s.weight, s.n = intr, ii, jj, kk, tg, wg, rec["n"]
            got_p, got_x = run.poses.cpu().numpy(), run.patches.cpu().numpy()   # nothing touched them since the BA
            ba_checks.check_end_state("global", s, got_p, got_x, p64, x64)
            assert not np.array_equal(got_p[rec["t0"]:rec["n"]], p0[rec["t0"]:rec["n"]])
            assert ops.ba_status(dev) == (0, 0, 0, 0)
    assert checked_global, "the stream never ran a global bundle adjustment"
    assert run.n_global >= 2             # ... and did so again GLOBAL_OPT_FREQ frames later


def test_corr_patch_ring_of_a_thousand_frames():
    """the fused correlation with the LOOP_CLOSURE patch ring (pmem = MAX_EDGE_AGE = 1000, M = 96: kmod = 96,000 tiles,
    slam.py:66-71,319): raw patch ids far beyond the ring, wrapped by the kernel's reciprocal-multiply modulus"""
    rng = np.random.default_rng(33)
    C, H, W, mem, Ng, E = 24, 24, 32, 4, 96000, 2000
    f1 = (rng.standard_normal((mem, C, H, W)) / 4).astype(np.float16)
    f2 = f1.reshape(mem, C, H // 4, 4, W // 4, 4).astype(np.float32).mean((3, 5)).astype(np.float16)
    gmap = (rng.standard_normal((Ng, C, 3, 3)) / 4).astype(np.float16)
    coords = np.empty((E, 2, 3, 3), np.float32)
    cx, cy = rng.uniform(2, W - 2, E), rng.uniform(2, H - 2, E)
    off = np.arange(3.0) - 1
    coords[:, 0] = cx[:, None, None] + off[None, None, :]
    coords[:, 1] = cy[:, None, None] + off[None, :, None]
    kk = rng.integers(0, 40 * Ng, E).astype(np.int64)        # frames long gone by: ids up to 3.8 M
    kk[:8] = [0, Ng - 1, Ng, Ng + 1, 2 * Ng - 1, 39 * Ng + 95999, 95999, 96000]
    jj = rng.integers(0, 30 * mem, E).astype(np.int64)
    dev = torch.device(DEV)
    r1, r2 = ops.alloc_fmap_ring(mem, C, H, W, dev), ops.alloc_fmap_ring(mem, C, H // 4, W // 4, dev)
    ops.fmap_interior(r1).copy_(T(f1).permute(0, 2, 3, 1))
    ops.fmap_interior(r2).copy_(T(f2).permute(0, 2, 3, 1))
    pm = ops.gmap_to_pixel_major(T(gmap))
    out = ops.corr_fused(pm, r1, r2, T(coords)[None], T(kk), T(jj), kmod=Ng, jmod=mem, pixel_major=True)
    truth = O.slam_corr(gmap, f1, f2, coords, kk % Ng, jj % mem, 3, "truth")
    assert np.abs(out[0].float().cpu().numpy() - truth).max() <= _corr_tol(truth)


@pytest.mark.parametrize("tag", ["fc", "win"])
def test_ba_py_mirror_vs_reference_golden(golden_dir, tag):
    """cdv_slam_amd.ba.BA == the reference's own cdvslam/ba.py run on the same inputs (tests/golden/ba_py_*.npz,
    generated by tests/golden/make_golden.py): both `ep` settings, a second step from the first result, and the
    structure-only branch.  Tolerances as in the oracle's own golden test (float32 Gauss-Newton)."""
    from cdv_slam_amd import ba
    from cdv_slam_amd.lietorch import SE3
    g = np.load(os.path.join(golden_dir, "ba_py_%s.npz" % tag))
    G = lambda k: T(g[k].astype(np.float32) if g[k].dtype.kind == "f" else g[k])
    args = (G("intrinsics")[None], G("target")[None], G("weight")[None], torch.tensor([1e-4], device=DEV), G("ii"),
            G("jj"), G("kk"), [float(b) for b in g["bounds"]])
    for ep in (1.0, 100.0):
        tol = 1e-4 if ep == 1.0 else 2e-5
        P2, X2 = ba.BA(SE3(G("poses")[None]), G("patches")[None], *args, ep=ep, fixedp=1)
        assert isinstance(P2, SE3)
        assert np.allclose(P2.data[0].cpu().numpy(), g["poses_ep%g" % ep], atol=tol)
        assert np.allclose(X2[0].cpu().numpy(), g["patches_ep%g" % ep], rtol=10 * tol, atol=tol)
        P3, X3 = ba.BA(P2, X2, *args, ep=ep, fixedp=1)
        assert np.allclose(P3.data[0].cpu().numpy(), g["poses2_ep%g" % ep], atol=3 * tol)
        assert np.allclose(X3[0].cpu().numpy(), g["patches2_ep%g" % ep], rtol=30 * tol, atol=3 * tol)
    Ps, Xs = ba.BA(SE3(G("poses")[None]), G("patches")[None], *args, ep=1.0, fixedp=1, structure_only=True)
    assert np.allclose(Xs[0].cpu().numpy(), g["patches_structure_only"], rtol=2e-4, atol=2e-5)
    assert torch.equal(Ps.data, G("poses")[None])


def test_ba_py_mirror_vs_reference_run_on_configs0():
    """BASELINE configs[0] (10 x 96 fully connected, E = 9,600): cdv_slam_amd.ba.BA against what the reference's own
    cdvslam/ba.py:86-185 produced on the same inputs (tests/golden/ba_py_pr1.npz), two successive calls and the
    structure-only branch"""
    from cdv_slam_amd import ba
    from cdv_slam_amd.lietorch import SE3
    from tests import golden_util
    g = golden_util.load_ba_pr1()
    args = (T(g["intrinsics"])[None], T(g["target"])[None], T(g["weight"])[None], torch.tensor([1e-4], device=DEV),
            T(g["ii"]), T(g["jj"]), T(g["kk"]), [float(b) for b in g["bounds"]])
    P1, X1 = ba.BA(SE3(T(g["poses"])[None]), T(g["patches"])[None], *args, ep=1.0, fixedp=1)
    e1 = (np.abs(P1.data[0].cpu().numpy() - g["poses1"]).max(), np.abs(X1[0, :, 2, 0, 0].cpu().numpy() - g["d1"]).max())
    P2, X2 = ba.BA(P1, X1, *args, ep=1.0, fixedp=1)
    e2 = (np.abs(P2.data[0].cpu().numpy() - g["poses2"]).max(), np.abs(X2[0, :, 2, 0, 0].cpu().numpy() - g["d2"]).max())
    print("ba.py mirror vs reference run (pr1): call 1 poses %.2e depth %.2e, call 2 poses %.2e depth %.2e" % (e1 + e2))
    # the reference is a float32 Gauss-Newton on a weak-gauge system (one fixed pose): tests/ba_checks.py BA_TOL['pr1']
    assert e1[0] <= 3e-5 and e1[1] <= 1e-4 and e2[0] <= 6e-5 and e2[1] <= 2e-4
    assert torch.equal(X2[0, :, :2], T(g["patches"])[:, :2]) and torch.equal(X2[0, :, 2], X2[0, :, 2, :1, :1].expand(-1, 3, 3))
    _, Xs = ba.BA(SE3(T(g["poses"])[None]), T(g["patches"])[None], *args, ep=1.0, fixedp=1, structure_only=True)
    assert np.abs(Xs[0, :, 2, 0, 0].cpu().numpy() - g["d_structure_only"]).max() <= 2e-5


def test_fastba_hip_vs_reference_ba_py_run_on_configs0():
    """the HIP fastba (cdv_ba_forward through ops.ba_forward) against the reference's own ba.py run on BASELINE
    configs[0]: ep = 1.0 is fastba's damping (ba_cuda.cu:589 == ba.py:66-73), and on this state no gate the two differ in
    fires (checked on the CPU in tests/test_oracle_golden.py), so one fastba iteration == one ba.py call and two
    iterations == two successive calls, to the float32 weak-gauge bounds BA_TOL['pr1'] -- plus the gauge-free ATE."""
    from cdv_slam_amd import metrics
    from tests import golden_util
    g = golden_util.load_ba_pr1()
    n, M = int(g["frames"]), int(g["M"])
    tol = ba_checks.BA_TOL["pr1"]
    for it, pk, dk in ((1, "poses1", "d1"), (2, "poses2", "d2")):
        poses, patches = T(g["poses"]).clone(), T(g["patches"]).clone()
        ops.ba_forward(poses, patches, T(g["intrinsics"]), T(g["target"]), T(g["weight"]), torch.tensor([1e-4], device=DEV),
                       T(g["ii"]), T(g["jj"]), T(g["kk"]), M, 1, n, it, False)
        torch.cuda.synchronize()
        p, d = poses.cpu().numpy(), patches[:, 2, 0, 0].cpu().numpy()
        got = dict(t=np.abs(p[:, :3] - g[pk][:, :3]).max(), q=np.abs(p[:, 3:] - g[pk][:, 3:]).max(),
                   d=(np.abs(d - g[dk]) / np.maximum(np.abs(g[dk]), 1e-2)).max(), ate=metrics.ate_rmse(g[pk][:n], p[:n]))
        print("HIP fastba x%d vs reference ba.py (pr1): " % it + "  ".join("%s %.2e" % kv for kv in got.items()))
        ba_checks._log("vs_reference_ba_py", "pr1_it%d" % it, got, {k: tol[k] * it for k in got})
        for k in got:
            assert got[k] <= tol[k] * it, (it, k, got[k])
        # in-place contract on the reference's state: the fixed pose and the x / y planes are untouched, nine equal depths
        assert torch.equal(poses[0], T(g["poses"])[0]) and torch.equal(patches[:, :2], T(g["patches"])[:, :2])
        assert torch.equal(patches[:n * M, 2], patches[:n * M, 2, :1, :1].expand(-1, 3, 3))


def test_fastba_hip_vs_reference_ba_py_at_euroc_intrinsics(golden_dir):
    """the HIP fastba against the reference's own ba.py (float64, two successive calls at ep = 1.0) at the EuRoC calibration
    with bounds = [-64, -64, 2 cx + 64, 2 cy + 64] -- the gates coincide (tests/test_oracle_golden.py checks it), edges
    reproject into the band 2 cx + 64 < u < W + 64 -- to the bounds of the well-conditioned class BA_TOL['default'] (two
    fixed poses anchor scale)"""
    from cdv_slam_amd import metrics
    g = np.load(os.path.join(golden_dir, "ba_py_euroc.npz"))
    n, M, t0 = int(max(g["ii"].max(), g["jj"].max())) + 1, 8, int(g["t0"])
    tol = ba_checks.BA_TOL["default"]
    unit = lambda q: q / np.linalg.norm(q, axis=1, keepdims=True)
    for it, pk, xk in ((1, "poses1", "patches1"), (2, "poses2", "patches2")):
        poses, patches = T(g["poses"]).clone(), T(g["patches"]).clone()
        ops.ba_forward(poses, patches, T(g["intrinsics"]), T(g["target"]), T(g["weight"]), torch.tensor([1e-4], device=DEV),
                       T(g["ii"]), T(g["jj"]), T(g["kk"]), M, t0, n, it, False)
        torch.cuda.synchronize()
        p, d, dr = poses.cpu().numpy(), patches[:, 2, 0, 0].cpu().numpy(), g[xk][:, 2, 0, 0]
        got = dict(t=np.abs(p[:, :3] - g[pk][:, :3]).max(), q=np.abs(unit(p[:, 3:]) - unit(g[pk][:, 3:])).max(),
                   d=(np.abs(d - dr) / np.maximum(np.abs(dr), 1e-2)).max(), ate=metrics.ate_rmse(g[pk][:n], p[:n]))
        ba_checks._log("vs_reference_ba_py", "euroc_it%d" % it, got, {k: tol[k] * it for k in got})
        for k in got:
            assert got[k] <= tol[k] * it, (it, k, got[k])


def test_ba_gate_band_of_the_calibrated_in_bounds_gate():
    """fastba's in-bounds gate is u < 2 cx + 64, v < 2 cy + 64 (ba_cuda.cu:305-306), not an image-size gate: with EuRoC's
    cx = 91.8 (W / 2 = 94) edges whose centres reproject into 247.6 < u < 252 carry nonzero weight and must be masked.
    The HIP window solver equals the float64 oracle on such a graph; the oracle masks those edges (their weights set to
    zero change nothing, bit for bit), and so does the HIP path."""
    from tests import golden_util
    st = golden_util.euroc_window_state()
    args = lambda w: (st.poses, st.patches, st.intrinsics[0], st.target, w, st.lmbda, st.ii, st.jj, st.kk, st.t0, st.n)
    # edges in the band at both states the two iterations evaluate the gate at
    p1, x1, _ = O.fastba(*args(st.weight), 1, np.float64)
    band = golden_util.euroc_gate_band(st) & golden_util.euroc_gate_band(st, p1)
    assert band.sum() >= 5 and (st.weight[band] > 0).all()
    p64, x64, info = O.fastba(*args(st.weight), 2, np.float64)
    assert info == 0
    w0 = st.weight.copy()
    w0[band] = 0
    q64, y64, _ = O.fastba(*args(w0), 2, np.float64)
    assert np.array_equal(p64, q64) and np.array_equal(x64, y64)
    # those edges lie between the calibrated gate and the image-size one
    u = O.fastba_reproject(st.poses, st.patches, st.intrinsics[0], st.ii, st.jj, st.kk, dtype=np.float64)[:, 0, 1, 1]
    assert (u[band] > 2 * np.float64(st.intrinsics[0, 2]) + 64).all() and (u[band] < st.cfg.wd // 4 + 64).all()
    poses, patches, _ = _run_ba(st, iterations=2)
    tol = ba_checks.BA_TOL["default"]
    d, d64 = patches[:, 2, 0, 0], x64[:, 2, 0, 0]
    assert np.abs(poses[:, :3] - p64[:, :3]).max() <= tol["t"] and np.abs(poses[:, 3:] - p64[:, 3:]).max() <= tol["q"]
    assert (np.abs(d - d64) / np.maximum(np.abs(d64), 1e-2)).max() <= tol["d"]
    st0 = golden_util.euroc_window_state()
    st0.weight = w0
    poses0, patches0, _ = _run_ba(st0, iterations=2)
    assert np.array_equal(poses, poses0) and np.array_equal(patches, patches0)


def test_ba_reads_the_intrinsics_of_row_zero_only():
    """fastba takes one camera, intrinsics[0] (ba_cuda.cu:255-258): other rows changed -> bit-identical output; row 0
    changed -> a different one"""
    from tests import golden_util
    st = golden_util.euroc_window_state()
    poses, patches, _ = _run_ba(st, iterations=2)
    st.intrinsics[1:] *= np.float32([1.1, 0.9, 1.05, 0.95])
    p1, x1, _ = _run_ba(st, iterations=2)
    assert np.array_equal(poses, p1) and np.array_equal(patches, x1)
    st.intrinsics[0] *= np.float32([1.0, 1.0, 1.01, 1.0])
    p2, x2, _ = _run_ba(st, iterations=2)
    assert np.abs(p2 - poses).max() > 1e-5


def test_patchify_vs_reference_python_layer(golden_dir):
    """altcorr.patchify (one launch: gather + blend) and ops.patchify_multi against the outputs of the reference's own
    cdvslam/altcorr/correlation.py:51-71 (tests/golden/patchify_py.npz): three modes, r = 0 / 1 / 3, f16 and f32 maps,
    batch 2, corners and far-outside coordinates"""
    from cdv_slam_amd import altcorr
    g = np.load(os.path.join(golden_dir, "patchify_py.npz"))
    coords = T(g["coords"])
    for tag in ("f16", "f32"):
        net = T(g["net16" if tag == "f16" else "net32"])
        for r in (0, 1, 3):
            for mode in ("bilinear", "upperleft", "raw"):
                want = g["%s_r%d_%s" % (tag, r, mode)]
                got = altcorr.patchify(net, coords, r, mode=mode).cpu().numpy()
                assert got.dtype == want.dtype and got.shape == want.shape, (tag, r, mode)
                if mode == "bilinear":
                    assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (tag, r, mode)
                else:
                    assert np.array_equal(got, want), (tag, r, mode)
            for b in range(net.shape[0]):                       # the one-launch form of a frame's calls (batch 1)
                multi = ops.patchify_multi([dict(net=net[b], radius=r, mode="bilinear"), dict(net=net[b], radius=r, mode="upperleft")],
                                           coords[b])
                assert np.abs(multi[0][0].cpu().numpy() - g["%s_r%d_bilinear" % (tag, r)][b]).max() <= 4e-6
                assert np.array_equal(multi[1][0].cpu().numpy(), g["%s_r%d_upperleft" % (tag, r)][b])


def test_transform_vs_reference_run_on_small():
    """cdv_transform against the reference's own projective_ops.py:53-130 on every 6th edge of the `small` graph with
    per-frame intrinsics (tests/golden/pops_small_f32.npz)"""
    from cdv_slam_amd import projective_ops as pops
    from cdv_slam_amd.lietorch import SE3
    from tests import golden_util
    g = golden_util.load_pops_small()
    poses, patches, intr = T(g["poses"])[None], T(g["patches"])[None], T(g["intrinsics"])[None]
    ii, jj, kk = T(g["ii"]), T(g["jj"]), T(g["kk"])
    x1 = pops.transform(SE3(poses), patches, intr, ii, jj, kk)
    assert np.abs(x1[0].cpu().numpy() - g["coords"]).max() < 1e-3
    x1j, v, (Ji, Jj, Jz) = pops.transform(SE3(poses), patches, intr, ii, jj, kk, jacobian=True)
    assert np.array_equal(v[0].cpu().numpy(), g["valid"])
    assert np.abs(x1j[0, :, 1, 1].cpu().numpy() - g["coords_jac_centre"]).max() < 1e-3
    for a, b in ((Ji, g["Ji"]), (Jj, g["Jj"]), (Jz, g["Jz"])):
        assert np.allclose(a[0].cpu().numpy(), b, rtol=2e-4, atol=1e-4 * np.abs(b).max())
    x1v, val = pops.transform(SE3(poses), patches, intr, ii, jj, kk, valid=True)
    assert np.array_equal(val[0].cpu().numpy(), g["validpx"])
    fm, fv = pops.flow_mag(SE3(poses), patches, intr, ii, jj, kk, beta=0.5)
    assert np.allclose(fm[0].cpu().numpy(), g["flow_mag"], atol=2e-3) and np.array_equal(fv[0].cpu().numpy(), g["flow_valid"])
    m = g["point_cloud_centre"].shape[0]
    ix = T((np.arange(m) // 16).astype(np.int64))
    pc = pops.point_cloud(SE3(poses), patches[:, :m], intr, ix)
    assert np.allclose(pc[0, :, 1, 1].cpu().numpy(), g["point_cloud_centre"], rtol=1e-4, atol=1e-4)


def test_fused_flow_mag_point_cloud_patchify_vs_composed():
    """the one-launch forms of pops.flow_mag / pops.point_cloud / altcorr.patchify(mode=...) against the op-by-op
    composition the reference writes (projective_ops.py:115-130, correlation.py:51-71) and the oracle"""
    from cdv_slam_amd import projective_ops as pops, altcorr
    from cdv_slam_amd.lietorch import SE3
    st = synth.make_state("small")
    poses, patches, intr = T(st.poses)[None], T(st.patches)[None], T(st.intrinsics)[None]
    ii, jj, kk = T(st.ii), T(st.jj), T(st.kk)
    # flow_mag: fused vs composed out of three transforms
    flow, val = pops.flow_mag(SE3(poses), patches, intr, ii, jj, kk, beta=0.5)
    c0 = pops.transform(SE3(poses), patches, intr, ii, ii, kk)
    c1, v1 = pops.transform(SE3(poses), patches, intr, ii, jj, kk, valid=True)
    c2 = pops.transform(SE3(poses), patches, intr, ii, jj, kk, tonly=True)
    want = 0.5 * (c1 - c0).norm(dim=-1) + 0.5 * (c2 - c0).norm(dim=-1)
    assert flow.shape == want.shape and val.dtype == torch.bool
    assert float((flow - want).abs().max()) <= 2e-3 and torch.equal(val, v1 > 0.5)
    # point_cloud: fused vs inv * iproj, and vs the oracle's Lie arithmetic
    m = 200
    ix = T((np.arange(m) // st.cfg.M).astype(np.int64))
    pc = pops.point_cloud(SE3(poses), patches[:, :m], intr, ix)
    comp = SE3(poses)[:, ix, None, None].inv() * pops.iproj(patches[:, :m], intr[:, ix])
    assert pc.shape == (1, m, 3, 3, 4) and float((pc - comp).abs().max()) <= 1e-5 * float(comp.abs().max())
    # patchify with blend modes: fused vs gather + four slice products, float16 and float32 maps
    fmap = T(st.fmap1[:2])                                   # [2,C,h,w] f16
    M = 64
    rng = np.random.default_rng(3)
    coords = T(np.stack([rng.uniform(-2, fmap.shape[-1] + 1, (2, M)), rng.uniform(-2, fmap.shape[-2] + 1, (2, M))], -1)
               .astype(np.float32))
    for net in (fmap, fmap.float()):
        for r in (0, 1):
            raw = ops.patchify_forward(net, coords, r)
            off = coords - coords.floor()
            dx, dy = off[:, :, None, None, None].unbind(dim=-1)
            d = 2 * r + 1
            want = ((1 - dy) * (1 - dx) * raw[..., :d, :d] + (1 - dy) * dx * raw[..., :d, 1:]
                    + dy * (1 - dx) * raw[..., 1:, :d] + dy * dx * raw[..., 1:, 1:])
            got = altcorr.patchify(net, coords, r, mode='bilinear')
            assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
            assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
            ul = altcorr.patchify(net, coords, r, mode='upperleft')
            assert ul.dtype == net.dtype and torch.equal(ul, raw[..., :1, :1])


def test_patchify_frame_in_one_launch():
    """cdv_patchify_multi: the four altcorr.patchify calls of a new frame (net_cdv.py:355-374: imap at the DINO scale with
    the configured sampling mode, gmap, colours at 4 (c + 0.5), patches from the coordinate / inverse-depth grid) against
    the four separate calls on coordinates scaled with torch ops as the reference does -- bit-identical"""
    _patchify_frame(24, 32, 7, 9)


def test_patchify_frame_in_one_launch_euroc():
    """the same on EuRoC's 120x188 maps with a DINO grid (34x53) that does not divide them"""
    _patchify_frame(120, 188, 34, 53)


def _patchify_frame(h, w, dh, dw):
    from cdv_slam_amd import altcorr
    g = torch.Generator(device="cpu").manual_seed(11)
    M = 96
    fmap = (torch.randn((1, 24, h, w), generator=g) / 4).half().to(DEV)
    imap = torch.randn((1, 384, dh, dw), generator=g).half().to(DEV)          # DINO features, coarser grid
    image = torch.rand((1, 3, 4 * h, 4 * w), generator=g).to(DEV)
    disps = (torch.rand((h, w), generator=g) * 0.75 + 0.25).to(DEV)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs.to(DEV), ys.to(DEV), disps])[None]               # coords_grid_with_index: (x, y, disparity)
    coords = torch.stack([torch.rand(M, generator=g) * (w + 4) - 2, torch.rand(M, generator=g) * (h + 4) - 2], -1)[None].to(DEV)
    s_f2i = torch.tensor([float(dw) / w, float(dh) / h], device=DEV)           # (x, y) scale feature grid -> DINO grid
    for imode in ("bilinear", "upperleft"):
        want = [altcorr.patchify(imap, s_f2i * coords, 0, mode=imode), altcorr.patchify(fmap, coords, 1),
                altcorr.patchify(image, 4 * (coords + 0.5), 0), altcorr.patchify(grid, coords, 1)]
        got = ops.patchify_multi([dict(net=imap, radius=0, mode=imode, scale=(float(dw) / w, float(dh) / h)),
                                  dict(net=fmap, radius=1), dict(net=image, radius=0, scale=4.0, offset=0.5),
                                  dict(net=grid, radius=1)], coords)
        for a, b in zip(got, want):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _loop_scene(n=90, M=16, seed=5):
    """a camera going round a circle of 60 frames: frame t sees again what frame t - 60 saw"""
    rng = np.random.default_rng(seed)
    N = n + 6
    ang = 2 * np.pi * np.arange(N) / 60.0
    poses = np.zeros((N, 7), np.float32); poses[:, 6] = 1
    poses[:, 0] = 0.5 * np.cos(ang) + rng.normal(0, 0.01, N)
    poses[:, 1] = 0.5 * np.sin(ang) + rng.normal(0, 0.01, N)
    poses[:, 2] = rng.normal(0, 0.01, N)
    h, w = 96, 128
    cx, cy = rng.uniform(8, w - 8, N * M), rng.uniform(8, h - 8, N * M)
    patches = np.zeros((N * M, 3, 3, 3), np.float32)
    off = np.arange(3.0) - 1
    patches[:, 0] = cx[:, None, None] + off[None, None, :]
    patches[:, 1] = cy[:, None, None] + off[None, :, None]
    patches[:, 2] = rng.uniform(0.25, 1.0, N * M)[:, None, None]
    for f in (10, 25, 41):   # three source frames far along +z: their points fall behind the recent cameras (Z < 0.2)
        poses[f, 2] = 3.0
    intr = np.tile(np.array([64, 64, 64, 48], np.float32), (N, 1))
    ix = np.repeat(np.arange(N), M)
    return poses, patches, intr, ix, n, M


def test_edges_loop_vs_the_reference_composition():
    """cdv_loop_flow + loop.edges_loop (PatchGraph.edges_loop, patchgraph.py:71-97) against the reference's own sequence
    of operations -- flatmeshgrid candidates, pops.flow_mag on the patch centres, reductions over groups of M,
    reduce_edges -- built from the operator surface: same per-pair flow (summation order apart), same inf pattern,
    same chosen edges"""
    from cdv_slam_amd import loop, projective_ops as pops
    from cdv_slam_amd.lietorch import SE3
    poses, patches, intr, ix, n, M = _loop_scene()
    tp, tpa, ti, tix = T(poses), T(patches), T(intr), T(ix)
    RW, AGE, GOF, KI, TH = 22, 1000, 15, 4, 64.0
    l = n - RW
    jr = torch.arange(n - GOF, n - KI, device=DEV)
    kr = torch.arange(max(l - AGE, 0) * M, l * M, device=DEV)
    jj, kk = [t.reshape(-1) for t in torch.meshgrid(jr, kr, indexing="ij")]
    ii = tix[kk]
    fm, val = pops.flow_mag(SE3(tp[None]), tpa[None][..., 1, 1].reshape(1, -1, 3, 1, 1), ti[None], ii, jj, kk, beta=0.5)
    fsum = (fm * val).reshape(-1, M).sum(1).float()
    nval = val.reshape(-1, M).sum(1).clamp(min=1)
    want = torch.where(nval > M * 0.75, fsum / nval, torch.full_like(fsum, float("inf")))
    got = loop.loop_flow(tp, tpa, ti, tix, M, n - GOF, GOF - KI, max(l - AGE, 0), l - max(l - AGE, 0), 0.5).reshape(-1)
    inf_w, inf_g = torch.isinf(want), torch.isinf(got)
    assert torch.equal(inf_w, inf_g) and inf_w.any() and (~inf_w).any()
    assert torch.allclose(got[~inf_g], want[~inf_w], rtol=1e-5, atol=1e-4)
    mask = want < TH
    assert mask.any()
    es = loop.reduce_edges(want[mask].cpu().numpy(), ii[::M][mask].cpu().numpy(), jj[::M][mask].cpu().numpy(), 1000, 1)
    assert len(es) > 3 and (es[:, 1] - es[:, 0] >= 30).all()
    kk_g, jj_g = loop.edges_loop(tp, tpa, ti, tix, n, M, removal_window=RW, max_edge_age=AGE, global_opt_freq=GOF,
                                 keyframe_index=KI, backend_thresh=TH)
    want_kk = (torch.as_tensor(es[:, 0], device=DEV)[:, None] * M + torch.arange(M, device=DEV)[None]).reshape(-1)
    want_jj = torch.as_tensor(es[:, 1], device=DEV)[:, None].repeat(1, M).reshape(-1)
    assert torch.equal(kk_g, want_kk) and torch.equal(jj_g, want_jj)
    # nothing old enough yet: no edges
    k0, j0_ = loop.edges_loop(tp, tpa, ti, tix, 20, M)
    assert k0.numel() == 0 and j0_.numel() == 0


@pytest.mark.parametrize("name", ["default", "stress"])
def test_ate_against_the_oracle_trajectory(name):
    """the BASELINE metric's second half, in the only form available without the datasets: ATE-RMSE (Sim(3)-aligned, as
    evaluate_tartan.py:63-70) of the window's trajectory after the GPU update against the float64 oracle's trajectory
    from the same patch-graph state: within 1e-4"""
    from cdv_slam_amd import metrics
    from cdv_slam_amd.update import UpdatePath
    st = synth.make_state(name)
    up = UpdatePath(st, torch.device(DEV))
    up.step()
    torch.cuda.synchronize()
    p_o, x_o, _ = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj, st.kk,
                           st.t0, st.n, 2, np.float64)
    got = up.poses.cpu().numpy()
    lo = max(st.t0 - 12, 0)     # the free poses and the fixed ones before them (so that the alignment is well posed)
    ate = metrics.ate_rmse(p_o[lo:st.n], got[lo:st.n])
    moved = metrics.ate_rmse(st.poses[lo:st.n], got[lo:st.n])
    assert ate < 1e-4, ate
    assert moved > 10 * ate     # the update did move the trajectory by much more than the two disagree
    if name == "default":
        # ten more updates on both sides (bundle adjustment on the evolving state, fixed targets): no drift apart
        p, pat = p_o, x_o
        for _ in range(10):
            up.step()
            p, pat, _ = O.fastba(p, pat, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj, st.kk, st.t0, st.n,
                                 2, np.float64)
        torch.cuda.synchronize()
        assert metrics.ate_rmse(p[lo:st.n], up.poses.cpu().numpy()[lo:st.n]) < 1e-4


def test_single_pixel_patches():
    """P = 1 patches (the structure-only caller of the classic loop closure passes 1x1 patches, long_term.py:118-135):
    reprojection, BA and the fused helpers take the centre-pixel code path"""
    from cdv_slam_amd import projective_ops as pops
    from cdv_slam_amd.lietorch import SE3
    st = synth.make_state("small", features=False)
    p1 = np.ascontiguousarray(st.patches[:, :, 1:2, 1:2])
    coords = ops.transform(T(st.poses)[None], T(p1)[None], T(st.intrinsics)[None], T(st.ii), T(st.jj), T(st.kk))
    want = O.transform(st.poses, p1, st.intrinsics, st.ii, st.jj, st.kk)
    assert coords.shape == (1, st.E, 1, 1, 2) and np.abs(coords[0].cpu().numpy() - want).max() <= 1e-3
    poses, patches = T(st.poses).clone(), T(p1).clone()
    ops.ba_forward(poses, patches, T(st.intrinsics), T(st.target), T(st.weight), torch.tensor([st.lmbda], device=DEV),
                   T(st.ii), T(st.jj), T(st.kk), st.cfg.M, st.t0, st.n, 2, False)
    p64, x64, info = O.fastba(st.poses, p1, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj, st.kk, st.t0,
                              st.n, 2, np.float64)
    st1 = synth.make_state("small", features=False)
    st1.patches = p1
    ba_checks.check_end_state("small", st1, poses.cpu().numpy(), patches.cpu().numpy(), p64, x64)
    flow, val = pops.flow_mag(SE3(T(st.poses)[None]), T(p1)[None], T(st.intrinsics)[None], T(st.ii), T(st.jj), T(st.kk))
    assert flow.shape == (1, st.E, 1, 1) and bool(torch.isfinite(flow).all())


def test_ba_structure_only_and_gates():
    """t1 == t0 branch (ba_cuda.cu:550-560, caller long_term.py:124-125) and the depth clamps"""
    st = synth.make_state("small", features=False)
    # make some updates run into the gates: huge residuals (masked), very small depth
    st.target[::7] += 500.0
    st.patches[np.unique(st.kk)[::5], 2] = 1e-5
    poses, patches, _ = _run_ba(st, iterations=3, t0=st.n, t1=st.n)
    p64, x64, _ = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                           st.kk, st.n, st.n, 3, np.float64)
    assert np.array_equal(poses, st.poses)
    d, d64 = patches[:, 2, 0, 0], x64[:, 2, 0, 0]
    assert np.abs(d - d64).max() <= 2e-4 * np.maximum(np.abs(d64), 1e-2).max()
    assert d.min() >= 1e-4


def test_ba_window_is_bitwise_reproducible():
    """the slab paths (N <= 10: ba_win.hip, N <= 32: ba_mid.hip) sum everything in a fixed order: two runs give
    identical bits -- also when other kernels have run in between and when the workspace was used for another graph
    meanwhile"""
    for name in ("default", "pr1", "stress", "mid19_m5"):
        st, _ = _make(name)
        p1, x1, _ = _run_ba(st, iterations=2)
        other = synth.make_state("small", features=False)
        _run_ba(other, iterations=1)
        p2, x2, _ = _run_ba(st, iterations=2)
        assert np.array_equal(p1, p2) and np.array_equal(x1, x2), name
        assert not np.array_equal(p1, st.poses)


def test_ba_never_dereferences_unwritten_index_slots():
    """Regression for the round-2 abort ("the 11:36 abort"): the chunk-slot (ELL) copy of the edge
    records has 32 slots per patch and the index build writes only the first deg(patch) of them; the chunk kernels load
    all their first-round slots unconditionally and must replace what lies beyond a patch's degree BEFORE any field is used
    as an index (settle_rec).  Here the index and BA workspaces are filled with a poison pattern (huge positive ints /
    NaN-ish floats) before their first use, as a fresh allocation may be: the update must neither fault nor change."""
    for name, cap in (("default", None), ("init", None), ("stress", None), ("mid19_m5", None), ("default", 2304), ("stress", 4704)):
        st, _ = _make(name)
        g0 = ops.GraphIndex(torch.device(DEV), E_cap=st.E, k_range=st.cfg.buffer_size * st.cfg.M, table_capacity=cap)
        want_p, want_x, _ = _run_ba_on(st, g0)
        g = ops.GraphIndex(torch.device(DEV), E_cap=st.E, k_range=st.cfg.buffer_size * st.cfg.M, table_capacity=cap)
        g.ws.view(torch.int32).fill_(0x7F7F7F7F)
        lib = ops._lib.load()
        # whoever (re)allocates a workspace initialises it: the contract of cdv_graph_workspace_init
        ops._lib.check(lib.cdv_graph_workspace_init(ops._p(g.ws), g.ws_bytes, g.E_cap, g.k_range, ops._stream()), "init")
        dev = torch.device(DEV)
        ws = ops._ba_workspace(dev, st.E, max(min(st.E, len(st.patches)), cap or 0), st.n - st.t0)   # the one ba_forward picks up
        ws.fill_(0x7F)
        ops._lib.check(lib.cdv_ba_workspace_init(ops._p(ws), ops._stream()), "init")   # as after a fresh allocation
        ops._ba_bound.pop(ws.data_ptr(), None)      # ... and binds its event counters (ba_forward does, for the index it is given)
        poses, patches = T(st.poses).clone(), T(st.patches).clone()
        ops.ba_forward(poses, patches, T(st.intrinsics), T(st.target), T(st.weight), torch.tensor([st.lmbda], device=DEV),
                       T(st.ii), T(st.jj), T(st.kk), st.cfg.M, st.t0, st.n, 2, False, graph=g)
        torch.cuda.synchronize()
        assert ops.ba_status(raise_on_error=False) == (0, 0, 0, 0), name
        assert np.array_equal(poses.cpu().numpy(), want_p) and np.array_equal(patches.cpu().numpy(), want_x), name


@pytest.mark.parametrize("variant", ["small", "mid15", "mid19_m5"])
def test_ba_window_irregular_graph(variant):
    """edge lists the front-end never builds but the API admits: a random third of the edges dropped (ragged patch
    degrees, chunks whose lanes belong to different frame pairs), the edge order shuffled, a few DUPLICATED edges and a
    few self edges (i == j) of free frames; on the N <= 10 and on the N <= 32 path.  Duplicated edges and patches with two
    source frames are the cases that sum through LDS float atomics (arrival order: include/cdvslam_hip.h says so): held to the
    stated tolerances against the float64 oracle, NOT bit for bit"""
    st, _ = _make(variant)
    rng = np.random.default_rng(17)
    keep = rng.random(st.E) > 0.33
    sel = np.flatnonzero(keep)
    sel = np.concatenate([sel, sel[rng.integers(0, len(sel), 40)]])      # duplicates
    rng.shuffle(sel)
    st.ii, st.jj, st.kk = st.ii[sel].copy(), st.jj[sel].copy(), st.kk[sel].copy()
    st.target, st.weight = st.target[sel].copy(), st.weight[sel].copy()
    assert (st.ii == st.jj).any() and ((st.ii == st.jj) & (st.ii >= st.t0)).any()
    _, _, dbg = _run_ba(st, iterations=1, debug=True)
    _, _, info, o = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                             st.kk, st.t0, st.n, 1, np.float64, debug=True)
    U = len(o["kx"])
    for key, got, want in (("S", dbg["S"], o["S"]), ("y", dbg["y"], o["y"]), ("C", dbg["C"][:U], o["C"]),
                           ("u", dbg["u"][:U], o["u"]), ("E", dbg["E"][:, :U], o["E"])):
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max(), key
    poses, patches, _ = _run_ba(st, iterations=2)
    p64, x64, _ = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj, st.kk,
                           st.t0, st.n, 2, np.float64)
    ba_checks.check_end_state("small", st, poses, patches, p64, x64)


@pytest.mark.parametrize("name,mode", [("default", 1), ("default", 2), ("stress", 1), ("stress", 2), ("global", 1), ("global", 2), ("global", 3)])
def test_ba_handoff_is_all_or_nothing(name, mode):
    """The solve -> retract hand-off inside a finish launch, with faults injected (cdv_ba_test_handoff): mode 1 -- the solver
    stalls before its commit (N <= 32: the retract workgroups run out of patience, decide ABANDONED, the solver publishes
    nothing) / the global back substitution withholds a block: the hand-off word is set, the event is counted, and poses
    and patches are BIT-IDENTICAL to the input -- in every workgroup, not in some.  mode 2 -- the solver stalls after its
    commit: the retract workgroups lose patience, learn that the solution is coming, wait on; the result is the undisturbed
    one bit for bit.  mode 3 (global path) -- a diagonal block of the one-launch factorisation never raises its flag: every
    workgroup that needs it gives up, the launch drains, nothing is applied.  Afterwards the workspace works as if nothing
    had happened."""
    from cdv_slam_amd import _lib
    lib = _lib.load()
    st = synth.make_state(name, features=False)
    dev = torch.device(DEV)
    g = ops.GraphIndex(dev, E_cap=st.E, k_range=st.cfg.buffer_size * st.cfg.M)
    call = lambda po, pa: ops.ba_forward(po, pa, T(st.intrinsics), T(st.target), T(st.weight), torch.tensor([st.lmbda], device=DEV),
                                         T(st.ii), T(st.jj), T(st.kk), st.cfg.M, st.t0, st.n, 2, name == "global", graph=g)
    want_p, want_x = T(st.poses).clone(), T(st.patches).clone()
    call(want_p, want_x)
    torch.cuda.synchronize()
    assert ops.ba_status(dev) == (0, 0, 0, 0) and not torch.equal(want_p, T(st.poses))
    before = ops.ba_event_counts(dev)
    os.environ["CDV_CHECK"] = "0"
    try:
        assert lib.cdv_ba_test_handoff(mode) == 0
        poses, patches = T(st.poses).clone(), T(st.patches).clone()
        call(poses, patches)
        torch.cuda.synchronize()
        info = ops.ba_status(dev, raise_on_error=False)
        if mode in (1, 3):
            assert info[2] == 1, info
            assert torch.equal(poses, T(st.poses)) and torch.equal(patches, T(st.patches))       # nothing applied, anywhere
            assert ops.ba_event_counts(dev)[2] > before[2]
            with pytest.raises(_lib.CdvError, match="hand-off"):
                ops.ba_status(dev)
        else:
            assert info == (0, 0, 0, 0), info
            assert torch.equal(poses, want_p) and torch.equal(patches, want_x)
    finally:
        lib.cdv_ba_test_handoff(0)
        os.environ["CDV_CHECK"] = "1"
    poses, patches = T(st.poses).clone(), T(st.patches).clone()
    call(poses, patches)
    torch.cuda.synchronize()
    assert ops.ba_status(dev) == (0, 0, 0, 0)
    assert torch.equal(poses, want_p) and torch.equal(patches, want_x)


def test_ba_status_is_reported():
    """the failure words of the BA launches reach the caller (the reference ignores cholesky_ex's info, ba_cuda.cu:576,590,
    and exits on capacity errors, block_e.cu:20-27): U_max too small -> the update is skipped and says so; a system that
    is not positive definite -> said so; the next well-formed call on the same workspace works"""
    from cdv_slam_amd import _lib
    st = synth.make_state("small", features=False)
    dev = torch.device(DEV)
    args = lambda po, pa, w: (po, pa, T(st.intrinsics), T(st.target), w, torch.tensor([st.lmbda], device=DEV), T(st.ii),
                              T(st.jj), T(st.kk), st.cfg.M, st.t0, st.n, 2, False)
    poses, patches = T(st.poses).clone(), T(st.patches).clone()
    before = ops.ba_event_counts(dev)
    os.environ["CDV_CHECK"] = "0"
    try:
        # 1. U_max smaller than the number of unique patches
        ops.ba_forward(*args(poses, patches, T(st.weight)), U_max=8)
        torch.cuda.synchronize()
        assert torch.equal(poses, T(st.poses)) and torch.equal(patches, T(st.patches))      # skipped, not garbage
        info = ops.ba_status(dev, raise_on_error=False)
        assert info[1] == 1 and info[0] == 0
        with pytest.raises(_lib.CdvError, match="U_max"):
            ops.ba_status(dev)
        assert ops.ba_event_counts(dev)[1] == before[1] + 2                                 # one event per iteration
        os.environ["CDV_CHECK"] = "1"
        with pytest.raises(_lib.CdvError, match="U_max"):
            ops.ba_forward(*args(poses, patches, T(st.weight)), U_max=8)
        os.environ["CDV_CHECK"] = "0"
        # 2. negative weights: B is negative definite, the damped system has negative pivots
        ops.ba_forward(*args(poses.clone(), patches.clone(), -100.0 * T(st.weight)))
        info = ops.ba_status(dev, raise_on_error=False)
        assert info[0] != 0 and info[1] == 0
        with pytest.raises(_lib.CdvError, match="positive definite"):
            ops.ba_status(dev)
        assert ops.ba_event_counts(dev)[0] > before[0]
        # 3. the workspace recovers by itself
        ops.ba_forward(*args(poses, patches, T(st.weight)))
        assert ops.ba_status(dev) == (0, 0, 0, 0)
        p64, x64, _ = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                               st.kk, st.t0, st.n, 2, np.float64)
        ba_checks.check_end_state("small", st, poses.cpu().numpy(), patches.cpu().numpy(), p64, x64)
        # 4. a graph whose patch ids exceed the index capacity: neighbors say "none", BA is skipped and says so
        g = ops.GraphIndex(dev, E_cap=st.E, k_range=8)
        g.build(T(st.jj), T(st.kk), with_neighbors=True)
        ix, jx = g.neighbors()
        assert bool((ix == -1).all()) and bool((jx == -1).all())
        ops.ba_forward(*args(poses.clone(), patches.clone(), T(st.weight)), graph=g)
        assert ops.ba_status(dev, raise_on_error=False)[3] == 1
        with pytest.raises(_lib.CdvError, match="range"):
            ops.ba_status(dev)
    finally:
        os.environ["CDV_CHECK"] = "1"


@pytest.mark.parametrize("M", [8, 12, 16, 20])
def test_ba_mid_path_on_a_table_with_few_patches_per_frame(M):
    """10 < N <= 32 on a patch TABLE whose capacity is a multiple of the patches per frame, with cuda_ba.forward's PPF passed
    on: frames of 8 and 12 patches must NOT be cut per frame (a frame would be a workgroup and a slab of its own: more slabs
    than the workspace holds -- the round-4 advisor's out-of-bounds write), 16 and 20 may.  Either way: the ranked index's
    result to rounding, the float64 oracle's within the stated bounds, clean status, and the bytes behind the workspace's
    slab area untouched."""
    st = synth.make_state("small", features=False, opt_window=15, M=M)
    dev = torch.device(DEV)
    N = st.n - st.t0
    assert 10 < N <= 32
    cap = (st.cfg.removal_window + 2) * M
    gt = ops.GraphIndex(dev, E_cap=st.E, k_range=st.cfg.buffer_size * M, table_capacity=cap)
    gr = ops.GraphIndex(dev, E_cap=st.E, k_range=st.cfg.buffer_size * M)
    pt, xt, _ = _run_ba_on(st, gt)
    assert gt.is_table
    assert ops.ba_status(dev) == (0, 0, 0, 0)
    pr, xr, _ = _run_ba_on(st, gr)
    assert not gr.is_table
    assert np.abs(pt - pr).max() <= 5e-6 and np.abs(xt - xr).max() <= 5e-5
    p64, x64, _ = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj, st.kk,
                           st.t0, st.n, 2, np.float64)
    ba_checks.check_end_state("small", st, pt, xt, p64, x64)
    assert gt.events.counts() == [0, 0, 0, 0]


def test_events_are_counted_per_index_and_cost_nobody_else_their_table():
    """Failure events belong to the index the bundle adjustment ran over (GraphIndex.events), not to the device: an index whose
    table is too small for its ids counts graph-range events on ITS block, gives ITS table up at its next call and goes on
    ranked -- while an UpdatePath on the same device keeps its table and keeps stepping.  (Round 4: per-device counters; the
    stream runner's events took the headline path's table away.)  And an UpdatePath whose OWN table fails falls back to the
    ranked prologue instead of asking for a table of capacity 0."""
    from cdv_slam_amd.update import UpdatePath
    st = synth.make_state("small")
    dev = torch.device(DEV)
    up = UpdatePath(st, dev)
    up.step()
    torch.cuda.synchronize()
    cap = up.graph.table_capacity
    assert up.graph.is_table and cap > 0
    call = lambda g: ops.ba_forward(T(st.poses).clone(), T(st.patches).clone(), T(st.intrinsics), T(st.target), T(st.weight),
                                    torch.tensor([st.lmbda], device=DEV), T(st.ii), T(st.jj), T(st.kk), st.cfg.M, st.t0, st.n,
                                    2, False, graph=g)
    other = ops.GraphIndex(dev, E_cap=st.E, k_range=st.cfg.buffer_size * st.cfg.M, table_capacity=8)
    os.environ["CDV_CHECK"] = "0"
    try:
        call(other)
        torch.cuda.synchronize()
        assert other.is_table and other.events.counts()[3] == 2          # one per iteration, on ITS block
        assert up.graph.events.counts() == [0, 0, 0, 0]
        before = up.poses.clone()
        out = up.step()
        torch.cuda.synchronize()
        assert up.graph.table_capacity == cap and up.graph.is_table      # untouched by the neighbour's trouble
        assert not torch.equal(up.poses, before) and bool((out["ix"] >= -1).all())
        with pytest.warns(RuntimeWarning, match="falling back to the ranked index"):
            call(other)
        torch.cuda.synchronize()
        assert other.table_capacity == 0 and not other.is_table
        assert other.events.counts()[3] == 2                             # the ranked index holds the ids: no new event
        # an UpdatePath whose own table is too small: first update skipped and counted, then on with the ranked index
        up2 = UpdatePath(st, dev)
        up2.graph.table_capacity = 8
        start = up2.poses.clone()
        up2.step()
        torch.cuda.synchronize()
        assert torch.equal(up2.poses, start) and up2.graph.events.counts()[3] == 2
        with pytest.warns(RuntimeWarning, match="falling back to the ranked index"):
            up2.step()
        out2 = up2.step()
        torch.cuda.synchronize()
        assert up2.graph.table_capacity == 0 and not up2.graph.is_table
        assert not torch.equal(up2.poses, start) and up2.graph.events.counts()[3] == 2      # no event since the fallback
        ix_o, jx_o = O.neighbors(st.kk, st.jj)
        assert np.array_equal(out2["ix"].cpu().numpy(), ix_o) and np.array_equal(out2["jx"].cpu().numpy(), jx_o)
        assert ops.ba_event_counts(dev)[3] >= 4                          # the device total is the sum over the blocks
    finally:
        os.environ["CDV_CHECK"] = "1"


def test_ba_dropin_inplace_contract():
    """fastba.BA(poses view of the state buffer, ...) mutates the buffers in place and returns []"""
    from cdv_slam_amd import fastba
    from cdv_slam_amd.lietorch import SE3
    st = synth.make_state("small", features=False)
    poses_ = T(st.poses).clone()
    patches_ = T(st.patches).clone()
    N, M = st.cfg.buffer_size, st.cfg.M
    res = fastba.BA(SE3(poses_.view(1, N, 7)), patches_.view(1, N * M, 3, 3, 3), T(st.intrinsics).view(1, N, 4),
                    T(st.target)[None], T(st.weight)[None], torch.as_tensor([1e-4], device=DEV), T(st.ii), T(st.jj),
                    T(st.kk), st.t0, st.n, M=M, iterations=2, eff_impl=False)
    assert res == []
    torch.cuda.synchronize()
    assert not torch.equal(poses_, T(st.poses))
    p64, _, _ = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj, st.kk,
                         st.t0, st.n, 2, np.float64)
    assert np.abs(poses_.cpu().numpy() - p64).max() < 1e-4


def test_update_path_end_to_end():
    import __graft_entry__ as ge
    ge.smoke()


def test_global_ba_is_bitwise_reproducible():
    """more than 32 free poses: every sum has one owner and a fixed order here too (patch owners for E, C, u; frame-pair
    owners for B, v; pose owners for the diagonal blocks; tile owners for the Schur products) -- two runs, the same bits"""
    st = synth.make_state("global", features=False)
    assert st.n - st.t0 > 32
    a = _run_ba(st, iterations=2)
    b = _run_ba(st, iterations=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _, _, d1 = _run_ba(st, iterations=1, debug=True)
    _, _, d2 = _run_ba(st, iterations=1, debug=True)
    for key in ("S", "y", "dX", "E", "C", "u"):
        assert torch.equal(d1[key], d2[key]), key


def test_global_ba_irregular_graph():
    """more than 32 free poses on edge lists the front-end never builds but the API admits: a third of the edges dropped,
    the order shuffled, duplicated edges (the same patch to the same target frame twice: neighbours in the patch's list),
    self edges (i == j), and patches whose edges name TWO source frames (the patch owner of E switches its lane to
    read-modify-writes; the pair index simply files the edge under another pair) -- intermediates against the float64
    oracle, and the same bits from run to run"""
    st = synth.make_state("global", features=False)
    N = st.n - st.t0
    assert N > 32
    rng = np.random.default_rng(23)
    sel = np.flatnonzero(rng.random(st.E) > 0.33)
    sel = np.concatenate([sel, sel[rng.integers(0, len(sel), 60)]])      # duplicates
    rng.shuffle(sel)
    st.ii, st.jj, st.kk = st.ii[sel].copy(), st.jj[sel].copy(), st.kk[sel].copy()
    st.target, st.weight = st.target[sel].copy(), st.weight[sel].copy()
    # self edges of free frames, and a second source frame for some edges (free and fixed ones)
    pick = rng.choice(len(sel), 80, replace=False)
    st.jj[pick[:30]] = st.ii[pick[:30]]
    st.ii[pick[30:70]] = rng.integers(st.t0, st.n, 40)
    st.ii[pick[70:]] = rng.integers(0, max(st.t0, 1), 10)
    assert ((st.ii == st.jj) & (st.ii >= st.t0)).any()
    _, _, dbg = _run_ba(st, iterations=1, debug=True)
    _, _, info, o = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                             st.kk, st.t0, st.n, 1, np.float64, debug=True)
    assert info == 0
    U = len(o["kx"])
    S = np.tril(dbg["S"].cpu().numpy())
    assert np.abs(S - np.tril(o["S"])).max() <= 1e-4 * np.abs(o["S"]).max()
    for key, got, want in (("y", dbg["y"], o["y"]), ("C", dbg["C"][:U], o["C"]), ("u", dbg["u"][:U], o["u"]),
                           ("E", dbg["E"][:, :U], o["E"])):
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max(), key
    _, _, dbg2 = _run_ba(st, iterations=1, debug=True)
    for key in ("S", "y", "dX", "E", "C", "u"):
        assert torch.equal(dbg[key], dbg2[key]), key
    a = _run_ba(st, iterations=2)
    b = _run_ba(st, iterations=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()


# ---------------------------------------------------------------------------------------------------
# size-independent properties at the benchmark sizes (no oracle run needed: they hold bit for bit)
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["default", "stress"])
def test_corr_properties_at_benchmark_size(name):
    """linearity and equivariance of the fused correlation on the benchmark workloads (E = 47,712 / 97,412).
    (1) Doubling every feature map doubles every output: products and sums scale by a power of two without rounding
    (f16 storage, f32 accumulation, f16 raw volume, bilinear blend), except where a value passes through half precision's
    SUBNORMAL range, whose spacing (6e-8) is absolute -- so: equal to within one unit in the last place + two subnormal
    steps, and bit for bit on more than 99 % of the outputs; any dropped or doubly counted term breaks it.  (2) Permuting the edge list permutes the output rows, bit for bit -- through the index-independent direct call
    and with the processing order of a permuted list's own index.  (3) A patch tile of zeros gives zeros."""
    from cdv_slam_amd.update import UpdatePath
    st = synth.make_state(name)
    up = UpdatePath(st, torch.device(DEV))
    coords = _gpu_coords(st)
    base = ops.corr_fused(up.gmap, up.fmap1, up.fmap2, coords, up.kk, up.jj, kmod=up.kmod, jmod=up.jmod)
    torch.cuda.synchronize()
    assert base.shape == (1, st.E, 882) and bool(torch.isfinite(base.float()).all())
    assert float(base.float().abs().max()) < 2.0 ** 14          # doubling stays inside half precision
    # (1) linearity in the maps
    twice = ops.corr_fused(up.gmap, up.fmap1 * 2, up.fmap2 * 2, coords, up.kk, up.jj, kmod=up.kmod, jmod=up.jmod)
    def doubled(t):
        want = (base * 2).float()
        diff = (t.float() - want).abs()
        assert bool((diff <= want.abs() * 2.0 ** -10 + 2.4e-7).all())
        assert float((diff == 0).float().mean()) > 0.99
    doubled(twice)
    # ... and in the patch tiles
    doubled(ops.corr_fused(up.gmap * 2, up.fmap1, up.fmap2, coords, up.kk, up.jj, kmod=up.kmod, jmod=up.jmod))
    # (2) edge permutation
    perm = torch.randperm(st.E, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    pc, pk, pj = coords[:, perm].contiguous(), up.kk[perm].contiguous(), up.jj[perm].contiguous()
    permuted = ops.corr_fused(up.gmap, up.fmap1, up.fmap2, pc, pk, pj, kmod=up.kmod, jmod=up.jmod)
    assert torch.equal(permuted, base[:, perm])
    g = ops.GraphIndex(torch.device(DEV), E_cap=st.E, k_range=len(st.patches))
    g.build(pj, pk, force=True)
    ordered = ops.corr_fused(up.gmap, up.fmap1, up.fmap2, pc, pk, pj, kmod=up.kmod, jmod=up.jmod,
                             order_ptr=g.corr_order_ptr())
    assert torch.equal(ordered, base[:, perm])
    # (3) zero tiles
    zeros = ops.corr_fused(torch.zeros_like(up.gmap), up.fmap1, up.fmap2, coords, up.kk, up.jj, kmod=up.kmod, jmod=up.jmod)
    assert float(zeros.float().abs().max()) == 0.0


@pytest.mark.parametrize("name", ["default", "stress", "global"])
def test_ba_with_zero_weights_changes_nothing(name):
    """a bundle adjustment whose residuals all carry weight zero has B = 0, v = 0, E = 0, u = 0: the damped system is
    the identity with a zero right-hand side, dX = 0, dZ = 0 -- poses and patches must come back BIT FOR BIT (Exp(0) T = T,
    d + 0 = d), on all three paths (10, 22 and 79 free poses) at their full sizes; the status words stay clear"""
    st = synth.make_state(name, features=False)
    st.weight = np.zeros_like(st.weight)
    assert st.patches[np.unique(st.kk), 2].max() < 20.0 and st.patches[np.unique(st.kk), 2].min() > 1e-4   # no clamp fires
    poses, patches, _ = _run_ba(st, iterations=2)
    assert np.array_equal(poses, st.poses)
    assert np.array_equal(patches, st.patches)
    assert ops.ba_status(torch.device(DEV)) == (0, 0, 0, 0)


@pytest.mark.parametrize("iterations", [1, 2])
def test_update_captured_as_a_hipgraph_replays_bit_for_bit(iterations):
    """a whole update -- ring ingest, table build, reprojection, two-level correlation, neighbors, BA -- captured into a
    hipGraph (every entry point only enqueues on the given stream) and replayed: the same bits as the eager launches, replay
    after replay.  The hand-off tags between the BA's launches are per-launch tokens taken from host state when a call is
    enqueued, so a replay carries the tokens of the capture: each iteration's first launch therefore clears the tags of the
    launch that follows (an odd number of iterations per call would otherwise meet its own tags from the replay before)."""
    from cdv_slam_amd.update import UpdatePath
    st = synth.make_state("small")
    dev = torch.device(DEV)

    def run(up, stepper, n):
        outs = []
        up.reset()
        for _ in range(n):
            r = stepper()
            torch.cuda.synchronize()
            outs.append((up.poses.clone(), up.patches.clone(), r["corr"].clone(), r["ix"].clone(), r["jx"].clone()))
        return outs

    eager = UpdatePath(st, dev)
    want = run(eager, lambda: eager.step(iterations=iterations), 3)
    cap = UpdatePath(st, dev)
    for _ in range(3):
        cap.step(iterations=iterations)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    os.environ["CDV_CHECK"] = "0"      # (CDV_CHECK=1 reads the status words back after every BA: a synchronisation, not capturable)
    try:
        with torch.cuda.graph(g):
            held = cap.step(iterations=iterations)
    finally:
        os.environ["CDV_CHECK"] = "1"
    torch.cuda.synchronize()

    def replay():
        g.replay()
        return held
    got = run(cap, replay, 3)
    for a, b in zip(want, got):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert ops.ba_status(dev) == (0, 0, 0, 0)


def test_global_ba_captured_as_a_hipgraph_replays_bit_for_bit():
    """cdv_ba_forward on the GLOBAL path (79 free poses: pair index, Schur products, one-launch factorisation, back
    substitution with in-launch hand-offs) captured into a hipGraph and replayed: the eager calls' bits, replay after replay,
    status clean.  Round 4's replays died with a GPU memory fault at the second replay: the call enqueued a hipMemsetAsync
    (the (a, b) -> pair table), which becomes a memset NODE whose replay is not the eager memset's (found by replaying
    prefixes of the call: the fault appears with the first kernel that reads the table, and goes when a kernel does the
    zeroing).  The library now enqueues kernels only.  Also captured here: a FIRST call on a fresh workspace (its one-time
    initialisation is part of the graph then, and harmless to replay)."""
    st = synth.make_state("global", features=False)
    dev = torch.device(DEV)
    assert st.n - st.t0 > 32
    args = (T(st.intrinsics), T(st.target), T(st.weight), torch.tensor([st.lmbda], device=DEV), T(st.ii), T(st.jj), T(st.kk))

    def run(stepper, poses, patches, n):
        outs = []
        for _ in range(n):
            poses.copy_(T(st.poses)); patches.copy_(T(st.patches))
            stepper()
            torch.cuda.synchronize()
            outs.append((poses.clone(), patches.clone()))
        return outs

    g = ops.GraphIndex(dev, E_cap=st.E, k_range=st.cfg.buffer_size * st.cfg.M)
    pe, xe = T(st.poses).clone(), T(st.patches).clone()
    want = run(lambda: ops.ba_forward(pe, xe, *args, st.cfg.M, st.t0, st.n, 2, True, graph=g), pe, xe, 2)
    assert torch.equal(want[0][0], want[1][0]) and not torch.equal(want[0][0], T(st.poses))
    os.environ["CDV_CHECK"] = "0"      # (CDV_CHECK=1 reads the status words back after every BA: not capturable)
    try:
        for warm in (2, 0):            # captured after two eager calls / as the very first call on a fresh BA workspace
            if warm == 0:
                ops._ba_ws.pop(dev, None)
            pc, xc = T(st.poses).clone(), T(st.patches).clone()
            gi = ops.GraphIndex(dev, E_cap=st.E, k_range=st.cfg.buffer_size * st.cfg.M)
            gi.build(args[5], args[6], ii=args[4])
            call = lambda: ops.ba_forward(pc, xc, *args, st.cfg.M, st.t0, st.n, 2, True, graph=gi)
            for _ in range(warm):
                call()
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                call()
            torch.cuda.synchronize()
            got = run(cg.replay, pc, xc, 4)
            for a, b in got:
                assert torch.equal(a, want[0][0]) and torch.equal(b, want[0][1]), warm
            assert ops.ba_status(dev) == (0, 0, 0, 0)
            assert gi.events.counts() == [0, 0, 0, 0]
    finally:
        os.environ["CDV_CHECK"] = "1"


def test_global_path_just_above_the_mid_path():
    """35 free poses -- the smallest systems the global path serves (the mid path ends at 32): five 8-pose panels with a
    ragged last one, a 210-unknown system padded to four 64-blocks.  Intermediates against the float64 oracle, the solve's
    backward error, the same bits from run to run."""
    st = synth.make_state("small", features=False, frames=40, opt_window=35, removal_window=40, buffer_size=48)
    N = st.n - st.t0
    assert 32 < N < 40
    _, _, dbg = _run_ba(st, iterations=1, debug=True)
    _, _, info, o = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj,
                             st.kk, st.t0, st.n, 1, np.float64, debug=True)
    assert info == 0
    U = len(o["kx"])
    S = np.tril(dbg["S"].cpu().numpy())
    assert np.abs(S - np.tril(o["S"])).max() <= 1e-4 * np.abs(o["S"]).max()
    for key, got, want in (("y", dbg["y"], o["y"]), ("C", dbg["C"][:U], o["C"]), ("u", dbg["u"][:U], o["u"]),
                           ("E", dbg["E"][:, :U], o["E"])):
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max(), key
    # the kernel's own solve: S dX = y to float32 accuracy (S symmetric from its lower triangle)
    Sg = dbg["S"].cpu().numpy().astype(np.float64)
    Sg = np.tril(Sg) + np.tril(Sg, -1).T
    dX = dbg["dX"].cpu().numpy().astype(np.float64).reshape(-1)
    y = dbg["y"].cpu().numpy().astype(np.float64)
    assert np.linalg.norm(Sg @ dX - y) <= 2e-5 * (np.linalg.norm(Sg, 2) * np.linalg.norm(dX) + np.linalg.norm(y))
    _, _, dbg2 = _run_ba(st, iterations=1, debug=True)
    for key in ("S", "y", "dX", "E", "C", "u"):
        assert torch.equal(dbg[key], dbg2[key]), key
    a, b = _run_ba(st, iterations=2), _run_ba(st, iterations=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert ops.ba_status(torch.device(DEV)) == (0, 0, 0, 0)
