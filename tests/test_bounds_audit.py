"""Guard-band audit of the static entry points of include/cdvslam_hip.h (tests/guard_arena.py): every tensor of a call is
carved out of one buffer, flush between two guard bands; after the call (a) every guard byte is intact, (b) the outputs of a
NaN-guarded and a zero-guarded run are bit-identical, (c) the result meets the reference and the tolerance of the entry
point's parity test, (d) it equals the ops.* wrapper's ordinary call bit for bit.  Sizes are the tails of each kernel's own
launch geometry (the constant is named next to each list); index arguments aim at element 0 and at the LAST element of
every indexed array, which ends at its guard.  Small launches only.

AUDITED / EXEMPT are the coverage table tests/test_guard_arena_cpu.py holds against the header."""
import ctypes

import numpy as np
import pytest
import torch

from cdv_slam_amd import _lib, ops
from oracle import oracle as O
from oracle.edges_py import EdgesPy
from tests import guard_arena as GA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32, I64, I32, U8 = torch.float16, torch.float32, torch.int64, torch.int32, torch.uint8
PADX, PADY = ops.FMAP_PADX, ops.FMAP_PADY

AUDITED = {
    "cdv_lie_op": "test_lie_op",
    "cdv_transform": "test_transform", "cdv_fastba_reproject": "test_fastba_reproject", "cdv_flow_mag": "test_flow_mag",
    "cdv_point_cloud": "test_point_cloud", "cdv_loop_flow": "test_loop_flow",
    "cdv_gmap_to_pixel_major": "test_gmap_to_pixel_major", "cdv_fmap_to_nhwc": "test_fmap_to_nhwc",
    "cdv_fmap_ingest": "test_ingest", "cdv_frame_ingest": "test_ingest",
    "cdv_fmap_sync_nhwc": "test_shadow_sync", "cdv_shadows_sync": "test_shadow_sync",
    "cdv_corr_fwd": "test_corr_fwd", "cdv_corr_fused": "test_corr_fused",
    "cdv_corr_level_checked_interleaved": "test_corr_level_checked", "cdv_corr_fused_stream": "test_prologue_table_and_corr_stream",
    "cdv_patchify_fwd": "test_patchify", "cdv_patchify_blend": "test_patchify", "cdv_patchify_multi": "test_patchify_multi",
    "cdv_corr_bwd": "test_corr_bwd", "cdv_patchify_bwd": "test_patchify_bwd",
    "cdv_graph_build": "test_graph_ranked", "cdv_graph_build_edges": "test_graph_ranked", "cdv_graph_get_unique": "test_graph_ranked",
    "cdv_neighbors": "test_graph_ranked", "cdv_graph_build_table": "test_graph_table",
    "cdv_update_prologue": "test_prologue_ranked", "cdv_update_prologue_table": "test_prologue_table_and_corr_stream",
    "cdv_edges_frame": "test_edges_frame_append", "cdv_edges_append": "test_edges_frame_append", "cdv_edges_remove": "test_edges_remove",
    "cdv_edges_keyframe_shift": "test_keyframe_shifts", "cdv_frames_keyframe_shift": "test_keyframe_shifts",
    "cdv_ba_forward": "test_ba_forward",
}
_HOST = "host-only call: no device memory is written"
_STREAM = "device-stream family: tests/stream_audit.py audits it at every frame"
EXEMPT = {
    "cdv_graph_workspace_init": "workspace_init call: zeroes the workspace the graph audits size exactly and guard",
    "cdv_ba_workspace_init": "workspace_init call: host bookkeeping, the workspace is guarded in test_ba_forward",
    "cdv_ba_bind_status_counters": "bind call: " + _HOST, "cdv_ba_set_patches_per_frame": "set call: " + _HOST,
    "cdv_graph_bind_corr_stream": "bind call: " + _HOST, "cdv_stream_motion": "pointer getter: " + _HOST,
    "cdv_graph_table_offsets": "query: out7 is a host array; " + _HOST,
    "cdv_ba_factor_ticket": "test hook: out is a host array; " + _HOST,
    "cdv_update_prologue_table_dyn": _STREAM, "cdv_corr_fused_stream_dyn": _STREAM, "cdv_ba_forward_dyn": _STREAM,
    "cdv_stream_frame_begin": _STREAM, "cdv_stream_operator_stub": _STREAM, "cdv_stream_points": _STREAM,
    "cdv_stream_keyframe": _STREAM, "cdv_stream_frame": _STREAM,
}

# tail sizes by launch geometry
N256 = [1, 255, 256, 257, 1009]          # one lane per row / edge, 256 lanes per workgroup (lie.hip, edges.hip, graph.hip, prologue.hip)
N64 = [1, 63, 64, 65, 129, 1009]         # reproject.hip: `threads = 64`, one lane per edge
E_FUSED = [1, 3, 4, 5, 31, 32, 33, 257, 1009]    # corr.hip: CW = 4 edge-waves per workgroup, 8 * ceil(E / (8 * CW)) workgroups


def lib():
    return _lib.load()


def S():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def ok(rc, what):
    _lib.check(rc, what)


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def run(what, fn, row_bytes=0, capacity=1 << 22):
    return {k: v.numpy() for k, v in GA.run_twice(fn, DEV, row_bytes, capacity, what).items()}


def eq(a, b):
    return GA.same_bits(a, b)


# ---------------------------------------------------------------------------------------------------
# Lie ops: rows of 3 / 4 / 6 / 7 / 16 elements end unaligned
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", [O.SO3, O.SE3])
@pytest.mark.parametrize("dtype,tol", [(np.float32, 2e-6), (np.float64, 1e-13)])
def test_lie_op(group, dtype, tol):
    td = torch.float32 if dtype == np.float32 else torch.float64
    K, N = (6, 7) if group == O.SE3 else (3, 4)
    for n in N256:
        rng = np.random.default_rng(n)
        a = (0.5 * rng.standard_normal((n, K))).astype(dtype)
        a[0] = 0
        b = rng.standard_normal((n, K)).astype(dtype)
        p3, p4 = rng.standard_normal((n, 3)).astype(dtype), rng.standard_normal((n, 4)).astype(dtype)
        X, Y = O.lie(group, "exp", a, dtype=dtype), O.lie(group, "exp", b, dtype=dtype)
        for op, x, y in (("exp", a, None), ("log", X, None), ("inv", X, None), ("mul", X, Y), ("adj", X, b), ("adjT", X, b),
                         ("act", X, p3), ("act4", X, p4), ("matrix", X, None)):
            want = O.lie(group, op, x, y, dtype=dtype).reshape(n, -1)
            od = want.shape[1]

            def fn(ar):
                xt = ar.tensor("x", x)
                yt = ar.tensor("y", y) if y is not None else None
                z = ar.tensor("z", (n, od), td)
                ok(lib().cdv_lie_op(group, ops.LIE_OPS[op], ops._DT[td], n, P(xt), P(yt), P(z), S()), "cdv_lie_op")
                return {"z": z}
            got = run("cdv_lie_op %s n=%d" % (op, n), fn, row_bytes=od * want.itemsize)["z"]
            bound = tol if op == "exp" else tol * 8 * max(1.0, np.abs(want).max())
            assert np.allclose(got, want, atol=bound), (op, n)
            assert eq(got, ops.lie_op(group, op, T(x), None if y is None else T(y))), (op, n)


# ---------------------------------------------------------------------------------------------------
# reprojection
# ---------------------------------------------------------------------------------------------------

def _scene(n, M, Pp, seed=0, far=()):
    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 7), np.float32)
    poses[:, 6] = 1
    poses[:, :3] = rng.normal(0, 0.03, (n, 3))
    poses[:, 3:6] = rng.normal(0, 0.01, (n, 3))
    for f in far:
        poses[f, 2] = 3.0
    m = n * M
    h, w = 96, 128
    cx, cy = rng.uniform(8, w - 8, m), rng.uniform(8, h - 8, m)
    off = np.arange(float(Pp)) - Pp // 2
    patches = np.zeros((m, 3, Pp, Pp), np.float32)
    patches[:, 0] = cx[:, None, None] + off[None, None, :]
    patches[:, 1] = cy[:, None, None] + off[None, :, None]
    patches[:, 2] = rng.uniform(0.25, 1.0, m)[:, None, None]
    intr = np.stack([rng.uniform(60, 70, n), rng.uniform(55, 65, n), rng.uniform(60, 68, n), rng.uniform(44, 52, n)], -1).astype(np.float32)
    ix = np.repeat(np.arange(n), M).astype(np.int64)
    return poses, patches, intr, ix


def _edges(E, n, m, ix, seed=1):
    """E edges; the first aims at the LAST patch (its frame is the last pose / intrinsics row) and target frame 0, the last
    at patch 0 and the last frame"""
    rng = np.random.default_rng(seed + E)
    kk = rng.integers(0, m, E).astype(np.int64)
    jj = rng.integers(0, n, E).astype(np.int64)
    kk[0], jj[0] = m - 1, 0
    if E > 1:
        kk[-1], jj[-1] = 0, n - 1
    return ix[kk].copy(), jj, kk


def _carve_scene(ar, poses, patches, intr, ii, jj, kk):
    n, m = len(poses), len(patches)
    return (ar.tensor("poses", poses), ar.tensor("patches", patches), ar.tensor("intrinsics", intr),
            ar.tensor("ii", ii, index_max=n - 1), ar.tensor("jj", jj, index_max=n - 1), ar.tensor("kk", kk, index_max=m - 1))


@pytest.mark.parametrize("Pp", [3, 1])
def test_transform(Pp):
    n, M = 5, 4
    poses, patches, intr, ix = _scene(n, M, Pp)
    for E in N64:
        ii, jj, kk = _edges(E, n, n * M, ix)
        for e2pp in (False, True):
            for tonly in (False, True):
                flags = (1 if e2pp else 0) | (2 if tonly else 0)
                res = {}
                for vp, jac in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    def fn(ar):
                        tp, tpa, ti, tii, tjj, tkk = _carve_scene(ar, poses, patches, intr, ii, jj, kk)
                        c = ar.tensor("coords", (E, 2, Pp, Pp) if e2pp else (E, Pp, Pp, 2), F32)
                        v = ar.tensor("validpx", (E, Pp, Pp), F32) if vp else None
                        va, Ji, Jj, Jz = ((ar.tensor("valid", (E,), F32), ar.tensor("Ji", (E, 2, 6), F32), ar.tensor("Jj", (E, 2, 6), F32),
                                           ar.tensor("Jz", (E, 2), F32)) if jac else (None,) * 4)
                        ok(lib().cdv_transform(P(tp), P(tpa), P(ti), P(tii), P(tjj), P(tkk), E, Pp, flags, P(c), P(v), P(va), P(Ji),
                                               P(Jj), P(Jz), S()), "cdv_transform")
                        return {"coords": c, "validpx": v, "valid": va, "Ji": Ji, "Jj": Jj, "Jz": Jz}
                    res[(vp, jac)] = run("cdv_transform E=%d flags=%d vp=%d jac=%d" % (E, flags, vp, jac), fn, row_bytes=48)
                full = res[(1, 1)]
                for key, r in res.items():      # an optional output passed as NULL changes nothing else, bit for bit
                    for name, val in r.items():
                        assert eq(val, full[name]), (E, flags, key, name)
                wc, wv, (wJi, wJj, wJz) = O.transform(poses, patches, intr, ii, jj, kk, jacobian=True, tonly=tonly, dtype=np.float64)
                _, wvp = O.transform(poses, patches, intr, ii, jj, kk, valid=True, tonly=tonly, dtype=np.float64)
                got = full["coords"].transpose(0, 2, 3, 1) if e2pp else full["coords"]
                assert np.abs(got - wc).max() < 1e-3, (E, flags)
                assert np.array_equal(full["validpx"], wvp) and np.array_equal(full["valid"], wv)
                for a, b in ((full["Ji"], wJi), (full["Jj"], wJj), (full["Jz"], wJz.reshape(E, 2))):
                    assert np.allclose(a, b, rtol=1e-4, atol=1e-4 * np.abs(b).max()), (E, flags)
                w = ops.transform(T(poses)[None], T(patches)[None], T(intr)[None], T(ii), T(jj), T(kk), layout_e2pp=e2pp, jacobian=True,
                                  tonly=tonly)
                assert eq(w[0], full["coords"]) and eq(w[1], full["valid"]) and eq(w[2][0], full["Ji"]) and eq(w[2][2], full["Jz"])
                w = ops.transform(T(poses)[None], T(patches)[None], T(intr)[None], T(ii), T(jj), T(kk), layout_e2pp=e2pp, valid=True,
                                  tonly=tonly)
                assert eq(w[0], full["coords"]) and eq(w[1], full["validpx"])


@pytest.mark.parametrize("Pp", [3, 1])
def test_fastba_reproject(Pp):
    n, M = 5, 4
    poses, patches, intr, ix = _scene(n, M, Pp)
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1, keepdims=True)      # this kernel does not normalise
    for E in N64:
        ii, jj, kk = _edges(E, n, n * M, ix)

        def fn(ar):
            tp, tpa, ti, tii, tjj, tkk = _carve_scene(ar, poses, patches, intr[:1], ii, jj, kk)      # row 0 is all it may read
            c = ar.tensor("coords", (E, 2, Pp, Pp), F32)
            ok(lib().cdv_fastba_reproject(P(tp), P(tpa), P(ti), P(tii), P(tjj), P(tkk), E, Pp, P(c), S()), "cdv_fastba_reproject")
            return {"coords": c}
        got = run("cdv_fastba_reproject E=%d" % E, fn, row_bytes=72)["coords"]
        want = O.fastba_reproject(poses, patches, intr[0], ii, jj, kk, dtype=np.float64)
        assert np.abs(got - want).max() < 1e-3, E
        assert eq(got, ops.fastba_reproject(T(poses), T(patches), T(intr), T(ii), T(jj), T(kk))), E


@pytest.mark.parametrize("Pp", [3, 1])
def test_flow_mag(Pp):
    n, M = 5, 4
    poses, patches, intr, ix = _scene(n, M, Pp)
    for E in N64:
        ii, jj, kk = _edges(E, n, n * M, ix)

        def fn(ar):
            tp, tpa, ti, tii, tjj, tkk = _carve_scene(ar, poses, patches, intr, ii, jj, kk)
            f, v = ar.tensor("flow", (E, Pp, Pp), F32), ar.tensor("valid", (E, Pp, Pp), U8)
            ok(lib().cdv_flow_mag(P(tp), P(tpa), P(ti), P(tii), P(tjj), P(tkk), E, Pp, 0.5, P(f), P(v), S()), "cdv_flow_mag")
            return {"flow": f, "valid": v}
        got = run("cdv_flow_mag E=%d" % E, fn, row_bytes=36)
        c0 = O.transform(poses, patches, intr, ii, ii, kk, dtype=np.float64)
        c1, v1 = O.transform(poses, patches, intr, ii, jj, kk, valid=True, dtype=np.float64)
        c2 = O.transform(poses, patches, intr, ii, jj, kk, tonly=True, dtype=np.float64)
        want = 0.5 * np.linalg.norm(c1 - c0, axis=-1) + 0.5 * np.linalg.norm(c2 - c0, axis=-1)
        assert np.abs(got["flow"] - want).max() <= 2e-3 and np.array_equal(got["valid"] != 0, v1 > 0.5), E
        wf, wv = ops.flow_mag(T(poses)[None], T(patches)[None], T(intr)[None], T(ii), T(jj), T(kk), 0.5)
        assert eq(wf, got["flow"]) and np.array_equal(wv[0].cpu().numpy(), got["valid"] != 0), E


def _points64(poses, patches, intr, ix):
    m, Pp = len(ix), patches.shape[-1]
    fx, fy, cx, cy = (intr[ix].astype(np.float64)[:, i, None, None] for i in range(4))
    x, y, d = (patches[:m, i].astype(np.float64) for i in range(3))
    X = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x), d], -1).reshape(-1, 4)
    G = np.repeat(O.lie(O.SE3, "inv", poses[ix].astype(np.float64), dtype=np.float64), Pp * Pp, 0)
    return O.lie(O.SE3, "act4", G, X, dtype=np.float64).reshape(m, Pp, Pp, 4)


@pytest.mark.parametrize("Pp", [3, 1])
def test_point_cloud(Pp):
    for m in N64:
        n = min(m, 7)
        poses, patches, intr, _ = _scene(n, (m + n - 1) // n, Pp, seed=m)
        patches = patches[:m]
        ix = (np.arange(m) % n).astype(np.int64)
        ix[0], ix[-1] = n - 1, (0 if m > 1 else n - 1)

        def fn(ar):
            tp, tpa, ti = ar.tensor("poses", poses), ar.tensor("patches", patches), ar.tensor("intrinsics", intr)
            tix = ar.tensor("ix", ix, index_max=n - 1)
            pts = ar.tensor("points", (m, Pp, Pp, 4), F32)
            ok(lib().cdv_point_cloud(P(tp), P(tpa), P(ti), P(tix), m, Pp, P(pts), S()), "cdv_point_cloud")
            return {"points": pts}
        got = run("cdv_point_cloud M=%d" % m, fn, row_bytes=144)["points"]
        assert np.allclose(got, _points64(poses, patches, intr, ix), rtol=1e-4, atol=1e-4), m
        assert eq(got, ops.point_cloud(T(poses)[None], T(patches)[None], T(intr)[None], T(ix))), m


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129])      # reproject.hip loop_flow_kernel: 64 lanes stride over a frame's M patches
def test_loop_flow(M):
    from cdv_slam_amd import loop
    n = 9
    poses, patches, intr, ix = _scene(n, M, 3, seed=M, far=(1,))
    for j0, nj, f0, nf in ((0, n, 0, n), (n - 1, 1, 0, 1), (0, 1, n - 1, 1), (5, 3, 0, 3)):      # first / last frame as source and target
        def fn(ar):
            tp, tpa, ti = ar.tensor("poses", poses), ar.tensor("patches", patches), ar.tensor("intrinsics", intr)
            tix = ar.tensor("ix", ix, index_max=n - 1)
            out = ar.tensor("flow", (nj, nf), F32)
            ok(lib().cdv_loop_flow(P(tp), P(tpa), P(ti), P(tix), M, 3, j0, nj, f0, nf, 0.5, P(out), S()), "cdv_loop_flow")
            return {"flow": out}
        got = run("cdv_loop_flow M=%d" % M, fn, row_bytes=4 * nf)["flow"]
        jr, fr = np.arange(j0, j0 + nj), np.arange(f0, f0 + nf)
        jj = np.repeat(jr, nf * M)
        kk = np.tile((fr[:, None] * M + np.arange(M)[None]).reshape(-1), nj)
        ii = ix[kk]
        cen = np.ascontiguousarray(patches[:, :, 1:2, 1:2])
        c0 = O.transform(poses, cen, intr, ii, ii, kk, dtype=np.float64)
        c1, v1 = O.transform(poses, cen, intr, ii, jj, kk, valid=True, dtype=np.float64)
        c2 = O.transform(poses, cen, intr, ii, jj, kk, tonly=True, dtype=np.float64)
        fm = (0.5 * np.linalg.norm(c1 - c0, axis=-1) + 0.5 * np.linalg.norm(c2 - c0, axis=-1)).reshape(-1, M)
        val = (v1 > 0.5).reshape(-1, M)
        nval = np.maximum(val.sum(1), 1)
        want = np.where(val.sum(1) > 0.75 * M, (fm * val).sum(1) / nval, np.inf).reshape(nj, nf)
        assert np.array_equal(np.isinf(got), np.isinf(want)), (M, j0)
        fin = np.isfinite(want)
        assert np.allclose(got[fin], want[fin], rtol=1e-5, atol=1e-4), (M, j0)
        assert eq(got, loop.loop_flow(T(poses), T(patches), T(intr), T(ix), M, j0, nj, f0, nf, 0.5)), (M, j0)


# ---------------------------------------------------------------------------------------------------
# layout converters: everything outside the range keeps its previous bits
# ---------------------------------------------------------------------------------------------------

def _pattern16(shape, seed):
    """finite f16 bit patterns that no conversion of the inputs below produces by accident"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0x4400, 0x7000, int(np.prod(shape))).astype(np.uint16)).view(np.float16).reshape(shape)


def _maps(shape, seed, scale=4.0):
    return (np.random.default_rng(seed).standard_normal(shape) / scale).astype(np.float16)


def _to_ring(planar):
    """planar [N,C,H,W] -> padded channels-last ring with zero margins"""
    N, C, H, W = planar.shape
    ring = np.zeros((N, H + 2 * PADY, W + 2 * PADX, C), np.float16)
    ring[:, PADY:PADY + H, PADX:PADX + W] = planar.transpose(0, 2, 3, 1)
    return ring


@pytest.mark.parametrize("C", [8, 24])
def test_gmap_to_pixel_major(C):
    # rings.hip gmap_pm_kernel: one lane per (tile, pixel, 8-channel group), 256 lanes: 9 C / 8 lanes per tile
    per = 9 * C // 8
    sizes = sorted({1, 2, 256 // per, 256 // per + 1, 512 // per + 1, 1009})
    for Ng in sizes:
        g = _maps((Ng, C, 3, 3), Ng)
        pre = _pattern16((Ng, 9, C), Ng + 1)
        ranges = {(0, Ng), (0, 1), (Ng - 1, 1)} | ({(1, Ng - 2)} if Ng > 2 else set())
        for first, count in sorted(ranges):
            def fn(ar):
                src, dst = ar.tensor("gmap_planar", g), ar.tensor("gmap_pm", pre)
                ok(lib().cdv_gmap_to_pixel_major(P(src), P(dst), Ng, C, first, count, S()), "cdv_gmap_to_pixel_major")
                return {"pm": dst}
            got = run("cdv_gmap_to_pixel_major Ng=%d [%d,+%d)" % (Ng, first, count), fn, row_bytes=18 * C)["pm"]
            want = pre.copy()
            want[first:first + count] = g[first:first + count].reshape(count, C, 9).transpose(0, 2, 1)
            assert eq(got, want), (Ng, first, count)
            out = T(pre).clone()
            assert eq(ops.gmap_to_pixel_major(T(g), out=out, first=first, count=count), got)


@pytest.mark.parametrize("C", [8, 24])
def test_fmap_to_nhwc(C):
    # rings.hip nchw_to_nhwc_kernel: one lane per (slot, pixel, 8-channel group), 256 lanes; H x W = 4 x 4: 16 C / 8 lanes a slot
    H, W = 4, 4
    per = H * W * C // 8
    for count_all in sorted({1, 256 // per - 1, 256 // per, 256 // per + 1, 512 // per + 1, 67}):
        N = max(count_all, 1)
        src_np = _maps((N, C, H, W), N)
        pre = _pattern16((N, H + 2 * PADY, W + 2 * PADX, C), N + 7)
        ranges = {(0, N), (0, 1), (N - 1, 1)} | ({(1, N - 2)} if N > 2 else set())
        for first, count in sorted(ranges):
            def fn(ar):
                src, dst = ar.tensor("src_nchw", src_np), ar.tensor("dst_nhwc", pre)
                ok(lib().cdv_fmap_to_nhwc(P(src), P(dst), N, C, H, W, first, count, S()), "cdv_fmap_to_nhwc")
                return {"ring": dst}
            got = run("cdv_fmap_to_nhwc N=%d [%d,+%d)" % (N, first, count), fn, row_bytes=(W + 2 * PADX) * C * 2, capacity=1 << 24)["ring"]
            want = pre.copy()
            want[first:first + count, PADY:PADY + H, PADX:PADX + W] = src_np[first:first + count].transpose(0, 2, 3, 1)
            assert eq(got, want), (N, first, count)      # the slots outside the range and every margin keep their bits


def _pool4(f):
    C, H, W = f.shape
    return f.reshape(C, H // 4, 4, W // 4, 4).astype(np.float32).mean((2, 4))


@pytest.mark.parametrize("with_tiles", [False, True])
def test_ingest(with_tiles):
    """cdv_fmap_ingest / cdv_frame_ingest: the first and the LAST ring slot, with and without the planar rings, tile ranges
    at both ends of the tile array.  rings.hip fmap_ingest_kernel: (H/4)(W/4)(C/8) * 16 lanes, 256 a workgroup."""
    from tests.stream_audit import f16_ulps
    C, slots, Ng = 8, 3, 40
    for H, W in ((4, 4), (12, 20), (16, 16), (16, 20)):      # 16, 240, 256, 320 lanes
        f = _maps((C, H, W), H * W)
        g = _maps((Ng, C, 3, 3), 5)
        pre1, pre2 = _pattern16((slots, H + 2 * PADY, W + 2 * PADX, C), 1), _pattern16((slots, H // 4 + 2 * PADY, W // 4 + 2 * PADX, C), 2)
        prep1, prep2 = _pattern16((slots, C, H, W), 3), _pattern16((slots, C, H // 4, W // 4), 4)
        prepm = _pattern16((Ng, 9, C), 6)
        for slot in (0, slots - 1):
            for planar in (False, True):
                for gfirst, gcount in (((0, 1), (Ng - 29, 29), (0, Ng)) if with_tiles else ((0, 0),)):
                    def fn(ar):
                        src = ar.tensor("fmap_chw", f)
                        r1, r2 = ar.tensor("fmap1_nhwc", pre1), ar.tensor("fmap2_nhwc", pre2)
                        p1, p2 = (ar.tensor("fmap1_nchw", prep1), ar.tensor("fmap2_nchw", prep2)) if planar else (None, None)
                        if with_tiles:
                            gp, pm = ar.tensor("gmap_planar", g), ar.tensor("gmap_pm", prepm)
                            ok(lib().cdv_frame_ingest(P(src), P(r1), P(r2), P(p1), P(p2), slot, C, H, W, P(gp), P(pm), Ng, gfirst, gcount,
                                                      S()), "cdv_frame_ingest")
                        else:
                            pm = None
                            ok(lib().cdv_fmap_ingest(P(src), P(r1), P(r2), P(p1), P(p2), slot, C, H, W, S()), "cdv_fmap_ingest")
                        return {"r1": r1, "r2": r2, "p1": p1, "p2": p2, "pm": pm}
                    got = run("ingest %dx%d slot %d" % (H, W, slot), fn, row_bytes=(W + 2 * PADX) * C * 2, capacity=1 << 23)
                    w1 = pre1.copy()
                    w1[slot, PADY:PADY + H, PADX:PADX + W] = f.transpose(1, 2, 0)
                    assert eq(got["r1"], w1)
                    pooled = _pool4(f).astype(np.float16)
                    w2 = got["r2"].copy()
                    w2[slot, PADY:PADY + H // 4, PADX:PADX + W // 4] = pre2[slot, PADY:PADY + H // 4, PADX:PADX + W // 4]
                    assert eq(w2, pre2), "level-1 ring touched outside the slot's interior"
                    lvl1 = got["r2"][slot, PADY:PADY + H // 4, PADX:PADX + W // 4].transpose(2, 0, 1)
                    assert int(f16_ulps(torch.as_tensor(lvl1.copy()), torch.as_tensor(pooled)).max()) <= 1      # stream_audit.FMAP2_ULPS
                    if planar:
                        wp1, wp2 = prep1.copy(), prep2.copy()
                        wp1[slot], wp2[slot] = f, lvl1
                        assert eq(got["p1"], wp1) and eq(got["p2"], wp2)
                    if with_tiles:
                        wpm = prepm.copy()
                        wpm[gfirst:gfirst + gcount] = g[gfirst:gfirst + gcount].reshape(gcount, C, 9).transpose(0, 2, 1)
                        assert eq(got["pm"], wpm)
                    # the wrapper's ordinary call
                    r1, r2 = T(pre1).clone(), T(pre2).clone()
                    pm = T(prepm).clone()
                    ops.fmap_ingest(T(f), r1, r2, slot, gmap=T(g) if with_tiles else None, gmap_pm=pm if with_tiles else None,
                                    gmap_first=gfirst, gmap_count=gcount)
                    assert eq(r1, got["r1"]) and eq(r2, got["r2"]) and (not with_tiles or eq(pm, got["pm"]))


@pytest.mark.parametrize("fused", [False, True])
def test_shadow_sync(fused):
    """cdv_fmap_sync_nhwc / cdv_shadows_sync: first sync converts every slot, the next one only the slot that changed -- the
    first and the last; the workspace is sized exactly by cdv_fmap_sync_workspace_bytes"""
    C, N, Ng = 8, 5, 30
    shapes = ((8, 12), (2, 3))
    for changed in (0, N - 1):
        srcs = [_maps((N, C, h, w), 10 + h) for h, w in shapes]
        srcs2 = [s.copy() for s in srcs]
        for s in srcs2:
            s[changed] = _maps(s[changed].shape, 99)
        g = _maps((Ng, C, 3, 3), 3)
        pats = [_pattern16((N, h + 2 * PADY, w + 2 * PADX, C), 20 + h) for h, w in shapes]
        wsb = int(lib().cdv_fmap_sync_workspace_bytes(N))

        def fn(ar):
            src = [ar.tensor("src%d" % i, s) for i, s in enumerate(srcs)]
            dst = [ar.tensor("dst%d" % i, s.shape[:1] + (s.shape[2] + 2 * PADY, s.shape[3] + 2 * PADX, C), F16) for i, s in enumerate(srcs)]
            ws = [ar.tensor("ws%d" % i, (wsb,), U8) for i in range(2)]
            gp, pm = ar.tensor("gmap_planar", g), ar.tensor("gmap_pm", (Ng, 9, C), F16)

            def sync(parity):
                if fused:
                    rings = (_lib.ShadowRing * 2)()
                    for i, r in enumerate(rings):
                        r.src_nchw, r.dst_nhwc, r.ws, r.N = P(src[i]), P(dst[i]), P(ws[i]), N
                        r.C, r.H, r.W, r.parity = C, shapes[i][0], shapes[i][1], parity
                    ok(lib().cdv_shadows_sync(ctypes.cast(rings, ctypes.c_void_p), 2, P(gp), P(pm), Ng, C, S()), "cdv_shadows_sync")
                else:
                    for i in range(2):
                        ok(lib().cdv_fmap_sync_nhwc(P(src[i]), P(dst[i]), N, C, shapes[i][0], shapes[i][1], P(ws[i]), parity, S()),
                           "cdv_fmap_sync_nhwc")
            sync(0)
            first = [d.clone() for d in dst]
            for i in range(2):
                dst[i].copy_(T(pats[i]))
                src[i].copy_(T(srcs2[i]))
            sync(1)
            return {"first0": first[0], "first1": first[1], "dst0": dst[0], "dst1": dst[1], "pm": pm if fused else None}
        got = run("shadow sync fused=%d changed=%d" % (fused, changed), fn, row_bytes=(12 + 2 * PADX) * C * 2, capacity=1 << 23)
        for i in range(2):
            assert eq(got["first%d" % i], _to_ring(srcs[i])), "first sync: interior converted, margins left zero"
            want = pats[i].copy()
            h, w = shapes[i]
            want[changed, PADY:PADY + h, PADX:PADX + w] = srcs2[i][changed].transpose(1, 2, 0)
            assert eq(got["dst%d" % i], want), "second sync touched more than the changed slot's interior"
        if fused:
            assert eq(got["pm"], g.reshape(Ng, C, 9).transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------------------
# correlation forward
# ---------------------------------------------------------------------------------------------------

def _corr_tol(truth):
    return 2.0 ** -8 * np.abs(truth).max() + 2.0 ** -10


def _border_coords(E, dims, seed, Pp=3):
    """Pp x Pp patches whose windows sit on each border and corner of maps of size dims = [(H, W, scale), ...], inside and outside"""
    rng = np.random.default_rng(seed)
    off = np.arange(float(Pp)) - Pp // 2
    coords = np.empty((E, 2, Pp, Pp), np.float32)
    for e in range(E):
        H, W, s = dims[e % len(dims)]
        xs = [0.0, W - 1.0, W - 0.5, W / 2 + 0.3, -2.5, W + 1.75, 0.4]
        ys = [0.0, H - 1.0, H / 2 + 0.6, H - 0.25, H + 2.0, -1.5, 0.2]
        k = e // len(dims)
        cx, cy = s * xs[k % 7], s * ys[(k // 7 + k) % 7]
        sc = s * rng.uniform(0.5, 1.5)
        coords[e, 0] = cx + sc * off[None, :]
        coords[e, 1] = cy + sc * off[:, None]
    return coords


def _ring_idx(E, Ng, slots, seed, wrap):
    rng = np.random.default_rng(seed)
    kk = rng.integers(0, Ng, E).astype(np.int64)
    jj = rng.integers(0, slots, E).astype(np.int64)
    kk[0], jj[0] = Ng - 1, slots - 1          # the last tile and the last ring slot ...
    if E > 1:
        kk[-1], jj[-1] = 0, 0                 # ... and element 0
    if wrap:
        kk += Ng * rng.integers(0, 4, E)
        jj += slots * rng.integers(0, 4, E)
    return kk, jj


H0, W0, H1, W1 = 20, 28, 30, 47      # level 1 with an odd side (EuRoC's 30 x 47); the levels are independent rings here


def _corr_inputs(C, E, seed, wrap):
    Ng, slots = 7, 3
    g = _maps((Ng, C, 3, 3), seed)
    f0, f1 = _maps((slots, C, H0, W0), seed + 1), _maps((slots, C, H1, W1), seed + 2)
    coords = _border_coords(E, [(H0, W0, 1.0), (H1, W1, 4.0)], seed)
    kk, jj = _ring_idx(E, Ng, slots, seed, wrap)
    return g, f0, f1, coords, kk, jj, Ng, slots


@pytest.mark.parametrize("C,nlev,pm,order,wrap", [(24, 2, 1, 1, 1), (24, 2, 0, 0, 0), (24, 1, 0, 1, 0), (24, 1, 1, 0, 1), (8, 2, 1, 0, 1),
                                                   (8, 1, 0, 1, 0), (32, 2, 0, 1, 1), (32, 1, 1, 0, 0), (128, 2, 0, 0, 1), (128, 1, 1, 0, 0),
                                                   (128, 2, 1, 1, 0)])
def test_corr_fused(C, nlev, pm, order, wrap):
    for E in E_FUSED:      # C = 128: corr_wide_kernel<4>, four edges per workgroup -- the same unit
        g, f0, f1, coords, kk, jj, Ng, slots = _corr_inputs(C, E, 100 * C + E, wrap)
        gin = g.reshape(Ng, C, 9).transpose(0, 2, 1).copy() if pm else g
        perm = np.random.default_rng(E).permutation(E).astype(np.int32)
        r0, r1 = _to_ring(f0), _to_ring(f1)

        def fn(ar):
            tg = ar.tensor("gmap", gin)
            t0 = ar.tensor("fmap0_nhwc", r0)
            t1 = ar.tensor("fmap1_nhwc", r1) if nlev == 2 else None
            tc = ar.tensor("coords", coords)
            tk, tj = ar.tensor("kk", kk, index_max=Ng - 1), ar.tensor("jj", jj, index_max=slots - 1)
            to = ar.tensor("order", perm, index_max=E - 1) if order else None
            out = ar.tensor("out", (E, 441 * nlev), F16)
            ok(lib().cdv_corr_fused(P(tg), P(t0), P(t1), P(tc), P(tk), P(tj), P(to), P(out), E, Ng, slots, C, H0, W0, H1 if nlev == 2 else 0,
                                    W1 if nlev == 2 else 0, 1.0, 4.0, nlev, Ng if wrap else 0, slots if wrap else 0, pm, S()), "cdv_corr_fused")
            return {"out": out, "ring0": t0, "ring1": t1}
        got = run("cdv_corr_fused C=%d E=%d" % (C, E), fn, row_bytes=882 * 2, capacity=1 << 25)
        assert eq(got["ring0"], r0) and (nlev == 1 or eq(got["ring1"], r1)), "ring (margins) modified"
        if nlev == 2:
            truth = O.slam_corr(g, f0, f1, coords, kk % Ng, jj % slots, 3, "truth")
        else:
            truth = O.corr(g, f0, coords, kk % Ng, jj % slots, 3, "truth").reshape(E, -1)
        assert np.isfinite(got["out"]).all()
        assert np.abs(got["out"].astype(np.float64) - truth).max() <= _corr_tol(truth), (C, E)
        tperm = T(perm)      # held until the wrapper's launch has read it
        w = ops.corr_fused(T(gin), T(r0), T(r1) if nlev == 2 else None, T(coords)[None], T(kk), T(jj), kmod=Ng if wrap else 0,
                           jmod=slots if wrap else 0, order_ptr=P(tperm) if order else None, pixel_major=bool(pm))
        torch.cuda.synchronize()
        assert eq(w, got["out"]), (C, E)


@pytest.mark.parametrize("C,pm", [(24, 1), (8, 0)])
@pytest.mark.parametrize("level", [0, 1])
def test_corr_level_checked(C, pm, level):
    """the second call of the reference's pair: edges whose coords equal coords_ref * ref_mul keep what is there, the others are
    recomputed into their level's interleaved half; the OTHER level's halves are untouched bit for bit"""
    for E in E_FUSED:
        g, f0, f1, cref, kk, jj, Ng, slots = _corr_inputs(C, E, 7 * C + E + level, True)
        gin = g.reshape(Ng, C, 9).transpose(0, 2, 1).copy() if pm else g
        fm, (H, W), scale = ((f0, (H0, W0), 1.0) if level == 0 else (f1, (H1, W1), 1.0))      # as the pairing calls it: coords in the level's units
        ring = _to_ring(fm)
        pre = _pattern16((E, 441, 2), E)
        for which in ("all", "none", "third"):
            match = {"all": np.ones(E, bool), "none": np.zeros(E, bool), "third": np.arange(E) % 3 != 0}[which]
            ref_mul = 0.25
            coords = (cref * np.float32(ref_mul)).astype(np.float32)
            coords[~match] += np.float32(0.375)

            def fn(ar):
                tg, tr = ar.tensor("gmap", gin), ar.tensor("fmap_nhwc", ring)
                tc, tcr = ar.tensor("coords", coords), ar.tensor("coords_ref", cref)
                tk, tj = ar.tensor("kk", kk, index_max=Ng - 1), ar.tensor("jj", jj, index_max=slots - 1)
                out = ar.tensor("out", pre)
                ok(lib().cdv_corr_level_checked_interleaved(P(tg), P(tr), P(tc), P(tcr), ref_mul, P(tk), P(tj), P(out), level, E, Ng, slots,
                                                            C, H, W, scale, Ng, slots, pm, S()), "cdv_corr_level_checked_interleaved")
                return {"out": out, "ring": tr}
            got = run("corr_level_checked %s E=%d" % (which, E), fn, row_bytes=882 * 2, capacity=1 << 23)
            assert eq(got["ring"], ring)
            out = got["out"]
            assert eq(out[:, :, 1 - level], pre[:, :, 1 - level]), "the other level's halves were written"
            assert eq(out[match][:, :, level], pre[match][:, :, level]), "a matching edge was recomputed"
            if (~match).any():
                truth = O.corr(g, fm, coords / np.float32(scale), kk % Ng, jj % slots, 3, "truth").reshape(E, 441)
                d = np.abs(out[~match][:, :, level].astype(np.float64) - truth[~match])
                assert d.max() <= _corr_tol(truth), (which, E)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("radius,Pp", [(1, 3), (3, 3), (0, 4)])
def test_corr_fwd(dtype, radius, Pp):
    # altcorr_fwd.hip corr_generic_kernel: one lane per output element, 256 lanes; an edge has P^2 (2 r + 1)^2 of them.  With 3 x 3
    # patches that is odd and never fills a workgroup exactly; P = 4, r = 0 gives 16 per edge: M = 15 / 16 / 17 are one short of,
    # exactly and one over 256 lanes
    D1 = 2 * radius + 1
    per = Pp * Pp * D1 * D1
    C, N1, N2, H, W = 5, 6, 3, 30, 47
    sizes = {1, 2, 256 // per, 256 // per + 1, 512 // per + 1, 101} - {0}
    if 256 % per == 0:
        sizes |= {256 // per - 1}
    for M in sorted(sizes):
        f1, f2 = _maps((N1, C, Pp, Pp), M).astype(dtype), _maps((N2, C, H, W), M + 1).astype(dtype)
        coords = _border_coords(M, [(H, W, 1.0)], M, Pp)
        us, vs = _ring_idx(M, N1, N2, M, False)
        td = F16 if dtype == np.float16 else F32

        def fn(ar):
            a, b, c = ar.tensor("fmap1", f1), ar.tensor("fmap2", f2), ar.tensor("coords", coords)
            u, v = ar.tensor("us", us, index_max=N1 - 1), ar.tensor("vs", vs, index_max=N2 - 1)
            out = ar.tensor("out", (M, D1, D1, Pp, Pp), td)
            ok(lib().cdv_corr_fwd(P(a), P(b), P(c), P(u), P(v), P(out), M, N1, N2, C, Pp, H, W, radius, ops._DT[td], S()), "cdv_corr_fwd")
            return {"out": out}
        got = run("cdv_corr_fwd M=%d" % M, fn, row_bytes=per * 4)["out"]
        truth = O.corr(f1, f2, coords, us, vs, radius, "truth")
        if dtype == np.float16:
            assert np.abs(got.astype(np.float64) - truth).max() <= _corr_tol(truth), M
        else:
            assert np.allclose(got, truth, rtol=1e-5, atol=1e-5), M
        assert eq(got, ops.corr_forward_plain(T(f1)[None], T(f2)[None], T(coords)[None], T(us), T(vs), radius)), M


# ---------------------------------------------------------------------------------------------------
# patchify
# ---------------------------------------------------------------------------------------------------

def _centres(M, H, W, seed):
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-3, W + 3, M), rng.uniform(-3, H + 3, M)], -1).astype(np.float32)
    edge = np.array([[W - 1.0, H - 1.0], [0.0, 0.0], [W - 0.5, 3.25], [4.5, H - 0.25], [W + 2.0, 2.0], [-2.5, H + 1.0]], np.float32)
    c[:min(M, len(edge))] = edge[:M]      # the last row / column, the first, just outside
    return c


M_PATCH = [1, 2, 63, 64, 65]


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_patchify(dtype):
    td = F16 if dtype == np.float16 else F32
    B, C, H, W = 2, 5, 11, 13
    net = _maps((B, C, H, W), 4, 1.0).astype(dtype)
    for M in M_PATCH:
        coords = np.stack([_centres(M, H, W, M + b) for b in range(B)])
        for r in (0, 1, 3):
            D = 2 * r + 2

            def fn(ar):
                n, c = ar.tensor("net", net), ar.tensor("coords", coords)
                out = ar.tensor("patches", (B, M, C, D, D), td)
                ok(lib().cdv_patchify_fwd(P(n), P(c), P(out), B, M, C, H, W, r, ops._DT[td], S()), "cdv_patchify_fwd")
                return {"out": out}
            got = run("cdv_patchify_fwd M=%d r=%d" % (M, r), fn, row_bytes=C * D * D * 4)["out"]
            for b in range(B):
                assert eq(got[b], O.patchify_raw(net[b], coords[b], r)), (M, r)
            assert eq(got, ops.patchify_forward(T(net), T(coords), r)), (M, r)
            for mode, name in ((1, "bilinear"), (2, "upperleft")):
                d = 1 if mode == 2 else 2 * r + 1
                to = td if mode == 2 else F32

                def fn2(ar):
                    n, c = ar.tensor("net", net), ar.tensor("coords", coords)
                    out = ar.tensor("out", (B, M, C, d, d), to)
                    ok(lib().cdv_patchify_blend(P(n), P(c), P(out), B, M, C, H, W, r, mode, ops._DT[td], S()), "cdv_patchify_blend")
                    return {"out": out}
                gb = run("cdv_patchify_blend M=%d r=%d mode=%d" % (M, r, mode), fn2, row_bytes=C * d * d * 4)["out"]
                for b in range(B):
                    want = O.patchify(net[b], coords[b], r, name)
                    if mode == 2:
                        assert eq(gb[b], want), (M, r)
                    else:
                        assert np.allclose(gb[b], want, atol=1e-6 * max(1.0, np.abs(want).max())), (M, r)
                assert eq(gb, ops.patchify_blend(T(net), T(coords), r, name)), (M, r, mode)


@pytest.mark.parametrize("n_jobs", [1, 8])
def test_patchify_multi(n_jobs):
    specs = [(np.float16, 8, 6, 8, 1, 1, 1.0, 0.0), (np.float32, 3, 24, 32, 0, 1, 4.0, 0.5), (np.float16, 16, 3, 4, 0, 2, 0.5, 0.0),
             (np.float32, 3, 6, 8, 1, 1, 1.0, 0.0), (np.float16, 5, 6, 8, 3, 1, 1.0, 0.0), (np.float32, 2, 6, 8, 0, 2, 1.0, 0.0),
             (np.float16, 8, 12, 16, 1, 2, 2.0, 0.25), (np.float32, 1, 6, 8, 2, 1, 1.0, 0.0)][:n_jobs]
    nets = [_maps((C, H, W), 30 + i, 1.0).astype(dt) for i, (dt, C, H, W, *_) in enumerate(specs)]
    for M in M_PATCH:
        coords = _centres(M, 6, 8, M)

        def fn(ar):
            c = ar.tensor("coords", coords)
            jobs = (_lib.PatchifyJob * n_jobs)()
            outs = {}
            for i, (dt, C, H, W, r, mode, sc, of) in enumerate(specs):
                n = ar.tensor("net%d" % i, nets[i])
                d = 1 if mode == 2 else 2 * r + 1
                td = F16 if dt == np.float16 else F32
                o = ar.tensor("out%d" % i, (M, C, d, d), td if mode == 2 else F32)
                j = jobs[i]
                j.net, j.out, j.C, j.H, j.W, j.radius, j.mode, j.dtype = P(n), P(o), C, H, W, r, mode, ops._DT[td]
                j.sx = j.sy = sc
                j.ox = j.oy = of
                outs["out%d" % i] = o
            ok(lib().cdv_patchify_multi(ctypes.cast(jobs, ctypes.c_void_p), n_jobs, P(c), M, S()), "cdv_patchify_multi")
            return outs
        got = run("cdv_patchify_multi jobs=%d M=%d" % (n_jobs, M), fn, row_bytes=16 * 49 * 4)
        w = ops.patchify_multi([dict(net=T(nets[i]), radius=r, mode="upperleft" if mode == 2 else "bilinear", scale=sc, offset=of)
                                for i, (dt, C, H, W, r, mode, sc, of) in enumerate(specs)], T(coords))
        for i, (dt, C, H, W, r, mode, sc, of) in enumerate(specs):
            cc = ((coords + np.float32(of)) * np.float32(sc)).astype(np.float32)      # the reference's two float operations
            want = O.patchify(nets[i], cc, r, "upperleft" if mode == 2 else "bilinear")
            g = got["out%d" % i]
            assert eq(g, want) if mode == 2 else np.allclose(g, want, atol=1e-6 * max(1.0, np.abs(want).max())), (i, M)
            assert eq(w[i], g), (i, M)


# ---------------------------------------------------------------------------------------------------
# backward: the byte queries are the contract
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("need", [(True, True), (True, False), (False, True)])
def test_corr_bwd(need):
    from tests.test_corr_backward import _close, _corr_truth
    C, N1, N2, H, W, r = 5, 6, 3, 9, 13, 1
    D1 = 2 * r + 1
    # corr_bwd.hip: the entry kernels (count / fill / order) run 256 lanes over the M * 4 window corners: M = 64 fills a workgroup
    for M in (1, 63, 64, 65, 129, 1009):
        f1, f2 = _maps((N1, C, 3, 3), M, 1.0).astype(np.float32), _maps((N2, C, H, W), M + 1, 1.0).astype(np.float32)
        coords = _border_coords(M, [(H, W, 1.0)], M)
        us, vs = _ring_idx(M, N1, N2, M, False)
        grad = np.random.default_rng(M).standard_normal((M, D1, D1, 3, 3)).astype(np.float32)
        wsb = int(lib().cdv_corr_bwd_workspace_bytes(M, N1, N2, 3, H, W, r))

        def fn(ar):
            a, b, c = ar.tensor("fmap1", f1), ar.tensor("fmap2", f2), ar.tensor("coords", coords)
            u, v = ar.tensor("us", us, index_max=N1 - 1), ar.tensor("vs", vs, index_max=N2 - 1)
            gr = ar.tensor("grad", grad)
            g1 = ar.tensor("fmap1_grad", f1.shape, F32) if need[0] else None
            g2 = ar.tensor("fmap2_grad", f2.shape, F32) if need[1] else None
            ws = ar.tensor("workspace", (wsb,), U8, fill=0xA5)
            ok(lib().cdv_corr_bwd(P(a), P(b), P(c), P(u), P(v), P(gr), P(g1), P(g2), P(ws), M, N1, N2, C, 3, H, W, r, S()), "cdv_corr_bwd")
            return {"g1": g1, "g2": g2}
        got = run("cdv_corr_bwd M=%d" % M, fn, row_bytes=W * 4, capacity=1 << 23)
        w1, w2 = ops.corr_backward(T(f1)[None], T(f2)[None], T(coords)[None], T(us), T(vs), T(grad)[None], r, need=need)
        t1, t2, m1, m2 = _corr_truth(torch.tensor(f1)[None], torch.tensor(f2)[None], torch.tensor(coords)[None], torch.tensor(us),
                                     torch.tensor(vs), torch.tensor(grad)[None], r)
        for key, wrap, ref, mag in (("g1", w1, t1, m1), ("g2", w2, t2, m2)):
            if key in got:
                assert eq(got[key], wrap[0]), (key, M)
                _close(torch.as_tensor(got[key])[None], ref, mag)      # the bound of test_corr_backward_matches_float64_truth


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_patchify_bwd(dtype):
    td = F16 if dtype == np.float16 else F32
    B, C, H, W, r = 2, 5, 11, 13, 1
    D = 2 * r + 2
    for M in M_PATCH:
        coords = np.stack([_centres(M, H, W, M + b) for b in range(B)])
        pg = np.random.default_rng(M).standard_normal((B, M, C, D, D)).astype(dtype)
        wsb = int(lib().cdv_patchify_bwd_workspace_bytes(B, M, H, W, r))

        def fn(ar):
            g, c = ar.tensor("patch_grad", pg), ar.tensor("coords", coords)
            out = ar.tensor("net_grad", (B, C, H, W), td)
            ws = ar.tensor("workspace", (wsb,), U8, fill=0xA5)
            ok(lib().cdv_patchify_bwd(P(g), P(c), P(out), P(ws), B, M, C, H, W, r, ops._DT[td], S()), "cdv_patchify_bwd")
            return {"out": out}
        got = run("cdv_patchify_bwd M=%d" % M, fn, row_bytes=W * 4)["out"]
        from tests.test_corr_backward import _close
        assert eq(got, ops.patchify_backward(T(np.zeros((B, C, H, W), dtype)), T(coords), T(pg), r)), M
        want, mag = np.zeros((B, C, H, W), np.float64), np.zeros((B, C, H, W), np.float64)      # the adjoint of the gather, in float64
        for b in range(B):
            for m in range(M):
                x0, y0 = int(np.floor(coords[b, m, 0])) - r, int(np.floor(coords[b, m, 1])) - r
                for dy in range(D):
                    for dx in range(D):
                        if 0 <= y0 + dy < H and 0 <= x0 + dx < W:
                            want[b, :, y0 + dy, x0 + dx] += pg[b, m, :, dy, dx].astype(np.float64)
                            mag[b, :, y0 + dy, x0 + dx] += np.abs(pg[b, m, :, dy, dx].astype(np.float64))
        _close(torch.as_tensor(got), torch.as_tensor(want), torch.as_tensor(mag), f16=dtype == np.float16)      # test_corr_backward's bound


# ---------------------------------------------------------------------------------------------------
# patch-graph index
# ---------------------------------------------------------------------------------------------------

def _graph_lists(E, seed=0):
    """edge lists whose patch ids span [0, k_range) exactly; every (patch, frame) pair at most once per few edges"""
    rng = np.random.default_rng(seed + E)
    k_range = max(1, E // 6)
    n = 9
    kk = rng.integers(0, k_range, E).astype(np.int64)
    kk[0] = k_range - 1
    kk[-1] = 0 if E > 1 else k_range - 1
    jj = rng.integers(0, n, E).astype(np.int64)
    jj[0], jj[-1] = (n - 1, 0) if E > 1 else (n - 1, n - 1)
    ii = (kk % n).astype(np.int64)
    return ii, jj, kk, k_range, n


def _graph_ws(ar, E, k_range):
    nbytes = int(lib().cdv_graph_workspace_bytes(E, k_range))
    ws = ar.tensor("graph_ws", (nbytes,), U8)
    ok(lib().cdv_graph_workspace_init(P(ws), nbytes, E, k_range, S()), "cdv_graph_workspace_init")
    return ws, nbytes


def _meta(ws):
    m = (ctypes.c_int64 * 8)()
    ok(lib().cdv_graph_read_meta_host(P(ws), m, S()), "cdv_graph_read_meta_host")
    return list(m)


@pytest.mark.parametrize("entry", ["build", "build_edges"])
def test_graph_ranked(entry):
    """workspace sized exactly by cdv_graph_workspace_bytes(E_max, k_range) with E == E_max and the id range == k_range; kx of
    capacity U exactly; ix / jx guarded"""
    for E in N256:
        ii, jj, kk, k_range, n = _graph_lists(E)
        kx_w, ku_w = O.unique(kk)
        U = len(kx_w)

        def fn(ar):
            ws, nbytes = _graph_ws(ar, E, k_range)
            ti, tj, tk = ar.tensor("ii", ii, index_max=n - 1), ar.tensor("jj", jj, index_max=n - 1), ar.tensor("kk", kk, index_max=k_range - 1)
            ix, jx = ar.tensor("ix", (E,), I64, fill=-7), ar.tensor("jx", (E,), I64, fill=-7)
            if entry == "build":
                ok(lib().cdv_graph_build(P(tj), P(tk), E, P(ws), nbytes, E, k_range, S()), "cdv_graph_build")
                ok(lib().cdv_neighbors(P(ws), E, P(ix), P(jx), S()), "cdv_neighbors")
            else:
                ok(lib().cdv_graph_build_edges(P(ti), P(tj), P(tk), E, P(ws), nbytes, E, k_range, P(ix), P(jx), S()), "cdv_graph_build_edges")
            meta = _meta(ws)
            assert meta[0] == U and meta[6] == 0 and meta[7] == E, meta
            kx, ku = ar.tensor("kx", (U,), I64, fill=-7), ar.tensor("ku", (E,), I64, fill=-7)
            ok(lib().cdv_graph_get_unique(P(ws), P(kx), U, P(ku), E, S()), "cdv_graph_get_unique")
            return {"ix": ix, "jx": jx, "kx": kx, "ku": ku}
        got = run("cdv_graph_%s E=%d" % (entry, E), fn, row_bytes=8, capacity=1 << 23)
        ix_w, jx_w = O.neighbors(kk, jj)
        assert eq(got["kx"], kx_w) and eq(got["ku"], ku_w) and eq(got["ix"], ix_w) and eq(got["jx"], jx_w), E
        g = ops.GraphIndex(torch.device(DEV), E_cap=E, k_range=k_range)
        g.build(T(jj), T(kk), with_neighbors=True, ii=T(ii) if entry == "build_edges" else None)
        wkx, wku = g.unique()
        assert eq(wkx, got["kx"]) and eq(wku, got["ku"]) and eq(g.neighbors()[0], got["ix"]) and eq(g.neighbors()[1], got["jx"])


def test_graph_table():
    for E in N256:
        ii, jj, kk, k_range, n = _graph_lists(E, seed=3)
        cap = k_range                      # a slot per id, the last slot used

        def fn(ar):
            ws, nbytes = _graph_ws(ar, E, k_range)
            ti, tj, tk = ar.tensor("ii", ii, index_max=n - 1), ar.tensor("jj", jj, index_max=n - 1), ar.tensor("kk", kk, index_max=k_range - 1)
            ix, jx = ar.tensor("ix", (E,), I64, fill=-7), ar.tensor("jx", (E,), I64, fill=-7)
            ok(lib().cdv_graph_build_table(P(ti), P(tj), P(tk), E, P(ws), nbytes, E, k_range, cap, P(ix), P(jx), S()), "cdv_graph_build_table")
            assert _meta(ws)[6] == 0
            order = lib().cdv_graph_corr_order(P(ws))
            o = torch.empty(E, dtype=I32, device=DEV)
            s, e = ar.span("graph_ws")
            off = order - ws.data_ptr()
            assert 0 <= off and off + 4 * E <= e - s, "the correlation order lies outside the workspace"
            o.copy_(ws[off:off + 4 * E].view(I32))
            # inside a target-frame bin the order is arrival order (an LDS counter, graph.hip): only its canonical form is compared
            torch.cuda.synchronize()
            bins = jj[o.cpu().numpy()] % 32
            assert int((np.diff(bins) != 0).sum()) == len(np.unique(bins)) - 1, "the processing order is not grouped by jj mod 32"
            return {"ix": ix, "jx": jx, "order": o.sort().values}
        got = run("cdv_graph_build_table E=%d" % E, fn, row_bytes=8, capacity=1 << 23)
        ix_w, jx_w = O.neighbors(kk, jj)
        assert eq(got["ix"], ix_w) and eq(got["jx"], jx_w), E
        assert np.array_equal(got["order"], np.arange(E)), "the processing order is not a permutation"
        g = ops.GraphIndex(torch.device(DEV), E_cap=E, k_range=k_range, table_capacity=cap)
        g.build_table(T(jj), T(kk), ii=T(ii), with_neighbors=True)
        assert eq(g.neighbors()[0], got["ix"]) and eq(g.neighbors()[1], got["jx"])


# ---------------------------------------------------------------------------------------------------
# start of an update in one launch
# ---------------------------------------------------------------------------------------------------

def _prologue_inputs(E):
    C, H, W, slots, M, n = 8, 8, 12, 3, 4, 6
    poses, patches, intr, ix = _scene(n, M, 3, seed=E)
    Ng = n * M
    ii, jj, kk = _edges(E, n, Ng, ix, seed=5)
    f, g = _maps((C, H, W), E), _maps((Ng, C, 3, 3), E + 1)
    pre = (_pattern16((slots, H + 2 * PADY, W + 2 * PADX, C), 1), _pattern16((slots, H // 4 + 2 * PADY, W // 4 + 2 * PADX, C), 2),
           _pattern16((Ng, 9, C), 3))
    return C, H, W, slots, M, n, Ng, poses, patches, intr, ii, jj, kk, f, g, pre


def _check_prologue(got, E, inp, slot, gfirst, gcount):
    from tests.stream_audit import f16_ulps
    C, H, W, slots, M, n, Ng, poses, patches, intr, ii, jj, kk, f, g, pre = inp
    w1 = pre[0].copy()
    w1[slot, PADY:PADY + H, PADX:PADX + W] = f.transpose(1, 2, 0)
    assert eq(got["r1"], w1)
    w2 = got["r2"].copy()
    inner = (slot, slice(PADY, PADY + H // 4), slice(PADX, PADX + W // 4))
    lvl1 = w2[inner].copy()
    w2[inner] = pre[1][inner]
    assert eq(w2, pre[1])
    assert int(f16_ulps(torch.as_tensor(lvl1.transpose(2, 0, 1).copy()), torch.as_tensor(_pool4(f).astype(np.float16))).max()) <= 1
    wpm = pre[2].copy()
    wpm[gfirst:gfirst + gcount] = g[gfirst:gfirst + gcount].reshape(gcount, C, 9).transpose(0, 2, 1)
    assert eq(got["pm"], wpm)
    want = O.transform(poses, patches, intr, ii, jj, kk, dtype=np.float64)
    assert np.abs(got["coords"] - want.transpose(0, 3, 1, 2)).max() < 1e-3
    ix_w, jx_w = O.neighbors(kk, jj)
    assert eq(got["ix"], ix_w) and eq(got["jx"], jx_w)


def test_prologue_ranked():
    for E in N256:      # prologue.hip: n_tf = ceil(E / 256) reprojection workgroups next to the ingest and the histogram
        inp = _prologue_inputs(E)
        C, H, W, slots, M, n, Ng, poses, patches, intr, ii, jj, kk, f, g, pre = inp
        slot, gfirst, gcount = slots - 1, Ng - M, M

        def fn(ar):
            ws, nbytes = _graph_ws(ar, E, Ng)
            src, r1, r2 = ar.tensor("fmap_chw", f), ar.tensor("fmap1_nhwc", pre[0]), ar.tensor("fmap2_nhwc", pre[1])
            gp, pm = ar.tensor("gmap_planar", g), ar.tensor("gmap_pm", pre[2])
            tp, tpa, ti, tii, tjj, tkk = _carve_scene(ar, poses, patches, intr, ii, jj, kk)
            c = ar.tensor("coords", (E, 2, 3, 3), F32)
            ix, jx = ar.tensor("ix", (E,), I64, fill=-7), ar.tensor("jx", (E,), I64, fill=-7)
            ok(lib().cdv_update_prologue(P(src), P(r1), P(r2), slot, C, H, W, P(gp), P(pm), Ng, gfirst, gcount, P(tp), P(tpa), P(ti), P(tii),
                                         P(tjj), P(tkk), E, 1, P(c), P(ws), nbytes, E, Ng, P(ix), P(jx), S()), "cdv_update_prologue")
            return {"r1": r1, "r2": r2, "pm": pm, "coords": c, "ix": ix, "jx": jx}
        got = run("cdv_update_prologue E=%d" % E, fn, row_bytes=(W + 2 * PADX) * C * 2, capacity=1 << 23)
        _check_prologue(got, E, inp, slot, gfirst, gcount)
        sep = ops.transform(T(poses)[None], T(patches)[None], T(intr)[None], T(ii), T(jj), T(kk), layout_e2pp=True)
        assert eq(sep, got["coords"]), "the prologue's coords differ from cdv_transform's"
        gi = ops.GraphIndex(torch.device(DEV), E_cap=E, k_range=Ng)
        w1, w2, wpm = T(pre[0]).clone(), T(pre[1]).clone(), T(pre[2]).clone()
        wc = ops.update_prologue(gi, T(f), w1, w2, slot, T(g), wpm, gfirst, gcount, T(poses), T(patches), T(intr), T(ii), T(jj), T(kk))
        wix, wjx = gi.neighbors()
        assert eq(wc, got["coords"]) and eq(wix, got["ix"]) and eq(wjx, got["jx"]), "ops.update_prologue gives other bits"
        assert eq(w1, got["r1"]) and eq(w2, got["r2"]) and eq(wpm, got["pm"])


def test_prologue_table_and_corr_stream():
    """cdv_update_prologue_table, then cdv_corr_fused_stream on the packed stream it wrote into the workspace: the rings'
    last slot and the last tiles are the ones the new frame goes to and the edges read"""
    for E in N256 + [3, 5, 33]:
        inp = _prologue_inputs(E)
        C, H, W, slots, M, n, Ng, poses, patches, intr, ii, jj, kk, f, g, pre = inp
        slot, gfirst, gcount = slots - 1, Ng - M, M
        rng = np.random.default_rng(E)
        f0, f1 = _maps((slots, C, H, W), E + 2), _maps((slots, C, H // 4, W // 4), E + 3)
        f0[slot] = f
        patches = patches.copy()
        patches[:, 0] *= W / 128.0            # reprojections that land on the small maps
        patches[:, 1] *= H / 96.0
        intr2 = intr * np.float32(W / 128.0)
        inp = (C, H, W, slots, M, n, Ng, poses, patches, intr2, ii, jj, kk, f, g, pre)
        gfull = g.reshape(Ng, C, 9).transpose(0, 2, 1).copy()
        ring0, ring1 = _to_ring(f0), _to_ring(f1)

        def fn(ar):
            ws, nbytes = _graph_ws(ar, E, Ng)
            src, r1, r2 = ar.tensor("fmap_chw", f), ar.tensor("fmap1_nhwc", pre[0]), ar.tensor("fmap2_nhwc", pre[1])
            gp, pm = ar.tensor("gmap_planar", g), ar.tensor("gmap_pm", pre[2])
            tp, tpa, ti, tii, tjj, tkk = _carve_scene(ar, poses, patches, intr2, ii, jj, kk)
            c = ar.tensor("coords", (E, 2, 3, 3), F32)
            ix, jx = ar.tensor("ix", (E,), I64, fill=-7), ar.tensor("jx", (E,), I64, fill=-7)
            ok(lib().cdv_graph_bind_corr_stream(P(ws), P(c), Ng, slots, Ng, slots, 1.0), "cdv_graph_bind_corr_stream")
            ok(lib().cdv_update_prologue_table(P(src), P(r1), P(r2), slot, C, H, W, P(gp), P(pm), Ng, gfirst, gcount, P(tp), P(tpa), P(ti),
                                               P(tii), P(tjj), P(tkk), E, P(c), P(ws), nbytes, E, Ng, Ng, P(ix), P(jx), S()),
               "cdv_update_prologue_table")
            rec = lib().cdv_graph_corr_records(P(ws))
            s, e = ar.span("graph_ws")
            assert rec and 0 <= rec - ws.data_ptr() and rec - ws.data_ptr() + 96 * E <= e - s, "the record stream lies outside the workspace"
            # the correlation reads whole rings of its own (the prologue's are pattern-filled for the converter check)
            q0, q1, qg = ar.tensor("corr_fmap0", ring0), ar.tensor("corr_fmap1", ring1), ar.tensor("corr_gmap_pm", gfull)
            out = ar.tensor("corr_out", (E, 882), F16)
            ok(lib().cdv_corr_fused_stream(P(qg), P(q0), P(q1), rec, P(out), E, Ng, slots, C, H, W, H // 4, W // 4, 1.0, 4.0, 1, S()),
               "cdv_corr_fused_stream")
            return {"r1": r1, "r2": r2, "pm": pm, "coords": c, "ix": ix, "jx": jx, "corr": out}
        got = run("cdv_update_prologue_table E=%d" % E, fn, row_bytes=882 * 2, capacity=1 << 23)
        _check_prologue(got, E, inp, slot, gfirst, gcount)
        truth = O.slam_corr(g, f0, f1, got["coords"], kk % Ng, jj % slots, 3, "truth")
        assert np.isfinite(got["corr"]).all()
        assert np.abs(got["corr"].astype(np.float64) - truth).max() <= _corr_tol(truth), E
        w = ops.corr_fused(T(gfull), T(ring0), T(ring1), T(got["coords"])[None], T(kk), T(jj), kmod=Ng, jmod=slots, pixel_major=True)
        assert eq(w, got["corr"]), "the stream form differs from cdv_corr_fused on the same coordinates"
        gi = ops.GraphIndex(torch.device(DEV), E_cap=E, k_range=Ng, table_capacity=Ng)
        cbuf = torch.empty((1, E, 2, 3, 3), dtype=F32, device=DEV)
        gi.bind_corr_stream(cbuf, Ng, slots, Ng, slots)
        w1, w2, wpm = T(pre[0]).clone(), T(pre[1]).clone(), T(pre[2]).clone()
        wc = ops.update_prologue_table(gi, T(f), w1, w2, slot, T(g), wpm, gfirst, gcount, T(poses), T(patches), T(intr2), T(ii), T(jj), T(kk),
                                       coords_out=cbuf)
        wix, wjx = gi.neighbors()
        assert eq(wc, got["coords"]) and eq(wix, got["ix"]) and eq(wjx, got["jx"]), "ops.update_prologue_table gives other bits"
        assert eq(w1, got["r1"]) and eq(w2, got["r2"]) and eq(wpm, got["pm"])
        tg, t0, t1 = T(gfull), T(ring0), T(ring1)
        ws = ops.corr_fused_stream(tg, t0, t1, gi.corr_records_ptr(), E)
        torch.cuda.synchronize()
        assert eq(ws, got["corr"]), "ops.corr_fused_stream gives other bits"


# ---------------------------------------------------------------------------------------------------
# edge bookkeeping: filled exactly to capacity
# ---------------------------------------------------------------------------------------------------

def test_edges_frame_append():
    M, r = 8, 5
    for n in (1, 2, 5, 6, 9):      # edges.hip edges_frame_kernel: 256 lanes over M (r - 1) + M r new edges: 8, 24, 72, 72 ...
        g = EdgesPy()
        ix = np.repeat(np.arange(n), M).astype(np.int64)
        for E0 in (0, 3):
            g.ii = g.jj = g.kk = np.arange(E0, dtype=np.int64)
            g.append_factors(*g.edges_forw(n, M, r), ix)
            g.append_factors(*g.edges_back(n, M, r), ix)
            cap = len(g.ii)

            def fn(ar):
                ti, tj, tk = (ar.tensor(nm, np.concatenate([np.arange(E0), np.full(cap - E0, -7)]).astype(np.int64), index_max=n - 1)
                              for nm in ("ii", "jj", "kk"))
                tix = ar.tensor("ix", ix, index_max=n - 1)
                added = ctypes.c_int64(-1)
                ok(lib().cdv_edges_frame(P(ti), P(tj), P(tk), P(tix), E0, cap, n, M, r, ctypes.addressof(added), S()), "cdv_edges_frame")
                assert added.value == cap - E0
                return {"ii": ti, "jj": tj, "kk": tk}
            got = run("cdv_edges_frame n=%d" % n, fn, row_bytes=8)
            assert eq(got["ii"], g.ii) and eq(got["jj"], g.jj) and eq(got["kk"], g.kk), (n, E0)
    n = 7
    ix = np.repeat(np.arange(n), M).astype(np.int64)
    for count in N256:
        rng = np.random.default_rng(count)
        nk, nj = rng.integers(0, n * M, count).astype(np.int64), rng.integers(0, n, count).astype(np.int64)
        nk[0], nk[-1] = n * M - 1, (0 if count > 1 else n * M - 1)
        E0 = 5
        cap = E0 + count
        base = np.concatenate([np.arange(E0), np.full(count, -7)]).astype(np.int64)

        def fn(ar):
            ti, tj, tk = (ar.tensor(nm, base, index_max=n - 1) for nm in ("ii", "jj", "kk"))
            tix = ar.tensor("ix", ix, index_max=n - 1)
            tnk, tnj = ar.tensor("new_k", nk, index_max=n * M - 1), ar.tensor("new_j", nj, index_max=n - 1)
            ok(lib().cdv_edges_append(P(ti), P(tj), P(tk), P(tix), P(tnk), P(tnj), E0, count, cap, S()), "cdv_edges_append")
            return {"ii": ti, "jj": tj, "kk": tk}
        got = run("cdv_edges_append count=%d" % count, fn, row_bytes=8)
        head = np.arange(E0)
        assert eq(got["kk"], np.concatenate([head, nk])) and eq(got["jj"], np.concatenate([head, nj])), count
        assert eq(got["ii"], np.concatenate([head, ix[nk]])), count


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("with_net", [False, True])
def test_edges_remove(store, with_net):
    NB = 12      # bytes of a hidden-state row
    for E in [1, 255, 256, 257, 1023, 1024, 1025, 2053]:      # edges.hip: grid_of(E, 1024, .) workgroups of 256 lanes
        rng = np.random.default_rng(E)
        ii, jj, kk = (rng.integers(0, 50, E).astype(np.int64) for _ in range(3))
        tgt, wgt = rng.standard_normal((E, 2)).astype(np.float32), rng.uniform(0, 1, (E, 2)).astype(np.float32)
        net = rng.integers(0, 255, (E, NB)).astype(np.uint8)
        last = np.zeros(E, bool)
        last[-1] = True
        for name, mask in (("all", np.ones(E, bool)), ("none", np.zeros(E, bool)), ("last", last), ("random", rng.uniform(size=E) < 0.4)):
            r0 = 3
            nrem = int(mask.sum())
            wsb = int(lib().cdv_edges_workspace_bytes(E))

            def fn(ar):
                rm = ar.tensor("remove", mask.astype(np.uint8))
                ws = ar.tensor("ws", (wsb,), U8)
                ins = [ar.tensor(nm, a, index_max=49) for nm, a in (("ii", ii), ("jj", jj), ("kk", kk), ("target", tgt), ("weight", wgt))]
                tn = ar.tensor("net", net) if with_net else None
                outs = [ar.tensor(nm + "_out", a.shape, t, fill=fl) for nm, a, t, fl in (("ii", ii, I64, -7), ("jj", jj, I64, -7),
                        ("kk", kk, I64, -7), ("target", tgt, F32, -7.0), ("weight", wgt, F32, -7.0))]
                no = ar.tensor("net_out", net.shape, U8, fill=0x5A) if with_net else None
                rs = [ar.tensor(nm + "_r", (r0 + nrem,) + a.shape[1:], t, fill=fl) for nm, a, t, fl in (("ii", ii, I64, -7),
                      ("jj", jj, I64, -7), ("kk", kk, I64, -7), ("target", tgt, F32, -7.0), ("weight", wgt, F32, -7.0))] if store else [None] * 5
                counts = (ctypes.c_int32 * 2)(-1, -1)
                ok(lib().cdv_edges_remove(P(rm), E, P(ws), *[P(t) for t in ins], P(tn), NB, *[P(t) for t in outs], P(no),
                                          *[P(t) for t in rs], r0, counts, S()), "cdv_edges_remove")
                torch.cuda.synchronize()
                assert list(counts) == [E - nrem, nrem]
                res = {"o%d" % i: t for i, t in enumerate(outs)}
                res["net_out"] = no
                res.update({"r%d" % i: t for i, t in enumerate(rs)})
                return res
            got = run("cdv_edges_remove %s E=%d" % (name, E), fn, row_bytes=NB)
            for i, a in enumerate((ii, jj, kk, tgt, wgt)):
                fillv = np.full((nrem,) + a.shape[1:], -7, a.dtype)
                assert eq(got["o%d" % i], np.concatenate([a[~mask], fillv])), (name, E, i)      # compacted; the rest untouched
                if store:
                    assert eq(got["r%d" % i], np.concatenate([np.full((r0,) + a.shape[1:], -7, a.dtype), a[mask]])), (name, E, i)
            if with_net:
                assert eq(got["net_out"], np.concatenate([net[~mask], np.full((nrem, NB), 0x5A, np.uint8)])), (name, E)


def test_keyframe_shifts():
    M = 4
    for E in N256:
        rng = np.random.default_rng(E)
        ii, jj = rng.integers(0, 12, E).astype(np.int64), rng.integers(0, 12, E).astype(np.int64)
        kk = ii * M + rng.integers(0, M, E)
        k = 5

        def fn(ar):
            ti, tj, tk = ar.tensor("ii", ii, index_max=11), ar.tensor("jj", jj, index_max=11), ar.tensor("kk", kk, index_max=12 * M - 1)
            ok(lib().cdv_edges_keyframe_shift(P(ti), P(tj), P(tk), E, k, M, S()), "cdv_edges_keyframe_shift")
            return {"ii": ti, "jj": tj, "kk": tk}
        got = run("cdv_edges_keyframe_shift E=%d" % E, fn, row_bytes=8)
        assert eq(got["kk"], np.where(ii > k, kk - M, kk)) and eq(got["ii"], np.where(ii > k, ii - 1, ii)), E
        assert eq(got["jj"], np.where(jj > k, jj - 1, jj)), E
    # frame buffers that end at their guard: 28-byte (4-byte pieces) and 16-byte slots, a ring whose LAST slot is read and written
    N, mem = 9, 4
    rng = np.random.default_rng(1)
    poses, intr = rng.standard_normal((N, 7)).astype(np.float32), rng.standard_normal((N, 4)).astype(np.float32)
    ring = _maps((mem, 5, 2, 8), 2)                # 160-byte slots
    big = rng.standard_normal((N, 1027)).astype(np.float32)      # 4108-byte slots: 1027 pieces, beyond one 256-lane workgroup trip
    for k, n in ((0, N), (N - 2, N), (3, 8), (7, 8), (2, 3)):
        def fn(ar):
            ts = [ar.tensor(nm, a) for nm, a in (("poses", poses), ("intrinsics", intr), ("ring", ring), ("big", big))]
            bufs = (_lib.FrameBuf * 4)()
            for b, t, mod in zip(bufs, ts, (0, 0, mem, 0)):
                b.base, b.slot_bytes, b.modulus = P(t), t[0].numel() * t.element_size(), mod
            ok(lib().cdv_frames_keyframe_shift(ctypes.cast(bufs, ctypes.c_void_p), 4, k, n, S()), "cdv_frames_keyframe_shift")
            return dict(zip(("poses", "intrinsics", "ring", "big"), ts))
        got = run("cdv_frames_keyframe_shift k=%d n=%d" % (k, n), fn, row_bytes=4108)
        want = [a.copy() for a in (poses, intr, ring, big)]
        for i in range(k, n - 1):
            for a, mod in zip(want, (0, 0, mem, 0)):
                a[i % mod if mod else i] = a[(i + 1) % mod if mod else i + 1].copy()
        for nm, w in zip(("poses", "intrinsics", "ring", "big"), want):
            assert eq(got[nm], w), (nm, k, n)


# ---------------------------------------------------------------------------------------------------
# bundle adjustment
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kw,tolname,index", [("small", {}, "small", "ranked"), ("small", dict(opt_window=15), "small", "ranked"),
                                                   ("global", {}, "global", "ranked"), ("small", {}, "small", "table"),
                                                   ("small", dict(opt_window=15), "small", "table")],
                         ids=["window", "mid15", "global", "window-table", "mid15-table"])
@pytest.mark.parametrize("debug", [False, True])
def test_ba_forward(name, kw, tolname, index, debug):
    """workspaces sized exactly by their byte queries, U_max == the number of unique patches (ranked index) resp. the table
    capacity (table index: the slab kernels work through every slot), dbg of the documented length, state arrays that end at
    the last frame / patch the graph uses
    (the global path, more than 32 free poses, takes the ranked index only: include/cdvslam_hip.h)"""
    from cdv_slam_amd import synth
    from tests import ba_checks
    st = synth.make_state(name, features=False, **kw)
    E, N = len(st.kk), st.n - st.t0
    kx = np.unique(st.kk)
    U = len(kx)
    k_range = int(st.kk.max() - st.kk.min() + 1)
    n_used, m_used = int(max(st.ii.max(), st.jj.max())) + 1, int(st.kk.max()) + 1
    poses0, patches0, intr = st.poses[:n_used].copy(), st.patches[:m_used].copy(), st.intrinsics[:1].copy()
    target, weight = st.target.reshape(-1, 2).astype(np.float32), st.weight.reshape(-1, 2).astype(np.float32)
    cap = k_range if index == "table" else 0      # a slot per id between the oldest and the newest patch with an edge
    assert cap <= 65536
    U_max = cap if index == "table" else U
    n6, Us = 6 * N, (U_max + 63) // 64 * 64
    dbg_len = n6 * n6 + 2 * n6 + 3 * Us + n6 * Us
    gb, bb = int(lib().cdv_graph_workspace_bytes(E, k_range)), int(lib().cdv_ba_workspace_bytes(E, U_max, N))

    def fn(ar):
        gws = ar.tensor("graph_ws", (gb,), U8)
        ok(lib().cdv_graph_workspace_init(P(gws), gb, E, k_range, S()), "cdv_graph_workspace_init")
        bws = ar.tensor("ba_ws", (bb,), U8)
        ok(lib().cdv_ba_workspace_init(P(bws), S()), "cdv_ba_workspace_init")
        tp, tpa, ti = ar.tensor("poses", poses0), ar.tensor("patches", patches0), ar.tensor("intrinsics", intr)
        tt, tw, tl = ar.tensor("target", target), ar.tensor("weight", weight), ar.tensor("lmbda", np.array([st.lmbda], np.float32))
        tii, tjj, tkk = (ar.tensor("ii", st.ii, index_max=n_used - 1), ar.tensor("jj", st.jj, index_max=n_used - 1),
                         ar.tensor("kk", st.kk, index_max=m_used - 1))
        dbg = ar.tensor("dbg", (dbg_len,), F32) if debug else None
        if index == "table":
            ok(lib().cdv_graph_build_table(P(tii), P(tjj), P(tkk), E, P(gws), gb, E, k_range, cap, None, None, S()), "cdv_graph_build_table")
        else:
            ok(lib().cdv_graph_build_edges(P(tii), P(tjj), P(tkk), E, P(gws), gb, E, k_range, None, None, S()), "cdv_graph_build_edges")
        ok(lib().cdv_ba_forward(P(tp), P(tpa), P(ti), P(tt), P(tw), P(tl), P(tii), P(tjj), P(tkk), E, 3, st.t0, st.n, 2, P(gws), P(bws), bb,
                                U_max, P(dbg), S()), "cdv_ba_forward")
        info = (ctypes.c_int32 * 4)()
        assert lib().cdv_ba_status(P(bws), info, S()) == 0, list(info)
        lib().cdv_workspace_forget(P(gws))
        lib().cdv_workspace_forget(P(bws))
        return {"poses": tp, "patches": tpa, "dbg": dbg}
    got = run("cdv_ba_forward %s" % name, fn, row_bytes=4 * max(n6, 64), capacity=max(1 << 25, 2 * (gb + bb) + (1 << 24)))
    p64, x64, info = O.fastba(st.poses, st.patches, st.intrinsics[0], st.target, st.weight, st.lmbda, st.ii, st.jj, st.kk, st.t0, st.n, 2,
                              np.float64)
    assert info == 0
    poses, patches = st.poses.copy(), st.patches.copy()
    poses[:n_used], patches[:m_used] = got["poses"], got["patches"]
    ba_checks.check_end_state(tolname, st, poses, patches, p64, x64)
    assert eq(got["poses"][:st.t0], poses0[:st.t0]), "a pose outside [t0, t1) changed"
    untouched = np.setdiff1d(np.arange(m_used), kx)
    assert eq(got["patches"][untouched], patches0[untouched]), "a patch without an edge changed"
    # the wrapper's ordinary call on an index of the same form
    g = ops.GraphIndex(torch.device(DEV), E_cap=E, k_range=k_range, table_capacity=cap or None)
    wp, wpa = T(poses0).clone(), T(patches0).clone()
    wd = ops.ba_forward(wp, wpa, T(intr), T(target), T(weight), torch.tensor([st.lmbda], dtype=F32, device=DEV), T(st.ii), T(st.jj), T(st.kk),
                        0, st.t0, st.n, 2, debug=debug, U_max=U_max, graph=g)
    torch.cuda.synchronize()
    assert g.is_table == (index == "table")
    assert eq(wp, got["poses"]) and eq(wpa, got["patches"]), "the wrapper's call gives other bits"
    if debug and index == "ranked":
        assert eq(wd["S"], got["dbg"][:n6 * n6]) and eq(wd["y"], got["dbg"][n6 * n6:n6 * n6 + n6])
