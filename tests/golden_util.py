"""TEST INFRASTRUCTURE: loaders for the benchmark-size fixtures of tests/golden/make_golden.py (`bench-size`)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rebuild_patches(xy, d):
    """[P,2,3] grid values + [P] inverse depth -> patches [P,3,3,3] (x plane, y plane, inverse depth plane)"""
    P = len(d)
    patches = np.empty((P, 3, 3, 3), np.float32)
    patches[:, 0] = xy[:, 0, None, :]
    patches[:, 1] = xy[:, 1, :, None]
    patches[:, 2] = d[:, None, None]
    return patches


def load_ba_pr1():
    """BASELINE configs[0]: inputs of the reference's ba.py run + its outputs after one and two calls"""
    g = dict(np.load(os.path.join(GOLDEN, "ba_py_pr1.npz")))
    n, M = int(g["frames"]), int(g["M"])
    g["patches"] = rebuild_patches(g["patch_xy"], g["patch_d"])
    kk, jj = np.meshgrid(np.arange(n * M), np.arange(n), indexing="ij")     # fully connected: every patch to every frame
    g["kk"], g["jj"] = kk.reshape(-1).astype(np.int64), jj.reshape(-1).astype(np.int64)
    g["ii"] = g["kk"] // M
    return g


def load_pops_small():
    g = dict(np.load(os.path.join(GOLDEN, "pops_small_f32.npz")))
    g["patches"] = rebuild_patches(g["patch_xy"], g["patch_d"])
    return g


# ---------------------------------------------------------------------------------------------------
# round 6: the EuRoC settings (tests/golden/make_golden.py euroc)
# ---------------------------------------------------------------------------------------------------

CORR_EUROC_SEED = 20261016


def sha256_u8(a):
    """sha256 of an array's bytes as 32 uint8 (the fixtures hold numeric arrays only)"""
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def euroc_window_state():
    """the `tiny` window graph (6 frames x 8 patches, poses 2..5 free) at 480x752 with the EuRoC calibration, six patches
    moved to the right of the image so that their edges reproject around x = 2 cx + 64 = 247.6 (fastba's in-bounds gate,
    ba_cuda.cu:305-306) and W + 64 = 252 (what that gate would be with cx == W / 2); their targets follow them"""
    from cdv_slam_amd import synth
    st = synth.make_state("tiny", features=False, ht=480, wd=752, intr=synth.EUROC_INTR)
    M = st.cfg.M
    moved = M * np.arange(1, 6) + 3                         # one patch of each free frame ...
    moved = np.append(moved, 2 * M + 6)                     # ... and a second one in frame 2
    xs = np.array([243.38, 249.28, 245.27, 251.19, 248.3, 251.12], np.float32)
    st.patches[moved, 0] += (xs - st.patches[moved, 0, 1, 1])[:, None, None]
    rng = np.random.default_rng(6)
    e = np.isin(st.kk, moved)
    centres = st.patches[:, :2, 1, 1].astype(np.float64)
    proj = synth._reproject_centres(st.poses.astype(np.float64), centres, st.patches[:, 2, 1, 1].astype(np.float64),
                                    st.intrinsics[0].astype(np.float64), st.ii[e], st.jj[e], st.kk[e])
    st.target[e] = (proj + rng.normal(0, 0.25, proj.shape)).astype(np.float32)
    st.t0 = 2           # two fixed poses: one fixed pose leaves scale to the damping alone (tests/ba_checks.py)
    return st


def euroc_gate_band(st, poses=None):
    """edges whose centre reprojects (fastba's projection, float64) into 2 cx + 64 < u < W + 64: masked by the calibrated
    gate, kept by an image-size one"""
    from oracle import oracle as O
    poses = st.poses if poses is None else poses
    u = O.fastba_reproject(poses, st.patches, st.intrinsics[0], st.ii, st.jj, st.kk, dtype=np.float64)[:, 0, 1, 1]
    cx = np.float64(st.intrinsics[0, 2])
    return (u > 2 * cx + 64) & (u < st.cfg.wd // st.cfg.res + 64)


def corr_pin_euroc_inputs():
    """inputs of corr_pin_euroc.npz: level-0 maps 120x188 drawn from CORR_EUROC_SEED, level 1 (30x47, an odd width) as
    slam.py:682 makes it (torch's 4x4 average pool, stored in half), patch features, and 96 edges of which most aim at the
    right / bottom border of level 1 (level-1 x in {46, 46.5, 47.25, 49.75}, y in {29, 29.5, 30.25, 32.75}) or have wide
    footprints"""
    import torch
    rng = np.random.default_rng(CORR_EUROC_SEED)
    mem, C, H, W, Ng, E = 2, 24, 120, 188, 24, 96
    fmap1 = (rng.standard_normal((mem, C, H, W)) / 4).astype(np.float16)
    fmap2 = torch.nn.functional.avg_pool2d(torch.from_numpy(fmap1).float(), 4, 4).half().numpy()
    gmap = (rng.standard_normal((Ng, C, 3, 3)) / 4).astype(np.float16)
    cx, cy = rng.uniform(8, W - 8, E), rng.uniform(8, H - 8, E)
    sc = rng.uniform(0.5, 1.6, E)
    right, bottom = [46.0, 46.5, 47.25, 49.75], [29.0, 29.5, 30.25, 32.75]
    for a, x1 in enumerate(right):                      # the odd right edge, with the bottom border and the corner
        cx[4 * a:4 * a + 4] = 4 * x1
        cy[4 * a + 1:4 * a + 4] = [4 * y for y in bottom[:3]]
    cy[16:20] = [4 * y for y in bottom]                 # the bottom border alone
    sc[16:24] = [1.0, 2.5, 1.0, 2.5, 1.0, 2.5, 1.0, 2.5]
    cy[20:24] = [4 * y for y in bottom]
    cx[24:32] = [4 * 45.5, 4 * 46.75, 4 * 44.0, 4 * 47.0, 180.0, 150.0, 4 * 46.25, 4 * 48.0]     # wide footprints
    cy[24:32] = [4 * 28.0, 4 * 29.25, 100.0, 4 * 30.0, 4 * 29.75, 4 * 29.5, 60.0, 4 * 31.0]
    sc[24:32] = [4.0, 6.0, 8.0, 10.0, 5.5, 7.25, 9.0, 12.0]
    cx[32:36] = [W - 1.0, W - 0.5, W - 1.75, 0.0]      # the level-0 borders
    cy[32:36] = [H - 1.0, 50.0, H - 0.25, H - 1.0]
    off = np.arange(3.0) - 1
    coords = np.empty((E, 2, 3, 3), np.float32)
    coords[:, 0] = cx[:, None, None] + sc[:, None, None] * off[None, None, :]
    coords[:, 1] = cy[:, None, None] + sc[:, None, None] * off[None, :, None]
    ii = rng.integers(0, Ng, E).astype(np.int64)
    jj = rng.integers(0, mem, E).astype(np.int64)
    return dict(fmap1=fmap1, fmap2=fmap2, gmap=gmap, coords=coords, ii=ii, jj=jj)


def load_corr_pin_euroc():
    """corr_pin_euroc.npz with its feature maps regenerated from the stored seed (and checked against their stored sha256)"""
    g = dict(np.load(os.path.join(GOLDEN, "corr_pin_euroc.npz")))
    assert int(g["seed"]) == CORR_EUROC_SEED
    z = corr_pin_euroc_inputs()
    assert z["fmap1"].shape == tuple(g["shape"])
    assert np.array_equal(sha256_u8(z["fmap1"]), g["fmap1_sha256"]), "corr_pin_euroc: level-0 map generator changed"
    assert np.array_equal(sha256_u8(z["fmap2"]), g["fmap2_sha256"]), "corr_pin_euroc: level-1 map generator changed"
    for k in ("gmap", "coords", "ii", "jj"):
        assert np.array_equal(z[k], g[k]), k
    g["fmap1"], g["fmap2"] = z["fmap1"], z["fmap2"]
    return g
