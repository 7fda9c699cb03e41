"""A plain numpy truth for the backward of the fused projective_ops.transform, next to tests/lie_grad_truth.py and in its style.

Forward (projective_ops.py:53-69 of the reference): per edge e with i, j, k = ii, jj, kk[e]
    X0 = ((x - cx_i) / fx_i, (y - cy_i) / fy_i, 1, d),  G = Gj Gi^-1,  X1 = G X0,  D = 1 / max(Z, 0.1),
    (u, v) = (fx_j D X + cx_j, fy_j D Y + cy_j)
Backward, composed from the closed forms of lie_grad_truth.vjp (act4, mul, inv) and the two pinhole maps: with the incoming
gradient (gu, gv) of a pixel
    q = (fx_j D gu, fy_j D gv, -[Z >= 0.1] D^2 (fx_j X gu + fy_j Y gv), 0)
    act4:  dG = q [[X1_w I, -[X1_xyz]x], [0]] summed over the pixels of the edge,  dX0 = q M(G)
    mul:   dGj = dG,  dGi^-1 = dG Ad(Gj);      inv:  dGi = -dGi^-1 Ad(Gi^-1)
    dpatches[k] += (dX0_x / fx_i, dX0_y / fy_i, dX0_w);   dposes[j] += dGj;   dposes[i] += dGi
The pose gradient is the package's: the left-perturbation row vector in words 0..5 of the 7-word row, word 6 zero.

`forward` / `vjp` take a dtype as lie_truth does (REF is the truth; float32 says what the format costs and gives the tests
their bound); `fd_vjp` is central differences (h = 2^-16, poses moved as Exp(h e_k) X) of `forward` in REF alone.
`make_case` fixes the inputs of the GPU tests (tests/test_transform_backward.py); tests/test_pops_grad_truth_cpu.py holds vjp
against fd_vjp and asserts the conditions on those inputs."""
import numpy as np

import lie_cases as LC
import lie_grad_truth as GT
import lie_truth as LT

REF, SE3 = LT.REF, LT.SE3
H = GT.H
U32 = LC.U[np.dtype(np.float32)]
CLAMP = 0.1
CLAMP_MARGIN = 1e-3          # every pixel's Z is at least this far from the clamp, so that float32 takes the truth's branch


def _edge_terms(poses, patches, intr, ii, jj, kk, dtype):
    poses, patches, intr = (np.asarray(a, dtype) for a in (poses, patches, intr))
    m, _, P, _ = patches.shape
    PP = P * P
    pk = patches.reshape(m, 3, PP)[kk]                                   # [E, 3, PP]
    Ki, Kj = intr[ii], intr[jj]
    X0 = np.stack([(pk[:, 0] - Ki[:, 2:3]) / Ki[:, 0:1], (pk[:, 1] - Ki[:, 3:4]) / Ki[:, 1:2], np.ones_like(pk[:, 0]), pk[:, 2]], -1)
    Pi, Pj = poses[ii], poses[jj]
    Pinv = LT.se3_inv(Pi, dtype)
    G = LT.se3_mul(Pj, Pinv, dtype)
    Grep = np.repeat(G, PP, 0)
    X1 = LT.se3_act4(Grep, X0.reshape(-1, 4), dtype).reshape(len(ii), PP, 4)
    return Ki, Kj, X0, Pi, Pj, Pinv, Grep, X1


def forward(poses, patches, intr, ii, jj, kk, dtype=REF):
    """(coords [E, PP, 2], Z [E, PP])"""
    dt = np.dtype(dtype).type
    Ki, Kj, X0, Pi, Pj, Pinv, Grep, X1 = _edge_terms(poses, patches, intr, ii, jj, kk, dtype)
    D = dt(1) / np.maximum(X1[..., 2], dt(CLAMP))
    u = Kj[:, 0:1] * (D * X1[..., 0]) + Kj[:, 2:3]
    v = Kj[:, 1:2] * (D * X1[..., 1]) + Kj[:, 3:4]
    return np.stack([u, v], -1), X1[..., 2]


def edge_vjp(poses, patches, intr, ii, jj, kk, grad, dtype=REF):
    """per-edge contributions: (dGj [E, 7], dGi [E, 7], dpatch [E, 3, PP])"""
    dt = np.dtype(dtype).type
    E = len(ii)
    Ki, Kj, X0, Pi, Pj, Pinv, Grep, X1 = _edge_terms(poses, patches, intr, ii, jj, kk, dtype)
    PP = X1.shape[1]
    g = np.asarray(grad, dtype).reshape(E, PP, 2)
    X, Y, Z = X1[..., 0], X1[..., 1], X1[..., 2]
    D = dt(1) / np.maximum(Z, dt(CLAMP))
    fx, fy = Kj[:, 0:1], Kj[:, 1:2]
    q = np.stack([fx * D * g[..., 0], fy * D * g[..., 1],
                  np.where(Z >= dt(CLAMP), -(D * D) * (fx * X * g[..., 0] + fy * Y * g[..., 1]), dt(0)), np.zeros_like(Z)], -1)
    dG_px, dX0 = GT.vjp(SE3, "act4", q.reshape(-1, 4), Grep, X0.reshape(-1, 4), dtype=dtype)
    dG_px = dG_px.reshape(E, PP, 7)
    dG = dG_px[:, 0].copy()
    for p in range(1, PP):                                               # ascending pixels, every partial sum in `dtype`
        dG = dG + dG_px[:, p]
    dGj, dGinv = GT.vjp(SE3, "mul", dG, Pj, Pinv, dtype=dtype)
    dGi, _ = GT.vjp(SE3, "inv", dGinv, Pi, dtype=dtype)
    dX0 = dX0.reshape(E, PP, 4)
    dpatch = np.stack([dX0[..., 0] / Ki[:, 0:1], dX0[..., 1] / Ki[:, 1:2], dX0[..., 3]], 1)
    return dGj, dGi, dpatch


def vjp(poses, patches, intr, ii, jj, kk, grad, dtype=REF):
    """{dposes [n, 7], dpatches [m, 3, P, P]} and, under S_*, per output word the sum of the absolute values of its per-edge
    contributions.  Edges are added in ascending order, every partial sum in `dtype`."""
    n, (m, _, P, _) = len(poses), np.shape(patches)
    dGj, dGi, dpatch = edge_vjp(poses, patches, intr, ii, jj, kk, grad, dtype)
    out = {"dposes": np.zeros((n, 7), dtype), "dpatches": np.zeros((m, 3, P * P), dtype),
           "S_dposes": np.zeros((n, 7), dtype), "S_dpatches": np.zeros((m, 3, P * P), dtype)}
    for e in range(len(ii)):
        out["dposes"][jj[e]] += dGj[e]
        out["dposes"][ii[e]] += dGi[e]
        out["S_dposes"][jj[e]] += np.abs(dGj[e])
        out["S_dposes"][ii[e]] += np.abs(dGi[e])
        out["dpatches"][kk[e]] += dpatch[e]
        out["S_dpatches"][kk[e]] += np.abs(dpatch[e])
    for k in ("dpatches", "S_dpatches"):
        out[k] = out[k].reshape(m, 3, P, P)
    return out


def fd_vjp(poses, patches, intr, ii, jj, kk, grad, h=H):
    """{dposes, dpatches} by central differences of `forward` in REF"""
    poses, patches = np.asarray(poses, REF), np.asarray(patches, REF)
    n, m = len(poses), len(patches)
    g = np.asarray(grad, REF).reshape(len(ii), -1, 2)

    def loss(p, x):
        return (forward(p, x, intr, ii, jj, kk)[0] * g).sum()

    dposes = np.zeros((n, 7), REF)
    for f in range(n):
        for k in range(6):
            e = np.zeros((1, 6), REF)
            e[0, k] = REF(h)
            hi, lo = poses.copy(), poses.copy()
            hi[f] = LT.se3_mul(LT.se3_exp(e), poses[f:f + 1])[0]
            lo[f] = LT.se3_mul(LT.se3_exp(-e), poses[f:f + 1])[0]
            dposes[f, k] = (loss(hi, patches) - loss(lo, patches)) / REF(2 * h)
    dpatches = np.zeros(patches.shape, REF)
    flat = dpatches.reshape(-1)
    for w in range(flat.size):
        hi, lo = patches.copy().reshape(-1), patches.copy().reshape(-1)
        hi[w] += REF(h)
        lo[w] -= REF(h)
        flat[w] = (loss(poses, hi.reshape(patches.shape)) - loss(poses, lo.reshape(patches.shape))) / REF(2 * h)
    return {"dposes": dposes, "dpatches": dpatches}


def bounds(case, want=None):
    """(want, {name: per-word bound}): 4 |truth evaluated in float32 - truth| + 4 u max(1, S), S the sum of the absolute values
    of the word's per-edge contributions (the rule of lie_grad_truth.bounds, per output word)"""
    args = (case["poses"], case["patches"], case["intr"], case["ii"], case["jj"], case["kk"], case["grad"])
    want = vjp(*args) if want is None else want
    low = vjp(*args, dtype=np.float32)
    out = {}
    for k in ("dposes", "dpatches"):
        cost = np.abs(low[k].astype(REF) - want[k])
        out[k] = np.asarray(4 * cost + 4 * U32 * np.maximum(1.0, want["S_" + k]), np.float64)
    return want, out


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------

MAP_W, MAP_H = 47, 30
BEHIND = 1.2          # the last frame of a case is frame 0 pushed this far along -z: Z = 1 - 1.2 d over an edge 0 -> last


def make_case(E, n, P=3, m=None, seed=0, structure=False):
    """float32 inputs of one call, seeded.  Poses se3_exp(0.3 randn) with stored quaternions scaled by 1 +- 1e-3; per-frame
    intrinsics, four distinct values that differ between frames; pixel grids around centres inside a 47 x 30 map; inverse
    depths in [0.1, 2]; random edges.  n >= 2: the last frame is frame 0 translated along -z and the first edges go from frame
    0 to it, so that pixels land on both sides of the clamp (Z < 0.1, Z < 0).  Inverse depths are redrawn until every
    pixel's Z (float64) is at least CLAMP_MARGIN from the clamp.
    structure=True (the size tests): m >= 4; patch 0 has min(300, E // 2) duplicate edges (the same i, j), patch m - 1 has none,
    frame 1 is never a source and frame 2 never a target (n >= 4), and the last edge has ii == jj."""
    rng = np.random.default_rng(1000 * seed + 7 * E + n + 100 * P)
    m = m if m is not None else max(4, min(E, 40))
    poses = np.asarray(LT.se3_exp(0.3 * rng.standard_normal((n, 6))), np.float64)
    if n >= 2:
        back = np.zeros((1, 7))
        back[0, 2], back[0, 6] = -BEHIND, 1.0
        poses[n - 1] = np.asarray(LT.se3_mul(back, poses[0:1]), np.float64)[0]
    poses[:, 3:] *= 1.0 + 1e-3 * rng.choice([-1.0, 1.0], (n, 1))
    poses = poses.astype(np.float32)
    f = np.arange(n)[:, None]
    intr = (np.array([[38.0, 41.0, 23.5, 15.0]]) + f * np.array([[0.75, -0.5, 0.25, -0.125]])
            + rng.uniform(-0.05, 0.05, (n, 4))).astype(np.float32)
    centre = np.stack([rng.uniform(2, MAP_W - 3, m), rng.uniform(2, MAP_H - 3, m)], 1)
    off = np.arange(P) - P // 2
    patches = np.zeros((m, 3, P, P))
    patches[:, 0] = centre[:, 0, None, None] + off[None, None, :]
    patches[:, 1] = centre[:, 1, None, None] + off[None, :, None]
    patches[:, 2] = rng.uniform(0.1, 2.0, (m, P, P))
    ii, jj, kk = rng.integers(0, n, E), rng.integers(0, n, E), rng.integers(0, m, E)
    nb = min(3, E)                                   # edges 0 -> last frame: both sides of the clamp
    if structure:
        assert m >= 4
        kk = rng.integers(1, m - 1, E)
        if n >= 4:
            ii = np.where(ii == 1, 0, ii)
            jj = np.where(jj == 2, 3, jj)
        nb = min(300, E // 2)                            # a patch cannot have more edges than there are: half of them below 600
        kk[:nb] = 0
    else:
        kk[:nb] = np.arange(nb)
    ii[:nb], jj[:nb] = 0, n - 1
    if structure:
        ii[E - 1] = jj[E - 1] = 3 if n >= 4 else 0
    if n >= 2:                                           # over 0 -> last: Z = 1 - 1.2 d = -0.8 (behind), 0.04 (below the clamp), 0.64
        P2 = patches.reshape(m, 3, P * P)
        for e in range(nb):
            P2[kk[e], 2] = np.array([1.5, 0.8, 0.3])[(e * (0 if structure else 1) + np.arange(P * P)) % 3]
    patches = patches.astype(np.float32)
    for _ in range(64):
        Z = np.asarray(forward(poses, patches, intr, ii, jj, kk)[1], np.float64)
        bad = np.abs(Z - CLAMP) < 2 * CLAMP_MARGIN
        if not bad.any():
            break
        P2 = patches.reshape(m, 3, P * P)
        for e, p in zip(*np.nonzero(bad)):
            P2[kk[e], 2, p] = np.float32(rng.uniform(0.1, 2.0))
    grad = rng.standard_normal((E, P, P, 2)).astype(np.float32)
    return {"poses": poses, "patches": patches, "intr": intr, "ii": ii.astype(np.int64), "jj": jj.astype(np.int64),
            "kk": kk.astype(np.int64), "grad": grad, "E": E, "n": n, "m": m, "P": P}


def clamp_report(case):
    """(smallest |Z - 0.1|, pixels with Z >= 0.1, pixels with Z < 0.1, pixels with Z < 0) of a case, Z in float64"""
    Z = np.asarray(forward(case["poses"], case["patches"], case["intr"], case["ii"], case["jj"], case["kk"], np.float64)[1])
    return float(np.abs(Z - CLAMP).min()), int((Z >= CLAMP).sum()), int((Z < CLAMP).sum()), int((Z < 0).sum())


TRUTH_CASES = [(257, 5, 3), (257, 5, 1)]                          # (E, n, P) of the truth / reproducibility / capture tests
SIZES_E = [1, 255, 256, 257, 1000]
SIZES_N = [1, 4, 33, 65]
