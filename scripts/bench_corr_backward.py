"""Time the altcorr backward passes (ops.corr_backward / ops.patchify_backward) at the training shapes and print one
JSON line: HIP-event medians, algorithmic bytes, the fraction of an 8 TB/s roofline, and, at the sparse shape, a torch
composition of the reference's stages (index_put_ slices for the blend adjoint, index_add_ for the scatters).

    python scripts/bench_corr_backward.py [--iters N] [--no-torch]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdv_slam_amd import ops  # noqa: E402

DEV = "cuda:0"
ROOF = 8e12      # bytes / s


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def corr_case(n_frames, ppi, M, C, H, W, level, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    N1 = n_frames * ppi
    f1 = torch.randn(1, N1, C, 3, 3, device=DEV, generator=g)
    f2 = torch.randn(1, n_frames, C, H // level, W // level, device=DEV, generator=g)
    x = torch.rand(1, M, 1, 1, 1, device=DEV, generator=g) * W
    y = torch.rand(1, M, 1, 1, 1, device=DEV, generator=g) * H
    coords = (torch.cat([x, y], 2) + torch.randn(1, M, 2, 3, 3, device=DEV, generator=g)) / level
    ii = torch.randint(0, N1, (M,), device=DEV, generator=g)
    jj = torch.randint(0, n_frames, (M,), device=DEV, generator=g)
    grad = torch.randn(1, M, 7, 7, 3, 3, device=DEV, generator=g)
    return f1, f2, coords, ii, jj, grad


def corr_bytes(f1, f2, coords, grad):
    M = coords.shape[1]
    return (grad.numel() * 4 + coords.numel() * 4 + M * 16 + 2 * (f1.numel() + f2.numel()) * 4)


def torch_corr_backward(f1, f2, coords, ii, jj, grad, r):
    """the reference's stages (correlation_kernel.cu:236-285, :139-190) as torch ops, batch 1"""
    D = 2 * r + 2
    N1, C, P = f1.shape[1], f1.shape[2], f1.shape[3]
    N2, H, W = f2.shape[1], f2.shape[3], f2.shape[4]
    M = coords.shape[1]
    g = grad.permute(0, 1, 3, 2, 4, 5)
    x, y = coords[:, :, 0, None, None], coords[:, :, 1, None, None]
    dx, dy = x - x.floor(), y - y.floor()
    shape = (1, M, D, D, P, P)
    g1, g2, g3, g4 = (torch.zeros(shape, device=DEV) for _ in range(4))
    g1[:, :, :D - 1, :D - 1] = (1 - dx) * (1 - dy) * g
    g2[:, :, :D - 1, 1:] = dx * (1 - dy) * g
    g3[:, :, 1:, :D - 1] = (1 - dx) * dy * g
    g4[:, :, 1:, 1:] = dx * dy * g
    cg = (g1 + g2 + g3 + g4)[0]                                              # [M,D,D,P,P]
    off = torch.arange(D, device=DEV) - r
    rows = coords[0, :, 1].floor().long()[:, None, None] + off[None, :, None, None, None]   # [M,D,1,P,P]
    cols = coords[0, :, 0].floor().long()[:, None, None] + off[None, None, :, None, None]   # [M,1,D,P,P]
    inside = (rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)
    pix = (rows.clamp(0, H - 1) * W + cols.clamp(0, W - 1)).expand(M, D, D, P, P)
    cg = torch.where(inside, cg, torch.zeros((), device=DEV))
    idx = ((jj[:, None] * C + torch.arange(C, device=DEV)[None])[:, :, None, None, None, None] * (H * W)
           + pix[:, None])                                                   # [M,C,D,D,P,P]
    samples = f2.reshape(-1)[idx]
    d1 = (cg[:, None] * samples).sum((2, 3))                                  # [M,C,P,P]
    fg1 = torch.zeros_like(f1[0]).index_add_(0, ii, d1)
    contrib = cg[:, None] * f1[0][ii][:, :, None, None]                      # [M,C,D,D,P,P]
    fg2 = torch.zeros(N2 * C * H * W, device=DEV).index_add_(0, idx.reshape(-1), contrib.reshape(-1))
    return fg1, fg2.view(N2, C, H, W)


def patch_case(n_frames, ppi, C, H, W, r, dtype, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    net = torch.randn(n_frames, C, H, W, device=DEV, generator=g).to(dtype)
    coords = torch.stack([torch.rand(n_frames, ppi, device=DEV, generator=g) * W,
                          torch.rand(n_frames, ppi, device=DEV, generator=g) * H], -1)
    D = 2 * r + 2
    pg = torch.randn(n_frames, ppi, C, D, D, device=DEV, generator=g).to(dtype)
    return net, coords, pg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    res = {"metric": "altcorr_backward_us", "roofline_TBps": ROOF / 1e12, "corr": {}, "patchify": {}}
    H, W, NF = 120, 160, 15
    corr_shapes = [("sparse_l0", 80, 18000, 24, 1), ("sparse_l1", 80, 18000, 24, 4),
                   ("dense_l0", 1530, 340000, 24, 1), ("dense_l1", 1530, 340000, 24, 4),
                   ("dpvo_c128_l0", 96, 18000, 128, 1), ("dpvo_c128_l1", 96, 18000, 128, 4)]
    for name, ppi, M, C, lev in corr_shapes:
        f1, f2, coords, ii, jj, grad = corr_case(NF, ppi, M, C, H, W, lev)
        t = timed(lambda: ops.corr_backward(f1, f2, coords, ii, jj, grad, 3), a.iters)
        nb = corr_bytes(f1, f2, coords, grad)
        row = {"M": M, "C": C, "H": H // lev, "W": W // lev, "us": round(t, 1), "MB": round(nb / 1e6, 1),
               "roofline_frac": round(nb / ROOF / (t * 1e-6), 4)}
        if name.startswith("sparse") and not a.no_torch:
            tt = timed(lambda: torch_corr_backward(f1, f2, coords, ii, jj, grad, 3), max(3, a.iters // 4), warmup=1)
            row["torch_us"] = round(tt, 1)
            row["speedup_vs_torch"] = round(tt / t, 1)
        res["corr"][name] = row
        del f1, f2, coords, ii, jj, grad
        torch.cuda.empty_cache()
    for name, ppi, C, r in [("gmap_ppi80", 80, 24, 1), ("gmap_ppi1530", 1530, 24, 1),
                            ("imap_ppi80", 80, 384, 0), ("imap_ppi1530", 1530, 384, 0)]:
        dtype = torch.float32
        net, coords, pg = patch_case(NF, ppi, C, H, W, r, dtype)
        t = timed(lambda: ops.patchify_backward(net, coords, pg, r), a.iters)
        nb = pg.numel() * pg.element_size() + coords.numel() * 4 + net.numel() * net.element_size()
        row = {"B": NF, "M": ppi, "C": C, "r": r, "us": round(t, 1), "MB": round(nb / 1e6, 2),
               "roofline_frac": round(nb / ROOF / (t * 1e-6), 4)}
        if ppi == 80 and not a.no_torch:
            D = 2 * r + 2

            def torch_patch():
                off = torch.arange(D, device=DEV) - r
                rows = coords[..., 1].floor().long()[:, :, None, None] + off[None, None, :, None]
                cols = coords[..., 0].floor().long()[:, :, None, None] + off[None, None, None, :]
                ok = (rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)
                pix = (rows.clamp(0, H - 1) * W + cols.clamp(0, W - 1)).expand(NF, ppi, D, D)
                bc = (torch.arange(NF, device=DEV)[:, None, None] * C + torch.arange(C, device=DEV)[None, None, :])
                idx = bc[:, :, :, None, None] * (H * W) + pix[:, :, None]
                v = torch.where(ok[:, :, None], pg, torch.zeros((), device=DEV, dtype=pg.dtype))
                return torch.zeros(net.numel(), device=DEV, dtype=dtype).index_add_(0, idx.reshape(-1), v.reshape(-1))

            tt = timed(torch_patch, max(3, a.iters // 4), warmup=1)
            row["torch_us"] = round(tt, 1)
            row["speedup_vs_torch"] = round(tt / t, 1)
        res["patchify"][name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
