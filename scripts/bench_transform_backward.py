"""Time projective_ops.transform forward + backward at the training shapes and write profiles/transform_bwd_bench.json.

n = 15 frames, P = 3, the edge set the reference's training forward builds (net_cdv.py:504-505: every patch of the 15 frames
against every frame), at 80 and at 1530 patches per frame (E = 18,000 and 344,250).  Two contenders on the same inputs,
alternating in one process:
  fused      projective_ops.transform under autograd: cdv_transform forward, cdv_transform_bwd backward
  composed   what training used before the fused backward: the reference's formula over this package's iproj / proj and
             differentiable Lie classes (a dozen launches each way)
The loss is the net_cdv.py pattern (`coords.permute(0, 1, 4, 2, 3).contiguous()` weighted and summed).  Forward and backward are
timed apart (the backward as `torch.autograd.grad` on a graph kept alive) with HIP events; each figure is the median over
`--iters` batches of `--batch` calls after a warm-up, three alternating rounds, the median round kept.  Gradients of the two
contenders are compared before anything is timed.

    python scripts/bench_transform_backward.py [--iters N] [--batch B] [--out PATH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cdv_slam_amd import ops  # noqa: E402
from cdv_slam_amd import projective_ops as pops  # noqa: E402
from cdv_slam_amd.lietorch import SE3  # noqa: E402

DEV = "cuda:0"
FRAMES, P = 15, 3


def timed(fn, iters, batch, warmup=3):
    """median microseconds per call over `iters` event-timed batches of `batch` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / batch)
    ts.sort()
    return {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}


def make_inputs(ppi, gen):
    n, m = FRAMES, FRAMES * ppi
    poses = ops.lie_op(3, "exp", 0.1 * torch.randn(n, 6, device=DEV, generator=gen))[None]
    intr = torch.tensor([[38.0, 41.0, 23.5, 15.0]], device=DEV).repeat(n, 1)[None] + 0.1 * torch.rand(1, n, 4, device=DEV, generator=gen)
    cx = 2 + 42 * torch.rand(m, device=DEV, generator=gen)
    cy = 2 + 25 * torch.rand(m, device=DEV, generator=gen)
    off = torch.arange(P, device=DEV, dtype=torch.float32) - P // 2
    patches = torch.empty(1, m, 3, P, P, device=DEV)
    patches[0, :, 0] = cx[:, None, None] + off[None, None, :]
    patches[0, :, 1] = cy[:, None, None] + off[None, :, None]
    patches[0, :, 2] = 0.2 + 0.8 * torch.rand(m, P, P, device=DEV, generator=gen)
    ix = torch.arange(m, device=DEV) // ppi
    kk, jj = (t.reshape(-1) for t in torch.meshgrid(torch.arange(m, device=DEV), torch.arange(n, device=DEV), indexing="ij"))
    return poses, patches, intr, ix[kk].contiguous(), jj.contiguous(), kk.contiguous()


def fused_forward(poses, patches, intr, ii, jj, kk):
    return pops.transform(SE3(poses), patches, intr, ii, jj, kk)


def composed_forward(poses, patches, intr, ii, jj, kk):
    G = SE3(poses)
    Gij = G[:, jj] * G[:, ii].inv()
    X1 = Gij[:, :, None, None] * pops.iproj(patches[:, kk], intr[:, ii])
    return pops.proj(X1, intr[:, jj])


def bench_shape(ppi, iters, batch, gen):
    poses, patches, intr, ii, jj, kk = make_inputs(ppi, gen)
    E, n, m = ii.numel(), FRAMES, patches.shape[1]
    w = torch.randn(1, E, 2, P, P, device=DEV, generator=gen)
    ways = {"fused": fused_forward, "composed": composed_forward}
    grads, state = {}, {}
    for k, fwd in ways.items():
        p, x = poses.clone().requires_grad_(), patches.clone().requires_grad_()
        loss = (fwd(p, x, intr, ii, jj, kk).permute(0, 1, 4, 2, 3).contiguous() * w).sum()
        state[k] = (p, x, loss)
        grads[k] = torch.autograd.grad(loss, (p, x), retain_graph=True)
    scale = [float(g.abs().max()) for g in grads["fused"]]
    agree = {"dposes_max_abs_difference": float((grads["fused"][0] - grads["composed"][0]).abs().max()), "dposes_scale": scale[0],
             "dpatches_max_abs_difference": float((grads["fused"][1] - grads["composed"][1]).abs().max()), "dpatches_scale": scale[1]}

    def forward_of(k):
        p, x, _ = state[k]
        return lambda: (ways[k](p, x, intr, ii, jj, kk).permute(0, 1, 4, 2, 3).contiguous() * w).sum()

    def backward_of(k):
        p, x, loss = state[k]
        return lambda: torch.autograd.grad(loss, (p, x), retain_graph=True)

    res = {k: {"forward": [], "backward": []} for k in ways}
    for _ in range(3):
        for k in ways:
            res[k]["forward"].append(timed(forward_of(k), iters, batch))
            res[k]["backward"].append(timed(backward_of(k), iters, batch))
    out = {k: {part: sorted(v, key=lambda r: r["median_us"])[1] for part, v in parts.items()} for k, parts in res.items()}
    for k in out:
        out[k]["total_median_us"] = out[k]["forward"]["median_us"] + out[k]["backward"]["median_us"]
    PP = P * P
    return {"ppi": ppi, "E": E, "n": n, "m": m, "P": P, "timing": out,
            "fused_over_composed": out["fused"]["total_median_us"] / out["composed"]["total_median_us"], "agreement": agree,
            # what has to move: forward inputs + coords out; backward the same inputs + grad in, the gradients out
            "algorithmic_bytes": {"forward": 4 * (7 * n + 4 * n + 3 * PP * m + 2 * PP * E) + 8 * 3 * E,
                                  "backward": 4 * (7 * n + 4 * n + 3 * PP * m + 2 * PP * E + 7 * n + 3 * PP * m) + 8 * 3 * E,
                                  "backward_workspace_traffic": 2 * 4 * (3 * PP * E + 2 * E)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_bwd_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transform_backward: needs the GPU (no CPU fallback, no CPU timing)")
    gen = torch.Generator(device=DEV).manual_seed(0)
    out = {"shapes": [bench_shape(ppi, args.iters, args.batch, gen) for ppi in (80, 1530)], "iters": args.iters, "batch": args.batch,
           "timed": "forward = transform + permute/contiguous + weighted sum; backward = torch.autograd.grad of that loss by poses and patches",
           "device": torch.cuda.get_device_name(0), "library": ops.version()}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
