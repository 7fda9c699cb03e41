"""Time the Lie-op backward (ops.lie_backward, cdv_lie_bwd) at the training shape and write profiles/lie_bwd_bench.json.

The act4 backward of one pose against its nine points (Gij[:, :, None, None] * X0 of projective_ops.transform), 47,712
poses x 9 points, float32, three ways, alternating in one process:
  grouped      the pose operand unexpanded, its gradient summed in the kernel
  expand_sum   the ungrouped call on expanded pose rows, then torch's sum over the nine rows
  torch        a torch composition of the same formulas (quaternion to matrix, matmul, cross, sum)
and the mul and log backward at 47,712 rows.  Each figure is the median over `--iters` HIP-event-timed batches of `--batch`
launches, after a warm-up of every shape; the outputs of the three ways are compared before anything is timed.

    python scripts/bench_lie_backward.py [--iters N] [--batch B] [--out PATH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cdv_slam_amd import ops  # noqa: E402

DEV = "cuda:0"
POSES, POINTS = 47712, 9


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


def torch_act4_backward(g, X, p):
    """dX [n, 7], dp [n * m, 4] of q = X p, pose rows X [n, 7] against points p [n, m, 4]"""
    t, q = X[:, :3], X[:, 3:] / X[:, 3:].norm(dim=1, keepdim=True)
    x, y, z, w = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    g3, pw = g[..., :3], p[..., 3:]
    qv = torch.matmul(p[..., :3], R.transpose(1, 2)) + pw * t[:, None]
    dp = torch.cat([torch.matmul(g3, R), (g3 * t[:, None]).sum(-1, keepdim=True) + g[..., 3:]], -1)
    dX = torch.cat([(pw * g3).sum(1), torch.linalg.cross(qv, g3).sum(1), X.new_zeros(len(X), 1)], 1)
    return dX, dp.reshape(-1, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lie_bwd_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lie_backward: needs the GPU (no CPU fallback, no CPU timing)")
    gen = torch.Generator(device=DEV).manual_seed(0)
    n, m = POSES, POINTS
    X = ops.lie_op(3, "exp", 0.3 * torch.randn(n, 6, device=DEV, generator=gen))
    Y = ops.lie_op(3, "exp", 0.3 * torch.randn(n, 6, device=DEV, generator=gen))
    p = torch.randn(n * m, 4, device=DEV, generator=gen)
    g4 = torch.randn(n * m, 4, device=DEV, generator=gen)
    g7 = torch.randn(n, 7, device=DEV, generator=gen)
    g6 = torch.randn(n, 6, device=DEV, generator=gen)

    def grouped():
        return ops.lie_backward(3, "act4", g4, X, p, rep=(m, 1))

    def expand_sum():
        dx, dp = ops.lie_backward(3, "act4", g4, X[:, None].expand(-1, m, -1).reshape(-1, 7), p)
        return dx.view(n, m, 7).sum(1), dp

    def composed():
        return torch_act4_backward(g4.view(n, m, 4), X, p.view(n, m, 4))

    a, b, c = grouped(), expand_sum(), composed()
    agree = {"grouped_vs_expand_sum_dx": float((a[0] - b[0]).abs().max()), "grouped_vs_torch_dx": float((a[0] - c[0]).abs().max()),
             "dp_bit_equal": bool(torch.equal(a[1], b[1])), "grouped_vs_torch_dp": float((a[1] - c[1]).abs().max()),
             "dx_scale": float(a[0].abs().max())}
    ways = {"grouped": grouped, "expand_sum": expand_sum, "torch": composed}
    res = {k: [] for k in ways}
    for _ in range(3):                              # alternate the three ways: three rounds each, the median round is kept
        for k, fn in ways.items():
            res[k].append(timed(fn, args.iters, args.batch))
    act4 = {k: sorted(v, key=lambda r: r["median_us"])[1] for k, v in res.items()}
    out = {"shape": {"poses": n, "points": m, "dtype": "float32", "group": "SE3"}, "iters": args.iters, "batch": args.batch,
           "act4_backward": act4, "agreement": agree,
           "bytes_grouped": 4 * (n * m * (4 + 4 + 4) + n * (7 + 7)), "bytes_expand_sum": 4 * (n * m * (4 + 4 + 4 + 7 + 7 + 7) + n * (7 + 7)),
           "mul_backward": timed(lambda: ops.lie_backward(3, "mul", g7, X, Y), args.iters, args.batch),
           "log_backward": timed(lambda: ops.lie_backward(3, "log", g6, X), args.iters, args.batch),
           "device": torch.cuda.get_device_name(0), "library": ops.version()}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
