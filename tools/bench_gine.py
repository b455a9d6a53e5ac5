"""GINE aggregation: the fused kernel projecting edge attributes itself against the
same kernel fed a kgx_dense projection and against the composed form; one JSON
line per measurement.  One process per shape:

  python tools/bench_gine.py --what rmat [--reps 20] [--warmup 3]
  python tools/bench_gine.py --what mol

Shapes:
  rmat  R-MAT 1,000,000 nodes / 10,000,000 edges, F = 128, D = 16
  mol   200,000 chains of 10 nodes (in-degree <= 2, molecule-like), F = 256, D = 8

Legs, alternating on every repetition (the measuring windows are the repetitions):
  fused-projected  ops.gine_aggregate(g, x, a, weight=W, bias=b)
  fused-plain      ops.gine_aggregate(g, x, ops.dense(a, W, b)): the [E, F] table written and re-read
  composed         relu(x[src] + ops.dense(a, W, b)) in torch, reduced by edge id with ops.aggregate
Directions: forward (no_grad), and forward + backward of a fixed cotangent to x, W
and b.  Device-event times around each leg's calls; outputs compared once first.
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "keras-geometric_amd")]

import torch  # noqa: E402

from keras_geometric_amd import graph as G  # noqa: E402
from keras_geometric_amd import ops, synthetic  # noqa: E402

SHAPES = {"rmat": (1_000_000, 10_000_000, 128, 16), "mol": (2_000_000, 0, 256, 8)}


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "calls": len(ms)}


def edges(name, N, E, dev):
    if name == "rmat":
        ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
        return ei[0].contiguous(), ei[1].contiguous()
    # chains of 10 nodes, both directions: every node has one or two in-edges
    i = torch.arange(N - 1, device=dev, dtype=torch.int32)
    i = i[(i % 10) != 9]
    src, dst = torch.cat([i, i + 1]), torch.cat([i + 1, i])
    perm = torch.randperm(src.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    return src[perm].contiguous(), dst[perm].contiguous()


def run(name, reps, warmup):
    N, E, F, D = SHAPES[name]
    dev = torch.device("cuda", 0)
    src, dst = edges(name, N, E, dev)
    E = src.numel()
    g = G.build_csr(src, dst, N, N, n_features=F)
    G.transpose(g)  # built once, as a training loop's cache keeps it
    gen = torch.Generator(device=dev).manual_seed(0)
    x, cot = (torch.randn((N, F), device=dev, generator=gen) for _ in range(2))
    a = torch.randn((E, D), device=dev, generator=gen)
    W, b = 0.3 * torch.randn((D, F), device=dev, generator=gen), torch.randn(F, device=dev, generator=gen)
    s64, what = src.long(), f"{name}: N={N} E={E} F={F} D={D} max_degree={g.max_degree}"

    def composed(x_, W_, b_):
        msg = torch.relu(x_[s64] + ops.dense(a, W_, b_))
        return ops.aggregate(g, msg, "sum", by_edge=True)

    legs = {
        "fused-projected": lambda x_, W_, b_: ops.gine_aggregate(g, x_, a, weight=W_, bias=b_),
        "fused-plain": lambda x_, W_, b_: ops.gine_aggregate(g, x_, ops.dense(a, W_, b_)),
        "composed": composed,
    }
    with torch.no_grad():
        ref = legs["composed"](x, W, b)
        for n in ("fused-projected", "fused-plain"):
            y = legs[n](x, W, b)
            print(json.dumps({"shape": what, "what": f"{n} vs composed, max |diff| / max(1, |value|)",
                              "value": float(((y - ref).abs() / ref.abs().clamp_min(1.0)).max())}), flush=True)
        del ref, y

    def forward(n):
        with torch.no_grad():
            return legs[n](x, W, b)

    def both(n):
        x_, W_, b_ = (t.detach().requires_grad_(True) for t in (x, W, b))
        legs[n](x_, W_, b_).backward(cot)
        return x_.grad, W_.grad, b_.grad

    for direction, step in (("forward", forward), ("forward+backward", both)):
        ms = {n: [] for n in legs}
        for i in range(reps + warmup):
            for n in legs:
                t, out = timed(lambda: step(n))
                del out
                if i >= warmup:
                    ms[n].append(t)
        for n in ms:
            print(json.dumps({"shape": what, "direction": direction, "leg": n, **summary(ms[n])}), flush=True)
        med = {n: statistics.median(ms[n]) for n in ms}
        print(json.dumps({"shape": what, "direction": direction, "ratios of medians": {
            "fused-plain / fused-projected": round(med["fused-plain"] / med["fused-projected"], 3),
            "composed / fused-projected": round(med["composed"] / med["fused-projected"], 3)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--what", required=True, choices=sorted(SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gine: no ROCm device; times are measured on the GPU only")
    run(args.what, args.reps, args.warmup)


if __name__ == "__main__":
    main()
