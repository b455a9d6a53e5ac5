"""Four statistics of every neighbourhood (mean, max, min, std: the PNA set):
the fused ops.multi_aggregate against the four separate ops.aggregate calls;
one JSON line per measurement.

  python tools/bench_multi_aggr.py [--reps 50] [--warmup 5] [--shape rmat,c5] [--exact]

Shapes:
  rmat  R-MAT, 1,000,000 nodes / 10,000,000 edges, F 128
  c5    the C5 graph's shape (R-MAT, 2,449,029 nodes / 123,718,280 edges), F 100

Legs, alternating on every repetition (fused, composed, fused, ...):
  fused     one kgx_multi_aggr launch (+ its fix-up): every neighbour row gathered once
  composed  ops.aggregate four times and a concatenation: what a model had to do before
Directions: forward (no_grad), and forward + backward (the gradient with respect
to x of a fixed random cotangent).  Device-event times around each leg's calls.
The graph, its schedule and its transpose are built before the timed region.
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "keras-geometric_amd")]

import torch  # noqa: E402

import keras_geometric_amd as kgx  # noqa: E402
from keras_geometric_amd import graph as G  # noqa: E402
from keras_geometric_amd import ops, synthetic  # noqa: E402

NAMES = ["mean", "max", "min", "std"]
SHAPES = {"rmat": (1_000_000, 10_000_000, 128), "c5": (2_449_029, 123_718_280, 100)}


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


def run(shape, N, E, F, reps, warmup, exact):
    dev = torch.device("cuda", 0)
    ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
    g = kgx.build_csr(ei[0].contiguous(), ei[1].contiguous(), N, N, n_features=F)
    G.transpose(g)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((N, F), device=dev, generator=gen) + 3.0
    cot = torch.randn((N, len(NAMES) * F), device=dev, generator=gen)
    what = f"{shape}: R-MAT N={N} E={E} F={F}, {'+'.join(NAMES)}, {'EXACT' if exact else 'scheduled'}, " \
           f"{g.n_split} split rows"

    def fused(t):
        return ops.multi_aggregate(g, t, NAMES, exact=exact)

    def composed(t):
        return torch.cat([ops.aggregate(g, t, n, exact=exact) for n in NAMES], dim=1)

    def forward(leg):
        with torch.no_grad():
            return leg(x)

    def both(leg):
        t = x.detach().requires_grad_(True)
        leg(t).backward(cot)
        return t.grad

    for direction, step in (("forward", forward), ("forward+backward", both)):
        ms = {"fused": [], "composed": []}
        for i in range(reps + warmup):
            for name, leg in (("fused", fused), ("composed", composed)):
                t, out = timed(lambda: step(leg))
                del out
                if i >= warmup:
                    ms[name].append(t)
        for name in ms:
            print(json.dumps({"shape": what, "direction": direction, "leg": name, **summary(ms[name])}), flush=True)
        print(json.dumps({"shape": what, "direction": direction, "what": "composed / fused (medians)",
                          "ratio": round(statistics.median(ms["composed"]) / statistics.median(ms["fused"]), 3),
                          "ranges_overlap": not max(ms["fused"]) < min(ms["composed"])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="rmat,c5")
    ap.add_argument("--exact", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_aggr: no ROCm device; times are measured on the GPU only")
    for shape in args.shape.split(","):
        N, E, F = SHAPES[shape]
        run(shape, N, E, F, args.reps, args.warmup, args.exact)
        kgx.clear_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
