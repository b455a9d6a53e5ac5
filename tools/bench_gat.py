"""GAT attention aggregation: the fused kernels (kgx_gat / kgx_gat_backward) against the composed torch
form of the same commit (ops.gat_aggregate(fused=False)), with kgx_gatv2 timed beside them at the same
shape; one JSON line per measurement.  One process per shape:

  python tools/bench_gat.py --shape c3   [--reps 10] [--warmup 3] [--edge]
  python tools/bench_gat.py --shape wide

Shapes, as the other attention benches quote them:
  c3    R-MAT 1,000,000 nodes / 10,000,000 edges + self loops, 8 heads x 16 channels
  wide  R-MAT 250,000 nodes / 2,500,000 edges + self loops, 8 heads x 64 channels

Legs, alternating on every repetition (the measuring windows are the repetitions):
  fused     ops.gat_aggregate(g, h, a_src, a_dst, ...)
  composed  ops.gat_aggregate(..., fused=False)
  gatv2     ops.gatv2_aggregate(g, h, h, att, ...)
Directions: forward (no_grad), and forward + backward of a fixed cotangent to every differentiable input.
Device-event times around each leg's calls, allocations included; the spread is min .. max of the
repetitions.  --edge adds the scalar edge table ([E + N, heads], input order) to fused and composed.
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

SHAPES = {"c3": (1_000_000, 10_000_000, 8, 16), "wide": (250_000, 2_500_000, 8, 64)}
SLOPE = 0.2


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


def run(name, reps, warmup, with_edge):
    N, E, H, C = SHAPES[name]
    dev = torch.device("cuda", 0)
    ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
    g = G.build_csr(ei[0].contiguous(), ei[1].contiguous(), N, N, self_loops=True, n_features=H * C)
    t = G.transpose(g)  # built once, as a training loop's cache keeps it
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)  # noqa: E731
    h, a_src, a_dst, bias, cot = rnd(N, H * C), rnd(N, H), rnd(N, H), rnd(H * C), rnd(N, H * C)
    att = 0.3 * rnd(1, H, C)
    edge = 0.5 * rnd(E + N, H) if with_edge else None
    what = (f"rmat+loops {name}: N={N} kept={g.kept} H={H} C={C} edge={with_edge} split_len={g.split_len} "
            f"split_rows={g.n_split} t_split_rows={t.n_split}")

    def gat(fused):
        def call(h, a_src, a_dst, bias, edge=None):
            return ops.gat_aggregate(g, h, a_src, a_dst, H, C, SLOPE, bias=bias, edge=edge, fused=fused)
        return call, [h, a_src, a_dst, bias] + ([edge] if with_edge else [])

    def gatv2(h, att, bias):
        return ops.gatv2_aggregate(g, h, h, att, H, C, SLOPE, bias=bias)

    legs = {"fused": gat(True), "composed": gat(False), "gatv2": (gatv2, [h, att, bias])}
    with torch.no_grad():
        ref, y = legs["composed"][0](*legs["composed"][1]), legs["fused"][0](*legs["fused"][1])
        print(json.dumps({"shape": what, "what": "fused vs composed, max |diff| / max(1, |value|)",
                          "value": float(((y - ref).abs() / ref.abs().clamp_min(1.0)).max())}), flush=True)
        del ref, y

    def forward(n):
        with torch.no_grad():
            return legs[n][0](*legs[n][1])

    def both(n):
        leaves = [v.detach().requires_grad_(True) for v in legs[n][1]]
        legs[n][0](*leaves).backward(cot)
        return [v.grad for v in leaves]

    for direction, step in (("forward", forward), ("forward+backward", both)):
        ms = {n: [] for n in legs}
        for i in range(reps + warmup):
            for n in legs:
                dt, out = timed(lambda: step(n))
                del out
                if i >= warmup:
                    ms[n].append(dt)
        for n in ms:
            print(json.dumps({"shape": what, "direction": direction, "leg": n, **summary(ms[n])}), flush=True)
        print(json.dumps({"shape": what, "direction": direction, "ratio of medians, composed / fused": round(
            statistics.median(ms["composed"]) / statistics.median(ms["fused"]), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=list(SHAPES), required=True)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--edge", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gat: no ROCm device; times are measured on the GPU only")
    run(args.shape, args.reps, args.warmup, args.edge)


if __name__ == "__main__":
    main()
