"""Softmax aggregation (the aggregation of GENConv): the fused kernels (kgx_softmax_aggr /
kgx_softmax_aggr_backward) against the composed torch form of the same commit
(ops.softmax_aggregate(fused=False)); one JSON line per measurement.  One process per shape:

  python tools/bench_softmax_aggr.py --shape f128   [--reps 10] [--warmup 3] [--edge]
  python tools/bench_softmax_aggr.py --shape f256

Shapes:
  f128  R-MAT 1,000,000 nodes / 10,000,000 edges, F = 128
  f256  R-MAT 250,000 nodes / 2,500,000 edges, F = 256

Legs, alternating on every repetition (the measuring windows are the repetitions):
  fused     ops.softmax_aggregate(g, x, temp, message="gen")      temp [F], learnt (its gradient is taken)
  composed  ops.softmax_aggregate(..., fused=False)
Directions: forward (no_grad), and forward + backward of a fixed cotangent to x, temp (and edge).
Device-event times around each leg's calls, allocations included; the spread is min .. max of the
repetitions.  --edge adds an edge table ([E, F], input order).

Every fused line also carries the op's algorithmic bytes, counted from the shapes (every table row and index
the kernels must read or write once, float32 / int32), and that count over the median time as a fraction of
8 TB/s:
  forward   per slot  x (, e) row and col (, eid);  per node  out written (+ stats M | S | Q when training)
  backward  pack:             per node g, out, M, S read, the packed 3F row written
            destination pass: (edge only) per slot x, e rows read, d e written, col, eid; per node g, out, M, S read
            source pass:      per slot the packed 3F row (, e) read and t_col (, t_eid);  per node x read, d x written
            d temp:           per node g, out, Q read
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

SHAPES = {"f128": (1_000_000, 10_000_000, 128), "f256": (250_000, 2_500_000, 256)}
HBM_PEAK = 8e12  # bytes / s


def algorithmic_bytes(N, kept, F, with_edge):
    row, e = 4 * F, 1 if with_edge else 0
    fwd = kept * ((1 + e) * row + 4 + 4 * e) + N * row
    train_fwd = fwd + N * 3 * row
    pack = N * 7 * row
    dst = e * (kept * (3 * row + 8) + N * 4 * row)
    src = kept * ((3 + e) * row + 4 + 4 * e) + N * 2 * row
    return {"forward": fwd, "forward+backward": train_fwd + pack + dst + src + N * 3 * row}


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
    N, E, F = SHAPES[name]
    dev = torch.device("cuda", 0)
    ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
    g = G.build_csr(ei[0].contiguous(), ei[1].contiguous(), N, N, n_features=F)
    t = G.transpose(g)  # built once, as a training loop's cache keeps it
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)  # noqa: E731
    x, cot = rnd(N, F), rnd(N, F)
    temp = 0.25 + 1.75 * torch.rand(F, device=dev, generator=gen)
    edge = rnd(E, F) if with_edge else None
    what = (f"rmat {name}: N={N} kept={g.kept} F={F} edge={with_edge} split_len={g.split_len} "
            f"split_rows={g.n_split} t_split_rows={t.n_split}")
    nbytes = algorithmic_bytes(N, g.kept, F, with_edge)

    def call(fused, x, temp, edge=None):
        return ops.softmax_aggregate(g, x, temp, edge=edge, message="gen", fused=fused)

    inputs = [x, temp] + ([edge] if with_edge else [])
    legs = {"fused": True, "composed": False}
    with torch.no_grad():
        ref, y = call(False, *inputs), call(True, *inputs)
        print(json.dumps({"shape": what, "what": "fused vs composed, max |diff| / max(1, |value|)",
                          "value": float(((y - ref).abs() / ref.abs().clamp_min(1.0)).max())}), flush=True)
        del ref, y

    def forward(n):
        with torch.no_grad():
            return call(legs[n], *inputs)

    def both(n):
        leaves = [v.detach().requires_grad_(True) for v in inputs]
        call(legs[n], *leaves).backward(cot)
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
            line = {"shape": what, "direction": direction, "leg": n, **summary(ms[n])}
            if n == "fused":
                line["algorithmic_bytes"] = nbytes[direction]
                line["fraction_of_8TBps"] = round(nbytes[direction] / (statistics.median(ms[n]) * 1e-3) / HBM_PEAK, 4)
            print(json.dumps(line), flush=True)
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
        raise SystemExit("bench_softmax_aggr: no ROCm device; times are measured on the GPU only")
    run(args.shape, args.reps, args.warmup, args.edge)


if __name__ == "__main__":
    main()
