"""R-GCN layer map: the fused kernel (kgx_rgcn_run) against the composed form (kgx_spmm over the
composite graph into the [N, R * F_in] table, then kgx_dense / the library GEMM); one JSON line per
measurement.  One process per shape:

  python tools/bench_rgcn.py --relations 8 [--reps 10] [--warmup 3]
  python tools/bench_rgcn.py --relations 64

Shape: R-MAT 1,000,000 nodes / 10,000,000 edges, F 128 -> 128, type = a fixed hash of the input edge
id mod R, mean aggregation, root weight and bias.

Legs, alternating on every repetition (the measuring windows are the repetitions):
  fused     ops.rgcn_aggregate(rg, x, W, root, b)
  composed  ops.rgcn_aggregate(rg, x, W, root, b, fused=False)
Directions: forward (no_grad), and forward + backward of a fixed cotangent to x, W, root and b.
Device-event times around each leg's calls, allocations included; outputs compared once first.
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

N, E, F_IN, F_OUT = 1_000_000, 10_000_000, 128, 128


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


def run(R, reps, warmup):
    dev = torch.device("cuda", 0)
    ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
    eid = torch.arange(E, device=dev, dtype=torch.int64)
    etype = (((eid * 2654435761) >> 7) % R).to(torch.int32)  # a fixed multiplicative hash of the edge id
    rg = G.build_relation_csr(ei[0].contiguous(), ei[1].contiguous(), etype, N, N, R)
    G.transpose(rg.graph)  # built once, as a training loop's cache keeps it
    gen = torch.Generator(device=dev).manual_seed(0)
    x, cot = torch.randn((N, F_IN), device=dev, generator=gen), torch.randn((N, F_OUT), device=dev, generator=gen)
    W = torch.randn((R, F_IN, F_OUT), device=dev, generator=gen) * F_IN ** -0.5
    root, b = torch.randn((F_IN, F_OUT), device=dev, generator=gen) * F_IN ** -0.5, torch.randn(F_OUT, device=dev, generator=gen)
    what = (f"rmat: N={N} E={E} F={F_IN}->{F_OUT} R={R} pieces={rg.n_pieces} split_pieces={rg.n_split_pieces} "
            f"piece_len={rg.piece_len}")
    legs = {"fused": None, "composed": False}  # None: the kernel, on this supported shape

    def call(n, *t):
        return ops.rgcn_aggregate(rg, *t, fused=legs[n])

    with torch.no_grad():
        ref, y = call("composed", x, W, root, b), call("fused", x, W, root, b)
        print(json.dumps({"shape": what, "what": "fused vs composed, max |diff| / max(1, |value|)",
                          "value": float(((y - ref).abs() / ref.abs().clamp_min(1.0)).max())}), flush=True)
        del ref, y

    def forward(n):
        with torch.no_grad():
            return call(n, x, W, root, b)

    def both(n):
        t = [v.detach().requires_grad_(True) for v in (x, W, root, b)]
        call(n, *t).backward(cot)
        return [v.grad for v in t]

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
        print(json.dumps({"shape": what, "direction": direction, "ratio of medians, composed / fused": round(
            statistics.median(ms["composed"]) / statistics.median(ms["fused"]), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--relations", type=int, required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rgcn: no ROCm device; times are measured on the GPU only")
    run(args.relations, args.reps, args.warmup)


if __name__ == "__main__":
    main()
