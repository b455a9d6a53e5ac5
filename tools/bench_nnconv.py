"""NNConv's layer map: the fused kernel (kgx_nnconv_run) against the composed form (per plane a weighted
kgx_spmm sum into an [N, F_in] scratch and a kgx_dense product); one JSON line per measurement.  One
process per shape:

  python tools/bench_nnconv.py --shape rmat [--reps 10] [--warmup 3]
  python tools/bench_nnconv.py --shape mol

Shapes:
  rmat  R-MAT 1,000,000 nodes / 10,000,000 edges, F 64 -> 64, D = 16
  mol   200,000 chains of 10 nodes (in-degree <= 2, molecule-like), F 128 -> 128, D = 8
Sum aggregation, weight_bias, root weight and bias.  The first line states what the literal form's
[E, F_in * F_out] weight tensor would need.

Legs, alternating on every repetition (the measuring windows are the repetitions):
  fused     ops.nnconv_aggregate(g, x, coef, W, B, root, b, fused=True)
  composed  ops.nnconv_aggregate(g, x, coef, W, B, root, b, fused=False)
Directions: forward (no_grad), and forward + backward of a fixed cotangent to x, coef, W, B, root and b.
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

SHAPES = {"rmat": (1_000_000, 10_000_000, 64, 64, 16), "mol": (2_000_000, 0, 128, 128, 8)}


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
    N, E, F_in, F_out, D = SHAPES[name]
    dev = torch.device("cuda", 0)
    src, dst = edges(name, N, E, dev)
    E = src.numel()
    g = G.build_csr(src, dst, N, N, n_features=F_in)
    t = G.transpose(g)  # built once, as a training loop's cache keeps it
    n_split = G.csr_pieces(g)[1], G.csr_pieces(t)[1]
    gen = torch.Generator(device=dev).manual_seed(0)
    x, cot = torch.randn((N, F_in), device=dev, generator=gen), torch.randn((N, F_out), device=dev, generator=gen)
    coef = torch.randn((E, D), device=dev, generator=gen)
    W = torch.randn((D, F_in, F_out), device=dev, generator=gen) * (D * F_in) ** -0.5
    B, root = (torch.randn((F_in, F_out), device=dev, generator=gen) * F_in ** -0.5 for _ in range(2))
    b = torch.randn(F_out, device=dev, generator=gen)
    what = (f"{name}: N={N} E={E} F={F_in}->{F_out} D={D} max_degree={g.max_degree} split_pieces={n_split[0]} "
            f"(transpose {n_split[1]})")
    print(json.dumps({"shape": what, "what": "bytes of the literal form's [E, F_in * F_out] fp32 weights",
                      "value": 4 * E * F_in * F_out}), flush=True)
    legs = {"fused": True, "composed": False}

    def call(n, *v):
        return ops.nnconv_aggregate(g, *v, fused=legs[n])

    with torch.no_grad():
        ref, y = call("composed", x, coef, W, B, root, b), call("fused", x, coef, W, B, root, b)
        print(json.dumps({"shape": what, "what": "fused vs composed, max |diff| / max(1, |value|)",
                          "value": float(((y - ref).abs() / ref.abs().clamp_min(1.0)).max())}), flush=True)
        del ref, y

    def forward(n):
        with torch.no_grad():
            return call(n, x, coef, W, B, root, b)

    def both(n):
        v = [u.detach().requires_grad_(True) for u in (x, coef, W, B, root, b)]
        call(n, *v).backward(cot)
        return [u.grad for u in v]

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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nnconv: no ROCm device; times are measured on the GPU only")
    run(args.shape, args.reps, args.warmup)


if __name__ == "__main__":
    main()
