"""The k-NN graph build: the fused kernel (kgx_knn) against the composed form (per segment, chunked
torch.cdist + topk) on the same GPU, and the DynamicEdgeConv layer on top of it.

  python tools/bench_knn.py --shape clouds [--reps 10] [--warmup 3]
  python tools/bench_knn.py --shape big

  clouds  32 clouds x 1 024 points, k = 20, at D = 3 (coordinates, the direct path) and D = 64 (the MFMA
          path), then DynamicEdgeConv(64, k = 20) on the D = 64 features, forward and forward + backward
  big     one cloud of 100 000 points, k = 16, at D = 3 and D = 64

Legs, alternating within every repetition (device events, allocations included):
  fused     knn_graph(x, k, batch)                        one kgx_knn launch (plus its preparation for D > 8)
  composed  per segment, query chunks of 4 096: torch.cdist(chunk, cloud) and topk(k + 1, largest=False)
The composed leg writes a [chunk, cloud] distance block per call; the fused one nothing of that size.
One JSON line per result.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "keras-geometric_amd")]

import torch  # noqa: E402

import keras_geometric_amd as kgx  # noqa: E402

SHAPES = {"clouds": (32, 1024, 20), "big": (1, 100_000, 16)}
CHUNK = 4096


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


def composed(x, k, clouds, points):
    """Neighbour table [N, k] without the point itself: cdist + topk per cloud and chunk of queries."""
    out = []
    for c in range(clouds):
        xs = x[c * points:(c + 1) * points]
        for q0 in range(0, points, CHUNK):
            d = torch.cdist(xs[q0:q0 + CHUNK], xs)
            out.append(d.topk(k + 1, dim=1, largest=False).indices[:, 1:] + c * points)
    return torch.cat(out)


def alternate(legs, reps, warmup, what):
    ms = {n: [] for n in legs}
    for i in range(reps + warmup):
        for n, fn in legs.items():
            dt, out = timed(fn)
            del out
            if i >= warmup:
                ms[n].append(dt)
    for n in ms:
        print(json.dumps({**what, "leg": n, **summary(ms[n])}), flush=True)
    if "composed" in ms:
        print(json.dumps({**what, "ratio of medians, composed / fused": round(
            statistics.median(ms["composed"]) / statistics.median(ms["fused"]), 3)}), flush=True)


def run(name, reps, warmup):
    clouds, points, k = SHAPES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    N = clouds * points
    batch = torch.arange(clouds, device=dev).repeat_interleave(points)
    for D in (3, 64):
        x = torch.randn((N, D), device=dev, generator=gen)
        what = {"shape": f"{name}: {clouds} x {points} points, D={D}, k={k}"}
        with torch.no_grad():
            a = kgx.knn(x, x, k + 1, batch, batch)[:, 1:].long()  # with the point itself, as the composed form finds it
            b = composed(x, k, clouds, points)
            same = float((a.sort(1).values == b.sort(1).values).float().mean())
            print(json.dumps({**what, "what": "fraction of neighbour slots equal, fused vs composed", "value": same}),
                  flush=True)
            print(json.dumps({**what, "what": "bytes of a full fp32 distance table per cloud", "value": 4 * points * points}),
                  flush=True)
            alternate({"fused": lambda: kgx.knn_graph(x, k, batch), "composed": lambda: composed(x, k, clouds, points)},
                      reps, warmup, {**what, "direction": "graph build"})
    if name != "clouds":
        return
    layer = kgx.DynamicEdgeConv(64, k)
    cot = torch.randn((N, 64), device=dev, generator=gen)
    what = {"shape": f"{name}: DynamicEdgeConv(64, k={k}) on {clouds} x {points} points, F=64"}

    def forward():
        with torch.no_grad():
            return layer([x, batch])

    def both():
        v = x.detach().requires_grad_(True)
        layer([v, batch]).backward(cot)
        return v.grad

    def graph_only():
        return kgx.knn_csr(x, k, batch, n_features=64)

    alternate({"fused": forward, "graph build alone (knn_csr)": graph_only}, reps, warmup, {**what, "direction": "forward"})
    alternate({"fused": both}, reps, warmup, {**what, "direction": "forward+backward"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn: no ROCm device; times are measured on the GPU only")
    run(args.shape, args.reps, args.warmup)


if __name__ == "__main__":
    main()
