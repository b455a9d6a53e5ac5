"""kgx_softmax_pool (the attention readouts' fused softmax pooling) against the
composed torch form on the same device; prints one JSON line per measurement.

  python tools/bench_softmax_pool.py [--reps 20] [--nodes 10000000] [--features 128]

Shapes: one graph of N nodes at chunk lengths 256 / 1024 / 4096 (and the
library's default), and a batch of N / 100 graphs of about 100 nodes each.
Composed forms: torch.softmax, multiply, sum for the single graph; segment ops
(scatter amax, exp, index_add, divide, multiply, index_add) for the batch.
Bandwidth is over the algorithmic bytes N*F*4 + N*4 (x and the scores, read
once); `frac_of_copy` is that bandwidth over the 6.29 TB/s float4-copy ceiling.
"""

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "keras-geometric_amd")]

import torch  # noqa: E402

from keras_geometric_amd import graph as G  # noqa: E402
from keras_geometric_amd import ops as kops  # noqa: E402

COPY_CEILING_TBPS = 6.29


def timeit(fn, reps):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def scaled_diff(a, b):
    return ((a.double() - b.double()).abs() / b.double().abs().clamp_min(1)).max().item()


def report(shape, what, ms, alg_bytes, **extra):
    tbps = alg_bytes / ms / 1e9
    print(json.dumps({"shape": shape, "what": what, "ms": round(ms, 4), "alg_TBps": round(tbps, 3),
                      "frac_of_copy": round(tbps / COPY_CEILING_TBPS, 3), **extra}), flush=True)


def torch_single(x, s):
    return (torch.softmax(s, dim=0).unsqueeze(1) * x).sum(0, keepdim=True)


def torch_batch(x, s, seg, n_seg):
    kw = dict(device=x.device, dtype=x.dtype)
    m = torch.full((n_seg,), float("-inf"), **kw).scatter_reduce(0, seg, s, "amax")
    e = torch.exp(s - m[seg])
    den = torch.zeros(n_seg, **kw).index_add(0, seg, e)
    return torch.zeros((n_seg, x.shape[1]), **kw).index_add(0, seg, (e / den[seg]).unsqueeze(1) * x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--features", type=int, default=128)
    ap.add_argument("--chunks", default="256,1024,4096")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, F = args.nodes, args.features
    alg = N * F * 4 + N * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((N, F), device=dev, generator=gen) + 2.0
    s = 3.0 * torch.randn(N, device=dev, generator=gen)
    u = torch.randn(F, device=dev, generator=gen) / F ** 0.5
    gout = torch.randn((1, F), device=dev, generator=gen)

    with torch.no_grad():
        shape = f"one graph N={N} F={F}"
        ref = torch_single(x.double(), s.double())  # float64: what both fp32 forms are measured against
        report(shape, "torch softmax * x, sum", timeit(lambda: torch_single(x, s), args.reps), alg,
               max_scaled_diff_vs_float64=scaled_diff(torch_single(x, s), ref))
        c1 = torch.full((1,), 0.1, device=dev)
        report(shape, "torch x @ u, tanh, softmax * x, sum",
               timeit(lambda: torch_single(x, torch.tanh(x @ u + c1)), args.reps), alg)
        for chunk in [int(c) for c in args.chunks.split(",") if c] + [G.pool_chunk_len(N)]:
            g = G.single_segment_graph(N, dev, chunk_len=chunk)
            ms = timeit(lambda: kops.softmax_pool(g, x, s), args.reps)
            report(shape, f"kgx_softmax_pool chunk={chunk}", ms, alg, n_items=g.n_items,
                   max_scaled_diff_vs_float64=scaled_diff(kops.softmax_pool(g, x, s), ref))
            ms = timeit(lambda: kops.softmax_pool(g, x, score_u=u, score_c=c1, tanh=True), args.reps)
            report(shape, f"kgx_softmax_pool fused score chunk={chunk}", ms, alg, n_items=g.n_items)

    # backward of the single graph: one pass over x, grad_x written
    g = G.single_segment_graph(N, dev)
    xg, sg = x.clone().requires_grad_(True), s.clone().requires_grad_(True)

    def kgx_step():
        xg.grad = sg.grad = None
        kops.softmax_pool(g, xg, sg).backward(gout)

    def torch_step():
        xg.grad = sg.grad = None
        torch_single(xg, sg).backward(gout)

    report(shape, "kgx forward + backward", timeit(kgx_step, max(args.reps // 4, 3)), alg)
    report(shape, "torch forward + backward", timeit(torch_step, max(args.reps // 4, 3)), alg)
    del xg, sg

    with torch.no_grad():
        n_seg = max(N // 100, 1)
        sizes = torch.randint(50, 151, (n_seg,), device=dev, generator=gen)
        seg = torch.repeat_interleave(torch.arange(n_seg, device=dev), sizes)[:N]
        n = int(seg.numel())
        xb, sb = x[:n], s[:n]
        shape = f"{n_seg} graphs of ~100 nodes N={n} F={F}"
        gb = G.build_csr(torch.arange(n, dtype=torch.int32, device=dev), seg.to(torch.int32), n, n_seg,
                         segment_only=True)
        algb = n * F * 4 + n * 4
        ref = torch_batch(xb.double(), sb.double(), seg, n_seg)
        report(shape, "torch segment ops", timeit(lambda: torch_batch(xb, sb, seg, n_seg), args.reps), algb,
               max_scaled_diff_vs_float64=scaled_diff(torch_batch(xb, sb, seg, n_seg), ref))
        report(shape, "kgx_softmax_pool", timeit(lambda: kops.softmax_pool(gb, xb, sb), args.reps), algb,
               n_items=gb.n_items, n_split=gb.n_split,
               max_scaled_diff_vs_float64=scaled_diff(kops.softmax_pool(gb, xb, sb), ref))
        cb = torch.randn(n_seg, device=dev, generator=gen)
        report(shape, "kgx_softmax_pool fused score",
               timeit(lambda: kops.softmax_pool(gb, xb, score_u=u, score_c=cb, tanh=True), args.reps), algb)


if __name__ == "__main__":
    main()
