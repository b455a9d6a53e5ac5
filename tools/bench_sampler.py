"""NeighborSampler.sample against a composed-torch sampler on the same device,
and the sampler's share of a SAGEConv training step; one JSON line per
measurement.

  python tools/bench_sampler.py [--reps 50] [--warmup 5] [--nodes 2449029] [--edges 123718280]
                                [--seeds 1024] [--fanouts 15,10] [--features 100]

Graph: the C5-shaped R-MAT (bench.py --config c5).  Every timed call takes a
different batch of seeds (the same batches for both samplers).  The torch form
gathers the candidate slots of the frontier rows, draws one torch.rand key per
candidate, takes each row's k smallest keys by one sort of (row + key), applies
torch.unique and relabels through a dense map.  It draws different samples, so
only times are compared.  Times are host clocks around work that ends in a
device synchronise (both samplers return host-visible counts).
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "keras-geometric_amd")]

import torch  # noqa: E402

import keras_geometric_amd as kgx  # noqa: E402
from keras_geometric_amd import sampling, synthetic  # noqa: E402


class TorchSampler:
    """The sampler a user would compose from torch ops on the device."""

    def __init__(self, g, fanouts):
        self.rowptr = g.rowptr.long()
        self.col = g.col.long()
        self.deg = g.deg.long()
        self.fanouts = fanouts
        self.map = torch.full((g.n_dst,), -1, dtype=torch.long, device=g.device)

    def sample(self, seeds):
        dev = seeds.device
        nodes = frontier = seeds.long()
        srcs, dsts = [], []
        for k in self.fanouts:
            n_f = frontier.numel()
            if n_f == 0:
                break
            d = self.deg[frontier]
            off = torch.cumsum(d, 0) - d
            total = int(d.sum())
            seg = torch.repeat_interleave(torch.arange(n_f, device=dev), d, output_size=total)
            slots = self.rowptr[frontier][seg] + (torch.arange(total, device=dev) - off[seg])
            # segment top-k: one sort by (row, random key), keep the first k of every row
            order = torch.argsort(seg.double() + torch.rand(total, device=dev, dtype=torch.float64))
            keep = (torch.arange(total, device=dev) - off[seg]) < k  # seg is sorted: rank within the row
            src = self.col[slots[order][keep]]
            row = seg[keep]
            self.map[nodes] = torch.arange(nodes.numel(), device=dev)
            new = torch.unique(src[self.map[src] < 0])
            self.map[new] = nodes.numel() + torch.arange(new.numel(), device=dev)
            srcs.append(self.map[src])
            dsts.append(self.map[frontier][row])
            self.map[nodes] = -1
            self.map[new] = -1
            nodes = torch.cat([nodes, new])
            frontier = new
        ei = torch.stack([torch.cat(srcs), torch.cat(dsts)]).to(torch.int32)
        return nodes.to(torch.int32), ei


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "mean_ms": round(statistics.fmean(ms), 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=2_449_029)
    ap.add_argument("--edges", type=int, default=123_718_280)
    ap.add_argument("--seeds", type=int, default=1024)
    ap.add_argument("--fanouts", default="15,10")
    ap.add_argument("--features", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler: no ROCm device; times are measured on the GPU only")
    dev = torch.device("cuda", 0)
    fanouts = [int(k) for k in args.fanouts.split(",")]
    N, E, F = args.nodes, args.edges, args.features
    shape = f"R-MAT N={N} E={E}, {args.seeds} seeds, fanouts {fanouts}"

    ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
    ms, sampler = clock(lambda: kgx.NeighborSampler(ei, N, fanouts, seed=0))
    print(json.dumps({"shape": shape, "what": "NeighborSampler build (CSR, once)", "ms": round(ms, 2)}), flush=True)
    g = sampler.graph
    tsampler = TorchSampler(g, fanouts)
    gen = torch.Generator(device=dev).manual_seed(0)
    n_batches = args.reps + args.warmup
    perm = torch.randperm(N, device=dev, generator=gen)
    batches = [perm[(i * args.seeds) % max(N - args.seeds, 1):][: args.seeds].to(torch.int32).contiguous()
               for i in range(n_batches)]

    # the two samplers, alternating, on the same batches
    t_kgx, t_torch, sizes = [], [], []
    for i, b in enumerate(batches):
        a_ms, sub = clock(lambda: sampler.sample(b, epoch=i))
        b_ms, (t_nodes, t_ei) = clock(lambda: tsampler.sample(b))
        if i >= args.warmup:
            t_kgx.append(a_ms)
            t_torch.append(b_ms)
            sizes.append((sub.node_ids.numel(), sub.edge_index.shape[1], t_nodes.numel(), t_ei.shape[1]))
    mean = lambda j: round(statistics.fmean(s[j] for s in sizes), 1)  # noqa: E731
    print(json.dumps({"shape": shape, "what": "NeighborSampler.sample (HIP)", **summary(t_kgx),
                      "mean_nodes": mean(0), "mean_edges": mean(1)}), flush=True)
    print(json.dumps({"shape": shape, "what": "composed torch sampler", **summary(t_torch),
                      "mean_nodes": mean(2), "mean_edges": mean(3)}), flush=True)
    print(json.dumps({"shape": shape, "what": "torch / HIP (median)",
                      "ratio": round(statistics.median(t_torch) / statistics.median(t_kgx), 3)}), flush=True)

    # where the HIP sampler's time goes: each entry point per hop (each ends in one synchronise)
    parts = {}
    for i, b in enumerate(batches):
        nodes = frontier = b
        seed64 = sampling.epoch_seed(0, i)
        for hop, k in enumerate(fanouts):
            if frontier.numel() == 0:
                break
            s_ms, (rowptr, src, eid) = clock(lambda: sampling.sample_neighbors(g, frontier, k, seed64, hop))
            r_ms, (new, s_l, d_l) = clock(lambda: sampling.relabel_frontier(nodes, frontier, rowptr, src,
                                                                            sampler._map[:N]))
            if i >= args.warmup:
                parts.setdefault(f"hop{hop} kgx_sample_neighbors", []).append(s_ms)
                parts.setdefault(f"hop{hop} kgx_relabel_frontier", []).append(r_ms)
            nodes = torch.cat([nodes, new])
            frontier = new
    for name, v in parts.items():
        print(json.dumps({"shape": shape, "what": name, **summary(v)}), flush=True)

    # the sampler's share of a training step: sample, then gather + SAGEConv forward + backward
    x = torch.randn((N, F), device=dev, generator=gen)
    gout = torch.randn((args.seeds, F), device=dev, generator=gen)
    torch.manual_seed(0)
    layer = kgx.SAGEConv(F, aggregator="mean")
    t_sample, t_step = [], []
    for i, b in enumerate(batches):
        a_ms, sub = clock(lambda: sampler.sample(b, epoch=i))

        def step():
            for w in layer.weights:
                w.grad = None
            layer([sub.gather(x), sub.edge_index])[: sub.n_seeds].backward(gout)

        s_ms, _ = clock(step)
        if i >= args.warmup:
            t_sample.append(a_ms)
            t_step.append(s_ms)
    share = statistics.median(t_sample) / (statistics.median(t_sample) + statistics.median(t_step))
    print(json.dumps({"shape": shape, "what": "sample (inside the training loop)", **summary(t_sample)}), flush=True)
    print(json.dumps({"shape": shape, "what": f"gather + SAGEConv(mean, F={F}) forward + backward on the subgraph",
                      **summary(t_step)}), flush=True)
    print(json.dumps({"shape": shape, "what": "sampler share of the training step (medians)",
                      "share": round(share, 3)}), flush=True)


if __name__ == "__main__":
    main()
