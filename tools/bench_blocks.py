"""A 2-layer SAGEConv training step on a sampled mini-batch, over the merged
subgraph and over layer-wise blocks; one JSON line per measurement.

  python tools/bench_blocks.py [--reps 50] [--warmup 5] [--nodes 2449029] [--edges 123718280]
                               [--seeds 1024] [--fanouts 15,10] [--features 100]

Graph, seeds and fanouts as tools/bench_sampler.py (the C5-shaped R-MAT).
Every timed batch takes different seeds, and both legs run on every batch, one
after the other:

  merged  sub = sampler.sample(b); the CSR of sub.edge_index and its transpose
          through the layers' graph cache (kgx_csr_build2, torch.sort,
          kgx_csr_build2, their schedules); both layers over all of sub's rows
  blocks  the same draw; sample_blocks' kgx_block_csr per layer and the blocks'
          schedules; layer l over blocks[l]

Each leg is timed in three parts (sample, graph / block build, gather + the two
layers forward + backward), host clock around work that ends in a device
synchronise.  Synchronises are counted as calls of the library entry points
that end in one (kgx.h says which); the layers add none in either leg.
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
from keras_geometric_amd import _native as nat  # noqa: E402
from keras_geometric_amd import graph as G  # noqa: E402
from keras_geometric_amd import synthetic  # noqa: E402
from keras_geometric_amd.layers._edges import graph_for  # noqa: E402

SYNCING = ("kgx_csr_build", "kgx_csr_build2", "kgx_schedule_build", "kgx_schedule_suffixes", "kgx_tiny_pack",
           "kgx_sample_neighbors", "kgx_relabel_frontier", "kgx_block_csr")


class SyncCounter:
    """Counts calls of the entry points that synchronise the stream."""

    def __init__(self):
        self.n = 0
        lib = nat.lib()
        for name in SYNCING:
            setattr(lib, name, self._wrap(getattr(lib, name)))

    def _wrap(self, fn):
        def call(*args):
            self.n += 1
            return fn(*args)

        return call

    def take(self) -> int:
        n, self.n = self.n, 0
        return n


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
        raise SystemExit("bench_blocks: no ROCm device; times are measured on the GPU only")
    dev = torch.device("cuda", 0)
    fanouts = [int(k) for k in args.fanouts.split(",")]
    N, E, F = args.nodes, args.edges, args.features
    shape = f"R-MAT N={N} E={E}, {args.seeds} seeds, fanouts {fanouts}, {len(fanouts)}-layer SAGEConv(mean, F={F})"

    ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
    sampler = kgx.NeighborSampler(ei, N, fanouts, seed=0)
    gen = torch.Generator(device=dev).manual_seed(0)
    perm = torch.randperm(N, device=dev, generator=gen)
    batches = [perm[(i * args.seeds) % max(N - args.seeds, 1):][: args.seeds].to(torch.int32).contiguous()
               for i in range(args.reps + args.warmup)]
    x = torch.randn((N, F), device=dev, generator=gen)
    gout = torch.randn((args.seeds, F), device=dev, generator=gen)
    torch.manual_seed(0)
    layers = [kgx.SAGEConv(F, aggregator="mean") for _ in fanouts]
    syncs = SyncCounter()

    def zero_grads():
        for layer in layers:
            for w in layer.weights:
                w.grad = None

    def merged_build(sub):
        n = int(sub.node_ids.numel())
        return G.transpose(graph_for(sub.edge_index, sub.edge_index, n, n, n_features=F))

    def merged_step(sub):
        zero_grads()
        h = sub.gather(x)
        for layer in layers:
            h = layer([h, sub.edge_index])
        h[: sub.n_seeds].backward(gout)

    def blocks_step(blocks):
        zero_grads()
        h = blocks.gather(x)
        for layer, blk in zip(layers, blocks):
            h = layer([h, blk])
        h.backward(gout)

    legs = {"merged": {}, "blocks": {}}
    rows = {"merged": [], "blocks": []}
    for i, b in enumerate(batches):
        rec = {"merged": {}, "blocks": {}}
        # merged subgraph
        rec["merged"]["sample"], sub = clock(lambda: sampler.sample(b, epoch=i))
        rec["merged"]["sample_syncs"] = syncs.take()
        rec["merged"]["build"], _ = clock(lambda: merged_build(sub))
        rec["merged"]["build_syncs"] = syncs.take()
        rec["merged"]["layers"], _ = clock(lambda: merged_step(sub))
        rec["merged"]["layers_syncs"] = syncs.take()
        # blocks
        rec["blocks"]["sample"], hops = clock(lambda: sampler._sample_hops(b, i))
        rec["blocks"]["sample_syncs"] = syncs.take()
        rec["blocks"]["build"], blocks = clock(lambda: sampler._blocks_of(*hops, n_features=F))
        rec["blocks"]["build_syncs"] = syncs.take()
        rec["blocks"]["layers"], _ = clock(lambda: blocks_step(blocks))
        rec["blocks"]["layers_syncs"] = syncs.take()
        if i < args.warmup:
            continue
        for leg in legs:
            rec[leg]["total"] = rec[leg]["sample"] + rec[leg]["build"] + rec[leg]["layers"]
            rec[leg]["total_syncs"] = sum(rec[leg][f"{k}_syncs"] for k in ("sample", "build", "layers"))
            for k, v in rec[leg].items():
                legs[leg].setdefault(k, []).append(v)
        n_sub = int(sub.node_ids.numel())
        rows["merged"].append([n_sub] * len(layers))
        rows["blocks"].append([blk.n_dst for blk in blocks])

    what = {"sample": "sample", "build": "graph / block build (CSR, transpose, schedules)",
            "layers": "gather + layers forward + backward", "total": "sample + build + layers"}
    for leg, parts in legs.items():
        for k, name in what.items():
            line = {"shape": shape, "leg": leg, "what": name, **summary(parts[k])}
            if f"{k}_syncs" in parts:
                line["syncs_per_batch"] = statistics.median(parts[f"{k}_syncs"])
            print(json.dumps(line), flush=True)
        print(json.dumps({"shape": shape, "leg": leg, "what": "rows computed per layer (mean over batches)",
                          "rows": [round(statistics.fmean(r[j] for r in rows[leg]), 1)
                                   for j in range(len(layers))]}), flush=True)
    ratio = lambda k: round(statistics.median(legs["merged"][k]) / statistics.median(legs["blocks"][k]), 3)  # noqa: E731
    print(json.dumps({"shape": shape, "what": "merged / blocks (medians)",
                      **{k: ratio(k) for k in ("build", "layers", "total")}}), flush=True)


if __name__ == "__main__":
    main()
