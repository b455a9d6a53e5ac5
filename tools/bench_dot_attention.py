"""Dot-product graph attention: the fused ops.dot_attention against the composed
form a user had to write before it, and against ops.gatv2_aggregate on the
same graph as a yardstick; one JSON line per measurement.

  python tools/bench_dot_attention.py [--reps 20] [--warmup 3] [--what c3,wide] [--no-composed]
  python tools/bench_dot_attention.py --edge [--reps 20] [--warmup 3] [--what c3,wide]

Shapes (run each under its own time limit):
  c3    R-MAT 1,000,000 nodes / 10,000,000 edges, 8 heads x 16 channels
  wide  R-MAT 250,000 nodes / 2,500,000 edges, 8 heads x 64 channels

Legs, alternating on every repetition (fused, composed, gatv2, fused, ...):
  fused     ops.dot_attention(g, q, k, v, H, C)
  composed  per head ops.edge_dot_graph (the scores), one torch segment
            softmax over the [E, H] scores (scatter_reduce amax, exp,
            index_add, divide), per head a weighted kgx_spmm sum of the value
            rows (its backward: the weighted sum over the transposed graph for
            d v, ops.edge_dot_graph(grad, v) for d alpha)
  gatv2     ops.gatv2_aggregate on the same graph and width: one gathered row
            per edge where the fused dot-product kernel gathers two
Directions: forward (no_grad), and forward + backward (the gradients of a
fixed random cotangent with respect to q, k, v; h_src, h_dst, att for gatv2).
Device-event times around each leg's calls.  The fused and composed outputs
are compared once (largest |difference| / max(1, |value|)) before timing.

--edge measures the attention WITH edge features (ops.dot_attention(edge=...),
a projected edge row per edge added to k_j and v_j) instead; legs, alternating:
  edge-input  fused, the [E, H C] table in input-edge order, gathered by edge id
  edge-csr    fused, the table permuted into CSR slot order, streamed
  no-edge     the fused op without the edge operand: the floor
  composed    k[src] + e and v[src] + e materialised as [E, H C] tensors (timed),
              then the fused op without edge features on the expanded graph (one
              source per edge); its backward is autograd's through the gathers
Forward + backward there takes the gradients with respect to q, k, v and e.
Then the two ways a layer can feed the op, from edge_attr [E, 16] and a
projection W [16, H C] (as layers.Dense computes it), gradients with respect to both included:
  proj-input  e = edge_attr W in input-edge order, gathered by edge id
  proj-csr    e = edge_attr[eid] W, streamed in CSR slot order

KGX_DOT_K / KGX_DOT_U (csrc/dot_attention.hip) select channels per lane and
edges per rescale for A/B runs of the fused leg; they are read once per process.
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

EDGE_DIM = 16  # --edge: width of the unprojected edge_attr of the proj-* legs
SHAPES = {"c3": (1_000_000, 10_000_000, 8, 16), "wide": (250_000, 2_500_000, 8, 64)}


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


class _WeightedSum(torch.autograd.Function):
    """out[i] = sum_e alpha_e v[src_e] over one head, alpha in input-edge order:
    the weighted kgx_spmm and the existing kernels its backward needs."""

    @staticmethod
    def forward(ctx, v, alpha, g):
        ctx.g = g
        ctx.save_for_backward(v, alpha)
        return ops._weighted_sum(g, v, alpha.index_select(0, g.eid.long()))

    @staticmethod
    def backward(ctx, grad):
        v, alpha = ctx.saved_tensors
        g = ctx.g
        t = G.transpose(g)
        grad = grad.contiguous()
        d_v = ops._weighted_sum(t, grad, alpha.index_select(0, t.eid.long()))
        d_alpha = ops.edge_dot_graph(g, grad, v, check=False)
        return d_v, d_alpha, None


def composed(g, dst, q, k, v, H, C):
    scale = C ** -0.5
    s = torch.stack([ops.edge_dot_graph(g, q[:, h * C:(h + 1) * C], k[:, h * C:(h + 1) * C], check=False)
                     for h in range(H)], dim=1) * scale  # [E, H], input-edge order
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((g.n_dst, H), float("-inf"), device=s.device).scatter_reduce(0, idx, s.detach(), "amax")
    ex = torch.exp(s - mx[dst])
    alpha = ex / torch.zeros((g.n_dst, H), device=s.device).index_add(0, dst, ex)[dst]
    return torch.cat([_WeightedSum.apply(v[:, h * C:(h + 1) * C], alpha[:, h].contiguous(), g) for h in range(H)],
                     dim=1)


def run(name, reps, warmup, with_composed):
    N, E, H, C = SHAPES[name]
    dev = torch.device("cuda", 0)
    ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
    g = G.build_csr(ei[0].contiguous(), ei[1].contiguous(), N, N, n_features=H * C)
    G.transpose(g)  # built once, as a training loop's cache keeps it
    dst = ei[1].long()
    gen = torch.Generator(device=dev).manual_seed(0)
    q, k, v, cot = (torch.randn((N, H * C), device=dev, generator=gen) for _ in range(4))
    att = 0.3 * torch.randn((H, C), device=dev, generator=gen)
    what = f"{name}: R-MAT N={N} E={E} H={H} C={C}"
    print(json.dumps({"shape": what, "kept_edges": g.kept, "n_split": g.n_split, "max_degree": g.max_degree,
                      "t_n_split": G.transpose(g).n_split}), flush=True)

    legs = {"fused": lambda a, b, c: ops.dot_attention(g, a, b, c, H, C)}
    if with_composed:
        legs["composed"] = lambda a, b, c: composed(g, dst, a, b, c, H, C)
        with torch.no_grad():
            yf, yc = legs["fused"](q, k, v), legs["composed"](q, k, v)
        print(json.dumps({"shape": what, "what": "fused vs composed, max |diff| / max(1, |value|)",
                          "value": float(((yf - yc).abs() / yc.abs().clamp_min(1.0)).max())}), flush=True)
        del yf, yc
    legs["gatv2"] = lambda a, b, c: ops.gatv2_aggregate(g, a, b, att, H, C, 0.2)

    def forward(leg):
        with torch.no_grad():
            return leg(q, k, v) if leg is not legs["gatv2"] else leg(k, q, None)

    def both(leg):
        a, b, c = (t.detach().requires_grad_(True) for t in (q, k, v))
        if leg is legs["gatv2"]:
            w = att.detach().requires_grad_(True)
            ops.gatv2_aggregate(g, b, a, w, H, C, 0.2).backward(cot)
            return a.grad, b.grad, w.grad
        leg(a, b, c).backward(cot)
        return a.grad, b.grad, c.grad

    for direction, step in (("forward", forward), ("forward+backward", both)):
        ms = {n: [] for n in legs}
        for i in range(reps + warmup):
            for n, leg in legs.items():
                t, out = timed(lambda: step(leg))
                del out
                if i >= warmup:
                    ms[n].append(t)
        for n in ms:
            print(json.dumps({"shape": what, "direction": direction, "leg": n, **summary(ms[n])}), flush=True)
        med = {n: statistics.median(ms[n]) for n in ms}
        ratios = {"fused / gatv2": round(med["fused"] / med["gatv2"], 3)}
        if with_composed:
            ratios["composed / fused"] = round(med["composed"] / med["fused"], 3)
        print(json.dumps({"shape": what, "direction": direction, "ratios of medians": ratios}), flush=True)
    torch.cuda.empty_cache()


def run_edge(name, reps, warmup):
    N, E, H, C = SHAPES[name]
    dev = torch.device("cuda", 0)
    ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
    g = G.build_csr(ei[0].contiguous(), ei[1].contiguous(), N, N, n_features=H * C)
    G.transpose(g)
    if g.kept != E:
        raise SystemExit("bench_dot_attention --edge: the graph dropped edges")
    src = ei[0].long()
    g2 = G.build_csr(torch.arange(E, dtype=torch.int32, device=dev), ei[1].contiguous(), E, N, n_features=H * C)
    G.transpose(g2)
    gen = torch.Generator(device=dev).manual_seed(0)
    q, k, v, cot = (torch.randn((N, H * C), device=dev, generator=gen) for _ in range(4))
    e_in = torch.randn((E, H * C), device=dev, generator=gen)
    e_csr = e_in[g.eid.long()].contiguous()
    what = f"{name}: R-MAT N={N} E={E} H={H} C={C}, edge features"
    print(json.dumps({"shape": what, "kept_edges": g.kept, "n_split": g.n_split, "max_degree": g.max_degree,
                      "t_n_split": G.transpose(g).n_split}), flush=True)

    legs = {
        "edge-input": lambda a, b, c, e: ops.dot_attention(g, a, b, c, H, C, edge=e, edge_order="input"),
        "edge-csr": lambda a, b, c, e: ops.dot_attention(g, a, b, c, H, C, edge=e, edge_order="csr"),
        "no-edge": lambda a, b, c, e: ops.dot_attention(g, a, b, c, H, C),
        "composed": lambda a, b, c, e: ops.dot_attention(g2, a, b[src] + e, c[src] + e, H, C),
    }
    table = {"edge-input": e_in, "edge-csr": e_csr, "no-edge": e_in, "composed": e_in}
    with torch.no_grad():
        ref = legs["composed"](q, k, v, e_in)
        for n in ("edge-input", "edge-csr"):
            y = legs[n](q, k, v, table[n])
            print(json.dumps({"shape": what, "what": f"{n} vs composed, max |diff| / max(1, |value|)",
                              "value": float(((y - ref).abs() / ref.abs().clamp_min(1.0)).max())}), flush=True)
        del ref, y

    def forward(n):
        with torch.no_grad():
            return legs[n](q, k, v, table[n])

    def both(n):
        a, b, c, e = (t.detach().requires_grad_(True) for t in (q, k, v, table[n]))
        legs[n](a, b, c, e).backward(cot)
        return a.grad, b.grad, c.grad, e.grad

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
            "edge-input / no-edge": round(med["edge-input"] / med["no-edge"], 3),
            "edge-csr / no-edge": round(med["edge-csr"] / med["no-edge"], 3),
            "edge-csr / edge-input": round(med["edge-csr"] / med["edge-input"], 3),
            "composed / edge-input": round(med["composed"] / med["edge-input"], 3)}}), flush=True)
    del e_in, e_csr, table
    torch.cuda.empty_cache()

    # what TransformerConv has to choose between: project in input order, or gather edge_attr into CSR order first
    ea = torch.randn((E, EDGE_DIM), device=dev, generator=gen)
    W = torch.randn((EDGE_DIM, H * C), device=dev, generator=gen) / EDGE_DIM ** 0.5
    eid = g.eid.long()

    def project(x, w):  # as layers.Dense: kgx_dense where it takes the shape (N <= 256), else torch's GEMM
        return ops.dense(x, w, None) if ops.dense_supported(x, w) else x @ w

    proj = {
        "proj-input": lambda a, b, c, x, w: ops.dot_attention(g, a, b, c, H, C, edge=project(x, w),
                                                              edge_order="input"),
        "proj-csr": lambda a, b, c, x, w: ops.dot_attention(g, a, b, c, H, C, edge=project(x[eid], w),
                                                            edge_order="csr"),
    }

    def p_forward(n):
        with torch.no_grad():
            return proj[n](q, k, v, ea, W)

    def p_both(n):
        a, b, c, x, w = (t.detach().requires_grad_(True) for t in (q, k, v, ea, W))
        proj[n](a, b, c, x, w).backward(cot)
        return a.grad, b.grad, c.grad, x.grad, w.grad

    for direction, step in (("forward", p_forward), ("forward+backward", p_both)):
        ms = {n: [] for n in proj}
        for i in range(reps + warmup):
            for n in proj:
                t, out = timed(lambda: step(n))
                del out
                if i >= warmup:
                    ms[n].append(t)
        for n in ms:
            print(json.dumps({"shape": what, "direction": direction, "leg": n, **summary(ms[n])}), flush=True)
        print(json.dumps({"shape": what, "direction": direction, "ratios of medians": {
            "proj-csr / proj-input": round(statistics.median(ms["proj-csr"]) / statistics.median(ms["proj-input"]),
                                           3)}}), flush=True)
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--what", default="c3,wide")
    ap.add_argument("--no-composed", action="store_true", help="time the fused and gatv2 legs only (A/B sweeps)")
    ap.add_argument("--edge", action="store_true", help="measure the attention with edge features instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dot_attention: no ROCm device; times are measured on the GPU only")
    for name in args.what.split(","):
        if name not in SHAPES:
            raise SystemExit(f"bench_dot_attention: unknown shape {name!r}")
        if args.edge:
            run_edge(name, args.reps, args.warmup)
        else:
            run(name, args.reps, args.warmup, not args.no_composed)


if __name__ == "__main__":
    main()
