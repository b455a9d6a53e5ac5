"""GATv2 attention with edge features: the fused ops.gatv2_aggregate(edge=...)
against the op without an edge table (this build's, and optionally another
build's of the library) and against the composed form a user had to write
before it; one JSON line per measurement.

  python tools/bench_gatv2_edge.py [--reps 20] [--warmup 3] [--what c3,wide] [--no-composed]
                                   [--other-lib PATH]

Shapes (run each under its own time limit):
  c3    R-MAT 1,000,000 nodes / 10,000,000 edges + self loops, 8 heads x 16 channels
  wide  R-MAT 250,000 nodes / 2,500,000 edges + self loops, 8 heads x 64 channels

Legs, alternating on every repetition (measuring windows are the repetitions):
  no-edge     ops.gatv2_aggregate(g, h, h, att, H, C, 0.2): the floor
  edge-input  the same with edge=[E + n, H C] in input-edge order (rows E + i the
              loop of node i), gathered by edge id
  edge-csr    the table permuted into CSR slot order, streamed
  composed    gather h_i and h_j as [E', H, C], add (and add e), leaky ReLU, score,
              a torch segment softmax over the [E', H] scores, then per head a
              weighted kgx_spmm sum of h_j (its backward: the weighted sum over
              the transposed graph and ops.edge_dot_graph, autograd for the rest)
Directions: forward (no_grad), and forward + backward (the gradients of a fixed
random cotangent with respect to h, att and e).  Device-event times around
each leg's calls.  Outputs are compared once before timing.

--other-lib PATH: a second libkgx.so (the parent commit's build).  Two more legs
call kgx_gatv2 (+ kgx_gatv2_backward) straight through ctypes on preallocated
buffers, once on each library, so that the same Python runs around both:
  raw-this    this build's library
  raw-other   the library at PATH
They run before the other legs of a repetition and swap places on every
repetition (what ran just before a leg moves its time by several per cent);
"raw-this / raw-other" is the no-edge product path of this build over the
other's.
"""

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "keras-geometric_amd")]

import torch  # noqa: E402

from keras_geometric_amd import _native as nat  # noqa: E402
from keras_geometric_amd import graph as G  # noqa: E402
from keras_geometric_amd import ops, synthetic  # noqa: E402

SLOPE = 0.2
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
    """out[i] = sum_e alpha_e v[src_e] over one head, alpha in edge-id order:
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


def composed(g, src, dst, h, att, e, H, C):
    """The attention of edge id order [E', ...] with the E' x H x C intermediates materialised."""
    n = g.n_dst
    hh = h.view(n, H, C)
    z = hh[dst] + hh[src]
    if e is not None:
        z = z + e.view(-1, H, C)
    s = (torch.nn.functional.leaky_relu(z, SLOPE) * att.view(1, H, C)).sum(-1)  # [E', H]
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((n, H), float("-inf"), device=s.device).scatter_reduce(0, idx, s.detach(), "amax")
    ex = torch.exp(s - mx[dst])
    alpha = ex / (torch.zeros((n, H), device=s.device).index_add(0, dst, ex)[dst] + 1e-10)
    return torch.cat([_WeightedSum.apply(h[:, k * C:(k + 1) * C], alpha[:, k].contiguous(), g) for k in range(H)],
                     dim=1)


def _other_lib(path):
    handle = ctypes.CDLL(str(path))
    for name in ("kgx_gatv2", "kgx_gatv2_backward"):
        fn = getattr(handle, name)
        fn.argtypes = nat._SIGNATURES[name]
        fn.restype = ctypes.c_int
    return handle


def _raw_leg(lib, g, h, att, cot, H, C):
    """kgx_gatv2 / kgx_gatv2_backward of `lib` on preallocated buffers: (forward, forward + backward)."""
    dev, n, HC = h.device, g.n_dst, H * C
    t = G.transpose(g)
    items, _, split, _, n_slots = g.work(False)
    t_items, _, t_split, _, t_slots = t.work(False)
    n_items, n_split = ops._sched_counts(items, split)
    t_n_items, t_n_split = ops._sched_counts(t_items, t_split)
    f32 = dict(dtype=torch.float32, device=dev)
    out, stats = torch.empty((n, HC), **f32), torch.empty((n, 2 * H), **f32)
    partials = ops._attn_partials(dev, items, n_split, n_slots, H, C)
    g_src, g_dst, g_att = torch.empty((n, HC), **f32), torch.empty((n, HC), **f32), torch.zeros(HC, **f32)
    alpha, ds = torch.empty((g.kept, H), **f32), torch.empty((g.kept, H), **f32)
    bpart = torch.empty((max(n_slots, t_slots, 1), HC), **f32)
    slot = ops._fwd_slot32(t)
    a = att.reshape(-1).contiguous()
    P = nat.ptr

    def forward():
        rc = lib.kgx_gatv2(P(g.rowptr), P(g.rows), n, P(items), n_items, P(split), n_split, P(g.col), P(h), P(h),
                           h.stride(0), P(a), H, C, SLOPE, P(out), out.stride(0), None, P(partials), P(stats), None,
                           0.0, 0, nat.stream(dev))
        assert rc == 0, rc
        return out

    def both():
        forward()
        g_att.zero_()
        rc = lib.kgx_gatv2_backward(
            P(g.rowptr), P(g.rows), n, P(items), n_items, P(split), n_split, P(g.col), P(h), P(h), h.stride(0), P(a),
            H, C, SLOPE, P(out), out.stride(0), None, P(stats), P(cot), cot.stride(0), P(t.rowptr), P(t.rows), n,
            P(t_items), t_n_items, P(t_split), t_n_split, P(t.col), P(slot), P(g_src), P(g_dst), g_src.stride(0),
            P(g_att), P(alpha), P(ds), P(bpart), None, 0.0, 0, nat.stream(dev))
        assert rc == 0, rc
        return g_src

    return forward, both


def run(name, reps, warmup, with_composed, other):
    N, E, H, C = SHAPES[name]
    HC = H * C
    dev = torch.device("cuda", 0)
    ei = synthetic.rmat_edge_index(N, E, seed=0, device=dev)
    g = G.build_csr(ei[0].contiguous(), ei[1].contiguous(), N, N, self_loops=True, n_features=HC)
    G.transpose(g)  # built once, as a training loop's cache keeps it
    if g.kept != E + N:
        raise SystemExit("bench_gatv2_edge: the graph dropped edges")
    loops = torch.arange(N, device=dev)
    src, dst = torch.cat([ei[0].long(), loops]), torch.cat([ei[1].long(), loops])  # edge id order, loops E + i
    # the composed form scores a graph's own input edges (ops.edge_dot_graph takes no added loop slots):
    # the same edges with the loops listed as input edges E + i
    gc = None
    if with_composed:
        gc = G.build_csr(src.to(torch.int32), dst.to(torch.int32), N, N, n_features=HC)
        G.transpose(gc)
        assert torch.equal(gc.eid, g.eid) and torch.equal(gc.col, g.col)
    gen = torch.Generator(device=dev).manual_seed(0)
    h, cot = (torch.randn((N, HC), device=dev, generator=gen) for _ in range(2))
    att = 0.3 * torch.randn((H, C), device=dev, generator=gen)
    e_in = torch.randn((E + N, HC), device=dev, generator=gen)
    e_csr = e_in[g.eid.long()].contiguous()
    what = f"{name}: R-MAT N={N} E={E} + loops, H={H} C={C}"
    print(json.dumps({"shape": what, "kept_edges": g.kept, "n_split": g.n_split, "max_degree": g.max_degree,
                      "t_n_split": G.transpose(g).n_split}), flush=True)

    legs = {
        "no-edge": lambda x, a, e: ops.gatv2_aggregate(g, x, x, a, H, C, SLOPE),
        "edge-input": lambda x, a, e: ops.gatv2_aggregate(g, x, x, a, H, C, SLOPE, edge=e, edge_order="input"),
        "edge-csr": lambda x, a, e: ops.gatv2_aggregate(g, x, x, a, H, C, SLOPE, edge=e, edge_order="csr"),
    }
    table = {"no-edge": None, "edge-input": e_in, "edge-csr": e_csr, "composed": e_in, "composed-no-edge": None}
    if with_composed:
        legs["composed"] = lambda x, a, e: composed(gc, src, dst, x, a, e, H, C)
        legs["composed-no-edge"] = lambda x, a, e: composed(gc, src, dst, x, a, None, H, C)
        with torch.no_grad():
            ref = legs["composed"](h, att, e_in)
            for n in ("edge-input", "edge-csr"):
                y = legs[n](h, att, table[n])
                print(json.dumps({"shape": what, "what": f"{n} vs composed, max |diff| / max(1, |value|)",
                                  "value": float(((y - ref).abs() / ref.abs().clamp_min(1.0)).max())}), flush=True)
            del ref, y
    raw = {}
    if other is not None:
        raw["raw-this"] = _raw_leg(nat.lib(), g, h, att, cot, H, C)
        raw["raw-other"] = _raw_leg(other, g, h, att, cot, H, C)
        with torch.no_grad():
            a, b = raw["raw-this"][0]().clone(), raw["raw-other"][0]().clone()
            print(json.dumps({"shape": what, "what": "raw-this vs raw-other, out bit-identical",
                              "value": bool(torch.equal(a, b))}), flush=True)
            del a, b

    def forward(n):
        if n in raw:
            return raw[n][0]()
        with torch.no_grad():
            return legs[n](h, att, table[n])

    def both(n):
        if n in raw:
            return raw[n][1]()
        x, a = h.detach().requires_grad_(True), att.detach().requires_grad_(True)
        e = None if table[n] is None else table[n].detach().requires_grad_(True)
        legs[n](x, a, e).backward(cot)
        return x.grad, a.grad, None if e is None else e.grad

    # the two raw legs run first and swap places on every repetition: each follows the repetition's
    # last (heaviest) leg half of the time and the other raw leg the other half
    names = list(raw) + list(legs)
    for direction, step in (("forward", forward), ("forward+backward", both)):
        ms = {n: [] for n in names}
        for i in range(reps + warmup):
            order = names[1::-1] + names[2:] if raw and i % 2 else names
            for n in order:
                t, out = timed(lambda: step(n))
                del out
                if i >= warmup:
                    ms[n].append(t)
        for n in ms:
            print(json.dumps({"shape": what, "direction": direction, "leg": n, **summary(ms[n])}), flush=True)
        med = {n: statistics.median(ms[n]) for n in ms}
        ratios = {"edge-input / no-edge": round(med["edge-input"] / med["no-edge"], 3),
                  "edge-csr / no-edge": round(med["edge-csr"] / med["no-edge"], 3)}
        if with_composed:
            ratios["composed / edge-input"] = round(med["composed"] / med["edge-input"], 3)
            ratios["composed-no-edge / no-edge"] = round(med["composed-no-edge"] / med["no-edge"], 3)
        if raw:
            ratios["raw-this / raw-other"] = round(med["raw-this"] / med["raw-other"], 4)
            ratios["raw-other spread (max - min) / median"] = round(
                (max(ms["raw-other"]) - min(ms["raw-other"])) / med["raw-other"], 4)
        print(json.dumps({"shape": what, "direction": direction, "ratios of medians": ratios}), flush=True)
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--what", default="c3,wide")
    ap.add_argument("--no-composed", action="store_true", help="time the fused legs only")
    ap.add_argument("--other-lib", default=None, help="a second libkgx.so whose kgx_gatv2 is timed beside this one's")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gatv2_edge: no ROCm device; times are measured on the GPU only")
    other = _other_lib(args.other_lib) if args.other_lib else None
    for name in args.what.split(","):
        if name not in SHAPES:
            raise SystemExit(f"bench_gatv2_edge: unknown shape {name!r}")
        run(name, args.reps, args.warmup, not args.no_composed, other)


if __name__ == "__main__":
    main()
