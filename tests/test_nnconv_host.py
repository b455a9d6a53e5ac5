"""CPU-only checks for NNConv: the fixture's properties under the plain-CSR piece rule, the float64
restatement of tests/nnconv_ref.py on a hand-computed case, and the layer's argument handling."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import nnconv_ref as NR
import rgcn_ref as R


def test_fixture_has_the_properties_for_plain_csr_pieces():
    src, dst, _ = R.make_graph()
    deg = np.bincount(dst, minlength=R.N_DST)
    pieces = np.maximum(1, -(-deg // R.PIECE_LEN))
    assert pieces.sum() > 64 and pieces.sum() % 64 != 0 and pieces.sum() <= 128  # one full tile, one ragged
    assert np.flatnonzero(pieces > 1).tolist() == [R.HUB, R.SECOND] and pieces[R.HUB] > 8 and pieces[R.SECOND] == 2
    assert all(deg[i] == 0 for i in R.EMPTY_NODES) and R.N_SRC > R.N_DST
    pair = np.stack([src, dst], 1)
    assert len(np.unique(pair, axis=0)) < len(pair)  # duplicate edges
    assert not np.array_equal(np.argsort(dst, kind="stable"), np.arange(dst.size))  # eid is not the identity


def test_restatement_on_three_edges():
    # edges 1 -> 0 (c = 2), 2 -> 0 (c = -1), 0 -> 1 (c = 3); F_in = F_out = D = 1, W = 5, B = 1, root = 10, b = 0.5
    x = torch.tensor([[1.0], [2.0], [4.0]])
    coef = torch.tensor([[2.0], [-1.0], [3.0]])
    W, B, root, b = torch.tensor([[[5.0]]]), torch.tensor([[1.0]]), torch.tensor([[10.0]]), torch.tensor([0.5])
    gout = torch.tensor([[1.0], [2.0]])
    src, dst = np.array([1, 2, 0]), np.array([0, 0, 1])
    # Theta = 11, -4, 16; messages 22, -16 into node 0 and 16 into node 1
    r = NR.nnconv64(x, coef, W, B, root, b, src, dst, 2, False, gout)
    assert r["out"].flatten().tolist() == [0.5 + 10 + 6, 0.5 + 20 + 16]
    assert r["A_out"].flatten().tolist() == [0.5 + 10 + 2 * 11 + 4 * 6, 0.5 + 20 + 16]
    assert r["d_x"].flatten().tolist() == [2 * 16 + 10, 11 + 20, -4]
    assert r["d_coef"].flatten().tolist() == [2 * 5 * 1, 4 * 5 * 1, 1 * 5 * 2]
    assert r["d_W"].item() == 2 * 2 - 4 + 3 * 2 and r["d_B"].item() == 2 + 4 + 2
    assert r["d_root"].item() == 1 + 4 and r["d_b"].item() == 3
    m = NR.nnconv64(x, coef, W, B, None, None, src, dst, 2, True, gout)
    assert m["out"].flatten().tolist() == [3.0, 16.0] and m["d_x"].flatten().tolist() == [32.0, 5.5, -2.0]


def test_layer_arguments_and_config():
    import keras_geometric_amd as kgx

    assert kgx.ECConv is kgx.NNConv
    for bad in ({"aggregator": "max"}, {"edge_hidden": 0}, {"edge_hidden": (4, -1)}):
        with pytest.raises(ValueError, match="aggregator|edge_hidden"):
            kgx.NNConv(8, **bad)
    layer = kgx.NNConv(8, edge_hidden=7, aggregator="mean", root_weight=False, name="ec")
    assert layer.edge_hidden == [7] and layer.compute_output_shape([(30, 20), (2, 5), (5, 3)]) == (30, 8)
    clone = kgx.NNConv.from_config(layer.get_config())
    assert clone.get_config() == layer.get_config() and clone.aggregator == "mean" and not clone.root_weight
    assert kgx.NNConv(8).get_config()["edge_hidden"] is None
    x, ei = torch.zeros(3, 4), torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="needs edge_attr"):
        layer.call([x, ei])
    with pytest.raises(ValueError, match="both"):
        layer.call([x, ei, torch.zeros(2, 1)], edge_attr=torch.zeros(2, 1))
    with pytest.raises(ValueError, match="list or tuple"):
        layer.call(x)
