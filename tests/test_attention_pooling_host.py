"""AttentionPooling / Set2Set: the host-side layer contract (constructor
defaults, the reference's validation messages, output shapes, config round
trip: attention_pooling.py and the reference's tests/test_pooling.py:260-520)
and kgx_softmax_pool's argument validation, which returns before any device
call (CPU)."""

import ctypes

import pytest

from keras_geometric_amd import AttentionPooling, Set2Set
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import layers

P = ctypes.c_void_p(16)  # a non-null, 16-byte aligned pointer that is never dereferenced


def test_exported_from_layers_and_package():
    assert layers.AttentionPooling is AttentionPooling and layers.Set2Set is Set2Set
    assert "AttentionPooling" in layers.__all__ and "Set2Set" in layers.__all__


def test_attention_pooling_defaults_and_validation():
    layer = AttentionPooling()
    assert layer.attention_dim is None and layer.dropout_rate == 0.0
    assert layer.attention_dense is None and layer.attention_score is None and layer.dropout_layer is None
    layer = AttentionPooling(attention_dim=32, dropout=0.1)
    assert layer.attention_dim == 32 and layer.dropout_rate == 0.1
    with pytest.raises(ValueError, match="attention_dim must be positive, got 0"):
        AttentionPooling(attention_dim=0)
    with pytest.raises(ValueError, match="attention_dim must be positive, got -5"):
        AttentionPooling(attention_dim=-5)
    with pytest.raises(ValueError, match=r"dropout must be in \[0, 1\], got 1.5"):
        AttentionPooling(dropout=1.5)
    with pytest.raises(ValueError, match=r"dropout must be in \[0, 1\], got -0.1"):
        AttentionPooling(dropout=-0.1)


def test_attention_pooling_shapes_and_config():
    layer = AttentionPooling(attention_dim=16, dropout=0.25)
    assert layer.compute_output_shape((100, 64)) == (1, 64)
    assert layer.compute_output_shape([(100, 64), (100,)]) == (None, 64)
    with pytest.raises(ValueError, match="Expected input shape to be 2D"):
        layer.compute_output_shape((100, 64, 3))
    with pytest.raises(ValueError, match="Expected input shape to be 2D"):
        layer.build((100,))
    with pytest.raises(ValueError, match="Input feature dimension cannot be None"):
        layer.build((100, None))
    config = layer.get_config()
    assert config["attention_dim"] == 16 and config["dropout"] == 0.25
    new = AttentionPooling.from_config(config)
    assert new.attention_dim == 16 and new.dropout_rate == 0.25 and new.name == layer.name
    assert new.attention_dense is None


def test_set2set_defaults_and_validation():
    layer = Set2Set(output_dim=32)
    assert layer.output_dim == 32 and layer.processing_steps == 3 and layer.lstm_units == 32
    assert layer.dropout_rate == 0.0
    assert layer.lstm_cell is None and layer.attention_dense is None and layer.dropout_layer is None
    assert Set2Set(output_dim=32, lstm_units=16).lstm_units == 16
    with pytest.raises(ValueError, match="output_dim must be positive, got 0"):
        Set2Set(output_dim=0)
    with pytest.raises(ValueError, match="processing_steps must be positive, got 0"):
        Set2Set(output_dim=8, processing_steps=0)
    with pytest.raises(ValueError, match=r"dropout must be in \[0, 1\], got 2"):
        Set2Set(output_dim=8, dropout=2)


def test_set2set_shapes_and_config():
    layer = Set2Set(output_dim=32, processing_steps=4, lstm_units=24, dropout=0.2)
    # concat(h, pooled) = lstm_units + F: what the reference's code returns (:215, :243)
    assert layer.compute_output_shape((100, 32)) == (1, 24 + 32)
    assert layer.compute_output_shape([(100, 32), (100,)]) == (None, 24 + 32)
    with pytest.raises(ValueError, match="Expected input shape to be 2D"):
        layer.compute_output_shape((100, 32, 2))
    with pytest.raises(ValueError, match="Input feature dimension cannot be None"):
        layer.compute_output_shape((100, None))
    config = layer.get_config()
    for key in ("output_dim", "processing_steps", "lstm_units", "dropout"):
        assert key in config
    assert (config["output_dim"], config["processing_steps"], config["lstm_units"], config["dropout"]) == (
        32, 4, 24, 0.2)
    new = Set2Set.from_config(config)
    assert (new.output_dim, new.processing_steps, new.lstm_units, new.dropout_rate) == (32, 4, 24, 0.2)
    assert new.lstm_cell is None


def test_pool_chunk_len():
    assert G.pool_chunk_len(1) == 64 and G.pool_chunk_len(5000) == 64
    assert G.pool_chunk_len(10_000_000) == G.POOL_CHUNK_MAX
    for n in (100, 70_000, 300_000, 10**7):
        c = G.pool_chunk_len(n)
        assert c & (c - 1) == 0 and 64 <= c <= G.POOL_CHUNK_MAX


# -- C-ABI: every rejection below returns before a device call ----------------
def _fwd(lib, *, rowptr=P, rows=P, n_seg=4, items=None, n_items=0, split=None, n_split=0, idx=None, x=P, ld_x=8,
         F=8, s=P, u=None, c=None, flags=0, s_out=None, out=P, ld_out=8, stats=P, partials=None):
    return lib.kgx_softmax_pool(rowptr, rows, n_seg, items, n_items, split, n_split, idx, x, ld_x, F, s, u, c, flags,
                                s_out, out, ld_out, stats, partials, None)


def _bwd(lib, *, N=10, n_seg=4, seg=None, x=P, ld_x=8, F=8, s=P, stats=P, out=P, ld_out=8, grad=P, ld_grad=8,
         grad_x=P, ld_gx=8, grad_s=P):
    return lib.kgx_softmax_pool_backward(N, n_seg, seg, x, ld_x, F, s, stats, out, ld_out, grad, ld_grad, grad_x,
                                         ld_gx, grad_s, None)


@pytest.fixture(scope="module")
def lib():
    return nat.lib()


def test_abi_constants():
    assert nat.POOL_MAX_F >= 256 and nat.POOL_SCORE_TANH == 1
    assert {"kgx_softmax_pool", "kgx_softmax_pool_backward"} <= set(nat.exported_symbols())


def test_softmax_pool_rejects_null_pointers(lib):
    for kw in ({"rowptr": None}, {"x": None}, {"out": None}, {"rows": None}):
        assert _fwd(lib, **kw) == nat.KGX_ERR_ARG, kw
        assert b"null pointer" in lib.kgx_last_error()
    assert _fwd(lib, F=0) == nat.KGX_ERR_ARG
    assert _fwd(lib, n_seg=0) == nat.KGX_OK  # nothing to do is not an error


def test_softmax_pool_wants_exactly_one_score_source(lib):
    assert _fwd(lib, s=P, u=P, c=P, s_out=P) == nat.KGX_ERR_ARG
    assert b"exactly one score source" in lib.kgx_last_error()
    assert _fwd(lib, s=None) == nat.KGX_ERR_ARG
    assert b"exactly one score source" in lib.kgx_last_error()
    # the fused form needs its per-segment constant and somewhere to keep the scores
    assert _fwd(lib, s=None, u=P, c=None, s_out=P) == nat.KGX_ERR_ARG
    assert _fwd(lib, s=None, u=P, c=P, s_out=None) == nat.KGX_ERR_ARG
    assert _fwd(lib, flags=nat.POOL_SCORE_TANH) == nat.KGX_ERR_ARG  # tanh of given scores: not a thing


def test_softmax_pool_rejects_short_leading_dimensions(lib):
    assert _fwd(lib, ld_x=7) == nat.KGX_ERR_ARG
    assert b"leading dimension" in lib.kgx_last_error()
    assert _fwd(lib, ld_out=7) == nat.KGX_ERR_ARG
    assert b"leading dimension" in lib.kgx_last_error()


def test_softmax_pool_split_rows_need_partials(lib):
    assert _fwd(lib, items=P, n_items=5, split=P, n_split=1, partials=None) == nat.KGX_ERR_ARG
    assert b"partials" in lib.kgx_last_error()
    assert _fwd(lib, items=P, n_items=5, split=None, n_split=1, partials=P) == nat.KGX_ERR_ARG


def test_softmax_pool_unsupported_width(lib):
    F = nat.POOL_MAX_F + 1
    assert _fwd(lib, F=F, ld_x=F, ld_out=F) == nat.KGX_ERR_UNSUPPORTED
    assert b"unsupported" in lib.kgx_last_error()
    assert _bwd(lib, F=F, ld_x=F, ld_out=F, ld_grad=F, ld_gx=F) == nat.KGX_ERR_UNSUPPORTED


def test_softmax_pool_backward_validation(lib):
    for kw in ({"x": None}, {"s": None}, {"stats": None}, {"out": None}, {"grad": None}, {"grad_x": None},
               {"grad_s": None}):
        assert _bwd(lib, **kw) == nat.KGX_ERR_ARG, kw
        assert b"null pointer" in lib.kgx_last_error()
    for kw in ({"ld_x": 7}, {"ld_out": 7}, {"ld_grad": 7}, {"ld_gx": 7}):
        assert _bwd(lib, **kw) == nat.KGX_ERR_ARG, kw
        assert b"leading dimension" in lib.kgx_last_error()
    assert _bwd(lib, N=0) == nat.KGX_OK
