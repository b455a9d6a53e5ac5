"""csrc/kgx_attn_layout.h against its Python mirrors (CPU only).

The header is the one statement of the attention kernels' lane-layout rules;
tests/host/attn_layout_main.cpp includes nothing else and prints, for each
(heads, channels, alignment, leading dimension), `K LH G` of the forward rule
(attn_pick_k: kgx_gatv2, kgx_dot_attention and its backward) and of the GATv2
backward's (attn_pick_k_smallest).  Both must equal gatv2_ref.fwd_layout /
bwd_layout (dot_attention_ref.layout is the former), which the GPU modules'
shape lists and gatv2_ref.LAYOUTS / dot_attention_ref.LAYOUTS are written
against, and the forward's partial stride must equal the one ops.py allocates.
"""

from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

import dot_attention_ref as DR
import gatv2_ref as GR

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "keras-geometric_amd" / "csrc"
MAIN = ROOT / "tests" / "host" / "attn_layout_main.cpp"

UNSUPPORTED = (8, 130)  # 130 channels: no float4 piece divides them, and 8 x 65 float2 lanes are more than 64
SHAPES = sorted(set(GR.SHAPES) | set(GR.DEEP_SHAPES) | set(GR.DOMINANT_SHAPES) | set(DR.SHAPES) | set(DR.ODD_SHAPES)
                | set(DR.DEEP_SHAPES) | set(DR.DOMINANT_SHAPES) | {UNSUPPORTED})
ALIGNMENTS = (16, 8, 4)


def _host_compiler():
    """The clang++ that hipcc wraps, or None."""
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    for c in (rocm / "llvm" / "bin" / "clang++", rocm / "lib" / "llvm" / "bin" / "clang++"):
        if c.exists():
            return str(c)
    hipcc = shutil.which("hipcc")
    if hipcc:
        c = Path(hipcc).resolve().parents[1] / "llvm" / "bin" / "clang++"
        if c.exists():
            return str(c)
    return None


def _cases():
    return [(h, c, al, ld) for (h, c) in SHAPES for al in ALIGNMENTS for ld in (h * c, h * c + 1)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("hipcc's host compiler (clang++) not available")
    exe = tmp_path_factory.mktemp("attn_layout") / "attn_layout"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(MAIN), "-o", str(exe)], check=True)
    args = [str(v) for case in _cases() for v in case]
    out = subprocess.run([str(exe), *args], check=True, capture_output=True, text=True).stdout
    rows = [[int(v) for v in line.split()] for line in out.splitlines()]
    assert len(rows) == len(_cases())
    return dict(zip(_cases(), rows))


def _klg(heads, layout):
    return [0, 0, 0] if layout is None else [layout[0], layout[1], GR.group_lanes(heads, layout)]


def test_rules_equal_the_python_mirrors(printed):
    for (h, c, al, ld), row in printed.items():
        assert row[0:3] == _klg(h, DR.layout(h, c, ld=ld, aligned=al)), ("forward", h, c, al, ld, row)
        assert row[3:6] == _klg(h, GR.bwd_layout(h, c, ld=ld, aligned=al)), ("backward", h, c, al, ld, row)


def test_documented_k_columns(printed):
    """gatv2_ref.LAYOUTS (forward K, backward K) and dot_attention_ref.LAYOUTS (K, LH)
    for aligned contiguous inputs, the tables the GPU modules' docstrings point to."""
    for (h, c), (kf, kb) in GR.LAYOUTS.items():
        row = printed[(h, c, 16, h * c)]
        assert (row[0], row[3]) == (kf, kb), (h, c, row)
    for (h, c), (k, lh) in DR.LAYOUTS.items():
        assert printed[(h, c, 16, h * c)][0:2] == [k, lh], (h, c)


def test_shape_past_64_lanes_is_unsupported(printed):
    h, c = UNSUPPORTED
    for al in ALIGNMENTS:
        for ld in (h * c, h * c + 1):
            assert printed[(h, c, al, ld)][0:6] == [0] * 6
            assert DR.layout(h, c, ld=ld, aligned=al) is None and GR.bwd_layout(h, c, ld=ld, aligned=al) is None


def test_partial_stride_equals_the_python_allocation(printed):
    from keras_geometric_amd import ops as kops

    items = torch.zeros((1, 4), dtype=torch.int32)
    for (h, c, al, ld), row in printed.items():
        if al == 16 and ld == h * c:
            assert kops._attn_partials(torch.device("cpu"), items, 1, 1, h, c).shape == (1, row[6]), (h, c)
