"""The argument structs of include/kgx.h against their ctypes mirrors (CPU only).

tests/host/abi_layout_main.c includes the header as C11 and prints sizeof and
every field's offsetof for kgx_work, kgx_slice, kgx_spmm_args and
kgx_fused_args; _native.Work / Slice / SpmmArgs / FusedArgs must have the same
field names in the same order at the same offsets, the same size, and no
implicit padding (the field sizes add up to sizeof, so a field the program or
the binding does not list shows as a gap).
"""

from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import pytest

import test_attn_layout_host as AL

ROOT = Path(__file__).resolve().parents[1]
MAIN = ROOT / "tests" / "host" / "abi_layout_main.c"
MIRRORS = {"kgx_work": "Work", "kgx_slice": "Slice", "kgx_spmm_args": "SpmmArgs", "kgx_fused_args": "FusedArgs"}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{struct: (sizeof, [(field, offset, size), ...])} as the C compiler lays them out."""
    cxx = AL._host_compiler()
    if cxx is None:
        pytest.skip("hipcc's host compiler (clang++) not available")
    exe = tmp_path_factory.mktemp("abi_layout") / "abi_layout"
    subprocess.run([cxx, "-x", "c", "-std=c11", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(MAIN),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    structs: dict = {}
    for line in out.splitlines():
        a, b, c = line.split()
        if a == "struct":
            fields: list = []
            structs[b] = (int(c), fields)
        else:
            fields.append((a, int(b), int(c)))
    return structs


def test_the_program_prints_the_four_structs(printed):
    assert list(printed) == list(MIRRORS)


@pytest.mark.parametrize("c_name", list(MIRRORS))
def test_mirror_equals_the_header(printed, c_name):
    from keras_geometric_amd import _native as nat

    mirror = getattr(nat, MIRRORS[c_name])
    size, fields = printed[c_name]
    assert [f[0] for f in mirror._fields_] == [f[0] for f in fields]
    for name, offset, fsize in fields:
        desc = getattr(mirror, name)
        assert (desc.offset, desc.size) == (offset, fsize), (c_name, name)
    assert ctypes.sizeof(mirror) == size


@pytest.mark.parametrize("c_name", list(MIRRORS))
def test_no_implicit_padding(printed, c_name):
    from keras_geometric_amd import _native as nat

    size, fields = printed[c_name]
    assert sum(f[2] for f in fields) == size, f"{c_name}: padding, or a field the layout program does not print"
    mirror = getattr(nat, MIRRORS[c_name])
    assert sum(getattr(mirror, f[0]).size for f in mirror._fields_) == ctypes.sizeof(mirror)
