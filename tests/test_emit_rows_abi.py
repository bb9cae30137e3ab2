"""The C-ABI boundary of ingot_gpu_emit_packets_rows, checked without a GPU: a C
probe compiled against include/ingot_gpu.h gives ingot_emit_set_rows' size and
offsets and INGOT_EMIT_BYTES, and the library exports the call."""
import ctypes
import subprocess
from pathlib import Path

import pytest

from ingot_amd import _lib, abi

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("at", "field", "source", "add", "by", "_pad", "pitch", "d_values")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("emit_rows_abi")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ingot_gpu.h"',
             "int main(void){",
             'printf("sizeof %zu\\n", sizeof(ingot_emit_set_rows));',
             'printf("INGOT_EMIT_BYTES %d\\n", (int)INGOT_EMIT_BYTES);',
             'printf("INGOT_MAX_EMIT_SETS %d\\n", (int)INGOT_MAX_EMIT_SETS);']
    lines += [f'printf("{f} %zu\\n", offsetof(ingot_emit_set_rows, {f}));' for f in FIELDS]
    lines.append("return 0;}")
    src = d / "probe.c"
    src.write_text("\n".join(lines))
    exe = d / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_layout_matches_c(probe):
    assert probe["sizeof"] == 24 == abi.EMIT_SET_ROWS_DTYPE.itemsize
    assert ctypes.sizeof(abi.IngotEmitSetRows) == 24
    for f in FIELDS:
        assert probe[f] == abi.EMIT_SET_ROWS_DTYPE.fields[f][1], f
        assert probe[f] == getattr(abi.IngotEmitSetRows, f).offset, f
    assert abi.EMIT_SET_ROWS_DTYPE.fields["add"][0] == "<i4"
    assert abi.EMIT_SET_ROWS_DTYPE.fields["d_values"][0].itemsize == ctypes.sizeof(ctypes.c_void_p)


def test_constants(probe):
    assert probe["INGOT_EMIT_BYTES"] == 4 == int(abi.EmitSource.BYTES)
    assert probe["INGOT_MAX_EMIT_SETS"] == abi.MAX_EMIT_SETS
    assert [int(s) for s in abi.EmitSource] == [0, 1, 2, 3, 4]


def test_array_builder():
    a = abi.emit_set_rows_array([(14, abi.WideField.V6_DESTINATION, abi.EmitSource.BYTES, 0,
                                  abi.EditBy.ROW, 32, 0x1000),
                                 (54, abi.Field.UDP_LENGTH, abi.EmitSource.LENGTH, -8, 0, 0, None)])
    assert a.tobytes() == (bytes([14, 0, 67, 4, 0, 0, 0, 0, 1, 0, 0, 0, 32, 0, 0, 0])
                           + (0x1000).to_bytes(8, "little")
                           + bytes([54, 0, int(abi.Field.UDP_LENGTH), 0, 0xF8, 0xFF, 0xFF, 0xFF])
                           + bytes(16))


def test_symbol_is_exported():
    from ingot_amd.build import build

    build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert any(line.split()[-1] == "ingot_gpu_emit_packets_rows" and " T " in line
               for line in out.splitlines())
    assert "ingot_gpu_emit_packets_rows" in _lib.SIGNATURES
    # NULL context: refused before any device work
    lib = _lib.load()
    assert lib.ingot_gpu_emit_packets_rows(None, None, 0, None, 0, None, 0, None, 0, None, None,
                                           None, 0, None, None, None) == -1
