"""The C-ABI boundary of ingot_gpu_parse_read_modify_rows, checked without a
GPU: the call adds no struct or enum (a C probe compiled against
include/ingot_gpu.h takes the prototype's address with the reused
ingot_edit_rows in it), the library exports it, and a NULL context is refused."""
import ctypes
import subprocess
from pathlib import Path

import pytest

from ingot_amd import _lib, abi

ROOT = Path(__file__).resolve().parent.parent
NAME = "ingot_gpu_parse_read_modify_rows"
FIELDS = ("layer", "field", "op", "index", "value", "source", "by", "_pad", "pitch", "d_values")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("modify_read_rows_abi")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ingot_gpu.h"',
             # the prototype, argument for argument
             "typedef int (*fn)(ingot_gpu_ctx*, uint8_t*, const uint64_t*, const uint16_t*,",
             "    const uint32_t*, uint64_t, int, const ingot_edit_rows*, uint32_t, const uint32_t*,",
             "    uint32_t, uint32_t, ingot_rec*, uint16_t*, void*);",
             f'_Static_assert(_Generic(&{NAME}, fn: 1, default: 0), "prototype");',
             "int main(void){",
             'printf("sizeof %zu\\n", sizeof(ingot_edit_rows));',
             'printf("INGOT_EDIT_BYTES %d\\n", (int)INGOT_EDIT_BYTES);',
             'printf("INGOT_BY_ROW %d\\n", (int)INGOT_BY_ROW);',
             'printf("INGOT_FW_V6_DESTINATION %d\\n", (int)INGOT_FW_V6_DESTINATION);',
             'printf("ROW_NONE_IS_MAX %d\\n", (int)(INGOT_ROW_NONE == 0xffffffffu));',
             'printf("declared 1\\n");']
    lines += [f'printf("{f} %zu\\n", offsetof(ingot_edit_rows, {f}));' for f in FIELDS]
    lines.append("return 0;}")
    src = d / "probe.c"
    src.write_text("\n".join(lines))
    exe = d / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_the_reused_struct_and_enums(probe):
    assert probe["declared"] == 1
    assert probe["sizeof"] == 24 == abi.EDIT_ROWS_DTYPE.itemsize
    for f in FIELDS:
        assert probe[f] == abi.EDIT_ROWS_DTYPE.fields[f][1], f
        assert probe[f] == getattr(abi.IngotEditRows, f).offset, f
    assert probe["INGOT_EDIT_BYTES"] == int(abi.EditSource.BYTES)
    assert probe["INGOT_BY_ROW"] == int(abi.EditBy.ROW)
    assert probe["INGOT_FW_V6_DESTINATION"] == int(abi.WideField.V6_DESTINATION)
    assert probe["ROW_NONE_IS_MAX"] == 1 and abi.ROW_NONE == 0xFFFFFFFF


def test_symbol_is_exported():
    from ingot_amd.build import build

    build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert any(line.split()[-1] == NAME and " T " in line for line in out.splitlines())
    assert NAME in _lib.SIGNATURES
    # one argument more than the contiguous call takes in the frames' place
    assert len(_lib.SIGNATURES[NAME][1]) == 15
    # NULL context: refused before any device work
    lib = _lib.load()
    assert getattr(lib, NAME)(None, None, None, None, None, 0, 0, None, 0, None, 0, 0, None, None,
                              None) == -1


def test_the_wrapper_exists():
    import inspect

    import ingot_amd

    sig = inspect.signature(ingot_amd.Context.parse_read_modify_rows)
    assert list(sig.parameters) == ["self", "arena", "seg_off", "seg_len", "pkt_seg", "chain",
                                    "edits", "rows", "n_rows", "csum", "out", "chunk", "stream"]
