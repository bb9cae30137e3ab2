"""The C-ABI boundary of ingot_gpu_emit_packets_read_rows, checked without a
GPU: the library exports the call, the Python binding knows its signature, a
NULL context is refused, and tools/emit_read_rows_selftest.cpp (every EINVAL of
the header's list in its order, as a stand-alone program) prints its OK line."""
import subprocess
from pathlib import Path

from ingot_amd import _lib
from ingot_amd.build import ARCH, build, hipcc

ROOT = Path(__file__).resolve().parent.parent
NAME = "ingot_gpu_emit_packets_read_rows"


def test_symbol_is_exported():
    build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert any(line.split()[-1] == NAME and " T " in line for line in out.splitlines())
    assert NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME][1]) == 20
    # NULL context: refused before any device work
    lib = _lib.load()
    assert getattr(lib, NAME)(None, None, 0, None, 0, None, 0, None, 0, None, None, None, None,
                              None, None, 4, None, None, None, None) == -1


def test_selftest_program(tmp_path):
    """The argument checks as a program of their own (no sanitizer here)."""
    build()
    exe = tmp_path / "emit_read_rows_selftest"
    cmd = [hipcc(), "-x", "hip", f"--offload-arch={ARCH}", "-std=c++17", "-O1",
           f"-I{ROOT / 'include'}", str(ROOT / "tools" / "emit_read_rows_selftest.cpp"),
           f"-L{_lib.LIB_PATH.parent}", "-lingot_gpu", f"-Wl,-rpath,{_lib.LIB_PATH.parent}",
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "emit_read_rows selftest: OK" in r.stdout
