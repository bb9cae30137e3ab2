"""The C API's host layer against its recorded behaviour, without a GPU.

tools/api_args_selftest.cpp compiles api.cpp and resolve.cpp into a program
whose launchers are stubs, runs a fixed corpus of calls through every entry
point and prints, per group, a digest over each call's return code, the
launcher it reached and every field of the argument block it built.
tests/golden/api_args.txt is that output from before the host layer was split
into api.cpp and resolve.cpp: a refactor of the host layer keeps it, and a
change of behaviour has to replace it on purpose.
"""
from __future__ import annotations

import subprocess
from pathlib import Path

from ingot_amd.build import ARCH, hipcc

ROOT = Path(__file__).resolve().parent.parent


def test_host_layer_matches_recorded_argument_blocks(tmp_path):
    exe = tmp_path / "api_args_selftest"
    cmd = [hipcc(), "-x", "hip", f"--offload-arch={ARCH}", "-std=c++17", "-O1",
           f"-I{ROOT / 'include'}", str(ROOT / "tools" / "api_args_selftest.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = (ROOT / "tests" / "golden" / "api_args.txt").read_text().splitlines()
    got = r.stdout.splitlines()
    assert [ln.split()[0] for ln in got] == [ln.split()[0] for ln in want]
    differing = [(g, w) for g, w in zip(got, want) if g != w]
    assert not differing, "groups whose cases differ (run the program with --verbose):\n" + \
        "\n".join(f"  got {g}\n want {w}" for g, w in differing)
