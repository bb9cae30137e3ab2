"""The checksum definition (tests/csum_model.py) against published vectors and
a second, byte-wise formulation, and the C ABI of the two checksum calls
without a GPU.  tests/golden/csum_kats.json holds the vectors and hand-built
frames; tests/golden/make_csum_kats.py wrote it."""
import ctypes
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
from ingot_amd import _lib, abi
from ingot_amd.abi import CSUM_L3, CSUM_L4, Chain
from tests import csum_frames as cf
from tests import csum_model as model

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "csum_kats.json").read_text())
NONE, OK, BAD, ZERO, SHORT, FRAGMENT = range(6)


# ---------------------------------------------------------------------------
# The second formulation: one byte at a time, big-endian, the carry brought
# round after every add (RFC 1071 section 1, steps 1-2 taken literally).
# ---------------------------------------------------------------------------
def bw_add(acc: int, data: bytes, skip=()) -> int:
    """`data` starts on a word boundary; the bytes at the indices in `skip`
    count as 0."""
    for k, b in enumerate(data):
        if k in skip:
            continue
        acc += b << 8 if k % 2 == 0 else b
        if acc > 0xFFFF:
            acc = (acc & 0xFFFF) + 1
    return acc


def bw_row(f: bytes, rec, what: int):
    """ingot_csum of one frame, verify mode, byte-wise."""
    row = [NONE, NONE, 0, 0, 0]
    L, k3, k4 = len(f), int(rec["l3_kind"]), int(rec["l4_kind"])
    o3, o4, pay = int(rec["l3_off"]), int(rec["l4_off"]), int(rec["payload_off"])
    if int(rec["status"]) or k3 not in (1, 2) or o3 + (20 if k3 == 1 else 40) > L:
        return row
    if k3 == 1 and what & CSUM_L3:
        hl = max(20, (f[o3] & 15) * 4)
        if o3 + hl <= L:
            s0 = bw_add(0, f[o3:o3 + hl], skip=(10, 11))
            row[2] = 0xFFFF - s0
            row[0] = OK if bw_add(s0, f[o3 + 10:o3 + 12]) == 0xFFFF else BAD
    fixed = 20 if k3 == 1 else 40
    if not what & CSUM_L4 or k4 not in (1, 2, 3, 4):
        return row
    if not (o3 + fixed <= o4 and o4 + (20 if k4 == 1 else 8) <= pay <= L):
        return row
    if k3 == 1:
        end = o3 + f[o3 + 2] * 256 + f[o3 + 3]
        frag = bool(f[o3 + 6] & 0x3F) or f[o3 + 7] != 0
    else:
        end = o3 + 40 + f[o3 + 4] * 256 + f[o3 + 5]
        frag, pos, h = False, o3 + 40, f[o3 + 6]
        for _ in range(int(rec["n_v6ext"])):
            if pos + 8 > o4:
                break
            if h == 44:
                frag = frag or f[pos + 2] != 0 or (f[pos + 3] & 0xF9) != 0
            h, pos = f[pos], pos + (8 if h == 44 else 8 + 8 * f[pos + 1])
    if end > L or end < pay:
        row[1] = SHORT
        return row
    if frag:
        row[1] = FRAGMENT
        return row
    n = end - o4
    at = {1: 16, 2: 6, 3: 2, 4: 2}[k4]
    if k4 == 3:
        acc = 0
    elif k3 == 1:
        acc = bw_add(0, f[o3 + 12:o3 + 20] + bytes([0, f[o3 + 9]]) + bytes([n >> 8, n & 255]))
    else:
        acc = bw_add(0, f[o3 + 8:o3 + 40] + n.to_bytes(4, "big") +
                     bytes([0, 0, 0, int(rec["l4_proto"])]))
    s0 = bw_add(acc, f[o4:end], skip=(at, at + 1))
    c = 0xFFFF - s0
    row[3] = 0xFFFF if (k4 == 2 and c == 0) else c
    row[4] = n
    field = f[o4 + at:o4 + at + 2]
    if k4 == 2 and field == b"\0\0":
        row[1] = ZERO
    else:
        row[1] = OK if bw_add(s0, field) == 0xFFFF else BAD
    return row


def kat_frames():
    for k in KATS["frames"]:
        f = bytes.fromhex(k["frame"])
        rec = oracle.parse_batch(*cf.place([f])[:3], Chain[k["chain"]])[0]
        yield k, f, rec


def test_rfc1071_example():
    v = KATS["rfc1071_section3"]
    data = bytes.fromhex(v["bytes"])
    assert data == bytes.fromhex("0001f203f4f5f6f7")
    assert model.ones_sum(data) == int(v["sum"], 16) == 0xDDF2
    assert model.checksum(data) == int(v["checksum"], 16) == 0x220D
    assert bw_add(0, data) == 0xDDF2
    # byte order independence (RFC 1071 section 2 (B)): the swapped words' sum is the swapped sum
    swapped = bytes(data[k ^ 1] for k in range(len(data)))
    assert model.ones_sum(swapped) == 0xF2DD
    # an odd last byte is padded with 0
    assert model.ones_sum(b"\x12\x34\x56") == 0x1234 + 0x5600 == bw_add(0, b"\x12\x34\x56")


def test_ipv4_header_vector():
    v = KATS["ipv4_header"]
    hdr = bytes.fromhex(v["header"])
    assert hdr == bytes.fromhex("450000730000400040110000c0a80001c0a800c7")
    assert model.checksum(hdr) == int(v["checksum"], 16) == 0xB861
    assert 0xFFFF - bw_add(0, hdr) == 0xB861
    f = cf.eth(0x0800) + hdr[:10] + bytes.fromhex("b861") + hdr[12:] + bytes(0x73 - 20)
    rec = oracle.parse_batch(*cf.place([f])[:3], Chain.GenericUlp)[0]
    r = model.one(np.frombuffer(f, dtype=np.uint8), rec, CSUM_L3, False)
    assert r[0] == OK and r[2] == 0xB861


def test_golden_frames_cover_the_cases():
    names = {k["name"] for k in KATS["frames"]}
    assert len(names) == len(KATS["frames"]) >= 12
    states = {(r[0], r[1]) for r in (k["row"] for k in KATS["frames"])}
    assert {s[1] for s in states} == {NONE, OK, BAD, ZERO, SHORT, FRAGMENT}
    assert {s[0] for s in states} == {NONE, OK, BAD}


def test_model_and_bytewise_agree_with_the_golden_rows():
    for k, f, rec in kat_frames():
        a = np.frombuffer(f, dtype=np.uint8)
        for what in (CSUM_L3, CSUM_L4, CSUM_L3 | CSUM_L4):
            want = list(k["row"])
            if not what & CSUM_L3:
                want[0] = want[2] = 0
            if not what & CSUM_L4:
                want[1] = want[3] = want[4] = 0
            assert list(model.one(a, rec, what, False)) == want, (k["name"], what)
            assert bw_row(f, rec, what) == want, (k["name"], what)


def test_model_fill_passes_the_receiver_check():
    """Fill, then the byte-wise receiver: every filled layer sums to 0xffff,
    every byte but the fields is untouched, rows SHORT / FRAGMENT / NONE are
    unwritten."""
    for k, f, rec in kat_frames():
        a = np.frombuffer(f, dtype=np.uint8).copy()
        row = model.one(a, rec, CSUM_L3 | CSUM_L4, True)
        before = k["row"]
        assert a.tobytes().hex() == k["filled"], k["name"]
        diff = {int(x) for x in np.nonzero(a != np.frombuffer(f, dtype=np.uint8))[0]}
        allowed = set()
        o3, o4 = int(rec["l3_off"]), int(rec["l4_off"])
        if before[0] in (OK, BAD):
            assert row[0] == OK and row[2] == before[2]
            allowed |= {o3 + 10, o3 + 11}
            hl = max(20, (a[o3] & 15) * 4)
            assert bw_add(0, a[o3:o3 + hl].tobytes()) == 0xFFFF, k["name"]
        else:
            assert row[0] == NONE
        if before[1] in (OK, BAD, ZERO):
            assert row[1] == OK and row[3:] == tuple(before[3:])
            at = {1: 16, 2: 6, 3: 2, 4: 2}[int(rec["l4_kind"])]
            allowed |= {o4 + at, o4 + at + 1}
            after = bw_row(a.tobytes(), rec, CSUM_L4)
            assert after[1] == OK and after[3] == row[3], k["name"]
            if int(rec["l4_kind"]) == 2:
                assert a[o4 + 6] or a[o4 + 7]  # UDP: never 0 on the wire
        else:
            assert row[1] == before[1]
        assert diff <= allowed, k["name"]
        assert list(model.one(a, rec, CSUM_L3 | CSUM_L4, False))[:2] == list(row[:2])


def test_batch_entry_points_match_one():
    frames = [bytes.fromhex(k["frame"]) for k in KATS["frames"] if k["chain"] == "GenericUlp"]
    arena, off, lens = cf.place(frames, misalign=3, gap=5)
    recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    rows = model.verify(arena, off, lens, recs)
    assert rows.dtype == abi.CSUM_DTYPE and len(rows) == len(frames)
    for i, f in enumerate(frames):
        assert tuple(rows[i]) == model.one(np.frombuffer(f, dtype=np.uint8), recs[i], 3, False)
    with pytest.raises(ValueError):
        model.verify(arena, off, lens, recs, what=4)


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ingot_amd.build import build

    build()
    return _lib.load()


def test_csum_layout_matches_c(tmp_path):
    fields = [f[0] for f in abi.IngotCsum._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ingot_gpu.h"',
             "int main(void){", 'printf("size %zu\\n", sizeof(ingot_csum));']
    lines += [f'printf("{f} %zu\\n", offsetof(ingot_csum, {f}));' for f in fields]
    lines += ['printf("states %d %d %d %d %d %d\\n", INGOT_CSUM_NONE, INGOT_CSUM_OK, '
              'INGOT_CSUM_BAD, INGOT_CSUM_ZERO, INGOT_CSUM_SHORT, INGOT_CSUM_FRAGMENT);',
              'printf("what %u %u\\n", INGOT_CSUM_L3, INGOT_CSUM_L4);',
              'printf("abi %d\\n", INGOT_GPU_ABI_VERSION);', "return 0;}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)],
                   check=True)
    got = {ln.split()[0]: ln.split()[1:] for ln in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert got["size"] == ["8"] and ctypes.sizeof(abi.IngotCsum) == 8
    assert abi.CSUM_DTYPE.itemsize == 8
    for f in fields:
        assert int(got[f][0]) == getattr(abi.IngotCsum, f).offset == abi.CSUM_DTYPE.fields[f][1]
    assert [int(x) for x in got["states"]] == [int(s) for s in abi.CsumState]
    assert [int(x) for x in got["what"]] == [abi.CSUM_L3, abi.CSUM_L4]
    assert int(got["abi"][0]) == abi.ABI_VERSION == 4


def test_checksum_argument_validation_without_gpu(lib):
    null = ctypes.c_void_p(0)
    assert lib.ingot_gpu_abi_version() == 4
    for fn in (lib.ingot_gpu_checksum_verify, lib.ingot_gpu_checksum_fill):
        assert fn(null, None, None, None, 64, 10, None, 3, None, None) == -1  # NULL context
        # a bad `what` is refused before the context is looked at more closely
        fake = ctypes.c_void_p(1)
        for what in (0, 4, 7, 0x80000001):
            assert fn(fake, None, None, None, 64, 10, None, what, None, None) == -1, what
