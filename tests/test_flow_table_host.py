"""The host side of the flow table (ingot_gpu_flow_table_*), through the real
library, which loads without a GPU: sizes and layout, neighbours one bit
apart, duplicates, the load limit, wrapping probe chains, a 2^18-key table and
every EINVAL.  No GPU."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ingot_amd
from ingot_amd import _lib, abi
from ingot_amd.abi import ROW_NONE
from tests import flow_lookup_cases as cases

ROOT = Path(__file__).resolve().parent.parent
EINVAL, ERANGE = -1, -5
V4, V6, TCP, UDP = cases.V4, cases.V6, cases.TCP, cases.UDP


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def count_of(table) -> int:
    """The header's count (dword 2)."""
    return int(table[:64].view("<u4")[2])


def random_keys(n, seed):
    """n distinct valid keys: IPv4 and IPv6, TCP / UDP / ICMP."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 32, (n, 10), dtype=np.uint64).astype(np.uint32)
    v4 = rng.random(n) < 0.5
    k[v4, 3:9] = 0
    proto = rng.choice([1, 6, 17, 58], n).astype(np.uint32)
    k[:, 9] = (np.where(v4, V4, V6).astype(np.uint32) << 8) | proto
    assert len({x.tobytes() for x in k}) == n
    return k


def test_bytes_and_layout(lib, tmp_path):
    assert ingot_amd.flow_table_bytes(16) == 64 * 17
    assert ingot_amd.flow_table_bytes(1 << 26) == 64 * ((1 << 26) + 1)
    for bad in (0, 1, 8, 15, 17, 24, (1 << 26) + 1, 1 << 27, 0xFFFFFFFF):
        assert ingot_amd.flow_table_bytes(bad) == 0, bad
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ingot_gpu.h"\n'
                   'int main(void){printf("%zu %zu %u %u %u\\n", sizeof(ingot_flow_key),'
                   "offsetof(ingot_flow_key, w), INGOT_FLOW_TABLE_MIN_SLOTS,"
                   "INGOT_FLOW_TABLE_MAX_SLOTS, INGOT_FLOW_TABLE_MAX_PROBE);return 0;}")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)],
                   check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in got] == [40, 0, abi.FLOW_TABLE_MIN_SLOTS, abi.FLOW_TABLE_MAX_SLOTS,
                                     abi.FLOW_TABLE_MAX_PROBE]
    assert abi.FLOW_KEY_DTYPE.itemsize == 40 == abi.FLOW_KEY_BYTES


def test_empty_table_finds_nothing(lib):
    t = ingot_amd.flow_table_build(np.zeros((0, 10), np.uint32), [], 16)
    assert t.nbytes == 64 * 17 and t.ctypes.data % 64 == 0
    assert count_of(t) == 0 and not t[64:].any()
    assert ingot_amd.flow_table_find(t, cases.key4(1, 2, 3, 4)) == ROW_NONE
    # build with NULL arrays and no keys
    assert lib.ingot_gpu_flow_table_build(None, None, 0, 16, t.ctypes.data, t.nbytes) == 0


def test_single_bit_neighbours():
    base = np.array([0x20010DB8, 0x00000001, 0x0A0B0C0D, 0x00000002, 0x20010DB8, 0x000000C7,
                     0x01020304, 0x00000009, (40000 << 16) | 53, (V6 << 8) | UDP], np.uint32)
    near = cases.neighbours(base)
    assert len(near) == 1 + 9 * 32 + 8
    # the IPv4 / IPv6 alias: the same nine words, the kind differs
    v4 = cases.key4(0x0A000001, 0x0A000002, 1000, 2000)
    v6_alias = v4.copy()
    v6_alias[9] = (V6 << 8) | UDP
    # TCP versus UDP between the same ports
    tcp = cases.key4(0x0A000001, 0x0A000002, 1000, 2000, proto=TCP)
    k = np.vstack([near, v4[None], v6_alias[None], tcp[None]])
    assert len({x.tobytes() for x in k}) == len(k)
    rows = np.random.default_rng(7).integers(0, 0xFFFFFFFF, len(k),
                                             dtype=np.uint64).astype(np.uint32)
    rows[0], rows[1] = 0, 0xFFFFFFFE  # the smallest and the largest row
    t = ingot_amd.flow_table_build(k, rows, 1024)
    assert count_of(t) == len(k)
    assert (ingot_amd.flow_table_find(t, k) == rows).all()
    # and through the dtype view, one key at a time
    rec = np.ascontiguousarray(k).view(abi.FLOW_KEY_DTYPE).reshape(-1)
    assert ingot_amd.flow_table_find(t, rec[1]) == 0xFFFFFFFE
    assert ingot_amd.flow_table_find(t, rec[0]) == 0


def test_duplicate_key_last_row_wins():
    k = np.array([cases.key4(1, 2, 3, 4), cases.key4(5, 6, 7, 8), cases.key4(1, 2, 3, 4)], np.uint32)
    t = ingot_amd.flow_table_build(k, [10, 20, 30], 16)
    assert count_of(t) == 2
    assert ingot_amd.flow_table_find(t, k).tolist() == [30, 20, 30]
    ingot_amd.flow_table_insert(t, k[1], 21)
    assert count_of(t) == 2 and ingot_amd.flow_table_find(t, k[1]) == 21


def test_half_full_builds_and_one_more_is_erange(lib):
    slots = 64
    k = random_keys(slots // 2 + 1, seed=3)
    rows = np.arange(len(k), dtype=np.uint32)
    t = ingot_amd.flow_table_build(k[:-1], rows[:-1], slots)
    assert count_of(t) == slots // 2
    before = t.copy()
    assert lib.ingot_gpu_flow_table_insert(t.ctypes.data, t.nbytes, k[-1:].ctypes.data,
                                           99) == ERANGE
    assert t.tobytes() == before.tobytes()  # left as it was
    assert (ingot_amd.flow_table_find(t, k[:-1]) == rows[:-1]).all()
    assert ingot_amd.flow_table_find(t, k[-1]) == ROW_NONE
    # replacing a present key's row is no new key: allowed on a half-full table
    ingot_amd.flow_table_insert(t, k[0], 77)
    assert ingot_amd.flow_table_find(t, k[0]) == 77 and count_of(t) == slots // 2
    buf = np.zeros(t.nbytes, np.uint8)
    assert lib.ingot_gpu_flow_table_build(k.ctypes.data, rows.ctypes.data, len(k), slots,
                                          buf.ctypes.data, buf.nbytes) == ERANGE
    with pytest.raises(RuntimeError):
        ingot_amd.flow_table_build(k, rows, slots)


def test_wrapping_probe_chain():
    chain = cases.wrap_chain()
    assert len(chain) == 9
    assert all(ingot_amd.flow_key_hash(k) & 15 == 15 for k in chain)
    assert (ingot_amd.flow_key_hash(chain) & 15 == 15).all()
    rows = np.arange(100, 108, dtype=np.uint32)
    t = ingot_amd.flow_table_build(chain[:8], rows, 16)
    # slot 15, then slots 0..6: the chain wrapped
    slot_kind = t[64:].view("<u4").reshape(16, 16)[:, 9]
    assert (np.nonzero(slot_kind)[0] == [0, 1, 2, 3, 4, 5, 6, 15]).all()
    assert (ingot_amd.flow_table_find(t, chain[:8]) == rows).all()
    assert ingot_amd.flow_table_find(t, chain[8]) == ROW_NONE  # same home, never inserted


def test_probe_limit_is_erange(lib):
    """MAX_PROBE keys with one home fill slots home .. home + 127; one more
    would land 128 slots from home."""
    slots, want = 1024, abi.FLOW_TABLE_MAX_PROBE + 1
    out, dport = [], 0
    k = np.zeros((1, 10), np.uint32)
    k[0, 0], k[0, 1], k[0, 9] = 0x0A000001, 0x0A000002, (V4 << 8) | UDP
    h = lib.ingot_gpu_flow_key_hash
    while len(out) < want:
        k[0, 2] = dport
        if h(k.ctypes.data) & (slots - 1) == 5:
            out.append(k[0].copy())
        dport += 1
    keys = np.array(out, np.uint32)
    rows = np.arange(want, dtype=np.uint32)
    t = ingot_amd.flow_table_build(keys[:-1], rows[:-1], slots)
    before = t.copy()
    assert lib.ingot_gpu_flow_table_insert(t.ctypes.data, t.nbytes, keys[-1:].ctypes.data,
                                           1) == ERANGE
    assert t.tobytes() == before.tobytes()
    assert (ingot_amd.flow_table_find(t, keys[:-1]) == rows[:-1]).all()
    assert ingot_amd.flow_table_find(t, keys[-1]) == ROW_NONE


def test_quarter_million_keys():
    n = 1 << 18
    k = random_keys(2 * n, seed=18)
    rows = np.random.default_rng(1).integers(0, 0xFFFFFFFF, n, dtype=np.uint64).astype(np.uint32)
    t = ingot_amd.flow_table_build(k[:n], rows, 2 * n)  # within MAX_PROBE, or this raises
    assert count_of(t) == n
    assert (ingot_amd.flow_table_find(t, k[:n]) == rows).all()
    assert (ingot_amd.flow_table_find(t, k[n:]) == ROW_NONE).all()


def test_every_einval(lib):
    good = cases.key4(1, 2, 3, 4)[None].copy()
    rows = np.array([5], np.uint32)
    t = ingot_amd.flow_table_build(good, rows, 16)
    tp, tb, kp, rp = t.ctypes.data, t.nbytes, good.ctypes.data, rows.ctypes.data
    build, insert, find = (lib.ingot_gpu_flow_table_build, lib.ingot_gpu_flow_table_insert,
                           lib.ingot_gpu_flow_table_find)
    big = np.zeros(64 * 33, np.uint8)
    # slots not a power of two in [MIN, MAX]
    for slots in (0, 8, 24, 1 << 27):
        assert build(kp, rp, 1, slots, big.ctypes.data, 64 * (slots + 1)) == EINVAL, slots
    # table_bytes != 64 * (slots + 1)
    assert build(kp, rp, 1, 16, big.ctypes.data, 64 * 17 - 1) == EINVAL
    assert build(kp, rp, 1, 16, big.ctypes.data, 64 * 33) == EINVAL
    assert build(kp, rp, 1, 32, big.ctypes.data, 64 * 17) == EINVAL
    # NULL pointers
    assert build(kp, rp, 1, 16, None, tb) == EINVAL
    assert build(None, rp, 1, 16, tp, tb) == EINVAL
    assert build(kp, None, 1, 16, tp, tb) == EINVAL
    assert insert(None, tb, kp, 1) == EINVAL
    assert insert(tp, tb, None, 1) == EINVAL
    assert find(None, tb, kp) == ROW_NONE
    assert find(tp, tb, None) == ROW_NONE
    assert lib.ingot_gpu_flow_key_hash(None) == 0
    # keys no packet can have: kind 0 and 3, reserved upper bits
    for w9 in (UDP, (3 << 8) | UDP, (V4 << 8) | UDP | (1 << 16), (V4 << 8) | UDP | (1 << 31)):
        bad = good.copy()
        bad[0, 9] = w9
        assert build(bad.ctypes.data, rp, 1, 16, big.ctypes.data, tb) == EINVAL, hex(w9)
        assert insert(tp, tb, bad.ctypes.data, 1) == EINVAL, hex(w9)
        assert find(tp, tb, bad.ctypes.data) == ROW_NONE
    # a row equal to INGOT_ROW_NONE
    none = np.array([ROW_NONE], np.uint32)
    assert build(kp, none.ctypes.data, 1, 16, big.ctypes.data, tb) == EINVAL
    assert insert(tp, tb, kp, ROW_NONE) == EINVAL
    # a buffer whose header does not match table_bytes: a 32-slot size over a
    # 16-slot header, and a buffer that was never built
    big[:tb] = t
    assert insert(big.ctypes.data, 64 * 33, kp, 1) == EINVAL
    assert find(big.ctypes.data, 64 * 33, kp) == ROW_NONE
    raw = np.zeros(tb, np.uint8)
    assert insert(raw.ctypes.data, tb, kp, 1) == EINVAL
    assert find(raw.ctypes.data, tb, kp) == ROW_NONE
    # none of the refused calls touched the good table
    assert ingot_amd.flow_table_find(t, good[0]) == 5 and count_of(t) == 1
