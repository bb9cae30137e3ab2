"""Inputs shared by tests/test_flow_lookup_model.py, tests/test_flow_table_host.py
(CPU), and by the device tests to come.  TEST INFRASTRUCTURE ONLY.

Everything is computed once (lru_cache) and read-only.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import ingot_amd
from ingot_amd.abi import Chain, GenProfile
from ingot_amd.hostgen import gen_frames_host
from tests import csum_frames as cf
from tests import flow_lookup_model as model

TCP, UDP = 6, 17
V4, V6 = 1, 2


# ---------------------------------------------------------------------------
# Generated frames
# ---------------------------------------------------------------------------
def frames_of(profile, n, seed=91):
    a, o, ln = gen_frames_host(profile, n, seed=seed, slack=64)
    return [a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, ln)]


@lru_cache(maxsize=None)
def placed(profile, n, seed=91, misalign=3):
    """Generated frames packed back to back from a misaligned start; gaps and
    tail 0xA5."""
    arena, off, lens = cf.place(frames_of(profile, n, seed), misalign=misalign)
    arena.setflags(write=False)
    return arena, off, lens


class Case:
    """Frames, the table's keys and rows, and what the model says of them."""

    def __init__(self, arena, off, lens, chain, tab_keys, tab_rows, stride=0, n=None):
        self.arena, self.off, self.lens, self.chain = arena, off, lens, chain
        self.stride = stride
        self.n = len(off) if n is None else n
        self.keys, self.recs = model.keys(arena, off, lens, chain, stride=stride, n=self.n)
        self.tab_keys, self.tab_rows = tab_keys, tab_rows
        self.rows, self.miss = model.lookup(self.keys, model.table(tab_keys, tab_rows))
        for a in (self.keys, self.recs, self.rows, self.miss):
            a.setflags(write=False)

    @property
    def hit(self):
        return self.rows != ingot_amd.ROW_NONE

    @property
    def no_key(self):
        return ~model.has_key(self.keys)


def unique_keys(k):
    """The distinct keys of `k` (rows with a key), in order of first sight."""
    seen, out = set(), []
    for x in k[model.has_key(k)]:
        b = x.tobytes()
        if b not in seen:
            seen.add(b)
            out.append(x)
    return np.array(out, dtype=np.uint32).reshape(-1, 10)


MAIN_N = 20000
MAIN_ROWS = 1 << 14  # the action table of the main case


@lru_cache(maxsize=None)
def main_case() -> Case:
    """20,000 frames, FLOWS interleaved with ADVERSARIAL; the table holds the
    keys of the first half, key j -> row (7 j + 3) mod MAIN_ROWS (distinct: the
    first half has fewer than MAIN_ROWS keys).  So the first half hits, the
    second half's FLOWS frames mostly miss, and most ADVERSARIAL frames have no
    key."""
    fl, ad = frames_of(GenProfile.FLOWS, MAIN_N // 2), frames_of(GenProfile.ADVERSARIAL, MAIN_N // 2)
    frames = [f for pair in zip(fl, ad) for f in pair]
    arena, off, lens = cf.place(frames, misalign=3)
    arena.setflags(write=False)
    k, _ = model.keys(arena, off[:MAIN_N // 2], lens[:MAIN_N // 2], Chain.GenericUlp)
    tab_keys = unique_keys(k)
    assert len(tab_keys) < MAIN_ROWS
    tab_rows = ((7 * np.arange(len(tab_keys)) + 3) % MAIN_ROWS).astype(np.uint32)
    return Case(arena, off, lens, Chain.GenericUlp, tab_keys, tab_rows)


def slots_for(n_keys: int) -> int:
    """The smallest table `n_keys` fit: a power of two >= max(16, 2 n_keys)."""
    s = 16
    while s < 2 * n_keys:
        s *= 2
    return s


# ---------------------------------------------------------------------------
# Hand-built keys and their frames
# ---------------------------------------------------------------------------
def key4(src: int, dst: int, sport: int, dport: int, proto: int = UDP) -> np.ndarray:
    k = np.zeros(10, dtype=np.uint32)
    k[0], k[1], k[2], k[9] = src, dst, (sport << 16) | dport, (V4 << 8) | proto
    return k


def frame_of(key) -> bytes:
    """An Ethernet / IPv4 or IPv6 / TCP or UDP frame whose key is `key`."""
    kind, proto = int(key[9]) >> 8, int(key[9]) & 0xFF
    na = 2 if kind == V4 else 8
    addrs = b"".join(int(w).to_bytes(4, "big") for w in key[:na])
    ports = int(key[na]).to_bytes(4, "big")
    l4 = ports + (bytes(8) + bytes([0x50, 0x10]) + bytes(6) if proto == TCP
                  else cf.u16(8 + 6) + cf.u16(0)) + b"flows!"
    if kind == V4:
        l3 = bytes([0x45, 0]) + cf.u16(20 + len(l4)) + bytes(4) + bytes([64, proto, 0, 0]) + addrs
        return cf.eth(0x0800) + l3 + l4
    l3 = bytes([0x60, 0, 0, 0]) + cf.u16(len(l4)) + bytes([proto, 64]) + addrs
    return cf.eth(0x86DD) + l3 + l4


@lru_cache(maxsize=None)
def wrap_chain(slots: int = 16, count: int = 9):
    """`count` IPv4/UDP keys (one flow's addresses, the destination port
    varied) whose home is the last slot of a `slots`-slot table, so their probe
    chain wraps to slot 0."""
    out, dport = [], 1
    while len(out) < count:
        k = key4(0x0A000001, 0x0A000002, 40000, dport)
        if ingot_amd.flow_key_hash(k) & (slots - 1) == slots - 1:
            out.append(k)
        dport += 1
    out = np.array(out, dtype=np.uint32)
    out.setflags(write=False)
    return out


def neighbours(k):
    """`k` and every key one bit away from it that is still a valid key: all
    bits of words 0-8; of word 9 the protocol bits and the two kind bits (each
    flip of those turns kind 1 into 3 or 0, neither valid, so they are left
    out, as are the reserved bits)."""
    out = [k.copy()]
    for w in range(9):
        for b in range(32):
            x = k.copy()
            x[w] ^= np.uint32(1 << b)
            out.append(x)
    for b in range(8):
        x = k.copy()
        x[9] ^= np.uint32(1 << b)
        out.append(x)
    return np.array(out, dtype=np.uint32)
