"""The definition of the flow key and of the exact-match lookup
(the flow table of include/ingot_gpu.h; the device calls are still to come), written
without the library: keys from the oracle's records plus the frame bytes, the
lookup as a dict.  TEST INFRASTRUCTURE ONLY.

A packet has a key when its record is Ok and names an L3 layer.  Words 0-8 are
the flow hash's input as big-endian words (source address, destination
address, then the L4 header's first word when the L4 layer is TCP or UDP;
IPv4 fills words 0-2, IPv6 words 0-8; zero after); word 9 is
(l3_kind << 8) | l4_proto.  A packet without a key has ten zero words.
"""
from __future__ import annotations

import numpy as np

import oracle
from ingot_amd.abi import ROW_NONE, L3Kind, L4Kind


def be32(arena, at: int) -> int:
    return int.from_bytes(arena[at:at + 4].tobytes(), "big")


def keys(arena, off, lens, chain, stride: int = 0, n: int | None = None):
    """-> (keys (n, 10) uint32, records).  off None: slots of `stride`."""
    recs = oracle.parse_batch(arena, off, lens, chain, stride=stride, n=n)
    out = np.zeros((len(recs), 10), dtype=np.uint32)
    for i, r in enumerate(recs):
        if r["status"] != 0 or r["l3_kind"] == L3Kind.NONE:
            continue
        o = int(off[i]) if off is not None else i * stride
        v6 = r["l3_kind"] == L3Kind.IPV6
        a = o + int(r["l3_off"]) + (8 if v6 else 12)
        na = 8 if v6 else 2
        for k in range(na):
            out[i, k] = be32(arena, a + 4 * k)
        if r["l4_kind"] in (L4Kind.TCP, L4Kind.UDP):
            out[i, na] = be32(arena, o + int(r["l4_off"]))
        out[i, 9] = (int(r["l3_kind"]) << 8) | int(r["l4_proto"])
    return out, recs


def has_key(k) -> np.ndarray:
    return k[:, 9] != 0


def table(k, rows) -> dict:
    """keys[i] -> rows[i], in order: the last one wins."""
    return {bytes(x.tobytes()): int(r) for x, r in zip(k, rows)}


def lookup(k, tab: dict):
    """-> (rows u32[n], the miss indices ascending): ROW_NONE for a packet
    without a key (not a miss) and for a key the table does not hold (a miss)."""
    rows = np.full(len(k), ROW_NONE, dtype=np.uint32)
    miss = []
    for i, x in enumerate(k):
        if x[9] == 0:
            continue
        r = tab.get(x.tobytes())
        if r is None:
            miss.append(i)
        else:
            rows[i] = r
    return rows, np.array(miss, dtype=np.uint32)
