"""The definition of ingot_gpu_checksum_verify_read / ingot_gpu_checksum_fill_read
(include/ingot_gpu.h), in numpy / Python.  TEST INFRASTRUCTURE ONLY.

A chunked packet's row is the row tests/csum_model.py gives for its logical
frame (the chunks concatenated, cut at 65,535 bytes) with its record, under
one added rule: a header is read from one chunk.  The span [a, b) lies in one
chunk when some chunk k has start_k <= a and b <= start_k + len_k, start_k
the logical offset of its first byte:

  - [l3_off, l3_off + fixed) (20 B for IPv4, 40 for IPv6) must lie in one
    chunk, else the row is NONE / NONE;
  - L3: [l3_off, l3_off + max(20, ihl * 4)) must lie in one chunk, else L3 is
    NONE;
  - L4: [l3_off, l4_off) and [l4_off, payload_off) must each lie in one chunk,
    else L4 is NONE.

A layer the rule refuses is treated as not selected: NONE and zeros.  `fill`
writes the field bytes back into the chunk that holds them.

Packets are given either as a list of chunk lists ([[chunk, ...], ...], the
chunks bytes-like; for `fill`, writable: bytearray or numpy u8) or as the
chunk tables (arena, seg_off, seg_len, pkt_seg) of ingot_gpu_parse_read, which
`fill` then writes in place.
"""
from __future__ import annotations

import numpy as np

from ingot_amd.abi import CSUM_DTYPE, CSUM_L3, CSUM_L4, L3Kind
from tests import csum_model

MAX_FRAME = 65535  # parse_read: later bytes are not seen


def _as_u8(c):
    return c if isinstance(c, np.ndarray) else np.frombuffer(c, dtype=np.uint8)


def views(src):
    """-> per packet, the list of its chunks as numpy u8 views."""
    if isinstance(src, tuple):
        arena, seg_off, seg_len, pkt_seg = src
        out = []
        for i in range(len(pkt_seg) - 1):
            lo, hi = int(pkt_seg[i]), int(pkt_seg[i + 1])
            out.append([arena[int(seg_off[k]):int(seg_off[k]) + int(seg_len[k])]
                        for k in range(lo, hi)])  # hi < lo: no chunks
        return out
    return [[_as_u8(c) for c in chunks] for chunks in src]


def logical(chunks):
    """-> (the logical frame: a copy, [(start, length)] of every chunk inside it)."""
    spans, start = [], 0
    for c in chunks:
        ln = min(len(c), MAX_FRAME - start)
        spans.append((start, ln))
        start += ln
    parts = [c[:ln] for c, (_, ln) in zip(chunks, spans)]
    f = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return f.astype(np.uint8, copy=True), spans


def in_one(spans, a: int, b: int) -> bool:
    return any(s <= a and b <= s + ln for s, ln in spans)


def one(chunks, rec, what: int, fill: bool):
    """One packet (its chunks as numpy u8 views, writable when `fill`) and its
    record -> (l3_state, l4_state, l3_sum, l4_sum, l4_len)."""
    none = (csum_model.NONE, csum_model.NONE, 0, 0, 0)
    f, spans = logical(chunks)
    l3_kind = int(rec["l3_kind"])
    l3_off, l4_off, pay = int(rec["l3_off"]), int(rec["l4_off"]), int(rec["payload_off"])
    if int(rec["status"]) != 0 or l3_kind not in (int(L3Kind.IPV4), int(L3Kind.IPV6)):
        return none
    v4 = l3_kind == int(L3Kind.IPV4)
    fixed = 20 if v4 else 40
    if not in_one(spans, l3_off, l3_off + fixed):
        return none
    if v4 and not in_one(spans, l3_off, l3_off + max(20, (int(f[l3_off]) & 0xF) * 4)):
        what &= ~CSUM_L3
    if not (in_one(spans, l3_off, l4_off) and in_one(spans, l4_off, pay)):
        what &= ~CSUM_L4
    if what == 0:
        return none
    before = f.copy()
    row = csum_model.one(f, rec, what, fill)
    if fill:
        for at in np.nonzero(f != before)[0]:  # field bytes: back to their chunk
            for c, (s, ln) in zip(chunks, spans):
                if s <= at < s + ln:
                    c[at - s] = f[at]
    return row


def _run(src, recs, what, fill):
    if what == 0 or what & ~(CSUM_L3 | CSUM_L4):
        raise ValueError("what")
    packets = views(src)
    out = np.zeros(len(packets), dtype=CSUM_DTYPE)
    for i, chunks in enumerate(packets):
        out[i] = one(chunks, recs[i], what, fill)
    return out


def verify(src, recs, what: int = CSUM_L3 | CSUM_L4):
    return _run(src, recs, what, False)


def fill(src, recs, what: int = CSUM_L3 | CSUM_L4):
    """In place on the chunks (the tables' arena); returns the rows after writing."""
    return _run(src, recs, what, True)
