"""Chunked batches shared by tests/test_emit_read_rows_model.py,
tests/test_emit_read_rows.py and tools/bigfuzz.py.  TEST INFRASTRUCTURE ONLY.

The header stacks, operand tables and row indices are tests/emit_rows_cases.py's;
this file cuts the payloads into chunks and gives the guarded packets
descriptors that must never be used.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from tests import csum_read_cases as chunks
from tests import emit_csum_cases as cases
from tests import emit_rows_cases as rc

MISALIGN = tuple(range(16)) + (5, 11, 2)
POISON_OFF = 1 << 60   # a guarded packet's chunks: no such address
POISON_DST = 1 << 41   # and its destination: far outside the arena


def cut_random(frame: bytes, pieces: int, rng, edge: bool = False) -> list:
    """`frame` in `pieces` chunks at random offsets (equal offsets give empty
    chunks).  edge (pieces >= 4): the second chunk is empty and the third holds
    one byte."""
    hi = len(frame)
    cuts = sorted(int(c) for c in rng.integers(0, hi + 1, pieces - 1))
    if edge and pieces >= 4:
        cuts[1] = cuts[0]
        cuts[2] = min(cuts[0] + 1, hi)
        cuts = sorted(cuts)
    return chunks.cut_at(frame, cuts)


def two_chunks(src, off, ln, rng):
    """Contiguous payloads -> chunk tables with every payload cut once."""
    frames = chunks.frames_of(src, off, ln)
    return chunks.place([cut_random(f, 2, rng) for f in frames], misalign=MISALIGN, gap=1)


def pack_live(tot, live, rng, first: int = 5):
    """Destination offsets of the emitted packets one after another with 0..3
    byte gaps; a guarded packet owns no bytes and its neighbours are packed
    against each other with no gap -> (dst_off u64, arena size)."""
    n = len(tot)
    tot = np.where(live, np.asarray(tot).astype(np.int64), 0)
    gaps = rng.integers(0, 4, n)
    gaps[~live] = 0
    gaps[np.r_[~live[1:], False]] = 0
    dst_off = (np.cumsum(np.r_[0, (tot + gaps)[:-1]]) + first).astype(np.uint64)
    return dst_off, int(dst_off[-1] + tot[-1] + 64)


def batch(n: int, hdr_len: int, rng, rows=None, n_rows: int = 0, pieces: int = 2,
          lengths=None, window: bool = True, poison: bool = True, edge: bool = False):
    """-> namespace(tables=(arena, seg_off, seg_len, pkt_seg), seg_off, frm,
    take, t, dst_off, size).  Packet i's logical frame is 0..7 junk bytes, its
    payload (`lengths`, default emit_rows_cases.lengths) and 0..5 junk bytes,
    cut into `pieces` chunks (`edge`: as cut_random); frm / take select the
    payload (window False: no junk, frm = take = None).  A guarded packet keeps its (non-empty) chunk
    range, and (poison) every chunk of it has offset 2^60 and length 65,535,
    its destination lies outside the arena and its frm / take are arbitrary."""
    live = np.ones(n, bool) if rows is None else np.asarray(rows).astype(np.uint64) < n_rows
    ln = rc.lengths(n, rng, live) if lengths is None else np.asarray(lengths, np.uint16)
    src, off = cases.random_source(ln, rng)
    pays = chunks.frames_of(src, off, ln)
    frm = np.zeros(n, np.uint16)
    packets = []
    for i, p in enumerate(pays):
        pre = int(rng.integers(0, 8)) if window and len(p) + 7 <= 65535 else 0
        post = int(rng.integers(0, 6)) if window else 0
        frame = bytes(rng.integers(0, 256, pre, dtype=np.uint8)) + p + \
            bytes(rng.integers(0, 256, post, dtype=np.uint8))
        frm[i] = pre
        packets.append(cut_random(frame, pieces, rng, edge))
    arena, seg_off, seg_len, pkt_seg = chunks.place(packets, misalign=MISALIGN, gap=1)
    take = ln.copy()
    dst_off, size = pack_live(hdr_len + ln.astype(np.int64), live, rng)
    seg_off, seg_len = seg_off.copy(), seg_len.copy()
    if poison:
        for i in np.nonzero(~live)[0]:
            seg_off[int(pkt_seg[i]):int(pkt_seg[i + 1])] = POISON_OFF
            seg_len[int(pkt_seg[i]):int(pkt_seg[i + 1])] = 65535
        dst_off[~live] = POISON_DST
        frm[~live] = rng.integers(0, 1 << 16, int((~live).sum()))
        take[~live] = rng.integers(0, 1 << 16, int((~live).sum()))
    t = np.where(live, ln, 0).astype(np.uint16)
    return SimpleNamespace(tables=(arena, seg_off, seg_len, pkt_seg), seg_off=seg_off,
                           frm=frm if window else None, take=take if window else None, t=t,
                           dst_off=dst_off, size=size)
