"""Chunked packets for the checksum-over-chunks tests (tests/
test_csum_read_model.py, tests/test_csum_read.py, tools/bigfuzz.py): the
cutter that turns a contiguous frame into the chunk list a receiver would
hold, and a placement helper that puts every chunk at a chosen misalignment
with filler bytes between the chunks (oracle.segments always aligns to 16)."""
from __future__ import annotations

import numpy as np


def cut(frame: bytes, rec, rng) -> list:
    """`frame` -> its chunks.  Header cuts only at a random subset of {14,
    l3_off, l4_off, payload_off} of the frame's contiguous record `rec`
    (ingot parses a header from one slice: a cut inside one is a
    StraddledHeader), 0-3 more cuts anywhere in [payload_off, len], and with
    probability 0.2 an empty chunk after the chunk that holds payload_off (an
    empty chunk before the headers end would make parse_read fail)."""
    n = len(frame)
    ok = int(rec["status"]) == 0
    pay = min(int(rec["payload_off"]), n) if ok else n
    edges = {14}
    if ok:
        edges |= {int(rec["l3_off"]), int(rec["l4_off"]), pay}
    cuts = {e for e in edges if rng.random() < 0.5}
    for _ in range(int(rng.integers(0, 4))):
        cuts.add(int(rng.integers(pay, n + 1)))
    bounds = [0] + sorted(c for c in cuts if 0 < c < n) + [n]
    chunks = [frame[a:b] for a, b in zip(bounds, bounds[1:])]
    if rng.random() < 0.2:
        holds = max(k for k, a in enumerate(bounds[:-1]) if a <= pay)
        chunks.insert(int(rng.integers(holds + 1, len(chunks) + 1)), b"")
    return chunks


def cut_at(frame: bytes, cuts) -> list:
    """`frame` cut at exactly the given offsets (repeats give empty chunks)."""
    bounds = [0] + sorted(cuts) + [len(frame)]
    return [frame[a:b] for a, b in zip(bounds, bounds[1:])]


def place(packets, misalign=0, gap: int = 3, fill: int = 0xA5):
    """[[chunk bytes, ...], ...] -> (arena u8, seg_off u64, seg_len u16,
    pkt_seg u32).  Chunk c (counted over the whole batch) starts at the first
    address >= the previous chunk's end + `gap` whose low four bits are
    `misalign` (an int, or a sequence indexed by c modulo its length); every
    byte that belongs to no chunk is `fill`.  An empty chunk gets the offset
    it would start at, inside the arena.  As in oracle.segments, one
    unreferenced trailing entry keeps the tables non-empty."""
    mis = [misalign] if isinstance(misalign, int) else list(misalign)
    seg_off, seg_len, pkt_seg, o, c = [], [], [0], 16, 0
    for chunks in packets:
        for ch in chunks:
            o += gap
            o += (mis[c % len(mis)] - o) % 16
            seg_off.append(o)
            seg_len.append(len(ch))
            o += len(ch)
            c += 1
        pkt_seg.append(len(seg_off))
    seg_off.append(o)
    seg_len.append(0)
    arena = np.full((o + 64 + 15) // 16 * 16, fill, dtype=np.uint8)
    k = 0
    for chunks in packets:
        for ch in chunks:
            arena[seg_off[k]:seg_off[k] + len(ch)] = np.frombuffer(bytes(ch), dtype=np.uint8)
            k += 1
    return (arena, np.array(seg_off, dtype=np.uint64), np.array(seg_len, dtype=np.uint16),
            np.array(pkt_seg, dtype=np.uint32))


def frames_of(arena, off, lens, stride: int = 0):
    """The frames of a contiguous arena as bytes."""
    n = len(off) if off is not None else len(arena) // stride
    out = []
    for i in range(n):
        o = int(off[i]) if off is not None else i * stride
        ln = int(lens[i]) if lens is not None else stride
        out.append(arena[o:o + ln].tobytes())
    return out
