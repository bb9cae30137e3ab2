"""The definition of ingot_gpu_emit_packets_read (include/ingot_gpu.h), in
numpy / Python.  TEST INFRASTRUCTURE ONLY.

Written from the header comment, not from the kernel.  The call is
ingot_gpu_emit_packets_csum over a linear copy of each packet's payload, so
the model is exactly that: `linearise` applies the payload rule to the chunk
tables, `apply` runs the oracle's plain emit over the result and then
tests/emit_csum_model.py's sums.

Payload rule.  Packet i is the chunks pkt_seg[i] .. pkt_seg[i+1] of (seg_off,
seg_len), in order; pkt_seg[i+1] < pkt_seg[i] counts as no chunks.  The
logical frame is the chunks concatenated and cut at 65,535 bytes; L is its
length.  f = min(frm[i], L) (frm None: 0), t = min(take[i], L - f) (take None:
L - f); the payload is the logical bytes [f, f + t).
"""
from __future__ import annotations

import numpy as np

import oracle
from tests import emit_csum_model

CUT = 65535


def linearise(arena, seg_off, seg_len, pkt_seg, frm=None, take=None):
    """-> (src u8, off u64, lens u16): the payloads back to back (64 spare
    bytes after the last, so the contiguous calls may read their 16-B blocks)."""
    arena = np.asarray(arena, dtype=np.uint8)
    n = len(pkt_seg) - 1
    parts, off, lens, o = [], [], [], 0
    for i in range(n):
        s0, s1 = int(pkt_seg[i]), int(pkt_seg[i + 1])
        frame = b""
        for k in range(s0, s1):  # empty when the bounds are reversed
            if len(frame) >= CUT:
                break
            if int(seg_len[k]):  # an empty chunk's offset is never used
                frame += arena[int(seg_off[k]):int(seg_off[k]) + int(seg_len[k])].tobytes()
        frame = frame[:CUT]
        L = len(frame)
        f = min(int(frm[i]), L) if frm is not None else 0
        t = min(int(take[i]), L - f) if take is not None else L - f
        parts.append(frame[f:f + t])
        off.append(o)
        lens.append(t)
        o += t
    src = np.frombuffer(b"".join(parts) + bytes(64), dtype=np.uint8).copy()
    return src, np.array(off, dtype=np.uint64), np.array(lens, dtype=np.uint16)


def apply(dst, hdr: bytes, sets, sums, arena, seg_off, seg_len, pkt_seg, dst_off, frm=None,
          take=None):
    """In place on `dst` (numpy u8).  Returns (dst, lens): the arena after the
    call and the values of d_taken."""
    src, off, lens = linearise(arena, seg_off, seg_len, pkt_seg, frm, take)
    oracle.emit_batch(hdr, sets, src, off, lens, dst, dst_off)
    emit_csum_model.apply(dst, hdr, list(sums or ()), dst_off, lens, sets)
    return dst, lens
