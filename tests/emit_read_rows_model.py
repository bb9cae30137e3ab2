"""The definition of ingot_gpu_emit_packets_read_rows (include/ingot_gpu.h), in
numpy / Python.  TEST INFRASTRUCTURE ONLY.

Written from the header's equivalence, on top of the two definitions that
exist: `emit_read_model.linearise` applies the payload rule of
ingot_gpu_emit_packets_read to the chunk tables and gives every packet's P_i
and t; `emit_rows_model.apply` is ingot_gpu_emit_packets_rows over those linear
payloads (setters in list order, sums after them, the row guard).

A packet whose row index is >= n_rows is not emitted: the arena keeps whatever
it held there, none of its chunks is looked at (its entries of seg_off /
seg_len may be garbage), and its `taken` is 0.

Sets are in emit_rows_model's host form.
"""
from __future__ import annotations

import numpy as np

from tests import emit_read_model, emit_rows_model


def apply(dst, hdr: bytes, sets, sums, arena, seg_off, seg_len, pkt_seg, dst_off, rows=None,
          n_rows: int = 0, frm=None, take=None):
    """In place on `dst` (numpy u8).  Returns (dst, taken): the arena after the
    call and the values of d_taken."""
    n = len(pkt_seg) - 1
    live = emit_rows_model.emitted(n, rows, n_rows)
    # a guarded packet has no chunks as far as the call is concerned
    seg = np.asarray(pkt_seg).astype(np.int64)
    lo, hi = seg[:-1].copy(), seg[1:].copy()
    hi[~live] = lo[~live]
    src_parts, off, lens, o = [], np.zeros(n, np.uint64), np.zeros(n, np.uint16), 0
    for i in range(n):
        if not live[i]:
            continue
        s, _, ln = emit_read_model.linearise(
            arena, seg_off, seg_len, np.array([lo[i], hi[i]]),
            None if frm is None else np.asarray(frm)[i:i + 1],
            None if take is None else np.asarray(take)[i:i + 1])
        src_parts.append(s[:int(ln[0])])
        off[i], lens[i] = o, ln[0]
        o += int(ln[0])
    src = np.concatenate(src_parts + [np.zeros(64, np.uint8)])
    emit_rows_model.apply(dst, hdr, sets, sums, src, off, lens, dst_off, rows, n_rows)
    return dst, lens


def check_args(ctx_ok: bool, hdr, hdr_len: int, sets, n_sets: int, sums, have_row: bool, n: int,
               dst_ok: bool = True, tables_ok: bool = True) -> None:
    """The argument errors of the call, raised (ValueError naming the step of
    the header's list) in its order.  Step 2 is steps 2 to 4 of
    emit_rows_model.check_args, named "2.<its step>"."""
    if not ctx_ok:
        raise ValueError("1: ctx NULL")
    try:
        emit_rows_model.check_args(True, hdr, hdr_len, sets, n_sets, sums, have_row, 0, True)
    except ValueError as err:
        raise ValueError(f"2.{err}") from None
    if n == 0:
        return
    if not dst_ok:
        raise ValueError("4: d_dst / d_dst_off NULL")
    if not tables_ok:
        raise ValueError("5: NULL chunk table")
