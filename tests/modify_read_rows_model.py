"""The definition of ingot_gpu_parse_read_modify_rows (include/ingot_gpu.h), in
numpy / Python.  TEST INFRASTRUCTURE ONLY.

Written from the header's text, not from the kernel: the two existing calls
composed.  For each packet:
  1. tests/modify_read_model.parse of its chunks (oracle.parse_read_batch): the
     parse sees the bytes before the edits, and the records and chunk indices
     are what it returns, for every packet;
  2. a packet that is not Ok, and (with `rows`) a packet whose rows[i] >= n_rows,
     keeps every byte;
  3. the chunks concatenated are the logical frame;
  4. tests/modify_rows_model.edit_packet on it: the packet's own concrete edit
     list from the tables (by packet or by row), narrow fields as big-endian bit
     runs, wide fields as byte slices, at the record's logical offsets;
  5. tests/modify_rows_model.sums when what != 0 (the IPv6 pseudo-header and
     the tunnel ranges included; inner sums before OUTER_L4; parity by logical
     offset, since the sums are taken over the logical frame);
  6. the bytes are scattered back into the chunks; everything else in the
     arena is unchanged.
"""
from __future__ import annotations

import numpy as np

from ingot_amd.abi import CSUM_L3, CSUM_L4, CSUM_OUTER_L4, Chain
from tests import modify_read_model as mrm
from tests import modify_rows_model as rows_model

TUN = Chain.GeneveOverV6Tunnel


def gather(arena, seg_off, seg_len, ks):
    """The logical frame of the chunks `ks`."""
    parts = [arena[int(seg_off[k]):int(seg_off[k]) + int(seg_len[k])] for k in ks]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def scatter(want, seg_off, seg_len, ks, frame) -> None:
    x = 0
    for k in ks:
        o, ln = int(seg_off[k]), int(seg_len[k])
        want[o:o + ln] = frame[x:x + ln]
        x += ln


def apply(tables, chain, edits, rows=None, n_rows: int = 0, what: int = 0, parsed=None):
    """-> (the arena after the call, the records, the chunk indices): what
    ingot_gpu_parse_read_modify_rows must leave of `tables` = (arena, seg_off,
    seg_len, pkt_seg).  `edits` and `rows` are tests/modify_rows_model's.
    `parsed`: modify_read_model.parse(tables, chain), when the caller has it."""
    if what & ~(CSUM_L3 | CSUM_L4 | CSUM_OUTER_L4) or ((what & CSUM_OUTER_L4) and chain != TUN):
        raise ValueError("what")
    arena, seg_off, seg_len, pkt_seg = tables
    recs, gf, chunk = parsed if parsed is not None else mrm.parse(tables, chain)
    want = np.array(arena)
    for i in range(len(pkt_seg) - 1):
        if int(recs["status"][i]) != 0:
            continue
        if rows is not None and int(rows[i]) >= n_rows:
            continue
        ks = range(int(pkt_seg[i]), int(pkt_seg[i + 1]))
        before = gather(arena, seg_off, seg_len, ks)
        after = before.copy()
        outer = gf["outer"][i] if chain == TUN else None
        rows_model.edit_packet(after, chain, recs[i], outer, edits, i, rows)
        if what:
            rows_model.sums(before, after, chain, recs[i], what,
                            int(outer["outer_udp_off"]) if chain == TUN else None)
        scatter(want, seg_off, seg_len, ks, after)
    return want, recs, chunk
