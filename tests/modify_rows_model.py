"""The definition of ingot_gpu_parse_modify_rows (include/ingot_gpu.h), in
numpy / Python.  TEST INFRASTRUCTURE ONLY.

Written from the header's text, not from the kernel.  For each packet:
  1. oracle.parse_batch's record (the tunnel's outer offsets from
     oracle.geneve_fields_batch);
  2. the row guard: with `rows`, a packet whose rows[i] >= n_rows keeps every
     byte;
  3. for a packet that parsed Ok the packet's own concrete edit list is built
     from the tables: edit k's operand is its int, row i of its table, or row
     rows[i] of it (("row", table));
  4. narrow fields go through tests/modify_read_model.edit_frame (big-endian
     bit runs, ops wrapping modulo 2^width); a wide field is a byte-slice
     assignment at its header + 0 / 6 (Ethernet) or + 8 / 24 (IPv6);
  5. the selected checksums from the words before and after, as
     tests/csum_update_model.one does, with the covered ranges the call adds:
     the IPv6 addresses in the L4 sum's pseudo-header, and the tunnel's outer
     IPv6 addresses in the outer UDP sum's.

Tables here are numpy arrays indexed by row: (rows,) or (rows, 1) integers for
narrow fields, (rows, 6 | 16) uint8 for wide ones.  Pitch is a matter of the
ABI only (a table may be a strided view of a larger one).
"""
from __future__ import annotations

import numpy as np

import oracle
from ingot_amd.abi import (CSUM_L3, CSUM_L4, CSUM_OUTER_L4, Chain, EditOp, L3Kind, L4Kind,
                           WideField)
from tests import csum_update_model as upd
from tests import modify_read_model as mrm

TUN = Chain.GeneveOverV6Tunnel
# wide field -> (header kind, byte offset in the header, bytes)
WIDE = {WideField.ETH_DESTINATION: ("ETH", 0, 6), WideField.ETH_SOURCE: ("ETH", 6, 6),
        WideField.V6_SOURCE: ("V6", 8, 16), WideField.V6_DESTINATION: ("V6", 24, 16)}
_FIELD_AT = {int(L4Kind.TCP): 16, int(L4Kind.UDP): 6, int(L4Kind.ICMPV4): 2,
             int(L4Kind.ICMPV6): 2}
_FIXED = {int(L4Kind.TCP): 20, int(L4Kind.UDP): 8, int(L4Kind.ICMPV4): 4, int(L4Kind.ICMPV6): 4}
_PSEUDO = (int(L4Kind.TCP), int(L4Kind.UDP), int(L4Kind.ICMPV6))


def is_wide(field) -> bool:
    return int(field) in [int(w) for w in WIDE]


def operand(op, i: int, rows):
    """Edit operand `op` for packet i: an int, or the bytes of a wide field."""
    if isinstance(op, tuple):
        assert op[0] == "row"
        op, i = op[1], int(rows[i])
    if isinstance(op, np.ndarray):
        v = op[i]
        return bytes(v) if v.dtype == np.uint8 and v.ndim == 1 and v.size > 1 else \
            int(np.asarray(v).reshape(-1)[0])
    return int(op)


def edit_packet(f, chain, rec, outer, edits, i: int, rows) -> None:
    """Packet i's edits, in order, on its frame `f` (numpy u8, in place)."""
    for e in edits:
        layer, field, op = int(e[0]), e[1], e[2]
        index = int(e[4]) if len(e) > 4 else 0
        v = operand(e[3], i, rows)
        if is_wide(field):
            assert EditOp(op) == EditOp.SET
            kind, at, nbytes = WIDE[WideField(int(field))]
            have, h = mrm.header_at(chain, rec, outer, layer, index)
            if have == kind:
                assert len(v) == nbytes
                f[h + at:h + at + nbytes] = np.frombuffer(v, np.uint8)
        else:
            mrm.edit_frame(f, chain, rec, outer, [(layer, field, op, v & 0xFFFFFFFF, index)])


def sums(b, a, chain, rec, what: int, o_udp=None) -> None:
    """One Ok frame: `b` before the call, `a` (writable) after the edits; the
    selected checksum fields of `a` are updated (RFC 1624 eqn. 3 over the
    covered words, tests/csum_update_model)."""
    L = len(a)
    l3_kind, l4_kind = int(rec["l3_kind"]), int(rec["l4_kind"])
    l3_off, l4_off = int(rec["l3_off"]), int(rec["l4_off"])
    v4, v6 = l3_kind == int(L3Kind.IPV4), l3_kind == int(L3Kind.IPV6)
    if (what & CSUM_L3) and v4:
        hl = min(max(20, (int(a[l3_off]) & 0xF) * 4), L - l3_off)
        upd._apply(a, l3_off + 10, upd.delta(b, a, [(l3_off, l3_off + hl)], l3_off + 10), False)
    if (what & CSUM_L4) and l4_kind in _FIELD_AT:
        later_fragment = v4 and (upd._word(a, l3_off + 6) & 0x1FFF) != 0
        if not later_fragment:
            ranges = [(l4_off, l4_off + _FIXED[l4_kind])]
            if v4 and l4_kind in _PSEUDO:
                ranges.append((l3_off + 12, l3_off + 20))
            if v6 and l4_kind in _PSEUDO:
                ranges.append((l3_off + 8, l3_off + 40))
            field = l4_off + _FIELD_AT[l4_kind]
            upd._apply(a, field, upd.delta(b, a, ranges, field), l4_kind == int(L4Kind.UDP))
    if what & CSUM_OUTER_L4:
        # after the inner sums; the pseudo-header is the outer IPv6 header's
        # addresses (the header follows the 14-B outer Ethernet)
        o = int(o_udp)
        upd._apply(a, o + 6, upd.delta(b, a, [(o, L), (14 + 8, 14 + 40)], o + 6), True)


def apply_whats(arena, off, lens, chain, edits, whats, rows=None, n_rows: int = 0,
                stride: int = 0, n=None):
    """apply() for several `what` values at once -> ([the arena after the call
    under each of `whats`], the records).  The edits do not depend on `what`,
    so they are made once; a frame whose bytes they left as they were has D = 0
    for every sum (no field is written) and is not summed."""
    for what in whats:
        if what & ~(CSUM_L3 | CSUM_L4 | CSUM_OUTER_L4) or ((what & CSUM_OUTER_L4) and chain != TUN):
            raise ValueError("what")
    if n is None:
        n = len(off)
    recs = oracle.parse_batch(arena, off, lens, chain, stride=stride, n=n)
    outer = None
    if chain == TUN:
        outer = oracle.geneve_fields_batch(arena, off, lens, stride=stride, n=n)["outer"]
    plain = np.array(arena)
    moved = []
    for i in range(n):
        if int(recs["status"][i]) != 0:
            continue
        if rows is not None and int(rows[i]) >= n_rows:
            continue
        o = int(off[i]) if off is not None else i * stride
        ln = int(lens[i]) if lens is not None else stride
        if off is None:
            ln = min(ln, stride)  # a slot holds at most one frame
        out_i = outer[i] if chain == TUN else None
        edit_packet(plain[o:o + ln], chain, recs[i], out_i, edits, i, rows)
        if plain[o:o + ln].tobytes() != arena[o:o + ln].tobytes():
            moved.append((i, o, ln))
    out = []
    for what in whats:
        want = plain.copy()
        for i, o, ln in moved if what else ():
            sums(arena[o:o + ln], want[o:o + ln], chain, recs[i], what,
                 int(outer[i]["outer_udp_off"]) if chain == TUN else None)
        out.append(want)
    return out, recs


def apply(arena, off, lens, chain, edits, rows=None, n_rows: int = 0, what: int = 0,
          stride: int = 0, n=None):
    """-> (the arena after the call, the records).  Every frame that is edited
    is summed, changed or not (apply_whats' shortcut is held to this by
    tests/test_modify_rows_sweep_model.py)."""
    if what & ~(CSUM_L3 | CSUM_L4 | CSUM_OUTER_L4) or ((what & CSUM_OUTER_L4) and chain != TUN):
        raise ValueError("what")
    if n is None:
        n = len(off)
    recs = oracle.parse_batch(arena, off, lens, chain, stride=stride, n=n)
    outer = None
    if chain == TUN:
        outer = oracle.geneve_fields_batch(arena, off, lens, stride=stride, n=n)["outer"]
    want = np.array(arena)
    for i in range(n):
        if int(recs["status"][i]) != 0:
            continue
        if rows is not None and int(rows[i]) >= n_rows:
            continue
        o = int(off[i]) if off is not None else i * stride
        ln = int(lens[i]) if lens is not None else stride
        if off is None:
            ln = min(ln, stride)  # a slot holds at most one frame
        before = arena[o:o + ln]
        after = want[o:o + ln]
        out_i = outer[i] if chain == TUN else None
        edit_packet(after, chain, recs[i], out_i, edits, i, rows)
        if what:
            sums(before, after, chain, recs[i], what,
                 int(out_i["outer_udp_off"]) if chain == TUN else None)
    return want, recs
