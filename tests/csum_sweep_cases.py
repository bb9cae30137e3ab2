"""Batches, edit lists and crafted emit cases shared by
tests/test_csum_sweep_model.py (CPU), tests/test_modify_csum_sweep.py and
tests/test_emit_csum_edges.py (GPU).  TEST INFRASTRUCTURE ONLY.

Rewrite side: one small batch per chain (hand-built frames of
tests/csum_frames.py; the tunnel: generated Geneve frames), indexed at odd
addresses and as fixed slots, with every checksum made valid by
tests/csum_model.py's fill; the single-edit sweep over every field, layer, op
and a few values; named lists of dependent edits; seeded random lists.
`define` is the definition (oracle rewrite + tests/csum_update_model.py),
`two_pass` the rewrite followed by a checksum fill, `qualifies` the frames on
which the two must agree.

Emit side: crafted batches for ingot_gpu_emit_packets_csum whose sums land on
0 / 0xffff and their neighbours, the largest sums, and the largest header
blocks.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

import oracle
from ingot_amd import Chain, EditOp, EmitSource, EmitSum, Field, GenProfile
from ingot_amd import emit as E
from ingot_amd.abi import CSUM_L3, CSUM_L4, CSUM_OUTER_L4, MAX_EDITS, MAX_EMIT_SETS, L3Kind, L4Kind
from ingot_amd.hostgen import gen_frames_host
from tests import csum_frames as cf
from tests import csum_model as model
from tests import csum_update_model as upd
from tests import emit_csum_cases as ecases
from tests import emit_csum_model as emodel

TUN = Chain.GeneveOverV6Tunnel
OK, NONE = int(model.OK), int(model.NONE)
SET, ADD, SUB, AND, OR, XOR = (EditOp.SET, EditOp.ADD, EditOp.SUB, EditOp.AND, EditOp.OR,
                               EditOp.XOR)
F = Field

# enum ingot_field -> width in bits (the setters' geometry, include/ingot_gpu.h)
FIELD_BITS = dict(zip(Field, (
    16, 3, 1, 12, 16,
    4, 4, 6, 2, 16, 16, 3, 13, 8, 8, 16, 32, 32,
    4, 6, 2, 20, 16, 8, 8,
    16, 16, 32, 32, 4, 4, 8, 16, 16, 16,
    16, 16, 16, 16, 8, 8, 16,
    2, 6, 8, 16, 24, 8)))
assert len(FIELD_BITS) == len(Field) == 48

# fields the fused update refuses: they move a sum's extent or pseudo-header
REFUSED = (F.V4_IHL, F.V4_TOTAL_LEN, F.V4_PROTOCOL, F.V6_PAYLOAD_LEN, F.V6_NEXT_HEADER)
CSUM_FIELDS = (F.V4_CHECKSUM, F.TCP_CHECKSUM, F.UDP_CHECKSUM, F.ICMP_CHECKSUM)
ALLOWED = tuple(f for f in Field if f not in REFUSED)

CHAINS = (Chain.UdpParser, Chain.GenericUlp, Chain.VlanUlp, TUN)
# (layer, vlan index) of every layer of a chain; the header kinds found there
LAYERS = {
    Chain.UdpParser: ((0, 0), (1, 0), (2, 0)),
    Chain.GenericUlp: ((0, 0), (1, 0), (2, 0)),
    Chain.VlanUlp: ((0, 0), (1, 0), (1, 1), (2, 0), (3, 0)),
    TUN: tuple((k, 0) for k in range(7)),
}
_L3, _L4 = ("V4", "V6"), ("TCP", "UDP", "ICMP")
LAYER_KINDS = {
    Chain.UdpParser: (("ETH",), _L3, ("UDP",)),
    Chain.GenericUlp: (("ETH",), _L3, _L4),
    Chain.VlanUlp: (("ETH",), ("VLAN",), _L3, _L4),
    TUN: (("ETH",), ("V6",), ("UDP",), ("GENEVE",), ("ETH",), _L3, _L4),
}
L3_LAYER = {Chain.UdpParser: 1, Chain.GenericUlp: 1, Chain.VlanUlp: 2, TUN: 5}
WHATS = {c: (CSUM_L3, CSUM_L4, CSUM_L3 | CSUM_L4) for c in CHAINS}
WHATS[TUN] = (CSUM_L3, CSUM_L4, CSUM_OUTER_L4, CSUM_L3 | CSUM_L4, 7)


def kind_of(field) -> str:
    return Field(field).name.split("_")[0]


def applies(chain, layer: int, field) -> bool:
    """Whether `field`'s header can be the one at `layer` of `chain`."""
    return kind_of(field) in LAYER_KINDS[chain][layer]


def fields_of(chain):
    """The fields some layer of `chain` can hold."""
    return tuple(f for f in Field if any(applies(chain, l, f)
                                         for l in range(len(LAYER_KINDS[chain]))))


# ---------------------------------------------------------------------------
# Batches
# ---------------------------------------------------------------------------
# arena: read-only u8; off / lens: what the call takes (None for slots);
# starts / lengths: every frame's place, for the models; keep: the frames whose
# sums the fill computes (before any edit); o_udp: tunnel only.
Batch = namedtuple("Batch", "arena off lens stride n starts lengths keep o_udp")


def _pay(k: int, n: int) -> bytes:
    return bytes((7 * i + 13 * k + 1) & 0xFF for i in range(n))


def frame_kinds(vlan=(), size=None):
    """IPv4 and IPv6 x TCP, UDP, ICMP x payloads of 0, 1 and 37 B; IPv4 with
    options; a first fragment (MF set); a later fragment.  `size`: one frame
    per kind, its payload chosen so that the frame is exactly `size` bytes."""
    kinds = [(l3, p, {}) for l3 in ("v4", "v6") for p in (cf.TCP, cf.UDP, "icmp")]
    kinds += [("v4", cf.UDP, dict(options=bytes([0x94, 4, 0, 0, 1, 1, 1, 0]))),
              ("v4", cf.TCP, dict(flags_frag=0x2000)),
              ("v4", cf.UDP, dict(flags_frag=0x00B9))]
    out = []
    for k, (l3, p, kw) in enumerate(kinds):
        if p == "icmp":
            p = cf.ICMP4 if l3 == "v4" else cf.ICMP6
        base = len(cf.frame(l3, p, b"", vlan=vlan, **kw))
        pays = (0, 1, 37) if size is None and not kw else (5,) if size is None else (size - base,)
        out += [cf.frame(l3, p, _pay(k + j, n), vlan=vlan, **kw) for j, n in enumerate(pays)]
    if size is not None:
        assert {len(f) for f in out} == {size}
    return out


def _frames_for(chain, size=None):
    if chain == Chain.VlanUlp:
        return frame_kinds((0x0123,), size) + frame_kinds((0x0123, 0x0456), size)
    return frame_kinds((), size)


def _fill_chain(chain):
    return Chain.GenericUlp if chain == Chain.UdpParser else chain


def _finish(arena, off, lens, stride, n, starts, lengths, chain):
    """Make every sum valid (the tunnel: inner sums, then the outer UDP sum
    under a UdpParser parse) and freeze the batch."""
    fc = _fill_chain(chain)
    rows = model.fill(arena, starts, lengths, oracle.parse_batch(arena, starts, lengths, fc))
    keep = (rows["l4_state"] == OK) & ((rows["l3_state"] == OK) | (rows["l3_state"] == NONE))
    o_udp = None
    if chain == TUN:
        rows_o = model.fill(arena, starts, lengths,
                            oracle.parse_batch(arena, starts, lengths, Chain.UdpParser),
                            what=CSUM_L4)
        keep &= rows_o["l4_state"] == OK
        o_udp = oracle.geneve_fields_batch(arena, starts, lengths)["outer"]["outer_udp_off"]
    arena.setflags(write=False)
    return Batch(arena, off, lens, stride, n, starts, lengths, keep, o_udp)


def _tunnel_frames():
    a, o, ln = gen_frames_host(GenProfile.GENEVE, 60, seed=31, slack=64)
    return [a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, ln)] * 2


def _indexed_from(frames, chain, prepare=None):
    gap, mis = (2, 9) if chain == TUN else (3, 1)
    arena, off, lens = cf.place(frames, gap=gap, misalign=mis)
    if prepare:
        prepare(arena, off, lens, chain)
    return _finish(arena, off, lens, 0, len(off), off, lens, chain)


def _strided_from(frames, chain, prepare=None):
    stride = (max(len(f) for f in frames) + 15) // 16 * 16
    n = len(frames)
    arena = np.zeros(n * stride + 64, np.uint8)  # (the tunnel's frames are padded with 0)
    for i, f in enumerate(frames):
        arena[i * stride:i * stride + len(f)] = np.frombuffer(f, np.uint8)
    starts = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    lengths = np.full(n, stride, np.uint16)
    if prepare:
        prepare(arena, starts, lengths, chain)
    return _finish(arena, None, None, stride, n, starts, lengths, chain)


def _source_frames(chain, layout):
    if chain == TUN:
        return _tunnel_frames()
    reps = 2 if chain == Chain.VlanUlp else 4
    if layout == "indexed":
        return _frames_for(chain) * reps  # 84 frames: two waves
    return _frames_for(chain, 128) * (reps * 2)  # 72 slots of 128 B


@lru_cache(maxsize=None)
def batch(chain, layout: str, prepared: bool = False) -> Batch:
    """layout "indexed": frames at odd addresses, 0xA5 between them; "strided":
    fixed slots (128 B; the tunnel: its longest frame rounded up to 16 B).
    UdpParser shares GenericUlp's frames.  `prepared`: see `_edge_sums`."""
    frames = _source_frames(chain, layout)
    make = _indexed_from if layout == "indexed" else _strided_from
    b = make(frames, chain, _edge_sums if prepared else None)
    assert b.n > 64
    return b


def source_frames(chain, layout: str = "indexed"):
    """The frames batch(chain, layout) is made of."""
    return _source_frames(chain, layout)


def batch_of(frames, chain, prepare=None) -> Batch:
    """An indexed batch of `frames` as batch(chain, "indexed") lays them out,
    every sum made valid; prepare(arena, off, lens, chain) runs before the
    fill."""
    return _indexed_from(list(frames), chain, prepare)


@lru_cache(maxsize=None)
def batch_at(chain, mis: int) -> Batch:
    """The chain's frames (once), every one of them `mis` bytes into a 16-B
    block: where the staged window ends inside a frame follows `mis`, so over
    mis = 0..15 it ends inside every field it can."""
    frames = _tunnel_frames()[:60] if chain == TUN else _frames_for(chain)
    offsets, o = [], 0
    for f in frames:
        offsets.append(o + mis)
        o += (mis + len(f) + 15) // 16 * 16 + 16
    arena, off, lens = cf.place(frames, offsets=offsets)
    return _finish(arena, off, lens, 0, len(off), off, lens, chain)


def _edge_sums(arena, starts, lengths, chain):
    """In place, before the fill: every IPv4 header's identification and every
    UDP header's source port are solved so that the header / segment words add
    up to 0xffff, a computed checksum of 0: IPv4 writes 0x0000, UDP 0xffff.
    After the fill every second IPv4 header's field is forced to the other
    representation of the same sum, 0xffff (_other_repr)."""
    fc = _fill_chain(chain)
    recs = oracle.parse_batch(arena, starts, lengths, fc)
    where = []
    for i in range(len(starts)):
        r, o = recs[i], int(starts[i])
        if int(r["status"]) != 0:
            continue
        if int(r["l3_kind"]) == int(L3Kind.IPV4):
            where.append((i, o + int(r["l3_off"]) + 4, o + int(r["l3_off"]) + 10, CSUM_L3))
        if int(r["l4_kind"]) == int(L4Kind.UDP):
            where.append((i, o + int(r["l4_off"]), o + int(r["l4_off"]) + 6, CSUM_L4))
    for _, word, _, _ in where:
        arena[word:word + 2] = 0
    # the sum is linear: with the word at 0 the fill writes c; the word c then
    # makes the words add up to 0xffff.  L3 first (the L4 fill does not cover it)
    for what in (CSUM_L3, CSUM_L4):
        scratch = arena.copy()
        model.fill(scratch, starts, lengths, recs)
        for _, word, field, w in where:
            if w == what:
                arena[word:word + 2] = scratch[field:field + 2]


def other_repr(b: Batch, chain):
    """-> (a copy of `b` in which every second IPv4 checksum of 0x0000 reads
    0xffff, the field offsets that hold 0x0000, those that hold 0xffff, the UDP
    field offsets that hold 0xffff)."""
    arena = b.arena.copy()
    recs = oracle.parse_batch(arena, b.starts, b.lengths, _fill_chain(chain))
    zero, ones, udp = [], [], []
    for i in range(b.n):
        r, o = recs[i], int(b.starts[i])
        if int(r["status"]) != 0:
            continue
        if int(r["l3_kind"]) == int(L3Kind.IPV4):
            at = o + int(r["l3_off"]) + 10
            if arena[at] == 0 and arena[at + 1] == 0:
                if len(zero) > len(ones):
                    arena[at:at + 2] = 0xFF
                    ones.append(at)
                else:
                    zero.append(at)
        if int(r["l4_kind"]) == int(L4Kind.UDP):
            at = o + int(r["l4_off"]) + 6
            if arena[at] == 0xFF and arena[at + 1] == 0xFF:
                udp.append(at)
    arena.setflags(write=False)
    return b._replace(arena=arena), zero, ones, udp


# ---------------------------------------------------------------------------
# The definition, the two-pass way, and where they must agree
# ---------------------------------------------------------------------------
def changed_frames(b: Batch, after) -> np.ndarray:
    idx = np.nonzero(after != b.arena)[0]
    if idx.size == 0:
        return idx
    return np.unique(np.searchsorted(b.starts, idx.astype(np.uint64), side="right") - 1)


def define(b: Batch, chain, edits, what):
    """-> (the definition's arena, the rewrite alone, the records, the frames
    the rewrite changed).  A frame the rewrite left alone has a delta of 0 for
    every sum, so csum_update_model touches only the changed ones
    (tests/test_csum_sweep_model.py holds this shortcut to the full update)."""
    rewritten = np.array(b.arena)
    recs = oracle.parse_modify_batch(rewritten, b.off, b.lens, chain, edits, stride=b.stride,
                                     n=b.n)
    ch = changed_frames(b, rewritten)
    want = rewritten.copy()
    if what and ch.size:
        upd.update(b.arena, want, b.starts[ch], b.lengths[ch], recs[ch], what,
                   o_udp=None if b.o_udp is None else b.o_udp[ch])
    return want, rewritten, recs, ch


def _fill_ok(b, chain, arena, recs, ch, what, outer):
    """Checksum fill of frames `ch` of `arena` in place -> the frames (a mask
    over `ch`) whose sums it computed."""
    ok = np.ones(len(ch), bool)
    if what:
        rows = model.fill(arena, b.starts[ch], b.lengths[ch], recs[ch], what=what)
        if what & CSUM_L4:
            ok &= rows["l4_state"] == OK
        if what & CSUM_L3:
            ok &= (rows["l3_state"] == OK) | (rows["l3_state"] == NONE)
    if outer:
        o_rec = oracle.parse_batch(arena, b.starts[ch], b.lengths[ch], Chain.UdpParser)
        ok &= model.fill(arena, b.starts[ch], b.lengths[ch], o_rec, what=CSUM_L4)["l4_state"] == OK
    return ok


def qualifies(b: Batch, chain, edits, rewritten, recs, ch) -> np.ndarray:
    """The frames (mask over the batch) on which the fused update must equal
    rewrite + fill: fill sums the frame both before and after the rewrite, and
    the list edits no checksum field."""
    if any(e[1] in CSUM_FIELDS for e in edits):
        return np.zeros(b.n, bool)
    q = b.keep.copy()
    if ch.size:
        q[ch] &= _fill_ok(b, chain, rewritten.copy(), recs, ch, CSUM_L3 | CSUM_L4, chain == TUN)
    return q


def two_pass(b: Batch, chain, rewritten, recs, ch, what) -> np.ndarray:
    """The rewrite followed by a checksum fill of the same sums (inner first,
    then the tunnel's outer UDP sum under a UdpParser parse)."""
    tp = rewritten.copy()
    if ch.size:
        _fill_ok(b, chain, tp, recs, ch, what & (CSUM_L3 | CSUM_L4), bool(what & CSUM_OUTER_L4))
    return tp


def frames_differ(b: Batch, got, want, frames):
    """The first of `frames` (indices) whose bytes differ, or None."""
    for i in frames:
        o, ln = int(b.starts[i]), int(b.lengths[i])
        if got[o:o + ln].tobytes() != want[o:o + ln].tobytes():
            return int(i)
    return None


# ---------------------------------------------------------------------------
# Edit lists
# ---------------------------------------------------------------------------
def sweep_values(field, layer: int, seed: int = 2024):
    """1, all-ones, the field's own top bit, one seeded random word."""
    rng = np.random.default_rng([seed, int(field), layer])
    return (1, 0xFFFFFFFF, 1 << (FIELD_BITS[Field(field)] - 1), int(rng.integers(0, 1 << 32)))


def sweep(chain, field, ops=tuple(EditOp)):
    """The single-edit sweep of `field`: (layer, field, op, value, index) over
    every layer of the chain (VLAN: both tag indices), `ops`, and four values."""
    for layer, index in LAYERS[chain]:
        for op in ops:
            for v in sweep_values(field, layer):
                yield (layer, Field(field), op, v, index)


def tag(chain, layout, edit_or_edits, what):
    """What a failing case is called: chain, layout, layer, field, op, value, what."""
    edits = [edit_or_edits] if not isinstance(edit_or_edits, list) else edit_or_edits
    es = [f"L{e[0]}{'[%d]' % e[4] if len(e) > 4 and e[4] else ''} {Field(e[1]).name} "
          f"{EditOp(e[2]).name} {e[3]:#x}" for e in edits]
    return f"{Chain(chain).name} {layout} what={what}: " + "; ".join(es)


def dependent_lists(chain):
    """-> [(name, edits, prepared)]: lists whose edits depend on one another.
    `prepared` lists run on batch(chain, layout, prepared=True) after
    other_repr (sums of 0 in both representations)."""
    l3 = L3_LAYER[chain]
    l4 = l3 + 1
    V = 0x5AA5C33C
    out = [
        ("twice set add", [(l3, F.V4_SOURCE, SET, 0x0A000001), (l3, F.V4_SOURCE, ADD, 0x01FF02FE)]),
        ("twice sub sub", [(l4, F.UDP_DESTINATION, SUB, 1), (l4, F.UDP_DESTINATION, SUB, 0xFFFF),
                           (l4, F.TCP_SEQUENCE, SUB, 0x01020305), (l4, F.TCP_SEQUENCE, SUB, 7),
                           (l3, F.V6_HOP_LIMIT, SUB, 1), (l3, F.V6_HOP_LIMIT, SUB, 64)]),
        # 4-byte fields that lie across the end of the staged window in some
        # frames (48 B from the 16-B block an indexed frame starts in, 64 B of
        # a slot): the second edit's read takes bytes from both sides
        ("twice across the window", [
            (l3, F.V4_DESTINATION, XOR, V), (l3, F.V4_DESTINATION, ADD, 0x01FF02FE),
            (l4, F.TCP_SEQUENCE, XOR, V), (l4, F.TCP_SEQUENCE, SUB, 0x01FF02FE),
            (l4, F.TCP_ACKNOWLEDGEMENT, XOR, V), (l4, F.TCP_ACKNOWLEDGEMENT, ADD, 0x01FF02FE),
            (l4, F.UDP_DESTINATION, XOR, 0xFFFF), (l4, F.UDP_DESTINATION, ADD, 0x0101),
            (l4, F.UDP_SOURCE, XOR, 0xFFFF), (l4, F.UDP_SOURCE, SUB, 0x0101)]),
        ("dscp ecn", [(l3, F.V4_DSCP, SET, 0x2E), (l3, F.V4_ECN, OR, 3), (l3, F.V4_DSCP, XOR, 0x3F),
                      (l3, F.V4_ECN, SUB, 1)]),
        ("flags offset kept 0", [(l3, F.V4_FLAGS, XOR, 2), (l3, F.V4_FRAGMENT_OFFSET, SET, 0)]),
        ("flags offset moved", [(l3, F.V4_FLAGS, SET, 1), (l3, F.V4_FRAGMENT_OFFSET, SET, 0x1ABC)]),
        ("offset moved and back", [(l3, F.V4_FRAGMENT_OFFSET, ADD, 0x1FFF),
                                   (l3, F.V4_FLAGS, XOR, 7), (l3, F.V4_FRAGMENT_OFFSET, ADD, 1)]),
        ("tcp byte 12 13", [(l4, F.TCP_DATA_OFFSET, SET, 6), (l4, F.TCP_RESERVED, XOR, 0xF),
                            (l4, F.TCP_FLAGS, AND, 0x12), (l4, F.TCP_DATA_OFFSET, SUB, 1)]),
        ("v6 first word", [(l3, F.V6_VERSION, SET, 6), (l3, F.V6_DSCP, ADD, 0x15),
                           (l3, F.V6_ECN, XOR, 3), (l3, F.V6_FLOW_LABEL, SET, 0xFFFFF),
                           (l3, F.V6_DSCP, SUB, 0x3F), (l3, F.V6_FLOW_LABEL, ADD, 1)]),
        ("csum first", [(l3, F.V4_CHECKSUM, ADD, 0x0101), (l3, F.V4_HOP_LIMIT, SUB, 1),
                        (l3, F.V4_SOURCE, SET, 0xC0A80A0A), (l4, F.UDP_CHECKSUM, XOR, 0x8001),
                        (l4, F.UDP_SOURCE, ADD, 7), (l4, F.TCP_CHECKSUM, SET, 0),
                        (l4, F.TCP_DESTINATION, SET, 8443), (l4, F.ICMP_CHECKSUM, SUB, 1),
                        (l4, F.ICMP_CODE, ADD, 1)]),
        ("csum middle", [(l3, F.V4_HOP_LIMIT, SUB, 1), (l3, F.V4_CHECKSUM, ADD, 0x0101),
                         (l3, F.V4_SOURCE, SET, 0xC0A80A0A), (l4, F.UDP_SOURCE, ADD, 7),
                         (l4, F.UDP_CHECKSUM, XOR, 0x8001), (l4, F.UDP_DESTINATION, SUB, 1),
                         (l4, F.TCP_DESTINATION, SET, 8443), (l4, F.TCP_CHECKSUM, SET, 0),
                         (l4, F.TCP_WINDOW_SIZE, ADD, 1), (l4, F.ICMP_TY, SET, 0),
                         (l4, F.ICMP_CHECKSUM, SUB, 1), (l4, F.ICMP_CODE, ADD, 1)]),
        ("csum last", [(l3, F.V4_HOP_LIMIT, SUB, 1), (l3, F.V4_SOURCE, SET, 0xC0A80A0A),
                       (l3, F.V4_CHECKSUM, ADD, 0x0101), (l4, F.UDP_SOURCE, ADD, 7),
                       (l4, F.UDP_CHECKSUM, XOR, 0x8001), (l4, F.TCP_DESTINATION, SET, 8443),
                       (l4, F.TCP_CHECKSUM, SET, 0xFFFF), (l4, F.ICMP_CODE, ADD, 1),
                       (l4, F.ICMP_CHECKSUM, SET, 0xFFFF)]),
    ]
    # 16 edits, all on an IPv4 / TCP frame: every field to all-ones, every
    # field to 0, and eight fields to all-ones and back to 0 (the largest
    # terms, which must telescope)
    v4tcp = [(l3, F.V4_VERSION), (l3, F.V4_DSCP), (l3, F.V4_ECN), (l3, F.V4_IDENTIFICATION),
             (l3, F.V4_HOP_LIMIT), (l3, F.V4_SOURCE), (l3, F.V4_DESTINATION), (l4, F.TCP_SOURCE),
             (l4, F.TCP_DESTINATION), (l4, F.TCP_SEQUENCE), (l4, F.TCP_ACKNOWLEDGEMENT),
             (l4, F.TCP_DATA_OFFSET), (l4, F.TCP_RESERVED), (l4, F.TCP_FLAGS),
             (l4, F.TCP_WINDOW_SIZE), (l4, F.TCP_URGENT_PTR)]
    assert len(v4tcp) == MAX_EDITS
    out += [
        ("16 to all-ones", [(l, f, OR, 0xFFFFFFFF) for l, f in v4tcp]),
        ("16 to zero", [(l, f, AND, 0) for l, f in v4tcp]),
        ("8 to all-ones and back", [e for l, f in v4tcp[3:11]
                                    for e in ((l, f, SET, 0xFFFFFFFF), (l, f, SET, 0))]),
    ]
    nat = [(l3, F.V4_SOURCE, SET, 0x0A000001), (l3, F.V4_DESTINATION, SET, 0x0A000002),
           (l3, F.V4_HOP_LIMIT, SUB, 1), (l3, F.V4_DSCP, SET, 0x2E),
           (l3, F.V4_IDENTIFICATION, ADD, 1), (l3, F.V6_HOP_LIMIT, SUB, 1),
           (l3, F.V6_FLOW_LABEL, XOR, 0xABCDE), (l4, F.UDP_SOURCE, SET, 40001),
           (l4, F.UDP_DESTINATION, SUB, 1), (l4, F.TCP_SOURCE, SET, 40001),
           (l4, F.TCP_DESTINATION, SET, 8443), (l4, F.TCP_SEQUENCE, ADD, 0x00010000),
           (l4, F.TCP_ACKNOWLEDGEMENT, SUB, 0x00010000), (l4, F.ICMP_CODE, ADD, 1)]
    if chain == Chain.VlanUlp:
        nat += [(1, F.VLAN_VID, SET, 0x7FF, 0), (1, F.VLAN_PRIORITY, SET, 5, 1)]
    elif chain == TUN:
        nat += [(3, F.GENEVE_VNI, SET, 0xABCDEF), (2, F.UDP_SOURCE, XOR, 0x0FF0)]
    else:
        nat += [(l3, F.V6_DSCP, SET, 0x2E), (l4, F.TCP_WINDOW_SIZE, SUB, 1)]
    assert len(nat) == MAX_EDITS
    out.append(("16 nat", nat))
    out = [(n, e, False) for n, e in out]
    # an edit and its inverse, and single edits, on sums of 0 / 0xffff
    out += [
        ("inverse xor xor", [(l3, F.V4_DESTINATION, XOR, V), (l3, F.V4_DESTINATION, XOR, V),
                             (l4, F.UDP_DESTINATION, XOR, 0xF00F),
                             (l4, F.UDP_DESTINATION, XOR, 0xF00F)], True),
        ("inverse add sub", [(l3, F.V4_HOP_LIMIT, ADD, 9), (l3, F.V4_HOP_LIMIT, SUB, 9),
                             (l4, F.UDP_SOURCE, ADD, 0x1234),
                             (l4, F.UDP_SOURCE, SUB, 0x1234)], True),
        ("from zero sums", [(l3, F.V4_HOP_LIMIT, SUB, 1), (l4, F.UDP_SOURCE, ADD, 1)], True),
        ("by 0xffff", [(l3, F.V4_IDENTIFICATION, XOR, 0xFFFF),
                       (l4, F.UDP_DESTINATION, XOR, 0xFFFF)], True),
    ]
    assert all(len(e) <= MAX_EDITS for _, e, _ in out)
    return out


def random_lists(chain, count: int = 200, seed: int = 77):
    """`count` seeded lists of 1-16 edits over the allowed fields, all ops and
    layers; four in five edits name a field its layer can hold."""
    rng = np.random.default_rng([seed, int(chain)])
    layers = LAYERS[chain]
    fitting = [(l, i, f) for l, i in layers for f in ALLOWED if applies(chain, l, f)]
    ops = tuple(EditOp)
    out = []
    for _ in range(count):
        edits = []
        for _ in range(int(rng.integers(1, MAX_EDITS + 1))):
            if rng.random() < 0.8:
                l, i, f = fitting[int(rng.integers(len(fitting)))]
            else:
                l, i = layers[int(rng.integers(len(layers)))]
                f = ALLOWED[int(rng.integers(len(ALLOWED)))]
            bits = FIELD_BITS[f]
            v = int(rng.integers(0, 1 << 32)) if rng.random() < 0.5 else \
                int(rng.integers(0, 1 << bits))
            if rng.random() < 0.15:
                v = (0, 1, (1 << bits) - 1, 0xFFFFFFFF)[int(rng.integers(4))]
            edits.append((l, f, ops[int(rng.integers(len(ops)))], v, i))
        out.append(edits)
    return out


# ---------------------------------------------------------------------------
# Emit with checksums: crafted batches
# ---------------------------------------------------------------------------
# a crafted batch: what the call takes (host form) and the bytes the named
# packets' checksum fields must hold; checks = [(packet, field offset in the
# packet, bytes, note)]
EmitCase = namedtuple("EmitCase", "name hdr sets sums src off lens dst_off size checks")

CRAFTED_AT = (0, 63, 64, 255, 256, 599)  # wave and group edges, the last packet
N_CRAFTED = 600
ZERO_LENGTHS = (2, 3, 17, 1025)


def _udp_sum(sums):
    return next(s for s in sums if int(s[0]) == int(EmitSum.UDP))


def _place(lens, hdr_len, dmis_of, rng, first=5):
    """Destination offsets: one packet after another with 0-3 B between them;
    packet k of `dmis_of` starts at an address = dmis_of[k] mod 16."""
    off, o = [], first
    for k, ln in enumerate(np.asarray(lens).astype(np.int64)):
        o += int(rng.integers(0, 4))
        if k in dmis_of:
            o += (dmis_of[k] - o) % 16
        off.append(o)
        o += hdr_len + int(ln)
    return np.array(off, np.uint64), o + 64


def _model(hdr, sets, sums, src, off, lens, dst_off, size, only=None):
    want = np.full(size, 0xA5, np.uint8)
    oracle.emit_batch(hdr, sets, src, off, lens, want, dst_off)
    if only is None:
        return emodel.apply(want, hdr, sums, dst_off, lens, sets)
    emodel.check_args(bytes(hdr), sets, sums)
    for k in only:
        o = int(dst_off[k])
        emodel.one(want[o:o + len(hdr) + int(lens[k])], bytes(hdr), sums)
    return want


def _be16(a, at):
    return (int(a[at]) << 8) | int(a[at + 1])


def computed_zero_cases(name: str, dmis: int, seed: int = 5):
    """Two batches of 600 for stack `name`: at CRAFTED_AT sit packets of the
    four ZERO_LENGTHS whose first payload word makes the UDP segment add up to
    0xffff (a computed 0, written 0xffff), to 0xfffe (0x0001) and to 0x10000
    (0xfffe), all at destination misalignment `dmis`."""
    combos = [(ln, v) for ln in ZERO_LENGTHS for v in (0, -1, 1)]
    out = []
    for half in range(2):
        rng = np.random.default_rng([seed, dmis, half, ecases.STACKS.index(name)])
        mine = {CRAFTED_AT[(k + dmis) % 6]: combos[6 * half + k] for k in range(6)}
        lens = rng.integers(0, 200, N_CRAFTED).astype(np.uint16)
        for k, (ln, _) in mine.items():
            lens[k] = ln
        src, off = ecases.random_source(lens, rng)
        hdr, sets, sums = ecases.stack(name, N_CRAFTED, rng)
        fat = _udp_sum(sums)[1] + 6
        dst_off, size = _place(lens, len(hdr), {k: dmis for k in mine}, rng)
        for k in mine:
            src[int(off[k]):int(off[k]) + 2] = 0
        base = _model(hdr, sets, sums, src, off, lens, dst_off, size, only=mine)
        checks = []
        for k, (ln, v) in mine.items():
            c = _be16(base, int(dst_off[k]) + fat)
            # with the word at 0 the field is c: the words add up to ~c, and
            # the word c + v makes them 0xffff + v
            assert 1 <= c <= 0xFFFD, c
            w = c + v
            src[int(off[k])], src[int(off[k]) + 1] = w >> 8, w & 0xFF
            want = {0: b"\xff\xff", -1: b"\x00\x01", 1: b"\xff\xfe"}[v]
            checks.append((k, fat, want, f"len {ln} word c{v:+d}"))
        out.append(EmitCase(f"{name} dmis {dmis} #{half}", hdr, sets, sums, src, off, lens,
                            dst_off, size, checks))
    return out


def ipv4_zero_case(name: str, seed: int = 6):
    """Stack `name` (geneve_v4 / vlan_v4opt) with a per-packet identification:
    at CRAFTED_AT it is solved so that the IPv4 header words add up to 0xffff
    (field 00 00: IPv4 has no 0xffff mapping) and to its two neighbours; the
    crafted packets take destination misalignments 0, 1, 6, 7, 14 and 15."""
    rng = np.random.default_rng([seed, ecases.STACKS.index(name)])
    n = N_CRAFTED
    lens = rng.integers(0, 200, n).astype(np.uint16)
    src, off = ecases.random_source(lens, rng)
    hdr, sets, sums = ecases.stack(name, n, rng)
    v4_at = next(s for s in sums if int(s[0]) == int(EmitSum.IPV4))[1]
    ident = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
    sets = [s for s in sets if s[1] != F.V4_IDENTIFICATION] + \
        [(v4_at, F.V4_IDENTIFICATION, EmitSource.U16, 0, ident)]
    mine = dict(zip(CRAFTED_AT, (0, -1, 1, 0, 1, -1)))
    dst_off, size = _place(lens, len(hdr), dict(zip(CRAFTED_AT, (0, 1, 6, 7, 14, 15))), rng)
    for k in mine:
        ident[k] = 0
    base = _model(hdr, sets, sums, src, off, lens, dst_off, size, only=mine)
    checks = []
    for k, v in mine.items():
        c = _be16(base, int(dst_off[k]) + v4_at + 10)
        assert 1 <= c <= 0xFFFD, c
        ident[k] = c + v
        want = {0: b"\x00\x00", -1: b"\x00\x01", 1: b"\xff\xfe"}[v]
        checks.append((k, v4_at + 10, want, f"identification c{v:+d}"))
    return EmitCase(f"{name} ipv4 zero", hdr, sets, sums, src, off, lens, dst_off, size, checks)


def largest_sum_case(name: str, parity: int, smis: int, seed: int = 7):
    """Stack `name`: payloads of all 0xff and of all 0x00 at every length of
    EDGE_LENGTHS and at the lengths that make the UDP segment S = 65,534,
    65,535 and 65,536 bytes (the last is no datagram and keeps its field), in
    a batch of 600 with CRAFTED_AT among their places.  Crafted packets start
    at destination addresses of `parity` and source misalignment `smis`."""
    rng = np.random.default_rng([seed, parity, smis, ecases.STACKS.index(name)])
    n = N_CRAFTED
    hdr, sets, sums = ecases.stack(name, n, rng)
    u_at = _udp_sum(sums)[1]
    lengths = list(ecases.EDGE_LENGTHS) + [S - (len(hdr) - u_at) for S in (65534, 65535, 65536)]
    assert lengths[-1] <= 65535 and len(hdr) - u_at + ecases.EDGE_LENGTHS[-1] > 65535
    crafted = [(ln, fill) for ln in lengths for fill in (0xFF, 0x00)]
    places = list(CRAFTED_AT) + [k for k in range(20, 580, 21)]
    places = places[:len(crafted)]
    assert len(places) == len(crafted) and len(set(places)) == len(places)
    lens = rng.integers(0, 200, n).astype(np.uint16)
    for k, (ln, _) in zip(places, crafted):
        lens[k] = ln
    # sources: every payload 16-B aligned + `smis` for the crafted ones
    ln64 = lens.astype(np.int64)
    off = np.zeros(n, np.int64)
    o = 0
    for k in range(n):
        o = (o + 15) // 16 * 16 + (smis if k in places else int(rng.integers(0, 16)))
        off[k] = o
        o += int(ln64[k])
    src = rng.integers(0, 256, o + 64, dtype=np.uint8)
    for k, (ln, fill) in zip(places, crafted):
        src[int(off[k]):int(off[k]) + ln] = fill
    dmis_of = {k: parity + 2 * int(rng.integers(0, 8)) for k in places}
    dst_off, size = _place(lens, len(hdr), dmis_of, rng)
    checks = []
    for k, (ln, fill) in zip(places, crafted):
        if len(hdr) - u_at + ln > 65535:  # no datagram: the field is as emitted
            checks.append((k, u_at + 6, bytes(hdr[u_at + 6:u_at + 8]), f"len {ln} kept"))
    return EmitCase(f"{name} largest parity {parity} smis {smis}", hdr, sets, sums, src,
                    off.astype(np.uint64), lens, dst_off, size, checks)


V6_S, V6_D = ecases.V6_S, ecases.V6_D


def _geneve_opts(total: int) -> bytes:
    """`total` bytes of Geneve options, each at most 4 + 124 B."""
    out, k = b"", 0
    while len(out) < total:
        data = min(124, total - len(out) - 4)
        out += E.geneve_opt(0x0129, k, bytes((3 * i + k) & 0xFF for i in range(data)))
        k += 1
    assert len(out) == total
    return out


def big_stack(name: str, n: int, rng):
    """-> (hdr, sets, sums): header blocks near the 256-B limit, with the most
    setters the call takes; one setter targets a checksum field that a named
    sum must override."""
    def u16():
        return rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)

    def u32(bits=32):
        return rng.integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)

    L, U16, U32, VAL = EmitSource.LENGTH, EmitSource.U16, EmitSource.U32, EmitSource.VALUE
    if name == "geneve_v6_opts":
        # Eth / IPv6 / UDP / Geneve + 184 B of options: the field sits early,
        # the header part of the segment is long (254 B in all)
        hdr = (E.ethernet(ecases.MAC_D, ecases.MAC_S, 0x86DD) + E.ipv6(V6_S, V6_D, 17)
               + E.udp(0xC0DE, 6081) + E.geneve(0x123456, options=_geneve_opts(184)))
        sets = [(14, F.V6_PAYLOAD_LEN, L, -40), (54, F.UDP_LENGTH, L, 0),
                (54, F.UDP_SOURCE, U16, 0, u16()), (62, F.GENEVE_VNI, U32, 0, u32(24)),
                (14, F.V6_FLOW_LABEL, U32, 0, u32(20)), (14, F.V6_HOP_LIMIT, VAL, 0xF0),
                (54, F.UDP_CHECKSUM, U16, 0, u16()), (14, F.V6_DSCP, VAL, 0x2E)]
        sums = [(EmitSum.UDP, 54, 14)]
    elif name == "geneve_v4_opts":
        # the IPv4 variant, both sums named, setters on both checksum fields
        hdr = (E.ethernet(ecases.MAC_D, ecases.MAC_S, 0x0800)
               + E.ipv4(ecases.V4_S, ecases.V4_D, 17) + E.udp(0xC0DE, 6081)
               + E.geneve(0x00ABCD, options=_geneve_opts(204)))
        sets = [(14, F.V4_TOTAL_LEN, L, 0), (34, F.UDP_LENGTH, L, 0),
                (14, F.V4_SOURCE, U32, 0, u32()), (14, F.V4_IDENTIFICATION, U16, 0, u16()),
                (34, F.UDP_SOURCE, U16, 0, u16()), (42, F.GENEVE_VNI, U32, 0, u32(24)),
                (34, F.UDP_CHECKSUM, U16, 0, u16()), (14, F.V4_CHECKSUM, U16, 0, u16())]
        sums = [(EmitSum.IPV4, 14), (EmitSum.UDP, 34, 14)]
    elif name == "vlan_v6_hbh":
        # Eth / VLAN / IPv6 + a 176-B hop-by-hop header / UDP / Geneve + one
        # option: at = 234, l3_at = 18; the field's chunk is the region's last,
        # and the pseudo-header's next header is the constant 17, not the
        # header's own byte (0)
        hbh = E.ipv6_ext_6564(17, bytes((5 * i + 1) & 0xFF for i in range(174)))
        assert len(hbh) == 176
        hdr = (E.ethernet(ecases.MAC_D, ecases.MAC_S, 0x8100) + E.vlan(0x123, 0x86DD)
               + E.ipv6(V6_S, V6_D, 0, v6ext=hbh) + E.udp(0xC0DE, 6081)
               + E.geneve(0x123456, options=E.geneve_opt(0x0129, 0)))
        assert len(hdr) == 254
        sets = [(18, F.V6_PAYLOAD_LEN, L, -40), (234, F.UDP_LENGTH, L, 0),
                (234, F.UDP_SOURCE, U16, 0, u16()), (242, F.GENEVE_VNI, U32, 0, u32(24)),
                (18, F.V6_FLOW_LABEL, U32, 0, u32(20)), (14, F.VLAN_VID, U16, 0, u16()),
                (234, F.UDP_CHECKSUM, U16, 0, u16()), (18, F.V6_HOP_LIMIT, VAL, 0xF0)]
        sums = [(EmitSum.UDP, 234, 18)]
    elif name == "v6_dstopts":
        # small: Eth / IPv6 + an 8-B destination-options header / UDP
        hdr = (E.ethernet(ecases.MAC_D, ecases.MAC_S, 0x86DD)
               + E.ipv6(V6_S, V6_D, 60, v6ext=E.ipv6_ext_6564(17, bytes([1, 4, 0, 0, 0, 0])))
               + E.udp(0x1234, 4789))
        sets = [(14, F.V6_PAYLOAD_LEN, L, -40), (62, F.UDP_LENGTH, L, 0),
                (62, F.UDP_SOURCE, U16, 0, u16())]
        sums = [(EmitSum.UDP, 62, 14)]
    else:
        raise KeyError(name)
    assert len(hdr) <= 256 and len(sets) <= MAX_EMIT_SETS
    return hdr, sets, sums


BIG_STACKS = ("geneve_v6_opts", "geneve_v4_opts", "vlan_v6_hbh", "v6_dstopts")


def big_header_case(name: str, seed: int = 8):
    """257 packets (a group and one more) under big_stack(name), every length
    of EDGE_LENGTHS among them."""
    rng = np.random.default_rng([seed, BIG_STACKS.index(name)])
    n = 257
    lens = rng.integers(0, 300, n).astype(np.uint16)
    lens[rng.permutation(n)[:len(ecases.EDGE_LENGTHS)]] = np.asarray(ecases.EDGE_LENGTHS, np.uint16)
    src, off = ecases.random_source(lens, rng)
    hdr, sets, sums = big_stack(name, n, rng)
    dst_off, size = ecases.pack(lens, len(hdr), rng)
    return EmitCase(f"big {name}", hdr, sets, sums, src, off, lens, dst_off, size, [])


def emit_model(c: EmitCase) -> np.ndarray:
    """The definition's arena of a crafted batch (0xA5 where no packet is)."""
    return _model(c.hdr, c.sets, c.sums, c.src, c.off, c.lens, c.dst_off, c.size)


def held(c: EmitCase, got) -> None:
    """The crafted packets' checksum fields hold the bytes they were built for."""
    for k, at, want, note in c.checks:
        o = int(c.dst_off[k]) + at
        assert got[o:o + 2].tobytes() == want, (c.name, k, note, got[o:o + 2].tobytes().hex())


def bytewise_receiver_ok(pkt, hdr, sums) -> bool:
    """RFC 1071 byte by byte over the pseudo-header and the UDP segment of one
    emitted packet, field included: a receiver accepts when it is 0xffff."""
    _, at, l3 = _udp_sum(sums)
    S = len(pkt) - at
    if hdr[l3] >> 4 == 4:
        pseudo = bytes(pkt[l3 + 12:l3 + 20]) + bytes([0, 17]) + S.to_bytes(2, "big")
    else:
        pseudo = bytes(pkt[l3 + 8:l3 + 40]) + S.to_bytes(4, "big") + bytes([0, 0, 0, 17])
    total = 0
    for data in (pseudo, bytes(pkt[at:])):
        d = np.frombuffer(data, np.uint8)  # even places are the words' high bytes
        total += (int(d[0::2].sum(dtype=np.uint64)) << 8) + int(d[1::2].sum(dtype=np.uint64))
    while total >> 16:
        total = (total & 0xFFFF) + (total >> 16)
    return total == 0xFFFF
