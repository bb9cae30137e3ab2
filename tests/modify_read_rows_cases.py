"""Chunked batches, edit lists and tables shared by
tests/test_modify_read_rows_model.py (CPU), tests/test_modify_read_rows.py
(GPU), tools/bigfuzz.py and tools/modify_rows_probe.py.  TEST INFRASTRUCTURE
ONLY.

Chunk tables come from tests/modify_read_cases.py (cut_set, header_cuts,
single_chunk_tables) and tests/csum_read_cases.py (cut, cut_at, place); frames
whose sums are right, tables and device_edits from tests/modify_rows_cases.py.
mixed_edits / mixed_rows restate the patterns of tests/test_modify_rows.py.

Every batch the GPU file uses is a Batch made by batch() (or a named builder
below, registered in GPU_BATCHES), so that tests/test_modify_read_rows_model.py
can hold each of them to the chunk paths it is meant to reach.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

import oracle
from ingot_amd import abi
from ingot_amd.abi import ROW_NONE, Chain, EditOp, Field, WideField
from tests import csum_frames as cf
from tests import csum_read_cases as cases
from tests import modify_read_cases as mc
from tests import modify_read_model as mrm
from tests import modify_rows_cases as rc
from tests import modify_rows_model as rows_model
from tests.modify_rows_cases import col_u16, col_u32

TUN = Chain.GeneveOverV6Tunnel
SET, ADD, SUB, XOR, OR = EditOp.SET, EditOp.ADD, EditOp.SUB, EditOp.XOR, EditOp.OR
CHAINS = (Chain.UdpParser, Chain.GenericUlp, Chain.VlanUlp, TUN)
L3_LABEL = {Chain.UdpParser: 1, Chain.GenericUlp: 1, Chain.VlanUlp: 2, TUN: 5}
PROFILE = {Chain.UdpParser: "MIXED", Chain.GenericUlp: "MIXED", Chain.VlanUlp: "VLAN_V6EH",
           TUN: "GENEVE"}
FULL_WHAT = {Chain.UdpParser: 3, Chain.GenericUlp: 3, Chain.VlanUlp: 3, TUN: 7}
N_ROWS = 37

# tables: (arena, seg_off, seg_len, pkt_seg); rows None: no d_row
Batch = namedtuple("Batch", "name tables chain edits rows n_rows")


def valid_whats(chain):
    return tuple(range(8)) if chain == TUN else tuple(range(4))


# ---------------------------------------------------------------------------
# Rows and edit lists (the patterns of tests/test_modify_rows.py)
# ---------------------------------------------------------------------------
def mixed_rows(n, seed=5):
    """Valid rows, INGOT_ROW_NONE and n_rows itself."""
    rows = np.random.default_rng(seed).integers(0, N_ROWS, n).astype(np.uint32)
    rows[2::5] = ROW_NONE
    rows[3::11] = N_ROWS
    return rows


def mixed_edits(chain, n, seed=1):
    """VALUE, U16, U32 and BYTES operands, by packet (table `t`, 32-B rows) and
    by row (table `r`); ops other than SET on per-packet operands; UDP's source
    edited twice; a 32-bit operand into a 16-bit field; byte rows at odd
    addresses."""
    t, r = rc.nat_table(n, seed), rc.nat_table(N_ROWS, seed + 100)
    dense = (np.arange(n, dtype=np.uint16) * 3 + 1) % 7  # a dense array: pitch 0
    l3 = L3_LABEL[chain]
    l4 = l3 + 1
    e = [(l3, Field.V4_SOURCE, SET, col_u32(t)), (l4, Field.UDP_SOURCE, SET, col_u16(t)),
         (l4, Field.TCP_SEQUENCE, ADD, ("row", col_u32(r))), (l3, Field.V4_HOP_LIMIT, SUB, 1),
         (l3, Field.V6_HOP_LIMIT, SUB, dense), (l3, WideField.V6_SOURCE, SET, ("row", r[:, 16:32])),
         (l3, WideField.V6_DESTINATION, SET, t[:, 13:29]),
         (0, WideField.ETH_DESTINATION, SET, t[:, 8:14]),
         (0, WideField.ETH_SOURCE, SET, ("row", r[:, 1:7])),
         (l4, Field.UDP_SOURCE, XOR, ("row", col_u16(r, 4))),
         (l4, Field.TCP_DESTINATION, SET, col_u32(t, 20)), (l3, Field.V4_DSCP, OR, col_u16(t, 24)),
         (l4, Field.ICMP_CODE, ADD, col_u16(t, 26))]
    if chain == Chain.VlanUlp:
        e += [(1, Field.VLAN_VID, ADD, col_u16(t, 28), 1), (1, Field.VLAN_PRIORITY, XOR, dense, 0)]
    if chain == TUN:
        e = e[:11] + [(1, WideField.V6_SOURCE, SET, t[:, 16:32]),
                      (4, WideField.ETH_SOURCE, SET, ("row", r[:, 20:26])),
                      (3, Field.GENEVE_VNI, SET, col_u32(t, 0)),
                      (2, Field.UDP_SOURCE, XOR, col_u16(t, 30)),
                      (1, WideField.V6_DESTINATION, SET, ("row", r[:, 7:23]))]
    assert len(e) <= abi.MAX_EDITS
    return e


def value_edits(edits):
    """A VALUE-only narrow list (ingot_edit tuples) as parse_modify_rows takes it."""
    return [tuple(e) for e in edits]


# ---------------------------------------------------------------------------
# Frames
# ---------------------------------------------------------------------------
def _crafted(chain):
    """Frames the generator sets may lack: no payload (the L4 header in the
    packet's last chunk), QinQ under VlanUlp (headers in chunks 3 and 4)."""
    if chain == TUN:
        arena, off, lens = rc.right_sum_tunnel_frames()
        recs = oracle.parse_batch(arena, off, lens, TUN)
        fs = cases.frames_of(arena, off, lens)
        # (cut at payload_off: the lengths inside no longer fit; the parse does
        # not look at them, and the model and the device see the same bytes)
        return [fs[0][:int(recs["payload_off"][0])], fs[7], fs[20][:int(recs["payload_off"][20])],
                fs[30]]
    vl = ((), (5,), (5, 6)) if chain == Chain.VlanUlp else ((),)
    out = []
    for v in vl:
        out += [cf.frame("v4", cf.UDP, b"", vlan=v), cf.frame("v6", cf.TCP, b"", vlan=v),
                cf.frame("v6", cf.UDP, bytes(range(9)), vlan=v),
                cf.frame("v4", cf.TCP, bytes(range(5)), vlan=v)]
    return out


@lru_cache(maxsize=None)
def frames(profile: str, chain, cutter: str, n: int):
    """`n` frames of modify_read_cases.cut_set with the crafted ones spread
    among them (from n = 64 on) -> (frames, their contiguous records, the
    tunnel's outer blocks or None, cut_set's own chunked packets)."""
    arena, off, lens, packets = mc.cut_set(profile, chain, cutter, n)
    fs = cases.frames_of(arena, off, lens)
    swapped = set()
    if n >= 64:
        extra = _crafted(chain)
        for j, f in enumerate(extra):
            at = 1 + j * ((n - 2) // len(extra))
            fs[at] = f
            swapped.add(at)
    a2, o2, l2 = cf.place(fs)
    recs = oracle.parse_batch(a2, o2, l2, chain)
    outer = oracle.geneve_fields_batch(a2, o2, l2)["outer"] if chain == TUN else None
    packets = [None if i in swapped else p for i, p in enumerate(packets)]
    return fs, recs, outer, packets


def not_ok(packets, fs):
    """Three packets that do not parse Ok, in place (n >= 12): a header cut in
    two (StraddledHeader), no chunks, a truncated frame (TooSmall)."""
    if len(packets) >= 12:
        packets[5] = cases.cut_at(fs[5], [17])
        packets[9] = []
        packets[11] = [fs[11][:16]]
    return packets


def chunk_packets(profile, chain, cutter, n, style):
    """style "cut": cut_set's own cuts (csum_read_cases.cut, or split anywhere
    for the adversarial sets); "headers": one header per chunk; "single"."""
    fs, recs, outer, own = frames(profile, chain, cutter, n)
    rng = np.random.default_rng(29)
    out = []
    for i, f in enumerate(fs):
        if style == "single":
            out.append([f])
        elif style == "headers":
            vl = int(recs["n_vlan"][i]) if chain == Chain.VlanUlp else 0
            cuts = mc.header_cuts(chain, recs[i], None if outer is None else outer[i], vl)
            out.append(cases.cut_at(f, [c for c in cuts if c < len(f)]))
        else:
            out.append(own[i] if own[i] is not None else cases.cut(f, recs[i], rng))
    # (one chunk per packet stays comparable with the contiguous call)
    return out if style == "single" else not_ok(out, fs)


def place_descending(packets, gap: int = 3, misalign=(7, 2, 13, 8, 5, 0, 10, 15, 1, 4, 11, 6, 3)):
    """The batch's chunks at descending addresses (chunk c + 1 below chunk c),
    starts at every address mod 4 (13 misalignments against any chunk count)."""
    flat = [ch for p in packets for ch in p]
    arena, so, sl, _ = cases.place([[ch] for ch in reversed(flat)], misalign=list(misalign),
                                   gap=gap)
    so = np.r_[so[:-1][::-1], so[-1:]]
    sl = np.r_[sl[:-1][::-1], sl[-1:]]
    ps = np.cumsum([0] + [len(p) for p in packets]).astype(np.uint32)
    return arena, so, sl, ps


def _freeze(tables):
    for a in tables:
        a.setflags(write=False)
    return tuple(tables)


@lru_cache(maxsize=None)
def batch(chain, n: int, style: str = "cut", by_row: bool = True, placement: str = "ascending",
          profile: str = None, cutter: str = "cut", seed: int = 1) -> Batch:
    """The chain's generator set at `n` packets, chunked by `style`, every
    chunk at its own misalignment 0..15; the chain's mixed edit list and (by_row)
    mixed rows.  by_row False: the BY_ROW operands by packet instead, no d_row."""
    profile = profile or PROFILE[chain]
    packets = chunk_packets(profile, chain, cutter, n, style)
    if placement == "descending":
        tables = place_descending(packets)
    else:
        tables = cases.place(packets, misalign=tuple(range(16)) + (5,), gap=1)
    edits = mixed_edits(chain, n, seed)
    rows = mixed_rows(n) if by_row else None
    if not by_row:
        big = rc.nat_table(n, seed + 200)  # (the by-row tables hold N_ROWS rows only)
        edits = [(*e[:3], _by_packet(e[3], big), *e[4:]) for e in edits]
    return Batch(f"{chain.name}-{n}-{style}-{placement}-{'rows' if by_row else 'packets'}",
                 _freeze(tables), chain, edits, rows, N_ROWS if by_row else 0)


def _by_packet(op, big):
    """A ("row", table) operand as a by-packet view of `big` with the same row
    width and element type."""
    if not isinstance(op, tuple):
        return op
    t = op[1]
    if t.dtype == np.uint8:
        return big[:, 3:3 + t.shape[1]]
    return col_u32(big, 8) if t.dtype.itemsize == 4 else col_u16(big, 6)


@lru_cache(maxsize=None)
def tile_batch(n: int) -> Batch:
    """Tile edges: MIXED frames from cut_set under GenericUlp."""
    return batch(Chain.GenericUlp, n)


# ---------------------------------------------------------------------------
# Which chunk an applied piece lands in
# ---------------------------------------------------------------------------
def pieces_of(e):
    """Edit tuple -> [(header kind, byte offset in the header, bytes)]: the
    4-byte (a MAC's last: 2-byte) pieces of a wide field, a narrow field's
    covering bytes."""
    field = e[1]
    if rows_model.is_wide(field):
        kind, at, nb = rows_model.WIDE[WideField(int(field))]
        return [(kind, at + b, min(4, nb - b)) for b in range(0, nb, 4)]
    kind, first, bits = mrm.GEOMETRY[Field(field)]
    lo, hi = first // 8, (first + bits + 7) // 8
    return [(kind, lo, hi - lo)]


def applied_pieces(b: Batch, parsed=None):
    """Every piece applied to an Ok, unguarded packet -> [(packet, chunk index,
    chunks of the packet, chunk address of the piece, bytes)]."""
    arena, seg_off, seg_len, pkt_seg = b.tables
    recs, gf, _ = parsed if parsed is not None else mrm.parse(b.tables, b.chain)
    out = []
    for i in range(len(pkt_seg) - 1):
        if int(recs["status"][i]) != 0 or (b.rows is not None and int(b.rows[i]) >= b.n_rows):
            continue
        ks = list(range(int(pkt_seg[i]), int(pkt_seg[i + 1])))
        starts = np.cumsum([0] + [int(seg_len[k]) for k in ks])
        outer = gf["outer"][i] if b.chain == TUN else None
        for e in b.edits:
            index = int(e[4]) if len(e) > 4 else 0
            for kind, at, nb in pieces_of(e):
                have, h = mrm.header_at(b.chain, recs[i], outer, int(e[0]), index)
                if have != kind:
                    continue
                x = h + at
                c = int(np.searchsorted(starts, x, side="right")) - 1
                while int(seg_len[ks[c]]) == 0:
                    c += 1
                assert x + nb <= starts[c + 1], "a piece lies in one chunk"
                out.append((i, c, len(ks), int(seg_off[ks[c]]) + x - int(starts[c]), nb))
    return out


def paths(b: Batch, parsed=None):
    """The chunk paths of the kernel's view that the batch's applied pieces
    take: "first" (chunk 0), "prefetched" (chunk 1-3, not the packet's last),
    "last" (the packet's last chunk, not chunk 0), "late" (index >= 4)."""
    got = set()
    for _, c, nk, _, _ in applied_pieces(b, parsed):
        if c == 0:
            got.add("first")
        if 1 <= c <= 3 and c + 1 < nk:
            got.add("prefetched")
        if c > 0 and c + 1 == nk:
            got.add("last")
        if c >= 4:
            got.add("late")
    return got


def expected_paths(b: Batch, style: str):
    """What a batch chunked by `style` must reach, wherever its chain allows:
    index >= 4 only for the tunnel (inner Ethernet, L3, L4 at 4-6) and QinQ
    under VlanUlp; GenericUlp and UdpParser cannot get there (parse_read
    rejects a packet with an empty chunk between headers)."""
    if style == "single":
        return {"first"}
    want = {"first", "prefetched", "last"}
    if style == "headers" and b.chain in (TUN, Chain.VlanUlp):
        want.add("late")
    return want


# ---------------------------------------------------------------------------
# Named batches of the GPU file
# ---------------------------------------------------------------------------
def dependent_lists(chain, n):
    """Lists that only come out right when a later edit, or csum_finish, reads
    what the located store wrote: a field SET twice from two tables; a wide
    SET, then narrow ops on bytes next to and inside what wide pieces wrote
    (ETH plus the VLAN and L4 cases); a checksum field SET from a table, then
    updated by `what`."""
    t, r = rc.nat_table(n, 31), rc.nat_table(N_ROWS, 32)
    l3 = L3_LABEL[chain]
    l4 = l3 + 1
    twice = [(l3, Field.V4_SOURCE, SET, col_u32(t)),
             (l3, Field.V4_SOURCE, SET, ("row", col_u32(r))),
             (l3, WideField.V6_DESTINATION, SET, t[:, 3:19]),
             (l3, WideField.V6_DESTINATION, SET, ("row", r[:, 16:32])),
             (l4, Field.UDP_DESTINATION, SET, col_u16(t)),
             (l4, Field.UDP_DESTINATION, SET, ("row", col_u16(r, 8))),
             (l4, Field.TCP_SOURCE, SET, ("row", col_u16(r, 8))),
             (l4, Field.TCP_SOURCE, SET, col_u16(t, 2))]
    wide_then_narrow = [(0, WideField.ETH_SOURCE, SET, t[:, 8:14]),
                        (0, WideField.ETH_DESTINATION, SET, ("row", r[:, 1:7])),
                        (0, Field.ETH_ETHERTYPE, XOR, 0),
                        (l4, Field.TCP_SEQUENCE, SET, col_u32(t, 20)),
                        (l4, Field.TCP_SEQUENCE, ADD, ("row", col_u32(r, 4))),
                        (l4, Field.TCP_DATA_OFFSET, OR, 0),
                        (l4, Field.UDP_SOURCE, SET, col_u16(t, 4)),
                        (l4, Field.UDP_SOURCE, SUB, 1),
                        (l3, Field.V6_HOP_LIMIT, SET, col_u16(t, 6)),
                        (l3, Field.V6_HOP_LIMIT, SUB, 1),
                        (l3, Field.V4_HOP_LIMIT, SET, col_u16(t, 6)),
                        (l3, Field.V4_DSCP, XOR, 0x15)]
    if chain == Chain.VlanUlp:
        wide_then_narrow += [(1, Field.VLAN_ETHERTYPE, SET, col_u16(t, 10), 0),
                             (1, Field.VLAN_VID, ADD, 1, 0), (1, Field.VLAN_PRIORITY, XOR, 5, 1)]
    if chain == TUN:
        wide_then_narrow += [(4, WideField.ETH_SOURCE, SET, t[:, 8:14]),
                             (4, Field.ETH_ETHERTYPE, XOR, 0),
                             (3, Field.GENEVE_VNI, SET, col_u32(t, 12))]
    csum_set = [(l3, Field.V4_CHECKSUM, SET, col_u16(t, 14)), (l3, Field.V4_HOP_LIMIT, SUB, 1),
                (l4, Field.UDP_CHECKSUM, SET, ("row", col_u16(r, 2))),
                (l4, Field.UDP_SOURCE, ADD, 3),
                (l4, Field.TCP_CHECKSUM, SET, col_u16(t, 16)),
                (l4, Field.TCP_SEQUENCE, XOR, col_u32(t, 24)),
                (l4, Field.ICMP_CHECKSUM, SET, col_u16(t, 18)), (l4, Field.ICMP_CODE, ADD, 1),
                (l3, WideField.V6_SOURCE, SET, ("row", r[:, 9:25]))]
    if chain == TUN:
        csum_set += [(2, Field.UDP_CHECKSUM, SET, col_u16(t, 30)),
                     (1, WideField.V6_SOURCE, SET, t[:, 16:32])]
    return [("set twice", twice), ("wide, then narrow", wide_then_narrow),
            ("checksum set, then updated", csum_set)]


def with_edits(b: Batch, name: str, edits, rows=None, n_rows=None) -> Batch:
    """`b` with another list (and, if given, other rows / another n_rows)."""
    return Batch(f"{b.name}/{name}", b.tables, b.chain, edits, b.rows if rows is None else rows,
                 b.n_rows if n_rows is None else n_rows)


def one_survivor_rows(n):
    """One row below n_rows per 64-packet tile, at a different lane each."""
    rows = np.full(n, ROW_NONE, np.uint32)
    for t in range((n + 63) // 64):
        rows[min(n - 1, 64 * t + (13 * t + 7) % 64)] = t % N_ROWS
    return rows


def receiver_batch(tunnel: bool) -> Batch:
    """Frames whose every sum is right, one header per chunk, a wide-and-narrow
    list by packet."""
    arena, off, lens = rc.right_sum_tunnel_frames() if tunnel else rc.right_sum_frames()
    chain = TUN if tunnel else Chain.VlanUlp
    recs = oracle.parse_batch(arena, off, lens, chain)
    outer = oracle.geneve_fields_batch(arena, off, lens)["outer"] if tunnel else None
    packets = []
    for i, f in enumerate(cases.frames_of(arena, off, lens)):
        cuts = mc.header_cuts(chain, recs[i], None if outer is None else outer[i],
                              0 if tunnel else int(recs["n_vlan"][i]))
        packets.append(cases.cut_at(f, [c for c in cuts if c < len(f)]))
    tables = cases.place(packets, misalign=tuple(range(16)) + (9,), gap=2)
    t = rc.nat_table(len(off), 11)
    edits = rc.tunnel_edits(t) if tunnel else rc.nat_edits(t, 2)
    return Batch("receiver-" + chain.name, _freeze(tables), chain, edits, None, 0)


def placement_edits(chain, n):
    """2-, 4-, 6- and 16-byte whole-byte SETs; the byte tables' rows at odd
    addresses and odd pitches (35 and 19 bytes)."""
    rng = np.random.default_rng(41)
    a, b = rng.integers(0, 256, (n, 35), dtype=np.uint8), rng.integers(0, 256, (N_ROWS, 19),
                                                                       dtype=np.uint8)
    t = rc.nat_table(n, 42)
    l3 = L3_LABEL[chain]
    l4 = l3 + 1
    e = [(l4, Field.UDP_SOURCE, SET, col_u16(t)), (l4, Field.TCP_DESTINATION, SET, col_u16(t, 6)),
         (l3, Field.V4_DESTINATION, SET, col_u32(t, 8)),
         (l4, Field.TCP_SEQUENCE, SET, col_u32(t, 12)),
         (0, WideField.ETH_DESTINATION, SET, a[:, 1:7]),
         (0, WideField.ETH_SOURCE, SET, ("row", b[:, 3:9])),
         (l3, WideField.V6_SOURCE, SET, a[:, 9:25]),
         (l3, WideField.V6_DESTINATION, SET, ("row", b[:, 1:17])),
         (l3, Field.V6_HOP_LIMIT, SET, col_u16(t, 16)), (l3, Field.V4_IDENTIFICATION, SET, 0xBEEF)]
    if chain == TUN:
        e += [(4, WideField.ETH_DESTINATION, SET, a[:, 27:33]),
              (1, WideField.V6_SOURCE, SET, a[:, 17:33]), (2, Field.UDP_SOURCE, SET, col_u16(t, 18))]
    return e


def neighbours(b: Batch, parsed=None):
    """Arena indices of the byte before and the byte after every applied piece."""
    idx = set()
    for _, _, _, at, nb in applied_pieces(b, parsed):
        idx.update((at - 1, at + nb))
    return np.array(sorted(idx))


@lru_cache(maxsize=None)
def value_batch(profile: str, chain, cutter: str, n: int = 300) -> Batch:
    """One of modify_read_cases.CUT_SETS with the VALUE-only NAT list."""
    _, _, _, packets = mc.cut_set(profile, chain, cutter, n)
    tables = cases.place(packets, misalign=tuple(range(16)) + (5,), gap=1)
    return Batch(f"value-{profile}-{chain.name}-{cutter}", _freeze(tables), chain,
                 value_edits(mc.nat_list(chain)[0]), None, 0)


@lru_cache(maxsize=None)
def not_ok_batch() -> Batch:
    """ADVERSARIAL frames split anywhere (StraddledHeader), a truncated frame
    (TooSmall) and packets with no chunks."""
    return batch(Chain.GenericUlp, 300, profile="ADVERSARIAL", cutter="split")


def gpu_batches():
    """Every batch tests/test_modify_read_rows.py runs -> [(Batch, style of its
    chunks, what it must hold: "paths", "guarded", "not ok", "mod 4")].  A
    batch of one packet, one without d_row and one whose every packet is
    guarded cannot hold all of them; what each of those still must hold is
    listed here."""
    full = ("paths", "guarded", "not ok", "mod 4")
    out = [(tile_batch(1), "cut", ()), (tile_batch(63), "cut", full), (tile_batch(64), "cut", full),
           (tile_batch(65), "cut", full), (tile_batch(129), "cut", full)]
    for chain in CHAINS:
        b = batch(chain, 257, "headers")
        out.append((b, "headers", full))
        out += [(with_edits(b, name, edits), "headers", ("guarded", "not ok"))
                for name, edits in dependent_lists(chain, 257)]
        out.append((batch(chain, 129, "single"), "single", ("paths", "guarded", "mod 4")))
        d = batch(chain, 257, "headers", placement="descending")
        out.append((with_edits(d, "placement", placement_edits(chain, 257)), "headers",
                    ("paths", "guarded", "not ok", "mod 4")))
    out += [(value_batch(*s), "cut", ("paths",)) for s in mc.CUT_SETS if s[2] == "cut"]
    out += [(value_batch(*s), "split", ()) for s in mc.CUT_SETS if s[2] == "split"]
    g = batch(Chain.GenericUlp, 257)
    out += [(g, "cut", full), (with_edits(g, "survivors", g.edits, one_survivor_rows(257)), "cut",
                               ("guarded", "not ok")),
            (batch(Chain.GenericUlp, 257, by_row=False), "cut", ("paths", "not ok", "mod 4")),
            (not_ok_batch(), "split", ("guarded", "not ok")),
            (batch(Chain.GenericUlp, 833), "cut", full)]
    return out


def random_lists(chain, n: int, count: int, seed: int):
    """`count` random mixed lists (tools/bigfuzz.py): 4 to 12 edits each, a
    third of them wide fields; narrow fields (never a refused one) with any
    op; operands VALUE, U16 or U32, by packet or by row, at random aligned
    columns of two NAT tables; mostly at layers that can hold the field."""
    from tests import csum_sweep_cases as sc

    rng = np.random.default_rng(seed)
    t, r = rc.nat_table(n, seed + 1), rc.nat_table(N_ROWS, seed + 2)
    kinds = sc.LAYER_KINDS[chain]
    fields = [f for f in sc.fields_of(chain) if f in sc.ALLOWED]
    out = []
    for _ in range(count):
        edits = []
        while len(edits) < int(rng.integers(4, 13)):
            by_row = rng.random() < 0.4
            tab = r if by_row else t
            w = (lambda x: ("row", x)) if by_row else (lambda x: x)
            if rng.random() < 0.33:
                field = list(WideField)[int(rng.integers(4))]
                kind, _, nb = rows_model.WIDE[field]
                layers = [k for k, ks in enumerate(kinds) if kind in ks]
                layer = layers[int(rng.integers(len(layers)))]
                at = int(rng.integers(0, 32 - nb + 1))
                edits.append((layer, field, SET, w(tab[:, at:at + nb])))
                continue
            field = fields[int(rng.integers(len(fields)))]
            layers = [(la, ix) for la, ix in sc.LAYERS[chain] if sc.applies(chain, la, field)]
            if rng.random() < 0.1:
                layers = list(sc.LAYERS[chain])
            layer, index = layers[int(rng.integers(len(layers)))]
            op = list(EditOp)[int(rng.integers(6))]
            src = int(rng.integers(3))
            if src == 0:
                operand = int(rng.integers(0, 1 << 32))
            elif src == 1:
                operand = w(col_u16(tab, 2 * int(rng.integers(16))))
            else:
                operand = w(col_u32(tab, 4 * int(rng.integers(8))))
            edits.append((layer, field, op, operand, index))
        out.append(edits)
    return out


def logical(arena, tables, i) -> bytes:
    return mc.logical(arena, tables, i)
