"""Frames, tables and edit lists of the deterministic sweep of
ingot_gpu_parse_modify_rows, shared by tests/test_modify_rows_sweep_model.py
(CPU) and tests/test_modify_rows_sweep.py (GPU).  TEST INFRASTRUCTURE ONLY;
numpy only.

A case is a Group: a batch of tests/csum_sweep_cases.py (frames whose sums are
right), an edit list in tests/modify_rows_model.py's form (numpy tables), the
row array, and the `what` values it runs under.  The definition is
tests/modify_rows_model.py; `second_way` is the plain rewrite (what = 0)
followed by the from-scratch fill of the same sums, on the frames the fill sums
before and after.

  A  narrow fields: the single-edit sweep by packet and by row
  B  wide fields: every layer, across the staged window's end, 64 pieces
  C  checksum value edges of the covered ranges the call adds
  D  tables: pitches, row offsets, the row guard
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

import oracle
from ingot_amd import Chain, EditOp, Field
from ingot_amd.abi import CSUM_L4, ROW_NONE, L3Kind, L4Kind, WideField
from tests import csum_model as model
from tests import csum_sweep_cases as sc
from tests import modify_read_model as mrm
from tests import modify_rows_cases as cases
from tests import modify_rows_model as rows_model

TUN = sc.TUN
SET = EditOp.SET
W = WideField
V6S, V6D, MACD, MACS = W.V6_SOURCE, W.V6_DESTINATION, W.ETH_DESTINATION, W.ETH_SOURCE
WIDTH = {MACD: 6, MACS: 6, V6S: 16, V6D: 16}
# the layers that can hold a wide field (include/ingot_gpu.h, "Fields")
WIDE_LAYERS = {c: {MACD: (0,), MACS: (0,), V6S: (sc.L3_LAYER[c],), V6D: (sc.L3_LAYER[c],)}
               for c in sc.CHAINS}
WIDE_LAYERS[TUN] = {MACD: (0, 4), MACS: (0, 4), V6S: (1, 5), V6D: (1, 5)}
WINDOW = {c: 48 for c in sc.CHAINS}  # the indexed launch's staged bytes
WINDOW[TUN] = 128

Group = namedtuple("Group", "name b chain edits rows n_rows whats")


def full(chain) -> int:
    return sc.WHATS[chain][-1]


def all_whats(chain):
    return (0,) + sc.WHATS[chain]


def by_row(x):
    return ("row", x)


def expected(g: Group):
    """-> ([the definition's arena under each of g.whats], the records)."""
    b = g.b
    return rows_model.apply_whats(b.arena, b.off, b.lens, g.chain, g.edits, g.whats, rows=g.rows,
                                  n_rows=g.n_rows, stride=b.stride, n=b.n)


def definition(g: Group, what: int):
    """rows_model.apply itself, one `what`."""
    b = g.b
    return rows_model.apply(b.arena, b.off, b.lens, g.chain, g.edits, rows=g.rows,
                            n_rows=g.n_rows, what=what, stride=b.stride, n=b.n)


def second_way(g: Group, plain, recs, what: int):
    """-> (rewrite + fill of the sums of `what`, the changed frames on which it
    must equal the definition).  `plain`: the definition under what = 0."""
    ch = sc.changed_frames(g.b, plain)
    q = sc.qualifies(g.b, g.chain, g.edits, plain, recs, ch)
    return sc.two_pass(g.b, g.chain, plain, recs, ch, what), ch[q[ch]], ch


def headers(b, chain):
    """-> (records, the tunnel's outer blocks or None) of a batch."""
    recs = oracle.parse_batch(b.arena, b.off, b.lens, chain, stride=b.stride, n=b.n)
    outer = None
    if chain == TUN:
        outer = oracle.geneve_fields_batch(b.arena, b.off, b.lens, stride=b.stride,
                                           n=b.n)["outer"]
    return recs, outer


def header_offsets(b, chain, layer: int, kind: str):
    """Per frame: the offset in the frame of the `kind` header at `layer`, or
    -1 (not Ok, or another kind there)."""
    recs, outer = headers(b, chain)
    out = np.full(b.n, -1, np.int64)
    for i in range(b.n):
        if int(recs["status"][i]) == 0:
            have, h = mrm.header_at(chain, recs[i], None if outer is None else outer[i], layer, 0)
            if have == kind:
                out[i] = h
    return out


def own_bytes(b, chain, layer: int, wf) -> np.ndarray:
    """(n, 6 | 16): the bytes wide field `wf` at `layer` holds in each frame
    (zeros where the frame has no such header)."""
    kind, at, nb = rows_model.WIDE[W(int(wf))]
    h = header_offsets(b, chain, layer, kind)
    out = np.zeros((b.n, nb), np.uint8)
    for i in np.nonzero(h >= 0)[0]:
        o = int(b.starts[i]) + int(h[i]) + at
        out[i] = b.arena[o:o + nb]
    return out


def kinds(b, chain):
    """Per frame (l3 kind, l4 kind) names, or None when it does not parse Ok."""
    recs, _ = headers(b, chain)
    l3 = {int(L3Kind.IPV4): "v4", int(L3Kind.IPV6): "v6"}
    l4 = {int(L4Kind.TCP): "tcp", int(L4Kind.UDP): "udp", int(L4Kind.ICMPV4): "icmp4",
          int(L4Kind.ICMPV6): "icmp6"}
    return [None if int(r["status"]) else (l3.get(int(r["l3_kind"])), l4.get(int(r["l4_kind"])))
            for r in recs]


def sum_fields(b, chain):
    """Per frame: the arena offsets of its (L3, L4, outer UDP) checksum fields,
    -1 where it has none."""
    recs, outer = headers(b, chain)
    out = np.full((b.n, 3), -1, np.int64)
    for i in range(b.n):
        r, o = recs[i], int(b.starts[i])
        if int(r["status"]):
            continue
        if int(r["l3_kind"]) == int(L3Kind.IPV4):
            out[i, 0] = o + int(r["l3_off"]) + 10
        at = rows_model._FIELD_AT.get(int(r["l4_kind"]))
        if at is not None:
            out[i, 1] = o + int(r["l4_off"]) + at
        if outer is not None:
            out[i, 2] = o + int(outer[i]["outer_udp_off"]) + 6
    return out


def be16(a, at: int) -> int:
    return (int(a[at]) << 8) | int(a[at + 1])


# ---------------------------------------------------------------------------
# A. Narrow fields: one sweep edit by packet and by row
# ---------------------------------------------------------------------------
SWEEP_ROWS = 5


def _pattern(n: int) -> np.ndarray:
    """A 32-bit word per packet; neighbours differ in many bits."""
    return (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)


def _as(v, wide: bool) -> np.ndarray:
    return (v & np.uint64(0xFFFFFFFF)).astype(np.uint32) if wide else \
        (v & np.uint64(0xFFFF)).astype(np.uint16)


def packet_operand(field, value: int, n: int) -> np.ndarray:
    """The sweep value XORed with a per-packet pattern, in the source that does
    not match the field's width: U16 for fields wider than 16 bits (zero
    extension), U32 for the others (masking; ADD / SUB wrap modulo 2^width)."""
    return _as(np.uint64(value) ^ _pattern(n), sc.FIELD_BITS[Field(field)] <= 16)


def row_table(field, value: int) -> np.ndarray:
    """SWEEP_ROWS rows in the other source: U32 for fields wider than 16 bits,
    U16 for the others."""
    return _as(np.uint64(value) ^ _pattern(SWEEP_ROWS + 3)[3:], sc.FIELD_BITS[Field(field)] > 16)


def sweep_rows(n: int) -> np.ndarray:
    """d_row cycling 0..4; every seventh packet guarded (INGOT_ROW_NONE and
    n_rows in turn)."""
    rows = (np.arange(n) % SWEEP_ROWS).astype(np.uint32)
    rows[6::14] = ROW_NONE
    rows[13::14] = SWEEP_ROWS
    return rows


def sweep_forms(chain, b, e, whats):
    """Sweep edit `e` (layer, field, op, value, index) -> its BY_PACKET and
    BY_ROW groups."""
    layer, field, op, value, index = e
    name = sc.tag(chain, "indexed", e, "*")
    return (Group(name + " by packet", b, chain,
                  [(layer, field, op, packet_operand(field, value, b.n), index)], None, 0, whats),
            Group(name + " by row", b, chain,
                  [(layer, field, op, by_row(row_table(field, value)), index)], sweep_rows(b.n),
                  SWEEP_ROWS, whats))


# ---------------------------------------------------------------------------
# B. Wide fields
# ---------------------------------------------------------------------------
WIDE_AT = {MACD: 8, MACS: 21, V6S: 16, V6D: 3}  # where a 32-B table row holds each field
N_ROWS = 11


def col(t, wf, at=None):
    at = WIDE_AT[wf] if at is None else at
    return t[:, at:at + WIDTH[wf]]


def spread_rows(n: int, n_rows: int = N_ROWS, guarded: bool = True) -> np.ndarray:
    rows = ((np.arange(n) * 3 + 1) % n_rows).astype(np.uint32)
    if guarded:
        rows[5::9] = ROW_NONE
        rows[7::13] = n_rows
    return rows


@lru_cache(maxsize=None)
def strided_with_lens(chain):
    """batch(chain, "strided") with a length array (every slot full)."""
    b = sc.batch(chain, "strided")
    return b._replace(lens=b.lengths.astype(np.uint16))


def wide_layer_groups(chain):
    """3. every wide field at every layer of the chain, by packet and by row,
    under every `what`; the indexed batch and the slots with and without a
    length array."""
    for lname, b in (("indexed", sc.batch(chain, "indexed")),
                     ("strided", sc.batch(chain, "strided")),
                     ("strided+lens", strided_with_lens(chain))):
        t, r = cases.nat_table(b.n, 41), cases.nat_table(N_ROWS, 42)
        rows = spread_rows(b.n)
        for wf in W:
            for layer in sorted({l for l, _ in sc.LAYERS[chain]}):
                name = f"{Chain(chain).name} {lname} L{layer} {wf.name}"
                yield Group(name + " by packet", b, chain, [(layer, wf, SET, col(t, wf))], None, 0,
                            all_whats(chain))
                yield Group(name + " by row", b, chain, [(layer, wf, SET, by_row(col(r, wf)))],
                            rows, N_ROWS, all_whats(chain))


def holds(chain, layer: int, wf) -> bool:
    return layer in WIDE_LAYERS[chain][wf]


def window_groups(chain, b, restore_only: bool = False):
    """4. lists over one batch_at(chain, mis) batch (or, restore_only, any
    batch): addresses set once, set twice (by packet, then by row from another
    table), set and restored from the frames' own bytes, and both MACs.
    -> [(group, whether the call must leave every byte as it was)]."""
    t, t2, r = cases.nat_table(b.n, 43), cases.nat_table(b.n, 44), cases.nat_table(N_ROWS, 45)
    rows = spread_rows(b.n, guarded=False)
    whats = (0, full(chain))
    out = []

    def add(name, edits, rw=None, same=False):
        out.append((Group(f"{Chain(chain).name} {name}", b, chain, edits, rw,
                          N_ROWS if rw is not None else 0, whats), same))

    for layer in WIDE_LAYERS[chain][V6S]:
        for wf in (V6S, V6D):
            if not restore_only:
                add(f"L{layer} {wf.name} once", [(layer, wf, SET, col(t, wf))])
                add(f"L{layer} {wf.name} twice",
                    [(layer, wf, SET, col(t, wf)), (layer, wf, SET, by_row(col(r, wf)))], rows)
            add(f"L{layer} {wf.name} restored",
                [(layer, wf, SET, col(t2, wf)), (layer, wf, SET, own_bytes(b, chain, layer, wf))],
                same=True)
    for layer in WIDE_LAYERS[chain][MACD]:
        if not restore_only:
            add(f"L{layer} both MACs", [(layer, MACD, SET, col(t, MACD)),
                                        (layer, MACS, SET, by_row(col(r, MACS)))], rows)
        add(f"L{layer} both MACs restored",
            [(layer, MACD, SET, col(t2, MACD)), (layer, MACS, SET, col(t2, MACS)),
             (layer, MACS, SET, own_bytes(b, chain, layer, MACS)),
             (layer, MACD, SET, own_bytes(b, chain, layer, MACD))], same=True)
    return out


def window_ends(chain, mis: int):
    """Where the staged window of batch_at(chain, mis)'s frames ends, as
    {(field, layer): the set of byte positions 1..15 inside that address}.  An
    indexed frame's window starts at the 16-B block its first byte lies in, so
    it holds the frame's first WINDOW - mis bytes."""
    b = sc.batch_at(chain, mis)
    assert (b.off % 16 == mis).all()
    end = WINDOW[chain] - mis
    out = {}
    for layer in WIDE_LAYERS[chain][V6S]:
        h = header_offsets(b, chain, layer, "V6")
        for wf in (V6S, V6D):
            at = rows_model.WIDE[wf][1]
            pos = {end - (int(x) + at) for x in h[h >= 0]}
            out[(wf, layer)] = {p for p in pos if 1 <= p <= 15}
    return out


@lru_cache(maxsize=None)
def batch_65(chain):
    frames = sc.source_frames(chain)
    return sc.batch_of((frames * 2)[:65], chain)


def pieces64_groups(chain):
    """5. sixteen edits = 64 pieces: V6_SOURCE and V6_DESTINATION in turn, by
    packet and by row in turn, each from its own column of a 256-B-row table;
    then the same with rows of all 0x00 and all 0xff in turn."""
    b = batch_65(chain)
    assert b.n == 65
    rng = np.random.default_rng(46)
    rows = spread_rows(b.n)
    tables = {"random": (rng.integers(0, 256, (b.n, 256), dtype=np.uint8),
                         rng.integers(0, 256, (N_ROWS, 256), dtype=np.uint8))}
    flip = [np.repeat(((np.arange(k)[:, None] + np.arange(16)[None, :] // 2) % 2 * 0xFF)
                      .astype(np.uint8), 16, axis=1) for k in (b.n, N_ROWS)]
    tables["00 / ff"] = tuple(flip)
    for layer in WIDE_LAYERS[chain][V6S]:
        for tname, (t, r) in tables.items():
            edits = []
            for k in range(16):
                src = r if k % 4 >= 2 else t  # packet, packet, row, row: both for each field
                operand = src[:, 16 * k:16 * k + 16]
                edits.append((layer, V6D if k % 2 else V6S, SET,
                              by_row(operand) if src is r else operand))
            yield Group(f"{Chain(chain).name} L{layer} 64 pieces {tname}", b, chain, edits, rows,
                        N_ROWS, (full(chain),))


# ---------------------------------------------------------------------------
# C. Checksum value edges of the new covered ranges
# ---------------------------------------------------------------------------
def own_u32(b, chain, layer: int, field) -> np.ndarray:
    """(n,) uint32: the value narrow 32-bit `field` (V4_SOURCE / _DESTINATION)
    holds in each frame, 0 where the frame has no IPv4 header at `layer`."""
    at = {Field.V4_SOURCE: 12, Field.V4_DESTINATION: 16}[Field(field)]
    h = header_offsets(b, chain, layer, "V4")
    out = np.zeros(b.n, np.uint32)
    for i in np.nonzero(h >= 0)[0]:
        o = int(b.starts[i]) + int(h[i]) + at
        out[i] = int.from_bytes(b.arena[o:o + 4].tobytes(), "big")
    return out


def _words(t, old: int, new: int) -> np.ndarray:
    """`t` (n, 16) with every aligned 16-bit word `old` replaced by `new`."""
    w = t.reshape(len(t), -1, 2).copy()
    hit = (w[:, :, 0] == (old >> 8)) & (w[:, :, 1] == (old & 0xFF))
    w[hit] = (new >> 8, new & 0xFF)
    return w.reshape(t.shape)


def _zero_words(arena, starts, lengths, chain):
    """prepare(): 16-bit words 2 and 5 of the tunnel frames' outer and inner
    IPv6 addresses are 0 (the generated addresses hold no such word), then
    csum_sweep_cases' edge sums."""
    recs = oracle.parse_batch(arena, starts, lengths, chain)
    for i in np.nonzero(recs["status"] == 0)[0]:
        inner_v6 = int(recs["l3_kind"][i]) == int(L3Kind.IPV6)
        at = [14] + ([int(recs["l3_off"][i])] if inner_v6 else [])
        for h in at:
            for w in (8 + 4, 8 + 10, 24 + 4, 24 + 10):
                o = int(starts[i]) + h + w
                arena[o:o + 2] = 0
    sc._edge_sums(arena, starts, lengths, chain)


@lru_cache(maxsize=None)
def edge_batch(chain):
    """batch(chain, "indexed", prepared) in both representations of a zero sum
    -> (batch, IPv4 fields 0x0000, IPv4 fields 0xffff, UDP fields 0xffff)."""
    if chain == TUN:
        return sc.other_repr(sc.batch_of(sc.source_frames(TUN), TUN, _zero_words), chain)
    return sc.other_repr(sc.batch(chain, "indexed", True), chain)


def delta_zero_groups(chain):
    """6. edits whose covered words change by 0 mod 0xffff: every sum field
    keeps its bytes.  -> [(way, group)]; the ways: "same", "permuted", "swapped",
    "0000 to ffff", "ffff to 0000"."""
    b = edge_batch(chain)[0]
    l3 = sc.L3_LAYER[chain]
    ident = np.arange(b.n, dtype=np.uint32)  # BY_ROW with every packet on its own row
    whats = (full(chain),)
    S, D = Field.V4_SOURCE, Field.V4_DESTINATION
    v6 = {(l, wf): own_bytes(b, chain, l, wf) for l in WIDE_LAYERS[chain][V6S] for wf in (V6S, V6D)}
    v4 = {f: own_u32(b, chain, l3, f) for f in (S, D)}
    mac = {(l, wf): own_bytes(b, chain, l, wf) for l in WIDE_LAYERS[chain][MACD][1:]
           for wf in (MACD, MACS)}

    def lists(f6, f4, fm):
        e = []
        for (l, wf), t in v6.items():
            new = f6(l, wf, t)
            e.append((l, wf, SET, by_row(new) if wf == V6D else new))
        for f, t in v4.items():
            new = f4(f, t)
            e.append((l3, f, SET, by_row(new) if f == D else new))
        for (l, wf), t in mac.items():
            e.append((l, wf, SET, fm(l, wf, t)))
        return e

    def rot(x):
        return ((x << np.uint32(16)) | (x >> np.uint32(16))).astype(np.uint32)

    other6 = {V6S: V6D, V6D: V6S}
    otherm = {MACS: MACD, MACD: MACS}
    out = [
        ("same", lists(lambda l, wf, t: t, lambda f, t: t, lambda l, wf, t: t)),
        ("permuted", lists(lambda l, wf, t: np.roll(t, 2, axis=1), lambda f, t: rot(t),
                           lambda l, wf, t: np.roll(t, 2, axis=1))),
        ("swapped", lists(lambda l, wf, t: v6[(l, other6[wf])], lambda f, t: v4[D if f == S else S],
                          lambda l, wf, t: mac[(l, otherm[wf])])),
    ]
    ff = [(l, wf, SET, _words(t, 0, 0xFFFF)) for (l, wf), t in v6.items()]
    out = [(way, Group(f"{Chain(chain).name} delta 0: {way}", b, chain, e, ident, b.n, whats))
           for way, e in out + [("0000 to ffff", ff)]]
    # ... and back, on the frames the definition makes of that
    b_ff = b._replace(arena=expected(out[-1][1])[0][0])
    b_ff.arena.setflags(write=False)
    back = [(l, wf, SET, t) for (l, wf), t in v6.items()]
    out.append(("ffff to 0000", Group(f"{Chain(chain).name} delta 0: ffff to 0000", b_ff, chain,
                                      back, ident, b.n, whats)))
    return out


def fill_all(b, chain, arena):
    """Every sum of every frame from scratch, in place (inner first, then the
    tunnel's outer UDP sum under a UdpParser parse)."""
    recs = oracle.parse_batch(arena, b.starts, b.lengths, sc._fill_chain(chain))
    model.fill(arena, b.starts, b.lengths, recs)
    if chain == TUN:
        model.fill(arena, b.starts, b.lengths,
                   oracle.parse_batch(arena, b.starts, b.lengths, Chain.UdpParser), what=CSUM_L4)


# what the solved word is for -> (its offset v from the value that makes the
# covered words add up to 0xffff, the field's bytes for UDP, for TCP / ICMPv6)
TARGETS = {"computed 0": (0, b"\xff\xff", b"\x00\x00"), "0x0001": (-1, b"\x00\x01", b"\x00\x01"),
           "0xfffe": (1, b"\xff\xfe", b"\xff\xfe")}


def solved_table(b, chain, layer: int, wf, word: int, which: int, v: int, seed: int):
    """-> (an (n, width) table of seeded bytes whose 16-bit word `word` is
    solved per packet so that the words sum `which` (1: L4, 2: the tunnel's
    outer UDP) covers add up to 0xffff + v after `wf` at `layer` is SET from
    it; the packets solved).  The sum is linear in the word: with the word at 0
    the from-scratch field is c, so the covered words add up to ~c, and the
    word c + v makes them 0xffff + v."""
    rng = np.random.default_rng([seed, int(wf), layer, word, which, v + 1])
    t = rng.integers(0, 256, (b.n, WIDTH[wf]), dtype=np.uint8)
    t[:, 2 * word:2 * word + 2] = 0
    plain = expected(Group("", b, chain, [(layer, wf, SET, t)], None, 0, (0,)))[0][0]
    fill_all(b, chain, plain)
    fields = sum_fields(b, chain)[:, which]
    have = header_offsets(b, chain, layer, rows_model.WIDE[wf][0]) >= 0
    solved = np.zeros(b.n, bool)
    for i in np.nonzero(have & b.keep & (fields >= 0))[0]:
        c = be16(plain, int(fields[i]))
        if 1 <= c <= 0xFFFD:
            w = c + v
            t[i, 2 * word], t[i, 2 * word + 1] = w >> 8, w & 0xFF
            solved[i] = True
    return t, solved


def _outer_zero(arena, starts, lengths, chain):
    """prepare(): the outer UDP source port solved so that the outer sum is a
    computed 0 (field 0xffff) once every sum is filled."""
    model.fill(arena, starts, lengths, oracle.parse_batch(arena, starts, lengths, TUN))
    o_recs = oracle.parse_batch(arena, starts, lengths, Chain.UdpParser)
    ports = [int(starts[i]) + int(o_recs["l4_off"][i]) for i in range(len(starts))]
    for p in ports:
        arena[p:p + 2] = 0
    scratch = arena.copy()
    model.fill(scratch, starts, lengths, o_recs, what=CSUM_L4)
    for p in ports:
        arena[p:p + 2] = scratch[p + 6:p + 8]


@lru_cache(maxsize=None)
def tunnel_outer_zero_batch():
    return sc.batch_of(sc.source_frames(TUN)[:60], TUN, _outer_zero)


def scatter(t, seed: int):
    """A by-packet table as a by-row one: -> (rows, the table with packet i's
    row at rows[i])."""
    perm = np.random.default_rng(seed).permutation(len(t)).astype(np.uint32)
    r = np.empty_like(t)
    r[perm] = t
    return perm, r


def solved_groups(chain):
    """7. -> [(group, which sum, {target name: the packets solved for it})]:
    packet i is solved for target (i + i // 60) % 3; by packet and by row."""
    l3 = sc.L3_LAYER[chain]
    plans = [("L4 through the source", sc.batch(chain, "indexed"), l3, V6S, 5, 1)]
    if chain == TUN:
        plans += [("outer through an outer address", sc.batch(chain, "indexed"), 1, V6D, 2, 2),
                  ("outer through an inner MAC", sc.batch(chain, "indexed"), 4, MACS, 1, 2),
                  ("inner L4 under an outer sum of 0", tunnel_outer_zero_batch(), 5, V6S, 6, 1)]
    out = []
    for k, (name, b, layer, wf, word, which) in enumerate(plans):
        t = np.zeros((b.n, WIDTH[wf]), np.uint8)
        hit = {}
        for j, (target, (v, _, _)) in enumerate(TARGETS.items()):
            tj, solved = solved_table(b, chain, layer, wf, word, which, v, 50 + k)
            mine = (np.arange(b.n) + np.arange(b.n) // 60) % 3 == j
            t[mine] = tj[mine]
            hit[target] = np.nonzero(mine & solved)[0]
        rows, r = scatter(t, 60 + k)
        whats = (full(chain),)
        title = f"{Chain(chain).name} solved: {name}"
        out.append((Group(title + " by packet", b, chain, [(layer, wf, SET, t)], None, 0, whats),
                    which, hit))
        out.append((Group(title + " by row", b, chain, [(layer, wf, SET, by_row(r))], rows, b.n,
                          whats), which, hit))
    return out


@lru_cache(maxsize=None)
def still_batch(chain):
    """The chain's frames twice; in the second copy every UDP checksum field
    (the tunnel: the outer one) is 0, "no checksum".  -> (batch, those frames)."""
    frames = sc.source_frames(chain)[:60] if chain == TUN else sc._frames_for(chain)
    b = sc.batch_of(frames * 2, chain)
    arena = b.arena.copy()
    fields = sum_fields(b, chain)
    kind = kinds(b, chain)
    zeroed = []
    for i in range(len(frames), b.n):
        at = int(fields[i, 2 if chain == TUN else 1])
        if at >= 0 and (chain == TUN or kind[i][1] == "udp") and b.keep[i]:
            arena[at:at + 2] = 0
            zeroed.append(i)
    keep = b.keep.copy()
    keep[zeroed] = False
    arena.setflags(write=False)
    return b._replace(arena=arena, keep=keep), np.array(zeroed)


def still_groups(chain):
    """8. per-packet wide and narrow address edits (the tunnel: the outer
    addresses and an inner MAC too) over still_batch."""
    b, _ = still_batch(chain)
    l3 = sc.L3_LAYER[chain]
    t, r = cases.nat_table(b.n, 47), cases.nat_table(N_ROWS, 48)
    rows = spread_rows(b.n, guarded=False)
    edits = [(l3, V6S, SET, col(t, V6S)), (l3, V6D, SET, by_row(col(r, V6D))),
             (l3, Field.V4_SOURCE, SET, cases.col_u32(t, 0)),
             (l3, Field.V4_DESTINATION, SET, by_row(cases.col_u32(r, 4)))]
    if chain == TUN:
        edits += [(1, V6S, SET, by_row(col(r, V6S))), (1, V6D, SET, col(t, V6D)),
                  (4, MACS, SET, col(t, MACS))]
    return [Group(f"{Chain(chain).name} still", b, chain, edits, rows, N_ROWS, all_whats(chain))]


# ---------------------------------------------------------------------------
# D. Tables and rows
# ---------------------------------------------------------------------------
@lru_cache(maxsize=None)
def batch_n(chain, n: int, rot: int = 0):
    """`n` of the chain's frames in turn, from frame `rot`."""
    frames = sc.source_frames(chain)
    frames = frames[rot:] + frames[:rot]
    return sc.batch_of((frames * (n // len(frames) + 1))[:n], chain)


def pitched(rng, n: int, width: int, pitch: int, at: int = 0, dtype=np.uint8) -> np.ndarray:
    """(n, width) `dtype` view, rows `pitch` bytes apart, starting `at` bytes
    into its root array (tests/modify_rows_cases.device_edits uploads the root
    and rebuilds the view: the device sees the same pitch and at mod 4)."""
    isz = np.dtype(dtype).itemsize
    assert pitch % isz == 0 and at % isz == 0 and pitch >= width * isz
    root = rng.integers(0, 256, at + n * pitch, dtype=np.uint8)
    return root[at:].view(dtype).reshape(n, pitch // isz)[:, :width]


BYTE_PITCHES = ("exact", "odd", 32, 4096)  # (pitch 0 is the ABI's name for "exact")


def byte_table_groups():
    """9. MAC and IPv6 tables at device addresses 0..3 mod 4 with rows exactly
    their width, one byte more (the alignment changes from row to row), 32 and
    4096 bytes apart; by packet and by row; n = 129."""
    chain = Chain.GenericUlp
    b = batch_n(chain, 129)
    rows = spread_rows(b.n)
    rng = np.random.default_rng(49)
    for at in range(4):
        for p in BYTE_PITCHES:
            for by in ("packet", "row"):
                edits = []
                for layer, wf in ((0, MACD), (1, V6S), (0, MACS), (1, V6D)):
                    w = WIDTH[wf]
                    t = pitched(rng, b.n if by == "packet" else N_ROWS, w,
                                {"exact": w, "odd": w + 1}.get(p, p), at)
                    edits.append((layer, wf, SET, by_row(t) if by == "row" else t))
                yield Group(f"byte tables at {at} mod 4, pitch {p}, by {by}", b, chain, edits,
                            rows if by == "row" else None, N_ROWS if by == "row" else 0, (3,))


def int_table_groups():
    """10. U16 tables 2 and 6 bytes apart, U32 tables 4 and 12 (pitch 0: the
    device test's raw call); BY_ROW over 37 rows 65,536 bytes apart."""
    chain = Chain.GenericUlp
    b = batch_n(chain, 129)
    rng = np.random.default_rng(50)
    F = Field
    for p16, p32 in ((2, 4), (6, 12)):
        edits = [(2, F.UDP_SOURCE, SET, pitched(rng, b.n, 1, p16, 0, np.uint16)),
                 (2, F.TCP_DESTINATION, EditOp.ADD, pitched(rng, b.n, 1, p16, 2, np.uint16)),
                 (1, F.V4_SOURCE, EditOp.XOR, pitched(rng, b.n, 1, p16, 0, np.uint16)),
                 (1, F.V4_DESTINATION, SET, pitched(rng, b.n, 1, p32, 4, np.uint32)),
                 (2, F.TCP_SEQUENCE, EditOp.SUB, pitched(rng, b.n, 1, p32, 0, np.uint32)),
                 (1, F.V6_HOP_LIMIT, SET, pitched(rng, b.n, 1, p32, 0, np.uint32))]
        yield Group(f"integer tables, pitch {p16} / {p32}", b, chain, edits, None, 0, (3,))
    rows = spread_rows(b.n, 37)
    edits = [(1, F.V4_SOURCE, SET, by_row(pitched(rng, 37, 1, 65536, 0, np.uint32))),
             (2, F.UDP_DESTINATION, SET, by_row(pitched(rng, 37, 1, 65536, 2, np.uint16))),
             (1, V6S, SET, by_row(pitched(rng, 37, 16, 65536, 1)))]
    yield Group("37 rows 65,536 bytes apart", b, chain, edits, rows, 37, (3,))


GUARD_ROWS = 37
BIG_ROWS = 1 << 20


def guard_edits(n: int, n_rows: int, seed: int = 51):
    """A VALUE edit per L3 kind, by-row narrow and wide operands from tables of
    max(n_rows, 1) rows, and a by-packet MAC."""
    rng = np.random.default_rng(seed)
    k = max(n_rows, 1)
    F = Field
    return [(1, F.V4_HOP_LIMIT, EditOp.SUB, 1), (1, F.V6_HOP_LIMIT, EditOp.SUB, 1),
            (1, F.V4_SOURCE, SET, by_row(rng.integers(0, 1 << 32, k, dtype=np.uint64)
                                         .astype(np.uint32))),
            (1, V6S, SET, by_row(rng.integers(0, 256, (k, 16), dtype=np.uint8))),
            (0, MACD, SET, rng.integers(0, 256, (n, 6), dtype=np.uint8))]


def guard_groups():
    """12. -> [(group, the packets the guard must leave alone)] at the tile
    edges n = 1, 63, 64, 65 (and 300 packets over a 2^20-row table)."""
    chain = Chain.GenericUlp
    out = []
    for n in (1, 63, 64, 65):
        b = batch_n(chain, n)
        i = np.arange(n)
        R = GUARD_ROWS
        edge = np.array([0, R - 1, R, 0x7FFFFFFF, 0x80000000, ROW_NONE], np.uint32)
        plans = [("n_rows = 0", np.zeros(n, np.uint32), 0),
                 ("n_rows = 0, rows of every size", edge[(i + 1) % 6], 0),
                 ("n_rows = 1", np.array([0, 1, ROW_NONE], np.uint32)[i % 3], 1),
                 ("the guard's edges", edge[(i + n) % 6], R),
                 ("one row", np.full(n, 5, np.uint32), R)]
        for name, rows, n_rows in plans:
            out.append((Group(f"{name}, n = {n}", b, chain, guard_edits(n, n_rows), rows, n_rows,
                              (3,)), np.nonzero(rows >= n_rows)[0]))
    b = batch_n(chain, 300)
    rows = np.random.default_rng(52).integers(0, BIG_ROWS, b.n).astype(np.uint32)
    rows[:4] = (0, BIG_ROWS - 1, BIG_ROWS, ROW_NONE)
    out.append((Group("2^20 rows, 300 packets", b, chain, guard_edits(b.n, BIG_ROWS), rows,
                      BIG_ROWS, (3,)), np.nonzero(rows >= BIG_ROWS)[0]))
    return out


def far_rows(n: int, seed: int = 53):
    """11. the dense operands of the row-offset test: -> ((n,) uint32, (n, 16)
    uint8); the device test writes row i of each 1 MiB * i into its table."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
            rng.integers(0, 256, (n, 16), dtype=np.uint8))
