"""Deterministic cases for ingot_gpu_emit_packets_rows, shared by
tests/test_emit_rows_sweep_model.py (CPU) and tests/test_emit_rows_sweep.py
(GPU).  TEST INFRASTRUCTURE ONLY.

  A  every narrow field through one set: VALUE, a table by packet and by row
     in the matching and the other integer source, `add` at its wraps, LENGTH
  B  the wide fields at every place of a 254-B block from tables of every
     alignment, 32 pieces, the smallest blocks, sets that overwrite each other
  C  UDP and IPv4 sums landing on 0 / 0xffff and their neighbours through a
     word of a table operand; all-0xff / all-0x00 operands under the longest
     datagram
  D  rows 1 MiB apart past 2^32, the row guard alone, n_rows = 0, one survivor

A Job is one call: a rc.Case (tables as views of uploadable backing arrays)
and the Batch it is emitted over.  The definition of a Job's result is
tests/emit_rows_model.py.  `emulate` is a second way to the same bytes, in
plain Python from the header's wording and the bit places of
tests/modify_read_model.GEOMETRY; it also takes a named fault, so that the CPU
file can show which case would catch a device that made that mistake.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

from ingot_amd import EmitSource, EmitSum, Field, WideField
from ingot_amd import emit as E
from ingot_amd.abi import WIDE_BYTES
from tests import csum_sweep_cases as sc
from tests import emit_csum_cases as cases
from tests import emit_csum_model as emodel
from tests import emit_rows_cases as rc
from tests import emit_rows_model as model
from tests import modify_read_model as mrm

LENGTH, U16, U32, VALUE, BYTES = (EmitSource.LENGTH, EmitSource.U16, EmitSource.U32,
                                  EmitSource.VALUE, EmitSource.BYTES)
ROW_NONE = rc.ROW_NONE

# src / off / lens / dst_off / size: what the call takes (guarded packets'
# descriptors poisoned); rows: None or the row array
Batch = namedtuple("Batch", "src off lens dst_off size rows n_rows")
# pitch: {set index: the device table's pitch} where it is not the view's;
# checks: [(packet, offset in the packet, bytes, note)] a crafted case was built for
Job = namedtuple("Job", "tag case b pitch checks", defaults=({}, ()))


def live(b: Batch) -> np.ndarray:
    return model.emitted(len(b.lens), b.rows, b.n_rows)


def expected(job: Job) -> np.ndarray:
    """The definition's arena."""
    c, b = job.case, job.b
    want = np.full(b.size, 0xA5, np.uint8)
    return model.apply(want, c.hdr, c.host_sets(), c.sums, b.src, b.off, b.lens, b.dst_off,
                       b.rows, b.n_rows)


def held(job: Job, got) -> None:
    """The crafted packets' fields hold the bytes they were built for."""
    for k, at, want, note in job.checks:
        o = int(job.b.dst_off[k]) + at
        assert got[o:o + 2].tobytes() == want, (job.tag, k, note, got[o:o + 2].tobytes().hex())


# ---------------------------------------------------------------------------
# Batches and tables
# ---------------------------------------------------------------------------
def place(lens, hdr_len: int, rng, rows=None, n_rows: int = 0, dmis_of=None) -> Batch:
    """rc.batch with the lengths given and, for the packets of `dmis_of`, the
    destination address mod 16: one packet after another, 0-3 B between them,
    none next to a guarded packet, whose own descriptors are poisoned."""
    lens = np.asarray(lens, np.uint16).copy()
    n = len(lens)
    alive = model.emitted(n, rows, n_rows)
    src, off = cases.random_source(lens, rng)
    dst, o = np.zeros(n, np.uint64), 5
    for k in range(n):
        if not alive[k]:
            continue
        if dmis_of and k in dmis_of:
            o += (dmis_of[k] - o) % 16
        elif (k == 0 or alive[k - 1]) and (k + 1 == n or alive[k + 1]):
            o += int(rng.integers(0, 4))
        dst[k] = o
        o += hdr_len + int(lens[k])
    off = off.copy()
    off[~alive], lens[~alive], dst[~alive] = 1 << 40, 65535, 1 << 41
    return Batch(src, off, lens, dst, o + 64, rows, n_rows)


def table(backing: dict, key: str, values, lead: int = 0, pitch: int = 0) -> rc.View:
    """`values` ((rows,) u16 / u32 or (rows, width) u8) as a table `lead`
    bytes into a new backing array `key`, rows `pitch` (default: width) apart,
    0x5A between and around them."""
    v = np.ascontiguousarray(values)
    raw = v.view(np.uint8).reshape(len(v), -1)
    rows, width = raw.shape
    pitch = pitch or width
    buf = np.full(lead + rows * pitch + 8, 0x5A, np.uint8)
    np.lib.stride_tricks.as_strided(buf[lead:], (rows, width), (pitch, 1))[:] = raw
    backing[key] = buf
    return rc.View(key, lead, width, pitch, rows, v.dtype)


N_SWEEP, SWEEP_ROWS = 65, 5
SWEEP_GUARDED = tuple(range(6, N_SWEEP, 7))


@lru_cache(maxsize=None)
def sweep_batch(hdr_len: int, with_rows: bool) -> Batch:
    """65 packets (two prologue waves, the second with one live lane), the
    lengths of rc.lengths, the first 32 at destination addresses 5k mod 16 so
    that every misalignment is an emitted packet's.  with_rows: 5 rows, every
    seventh packet guarded, the last row used."""
    rng = np.random.default_rng([41, hdr_len, int(with_rows)])
    rows = rc.row_indices(N_SWEEP, SWEEP_ROWS, rng, guarded=SWEEP_GUARDED) if with_rows else None
    alive = model.emitted(N_SWEEP, rows, SWEEP_ROWS)
    b = place(rc.lengths(N_SWEEP, rng, alive), hdr_len, rng, rows, SWEEP_ROWS,
              {k: (5 * k) % 16 for k in range(32)})
    assert {int(d) % 16 for d in b.dst_off[alive]} == set(range(16))
    assert rows is None or (SWEEP_ROWS - 1) in rows.tolist()
    assert 65535 in b.lens[alive].tolist()
    return b


# ---------------------------------------------------------------------------
# A. Narrow fields
# ---------------------------------------------------------------------------
_PARTS = (("ETH", E.ethernet(cases.MAC_D, cases.MAC_S, 0x8100)), ("VLAN", E.vlan(0x123, 0x0800)),
          ("V4", E.ipv4(cases.V4_S, cases.V4_D, 6)), ("V6", E.ipv6(cases.V6_S, cases.V6_D, 6)),
          ("TCP", E.tcp(1, 2)), ("UDP", E.udp(3, 4)), ("ICMP", E.icmp(8, 0)),
          ("GENEVE", E.geneve(0x123456)))
KIND_AT, _o = {}, 0
for _k, _h in _PARTS:
    KIND_AT[_k] = _o
    _o += len(_h)
BLOCK_LEN = _o  # one header of every kind back to back
assert BLOCK_LEN == 14 + 4 + 20 + 40 + 20 + 8 + 8 + 8
FILLS = (0x00, 0xFF)
FORMS = ("value", "by packet", "by row", "add", "length")


def field_at(field) -> int:
    return KIND_AT[sc.kind_of(field)]


def sweep_values(field):
    """1, all ones, the top bit alone, a word wider than the field, one seeded
    random word."""
    bits = sc.FIELD_BITS[Field(field)]
    rng = np.random.default_rng([2025, int(field)])
    return (1, (1 << bits) - 1, 1 << (bits - 1), 0xFFFFFFFF, int(rng.integers(0, 1 << 32)))


def sources_for(field):
    """(the integer source that does not match the field's width, the one that does)"""
    return (U32, U16) if sc.FIELD_BITS[Field(field)] <= 16 else (U16, U32)


def _cycled(vals, rows: int, source) -> np.ndarray:
    """Rows cycle through `vals`; from the second turn on, XOR a pattern of
    the packet's turn."""
    t = np.array([vals[i % len(vals)] ^ ((i // len(vals)) * 0x9E3779B1 & 0xFFFFFFFF)
                  for i in range(rows)], np.uint64)
    return t.astype(np.uint32) if source == U32 else (t & 0xFFFF).astype(np.uint16)


# add: 0, 1, -1 and the value that takes a row of the table exactly to 2^16 / 2^32
ADD_ROWS = {U16: (0, 0xFFFF, 0x8001, 1), U32: (0, 0xFFFFFFFF, 0x80000001, 1)}
ADDS = {U16: (0, 1, -1, 0x7FFF), U32: (0, 1, -1, 0x7FFFFFFF)}


def narrow_jobs(field, form: str):
    """The Jobs of one (field, form): one set on the block of every header
    kind, prefilled with 0x00 and with 0xFF, no sums."""
    field = Field(field)
    at = field_at(field)
    name = field.name

    def job(tag, fill, source, add, tab=None, by_row=False):
        backing = {}
        s = (at, field, source, add)
        if tab is not None:
            view = table(backing, "t", tab)
            s += ((("row", view) if by_row else view),)
        case = rc.Case(bytes([fill]) * BLOCK_LEN, [s], None, backing)
        return Job(f"{name} {form} fill {fill:#04x} {tag}", case, sweep_batch(BLOCK_LEN, by_row))

    for fill in FILLS:
        if form == "value":
            for v in sweep_values(field):
                yield job(f"{v:#x}", fill, VALUE, v)
        elif form in ("by packet", "by row"):
            rows = SWEEP_ROWS if form == "by row" else N_SWEEP
            for source in sources_for(field):
                yield job(source.name, fill, source, 0,
                          _cycled(sweep_values(field), rows, source), form == "by row")
        elif form == "add":
            for source in (U16, U32):
                rows = ADD_ROWS[source] + (sweep_values(field)[4],)
                for add in ADDS[source]:
                    yield job(f"{source.name} {add:+#x}", fill, source, add,
                              _cycled(rows, N_SWEEP, source))
        elif form == "length":
            for add in (0, -at):
                yield job(f"{add:+d}", fill, LENGTH, add)
        else:
            raise KeyError(form)


# ---------------------------------------------------------------------------
# B. Wide fields and piece limits
# ---------------------------------------------------------------------------
WIDE = tuple(WideField)
BIG = 254
# table layouts -> (first byte of the table in its 4-B aligned backing array,
# pitch of a MAC table, pitch of an address table)
LAYOUTS = {"odd": (1, 6, 16), "2-aligned": (2, 6, 16), "4-aligned": (0, 8, 16),
           "pitch": (0, 7, 17)}


def layout_of(name: str, width: int):
    lead, mac, v6 = LAYOUTS[name]
    return lead, (mac if width == 6 else v6)


def piece_kinds(lead: int, pitch: int, width: int):
    """The wire-order pieces of a wide set whose table starts `lead` bytes
    into a 4-B aligned array: {(piece bytes, one aligned load)}, by the
    header's rule (a piece is loaded whole when its address and the pitch are
    multiples of its size)."""
    return {(min(4, width - b), ((lead + b) | pitch) % min(4, width - b) == 0)
            for b in range(0, width, 4)}


def _pattern_block(n: int) -> bytes:
    return bytes((7 * i + 3) & 0xFF for i in range(n))


def _rows_of(rng, rows: int, width: int) -> np.ndarray:
    return rng.integers(0, 256, (rows, width), dtype=np.uint8)


def wide_ats(wf) -> list:
    """Every 13th place of the field in a 254-B block (13 is odd: 16 steps
    visit every at mod 16), and the last one, ending at the block's end."""
    last = BIG - model.WIDE_AT[wf] - WIDE_BYTES[wf]
    return sorted(set(range(0, last + 1, 13)) | {last})


def wide_at_jobs(wf):
    """`wf` at each of wide_ats, eight sets a call, by packet and by row in
    turn, from tables of each layout."""
    wf = WideField(wf)
    width = WIDE_BYTES[wf]
    b = sweep_batch(BIG, True)
    ats = wide_ats(wf)
    assert {a % 16 for a in ats} == set(range(16))
    for lay in LAYOUTS:
        lead, pitch = layout_of(lay, width)
        for c0 in range(0, len(ats), model.MAX_SETS):
            rng = np.random.default_rng([43, int(wf), c0, lead, pitch])
            backing = {}
            tp = table(backing, "tp", _rows_of(rng, N_SWEEP, width), lead, pitch)
            tr = table(backing, "tr", _rows_of(rng, SWEEP_ROWS, width), lead, pitch)
            sets = [(a, wf, BYTES, 0, tp if k % 2 == 0 else ("row", tr))
                    for k, a in enumerate(ats[c0:c0 + model.MAX_SETS])]
            yield Job(f"{wf.name} {lay} at {ats[c0]}..", rc.Case(_pattern_block(BIG), sets, None,
                                                                 backing), b)


N_PIECES, PIECES_ROWS = 130, 7
# V6_SOURCE at 30 is the destination address's place; the rest lie in the options
V6_PLACES = ((14, WideField.V6_SOURCE), (30, WideField.V6_SOURCE), (50, WideField.V6_DESTINATION),
             (85, WideField.V6_SOURCE), (90, WideField.V6_DESTINATION), (131, WideField.V6_SOURCE),
             (150, WideField.V6_DESTINATION), (230, WideField.V6_SOURCE))
MAC_PLACES = ((0, WideField.ETH_DESTINATION), (6, WideField.ETH_DESTINATION),
              (71, WideField.ETH_DESTINATION), (97, WideField.ETH_DESTINATION),
              (110, WideField.ETH_SOURCE), (159, WideField.ETH_DESTINATION),
              (200, WideField.ETH_SOURCE), (242, WideField.ETH_SOURCE))


def pieces_jobs():
    """Eight address sets (32 pieces) and eight MAC sets (16 pieces) on the
    254-B Geneve block, by packet and by row in turn, one table layout after
    the other, with the block's UDP sum and without."""
    for what, places in (("v6", V6_PLACES), ("mac", MAC_PLACES)):
        assert len({a for a, _ in places}) == model.MAX_SETS
        rng = np.random.default_rng([47, len(what)])
        hdr, _, sums = sc.big_stack("geneve_v6_opts", 1, rng)
        assert len(hdr) == BIG
        rows = rc.row_indices(N_PIECES, PIECES_ROWS, rng, guarded=(0, 63, 64, 65, N_PIECES - 1))
        b = Batch(*rc.batch(N_PIECES, BIG, rng, rows, PIECES_ROWS), rows, PIECES_ROWS)
        backing, sets = {}, []
        for k, (a, wf) in enumerate(places):
            width = WIDE_BYTES[wf]
            lead, pitch = layout_of(list(LAYOUTS)[k % 4], width)
            by_row = k % 2 == 1
            t = table(backing, f"t{k}", _rows_of(rng, PIECES_ROWS if by_row else N_PIECES, width),
                      lead, pitch)
            sets.append((a, wf, BYTES, 0, ("row", t) if by_row else t))
        for sm in (sums, None):
            yield Job(f"8 {what} sets, sums {sm}", rc.Case(hdr, sets, sm, backing), b)


SHORT = (0, 1, 2, 15, 16, 17)


def small_block_jobs():
    """A 12-B block whose last six bytes are ETH_SOURCE (by packet, an odd
    table) and a 14-B Ethernet header with both MACs by row and the ethertype
    by packet; payloads of 0, 1, 2, 15, 16 and 17 B at every destination
    misalignment: whole packets inside one 16-B chunk."""
    eth = E.ethernet(cases.MAC_D, cases.MAC_S, 0x86DD)
    lens = [SHORT[k % 6] for k in range(96)]
    dmis = {k: k // 6 for k in range(96)}
    rng = np.random.default_rng(53)
    backing = {}
    t = table(backing, "t", _rows_of(rng, 96, 6), 1, 6)
    yield Job("12-B block", rc.Case(eth[:12], [(0, WideField.ETH_SOURCE, BYTES, 0, t)], None,
                                    backing), place(lens, 12, rng, dmis_of=dmis))
    rows = rng.integers(0, 5, 96, dtype=np.uint64).astype(np.uint32)
    rows[95] = 4
    backing = {}
    sets = [(0, WideField.ETH_DESTINATION, BYTES, 0,
             ("row", table(backing, "d", _rows_of(rng, 5, 6), 2, 6))),
            (0, WideField.ETH_SOURCE, BYTES, 0,
             ("row", table(backing, "s", _rows_of(rng, 5, 6), 0, 8))),
            (0, Field.ETH_ETHERTYPE, U16, 0,
             table(backing, "e", rng.integers(0, 1 << 16, 96, dtype=np.uint64).astype(np.uint16)))]
    yield Job("14-B block", rc.Case(eth, sets, None, backing),
              place(lens, 14, rng, rows, 5, dmis))


ORDERS = ("wide narrow wide", "wide wide narrow", "narrow wide wide")


def restore_jobs():
    """On v6_udp with its sum: the IPv6 source and the Ethernet destination
    set from one table, a narrow set inside each (a u16 at bytes 30..31, the
    24-bit field at bytes 4..6), and the wide set again from another table, in
    the three orders that differ.  -> (Job, the wide table that must show,
    whether the narrow sets show)."""
    n, n_rows = 130, 7
    for order in ORDERS:
        rng = np.random.default_rng(59)
        base = rc.stack("v6_udp", "dense", n, n_rows, rng)
        rows = rc.row_indices(n, n_rows, rng, guarded=(1, 64, n - 1))
        b = Batch(*rc.batch(n, len(base.hdr), rng, rows, n_rows), rows, n_rows)
        backing = {}
        u16 = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
        u32 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        w1 = [(14, WideField.V6_SOURCE, BYTES, 0, table(backing, "a1", _rows_of(rng, n, 16), 1)),
              (0, WideField.ETH_DESTINATION, BYTES, 0,
               ("row", table(backing, "m1", _rows_of(rng, n_rows, 6))))]
        w2 = [(14, WideField.V6_SOURCE, BYTES, 0,
               ("row", table(backing, "a2", _rows_of(rng, n_rows, 16)))),
              (0, WideField.ETH_DESTINATION, BYTES, 0, table(backing, "m2", _rows_of(rng, n, 6), 2))]
        nar = [(30, Field.UDP_SOURCE, U16, 3, table(backing, "u16", u16)),
               (0, Field.GENEVE_VNI, U32, 0, table(backing, "u32", u32))]
        parts = {"wide": iter((w1, w2)), "narrow": iter((nar,))}
        sets = base.sets[:2] + [s for word in order.split() for s in next(parts[word])]
        assert len(sets) == model.MAX_SETS
        yield (Job(order, rc.Case(base.hdr, sets, base.sums, backing), b),
               order.endswith("narrow"))


# ---------------------------------------------------------------------------
# C. Sums at their edges, operands from tables
# ---------------------------------------------------------------------------
N_ROWS_C = 16
# stack -> (what is solved, the table's backing key, by row)
SOLVED = (("opte", "udp", "v6d", True), ("v6_udp", "udp", "v6s", False),
          ("geneve_v4", "udp", "v4s", True), ("geneve_v4", "v4", "v4s", True))
WANT = {"udp": {0: b"\xff\xff", -1: b"\x00\x01", 1: b"\xff\xfe"},
        "v4": {0: b"\x00\x00", -1: b"\x00\x01", 1: b"\xff\xfe"}}
BIG_AT = 300  # the packet whose segment is longer than any datagram


def _be16(a, at):
    return (int(a[at]) << 8) | int(a[at + 1])


def solved_job(name: str, what: str, key: str, by_row: bool, rot: int) -> Job:
    """600 packets of stack `name`; for the packets at sc.CRAFTED_AT one 16-bit
    word of table `key` (word 5 of the IPv6 address; the low half of V4_SOURCE)
    is solved so that the words of the sum named `what` add up to 0xffff,
    0xfffe and 0x10000: place j takes the value (j + rot) mod 3 of those.
    By row, every crafted packet has a row of its own.  The crafted packets
    start at both parities, with the field inside one 16-B chunk and across
    two.  Packet 300 is 65,535 B long: no datagram, its UDP field is left."""
    rng = np.random.default_rng([61, [s[:2] for s in SOLVED].index((name, what)), rot])
    n = sc.N_CRAFTED
    case = rc.stack(name, "dense", n, N_ROWS_C, rng)
    u = next(s for s in case.sums if int(s[0]) == int(EmitSum.UDP))
    fat = u[1] + 6 if what == "udp" else next(s for s in case.sums
                                              if int(s[0]) == int(EmitSum.IPV4))[1] + 10
    rows = None
    if by_row:
        rows = rng.integers(0, 10, n, dtype=np.uint64).astype(np.uint32)
        rows[100], rows[101] = N_ROWS_C, ROW_NONE
        for j, k in enumerate(sc.CRAFTED_AT):
            rows[k] = 10 + j
    if name == "v6_udp":  # a by-packet set on the field itself: the sum overrides it
        t = table(case.backing, "csum", rng.integers(0, 1 << 16, n, dtype=np.uint64)
                  .astype(np.uint16))
        case.sets.append((u[1], Field.UDP_CHECKSUM, U16, 0, t))
    lens = rng.integers(0, 200, n).astype(np.uint16)
    lens[BIG_AT] = 65535
    across = (15 - fat) % 16
    dmis = dict(zip(sc.CRAFTED_AT, (0, 1, across, 6, across, 15)))
    for j, k in enumerate(sc.CRAFTED_AT):
        lens[k] = sc.ZERO_LENGTHS[(j + rot) % 4]
    b = place(lens, len(case.hdr), rng, rows, N_ROWS_C, dmis)
    view = next(s[4] for s in case.sets if len(s) > 4 and
                (s[4][1] if isinstance(s[4], tuple) else s[4]).name == key)
    view = view[1] if isinstance(view, tuple) else view
    add = next(s[3] for s in case.sets if s[1] == Field.V4_SOURCE) if key == "v4s" else 0
    buf = case.backing[key]

    def put(k, word):
        r = int(rows[k]) if by_row else k
        o = view.first + r * view.pitch
        if key == "v4s":  # the set's value is table + add: high half 0x0a63, low half `word`
            buf[o:o + 4] = np.frombuffer(int(((0x0A63 << 16 | word) - add) & 0xFFFFFFFF)
                                         .to_bytes(4, "little"), np.uint8)
        else:
            buf[o + 10], buf[o + 11] = word >> 8, word & 0xFF

    checks = []
    for j, k in enumerate(sc.CRAFTED_AT):
        v = (0, -1, 1)[(j + rot) % 3]
        put(k, 0)
        o, ln = int(b.off[k]), int(b.lens[k])
        r = int(rows[k]) if by_row else k
        c = _be16(model.one(case.hdr, case.host_sets(), case.sums, b.src[o:o + ln], k, r), fat)
        # with the word at 0 the field is c: the other words add up to ~c, and
        # the word c + v makes them 0xffff + v
        assert 1 <= c <= 0xFFFD, c
        put(k, c + v)
        checks.append((k, fat, WANT[what][v], f"{key} word c{v:+d}"))
    if what == "udp":
        kept = bytes(case.hdr[fat:fat + 2])
        if name == "v6_udp":
            kept = int(case.backing["csum"].view(np.uint16)[BIG_AT]).to_bytes(2, "big")
        checks.append((BIG_AT, fat, kept, "no datagram: the field is as emitted"))
    return Job(f"{name} {what} solved in {key} #{rot}", case, b, {}, tuple(checks))


def solved_jobs():
    for name, what, key, by_row in SOLVED:
        for rot in range(3):
            yield solved_job(name, what, key, by_row, rot)


def extreme_jobs(name: str):
    """Every table of stack `name` all 0xff and all 0x00 under all-0xff
    payloads: the longest datagram (S = 65,535) and one byte more (its field
    is left), at both destination parities, and a few short ones."""
    for fill in (0xFF, 0x00):
        rng = np.random.default_rng([67, rc.STACKS.index(name)])
        n, n_rows = 8, 3
        case = rc.stack(name, "dense", n, n_rows, rng)
        for a in case.backing.values():
            a[:] = fill
        u = next(s for s in case.sums if int(s[0]) == int(EmitSum.UDP))
        longest = 65535 - (len(case.hdr) - u[1])
        lens = [longest, longest + 1, 0, 1, longest, longest + 1, 17, 1024]
        rows = (np.arange(n) % n_rows).astype(np.uint32)
        b = place(lens, len(case.hdr), rng, rows, n_rows,
                  dict(enumerate((0, 0, 2, 3, 1, 1, 4, 5))))
        b.src[:] = 0xFF
        kept = bytes(case.hdr[u[1] + 6:u[1] + 8])
        checks = tuple((k, u[1] + 6, kept, "S = 65,536") for k in (1, 5))
        yield Job(f"{name} tables {fill:#04x}", case, b, {}, checks)


# ---------------------------------------------------------------------------
# D. Tables, rows, guard
# ---------------------------------------------------------------------------
FAR_ROWS, FAR_PITCH = 4099, 1 << 20


def far_job(kind: str) -> Job:
    """A by-row table ("u32": V4_SOURCE of geneve_v4; "v6": the IPv6
    destination of opte) of 4,099 rows that the device test places 1 MiB
    apart: rows 4,096.. lie past 2^32.  The Job's own table is dense."""
    rng = np.random.default_rng([71, len(kind)])
    n = 70
    hdr, _, sums = cases.stack("geneve_v4" if kind == "u32" else "opte", 1, rng)
    backing = {}
    if kind == "u32":
        t = table(backing, "far", rng.integers(0, 1 << 32, FAR_ROWS, dtype=np.uint64)
                  .astype(np.uint32))
        sets = [(14, Field.V4_TOTAL_LEN, LENGTH, 0), (34, Field.UDP_LENGTH, LENGTH, 0),
                (14, Field.V4_SOURCE, U32, 0, ("row", t))]
    else:
        t = table(backing, "far", _rows_of(rng, FAR_ROWS, 16))
        sets = [(14, Field.V6_PAYLOAD_LEN, LENGTH, -40), (54, Field.UDP_LENGTH, LENGTH, 0),
                (14, WideField.V6_DESTINATION, BYTES, 0, ("row", t))]
    rows = rng.integers(0, FAR_ROWS, n, dtype=np.uint64).astype(np.uint32)
    rows[:8] = (4096, 4097, 4098, 0, 1, 4095, FAR_ROWS, ROW_NONE)
    rows[64:67] = (4098, 2, 4097)
    assert (FAR_ROWS - 1) * FAR_PITCH >= 1 << 32
    b = place(rng.integers(0, 120, n), len(hdr), rng, rows, FAR_ROWS)
    return Job(f"rows 1 MiB apart, {kind}", rc.Case(hdr, sets, sums, backing), b, {2: FAR_PITCH})


def guard_jobs():
    """-> [(Job, whether anything is emitted)]: a row array and no BY_ROW set;
    n_rows = 0 (nothing is written); one survivor in each prologue subgroup."""
    out = []
    rng = np.random.default_rng(73)
    n, n_rows = 130, 7
    rows = rc.row_indices(n, n_rows, rng, guarded=(0, 5, 63, 64, 100, n - 1))
    case = rc.stack("v6_udp", "dense", n, n_rows, rng)
    assert not any(isinstance(s[-1], tuple) for s in case.sets)
    out.append((Job("guard only", case, Batch(*rc.batch(n, len(case.hdr), rng, rows, n_rows),
                                              rows, n_rows)), True))
    for name in ("opte", "v6_udp"):
        rows = rng.integers(0, 3, n, dtype=np.uint64).astype(np.uint32)
        rows[7] = ROW_NONE
        case = rc.stack(name, "dense", n, 1, rng)
        out.append((Job(f"n_rows = 0, {name}", case,
                        Batch(*rc.batch(n, len(case.hdr), rng, rows, 0), rows, 0)), False))
    for sub, lane in enumerate((10, 63, 0, 33)):
        n = 256
        rows = np.where(np.arange(n) % 2 == 0, 1, ROW_NONE).astype(np.uint32)
        rows[64 * sub + lane] = 0
        case = rc.stack("opte", "dense", n, 1, rng)
        out.append((Job(f"one survivor, subgroup {sub}", case,
                        Batch(*rc.batch(n, len(case.hdr), rng, rows, 1), rows, 1)), True))
    return out


def pitch_zero_job() -> Job:
    """opte with every table dense: the raw call may name each pitch as 0."""
    rng = np.random.default_rng(79)
    n, n_rows = 130, 7
    rows = rc.row_indices(n, n_rows, rng, guarded=(3, 64))
    case = rc.stack("opte", "dense", n, n_rows, rng)
    return Job("pitch 0", case, Batch(*rc.batch(n, len(case.hdr), rng, rows, n_rows), rows, n_rows))


# ---------------------------------------------------------------------------
# The second way, and the faults a device could have
# ---------------------------------------------------------------------------
FAULTS = {
    "rshift": "A", "add after mask": "A", "u32 as u16": "A", "row is packet": "A", "length": "A",
    "be32": "B", "mac tail": "B", "first wins": "B",
    "udp zero": "C",
    "offset 32": "D", "guard": "D",
}


def _set_field(h: bytearray, first_bit: int, bits: int, v: int, fault, masked: bool) -> None:
    """The header's setter: the covering bytes of bits [first_bit, + bits),
    most significant first, take v's low `bits` bits; every other bit stays."""
    pos, bit = first_bit // 8, first_bit % 8
    nbytes = (bit + bits + 7) // 8
    rshift = (8 - (bit + bits) % 8) % 8
    if fault == "rshift" and rshift:
        rshift -= 1
    fm = (1 << bits) - 1
    m = fm << rshift
    vb = ((v & fm) if masked else v) << rshift
    for k in range(nbytes):
        shb = 8 * (nbytes - 1 - k)
        mb = (m >> shb) & 0xFF
        h[pos + k] = (h[pos + k] & ~mb & 0xFF) | ((vb >> shb) & (mb if masked else 0xFF))


def _row(t, row: int, pitch: int, fault):
    """Row `row` of host table `t` -> its bytes (u8 array) or integer; a row
    the table does not hold reads as 0."""
    if fault == "offset 32":
        o = (row * pitch) & 0xFFFFFFFF
        row = o // pitch if o % pitch == 0 else len(t)
    a = np.asarray(t)
    if row >= len(a):
        return np.zeros(a.shape[1:] or (1,), a.dtype).reshape(-1)
    return np.asarray(a[row]).reshape(-1)


def emulate(job: Job, fault=None):
    """-> (arena, packets whose descriptors point outside the arenas).  The
    call in plain Python: the row guard, the sets in list order (a wide field
    in wire-order pieces of 4 and, a MAC's last, 2 bytes), the payload, the
    sums.  `fault` (a key of FAULTS) makes one mistake on the way."""
    case, b = job.case, job.b
    hdr = bytes(case.hdr)
    H = len(hdr)
    pairs = list(zip(range(len(case.sets)), case.sets, case.host_sets()))
    if fault == "first wins":
        pairs.reverse()
    arena = np.full(b.size, 0xA5, np.uint8)
    outside = 0
    for i in range(len(b.lens)):
        r = i
        if b.rows is not None:
            r = int(b.rows[i])
            if (r > b.n_rows) if fault == "guard" else (r >= b.n_rows):
                continue
        d, o, ln = int(b.dst_off[i]), int(b.off[i]), int(b.lens[i])
        if d + H + ln > b.size or o + ln > len(b.src):
            outside += 1
            continue
        h = bytearray(hdr)
        for k, s, e in pairs:
            at, field, source, add = int(e[0]), e[1], EmitSource(int(e[2])), int(e[3])
            by_row, t = model._table(e)
            row = (i if fault == "row is packet" else r) if by_row else i
            if t is not None:
                view = s[4][1] if isinstance(s[4], tuple) else s[4]
                val = _row(t, row, job.pitch.get(k, view.pitch), fault)
            if source == BYTES:
                wf = WideField(int(field))
                pos = at + model.WIDE_AT[wf]
                for p0 in range(0, WIDE_BYTES[wf], 4):
                    piece = bytes(val[p0:p0 + 4])
                    if len(piece) == 4 and fault == "be32":
                        piece = piece[::-1]
                    if len(piece) == 2 and fault == "mac tail":
                        piece = bytes(val[0:2])
                    h[pos + p0:pos + p0 + len(piece)] = piece
                continue
            _, first, bits = mrm.GEOMETRY[Field(int(field))]
            masked = True
            if source == LENGTH:
                v = H + ln - (0 if fault == "length" else at) + add
            elif source == VALUE:
                v = add
            else:
                tv = int(val[0])
                if source == U32 and fault == "u32 as u16":
                    tv &= 0xFFFF
                if fault == "add after mask":
                    tv, masked = tv & ((1 << bits) - 1), False
                v = tv + add
            _set_field(h, 8 * at + first, bits, v & 0xFFFFFFFF, fault, masked)
        pkt = np.concatenate([np.frombuffer(bytes(h), np.uint8), b.src[o:o + ln]])
        if case.sums:
            emodel.one(pkt, hdr, case.sums)
            if fault == "udp zero":
                u = next(s for s in case.sums if int(s[0]) == int(EmitSum.UDP))
                if H + ln - u[1] <= 65535 and bytes(pkt[u[1] + 6:u[1] + 8]) == b"\xff\xff":
                    pkt[u[1] + 6:u[1] + 8] = 0
        arena[d:d + H + ln] = pkt
    return arena, outside
