"""Batches and expected results shared by tests/test_dispatch_cases.py (CPU) and
tests/test_dispatch_variants.py (GPU): the kernel variants a tuning key or the
arena's memory kind selects, and the second trip round every grid-stride tile
loop.  TEST INFRASTRUCTURE ONLY.

Nothing here defines an operation.  Every expected value comes from the
existing definitions: the oracle, tests/csum_update_model.py (through
csum_sweep_cases.define and modify_read_cases.contiguous_definition),
tests/csum_read_model.py and tests/emit_read_model.py.

N = 833 packets is 13 full 64-packet tiles and a last tile of one packet.  The
kernels' loop is `for (t = block * 4 + wave; t < tiles; t += blocks * 4)`
(walk.h: grid_for), so with INGOT_TUNE_MAX_BLOCKS = 1 waves 0 and 1 make four
trips and waves 2 and 3 three, the one-packet tile being wave 1's fourth; with
3 blocks waves 0 and 1 of block 0 make two trips and every other wave one.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

import oracle
from ingot_amd import Chain, EditOp, Field, GenProfile
from ingot_amd.hostgen import gen_frames_host
from tests import csum_read_cases as cases
from tests import csum_sweep_cases as sc
from tests import modify_read_cases as mc

TUN = Chain.GeneveOverV6Tunnel
F, SET = Field, EditOp.SET

N = 833
WAVE, WAVES = 64, 4   # packets per tile, waves per block (kernels.h)
TILES = 14
BLOCKS = (1, 3)       # the INGOT_TUNE_MAX_BLOCKS values every loop test runs
CLASSES = 4           # trips of a wave with one block: (i // 64) // 4


def tiles_of(n: int) -> int:
    return (n + WAVE - 1) // WAVE


def trips(n: int, blocks: int):
    """-> {(block, wave): [tile, ...]}: the tiles each wave of a grid capped
    at `blocks` blocks walks, in order (grid_for + the kernels' loop)."""
    tiles = tiles_of(n)
    grid = max(1, min((tiles + WAVES - 1) // WAVES, blocks or 65536))
    return {(b, w): list(range(b * WAVES + w, tiles, grid * WAVES))
            for b in range(grid) for w in range(WAVES)}


def iteration_class(i):
    """The trip (0-based) on which packet i is handled with one block."""
    return (np.asarray(i) // WAVE) // WAVES


def per_class(mask) -> list:
    """How many packets of a boolean mask over the batch fall in each class."""
    cls = iteration_class(np.arange(len(mask)))
    return [int(np.asarray(mask)[cls == c].sum()) for c in range(CLASSES)]


def repeated(frames, n: int = N):
    return (list(frames) * (n // len(frames) + 1))[:n]


# ---------------------------------------------------------------------------
# A. the contiguous rewrite (k_parse, OUT_MODIFY)
# ---------------------------------------------------------------------------
LAYOUTS = ("indexed", "strided")


@lru_cache(maxsize=None)
def rewrite_batch(chain, layout: str, prepared: bool = False) -> sc.Batch:
    """csum_sweep_cases' frames of `chain` repeated to N.  "indexed": at odd
    addresses, 0xA5 between them (sc._indexed_from); "strided": the same frame
    kinds, each exactly 128 B, in 128-B slots (the tunnel: its frames padded to
    the longest, sc._strided_from).  Every sum is valid.  `prepared`: the sums
    of 0 in both representations (sc._edge_sums, sc.other_repr)."""
    if chain == TUN:
        base = sc._tunnel_frames()
    else:
        base = sc._frames_for(chain) if layout == "indexed" else sc._frames_for(chain, 128)
    make = sc._indexed_from if layout == "indexed" else sc._strided_from
    b = make(repeated(base), chain, sc._edge_sums if prepared else None)
    if prepared:
        b = sc.other_repr(b, chain)[0]
    assert b.n == N and (layout == "indexed" or chain == TUN or b.stride == 128)
    return b


def set_twice(chain):
    """Every frame kind gets one field SET and then SET again; the 4-byte ones
    lie across the end of the staged window in some frames."""
    l3 = sc.L3_LAYER[chain]
    l4 = l3 + 1
    return [(l3, F.V4_DESTINATION, SET, 0x0A0B0C0D), (l3, F.V4_DESTINATION, SET, 0xC0A80102),
            (l3, F.V6_FLOW_LABEL, SET, 0xFFFFF), (l3, F.V6_FLOW_LABEL, SET, 0x12345),
            (l4, F.TCP_SEQUENCE, SET, 0xFFFFFFFF), (l4, F.TCP_SEQUENCE, SET, 0x01020304),
            (l4, F.UDP_DESTINATION, SET, 0xFFFF), (l4, F.UDP_DESTINATION, SET, 4789),
            (l4, F.ICMP_CODE, SET, 0xFF), (l4, F.ICMP_CODE, SET, 3)]


@lru_cache(maxsize=None)
def rewrite_lists(chain):
    """-> ((name, edits, prepared), ...): the NAT list, the chain's dependent
    lists and a list that SETs one field twice."""
    out = [("nat", mc.nat_list(chain)[0], False)]
    out += [(n, e, p) for n, e, p in sc.dependent_lists(chain)]
    out.append(("set twice", set_twice(chain), False))
    return tuple((n, tuple(e), p) for n, e, p in out)


def rewrite_whats(chain):
    """0 = the plain rewrite, then every `what` of the chain (the tunnel's
    include the outer sum alone and all three, 7)."""
    return (0,) + tuple(sc.WHATS[chain])


Rewrite = namedtuple("Rewrite", "batch edits want recs changed two_pass both")


@lru_cache(maxsize=None)
def rewrite_expected(chain, layout: str, k: int, what: int) -> Rewrite:
    """List k of rewrite_lists(chain) under `what` on the chain's batch: the
    definition (sc.define), and where sc.qualifies says so the rewrite
    followed by a checksum fill (`two_pass`, to hold on frames `both`)."""
    _, edits, prepared = rewrite_lists(chain)[k]
    edits = list(edits)
    b = rewrite_batch(chain, layout, prepared)
    want, rewritten, recs, ch = sc.define(b, chain, edits, what)
    tp = both = None
    # (the prepared batches hold sums in the representation a fill does not
    # write: the definition only, as tests/test_modify_csum_sweep.py)
    if what and not prepared and ch.size:
        q = sc.qualifies(b, chain, edits, rewritten, recs, ch)
        both = ch[q[ch]]
        tp = sc.two_pass(b, chain, rewritten, recs, ch, what) if both.size else None
    want.setflags(write=False)
    return Rewrite(b, edits, want, recs, ch, tp, both)


def rewrite_slice(b: sc.Batch, lo: int, hi: int) -> sc.Batch:
    """Frames [lo, hi) of `b` as a batch of their own over the same arena."""
    if b.off is None:
        cut = lo * b.stride
        arena = b.arena[cut:]
        starts = b.starts[lo:hi] - np.uint64(cut)
        off = lens = None
    else:
        arena, starts = b.arena, b.starts[lo:hi]
        off, lens = b.off[lo:hi], b.lens[lo:hi]
    return sc.Batch(arena, off, lens, b.stride, hi - lo, starts, b.lengths[lo:hi], b.keep[lo:hi],
                    None if b.o_udp is None else b.o_udp[lo:hi])


# ---------------------------------------------------------------------------
# B. the parse and parse_read
# ---------------------------------------------------------------------------
SLOT = 256


@lru_cache(maxsize=None)
def parse_frames(tunnel: bool):
    """N ADVERSARIAL frames back to back (the tunnel chain: GENEVE_ADVERSARIAL)
    -> (arena, off, lens), read-only."""
    prof = GenProfile.GENEVE_ADVERSARIAL if tunnel else GenProfile.ADVERSARIAL
    arena, off, lens = gen_frames_host(prof, N, seed=4444, slack=64)
    assert (off == np.cumsum(lens, dtype=np.uint64) - lens).all()  # parse_packed's layout
    for a in (arena, off, lens):
        a.setflags(write=False)
    return arena, off, lens


@lru_cache(maxsize=None)
def slot_frames():
    """N VLAN_V6EH frames in 256-B slots with their lengths -> (arena, lens)."""
    arena, _, lens = gen_frames_host(GenProfile.VLAN_V6EH, N, seed=4545, stride=SLOT, slack=64)
    arena.setflags(write=False)
    lens.setflags(write=False)
    return arena, lens


@lru_cache(maxsize=None)
def parse_expected(chain):
    """The oracle over parse_frames and slot_frames -> dict: rec / fld
    (indexed frames), srec / sfld (slots); field blocks as the chain's own
    (ingot_geneve_fields for the tunnel)."""
    arena, off, lens = parse_frames(chain == TUN)
    sarena, slens = slot_frames()
    if chain == TUN:
        rec = oracle.parse_batch(arena, off, lens, chain)
        fld = oracle.geneve_fields_batch(arena, off, lens)
        srec = oracle.parse_batch(sarena, None, slens, chain, stride=SLOT, n=N)
        sfld = oracle.geneve_fields_batch(sarena, None, slens, stride=SLOT, n=N)
    else:
        rec, fld = oracle.parse_batch(arena, off, lens, chain, fields=True)
        srec, sfld = oracle.parse_batch(sarena, None, slens, chain, stride=SLOT, n=N, fields=True)
    return dict(rec=rec, fld=fld, srec=srec, sfld=sfld)


@lru_cache(maxsize=None)
def read_tables(chain):
    """parse_frames' frames cut into 1-8 chunks (tests/test_parse_read.py's
    split_many), every chunk stored on its own (oracle.segments)."""
    from tests.test_parse_read import split_many

    arena, off, lens = parse_frames(chain == TUN)
    packets = split_many(cases.frames_of(arena, off, lens), seed=23 + int(chain))
    tables = oracle.segments(packets)
    for a in tables:
        a.setflags(write=False)
    return tables


@lru_cache(maxsize=None)
def read_expected(chain):
    """oracle.parse_read_batch over read_tables(chain) -> (records, field
    blocks of the chain's kind, chunk indices)."""
    return oracle.parse_read_batch(*read_tables(chain), chain,
                                   fields="geneve" if chain == TUN else "fields")


# ---------------------------------------------------------------------------
# C. the rewrite over chunk lists (k_parse_read_modify)
# ---------------------------------------------------------------------------
Chunked = namedtuple("Chunked", "arena off lens tables")


@lru_cache(maxsize=None)
def chunked_batch(profile: str, chain, cutter: str, n: int = N) -> Chunked:
    """One of modify_read_cases.CUT_SETS at `n` packets: the contiguous frames
    (valid sums, every checksum state present) and their chunks, each chunk at
    its own misalignment 0..15 with one filler byte before it."""
    arena, off, lens, packets = mc.cut_set(profile, chain, cutter, n)
    tables = cases.place(packets, misalign=tuple(range(16)), gap=1)
    for a in (arena,) + tables:
        a.setflags(write=False)
    return Chunked(arena, off, lens, tables)


def map_back(c: Chunked, chain, contiguous_after):
    """The contiguous frames after a rewrite, written back through the chunk
    tables: packets whose chunked record is Ok take the contiguous frame's
    bytes chunk by chunk (such a record equals the contiguous one), every
    other byte of the chunk arena is the original.  -> (arena, records, chunk
    indices) as ingot_gpu_parse_read_modify must leave them."""
    arena, seg_off, seg_len, pkt_seg = c.tables
    recs, _, chunk = oracle.parse_read_batch(*c.tables, chain)
    crecs = oracle.parse_batch(c.arena, c.off, c.lens, chain)
    want = np.array(arena)
    for i in np.nonzero(recs["status"] == 0)[0]:
        assert recs[i].tobytes() == crecs[i].tobytes(), i
        x = int(c.off[i])
        for k in range(int(pkt_seg[i]), int(pkt_seg[i + 1])):
            o, ln = int(seg_off[k]), int(seg_len[k])
            want[o:o + ln] = contiguous_after[x:x + ln]
            x += ln
        assert x == int(c.off[i]) + int(c.lens[i]), i
    return want, recs, chunk


@lru_cache(maxsize=None)
def chunked_expected(profile: str, chain, cutter: str, what: int, n: int = N):
    """The NAT list (modify_read_cases.nat_list) under `what` (0: the plain
    rewrite): modify_read_cases.contiguous_definition on the logical frames,
    mapped back through the tables."""
    c = chunked_batch(profile, chain, cutter, n)
    edits, _ = mc.nat_list(chain)
    rew, _ = mc.contiguous_definition(c.arena, c.off, c.lens, chain, edits, what)
    want, recs, chunk = map_back(c, chain, rew)
    want.setflags(write=False)
    return want, recs, chunk


def rewritten_packets(c: Chunked, want) -> np.ndarray:
    """Mask over the batch: the packets some chunk byte of which changed."""
    _, seg_off, seg_len, pkt_seg = c.tables
    diff = np.asarray(want) != c.tables[0]
    out = np.zeros(len(pkt_seg) - 1, bool)
    for i in range(len(out)):
        out[i] = any(diff[int(seg_off[k]):int(seg_off[k]) + int(seg_len[k])].any()
                     for k in range(int(pkt_seg[i]), int(pkt_seg[i + 1])))
    return out


# ---------------------------------------------------------------------------
# D. mblk chains in mapped host memory
# ---------------------------------------------------------------------------
HOST_SETS = (("MIXED", Chain.GenericUlp, 3000), ("GENEVE", TUN, 1000))


def host_chains(profile: str, chain, n: int) -> Chunked:
    """`n` generator frames cut by csum_read_cases.cut under `chain`."""
    return chunked_batch(profile, chain, "cut", n)


def emit_from_take(lens, rng):
    """Random d_from / d_take, half of the packets whole (as tools/bigfuzz.py's
    emit_read_cases draws them)."""
    n = len(lens)
    ln = np.asarray(lens).astype(np.int64)
    whole = rng.random(n) < 0.5
    frm = np.where(whole, 0, rng.integers(0, ln + 10)).astype(np.uint16)
    take = np.where(rng.random(n) < 0.5, 65535, rng.integers(0, ln + 10)).astype(np.uint16)
    return frm, take
