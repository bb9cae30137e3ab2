"""The batches of tests/dispatch_cases.py, held to account on the CPU: the
GPU tests of tests/test_dispatch_variants.py would be vacuous if the later
trips round a kernel's tile loop had nothing to rewrite, nothing to refuse, or
if a packet's expected bytes depended on its neighbours.  Every figure here
comes from the definitions alone (the oracle, csum_sweep_cases.define,
modify_read_cases.contiguous_definition); no device is involved."""
import numpy as np
import pytest

import oracle
from ingot_amd import Chain
from tests import csum_sweep_cases as sc
from tests import dispatch_cases as dc
from tests import modify_read_cases as mc
from tests import modify_read_model

TUN = dc.TUN
chains = pytest.mark.parametrize("chain", sc.CHAINS, ids=lambda c: c.name)
cut_sets = pytest.mark.parametrize("profile,chain,cutter", mc.CUT_SETS,
                                   ids=[f"{p}-{c.name}-{k}" for p, c, k in mc.CUT_SETS])
# the cut sets every packet of which the NAT list rewrites
ALL_REWRITTEN = [("MIXED", Chain.GenericUlp, "cut"), ("VLAN_V6EH", Chain.VlanUlp, "cut"),
                 ("GENEVE", TUN, "cut")]


def test_tile_count_and_trips():
    """833 packets: 14 tiles, the last of one packet.  One block: waves 0 and 1
    make four trips, waves 2 and 3 three, and the one-packet tile is wave 1's
    fourth.  Three blocks: waves 0 and 1 of block 0 make two trips, every other
    wave one, so waves with and without a second trip share a block."""
    assert dc.tiles_of(dc.N) == dc.TILES == 14 and dc.N - 13 * dc.WAVE == 1
    one = dc.trips(dc.N, 1)
    assert [len(one[0, w]) for w in range(4)] == [4, 4, 3, 3]
    assert one[0, 1] == [1, 5, 9, 13]
    three = dc.trips(dc.N, 3)
    assert len(three) == 12
    assert [len(three[0, w]) for w in range(4)] == [2, 2, 1, 1] and three[0, 1] == [1, 13]
    assert all(len(three[b, w]) == 1 for b in (1, 2) for w in range(4))
    for blocks in dc.BLOCKS:  # every tile is walked exactly once
        walked = sorted(t for ts in dc.trips(dc.N, blocks).values() for t in ts)
        assert walked == list(range(dc.TILES))
    # the trip a packet is handled on with one block is its iteration class
    for (_, w), ts in one.items():
        for trip, t in enumerate(ts):
            assert int(dc.iteration_class(t * dc.WAVE)) == trip
    assert dc.per_class(np.ones(dc.N, bool)) == [256, 256, 256, 65]
    # the default grid makes no second trip at any size the suite uses
    assert all(len(ts) == 1 for ts in dc.trips(16_777_216, 0).values())


# ---------------------------------------------------------------------------
# A. the contiguous rewrite
# ---------------------------------------------------------------------------
@chains
@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_rewrite_batches_rewrite_on_every_trip(chain, layout):
    """Every list that rewrites anything does so in all four iteration
    classes; the NAT list and the twice-set list rewrite the one-packet tile
    (packet 832) and, but for UdpParser's TCP / ICMP frames, every packet."""
    still = set()
    for k, (name, _, _) in enumerate(dc.rewrite_lists(chain)):
        for what in dc.rewrite_whats(chain):
            e = dc.rewrite_expected(chain, layout, k, what)
            assert e.batch.n == dc.N
            mask = np.zeros(dc.N, bool)
            mask[e.changed] = True
            counts = dc.per_class(mask)
            assert all(c > 0 for c in counts) or not any(counts), (name, what, counts)
            if not any(counts):
                still.add(name)
            if name in ("nat", "set twice"):
                assert mask[dc.N - 1], (name, what)
                if chain != Chain.UdpParser:
                    assert counts == [256, 256, 256, 65], (name, what, counts)
    # only an edit and its inverse, and TCP's fields under UdpParser, move nothing
    allowed = {"inverse xor xor", "inverse add sub"}
    assert still <= allowed | ({"tcp byte 12 13"} if chain == Chain.UdpParser else set()), still


@chains
@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_rewrite_batches_hold_packets_that_are_not_ok(chain, layout):
    """UdpParser refuses the TCP and ICMP frames: packets that must not be
    stored to sit in every iteration class.  (The other chains parse every
    frame of these batches; their refusals are tests B and C's.)"""
    e = dc.rewrite_expected(chain, layout, 0, 0)
    not_ok = dc.per_class(e.recs["status"] != 0)
    if chain == Chain.UdpParser:
        assert min(not_ok) >= 31, not_ok
    else:
        assert not any(not_ok), not_ok
    starts = e.batch.starts
    for i in np.nonzero(e.recs["status"] != 0)[0]:
        o, ln = int(starts[i]), int(e.batch.lengths[i])
        assert e.want[o:o + ln].tobytes() == e.batch.arena[o:o + ln].tobytes(), i


@chains
@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_rewrite_definition_and_two_pass_agree_where_they_must(chain, layout):
    """On the frames sc.qualifies names, the definition equals the rewrite
    followed by a checksum fill, under every `what` (the tunnel's included)."""
    held = 0
    for k in range(len(dc.rewrite_lists(chain))):
        for what in dc.rewrite_whats(chain):
            e = dc.rewrite_expected(chain, layout, k, what)
            if e.two_pass is not None:
                assert sc.frames_differ(e.batch, e.want, e.two_pass, e.both) is None, (k, what)
                held += len(e.both)
    assert held > 5 * dc.N, held


@chains
@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_rewrite_of_256_packets_alone_is_the_whole_batch_rewrite(chain, layout):
    """The definition applied to packets [256 k, 256 (k + 1)) alone gives those
    packets' bytes of the whole-batch definition and leaves every other byte:
    no packet's result depends on another's, so nothing excuses a difference
    between launch shapes."""
    lists = dc.rewrite_lists(chain)
    for k in (0, len(lists) - 1):  # the NAT list, the twice-set list
        for what in (0, dc.rewrite_whats(chain)[-1]):
            e = dc.rewrite_expected(chain, layout, k, what)
            b = e.batch
            for c in range(dc.CLASSES):
                lo, hi = 256 * c, min(256 * (c + 1), dc.N)
                sub = dc.rewrite_slice(b, lo, hi)
                want, _, recs, _ = sc.define(sub, chain, e.edits, what)
                assert recs.tobytes() == e.recs[lo:hi].tobytes()
                shift = len(b.arena) - len(sub.arena)
                whole = np.array(b.arena[shift:])
                a, z = int(b.starts[lo]) - shift, int(b.starts[hi - 1] + b.lengths[hi - 1]) - shift
                whole[a:z] = e.want[shift:][a:z]
                assert want.tobytes() == whole.tobytes(), (k, what, c)


# ---------------------------------------------------------------------------
# B. the parse and parse_read
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chain", list(Chain), ids=lambda c: c.name)
def test_parse_batches_hold_both_outcomes_on_every_trip(chain):
    """Packets that parse and packets that do not, in every iteration class:
    indexed frames, slots (VLAN_V6EH under VlanUlp: all Ok; under the tunnel:
    none) and chunked packets."""
    e = dc.parse_expected(chain)
    bad = dc.per_class(e["rec"]["status"] != 0)
    ok = dc.per_class(e["rec"]["status"] == 0)
    s_ok = dc.per_class(e["srec"]["status"] == 0)
    assert min(bad) >= 31, bad
    assert min(s_ok) >= 16 or chain == TUN, s_ok
    # (few ADVERSARIAL frames hold a UDP datagram: the slots supply UdpParser's Ok packets)
    assert min(a + b for a, b in zip(ok, s_ok)) >= 1, (ok, s_ok)
    tables = dc.read_tables(chain)
    assert len(tables[3]) == dc.N + 1
    per_packet = np.diff(tables[3].astype(np.int64))
    assert per_packet.max() == 8 and per_packet.min() == 1  # past the prefetched descriptors
    recs, _, chunk = dc.read_expected(chain)
    assert min(dc.per_class(recs["status"] != 0)) >= 31
    assert min(dc.per_class(chunk > 0)) >= 1  # the remainder lies past chunk 0 somewhere


# ---------------------------------------------------------------------------
# C. the rewrite over chunk lists
# ---------------------------------------------------------------------------
@cut_sets
def test_chunked_batches_rewrite_and_refuse_on_every_trip(profile, chain, cutter):
    """Packets rewritten, and packets that are not Ok, per iteration class.
    MIXED, VLAN_V6EH and GENEVE: all 833 rewritten, the one-packet tile
    included.  MIXED under UdpParser and the ADVERSARIAL sets: at least 31
    packets that are not Ok in every class, so "no store for a packet that is
    not Ok" is tested on every trip.  The ADVERSARIAL sets rewrite at least 5
    packets in each of the three full classes; among the last 65 packets of
    these generator seeds none parses to an IP header, so their fourth trip
    tests only that nothing is stored (the other four sets rewrite on it)."""
    c = dc.chunked_batch(profile, chain, cutter)
    assert len(c.tables[3]) == dc.N + 1
    edits, what = mc.nat_list(chain)
    for w in (0, what):
        want, recs, chunk = dc.chunked_expected(profile, chain, cutter, w)
        moved = dc.rewritten_packets(c, want)
        counts, not_ok = dc.per_class(moved), dc.per_class(recs["status"] != 0)
        assert not (moved & (recs["status"] != 0)).any()
        if (profile, chain, cutter) in ALL_REWRITTEN:
            assert counts == [256, 256, 256, 65] and moved[dc.N - 1]
        elif cutter == "split":
            assert min(counts[:3]) >= 5 and min(not_ok) >= 31, (counts, not_ok)
            assert (recs["status"] == 4).sum() > 100  # StraddledHeader
        else:
            assert min(counts) >= 5 and min(not_ok) >= 31, (counts, not_ok)
        # the mapped-back contiguous definition is the chunked definition
        # (tests/modify_read_model.py), byte for byte
        m_want, m_recs, m_chunk = modify_read_model.apply(c.tables, chain, edits, w)
        assert m_want.tobytes() == want.tobytes()
        assert m_recs.tobytes() == recs.tobytes() and (m_chunk == chunk).all()


@cut_sets
def test_chunked_rewrite_of_256_packets_alone_is_the_whole_batch_rewrite(profile, chain, cutter):
    """As for the contiguous batches: packets [256 k, 256 (k + 1)) rewritten
    alone get the bytes they get in the whole batch."""
    c = dc.chunked_batch(profile, chain, cutter)
    edits, what = mc.nat_list(chain)
    want, recs, _ = dc.chunked_expected(profile, chain, cutter, what)
    _, seg_off, seg_len, pkt_seg = c.tables
    for k in range(dc.CLASSES):
        lo, hi = 256 * k, min(256 * (k + 1), dc.N)
        rew, crecs = mc.contiguous_definition(c.arena, c.off[lo:hi], c.lens[lo:hi], chain, edits,
                                              what)
        for i in range(lo, hi):
            ok = int(recs["status"][i]) == 0
            assert not ok or crecs[i - lo].tobytes() == recs[i].tobytes()
            o, ln = int(c.off[i]), int(c.lens[i])
            logical = mc.logical(want, c.tables, i)
            assert logical == (rew if ok else c.arena)[o:o + ln].tobytes(), i
        rest = np.ones(len(rew), bool)
        rest[int(c.off[lo]):int(c.off[hi - 1]) + int(c.lens[hi - 1])] = False
        assert (rew[rest] == c.arena[rest]).all()


# ---------------------------------------------------------------------------
# D. chains in host memory
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("profile,chain,n", dc.HOST_SETS, ids=lambda x: getattr(x, "name", str(x)))
def test_host_chains_are_chunked_and_rewritten(profile, chain, n):
    c = dc.host_chains(profile, chain, n)
    per_packet = np.diff(c.tables[3].astype(np.int64))
    assert len(per_packet) == n and per_packet.max() >= 5 and (per_packet >= 2).sum() > n // 2
    want, recs, _ = dc.chunked_expected(profile, chain, "cut", mc.nat_list(chain)[1], n)
    assert (recs["status"] == 0).all()
    assert dc.rewritten_packets(c, want).all()
    crecs = oracle.parse_batch(c.arena, c.off, c.lens, chain)
    assert crecs.tobytes() == recs.tobytes()
