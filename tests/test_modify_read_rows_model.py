"""tests/modify_read_rows_model.py, the definition of
ingot_gpu_parse_read_modify_rows, held to the two definitions it composes, to a
from-scratch receiver, and to the batches and the comparison that
tests/test_modify_read_rows.py relies on.  CPU only."""
from functools import lru_cache

import numpy as np
import pytest

import oracle
from ingot_amd.abi import CSUM_L4, CSUM_OUTER_L4, L3Kind, Chain
from tests import csum_frames as cf
from tests import csum_update_model as upd
from tests import modify_read_cases as mc
from tests import modify_read_model as mrm
from tests import modify_read_rows_cases as rc2
from tests import modify_read_rows_model as model
from tests import modify_rows_cases as rc
from tests import modify_rows_model as rows_model

TUN = Chain.GeneveOverV6Tunnel


@pytest.mark.parametrize("chain", rc2.CHAINS, ids=lambda c: c.name)
def test_one_chunk_per_packet_is_parse_modify_rows(chain):
    b = rc2.batch(chain, 129, "single")
    arena, seg_off, seg_len, _ = b.tables
    off, lens = seg_off[:129], seg_len[:129]
    parsed = mrm.parse(b.tables, chain)
    moved = 0
    for what in rc2.valid_whats(chain):
        got, recs, chunk = model.apply(b.tables, chain, b.edits, b.rows, b.n_rows, what, parsed)
        want, w_recs = rows_model.apply(arena, off, lens, chain, b.edits, b.rows, b.n_rows, what)
        assert got.tobytes() == want.tobytes(), what
        assert recs.tobytes() == w_recs.tobytes()
        moved += int((got != arena).any())
    assert moved == len(rc2.valid_whats(chain))


@pytest.mark.parametrize("profile,chain,cutter", mc.CUT_SETS,
                         ids=[f"{p}-{c.name}-{k}" for p, c, k in mc.CUT_SETS])
def test_value_only_lists_are_parse_read_modify(profile, chain, cutter):
    b = rc2.value_batch(profile, chain, cutter)
    parsed = mrm.parse(b.tables, chain)
    _, full = mc.nat_list(chain)
    for what in (0, full):
        got, recs, chunk = model.apply(b.tables, chain, b.edits, what=what, parsed=parsed)
        want, w_recs, w_chunk = mrm.apply(b.tables, chain, b.edits, what, parsed=parsed)
        assert got.tobytes() == want.tobytes(), what
        assert recs.tobytes() == w_recs.tobytes() and (chunk == w_chunk).all()
    assert (got != b.tables[0]).any()


@pytest.mark.parametrize("tunnel", [False, True])
def test_a_receiver_verifies_every_selected_sum(tunnel):
    """Frames whose sums are right, one header per chunk, NAT66 + MACs + narrow
    fields under the full `what`: tests/csum_model, from scratch over the
    logical frames, finds every sum in the state it was in."""
    b = rc2.receiver_batch(tunnel)
    src = rc.right_sum_tunnel_frames() if tunnel else rc.right_sum_frames()
    before = rc.states(*src, b.chain)
    assert rc.all_ok(before).mean() >= 0.9
    got, recs, _ = model.apply(b.tables, b.chain, b.edits, what=rc2.FULL_WHAT[b.chain])
    assert (recs["status"] == 0).all()
    n = len(recs)
    frames = [rc2.logical(got, b.tables, i) for i in range(n)]
    assert all(f != rc2.logical(b.tables[0], b.tables, i) for i, f in enumerate(frames))
    after = rc.states(*cf.place(frames, misalign=3), b.chain)
    assert (after == before).all(), np.nonzero((after != before).any(axis=1))[0][:5]


# ---------------------------------------------------------------------------
# No vacuous batch
# ---------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _batches():
    return rc2.gpu_batches()


def test_every_gpu_batch_reaches_what_it_is_meant_to():
    seen = set()
    for b, style, holds in _batches():
        parsed = mrm.parse(b.tables, b.chain)
        recs = parsed[0]
        ok = recs["status"] == 0
        pieces = rc2.applied_pieces(b, parsed)
        if "paths" in holds:
            want = rc2.expected_paths(b, style)
            got = rc2.paths(b, parsed)
            assert want <= got, (b.name, want - got)
            seen |= got
        if "guarded" in holds:
            assert (ok & (b.rows >= b.n_rows)).any(), b.name
        if "not ok" in holds:
            assert (~ok).any(), b.name
        if "mod 4" in holds:
            assert {at % 4 for _, _, _, at, nb in pieces if nb == 4} == {0, 1, 2, 3}, b.name
        if b.name.endswith("/survivors"):
            assert len({i for i, *_ in pieces}) >= 3  # (a survivor that parsed Ok, per tile)
        elif b.rows is None or (b.rows < b.n_rows).any():
            assert pieces, b.name
    assert seen == {"first", "prefetched", "last", "late"}


def test_index_four_and_later_only_where_the_chain_allows():
    for b, style, holds in _batches():
        if b.chain in (Chain.GenericUlp, Chain.UdpParser):
            assert "late" not in rc2.paths(b), b.name


# ---------------------------------------------------------------------------
# The comparison catches simulated device faults
# ---------------------------------------------------------------------------
SENTINEL = 0xEE


def outcome(b, what, edit=rows_model.edit_packet, sums=rows_model.sums, guard=True,
            before_of=lambda f, rec: f, after_hook=None, records=lambda recs, i: True):
    """model.apply with the hooks a faulty device is simulated through ->
    (arena, records as the device would leave them over a sentinel, chunk)."""
    arena, seg_off, seg_len, pkt_seg = b.tables
    recs, gf, chunk = mrm.parse(b.tables, b.chain)
    want = np.array(arena)
    out = np.full((len(recs), 16), SENTINEL, np.uint8)
    for i in range(len(pkt_seg) - 1):
        guarded = b.rows is not None and int(b.rows[i]) >= b.n_rows
        if records(recs, i) or not guarded:
            out[i] = np.frombuffer(recs[i].tobytes(), np.uint8)
        if int(recs["status"][i]) != 0 or (guard and guarded):
            continue
        ks = range(int(pkt_seg[i]), int(pkt_seg[i + 1]))
        before = model.gather(arena, seg_off, seg_len, ks)
        after = before.copy()
        outer = gf["outer"][i] if b.chain == TUN else None
        edit(after, b.chain, recs[i], outer, b.edits, i, b.rows)
        if what:
            sums(before_of(before, recs[i]), after, b.chain, recs[i], what,
                 int(outer["outer_udp_off"]) if b.chain == TUN else None)
        if after_hook:
            after_hook(after, before, recs[i], outer)
        model.scatter(want, seg_off, seg_len, ks, after)
    return want, out, chunk


def same(x, y) -> bool:
    """The GPU file's comparison: the whole arena, the records, the chunks."""
    return (x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
            and (x[2] == y[2]).all())


def _edit_wrapped_rows(f, chain, rec, outer, edits, i, rows):
    rows_model.edit_packet(f, chain, rec, outer, edits, i, rows % rc2.N_ROWS)


def _edit_rows_by_packet(f, chain, rec, outer, edits, i, rows):
    by_packet = np.arange(len(rows), dtype=np.uint32) % rc2.N_ROWS  # row i, not rows[i]
    rows_model.edit_packet(f, chain, rec, outer, edits, i, by_packet)


def _sums_without(v6_pseudo=False, outer_addresses=False):
    def sums(b, a, chain, rec, what, o_udp=None):
        b2 = np.array(b)
        if v6_pseudo and int(rec["l3_kind"]) == int(L3Kind.IPV6):
            # the addresses count as unchanged: their words fall out of the delta
            l3 = int(rec["l3_off"])
            rows_model.sums(b, a, chain, rec, what & ~CSUM_L4, o_udp)
            keep = a[l3 + 8:l3 + 40].copy()
            a[l3 + 8:l3 + 40] = b[l3 + 8:l3 + 40]
            b3 = np.array(b)
            rows_model.sums(b3, a, chain, rec, what & CSUM_L4, None)
            a[l3 + 8:l3 + 40] = keep
            return
        if outer_addresses and (what & CSUM_OUTER_L4):
            rows_model.sums(b, a, chain, rec, what & ~CSUM_OUTER_L4, o_udp)
            keep = a[22:54].copy()
            a[22:54] = b[22:54]
            rows_model.sums(b2, a, chain, rec, CSUM_OUTER_L4, o_udp)
            a[22:54] = keep
            return
        rows_model.sums(b, a, chain, rec, what, o_udp)
    return sums


def _zero_old_v6_source(f, rec):
    g = np.array(f)
    if int(rec["l3_kind"]) == int(L3Kind.IPV6):
        g[int(rec["l3_off"]) + 8:int(rec["l3_off"]) + 24] = 0
    return g


def test_the_comparison_catches_each_simulated_fault():
    g = rc2.batch(Chain.GenericUlp, 257, "headers")
    t = rc2.batch(TUN, 257, "headers")
    right = {b.name: outcome(b, rc2.FULL_WHAT[b.chain]) for b in (g, t)}
    for b in (g, t):  # the harness itself is the model
        w = model.apply(b.tables, b.chain, b.edits, b.rows, b.n_rows, rc2.FULL_WHAT[b.chain])
        assert right[b.name][0].tobytes() == w[0].tobytes()
        assert right[b.name][1].tobytes() == w[1].tobytes()

    def caught(b, **kw):
        return not same(outcome(b, rc2.FULL_WHAT[b.chain], **kw), right[b.name])

    assert caught(g, guard=False, edit=_edit_wrapped_rows), "the guard is ignored"
    assert caught(g, edit=_edit_rows_by_packet), "BY_ROW is read by packet"
    assert caught(g, sums=_sums_without(v6_pseudo=True)), "no IPv6 pseudo-header in L4"
    assert caught(t, sums=_sums_without(outer_addresses=True)), "no outer addresses in OUTER_L4"
    assert caught(g, before_of=_zero_old_v6_source), "old bytes taken as zero"
    assert caught(g, records=lambda recs, i: False), "a guarded packet's record is dropped"

    def swapped(after, before, rec, outer):
        if int(rec["l3_kind"]) == int(L3Kind.IPV6):
            at = int(rec["l3_off"]) + 24
            after[at:at + 4] = after[at:at + 4][::-1].copy()
    assert caught(g, after_hook=swapped), "a piece is byte-swapped"

    def widened(after, before, rec, outer):
        # the inner MAC source's 2-byte tail stored as 4 bytes: the ethertype goes
        at = int(outer["inner_eth_off"]) + 12
        after[at:at + 2] = 0
    assert caught(t, after_hook=widened), "a 2-byte MAC tail stored as 4 bytes"

    # a piece stored at its logical offset in chunk 0 (for a header in a later
    # chunk: past chunk 0's end, in the gap or in the next chunk)
    arena, seg_off, seg_len, pkt_seg = g.tables
    want = right[g.name][0]
    wrong = want.copy()
    moved = 0
    starts = {}
    for i, c, nk, at, nb in rc2.applied_pieces(g):
        if c == 0 or nb != 4:
            continue
        ks = range(int(pkt_seg[i]), int(pkt_seg[i + 1]))
        s = starts.setdefault(i, np.cumsum([0] + [int(seg_len[k]) for k in ks]))
        x = at - int(seg_off[ks[c]]) + int(s[c])
        o0 = int(seg_off[ks[0]])
        wrong[o0 + x:o0 + x + nb] = want[at:at + nb]
        wrong[at:at + nb] = arena[at:at + nb]
        moved += 1
    assert moved and wrong.tobytes() != want.tobytes(), "a piece stored into chunk 0"
