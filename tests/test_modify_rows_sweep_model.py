"""The cases of tests/modify_rows_sweep_cases.py on the references alone (no
GPU): what tests/test_modify_rows_sweep.py compares the device with is held
here to a second way of computing it, and every case is shown to reach the
edge it is named for.

The definition is tests/modify_rows_model.py (written from the header); the
second way is its plain rewrite (what = 0) followed by the from-scratch fill of
the same sums (tests/csum_model.py), on every frame that fill sums before and
after.  The frames left out of that comparison may only be the ones fill does
not sum: IPv4 fragments, a UDP field of 0, frames that did not parse Ok, and,
in the batches that hold IPv4 sums in the 0xffff representation, those frames
(fill writes 0x0000).
"""
from collections import Counter

import numpy as np
import pytest

from ingot_amd import Chain, EditOp, Field
from ingot_amd.abi import ROW_NONE
from tests import csum_model
from tests import csum_sweep_cases as sc
from tests import modify_read_model as mrm
from tests import modify_rows_sweep_cases as rc

TUN = sc.TUN
V6S, V6D, MACD, MACS = rc.V6S, rc.V6D, rc.MACD, rc.MACS
chains = pytest.mark.parametrize("chain", sc.CHAINS, ids=lambda c: c.name)


def _not_summed(b, chain):
    """The frames fill cannot sum, from the input alone: not Ok, an IPv4
    fragment (MF or an offset), a UDP (the tunnel: or outer UDP) field of 0."""
    fields = rc.sum_fields(b, chain)
    kind = rc.kinds(b, chain)
    recs, _ = rc.headers(b, chain)
    # (an IPv6 packet behind a Fragment header: fill's own walk of the EHs)
    state = csum_model.verify(b.arena, b.starts, b.lengths, recs)["l4_state"]
    out = set(np.nonzero(state == int(csum_model.FRAGMENT))[0].tolist())
    for i in range(b.n):
        if kind[i] is None:
            out.add(i)
            continue
        if kind[i][0] == "v4":
            o = int(b.starts[i]) + int(recs["l3_off"][i]) + 6
            if rc.be16(b.arena, o) & 0x3FFF:
                out.add(i)
        if kind[i][1] == "udp" and rc.be16(b.arena, int(fields[i, 1])) == 0:
            out.add(i)
        if chain == TUN and rc.be16(b.arena, int(fields[i, 2])) == 0:
            out.add(i)
    return out


def _held(g, outs, recs, whats=None, also_out=(), strict=True):
    """The definition's arenas `outs` (one per g.whats) against the second way
    under `whats` (default: all of g.whats but 0).  -> frames compared.
    `strict`: every changed frame is compared but the ones fill cannot sum
    (not for edits that themselves make a frame a fragment or end its parse)."""
    plain = outs[g.whats.index(0)] if 0 in g.whats else rc.definition(g, 0)[0]
    compared = 0
    allowed = None
    for what in (w for w in (g.whats if whats is None else whats) if w):
        tp, both, ch = rc.second_way(g, plain, recs, what)
        both = both[~np.isin(both, list(also_out))] if len(also_out) else both
        want = outs[g.whats.index(what)]
        bad = sc.frames_differ(g.b, want, tp, both)
        assert bad is None, (g.name, what, bad)
        if allowed is None:
            allowed = _not_summed(g.b, g.chain) | set(also_out)
        left = set(ch.tolist()) - set(both.tolist())
        assert not strict or left <= allowed, (g.name, sorted(left - allowed)[:5])
        compared += len(both)
    return compared


def _changed(g, out):
    return sc.changed_frames(g.b, out)


# ---------------------------------------------------------------------------
# The shortcut the expected values are computed with
# ---------------------------------------------------------------------------
def test_apply_whats_is_apply():
    """rows_model.apply_whats edits once and sums only the frames the edits
    changed; rows_model.apply, the definition, sums every edited frame."""
    groups = [g for c in sc.CHAINS for g in rc.pieces64_groups(c)]
    groups += [g for c in sc.CHAINS for _, g in rc.delta_zero_groups(c)]
    groups += [g for c in sc.CHAINS for g, _, _ in rc.solved_groups(c)]
    groups += [g for c in sc.CHAINS for g in rc.still_groups(c)]
    groups += [g for g, _ in rc.guard_groups()[:10]] + list(rc.int_table_groups())
    groups += [g for c in (Chain.VlanUlp, TUN) for g in list(rc.wide_layer_groups(c))[::7]]
    assert len(groups) > 90
    for g in groups:
        outs, recs = rc.expected(g)
        for what, out in list(zip(g.whats, outs))[-2:]:
            want, w_rec = rc.definition(g, what)
            assert recs.tobytes() == w_rec.tobytes()
            assert out.tobytes() == want.tobytes(), (g.name, what)


# ---------------------------------------------------------------------------
# A. Narrow fields by packet and by row
# ---------------------------------------------------------------------------
@chains
def test_narrow_forms(chain):
    """Every field x layer x {SET, ADD, SUB} with the all-ones sweep value in
    both forms: a field the chain's layers can hold moves frames and no other
    does; guarded packets keep every byte; a SET reads back as the operand
    modulo 2^width (U16 zero-extended, U32 masked), an ADD as old + operand
    modulo 2^width; the sums equal rewrite + fill."""
    b = sc.batch(chain, "indexed")
    recs, outer = rc.headers(b, chain)
    compared = 0
    for field in Field:
        whats = (0,) if field in sc.REFUSED else (0, rc.full(chain))
        kind, first, bits = mrm.GEOMETRY[field]
        moved = 0
        for e in sc.sweep(chain, field, ops=(EditOp.SET, EditOp.ADD, EditOp.SUB)):
            if e[3] != 0xFFFFFFFF:
                continue
            for g in rc.sweep_forms(chain, b, e, whats):
                outs, g_rec = rc.expected(g)
                assert g_rec.tobytes() == recs.tobytes()
                ch = _changed(g, outs[0])
                if ch.size:
                    assert sc.applies(chain, e[0], field), g.name
                moved += int(ch.size > 0)
                if g.rows is not None:
                    assert not set(ch.tolist()) & set(np.nonzero(g.rows >= g.n_rows)[0].tolist())
                if field not in sc.CSUM_FIELDS and len(whats) > 1:
                    compared += _held(g, outs, recs, strict=False)
                if g.rows is not None or e[2] == EditOp.SUB:
                    continue
                operand = g.edits[0][3]
                assert operand.dtype == (np.uint16 if bits > 16 else np.uint32)
                for i in range(b.n):
                    if int(recs["status"][i]):
                        continue
                    have, h = mrm.header_at(chain, recs[i], None if outer is None else outer[i],
                                            e[0], e[4])
                    if have != kind:
                        continue
                    o = int(b.starts[i])
                    old = mrm.get_bits(b.arena[o:o + int(b.lengths[i])], 8 * h + first, bits)
                    new = mrm.get_bits(outs[0][o:o + int(b.lengths[i])], 8 * h + first, bits)
                    want = int(operand[i]) + (old if e[2] == EditOp.ADD else 0)
                    assert new == want % (1 << bits), (g.name, i)
        assert (moved > 0) == (field in sc.fields_of(chain)), (field, moved)
    assert compared > 1000, compared


# ---------------------------------------------------------------------------
# B. Wide fields
# ---------------------------------------------------------------------------
@chains
def test_wide_fields_at_every_layer(chain):
    """A layer the header names for the field moves frames; every other layer
    leaves every byte alone.  Sums: every `what` on the indexed batch, all sums
    on the slots."""
    compared = 0
    for g in rc.wide_layer_groups(chain):
        layer, wf = g.edits[0][0], g.edits[0][1]
        outs, recs = rc.expected(g)
        if not rc.holds(chain, layer, wf):
            for out in outs:
                assert out.tobytes() == g.b.arena.tobytes(), g.name
            continue
        assert _changed(g, outs[0]).size > 5, g.name
        compared += _held(g, outs, recs, None if " indexed " in g.name else (rc.full(chain),))
    assert compared > (500 if chain == Chain.UdpParser else 1500), compared


# Where the staged window can end inside an IPv6 address.  An indexed frame's
# window holds its first 48 - mis bytes (33..48); the IPv6 header starts at
# byte 14, 18 or 22 (0, 1 or 2 VLAN tags), its source 8 and its destination 24
# bytes further.  So the end lies 1..10 bytes into the destination (38 is its
# earliest start, 48 the latest end) and 3..15 bytes into the source (22 +
# 8 = 30 is its latest start, 33 the earliest end): those are all the positions
# there are, and the 16 placements reach every one of them.
REACHABLE = {V6D: set(range(1, 11)), V6S: set(range(3, 16))}


def test_the_window_ends_inside_the_addresses():
    seen = {V6S: set(), V6D: set()}
    tunnel = {V6S: set(), V6D: set()}
    for mis in range(16):
        for chain in (Chain.GenericUlp, Chain.VlanUlp):
            for (wf, _), pos in rc.window_ends(chain, mis).items():
                seen[wf] |= pos
        for (wf, layer), pos in rc.window_ends(TUN, mis).items():
            if layer == 5:
                tunnel[wf] |= pos
            else:
                assert not pos  # (the outer addresses lie inside the window)
    assert seen == REACHABLE, seen
    # the tunnel's 128-B window ends inside the inner destination at every
    # byte, and in the last 7 bytes of the inner source (the inner IPv6 header
    # of these frames starts at byte 84 at the earliest)
    assert tunnel[V6S] == set(range(9, 16)) and tunnel[V6D] == set(range(1, 16)), tunnel


@chains
def test_across_the_window(chain):
    compared = restored = 0
    for mis in range(16):
        b = sc.batch_at(chain, mis)
        for g, same in rc.window_groups(chain, b):
            outs, recs = rc.expected(g)
            compared += _held(g, outs, recs)
            if same:
                restored += 1
                for out in outs:
                    assert out.tobytes() == b.arena.tobytes(), (g.name, mis)
            elif chain != Chain.UdpParser or "MAC" in g.name:
                assert _changed(g, outs[0]).size > 0, (g.name, mis)
    assert restored >= 16 * 3 and compared > (100 if chain == Chain.UdpParser else 500), compared
    # set and restored over both representations of a zero sum
    b, zero, ones, udp = rc.edge_batch(chain)
    if chain != Chain.UdpParser:
        assert len(zero) >= 8 and len(ones) >= 8 and len(udp) >= 8
    for g, same in rc.window_groups(chain, b, restore_only=True):
        assert same
        for out in rc.expected(g)[0]:
            assert out.tobytes() == b.arena.tobytes(), g.name


@chains
def test_64_pieces(chain):
    for g in rc.pieces64_groups(chain):
        assert len(g.edits) == 16 and 4 * len(g.edits) == 64 and g.b.n == 65
        assert all(e[1] in (V6S, V6D) for e in g.edits)
        assert len({id(e[3][1] if isinstance(e[3], tuple) else e[3]) for e in g.edits}) == 16
        outs, recs = rc.expected(g)
        n = _held(g, outs, recs)
        assert n >= (5 if chain == Chain.UdpParser else 15), (g.name, n)
        if "00 / ff" in g.name:
            for e in g.edits:
                t = e[3][1] if isinstance(e[3], tuple) else e[3]
                assert set(np.unique(t)) == {0, 0xFF} and (t.min(axis=1) == t.max(axis=1)).all()


# ---------------------------------------------------------------------------
# C. Checksum value edges
# ---------------------------------------------------------------------------
def _by_kind(g, frames):
    kind = rc.kinds(g.b, g.chain)
    return dict(Counter("/".join(kind[i]) for i in frames))


# packets whose covered words changed while every sum field kept its bytes, by
# (L3, L4) kind (the tunnel: the inner kinds; its outer sum is covered too)
DELTA_ZERO = {"UdpParser": {"same": {},
                            "permuted": {"v4/udp": 20, "v6/udp": 12},
                            "swapped": {"v4/udp": 20, "v6/udp": 12},
                            "0000 to ffff": {"v6/udp": 12},
                            "ffff to 0000": {"v6/udp": 12}},
              "GenericUlp": {"same": {},
                             "permuted": {"v4/tcp": 16,
                                          "v4/udp": 20,
                                          "v4/icmp4": 12,
                                          "v6/tcp": 12,
                                          "v6/udp": 12,
                                          "v6/icmp6": 12},
                             "swapped": {"v4/tcp": 16,
                                         "v4/udp": 20,
                                         "v4/icmp4": 12,
                                         "v6/tcp": 12,
                                         "v6/udp": 12,
                                         "v6/icmp6": 12},
                             "0000 to ffff": {"v6/tcp": 12, "v6/udp": 12, "v6/icmp6": 12},
                             "ffff to 0000": {"v6/tcp": 12, "v6/udp": 12, "v6/icmp6": 12}},
              "VlanUlp": {"same": {},
                          "permuted": {"v4/tcp": 16,
                                       "v4/udp": 20,
                                       "v4/icmp4": 12,
                                       "v6/tcp": 12,
                                       "v6/udp": 12,
                                       "v6/icmp6": 12},
                          "swapped": {"v4/tcp": 16,
                                      "v4/udp": 20,
                                      "v4/icmp4": 12,
                                      "v6/tcp": 12,
                                      "v6/udp": 12,
                                      "v6/icmp6": 12},
                          "0000 to ffff": {"v6/tcp": 12, "v6/udp": 12, "v6/icmp6": 12},
                          "ffff to 0000": {"v6/tcp": 12, "v6/udp": 12, "v6/icmp6": 12}},
              "GeneveOverV6Tunnel": {"same": {},
                                     "permuted": {"v6/tcp": 30,
                                                  "v4/tcp": 56,
                                                  "v4/udp": 28,
                                                  "v6/udp": 2,
                                                  "v4/icmp4": 2,
                                                  "v6/icmp6": 2},
                                     "swapped": {"v6/tcp": 30,
                                                 "v4/tcp": 56,
                                                 "v4/udp": 28,
                                                 "v6/udp": 2,
                                                 "v4/icmp4": 2,
                                                 "v6/icmp6": 2},
                                     "0000 to ffff": {"v6/tcp": 30,
                                                      "v4/tcp": 56,
                                                      "v4/udp": 28,
                                                      "v6/udp": 2,
                                                      "v4/icmp4": 2,
                                                      "v6/icmp6": 2},
                                     "ffff to 0000": {"v6/tcp": 30,
                                                      "v4/tcp": 56,
                                                      "v4/udp": 28,
                                                      "v6/udp": 2,
                                                      "v4/icmp4": 2,
                                                      "v6/icmp6": 2}}}


@chains
def test_delta_of_zero_keeps_the_field(chain):
    b, zero, ones, udp = rc.edge_batch(chain)
    own = np.searchsorted(b.starts, np.array(ones, np.uint64), side="right") - 1
    counts = {}
    for way, g in rc.delta_zero_groups(chain):
        outs, recs = rc.expected(g)
        out = outs[0]
        fields = rc.sum_fields(g.b, chain)
        for at in fields[fields >= 0]:
            assert out[at:at + 2].tobytes() == g.b.arena[at:at + 2].tobytes(), (g.name, at)
        if way == "same":
            assert out.tobytes() == g.b.arena.tobytes()
        # both representations are among the fields that were kept
        assert all(out[a] == 0 and out[a + 1] == 0 for a in zero)
        assert all(out[a] == 0xFF and out[a + 1] == 0xFF for a in ones + udp)
        counts[way] = _by_kind(g, _changed(g, out))
        _held(g, outs, recs, also_out=own.tolist())
    assert counts == DELTA_ZERO[chain.name], counts


# packets whose solved word put the named sum's field on each edge, by kind
SOLVED = {"UdpParser": {"L4 through the source: computed 0": {"v6/udp": 4},
                        "L4 through the source: 0x0001": {"v6/udp": 4},
                        "L4 through the source: 0xfffe": {"v6/udp": 4}},
          "GenericUlp": {"L4 through the source: computed 0": {"v6/tcp": 4,
                                                               "v6/udp": 4,
                                                               "v6/icmp6": 4},
                         "L4 through the source: 0x0001": {"v6/tcp": 4,
                                                           "v6/udp": 4,
                                                           "v6/icmp6": 4},
                         "L4 through the source: 0xfffe": {"v6/tcp": 4,
                                                           "v6/udp": 4,
                                                           "v6/icmp6": 4}},
          "VlanUlp": {"L4 through the source: computed 0": {"v6/tcp": 4,
                                                            "v6/udp": 4,
                                                            "v6/icmp6": 4},
                      "L4 through the source: 0x0001": {"v6/tcp": 4, "v6/udp": 4, "v6/icmp6": 4},
                      "L4 through the source: 0xfffe": {"v6/tcp": 4, "v6/udp": 4, "v6/icmp6": 4}},
          "GeneveOverV6Tunnel": {"L4 through the source: computed 0": {"v6/tcp": 9,
                                                                       "v6/icmp6": 1},
                                 "L4 through the source: 0x0001": {"v6/tcp": 10, "v6/udp": 1},
                                 "L4 through the source: 0xfffe": {"v6/tcp": 9,
                                                                   "v6/icmp6": 1,
                                                                   "v6/udp": 1},
                                 "outer through an outer address: computed 0": {"v6/tcp": 9,
                                                                                "v4/udp": 10,
                                                                                "v4/tcp": 18,
                                                                                "v4/icmp4": 1,
                                                                                "v6/icmp6": 1},
                                 "outer through an outer address: 0x0001": {"v4/tcp": 20,
                                                                            "v6/tcp": 10,
                                                                            "v6/udp": 1,
                                                                            "v4/udp": 9},
                                 "outer through an outer address: 0xfffe": {"v4/tcp": 18,
                                                                            "v4/udp": 9,
                                                                            "v6/tcp": 9,
                                                                            "v4/icmp4": 1,
                                                                            "v6/icmp6": 1,
                                                                            "v6/udp": 1},
                                 "outer through an inner MAC: computed 0": {"v6/tcp": 9,
                                                                            "v4/udp": 10,
                                                                            "v4/tcp": 18,
                                                                            "v4/icmp4": 1,
                                                                            "v6/icmp6": 1},
                                 "outer through an inner MAC: 0x0001": {"v4/tcp": 20,
                                                                        "v6/tcp": 10,
                                                                        "v6/udp": 1,
                                                                        "v4/udp": 9},
                                 "outer through an inner MAC: 0xfffe": {"v4/tcp": 18,
                                                                        "v4/udp": 9,
                                                                        "v6/tcp": 9,
                                                                        "v4/icmp4": 1,
                                                                        "v6/icmp6": 1,
                                                                        "v6/udp": 1},
                                 "inner L4 under an outer sum of 0: computed 0": {"v6/tcp": 5},
                                 "inner L4 under an outer sum of 0: 0x0001": {"v6/tcp": 5,
                                                                              "v6/udp": 1},
                                 "inner L4 under an outer sum of 0: 0xfffe": {"v6/tcp": 4,
                                                                              "v6/icmp6": 1}}}


@chains
def test_solved_addresses_land_on_the_edges(chain):
    counts = {}
    for g, which, hit in rc.solved_groups(chain):
        outs, recs = rc.expected(g)
        out = outs[0]
        fields = rc.sum_fields(g.b, chain)
        kind = rc.kinds(g.b, chain)
        for target, frames in hit.items():
            _, udp_bytes, other_bytes = rc.TARGETS[target]
            for i in frames:
                at = int(fields[i, which])
                is_udp = which == 2 or kind[i][1] == "udp"
                assert out[at:at + 2].tobytes() == (udp_bytes if is_udp else other_bytes), \
                    (g.name, target, i)
            key = g.name.split(": ")[1].rsplit(" by ", 1)[0] + ": " + target
            assert counts.setdefault(key, _by_kind(g, frames)) == _by_kind(g, frames)
        if "under an outer sum of 0" in g.name:
            # the inner field moved to its edge, the address words and that
            # field cancel in the outer sum: its 0xffff is kept
            for i in np.concatenate(list(hit.values())):
                at = int(fields[i, 2])
                assert g.b.arena[at:at + 2].tobytes() == out[at:at + 2].tobytes() == b"\xff\xff"
        _held(g, outs, recs)
    assert counts == SOLVED[chain.name], counts


# still_batch's packets by what must happen to their L4 (the tunnel: and outer
# UDP) field under the address edits, by kind
STILL = {"UdpParser": {"L4 stays": {"v4/udp": 6, "v6/udp": 3},
                       "L4 moves": {"v4/udp": 4, "v6/udp": 3}},
         "GenericUlp": {"L4 stays": {"v4/icmp4": 6, "v4/udp": 6, "v6/udp": 3},
                        "L4 moves": {"v4/tcp": 8,
                                     "v4/udp": 4,
                                     "v6/tcp": 6,
                                     "v6/udp": 3,
                                     "v6/icmp6": 6}},
         "VlanUlp": {"L4 stays": {"v4/icmp4": 12, "v4/udp": 12, "v6/udp": 6},
                     "L4 moves": {"v4/tcp": 16,
                                  "v4/udp": 8,
                                  "v6/tcp": 12,
                                  "v6/udp": 6,
                                  "v6/icmp6": 12}},
         "GeneveOverV6Tunnel": {"L4 stays": {"v4/icmp4": 2},
                                "L4 moves": {"v6/tcp": 30,
                                             "v4/tcp": 56,
                                             "v4/udp": 28,
                                             "v6/udp": 2,
                                             "v6/icmp6": 2}}}


@chains
def test_sums_that_must_not_move(chain):
    b, zeroed = rc.still_batch(chain)
    (g,) = rc.still_groups(chain)
    outs, recs = rc.expected(g)
    out = outs[g.whats.index(rc.full(chain))]
    fields = rc.sum_fields(b, chain)
    kind = rc.kinds(b, chain)
    l3_off = recs["l3_off"]
    ch = set(_changed(g, outs[0]).tolist())
    stay, move = [], []
    for i in sorted(ch):
        at = int(fields[i, 1])
        if at < 0:
            continue
        flags_at = int(b.starts[i]) + int(l3_off[i]) + 6
        frag = kind[i][0] == "v4" and rc.be16(b.arena, flags_at) & 0x1FFF
        zero = kind[i][1] == "udp" and rc.be16(b.arena, at) == 0
        kept = out[at:at + 2].tobytes() == b.arena[at:at + 2].tobytes()
        # the header: ICMPv4 has no pseudo-header, a later fragment's bytes are
        # no L4 header, a UDP field of 0 stays 0; a first fragment (MF set,
        # offset 0) IS updated, though fill does not sum it
        if kind[i][1] == "icmp4" or frag or zero:
            assert kept, (i, kind[i])
            stay.append(i)
        else:
            # (new addresses of random bytes: a delta of 0 mod 0xffff does not occur)
            assert not kept, (i, kind[i])
            move.append(i)
    counts = {"L4 stays": _by_kind(g, stay), "L4 moves": _by_kind(g, move)}
    if chain == TUN:
        assert set(zeroed.tolist()) <= ch and len(zeroed) == 59  # (one is a fragment)
        for i in range(b.n):
            at = int(fields[i, 2])
            assert (out[at:at + 2].tobytes() == b"\x00\x00") == (i in set(zeroed.tolist())), i
            assert i in zeroed or out[at:at + 2].tobytes() != b.arena[at:at + 2].tobytes(), i
    else:
        assert all(kind[i][1] == "udp" for i in zeroed) and set(zeroed.tolist()) <= set(stay)
        assert {kind[i][0] for i in zeroed} == ({"v4", "v6"})
    assert counts == STILL[chain.name], counts
    _held(g, outs, recs)


# ---------------------------------------------------------------------------
# D. Tables and rows (the model indexes a table by row; pitch is the ABI's)
# ---------------------------------------------------------------------------
def test_tables():
    groups = list(rc.byte_table_groups()) + list(rc.int_table_groups())
    assert len(groups) == 4 * 4 * 2 + 3
    compared = 0
    for g in groups:
        outs, recs = rc.expected(g)
        compared += _held(g, outs, recs)
        # the same operands as dense copies
        dense = [(*e[:3], ("row", np.ascontiguousarray(e[3][1])) if isinstance(e[3], tuple)
                  else np.ascontiguousarray(e[3]), *e[4:]) for e in g.edits]
        assert rc.expected(g._replace(edits=dense))[0][0].tobytes() == outs[0].tobytes()
        for e in g.edits:  # where the tables sit: what the device is to see
            t = e[3][1] if isinstance(e[3], tuple) else e[3]
            if g.name.startswith("byte tables"):
                at = int(g.name.split(" mod 4")[0][-1])
                root = rc.cases._root(t)
                assert (t.__array_interface__["data"][0] -
                        root.__array_interface__["data"][0]) % 4 == at
    assert compared > 2000, compared


def test_the_row_guard():
    groups = rc.guard_groups()
    assert len(groups) == 4 * 5 + 1
    for g, guarded in groups:
        outs, recs = rc.expected(g)
        out = outs[0]
        ch = set(_changed(g, out).tolist())
        assert not ch & set(guarded.tolist()), g.name
        if g.n_rows == 0:
            assert out.tobytes() == g.b.arena.tobytes() and len(guarded) == g.b.n
        else:
            # every other packet has a MAC of random bytes written
            assert ch == set(range(g.b.n)) - set(guarded.tolist()), g.name
        if "edges" in g.name and g.b.n >= 63:
            assert set(g.rows.tolist()) == {0, 36, 37, 0x7FFFFFFF, 0x80000000, ROW_NONE}
        if "one row" in g.name:
            assert len(set(g.rows.tolist())) == 1 and not len(guarded)
        _held(g, outs, recs)
    big = groups[-1][0]
    assert big.n_rows == 1 << 20 and big.b.n == 300 and len(groups[-1][1]) == 2
    assert {0, (1 << 20) - 1} <= set(big.rows.tolist())
