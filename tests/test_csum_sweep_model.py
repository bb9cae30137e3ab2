"""The cases of tests/csum_sweep_cases.py on the references alone (no GPU):
what tests/test_modify_csum_sweep.py and tests/test_emit_csum_edges.py compare
the device with is held here to a second, independent way of computing it.

Rewrite: every field is moved by some sweep case; the definition
(oracle.parse_modify_batch + csum_update_model.update) equals rewrite +
csum_model.fill on every frame that fill sums before and after the rewrite;
such frames are at least 0.75 of each batch, except where written below.
Emit: the crafted packets' fields hold the bytes they were built for, and a
byte-wise receiver accepts every datagram.
"""
import numpy as np
import pytest

import oracle
from ingot_amd import Chain, EditOp, EmitSum, Field
from ingot_amd.abi import CSUM_L3, CSUM_L4
from tests import csum_model
from tests import csum_sweep_cases as sc
from tests import csum_update_model as upd
from tests import emit_csum_cases as ecases

F, TUN = Field, sc.TUN
LAYOUTS = ("indexed", "strided")
chains = pytest.mark.parametrize("chain", sc.CHAINS, ids=lambda c: c.name)

# (field, layer) pairs left out of the 0.75 floor; the definition comparison
# still applies to whatever frames qualify.  None = every chain and layer.
FLOOR_EXCEPTIONS = {
    # every IPv4 frame becomes a fragment (offset != 0), which fill does not sum
    (F.V4_FRAGMENT_OFFSET, None): "turns IPv4 frames into fragments",
    # MF (bit 0 of the 3-bit field) set: a first fragment
    (F.V4_FLAGS, None): "sets MF on IPv4 frames: fragments",
    # the two-pass outer fill parses the rewritten frame as UdpParser: an
    # outer ethertype or IP version that is no longer IPv6 stops that parse
    (F.ETH_ETHERTYPE, 0): "tunnel: the outer parse of the two-pass way fails",
    (F.V6_VERSION, 1): "tunnel: the outer parse of the two-pass way fails",
}


def _excepted(chain, field, layer):
    if (field, None) in FLOOR_EXCEPTIONS:
        return True
    return chain == TUN and (field, layer) in FLOOR_EXCEPTIONS


def test_field_table_names_every_field():
    assert set(sc.FIELD_BITS) == set(Field) and len(Field) == 48
    assert set(sc.ALLOWED) | set(sc.REFUSED) == set(Field) and len(sc.REFUSED) == 5
    held = set()
    for chain in sc.CHAINS:
        held |= set(sc.fields_of(chain))
    assert held == set(Field)
    # the widths are the setters' own: a field set to all-ones reads back as
    # 2^bits - 1 through the oracle's field blocks for a sample of them
    for f, name in ((F.V4_DSCP, "v4_dscp"), (F.V4_FLAGS, "v4_flags"),
                    (F.V4_FRAGMENT_OFFSET, "v4_fragment_offset"), (F.V4_ECN, "v4_ecn_raw")):
        frame = sc.frame_kinds()[0]
        out, _ = oracle.parse_modify(frame, Chain.GenericUlp, [(1, f, EditOp.SET, 0xFFFFFFFF)])
        _, fld = oracle.parse_one(out, Chain.GenericUlp)
        assert int(fld[name]) == (1 << sc.FIELD_BITS[f]) - 1, name


@chains
def test_every_field_is_moved(chain):
    """Plain rewrite over all 48 fields: a field of the chain's headers that no
    (layer, op, value) moves on any frame is a hole in the batch."""
    for layout in LAYOUTS:
        b = sc.batch(chain, layout)
        moved = set()
        for field in Field:
            for e in sc.sweep(chain, field):
                _, rewritten, recs, ch = sc.define(b, chain, [e], 0)
                if ch.size:
                    assert sc.applies(chain, e[0], field), sc.tag(chain, layout, e, 0)
                    moved.add(field)
                    break
        assert moved == set(sc.fields_of(chain)), (layout, set(sc.fields_of(chain)) - moved)


@chains
def test_definition_equals_two_pass(chain):
    """Every sweep case with all the chain's sums selected (the device tests
    take every `what`): on the qualifying frames the definition is rewrite +
    fill, byte for byte.  The tunnel's slots hold the same frames as its
    indexed batch (padded) and are left to the device test."""
    compared = cases = 0
    for layout in LAYOUTS[:1] if chain == TUN else LAYOUTS:
        b = sc.batch(chain, layout)
        for field in sc.ALLOWED:
            for e in sc.sweep(chain, field):
                rewritten, recs, ch, q = None, None, None, None
                for what in sc.WHATS[chain][-1:]:
                    want, rewritten, recs, ch = sc.define(b, chain, [e], what)
                    if q is None:
                        q = sc.qualifies(b, chain, [e], rewritten, recs, ch)
                        if field not in sc.CSUM_FIELDS and not _excepted(chain, field, e[0]):
                            assert q.sum() >= 0.75 * b.n, (sc.tag(chain, layout, e, what),
                                                           int(q.sum()), b.n)
                    if not ch.size:
                        assert want.tobytes() == b.arena.tobytes()
                        continue
                    cases += 1
                    both = ch[q[ch]]
                    tp = sc.two_pass(b, chain, rewritten, recs, ch, what)
                    bad = sc.frames_differ(b, want, tp, both)
                    assert bad is None, (sc.tag(chain, layout, e, what), bad)
                    compared += len(both)
    floor = {Chain.UdpParser: 3_000}.get(chain, 9_000)  # (the issue's CPU run: 9,950, tunnel)
    assert compared > floor and cases > 500, (compared, cases)


@chains
def test_dependent_lists(chain):
    for layout in LAYOUTS:
        for name, edits, prepared in sc.dependent_lists(chain):
            b = sc.batch(chain, layout, prepared)
            zero = ones = udp = ()
            if prepared:
                b, zero, ones, udp = sc.other_repr(b, chain)
                if chain != Chain.UdpParser or layout == "strided":
                    assert len(zero) >= 8 and len(ones) >= 8 and len(udp) >= 8
            for what in sc.WHATS[chain]:
                t = (name, sc.tag(chain, layout, edits, what))
                want, rewritten, recs, ch = sc.define(b, chain, edits, what)
                q = sc.qualifies(b, chain, edits, rewritten, recs, ch)
                tp = sc.two_pass(b, chain, rewritten, recs, ch, what)
                if prepared:
                    # the prepared batch holds IPv4 sums in the 0xffff
                    # representation, which fill rewrites as 0x0000: those
                    # frames are compared with the definition only
                    own = np.searchsorted(b.starts, np.array(ones, np.uint64), side="right") - 1
                    q[own] = False
                assert sc.frames_differ(b, want, tp, ch[q[ch]]) is None, t
                if name.startswith("inverse"):
                    # an edit and its inverse: nothing moves, no field is written
                    assert want.tobytes() == b.arena.tobytes(), t
                    assert all(want[a] == 0 and want[a + 1] == 0 for a in zero), t
                    assert all(want[a] == 0xFF and want[a + 1] == 0xFF for a in ones), t
                    assert all(want[a] == 0xFF and want[a + 1] == 0xFF for a in udp), t
                elif any(sc.applies(chain, e[0], e[1]) for e in edits):
                    assert ch.size > 0, t


@chains
def test_shortcut_equals_full_update(chain):
    """define() updates only the frames the rewrite changed; the random lists
    hold that to csum_update_model.update over the whole batch."""
    touched = 0
    for layout in LAYOUTS:
        b = sc.batch(chain, layout)
        what = sc.WHATS[chain][-1]
        for edits in sc.random_lists(chain)[::4]:
            assert 1 <= len(edits) <= 16
            want, rewritten, recs, ch = sc.define(b, chain, edits, what)
            full = upd.update(b.arena, rewritten.copy(), b.starts, b.lengths, recs, what,
                              o_udp=b.o_udp)
            assert want.tobytes() == full.tobytes(), sc.tag(chain, layout, edits, what)
            touched += int(ch.size > 0)
    assert touched >= 60, touched


# ---------------------------------------------------------------------------
# Crafted emit cases
# ---------------------------------------------------------------------------
def _receiver(c: sc.EmitCase, got):
    """Every datagram (S <= 65,535) is accepted: packets that fit a 16-bit
    frame length through oracle.parse_batch + csum_model.verify, longer ones
    through the byte-wise sum of csum_sweep_cases."""
    H = len(c.hdr)
    tot = c.lens.astype(np.int64) + H
    vlan = c.hdr[12:14] == b"\x81\x00"
    chain = Chain.VlanUlp if vlan else Chain.GenericUlp
    fits = tot <= 65535
    idx = np.nonzero(fits)[0]
    recs = oracle.parse_batch(got, c.dst_off[idx], tot[idx].astype(np.uint16), chain)
    assert (recs["status"] == 0).all(), c.name
    rows = csum_model.verify(got, c.dst_off[idx], tot[idx].astype(np.uint16), recs,
                             CSUM_L3 | CSUM_L4)
    named_v4 = any(int(s[0]) == int(EmitSum.IPV4) for s in c.sums)
    bad = np.nonzero(rows["l4_state"] != sc.OK)[0]
    assert bad.size == 0, (c.name, idx[bad][:5], rows[bad][:5])
    if named_v4:
        assert (rows["l3_state"] == sc.OK).all(), c.name
    else:
        assert np.isin(rows["l3_state"], (sc.OK, sc.NONE)).all(), c.name
    u_at = sc._udp_sum(c.sums)[1]
    for k in np.nonzero(~fits)[0]:
        o = int(c.dst_off[k])
        if tot[k] - u_at <= 65535:
            assert sc.bytewise_receiver_ok(got[o:o + int(tot[k])], c.hdr, c.sums), (c.name, k)


@pytest.mark.parametrize("name", ecases.STACKS)
def test_emit_computed_zero(name):
    seen = set()
    for dmis in (0, 5, 15):  # (all 16 run on the device; the model has no alignment)
        for c in sc.computed_zero_cases(name, dmis):
            assert len(c.checks) == 6 and {k for k, *_ in c.checks} == set(sc.CRAFTED_AT)
            assert all(int(c.dst_off[k]) % 16 == dmis for k, *_ in c.checks)
            got = sc.emit_model(c)
            sc.held(c, got)
            _receiver(c, got)
            seen |= {(note, want) for _, _, want, note in c.checks}
    assert len(seen) == 12 and {w for _, w in seen} == {b"\xff\xff", b"\x00\x01", b"\xff\xfe"}


@pytest.mark.parametrize("name", ["geneve_v4", "vlan_v4opt"])
def test_emit_ipv4_zero(name):
    c = sc.ipv4_zero_case(name)
    got = sc.emit_model(c)
    assert sorted(w for _, _, w, _ in c.checks) == [b"\x00\x00"] * 2 + [b"\x00\x01"] * 2 + \
        [b"\xff\xfe"] * 2
    sc.held(c, got)
    _receiver(c, got)


@pytest.mark.parametrize("name", ecases.STACKS)
def test_emit_largest_sums(name):
    c = sc.largest_sum_case(name, 1, 5)
    u_at = sc._udp_sum(c.sums)[1]
    S = len(c.hdr) - u_at + c.lens.astype(np.int64)
    assert {65534, 65535, 65536} <= set(S.tolist()) and len(c.checks) == 4
    got = sc.emit_model(c)
    sc.held(c, got)
    _receiver(c, got)


@pytest.mark.parametrize("name", sc.BIG_STACKS)
def test_emit_big_headers(name):
    c = sc.big_header_case(name)
    hdr, sets, sums = c.hdr, c.sets, c.sums
    if name != "v6_dstopts":
        assert len(hdr) == 254 and len(sets) == 8
    if name == "vlan_v6_hbh":
        assert sums == [(EmitSum.UDP, 234, 18)]
    got = sc.emit_model(c)
    # the setter's value on a named checksum field is overridden
    _receiver(c, got)
