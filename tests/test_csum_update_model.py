"""The incremental checksum update's definition (tests/csum_update_model.py)
against RFC 1624's example, the hand-built vectors of
tests/golden/csum_update_kats.json (tests/golden/make_csum_update_kats.py wrote
it) and the two-pass way, rewrite + fill (tests/csum_model.py), on generated
traffic; and the C ABI of ingot_gpu_parse_modify_csum without a GPU."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

import oracle
from ingot_amd import _lib, abi
from ingot_amd.abi import CSUM_L3, CSUM_L4, CSUM_OUTER_L4, Chain, EditOp, Field, GenProfile
from ingot_amd.hostgen import gen_frames_host
from tests import csum_frames as cf
from tests import csum_model as model
from tests import csum_update_model as upd

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "csum_update_kats.json").read_text())
NONE, OK = 0, 1

# the issue's eight edits (GenericUlp: 1 = l3, 2 = l4)
EDITS = [(1, Field.V4_HOP_LIMIT, EditOp.SUB, 1), (1, Field.V4_SOURCE, EditOp.SET, 0x0A000001),
         (1, Field.V4_DESTINATION, EditOp.XOR, 0x00FF00FF),
         (2, Field.UDP_DESTINATION, EditOp.SUB, 1), (2, Field.TCP_SOURCE, EditOp.SET, 0),
         (2, Field.TCP_FLAGS, EditOp.OR, 0x10), (1, Field.V4_DSCP, EditOp.SET, 0x2E),
         (1, Field.V6_HOP_LIMIT, EditOp.SUB, 1)]


def kat_edits(k):
    return [(e[0], Field[e[1]], EditOp[e[2]], e[3]) for e in k["edits"]]


def model_run(f: bytes, chain: Chain, edits, what: int) -> bytes:
    arena, off, lens = cf.place([f])
    after = arena.copy()
    recs = oracle.parse_modify_batch(after, off, lens, chain, edits)
    o_udp = None
    if chain == Chain.GeneveOverV6Tunnel:
        o_udp = oracle.geneve_fields_batch(arena, off, lens)["outer"]["outer_udp_off"]
    upd.update(arena, after, off, lens, recs, what, o_udp=o_udp)
    assert after[len(f):].tobytes() == arena[len(f):].tobytes()  # nothing past the frame
    return after[:len(f)].tobytes()


def test_rfc1624_section4_example():
    v = {k: int(x, 16) for k, x in KATS["rfc1624_section4"].items()}
    assert (v["hc"], v["m"], v["m_new"], v["hc_new"]) == (0xDD2F, 0x5555, 0x3285, 0x0000)
    d = ((~v["m"] & 0xFFFF) + v["m_new"]) % 0xFFFF
    assert upd.eqn3(v["hc"], d) == v["hc_new"]
    # eqn. 3 never yields 0xffff (the sum is taken in [1, 0xffff]), where eqn. 2 would
    assert all(upd.eqn3(hc, dd) != 0xFFFF for hc in (0, 1, 0xDD2F, 0xFFFE, 0xFFFF)
               for dd in (1, 2, 0x7FFF, 0xFFFE))
    b = np.frombuffer(bytes.fromhex("55550000"), dtype=np.uint8)
    a = np.frombuffer(bytes.fromhex("32850000"), dtype=np.uint8)
    assert upd.delta(b, a, [(0, 4)], 2) == d


def test_kats_cover_the_cases():
    names = {k["name"] for k in KATS["frames"]}
    assert len(names) == len(KATS["frames"]) >= 24
    assert {k["what"] for k in KATS["frames"]} >= {1, 2, 3, 4, 7}
    assert {k["chain"] for k in KATS["frames"]} == {"GenericUlp", "VlanUlp", "GeneveOverV6Tunnel"}


@pytest.mark.parametrize("k", KATS["frames"], ids=lambda k: k["name"])
def test_model_reproduces_the_kats(k):
    f, chain = bytes.fromhex(k["frame"]), Chain[k["chain"]]
    got = model_run(f, chain, kat_edits(k), k["what"])
    assert got.hex() == k["after"]
    if k["fill_equal"]:
        # the two-pass way: rewrite, then fill (a tunnel frame: inner, then outer)
        a = np.frombuffer(oracle.parse_modify(f, chain, kat_edits(k))[0], dtype=np.uint8).copy()
        model.one(a, oracle.parse_batch(*cf.place([a.tobytes()])[:3], chain)[0], 3, True)
        if chain == Chain.GeneveOverV6Tunnel:
            model.one(a, oracle.parse_batch(*cf.place([a.tobytes()])[:3], Chain.UdpParser)[0],
                      2, True)
        assert got == a.tobytes()


def mixed_valid(n=2000, seed=31):
    """MIXED frames with every checksum the model sums made valid, and the
    rows of that fill."""
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=seed, slack=64)
    recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    rows = model.fill(arena, off, lens, recs)
    return arena, off, lens, rows


def test_update_equals_rewrite_plus_fill_on_mixed_traffic():
    arena, off, lens, rows = mixed_valid()
    n = len(off)
    after = arena.copy()
    recs = oracle.parse_modify_batch(after, off, lens, Chain.GenericUlp, EDITS)
    two_pass = after.copy()
    upd.update(arena, after, off, lens, recs, CSUM_L3 | CSUM_L4)
    model.fill(two_pass, off, lens, recs)
    keep = (rows["l4_state"] == OK) & ((rows["l3_state"] == OK) | (rows["l3_state"] == NONE))
    print("compared", int(keep.sum()), "of", n)
    assert keep.sum() >= 0.9 * n  # 1,908 of 2,000; the rest are IPv6 fragments
    kinds = set()
    for i in np.nonzero(keep)[0]:
        o, ln = int(off[i]), int(lens[i])
        assert after[o:o + ln].tobytes() == two_pass[o:o + ln].tobytes(), i
        kinds.add((int(recs[i]["l3_kind"]), int(recs[i]["l4_kind"])))
    assert {(1, 1), (1, 2), (2, 1), (2, 2)} <= kinds  # v4 / v6 x TCP / UDP were compared
    assert (after != arena).any()


def test_model_argument_checks():
    arena, off, lens = cf.place([bytes.fromhex(KATS["frames"][0]["frame"])])
    recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    for what in (0, 8, 0x10):
        with pytest.raises(ValueError):
            upd.update(arena, arena.copy(), off, lens, recs, what)
    with pytest.raises(ValueError):
        upd.update(arena, arena.copy(), off, lens, recs, CSUM_OUTER_L4)  # no offsets given


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ingot_amd.build import build

    build()
    return _lib.load()


def test_parse_modify_csum_argument_validation_without_gpu(lib):
    assert abi.CSUM_OUTER_L4 == 4
    fn = lib.ingot_gpu_parse_modify_csum
    e = abi.edits_array(EDITS)
    ep = e.ctypes.data_as(ctypes.c_void_p)
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(1)
    G, TUN = int(Chain.GenericUlp), int(Chain.GeneveOverV6Tunnel)
    assert fn(null, None, None, None, 64, 10, G, ep, len(e), 3, None, None) == -1  # NULL context
    # refused before the context is looked at more closely:
    for what in (0, 8, 9, 0x80000001):
        assert fn(fake, None, None, None, 64, 0, G, ep, len(e), what, None, None) == -1, what
    # the outer sum exists on the tunnel chain only
    assert fn(fake, None, None, None, 64, 0, G, ep, len(e), CSUM_OUTER_L4, None, None) == -1
    assert fn(fake, None, None, None, 64, 0, G, ep, len(e), 7, None, None) == -1
    tun = abi.edits_array([(5, Field.V4_HOP_LIMIT, EditOp.SUB, 1)])
    tp = tun.ctypes.data_as(ctypes.c_void_p)
    assert fn(fake, None, None, None, 64, 0, TUN, tp, 1, 7, None, None) == 0  # n == 0
    # fields that move a sum's extent or its pseudo-header
    for f in (Field.V4_IHL, Field.V4_TOTAL_LEN, Field.V4_PROTOCOL, Field.V6_PAYLOAD_LEN,
              Field.V6_NEXT_HEADER):
        bad = abi.edits_array([EDITS[0], (1, f, EditOp.SET, 5)])
        bp = bad.ctypes.data_as(ctypes.c_void_p)
        assert fn(fake, None, None, None, 64, 0, G, bp, 2, 3, None, None) == -1, f
        # ... which the plain rewrite takes
        assert lib.ingot_gpu_parse_modify(fake, None, None, None, 64, 0, G, bp, 2, None,
                                          None) == 0, f
    # parse_modify's own checks hold: too many edits, a layer the chain lacks
    assert fn(fake, None, None, None, 64, 0, G, ep, 17, 3, None, None) == -1
    far = abi.edits_array([(3, Field.V4_HOP_LIMIT, EditOp.SUB, 1)])
    assert fn(fake, None, None, None, 64, 0, G, far.ctypes.data_as(ctypes.c_void_p), 1, 3, None,
              None) == -1
    assert fn(fake, None, None, None, 64, 0, G, ep, len(e), 3, None, None) == 0  # n == 0
