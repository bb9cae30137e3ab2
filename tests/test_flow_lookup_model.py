"""The flow key's definition (tests/flow_lookup_model.py) pinned to the oracle:
a packet has a key exactly when oracle.flow_hist counts it, and words 0-8 are
the words the oracle's Toeplitz hash was computed over.  Then the shape of the
shared lookup case.  No GPU."""
import numpy as np
import pytest

import oracle
from ingot_amd.abi import ROW_NONE, Chain, GenProfile, L3Kind
from tests import flow_lookup_cases as cases
from tests import flow_lookup_model as model

FLOW_NONE = 0xFFFFFFFF
PROFILES = [GenProfile.ADVERSARIAL, GenProfile.MIXED, GenProfile.VLAN_V6EH, GenProfile.FLOWS,
            GenProfile.GENEVE, GenProfile.GENEVE_ADVERSARIAL]


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("chain", list(Chain))
def test_keys_are_the_oracles_hash_input(chain, profile):
    n = 600
    arena, off, lens = cases.placed(profile, n)
    k, recs = model.keys(arena, off, lens, chain)
    _, hashes = oracle.flow_hist(arena, off, lens, chain)
    counted = oracle.flow_hist.last_flows != FLOW_NONE
    assert (model.has_key(k) == counted).all()
    assert not k[~counted].any()  # the sentinel: 40 zero bytes
    for i in np.nonzero(counted)[0]:
        # zero words do not move a Toeplitz hash: all nine, as 36 bytes
        data = b"".join(int(w).to_bytes(4, "big") for w in k[i, :9])
        assert oracle.toeplitz(oracle.RSS_KEY, data) == hashes[i], i
        assert k[i, 9] == (int(recs["l3_kind"][i]) << 8) | int(recs["l4_proto"][i])
        assert k[i, 9] >> 8 in (L3Kind.IPV4, L3Kind.IPV6)
    # (UdpParser refuses TCP and the tunnel chain refuses plain frames)
    if profile in (GenProfile.MIXED, GenProfile.FLOWS) and chain in (Chain.GenericUlp,
                                                                     Chain.VlanUlp):
        assert counted.sum() > n // 2
    if profile == GenProfile.GENEVE and chain == Chain.GeneveOverV6Tunnel:
        assert counted.sum() > n // 2 and (recs["flags"][counted] & 2).all()  # inner layers


def test_ipv4_words_past_the_ports_are_zero():
    arena, off, lens = cases.placed(GenProfile.FLOWS, 600)
    k, recs = model.keys(arena, off, lens, Chain.GenericUlp)
    v4 = recs["l3_kind"] == L3Kind.IPV4
    assert v4.any() and not k[v4][:, 3:9].any()


def test_main_case_has_every_class():
    c = cases.main_case()
    assert c.n == 20000
    hit, no_key = c.hit, c.no_key
    miss = np.zeros(c.n, bool)
    miss[c.miss] = True
    assert not (hit & no_key).any() and not (hit & miss).any() and not (miss & no_key).any()
    assert (hit | miss | no_key).all()
    assert hit.sum() >= 64 and miss.sum() >= 64 and no_key.sum() >= 64
    # hits in the second half too (a flow of the first half seen again)
    assert hit[c.n // 2:].sum() >= 1
    assert (c.rows[~hit] == ROW_NONE).all() and (c.rows[hit] < cases.MAIN_ROWS).all()
    # rows are per key: equal keys, equal rows; different keys, different rows
    by_key = {}
    for x, r in zip(c.keys[hit], c.rows[hit]):
        assert by_key.setdefault(x.tobytes(), int(r)) == int(r)
    assert len(set(by_key.values())) == len(by_key) == len(c.tab_keys)


def test_lookup_model_last_row_wins():
    k = np.array([cases.key4(1, 2, 3, 4), cases.key4(1, 2, 3, 5), cases.key4(1, 2, 3, 4)],
                 dtype=np.uint32)
    tab = model.table(k, [7, 8, 9])
    probe = np.vstack([k[:2], cases.key4(9, 9, 9, 9)[None], np.zeros((1, 10), np.uint32)])
    rows, miss = model.lookup(probe, tab)
    assert rows.tolist() == [9, 8, ROW_NONE, ROW_NONE] and miss.tolist() == [2]
