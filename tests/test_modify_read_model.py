"""The definition of the rewrite over chunked packets
(tests/modify_read_model.py) without a GPU: its setter and checksum update
are pinned against the oracle's contiguous rewrite + tests/csum_update_model.py
on every Ok packet whose chunked record equals the contiguous record of its
logical frame (single-chunk packets: the whole single-edit sweep; the six cut
sets: no Ok packet may be left out), the IPv6 cut that is not Ok keeps every
byte, and the C ABI of the two calls."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
from ingot_amd import _lib
from ingot_amd.abi import Chain, Field
from tests import csum_frames as cf
from tests import csum_read_cases as cases
from tests import csum_sweep_cases as sc
from tests import modify_read_cases as mc
from tests import modify_read_model as model

ROOT = Path(__file__).resolve().parent.parent
TUN = Chain.GeneveOverV6Tunnel
N_CUT = 5_000
chains = pytest.mark.parametrize("chain", sc.CHAINS, ids=lambda c: c.name)


def test_geometry_table_is_the_setters():
    """Header kind and width per field as tests/csum_sweep_cases.py has them
    (the first bits are held by the sweep below: a wrong one moves other
    bytes than the oracle's setter)."""
    assert {f: g[2] for f, g in model.GEOMETRY.items()} == sc.FIELD_BITS
    assert {f: g[0] for f, g in model.GEOMETRY.items()} == {f: sc.kind_of(f) for f in Field}


@chains
def test_single_chunk_sweep_equals_the_oracle(chain):
    """One chunk per packet: parse_read is parse_slice, so over the whole
    single-edit sweep (every field, layer, op, four values, what 0 and every
    `what` of the chain) the model's arena is the contiguous definition's."""
    b = sc.batch(chain, "indexed")
    tables = mc.single_chunk_tables(b)
    parsed = model.parse(tables, chain)
    crecs = oracle.parse_batch(b.arena, b.starts, b.lengths, chain)
    assert parsed[0].tobytes() == crecs.tobytes()
    ok = int((crecs["status"] == 0).sum())
    assert ok >= b.n // 3  # (UdpParser takes the UDP frames only)
    moved = refused = 0
    for field in Field:
        for e in sc.sweep(chain, field):
            for what in (0,) + tuple(sc.WHATS[chain]):
                if what and field in sc.REFUSED:
                    refused += 1
                    continue
                want = sc.define(b, chain, [e], what)[0]
                got, recs, _ = model.apply(tables, chain, [e], what, parsed=parsed)
                assert got.tobytes() == want.tobytes(), sc.tag(chain, "one chunk", e, what)
                moved += int((got != b.arena).any())
    assert moved > 500 and refused > 0, (moved, refused)


@pytest.mark.parametrize("profile,chain,cutter", mc.CUT_SETS,
                         ids=[f"{p}-{c.name}-{k}" for p, c, k in mc.CUT_SETS])
def test_cut_sets_equal_the_oracle(profile, chain, cutter):
    """Every Ok packet of a cut set has the contiguous record of its logical
    frame, and the model's bytes are the contiguous definition's: the count of
    compared packets is the count of Ok packets."""
    arena, off, lens, packets = mc.cut_set(profile, chain, cutter, N_CUT)
    tables = cases.place(packets, misalign=list(range(16)) + [5, 11, 2], gap=1)
    parsed = model.parse(tables, chain)
    recs = parsed[0]
    crecs = oracle.parse_batch(arena, off, lens, chain)
    ok = np.nonzero(recs["status"] == 0)[0]
    same = [i for i in ok if recs[i].tobytes() == crecs[i].tobytes()]
    assert len(same) == len(ok), ("Ok with a differing record", sorted(set(ok) - set(same))[:5])
    assert len(ok) > (100 if cutter == "split" else N_CUT // 3), len(ok)
    if cutter == "split":
        assert (recs["status"] == 4).sum() > 100  # StraddledHeader
    nat, what = mc.nat_list(chain)
    lists = [(nat, what), (nat, 0)] + [(e, what) for e in sc.random_lists(chain, 3, seed=5)]
    for edits, w in lists:
        got, _, _ = model.apply(tables, chain, edits, w, parsed=parsed)
        rew, _ = mc.contiguous_definition(arena, off, lens, chain, edits, w)
        compared = 0
        for i in ok:
            o, ln = int(off[i]), int(lens[i])
            assert mc.logical(got, tables, i) == rew[o:o + ln].tobytes(), (i, w, edits)
            compared += 1
        assert compared == len(ok)
        # every other byte of the arena is the original
        bad = np.ones(len(recs), bool)
        bad[ok] = False
        for i in np.nonzero(bad)[0]:
            assert mc.logical(got, tables, i) == mc.logical(tables[0], tables, i), i
        changed = np.nonzero(got != tables[0])[0]
        assert changed.size > 0
        in_chunk = np.zeros(len(got) + 1, np.int32)
        for o, ln in zip(tables[1][:-1], tables[2][:-1]):
            in_chunk[int(o)] += 1
            in_chunk[int(o) + int(ln)] -= 1
        assert (np.cumsum(in_chunk)[changed] > 0).all(), "a byte outside every chunk changed"


def test_ipv6_cut_after_the_fixed_header_is_not_ok():
    """An IPv6 frame cut exactly after the 40-B fixed header, before its
    extension header: Unwanted at the L4 layer under the three non-tunnel
    chains (the chunk ends, so the extension chain is not walked), not Ok,
    and no byte may change."""
    g = cf.frame("v6", cf.UDP, bytes(range(33)), ext=((60, bytes(6)),))
    tables = cases.place([cases.cut_at(g, [54]), cases.cut_at(g, [14, 62])], misalign=[3, 9])
    for chain, l4_layer in ((Chain.GenericUlp, 2), (Chain.UdpParser, 2), (Chain.VlanUlp, 3)):
        recs = model.parse(tables, chain)[0]
        assert (int(recs["status"][0]), int(recs["err_layer"][0])) == (1, l4_layer), chain
        assert int(recs["status"][1]) == 0
        edits, what = mc.nat_list(chain)
        got, _, _ = model.apply(tables, chain, edits, what)
        assert mc.logical(got, tables, 0) == g
        assert mc.logical(got, tables, 1) != g  # the Ok neighbour is edited


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
NAMES = {"ingot_gpu_parse_read_modify": 12, "ingot_gpu_parse_read_modify_csum": 13}


@pytest.fixture(scope="module")
def lib():
    from ingot_amd.build import build

    build()
    return _lib.load()


def test_the_two_calls_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "ingot_gpu.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, nargs in NAMES.items():
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in exported and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert lib.ingot_gpu_abi_version() == 4
    assert re.search(r"^#define INGOT_GPU_ABI_VERSION 4$", header, flags=re.M)
    assert "a chunked form of ingot_gpu_parse_modify" not in header


def test_argument_validation_without_gpu(lib):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(1)
    plain, csum = lib.ingot_gpu_parse_read_modify, lib.ingot_gpu_parse_read_modify_csum
    assert plain(null, None, None, None, None, 10, 1, None, 0, None, None, None) == -1
    assert csum(null, None, None, None, None, 10, 1, None, 0, 3, None, None, None) == -1
    # checked before any device work: chain, the list's size, `what`
    assert plain(fake, None, None, None, None, 10, 99, None, 0, None, None, None) == -1
    assert plain(fake, None, None, None, None, 10, 1, None, 17, None, None, None) == -1
    assert plain(fake, None, None, None, None, 10, 1, None, 1, None, None, None) == -1
    for what in (0, 8, 4, 0x80000001):  # (4: OUTER_L4 on a chain that is not the tunnel)
        assert csum(fake, None, None, None, None, 10, 1, None, 0, what, None, None, None) == -1
    # n == 0 succeeds, then NULL tables are EINVAL
    assert plain(fake, None, None, None, None, 0, 1, None, 0, None, None, None) == 0
    assert csum(fake, None, None, None, None, 0, 1, None, 0, 3, None, None, None) == 0
    assert plain(fake, None, None, None, None, 10, 1, None, 0, None, None, None) == -1
    assert csum(fake, None, None, None, None, 10, 1, None, 0, 3, None, None, None) == -1
