"""ingot_gpu_parse_modify_rows without a GPU: its definition
(tests/modify_rows_model.py) pinned to the existing rewrite's, the new checksum
ranges checked against from-scratch sums, the row guard, the ABI's layout and
the Python mirror's host-side validation."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import ingot_amd
import oracle
from ingot_amd import Chain, EditOp, Field, GenProfile, abi
from ingot_amd.abi import (CSUM_L3, CSUM_L4, CSUM_OUTER_L4, ROW_NONE, EditBy, EditSource,
                           WideField)
from ingot_amd.hostgen import gen_frames_host
from tests import csum_update_model as upd
from tests import modify_rows_cases as cases
from tests import modify_rows_model as rows_model
from tests.test_modify import EDITS

ROOT = Path(__file__).resolve().parent.parent
TUN = Chain.GeneveOverV6Tunnel
SET = EditOp.SET


# ---------------------------------------------------------------------------
# 1. The model is pinned to the existing definition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chain", list(Chain))
def test_uniform_tables_are_the_existing_rewrite(chain):
    """Tables whose rows are all equal, no d_row, narrow fields only: the
    oracle's rewrite + tests/csum_update_model.update with the uniform list."""
    prof = {Chain.UdpParser: GenProfile.MIXED, Chain.GenericUlp: GenProfile.ADVERSARIAL,
            Chain.VlanUlp: GenProfile.VLAN_V6EH, TUN: GenProfile.GENEVE}[chain]
    n = 2000
    arena, off, lens = gen_frames_host(prof, n, seed=83, slack=64)
    edits = EDITS[chain]
    tabled = []
    for k, e in enumerate(edits):
        # 16-bit tables where the value fits, 32-bit ones otherwise, and every
        # third edit left a plain value
        dt = np.uint16 if e[3] <= 0xFFFF and k % 2 else np.uint32
        operand = e[3] if k % 3 == 2 else np.full(n, e[3], dtype=dt)
        tabled.append((e[0], e[1], e[2], operand, *e[4:]))
    for what in (0, CSUM_L3 | CSUM_L4, 7 if chain == TUN else CSUM_L4):
        want = arena.copy()
        w_rec = oracle.parse_modify_batch(want, off, lens, chain, edits)
        if what:
            o_udp = None
            if chain == TUN:
                o_udp = oracle.geneve_fields_batch(arena, off, lens)["outer"]["outer_udp_off"]
            upd.update(arena, want, off, lens, w_rec, what, o_udp=o_udp)
        got, recs = rows_model.apply(arena, off, lens, chain, tabled, what=what)
        assert recs.tobytes() == w_rec.tobytes()
        diff = np.nonzero(got != want)[0]
        assert diff.size == 0, (what, diff[:10])
        assert (got != arena).any()


# ---------------------------------------------------------------------------
# 2. The new checksum ranges, without the incremental formula
# ---------------------------------------------------------------------------
def _same_states(arena, off, lens, chain, edits, what, rows=None, n_rows=0):
    before = cases.states(arena, off, lens, chain)
    ok = cases.all_ok(before)
    assert ok.mean() >= 0.9, (int(ok.sum()), len(ok))
    got, _ = rows_model.apply(arena, off, lens, chain, edits, rows=rows, n_rows=n_rows, what=what)
    after = cases.states(got, off, lens, chain)
    # every packet keeps its state (Ok stays Ok; ZERO and FRAGMENT as they were)
    assert (after == before).all(), np.nonzero((after != before).any(axis=1))[0]
    return got


def test_nat_and_mac_rewrite_keep_every_sum_right():
    """NAT44, NAT66 and the next-hop MAC over v4 / v6 x TCP / UDP / ICMP, VLAN
    tags, IPv4 options, IPv6 EHs, a UDP checksum of 0 and two fragments."""
    arena, off, lens = cases.right_sum_frames()
    t = cases.nat_table(len(off), 7)
    got = _same_states(arena, off, lens, Chain.VlanUlp, cases.nat_edits(t, 2), CSUM_L3 | CSUM_L4)
    changed = [(got[int(o):int(o) + int(ln)] != arena[int(o):int(o) + int(ln)]).any()
               for o, ln in zip(off, lens)]
    assert all(changed)
    # ... and the same by row, from a smaller table
    t = cases.nat_table(16, 8)
    rows = (np.arange(len(off), dtype=np.uint32) * 7) % 16
    _same_states(arena, off, lens, Chain.VlanUlp, cases.nat_edits(t, 2, by="row"),
                 CSUM_L3 | CSUM_L4, rows=rows, n_rows=16)


def test_leaving_a_sum_out_breaks_it():
    """The comparison above can fail: NAT66 with L3 only leaves the L4 sums of
    the IPv6 TCP / UDP / ICMPv6 packets wrong."""
    arena, off, lens = cases.right_sum_frames()
    t = cases.nat_table(len(off), 7)
    before = cases.states(arena, off, lens, Chain.VlanUlp)
    got, recs = rows_model.apply(arena, off, lens, Chain.VlanUlp, cases.nat_edits(t, 2),
                                 what=CSUM_L3)
    after = cases.states(got, off, lens, Chain.VlanUlp)
    v6 = (recs["l3_kind"] == int(abi.L3Kind.IPV6)) & (before[:, 1] == cases.OK)
    assert v6.sum() >= 30 and (after[v6, 1] == 2).all()  # BAD


def test_tunnel_rewrite_keeps_all_three_sums_right():
    """The tunnel endpoints, the inner MACs, inner NAT44 / NAT66: inner v4 and
    inner v6, with and without the outer hop-by-hop EH and Geneve options."""
    arena, off, lens = cases.right_sum_tunnel_frames()
    t = cases.nat_table(len(off), 9)
    what = CSUM_L3 | CSUM_L4 | CSUM_OUTER_L4
    _same_states(arena, off, lens, TUN, cases.tunnel_edits(t), what)
    # each new range on its own: outer addresses, inner MACs, inner addresses
    for e in cases.tunnel_edits(t)[:5]:
        _same_states(arena, off, lens, TUN, [e], CSUM_OUTER_L4 | CSUM_L4)


# ---------------------------------------------------------------------------
# 3. The row guard
# ---------------------------------------------------------------------------
def test_guarded_rows_leave_the_packet_untouched():
    arena, off, lens = cases.right_sum_frames()
    n = len(off)
    t = cases.nat_table(8, 10)
    rows = (np.arange(n, dtype=np.uint32) * 5) % 8
    rows[::3] = ROW_NONE
    rows[1::7] = 8  # n_rows itself
    edits = cases.nat_edits(t, 2, by="row") + [(2, Field.V4_HOP_LIMIT, EditOp.SUB, 1),
                                               (2, Field.V6_HOP_LIMIT, EditOp.SUB, 1)]
    got, recs = rows_model.apply(arena, off, lens, Chain.VlanUlp, edits, rows=rows, n_rows=8,
                                 what=CSUM_L3 | CSUM_L4)
    assert (recs["status"] == 0).all()
    for i in range(n):
        o, ln = int(off[i]), int(lens[i])
        same = got[o:o + ln].tobytes() == arena[o:o + ln].tobytes()
        assert same == (int(rows[i]) >= 8), i


# ---------------------------------------------------------------------------
# 4. ABI
# ---------------------------------------------------------------------------
def test_edit_rows_layout_and_enums_match_the_header(tmp_path):
    assert abi.EDIT_ROWS_DTYPE.itemsize == ctypes.sizeof(abi.IngotEditRows) == 24
    fields = [f[0] for f in abi.IngotEditRows._fields_]
    enums = {"INGOT_FW_ETH_DESTINATION": WideField.ETH_DESTINATION,
             "INGOT_FW_ETH_SOURCE": WideField.ETH_SOURCE, "INGOT_FW_V6_SOURCE": WideField.V6_SOURCE,
             "INGOT_FW_V6_DESTINATION": WideField.V6_DESTINATION,
             "INGOT_EDIT_VALUE": EditSource.VALUE, "INGOT_EDIT_U16": EditSource.U16,
             "INGOT_EDIT_U32": EditSource.U32, "INGOT_EDIT_BYTES": EditSource.BYTES,
             "INGOT_BY_PACKET": EditBy.PACKET, "INGOT_BY_ROW": EditBy.ROW,
             "INGOT_ROW_NONE": ROW_NONE, "INGOT_F_COUNT": len(Field)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ingot_gpu.h"',
             "int main(void){", 'printf("size %zu\\n", sizeof(ingot_edit_rows));']
    lines += [f'printf("{f} %zu\\n", offsetof(ingot_edit_rows, {f}));' for f in fields]
    lines += [f'printf("{e} %llu\\n", (unsigned long long){e});' for e in enums]
    lines.append("return 0;}")
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(tmp_path / "probe.c"),
                    "-o", str(tmp_path / "probe")], check=True)
    got = dict(line.split() for line in subprocess.run(
        [str(tmp_path / "probe")], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == 24
    want = {"layer": 0, "field": 1, "op": 2, "index": 3, "value": 4, "source": 8, "by": 9,
            "_pad": 10, "pitch": 12, "d_values": 16}
    for f in fields:
        assert int(got[f]) == getattr(abi.IngotEditRows, f).offset == want[f], f
        assert abi.EDIT_ROWS_DTYPE.fields[f][1] == want[f], f
    for e, v in enums.items():
        assert int(got[e]) == int(v), e
    assert len(Field) == 48 and min(WideField) >= 64


# ---------------------------------------------------------------------------
# 5. Host validation (the device-less Context of tests/test_api_validation.py)
# ---------------------------------------------------------------------------
@pytest.fixture()
def ctx():
    c = object.__new__(ingot_amd.Context)  # no device needed: nothing is launched
    c._lib, c._h, c.device = None, None, 0
    return c


def _bufs(n=8):
    arena = torch.zeros(4096, dtype=torch.uint8)
    off = torch.arange(n, dtype=torch.int64) * 64
    lens = torch.full((n,), 60, dtype=torch.int32).to(torch.uint16)
    return arena, off, lens


def test_tables_are_validated_on_the_host(ctx):
    arena, off, lens = _bufs(8)
    G = Chain.GenericUlp
    u32 = torch.zeros(8, dtype=torch.int32)
    mac = torch.zeros((8, 6), dtype=torch.uint8)
    rows = torch.zeros(8, dtype=torch.int32)

    def call(edits, **kw):
        ctx.parse_modify_rows(arena, off, lens, G, edits, **kw)

    with pytest.raises(ValueError, match="must be uint16 or int16 or int32 or uint32"):
        call([(1, Field.V4_SOURCE, SET, u32.to(torch.int64))])  # wrong dtype
    with pytest.raises(ValueError, match="must be uint8 of shape"):
        call([(0, WideField.ETH_SOURCE, SET, mac.to(torch.int32))])  # wrong dtype, wide
    with pytest.raises(ValueError, match="holds 7 rows, needs at least 8"):
        call([(1, Field.V4_SOURCE, SET, u32[:7])])  # short BY_PACKET array
    with pytest.raises(ValueError, match="holds 8 rows, needs at least 9"):
        call([(1, Field.V4_SOURCE, SET, ("row", u32))], rows=rows, n_rows=9)  # short table
    with pytest.raises(ValueError, match="contiguous in its last dimension"):
        call([(0, WideField.ETH_SOURCE, SET, torch.zeros((8, 12), dtype=torch.uint8)[:, ::2])])
    with pytest.raises(ValueError, match=r"shape \(rows, 6\)"):
        call([(0, WideField.ETH_SOURCE, SET, torch.zeros((8, 5), dtype=torch.uint8))])
    with pytest.raises(ValueError, match="needs `rows`"):
        call([(1, Field.V4_SOURCE, SET, ("row", u32))])  # ("row", t) without rows
    with pytest.raises(ValueError, match="rows holds 7 elements, needs at least 8"):
        call([(1, Field.V4_SOURCE, SET, ("row", u32))], rows=rows[:7], n_rows=8)
    with pytest.raises(ValueError, match="rows must be int32 or uint32"):
        call([(1, Field.V4_SOURCE, SET, ("row", u32))], rows=rows.to(torch.int64), n_rows=8)
    with pytest.raises(ValueError, match="a wide field takes"):
        call([(0, WideField.ETH_SOURCE, SET, 5)])
    with pytest.raises(ValueError, match="must be contiguous"):
        call([(1, Field.V4_SOURCE, SET, torch.zeros(16, dtype=torch.int32)[::2])])
    # shapes in order: host tensors are refused only after the shape checks
    with pytest.raises(ValueError, match="must live on cuda:0"):
        call([(1, Field.V4_SOURCE, SET, u32), (0, WideField.ETH_SOURCE, SET, mac)])
