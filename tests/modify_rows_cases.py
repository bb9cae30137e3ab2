"""Frames, tables and edit lists shared by tests/test_modify_rows_model.py (CPU)
and tests/test_modify_rows.py (GPU).  TEST INFRASTRUCTURE ONLY.

Edit lists are written once, with numpy tables (tests/modify_rows_model.py's
form); device_edits() uploads each table's root array once and rebuilds every
operand as the same strided view of it, so a column of a (rows, 32) NAT table
reaches the device with pitch 32.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import oracle
from ingot_amd.abi import CSUM_L4, Chain, EditOp, Field, WideField
from tests import csum_frames as cf
from tests import csum_model as model
from tests.frames import geneve_outer

TUN = Chain.GeneveOverV6Tunnel
OK, NONE = 1, 0
SET = EditOp.SET


# ---------------------------------------------------------------------------
# Frames whose every sum is right
# ---------------------------------------------------------------------------
def _plain_frames():
    """v4 / v6 x TCP / UDP / ICMP under 0, 1 and 2 VLAN tags with payloads of
    0, 1, 7 and 32 bytes; IPv4 options; the IPv6 hop-by-hop EH; then the three
    packets whose L4 state is not Ok: a UDP checksum of 0, a first and a later
    IPv4 fragment."""
    out = []
    for l3, protos in (("v4", (cf.TCP, cf.UDP, cf.ICMP4)), ("v6", (cf.TCP, cf.UDP, cf.ICMP6))):
        for proto in protos:
            for vlan in ((), (5,), (5, 6)):
                for nb in (0, 1, 7, 32):
                    out.append(cf.frame(l3, proto, bytes(range(nb)), vlan=vlan))
    for proto in (cf.TCP, cf.UDP, cf.ICMP4):
        out.append(cf.frame("v4", proto, b"opts!", options=bytes([1, 1, 1, 1, 1, 1, 1, 0])))
    for proto in (cf.TCP, cf.UDP, cf.ICMP6):
        out.append(cf.frame("v6", proto, b"hop by hop", ext=((0, bytes(6)),)))
        out.append(cf.frame("v6", proto, b"x", vlan=(9,), ext=((0, bytes(6)), (60, bytes(14)))))
    special = [cf.frame("v4", cf.UDP, b"no checksum"),
               cf.frame("v4", cf.UDP, b"first fragment", flags_frag=0x2000),
               cf.frame("v4", cf.TCP, b"later fragment", flags_frag=0x0007)]
    return out, special


@lru_cache(maxsize=None)
def right_sum_frames(misalign: int = 3):
    """-> (arena, off, lens), read-only, VlanUlp-shaped, packed back to back
    from byte `misalign`; every sum filled by the from-scratch model, then the
    zero-checksum UDP packet's field cleared."""
    frames, special = _plain_frames()
    arena, off, lens = cf.place(frames + special, misalign=misalign)
    recs = oracle.parse_batch(arena, off, lens, Chain.VlanUlp)
    assert (recs["status"] == 0).all()
    model.fill(arena, off, lens, recs)
    z = int(off[len(frames)]) + int(recs["l4_off"][len(frames)]) + 6
    arena[z:z + 2] = 0
    arena.setflags(write=False)
    return arena, off, lens


def _tunnel_frames():
    rng = np.random.default_rng(20260117)
    out = []
    for l3, protos in (("v4", (cf.TCP, cf.UDP, cf.ICMP4)), ("v6", (cf.TCP, cf.UDP, cf.ICMP6))):
        for proto in protos:
            for hbh in (False, True):
                for opts in ((), ((0x0129, 0, b""),), ((0x0129, 1, bytes(8)), (0x0129, 2, b""))):
                    inner = cf.frame(l3, proto, bytes(range(11 + len(out) % 5)))
                    o = bytearray(geneve_outer(rng, opts=opts, hbh=hbh))
                    # the outer IPv6 payload length and the outer UDP length
                    # count the inner frame
                    u = 14 + 40 + (8 if hbh else 0)
                    for at in (14 + 4, u + 4):
                        v = int.from_bytes(o[at:at + 2], "big") + len(inner)
                        o[at:at + 2] = v.to_bytes(2, "big")
                    out.append(bytes(o) + inner)
    return out


@lru_cache(maxsize=None)
def right_sum_tunnel_frames(misalign: int = 3):
    """Geneve-over-IPv6 frames with inner v4 / v6 x TCP / UDP / ICMP; the inner
    sums filled under the tunnel chain's records, then the outer UDP sum under
    a UdpParser parse."""
    arena, off, lens = cf.place(_tunnel_frames(), misalign=misalign)
    recs = oracle.parse_batch(arena, off, lens, TUN)
    assert (recs["status"] == 0).all()
    model.fill(arena, off, lens, recs)
    model.fill(arena, off, lens, oracle.parse_batch(arena, off, lens, Chain.UdpParser),
               what=CSUM_L4)
    arena.setflags(write=False)
    return arena, off, lens


def states(arena, off, lens, chain):
    """From-scratch verify (tests/csum_model) -> per packet (l3 state, l4
    state[, the tunnel's outer UDP state])."""
    rows = model.verify(arena, off, lens, oracle.parse_batch(arena, off, lens, chain))
    cols = [rows["l3_state"], rows["l4_state"]]
    if chain == TUN:
        o = model.verify(arena, off, lens, oracle.parse_batch(arena, off, lens, Chain.UdpParser),
                         what=CSUM_L4)
        cols.append(o["l4_state"])
    return np.stack(cols, axis=1)


def all_ok(st) -> np.ndarray:
    """Per packet: every sum it has verifies (IPv6 has no L3 sum: NONE)."""
    ok = ((st[:, 0] == OK) | (st[:, 0] == NONE)) & (st[:, 1] == OK)
    return ok & (st[:, 2] == OK) if st.shape[1] > 2 else ok


# ---------------------------------------------------------------------------
# Tables and edit lists
# ---------------------------------------------------------------------------
def nat_table(rows: int, seed: int) -> np.ndarray:
    """A (rows, 32) uint8 NAT table: +0 IPv4 address (host-endian u32), +4 port
    (host-endian u16), +8 MAC (6 B, wire order), +16 IPv6 address (16 B)."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (rows, 32), dtype=np.uint8)


def col_u32(t, at=0):
    return t[:, at:at + 4].view("<u4")


def col_u16(t, at=4):
    return t[:, at:at + 2].view("<u2")


def nat_edits(t, l3: int, by=None):
    """NAT44 + NAT66 + next-hop MAC from one table `t` (nat_table): the L3
    layer at label `l3`, the L4 layer after it.  by = "row": BY_ROW."""
    w = (lambda x: ("row", x)) if by == "row" else (lambda x: x)
    l4 = l3 + 1
    return [(l3, Field.V4_SOURCE, SET, w(col_u32(t))), (l4, Field.UDP_SOURCE, SET, w(col_u16(t))),
            (l4, Field.TCP_SOURCE, SET, w(col_u16(t))),
            (l3, WideField.V6_SOURCE, SET, w(t[:, 16:32])),
            (0, WideField.ETH_DESTINATION, SET, w(t[:, 8:14])),
            (l3, WideField.V6_DESTINATION, SET, w(t[:, 12:28]))]


def tunnel_edits(t, by=None):
    """The tunnel endpoints (outer IPv6 addresses), the inner MACs and the inner
    NAT44 / NAT66, from one table."""
    w = (lambda x: ("row", x)) if by == "row" else (lambda x: x)
    return [(1, WideField.V6_SOURCE, SET, w(t[:, 16:32])),
            (1, WideField.V6_DESTINATION, SET, w(t[:, 0:16])),
            (4, WideField.ETH_DESTINATION, SET, w(t[:, 8:14])),
            (4, WideField.ETH_SOURCE, SET, w(t[:, 20:26])),
            (5, WideField.V6_SOURCE, SET, w(t[:, 6:22])),
            (5, Field.V4_DESTINATION, SET, w(col_u32(t))),
            (6, Field.UDP_DESTINATION, SET, w(col_u16(t))),
            (6, Field.TCP_SOURCE, EditOp.ADD, w(col_u16(t, 28)))]


def _root(a):
    while a.base is not None:
        a = a.base
    return a


def device_edits(torch, edits, cache=None):
    """The edit list with every numpy table replaced by the same strided view
    of a cuda copy of its root array (one upload per root)."""
    cache = {} if cache is None else cache
    tdt = {2: torch.int16, 4: torch.int32, 1: torch.uint8}

    def dev(a):
        root = _root(a)
        assert root.flags.c_contiguous
        if id(root) not in cache:
            cache[id(root)] = (root, torch.from_numpy(
                np.frombuffer(root.tobytes(), np.uint8).copy()).cuda())
        d = cache[id(root)][1]
        a2 = a if a.ndim == 2 else a.reshape(-1, 1) if a.flags.c_contiguous else a[:, None]
        assert a2.strides[1] in (a2.itemsize, 0) or a2.shape[1] == 1
        byte0 = a2.__array_interface__["data"][0] - root.__array_interface__["data"][0]
        isz = a2.itemsize
        assert byte0 % isz == 0 and a2.strides[0] % isz == 0 and a2.strides[0] > 0
        typed = d.view(tdt[isz]) if isz > 1 else d
        return torch.as_strided(typed, (a2.shape[0], a2.shape[1]), (a2.strides[0] // isz, 1),
                                byte0 // isz)

    out = []
    for e in edits:
        op = e[3]
        if isinstance(op, tuple):
            op = ("row", dev(op[1]))
        elif isinstance(op, np.ndarray):
            op = dev(op)
        out.append((*e[:3], op, *e[4:]))
    return out
