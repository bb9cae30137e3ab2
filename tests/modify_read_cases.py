"""Chunk tables, cutters and edit lists shared by tests/test_modify_read_model.py
(CPU), tests/test_modify_read.py (GPU), tools/bigfuzz.py and
tools/modify_csum_probe.py.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import oracle
from ingot_amd.abi import CSUM_L3, CSUM_L4, Chain, EditOp, Field, GenProfile
from tests import csum_read_cases as cases
from tests import csum_sweep_cases as sc
from tests import csum_update_model as upd

TUN = Chain.GeneveOverV6Tunnel
F, SET, SUB = Field, EditOp.SET, EditOp.SUB

# (profile, chain, cutter): the four generator sets of tests/test_csum_read.py
# (cut by csum_read_cases.cut) and ADVERSARIAL frames split anywhere
CUT_SETS = [("MIXED", Chain.GenericUlp, "cut"), ("VLAN_V6EH", Chain.VlanUlp, "cut"),
            ("GENEVE", TUN, "cut"), ("MIXED", Chain.UdpParser, "cut"),
            ("ADVERSARIAL", Chain.GenericUlp, "split"), ("ADVERSARIAL", Chain.VlanUlp, "split")]


def nat_list(chain):
    """Hop limit / TTL - 1, V4_SOURCE SET, L4 source port SET (tunnel: also
    GENEVE_VNI SET) and the sums to keep right."""
    l3 = sc.L3_LAYER[chain]
    edits = [(l3, F.V4_HOP_LIMIT, SUB, 1), (l3, F.V6_HOP_LIMIT, SUB, 1),
             (l3, F.V4_SOURCE, SET, 0x0A000001), (l3 + 1, F.UDP_SOURCE, SET, 40001),
             (l3 + 1, F.TCP_SOURCE, SET, 40001)]
    if chain == TUN:
        edits.append((3, F.GENEVE_VNI, SET, 0xABCDEF))
    return edits, (7 if chain == TUN else CSUM_L3 | CSUM_L4)


def cut_set(profile: str, chain, cutter: str, n: int):
    """-> (arena, off, lens, chunked packets): the frames and cuts of
    tests/test_csum_read.py's generator and adversarial tests, `n` frames."""
    from tests.test_checksum import prepare

    if cutter == "split":
        from tests.test_parse_read import split

        arena, off, lens, _, _ = prepare(GenProfile.ADVERSARIAL, n, Chain.GenericUlp, seed=4444)
        return arena, off, lens, split(cases.frames_of(arena, off, lens), seed=3)
    arena, off, lens, crecs, _ = prepare(GenProfile[profile], n, chain, seed=4343)
    rng = np.random.default_rng(17)
    frames = cases.frames_of(arena, off, lens)
    return arena, off, lens, [cases.cut(f, crecs[i], rng) for i, f in enumerate(frames)]


def single_chunk_tables(b: sc.Batch):
    """A contiguous batch as one chunk per packet (the frames in place)."""
    n = b.n
    seg_off = np.r_[b.starts.astype(np.uint64), np.uint64(0)]
    seg_len = np.r_[b.lengths.astype(np.uint16), np.uint16(0)]
    return np.array(b.arena), seg_off, seg_len, np.arange(n + 1, dtype=np.uint32)


def header_cuts(chain, rec, outer=None, vlans: int = 0):
    """One header per chunk: eth | vlan | vlan | l3 | l4 | payload (the
    tunnel: outer eth | v6 | udp | geneve | inner eth | l3 | l4 | payload)."""
    cuts = [14]
    if chain == TUN:
        cuts += [int(outer["outer_udp_off"]), int(outer["geneve_off"]),
                 int(outer["inner_eth_off"]), int(outer["inner_eth_off"]) + 14]
    cuts += [14 + 4 * (v + 1) for v in range(vlans)]
    if int(rec["status"]) == 0:
        cuts += [int(rec["l3_off"]), int(rec["l4_off"]), int(rec["payload_off"])]
    return sorted({c for c in cuts if c > 0})


def contiguous_definition(arena, off, lens, chain, edits, what):
    """oracle.parse_modify_batch + csum_update_model.update over contiguous
    frames -> (the arena after, the records)."""
    rew = np.array(arena)
    recs = oracle.parse_modify_batch(rew, off, lens, chain, edits)
    if what:
        o_udp = None
        if chain == TUN:
            o_udp = oracle.geneve_fields_batch(arena, off, lens)["outer"]["outer_udp_off"]
        idx = np.nonzero(rew != arena)[0]
        if idx.size:
            starts = np.asarray(off, np.uint64)
            ch = np.unique(np.searchsorted(starts, idx.astype(np.uint64), side="right") - 1)
            upd.update(arena, rew, starts[ch], np.asarray(lens)[ch], recs[ch], what,
                       o_udp=None if o_udp is None else o_udp[ch])
    return rew, recs


def logical(arena, tables, i) -> bytes:
    """Packet i's chunks of `tables`, read from `arena`, concatenated."""
    _, seg_off, seg_len, pkt_seg = tables
    return b"".join(arena[int(seg_off[k]):int(seg_off[k]) + int(seg_len[k])].tobytes()
                    for k in range(int(pkt_seg[i]), int(pkt_seg[i + 1])))
