"""The definition of ingot_gpu_parse_read_modify / _csum (include/ingot_gpu.h),
in numpy / Python.  TEST INFRASTRUCTURE ONLY.

Written from the header's text, not from the kernel.  For each packet:
  1. oracle.parse_read of its chunks;
  2. if the record is Ok, the chunks concatenated are the logical frame;
  3. the edits are applied in order at the record's logical offsets, through
     the field-geometry table below and oracle.be_bits / oracle.be_set_bits'
     semantics (big-endian bit runs, neighbouring bits preserved, the op
     wrapping modulo 2^width);
  4. tests/csum_update_model.one(before, after, rec, what, o_udp) on the
     logical frame (the tunnel's o_udp from oracle.parse_read_batch(...,
     fields="geneve"));
  5. the bytes are scattered back into the chunks;
  6. everything else in the arena is unchanged.
"""
from __future__ import annotations

import numpy as np

import oracle
from ingot_amd.abi import Chain, EditOp, Field, L3Kind, L4Kind
from tests import csum_update_model as upd

TUN = Chain.GeneveOverV6Tunnel

# enum ingot_field -> (header kind, first bit, width): the wire layouts of
# Ethernet, the 802.1Q tag, IPv4 (RFC 791), IPv6 (RFC 8200), TCP (RFC 9293),
# UDP (RFC 768), ICMP (RFC 792) and Geneve (RFC 8926)
GEOMETRY = {
    Field.ETH_ETHERTYPE: ("ETH", 96, 16),
    Field.VLAN_PRIORITY: ("VLAN", 0, 3), Field.VLAN_DEI: ("VLAN", 3, 1),
    Field.VLAN_VID: ("VLAN", 4, 12), Field.VLAN_ETHERTYPE: ("VLAN", 16, 16),
    Field.V4_VERSION: ("V4", 0, 4), Field.V4_IHL: ("V4", 4, 4), Field.V4_DSCP: ("V4", 8, 6),
    Field.V4_ECN: ("V4", 14, 2), Field.V4_TOTAL_LEN: ("V4", 16, 16),
    Field.V4_IDENTIFICATION: ("V4", 32, 16), Field.V4_FLAGS: ("V4", 48, 3),
    Field.V4_FRAGMENT_OFFSET: ("V4", 51, 13), Field.V4_HOP_LIMIT: ("V4", 64, 8),
    Field.V4_PROTOCOL: ("V4", 72, 8), Field.V4_CHECKSUM: ("V4", 80, 16),
    Field.V4_SOURCE: ("V4", 96, 32), Field.V4_DESTINATION: ("V4", 128, 32),
    Field.V6_VERSION: ("V6", 0, 4), Field.V6_DSCP: ("V6", 4, 6), Field.V6_ECN: ("V6", 10, 2),
    Field.V6_FLOW_LABEL: ("V6", 12, 20), Field.V6_PAYLOAD_LEN: ("V6", 32, 16),
    Field.V6_NEXT_HEADER: ("V6", 48, 8), Field.V6_HOP_LIMIT: ("V6", 56, 8),
    Field.TCP_SOURCE: ("TCP", 0, 16), Field.TCP_DESTINATION: ("TCP", 16, 16),
    Field.TCP_SEQUENCE: ("TCP", 32, 32), Field.TCP_ACKNOWLEDGEMENT: ("TCP", 64, 32),
    Field.TCP_DATA_OFFSET: ("TCP", 96, 4), Field.TCP_RESERVED: ("TCP", 100, 4),
    Field.TCP_FLAGS: ("TCP", 104, 8), Field.TCP_WINDOW_SIZE: ("TCP", 112, 16),
    Field.TCP_CHECKSUM: ("TCP", 128, 16), Field.TCP_URGENT_PTR: ("TCP", 144, 16),
    Field.UDP_SOURCE: ("UDP", 0, 16), Field.UDP_DESTINATION: ("UDP", 16, 16),
    Field.UDP_LENGTH: ("UDP", 32, 16), Field.UDP_CHECKSUM: ("UDP", 48, 16),
    Field.ICMP_TY: ("ICMP", 0, 8), Field.ICMP_CODE: ("ICMP", 8, 8),
    Field.ICMP_CHECKSUM: ("ICMP", 16, 16),
    Field.GENEVE_VERSION: ("GENEVE", 0, 2), Field.GENEVE_OPT_LEN: ("GENEVE", 2, 6),
    Field.GENEVE_FLAGS: ("GENEVE", 8, 8), Field.GENEVE_PROTOCOL_TYPE: ("GENEVE", 16, 16),
    Field.GENEVE_VNI: ("GENEVE", 32, 24), Field.GENEVE_RESERVED: ("GENEVE", 56, 8),
}
assert len(GEOMETRY) == len(Field) == 48

_L3 = {int(L3Kind.IPV4): "V4", int(L3Kind.IPV6): "V6"}
_L4 = {int(L4Kind.TCP): "TCP", int(L4Kind.UDP): "UDP", int(L4Kind.ICMPV4): "ICMP",
       int(L4Kind.ICMPV6): "ICMP"}


def header_at(chain, rec, outer, layer: int, index: int):
    """-> (header kind, logical offset) of chain layer `layer` of an Ok
    record, or (None, 0).  `outer`: the tunnel's outer field block."""
    l3 = (_L3.get(int(rec["l3_kind"])), int(rec["l3_off"]))
    l4 = (_L4.get(int(rec["l4_kind"])), int(rec["l4_off"]))
    eth = ("ETH", 0)
    if chain == TUN:
        table = [eth, ("V6", 14), ("UDP", int(outer["outer_udp_off"])),
                 ("GENEVE", int(outer["geneve_off"])), ("ETH", int(outer["inner_eth_off"])), l3, l4]
    elif chain == Chain.VlanUlp:
        vlan = ("VLAN" if index < int(rec["n_vlan"]) else None, 14 + 4 * index)
        table = [eth, vlan, l3, l4]
    else:
        table = [eth, l3, l4]
    return table[layer] if layer < len(table) else (None, 0)


def get_bits(f, first_bit: int, n_bits: int) -> int:
    """oracle.be_bits over the covering bytes of a bit run of a numpy byte array."""
    lo, hi = first_bit // 8, (first_bit + n_bits + 7) // 8
    return oracle.be_bits(f[lo:hi].tobytes(), first_bit - 8 * lo, n_bits)


def set_bits(f, first_bit: int, n_bits: int, value: int) -> None:
    """oracle.be_set_bits in place: only the run's bits change."""
    lo, hi = first_bit // 8, (first_bit + n_bits + 7) // 8
    new = oracle.be_set_bits(f[lo:hi].tobytes(), first_bit - 8 * lo, n_bits, value)
    f[lo:hi] = np.frombuffer(new, np.uint8)


def apply_op(cur: int, op, value: int, bits: int) -> int:
    op = EditOp(op)
    v = {EditOp.SET: value, EditOp.ADD: cur + value, EditOp.SUB: cur - value,
         EditOp.AND: cur & value, EditOp.OR: cur | value, EditOp.XOR: cur ^ value}[op]
    return v & ((1 << bits) - 1)


def edit_frame(f, chain, rec, outer, edits) -> None:
    """The edits, in order, on the logical frame `f` (numpy u8, in place)."""
    for e in edits:
        layer, field, op, value = int(e[0]), Field(e[1]), e[2], int(e[3])
        index = int(e[4]) if len(e) > 4 else 0
        kind, first, bits = GEOMETRY[field]
        have, h = header_at(chain, rec, outer, layer, index)
        if have != kind:
            continue
        set_bits(f, 8 * h + first, bits, apply_op(get_bits(f, 8 * h + first, bits), op, value, bits))


def parse(tables, chain):
    """oracle.parse_read_batch of `tables` -> (records, the tunnel's field
    blocks or None, chunk indices): the parse sees the bytes before the edits."""
    return oracle.parse_read_batch(*tables, chain, fields="geneve" if chain == TUN else None)


def apply(tables, chain, edits, what: int = 0, parsed=None):
    """-> (the arena after the call, the records, the chunk indices): what
    ingot_gpu_parse_read_modify (what == 0) / _csum must leave of `tables` =
    (arena, seg_off, seg_len, pkt_seg).  `parsed`: parse(tables, chain), when
    the caller already has it."""
    arena, seg_off, seg_len, pkt_seg = tables
    recs, gf, chunk = parsed if parsed is not None else parse(tables, chain)
    want = np.array(arena)
    for i in range(len(pkt_seg) - 1):
        if int(recs["status"][i]) != 0:
            continue
        # a packet none of whose headers an edit names keeps every byte (no
        # edit applies, every sum's delta is 0)
        out_i = gf["outer"][i] if chain == TUN else None
        if not any(header_at(chain, recs[i], out_i, int(e[0]), int(e[4]) if len(e) > 4 else 0)[0]
                   == GEOMETRY[Field(e[1])][0] for e in edits):
            continue
        ks = range(int(pkt_seg[i]), int(pkt_seg[i + 1]))
        before = np.concatenate([arena[int(seg_off[k]):int(seg_off[k]) + int(seg_len[k])]
                                 for k in ks])
        after = before.copy()
        outer = gf["outer"][i] if chain == TUN else None
        edit_frame(after, chain, recs[i], outer, edits)
        if what:
            upd.one(before, after, recs[i], what,
                    int(outer["outer_udp_off"]) if chain == TUN else None)
        x = 0
        for k in ks:
            o, ln = int(seg_off[k]), int(seg_len[k])
            want[o:o + ln] = after[x:x + ln]
            x += ln
    return want, recs, chunk
