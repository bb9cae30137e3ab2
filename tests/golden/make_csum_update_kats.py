"""Write tests/golden/csum_update_kats.json — vectors for the incremental
checksum update of ingot_gpu_parse_modify_csum.

RFC 1624 section 4's worked example, and hand-built frames
(tests/csum_frames.py) made valid with the checksum model's fill
(tests/csum_model.py) and then, where the case asks for it, changed by hand.
Each frame carries its edit list and `what`; `after` is the oracle's rewrite
followed by the update model (tests/csum_update_model.py).  `fill_equal`
marks the cases whose `after` must also equal rewrite + fill, which this
script asserts, as it asserts each case's own point (a field that must not
move, a result written as 0xffff, ...).

    python tests/golden/make_csum_update_kats.py   # rewrites the file
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

import oracle  # noqa: E402
from ingot_amd.abi import Chain, EditOp, Field  # noqa: E402
from tests import csum_frames as cf  # noqa: E402
from tests import csum_model as model  # noqa: E402
from tests import csum_update_model as upd  # noqa: E402

PAY = bytes(range(1, 12))  # 11 bytes: an odd last byte
G, V, T, U = Chain.GenericUlp, Chain.VlanUlp, Chain.GeneveOverV6Tunnel, Chain.UdpParser
SET, ADD, SUB, XOR, OR = EditOp.SET, EditOp.ADD, EditOp.SUB, EditOp.XOR, EditOp.OR
NAT = [(1, Field.V4_DESTINATION, SET, 0x0A000005), (2, Field.UDP_DESTINATION, SET, 8080),
       (2, Field.TCP_DESTINATION, SET, 8080), (1, Field.V4_HOP_LIMIT, SUB, 1)]


def parse(f: bytes, chain: Chain):
    return oracle.parse_batch(*cf.place([f])[:3], chain)[0]


def fill(f: bytes, chain: Chain) -> bytes:
    """Both levels of a tunnel frame: the inner sums, then the outer."""
    a = np.frombuffer(f, dtype=np.uint8).copy()
    model.one(a, parse(f, chain), 3, True)
    if chain == T:
        model.one(a, parse(a.tobytes(), U), 2, True)
    return a.tobytes()


def put16(f: bytes, at: int, v: int) -> bytes:
    return f[:at] + cf.u16(v) + f[at + 2:]


def tunnel(inner: bytes, vni: int = 0x123456, opts: bytes = b"") -> bytes:
    assert len(opts) % 4 == 0
    gen = bytes([len(opts) // 4, 0]) + cf.u16(0x6558) + vni.to_bytes(3, "big") + b"\0" + opts
    body = gen + inner
    udp = cf.u16(0xC001) + cf.u16(6081) + cf.u16(8 + len(body)) + cf.u16(0) + body
    return cf.eth(0x86DD) + cf.v6(cf.UDP, udp)


def run(f: bytes, chain: Chain, edits, what: int) -> bytes:
    arena, off, lens = cf.place([f])
    after = arena.copy()
    recs = oracle.parse_modify_batch(after, off, lens, chain, edits)
    o_udp = oracle.geneve_fields_batch(arena, off, lens)["outer"]["outer_udp_off"] \
        if chain == T else None
    upd.update(arena, after, off, lens, recs, what, o_udp=o_udp)
    return after[:len(f)].tobytes()


def rewrite_fill(f: bytes, chain: Chain, edits) -> bytes:
    return fill(oracle.parse_modify(f, chain, edits)[0], chain)


def be16(f: bytes, at: int) -> int:
    return int.from_bytes(f[at:at + 2], "big")


def cases():
    """-> (name, chain, frame, edits, what, fill_equal, check(before, after) or None)"""
    v4udp = fill(cf.frame("v4", cf.UDP, PAY), G)
    v4tcp = fill(cf.frame("v4", cf.TCP, PAY), G)
    yield "v4_udp_nat", G, v4udp, NAT, 3, True, None
    yield "v4_tcp_nat", G, v4tcp, NAT, 3, True, None
    yield "v4_udp_nat_l3_only", G, v4udp, NAT, 1, False, \
        lambda b, a: be16(a, 40) == be16(b, 40)
    yield "v4_tcp_nat_l4_only", G, v4tcp, NAT, 2, False, \
        lambda b, a: be16(a, 24) == be16(b, 24)
    yield "v6_tcp_ports", G, fill(cf.frame("v6", cf.TCP, PAY), G), \
        [(2, Field.TCP_SOURCE, SET, 0), (2, Field.TCP_FLAGS, OR, 0x10),
         (1, Field.V6_HOP_LIMIT, SUB, 1)], 3, True, None
    yield "v6_udp_port", G, fill(cf.frame("v6", cf.UDP, PAY), G), \
        [(2, Field.UDP_DESTINATION, SUB, 1)], 2, True, None
    yield "vlan_v4_udp_nat", V, fill(cf.frame("v4", cf.UDP, PAY, vlan=(7,)), V), \
        [(2, Field.V4_SOURCE, XOR, 0x00FF00FF), (3, Field.UDP_SOURCE, ADD, 1000),
         (2, Field.V4_DSCP, SET, 0x2E)], 3, True, None
    # ICMPv4 has no pseudo-header: an address edit moves the header sum only
    yield "icmp4_source_edit", G, fill(cf.frame("v4", cf.ICMP4, PAY), G), \
        [(1, Field.V4_SOURCE, SET, 0x0A0B0C0D)], 3, True, \
        lambda b, a: be16(a, 36) == be16(b, 36) and be16(a, 24) != be16(b, 24)
    yield "icmp4_code_edit", G, fill(cf.frame("v4", cf.ICMP4, PAY), G), \
        [(2, Field.ICMP_CODE, SET, 3)], 3, True, None
    yield "icmp6_code_edit", G, fill(cf.frame("v6", cf.ICMP6, PAY), G), \
        [(2, Field.ICMP_CODE, SET, 3), (2, Field.ICMP_TY, SET, 129)], 3, True, None
    for ihl, opts in ((6, bytes([1, 1, 1, 0])), (15, bytes([1] * 39 + [0]))):
        yield f"v4_options_ihl{ihl}", G, fill(cf.frame("v4", cf.UDP, PAY, options=opts), G), \
            NAT, 3, True, None
    # UDP: no checksum stays no checksum
    yield "udp_field_zero", G, put16(v4udp, 40, 0), NAT, 3, False, \
        lambda b, a: be16(a, 40) == 0 and be16(a, 24) != be16(b, 24)
    # UDP: a result of 0 is written as 0xffff (the port found by trying them all)
    for port in range(65536):
        e = [(2, Field.UDP_SOURCE, SET, port)]
        if be16(run(v4udp, G, e, 2), 40) == 0xFFFF:
            yield "udp_result_zero", G, v4udp, e, 2, True, lambda b, a: be16(a, 40) == 0xFFFF
            break
    else:
        raise AssertionError("no port gives a zero sum")
    # fragments: a later fragment's bytes at l4_off are not an L4 header
    later = put16(fill(cf.frame("v4", cf.UDP, PAY, flags_frag=0x0010), G), 40, 0x1234)
    yield "v4_later_fragment", G, later, NAT, 3, False, \
        lambda b, a: be16(a, 40) == 0x1234 and be16(a, 36) == 8080 and be16(a, 24) != be16(b, 24)
    first = put16(fill(cf.frame("v4", cf.TCP, PAY, flags_frag=0x2000), G), 50, 0x1234)
    yield "v4_first_fragment", G, first, NAT, 3, False, lambda b, a: be16(a, 50) != 0x1234
    # a sum that does not move keeps its representation, also 0xffff
    yield "add_sub_on_ffff", G, put16(v4tcp, 50, 0xFFFF), \
        [(2, Field.TCP_SOURCE, ADD, 1), (2, Field.TCP_SOURCE, SUB, 1)], 3, False, \
        lambda b, a: a == b
    # an edit of a checksum field is applied as written and left out of D
    yield "udp_checksum_edit_plus_port", G, v4udp, \
        [(2, Field.UDP_CHECKSUM, SET, 0xBEEF), (2, Field.UDP_SOURCE, ADD, 5)], 3, False, \
        lambda b, a: be16(a, 40) == upd.eqn3(0xBEEF, (~53 & 0xFFFF) + 58)
    yield "v4_checksum_edit_plus_hop_limit", G, v4tcp, \
        [(1, Field.V4_HOP_LIMIT, SUB, 1), (1, Field.V4_CHECKSUM, XOR, 0x0F0F)], 3, False, None
    yield "tcp_checksum_edit_alone", G, v4tcp, [(2, Field.TCP_CHECKSUM, SET, 0x5555)], 3, \
        False, lambda b, a: be16(a, 50) == 0x5555
    # a wrong input sum stays wrong by the same amount
    wrong = put16(v4tcp, 50, (be16(v4tcp, 50) + 0x0101) & 0xFFFF)
    yield "wrong_input_sum", G, wrong, NAT, 3, False, \
        lambda b, a: model.fold(be16(a, 50) + (0xFFFF - be16(rewrite_fill(b, G, NAT), 50))) \
        == 0x0101
    # the tunnel: inner sums first, then the outer UDP sum over everything
    tun = fill(tunnel(v4udp), T)
    tedits = [(5, Field.V4_DESTINATION, SET, 0x0A000005), (6, Field.UDP_DESTINATION, SET, 8080),
              (3, Field.GENEVE_VNI, SET, 0xABCDEF), (2, Field.UDP_SOURCE, XOR, 0x0FF0)]
    yield "tunnel_v4_udp_all", T, tun, tedits, 7, True, None
    yield "tunnel_v4_udp_outer_only", T, tun, tedits, 4, False, None
    yield "tunnel_v4_udp_inner_only", T, tun, tedits, 3, False, \
        lambda b, a: be16(a, 60) == be16(b, 60)
    tun6 = fill(tunnel(fill(cf.frame("v6", cf.TCP, PAY), G), opts=bytes([0, 1, 0x80, 1, 9, 9, 9, 9])), T)
    yield "tunnel_v6_tcp_options", T, tun6, \
        [(6, Field.TCP_DESTINATION, SET, 8080), (4, Field.ETH_ETHERTYPE, OR, 0),
         (5, Field.V6_HOP_LIMIT, SUB, 1), (3, Field.GENEVE_VNI, ADD, 1)], 7, True, None
    yield "tunnel_outer_field_zero", T, put16(tun, 60, 0), tedits, 7, False, \
        lambda b, a: be16(a, 60) == 0


def main() -> None:
    frames = []
    for name, chain, f, edits, what, fill_equal, check in cases():
        assert parse(f, chain)["status"] == 0, name
        after = run(f, chain, edits, what)
        if fill_equal:
            assert after == rewrite_fill(f, chain, edits), name
        if check is not None:
            assert check(f, after), name
        frames.append({
            "name": name, "chain": chain.name, "what": what, "fill_equal": fill_equal,
            "edits": [[e[0], e[1].name, e[2].name, e[3]] for e in edits],
            "frame": f.hex(), "after": after.hex()})
    out = {
        "rfc1624_section4": {"hc": "dd2f", "m": "5555", "m_new": "3285", "hc_new": "0000"},
        "frames": frames,
    }
    (HERE / "csum_update_kats.json").write_text(json.dumps(out, indent=1) + "\n")
    for k in frames:
        print(f"{k['name']:36s} what={k['what']} {len(k['frame']) // 2} B")


if __name__ == "__main__":
    main()
