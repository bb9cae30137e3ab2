"""Write tests/golden/csum_kats.json — the checksum vectors.

Two published vectors (RFC 1071 section 3's worked example and a well-known
IPv4 header) and a set of hand-built frames (tests/csum_frames.py).  Every
frame is built with its checksum fields 0, made valid with the model's fill
(tests/csum_model.py) and then, where the case asks for it, broken by hand;
its expected row is the one the byte-wise formulation of
tests/test_checksum_model.py gives (bw_row), and `filled` is the frame after
fill.  tests/test_checksum_model.py holds both formulations to these rows.

    python tests/golden/make_csum_kats.py   # rewrites csum_kats.json
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

import oracle  # noqa: E402
from ingot_amd.abi import Chain  # noqa: E402
from tests import csum_frames as cf  # noqa: E402
from tests import csum_model as model  # noqa: E402

PAY = bytes(range(1, 12))  # 11 bytes: an odd last byte


def valid(f: bytes, chain: Chain) -> bytearray:
    a = np.frombuffer(f, dtype=np.uint8).copy()
    rec = oracle.parse_batch(*cf.place([f])[:3], chain)[0]
    model.one(a, rec, 3, True)
    return bytearray(a.tobytes())


def put16(f: bytearray, at: int, v: int) -> bytearray:
    f[at:at + 2] = cf.u16(v)
    return f


def flip(f: bytearray, at: int) -> bytearray:
    f[at] ^= 0x40
    return f


def udp_sum_zero() -> bytes:
    """A UDP datagram whose computed checksum is 0 (sent as 0xffff)."""
    f = cf.frame("v4", cf.UDP, b"\x00\x00" + PAY)
    a = np.frombuffer(f, dtype=np.uint8).copy()
    rec = oracle.parse_batch(*cf.place([f])[:3], Chain.GenericUlp)[0]
    s0 = 0xFFFF - model.one(a, rec, 2, False)[3]  # the sum with the two payload bytes 0
    return cf.frame("v4", cf.UDP, cf.u16(0xFFFF - s0) + PAY)


G, V = Chain.GenericUlp, Chain.VlanUlp
CASES = [
    # name, chain, frame with zero fields, what is done to it after fill
    ("v4_tcp", G, cf.frame("v4", cf.TCP, PAY), None),
    ("v4_udp", G, cf.frame("v4", cf.UDP, PAY), None),
    ("v4_icmp", G, cf.frame("v4", cf.ICMP4, PAY), None),
    ("v6_tcp", G, cf.frame("v6", cf.TCP, PAY), None),
    ("v6_udp", G, cf.frame("v6", cf.UDP, PAY), None),
    ("v6_icmp", G, cf.frame("v6", cf.ICMP6, PAY), None),
    ("vlan_v4_udp", V, cf.frame("v4", cf.UDP, PAY, vlan=(0x2064,)), None),
    ("qinq_v6_tcp", V, cf.frame("v6", cf.TCP, PAY, vlan=(0x0001, 0x0FFE)), None),
    ("v4_options_tcp", G, cf.frame("v4", cf.TCP, PAY, options=bytes.fromhex("94040000")), None),
    ("v6_hop_by_hop_udp", G, cf.frame("v6", cf.UDP, PAY, ext=((0, bytes(6)),)), None),
    ("v6_hbh_16_dest_tcp", G,
     cf.frame("v6", cf.TCP, PAY, ext=((0, bytes(14)), (60, bytes.fromhex("010400000000")))), None),
    ("v4_fragment_first", G, cf.frame("v4", cf.UDP, PAY, flags_frag=0x2000), None),
    ("v4_fragment_later", G, cf.frame("v4", cf.UDP, PAY, flags_frag=0x00B9), None),
    ("v6_fragment", G, cf.frame("v6", cf.UDP, PAY, ext=(cf.frag_eh(185, 0),)), None),
    ("v6_fragment_first_after_hbh", G,
     cf.frame("v6", cf.TCP, PAY, ext=((0, bytes(6)), cf.frag_eh(0, 1))), None),
    ("v6_atomic_fragment", G, cf.frame("v6", cf.TCP, PAY, ext=(cf.frag_eh(0, 0),)), None),
    ("v4_udp_padded_to_60", G, cf.frame("v4", cf.UDP, b"\x07") + b"\xa5" * 17, None),
    ("v6_tcp_padded", G, cf.frame("v6", cf.TCP, PAY) + b"\x5a" * 3, None),
    ("v4_total_len_past_frame", G, cf.frame("v4", cf.UDP, PAY), lambda f: put16(f, 16, 40)),
    ("v4_total_len_inside_udp", G, cf.frame("v4", cf.UDP, PAY), lambda f: put16(f, 16, 27)),
    ("v6_payload_len_past_frame", G, cf.frame("v6", cf.TCP, PAY), lambda f: put16(f, 18, 32)),
    ("v6_payload_len_inside_tcp", G, cf.frame("v6", cf.TCP, PAY), lambda f: put16(f, 18, 19)),
    ("v4_udp_zero_field", G, cf.frame("v4", cf.UDP, PAY), lambda f: put16(f, 40, 0)),
    ("v6_udp_zero_field", G, cf.frame("v6", cf.UDP, PAY), lambda f: put16(f, 60, 0)),
    ("v4_udp_computed_zero", G, udp_sum_zero(), None),
    ("v4_tcp_payload_flipped", G, cf.frame("v4", cf.TCP, PAY), lambda f: flip(f, len(f) - 1)),
    ("v4_header_flipped", G, cf.frame("v4", cf.ICMP4, PAY), lambda f: flip(f, 22)),
    ("v6_icmp_flipped", G, cf.frame("v6", cf.ICMP6, PAY), lambda f: flip(f, 30)),
    ("arp_accepted", G, cf.eth(0x0806) + bytes(28), None),
    ("v4_tcp_truncated", G, cf.frame("v4", cf.TCP, b"")[:50], None),
]


def main() -> None:
    if not (HERE / "csum_kats.json").exists():  # the test module reads it on import
        (HERE / "csum_kats.json").write_text('{"frames": []}')
    from tests.test_checksum_model import bw_row

    frames = []
    for name, chain, zero, tweak in CASES:
        f = valid(zero, chain)
        if tweak:
            f = tweak(f)
        f = bytes(f)
        rec = oracle.parse_batch(*cf.place([f])[:3], chain)[0]
        a = np.frombuffer(f, dtype=np.uint8).copy()
        model.one(a, rec, 3, True)
        frames.append({"name": name, "chain": chain.name, "frame": f.hex(),
                       "row": bw_row(f, rec, 3), "filled": a.tobytes().hex()})
    out = {
        "rfc1071_section3": {"bytes": "0001f203f4f5f6f7", "sum": "ddf2", "checksum": "220d"},
        "ipv4_header": {"header": "450000730000400040110000c0a80001c0a800c7",
                        "checksum": "b861"},
        "frames": frames,
    }
    (HERE / "csum_kats.json").write_text(json.dumps(out, indent=1) + "\n")
    for k in frames:
        print(f"{k['name']:32s} {k['row']}")


if __name__ == "__main__":
    main()
