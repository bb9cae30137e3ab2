"""tests/emit_csum_model.py (the definition of ingot_gpu_emit_packets_csum)
against the path that is already pinned — oracle.emit_batch, a UdpParser parse
of the emitted arena, csum_model.fill — and against vectors worked by hand.
No GPU."""
import numpy as np
import pytest

import oracle
from ingot_amd import CSUM_L3, CSUM_L4, Chain, EmitSource, EmitSum, Field, GenProfile
from ingot_amd.hostgen import gen_frames_host
from tests import csum_model
from tests import emit_csum_cases as cases
from tests import emit_csum_model as model

OK = int(csum_model.OK)


@pytest.mark.parametrize("name", ["opte", "geneve_v4"])
def test_model_equals_emit_parse_fill(name):
    n = 2000
    rng = np.random.default_rng(41)
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=32, slack=64)
    hdr, sets, sums = cases.stack(name, n, rng)
    dst_off, size = cases.pack(lens, len(hdr), rng)
    emitted = np.full(size, 0xA5, np.uint8)
    oracle.emit_batch(hdr, sets, arena, off, lens, emitted, dst_off)
    got = model.apply(emitted.copy(), hdr, sums, dst_off, lens, sets)
    want = emitted.copy()
    tl = (lens.astype(np.int64) + len(hdr)).astype(np.uint16)
    recs = oracle.parse_batch(want, dst_off, tl, Chain.UdpParser)
    assert (recs["status"] == 0).all()
    rows = csum_model.fill(want, dst_off, tl, recs, CSUM_L3 | CSUM_L4)
    assert (rows["l4_state"] == OK).all()
    if name == "geneve_v4":
        assert (rows["l3_state"] == OK).all()
    assert got.tobytes() == want.tobytes()
    assert (got != emitted).sum() > n  # the fields were written


def _emit_one(hdr, payload, sums):
    pkt = np.frombuffer(bytes(hdr) + bytes(payload), np.uint8).copy()
    model.one(pkt, bytes(hdr), sums)
    return pkt


def test_hand_vectors():
    # UDP over IPv4, 20 + 8 B of headers: src 10.0.0.1, dst 10.0.0.2, ports
    # 1 -> 2, length 8 + payload
    def v4udp(payload, src=(10, 0, 0, 1)):
        ln = 8 + len(payload)
        ip = bytes([0x45, 0, 0, 20 + ln, 0, 0, 0, 0, 64, 17, 0xAA, 0xAA, *src, 10, 0, 0, 2])
        return ip + bytes([0, 1, 0, 2, ln >> 8, ln & 0xFF, 0x55, 0x55])

    sums = [(EmitSum.UDP, 20, 0), (EmitSum.IPV4, 0)]
    # odd payload length (3 B: 0x01 0x02 0x03).  By hand, 16-bit words:
    # pseudo 0a00+0001+0a00+0002+0011+000b = 141f; UDP 0001+0002+000b+0000 =
    # 000e; payload 0102+0300 = 0402; total 182f -> ~ = e7d0.
    # IPv4: 4500+001f+0000+0000+4011+0000+0a00+0001+0a00+0002 = 9933 -> 66cc
    pkt = _emit_one(v4udp(b"\1\2\3"), b"\1\2\3", sums)
    assert bytes(pkt[26:28]) == bytes([0xE7, 0xD0])
    assert bytes(pkt[10:12]) == bytes([0x66, 0xCC])
    # a computed 0 is sent as 0xffff: a 2-B payload that makes the words add
    # up to ffff.  Length 10: pseudo 141e, UDP 000d, together 142b; payload
    # ffff - 142b = ebd4
    pkt = _emit_one(v4udp(b"\xeb\xd4"), b"\xeb\xd4", sums)
    assert bytes(pkt[26:28]) == bytes([0xFF, 0xFF])
    # S > 65535: the UDP field keeps its bytes (0x5555), the IPv4 sum is
    # still written
    big = bytes(65535)
    pkt = _emit_one(v4udp(b"") , big, sums)
    assert bytes(pkt[26:28]) == bytes([0x55, 0x55])
    assert bytes(pkt[10:12]) != bytes([0xAA, 0xAA])
    # S == 65535 exactly is still a datagram: written
    pkt = _emit_one(v4udp(b""), bytes(65535 - 8), [(EmitSum.UDP, 20, 0)])
    assert bytes(pkt[26:28]) != bytes([0x55, 0x55])
    assert bytes(pkt[10:12]) == bytes([0xAA, 0xAA])  # not named: untouched


def test_v6_pseudo_header_by_hand():
    # IPv6 (40 B) + UDP (8 B) + 1 B payload 0x80.  Addresses ::1 -> ::2.
    ip = bytes([0x60, 0, 0, 0, 0, 9, 17, 64]) + bytes(15) + b"\1" + bytes(15) + b"\2"
    udp = bytes([0x10, 0x00, 0x20, 0x00, 0, 9, 0, 0])
    pkt = _emit_one(ip + udp, b"\x80", [(EmitSum.UDP, 40, 0)])
    # pseudo 0001+0002+0009 (length, low word)+0011 = 001d; UDP 1000+2000+0009
    # = 3009; payload 8000; total b026 -> ~ = 4fd9
    assert bytes(pkt[46:48]) == bytes([0x4F, 0xD9])


def test_argument_errors():
    hdr, sets, sums = cases.stack("geneve_v4", 1, np.random.default_rng(0))
    ok = lambda s, se=sets, h=hdr: model.check_args(h, se, s)  # noqa: E731
    ok(sums)
    ok([])
    bad = [
        [(EmitSum.UDP, 34, 14), (EmitSum.UDP, 34, 14)],          # two of one kind
        [(EmitSum.IPV4, 14), (EmitSum.UDP, 34, 14), (EmitSum.IPV4, 14)],  # too many
        [(2, 34, 14)],                                           # unknown kind
        [(EmitSum.UDP, 35, 14)], [(EmitSum.UDP, 34, 13)],        # odd offsets
        [(EmitSum.IPV4, 14, 2)],                                 # IPV4: l3_at != 0
        [(EmitSum.IPV4, 34)],                                    # version nibble
        [(EmitSum.IPV4, 40)],                                    # not a header at all
        [(EmitSum.UDP, len(hdr) - 6, 14)],                       # at + 8 > hdr_len
        [(EmitSum.UDP, 34, 0)],                                  # version at l3_at (Ethernet)
        [(EmitSum.UDP, 32, 14)],                                 # IP header ends after `at`
    ]
    for s in bad:
        with pytest.raises(ValueError):
            ok(s)
    for f in (Field.V4_VERSION, Field.V4_IHL, Field.V6_VERSION):
        with pytest.raises(ValueError):
            ok(sums, sets + [(14, f, EmitSource.VALUE, 4)])
    short = bytes(hdr[:14]) + bytes([0x44]) + bytes(hdr[15:])   # ihl 4
    with pytest.raises(ValueError):
        ok([(EmitSum.IPV4, 14)], sets, short)
    long_ = bytes(hdr[:14]) + bytes([0x4F]) + bytes(hdr[15:])   # ihl 15: 60 B > the block
    with pytest.raises(ValueError):
        ok([(EmitSum.IPV4, 14)], sets, long_)
    with pytest.raises(ValueError):
        ok([(EmitSum.UDP, 0, 0)], [], b"")
