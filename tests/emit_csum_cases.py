"""Header stacks, setters and sums shared by tests/test_emit_csum_model.py and
tests/test_emit_csum.py.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from ingot_amd import EmitSource, EmitSum, Field
from ingot_amd import emit as E

MAC_D, MAC_S = bytes.fromhex("a84025777776"), bytes.fromhex("a84025777777")
V6_S = bytes.fromhex("fd000000f70101000000000000000002")
V6_D = bytes.fromhex("fd000000f70101000000000000000001")
V4_S, V4_D = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])

# every payload length at which the chunk walk takes another turn; the last
# makes the UDP segment longer than any datagram (the field is left alone)
EDGE_LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4097, 8972, 65535)

STACKS = ("opte", "geneve_v4", "v6_udp", "vlan_v4opt", "preset")


def stack(name: str, n: int, rng):
    """-> (hdr, sets, sums): sets with numpy per-packet arrays (host form)."""
    u16 = lambda: rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)  # noqa: E731
    u32 = lambda bits=32: rng.integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    if name == "opte":
        # Eth / IPv6 / UDP / Geneve + option, per-packet entropy port and VNI
        hdr = (E.ethernet(MAC_D, MAC_S, 0x86DD) + E.ipv6(V6_S, V6_D, 17, hop_limit=0xF0)
               + E.udp(0xC0DE, 6081) + E.geneve(0x123456, options=E.geneve_opt(0x0129, 0)))
        sets = [(14, Field.V6_PAYLOAD_LEN, EmitSource.LENGTH, -40),
                (54, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
                (54, Field.UDP_SOURCE, EmitSource.U16, 0, u16()),
                (62, Field.GENEVE_VNI, EmitSource.U32, 0, u32(24))]
        return hdr, sets, [(EmitSum.UDP, 54, 14)]
    if name in ("geneve_v4", "preset"):
        # Eth / IPv4 / UDP / Geneve, a per-packet source address; "preset":
        # both fields start from a caller constant != 0
        pre = name == "preset"
        hdr = (E.ethernet(MAC_D, MAC_S, 0x0800)
               + E.ipv4(V4_S, V4_D, 17, hop_limit=0x40, checksum=0x1234 if pre else 0)
               + E.udp(0xC0DE, 6081, checksum=0xBEEF if pre else 0) + E.geneve(0x00ABCD))
        sets = [(14, Field.V4_TOTAL_LEN, EmitSource.LENGTH, 0),
                (34, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
                (14, Field.V4_SOURCE, EmitSource.U32, 0, u32())]
        return hdr, sets, [(EmitSum.IPV4, 14), (EmitSum.UDP, 34, 14)]
    if name == "v6_udp":
        # Eth / IPv6 / UDP: the field is 2 B before the payload
        hdr = (E.ethernet(MAC_D, MAC_S, 0x86DD) + E.ipv6(V6_S, V6_D, 17)
               + E.udp(0x1234, 4789))
        sets = [(14, Field.V6_PAYLOAD_LEN, EmitSource.LENGTH, -40),
                (54, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
                (54, Field.UDP_SOURCE, EmitSource.U16, 0, u16())]
        return hdr, sets, [(EmitSum.UDP, 54, 14)]
    if name == "vlan_v4opt":
        # Eth / VLAN / IPv4 + 8 B of options / UDP
        hdr = (E.ethernet(MAC_D, MAC_S, 0x8100) + E.vlan(0x123, 0x0800)
               + E.ipv4(V4_S, V4_D, 17, options=bytes([0x94, 4, 0, 0, 1, 1, 1, 0]))
               + E.udp(7, 4789))
        sets = [(18, Field.V4_TOTAL_LEN, EmitSource.LENGTH, 0),
                (46, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
                (18, Field.V4_IDENTIFICATION, EmitSource.U16, 0, u16())]
        return hdr, sets, [(EmitSum.UDP, 46, 18), (EmitSum.IPV4, 18)]
    raise KeyError(name)


def pack(lens, hdr_len: int, rng, max_gap: int = 3, first: int = 5):
    """Destination offsets: packets one after another with random 0..max_gap
    byte gaps -> (dst_off u64, arena size)."""
    tot = hdr_len + np.asarray(lens).astype(np.int64)
    gaps = rng.integers(0, max_gap + 1, len(tot))
    off = np.cumsum(np.r_[0, (tot + gaps)[:-1]]) + first
    return off.astype(np.uint64), int(off[-1] + tot[-1] + 64)


def random_source(lens, rng, max_gap: int = 19):
    """Random payload bytes at random misalignments -> (src u8, off u64)."""
    ln = np.asarray(lens).astype(np.int64)
    off = np.cumsum(np.r_[0, (ln + rng.integers(0, max_gap + 1, len(ln)))[:-1]]) + 3
    src = rng.integers(0, 256, int(off[-1] + ln[-1] + 64), dtype=np.uint8)
    return src, off.astype(np.uint64)
