"""The definition of ingot_gpu_checksum_verify / ingot_gpu_checksum_fill
(include/ingot_gpu.h), in numpy / Python.  TEST INFRASTRUCTURE ONLY.

Written from the RFCs, not from the kernel:
  RFC 1071   the Internet checksum: 16-bit big-endian words added with
             end-around carry, an odd last byte padded with 0, complemented;
  RFC 791    the IPv4 header checksum covers the header only;
  RFC 768    UDP: pseudo-header (source, destination, 0, protocol, UDP length),
             a computed 0 is sent as 0xffff, a field of 0 means "no checksum";
  RFC 793    TCP: the same pseudo-header with the TCP segment length;
  RFC 8200   section 8.1: the IPv6 pseudo-header (source, destination, 32-bit
             upper-layer length, 3 zero bytes, next header);
  RFC 4443   section 2.3: ICMPv6 is summed with the IPv6 pseudo-header;
  RFC 792    ICMPv4 has none;
  RFC 1624   the receiver's check: the sum including the field is 0xffff (-0).

Inputs are a frame arena, the frames' offsets and lengths, and the 16-B records
of `oracle.parse_batch` (any chain).  `verify` returns ingot_csum rows
(CSUM_DTYPE); `fill` writes the checksum bytes into the arena in place and
returns the rows after writing.
"""
from __future__ import annotations

import numpy as np

from ingot_amd.abi import CSUM_DTYPE, CSUM_L3, CSUM_L4, CsumState, L3Kind, L4Kind

NONE, OK, BAD, ZERO, SHORT, FRAGMENT = (int(s) for s in CsumState)
_MIN_L4 = {int(L4Kind.TCP): 20, int(L4Kind.UDP): 8, int(L4Kind.ICMPV4): 8, int(L4Kind.ICMPV6): 8}
_FIELD_AT = {int(L4Kind.TCP): 16, int(L4Kind.UDP): 6, int(L4Kind.ICMPV4): 2,
             int(L4Kind.ICMPV6): 2}


def fold(x: int) -> int:
    """End-around carry: a sum of 16-bit words folded to 16 bits."""
    while x >> 16:
        x = (x & 0xFFFF) + (x >> 16)
    return x


def word_sum(data) -> int:
    """The big-endian 16-bit words of `data` added as integers (not folded);
    an odd last byte is the high byte of a word whose low byte is 0."""
    b = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    n = len(b)
    s = int(b[0:n - (n & 1)].view(">u2").sum(dtype=np.uint64)) if n > 1 else 0
    if n & 1:
        s += int(b[n - 1]) << 8
    return s


def ones_sum(data) -> int:
    """RFC 1071: the folded ones'-complement sum of `data`."""
    return fold(word_sum(data))


def checksum(data) -> int:
    return ~ones_sum(data) & 0xFFFF


def _be16(f, at: int) -> int:
    return (int(f[at]) << 8) | int(f[at + 1])


def _v6_fragment(f, l3_off: int, l4_off: int, n_ext: int) -> bool:
    pos, h = l3_off + 40, int(f[l3_off + 6])
    for _ in range(n_ext):
        if pos + 8 > l4_off:
            break
        if h == 44:
            fo = _be16(f, pos + 2)
            if (fo >> 3) != 0 or (fo & 1):
                return True
            step = 8
        else:
            step = 8 + int(f[pos + 1]) * 8
        h = int(f[pos])
        pos += step
    return False


def one(f: np.ndarray, rec, what: int, fill: bool):
    """One frame (`f`: its bytes, a writable view when `fill`) and its record
    -> (l3_state, l4_state, l3_sum, l4_sum, l4_len)."""
    L = len(f)
    row = [NONE, NONE, 0, 0, 0]
    l3_kind, l4_kind = int(rec["l3_kind"]), int(rec["l4_kind"])
    l3_off, l4_off, pay = int(rec["l3_off"]), int(rec["l4_off"]), int(rec["payload_off"])
    if int(rec["status"]) != 0 or l3_kind not in (int(L3Kind.IPV4), int(L3Kind.IPV6)):
        return tuple(row)
    v4 = l3_kind == int(L3Kind.IPV4)
    fixed = 20 if v4 else 40
    if l3_off + fixed > L:
        return tuple(row)
    if v4 and (what & CSUM_L3):
        hl = max(20, (int(f[l3_off]) & 0xF) * 4)
        if l3_off + hl <= L:
            hdr = f[l3_off:l3_off + hl].copy()
            field = _be16(hdr, 10)
            hdr[10:12] = 0
            s0 = fold(word_sum(hdr))
            row[2] = ~s0 & 0xFFFF
            row[0] = OK if fold(s0 + field) == 0xFFFF else BAD
            if fill:
                f[l3_off + 10], f[l3_off + 11] = row[2] >> 8, row[2] & 0xFF
                row[0] = OK
    if not (what & CSUM_L4) or l4_kind not in _MIN_L4:
        return tuple(row)
    if not (l3_off + fixed <= l4_off and l4_off + _MIN_L4[l4_kind] <= pay <= L):
        return tuple(row)
    end = l3_off + _be16(f, l3_off + 2) if v4 else l3_off + 40 + _be16(f, l3_off + 4)
    if end > L or end < pay:
        row[1] = SHORT
        return tuple(row)
    if v4:
        frag = (_be16(f, l3_off + 6) & 0x3FFF) != 0
    else:
        frag = _v6_fragment(f, l3_off, l4_off, int(rec["n_v6ext"]))
    if frag:
        row[1] = FRAGMENT
        return tuple(row)
    seg_len = end - l4_off
    seg = f[l4_off:end].copy()
    at = _FIELD_AT[l4_kind]
    field = _be16(seg, at)
    seg[at:at + 2] = 0
    if l4_kind == int(L4Kind.ICMPV4):
        pseudo = b""
    elif v4:
        pseudo = bytes(f[l3_off + 12:l3_off + 20]) + bytes([0, int(f[l3_off + 9])]) + \
            seg_len.to_bytes(2, "big")
    else:
        pseudo = bytes(f[l3_off + 8:l3_off + 40]) + seg_len.to_bytes(4, "big") + \
            bytes([0, 0, 0, int(rec["l4_proto"])])
    s0 = fold(word_sum(pseudo) + word_sum(seg))
    csum = ~s0 & 0xFFFF
    udp = l4_kind == int(L4Kind.UDP)
    if udp and csum == 0:
        csum = 0xFFFF
    row[3], row[4] = csum, seg_len
    if fill:
        f[l4_off + at], f[l4_off + at + 1] = csum >> 8, csum & 0xFF
        row[1] = OK
    elif udp and field == 0:
        row[1] = ZERO
    else:
        row[1] = OK if fold(s0 + field) == 0xFFFF else BAD
    return tuple(row)


def _run(arena, off, lens, recs, what, stride, n, fill):
    if what == 0 or what & ~(CSUM_L3 | CSUM_L4):
        raise ValueError("what")
    if n is None:
        n = len(off) if off is not None else len(recs)
    out = np.zeros(n, dtype=CSUM_DTYPE)
    for i in range(n):
        o = int(off[i]) if off is not None else i * stride
        ln = int(lens[i]) if lens is not None else stride
        out[i] = one(arena[o:o + ln], recs[i], what, fill)
    return out


def verify(arena, off, lens, recs, what: int = CSUM_L3 | CSUM_L4, stride: int = 0, n=None):
    return _run(arena, off, lens, recs, what, stride, n, False)


def fill(arena, off, lens, recs, what: int = CSUM_L3 | CSUM_L4, stride: int = 0, n=None):
    """In place on `arena` (numpy u8); returns the rows after writing."""
    return _run(arena, off, lens, recs, what, stride, n, True)
