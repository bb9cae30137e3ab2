"""The definition of ingot_gpu_emit_packets_csum (include/ingot_gpu.h), in
numpy / Python.  TEST INFRASTRUCTURE ONLY.

Written from the RFCs, not from the kernel (RFC 1071 the sum, RFC 791 the
IPv4 header checksum, RFC 768 UDP and its IPv4 pseudo-header, RFC 8200 section
8.1 the IPv6 pseudo-header), on top of tests/csum_model.py's `word_sum` /
`fold`.

`apply` takes the arena that `oracle.emit_batch(hdr, sets, ...)` produced —
the plain emit of the same arguments — and writes the two checksum-field
bytes of each named sum of each packet, in place.  Nothing else changes.

  sums = [(EmitSum.IPV4, at), (EmitSum.UDP, at, l3_at)], at most one of each.

  IPV4  field at `at + 10` := checksum of [at, at + 4 * ihl) of the emitted
        packet with the field as 0; ihl from the host block `hdr`.
  UDP   field at `at + 6`.  Segment: every emitted byte from `at` to the
        packet's end, S bytes, field as 0, an odd last byte padded with 0.
        Pseudo-header from the emitted packet at `l3_at`; IP version from
        `hdr[l3_at] >> 4`: IPv4 = source, destination, 0, 17, S (16 bits);
        IPv6 = source, destination, S (32 bits), 0, 0, 0, 17.  A result of 0
        is written as 0xffff.  S > 65535: the field is left as emitted.

The IPV4 sum is written first, whatever the order of `sums`, so a UDP segment
that covers the named IPv4 header sums its final bytes.
"""
from __future__ import annotations

import numpy as np

from ingot_amd.abi import EmitSum
from tests.csum_model import fold, word_sum

MAX_SUMS = 2


def check_args(hdr: bytes, sets, sums) -> None:
    """The argument errors of the call that concern the sums (ValueError)."""
    hdr = bytes(hdr)
    H = len(hdr)
    if len(sums) > MAX_SUMS:
        raise ValueError("too many sums")
    kinds = [int(s[0]) for s in sums]
    if len(set(kinds)) != len(kinds):
        raise ValueError("two sums of one kind")
    named = []
    for s in sums:
        kind, at = int(s[0]), int(s[1])
        l3_at = int(s[2]) if len(s) > 2 else 0
        if kind not in (int(EmitSum.IPV4), int(EmitSum.UDP)):
            raise ValueError("unknown kind")
        if at & 1 or l3_at & 1:
            raise ValueError("odd offset")
        if kind == int(EmitSum.IPV4):
            if l3_at != 0 or at >= H or hdr[at] >> 4 != 4:
                raise ValueError("IPV4: not an IPv4 header")
            ihl = hdr[at] & 0xF
            if ihl < 5 or at + 4 * ihl > H:
                raise ValueError("IPV4: header length")
            named.append(at)
        else:
            if at + 8 > H or l3_at >= H or hdr[l3_at] >> 4 not in (4, 6):
                raise ValueError("UDP: header / IP version")
            if l3_at + (20 if hdr[l3_at] >> 4 == 4 else 40) > at:
                raise ValueError("UDP: IP header does not end before the UDP header")
            named.append(l3_at)
    for e in sets:
        if getattr(e[1], "name", "") in ("V4_VERSION", "V4_IHL", "V6_VERSION") and \
                int(e[0]) in named:
            raise ValueError("setter on the version / ihl of a named header")


def one(pkt: np.ndarray, hdr: bytes, sums) -> None:
    """One emitted packet (`pkt`: a writable view of its hdr_len + len bytes)."""
    for s in sorted(sums, key=lambda s: int(s[0])):  # IPV4 (0) before UDP (1)
        kind, at = int(s[0]), int(s[1])
        if kind == int(EmitSum.IPV4):
            hl = (hdr[at] & 0xF) * 4
            h = pkt[at:at + hl].copy()
            h[10:12] = 0
            c = ~fold(word_sum(h)) & 0xFFFF
            pkt[at + 10], pkt[at + 11] = c >> 8, c & 0xFF
            continue
        l3_at = int(s[2])
        S = len(pkt) - at
        if S > 65535:
            continue
        seg = pkt[at:].copy()
        seg[6:8] = 0
        if hdr[l3_at] >> 4 == 4:
            pseudo = bytes(pkt[l3_at + 12:l3_at + 20]) + bytes([0, 17]) + S.to_bytes(2, "big")
        else:
            pseudo = bytes(pkt[l3_at + 8:l3_at + 40]) + S.to_bytes(4, "big") + bytes([0, 0, 0, 17])
        c = ~fold(word_sum(pseudo) + word_sum(seg)) & 0xFFFF
        c = c or 0xFFFF
        pkt[at + 6], pkt[at + 7] = c >> 8, c & 0xFF


def apply(arena: np.ndarray, hdr: bytes, sums, dst_off, lens, sets=()) -> np.ndarray:
    """In place on `arena` (numpy u8, the output of oracle.emit_batch with the
    same hdr / sets / dst_off / lens)."""
    hdr = bytes(hdr)
    check_args(hdr, sets, sums)
    H = len(hdr)
    for o, ln in zip(np.asarray(dst_off).astype(np.int64), np.asarray(lens).astype(np.int64)):
        one(arena[int(o):int(o) + H + int(ln)], hdr, sums)
    return arena
