"""The definition of ingot_gpu_parse_modify_csum's checksum update
(include/ingot_gpu.h), in numpy / Python.  TEST INFRASTRUCTURE ONLY.

Written from RFC 1624, not from the kernel: the kernel accumulates a term per
edited byte; this model compares the covered 16-bit words of the frame before
the call with the same words after the edits, so the two share no code path.

  RFC 1624 eqn. 3   HC' = ~(~HC + ~m + m')   in ones'-complement arithmetic
  RFC 768           UDP: a field of 0 means "no checksum"; a computed 0 is
                    sent as 0xffff

Words are the big-endian 16-bit words at even FRAME offsets (every header of
every chain starts at an even frame offset).  For a sum whose field holds HC
after the edits, D = sum of (~m + m') mod 0xffff over the covered words.
D == 0: the field is not written.  Otherwise x = (~HC + D) mod 0xffff taken
in [1, 0xffff] and HC' = ~x.

`before` is the arena before the call, `after` what
oracle.parse_modify_batch left of a copy of it (updated here in place),
`recs` its records, `o_udp` (tunnel chain only) the outer UDP header's offsets
from oracle.geneve_fields_batch (`outer_udp_off`).
"""
from __future__ import annotations

import numpy as np

from ingot_amd.abi import CSUM_L3, CSUM_L4, CSUM_OUTER_L4, L3Kind, L4Kind
from tests.csum_model import word_sum

_FIELD_AT = {int(L4Kind.TCP): 16, int(L4Kind.UDP): 6, int(L4Kind.ICMPV4): 2,
             int(L4Kind.ICMPV6): 2}
_FIXED = {int(L4Kind.TCP): 20, int(L4Kind.UDP): 8, int(L4Kind.ICMPV4): 4, int(L4Kind.ICMPV6): 4}
# the layers tests/csum_model.py sums with a pseudo-header (ICMPv4 has none)
_PSEUDO = (int(L4Kind.TCP), int(L4Kind.UDP), int(L4Kind.ICMPV6))


def _word(f, at: int) -> int:
    """The word at even frame offset `at`; a byte past the frame counts as 0."""
    lo = int(f[at + 1]) if at + 1 < len(f) else 0
    return (int(f[at]) << 8) | lo


def delta(b, a, ranges, field: int) -> int:
    """D over the words of the byte ranges [lo, hi) (even `lo`), the word at
    `field` left out: sum of (~m + m') mod 0xffff.  Since ~m = 0xffff - m,
    that is the words of `a` minus the words of `b`, mod 0xffff (a long range,
    the tunnel's outer sum, is then two numpy sums)."""
    d = 0
    for lo, hi in ranges:
        assert lo % 2 == 0
        d += word_sum(a[lo:hi]) - word_sum(b[lo:hi])
        if lo <= field < hi:
            d -= _word(a, field) - _word(b, field)
    return d % 0xFFFF


def eqn3(hc: int, d: int) -> int:
    """RFC 1624 eqn. 3 for a delta d != 0 (mod 0xffff)."""
    x = ((~hc & 0xFFFF) + d) % 0xFFFF
    if x == 0:
        x = 0xFFFF
    return ~x & 0xFFFF


def _apply(a, field: int, d: int, udp: bool) -> None:
    if d == 0:
        return  # the sum did not move: the representation is kept
    hc = _word(a, field)
    if udp and hc == 0:
        return
    n = eqn3(hc, d)
    if udp and n == 0:
        n = 0xFFFF
    a[field], a[field + 1] = n >> 8, n & 0xFF


def one(b: np.ndarray, a: np.ndarray, rec, what: int, o_udp=None) -> None:
    """One frame: `b` its bytes before the call, `a` (writable) after the
    edits; the selected checksum fields of `a` are updated."""
    if int(rec["status"]) != 0:
        return
    L = len(a)
    l3_kind, l4_kind = int(rec["l3_kind"]), int(rec["l4_kind"])
    l3_off, l4_off = int(rec["l3_off"]), int(rec["l4_off"])
    v4 = l3_kind == int(L3Kind.IPV4)
    if (what & CSUM_L3) and v4:
        hl = min(max(20, (int(a[l3_off]) & 0xF) * 4), L - l3_off)
        _apply(a, l3_off + 10, delta(b, a, [(l3_off, l3_off + hl)], l3_off + 10), False)
    if (what & CSUM_L4) and l4_kind in _FIELD_AT:
        later_fragment = v4 and (_word(a, l3_off + 6) & 0x1FFF) != 0
        if not later_fragment:
            ranges = [(l4_off, l4_off + _FIXED[l4_kind])]
            if v4 and l4_kind in _PSEUDO:
                ranges.append((l3_off + 12, l3_off + 20))
            field = l4_off + _FIELD_AT[l4_kind]
            _apply(a, field, delta(b, a, ranges, field), l4_kind == int(L4Kind.UDP))
    if what & CSUM_OUTER_L4:
        # after the inner sums: their rewritten fields are covered bytes
        o = int(o_udp)
        _apply(a, o + 6, delta(b, a, [(o, L)], o + 6), True)


def update(before, after, off, lens, recs, what, o_udp=None, stride: int = 0, n=None):
    """In place on `after` (numpy u8); returns it."""
    if what == 0 or what & ~(CSUM_L3 | CSUM_L4 | CSUM_OUTER_L4):
        raise ValueError("what")
    if (what & CSUM_OUTER_L4) and o_udp is None:
        raise ValueError("CSUM_OUTER_L4 needs the outer UDP offsets")
    if n is None:
        n = len(off) if off is not None else len(recs)
    for i in range(n):
        o = int(off[i]) if off is not None else i * stride
        ln = int(lens[i]) if lens is not None else stride
        one(before[o:o + ln], after[o:o + ln], recs[i], what,
            None if o_udp is None else o_udp[i])
    return after
