"""Hand-built frames for the checksum tests (tests/test_checksum_model.py,
tests/test_checksum.py).  Frames are laid out field by field with every
checksum field 0; the tests parse them with the oracle and run the model's
fill (tests/csum_model.py) to make them valid, then break them on purpose.
"""
from __future__ import annotations

import numpy as np

TCP, UDP, ICMP4, ICMP6 = 6, 17, 1, 58


def u16(v: int) -> bytes:
    return int(v & 0xFFFF).to_bytes(2, "big")


def eth(ethertype: int, vlan=()) -> bytes:
    tags = b"".join(u16(0x8100) + u16(v) for v in vlan)
    return bytes.fromhex("02aabbccdd0102aabbccdd02") + tags + u16(ethertype)


def l4(proto: int, payload: bytes) -> bytes:
    if proto == TCP:
        return (u16(49152) + u16(443) + (0x01020304).to_bytes(4, "big") + bytes(4) +
                bytes([0x50, 0x18]) + u16(0xFFFF) + u16(0) + u16(0) + payload)
    if proto == UDP:
        return u16(53) + u16(40000) + u16(8 + len(payload)) + u16(0) + payload
    return bytes([8 if proto == ICMP4 else 128, 0]) + u16(0) + u16(0x1234) + u16(1) + payload


def v4(proto: int, body: bytes, options: bytes = b"", flags_frag: int = 0x4000,
       total_len: int | None = None) -> bytes:
    assert len(options) % 4 == 0
    hl = 20 + len(options)
    tl = hl + len(body) if total_len is None else total_len
    return (bytes([0x40 | (hl // 4), 0]) + u16(tl) + u16(0x1C46) + u16(flags_frag) +
            bytes([64, proto]) + u16(0) + bytes([192, 168, 0, 1, 192, 168, 0, 199]) + options +
            body)


def v6(proto: int, body: bytes, ext=(), payload_len: int | None = None) -> bytes:
    """ext = ((type, bytes after the 2-byte EH head), ...): `type` is the
    value that selects the EH, so each EH's own next-header byte names the
    one after it (the last: `proto`)."""
    ehs, nh = b"", proto
    for ty, data in reversed(ext):
        assert (len(data) + 2) % 8 == 0
        ehs = bytes([nh, 0 if ty == 44 else (len(data) + 2) // 8 - 1]) + data + ehs
        nh = ty
    pl = len(ehs) + len(body) if payload_len is None else payload_len
    src = bytes.fromhex("20010db8000000000000000000000001")
    dst = bytes.fromhex("20010db80000000000000000000000c7")
    return bytes([0x60, 0, 0, 0]) + u16(pl) + bytes([nh, 64]) + src + dst + ehs + body


def frag_eh(offset8: int, more: int, ident: int = 0xCAFE) -> tuple:
    """An IPv6 Fragment header's bytes after (next header, reserved)."""
    return (44, u16((offset8 << 3) | more) + ident.to_bytes(4, "big"))


def frame(l3: str, proto: int, payload: bytes, vlan=(), **kw) -> bytes:
    body = l4(proto, payload)
    if l3 == "v4":
        return eth(0x0800, vlan) + v4(proto, body, **kw)
    return eth(0x86DD, vlan) + v6(proto, body, **kw)


def place(frames, offsets=None, gap: int = 0, fill: int = 0xA5, misalign: int = 0):
    """-> (arena u8, off u64, lens u16): frames at `offsets`, or one after
    another from byte `misalign` with `gap` bytes between them; every byte
    that belongs to no frame is `fill`."""
    if offsets is None:
        offsets, o = [], misalign
        for f in frames:
            offsets.append(o)
            o += len(f) + gap
    size = max(o + len(f) for o, f in zip(offsets, frames)) + 64
    arena = np.full((size + 15) // 16 * 16, fill, dtype=np.uint8)
    for o, f in zip(offsets, frames):
        arena[o:o + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
    return (arena, np.array(offsets, dtype=np.uint64),
            np.array([len(f) for f in frames], dtype=np.uint16))
