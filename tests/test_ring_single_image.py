"""The single-image ring kernel (the slot ring's default, INGOT_TUNE_PIPE_DEPTH
= 0: one LDS image per wave, restaged in place once the walk has read it;
the key's value 1 is EINVAL, as it always was) returns the oracle's
records, and depth 2's, byte for byte: every blocks-per-CU setting
(INGOT_TUNE_RING_GRID), both record widths, every tile order
(INGOT_TUNE_XCD_REMAP), and nothing is written past record n - 1.

Sizes: a lone frame, the clamped tail tile (63, 65, 257, 4097), one full tile
(64), and 40,000.  At those sizes a 256-CU device gives every wave at most one
tile whatever the blocks per CU (40,000 frames are 625 tiles; one block per CU
is already 1,024 waves), so the restage would never run.  Two things make it
run: INGOT_TUNE_PIPELINE = k (k tiles per wave, the same kernel) at every size,
and two larger sizes, 200,001 and 300,001 frames (3,126 and 4,688 tiles), where
some waves get one tile more than others at 1 to 3 and at 4 blocks per CU.
"""
import functools

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import Chain
from ingot_amd.abi import (TUNE_PIPE_DEPTH, TUNE_PIPELINE, TUNE_RING_GRID, TUNE_XCD_REMAP)

pytestmark = pytest.mark.gpu

CHAINS = (Chain.UdpParser, Chain.GenericUlp, Chain.VlanUlp)
SIZES = [1, 63, 64, 65, 257, 4096 + 1, 40_000, 200_001, 300_001]
SENTINEL = 0xA5
EINVAL = -1
PAD = 256  # records behind record n - 1 that must stay untouched
POOL = 768


def _u16(v):
    return bytes([(v >> 8) & 0xFF, v & 0xFF])


@functools.lru_cache(maxsize=None)
def _adversarial_pool(stride: int, seed: int) -> np.ndarray:
    """POOL slots of `stride` bytes: every combination of no tag / VLAN / QinQ,
    IPv4 without options / with options (ihl 6..15: in 128-B slots the L4
    header then lies past the 64-B window) / IPv6 / IPv6 with 1..3 extension
    headers, over TCP / UDP / ICMP.  A frame longer than the slot is cut at
    the slot's end (truncated: its headers claim bytes the slot does not
    hold); a shorter one is followed by random bytes."""
    rng = np.random.default_rng(seed)
    rnd = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    slots = np.zeros((POOL, stride), np.uint8)
    for k in range(POOL):
        tag, l3, l4k = k % 3, (k // 3) % 4, (k // 12) % 3
        v6 = l3 >= 2
        tags = (b"", _u16(0x8100) + rnd(2), _u16(0x88A8) + rnd(2) + _u16(0x8100) + rnd(2))[tag]
        proto = ((6, 17, 1), (6, 17, 58))[v6][l4k]
        l4 = rnd(4) + (bytes(8) + bytes([int(rng.integers(5, 16)) << 4, 2]) + rnd(6)
                       if proto == 6 else rnd(4))
        if not v6:
            ihl = 5 if l3 == 0 else int(rng.integers(6, 16))
            hdr = (bytes([0x40 | ihl, 0]) + rnd(6) + bytes([64, proto]) + rnd(10) +
                   rnd(4 * (ihl - 5)))
            et = 0x0800
        else:
            ehs, nxt = b"", proto
            for _ in range(0 if l3 == 2 else int(rng.integers(1, 4))):
                kind = int(rng.choice([0, 43, 60, 44]))
                units = 0 if kind == 44 else int(rng.integers(0, 3))
                ehs = bytes([nxt, units]) + rnd(6 + 8 * units) + ehs
                nxt = kind
            hdr = bytes([0x60]) + rnd(5) + bytes([nxt, 64]) + rnd(32) + ehs
            et = 0x86DD
        frame = rnd(12) + tags + _u16(et) + hdr + l4
        frame = (frame + rnd(stride))[:stride]
        slots[k] = np.frombuffer(frame, np.uint8)
    return slots


_cache: dict = {}


def _dataset(kind: str, stride: int, n: int):
    """(device arena, {chain: 16-B oracle records on the device}), computed
    once per (frames, slot size, n) and shared by every setting."""
    import torch

    key = (kind, stride, n)
    if key not in _cache:
        if kind == "c2":
            arena, _, _ = ingot_amd.gen_frames(ingot_amd.GenProfile.V4UDP64, n, seed=n, stride=stride)
            a_np = arena.cpu().numpy()
        else:
            rng = np.random.default_rng(n + stride)
            # a tile of slack: the tail tile's idle lanes address slots >= n
            a_np = np.concatenate([_adversarial_pool(stride, stride)[rng.integers(0, POOL, n)]
                                   .reshape(-1), np.zeros(64 * stride, np.uint8)])
            arena = torch.from_numpy(a_np).cuda()
        want = {c: torch.from_numpy(
            oracle.parse_batch(a_np, None, None, c, stride=stride, n=n, nthreads=8)
            .view(np.uint8).reshape(n, 16).copy()).cuda() for c in CHAINS}
        _cache[key] = (arena, want)
    return _cache[key]


def _ctx(depth, grid=0, remap=0, tpw=0):
    ctx = ingot_amd.Context(0)
    ctx.set_tuning(TUNE_PIPE_DEPTH, depth)
    ctx.set_tuning(TUNE_RING_GRID, grid)
    ctx.set_tuning(TUNE_XCD_REMAP, remap)
    ctx.set_tuning(TUNE_PIPELINE, tpw)
    return ctx


def _run(ctx, arena, stride, n, chain, width):
    """Records into a sentinel-filled buffer of n + PAD; -> (records, tail)."""
    import torch

    out = torch.full(((n + PAD), width), SENTINEL, dtype=torch.uint8, device="cuda")
    if width == 16:
        ctx.parse_strided(arena, stride, n, chain, out=out)
    else:
        ctx.parse_strided_compact(arena, stride, n, chain, out=out)
    return out[:n], out[n:]


# one image (depth 0, the default): blocks per CU 1..4 in the default order, every order at 2 and 3
# blocks per CU, and k tiles per wave (the restage at small n)
SETTINGS = [dict(grid=g) for g in (1, 2, 3, 4)] + \
    [dict(grid=g, remap=r) for g in (2, 3) for r in (1, 2, 3, 4, 5)] + \
    [dict(tpw=k) for k in (2, 3, 8)] + [dict(tpw=2, remap=3), dict(tpw=3, remap=2)]


@pytest.mark.parametrize("n", SIZES)
def test_single_image_ring_bit_exact(n):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctxs = [_ctx(0, **kw) for kw in SETTINGS]
    ref = _ctx(2)
    for kind, stride in (("c2", 64), ("adv", 64), ("adv", 128)):
        arena, want = _dataset(kind, stride, n)
        for chain in CHAINS:
            w16 = want[chain]
            w8 = torch.from_numpy(ingot_amd.rec16_to_rec8(
                ingot_amd.records_to_numpy(w16)).view(np.uint8).reshape(n, 8).copy()).cuda()
            for width, w in ((16, w16), (8, w8)):
                d2, _ = _run(ref, arena, stride, n, chain, width)
                assert torch.equal(d2, w), ("depth 2", kind, stride, chain, width)
                for kw, ctx in zip(SETTINGS, ctxs):
                    got, tail = _run(ctx, arena, stride, n, chain, width)
                    where = (kw, kind, stride, chain, width)
                    assert torch.equal(got, w), ("oracle", *where)
                    assert torch.equal(got, d2), ("depth 2", *where)
                    assert bool((tail == SENTINEL).all()), ("wrote past record n - 1", *where)


def test_adversarial_pool_covers_the_cases():
    """The host-built mix holds what it claims, by the oracle's own records:
    frames that parse and frames that fail in each chain, at both slot sizes
    (the 64-B slots cut the long header stacks short)."""
    for stride in (64, 128):
        a = np.concatenate([_adversarial_pool(stride, stride).reshape(-1), np.zeros(256, np.uint8)])
        for chain in CHAINS:
            st = ingot_amd.records_to_numpy(
                oracle.parse_batch(a, None, None, chain, stride=stride, n=POOL)
                .view(np.uint8).reshape(POOL, 16))["status"]
            assert (st == 0).any() and (st != 0).any(), (stride, chain)


def test_pipe_depth_range():
    """INGOT_TUNE_PIPE_DEPTH takes 0 (the default: one image for the slot
    ring) and 2 to 4; 1, 5 and negative values are EINVAL and leave the
    setting alone.  (0 cannot be EINVAL: by the ABI's rule for every knob it
    restores the default; 1 stays EINVAL as before, the single image being
    what the default selects.)  The call rejects before any launch, but a
    context needs a device."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = ingot_amd.Context(0)
    c.set_tuning(TUNE_PIPE_DEPTH, 3)
    for bad in (1, 5, -1, 64):
        assert c._lib.ingot_gpu_ctx_set_tuning(c._h, TUNE_PIPE_DEPTH, bad) == EINVAL, bad
    assert c.get_tuning(TUNE_PIPE_DEPTH) == 3
    for ok in (0, 2, 3, 4):
        c.set_tuning(TUNE_PIPE_DEPTH, ok)
        assert c.get_tuning(TUNE_PIPE_DEPTH) == ok
