"""The slot ring's tile loop with scalar cursors (k_parse_pipe: a wave-uniform
tile base plus a per-lane 32-bit offset for the staging loads, the
past-window pointer and the record store; the clamped addressing only in the
batch's tail tile; 64-B slots through the staging instruction's immediate
offset, every other stride through four per-lane offsets) returns the
oracle's records, and depth 2's, byte for byte, and writes nothing past
record n - 1.

Tiles per wave: INGOT_TUNE_PIPELINE = k gives every wave k tiles, and
INGOT_TUNE_XCD_REMAP = 4 (hardware block order) makes wave w of the W in the
grid take tiles w, w + W, ... .  At 769 frames (13 tiles) and k = 3 that is 5
waves in 2 blocks, W = 8: waves 0..4 run two tiles each, and the clamped tail
(tile 12) is wave 4's last tile.  At 65 frames the tail is a wave's only tile.

Frames: option-less IPv4/UDP ("decided": all its fields sit at fixed
offsets) and the kinds a fixed-offset reading cannot decide (_UNDECIDED).
"""
import functools

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import Chain
from ingot_amd.abi import TUNE_PIPE_DEPTH, TUNE_PIPELINE, TUNE_XCD_REMAP

pytestmark = pytest.mark.gpu

CHAINS = (Chain.UdpParser, Chain.GenericUlp, Chain.VlanUlp)
SIZES = [1, 63, 64, 65, 129, 769, 4097]
PIPELINES = (0, 2, 3, 8)
SENTINEL = 0xA5
PAD = 256  # records behind record n - 1 that must stay untouched
OK, UNWANTED, TOO_SMALL = 0, 1, 3


def _u16(v):
    return bytes([(v >> 8) & 0xFF, v & 0xFF])


def _v4(rnd, proto, ihl=5):
    return bytes([0x40 | ihl, 0]) + rnd(6) + bytes([64, proto]) + rnd(10) + rnd(4 * max(ihl - 5, 0))


def _v6(rnd, rng, proto, n_eh=0, units=None):
    ehs, nxt = b"", proto
    for _ in range(n_eh):
        kind = int(rng.choice([0, 43, 60, 44]))
        u = 0 if kind == 44 else (int(rng.integers(0, 3)) if units is None else units)
        ehs = bytes([nxt, u]) + rnd(6 + 8 * u) + ehs
        nxt = kind
    return bytes([0x60]) + rnd(5) + bytes([nxt, 64]) + rnd(32) + ehs


def _tcp(rnd, doff):
    return rnd(12) + bytes([doff << 4, 2]) + rnd(6) + rnd(4 * max(doff - 5, 0))


def _eth(rnd, et, tags=b""):
    return rnd(12) + tags + _u16(et)


def _decided(rnd, rng):
    return _eth(rnd, 0x0800) + _v4(rnd, 17) + rnd(8)


# The kinds a reading of fixed offsets cannot decide, one builder each.
_UNDECIDED = {
    "v4_options": lambda rnd, rng: _eth(rnd, 0x0800) + _v4(rnd, 17, int(rng.integers(6, 16))) + rnd(8),
    "v6_ext": lambda rnd, rng: _eth(rnd, 0x86DD) + _v6(rnd, rng, 17, int(rng.integers(1, 4))) + rnd(8),
    "vlan": lambda rnd, rng: _eth(rnd, 0x0800, _u16(0x8100) + rnd(2)) + _v4(rnd, 17) + rnd(8),
    "qinq": lambda rnd, rng: _eth(rnd, 0x0800, _u16(0x88A8) + rnd(2) + _u16(0x8100) + rnd(2)) +
    _v4(rnd, 17) + rnd(8),
    "arp": lambda rnd, rng: _eth(rnd, 0x0806) + rnd(28),
    "ethertype": lambda rnd, rng: _eth(rnd, 0x9000 | int(rng.integers(0, 256))) + rnd(40),
    "ihl_low": lambda rnd, rng: _eth(rnd, 0x0800) + _v4(rnd, 17, int(rng.integers(0, 5))) + rnd(8),
    "tcp": lambda rnd, rng: _eth(rnd, 0x0800) + _v4(rnd, 6) + _tcp(rnd, int(rng.integers(5, 8))),
    "tcp_past_slot": lambda rnd, rng: _eth(rnd, 0x0800) + _v4(rnd, 6) + _tcp(rnd, 15) + rnd(200),
    "icmp": lambda rnd, rng: _eth(rnd, 0x0800) + _v4(rnd, 1) + rnd(8),
    "icmp6": lambda rnd, rng: _eth(rnd, 0x86DD) + _v6(rnd, rng, 58) + rnd(8),
    "v6_udp": lambda rnd, rng: _eth(rnd, 0x86DD) + _v6(rnd, rng, 17) + rnd(8),
    "gre": lambda rnd, rng: _eth(rnd, 0x0800) + _v4(rnd, 47) + rnd(8),
    # cut at the slot's end: the headers claim bytes the slot does not hold
    "cut_v6_ext": lambda rnd, rng: _eth(rnd, 0x86DD) + _v6(rnd, rng, 17, 3, units=15),
    # a 72-B destination-options header: UDP starts at byte 126 (cut in a
    # 128-B slot at L4, in a 64-B slot at L3)
    "cut_l4": lambda rnd, rng: _eth(rnd, 0x86DD) + bytes([0x60]) + rnd(5) + bytes([60, 64]) + rnd(32) +
    bytes([17, 8]) + rnd(70) + rnd(8),
    "cut_qinq_opts": lambda rnd, rng: _eth(rnd, 0x0800, _u16(0x88A8) + rnd(2) + _u16(0x8100) + rnd(2)) +
    _v4(rnd, 17, 15) + rnd(8),
}
_KINDS = tuple(_UNDECIDED)


def _slots(classes, stride, seed):
    """One slot of `stride` bytes per entry of `classes` (-1: decided, k >= 0:
    _KINDS[k]); a frame longer than the slot is cut, a shorter one is followed
    by random bytes."""
    rng = np.random.default_rng(seed)
    rnd = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    out = np.zeros((len(classes), stride), np.uint8)
    for i, c in enumerate(classes):
        f = _decided(rnd, rng) if c < 0 else _UNDECIDED[_KINDS[c]](rnd, rng)
        out[i] = np.frombuffer((f + rnd(stride))[:stride], np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def _pool(stride):
    """A pool of 4 decided frames and 4 of every undecided kind."""
    classes = [-1] * 4 + [k for k in range(len(_KINDS)) for _ in range(4)]
    return _slots(classes, min(stride, 512), 1000 + stride)


def _mixed(n, stride, seed):
    """n slots drawn from the pool (wide slots: the pool's 512 bytes, then zeros)."""
    rng = np.random.default_rng(seed)
    pool = _pool(stride)
    a = np.zeros((n, stride), np.uint8)
    a[:, :pool.shape[1]] = pool[rng.integers(0, len(pool), n)]
    return a


_cache: dict = {}


def _dataset(key, make, stride, n, base=0):
    """(device arena view starting `base` bytes into its allocation, {chain:
    16-B oracle records on the device}); computed once per key."""
    import torch

    key = (key, stride, n, base)
    if key not in _cache:
        slots = make()
        assert slots.shape == (n, stride)
        a_np = slots.reshape(-1)
        buf = torch.zeros(base + a_np.size, dtype=torch.uint8, device="cuda")
        buf[base:] = torch.from_numpy(a_np).cuda()
        want = {c: torch.from_numpy(
            oracle.parse_batch(a_np, None, None, c, stride=stride, n=n, nthreads=8)
            .view(np.uint8).reshape(n, 16).copy()).cuda() for c in CHAINS}
        _cache[key] = (buf[base:], want)
    return _cache[key]


def _ctx(depth, tpw=0, remap=4):
    ctx = ingot_amd.Context(0)
    ctx.set_tuning(TUNE_PIPE_DEPTH, depth)
    ctx.set_tuning(TUNE_XCD_REMAP, remap)
    ctx.set_tuning(TUNE_PIPELINE, tpw)
    return ctx


def _run(ctx, arena, stride, n, chain, width):
    import torch

    out = torch.full(((n + PAD), width), SENTINEL, dtype=torch.uint8, device="cuda")
    if width == 16:
        ctx.parse_strided(arena, stride, n, chain, out=out)
    else:
        ctx.parse_strided_compact(arena, stride, n, chain, out=out)
    return out[:n], out[n:]


def _check(arena, want, stride, n, pipelines=PIPELINES, depths=(0,), what=()):
    """Every chain and record width, at each tiles-per-wave setting: the
    oracle's records, depth 2's on the device, and the sentinel behind."""
    import torch

    ref = _ctx(2)
    for chain in CHAINS:
        w16 = want[chain]
        w8 = torch.from_numpy(ingot_amd.rec16_to_rec8(
            ingot_amd.records_to_numpy(w16)).view(np.uint8).reshape(n, 8).copy()).cuda()
        for width, w in ((16, w16), (8, w8)):
            d2, _ = _run(ref, arena, stride, n, chain, width)
            assert torch.equal(d2, w), ("depth 2 vs oracle", *what, stride, n, chain, width)
            for depth in depths:
                for tpw in pipelines:
                    got, tail = _run(_ctx(depth, tpw), arena, stride, n, chain, width)
                    where = (*what, depth, tpw, stride, n, chain, width)
                    assert torch.equal(got, w), ("oracle", *where)
                    assert torch.equal(got, d2), ("depth 2", *where)
                    assert bool((tail == SENTINEL).all()), ("wrote past record n - 1", *where)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_tiles_per_wave(n):
    """64-B slots (immediate offsets) and 128-B slots (per-lane offsets and
    past-window reads), mixed frames; depths 0, 3 and 4 share the loop."""
    for stride in (64, 128):
        arena, want = _dataset("mixed", lambda: _mixed(n, stride, n), stride, n)
        _check(arena, want, stride, n, depths=(0, 3, 4) if n == 769 else (0,))


@pytest.mark.parametrize("stride,n", [(80, 769), (128, 769), (256, 769), (65520, 130)])
def test_strides(stride, n):
    arena, want = _dataset("mixed", lambda: _mixed(n, stride, stride), stride, n)
    _check(arena, want, stride, n, pipelines=(0, 3))


@pytest.mark.parametrize("base", [16, 48, 112])
def test_arena_base_not_line_aligned(base):
    for stride in (64, 80):
        n = 769
        arena, want = _dataset("mixed", lambda: _mixed(n, stride, base), stride, n, base=base)
        assert arena.data_ptr() % 128 == base
        _check(arena, want, stride, n, pipelines=(0, 3), what=(base,))


# Tile composition: 24 tiles less 5 frames (a clamped tail), 3 tiles per wave
# in hardware block order: 8 waves in 2 blocks, wave w runs tiles w, w + 8, w + 16.
_TILES, _W, _N = 24, 8, 24 * 64 - 5
_MIX_SEED = 7


def _tile_classes(kind):
    """Per-slot classes for the _N slots, and per tile whether every lane is decided."""
    rng = np.random.default_rng(_MIX_SEED)
    cls = np.full(_TILES * 64, -1, np.int64)
    if kind == "all_decided":
        fast = np.ones(_TILES, bool)
    elif kind == "all_undecided":
        cls[:] = rng.integers(0, len(_KINDS), cls.size)
        fast = np.zeros(_TILES, bool)
    elif kind == "one_undecided":
        for t in range(_TILES):
            cls[t * 64 + (0, 31, 63)[t % 3]] = t % len(_KINDS)
        fast = np.zeros(_TILES, bool)
    else:  # per tile: all decided, one undecided lane, or all undecided
        pick = rng.integers(0, 3, _TILES)
        for t in range(_TILES):
            if pick[t] == 1:
                cls[t * 64 + int(rng.integers(0, 64))] = int(rng.integers(0, len(_KINDS)))
            elif pick[t] == 2:
                cls[t * 64:(t + 1) * 64] = rng.integers(0, len(_KINDS), 64)
        fast = pick == 0
    return cls[:_N], fast


def test_drawn_tile_order_alternates():
    """The drawn classes give some wave fast -> fallback -> fast and another
    fallback -> fast -> fallback (wave w: tiles w, w + 8, w + 16)."""
    _, fast = _tile_classes("drawn")
    runs = {tuple(bool(fast[w + j * _W]) for j in range(3)) for w in range(_W)}
    assert (True, False, True) in runs and (False, True, False) in runs, runs


@pytest.mark.parametrize("kind", ["all_decided", "one_undecided", "all_undecided", "drawn"])
def test_tile_composition(kind):
    cls, _ = _tile_classes(kind)
    for stride in (64, 128):
        arena, want = _dataset(kind, lambda: _slots(cls, stride, 31 + stride), stride, _N)
        _check(arena, want, stride, _N, pipelines=(3,), what=(kind,))


def test_pools_cover_the_statuses():
    """By the oracle alone: the pool holds Ok frames and, in every chain,
    Unwanted and TooSmall at the L3 and at the L4 layer.  (A slot is at least
    64 bytes, so Ethernet and the VLAN tags, which end by byte 22, cannot be
    TooSmall, and neither layer returns Unwanted.)"""
    for stride in (64, 128):
        pool = _pool(stride)
        a = pool.reshape(-1)
        for chain in CHAINS:
            r = ingot_amd.records_to_numpy(
                oracle.parse_batch(a, None, None, chain, stride=stride, n=len(pool))
                .view(np.uint8).reshape(len(pool), 16))
            l3 = 2 if chain == Chain.VlanUlp else 1
            seen = set(zip(r["status"].tolist(), r["err_layer"].tolist()))
            assert any(s == OK for s, _ in seen), (stride, chain)
            for need in ((UNWANTED, l3), (UNWANTED, l3 + 1), (TOO_SMALL, l3), (TOO_SMALL, l3 + 1)):
                assert need in seen, (need, stride, chain, sorted(seen))
