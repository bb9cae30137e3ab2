"""ingot_gpu_parse_modify_csum on the device: the rewrite with the fused RFC
1624 checksum update, against its definition (tests/csum_update_model.py over
the oracle's rewrite) byte for byte, and against the two-pass way, rewrite +
checksum fill, on the packets that fill sums (at least 90 % of each batch)."""
import json
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import Chain, EditOp, Field, GenProfile
from ingot_amd.abi import (CSUM_L3, CSUM_L4, CSUM_OUTER_L4, TUNE_PIPE_DEPTH, TUNE_PIPELINE,
                           TUNE_WRITEBACK)
from ingot_amd.hostgen import gen_frames_host
from tests import csum_frames as cf
from tests import csum_model as model
from tests import csum_update_model as upd

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "csum_update_kats.json").read_text())
TUN = Chain.GeneveOverV6Tunnel
OK, NONE = 1, 0
SET, ADD, SUB, XOR, OR = EditOp.SET, EditOp.ADD, EditOp.SUB, EditOp.XOR, EditOp.OR


def edits_for(l3: int):
    """The eight edits of tests/test_csum_update_model.py, the L3 layer at
    label `l3` and the L4 layer after it."""
    l4 = l3 + 1
    return [(l3, Field.V4_HOP_LIMIT, SUB, 1), (l3, Field.V4_SOURCE, SET, 0x0A000001),
            (l3, Field.V4_DESTINATION, XOR, 0x00FF00FF), (l4, Field.UDP_DESTINATION, SUB, 1),
            (l4, Field.TCP_SOURCE, SET, 0), (l4, Field.TCP_FLAGS, OR, 0x10),
            (l3, Field.V4_DSCP, SET, 0x2E), (l3, Field.V6_HOP_LIMIT, SUB, 1)]


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return ingot_amd.Context(0)


def on_gpu(torch, c, arena, off, lens, chain, edits, what, stride=0, n=None):
    """-> (arena after the call, records), numpy."""
    d_arena = torch.from_numpy(np.array(arena)).cuda()  # (a copy: shared inputs are read-only)
    d_off = None if off is None else torch.from_numpy(off.view(np.int64)).cuda()
    d_len = None if lens is None else torch.from_numpy(lens.view(np.int16)).cuda()
    n = len(off) if n is None else n
    recs = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    c.parse_modify(d_arena, d_off, d_len, chain, edits, stride=stride, n=n, out=recs, csum=what)
    torch.cuda.synchronize()
    return d_arena.cpu().numpy(), recs.cpu().numpy()


def by_model(arena, off, lens, chain, edits, what, stride=0, n=None):
    """-> (the definition's arena, the rewrite alone, records)."""
    rewritten = arena.copy()
    recs = oracle.parse_modify_batch(rewritten, off, lens, chain, edits, stride=stride, n=n,
                                     nthreads=8)
    o_udp = None
    if chain == TUN:
        o_udp = oracle.geneve_fields_batch(arena, off, lens, stride=stride,
                                           n=n)["outer"]["outer_udp_off"]
    want = upd.update(arena, rewritten.copy(), off, lens, recs, what, o_udp=o_udp, stride=stride,
                      n=n)
    return want, rewritten, recs


def same(got, want, what=""):
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, (what, diff[:10], got[diff[:10]], want[diff[:10]])


def same_frames(got, want, off, lens, keep):
    assert keep.sum() >= 0.9 * len(keep), (int(keep.sum()), len(keep))
    for i in np.nonzero(keep)[0]:
        o, ln = int(off[i]), int(lens[i])
        assert got[o:o + ln].tobytes() == want[o:o + ln].tobytes(), i


# ---------------------------------------------------------------------------
# Indexed frames at odd addresses
# ---------------------------------------------------------------------------
@lru_cache(maxsize=None)
def valid_frames(profile, seed, chain, misalign):
    """2,000 generated frames, placed again one after another from byte
    `misalign` with 3 bytes between them, their checksums made valid; and the
    packets whose sums the fill computes."""
    a, o, ln = gen_frames_host(profile, 2000, seed=seed, slack=64)
    frames = [a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, ln)]
    arena, off, lens = cf.place(frames, gap=3, misalign=misalign)
    rows = model.fill(arena, off, lens, oracle.parse_batch(arena, off, lens, chain))
    keep = (rows["l4_state"] == OK) & ((rows["l3_state"] == OK) | (rows["l3_state"] == NONE))
    arena.setflags(write=False)
    return arena, off, lens, keep


# VLAN_V6EH seed 35: chosen on the CPU so that the packets fill sums (all but
# the profile's IPv6 fragments, 1,819 of 2,000) reach the 90 % the comparison
# with the two-pass way asks for; MIXED seed 31: 1,908.
@pytest.mark.parametrize("chain,profile,seed,l3,misalign", [
    (Chain.GenericUlp, GenProfile.MIXED, 31, 1, 1), (Chain.UdpParser, GenProfile.MIXED, 31, 1, 7),
    (Chain.VlanUlp, GenProfile.VLAN_V6EH, 35, 2, 13)])
def test_indexed_frames_at_odd_addresses(ctx, torch, chain, profile, seed, l3, misalign):
    """2,000 frames (a partial last tile) at odd addresses: word parity follows
    the frame offset, write-back sectors the address.  The 3-chunk window puts
    TCP's field past the staged bytes and UDP's inside: both store paths."""
    fill_chain = Chain.GenericUlp if chain == Chain.UdpParser else chain
    arena, off, lens, keep = valid_frames(profile, seed, fill_chain, misalign)
    edits = edits_for(l3)
    want, rewritten, w_rec = by_model(arena, off, lens, chain, edits, CSUM_L3 | CSUM_L4)
    got, recs = on_gpu(torch, ctx, arena, off, lens, chain, edits, CSUM_L3 | CSUM_L4)
    assert recs.tobytes() == w_rec.tobytes()
    same(got, want, chain)
    two_pass = rewritten.copy()
    model.fill(two_pass, off, lens, w_rec)
    same_frames(got, two_pass, off, lens, keep)
    # both store paths were taken: a rewritten checksum inside the staged
    # window (48 B from the 16-B block the frame starts in) and one past it
    if chain == Chain.GenericUlp:
        inside = past = 0
        for i in np.nonzero((w_rec["status"] == 0) & (w_rec["l4_kind"] != 0))[0]:
            at = int(w_rec["l4_off"][i]) + (0, 16, 6, 2, 2)[int(w_rec["l4_kind"][i])]
            a = int(off[i]) + at
            if got[a:a + 2].tobytes() != arena[a:a + 2].tobytes():
                staged_end = 48 - int(off[i]) % 16  # (device allocations are 16-B aligned)
                inside += at + 2 <= staged_end
                past += at >= staged_end
        assert inside > 100 and past > 100, (inside, past)


def test_plain_rewrite_is_unchanged(ctx, torch):
    """parse_modify(csum=0) takes the old call: the oracle's rewrite, byte for byte."""
    arena, off, lens, _ = valid_frames(GenProfile.MIXED, 31, Chain.GenericUlp, 1)
    want = arena.copy()
    w_rec = oracle.parse_modify_batch(want, off, lens, Chain.GenericUlp, edits_for(1))
    got, recs = on_gpu(torch, ctx, arena, off, lens, Chain.GenericUlp, edits_for(1), 0)
    assert recs.tobytes() == w_rec.tobytes()
    same(got, want)


# ---------------------------------------------------------------------------
# Slot rings (k_modify_pipe) and the same slots through k_parse
# ---------------------------------------------------------------------------
RING_N = 100_003  # as tests/test_modify.py's ring cases: a partial last tile
RING_EDITS = [(2, Field.UDP_DESTINATION, SUB, 1), (1, Field.V4_HOP_LIMIT, SUB, 1)]


@pytest.fixture(scope="module")
def ring64(ctx, torch):
    """V4UDP64 slots with valid checksums (the device's fill), what the
    definition makes of them, and the two-pass result."""
    n = RING_N
    d_arena, _, _ = ingot_amd.gen_frames(GenProfile.V4UDP64, n, stride=64)
    recs = ctx.parse_strided(d_arena, 64, n, Chain.UdpParser)
    ctx.checksum_fill(d_arena, None, None, recs, stride=64, n=n)
    torch.cuda.synchronize()
    arena = d_arena.cpu().numpy()
    want, _, w_rec = by_model(arena, None, None, Chain.UdpParser, RING_EDITS, 3, stride=64, n=n)
    d_two = torch.from_numpy(arena).cuda()
    ctx.parse_modify(d_two, None, None, Chain.UdpParser, RING_EDITS, stride=64, n=n)
    ctx.checksum_fill(d_two, None, None, recs, stride=64, n=n)
    torch.cuda.synchronize()
    assert (want != arena).any()
    return arena, want, w_rec, d_two.cpu().numpy()


@pytest.mark.parametrize("tune", [dict(depth=2, wb=16), dict(depth=2, wb=32), dict(depth=2, wb=64),
                                  dict(depth=3, wb=16), dict(depth=3, wb=32), dict(depth=3, wb=64),
                                  dict(depth=2, wb=64, pipe=3), dict(depth=3, wb=32, pipe=5),
                                  dict(pipe=1)])
def test_slot_ring_64(torch, ring64, tune):
    """64-B slots for every depth and write-back unit; pipe = k gives every
    wave k tiles, so the images rotate; pipe = 1 is k_parse on the same slots."""
    arena, want, w_rec, two_pass = ring64
    c = ingot_amd.Context(0)
    c.set_tuning(TUNE_PIPE_DEPTH, tune.get("depth", 0))
    c.set_tuning(TUNE_WRITEBACK, tune.get("wb", 0))
    c.set_tuning(TUNE_PIPELINE, tune.get("pipe", 0))
    got, recs = on_gpu(torch, c, arena, None, None, Chain.UdpParser, RING_EDITS, 3, stride=64,
                       n=RING_N)
    assert recs.tobytes() == w_rec.tobytes()
    same(got, want, tune)
    same(got, two_pass, tune)  # every slot is a whole IPv4 UDP packet: fill sums them all


@pytest.mark.parametrize("tune", [dict(), dict(depth=3, wb=16, pipe=3), dict(pipe=1)])
def test_slot_ring_128_field_past_the_window(ctx, torch, tune):
    """128-B slots holding IPv6 + TCP: the field at byte 70 lies past the
    64-B window, so it is stored directly; every third slot IPv4 + UDP."""
    n = 4 * 64 * 3 + 5
    pay6, pay4 = bytes(range(54)), bytes(range(86))
    frames = [cf.frame("v4", cf.UDP, pay4) if i % 3 == 2 else cf.frame("v6", cf.TCP, pay6)
              for i in range(n)]
    assert {len(f) for f in frames} == {128}
    arena = np.frombuffer(b"".join(frames), dtype=np.uint8).copy()
    for i in range(n):  # distinct ports and addresses
        arena[i * 128 + 5] = i & 0xFF
        o = i * 128 + (34 if i % 3 == 2 else 54)
        arena[o], arena[o + 1] = (i >> 8) & 0xFF, i & 0xFF
    rows = model.fill(arena, None, None, oracle.parse_batch(arena, None, None, Chain.GenericUlp,
                                                            stride=128, n=n), stride=128, n=n)
    assert (rows["l4_state"] == OK).all()
    edits = edits_for(1) + [(2, Field.TCP_DESTINATION, SET, 8443)]
    want, rewritten, w_rec = by_model(arena, None, None, Chain.GenericUlp, edits, 3, stride=128,
                                      n=n)
    c = ingot_amd.Context(0)
    c.set_tuning(TUNE_PIPE_DEPTH, tune.get("depth", 0))
    c.set_tuning(TUNE_WRITEBACK, tune.get("wb", 0))
    c.set_tuning(TUNE_PIPELINE, tune.get("pipe", 0))
    got, recs = on_gpu(torch, c, arena, None, None, Chain.GenericUlp, edits, 3, stride=128, n=n)
    assert recs.tobytes() == w_rec.tobytes()
    same(got, want, tune)
    model.fill(rewritten, None, None, w_rec, stride=128, n=n)
    same(got, rewritten, tune)
    assert (got[70::128 * 3] != arena[70::128 * 3]).any() or \
        (got[71::128 * 3] != arena[71::128 * 3]).any()  # TCP fields at byte 70 moved


# ---------------------------------------------------------------------------
# Hand-built frames
# ---------------------------------------------------------------------------
def kat_edits(k):
    return [(e[0], Field[e[1]], EditOp[e[2]], e[3]) for e in k["edits"]]


def test_hand_built_frames(ctx, torch):
    """Every vector of tests/golden/csum_update_kats.json, each with its own
    edits: ICMPv4 / ICMPv6, IPv4 options, a UDP field of 0, a result of 0
    written 0xffff, fragments, a sum that does not move, edits of checksum
    fields, a wrong input sum, the tunnel's three sums."""
    assert len(KATS["frames"]) >= 24
    for k in KATS["frames"]:
        f = bytes.fromhex(k["frame"])
        for mis in (0, 5):
            arena, off, lens = cf.place([f], misalign=mis)
            got, _ = on_gpu(torch, ctx, arena, off, lens, Chain[k["chain"]], kat_edits(k),
                            k["what"])
            assert got[mis:mis + len(f)].tobytes().hex() == k["after"], (k["name"], mis)
            rest = np.delete(got, np.arange(mis, mis + len(f)))
            assert (rest == 0xA5).all(), k["name"]  # nothing outside the frame was written


def test_hand_built_frames_one_batch(ctx, torch):
    """The GenericUlp vectors' frames as one batch under one NAT edit list."""
    frames = [bytes.fromhex(k["frame"]) for k in KATS["frames"] if k["chain"] == "GenericUlp"]
    arena, off, lens = cf.place(frames * 7, gap=1, misalign=3)  # 140+ frames: three tiles
    edits = edits_for(1) + [(2, Field.ICMP_CODE, ADD, 1), (2, Field.UDP_SOURCE, XOR, 0x8001)]
    want, _, w_rec = by_model(arena, off, lens, Chain.GenericUlp, edits, 3)
    got, recs = on_gpu(torch, ctx, arena, off, lens, Chain.GenericUlp, edits, 3)
    assert recs.tobytes() == w_rec.tobytes()
    same(got, want)


# ---------------------------------------------------------------------------
# Tunnel
# ---------------------------------------------------------------------------
def test_tunnel_inner_and_outer_sums(ctx, torch):
    """300 Geneve frames, inner sums filled under GENEVE_OVER_V6 and the outer
    UDP sum under a UDP_PARSER parse; edits on the inner L3 / L4 headers, the
    VNI and the outer UDP source; all three sums updated."""
    a, o, ln = gen_frames_host(GenProfile.GENEVE, 300, seed=31, slack=64)
    frames = [a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, ln)]
    arena, off, lens = cf.place(frames, gap=2, misalign=9)
    rows_i = model.fill(arena, off, lens, oracle.parse_batch(arena, off, lens, TUN))
    rows_o = model.fill(arena, off, lens, oracle.parse_batch(arena, off, lens, Chain.UdpParser),
                        what=CSUM_L4)
    keep = (rows_i["l4_state"] == OK) & ((rows_i["l3_state"] == OK) |
                                         (rows_i["l3_state"] == NONE)) & (rows_o["l4_state"] == OK)
    edits = [(5, Field.V4_DESTINATION, SET, 0x0A000005), (6, Field.UDP_DESTINATION, SUB, 1),
             (6, Field.TCP_DESTINATION, SET, 8443), (3, Field.GENEVE_VNI, SET, 0xABCDEF),
             (2, Field.UDP_SOURCE, XOR, 0x0FF0)]
    what = CSUM_L3 | CSUM_L4 | CSUM_OUTER_L4
    assert what == 7
    want, rewritten, w_rec = by_model(arena, off, lens, TUN, edits, what)
    got, recs = on_gpu(torch, ctx, arena, off, lens, TUN, edits, what)
    assert recs.tobytes() == w_rec.tobytes()
    same(got, want)
    model.fill(rewritten, off, lens, w_rec)  # the inner sums first, then the outer
    model.fill(rewritten, off, lens, oracle.parse_batch(rewritten, off, lens, Chain.UdpParser),
               what=CSUM_L4)
    same_frames(got, rewritten, off, lens, keep)  # 293 of 300
    assert (got != arena).any()


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------
def test_api_errors_on_a_live_context(ctx, torch):
    arena, off, lens, _ = valid_frames(GenProfile.MIXED, 31, Chain.GenericUlp, 1)
    d_arena = torch.from_numpy(arena.copy()).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_len = torch.from_numpy(lens.view(np.int16)).cuda()
    G = Chain.GenericUlp

    def call(chain, edits, what, n=None):
        ctx.parse_modify(d_arena, d_off, d_len, chain, edits, csum=what, n=n)

    for what in (8, 9, 0x80000001):  # (0 selects the plain rewrite in this wrapper)
        with pytest.raises(RuntimeError, match="parse_modify_csum"):
            call(G, edits_for(1), what)
    for what in (CSUM_OUTER_L4, 7):  # the outer sum: the tunnel chain only
        with pytest.raises(RuntimeError, match="parse_modify_csum"):
            call(G, edits_for(1), what)
    for f in (Field.V4_IHL, Field.V4_TOTAL_LEN, Field.V4_PROTOCOL, Field.V6_PAYLOAD_LEN,
              Field.V6_NEXT_HEADER):
        with pytest.raises(RuntimeError, match="parse_modify_csum"):
            call(G, [(1, f, SET, 5)], 3)
    lib, e = ctx._lib, ingot_amd.abi.edits_array(edits_for(1))
    import ctypes

    ep = e.ctypes.data_as(ctypes.c_void_p)
    assert lib.ingot_gpu_parse_modify_csum(ctx._h, None, None, None, 64, 0, int(G), ep, len(e), 0,
                                           None, None) == -1  # what == 0
    assert lib.ingot_gpu_parse_modify_csum(ctx._h, None, None, None, 64, 0, int(G), ep, len(e), 3,
                                           None, None) == 0  # n == 0 succeeds
    torch.cuda.synchronize()
    assert d_arena.cpu().numpy().tobytes() == arena.tobytes()  # no refused call wrote anything


# ---------------------------------------------------------------------------
# The C-ABI-only host
# ---------------------------------------------------------------------------
def test_cpp_nat_rewrite_example_on_device(torch):
    """tests/cpp/example_nat_rewrite.cpp, a fresh process: NAT + fused update
    on a slot ring, then ingot_gpu_checksum_verify finds no BAD sum."""
    exe = ROOT / "tests" / "cpp" / "build" / "example_nat_rewrite"
    if not exe.exists():
        from ingot_amd.build import build_cpp_tests

        build_cpp_tests()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 not OK before, 0 not OK after, 0 not rewritten" in r.stdout
