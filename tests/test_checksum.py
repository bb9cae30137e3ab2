"""ingot_gpu_checksum_verify / ingot_gpu_checksum_fill on the device against
the definition (tests/csum_model.py), bit for bit: the golden frames at every
misalignment, every segment length that takes another path through the chunk
run, generator traffic made valid and then broken on purpose, fill's write
set, and the two pipelines the calls exist for (decrement-and-forward,
encapsulation).  Needs an MI355X: `pytest -m gpu`."""
import json
from pathlib import Path

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import (CSUM_DTYPE, CSUM_L3, CSUM_L4, Chain, EditOp, EmitSource, Field, GenProfile,
                       emit as E)
from ingot_amd.hostgen import gen_frames_host
from tests import csum_frames as cf
from tests import csum_model as model

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "csum_kats.json").read_text())
NONE, OK, BAD, ZERO, SHORT, FRAGMENT = range(6)
TUN = Chain.GeneveOverV6Tunnel
BOTH = CSUM_L3 | CSUM_L4
GROUP = 256  # packets per workgroup of k_csum (ingot_amd/csrc/csum.hip)


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return ingot_amd.Context(0)


def _dev(torch, a):
    """A numpy array on the device (unsigned tables as the signed view of the same bits)."""
    a = np.ascontiguousarray(a)
    if a.dtype.fields:
        a = a.view(np.uint8)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
              np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()


def _rows(t):
    return t.cpu().numpy().view(CSUM_DTYPE).reshape(-1)


def _same_rows(got, want, what=""):
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def check_both_modes(ctx, torch, arena, off, lens, recs, what=BOTH, stride=0, n=None, tag=""):
    """verify == the model's rows; fill leaves the model's arena (every other
    byte untouched, the gaps included) and the model's rows; a verify of the
    filled arena finds no BAD and no ZERO.  Returns the model's verify rows."""
    d_off = None if off is None else _dev(torch, off)
    d_len = None if lens is None else _dev(torch, lens)
    d_rec = _dev(torch, recs).view(-1, 16)
    d_arena = _dev(torch, arena)
    want = model.verify(arena, off, lens, recs, what, stride, n)
    got = _rows(ctx.checksum_verify(d_arena, d_off, d_len, d_rec, what, stride=stride, n=n))
    _same_rows(got, want, tag + " verify")
    assert d_arena.cpu().numpy().tobytes() == arena.tobytes(), tag + ": verify wrote"
    filled = arena.copy()
    want_f = model.fill(filled, off, lens, recs, what, stride, n)
    out = torch.zeros((len(want), 8), dtype=torch.uint8, device="cuda")
    ctx.checksum_fill(d_arena, d_off, d_len, d_rec, what, stride=stride, n=n, out=out)
    _same_rows(_rows(out), want_f, tag + " fill")
    got_a = d_arena.cpu().numpy()
    bad = np.nonzero(got_a != filled)[0]
    assert bad.size == 0, (tag, "arena after fill", bad[:10], got_a[bad[:10]], filled[bad[:10]])
    after = _rows(ctx.checksum_verify(d_arena, d_off, d_len, d_rec, what, stride=stride, n=n))
    _same_rows(after, want_f, tag + " verify after fill")
    for k in ("l3_state", "l4_state"):
        assert not np.isin(after[k], (BAD, ZERO)).any(), tag
        quiet = np.isin(want[k], (NONE, SHORT, FRAGMENT))
        assert (after[k][quiet] == want[k][quiet]).all(), tag
    return want


# ---------------------------------------------------------------------------
# golden frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [Chain.GenericUlp, Chain.VlanUlp])
def test_golden_frames_at_every_misalignment(ctx, torch, chain):
    """Packed at every source misalignment 0-15 with 0xa5 between the frames:
    a read past a segment's end, or before its start, changes the sum."""
    kats = [k for k in KATS["frames"] if k["chain"] == chain.name]
    frames = [bytes.fromhex(k["frame"]) for k in kats]
    for mis in range(16):
        arena, off, lens = cf.place(frames, misalign=mis, gap=(mis * 7) % 5, fill=0xA5)
        recs = oracle.parse_batch(arena, off, lens, chain)
        want = check_both_modes(ctx, torch, arena, off, lens, recs, tag=f"{chain.name}@{mis}")
        for k, row in zip(kats, want):
            assert list(row.tolist()) == k["row"], (k["name"], mis)


# ---------------------------------------------------------------------------
# segment lengths
# ---------------------------------------------------------------------------
PAYLOADS = [0, 1, 2, 15, 16, 17, 31, 33, 1023, 1024, 1025, 1472, 8972, 65535 - 42]
KINDS = [("v4", cf.UDP), ("v6", cf.TCP), ("v4", cf.ICMP4), ("v6", cf.UDP), ("v4", cf.TCP),
         ("v6", cf.ICMP6)]


def _length_frames(n, start, ones, rng):
    out = []
    for i in range(n):
        p = PAYLOADS[(start + i) % len(PAYLOADS)]
        l3, proto = KINDS[i % len(KINDS)] if p < 60000 else ("v4", cf.UDP)  # 65,535-B frame
        pay = b"\xff" * p if ones else rng.integers(0, 256, p, dtype=np.uint8).tobytes()
        out.append(cf.frame(l3, proto, pay))
    return out


@pytest.mark.parametrize("ones", [True, False], ids=["ff", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, GROUP + 1])
def test_segment_lengths(ctx, torch, n, ones):
    """Every payload length of PAYLOADS (the last makes a 65,535-B frame, the
    most a u16 length allows), as all-0xff bytes (the largest sums) and as
    random ones, in batches that end inside a wave, at its edge, just past it
    and one packet past a workgroup's group.  An Ethernet frame's l4_off is
    always even, so the parity that decides the byte order of the sum — that
    of the segment's first byte's address — is set by where the frame lies:
    every batch runs with all frames at even and at odd addresses.  The
    checksums are valid (the model's fill) but for every fifth frame, one
    of whose segment bytes is flipped."""
    rng = np.random.default_rng(1000 + n)
    for start in (range(len(PAYLOADS)) if n == 1 else (0,)):
        frames = _length_frames(n, start, ones, rng)
        for parity in (0, 1):
            offsets, o = [], 16
            for f in frames:
                o += (o ^ parity) & 1
                offsets.append(o)
                o += len(f) + 3
            arena, off, lens = cf.place(frames, offsets=offsets, fill=0xA5)
            recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
            assert (recs["status"] == 0).all() and ((off + recs["l4_off"]) & 1 == parity).all()
            model.fill(arena, off, lens, recs)
            for i in range(0, n, 5):  # the source port (ICMP: the type): in no field
                arena[int(off[i]) + int(recs["l4_off"][i])] ^= 0x10
            want = check_both_modes(ctx, torch, arena, off, lens, recs,
                                    tag=f"n={n} start={start} parity={parity}")
            assert (want["l4_state"][0::5] == BAD).all()
            rest = np.ones(n, bool)
            rest[0::5] = False
            assert (want["l4_state"][rest] == OK).all()


# ---------------------------------------------------------------------------
# generator traffic
# ---------------------------------------------------------------------------
def prepare(profile, n, chain, seed, stride=None):
    """Generator frames -> (arena, off, lens, recs, stride) on the host with
    every state present.  The generator's checksums are random and its
    lengths exact, so: some lengths are lowered by 1-7 (padding), the model
    fills every checksum, and then chosen subsets are broken — a flipped last
    segment byte (BAD), the UDP field zeroed (ZERO), total_len / payload_len
    raised past the frame or lowered into the L4 header (SHORT)."""
    arena, off, lens = gen_frames_host(profile, n, seed=seed, stride=stride, slack=64)
    arena = arena.copy()
    st = stride or 0
    recs = oracle.parse_batch(arena, off, lens, chain, stride=st, n=n)
    rng = np.random.default_rng(seed)
    base = off.astype(np.int64) if off is not None else np.arange(n, dtype=np.int64) * st

    def len_at(i):  # where the L3 length field lies, and what it counts from
        o3 = int(recs["l3_off"][i])
        return (base[i] + o3 + 2, 0) if recs["l3_kind"][i] == 1 else (base[i] + o3 + 4, 40)

    def get_len(i):
        at, _ = len_at(i)
        return (int(arena[at]) << 8) | int(arena[at + 1])

    def set_len(i, v):
        at, _ = len_at(i)
        arena[at], arena[at + 1] = v >> 8, v & 0xFF

    # the rows that are summed at all (the generator's own checksums are random)
    summed = np.nonzero(np.isin(model.verify(arena, off, lens, recs, CSUM_L4, st, n)["l4_state"],
                                (OK, BAD, ZERO)))[0]
    pick = rng.permutation(summed)
    k = max(60, len(pick) // 12)
    pad, flip, zero, past, into = (pick[j * k:(j + 1) * k] for j in range(5))
    for i in pad:  # padding: the L3 length ends 1-7 bytes before the frame does
        room = get_len(i) + len_at(i)[1] + int(recs["l3_off"][i]) - int(recs["payload_off"][i])
        set_len(i, get_len(i) - min(int(rng.integers(1, 8)), room))
    model.fill(arena, off, lens, recs, BOTH, st, n)
    for i in flip:
        at, plus = len_at(i)
        arena[base[i] + int(recs["l3_off"][i]) + plus + get_len(i) - 1] ^= 1 << int(rng.integers(8))
    udp = [i for i in pick[5 * k:] if recs["l4_kind"][i] == 2][:k] + \
        [i for i in zero if recs["l4_kind"][i] == 2]
    for i in udp:
        arena[base[i] + int(recs["l4_off"][i]) + 6:base[i] + int(recs["l4_off"][i]) + 8] = 0
    L = lens.astype(np.int64) if lens is not None else np.full(n, st, np.int64)
    for i in past:
        set_len(i, int(L[i]) - int(recs["l3_off"][i]) - len_at(i)[1] + int(rng.integers(1, 300)))
    for i in into:
        set_len(i, max(0, int(recs["l4_off"][i]) + 4 - int(recs["l3_off"][i]) - len_at(i)[1]))
    return arena, off, lens, recs, st


GEN_CASES = [
    ("MIXED", Chain.GenericUlp, 20_000, None),
    ("VLAN_V6EH", Chain.VlanUlp, 20_000, None),
    ("FLOWS", Chain.GenericUlp, 20_000, None),
    ("ADVERSARIAL", Chain.GenericUlp, 20_000, None),
    ("GENEVE", TUN, 8_000, None),
    ("V4UDP64", Chain.UdpParser, 20_000, 64),  # 64-B slots, d_len NULL
]
# states every case's input must hold >= 50 rows of before the comparison counts
# (every MIXED and VLAN_V6EH frame parses down to an L4 header, so neither has
# a NONE row; the 64-B UDP slots have neither NONE nor fragments)
EVERY = {NONE, OK, BAD, ZERO, SHORT, FRAGMENT}
EXPECT = {"MIXED": EVERY - {NONE}, "VLAN_V6EH": EVERY - {NONE},
          "V4UDP64": EVERY - {FRAGMENT, NONE}}


@pytest.mark.parametrize("profile,chain,n,stride", GEN_CASES, ids=[c[0] for c in GEN_CASES])
def test_generator_frames(ctx, torch, profile, chain, n, stride):
    arena, off, lens, recs, st = prepare(GenProfile[profile], n, chain, seed=4242, stride=stride)
    want = model.verify(arena, off, lens, recs, BOTH, st, n)
    counts = np.bincount(want["l4_state"], minlength=6)
    for s in EXPECT.get(profile, EVERY):
        assert counts[s] >= 50, (profile, s, counts)
    c3 = np.bincount(want["l3_state"], minlength=3)
    assert c3[OK] >= 50, c3
    if profile != "ADVERSARIAL":  # its summed rows, the ones whose lengths are broken, are IPv6
        assert c3[BAD] >= 50, c3
    got = check_both_modes(ctx, torch, arena, off, lens, recs, stride=st, n=n, tag=profile)
    _same_rows(got, want)
    # the device's own parse gives the same rows as the oracle's records
    d_arena = _dev(torch, arena)
    d_off = None if off is None else _dev(torch, off)
    d_len = None if lens is None else _dev(torch, lens)
    d_rec = ctx.parse(d_arena, d_off, d_len, chain) if off is not None else \
        ctx.parse_strided(d_arena, st, n, chain, lens=d_len)
    for what in (CSUM_L3, CSUM_L4):
        w = model.verify(arena, off, lens, recs, what, st, n)
        _same_rows(_rows(ctx.checksum_verify(d_arena, d_off, d_len, d_rec, what, stride=st, n=n)),
                   w, f"{profile} what={what}")


def test_fill_without_rows_and_side_stream(ctx, torch):
    """d_out NULL is accepted by fill, and a launch on a side stream gives the
    default stream's result."""
    arena, off, lens, recs, _ = prepare(GenProfile.MIXED, 5_000, Chain.GenericUlp, seed=77)
    d_off, d_len, d_rec = _dev(torch, off), _dev(torch, lens), _dev(torch, recs).view(-1, 16)
    a0, a1, a2 = (_dev(torch, arena) for _ in range(3))
    rows0 = ctx.checksum_verify(a0, d_off, d_len, d_rec)
    out0 = torch.zeros((len(recs), 8), dtype=torch.uint8, device="cuda")
    ctx.checksum_fill(a0, d_off, d_len, d_rec, out=out0)
    assert ctx.checksum_fill(a1, d_off, d_len, d_rec) is None
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rows2 = ctx.checksum_verify(a2, d_off, d_len, d_rec, stream=side)
        out2 = torch.zeros((len(recs), 8), dtype=torch.uint8, device="cuda")
        ctx.checksum_fill(a2, d_off, d_len, d_rec, out=out2, stream=side)
    side.synchronize()
    torch.cuda.synchronize()
    want = arena.copy()
    model.fill(want, off, lens, recs)
    assert a0.cpu().numpy().tobytes() == want.tobytes()
    assert a1.cpu().numpy().tobytes() == want.tobytes()
    assert a2.cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(rows0, rows2) and torch.equal(out0, out2)


def test_argument_errors(ctx, torch):
    lib = ingot_amd._lib.load()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    r = torch.zeros((10, 16), dtype=torch.uint8, device="cuda")
    o = torch.zeros((10, 8), dtype=torch.uint8, device="cuda")
    off = torch.zeros(10, dtype=torch.int64, device="cuda")
    ln = torch.zeros(10, dtype=torch.int16, device="cuda")
    h, A, R, O, F, L = ctx._h, a.data_ptr(), r.data_ptr(), o.data_ptr(), off.data_ptr(), \
        ln.data_ptr()
    for fn in (lib.ingot_gpu_checksum_verify, lib.ingot_gpu_checksum_fill):
        for what in (0, 4, 8 | 1):
            assert fn(h, A, F, L, 0, 10, R, what, O, None) == -1
        assert fn(h, None, F, L, 0, 10, R, 3, O, None) == -1
        assert fn(h, A, F, L, 0, 10, None, 3, O, None) == -1
        assert fn(h, A, F, None, 0, 10, R, 3, O, None) == -1      # offsets without lengths
        for stride in (0, 24, 65536):
            assert fn(h, A, None, None, stride, 10, R, 3, O, None) == -5, stride
        assert fn(h, A + 4, None, None, 64, 10, R, 3, O, None) == -1  # slots: 16-B aligned
        assert fn(h, None, None, None, 0, 0, None, 3, None, None) == 0  # empty batch
    assert lib.ingot_gpu_checksum_verify(h, A, F, L, 0, 10, R, 3, None, None) == -1
    with pytest.raises(ValueError):
        ctx.checksum_verify(a, off, ln, r, what=0)
    with pytest.raises(ValueError):
        ctx.checksum_fill(a, off, ln, r[:5])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# the two pipelines
# ---------------------------------------------------------------------------
def test_decrement_and_forward(ctx, torch):
    """parse_modify decrementing hop_limit (the reference's parse_and_decr_v4
    edit) on valid frames leaves a stale IPv4 header checksum;
    checksum_fill(L3) with the rewrite's own records makes it valid again."""
    n = 20_000
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=31, slack=64)
    arena = arena.copy()
    recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    model.fill(arena, off, lens, recs)
    edits = [(1, Field.V4_HOP_LIMIT, EditOp.SUB, 1), (1, Field.V6_HOP_LIMIT, EditOp.SUB, 1)]
    d_arena, d_off, d_len = _dev(torch, arena), _dev(torch, off), _dev(torch, lens)
    d_rec = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    ctx.parse_modify(d_arena, d_off, d_len, Chain.GenericUlp, edits, out=d_rec)
    want = arena.copy()
    w_rec = oracle.parse_modify_batch(want, off, lens, Chain.GenericUlp, edits)
    assert d_rec.cpu().numpy().tobytes() == w_rec.tobytes()
    stale = _rows(ctx.checksum_verify(d_arena, d_off, d_len, d_rec, CSUM_L3))
    _same_rows(stale, model.verify(want, off, lens, w_rec, CSUM_L3))
    v4 = (w_rec["status"] == 0) & (w_rec["l3_kind"] == 1)
    assert v4.sum() > 1000 and (stale["l3_state"][v4] == BAD).all()
    rows = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
    ctx.checksum_fill(d_arena, d_off, d_len, d_rec, CSUM_L3, out=rows)
    _same_rows(_rows(rows), model.fill(want, off, lens, w_rec, CSUM_L3))
    assert d_arena.cpu().numpy().tobytes() == want.tobytes()
    after = _rows(ctx.checksum_verify(d_arena, d_off, d_len, d_rec))
    _same_rows(after, model.verify(want, off, lens, w_rec))
    assert (after["l3_state"][v4] == OK).all()
    assert not (after["l4_state"] == BAD).any()  # hop_limit is in no pseudo-header


def test_encapsulation(ctx, torch):
    """emit_packets with the OPTE Geneve stack over valid inner frames, a
    UDP_PARSER parse of the result, checksum_fill(L4): the outer UDP checksum
    is the model's over the whole encapsulated packet, and a GENEVE_OVER_V6
    parse + verify still finds the inner sums valid."""
    n = 8_000
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=32, slack=64)
    arena = arena.copy()
    model.fill(arena, off, lens, oracle.parse_batch(arena, off, lens, Chain.GenericUlp))
    hdr = (E.ethernet(bytes.fromhex("a84025777776"), bytes.fromhex("a84025777777"), 0x86DD)
           + E.ipv6(bytes.fromhex("fd000000f70101000000000000000002"),
                    bytes.fromhex("fd000000f70101000000000000000001"), 17, hop_limit=0xF0)
           + E.udp(0xC0DE, 6081, checksum=0) + E.geneve(0x123456, options=E.geneve_opt(0x0129, 0)))
    H = len(hdr)
    sets = [(14, Field.V6_PAYLOAD_LEN, EmitSource.LENGTH, -40),
            (54, Field.UDP_LENGTH, EmitSource.LENGTH, 0)]
    ln = lens.astype(np.int64)
    dst_off = (np.cumsum(np.r_[0, ln[:-1] + H + 3]) + 1).astype(np.uint64)  # every alignment
    tl = (ln + H).astype(np.uint16)
    size = int(dst_off[-1]) + int(tl[-1]) + 64
    d_dst = _dev(torch, np.full(size, 0xA5, np.uint8))
    d_doff, d_tl = _dev(torch, dst_off), _dev(torch, tl)
    ctx.emit_packets(hdr, sets, _dev(torch, arena), _dev(torch, off), _dev(torch, lens), d_dst,
                     d_doff)
    want = d_dst.cpu().numpy().copy()
    outer = ctx.parse(d_dst, d_doff, d_tl, Chain.UdpParser)
    w_outer = oracle.parse_batch(want, dst_off, tl, Chain.UdpParser)
    assert outer.cpu().numpy().tobytes() == w_outer.tobytes() and (w_outer["status"] == 0).all()
    before = _rows(ctx.checksum_verify(d_dst, d_doff, d_tl, outer, CSUM_L4))
    assert (before["l4_state"] == ZERO).all()  # the header block's constant
    rows = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
    ctx.checksum_fill(d_dst, d_doff, d_tl, outer, CSUM_L4, out=rows)
    w_rows = model.fill(want, dst_off, tl, w_outer, CSUM_L4)
    _same_rows(_rows(rows), w_rows)
    assert (w_rows["l4_state"] == OK).all() and (w_rows["l4_len"] == tl - 54).all()
    assert d_dst.cpu().numpy().tobytes() == want.tobytes()
    tun = ctx.parse(d_dst, d_doff, d_tl, TUN)
    w_tun = oracle.parse_batch(want, dst_off, tl, TUN)
    inner = _rows(ctx.checksum_verify(d_dst, d_doff, d_tl, tun))
    _same_rows(inner, model.verify(want, dst_off, tl, w_tun))
    plain = model.verify(arena, off, lens, oracle.parse_batch(arena, off, lens,
                                                              Chain.GenericUlp))
    assert (inner["l4_state"] == plain["l4_state"]).all() and not (inner["l4_state"] == BAD).any()
    assert (inner["l3_state"] == plain["l3_state"]).all() and not (inner["l3_state"] == BAD).any()
    assert (inner["l4_state"] == OK).sum() > 1000
