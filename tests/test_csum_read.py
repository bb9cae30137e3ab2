"""ingot_gpu_checksum_verify_read / ingot_gpu_checksum_fill_read on the device
against the definition (tests/csum_read_model.py), bit for bit: the golden
frames cut and placed at every misalignment, every lane parity a payload cut
can give, the shapes a chunk list can take, more pieces than the kernel's
table holds, the largest sums, generator traffic, and the two-chunk
encapsulation the calls exist for.  Needs an MI355X: `pytest -m gpu`."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import (CSUM_DTYPE, CSUM_L3, CSUM_L4, Chain, EmitSource, EmitSum, Field, GenProfile,
                       emit as E)
from ingot_amd.hostgen import gen_frames_host
from tests import csum_frames as cf
from tests import csum_model
from tests import csum_read_cases as cases
from tests import csum_read_model as model

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "csum_kats.json").read_text())
NONE, OK, BAD, ZERO, SHORT, FRAGMENT = range(6)
TUN = Chain.GeneveOverV6Tunnel
BOTH = CSUM_L3 | CSUM_L4
GROUP = 256    # packets per workgroup of k_csum_read (ingot_amd/csrc/csum.hip)
PIECES = 1024  # capacity of its piece table


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


def check_both_modes(ctx, torch, tables, recs, what=BOTH, tag=""):
    """verify == the model's rows and wrote nothing; fill leaves the model's
    arena (every other byte untouched, the gaps included) and the model's
    rows; a verify of the filled arena finds no BAD and no ZERO.  Returns the
    model's verify rows."""
    arena, seg_off, seg_len, pkt_seg = tables
    d_tab = (_dev(torch, seg_off), _dev(torch, seg_len), _dev(torch, pkt_seg))
    d_rec = _dev(torch, recs).view(-1, 16)
    d_arena = _dev(torch, arena)
    want = model.verify(tables, recs, what)
    got = _rows(ctx.checksum_verify_read(d_arena, *d_tab, d_rec, what))
    _same_rows(got, want, tag + " verify")
    assert d_arena.cpu().numpy().tobytes() == arena.tobytes(), tag + ": verify wrote"
    filled = arena.copy()
    want_f = model.fill((filled, seg_off, seg_len, pkt_seg), recs, what)
    out = torch.zeros((len(want), 8), dtype=torch.uint8, device="cuda")
    ctx.checksum_fill_read(d_arena, *d_tab, d_rec, what, out=out)
    _same_rows(_rows(out), want_f, tag + " fill")
    got_a = d_arena.cpu().numpy()
    bad = np.nonzero(got_a != filled)[0]
    assert bad.size == 0, (tag, "arena after fill", bad[:10], got_a[bad[:10]], filled[bad[:10]])
    after = _rows(ctx.checksum_verify_read(d_arena, *d_tab, d_rec, what))
    _same_rows(after, want_f, tag + " verify after fill")
    for k in ("l3_state", "l4_state"):
        assert not np.isin(after[k], (BAD, ZERO)).any(), tag
        quiet = np.isin(want[k], (NONE, SHORT, FRAGMENT))
        assert (after[k][quiet] == want[k][quiet]).all(), tag
    return want


def contiguous_recs(frames, chain=Chain.GenericUlp):
    return oracle.parse_batch(*cf.place(frames)[:3], chain)


def valid(frames, chain=Chain.GenericUlp):
    """The frames with every checksum filled by the contiguous model, and their records."""
    arena, off, lens = cf.place(frames)
    recs = oracle.parse_batch(arena, off, lens, chain)
    csum_model.fill(arena, off, lens, recs)
    return cases.frames_of(arena, off, lens), recs


def read_recs(tables, chain=Chain.GenericUlp):
    return oracle.parse_read_batch(*tables, chain)[0]


# ---------------------------------------------------------------------------
# golden frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [Chain.GenericUlp, Chain.VlanUlp])
def test_golden_frames_cut_at_every_misalignment(ctx, torch, chain):
    """The frames of csum_kats.json cut by `cut` with five seeds, every chunk
    placed at each misalignment 0-15 with 0xa5 between the chunks: the rows
    equal the stored rows wherever the chunked record is Ok."""
    kats = [k for k in KATS["frames"] if k["chain"] == chain.name]
    frames = [bytes.fromhex(k["frame"]) for k in kats]
    crecs = contiguous_recs(frames, chain)
    packets, rows = [], []
    for seed in range(5):
        rng = np.random.default_rng(seed)
        for k, f, r in zip(kats, frames, crecs):
            packets.append(cases.cut(f, r, rng))
            rows.append(k["row"])
    assert sum(len(p) > 1 for p in packets) > len(packets) // 2
    compared = 0
    for mis in range(16):
        tables = cases.place(packets, misalign=mis, gap=(mis * 7) % 5)
        recs = read_recs(tables, chain)
        want = check_both_modes(ctx, torch, tables, recs, tag=f"{chain.name}@{mis}")
        for j, (row, stored) in enumerate(zip(want, rows)):
            if recs["status"][j] == 0:
                assert list(row.tolist()) == stored, (j, mis)
                compared += 1
    assert compared > 16 * len(packets) // 2


# ---------------------------------------------------------------------------
# lane parity
# ---------------------------------------------------------------------------
def test_lane_parity_of_every_payload_cut(ctx, torch):
    """One UDP/IPv4 and one TCP/IPv6 frame with a 64-B payload of distinct
    bytes, cut into two payload pieces at every offset 0..64, times the second
    piece's address parity, times the first chunk's misalignment 0..15: a
    piece summed in the wrong byte lane changes the sum."""
    payload = bytes(range(101, 165))
    frames, recs = valid([cf.frame("v4", cf.UDP, payload), cf.frame("v6", cf.TCP, payload)])
    packets, mis, rr = [], [], []
    for f, r in zip(frames, recs):
        pay = int(r["payload_off"])
        for c in range(65):
            for parity in (0, 1):
                for m in range(16):
                    packets.append([f[:pay + c], f[pay + c:]])
                    mis += [m, (parity + 2 * (c % 8)) % 16]
                    rr.append(r)
    tables = cases.place(packets, misalign=mis, gap=1)
    assert ((tables[1][1:-1:2] & 1) == np.tile(np.repeat([0, 1], 16), 130)).all()
    recs = read_recs(tables)
    assert recs.tobytes() == np.array(rr).tobytes()
    want = check_both_modes(ctx, torch, tables, recs, tag="parity")
    assert (want["l4_state"] == OK).all()
    for i in range(0, len(packets), 3):  # a flipped payload byte of the second piece's chunk
        k = int(tables[3][i]) + 1
        if tables[2][k]:
            tables[0][int(tables[1][k])] ^= 0x40
    want = check_both_modes(ctx, torch, tables, recs, tag="parity, broken")
    assert (want["l4_state"] == BAD).sum() > len(packets) // 4


# ---------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------
def test_chunk_list_shapes(ctx, torch):
    frames, recs = valid([cf.frame("v4", cf.UDP, bytes(range(1, 38))),
                          cf.frame("v6", cf.TCP, bytes(range(7, 90))),
                          cf.frame("v4", cf.ICMP4, bytes(range(3, 24))),
                          cf.frame("v6", cf.ICMP6, bytes(range(9, 70))),
                          cf.frame("v4", cf.TCP, b"\xfe" * 301, options=bytes([1] * 4))])
    big, brec = valid([cf.frame("v4", cf.UDP, bytes(range(256)) * 255 + bytes(213))])
    assert len(big[0]) == 65535
    packets, want_state, names = [], [], []

    def add(name, chunks, state=OK):
        names.append(name)
        packets.append(chunks)
        want_state.append(state)

    for f, r in zip(frames, recs):
        l4, pay, n = int(r["l4_off"]), int(r["payload_off"]), len(f)
        add("1-byte payload chunks", [f[:pay]] + [f[k:k + 1] for k in range(pay, n)])
        add("1-byte chunks from l4_off's header on", [f[:l4], f[l4:pay]] +
            [f[k:k + 1] for k in range(pay, n)])
        add("empty chunks between pieces", [f[:pay], b"", f[pay:pay + 5], b"", b"", f[pay + 5:], b""])
        add("cut at l4_off", [f[:l4], f[l4:]])
        add("cut at payload_off", [f[:pay], f[pay:]])
        add("cut at l4_off, payload_off and end", [f[:l4], f[l4:pay], f[pay:], b"\x11" * 9])
        add("end inside a chunk that continues", [f[:pay + 3], f[pay + 3:] + b"\x77" * 7])
        add("padding right after the headers' chunk", [f[:l4], f[l4:] + b"\x77"])
        add("a whole trailing chunk past end", [f[:pay], f[pay:], b"\x99" * 33])
        add("end > L", [f[:pay], f[pay:n - 1]], SHORT)
        add("end > L, headers only", [f[:pay]], SHORT)
    f = big[0]
    add("65,535 B and more: later bytes are not seen", [f[:42], f[42:40001], f[40001:], b"\x55" * 300])
    add("the cut falls inside a chunk", [f[:42], f[42:40001], f[40001:] + b"\x55" * 300])
    add("65,535 B, a chunk short", [f[:42], f[42:40001], f[40001:65534]], SHORT)
    tables = cases.place(packets, misalign=[3, 8, 13, 0, 15, 6, 1], gap=2)
    recs = read_recs(tables)
    assert (recs["status"] == 0).all()
    want = check_both_modes(ctx, torch, tables, recs, tag="shapes")
    for name, row, st in zip(names, want, want_state):
        assert row["l4_state"] == st, (name, row)
    v4 = recs["l3_kind"] == 1
    assert (want["l3_state"][v4] == OK).all() and (want["l3_state"][~v4] == NONE).all()
    for what in (CSUM_L3, CSUM_L4):
        check_both_modes(ctx, torch, tables, recs, what, tag=f"shapes what={what}")


def test_rule_rows_on_the_device(ctx, torch):
    """Contiguous records supplied for chunks that cut a header: NONE where
    the rule says so, and those chunks are left unread and unwritten."""
    frames, recs = valid([cf.frame("v4", cf.TCP, bytes(range(40)), options=bytes([1] * 8)),
                          cf.frame("v6", cf.UDP, bytes(range(33)), ext=((60, bytes(6)),))])
    f, g = frames
    packets = [cases.cut_at(f, c) for c in ([14, 42, 62, 70], [50], [40], [36], [20], [15, 16])]
    packets += [cases.cut_at(g, c) for c in ([54], [14, 62, 70, 71], [66], [60])]
    rr = np.array([recs[0]] * 6 + [recs[1]] * 4)
    tables = cases.place(packets, misalign=[1, 6, 11], gap=4)
    want = check_both_modes(ctx, torch, tables, rr, tag="rule")
    got = [(int(r["l3_state"]), int(r["l4_state"])) for r in want]
    assert got == [(OK, OK), (OK, NONE), (NONE, NONE), (NONE, NONE), (NONE, NONE), (NONE, NONE),
                   (NONE, NONE), (NONE, OK), (NONE, NONE), (NONE, NONE)]
    # stale records: Ok records of other packets, and packets without chunks
    stale = np.roll(rr, 3)
    check_both_modes(ctx, torch, tables, stale, tag="stale")
    none = cases.place([[] for _ in packets])
    w = check_both_modes(ctx, torch, none, rr, tag="no chunks")
    assert (w["l3_state"] == NONE).all() and (w["l4_state"] == NONE).all()
    # pkt_seg[i+1] < pkt_seg[i] counts as no chunks
    arena, so, sl, ps = cases.place(packets[:3], misalign=5)
    ps = np.array([ps[0], ps[2], ps[1], ps[3]], dtype=np.uint32)
    w = check_both_modes(ctx, torch, (arena, so, sl, ps), rr[:3], tag="descending bounds")
    assert (int(w["l3_state"][1]), int(w["l4_state"][1])) == (NONE, NONE)


# ---------------------------------------------------------------------------
# more pieces than the table
# ---------------------------------------------------------------------------
def test_more_pieces_than_the_table(ctx, torch):
    """One packet whose 4,000-B payload lies in 1-B chunks between ordinary
    packets, and a full group of 256 packets of 8 pieces each: the piece table
    is filled in rounds and the accumulators persist."""
    rng = np.random.default_rng(5)
    long_ = cf.frame("v6", cf.UDP, rng.integers(0, 256, 4000, dtype=np.uint8).tobytes())
    few = [cf.frame("v4", cf.TCP, rng.integers(0, 256, 100 + 7 * k, dtype=np.uint8).tobytes())
           for k in range(20)]
    frames, recs = valid(few[:10] + [long_] + few[10:])
    packets = []
    for f, r in zip(frames, recs):
        pay = int(r["payload_off"])
        if len(f) > 4000:
            packets.append([f[:pay]] + [f[k:k + 1] for k in range(pay, len(f))])
        else:
            packets.append(cases.cut_at(f, [pay, pay + 31]))
    assert len(packets[10]) - 1 == 4000 > PIECES
    tables = cases.place(packets, misalign=[0, 1, 2, 3, 5, 8, 13], gap=1)
    rr = read_recs(tables)
    assert rr.tobytes() == recs.tobytes()
    want = check_both_modes(ctx, torch, tables, rr, tag="4000 pieces")
    assert (want["l4_state"] == OK).all() and want["l4_len"][10] == 4008

    frames, recs = valid([cf.frame("v4" if k % 2 else "v6", cf.UDP if k % 3 else cf.TCP,
                                   rng.integers(0, 256, 64 + k, dtype=np.uint8).tobytes())
                          for k in range(GROUP)])
    packets = []
    for k, (f, r) in enumerate(zip(frames, recs)):
        pay = int(r["payload_off"])
        cuts = [pay + 1 + (k % 5) + 7 * j for j in range(7)]  # 8 payload pieces
        packets.append(cases.cut_at(f, cuts))
        assert all(len(c) > 0 for c in packets[-1])
    assert GROUP * 8 > PIECES
    tables = cases.place(packets, misalign=list(range(16)) + [7], gap=0)
    rr = read_recs(tables)
    assert rr.tobytes() == recs.tobytes()
    tables[0][int(tables[1][int(tables[3][77]) + 6])] ^= 0x08  # a late piece of packet 77
    want = check_both_modes(ctx, torch, tables, rr, tag="256 x 8 pieces")
    assert (np.delete(want["l4_state"], 77) == OK).all() and want["l4_state"][77] == BAD


# ---------------------------------------------------------------------------
# largest sums
# ---------------------------------------------------------------------------
def test_largest_sums_and_a_zero_udp_sum(ctx, torch):
    """65,535 bytes of 0xff payload as two chunks with an odd cut and as 16
    chunks: neither class accumulator may overflow.  And a UDP sum that comes
    out 0 is given, and written, as 0xffff."""
    frames, recs = valid([cf.frame("v4", cf.UDP, b"\xff" * (65535 - 42))])
    f = frames[0]
    assert len(f) == 65535
    zero = cf.frame("v4", cf.UDP, bytes(2))
    zrec = contiguous_recs([zero])[0]
    s = csum_model.one(np.frombuffer(zero, dtype=np.uint8), zrec, CSUM_L4, False)[3]
    zero = zero[:-2] + bytes([s >> 8, s & 0xFF])  # the payload word that makes the sum 0xffff
    cuts16 = [42] + [42 + 4099 * k + (k & 1) for k in range(1, 15)]
    packets = [cases.cut_at(f, [32769]), cases.cut_at(f, [43]), cases.cut_at(f, cuts16),
               cases.cut_at(zero, [42, 43]), cases.cut_at(zero, [34])]
    assert len(packets[2]) == 16
    tables = cases.place(packets, misalign=[1, 0, 9, 15], gap=3)
    rr = read_recs(tables)
    assert (rr["status"] == 0).all()
    want = check_both_modes(ctx, torch, tables, rr, tag="largest")
    assert (want["l4_state"][:3] == OK).all() and (want["l4_len"][:3] == 65535 - 34).all()
    assert (want["l4_sum"][3:] == 0xFFFF).all() and (want["l4_state"][3:] == ZERO).all()


# ---------------------------------------------------------------------------
# batch edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_edges(ctx, torch, n):
    """Batches that end inside a wave, at its edge, just past it and one
    packet past a workgroup's group, with zero-chunk packets mixed in."""
    rng = np.random.default_rng(n)
    kinds = [("v4", cf.UDP), ("v6", cf.TCP), ("v4", cf.ICMP4), ("v6", cf.UDP), ("v4", cf.TCP),
             ("v6", cf.ICMP6)]
    frames = [cf.frame(*kinds[i % 6], rng.integers(0, 256, int(rng.integers(0, 200)),
                                                   dtype=np.uint8).tobytes()) for i in range(n)]
    frames, recs = valid(frames)
    packets = [cases.cut(f, r, rng) for f, r in zip(frames, recs)]
    for i in range(2, n, 7):
        packets[i] = []
    tables = cases.place(packets, misalign=list(range(16)) + [3, 9, 14], gap=2)
    rr = read_recs(tables)
    want = check_both_modes(ctx, torch, tables, rr, tag=f"n={n}")
    empty = np.zeros(n, bool)
    empty[2::7] = True
    assert (want["l4_state"][empty] == NONE).all() and (want["l4_state"][~empty] == OK).all()
    assert (rr["status"][~empty] == 0).all()


# ---------------------------------------------------------------------------
# generator traffic
# ---------------------------------------------------------------------------
GEN_CASES = [("MIXED", Chain.GenericUlp), ("VLAN_V6EH", Chain.VlanUlp), ("GENEVE", TUN),
             ("MIXED", Chain.UdpParser)]


@pytest.mark.parametrize("profile,chain", GEN_CASES, ids=[f"{p}-{c.name}" for p, c in GEN_CASES])
def test_generator_frames(ctx, torch, profile, chain):
    """20,000 generator frames with every state present (tests/test_checksum.py's
    prepare), cut by `cut`: both modes, with the device's own parse_read
    records."""
    from tests.test_checksum import prepare

    n = 20_000
    arena, off, lens, crecs, _ = prepare(GenProfile[profile], n, chain, seed=4343)
    rng = np.random.default_rng(17)
    frames = cases.frames_of(arena, off, lens)
    packets = [cases.cut(f, crecs[i], rng) for i, f in enumerate(frames)]
    tables = cases.place(packets, misalign=list(range(16)) + [5, 11, 2], gap=1)
    recs = read_recs(tables, chain)
    d = [_dev(torch, x) for x in tables]
    d_rec, _ = ctx.parse_read(*d, chain)
    assert d_rec.cpu().numpy().tobytes() == recs.tobytes()
    want = check_both_modes(ctx, torch, tables, recs, tag=profile)
    contiguous = csum_model.verify(arena, off, lens, recs)
    _same_rows(want, contiguous, "against the contiguous model")
    counts = np.bincount(want["l4_state"], minlength=6)
    for s in (OK, BAD, ZERO, SHORT):
        assert counts[s] >= 50, (profile, s, counts)
    got = _rows(ctx.checksum_verify_read(d[0], d[1], d[2], d[3], d_rec, CSUM_L4))
    _same_rows(got, model.verify(tables, recs, CSUM_L4), "what=L4")


def test_adversarial_frames_split_anywhere(ctx, torch):
    """ADVERSARIAL frames cut by tests/test_parse_read.py's split (edges
    anywhere, also inside headers): many StraddledHeader records, so NONE
    rows, and every Ok record still satisfies the rule."""
    from tests.test_checksum import prepare
    from tests.test_parse_read import split

    n = 20_000
    arena, off, lens, crecs, _ = prepare(GenProfile.ADVERSARIAL, n, Chain.GenericUlp, seed=4444)
    packets = split(cases.frames_of(arena, off, lens), seed=3)
    tables = cases.place(packets, misalign=list(range(16)) + [1], gap=2)
    recs = read_recs(tables)
    assert (recs["status"] == ingot_amd.ParseError.StraddledHeader).sum() > 500
    want = check_both_modes(ctx, torch, tables, recs, tag="adversarial")
    ok = recs["status"] == 0
    _same_rows(want[ok], csum_model.verify(arena, off, lens, recs)[ok], "Ok records")
    # few ADVERSARIAL frames carry a whole, unfragmented segment at all
    assert np.isin(want["l4_state"], (OK, BAD, ZERO)).sum() > 100
    assert (want["l4_state"] == FRAGMENT).sum() > 100
    assert (want["l4_state"][~ok] == NONE).all()


# ---------------------------------------------------------------------------
# one chunk per packet: the contiguous kernel's answer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mis", [0, 1, 15])
def test_one_chunk_per_packet_is_the_contiguous_call(ctx, torch, mis):
    """k_csum and k_csum_read share their header decode, block reduction and
    finish (csum.hip).  257 MIXED frames (a full group and one packet), the
    arena copied to byte misalignment `mis`, every packet one chunk, the same
    records for both: checksum_verify_read's rows are checksum_verify's, and
    checksum_fill_read leaves checksum_fill's rows and arena bytes."""
    n = GROUP + 1
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=257, slack=64)
    recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    moved = np.full(len(arena) + 16, 0xA5, np.uint8)
    moved[mis:mis + len(arena)] = arena
    d_off, d_len = _dev(torch, off + np.uint64(mis)), _dev(torch, lens)
    d_ps = _dev(torch, np.arange(n + 1, dtype=np.uint32))
    d_rec = _dev(torch, recs).view(-1, 16)
    d_a = _dev(torch, moved)
    assert d_a.data_ptr() % 16 == 0
    flat = _rows(ctx.checksum_verify(d_a, d_off, d_len, d_rec))
    _same_rows(_rows(ctx.checksum_verify_read(d_a, d_off, d_len, d_ps, d_rec)), flat, "verify")
    assert d_a.cpu().numpy().tobytes() == moved.tobytes()
    assert (flat["l4_len"] > 0).sum() > n // 2 and (flat["l3_state"] != NONE).sum() > n // 4
    d_b = d_a.clone()
    rows_a = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
    rows_b = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
    ctx.checksum_fill(d_a, d_off, d_len, d_rec, out=rows_a)
    ctx.checksum_fill_read(d_b, d_off, d_len, d_ps, d_rec, out=rows_b)
    _same_rows(_rows(rows_b), _rows(rows_a), "fill")
    got_a, got_b = d_a.cpu().numpy(), d_b.cpu().numpy()
    bad = np.nonzero(got_a != got_b)[0]
    assert bad.size == 0, ("arena after fill", bad[:10], got_a[bad[:10]], got_b[bad[:10]])
    assert (got_a != moved).sum() > n // 2  # the fill wrote


# ---------------------------------------------------------------------------
# aliased payload, the encapsulation, arguments, streams
# ---------------------------------------------------------------------------
def test_aliased_payload_chunk(ctx, torch):
    """Two packets whose payload chunk is the same bytes (verify only)."""
    pay = bytes(range(200, 255)) * 3
    a, b = cf.frame("v4", cf.UDP, pay), cf.frame("v6", cf.UDP, pay)
    frames, recs = valid([a, b])
    ha, hb = frames[0][:42], frames[1][:62]
    arena, so, sl, ps = cases.place([[ha, pay], [hb]], misalign=[2, 9, 4], gap=3)
    so = np.array([so[0], so[1], so[2], so[1], so[3]], dtype=np.uint64)
    sl = np.array([sl[0], sl[1], sl[2], sl[1], 0], dtype=np.uint16)
    ps = np.array([0, 2, 4], dtype=np.uint32)
    tables = (arena, so, sl, ps)
    rr = read_recs(tables)
    assert rr.tobytes() == recs.tobytes()
    want = model.verify(tables, rr)
    assert (want["l4_state"] == OK).all()
    d = [_dev(torch, x) for x in tables]
    _same_rows(_rows(ctx.checksum_verify_read(*d, _dev(torch, rr).view(-1, 16))), want)
    assert d[0].cpu().numpy().tobytes() == arena.tobytes()


def test_two_chunk_encapsulation(ctx, torch):
    """emit_headers writes the Geneve-over-IPv6 stack into slots; packet i is
    then (slot i, source frame i).  A UDP_PARSER parse_read of those chunks
    and checksum_fill_read(L4) give, chunk after chunk, the packet
    ingot_gpu_emit_packets_csum writes for the same arguments with the UDP sum
    named, and the source frames are untouched."""
    n = 4_000
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=33, slack=64)
    arena = arena.copy()
    csum_model.fill(arena, off, lens, oracle.parse_batch(arena, off, lens, Chain.GenericUlp))
    hdr = (E.ethernet(bytes.fromhex("a84025777776"), bytes.fromhex("a84025777777"), 0x86DD)
           + E.ipv6(bytes.fromhex("fd000000f70101000000000000000002"),
                    bytes.fromhex("fd000000f70101000000000000000001"), 17, hop_limit=0xF0)
           + E.udp(0xC0DE, 6081, checksum=0) + E.geneve(0x123456, options=E.geneve_opt(0x0129, 0)))
    H, stride = len(hdr), 128
    sets = [(14, Field.V6_PAYLOAD_LEN, EmitSource.LENGTH, -40),
            (54, Field.UDP_LENGTH, EmitSource.LENGTH, 0)]
    d_src, d_off, d_len = _dev(torch, arena), _dev(torch, off), _dev(torch, lens)
    # one arena for the tables: the header slots, then a copy of the source arena
    base = n * stride
    d_all = torch.full((base + len(arena),), 0xA5, dtype=torch.uint8, device="cuda")
    d_all[base:] = d_src
    ctx.emit_header_blocks(hdr, sets, d_len, d_all, stride=stride)
    seg_off = np.empty(2 * n + 1, dtype=np.uint64)
    seg_len = np.empty(2 * n + 1, dtype=np.uint16)
    seg_off[0:2 * n:2] = np.arange(n, dtype=np.uint64) * stride
    seg_off[1:2 * n:2] = off + np.uint64(base)
    seg_len[0:2 * n:2] = H
    seg_len[1:2 * n:2] = lens
    seg_off[-1], seg_len[-1] = 0, 0
    pkt_seg = (np.arange(n + 1) * 2).astype(np.uint32)
    d_tab = (_dev(torch, seg_off), _dev(torch, seg_len), _dev(torch, pkt_seg))
    recs, _ = ctx.parse_read(d_all, *d_tab, Chain.UdpParser)
    host_all = d_all.cpu().numpy().copy()
    w_rec = oracle.parse_read_batch(host_all, seg_off, seg_len, pkt_seg, Chain.UdpParser)[0]
    assert recs.cpu().numpy().tobytes() == w_rec.tobytes() and (w_rec["status"] == 0).all()
    before = _rows(ctx.checksum_verify_read(d_all, *d_tab, recs, CSUM_L4))
    assert (before["l4_state"] == ZERO).all()  # the header block's constant
    rows = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
    ctx.checksum_fill_read(d_all, *d_tab, recs, CSUM_L4, out=rows)
    w_rows = model.fill((host_all, seg_off, seg_len, pkt_seg), w_rec, CSUM_L4)
    _same_rows(_rows(rows), w_rows)
    assert (w_rows["l4_state"] == OK).all()
    assert (w_rows["l4_len"] == lens.astype(np.int64) + H - 54).all()
    got = d_all.cpu().numpy()
    assert got.tobytes() == host_all.tobytes()
    assert got[base:].tobytes() == arena.tobytes()  # the source frames are untouched
    # the copying call, same arguments, the UDP sum named
    ln = lens.astype(np.int64)
    dst_off = (np.cumsum(np.r_[0, ln[:-1] + H + 3]) + 1).astype(np.uint64)
    d_dst = torch.full((int(dst_off[-1]) + int(ln[-1]) + H + 64,), 0xA5, dtype=torch.uint8,
                       device="cuda")
    ctx.emit_packets(hdr, sets, d_src, d_off, d_len, d_dst, _dev(torch, dst_off),
                     sums=[(EmitSum.UDP, 54, 14)])
    copied = d_dst.cpu().numpy()
    for i in range(n):
        o = int(dst_off[i])
        two = got[i * stride:i * stride + H].tobytes() + \
            got[base + int(off[i]):base + int(off[i]) + int(lens[i])].tobytes()
        assert copied[o:o + H + int(lens[i])].tobytes() == two, i


def test_argument_errors(ctx, torch):
    lib = ingot_amd._lib.load()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    r = torch.zeros((10, 16), dtype=torch.uint8, device="cuda")
    o = torch.zeros((10, 8), dtype=torch.uint8, device="cuda")
    so = torch.zeros(10, dtype=torch.int64, device="cuda")
    sl = torch.zeros(10, dtype=torch.int16, device="cuda")
    ps = torch.arange(11, dtype=torch.int32, device="cuda")
    h, A, R, O, SO, SL, PS = ctx._h, a.data_ptr(), r.data_ptr(), o.data_ptr(), so.data_ptr(), \
        sl.data_ptr(), ps.data_ptr()
    for fn in (lib.ingot_gpu_checksum_verify_read, lib.ingot_gpu_checksum_fill_read):
        assert fn(None, A, SO, SL, PS, 10, R, 3, O, None) == -1
        for what in (0, 4, 8 | 1):
            assert fn(h, A, SO, SL, PS, 10, R, what, O, None) == -1
        assert fn(h, None, SO, SL, PS, 10, R, 3, O, None) == -1
        assert fn(h, A, None, SL, PS, 10, R, 3, O, None) == -1
        assert fn(h, A, SO, None, PS, 10, R, 3, O, None) == -1
        assert fn(h, A, SO, SL, None, 10, R, 3, O, None) == -1
        assert fn(h, A, SO, SL, PS, 10, None, 3, O, None) == -1
        assert fn(h, None, None, None, None, 0, None, 3, None, None) == 0  # empty batch
        assert fn(h, A, SO, SL, PS, 10, R, 3, O, None) == 0
    assert lib.ingot_gpu_checksum_verify_read(h, A, SO, SL, PS, 10, R, 3, None, None) == -1
    assert lib.ingot_gpu_checksum_fill_read(h, A, SO, SL, PS, 10, R, 3, None, None) == 0
    with pytest.raises(ValueError):
        ctx.checksum_verify_read(a, so, sl, ps, r, what=0)
    with pytest.raises(ValueError):
        ctx.checksum_fill_read(a, so, sl, ps, r[:5])
    torch.cuda.synchronize()


def test_fill_without_rows_on_a_side_stream(ctx, torch):
    """d_out NULL is accepted by fill, and a launch on a side stream gives
    the default stream's result."""
    rng = np.random.default_rng(8)
    arena, off, lens = gen_frames_host(GenProfile.MIXED, 3_000, seed=78, slack=64)
    crecs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    packets = [cases.cut(f, crecs[i], rng)
               for i, f in enumerate(cases.frames_of(arena, off, lens))]
    tables = cases.place(packets, misalign=list(range(16)) + [5], gap=1)
    recs = read_recs(tables)
    d_tab = [_dev(torch, x) for x in tables[1:]]
    d_rec = _dev(torch, recs).view(-1, 16)
    a0, a1 = _dev(torch, tables[0]), _dev(torch, tables[0])
    out0 = torch.zeros((len(recs), 8), dtype=torch.uint8, device="cuda")
    ctx.checksum_fill_read(a0, *d_tab, d_rec, out=out0)
    torch.cuda.synchronize()
    # A HIP stream of the test's own, wrapped for torch, and destroyed below:
    # torch hands out its pooled streams in turn, and which hardware queue a
    # stream shares decides what a doorbell wait stalls, so
    # this test draws none and the tests that run later get the streams they
    # always got.
    lib = ingot_amd._lib.load()
    raw = ctypes.c_void_p()
    lib.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lib.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    assert lib.hipStreamCreateWithFlags(ctypes.byref(raw), 1) == 0  # hipStreamNonBlocking
    side = torch.cuda.ExternalStream(raw.value)
    with torch.cuda.stream(side):
        assert ctx.checksum_fill_read(a1, *d_tab, d_rec, stream=side) is None
        rows1 = ctx.checksum_verify_read(a1, *d_tab, d_rec, stream=side)
    side.synchronize()
    torch.cuda.synchronize()
    assert lib.hipStreamDestroy(raw) == 0
    want = tables[0].copy()
    w_rows = model.fill((want,) + tables[1:], recs)
    assert a0.cpu().numpy().tobytes() == want.tobytes()
    assert a1.cpu().numpy().tobytes() == want.tobytes()
    _same_rows(_rows(out0), w_rows)
    _same_rows(_rows(rows1), w_rows)
