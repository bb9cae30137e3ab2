"""ingot_gpu_parse_read_modify_rows on the device against the definition
(tests/modify_read_rows_model.py): after every call the WHOLE arena equals the
model's arena (gaps, neighbours and payload chunks included), the records equal
oracle.parse_read_batch's and d_chunk the oracle's; both outputs are pre-filled
with a sentinel.  The batches are tests/modify_read_rows_cases.py's, each held
to the chunk paths it must reach by tests/test_modify_read_rows_model.py (the
emit_headers route makes its batch on the device and checks its own).  Default
stream only.  Needs an MI355X: `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import CSUM_DTYPE, CSUM_L4, Chain, EditOp, EmitSource, Field, GenProfile, abi
from ingot_amd import emit as E
from ingot_amd.abi import (CSUM_OUTER_L4, ROW_NONE, TUNE_MAX_BLOCKS, TUNE_READ_PLAN, EditBy,
                           EditSource, WideField)
from ingot_amd.hostgen import gen_frames_host
from tests import csum_model
from tests import modify_read_cases as mc
from tests import modify_read_model as mrm
from tests import modify_read_rows_cases as rc2
from tests import modify_read_rows_model as model
from tests import modify_rows_cases as rc

pytestmark = pytest.mark.gpu

TUN = Chain.GeneveOverV6Tunnel
SET, SUB = EditOp.SET, EditOp.SUB
OK = 1  # ingot_csum state
chains = pytest.mark.parametrize("chain", rc2.CHAINS, ids=lambda c: c.name)


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
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
              np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype)).copy()).cuda()


class Device:
    """A batch's tables on the device once; run() restores the arena, fills the
    outputs with sentinels, makes the call and returns (arena, records, chunk)
    as numpy."""

    def __init__(self, ctx, torch, tables, chain):
        self.ctx, self.torch, self.tables, self.chain = ctx, torch, tables, chain
        self.n = len(tables[3]) - 1
        self.pristine = _dev(torch, tables[0])
        self.arena = self.pristine.clone()
        self.tab = [_dev(torch, x) for x in tables[1:]]
        self.out = torch.zeros((self.n, 16), dtype=torch.uint8, device="cuda")
        self.chunk = torch.zeros(self.n, dtype=torch.int16, device="cuda")
        self.parsed = mrm.parse(tables, chain)
        self.uploads = {}

    def run(self, edits, rows, n_rows, what, ctx=None):
        self.arena.copy_(self.pristine)
        self.out.fill_(0xEE)
        self.chunk.fill_(-1)
        d_rows = None if rows is None else _dev(self.torch, rows)
        (ctx or self.ctx).parse_read_modify_rows(
            self.arena, *self.tab, self.chain, rc.device_edits(self.torch, edits, self.uploads),
            rows=d_rows, n_rows=n_rows, csum=what, out=self.out, chunk=self.chunk)
        self.torch.cuda.synchronize()
        return (self.arena.cpu().numpy(), self.out.cpu().numpy(),
                self.chunk.cpu().numpy().view(np.uint16))

    def check(self, edits, rows, n_rows, what, tag="", ctx=None):
        """The call against the model: whole arena, records, chunk indices.
        Returns the model's arena."""
        want, recs, w_chunk = model.apply(self.tables, self.chain, edits, rows, n_rows, what,
                                          parsed=self.parsed)
        got, g_rec, g_chunk = self.run(edits, rows, n_rows, what, ctx)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (tag, what, bad[:10], got[bad[:10]], want[bad[:10]],
                               self.tables[0][bad[:10]])
        assert g_rec.tobytes() == recs.tobytes(), (tag, "records")
        assert (g_chunk == w_chunk).all(), (tag, "chunk")
        return want


def check_batch(ctx, torch, b, what, dev=None, use=None):
    d = dev or Device(ctx, torch, b.tables, b.chain)
    return d, d.check(b.edits, b.rows, b.n_rows, what, b.name, ctx=use)


# ---------------------------------------------------------------------------
# Tile edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tile_edges(ctx, torch, n):
    b = rc2.tile_batch(n)
    _, want = check_batch(ctx, torch, b, 3)
    assert n == 1 or (want != b.tables[0]).any()


# ---------------------------------------------------------------------------
# Chains and sums: one header per chunk, tables by packet and by row
# ---------------------------------------------------------------------------
@chains
def test_chains_with_and_without_sums(ctx, torch, chain):
    b = rc2.batch(chain, 257, "headers")
    d = None
    for what in (0, rc2.FULL_WHAT[chain]):
        d, want = check_batch(ctx, torch, b, what, d)
        assert (want != b.tables[0]).any()


# ---------------------------------------------------------------------------
# Device against device
# ---------------------------------------------------------------------------
@chains
def test_one_chunk_per_packet_equals_parse_modify_rows(ctx, torch, chain):
    b = rc2.batch(chain, 129, "single")
    d = Device(ctx, torch, b.tables, chain)
    d_off, d_len = d.tab[0][:129].contiguous(), d.tab[1][:129].contiguous()
    d_rows = _dev(torch, b.rows)
    for what in (0, rc2.FULL_WHAT[chain]):
        want = d.check(b.edits, b.rows, b.n_rows, what, "one chunk")
        a = d.pristine.clone()
        recs = torch.zeros((129, 16), dtype=torch.uint8, device="cuda")
        ctx.parse_modify_rows(a, d_off, d_len, chain, rc.device_edits(torch, b.edits, d.uploads),
                              rows=d_rows, n_rows=b.n_rows, out=recs, csum=what)
        torch.cuda.synchronize()
        assert a.cpu().numpy().tobytes() == want.tobytes(), (what, "parse_modify_rows")
        assert recs.cpu().numpy().tobytes() == d.parsed[0].tobytes()
        assert (want != b.tables[0]).any()


@pytest.mark.parametrize("profile,chain,cutter", mc.CUT_SETS,
                         ids=[f"{p}-{c.name}-{k}" for p, c, k in mc.CUT_SETS])
def test_value_only_lists_equal_parse_read_modify_csum(ctx, torch, profile, chain, cutter):
    b = rc2.value_batch(profile, chain, cutter)
    d = Device(ctx, torch, b.tables, chain)
    _, full = mc.nat_list(chain)
    for what in (0, full):
        want = d.check(b.edits, None, 0, what, b.name)
        a = d.pristine.clone()
        out = torch.zeros((d.n, 16), dtype=torch.uint8, device="cuda")
        chunk = torch.zeros(d.n, dtype=torch.int16, device="cuda")
        ctx.parse_read_modify(a, *d.tab, chain, b.edits, csum=what, out=out, chunk=chunk)
        torch.cuda.synchronize()
        assert a.cpu().numpy().tobytes() == want.tobytes(), (what, "parse_read_modify")
        assert out.cpu().numpy().tobytes() == d.parsed[0].tobytes()
        assert (chunk.cpu().numpy().view(np.uint16) == d.parsed[2]).all()
    assert (want != b.tables[0]).any()


# ---------------------------------------------------------------------------
# Placements: the aligned and the byte form of the located store
# ---------------------------------------------------------------------------
@chains
def test_placements_and_neighbours(ctx, torch, chain):
    """Chunks at descending addresses, starts at every address mod 4; byte
    tables at odd addresses with pitches 35 and 19; 2-, 4-, 6- and 16-byte
    fields.  The bytes on both sides of every edited field are the model's
    (they are part of the whole-arena comparison; named here once more)."""
    b = rc2.with_edits(rc2.batch(chain, 257, "headers", placement="descending"), "placement",
                       rc2.placement_edits(chain, 257))
    d = None
    for what in (0, rc2.FULL_WHAT[chain]):
        d, want = check_batch(ctx, torch, b, what, d)
        got = d.arena.cpu().numpy()
        nb = rc2.neighbours(b, d.parsed)
        assert len(nb) > 500 and (got[nb] == want[nb]).all()
        assert (want != b.tables[0]).any()


# ---------------------------------------------------------------------------
# Dependent lists through the located store
# ---------------------------------------------------------------------------
@chains
def test_dependent_lists(ctx, torch, chain):
    base = rc2.batch(chain, 257, "headers")
    d = Device(ctx, torch, base.tables, chain)
    for name, edits in rc2.dependent_lists(chain, 257):
        b = rc2.with_edits(base, name, edits)
        for what in (rc2.FULL_WHAT[chain], 0):
            _, want = check_batch(ctx, torch, b, what, d)
            assert (want != b.tables[0]).any(), name


# ---------------------------------------------------------------------------
# The row guard
# ---------------------------------------------------------------------------
def test_guard_cases(ctx, torch):
    g = rc2.batch(Chain.GenericUlp, 257)
    d = Device(ctx, torch, g.tables, g.chain)
    # every packet guarded: nothing is written, records and chunks are parse_read's
    for rows, n_rows in ((np.full(257, ROW_NONE, np.uint32), rc2.N_ROWS), (g.rows, 0)):
        want = d.check(g.edits, rows, n_rows, 3, "all guarded")
        assert want.tobytes() == g.tables[0].tobytes()
    rec, chunk = ctx.parse_read(d.pristine, *d.tab, g.chain)
    torch.cuda.synchronize()
    assert d.out.cpu().numpy().tobytes() == rec.cpu().numpy().tobytes()
    assert (d.chunk.cpu().numpy() == chunk.cpu().numpy()).all()
    # one survivor per 64-packet tile
    s = rc2.with_edits(g, "survivors", g.edits, rc2.one_survivor_rows(257))
    _, want = check_batch(ctx, torch, s, 3, d)
    assert (want != g.tables[0]).any()
    # d_row NULL, BY_PACKET only: every Ok packet is edited, n_rows is ignored
    p = rc2.batch(Chain.GenericUlp, 257, by_row=False)
    d2 = Device(ctx, torch, p.tables, p.chain)
    want = d2.check(p.edits, None, 12345, 3, "no d_row")
    ok = np.nonzero(d2.parsed[0]["status"] == 0)[0]
    assert all(rc2.logical(want, p.tables, i) != rc2.logical(p.tables[0], p.tables, i) for i in ok)


def test_packets_that_are_not_ok_keep_every_byte(ctx, torch):
    from ingot_amd import ParseError

    b = rc2.not_ok_batch()
    d, want = check_batch(ctx, torch, b, 3)
    st = d.parsed[0]["status"]
    assert (st == ParseError.StraddledHeader).sum() > 20 and (st == ParseError.TooSmall).any()
    assert int(b.tables[3][10]) == int(b.tables[3][9])  # a packet with no chunks
    for i in np.nonzero(st != 0)[0]:
        assert rc2.logical(want, b.tables, i) == rc2.logical(b.tables[0], b.tables, i), i
    assert (want != b.tables[0]).any()


# ---------------------------------------------------------------------------
# Both kernels, later trips of the tile loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("blocks,plan", [(1, 0), (3, 0), (3, 1)])
def test_both_windows_and_later_trips(torch, blocks, plan):
    """833 packets are 14 tiles: with 1 or 3 blocks every wave takes later
    trips.  READ_PLAN 1 selects the 4-piece kernels."""
    c = ingot_amd.Context(0)
    c.set_tuning(TUNE_MAX_BLOCKS, blocks)
    c.set_tuning(TUNE_READ_PLAN, plan)
    b = rc2.batch(Chain.GenericUlp, 833)
    _, want = check_batch(c, torch, b, 3)
    assert (want != b.tables[0]).any()


@chains
def test_four_piece_window_on_every_chain(torch, chain):
    c = ingot_amd.Context(0)
    c.set_tuning(TUNE_READ_PLAN, 1)
    check_batch(c, torch, rc2.batch(chain, 257, "headers"), rc2.FULL_WHAT[chain])


# ---------------------------------------------------------------------------
# emit_headers, then this call over (slot, source frame)
# ---------------------------------------------------------------------------
def _rows(t):
    return t.cpu().numpy().view(CSUM_DTYPE).reshape(-1)


def test_emit_headers_route(ctx, torch):
    """emit_header_blocks writes the Geneve-over-IPv6 stack into slots; packet i
    is (slot i, source frame i), the outer UDP sum filled by checksum_fill_read.
    Then this call: the outer IPv6 destination and the outer MAC BY_ROW, the VNI
    from a u32 table, what = 7.  checksum_verify_read under a UdpParser
    parse_read reports the outer sum Ok for every packet, and the bytes are the
    model's."""
    n = 1_000
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
    base = n * stride
    d_all = torch.full((base + len(arena),), 0xA5, dtype=torch.uint8, device="cuda")
    d_all[base:] = _dev(torch, arena)
    ctx.emit_header_blocks(hdr, sets, _dev(torch, lens), d_all, stride=stride)
    seg_off = np.empty(2 * n + 1, dtype=np.uint64)
    seg_len = np.empty(2 * n + 1, dtype=np.uint16)
    seg_off[0:2 * n:2] = np.arange(n, dtype=np.uint64) * stride
    seg_off[1:2 * n:2] = off + np.uint64(base)
    seg_len[0:2 * n:2] = H
    seg_len[1:2 * n:2] = lens
    seg_off[-1], seg_len[-1] = 0, 0
    pkt_seg = (np.arange(n + 1) * 2).astype(np.uint32)
    d_tab = (_dev(torch, seg_off), _dev(torch, seg_len), _dev(torch, pkt_seg))
    o_rec, _ = ctx.parse_read(d_all, *d_tab, Chain.UdpParser)
    ctx.checksum_fill_read(d_all, *d_tab, o_rec, CSUM_L4)
    filled = _rows(ctx.checksum_verify_read(d_all, *d_tab, o_rec, CSUM_L4))
    assert (filled["l4_state"] == OK).all()
    torch.cuda.synchronize()
    tables = (d_all.cpu().numpy().copy(), seg_off, seg_len, pkt_seg)
    r = rc.nat_table(rc2.N_ROWS, 51)
    vni = np.random.default_rng(52).integers(0, 1 << 24, n).astype(np.uint32)
    rows = rc2.mixed_rows(n)
    edits = [(1, WideField.V6_DESTINATION, SET, ("row", r[:, 16:32])),
             (0, WideField.ETH_DESTINATION, SET, ("row", r[:, 1:7])),
             (3, Field.GENEVE_VNI, SET, vni), (5, Field.V4_HOP_LIMIT, SUB, 1),
             (5, Field.V6_HOP_LIMIT, SUB, 1)]
    d = Device(ctx, torch, tables, TUN)
    assert (d.parsed[0]["status"] == 0).sum() > n // 2
    want = d.check(edits, rows, rc2.N_ROWS, 7, "emit_headers route")
    assert (want[:base] != tables[0][:base]).any() and (want[base:] != tables[0][base:]).any()
    o_rec2, _ = ctx.parse_read(d.arena, *d.tab, Chain.UdpParser)
    assert o_rec2.cpu().numpy().tobytes() == o_rec.cpu().numpy().tobytes()
    after = _rows(ctx.checksum_verify_read(d.arena, *d.tab, o_rec2, CSUM_L4))
    assert (after["l4_state"] == OK).all(), np.nonzero(after["l4_state"] != OK)[0][:5]


# ---------------------------------------------------------------------------
# The raw ABI: every EINVAL of the header's list, in its order; n == 0
# ---------------------------------------------------------------------------
def test_every_einval_leaves_everything_alone(ctx, torch):
    b = rc2.tile_batch(64)
    d = Device(ctx, torch, b.tables, b.chain)
    d.out.fill_(0xEE)
    d.chunk.fill_(-1)
    d_rows = torch.zeros(64, dtype=torch.int32, device="cuda")
    tab = torch.zeros((64, 32), dtype=torch.uint8, device="cuda")
    p = tab.data_ptr()
    G, lib = int(Chain.GenericUlp), ctx._lib
    V, U16, U32, B = (int(x) for x in EditSource)
    PKT, ROW = int(EditBy.PACKET), int(EditBy.ROW)
    MAC, V6 = int(WideField.ETH_SOURCE), int(WideField.V6_SOURCE)
    F = Field
    A = d.arena.data_ptr()
    SO, SL, PS = (t.data_ptr() for t in d.tab)

    def call(edits, what=0, chain=G, rows=d_rows, n=64, arena_p=A, so=SO, sl=SL, ps=PS, h=ctx._h,
             n_edits=None, null_list=False, pad=0):
        e = abi.edit_rows_array(edits)
        e["_pad"] = pad
        return lib.ingot_gpu_parse_read_modify_rows(
            h, arena_p, so, sl, ps, n, chain,
            None if null_list else e.ctypes.data_as(ctypes.c_void_p),
            len(e) if n_edits is None else n_edits, None if rows is None else rows.data_ptr(),
            64, what, d.out.data_ptr(), d.chunk.data_ptr(), None)

    # (layer, field, op, index, value, source, by, pitch, d_values)
    good = (1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 32, p)
    refused = (1, F.V4_IHL, SET, 0, 5, V, PKT, 0, 0)
    bad = {  # in the header's order: 1. the call's own; 2. per edit; 3. `what`
        "NULL context": dict(edits=[good], h=None),
        "bad chain": dict(edits=[good], chain=99),
        "too many edits": dict(edits=[good] * 17),
        "NULL list": dict(edits=[good], null_list=True),
        "unknown narrow field": dict(edits=[(1, 48, SET, 0, 0, U32, PKT, 0, p)]),
        "field between the enums": dict(edits=[(1, 63, SET, 0, 0, B, PKT, 0, p)]),
        "field past the wide ones": dict(edits=[(1, 68, SET, 0, 0, B, PKT, 0, p)]),
        "unknown op": dict(edits=[(1, F.V4_SOURCE, 6, 0, 0, U32, PKT, 0, p)]),
        "layer out of range": dict(edits=[(3, F.V4_SOURCE, SET, 0, 0, U32, PKT, 0, p)]),
        "bad source": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, 4, PKT, 0, p)]),
        "bad by": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, 2, 0, p)]),
        "non-zero _pad": dict(edits=[good], pad=1),
        "value with a table": dict(edits=[(1, F.V4_SOURCE, SET, 0, 9, U32, PKT, 0, p)]),
        "NULL table": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 0, 0)]),
        "BYTES on a narrow field": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, B, PKT, 0, p)]),
        "U32 on a wide field": dict(edits=[(0, MAC, SET, 0, 0, U32, PKT, 0, p)]),
        "VALUE on a wide field": dict(edits=[(0, MAC, SET, 0, 5, V, PKT, 0, 0)]),
        "wide field with ADD": dict(edits=[(1, V6, EditOp.ADD, 0, 0, B, PKT, 0, p)]),
        "pitch below u32": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 2, p)]),
        "pitch below a MAC": dict(edits=[(0, MAC, SET, 0, 0, B, PKT, 5, p)]),
        "pitch below an address": dict(edits=[(1, V6, SET, 0, 0, B, PKT, 15, p)]),
        "odd u16 table": dict(edits=[(2, F.UDP_SOURCE, SET, 0, 0, U16, PKT, 0, p + 1)]),
        "odd u16 pitch": dict(edits=[(2, F.UDP_SOURCE, SET, 0, 0, U16, PKT, 3, p)]),
        "misaligned u32 table": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 0, p + 2)]),
        "misaligned u32 pitch": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 6, p)]),
        "BY_ROW without d_row": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, ROW, 0, p)],
                                     rows=None),
        "BY_ROW VALUE without d_row": dict(edits=[(1, F.V4_SOURCE, SET, 0, 7, V, ROW, 0, 0)],
                                           rows=None),
        "what above 7": dict(edits=[good], what=8),
        "OUTER_L4 outside the tunnel": dict(edits=[good], what=CSUM_OUTER_L4),
        "a refused field": dict(edits=[refused], what=3),
        # 1 to 3 come before "n == 0 succeeds"
        "what above 7, n == 0": dict(edits=[good], what=8, n=0),
        "a refused field, n == 0": dict(edits=[refused], what=3, n=0),
        "bad by, n == 0, no tables": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, 2, 0, p)], n=0,
                                          arena_p=None, so=None, sl=None, ps=None),
        # 3. n > 0: a NULL arena or chunk table
        "NULL arena": dict(edits=[good], arena_p=None),
        "NULL seg_off": dict(edits=[good], so=None),
        "NULL seg_len": dict(edits=[good], sl=None),
        "NULL pkt_seg": dict(edits=[good], ps=None),
    }
    for name, kw in bad.items():
        assert call(**kw) == -1, name
    # n == 0 succeeds whatever the device pointers are; a refused field without sums is an edit
    assert call([good], n=0, arena_p=None, so=None, sl=None, ps=None) == 0
    assert call([refused], n=0) == 0
    torch.cuda.synchronize()
    assert d.arena.cpu().numpy().tobytes() == b.tables[0].tobytes(), "a refused call wrote"
    assert (d.out.cpu().numpy() == 0xEE).all() and (d.chunk.cpu().numpy() == -1).all()
    assert not tab.any()
    # and the list they were made from is accepted
    assert call([good]) == 0
    torch.cuda.synchronize()
    assert (d.arena.cpu().numpy() != b.tables[0]).any()
    assert d.out.cpu().numpy().tobytes() == d.parsed[0].tobytes()


def test_wrapper_arguments(ctx, torch):
    b = rc2.tile_batch(64)
    d = Device(ctx, torch, b.tables, b.chain)
    t = torch.zeros((64, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):  # ("row", tensor) needs rows
        ctx.parse_read_modify_rows(d.arena, *d.tab, b.chain,
                                   [(1, WideField.V6_SOURCE, SET, ("row", t))])
    with pytest.raises(ValueError):  # pkt_seg of the wrong type
        ctx.parse_read_modify_rows(d.arena, d.tab[0], d.tab[1], d.tab[0], b.chain, [])
    # neither output given: (None, None); n == 0 through the wrapper
    assert ctx.parse_read_modify_rows(d.arena, *d.tab, b.chain,
                                      [(1, WideField.V6_SOURCE, SET, t)]) == (None, None)
    empty = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert ctx.parse_read_modify_rows(d.arena, d.tab[0], d.tab[1], empty, b.chain,
                                      [(1, Field.V4_HOP_LIMIT, SUB, 1)]) == (None, None)
    torch.cuda.synchronize()
