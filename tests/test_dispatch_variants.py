"""The kernels a tuning key or the arena's memory kind selects, and the second
trip round every grid-stride tile loop, on the device (batches and expected
values: tests/dispatch_cases.py, held to account by tests/test_dispatch_cases.py):

A. k_parse in rewrite mode, plain and with the fused RFC 1624 update, walking
   several tiles per wave (INGOT_TUNE_MAX_BLOCKS 1 and 3);
B. k_parse in every record / field mode and every form of k_parse_read, the
   same way;
C. k_parse_read_modify: the 4-piece window (INGOT_TUNE_READ_PLAN 1), the tile
   loop of both windows, plain record stores (INGOT_TUNE_CACHE_POLICY 4);
D. the chunked write calls over mblk chains in mapped host memory.

Every comparison is byte for byte: the whole arena (the bytes between frames
and chunks included), the records, the chunk indices, d_taken.  Each
docstring names the launcher condition the test relies on;
profiles/r16_dispatch_variants_kernels.csv lists the kernels this file
launched under a kernel trace.  Needs an MI355X: `pytest -m gpu`."""
import contextlib
import ctypes

import numpy as np
import pytest

import ingot_amd
from ingot_amd import CSUM_DTYPE, CSUM_L3, CSUM_L4, Chain, abi
from ingot_amd.abi import emit_sums_array
from tests import csum_read_model
from tests import csum_sweep_cases as sc
from tests import dispatch_cases as dc
from tests import emit_csum_cases as ecases
from tests import emit_read_model
from tests import modify_read_cases as mc
from tests import test_modify_read as tmr
from tests.test_hostmap import _page_aligned
from tests.test_modify_csum import same

pytestmark = pytest.mark.gpu
TUN = dc.TUN
BOTH = CSUM_L3 | CSUM_L4
chains = pytest.mark.parametrize("chain", sc.CHAINS, ids=lambda c: c.name)
every_chain = pytest.mark.parametrize("chain", list(Chain), ids=lambda c: c.name)
blocks = pytest.mark.parametrize("blocks", dc.BLOCKS)
cut_sets = pytest.mark.parametrize("profile,chain,cutter", mc.CUT_SETS,
                                   ids=[f"{p}-{c.name}-{k}" for p, c, k in mc.CUT_SETS])
host_sets = pytest.mark.parametrize("profile,chain,n", dc.HOST_SETS,
                                    ids=[f"{p}-{c.name}" for p, c, _ in dc.HOST_SETS])


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return ingot_amd.Context(0)


def tuned(**keys):
    """A context with INGOT_TUNE_<name> = value for every keyword, each read
    back: a key the library dropped would make the test prove nothing."""
    c = ingot_amd.Context(0)
    for name, value in keys.items():
        key = getattr(abi, "TUNE_" + name)
        c.set_tuning(key, value)
        assert c.get_tuning(key) == value, name
    return c


def _dev(torch, a):
    """A numpy array on the device (unsigned tables as the signed view of the same bits)."""
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)  # (shared inputs are read-only)
    if a.dtype.fields:
        a = a.view(np.uint8)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
              np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()


def _host(t):
    return t.cpu().numpy()


def _poison(torch, rows: int, width: int):
    """An output buffer no call has written: torch hands a freed block out
    again, so a fresh torch.empty may already hold the previous call's (equal)
    answer, and a tile the loop skipped would go unnoticed."""
    return torch.full((rows, width), 0xEE, dtype=torch.uint8, device="cuda")


def _no_chunk(torch, n: int):
    return torch.full((n,), -1, dtype=torch.int16, device="cuda")


def _same_rows(got, want, n, what):
    """Fixed-width rows (records, field blocks) byte for byte, naming the first rows that differ."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(n, -1)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(n, -1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:8], [int(dc.iteration_class(i)) for i in bad[:8]])


# ---------------------------------------------------------------------------
# A. grid-stride loop of the contiguous rewrite
# ---------------------------------------------------------------------------
@blocks
@pytest.mark.parametrize("layout", dc.LAYOUTS)
@chains
def test_rewrite_loop(torch, chain, layout, blocks):
    """k_parse<3 (tunnel 8), INDEXED | STRIDED, chain, OUT_MODIFY, ModifyArgs |
    ModifyCsumArgs> walking 4 and 3 (MAX_BLOCKS 1), 2 and 1 (MAX_BLOCKS 3)
    tiles per wave: launch_modify_as (parse.hip) takes grid_for(n, max_blocks)
    blocks.  Slots: PIPELINE = 1 makes the ring condition at parse.hip:371
    false, so the call reaches k_parse<3, STRIDED, OUT_MODIFY> instead of
    k_modify_pipe (the tunnel's slots go to k_parse<8, STRIDED> either way).
    The NAT list, every dependent list and a list that SETs fields twice,
    under what = 0 and every `what` of the chain; whole arena and records
    against csum_sweep_cases.define, and rewrite + fill where it qualifies."""
    keys = dict(MAX_BLOCKS=blocks)
    if layout == "strided":
        keys["PIPELINE"] = 1
    c = tuned(**keys)
    assert c.get_tuning(abi.TUNE_MAX_BLOCKS) == blocks
    moved = 0
    for k, (name, _, _) in enumerate(dc.rewrite_lists(chain)):
        for what in dc.rewrite_whats(chain):
            e = dc.rewrite_expected(chain, layout, k, what)
            b = e.batch
            t = (name, sc.tag(chain, f"{layout}/blocks={blocks}", e.edits, what))
            d_arena, recs = _dev(torch, b.arena), _poison(torch, b.n, 16)
            c.parse_modify(d_arena, None if b.off is None else _dev(torch, b.off),
                           None if b.lens is None else _dev(torch, b.lens), chain, e.edits,
                           stride=b.stride, n=b.n, out=recs, csum=what)
            got = _host(d_arena)
            _same_rows(_host(recs), e.recs, b.n, t)
            same(got, e.want, t)
            if e.two_pass is not None:
                bad = sc.frames_differ(b, got, e.two_pass, e.both)
                assert bad is None, (t, "two-pass", bad)
            moved += int(e.changed.size > 0)
    assert moved > 15 * len(dc.rewrite_whats(chain)), moved


# ---------------------------------------------------------------------------
# B. grid-stride loop of the parse and of parse_read
# ---------------------------------------------------------------------------
@blocks
@every_chain
def test_parse_loop(torch, chain, blocks):
    """k_parse in OUT_REC16, OUT_REC8 and OUT_FIELDS (the tunnel's field
    blocks included) over indexed, packed and slotted frames, several tiles
    per wave: launch_parse (parse.hip) takes grid_for(n, max_blocks) blocks.
    The slots carry a length array, which makes the ring condition
    (parse.hip:279) false: k_parse<3 (tunnel 8), STRIDED>, not the slot ring.
    Against the oracle, as tests/test_gpu_parity.py."""
    c = tuned(MAX_BLOCKS=blocks)
    assert c.get_tuning(abi.TUNE_MAX_BLOCKS) == blocks
    n = dc.N
    arena, off, lens = (_dev(torch, x) for x in dc.parse_frames(chain == TUN))
    sarena, slens = (_dev(torch, x) for x in dc.slot_frames())
    e = dc.parse_expected(chain)

    def out(width=16):
        return _poison(torch, n, width)

    _same_rows(_host(c.parse(arena, off, lens, chain, out=out())), e["rec"], n, "parse")
    _same_rows(_host(c.parse_packed(arena, lens, chain, out=out())), e["rec"], n, "parse_packed")
    _same_rows(_host(c.parse_strided(sarena, dc.SLOT, n, chain, lens=slens, out=out())),
               e["srec"], n, "parse_strided")
    if chain == TUN:
        width = ingot_amd.GENEVE_FIELDS_DTYPE.itemsize
        fld = c.geneve_fields(arena, off, lens, out=out(width))
        sfld = c.geneve_fields(sarena, None, slens, stride=dc.SLOT, n=n, out=out(width))
    else:
        width = ingot_amd.FIELDS_DTYPE.itemsize
        fld = c.fields(arena, off, lens, chain, out=out(width))
        sfld = c.fields(sarena, None, slens, chain, stride=dc.SLOT, n=n, out=out(width))
        _same_rows(_host(c.parse_compact(arena, off, lens, chain, out=out(8))),
                   ingot_amd.rec16_to_rec8(e["rec"]), n, "parse_compact")
        _same_rows(_host(c.parse_strided_compact(sarena, dc.SLOT, n, chain, lens=slens,
                                                 out=out(8))),
                   ingot_amd.rec16_to_rec8(e["srec"]), n, "parse_strided_compact")
    _same_rows(_host(fld), e["fld"], n, "fields")
    _same_rows(_host(sfld), e["sfld"], n, "fields, slots")


@blocks
@every_chain
def test_parse_read_loop(torch, chain, blocks):
    """Every form of k_parse_read, several tiles per wave (launch_segmented,
    read.hip, gets grid_for(n, max_blocks) from launch_parse): with READ_PLAN 0
    the two-array records <5, REC16> and field blocks <4, FIELDS>, the dense
    table <4, ., DENSE> in both modes and d_first <5, ., FIRST>; with READ_PLAN
    1 the 4-piece records <4, REC16> and d_first <4, ., FIRST>; with READ_PLAN
    17 d_first with lazy bounds <5, ., FIRST, LAZY>.  1-8 chunks per packet;
    records, field blocks and chunk indices against oracle.parse_read_batch."""
    n = dc.N
    tables = dc.read_tables(chain)
    w_rec, w_fld, w_chunk = dc.read_expected(chain)
    d = [_dev(torch, x) for x in tables]
    dense = (tables[1].astype(np.uint64) << np.uint64(16)) | tables[2].astype(np.uint64)
    d_dense = _dev(torch, dense)
    first = ingot_amd.first_chunks(d[1], d[2], d[3])
    kind = "geneve" if chain == TUN else "fields"

    def held(call, want, tag, **kw):
        width = want.dtype.itemsize
        out, chunk = call(out=_poison(torch, n, width), chunk=_no_chunk(torch, n), **kw)
        _same_rows(_host(out), want, n, tag)
        g = _host(chunk).view(np.uint16)
        assert np.array_equal(g, w_chunk), (tag, "chunk", np.nonzero(g != w_chunk)[0][:8])

    for plan in (0, 1, 17):
        c = tuned(MAX_BLOCKS=blocks, READ_PLAN=plan)
        assert c.get_tuning(abi.TUNE_MAX_BLOCKS) == blocks

        def two_array(**kw):
            return c.parse_read(*d, chain, **kw)

        def dense_table(**kw):
            return c.parse_read_dense(d[0], d_dense, d[3], chain, **kw)

        held(two_array, w_rec, (plan, "records"))
        held(two_array, w_rec, (plan, "first"), first=first)
        if plan == 0:
            held(two_array, w_fld, "fields", fields=kind)
            held(dense_table, w_rec, "dense")
            held(dense_table, w_fld, "dense fields", fields=kind)


# ---------------------------------------------------------------------------
# C. the chunked rewrite: loop, 4-piece window, store policy
# ---------------------------------------------------------------------------
SETTINGS = {
    "read_plan=1": dict(READ_PLAN=1),                      # the <4, ...> kernels
    "blocks=1": dict(MAX_BLOCKS=1),                        # the loop of <5, ...>
    "blocks=3,read_plan=1": dict(MAX_BLOCKS=3, READ_PLAN=1),  # the loop of <4, ...>
    "cache_policy=4": dict(CACHE_POLICY=4),                # plain record stores
}


@pytest.mark.parametrize("setting", list(SETTINGS))
@cut_sets
def test_chunked_rewrite_variants(torch, profile, chain, cutter, setting):
    """launch_read_modify_as (read.hip:441-458): READ_PLAN = 1 makes `four`
    true, k_parse_read_modify<4, chain, ModifyArgs | ModifyCsumArgs>; else <5,
    ...> with the line-completing window.  MAX_BLOCKS caps its grid, so the
    waves restage the image while the previous tile's byte stores are in
    flight; CACHE_POLICY = 4 gives p.policy 0, plain record stores.  The NAT
    list without and with the sums over 833 packets of every cut set, each
    chunk at its own misalignment: whole arena, records and chunk indices
    against modify_read_cases.contiguous_definition mapped back through the
    tables."""
    keys = SETTINGS[setting]
    c = tuned(**keys)
    if "MAX_BLOCKS" in keys:
        assert c.get_tuning(abi.TUNE_MAX_BLOCKS) == keys["MAX_BLOCKS"]
    cb = dc.chunked_batch(profile, chain, cutter)
    d = tmr.Device(c, torch, tuple(np.array(x) for x in cb.tables), chain)
    edits, what = mc.nat_list(chain)
    for w in (0, what):
        want, recs, chunk = dc.chunked_expected(profile, chain, cutter, w)
        got, g_rec, g_chunk = d.run(edits, w)
        same(got, want, (setting, w))
        _same_rows(g_rec, recs, dc.N, (setting, w, "records"))
        assert np.array_equal(g_chunk, chunk), (setting, w, np.nonzero(g_chunk != chunk)[0][:8])
        assert (want != cb.tables[0]).any()


@chains
def test_single_edit_sweep_under_the_four_piece_window(torch, chain):
    """READ_PLAN = 1, default grid: k_parse_read_modify<4, chain, ModifyArgs |
    ModifyCsumArgs> on tests/test_modify_read.py's single-edit sweep (the
    csum_sweep_cases frames cut one header per chunk; every field x layer x op,
    what = L3 | L4 and, every third case, the plain rewrite): every field's
    first bit under the other window."""
    tmr.test_single_edit_sweep(tuned(READ_PLAN=1), torch, chain, BOTH)


# ---------------------------------------------------------------------------
# D. the chunked write calls over mblk chains in host memory
# ---------------------------------------------------------------------------
@contextlib.contextmanager
def mapped(ctx, *arrays):
    """Page-aligned copies of `arrays` in pageable host memory, page-locked
    and mapped by ingot_gpu_host_map -> (the copies, their device addresses);
    unmapped on the way out, also after a failure."""
    host = [_page_aligned(a) for a in arrays]
    done = []
    try:
        dev = []
        for h in host:
            dev.append(ctx.host_map(h))
            done.append(h)
        yield host, dev
    finally:
        import torch

        torch.cuda.synchronize()
        for h in done:
            ctx.host_unmap(h)


@host_sets
def test_parse_read_modify_csum_over_host_chains(torch, ctx, profile, chain, n):
    """The chunk pool and its three tables stay in mapped host memory, records
    and chunk indices land there too.  No tuning key: t.host_arena alone makes
    `four` true (read.hip:447), the default route into k_parse_read_modify<4,
    chain, ModifyCsumArgs> (and ModifyArgs for the plain call).  The host bytes
    afterwards are the contiguous definition mapped back through the tables."""
    lib = ingot_amd.load_library()
    cb = dc.host_chains(profile, chain, n)
    edits, what = mc.nat_list(chain)
    assert what == (7 if chain == TUN else BOTH)
    e = ingot_amd.edits_array(edits)
    with mapped(ctx, *cb.tables, np.zeros((n, 16), np.uint8), np.zeros(n, np.uint16)) as (h, d):
        for w in (what, 0):
            want, recs, chunk = dc.chunked_expected(profile, chain, "cut", w, n)
            h[0][:] = cb.tables[0]
            h[4][:] = 0xEE
            h[5][:] = 0xFFFF
            if w:
                rc = lib.ingot_gpu_parse_read_modify_csum(ctx._h, d[0], d[1], d[2], d[3], n,
                                                          int(chain), e.ctypes.data, len(e), w,
                                                          d[4], d[5], None)
            else:
                rc = lib.ingot_gpu_parse_read_modify(ctx._h, d[0], d[1], d[2], d[3], n,
                                                     int(chain), e.ctypes.data, len(e), d[4],
                                                     d[5], None)
            assert rc == 0
            torch.cuda.synchronize()
            same(h[0], want, (profile, w))
            _same_rows(h[4], recs, n, (profile, w, "records"))
            assert np.array_equal(h[5], chunk), (profile, w, "chunk")
            assert dc.rewritten_packets(cb, want).all()
        for k in (1, 2, 3):  # the tables are read only
            assert h[k].tobytes() == cb.tables[k].tobytes()


def _csum_rows(a):
    return np.ascontiguousarray(a).view(CSUM_DTYPE).reshape(-1)


@host_sets
def test_checksum_fill_and_verify_read_over_host_chains(torch, ctx, profile, chain, n):
    """ingot_gpu_checksum_verify_read, _fill_read and the verify again over
    the same chains in mapped host memory (k_csum_read has one form; what is
    new is where its loads and its two-byte stores go), with the records
    ingot_gpu_parse_read wrote into mapped host memory; rows and host bytes
    against tests/csum_read_model.py."""
    lib = ingot_amd.load_library()
    cb = dc.host_chains(profile, chain, n)
    tables = cb.tables
    with mapped(ctx, *tables, np.zeros((n, 16), np.uint8), np.zeros(n, np.uint16),
                np.zeros((n, 8), np.uint8)) as (h, d):
        h[4][:] = 0xEE
        assert lib.ingot_gpu_parse_read(ctx._h, d[0], d[1], d[2], d[3], n, int(chain), d[4], d[5],
                                        None) == 0
        torch.cuda.synchronize()
        _, recs, chunk = dc.chunked_expected(profile, chain, "cut", 0, n)
        _same_rows(h[4], recs, n, "parse_read records")
        assert np.array_equal(h[5], chunk)

        def call(fn, want_rows, want_arena, tag):
            h[6][:] = 0xEE
            assert fn(ctx._h, d[0], d[1], d[2], d[3], n, d[4], BOTH, d[6], None) == 0
            torch.cuda.synchronize()
            got = _csum_rows(h[6])
            bad = np.nonzero(got.view(np.uint64) != want_rows.view(np.uint64))[0]
            assert bad.size == 0, (tag, bad[:5], got[bad[:5]], want_rows[bad[:5]])
            same(h[0], want_arena, tag)

        before = csum_read_model.verify(tables, recs, BOTH)
        call(lib.ingot_gpu_checksum_verify_read, before, tables[0], "verify")
        filled = tables[0].copy()
        rows = csum_read_model.fill((filled,) + tuple(tables[1:]), recs, BOTH)
        assert (filled != tables[0]).any()
        call(lib.ingot_gpu_checksum_fill_read, rows, filled, "fill")
        after = csum_read_model.verify((filled,) + tuple(tables[1:]), recs, BOTH)
        call(lib.ingot_gpu_checksum_verify_read, after, filled, "verify after fill")
        assert (after["l4_state"] == 1).sum() > n // 2  # OK


@host_sets
def test_emit_packets_read_from_host_chains(torch, ctx, profile, chain, n):
    """ingot_gpu_emit_packets_read with the source chunks and their tables in
    mapped host memory, the destination arena, d_from / d_take and d_taken on
    the device (k_emit_read has one form and a fixed grid; what is new is the
    pull-up across PCIe).  The OPTE stack with its UDP sum, random d_from /
    d_take; whole destination and d_taken against tests/emit_read_model.py."""
    lib = ingot_amd.load_library()
    cb = dc.host_chains(profile, chain, n)
    tables = cb.tables
    rng = np.random.default_rng(41 + n)
    hdr, sets, sums = ecases.stack("opte", n, rng)
    frm, take = dc.emit_from_take(cb.lens, rng)
    t = emit_read_model.linearise(*tables, frm, take)[2]
    assert (t < cb.lens).sum() > n // 8 and (t == cb.lens).sum() > n // 8
    dst_off, size = ecases.pack(t, len(hdr), rng)
    want, lens_want = emit_read_model.apply(np.full(size, 0xA5, np.uint8), hdr, sets, sums,
                                            *tables, dst_off, frm, take)
    d_dst = _dev(torch, np.full(size, 0xA5, np.uint8))
    d_taken = _dev(torch, np.full(n, 0xA5A5, np.uint16))
    d_off, d_frm, d_take = _dev(torch, dst_off), _dev(torch, frm), _dev(torch, take)
    vals = [_dev(torch, s[4]) if len(s) > 4 else None for s in sets]
    sa = ingot_amd.emit_sets_array([(s[0], s[1], s[2], s[3], None if v is None else v.data_ptr())
                                    for s, v in zip(sets, vals)])
    cs = emit_sums_array(sums)
    hb = (ctypes.c_uint8 * len(hdr)).from_buffer_copy(hdr)
    with mapped(ctx, *tables) as (h, d):
        rc = lib.ingot_gpu_emit_packets_read(
            ctx._h, ctypes.addressof(hb), len(hdr), sa.ctypes.data_as(ctypes.c_void_p), len(sa),
            cs.ctypes.data_as(ctypes.c_void_p), len(cs), d[0], d[1], d[2], d[3],
            d_frm.data_ptr(), d_take.data_ptr(), n, d_dst.data_ptr(), d_off.data_ptr(),
            d_taken.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert h[0].tobytes() == tables[0].tobytes()  # the source is read only
    taken = _host(d_taken).view(np.uint16)
    assert np.array_equal(taken, lens_want), np.nonzero(taken != lens_want)[0][:8]
    same(_host(d_dst), want, profile)
