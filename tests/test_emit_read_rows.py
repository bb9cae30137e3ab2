"""ingot_gpu_emit_packets_read_rows on the device against its definition
(tests/emit_read_rows_model.py): in every test the whole destination arena, the
0xA5 bytes between the packets and at the guarded packets' places included,
is byte-equal to the model's, and d_taken (prefilled with 0xA5A5) equals the
model's lengths.  Needs an MI355X: `pytest -m gpu`."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import Chain, EmitSource, EmitSum, Field, GenProfile, WideField
from ingot_amd import emit as E
from ingot_amd.abi import emit_set_rows_array, emit_sums_array
from ingot_amd.hostgen import gen_frames_host
from tests import csum_read_cases as chunks
from tests import emit_csum_cases as cases
from tests import emit_read_rows_cases as rrc
from tests import emit_read_rows_model as model
from tests import emit_rows_cases as rc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NP = 256  # packets per workgroup of k_emit_read, 64 per prologue wave


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
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
              np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()


def _opt(torch, a, dtype):
    return None if a is None else _dev(torch, np.asarray(a, dtype))


def _same(got, want, tag=""):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, bad[:10], got[bad[:10]], want[bad[:10]])


def _run(ctx, torch, case, tables, dst_off, size, rows=None, n_rows=0, frm=None, take=None,
         d_tables=None):
    """-> (destination arena started as 0xA5, d_taken started as 0xA5A5), numpy."""
    n = len(tables[3]) - 1
    d_dst = _dev(torch, np.full(size, 0xA5, np.uint8))
    d_taken = _dev(torch, np.full(n, 0xA5A5, np.uint16))
    backing = {k: _dev(torch, v) for k, v in case.backing.items()}
    d = d_tables or [_dev(torch, x) for x in tables]
    ctx.emit_packets_read_rows(case.hdr, case.device_sets(backing), *d, d_dst,
                               _dev(torch, np.asarray(dst_off, np.uint64)),
                               rows=_opt(torch, rows, np.uint32), n_rows=n_rows,
                               frm=_opt(torch, frm, np.uint16), take=_opt(torch, take, np.uint16),
                               taken=d_taken, sums=case.sums)
    return d_dst.cpu().numpy(), d_taken.cpu().numpy().view(np.uint16)


def _check(ctx, torch, case, tables, dst_off, size, rows=None, n_rows=0, frm=None, take=None,
           tag="", want=None, d_tables=None):
    """Device == model over the whole arena and d_taken -> (arena, taken, want)."""
    if want is None:
        want = model.apply(np.full(size, 0xA5, np.uint8), case.hdr, case.host_sets(), case.sums,
                           *tables, dst_off, rows, n_rows, frm, take)
    got, taken = _run(ctx, torch, case, tables, dst_off, size, rows, n_rows, frm, take, d_tables)
    _same(taken, want[1], (tag, "taken"))
    _same(got, want[0], tag)
    return got, taken, want


def _check_both(ctx, torch, case, b, rows=None, n_rows=0, tag=""):
    """_check with the stack's sums (k_emit_read<true, true>) and with none
    named (k_emit_read<false, true>) -> both arenas."""
    sums = case.sums
    assert sums
    args = (b.tables, b.dst_off, b.size, rows, n_rows, b.frm, b.take)
    d = [_dev(torch, x) for x in b.tables]
    with_sums = _check(ctx, torch, case, *args, tag=(tag, "sums"), d_tables=d)[0]
    case.sums = None
    try:
        return with_sums, _check(ctx, torch, case, *args, tag=(tag, "no sums"), d_tables=d)[0]
    finally:
        case.sums = sums


@pytest.mark.parametrize("form", rc.FORMS)
@pytest.mark.parametrize("name", rc.STACKS)
def test_stacks_and_tables(ctx, torch, name, form):
    """Every stack with every table form over 700 two-chunk packets (two group
    boundaries and a ragged tail) and 7 rows, with its sums and with none;
    guarded packets at lanes 0 and 63 of a subgroup and at the first and last
    packet of a group."""
    rng = np.random.default_rng(211 + 10 * rc.STACKS.index(name) + rc.FORMS.index(form))
    n, n_rows = 700, 7
    rows = rc.row_indices(n, n_rows, rng, guarded=(64, 127, 256, 511, 320, 383, n - 1))
    case = rc.stack(name, form, n, n_rows, rng)
    b = rrc.batch(n, len(case.hdr), rng, rows, n_rows)
    assert 65535 in b.t.tolist() and (n_rows - 1) in rows.tolist()
    assert {int(d) & 15 for d in b.dst_off[rows < n_rows]} == set(range(16))
    _check_both(ctx, torch, case, b, rows, n_rows, (name, form))


def test_alignment(ctx, torch):
    """4,096 two-chunk packets with a 37-byte payload cut at 5 and at 6: every
    destination x chunk-0 x chunk-1 misalignment, the IPv6 destination BY_ROW
    and the UDP sum.  (The bytes do not depend on the cut: one model run.)"""
    n, n_rows = 4096, 64
    rng = np.random.default_rng(310)
    hdr, _, sums = cases.stack("opte", 1, rng)
    table = rng.integers(0, 256, (n_rows, 16), dtype=np.uint8)
    sets = [(14, Field.V6_PAYLOAD_LEN, EmitSource.LENGTH, -40),
            (54, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
            (14, WideField.V6_DESTINATION, EmitSource.BYTES, 0,
             ("row", rc.View("v6d", 0, 16, 16, n_rows)))]
    case = rc.Case(hdr, sets, sums, {"v6d": table.reshape(-1)})
    rows = rc.row_indices(n, n_rows, rng)
    p = np.arange(n)
    stride = (len(hdr) + 37 + 15 + 16) // 16 * 16
    dst_off = (p * stride + p % 16).astype(np.uint64)
    size = n * stride + 64
    mis = np.stack([(p // 16) % 16, p // 256], axis=1).reshape(-1).tolist()
    pays = rng.integers(0, 256, (n, 37), dtype=np.uint8)
    want = None
    for c in (5, 6):
        packets = [chunks.cut_at(pays[i].tobytes(), [c]) for i in range(n)]
        tables = chunks.place(packets, misalign=mis)
        assert (tables[1][0:2 * n:2] % 16 == (p // 16) % 16).all()
        assert (tables[1][1:2 * n:2] % 16 == p // 256).all()
        want = _check(ctx, torch, case, tables, dst_off, size, rows, n_rows, tag=c, want=want)[2]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes(ctx, torch, n):
    """Batches that end inside, at and just past a prologue wave and a group,
    indexing a 65,536-row table, with the stack's sums and with none."""
    rng = np.random.default_rng(1500 + n)
    n_rows = 65536
    rows = rc.row_indices(n, n_rows, rng)
    case = rc.stack("opte", "struct32", n, n_rows, rng)
    ln = rng.integers(0, 400, n).astype(np.uint16)
    b = rrc.batch(n, len(case.hdr), rng, rows, n_rows, lengths=ln)
    _check_both(ctx, torch, case, b, rows, n_rows, n)


GUARDS = {
    "single": (700, [300]),
    "wave": (700, list(range(64, 128))),
    "group": (700, list(range(256, 512))),
    "all": (300, list(range(300))),
}


@pytest.mark.parametrize("where", sorted(GUARDS))
def test_row_guard(ctx, torch, where):
    """Packets whose row is n_rows or INGOT_ROW_NONE are not emitted.  Their
    chunks have seg_off 2^60 and seg_len 65,535, their dst_off points outside
    the arena, their from / take are arbitrary; their neighbours are packed
    against each other with no gap at an odd destination address and keep
    their edge bytes; d_taken of a guarded packet is 0.  With the UDP sum (the
    step-5 path) and without."""
    rng = np.random.default_rng(len(where) + 1700)
    n, guarded = GUARDS[where]
    n_rows = 7
    rows = rc.row_indices(n, n_rows, rng, guarded=guarded)
    assert set(rows[guarded].tolist()) <= {n_rows, rc.ROW_NONE}
    case = rc.stack("opte", "dense", n, n_rows, rng)
    assert case.sums == [(EmitSum.UDP, 54, 14)]
    ln = rng.integers(0, 300, n).astype(np.uint16)
    b = rrc.batch(n, len(case.hdr), rng, rows, n_rows, lengths=ln)
    live = rows < n_rows
    if live.any() and where != "all":
        after = guarded[-1] + 1
        before = guarded[0] - 1
        if int(b.dst_off[after]) % 2 == 0:  # the seam at an odd address
            b.dst_off[live] += np.uint64(1)
            b.size += 1
        assert int(b.dst_off[after]) % 2 == 1
        assert int(b.dst_off[before]) + len(case.hdr) + int(ln[before]) == int(b.dst_off[after])
    assert (b.seg_off[:2 * n][np.repeat(~live, 2)] == rrc.POISON_OFF).all()
    assert (b.dst_off[~live] >= b.size).all()
    both = _check_both(ctx, torch, case, b, rows, n_rows, where)
    if where == "all":
        assert all((got == 0xA5).all() for got in both)


@pytest.mark.parametrize("pieces", [5, 9])
def test_many_chunks(ctx, torch, pieces):
    """Packets of 5 and of 9 pieces (past the 4-piece LDS table), the second
    chunk empty and the third one byte; BY_PACKET and BY_ROW sets and the UDP
    sum; guarded packets among them."""
    rng = np.random.default_rng(1900 + pieces)
    n, n_rows = 300, 5
    rows = rc.row_indices(n, n_rows, rng, guarded=(0, 63, 64, 130, 131, 255, 256, n - 1))
    case = rc.stack("opte", "odd", n, n_rows, rng)
    ln = rng.integers(0, 600, n).astype(np.uint16)
    ln[:12] = np.arange(12)  # fewer bytes than pieces
    b = rrc.batch(n, len(case.hdr), rng, rows, n_rows, pieces=pieces, lengths=ln, edge=True)
    sl = b.tables[2][:n * pieces].reshape(n, pieces)  # place() adds one trailing entry
    live = rows < n_rows
    assert (sl[live][:, 1] == 0).all() and (sl[live][:, 2] <= 1).all() and (sl[live][:, 2] == 1).any()
    _check_both(ctx, torch, case, b, rows, n_rows, pieces)


def test_decapsulation(ctx, torch):
    """Chunked GeneveOverV6Tunnel frames; d_from = the inner L3 offset of the
    records; hdr = a 14-byte Ethernet header with both MACs BY_ROW and the
    inner ethertype per packet; no sums.  Then hdr_len == 0, n_sets == 0 with
    d_row given: the pull-up that skips guarded packets."""
    n, n_rows = 1000, 16
    rng = np.random.default_rng(2014)
    arena, off, lens = gen_frames_host(GenProfile["GENEVE"], n, seed=77, slack=64)
    recs = oracle.parse_batch(arena, off, lens, Chain.GeneveOverV6Tunnel)
    ok = recs["status"] == 0
    assert ok.sum() > n // 2
    frames = chunks.frames_of(arena, off, lens)
    packets = [chunks.cut(f, recs[i], rng) for i, f in enumerate(frames)]
    tables = chunks.place(packets, misalign=rrc.MISALIGN, gap=1)
    rows = rc.row_indices(n, n_rows, rng, guarded=(0, 63, 64, 500, 501, n - 1))
    rows[~ok] = rc.ROW_NONE  # a frame that is no tunnel packet has no flow
    live = rows < n_rows
    frm = np.where(ok, recs["l3_off"], lens).astype(np.uint16)
    inner = np.where(live, lens.astype(np.int64) - frm, 0).astype(np.uint16)
    macs = rng.integers(0, 256, n_rows * 12, dtype=np.uint8)
    etype = recs["ethertype"].astype(np.uint16)
    sets = [(0, WideField.ETH_DESTINATION, EmitSource.BYTES, 0,
             ("row", rc.View("macs", 0, 6, 12, n_rows))),
            (0, WideField.ETH_SOURCE, EmitSource.BYTES, 0,
             ("row", rc.View("macs", 6, 6, 12, n_rows))),
            (0, Field.ETH_ETHERTYPE, EmitSource.U16, 0, rc.View("etype", 0, 2, 2, n, np.uint16))]
    case = rc.Case(E.ethernet(bytes(6), bytes(6), 0), sets, None,
                   {"macs": macs, "etype": etype.view(np.uint8)})
    dst_off, size = rrc.pack_live(14 + inner.astype(np.int64), live, rng)
    got, taken, _ = _check(ctx, torch, case, tables, dst_off, size, rows, n_rows, frm=frm,
                           tag="ethernet")
    assert (taken == inner).all()
    for i in np.nonzero(live)[0][:100]:
        o, r = int(dst_off[i]), int(rows[i])
        assert got[o:o + 12].tobytes() == macs[12 * r:12 * r + 12].tobytes()
        assert got[o + 14:o + 14 + int(taken[i])].tobytes() == frames[i][int(frm[i]):]
    # what came out parses as the oracle parses the inner packets behind an Ethernet header
    tl = (taken.astype(np.int64) + 14).astype(np.uint16)
    out = oracle.parse_batch(got, dst_off[live], tl[live], Chain.GenericUlp)
    assert (out["status"] == 0).all()
    # the guarded pull-up: no header block, no sets
    bare = rc.Case(b"", [], None, {})
    dst_off, size = rrc.pack_live(inner.astype(np.int64), live, rng)
    got, taken, _ = _check(ctx, torch, bare, tables, dst_off, size, rows, n_rows, frm=frm,
                           tag="pull-up")
    assert (taken == inner).all()


def test_device_against_device(ctx, torch):
    """With no tables and d_row NULL the arena and d_taken are
    Context.emit_packets_read's, for every stack, with sums and without; on
    single-chunk packets the arena is Context.emit_packets_rows' with the same
    tables and rows."""
    rng = np.random.default_rng(2033)
    n = 700
    ln = rc.lengths(n, rng)
    src, off = cases.random_source(ln, rng)
    tables = rrc.two_chunks(src, off, ln, rng)
    d = [_dev(torch, x) for x in tables]
    for name in cases.STACKS:
        hdr, sets, sums = cases.stack(name, n, rng)
        dst_off, size = cases.pack(ln, len(hdr), rng)
        d_doff = _dev(torch, dst_off)
        dev_sets = [s if len(s) == 4 else (*s[:4], _dev(torch, s[4])) for s in sets]
        for sm in (sums, None):
            a = _dev(torch, np.full(size, 0xA5, np.uint8))
            b = _dev(torch, np.full(size, 0xA5, np.uint8))
            ta = _dev(torch, np.full(n, 0xA5A5, np.uint16))
            tb = _dev(torch, np.full(n, 0xA5A5, np.uint16))
            ctx.emit_packets_read(hdr, dev_sets, *d, a, d_doff, taken=ta, sums=sm or ())
            ctx.emit_packets_read_rows(hdr, dev_sets, *d, b, d_doff, taken=tb, sums=sm)
            _same(b.cpu().numpy(), a.cpu().numpy(), (name, sm))
            _same(tb.cpu().numpy(), ta.cpu().numpy(), (name, sm, "taken"))
            assert (ta.cpu().numpy().view(np.uint16) == ln).all()
    # single-chunk packets against emit_packets_rows
    n_rows = 7
    rows = rc.row_indices(n, n_rows, rng, guarded=(0, 63, 256, 511, n - 1))
    for name in rc.STACKS:
        case = rc.stack(name, "struct32", n, n_rows, rng)
        src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng, rows, n_rows, poison=False)
        backing = {k: _dev(torch, v) for k, v in case.backing.items()}
        dev = [_dev(torch, x) for x in (src, off, ln, dst_off)]
        d_rows = _dev(torch, rows)
        a = _dev(torch, np.full(size, 0xA5, np.uint8))
        b = _dev(torch, np.full(size, 0xA5, np.uint8))
        ctx.emit_packets_rows(case.hdr, case.device_sets(backing), dev[0], dev[1], dev[2], a,
                              dev[3], rows=d_rows, n_rows=n_rows, sums=case.sums)
        ctx.emit_packets_read_rows(case.hdr, case.device_sets(backing), dev[0], dev[1], dev[2],
                                   _dev(torch, np.arange(n + 1, dtype=np.uint32)), b, dev[3],
                                   rows=d_rows, n_rows=n_rows, sums=case.sums)
        _same(b.cpu().numpy(), a.cpu().numpy(), (name, "rows"))


def test_argument_errors(ctx, torch):
    """Every EINVAL of the header's list, in its order, each reached with the
    earlier checks satisfied and a later fault present; the model names the
    same step; nothing is launched (the arena keeps its fill)."""
    lib = ingot_amd.load_library()
    hdr, _, _ = cases.stack("opte", 4, np.random.default_rng(0))
    n = 4
    arena, so, sl, ps = chunks.place([[bytes(20), bytes(9)]] * n, misalign=(3, 8))
    src, so, sl, ps = (_dev(torch, x) for x in (arena, so, sl, ps))
    doff = _dev(torch, np.array([0, 120, 240, 360], np.uint64))
    dst = _dev(torch, np.full(512, 0xA5, np.uint8))
    row = _dev(torch, np.zeros(n, np.uint32))
    tab = _dev(torch, np.zeros(256, np.uint8))
    T = tab.data_ptr()
    good = dict(src=src.data_ptr(), so=so.data_ptr(), sl=sl.data_ptr(), ps=ps.data_ptr(),
                dst=dst.data_ptr(), doff=doff.data_ptr())
    PKT, ROW = 0, 1
    U16, VALUE, BYTES = EmitSource.U16, EmitSource.VALUE, EmitSource.BYTES

    def call(sets, sums=(), h=hdr, have_row=True, n_sets=None, null_sets=False, ctx_ok=True,
             n_pkts=n, null=()):
        sa = emit_set_rows_array(sets) if not hasattr(sets, "dtype") else sets
        cs = emit_sums_array(sums)
        hb = (ctypes.c_uint8 * max(len(h), 1)).from_buffer_copy(h or b"\0")
        p = {k: (None if k in null else v) for k, v in good.items()}
        n_sets = len(sa) if n_sets is None else n_sets
        rcode = lib.ingot_gpu_emit_packets_read_rows(
            ctx._h if ctx_ok else None, ctypes.addressof(hb), len(h),
            None if null_sets else sa.ctypes.data_as(ctypes.c_void_p), n_sets,
            cs.ctypes.data_as(ctypes.c_void_p), len(cs), row.data_ptr() if have_row else None, 1,
            p["src"], p["so"], p["sl"], p["ps"], None, None, n_pkts, p["dst"], p["doff"], None,
            None)
        step = None
        try:
            model.check_args(ctx_ok, h, len(h), None if null_sets else sa, n_sets, sums, have_row,
                             n_pkts, not ({"dst", "doff"} & set(null)),
                             not ({"src", "so", "sl", "ps"} & set(null)))
        except ValueError as err:
            step = str(err).split(":")[0]
        return rcode, step

    def einval(step, sets, **kw):
        rcode, got = call(sets, **kw)
        assert rcode == -1 and got == step, (step, got, rcode, sets, kw)

    ok = (14, WideField.V6_DESTINATION, BYTES, 0, ROW, 0, T)
    bad_set = (14, 48, 9, 0, PKT, 0, 0)
    udp, odd = [(EmitSum.UDP, 54, 14)], [(EmitSum.UDP, 55, 14)]
    everything = tuple(good)
    # 1
    einval("1", [bad_set], sums=odd, ctx_ok=False, null=everything)
    # 2: emit_args, then the sets in list order, then the sums
    einval("2.2", [bad_set], sums=odd, h=bytes(300), null=everything)
    einval("2.2", [bad_set] * 9, sums=odd, null=everything)
    einval("2.2", [ok], null_sets=True, sums=odd, null=everything)
    einval("2.3.1", [ok, bad_set], sums=odd, null=everything)
    einval("2.3.1", [ok, (54, Field.UDP_SOURCE, BYTES, 0, PKT, 0, T)], sums=odd)
    einval("2.3.1", [ok, (54, Field.UDP_SOURCE, U16, 0, PKT, 0, T + 1)], sums=odd)
    einval("2.3.1", [ok, (14, WideField.V6_SOURCE, BYTES, 0, PKT, 15, T)], sums=odd)
    einval("2.3.0", [ok], have_row=False, sums=odd, null=everything)
    einval("2.3.1", [ok, (len(hdr) - 39, WideField.V6_DESTINATION, BYTES, 0, PKT, 0, T)],
           sums=odd)
    einval("2.4", [ok], sums=odd, null=everything)
    einval("2.4", [ok], sums=udp + udp, null=everything)
    einval("2.4", [ok, (14, Field.V6_VERSION, VALUE, 6, PKT, 0, 0)], sums=udp, n_pkts=0)
    # 3: n == 0 succeeds whatever the device pointers are, after the checks above
    assert call([ok], sums=udp, n_pkts=0, null=everything) == (0, None)
    for name in good:
        assert call([ok], sums=udp, n_pkts=0, null=(name,)) == (0, None)
    # 4, then 5
    einval("4", [ok], sums=udp, null=("dst", "src"))
    einval("4", [ok], sums=udp, null=("doff", "ps"))
    for name in ("src", "so", "sl", "ps"):
        einval("5", [ok], sums=udp, null=(name,))
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()
    # and the same arguments without the faults are accepted
    assert call([ok], sums=udp) == (0, None)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() != 0xA5).any()


def test_python_table_validation(ctx, torch):
    """Context.emit_packets_read_rows refuses a table of the wrong dtype,
    shape, stride or row count on the host (emit_packets_rows' helper)."""
    rng = np.random.default_rng(4)
    n = 8
    case = rc.stack("opte", "dense", n, 4, rng)
    b = rrc.batch(n, len(case.hdr), rng, lengths=np.full(n, 40, np.uint16))
    dst = _dev(torch, np.full(b.size, 0xA5, np.uint8))
    args = (*[_dev(torch, x) for x in b.tables], dst, _dev(torch, b.dst_off))
    rows = _dev(torch, np.zeros(n, np.uint32))
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
    v6 = (14, WideField.V6_DESTINATION, EmitSource.BYTES, 0)
    for bad in (u8(n, 6), u8(n * 16), u8(n, 32)[:, ::2], u8(n - 1, 16),
                torch.zeros((n, 16), dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError):
            ctx.emit_packets_read_rows(case.hdr, [(*v6, bad)], *args)
    with pytest.raises(ValueError):  # ('row', tensor) without rows
        ctx.emit_packets_read_rows(case.hdr, [(*v6, ("row", u8(4, 16)))], *args)
    with pytest.raises(ValueError):  # a BY_ROW table shorter than n_rows
        ctx.emit_packets_read_rows(case.hdr, [(*v6, ("row", u8(3, 16)))], *args, rows=rows,
                                   n_rows=4)
    with pytest.raises(ValueError):  # a u32 table for a U16 set
        ctx.emit_packets_read_rows(case.hdr, [(54, Field.UDP_SOURCE, EmitSource.U16, 0,
                                               torch.zeros(n, dtype=torch.int32, device="cuda"))],
                                   *args)
    with pytest.raises(ValueError):  # rows of the wrong length
        ctx.emit_packets_read_rows(case.hdr, [], *args, rows=rows[:n - 1], n_rows=4)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()


def test_cpp_encap_chain_example_on_device(torch):
    """tests/cpp/example_encap_chain.cpp, a fresh process: flow bins over
    two-chunk packets -> one emit_packets_read_rows from a 64-row endpoint
    table with the UDP sum; the result parses as GENEVE_OVER_V6, every sum
    verifies, uncounted frames are not emitted."""
    exe = ROOT / "tests" / "cpp" / "build" / "example_encap_chain"
    if not exe.exists():
        from ingot_amd.build import build_cpp_tests

        build_cpp_tests()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("0 not parsed, 0 inner not OK, 0 outer not OK, 0 wrong fields, 0 stray bytes: OK"
            in r.stdout)
