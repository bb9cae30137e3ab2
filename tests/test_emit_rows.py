"""ingot_gpu_emit_packets_rows on the device against its definition
(tests/emit_rows_model.py): in every test the whole destination arena, the
0xA5 bytes between the packets and at the guarded packets' places included,
is byte-equal to the model's.  Needs an MI355X: `pytest -m gpu`."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ingot_amd
from ingot_amd import EmitSource, EmitSum, Field, WideField
from ingot_amd.abi import emit_set_rows_array, emit_sums_array
from tests import emit_csum_cases as cases
from tests import emit_rows_cases as rc
from tests import emit_rows_model as model

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NONE = rc.ROW_NONE


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


def _same(got, want, tag=""):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, bad[:10], got[bad[:10]], want[bad[:10]])


def _check(ctx, torch, case, src, off, lens, dst_off, size, rows=None, n_rows=0, tag=""):
    """Device == model over the whole arena (both start as 0xA5) -> the arena."""
    want = np.full(size, 0xA5, np.uint8)
    model.apply(want, case.hdr, case.host_sets(), case.sums, src, off, lens, dst_off, rows, n_rows)
    d_dst = _dev(torch, np.full(size, 0xA5, np.uint8))
    backing = {k: _dev(torch, v) for k, v in case.backing.items()}
    ctx.emit_packets_rows(case.hdr, case.device_sets(backing), _dev(torch, src),
                          _dev(torch, np.asarray(off, np.uint64)),
                          _dev(torch, np.asarray(lens, np.uint16)), d_dst,
                          _dev(torch, np.asarray(dst_off, np.uint64)),
                          rows=None if rows is None else _dev(torch, rows), n_rows=n_rows,
                          sums=case.sums)
    got = d_dst.cpu().numpy()
    _same(got, want, tag)
    return got


def _check_both(ctx, torch, case, *args, **kw):
    """_check with the stack's sums (k_emit<true, true, true>) and with none
    named (k_emit<true, false, true>) -> both arenas."""
    sums = case.sums
    assert sums
    with_sums = _check(ctx, torch, case, *args, **kw)
    case.sums = None
    try:
        return with_sums, _check(ctx, torch, case, *args, **kw)
    finally:
        case.sums = sums


@pytest.mark.parametrize("form", rc.FORMS)
@pytest.mark.parametrize("name", rc.STACKS)
def test_stacks_and_tables(ctx, torch, name, form):
    """Every stack with every table form, with its sums and with none: 700
    packets (two group boundaries and a ragged tail) over 7 rows, so many
    packets share a row; guarded packets at lanes 0 and 63 of a subgroup and
    at the end."""
    rng = np.random.default_rng(11 + 10 * rc.STACKS.index(name) + rc.FORMS.index(form))
    n, n_rows = 700, 7
    rows = rc.row_indices(n, n_rows, rng, guarded=(64, 127, 320, 383, n - 1))
    case = rc.stack(name, form, n, n_rows, rng)
    src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng, rows, n_rows)
    assert 65535 in ln[rows < n_rows].tolist() and (n_rows - 1) in rows.tolist()
    assert {int(d) & 15 for d in dst_off[rows < n_rows]} == set(range(16))
    _check_both(ctx, torch, case, src, off, ln, dst_off, size, rows, n_rows, (name, form))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 700])
def test_batch_sizes(ctx, torch, n):
    """Batches that end inside, at and just past a wave and a 256-packet
    group, indexing a 65,536-row table, with the stack's sums and with none."""
    rng = np.random.default_rng(500 + n)
    n_rows = 65536
    rows = rc.row_indices(n, n_rows, rng)
    for name in ("opte", "v6_udp"):
        case = rc.stack(name, "struct32", n, n_rows, rng)
        src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng, rows, n_rows)
        _check_both(ctx, torch, case, src, off, ln, dst_off, size, rows, n_rows, (name, n))
        # and without a row array: BY_PACKET tables only
        if name == "v6_udp":
            src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng)
            _check_both(ctx, torch, case, src, off, ln, dst_off, size, tag=(name, n, "no rows"))


@pytest.mark.parametrize("n_rows", [1, 7, 65536])
def test_row_counts(ctx, torch, n_rows):
    """1, 7 and 65,536 rows, with the stack's sums and with none."""
    rng = np.random.default_rng(600 + n_rows % 97)
    n = 300
    rows = rc.row_indices(n, n_rows, rng, guarded=(5, 6))
    for name in ("opte", "geneve_v4"):
        case = rc.stack(name, "dense", n, n_rows, rng)
        src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng, rows, n_rows)
        _check_both(ctx, torch, case, src, off, ln, dst_off, size, rows, n_rows, (name, n_rows))


GUARDS = {
    "lanes_0_63": [0, 63, 64, 127, 192, 255, 256, 319],
    "subgroup": list(range(64, 128)),
    "group": list(range(256, 512)),
    "last": [699],
    "first_group_and_tail": list(range(0, 256)) + list(range(690, 700)),
    "all": list(range(700)),
}


@pytest.mark.parametrize("where", sorted(GUARDS))
def test_row_guard(ctx, torch, where):
    """Packets whose row is n_rows or INGOT_ROW_NONE are not emitted: their
    neighbours, packed against each other with no gap, keep their edge bytes,
    and descriptors that point outside the arenas are never used; with the
    stack's sums and with none."""
    rng = np.random.default_rng(len(where) + 700)
    n, n_rows = 700, 7
    rows = rc.row_indices(n, n_rows, rng, guarded=GUARDS[where])
    for name in ("opte", "geneve_v4"):
        case = rc.stack(name, "dense", n, n_rows, rng)
        src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng, rows, n_rows)
        both = _check_both(ctx, torch, case, src, off, ln, dst_off, size, rows, n_rows,
                           (name, where))
        if where == "all":
            assert all((got == 0xA5).all() for got in both)


@pytest.mark.parametrize("first", ["wide", "narrow"])
def test_order_of_overlapping_sets(ctx, torch, first):
    """A narrow set on bytes a wide set also writes: the later one wins, in
    both orders (a u16 inside the IPv6 source, a 24-bit field across the end
    of the Ethernet destination)."""
    rng = np.random.default_rng(81)
    n = 130
    base = rc.stack("v6_udp", "dense", n, 0, rng)
    v6s = base.sets[2]
    t16 = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
    t32 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    mac = rng.integers(0, 256, (n, 6), dtype=np.uint8)
    backing = dict(base.backing, t16=t16.view(np.uint8), t32=t32.view(np.uint8),
                   mac=mac.reshape(-1))
    narrow = [(30, Field.UDP_SOURCE, EmitSource.U16, 3, rc.View("t16", 0, 2, 2, n, np.uint16)),
              (0, Field.GENEVE_VNI, EmitSource.U32, 0, rc.View("t32", 0, 4, 4, n, np.uint32))]
    wide = [v6s, (0, WideField.ETH_DESTINATION, EmitSource.BYTES, 0,
                  rc.View("mac", 0, 6, 6, n))]
    sets = base.sets[:2] + (wide + narrow if first == "wide" else narrow + wide) + base.sets[3:]
    case = rc.Case(base.hdr, sets, base.sums, backing)
    src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng)
    got = _check(ctx, torch, case, src, off, ln, dst_off, size, tag=first)
    # the two orders do differ where the sets overlap (packet 0, header bytes 30..31)
    d = int(dst_off[0])
    want16 = (int(t16[0]) + 3) & 0xFFFF
    in_block = (int(got[d + 30]) << 8 | int(got[d + 31])) == want16
    assert in_block == (first == "wide")


def test_without_tables_is_emit_packets_csum(ctx, torch):
    """No BYTES set, no BY_ROW set, no row array: byte for byte what
    emit_packets(..., sums=...) writes on the device, for every stack."""
    rng = np.random.default_rng(33)
    n = 700
    ln = rc.lengths(n, rng)
    src, off = cases.random_source(ln, rng)
    d_src, d_off, d_ln = _dev(torch, src), _dev(torch, off), _dev(torch, ln)
    for name in cases.STACKS:
        hdr, sets, sums = cases.stack(name, n, rng)
        dst_off, size = cases.pack(ln, len(hdr), rng)
        d_doff = _dev(torch, dst_off)
        dev_sets = [s if len(s) == 4 else (*s[:4], _dev(torch, s[4])) for s in sets]
        for sm in (sums, None):
            a = _dev(torch, np.full(size, 0xA5, np.uint8))
            b = _dev(torch, np.full(size, 0xA5, np.uint8))
            ctx.emit_packets(hdr, dev_sets, d_src, d_off, d_ln, a, d_doff, sums=sm)
            ctx.emit_packets_rows(hdr, dev_sets, d_src, d_off, d_ln, b, d_doff, sums=sm)
            _same(b.cpu().numpy(), a.cpu().numpy(), (name, sm))


def test_argument_errors(ctx, torch):
    """Every EINVAL of the header's list, in its order, each reached with the
    earlier checks satisfied; the model names the same step; nothing is
    launched (the arena keeps its fill)."""
    lib = ingot_amd.load_library()
    hdr, _, _ = cases.stack("opte", 4, np.random.default_rng(0))
    n = 4
    src = _dev(torch, np.arange(256, dtype=np.uint8))
    off = _dev(torch, np.array([0, 16, 32, 48], np.uint64))
    ln = _dev(torch, np.array([10, 11, 12, 13], np.uint16))
    doff = _dev(torch, np.array([0, 100, 200, 300], np.uint64))
    dst = _dev(torch, np.full(512, 0xA5, np.uint8))
    row = _dev(torch, np.zeros(n, np.uint32))
    tab = _dev(torch, np.zeros(256, np.uint8))
    T = tab.data_ptr()
    ptrs = [src.data_ptr(), off.data_ptr(), ln.data_ptr(), dst.data_ptr(), doff.data_ptr()]
    PKT, ROW = 0, 1
    U16, U32, VALUE, LENGTH, BYTES = (EmitSource.U16, EmitSource.U32, EmitSource.VALUE,
                                      EmitSource.LENGTH, EmitSource.BYTES)

    def call(sets, sums=(), h=hdr, h_len=None, have_row=True, n_sets=None, null_sets=False,
             ctx_ok=True, n_pkts=n, null_ptr=None):
        sa = emit_set_rows_array(sets) if not hasattr(sets, "dtype") else sets
        cs = emit_sums_array(sums)
        hb = (ctypes.c_uint8 * max(len(h), 1)).from_buffer_copy(h or b"\0")
        p = list(ptrs)
        if null_ptr is not None:
            p[null_ptr] = None
        h_len = len(h) if h_len is None else h_len
        n_sets = len(sa) if n_sets is None else n_sets
        rcode = lib.ingot_gpu_emit_packets_rows(
            ctx._h if ctx_ok else None, ctypes.addressof(hb), h_len,
            None if null_sets else sa.ctypes.data_as(ctypes.c_void_p), n_sets,
            cs.ctypes.data_as(ctypes.c_void_p), len(cs), row.data_ptr() if have_row else None, 1,
            p[0], p[1], p[2], n_pkts, p[3], p[4], None)
        step = None
        try:
            model.check_args(ctx_ok, h, h_len, None if null_sets else sa, n_sets, sums, have_row,
                             n_pkts, null_ptr is None)
        except ValueError as err:
            step = str(err).split(":")[0]
        return rcode, step

    def einval(step, sets, **kw):
        rcode, got = call(sets, **kw)
        assert rcode == -1 and got == step, (step, got, rcode, sets, kw)

    ok = (14, WideField.V6_DESTINATION, BYTES, 0, ROW, 0, T)
    einval("1", [ok], ctx_ok=False)
    einval("2", [ok], h=bytes(300))
    einval("2", [ok] * 9)
    einval("2", [ok], null_sets=True)
    # 3, in list order: a good set first, then the faulty one; each fault
    # also carries the next one, which must not be what is reported
    einval("3.1", [ok, (14, 48, 9, 0, PKT, 0, 0)])                        # field (and source)
    einval("3.1", [ok, (14, 68, BYTES, 0, PKT, 0, T)])                    # past the wide fields
    bad = emit_set_rows_array([ok, (14, Field.UDP_SOURCE, 5, 0, PKT, 0, T)])
    bad[1]["_pad"][0] = 1
    einval("3.1", bad)                                                    # source (and pad)
    bad = emit_set_rows_array([ok, (54, Field.UDP_SOURCE, U16, 0, 2, 0, T)])
    bad[1]["_pad"][2] = 1
    einval("3.1", bad)                                                    # pad (and by)
    einval("3.1", [ok, (54, Field.UDP_SOURCE, BYTES, 0, 2, 0, T)])        # by (and BYTES narrow)
    einval("3.1", [ok, (54, Field.UDP_SOURCE, BYTES, 0, PKT, 0, T)])      # BYTES on a narrow field
    einval("3.1", [ok, (14, WideField.V6_SOURCE, VALUE, 0, ROW, 0, 0)])   # VALUE on a wide field
    einval("3.1", [ok, (14, WideField.V6_SOURCE, U32, 0, PKT, 0, T)])
    for extra in ((ROW, 0, 0), (PKT, 4, 0), (PKT, 0, T)):                 # LENGTH / VALUE extras
        einval("3.1", [ok, (54, Field.UDP_LENGTH, LENGTH, 0, *extra)])
        einval("3.1", [ok, (54, Field.UDP_SOURCE, VALUE, 7, *extra)])
    einval("3.1", [ok, (54, Field.UDP_SOURCE, U16, 0, PKT, 0, 0)])        # NULL table
    einval("3.1", [ok, (14, WideField.V6_SOURCE, BYTES, 0, PKT, 0, 0)])
    einval("3.1", [ok, (14, WideField.V6_SOURCE, BYTES, 1, PKT, 8, T)])   # add (and pitch)
    einval("3.1", [ok, (14, WideField.V6_SOURCE, BYTES, 0, PKT, 15, T)])  # pitch < width
    einval("3.1", [ok, (0, WideField.ETH_SOURCE, BYTES, 0, PKT, 5, T)])
    einval("3.1", [ok, (54, Field.UDP_SOURCE, U16, 0, PKT, 1, T)])
    einval("3.1", [ok, (62, Field.GENEVE_VNI, U32, 0, PKT, 3, T + 2)])    # (and misaligned)
    einval("3.1", [ok, (54, Field.UDP_SOURCE, U16, 0, PKT, 0, T + 1)])    # misaligned table
    einval("3.1", [ok, (54, Field.UDP_SOURCE, U16, 0, PKT, 3, T)])        # misaligned pitch
    einval("3.1", [ok, (62, Field.GENEVE_VNI, U32, 0, PKT, 0, T + 2)])
    einval("3.1", [ok, (62, Field.GENEVE_VNI, U32, 0, PKT, 6, T)])
    einval("3.0", [ok], have_row=False)                                   # BY_ROW without d_row
    einval("3.0", [(len(hdr) - 39, WideField.V6_DESTINATION, BYTES, 0, ROW, 0, T)],
           have_row=False)                                                # (and outside hdr)
    einval("3.1", [ok, (len(hdr) - 39, WideField.V6_DESTINATION, BYTES, 0, PKT, 0, T)])
    einval("3.1", [ok, (len(hdr) - 11, WideField.ETH_SOURCE, BYTES, 0, PKT, 0, T)])
    einval("3.1", [ok, (len(hdr) - 1, Field.UDP_SOURCE, VALUE, 1, PKT, 0, 0)])
    # a wide field may end exactly at the block's end
    assert call([ok, (len(hdr) - 12, WideField.ETH_SOURCE, BYTES, 0, PKT, 0, T)],
                n_pkts=0) == (0, None)
    # 4: the sums' checks, after the sets'
    einval("4", [ok], sums=[(EmitSum.UDP, 55, 14)])
    einval("4", [ok], sums=[(EmitSum.UDP, 54, 14), (EmitSum.UDP, 54, 14)])
    einval("4", [ok, (14, Field.V6_VERSION, VALUE, 6, PKT, 0, 0)], sums=[(EmitSum.UDP, 54, 14)])
    einval("3.1", [ok, (14, 48, VALUE, 0, PKT, 0, 0)], sums=[(EmitSum.UDP, 55, 14)])
    # 5: n == 0 succeeds with NULL device pointers, after the checks above
    for k in range(5):
        assert call([ok], sums=[(EmitSum.UDP, 54, 14)], n_pkts=0, null_ptr=k) == (0, None)
    einval("4", [ok], sums=[(EmitSum.UDP, 55, 14)], n_pkts=0)
    # 6: NULL device pointers
    for k in range(5):
        einval("6", [ok], sums=[(EmitSum.UDP, 54, 14)], null_ptr=k)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()
    # and the same arguments without the faults are accepted
    assert call([ok], sums=[(EmitSum.UDP, 54, 14)]) == (0, None)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() != 0xA5).any()


def test_python_table_validation(ctx, torch):
    """Context.emit_packets_rows refuses a table of the wrong dtype, shape,
    stride or row count on the host."""
    rng = np.random.default_rng(4)
    n = 8
    case = rc.stack("opte", "dense", n, 4, rng)
    src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng)
    args = (_dev(torch, src), _dev(torch, off), _dev(torch, ln),
            _dev(torch, np.full(size, 0xA5, np.uint8)), _dev(torch, dst_off))
    rows = _dev(torch, np.zeros(n, np.uint32))
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
    v6 = (14, WideField.V6_DESTINATION, EmitSource.BYTES, 0)
    for bad in (u8(n, 6), u8(n * 16), u8(n, 32)[:, ::2], u8(n - 1, 16),
                torch.zeros((n, 16), dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError):
            ctx.emit_packets_rows(case.hdr, [(*v6, bad)], *args)
    with pytest.raises(ValueError):  # ('row', tensor) without rows
        ctx.emit_packets_rows(case.hdr, [(*v6, ("row", u8(4, 16)))], *args)
    with pytest.raises(ValueError):  # a BY_ROW table shorter than n_rows
        ctx.emit_packets_rows(case.hdr, [(*v6, ("row", u8(3, 16)))], *args, rows=rows, n_rows=4)
    with pytest.raises(ValueError):  # a u32 table for a U16 set
        ctx.emit_packets_rows(case.hdr, [(54, Field.UDP_SOURCE, EmitSource.U16, 0,
                                          torch.zeros(n, dtype=torch.int32, device="cuda"))],
                              *args)
    torch.cuda.synchronize()
    assert (args[3].cpu().numpy() == 0xA5).all()


def test_cpp_encap_table_example_on_device(torch):
    """tests/cpp/example_encap_table.cpp, a fresh process: flow bins -> one
    emit_packets_rows from a 64-row endpoint table with the UDP sum; the result
    parses as GENEVE_OVER_V6, every sum verifies, uncounted frames are not
    emitted."""
    exe = ROOT / "tests" / "cpp" / "build" / "example_encap_table"
    if not exe.exists():
        from ingot_amd.build import build_cpp_tests

        build_cpp_tests()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("0 not parsed, 0 inner not OK, 0 outer not OK, 0 wrong fields, 0 stray bytes: OK"
            in r.stdout)
