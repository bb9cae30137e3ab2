"""ingot_gpu_emit_packets_rows on the device over the deterministic cases of
tests/emit_rows_sweep_cases.py, against the definition
(tests/emit_rows_model.py) bit for bit: the destination starts as 0xA5 and the
whole arena, the bytes between the packets and at the guarded packets' places
included, equals the model's.

  A  every narrow field x {VALUE (also byte-equal to emit_packets on the
     device), by packet, by row, add, LENGTH}, on blocks prefilled 0x00 / 0xff
  B  every wide field at every place of a 254-B block from tables of every
     alignment; 32 pieces; 12- and 14-B blocks; set, overwritten, restored
  C  table words solved so that a sum lands on 0 / 0xffff and their
     neighbours; all-0xff / all-0x00 operands under the longest datagram
  D  rows past 2^32, pitch 0, the guard alone, n_rows = 0, one survivor

A names no sum: k_emit<true, false, true>; B and D run both rows kernels, C
the one with sums.  tests/test_emit_rows_sweep_model.py holds every expected
value to a second way of computing it on the CPU.  Needs an MI355X:
`pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

import ingot_amd
from ingot_amd import Field, WideField
from ingot_amd.abi import emit_set_rows_array, emit_sums_array
from tests import emit_rows_cases as rc
from tests import emit_rows_sweep_cases as sw
from tests.test_emit_rows import _check, _dev, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return ingot_amd.Context(0)


def run(ctx, torch, job, case=None):
    """Device == model over the whole arena -> the arena."""
    b = job.b
    got = _check(ctx, torch, case or job.case, b.src, b.off, b.lens, b.dst_off, b.size, b.rows,
                 b.n_rows, job.tag)
    sw.held(job, got)
    return got


# ---------------------------------------------------------------------------
# A. Narrow fields
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", sw.FORMS)
@pytest.mark.parametrize("field", list(Field), ids=lambda f: f.name)
def test_narrow_sweep(ctx, torch, field, form):
    moved = 0
    for job in sw.narrow_jobs(field, form):
        got = run(ctx, torch, job)
        moved += int((got[int(job.b.dst_off[0]):][:sw.BLOCK_LEN] != job.case.hdr[0]).any())
        if form != "value":
            continue
        # the sets kernel, the same set: byte-equal
        b, c = job.b, job.case
        d_dst = _dev(torch, np.full(b.size, 0xA5, np.uint8))
        ctx.emit_packets(c.hdr, c.sets, _dev(torch, b.src), _dev(torch, b.off),
                         _dev(torch, b.lens), d_dst, _dev(torch, b.dst_off))
        _same(d_dst.cpu().numpy(), got, job.tag + " as emit_packets")
    assert moved > 0


# ---------------------------------------------------------------------------
# B. Wide fields and piece limits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("wf", list(WideField), ids=lambda f: f.name)
def test_wide_at_every_place(ctx, torch, wf):
    for job in sw.wide_at_jobs(wf):
        run(ctx, torch, job)


def test_32_pieces(ctx, torch):
    for job in sw.pieces_jobs():
        run(ctx, torch, job)


def test_smallest_blocks(ctx, torch):
    for job in sw.small_block_jobs():
        run(ctx, torch, job)


def test_set_overwritten_restored(ctx, torch):
    arenas = [run(ctx, torch, job) for job, _ in sw.restore_jobs()]
    assert arenas[0].tobytes() == arenas[2].tobytes() != arenas[1].tobytes()


# ---------------------------------------------------------------------------
# C. Sums at their edges, operands from tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rot", range(3))
@pytest.mark.parametrize("name,what,key,by_row", sw.SOLVED, ids=lambda v: str(v))
def test_solved_table_words(ctx, torch, name, what, key, by_row, rot):
    job = sw.solved_job(name, what, key, by_row, rot)
    assert len(job.checks) == (7 if what == "udp" else 6)
    sw.held(job, sw.expected(job))  # the model's field is what the case was built for
    run(ctx, torch, job)


@pytest.mark.parametrize("name", rc.STACKS)
def test_extreme_operands(ctx, torch, name):
    for job in sw.extreme_jobs(name):
        run(ctx, torch, job)


# ---------------------------------------------------------------------------
# D. Tables, rows, guard
# ---------------------------------------------------------------------------
class _FarCase(rc.Case):
    """job.case with the device's set 2 taking its rows from `far`."""

    def __init__(self, case, far):
        super().__init__(case.hdr, case.sets, case.sums, {})
        self._host, self._far = case, far

    def host_sets(self):
        return self._host.host_sets()

    def device_sets(self, dev_backing):
        return [*self.sets[:2], (*self.sets[2][:4], ("row", self._far))]


@pytest.mark.parametrize("kind", ["u32", "v6"])
def test_row_offsets_past_4_gib(ctx, torch, kind):
    """BY_ROW rows 1 MiB apart: from row 4,096 on, r * pitch does not fit 32
    bits.  The table is an uninitialised 4,099 MiB allocation in which only
    the rows are written; every row lies inside it."""
    job = sw.far_job(kind)
    n, pitch = sw.FAR_ROWS, sw.FAR_PITCH
    dense = np.array(job.case.sets[2][4][1].numpy(job.case.backing))
    try:
        big = torch.empty(n * pitch, dtype=torch.uint8, device="cuda")
    except RuntimeError as err:  # (torch.OutOfMemoryError is one)
        pytest.skip(f"the {n}-MiB table was refused: {str(err)[:80]}")
    try:
        if kind == "u32":
            view = torch.as_strided(big.view(torch.int32), (n, 1), (pitch // 4, 1))
            view.copy_(torch.from_numpy(dense.view(np.int32).reshape(n, 1)).cuda())
        else:
            view = torch.as_strided(big, (n, 16), (pitch, 1))
            view.copy_(torch.from_numpy(np.ascontiguousarray(dense)).cuda())
        assert (n - 1) * pitch + 16 <= big.numel() and (n - 1) * pitch >= 1 << 32
        assert {4096, 4097, 4098} <= set(job.b.rows[sw.live(job.b)].tolist())
        run(ctx, torch, job, _FarCase(job.case, view))
    finally:
        del big
        torch.cuda.empty_cache()


def test_pitch_zero(ctx, torch):
    """The raw call with pitch 0, the ABI's name for a dense table, in every
    set that has a table (the Python mirror always passes the row stride)."""
    job = sw.pitch_zero_job()
    c, b = job.case, job.b
    dev = {k: _dev(torch, v) for k, v in c.backing.items()}
    sets = []
    for s in c.sets:
        if len(s) == 4:
            sets.append((*s, 0, 0, 0))
            continue
        by, view = (1, s[4][1]) if isinstance(s[4], tuple) else (0, s[4])
        assert view.pitch == view.width
        sets.append((*s[:4], by, 0, dev[view.name].data_ptr() + view.first))
    assert sum(1 for s in sets if s[6]) == 5
    sa, cs = emit_set_rows_array(sets), emit_sums_array(c.sums)
    hb = (ctypes.c_uint8 * len(c.hdr)).from_buffer_copy(c.hdr)
    args = [_dev(torch, a) for a in (b.rows, b.src, b.off, b.lens)]
    d_dst, d_doff = _dev(torch, np.full(b.size, 0xA5, np.uint8)), _dev(torch, b.dst_off)
    rv = ctx._lib.ingot_gpu_emit_packets_rows(
        ctx._h, ctypes.addressof(hb), len(c.hdr), sa.ctypes.data_as(ctypes.c_void_p), len(sa),
        cs.ctypes.data_as(ctypes.c_void_p), len(cs), args[0].data_ptr(), b.n_rows,
        args[1].data_ptr(), args[2].data_ptr(), args[3].data_ptr(), len(b.lens), d_dst.data_ptr(),
        d_doff.data_ptr(), None)
    assert rv == 0
    torch.cuda.synchronize()
    _same(d_dst.cpu().numpy(), sw.expected(job), job.tag)


def test_the_row_guard(ctx, torch):
    """A row array and no BY_ROW set; n_rows = 0; n_rows = 1 with one
    survivor in each prologue subgroup; each with its sums and with none."""
    for job, emits in sw.guard_jobs():
        sums = job.case.sums
        for sm in (sums, None):
            job.case.sums = sm
            try:
                got = run(ctx, torch, job)
            finally:
                job.case.sums = sums
            assert (got != 0xA5).any() == emits, job.tag
