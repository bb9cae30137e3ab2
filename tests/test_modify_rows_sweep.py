"""ingot_gpu_parse_modify_rows on the device over the deterministic cases of
tests/modify_rows_sweep_cases.py, against the definition
(tests/modify_rows_model.py) bit for bit: the whole arena, the 0xA5 bytes
between and after the frames included, and the records.

  A  every narrow field x layer x op x `what` as a VALUE edit (also byte-equal
     to parse_modify / parse_modify_csum on the device), by packet and by row;
     seeded random lists against parse_modify_csum on both layouts
  B  every wide field at every layer; addresses and MACs across the end of the
     staged window, set once, twice, and restored; 64 pieces
  C  deltas of 0 mod 0xffff, addresses solved so that a sum lands on 0 / 0xffff
     and their neighbours, packets whose sum must not move
  D  table addresses and pitches, row offsets past 2^32, the row guard

tests/test_modify_rows_sweep_model.py holds every expected value to a second
way of computing it on the CPU.  Needs an MI355X: `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

import ingot_amd
from ingot_amd import Chain, EditOp, Field
from ingot_amd.abi import EditSource
from tests import csum_sweep_cases as sc
from tests import modify_rows_cases as cases
from tests import modify_rows_sweep_cases as rc
from tests.test_modify_csum import on_gpu as uniform_on_gpu
from tests.test_modify_csum import same
from tests.test_modify_csum_sweep import _whats
from tests.test_modify_rows import check, on_gpu

pytestmark = pytest.mark.gpu
TUN = sc.TUN
SET = EditOp.SET
chains = pytest.mark.parametrize("chain", sc.CHAINS, ids=lambda c: c.name)


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return ingot_amd.Context(0)


def device(torch, c, g, what, edits=None):
    b = g.b
    return on_gpu(torch, c, b.arena, b.off, b.lens, g.chain, g.edits if edits is None else edits,
                  rows=g.rows, n_rows=g.n_rows, what=what, stride=b.stride, n=b.n)


def run(torch, c, g):
    """Group `g` under each of its `what` values against the definition.
    -> the definition's arenas."""
    outs, recs = rc.expected(g)
    for what, want in zip(g.whats, outs):
        got, g_rec = device(torch, c, g, what)
        assert g_rec.tobytes() == recs.tobytes(), (g.name, what)
        same(got, want, (g.name, what))
    return outs


def pitch_zero(torch, c, g, what):
    """The raw call with pitch 0, the ABI's name for a dense table, in every
    edit whose table is dense (the Python mirror always passes the row stride).
    -> (arena after the call, records, edits passed with pitch 0)."""
    b = g.b
    d_arena = torch.from_numpy(np.array(b.arena)).cuda()
    d_off = torch.from_numpy(b.off.view(np.int64)).cuda()
    d_len = torch.from_numpy(b.lens.view(np.int16)).cuda()
    d_rows = None if g.rows is None else torch.from_numpy(g.rows.view(np.int32)).cuda()
    recs = torch.empty((b.n, 16), dtype=torch.uint8, device="cuda")
    e, keep = c._edit_rows(cases.device_edits(torch, g.edits), b.n, d_rows, g.n_rows)
    dense = 0
    for k in range(len(e)):
        width = {int(EditSource.U16): 2, int(EditSource.U32): 4,
                 int(EditSource.BYTES): rc.WIDTH.get(int(e[k]["field"]))}.get(int(e[k]["source"]))
        if width is not None and int(e[k]["pitch"]) == width:
            e[k]["pitch"] = 0
            dense += 1
    rv = c._lib.ingot_gpu_parse_modify_rows(
        c._h, d_arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), 0, b.n, int(g.chain),
        e.ctypes.data_as(ctypes.c_void_p), len(e), None if d_rows is None else d_rows.data_ptr(),
        g.n_rows, what, recs.data_ptr(), None)
    assert rv == 0
    torch.cuda.synchronize()
    del keep
    return d_arena.cpu().numpy(), recs.cpu().numpy(), dense


# ---------------------------------------------------------------------------
# A. Narrow fields through this kernel
# ---------------------------------------------------------------------------
FORMS = ("value", "by packet", "by row")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("field", list(Field), ids=lambda f: f.name)
@chains
def test_single_edit_sweep(torch, ctx, chain, field, form):
    """Every case of the existing single-edit sweep under every `what`, in
    three forms (one test each, so that none outlasts the existing sweep's).  VALUE:
    the definition of the uniform rewrite, and byte-equal to parse_modify /
    parse_modify_csum on the device.  BY_PACKET (the sweep value XOR a pattern
    per packet, in the source that does not match the field's width) and
    BY_ROW (5 rows, every seventh packet guarded): tests/modify_rows_model."""
    b = sc.batch(chain, "indexed")
    whats = _whats(chain, "indexed", field)
    moved = 0
    for e in sc.sweep(chain, field):
        if form != "value":
            g = rc.sweep_forms(chain, b, e, whats)[FORMS.index(form) - 1]
            assert g.name.endswith(form)
            moved += int(run(torch, ctx, g)[0].tobytes() != b.arena.tobytes())
            continue
        for what in whats:
            want, _, recs, ch = sc.define(b, chain, [e], what)
            t = sc.tag(chain, "indexed", e, what)
            got, g_rec = on_gpu(torch, ctx, b.arena, b.off, b.lens, chain, [e], what=what)
            assert g_rec.tobytes() == recs.tobytes(), t
            same(got, want, t)
            u_got, u_rec = uniform_on_gpu(torch, ctx, b.arena, b.off, b.lens, chain, [e], what)
            assert u_rec.tobytes() == g_rec.tobytes() and u_got.tobytes() == got.tobytes(), t
            moved += int(ch.size > 0)
    assert (moved > 0) == (field in sc.fields_of(chain)), moved


@chains
def test_random_lists(torch, ctx, chain):
    """200 seeded lists of up to 16 VALUE edits on both layouts: this call,
    parse_modify_csum (slots: the ring kernel, where this call runs k_parse)
    and the definition agree on every byte."""
    lists = sc.random_lists(chain)
    assert len(lists) == 200 and max(len(e) for e in lists) == 16
    touched = 0
    for layout in ("indexed", "strided"):
        b = sc.batch(chain, layout)
        for k, edits in enumerate(lists):
            what = sc.WHATS[chain][k % len(sc.WHATS[chain])]
            want, _, recs, ch = sc.define(b, chain, edits, what)
            t = sc.tag(chain, layout, edits, what)
            got, g_rec = on_gpu(torch, ctx, b.arena, b.off, b.lens, chain, edits, what=what,
                                stride=b.stride, n=b.n)
            assert g_rec.tobytes() == recs.tobytes(), t
            same(got, want, t)
            u_got, u_rec = uniform_on_gpu(torch, ctx, b.arena, b.off, b.lens, chain, edits, what,
                                          stride=b.stride, n=b.n)
            assert u_rec.tobytes() == g_rec.tobytes() and u_got.tobytes() == got.tobytes(), t
            touched += int(ch.size > 0)
    assert touched >= 300, touched


# ---------------------------------------------------------------------------
# B. Wide fields
# ---------------------------------------------------------------------------
@chains
def test_wide_fields_at_every_layer(torch, ctx, chain):
    moved = 0
    for g in rc.wide_layer_groups(chain):
        outs = run(torch, ctx, g)
        changed = any(o.tobytes() != g.b.arena.tobytes() for o in outs)
        assert changed == rc.holds(chain, g.edits[0][0], g.edits[0][1]), g.name
        moved += int(changed)
    assert moved > 0


@chains
def test_across_the_window(torch, ctx, chain):
    """Every frame at each of the 16 places in its 16-B block: the window ends
    inside the addresses (tests/test_modify_rows_sweep_model.py shows where),
    so a 4-byte piece, and the second SET's read of the first SET's bytes,
    take bytes from both sides of that end."""
    for mis in range(16):
        b = sc.batch_at(chain, mis)
        assert (b.off % 16 == mis).all()
        for g, unchanged in rc.window_groups(chain, b):
            outs = run(torch, ctx, g)
            assert not unchanged or all(o.tobytes() == b.arena.tobytes() for o in outs), g.name
    # set and restored over both representations of a zero sum
    b = rc.edge_batch(chain)[0]
    for g, unchanged in rc.window_groups(chain, b, restore_only=True):
        for what in g.whats:
            got, _ = device(torch, ctx, g, what)
            assert got.tobytes() == b.arena.tobytes(), (g.name, what)


@chains
def test_64_pieces(torch, ctx, chain):
    for g in rc.pieces64_groups(chain):
        assert len(g.edits) == 16
        outs = run(torch, ctx, g)
        assert outs[0].tobytes() != g.b.arena.tobytes()


# ---------------------------------------------------------------------------
# C. Checksum value edges of the new covered ranges
# ---------------------------------------------------------------------------
@chains
def test_delta_of_zero_keeps_the_field(torch, ctx, chain):
    for way, g in rc.delta_zero_groups(chain):
        run(torch, ctx, g)
        got, _ = device(torch, ctx, g, g.whats[0])
        fields = rc.sum_fields(g.b, chain)
        for at in fields[fields >= 0]:
            assert got[at:at + 2].tobytes() == g.b.arena[at:at + 2].tobytes(), (g.name, at)
        assert way != "same" or got.tobytes() == g.b.arena.tobytes()


@chains
def test_solved_addresses_land_on_the_edges(torch, ctx, chain):
    for g, which, hit in rc.solved_groups(chain):
        run(torch, ctx, g)
        got, _ = device(torch, ctx, g, g.whats[0])
        fields = rc.sum_fields(g.b, chain)
        kind = rc.kinds(g.b, chain)
        for target, frames in hit.items():
            _, udp_bytes, other_bytes = rc.TARGETS[target]
            for i in frames:
                at = int(fields[i, which])
                is_udp = which == 2 or kind[i][1] == "udp"
                assert got[at:at + 2].tobytes() == (udp_bytes if is_udp else other_bytes), \
                    (g.name, target, i)


@chains
def test_sums_that_must_not_move(torch, ctx, chain):
    b, zeroed = rc.still_batch(chain)
    for g in rc.still_groups(chain):
        run(torch, ctx, g)
        got, _ = device(torch, ctx, g, rc.full(chain))
        fields = rc.sum_fields(b, chain)
        for i in zeroed:
            at = int(fields[i, 2 if chain == TUN else 1])
            assert got[at:at + 2].tobytes() == b"\x00\x00", i


# ---------------------------------------------------------------------------
# D. Tables and rows
# ---------------------------------------------------------------------------
def test_byte_tables(torch, ctx):
    """MAC and IPv6 rows at device addresses 0..3 mod 4, rows exactly their
    width apart (also as pitch 0), one byte more, 32 and 4096."""
    zero = 0
    for g in rc.byte_table_groups():
        outs = run(torch, ctx, g)
        if "pitch exact" in g.name:
            got, _, dense = pitch_zero(torch, ctx, g, g.whats[0])
            assert dense == 4
            same(got, outs[0], g.name + " as pitch 0")
            zero += 1
    assert zero == 8


def test_integer_tables(torch, ctx):
    groups = list(rc.int_table_groups())
    for g in groups:
        outs = run(torch, ctx, g)
        if "pitch 2 / 4" in g.name:
            got, _, dense = pitch_zero(torch, ctx, g, g.whats[0])
            assert dense == 6
            same(got, outs[0], g.name + " as pitch 0")
    assert len(groups) == 3


@pytest.mark.parametrize("kind", ["u32", "v6"])
def test_row_offsets_past_4_gib(torch, ctx, kind):
    """BY_PACKET rows 1 MiB apart: from packet 4,096 on, r * pitch does not fit
    32 bits.  The table is an uninitialised 4,099 MiB allocation in which only
    the rows are written; every row lies inside it."""
    n, pitch = 4099, 1 << 20
    b = rc.batch_n(Chain.GenericUlp, n, 9 if kind == "v6" else 0)
    u32, v6 = rc.far_rows(n)
    big = torch.empty(n * pitch, dtype=torch.uint8, device="cuda")
    try:
        if kind == "u32":
            view = torch.as_strided(big.view(torch.int32), (n, 1), (pitch // 4, 1))
            view.copy_(torch.from_numpy(u32.view(np.int32).reshape(n, 1)).cuda())
            field, dense = Field.V4_SOURCE, u32
        else:
            view = torch.as_strided(big, (n, 16), (pitch, 1))
            view.copy_(torch.from_numpy(v6).cuda())
            field, dense = rc.V6S, v6
        assert (n - 1) * pitch + 16 <= big.numel() and (n - 1) * pitch >= 1 << 32
        g = rc.Group(f"rows 1 MiB apart, {kind}", b, Chain.GenericUlp, [(1, field, SET, dense)],
                     None, 0, (3,))
        (want,), recs = rc.expected(g)
        got, g_rec = device(torch, ctx, g, 3, edits=[(1, field, SET, view)])
        assert g_rec.tobytes() == recs.tobytes()
        same(got, want, g.name)
        # packets 4,096..4,098 hold such a header: they took their own rows
        assert set(sc.changed_frames(b, want).tolist()) >= {4096, 4097, 4098}
    finally:
        del big
        torch.cuda.empty_cache()


def test_the_row_guard(torch, ctx):
    for g, guarded in rc.guard_groups():
        b = g.b
        got, recs = check(torch, ctx, b.arena, b.off, b.lens, g.chain, g.edits, rows=g.rows,
                          n_rows=g.n_rows, what=g.whats[0])
        assert (recs["status"] == 0).sum() >= 0.9 * b.n  # the records are written
        for i in guarded:
            o, ln = int(b.starts[i]), int(b.lengths[i])
            assert got[o:o + ln].tobytes() == b.arena[o:o + ln].tobytes(), (g.name, i)
        if g.n_rows == 0:
            assert got.tobytes() == b.arena.tobytes(), g.name
