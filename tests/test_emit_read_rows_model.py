"""tests/emit_read_rows_model.py (the definition of
ingot_gpu_emit_packets_read_rows) against the two definitions it joins: with no
table it is emit_read_model over the same chunks, on single-chunk packets it is
emit_rows_model over the same frames, and a guarded packet leaves nothing
behind.  No GPU."""
import numpy as np
import pytest

from tests import emit_csum_cases as cases
from tests import emit_read_model, emit_rows_model
from tests import emit_read_rows_cases as rrc
from tests import emit_read_rows_model as model
from tests import emit_rows_cases as rc


@pytest.mark.parametrize("name", ["opte", "geneve_v4", "v6_udp"])
def test_without_tables_is_the_chunked_model(name):
    """No table, no BY_ROW, no rows: emit_read_model's arena and lengths, over
    two-chunk packets with from / take."""
    rng = np.random.default_rng(1)
    ln = np.asarray(cases.EDGE_LENGTHS, np.uint16)
    n = len(ln)
    src, off = cases.random_source(ln, rng)
    tables = rrc.two_chunks(src, off, ln, rng)
    hdr, sets, sums = cases.stack(name, n, rng)
    for frm, take in ((None, None), (rng.integers(0, 20, n).astype(np.uint16),
                                     rng.integers(0, 5000, n).astype(np.uint16))):
        t = emit_read_model.linearise(*tables, frm, take)[2]
        dst_off, size = cases.pack(t, len(hdr), rng)
        want, wl = emit_read_model.apply(np.full(size, 0xA5, np.uint8), hdr, sets, sums, *tables,
                                         dst_off, frm, take)
        got, gl = model.apply(np.full(size, 0xA5, np.uint8), hdr, sets, sums, *tables, dst_off,
                              frm=frm, take=take)
        assert (gl == wl).all() and (gl == t).all()
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", rc.STACKS)
def test_one_chunk_is_the_rows_model(name):
    """One chunk per packet: emit_rows_model's arena, tables, rows and guard included."""
    rng = np.random.default_rng(2)
    n, n_rows = 40, 5
    rows = rc.row_indices(n, n_rows, rng, guarded=(0, 17, n - 1))
    case = rc.stack(name, "struct32", n, n_rows, rng)
    src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng, rows, n_rows, poison=False)
    tables = (src, off, ln, np.arange(n + 1, dtype=np.uint32))
    want = emit_rows_model.apply(np.full(size, 0xA5, np.uint8), case.hdr, case.host_sets(),
                                 case.sums, src, off, ln, dst_off, rows, n_rows)
    got, taken = model.apply(np.full(size, 0xA5, np.uint8), case.hdr, case.host_sets(), case.sums,
                             *tables, dst_off, rows, n_rows)
    live = rows < n_rows
    assert (taken[live] == ln[live]).all() and (taken[~live] == 0).all()
    assert got.tobytes() == want.tobytes()


def test_guarded_packet_leaves_the_arena():
    """A guarded packet, its chunks unreadable and its destination outside the
    arena: nothing is written, its neighbours are whole, taken is 0."""
    rng = np.random.default_rng(3)
    n, n_rows = 9, 4
    rows = rc.row_indices(n, n_rows, rng, guarded=(4,))
    case = rc.stack("opte", "dense", n, n_rows, rng)
    b = rrc.batch(n, len(case.hdr), rng, rows, n_rows, pieces=2)
    assert b.seg_off[2 * 4] == 1 << 60 and b.dst_off[4] >= b.size
    got, taken = model.apply(np.full(b.size, 0xA5, np.uint8), case.hdr, case.host_sets(),
                             case.sums, *b.tables, b.dst_off, rows, n_rows, b.frm, b.take)
    assert taken[4] == 0 and (taken[rows < n_rows] > 0).all()
    # packets 3 and 5 are packed against each other: 3's last byte, then 5's first
    end3 = int(b.dst_off[3]) + len(case.hdr) + int(taken[3])
    assert end3 == int(b.dst_off[5])
    # all guarded: the arena keeps its fill
    none = np.full(n, rc.ROW_NONE, np.uint32)
    got, taken = model.apply(np.full(b.size, 0xA5, np.uint8), case.hdr, case.host_sets(),
                             case.sums, *b.tables, b.dst_off, none, n_rows, b.frm, b.take)
    assert (got == 0xA5).all() and (taken == 0).all()


def test_check_args_names_the_step():
    from ingot_amd.abi import EmitSource, EmitSum, WideField, emit_set_rows_array

    hdr, _, _ = cases.stack("opte", 1, np.random.default_rng(0))
    ok = emit_set_rows_array([(14, WideField.V6_DESTINATION, EmitSource.BYTES, 0, 1, 0, 0x1000)])
    udp = [(EmitSum.UDP, 54, 14)]

    def step(*a, **kw):
        try:
            model.check_args(*a, **kw)
        except ValueError as err:
            return str(err).split(":")[0]
        return None

    assert step(False, hdr, 300, None, 9, udp, False, 4, False, False) == "1"
    assert step(True, hdr, 300, ok, 1, udp, True, 4, False, False) == "2.2"
    assert step(True, hdr, len(hdr), ok, 1, udp, False, 4, False, False) == "2.3.0"
    assert step(True, hdr, len(hdr), ok, 1, [(EmitSum.UDP, 55, 14)], True, 0) == "2.4"
    assert step(True, hdr, len(hdr), ok, 1, udp, True, 0, False, False) is None
    assert step(True, hdr, len(hdr), ok, 1, udp, True, 4, False, False) == "4"
    assert step(True, hdr, len(hdr), ok, 1, udp, True, 4, True, False) == "5"
    assert step(True, hdr, len(hdr), ok, 1, udp, True, 4) is None
