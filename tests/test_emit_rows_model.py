"""tests/emit_rows_model.py, the definition of ingot_gpu_emit_packets_rows,
pinned on the CPU: against the plain emit's definitions where the two calls
must agree, against an independent byte-wise receiver where they cannot, and
the order of its argument errors."""
import numpy as np
import pytest

import oracle
from ingot_amd import EmitSource, EmitSum, Field, WideField
from ingot_amd.abi import emit_set_rows_array
from tests import csum_sweep_cases as sc
from tests import emit_csum_cases as cases
from tests import emit_csum_model
from tests import emit_rows_cases as rc
from tests import emit_rows_model as model


def _batch(n, hdr, rng):
    ln = rc.lengths(n, rng)
    src, off = cases.random_source(ln, rng)
    dst_off, size = cases.pack(ln, len(hdr), rng)
    return src, off, ln, dst_off, size


@pytest.mark.parametrize("name", cases.STACKS)
def test_without_tables_is_the_plain_model(name):
    """No wide and no BY_ROW set: oracle.emit_batch + emit_csum_model.apply."""
    rng = np.random.default_rng(1)
    n = 40
    hdr, sets, sums = cases.stack(name, n, rng)
    src, off, ln, dst_off, size = _batch(n, hdr, rng)
    want = np.full(size, 0xA5, np.uint8)
    oracle.emit_batch(hdr, sets, src, off, ln, want, dst_off)
    emit_csum_model.apply(want, hdr, sums, dst_off, ln, sets)
    got = np.full(size, 0xA5, np.uint8)
    model.apply(got, hdr, sets, sums, src, off, ln, dst_off)
    assert (got == want).all()
    # the same sets by row through an identity row array
    by_row = [s if len(s) == 4 else (*s[:4], ("row", s[4])) for s in sets]
    got = np.full(size, 0xA5, np.uint8)
    model.apply(got, hdr, by_row, sums, src, off, ln, dst_off, np.arange(n, dtype=np.uint32), n)
    assert (got == want).all()


@pytest.mark.parametrize("name", rc.STACKS)
def test_one_shared_row_is_a_patched_header(name):
    """All packets take row 3: the plain model over a header block the host
    patched with that row's bytes and values."""
    rng = np.random.default_rng(2)
    n, n_rows, r = 30, 5, 3
    case = rc.stack(name, "struct32", n, n_rows, rng)
    sets = [s if len(s) == 4 or isinstance(s[4], tuple) else (*s[:4], ("row", s[4]))
            for s in case.host_sets()]  # v6_udp's by-packet tables: taken by row here
    src, off, ln, dst_off, size = _batch(n, case.hdr, rng)
    rows = np.full(n, r, np.uint32)
    got = np.full(size, 0xA5, np.uint8)
    model.apply(got, case.hdr, sets, case.sums, src, off, ln, dst_off, rows, n_rows)
    hdr, plain = bytearray(case.hdr), []
    for at, field, source, add, *t in sets:
        if source == EmitSource.BYTES:
            p = at + model.WIDE_AT[WideField(field)]
            hdr[p:p + t[0][1].shape[1]] = bytes(t[0][1][r])
        elif t:
            plain.append((at, field, EmitSource.VALUE, int(t[0][1][r]) + add))
        else:
            plain.append((at, field, source, add))
    want = np.full(size, 0xA5, np.uint8)
    oracle.emit_batch(bytes(hdr), plain, src, off, ln, want, dst_off)
    for o, length in zip(dst_off.astype(np.int64), ln.astype(np.int64)):
        emit_csum_model.one(want[o:o + len(hdr) + length], case.hdr, case.sums)
    assert (got == want).all()
    assert bytes(hdr) != bytes(case.hdr)


def test_guarded_packets_keep_the_fill():
    rng = np.random.default_rng(3)
    n, n_rows = 20, 4
    rows = rc.row_indices(n, n_rows, rng, guarded=(0, 7, 8, 19))
    case = rc.stack("opte", "dense", n, n_rows, rng)
    src, off, ln, dst_off, size = rc.batch(n, len(case.hdr), rng, rows, n_rows)
    got = np.full(size, 0xA5, np.uint8)
    model.apply(got, case.hdr, case.host_sets(), case.sums, src, off, ln, dst_off, rows, n_rows)
    covered = np.zeros(size, bool)
    for i in np.nonzero(rows < n_rows)[0]:
        covered[int(dst_off[i]):int(dst_off[i]) + len(case.hdr) + int(ln[i])] = True
    assert (got[~covered] == 0xA5).all() and covered.sum() > 0
    assert list(np.nonzero(~model.emitted(n, rows, n_rows))[0]) == [0, 7, 8, 19]
    # a guarded packet's neighbours sit against each other
    assert int(dst_off[6]) + len(case.hdr) + int(ln[6]) == int(dst_off[9])


@pytest.mark.parametrize("form", rc.FORMS)
def test_receiver_accepts_per_row_addresses(form):
    """IPv6 source and destination per packet: an independent byte-wise
    RFC 1071 receiver accepts every emitted packet's UDP sum."""
    rng = np.random.default_rng(4)
    n = 60
    case = rc.stack("v6_udp", form, n, 0, rng)
    src, off, ln, dst_off, size = _batch(n, case.hdr, rng)
    got = np.full(size, 0xA5, np.uint8)
    model.apply(got, case.hdr, case.host_sets(), case.sums, src, off, ln, dst_off)
    seen = set()
    for i in range(n):
        o, tot = int(dst_off[i]), len(case.hdr) + int(ln[i])
        pkt = got[o:o + tot]
        seen.add(bytes(pkt[22:54]))
        if tot - 54 <= 65535:
            assert sc.bytewise_receiver_ok(pkt, case.hdr, case.sums), i
    assert len(seen) == n  # the pseudo-header did vary


@pytest.mark.parametrize("first", ["wide", "narrow"])
def test_later_set_wins(first):
    hdr, _, _ = cases.stack("v6_udp", 1, np.random.default_rng(0))
    row = np.arange(0x40, 0x50, dtype=np.uint8).reshape(1, 16)
    wide = (14, WideField.V6_SOURCE, EmitSource.BYTES, 0, row)
    narrow = (30, Field.UDP_SOURCE, EmitSource.VALUE, 0xBEEF)
    sets = [wide, narrow] if first == "wide" else [narrow, wide]
    pkt = model.one(hdr, sets, (), np.zeros(3, np.uint8), 0, 0)
    want = bytearray(row.tobytes())
    if first == "wide":
        want[8:10] = b"\xbe\xef"
    assert bytes(pkt[22:38]) == bytes(want)


def test_argument_error_order():
    """Each fault is reported as its own step, and with two faults in one call
    the earlier step of the header's list is the one reported."""
    hdr, _, _ = cases.stack("opte", 1, np.random.default_rng(0))
    H, T = len(hdr), 0x1000
    B, U16, U32, VALUE, LENGTH = (EmitSource.BYTES, EmitSource.U16, EmitSource.U32,
                                  EmitSource.VALUE, EmitSource.LENGTH)
    ok = (14, WideField.V6_DESTINATION, B, 0, 1, 0, T)

    def step(sets, sums=(), ctx_ok=True, h=hdr, have_row=True, n=4, ptrs=True, n_sets=None):
        sa = None if sets is None else emit_set_rows_array(sets)
        count = (0 if sa is None else len(sa)) if n_sets is None else n_sets
        try:
            model.check_args(ctx_ok, h, len(h), sa, count, sums, have_row, n, ptrs)
        except ValueError as err:
            return str(err)
        return None

    assert step([ok]) is None
    assert step([ok], ctx_ok=False, h=bytes(300)).startswith("1:")
    assert step([(14, 99, 9, 0, 0, 0, 0)], h=bytes(300)).startswith("2:")
    assert step(None, n_sets=1).startswith("2:")
    assert step([ok] * 9).startswith("2:")
    # one set, two faults: the list's order decides
    ladder = [
        ((14, 99, 9, 0, 0, 0, 0), "unknown field"),
        ((14, Field.UDP_SOURCE, 9, 0, 7, 0, 0), "unknown source"),
        ((54, Field.UDP_SOURCE, B, 0, 7, 0, T), "unknown by"),
        ((54, Field.UDP_SOURCE, B, 0, 0, 1, 0), "BYTES and wide"),
        ((54, Field.UDP_LENGTH, LENGTH, 0, 0, 4, 0), "LENGTH / VALUE"),
        ((54, Field.UDP_SOURCE, VALUE, 0, 1, 0, 0), "LENGTH / VALUE"),
        ((14, WideField.V6_SOURCE, B, 5, 0, 3, 0), "NULL table"),
        ((14, WideField.V6_SOURCE, B, 5, 0, 3, T), "BYTES with add"),
        ((14, WideField.V6_SOURCE, B, 0, 1, 3, T), "pitch below"),
        ((62, Field.GENEVE_VNI, U32, 0, 1, 2, T), "pitch below"),
        ((62, Field.GENEVE_VNI, U32, 0, 1, 6, T), "misaligned"),
        ((54, Field.UDP_SOURCE, U16, 0, 1, 0, T + 1), "misaligned"),
        ((H, Field.UDP_SOURCE, U16, 0, 1, 0, T), "BY_ROW without"),
    ]
    by_packet = (14, WideField.V6_DESTINATION, B, 0, 0, 0, T)
    for e, what in ladder:
        msg = step([by_packet, e], have_row=what != "BY_ROW without")
        assert msg.startswith("3.1:") and what in msg, (e, msg)
    bad_pad = emit_set_rows_array([(54, Field.UDP_SOURCE, U16, 0, 7, 0, T)])
    bad_pad[0]["_pad"][1] = 9
    with pytest.raises(ValueError, match=r"3\.0: padding"):
        model.check_args(True, hdr, H, bad_pad, 1, (), True, 4, True)
    assert "outside hdr" in step([(H - 1, Field.UDP_SOURCE, VALUE, 0, 0, 0, 0)])
    assert "outside hdr" in step([(H - 39, WideField.V6_DESTINATION, B, 0, 0, 0, T)])
    assert step([(H - 40, WideField.V6_DESTINATION, B, 0, 0, 0, T)]) is None
    # the first faulty set of the list is the one named
    assert step([ok, (14, 99, 0, 0, 0, 0, 0), (14, 98, 0, 0, 0, 0, 0)]).startswith("3.1:")
    # the sets before the sums, the sums before n == 0, n == 0 before the pointers
    odd = [(EmitSum.UDP, 55, 14)]
    assert step([(14, 99, 0, 0, 0, 0, 0)], sums=odd).startswith("3.0:")
    assert step([ok], sums=odd, n=0, ptrs=False).startswith("4:")
    assert step([ok, (14, Field.V6_VERSION, VALUE, 6, 0, 0, 0)],
                sums=[(EmitSum.UDP, 54, 14)]).startswith("4:")
    assert step([ok], sums=[(EmitSum.UDP, 54, 14)], n=0, ptrs=False) is None
    assert step([ok], sums=[(EmitSum.UDP, 54, 14)], ptrs=False).startswith("6:")
