"""The cases of tests/emit_rows_sweep_cases.py on the references alone (no
GPU): what tests/test_emit_rows_sweep.py compares the device with (the
definition, tests/emit_rows_model.py) is held here to a second way of computing
it, every case is shown to reach the edge it is named for, and every listed
fault a device could have is shown to be caught by a case of its part.

Second ways: the field read back with oracle.be_bits at the bit places of
tests/modify_read_model.GEOMETRY (a table independent of the oracle's setter)
and every other bit against the prefill; the pasted bytes against the table's
rows; a byte-wise RFC 1071 receiver; and, for every case, the whole arena
against sweep_cases.emulate, the call in plain Python.
"""
import numpy as np
import pytest

import oracle
from ingot_amd import EmitSource, EmitSum, Field, WideField
from ingot_amd.abi import WIDE_BYTES
from tests import csum_sweep_cases as sc
from tests import emit_rows_cases as rc
from tests import emit_rows_model as model
from tests import emit_rows_sweep_cases as sw
from tests import modify_read_model as mrm

LENGTH, VALUE, BYTES = EmitSource.LENGTH, EmitSource.VALUE, EmitSource.BYTES


def _defined(job):
    """The definition's arena, equal to the plain-Python emit's."""
    want = sw.expected(job)
    got, outside = sw.emulate(job)
    bad = np.nonzero(got != want)[0]
    assert outside == 0 and bad.size == 0, (job.tag, bad[:8], got[bad[:8]], want[bad[:8]])
    return want


def _packets(job, arena):
    """(i, row index, the emitted packet's bytes) of every emitted packet."""
    b, H = job.b, len(job.case.hdr)
    for i in np.nonzero(sw.live(b))[0].tolist():
        d = int(b.dst_off[i])
        yield i, (i if b.rows is None else int(b.rows[i])), arena[d:d + H + int(b.lens[i])]


def _caught(fault, jobs):
    """The first of `jobs` on which a device with `fault` would differ from
    the definition (or use a guarded packet's descriptors)."""
    for job in jobs:
        got, outside = sw.emulate(job, fault)
        if outside or got.tobytes() != sw.expected(job).tobytes():
            return job.tag
    return None


# ---------------------------------------------------------------------------
# A. Narrow fields
# ---------------------------------------------------------------------------
def test_the_block_and_its_batches():
    assert set(sw.KIND_AT) == {g[0] for g in mrm.GEOMETRY.values()}
    for f in Field:
        kind, first, bits = mrm.GEOMETRY[f]
        assert kind == sc.kind_of(f) and bits == sc.FIELD_BITS[f]
        assert sw.field_at(f) + (first + bits + 7) // 8 <= sw.BLOCK_LEN
    for hdr_len in (sw.BLOCK_LEN, sw.BIG):
        for with_rows in (False, True):
            b = sw.sweep_batch(hdr_len, with_rows)
            alive = sw.live(b)
            assert len(b.lens) == 65 and alive[64]
            assert {int(d) % 16 for d in b.dst_off[alive]} == set(range(16))
            ln = set(b.lens[alive].tolist())
            assert ln >= set(sw.cases.EDGE_LENGTHS[:-1]) and (b.lens[alive] == 65535).sum() == 1
            if with_rows:
                assert set(np.nonzero(~alive)[0].tolist()) == set(range(6, 65, 7))
                assert set(b.rows[alive].tolist()) == set(range(5))
                assert (b.dst_off[~alive] >= b.size).all() and (b.off[~alive] >= len(b.src)).all()


@pytest.mark.parametrize("field", list(Field), ids=lambda f: f.name)
def test_narrow_sweep(field):
    """Every form of the field's sweep: the field reads back, at GEOMETRY's
    place, as (operand + add) mod 2^width, or LENGTH's count; every other bit
    of the block is the prefill; the sweep changes the block (no hole)."""
    _, first, bits = mrm.GEOMETRY[field]
    at, mask, H = sw.field_at(field), (1 << bits) - 1, sw.BLOCK_LEN
    shift = 8 * H - (8 * at + first + bits)
    moved, seen = 0, set()
    for form in sw.FORMS:
        for job in sw.narrow_jobs(field, form):
            want = _defined(job)
            (s,) = job.case.host_sets()
            source, add = EmitSource(int(s[2])), int(s[3])
            by_row, t = model._table(s)
            fill = job.case.hdr[0]
            rest = int.from_bytes(job.case.hdr, "big") & ~(mask << shift)
            values = set()
            for i, r, pkt in _packets(job, want):
                if source == LENGTH:
                    v = len(pkt) - at + add
                elif source == VALUE:
                    v = add
                else:
                    v = int(t[r if by_row else i]) + add
                blk = pkt[:H].tobytes()
                assert oracle.be_bits(blk[at:], first, bits) == v & mask, (job.tag, i)
                assert int.from_bytes(blk, "big") & ~(mask << shift) == rest, (job.tag, i)
                moved += int(blk != bytes([fill]) * H)
                values.add(v & mask)
            seen.add((form, source, by_row))
            if form in ("by packet", "by row"):
                # the sweep's values reach the field as they are (a U16 row
                # holds their low half)
                held = 0xFFFF if source == EmitSource.U16 else 0xFFFFFFFF
                assert {x & held & mask for x in sw.sweep_values(field)} <= values, job.tag
            if form == "add":
                # a row that + add is exactly 2^16 / 2^32, and one below 0
                tab = np.asarray(t).astype(np.int64)
                wrap = 1 << (16 if source == EmitSource.U16 else 32)
                assert add <= 0 or ((tab + add) == wrap).any(), job.tag
                assert add >= 0 or ((tab + add) < 0).any(), job.tag
    assert moved > 0
    mis, match = sw.sources_for(field)
    assert {("by packet", mis, False), ("by packet", match, False), ("by row", mis, True),
            ("by row", match, True), ("length", LENGTH, False), ("value", VALUE, False)} <= seen


A_FAULTS = {"rshift": sw.FORMS, "add after mask": ("add",), "u32 as u16": ("by packet", "by row"),
            "row is packet": ("by row",), "length": ("length",)}


@pytest.mark.parametrize("fault", sorted(A_FAULTS))
def test_narrow_faults_are_caught(fault):
    assert sw.FAULTS[fault] == "A"
    tag = _caught(fault, (j for f in Field for form in A_FAULTS[fault]
                          for j in sw.narrow_jobs(f, form)))
    assert tag is not None
    # and it is the fault, not the emulation, that differs
    assert _caught(None, sw.narrow_jobs(Field.V4_FRAGMENT_OFFSET, A_FAULTS[fault][0])) is None


def test_rshift_fault_is_caught_in_every_field_that_ends_inside_a_byte():
    inside = [f for f in Field if sum(mrm.GEOMETRY[f][1:]) % 8]
    assert len(inside) == 10 and {Field.VLAN_DEI, Field.V4_FLAGS, Field.V6_ECN} <= set(inside)
    for f in inside:
        assert _caught("rshift", sw.narrow_jobs(f, "value")) is not None, f


# ---------------------------------------------------------------------------
# B. Wide fields and piece limits
# ---------------------------------------------------------------------------
def _b_jobs():
    for wf in WideField:
        yield from sw.wide_at_jobs(wf)
    yield from sw.pieces_jobs()
    yield from sw.small_block_jobs()
    for job, _ in sw.restore_jobs():
        yield job


def _pasted(job, arena):
    """Every byte of a wide set that no later set covers is its table row's.
    -> bytes that differ from the block."""
    hdr = job.case.hdr
    sets = job.case.host_sets()
    owner = np.full(len(hdr), -1)
    for k, s in enumerate(sets):
        if EmitSource(int(s[2])) == BYTES:
            p = int(s[0]) + model.WIDE_AT[WideField(int(s[1]))]
            owner[p:p + WIDE_BYTES[WideField(int(s[1]))]] = k
        else:
            p, nb = model.field_span(s[1])
            owner[int(s[0]) + p:int(s[0]) + p + nb] = -1
    moved = 0
    for i, r, pkt in _packets(job, arena):
        for k, s in enumerate(sets):
            if EmitSource(int(s[2])) != BYTES:
                continue
            by_row, t = model._table(s)
            p = int(s[0]) + model.WIDE_AT[WideField(int(s[1]))]
            mine = np.nonzero(owner == k)[0]
            row = np.asarray(t[r if by_row else i], np.uint8)
            assert (pkt[mine] == row[mine - p]).all(), (job.tag, i, k)
            moved += int((pkt[mine] != np.frombuffer(hdr, np.uint8)[mine]).sum())
    return moved


@pytest.mark.parametrize("wf", list(WideField), ids=lambda f: f.name)
def test_wide_at_every_place(wf):
    ats, kinds, parity = [], set(), set()
    for job in sw.wide_at_jobs(wf):
        assert _pasted(job, _defined(job)) > 0
        for s in job.case.sets:
            view = s[4][1] if isinstance(s[4], tuple) else s[4]
            kinds |= sw.piece_kinds(view.first, view.pitch, view.width)
            parity.add(view.first % 2)
            ats.append(s[0])
    last = sw.BIG - model.WIDE_AT[wf] - WIDE_BYTES[wf]
    assert {a % 16 for a in ats} == set(range(16)) and max(ats) == last
    # every piece, loaded whole and byte by byte; tables at both parities
    sizes = (4, 2) if WIDE_BYTES[wf] == 6 else (4,)
    assert kinds == {(n, whole) for n in sizes for whole in (True, False)} and parity == {0, 1}
    # with every destination misalignment, a set's bytes meet a region chunk's
    # end at every phase
    b = sw.sweep_batch(sw.BIG, True)
    phases = {(int(d) + a + model.WIDE_AT[wf]) % 16 for d in b.dst_off[sw.live(b)] for a in ats}
    assert phases == set(range(16))


def test_piece_limits_and_small_blocks():
    jobs = list(sw.pieces_jobs())
    assert [len(j.case.sets) for j in jobs] == [8] * 4
    assert [bool(j.case.sums) for j in jobs] == [True, False, True, False]
    pieces = [sum((WIDE_BYTES[WideField(int(s[1]))] + 3) // 4 for s in j.case.sets) for j in jobs]
    assert pieces == [32, 32, 16, 16]
    for job in jobs:
        assert len(job.case.hdr) == 254
        assert {isinstance(s[4], tuple) for s in job.case.sets} == {True, False}
        want = _defined(job)
        assert _pasted(job, want) > 0
        if job.case.sums:
            assert all(sc.bytewise_receiver_ok(p, job.case.hdr, job.case.sums)
                       for _, _, p in _packets(job, want) if len(p) - 54 <= 65535)
    # the last sets end with the block
    assert 230 + 8 + 16 == 254 and 242 + 6 + 6 == 254
    small = list(sw.small_block_jobs())
    assert [len(j.case.hdr) for j in small] == [12, 14]
    for job in small:
        b = job.b
        assert _pasted(job, _defined(job)) > 0
        assert {(int(ln), int(d) % 16) for ln, d in zip(b.lens, b.dst_off)} == \
            {(ln, m) for ln in sw.SHORT for m in range(16)}
    assert small[1].b.rows is not None and sw.live(small[1].b).all()


def test_set_overwritten_restored():
    shown = []
    for job, narrow_last in sw.restore_jobs():
        want = _defined(job)
        assert _pasted(job, want) > 0
        sets = {(int(s[0]), int(s[1])): s for s in job.case.host_sets()}  # the last of each
        u16 = sets[(30, int(Field.UDP_SOURCE))]
        u32 = sets[(0, int(Field.GENEVE_VNI))]
        for i, r, pkt in _packets(job, want):
            a = (int(u16[4][i]) + 3) & 0xFFFF
            v = int(u32[4][i]) & 0xFFFFFF
            got = (bytes(pkt[30:32]) == a.to_bytes(2, "big"),
                   bytes(pkt[4:7]) == v.to_bytes(3, "big"))
            assert got == (narrow_last, narrow_last) or (a, v) == (0, 0), (job.tag, i)
        shown.append(want[:4096].tobytes())
    assert shown[0] == shown[2] != shown[1]  # the last wide set wins, wherever the narrow one was


B_FAULTS = ("be32", "mac tail", "first wins")


@pytest.mark.parametrize("fault", B_FAULTS)
def test_wide_faults_are_caught(fault):
    assert sw.FAULTS[fault] == "B"
    assert _caught(fault, _b_jobs()) is not None
    if fault == "first wins":
        assert _caught(fault, (j for j, _ in sw.restore_jobs())) is not None


# ---------------------------------------------------------------------------
# C. Sums at their edges
# ---------------------------------------------------------------------------
def _v4_header_ok(pkt, at):
    h = pkt[at:at + 20].astype(np.uint64)
    total = int((h[0::2] << np.uint64(8)).sum() + h[1::2].sum())
    while total >> 16:
        total = (total & 0xFFFF) + (total >> 16)
    return total == 0xFFFF


def _received(job, arena):
    """A byte-wise receiver accepts every emitted datagram (and IPv4 header);
    -> datagrams."""
    hdr, sums = job.case.hdr, job.case.sums
    u = next(s for s in sums if int(s[0]) == int(EmitSum.UDP))
    v4 = [s for s in sums if int(s[0]) == int(EmitSum.IPV4)]
    n = 0
    for i, _, pkt in _packets(job, arena):
        if v4:
            assert _v4_header_ok(pkt, int(v4[0][1])), (job.tag, i)
        if len(pkt) - u[1] > 65535:
            continue
        assert sc.bytewise_receiver_ok(pkt, hdr, sums), (job.tag, i)
        n += 1
    return n


def test_solved_table_words_land_on_the_edges():
    seen, places = set(), set()
    for job in sw.solved_jobs():
        want = _defined(job)
        sw.held(job, want)
        assert _received(job, want) >= 590
        name, what = job.tag.split()[:2]
        b = job.b
        for k, at, wanted, note in job.checks:
            seen.add((name, what, k, wanted))
            if k != sw.BIG_AT:
                places.add((name, what, int(b.dst_off[k]) % 2, (int(b.dst_off[k]) + at) % 16 == 15))
        assert len(b.lens) == 600 and int(b.lens[sw.BIG_AT]) == 65535
        assert all(sw.live(b)[k] for k in sc.CRAFTED_AT)
    for name, what, _, _ in sw.SOLVED:
        # every crafted place got every crafted value
        assert {(k, w) for n, t, k, w in seen if (n, t) == (name, what) and k != sw.BIG_AT} == \
            {(k, w) for k in sc.CRAFTED_AT for w in sw.WANT[what].values()}
        # both parities; the field inside one chunk and across two
        mine = {p[2:] for p in places if p[:2] == (name, what)}
        assert {p[0] for p in mine} == {0, 1} and {p[1] for p in mine} == {True, False}
    # the by-packet set on UDP_CHECKSUM shows only where no sum is taken
    job = next(j for j in sw.solved_jobs() if j.tag.startswith("v6_udp"))
    want = sw.expected(job)
    tab = job.case.backing["csum"].view(np.uint16)
    same = [i for i, _, p in _packets(job, want) if (int(p[60]) << 8 | int(p[61])) == int(tab[i])]
    assert sw.BIG_AT in same and len(same) <= 2


@pytest.mark.parametrize("name", rc.STACKS)
def test_extreme_operands(name):
    for job in sw.extreme_jobs(name):
        want = _defined(job)
        sw.held(job, want)
        assert _received(job, want) == 6
        u = next(s for s in job.case.sums if int(s[0]) == int(EmitSum.UDP))
        S = len(job.case.hdr) - u[1] + job.b.lens.astype(np.int64)
        assert sorted(S.tolist())[-4:] == [65535, 65535, 65536, 65536]
        assert {int(d) % 2 for d in job.b.dst_off[S == 65535]} == {0, 1}
        assert all(len(set(a.tolist())) == 1 for a in job.case.backing.values())


def test_udp_zero_fault_is_caught():
    assert sw.FAULTS["udp zero"] == "C"
    assert _caught("udp zero", sw.solved_jobs()) is not None


# ---------------------------------------------------------------------------
# D. Tables, rows, guard
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u32", "v6"])
def test_far_rows(kind):
    job = sw.far_job(kind)
    want = _defined(job)
    assert _received(job, want) > 60
    far = [i for i, r, _ in _packets(job, want) if r * sw.FAR_PITCH >= 1 << 32]
    assert len(far) >= 5 and sw.FAR_ROWS - 1 in job.b.rows.tolist()
    assert _caught("offset 32", [job]) is not None and sw.FAULTS["offset 32"] == "D"


def test_the_row_guard():
    jobs = sw.guard_jobs()
    for job, emits in jobs:
        want = _defined(job)
        assert (want != 0xA5).any() == emits, job.tag
        if "survivor" in job.tag:
            assert sw.live(job.b).sum() == 1
            (k,) = np.nonzero(sw.live(job.b))[0]
            assert k // 64 == int(job.tag[-1])
            d = int(job.b.dst_off[k])
            end = d + len(job.case.hdr) + int(job.b.lens[k])
            assert (want[:d] == 0xA5).all() and (want[end:] == 0xA5).all()
    assert sum("survivor" in j.tag for j, _ in jobs) == 4
    assert sw.FAULTS["guard"] == "D"
    for job in [j for j, _ in jobs] + [sw.pitch_zero_job()]:
        assert _caught("guard", [job]) is not None or "survivor" in job.tag, job.tag
    _defined(sw.pitch_zero_job())


def test_sources_and_ways():
    """Every EmitSource occurs by packet and, where the header allows it, by
    row; every fault has its part's test."""
    seen = set()
    jobs = [j for form in sw.FORMS for j in sw.narrow_jobs(Field.V6_FLOW_LABEL, form)]
    jobs += list(_b_jobs()) + list(sw.solved_jobs()) + [j for j, _ in sw.guard_jobs()]
    for job in jobs:
        seen |= {(EmitSource(int(s[2])), len(s) > 4 and isinstance(s[4], tuple))
                 for s in job.case.sets}
    assert seen == {(s, False) for s in EmitSource} | {(s, True) for s in EmitSource
                                                      if s not in (LENGTH, VALUE)}
    assert set(sw.FAULTS) == set(A_FAULTS) | set(B_FAULTS) | {"udp zero", "offset 32", "guard"}
