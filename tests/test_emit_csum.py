"""ingot_gpu_emit_packets_csum on the device against its definition
(tests/emit_csum_model.py over the oracle's plain emit): in every test the
whole destination arena, the 0xA5 bytes between the packets included, is
byte-equal to the model's.  Needs an MI355X: `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import (CSUM_DTYPE, CSUM_L3, CSUM_L4, Chain, EmitSource, EmitSum, Field,
                       GenProfile)
from ingot_amd.abi import emit_sums_array
from ingot_amd.hostgen import gen_frames_host
from tests import csum_model
from tests import emit_csum_cases as cases
from tests import emit_csum_model as model

pytestmark = pytest.mark.gpu
TUN = Chain.GeneveOverV6Tunnel


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


def _dev_sets(torch, sets):
    return [s if len(s) == 4 else (*s[:4], _dev(torch, s[4])) for s in sets]


def _want(hdr, sets, sums, src, off, lens, dst_off, size):
    want = np.full(size, 0xA5, np.uint8)
    oracle.emit_batch(hdr, sets, src, off, lens, want, dst_off)
    return model.apply(want, hdr, sums, dst_off, lens, sets)


def _run(ctx, torch, hdr, sets, sums, src, off, lens, dst_off, size, stream=None, d_src=None):
    """-> the destination arena after the call (numpy), started as 0xA5."""
    d_dst = _dev(torch, np.full(size, 0xA5, np.uint8))
    ctx.emit_packets(hdr, _dev_sets(torch, sets), _dev(torch, src) if d_src is None else d_src,
                     _dev(torch, np.asarray(off, np.uint64)),
                     _dev(torch, np.asarray(lens, np.uint16)), d_dst,
                     _dev(torch, np.asarray(dst_off, np.uint64)), stream=stream, sums=sums)
    if stream is not None:
        stream.synchronize()
    return d_dst.cpu().numpy()


def _same(got, want, tag=""):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, bad[:10], got[bad[:10]], want[bad[:10]])


def _check(ctx, torch, hdr, sets, sums, src, off, lens, dst_off, size, tag=""):
    got = _run(ctx, torch, hdr, sets, sums, src, off, lens, dst_off, size)
    _same(got, _want(hdr, sets, sums, src, off, lens, dst_off, size), tag)
    return got


def _kat_sets(kat):
    out = []
    for s in kat["sets"]:
        at, field, source, add = s[0], Field[s[1]], EmitSource[s[2]], s[3]
        if source in (EmitSource.U16, EmitSource.U32):
            dt = np.uint16 if source == EmitSource.U16 else np.uint32
            out.append((at, field, source, add, np.full(1, s[4], dtype=dt)))
        else:
            out.append((at, field, source, add))
    return out


@pytest.mark.parametrize("dmis", range(16))
def test_alignment_sweep(ctx, torch, kats, dmis):
    """One short packet at every destination x source misalignment (both
    parities of D + at; the field inside one chunk and across two): the emit
    KATs' tunnel stacks with the UDP sum, and every stack of this file."""
    rng = np.random.default_rng(dmis)
    work = []
    for kat in kats["emit_kats"]:
        if kat["after"] is not None:
            work.append((kat["name"], bytes.fromhex(kat["hdr"]), _kat_sets(kat),
                         [(EmitSum.UDP, 54, 14)], np.frombuffer(bytes.fromhex(kat["payload"]),
                                                                np.uint8)))
    for name in cases.STACKS:
        hdr, sets, sums = cases.stack(name, 1, rng)
        work.append((name, hdr, sets, sums, rng.integers(0, 256, 37, dtype=np.uint8)))
    for name, hdr, sets, sums, pay in work:
        for smis in range(16):
            src = np.zeros(smis + len(pay) + 64, np.uint8)
            src[smis:smis + len(pay)] = pay
            _check(ctx, torch, hdr, sets, sums, src, [smis], [len(pay)], [dmis],
                   dmis + len(hdr) + len(pay) + 64, (name, dmis, smis))


def _edge_batch(n, rng, lengths=cases.EDGE_LENGTHS):
    """n mixed-length payloads; every length of `lengths` is in the batch when
    it has room (the first ones otherwise), at random places."""
    ln = rng.integers(0, 1600, n).astype(np.uint16)
    k = min(n, len(lengths))
    ln[rng.permutation(n)[:k]] = np.asarray(lengths[len(lengths) - k:], np.uint16)
    return ln


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_group_edges(ctx, torch, n):
    """Batches that end inside, at and just past a wave, a 256-packet group
    and several groups, with payloads from 0 B to 65,535 B (packets that cross
    64-chunk steps, wave turns and whole turns of the 16 waves; the longest
    has no valid UDP length and keeps its field)."""
    rng = np.random.default_rng(300 + n)
    ln = _edge_batch(n, rng)
    if n >= len(cases.EDGE_LENGTHS):
        assert set(cases.EDGE_LENGTHS) <= set(ln.tolist())
    else:
        assert 65535 in ln.tolist()
    src, off = cases.random_source(ln, rng)
    for name in ("opte", "geneve_v4"):
        hdr, sets, sums = cases.stack(name, n, rng)
        dst_off, size = cases.pack(ln, len(hdr), rng)
        _check(ctx, torch, hdr, sets, sums, src, off, ln, dst_off, size, (name, n))


@pytest.mark.parametrize("name", cases.STACKS)
def test_stacks(ctx, torch, name):
    rng = np.random.default_rng(77)
    n = 700
    ln = _edge_batch(n, rng)
    src, off = cases.random_source(ln, rng)
    hdr, sets, sums = cases.stack(name, n, rng)
    dst_off, size = cases.pack(ln, len(hdr), rng)
    got = _check(ctx, torch, hdr, sets, sums, src, off, ln, dst_off, size, name)
    # each named sum alone as well
    for s in sums:
        _check(ctx, torch, hdr, sets, [s], src, off, ln, dst_off, size, (name, s))
    if name == "preset":
        # the caller's constants are gone wherever a sum was written, and kept
        # in the one packet that is no datagram
        long = int(np.nonzero(ln == 65535)[0][0])
        d = int(dst_off[long])
        assert bytes(got[d + 40:d + 42]) == bytes([0xBE, 0xEF])


@pytest.mark.parametrize("profile", ["MIXED", "VLAN_V6EH"])
def test_fuzz(ctx, torch, profile):
    n = 8000
    rng = np.random.default_rng(5)
    arena, off, lens = gen_frames_host(GenProfile[profile], n, seed=21, slack=64)
    for name in ("opte", "geneve_v4"):
        hdr, sets, sums = cases.stack(name, n, rng)
        dst_off, size = cases.pack(lens, len(hdr), rng, max_gap=3)
        _check(ctx, torch, hdr, sets, sums, arena, off, lens, dst_off, size, (profile, name))


@pytest.mark.parametrize("name", ["opte", "geneve_v4"])
def test_cross_check_three_calls(ctx, torch, name):
    """emit_packets + parse(UdpParser) + checksum_fill(L3 | L4) leaves the same
    arena (no packet here is longer than a datagram)."""
    rng = np.random.default_rng(9)
    n = 3000
    ln = _edge_batch(n, rng, cases.EDGE_LENGTHS[:-1])
    src, off = cases.random_source(ln, rng)
    hdr, sets, sums = cases.stack(name, n, rng)
    dst_off, size = cases.pack(ln, len(hdr), rng)
    one = _run(ctx, torch, hdr, sets, sums, src, off, ln, dst_off, size)
    d_dst = _dev(torch, np.full(size, 0xA5, np.uint8))
    d_doff = _dev(torch, dst_off)
    d_tl = _dev(torch, (ln.astype(np.int64) + len(hdr)).astype(np.uint16))
    ctx.emit_packets(hdr, _dev_sets(torch, sets), _dev(torch, src), _dev(torch, off),
                     _dev(torch, ln), d_dst, d_doff)
    recs = ctx.parse(d_dst, d_doff, d_tl, Chain.UdpParser)
    ctx.checksum_fill(d_dst, d_doff, d_tl, recs, CSUM_L3 | CSUM_L4)
    _same(one, d_dst.cpu().numpy(), name)
    _same(one, _want(hdr, sets, sums, src, off, ln, dst_off, size), name)


def test_round_trip_inner_states(ctx, torch):
    """A GENEVE_OVER_V6 parse of the result + checksum_verify: the inner
    layers' states are those of the source frames, and the outer UDP sum
    verifies."""
    n = 8000
    rng = np.random.default_rng(3)
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=32, slack=64)
    arena = arena.copy()
    csum_model.fill(arena, off, lens, oracle.parse_batch(arena, off, lens, Chain.GenericUlp))
    hdr, sets, sums = cases.stack("opte", n, rng)
    dst_off, size = cases.pack(lens, len(hdr), rng)
    d_dst = _dev(torch, np.full(size, 0xA5, np.uint8))
    d_arena, d_off, d_len = _dev(torch, arena), _dev(torch, off), _dev(torch, lens)
    d_doff = _dev(torch, dst_off)
    d_tl = _dev(torch, (lens.astype(np.int64) + len(hdr)).astype(np.uint16))
    ctx.emit_packets(hdr, _dev_sets(torch, sets), d_arena, d_off, d_len, d_dst, d_doff, sums=sums)
    rows = lambda t: t.cpu().numpy().view(CSUM_DTYPE).reshape(-1)  # noqa: E731
    inner = rows(ctx.checksum_verify(d_dst, d_doff, d_tl, ctx.parse(d_dst, d_doff, d_tl, TUN)))
    plain = rows(ctx.checksum_verify(d_arena, d_off, d_len,
                                     ctx.parse(d_arena, d_off, d_len, Chain.GenericUlp)))
    assert (inner["l3_state"] == plain["l3_state"]).all()
    assert (inner["l4_state"] == plain["l4_state"]).all()
    assert (inner["l4_state"] == csum_model.OK).sum() > 1000
    assert not (inner["l4_state"] == csum_model.BAD).any()
    outer = rows(ctx.checksum_verify(d_dst, d_doff, d_tl,
                                     ctx.parse(d_dst, d_doff, d_tl, Chain.UdpParser), CSUM_L4))
    assert (outer["l4_state"] == csum_model.OK).all()


def test_no_sums_is_plain_emit(ctx, torch):
    rng = np.random.default_rng(12)
    n = 1500
    ln = _edge_batch(n, rng)
    src, off = cases.random_source(ln, rng)
    hdr, sets, _ = cases.stack("preset", n, rng)
    dst_off, size = cases.pack(ln, len(hdr), rng)
    with_none = _run(ctx, torch, hdr, sets, None, src, off, ln, dst_off, size)
    with_empty = _run(ctx, torch, hdr, sets, [], src, off, ln, dst_off, size)
    _same(with_empty, with_none)
    want = np.full(size, 0xA5, np.uint8)
    oracle.emit_batch(hdr, sets, src, off, ln, want, dst_off)
    _same(with_empty, want)
    # hdr_len 0 (a gather copy) through the new entry point
    dst_off, size = cases.pack(ln, 0, rng)
    want = np.full(size, 0xA5, np.uint8)
    oracle.emit_batch(b"", [], src, off, ln, want, dst_off)
    _same(_run(ctx, torch, b"", [], [], src, off, ln, dst_off, size), want)


def test_argument_errors(ctx, torch):
    """Every argument error of the sums is EINVAL (-1) and nothing is written."""
    lib = ingot_amd.load_library()
    hdr, sets, sums = cases.stack("geneve_v4", 4, np.random.default_rng(0))
    dev_sets = _dev_sets(torch, sets)
    src = _dev(torch, np.arange(256, dtype=np.uint8))
    off = _dev(torch, np.array([0, 16, 32, 48], np.uint64))
    ln = _dev(torch, np.array([10, 11, 12, 13], np.uint16))
    doff = _dev(torch, np.array([0, 100, 200, 300], np.uint64))
    dst = _dev(torch, np.full(512, 0xA5, np.uint8))

    def call(h, set_rows, sum_arr, n_sums, null_sums=False):
        rows = [(s[0], s[1], s[2], s[3], s[4].data_ptr() if len(s) > 4 else None)
                for s in set_rows]
        sa = ingot_amd.emit_sets_array(rows)
        hb = (ctypes.c_uint8 * max(len(h), 1)).from_buffer_copy(h or b"\0")
        return lib.ingot_gpu_emit_packets_csum(
            ctx._h, ctypes.addressof(hb), len(h), sa.ctypes.data_as(ctypes.c_void_p), len(sa),
            None if null_sums else sum_arr.ctypes.data_as(ctypes.c_void_p), n_sums,
            src.data_ptr(), off.data_ptr(), ln.data_ptr(), 4, dst.data_ptr(), doff.data_ptr(),
            None)

    def einval(s, h=hdr, se=dev_sets, tag=""):
        arr = emit_sums_array(s)
        assert call(h, se, arr, len(arr)) == -1, (tag, s)
        with pytest.raises(ValueError):
            model.check_args(h, se, s)

    three = emit_sums_array([(EmitSum.IPV4, 14), (EmitSum.UDP, 34, 14), (EmitSum.IPV4, 14)])
    assert call(hdr, dev_sets, three, 3) == -1                      # n_sums > the maximum
    assert call(hdr, dev_sets, three, 1, null_sums=True) == -1      # NULL with n_sums > 0
    einval([(2, 34, 14)])                                           # unknown kind
    padded = emit_sums_array([(EmitSum.UDP, 34, 14)])
    padded[0]["_pad"][1] = 1
    assert call(hdr, dev_sets, padded, 1) == -1                     # non-zero padding
    einval([(EmitSum.UDP, 34, 14), (EmitSum.UDP, 34, 14)])          # two of one kind
    einval([(EmitSum.IPV4, 14), (EmitSum.IPV4, 14)])
    einval([(EmitSum.UDP, 35, 14)])                                 # odd at
    einval([(EmitSum.UDP, 34, 13)])                                 # odd l3_at
    einval([(EmitSum.IPV4, 15)])
    einval([(EmitSum.IPV4, 14, 2)])                                 # IPV4: l3_at != 0
    einval([(EmitSum.IPV4, 34)])                                    # version nibble != 4
    ihl4 = bytes(hdr[:14]) + bytes([0x44]) + bytes(hdr[15:])
    einval([(EmitSum.IPV4, 14)], ihl4)                              # ihl < 5
    ihl15 = bytes(hdr[:14]) + bytes([0x4F]) + bytes(hdr[15:])
    einval([(EmitSum.IPV4, 14)], ihl15)                             # at + 4 ihl > hdr_len
    einval([(EmitSum.UDP, len(hdr) - 6, 14)])                       # at + 8 > hdr_len
    einval([(EmitSum.UDP, 34, 0)])                                  # version at l3_at: 0xa
    einval([(EmitSum.UDP, 32, 14)])                                 # IPv4 header ends past at
    v6hdr, v6sets, _ = cases.stack("opte", 4, np.random.default_rng(0))
    einval([(EmitSum.UDP, 52, 14)], v6hdr, _dev_sets(torch, v6sets))  # IPv6: 40 B past at
    for f in (Field.V4_VERSION, Field.V4_IHL, Field.V6_VERSION):   # setters on a named header
        extra = dev_sets + [(14, f, EmitSource.VALUE, 4)]
        einval([(EmitSum.IPV4, 14)], hdr, extra, f)
        einval([(EmitSum.UDP, 34, 14)], hdr, extra, f)
    einval([(EmitSum.UDP, 0, 0)], b"", [])                          # hdr_len 0 with sums
    # emit_packets's own errors still come first
    assert call(bytes(300), [], emit_sums_array([]), 0) == -1
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()
    # and the same arguments without the faults are accepted
    ok = emit_sums_array(sums)
    assert call(hdr, dev_sets, ok, len(ok)) == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() != 0xA5).any()


def test_side_stream(ctx, torch):
    rng = np.random.default_rng(8)
    n = 2000
    ln = _edge_batch(n, rng)
    src, off = cases.random_source(ln, rng)
    hdr, sets, sums = cases.stack("opte", n, rng)
    dst_off, size = cases.pack(ln, len(hdr), rng)
    side = torch.cuda.Stream()
    d_src = _dev(torch, src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = _run(ctx, torch, hdr, sets, sums, src, off, ln, dst_off, size, stream=side,
                   d_src=d_src)
    _same(got, _want(hdr, sets, sums, src, off, ln, dst_off, size))
