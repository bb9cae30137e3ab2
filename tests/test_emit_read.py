"""ingot_gpu_emit_packets_read on the device against its definition
(tests/emit_read_model.py): in every test the whole destination arena, the
0xA5 bytes between the packets included, is byte-equal to the model's, and
d_taken equals the model's lengths.  Needs an MI355X: `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import (GENEVE_FIELDS_DTYPE, Chain, EmitSource, EmitSum, Field, GenProfile)
from ingot_amd import emit as E
from ingot_amd.abi import emit_sums_array
from ingot_amd.hostgen import gen_frames_host
from tests import csum_read_cases as chunks
from tests import emit_csum_cases as cases
from tests import emit_read_model as model

pytestmark = pytest.mark.gpu
TUN = Chain.GeneveOverV6Tunnel
NP = 256  # packets per workgroup of k_emit_read


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


def _u16(x):
    return None if x is None else np.asarray(x, np.uint16)


def _run(ctx, torch, hdr, sets, sums, tables, dst_off, size, frm=None, take=None, stream=None,
         d_tables=None):
    """-> (destination arena started as 0xA5, d_taken started as 0xA5A5), numpy."""
    n = len(tables[3]) - 1
    d_dst = _dev(torch, np.full(size, 0xA5, np.uint8))
    d_taken = _dev(torch, np.full(n, 0xA5A5, np.uint16))
    d = d_tables or [_dev(torch, x) for x in tables]
    ctx.emit_packets_read(hdr, _dev_sets(torch, sets), *d, d_dst,
                          _dev(torch, np.asarray(dst_off, np.uint64)),
                          frm=None if frm is None else _dev(torch, _u16(frm)),
                          take=None if take is None else _dev(torch, _u16(take)),
                          taken=d_taken, sums=sums, stream=stream)
    if stream is not None:
        stream.synchronize()
    return d_dst.cpu().numpy(), d_taken.cpu().numpy().view(np.uint16)


def _same(got, want, tag=""):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, bad[:10], got[bad[:10]], want[bad[:10]])


def _check(ctx, torch, hdr, sets, sums, tables, dst_off, size, frm=None, take=None, tag=""):
    want, lens = model.apply(np.full(size, 0xA5, np.uint8), hdr, sets, sums, *tables, dst_off,
                             _u16(frm), _u16(take))
    got, taken = _run(ctx, torch, hdr, sets, sums, tables, dst_off, size, frm, take)
    _same(taken, lens, (tag, "taken"))
    _same(got, want, tag)
    return got, lens


def _slots(n, total, dmis):
    """Destination offsets: slot i at a multiple of 16 plus dmis[i] -> (off, size)."""
    stride = (total + 15 + 16) // 16 * 16
    off = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.asarray(dmis, np.uint64)
    return off, int(n * stride + 64)


@pytest.mark.parametrize("name", ["geneve_v4", "opte"])
def test_alignment(ctx, torch, name):
    """4,096 two-chunk packets: every destination x chunk-0 x chunk-1
    misalignment, the boundary at an odd and at an even payload byte."""
    n = 4096
    rng = np.random.default_rng(10)
    hdr, sets, sums = cases.stack(name, n, rng)
    p = np.arange(n)
    dst_off, size = _slots(n, len(hdr) + 37, p % 16)
    mis = np.stack([(p // 16) % 16, p // 256], axis=1).reshape(-1).tolist()
    pays = rng.integers(0, 256, (n, 37), dtype=np.uint8)
    for c in (5, 6):
        packets = [chunks.cut_at(pays[i].tobytes(), [c]) for i in range(n)]
        tables = chunks.place(packets, misalign=mis)
        assert (tables[1][0:2 * n:2] % 16 == (p // 16) % 16).all()
        assert (tables[1][1:2 * n:2] % 16 == p // 256).all()
        _check(ctx, torch, hdr, sets, sums, tables, dst_off, size, tag=(name, c))


def test_cut_sweep(ctx, torch):
    """Every cut offset of a 40-byte payload at every destination misalignment;
    then two cuts one byte apart with an empty chunk between them."""
    rng = np.random.default_rng(11)
    n = 16 * 41
    hdr, sets, sums = cases.stack("opte", n, rng)
    dst_off, size = _slots(n, len(hdr) + 40, np.arange(n) % 16)
    pay = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    one = [chunks.cut_at(pay, [i // 16]) for i in range(n)]
    two = [chunks.cut_at(pay, [i // 16, i // 16, min(i // 16 + 1, 40)]) for i in range(n)]
    for tag, packets in (("one cut", one), ("two cuts", two)):
        tables = chunks.place(packets, misalign=(3, 0, 9, 14, 7, 12, 5), gap=1)
        _check(ctx, torch, hdr, sets, sums, tables, dst_off, size, tag=tag)


def test_many_pieces(ctx, torch):
    """More chunks than the kernel keeps per packet in LDS, and the 65,535 cut."""
    rng = np.random.default_rng(12)
    pay = rng.integers(0, 256, 600, dtype=np.uint8).tobytes()
    ones = [pay[k:k + 1] for k in range(600)]
    twos = [pay[k:k + 2] for k in range(0, 600, 2)]
    seventeens = []
    for k in range(0, 600, 17):
        seventeens += [pay[k:k + 17], b""]
    ff = b"\xff" * 65536
    full = [ff[k:k + 4093] for k in range(0, 65535, 4093)]
    full[-1] = ff[:65535 - 4093 * (len(full) - 1)]
    longer = full[:-1] + [full[-1] + b"\xff"]
    assert sum(map(len, full)) == 65535 and sum(map(len, longer)) == 65536
    packets = [ones, twos, seventeens, full, longer, full, [b""] + ones[:33]]
    n = len(packets)
    hdr, sets, sums = cases.stack("opte", n, rng)
    take = np.full(n, 65535, np.uint16)
    take[5] = 65400  # short enough to be a datagram: this one's sum is written
    tot = [len(hdr) + min(sum(map(len, p)), 65535) for p in packets]
    dst_off = (np.cumsum([0] + [t + 29 for t in tot[:-1]]) + 7).astype(np.uint64)
    size = int(dst_off[-1]) + tot[-1] + 64
    tables = chunks.place(packets, misalign=(1, 6, 11), gap=0)
    got, lens = _check(ctx, torch, hdr, sets, sums, tables, dst_off, size, take=take)
    assert lens.tolist() == [600, 600, 600, 65535, 65535, 65400, 33]
    # the two that are no datagram keep the field the header block gave them
    for i in (3, 4):
        assert bytes(got[int(dst_off[i]) + 60:int(dst_off[i]) + 62]) == hdr[60:62]


def _port_vni_stack(n, rng):
    hdr = (E.ethernet(cases.MAC_D, cases.MAC_S, 0x0800) + E.ipv4(cases.V4_S, cases.V4_D, 17)
           + E.udp(0xC0DE, 6081) + E.geneve(0x00ABCD))
    sets = [(14, Field.V4_TOTAL_LEN, EmitSource.LENGTH, 0),
            (34, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
            (34, Field.UDP_SOURCE, EmitSource.U16, 0,
             rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)),
            (42, Field.GENEVE_VNI, EmitSource.U32, 0,
             rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(np.uint32))]
    return hdr, sets, [(EmitSum.IPV4, 14), (EmitSum.UDP, 34, 14)]


def _cut(src, off, ln, rng):
    """csum_read_cases.cut by the oracle's records, then (random payloads
    rarely parse, and an unparsed frame is cut at 14 only) about half of the
    chunks cut once more at a random byte."""
    recs = oracle.parse_batch(src, off, ln, Chain.GenericUlp)
    packets = []
    for f, r in zip(chunks.frames_of(src, off, ln), recs):
        out = []
        for ch in chunks.cut(f, r, rng):
            if len(ch) > 1 and rng.random() < 0.5:
                k = int(rng.integers(1, len(ch)))
                out += [ch[:k], ch[k:]]
            else:
                out.append(ch)
        packets.append(out)
    return packets


def _edge_batch(n, rng, lengths=cases.EDGE_LENGTHS):
    ln = rng.integers(0, 1600, n).astype(np.uint16)
    k = min(n, len(lengths))
    ln[rng.permutation(n)[:k]] = np.asarray(lengths[len(lengths) - k:], np.uint16)
    return ln


@pytest.mark.parametrize("n", [1, NP - 1, NP, NP + 1, 2 * NP + 3])
def test_group_boundaries(ctx, torch, n):
    rng = np.random.default_rng(400 + n)
    ln = _edge_batch(n, rng)
    src, off = cases.random_source(ln, rng)
    packets = _cut(src, off, ln, rng)
    hdr, sets, sums = _port_vni_stack(n, rng)
    dst_off, size = cases.pack(ln, len(hdr), rng)
    tables = chunks.place(packets, misalign=tuple(range(16)) + (5, 11, 2), gap=1)
    _, lens = _check(ctx, torch, hdr, sets, sums, tables, dst_off, size, tag=n)
    assert (lens == ln).all()


def test_from_take_clamps(ctx, torch):
    """The clamp rows of tests/test_emit_read_model.py on the device, behind a
    header stack with both sums and as a bare copy."""
    a = bytes(range(10))
    big = np.random.default_rng(3).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    packets = [[a[:4], b"", a[4:]]] * 6
    packets += [[big[:40000], big[40000:65536]],
                [big[:30000], big[30000:60000], big[60000:70000]],
                [],
                [big[:65535], b"", big[65535:65540]]]
    frm = [10, 11, 3, 3, 0, 9, 65535, 65000, 0, 65534]
    take = [5, 5, 0, 100, 10, 65535, 9, 65535, 9, 65535]
    n = len(packets)
    arena, seg_off, seg_len, pkt_seg = chunks.place(packets, misalign=(5, 9, 14))
    # one more packet with reversed bounds, and an unreadable offset in every empty chunk
    pkt_seg = np.append(pkt_seg, pkt_seg[1]).astype(np.uint32)
    seg_off = np.where(seg_len == 0, np.uint64(1) << np.uint64(60), seg_off).astype(np.uint64)
    frm, take, n = frm + [0], take + [65535], n + 1
    tables = (arena, seg_off, seg_len, pkt_seg)
    rng = np.random.default_rng(13)
    for name in ("geneve_v4", None):
        hdr, sets, sums = cases.stack(name, n, rng) if name else (b"", [], [])
        for f, t in ((frm, take), (frm, None), (None, take), (None, None)):
            ln = model.linearise(*tables, _u16(f), _u16(t))[2]
            dst_off, size = cases.pack(ln, len(hdr), rng)
            _, lens = _check(ctx, torch, hdr, sets, sums, tables, dst_off, size, f, t,
                             tag=(name, f is None, t is None))
            if f is frm and t is take:
                assert lens.tolist() == [0, 0, 0, 7, 10, 1, 0, 535, 0, 1, 0]


def test_decapsulation(ctx, torch):
    """Chunked Geneve tunnel frames; d_from = the inner Ethernet offset that
    parse_read reports; hdr_len 0: the output is the inner frames."""
    n = 2000
    rng = np.random.default_rng(14)
    arena, off, lens = gen_frames_host(GenProfile["GENEVE"], n, seed=55, slack=64)
    crecs = oracle.parse_batch(arena, off, lens, TUN)
    frames = chunks.frames_of(arena, off, lens)
    packets = [chunks.cut(f, crecs[i], rng) for i, f in enumerate(frames)]
    tables = chunks.place(packets, misalign=tuple(range(16)) + (5, 11, 2), gap=1)
    d = [_dev(torch, x) for x in tables]
    gf, _ = ctx.parse_read(*d, TUN, fields="geneve")
    gf = gf.cpu().numpy().view(GENEVE_FIELDS_DTYPE).reshape(-1)
    ok = gf["inner"]["rec"]["status"] == 0
    assert ok.sum() > n // 2
    frm = np.where(ok, gf["outer"]["inner_eth_off"], lens).astype(np.uint16)
    inner_len = (lens.astype(np.int64) - frm).astype(np.uint16)
    dst_off, size = cases.pack(inner_len, 0, rng)
    got, taken = _check(ctx, torch, b"", [], [], tables, dst_off, size, frm=frm)
    assert (taken == inner_len).all()
    for i in np.nonzero(ok)[0][:200]:
        o = int(dst_off[i])
        assert got[o:o + int(taken[i])].tobytes() == frames[i][int(frm[i]):]
    # the inner frames parse as the oracle parses them
    d_rec = ctx.parse(_dev(torch, got), _dev(torch, dst_off), _dev(torch, taken), Chain.GenericUlp)
    want = oracle.parse_batch(got, dst_off, taken, Chain.GenericUlp)
    assert d_rec.cpu().numpy().tobytes() == want.tobytes()
    assert (want["status"][ok] == 0).all()


def test_no_sums_and_one_chunk(ctx, torch):
    """n_sums == 0 is ingot_gpu_emit_packets on the linearised source, hdr_len
    0 the pure pull-up, and one chunk per packet is ingot_gpu_emit_packets_csum
    over the same frames: the new kernel held to the old one on the device."""
    rng = np.random.default_rng(15)
    n = 1500
    ln = _edge_batch(n, rng)
    src, off = cases.random_source(ln, rng)
    packets = _cut(src, off, ln, rng)
    tables = chunks.place(packets, misalign=tuple(range(16)) + (7,), gap=2)
    hdr, sets, sums = cases.stack("preset", n, rng)

    def old(h, se, su, s, o, l, dst_off, size):
        d_dst = _dev(torch, np.full(size, 0xA5, np.uint8))
        ctx.emit_packets(h, _dev_sets(torch, se), _dev(torch, s), _dev(torch, o), _dev(torch, l),
                         d_dst, _dev(torch, dst_off), sums=su)
        return d_dst.cpu().numpy()

    lin = model.linearise(*tables)
    for h, se in ((hdr, sets), (b"", [])):
        dst_off, size = cases.pack(ln, len(h), rng)
        got, _ = _check(ctx, torch, h, se, [], tables, dst_off, size, tag=len(h))
        _same(got, old(h, se, None, *lin, dst_off, size), ("plain emit", len(h)))
    one = (src, off, ln, np.arange(n + 1, dtype=np.uint32))
    dst_off, size = cases.pack(ln, len(hdr), rng)
    got, _ = _check(ctx, torch, hdr, sets, sums, one, dst_off, size, tag="one chunk")
    _same(got, old(hdr, sets, sums, src, off, ln, dst_off, size), "emit_packets_csum")


@pytest.mark.parametrize("name", ["opte", "geneve_v4"])
def test_one_chunk_per_packet_is_emit_packets_csum(ctx, torch, name):
    """k_emit and k_emit_read share every step but the payload load
    (emit_common.h).  257 MIXED generator frames (a full group and one
    packet), every packet one chunk, no from / take, the stack's sums (`opte`:
    the UDP sum over IPv6; `geneve_v4`: the IPv4 and the UDP sum), the
    destinations at misalignments 0, 1 and 15: the two calls write identical
    bytes.  (emit_packets with `sums` is ingot_gpu_emit_packets_csum.)"""
    n = NP + 1
    src, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=257, slack=64)
    hdr, sets, sums = cases.stack(name, n, np.random.default_rng(18))
    d_sets = _dev_sets(torch, sets)
    d_src, d_off, d_len = _dev(torch, src), _dev(torch, off), _dev(torch, lens)
    d_ps = _dev(torch, np.arange(n + 1, dtype=np.uint32))
    for dmis in (0, 1, 15):
        dst_off, size = _slots(n, len(hdr) + int(lens.max()), np.full(n, dmis))
        d_dst_off = _dev(torch, dst_off)
        d_old = _dev(torch, np.full(size, 0xA5, np.uint8))
        d_new = d_old.clone()
        assert d_old.data_ptr() % 16 == 0 and d_new.data_ptr() % 16 == 0
        ctx.emit_packets(hdr, d_sets, d_src, d_off, d_len, d_old, d_dst_off, sums=sums)
        ctx.emit_packets_read(hdr, d_sets, d_src, d_off, d_len, d_ps, d_new, d_dst_off, sums=sums)
        old, new = d_old.cpu().numpy(), d_new.cpu().numpy()
        _same(new, old, (name, dmis))
        for i in (0, NP - 1, NP):  # the payload is there, behind the header block
            o = int(dst_off[i]) + len(hdr)
            assert new[o:o + int(lens[i])].tobytes() == \
                src[int(off[i]):int(off[i]) + int(lens[i])].tobytes(), (name, dmis, i)


def test_aliased_payload_and_streams(ctx, torch):
    """64 packets share one payload chunk behind their own header chunks; the
    same on a side stream."""
    rng = np.random.default_rng(16)
    n = 64
    pay = rng.integers(0, 256, 333, dtype=np.uint8).tobytes()
    heads = [rng.integers(0, 256, 14 + i % 5, dtype=np.uint8).tobytes() for i in range(n)]
    arena, so, sl, _ = chunks.place([[h] for h in heads] + [[pay]], misalign=(4, 13, 2, 7))
    seg_off = np.stack([so[:n], np.full(n, so[n])], axis=1).reshape(-1).astype(np.uint64)
    seg_len = np.stack([sl[:n], np.full(n, sl[n])], axis=1).reshape(-1).astype(np.uint16)
    tables = (arena, seg_off, seg_len, (2 * np.arange(n + 1)).astype(np.uint32))
    hdr, sets, sums = cases.stack("opte", n, rng)
    ln = np.array([len(h) + len(pay) for h in heads], np.uint16)
    dst_off, size = cases.pack(ln, len(hdr), rng)
    got, lens = _check(ctx, torch, hdr, sets, sums, tables, dst_off, size)
    assert (lens == ln).all()
    for i in range(n):
        o = int(dst_off[i]) + len(hdr)
        assert got[o:o + int(ln[i])].tobytes() == heads[i] + pay
    # A HIP stream of the test's own, wrapped for torch and destroyed below
    # (as tests/test_csum_read.py does): torch hands out its pooled streams in
    # turn, and which hardware queue a stream shares decides what a ring or a
    # doorbell wait stalls, so this test draws none and the
    # tests that run later get the streams they always got.
    lib = ingot_amd._lib.load()
    raw = ctypes.c_void_p()
    lib.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lib.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    assert lib.hipStreamCreateWithFlags(ctypes.byref(raw), 1) == 0  # hipStreamNonBlocking
    side = torch.cuda.ExternalStream(raw.value)
    d = [_dev(torch, x) for x in tables]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        again, _ = _run(ctx, torch, hdr, sets, sums, tables, dst_off, size, stream=side,
                        d_tables=d)
    side.synchronize()
    torch.cuda.synchronize()
    assert lib.hipStreamDestroy(raw) == 0
    _same(again, got, "side stream")


def test_argument_errors(ctx, torch):
    """Every EINVAL row of the header comment, with the destination left
    untouched; n == 0 succeeds with NULL device pointers.  (ERANGE cannot
    occur on gfx950: the largest header block fits its LDS, a static_assert of
    the kernel's source file.)"""
    lib = ingot_amd.load_library()
    hdr, sets, sums = cases.stack("geneve_v4", 4, np.random.default_rng(0))
    dev_sets = _dev_sets(torch, sets)
    arena, so, sl, ps = chunks.place([[bytes(20), bytes(9)]] * 4, misalign=(3, 8))
    src, so, sl, ps = (_dev(torch, x) for x in (arena, so, sl, ps))
    doff = _dev(torch, np.array([0, 100, 200, 300], np.uint64))
    dst = _dev(torch, np.full(512, 0xA5, np.uint8))
    good = dict(src=src.data_ptr(), so=so.data_ptr(), sl=sl.data_ptr(), ps=ps.data_ptr(),
                dst=dst.data_ptr(), doff=doff.data_ptr())

    def call(h=hdr, set_rows=dev_sets, su=sums, n=4, handle=None, n_sets=None, n_sums=None,
             null_hdr=False, null_sets=False, null_sums=False, **ptrs):
        p = {**good, **ptrs}
        rows = [(s[0], s[1], s[2], s[3], s[4].data_ptr() if len(s) > 4 else None)
                for s in set_rows]
        sa = ingot_amd.emit_sets_array(rows)
        cs = su if isinstance(su, np.ndarray) else emit_sums_array(su)
        hb = (ctypes.c_uint8 * max(len(h), 1)).from_buffer_copy(h or b"\0")
        return lib.ingot_gpu_emit_packets_read(
            ctx._h if handle is None else handle[0],
            None if null_hdr else ctypes.addressof(hb), len(h),
            None if null_sets else sa.ctypes.data_as(ctypes.c_void_p),
            len(sa) if n_sets is None else n_sets,
            None if null_sums else cs.ctypes.data_as(ctypes.c_void_p),
            len(cs) if n_sums is None else n_sums,
            p["src"], p["so"], p["sl"], p["ps"], None, None, n, p["dst"], p["doff"], None, None)

    assert call(handle=[None]) == -1                                   # NULL ctx
    # ingot_gpu_emit_packets's own
    assert call(h=bytes(300), set_rows=[], su=[]) == -1                # hdr_len > the maximum
    assert call(null_hdr=True) == -1                                   # hdr NULL, hdr_len > 0
    assert call(n_sets=9) == -1                                        # n_sets > the maximum
    assert call(null_sets=True) == -1                                  # sets NULL, n_sets > 0
    assert call(set_rows=[(60, Field.UDP_LENGTH, EmitSource.LENGTH, 0)], su=[]) == -1  # outside hdr
    assert call(set_rows=[(14, 200, EmitSource.VALUE, 0)], su=[]) == -1   # unknown field
    assert call(set_rows=[(14, Field.V4_SOURCE, 7, 0)], su=[]) == -1      # unknown source
    assert call(set_rows=[(14, Field.V4_SOURCE, EmitSource.U32, 0)], su=[]) == -1  # no values
    # ingot_gpu_emit_packets_csum's own
    assert call(n_sums=3) == -1                                        # n_sums > the maximum
    assert call(null_sums=True) == -1                                  # sums NULL, n_sums > 0
    assert call(su=[(2, 34, 14)]) == -1                                # unknown kind
    padded = emit_sums_array([(EmitSum.UDP, 34, 14)])
    padded[0]["_pad"][1] = 1
    assert call(su=padded) == -1                                       # non-zero padding
    assert call(su=[(EmitSum.UDP, 34, 14), (EmitSum.UDP, 34, 14)]) == -1  # two of one kind
    assert call(su=[(EmitSum.UDP, 35, 14)]) == -1                      # odd at
    assert call(su=[(EmitSum.UDP, 34, 13)]) == -1                      # odd l3_at
    assert call(su=[(EmitSum.IPV4, 14, 2)]) == -1                      # IPV4: l3_at != 0
    assert call(su=[(EmitSum.IPV4, 34)]) == -1                         # version nibble != 4
    ihl15 = bytes(hdr[:14]) + bytes([0x4F]) + bytes(hdr[15:])
    assert call(h=ihl15, su=[(EmitSum.IPV4, 14)]) == -1                # at + 4 ihl > hdr_len
    assert call(su=[(EmitSum.UDP, len(hdr) - 6, 14)]) == -1            # at + 8 > hdr_len
    assert call(su=[(EmitSum.UDP, 34, 0)]) == -1                       # version at l3_at
    assert call(su=[(EmitSum.UDP, 32, 14)]) == -1                      # IP header ends past at
    extra = dev_sets + [(14, Field.V4_IHL, EmitSource.VALUE, 5)]
    assert call(set_rows=extra) == -1                                  # setter on a named header
    assert call(h=b"", set_rows=[], su=[(EmitSum.UDP, 0, 0)]) == -1    # hdr_len 0 with sums
    # the device pointers, n > 0
    for name in good:
        assert call(**{name: None}) == -1, name
    # these checks come first even when n == 0
    assert call(n=0, su=[(EmitSum.UDP, 35, 14)]) == -1
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()
    # n == 0 succeeds whatever the device pointers are
    assert call(n=0, **{name: None for name in good}) == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()
    # and the same arguments without the faults are accepted
    assert call() == 0
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    want, _ = model.apply(np.full(512, 0xA5, np.uint8), hdr, sets, sums, arena,
                          so.cpu().numpy().view(np.uint64), sl.cpu().numpy().view(np.uint16),
                          ps.cpu().numpy().view(np.uint32), np.array([0, 100, 200, 300], np.uint64))
    _same(got, want)
