"""tests/emit_read_model.py (the definition of ingot_gpu_emit_packets_read)
against what is already pinned: the contiguous model over the same frames,
the payload rule worked by hand, an oracle parse + checksum verify of what it
emits, and the real library's argument check.  No GPU."""
import numpy as np
import pytest

import oracle
from ingot_amd import CSUM_L3, CSUM_L4, Chain, GenProfile, _lib
from ingot_amd.hostgen import gen_frames_host
from tests import csum_model
from tests import csum_read_cases as chunks
from tests import emit_csum_cases as cases
from tests import emit_csum_model
from tests import emit_read_model as model

OK = int(csum_model.OK)


def _contiguous(hdr, sets, sums, src, off, lens, dst_off, size):
    want = np.full(size, 0xA5, np.uint8)
    oracle.emit_batch(hdr, sets, src, off, lens, want, dst_off)
    return emit_csum_model.apply(want, hdr, sums, dst_off, lens, sets)


def _chunked(hdr, sets, sums, tables, dst_off, size, frm=None, take=None):
    got = np.full(size, 0xA5, np.uint8)
    return model.apply(got, hdr, sets, sums, *tables, dst_off, frm, take)


@pytest.mark.parametrize("name", cases.STACKS)
def test_one_chunk_is_the_contiguous_model(name):
    """(a) one chunk per packet: the contiguous model's arena byte for byte."""
    rng = np.random.default_rng(1)
    ln = np.asarray(cases.EDGE_LENGTHS, np.uint16)
    n = len(ln)
    src, off = cases.random_source(ln, rng)
    hdr, sets, sums = cases.stack(name, n, rng)
    dst_off, size = cases.pack(ln, len(hdr), rng)
    tables = (src, off, ln, np.arange(n + 1, dtype=np.uint32))
    got, taken = _chunked(hdr, sets, sums, tables, dst_off, size)
    assert (taken == ln).all()
    assert got.tobytes() == _contiguous(hdr, sets, sums, src, off, ln, dst_off, size).tobytes()


def test_cut_invariance():
    """(b) the arena does not depend on where the frames are cut, nor on where
    the chunks lie."""
    rng = np.random.default_rng(2)
    n = 64
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=7, slack=64)
    recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    frames = chunks.frames_of(arena, off, lens)
    hdr, sets, sums = cases.stack("opte", n, rng)
    dst_off, size = cases.pack(lens, len(hdr), rng)
    want = _contiguous(hdr, sets, sums, arena, off, lens, dst_off, size)
    for mis in (0, (1, 7, 15, 8, 3)):
        packets = [chunks.cut(f, r, rng) for f, r in zip(frames, recs)]
        got, taken = _chunked(hdr, sets, sums, chunks.place(packets, misalign=mis), dst_off, size)
        assert (taken == lens).all()
        assert got.tobytes() == want.tobytes(), mis
    # every cut offset of a 40-byte payload, single and doubled (an empty chunk)
    pay = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    packets = [chunks.cut_at(pay, [c]) for c in range(41)]
    packets += [chunks.cut_at(pay, [c, c]) for c in range(41)]
    packets += [chunks.cut_at(pay, [c, c + 1]) for c in range(40)]
    m = len(packets)
    hdr, sets, sums = cases.stack("geneve_v4", m, rng)
    ln = np.full(m, 40, np.uint16)
    src = np.frombuffer(pay * m + bytes(64), np.uint8)
    soff = (np.arange(m) * 40).astype(np.uint64)
    dst_off, size = cases.pack(ln, len(hdr), rng)
    want = _contiguous(hdr, sets, sums, src, soff, ln, dst_off, size)
    got, taken = _chunked(hdr, sets, sums, chunks.place(packets, misalign=tuple(range(16))),
                          dst_off, size)
    assert (taken == 40).all()
    assert got.tobytes() == want.tobytes()


def test_clamp_rows_by_hand():
    """(c) the payload rule, row by row."""
    a = bytes(range(10))            # logical bytes 0..9 in chunks of 4, 0, 6
    packets = [[a[:4], b"", a[4:]]] * 6
    arena, seg_off, seg_len, pkt_seg = chunks.place(packets, misalign=(5, 9, 14))
    frm = np.array([10, 11, 3, 3, 0, 9], np.uint16)     # = L, > L, .., .., 0, last byte
    take = np.array([5, 5, 0, 100, 10, 65535], np.uint16)  # .., .., 0, > L - from, = L, > 1
    src, off, lens = model.linearise(arena, seg_off, seg_len, pkt_seg, frm, take)
    assert lens.tolist() == [0, 0, 0, 7, 10, 1]
    rows = [src[int(o):int(o) + int(t)].tobytes() for o, t in zip(off, lens)]
    assert rows == [b"", b"", b"", a[3:], a, a[9:]]
    # NULL arrays: from 0, to the end
    src, off, lens = model.linearise(arena, seg_off, seg_len, pkt_seg)
    assert lens.tolist() == [10] * 6 and src[:60].tobytes() == a * 6
    src, off, lens = model.linearise(arena, seg_off, seg_len, pkt_seg, frm=frm)
    assert lens.tolist() == [0, 0, 7, 7, 10, 1]

    # chunks totalling 65,536 and 70,000 bytes: the last byte(s) are never seen
    big = np.random.default_rng(3).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    packets = [[big[:40000], big[40000:65536]],
               [big[:30000], big[30000:60000], big[60000:70000]],
               [],                                   # no chunks
               [big[:65535], b"", big[65535:65540]]]  # the cut falls on a chunk boundary
    arena, seg_off, seg_len, pkt_seg = chunks.place(packets, misalign=(3, 12))
    src, off, lens = model.linearise(arena, seg_off, seg_len, pkt_seg)
    assert lens.tolist() == [65535, 65535, 0, 65535]
    for i in (0, 1, 3):
        assert src[int(off[i]):int(off[i]) + 65535].tobytes() == big[:65535]
    frm = np.array([65535, 65000, 0, 65534], np.uint16)
    take = np.array([9, 65535, 9, 65535], np.uint16)
    src, off, lens = model.linearise(arena, seg_off, seg_len, pkt_seg, frm, take)
    assert lens.tolist() == [0, 535, 0, 1]
    assert src[int(off[1]):int(off[1]) + 535].tobytes() == big[65000:65535]
    assert src[int(off[3])] == big[65534]

    # reversed bounds count as no chunks; the neighbours are unaffected
    rev = np.array([0, 3, 1, 3], np.uint32)  # packet 1: chunks 3 .. 1
    arena, seg_off, seg_len, _ = chunks.place([[a[:4], a[4:6], a[6:]]], misalign=1)
    src, off, lens = model.linearise(arena, seg_off, seg_len, rev)
    assert lens.tolist() == [10, 0, 6]
    assert src[:16].tobytes() == a + a[4:]


@pytest.mark.parametrize("name", ["opte", "geneve_v4"])
def test_receiver_accepts(name):
    """(d) what the model emits from chunks parses Ok and its outer sums verify."""
    rng = np.random.default_rng(4)
    n = 300
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=11, slack=64)
    recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    packets = [chunks.cut(f, r, rng) for f, r in zip(chunks.frames_of(arena, off, lens), recs)]
    hdr, sets, sums = cases.stack(name, n, rng)
    dst_off, size = cases.pack(lens, len(hdr), rng)
    got, taken = _chunked(hdr, sets, sums, chunks.place(packets, misalign=(2, 13, 6)), dst_off,
                          size)
    tl = (taken.astype(np.int64) + len(hdr)).astype(np.uint16)
    out = oracle.parse_batch(got, dst_off, tl, Chain.UdpParser)
    assert (out["status"] == 0).all()
    rows = csum_model.verify(got, dst_off, tl, out, CSUM_L3 | CSUM_L4)
    assert (rows["l4_state"] == OK).all()
    if name == "geneve_v4":
        assert (rows["l3_state"] == OK).all()


def test_null_context_is_einval():
    """(e) through the real library: every check comes before device work."""
    from ingot_amd.build import build

    build()
    lib = _lib.load()
    assert lib.ingot_gpu_emit_packets_read(None, None, 0, None, 0, None, 0, None, None, None,
                                           None, None, None, 4, None, None, None, None) == -1
