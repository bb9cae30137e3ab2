"""The chunked checksum definition (tests/csum_read_model.py) without a GPU:
against the contiguous definition over cut generator frames, against a
byte-wise receiver that shares no code with either model, the one-chunk rule
by hand, and the C ABI of the two calls."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
from ingot_amd import _lib
from ingot_amd.abi import CSUM_L3, CSUM_L4, Chain, GenProfile
from ingot_amd.hostgen import gen_frames_host
from tests import csum_frames as cf
from tests import csum_model
from tests import csum_read_cases as cases
from tests import csum_read_model as model

ROOT = Path(__file__).resolve().parent.parent
NONE, OK, BAD, ZERO, SHORT, FRAGMENT = range(6)
BOTH = CSUM_L3 | CSUM_L4
PAIRS = [("MIXED", Chain.GenericUlp), ("VLAN_V6EH", Chain.VlanUlp),
         ("GENEVE", Chain.GeneveOverV6Tunnel), ("MIXED", Chain.UdpParser)]
N = 2_000


def prepared(profile, chain, seed):
    """Generator frames with every record's checksums filled valid by
    csum_model.fill, then a third broken (a flipped segment byte) ->
    (arena, off, lens, recs, chunked packets)."""
    arena, off, lens = gen_frames_host(GenProfile[profile], N, seed=seed, slack=64)
    arena = arena.copy()
    recs = oracle.parse_batch(arena, off, lens, chain)
    csum_model.fill(arena, off, lens, recs)
    for i in range(0, N, 3):
        if int(recs["status"][i]) == 0 and int(recs["l4_off"][i]) < int(lens[i]):
            arena[int(off[i]) + int(recs["l4_off"][i])] ^= 0x10
    rng = np.random.default_rng(seed + 1)
    frames = cases.frames_of(arena, off, lens)
    packets = [cases.cut(f, recs[i], rng) for i, f in enumerate(frames)]
    return arena, off, lens, recs, packets


@pytest.fixture(scope="module", params=PAIRS, ids=[f"{p}-{c.name}" for p, c in PAIRS])
def traffic(request):
    profile, chain = request.param
    return (chain,) + prepared(profile, chain, seed=900 + int(chain))


def test_chunked_rows_equal_the_contiguous_rows(traffic):
    """Cut by `cut`, parse_read gives the contiguous records, the chunked
    model's rows equal csum_model.verify's over the same frames, and no
    summed packet is lost to the one-chunk rule."""
    chain, arena, off, lens, recs, packets = traffic
    tables = cases.place(packets, misalign=range(16), gap=2)
    r_rec, _, _ = oracle.parse_read_batch(*tables, chain)
    assert r_rec.tobytes() == recs.tobytes()
    assert any(len(p) > 2 for p in packets) and any(b"" in p for p in packets)
    for what in (BOTH, CSUM_L3, CSUM_L4):
        want = csum_model.verify(arena, off, lens, recs, what)
        assert model.verify(tables, r_rec, what).tobytes() == want.tobytes(), what
        assert model.verify(packets, r_rec, what).tobytes() == want.tobytes(), what
    want = csum_model.verify(arena, off, lens, recs)
    summed = np.isin(want["l4_state"], (OK, BAD, ZERO))
    got = model.verify(tables, r_rec)
    assert summed.sum() > N // 3 and np.isin(got["l4_state"][summed], (OK, BAD, ZERO)).all()
    assert (want["l4_state"] == BAD).sum() > N // 10


# ---------------------------------------------------------------------------
# A receiver: the chunks concatenated, a plain RFC 1071 byte loop with the
# pseudo-header.  Shares no code with the models.
# ---------------------------------------------------------------------------
def rx_sum(data: bytes) -> int:
    acc = 0
    for k, b in enumerate(data):
        acc += b << 8 if k % 2 == 0 else b
    while acc >> 16:
        acc = (acc & 0xFFFF) + (acc >> 16)
    return acc


def rx_l4(f: bytes, rec) -> int:
    o3, o4, k4 = int(rec["l3_off"]), int(rec["l4_off"]), int(rec["l4_kind"])
    if int(rec["l3_kind"]) == 1:
        end = o3 + f[o3 + 2] * 256 + f[o3 + 3]
        n = end - o4
        pseudo = f[o3 + 12:o3 + 20] + bytes([0, f[o3 + 9], n >> 8, n & 255])
    else:
        end = o3 + 40 + f[o3 + 4] * 256 + f[o3 + 5]
        n = end - o4
        pseudo = f[o3 + 8:o3 + 40] + n.to_bytes(4, "big") + bytes([0, 0, 0, int(rec["l4_proto"])])
    if k4 == 3:  # ICMPv4: no pseudo-header
        pseudo = b""
    return rx_sum(pseudo + f[o4:end])


def test_fill_passes_a_bytewise_receiver(traffic):
    chain, arena, off, lens, recs, packets = traffic
    arena2, seg_off, seg_len, pkt_seg = cases.place(packets, misalign=range(5, 21), gap=1)
    before = arena2.copy()
    rows = model.fill((arena2, seg_off, seg_len, pkt_seg), recs)
    assert (rows["l4_state"] == OK).sum() > N // 3
    changed = np.nonzero(arena2 != before)[0]
    assert 0 < len(changed) <= 2 * ((rows["l3_state"] == OK).sum() + (rows["l4_state"] == OK).sum())
    for i, chunks in enumerate(model.views((arena2, seg_off, seg_len, pkt_seg))):
        f = b"".join(c.tobytes() for c in chunks)
        o3 = int(recs["l3_off"][i])
        if rows["l4_state"][i] == OK:
            assert rx_l4(f, recs[i]) == 0xFFFF, i
        if rows["l3_state"][i] == OK:
            assert rx_sum(f[o3:o3 + max(20, (f[o3] & 15) * 4)]) == 0xFFFF, i
    again = model.verify((arena2, seg_off, seg_len, pkt_seg), recs)
    assert not np.isin(again["l4_state"], (BAD, ZERO)).any()
    assert not (again["l3_state"] == BAD).any()
    assert again.tobytes() == rows.tobytes()


# ---------------------------------------------------------------------------
# the rule, by hand
# ---------------------------------------------------------------------------
def _rec(f, chain=Chain.GenericUlp):
    return oracle.parse_batch(*cf.place([f])[:3], chain)[0]


def _filled(f, rec):
    a = np.frombuffer(f, dtype=np.uint8).copy()
    csum_model.one(a, rec, BOTH, True)
    return a.tobytes()


def test_rule_rows_by_hand():
    """A contiguous record supplied for chunks that cut a header."""
    # IPv4 (options) / TCP: l3_off 14, ihl 7 (28 B), l4_off 42, payload_off 62
    f = cf.frame("v4", cf.TCP, bytes(range(40)), options=bytes([1] * 8))
    rec = _rec(f)
    assert (int(rec["l3_off"]), int(rec["l4_off"]), int(rec["payload_off"])) == (14, 42, 62)
    f = _filled(f, rec)
    whole = model.one([np.frombuffer(f, dtype=np.uint8)], rec, BOTH, False)
    assert whole[:2] == (OK, OK) and whole[4] == 60

    def row(cuts):
        return model.one([np.frombuffer(c, dtype=np.uint8) for c in cases.cut_at(f, cuts)], rec,
                         BOTH, False)

    assert row([14, 42, 62, 70]) == whole                 # cuts at the layer edges only
    assert row([50]) == (OK, NONE, whole[2], 0, 0)        # inside the TCP header
    assert row([40]) == (NONE, NONE, 0, 0, 0)             # inside the IPv4 options: L3 too,
    assert row([36]) == (NONE, NONE, 0, 0, 0)             # and L4 ([l3_off, l4_off) is cut)
    assert row([20]) == (NONE, NONE, 0, 0, 0)             # inside the fixed 20 B
    assert row([62, 63, 63, 90]) == whole                 # payload cuts, an empty chunk
    # IPv6 + a destination-options header / UDP: cut between the fixed header and the EH
    g = cf.frame("v6", cf.UDP, bytes(range(33)), ext=((60, bytes(6)),))
    rec6 = _rec(g)
    assert (int(rec6["l3_off"]), int(rec6["l4_off"]), int(rec6["n_v6ext"])) == (14, 62, 1)
    g = _filled(g, rec6)
    whole6 = model.one([np.frombuffer(g, dtype=np.uint8)], rec6, BOTH, False)
    assert whole6[:2] == (NONE, OK)
    cut6 = [np.frombuffer(c, dtype=np.uint8) for c in cases.cut_at(g, [54])]
    assert model.one(cut6, rec6, BOTH, False) == (NONE, NONE, 0, 0, 0)
    ok6 = [np.frombuffer(c, dtype=np.uint8) for c in cases.cut_at(g, [14, 62, 70, 71])]
    assert model.one(ok6, rec6, BOTH, False) == whole6
    # more than 65,535 bytes of chunks: later bytes are not seen
    big = cf.frame("v4", cf.UDP, b"\xff" * (65535 - 42))
    rb = _rec(big)
    big = _filled(big, rb)
    chunks = [np.frombuffer(c, dtype=np.uint8) for c in cases.cut_at(big, [42, 1001])]
    want = model.one(chunks, rb, BOTH, False)
    assert want[:2] == (OK, OK) and want[4] == 65535 - 34
    assert model.one(chunks + [np.full(100, 7, np.uint8)], rb, BOTH, False) == want


def test_fill_maps_fields_back_to_their_chunks():
    f = cf.frame("v4", cf.UDP, bytes(range(1, 30)))
    rec = _rec(f)
    chunks = [bytearray(c) for c in cases.cut_at(f, [14, 34, 42, 50])]
    rows = model.fill([chunks], [rec])
    assert tuple(rows[0])[:2] == (OK, OK)
    assert b"".join(chunks) == _filled(f, rec)
    assert [len(c) for c in chunks] == [14, 20, 8, 8, len(f) - 50]
    with pytest.raises(ValueError):
        model.verify([chunks], [rec], what=4)


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
NAMES = ("ingot_gpu_checksum_verify_read", "ingot_gpu_checksum_fill_read")


@pytest.fixture(scope="module")
def lib():
    from ingot_amd.build import build

    build()
    return _lib.load()


def test_the_two_calls_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "ingot_gpu.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in exported and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == 10
    assert lib.ingot_gpu_abi_version() == 4
    assert re.search(r"^#define INGOT_GPU_ABI_VERSION 4$", header, flags=re.M)


def test_argument_validation_without_gpu(lib):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(1)
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn(null, None, None, None, None, 10, None, 3, None, None) == -1  # NULL context
        for what in (0, 4, 7, 0x80000001):
            assert fn(fake, None, None, None, None, 10, None, what, None, None) == -1, what
