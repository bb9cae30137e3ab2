"""ingot_gpu_parse_read_modify / ingot_gpu_parse_read_modify_csum on the device
against the definition (tests/modify_read_model.py): after every call the
WHOLE arena equals the model's arena (gaps, neighbours and payload chunks
included), the records equal oracle.parse_read_batch's and d_chunk the
oracle's.  Needs an MI355X: `pytest -m gpu`."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import ingot_amd
import oracle
from ingot_amd import (CSUM_DTYPE, CSUM_L3, CSUM_L4, Chain, EditOp, EmitSource, Field, GenProfile,
                       emit as E)
from ingot_amd.hostgen import gen_frames_host
from tests import csum_frames as cf
from tests import csum_model
from tests import csum_read_cases as cases
from tests import csum_sweep_cases as sc
from tests import modify_read_cases as mc
from tests import modify_read_model as model

pytestmark = pytest.mark.gpu

TUN = Chain.GeneveOverV6Tunnel
F, SET, ADD, SUB, XOR = Field, EditOp.SET, EditOp.ADD, EditOp.SUB, EditOp.XOR
BOTH = CSUM_L3 | CSUM_L4
OK = 1  # ingot_csum state
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


def _dev(torch, a):
    """A numpy array on the device (unsigned tables as the signed view of the same bits)."""
    a = np.ascontiguousarray(a)
    if a.dtype.fields:
        a = a.view(np.uint8)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
              np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()


class Device:
    """A batch's tables on the device once; run() restores the arena, makes the
    call and returns (arena, records, chunk) as numpy."""

    def __init__(self, ctx, torch, tables, chain):
        self.ctx, self.torch, self.tables, self.chain = ctx, torch, tables, chain
        self.n = len(tables[3]) - 1
        self.pristine = _dev(torch, tables[0])
        self.arena = self.pristine.clone()
        self.tab = [_dev(torch, x) for x in tables[1:]]
        self.out = torch.zeros((self.n, 16), dtype=torch.uint8, device="cuda")
        self.chunk = torch.zeros(self.n, dtype=torch.int16, device="cuda")
        self.parsed = model.parse(tables, chain)

    def run(self, edits, what):
        self.arena.copy_(self.pristine)
        self.out.fill_(0xEE)
        self.chunk.fill_(-1)
        self.ctx.parse_read_modify(self.arena, *self.tab, self.chain, edits, csum=what,
                                   out=self.out, chunk=self.chunk)
        return (self.arena.cpu().numpy(), self.out.cpu().numpy(),
                self.chunk.cpu().numpy().view(np.uint16))

    def check(self, edits, what, tag=""):
        """The call against the model: whole arena, records, chunk indices.
        Returns the model's arena."""
        want, recs, w_chunk = model.apply(self.tables, self.chain, edits, what, parsed=self.parsed)
        got, g_rec, g_chunk = self.run(edits, what)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (tag, what, edits, bad[:10], got[bad[:10]], want[bad[:10]],
                               self.tables[0][bad[:10]])
        assert g_rec.tobytes() == recs.tobytes(), (tag, "records")
        assert (g_chunk == w_chunk).all(), (tag, "chunk")
        return want


def check(ctx, torch, tables, chain, edits, what, tag=""):
    return Device(ctx, torch, tables, chain).check(edits, what, tag)


def place_packed(packets, first: int = 16, fill: int = 0xA5):
    """Every chunk right after the previous one: no byte between them."""
    seg_off, seg_len, pkt_seg, o = [], [], [0], first
    for chunks in packets:
        for ch in chunks:
            seg_off.append(o)
            seg_len.append(len(ch))
            o += len(ch)
        pkt_seg.append(len(seg_off))
    seg_off.append(o)
    seg_len.append(0)
    arena = np.full((o + 64 + 15) // 16 * 16, fill, dtype=np.uint8)
    arena[first:o] = np.frombuffer(b"".join(b"".join(p) for p in packets), np.uint8)
    return (arena, np.array(seg_off, np.uint64), np.array(seg_len, np.uint16),
            np.array(pkt_seg, np.uint32))


def place_descending(packets, gap: int = 3, misalign=(7, 2, 13, 8)):
    """The batch's chunks at descending addresses: chunk c + 1 lies below
    chunk c, so a packet's header chunks come after its payload chunk."""
    flat = [ch for p in packets for ch in p]
    arena, so, sl, _ = cases.place([[ch] for ch in reversed(flat)], misalign=list(misalign),
                                   gap=gap)
    so = np.r_[so[:-1][::-1], so[-1:]]
    sl = np.r_[sl[:-1][::-1], sl[-1:]]
    ps = np.cumsum([0] + [len(p) for p in packets]).astype(np.uint32)
    return arena, so, sl, ps


@lru_cache(maxsize=None)
def header_chunked(chain, prepared: bool = False):
    """tests/csum_sweep_cases.py's small batch of `chain` cut one header per
    chunk (eth | vlan | vlan | l3 | l4 | payload; the tunnel: 8 chunks) ->
    the packets: headers in chunks past the four prefetched descriptors and in
    a packet's last chunk (frames without payload)."""
    b = sc.batch(chain, "indexed", prepared)
    if prepared:
        b = sc.other_repr(b, chain)[0]
    recs = oracle.parse_batch(b.arena, b.starts, b.lengths, chain)
    gf = oracle.geneve_fields_batch(b.arena, b.starts, b.lengths)["outer"] if chain == TUN else None
    packets = []
    for i, f in enumerate(cases.frames_of(b.arena, b.starts, b.lengths)):
        cuts = mc.header_cuts(chain, recs[i], None if gf is None else gf[i],
                              int(recs["n_vlan"][i]) if chain == Chain.VlanUlp else 0)
        packets.append(cases.cut_at(f, [c for c in cuts if c <= len(f)]))
    assert max(len(p) for p in packets) >= (8 if chain == TUN else 5 if chain == Chain.VlanUlp
                                            else 4)
    return packets


# ---------------------------------------------------------------------------
# 1. golden rewrite vectors
# ---------------------------------------------------------------------------
def test_golden_rewrite_vectors(ctx, torch, kats):
    """tests/test_modify.py's KATs cut at every subset of {14, l3_off, l4_off,
    payload_off}, every chunk at every misalignment 0..15, gaps 0 and 3: where
    the chunked record is the contiguous one, the logical frame afterwards is
    the stored `after`."""
    compared = 0
    for kat in kats["modify_kats"]:
        chain = Chain[kat["chain"]]
        f = bytes.fromhex(kat["frame"])
        edits = [(e[0], Field[e[1]], EditOp[e[2]], e[3], *e[4:]) for e in kat["edits"]]
        crec = oracle.parse_batch(*cf.place([f])[:3], chain)[0]
        edges = sorted({14, int(crec["l3_off"]), int(crec["l4_off"]), int(crec["payload_off"])})
        edges = [e for e in edges if 0 < e < len(f)]
        subsets = [[e for k, e in enumerate(edges) if m >> k & 1] for m in range(1 << len(edges))]
        packets, mis = [], []
        for cuts in subsets:
            for m in range(16):
                packets.append(cases.cut_at(f, cuts))
                mis += [(m + 5 * k) % 16 for k in range(len(cuts) + 1)]
                mis[-len(cuts) - 1] = m
        for gap in (0, 3):
            tables = cases.place(packets, misalign=mis, gap=gap)
            d = Device(ctx, torch, tables, chain)
            want = d.check(edits, 0, kat["name"])
            for i in range(d.n):
                if d.parsed[0][i].tobytes() == crec.tobytes():
                    assert mc.logical(want, tables, i).hex() == kat["after"], (kat["name"], i)
                    compared += 1
    assert compared > 7 * 16 * 2


# ---------------------------------------------------------------------------
# 2. single-edit sweep
# ---------------------------------------------------------------------------
SWEEP = [(c, w) for c in sc.CHAINS for w in sc.WHATS[c]]


@pytest.mark.parametrize("chain,what", SWEEP, ids=[f"{c.name}-{w}" for c, w in SWEEP])
def test_single_edit_sweep(ctx, torch, chain, what):
    """Every field x layer x op on the header-per-chunk batch, with `what` and
    (every third case) without: two values where the layer can hold the
    field (the tunnel: one), one where it cannot (nothing may be written
    then)."""
    tables = cases.place(header_chunked(chain), misalign=[1, 14, 6, 11, 0, 9, 3], gap=2)
    d = Device(ctx, torch, tables, chain)
    assert (d.parsed[0]["status"] == 0).sum() >= d.n // 3
    moved = k = 0
    for field in Field:
        for layer, index in sc.LAYERS[chain]:
            fits = sc.applies(chain, layer, field)
            vals = sc.sweep_values(field, layer)
            for j, op in enumerate(EditOp):
                # (the tunnel's seven layers: one value each)
                two = fits and chain != TUN
                for v in ((vals[j % 4], vals[(j + 2) % 4]) if two else (vals[j % 4],)):
                    e = (layer, field, op, v, index)
                    k += 1
                    w = 0 if field in sc.REFUSED or k % 3 == 0 else what
                    want = d.check([e], w, sc.tag(chain, "header chunks", e, w))
                    changed = (want != tables[0]).any()
                    assert fits or not changed
                    moved += int(changed)
    assert moved > 150, moved


# ---------------------------------------------------------------------------
# 3. dependent and twice-edited lists
# ---------------------------------------------------------------------------
def _csum_then_covered(chain):
    l3 = sc.L3_LAYER[chain]
    l4 = l3 + 1
    return [(l3, F.V4_CHECKSUM, SET, 0x1234), (l3, F.V4_HOP_LIMIT, SUB, 1),
            (l4, F.UDP_CHECKSUM, SET, 0xBEEF), (l4, F.UDP_SOURCE, ADD, 3),
            (l4, F.TCP_CHECKSUM, SET, 0xFFFF), (l4, F.TCP_SEQUENCE, XOR, 0x01020304),
            (l4, F.ICMP_CHECKSUM, SET, 0), (l4, F.ICMP_CODE, ADD, 1),
            (l3, F.V4_SOURCE, SET, 0xC0A80A0A)]


@chains
@pytest.mark.parametrize("placement", ["inside the window", "outside the window", "descending"])
def test_dependent_and_twice_edited_lists(ctx, torch, chain, placement):
    """The named lists of tests/csum_sweep_cases.py and a list that SETs a
    checksum field and then edits a covered field: (i) gap 0, later chunks
    inside chunk 0's staged window, (ii) gap >= 200, outside it, (iii) chunks
    at descending addresses, the header chunks after the payload chunk."""
    lists = sc.dependent_lists(chain) + [("csum set, then covered", _csum_then_covered(chain), False)]
    devs = {}
    for prepared in (False, True):
        packets = header_chunked(chain, prepared)
        if placement == "inside the window":
            tables = place_packed(packets, first=19)
        elif placement == "outside the window":
            tables = cases.place(packets, misalign=[4, 15, 9], gap=200)
        else:
            tables = place_descending(packets)
        devs[prepared] = Device(ctx, torch, tables, chain)
    if placement == "descending":
        so, ps = devs[False].tables[1], devs[False].tables[3]
        assert all(so[k + 1] < so[k] for k in range(int(ps[0]), int(ps[1]) - 1))
    moved = 0
    for name, edits, prepared in lists:
        d = devs[prepared]
        for what in (sc.WHATS[chain][-1], 0):
            want = d.check(edits, what, name)
            moved += int((want != d.tables[0]).any())
    assert moved > len(lists)


# ---------------------------------------------------------------------------
# 4. neighbours
# ---------------------------------------------------------------------------
def test_neighbours_stay_intact(ctx, torch):
    """257 packets back to back without a byte between chunks, all edited at
    the last bytes of a chunk (ETH_ETHERTYPE, cut at 14), the first byte of a
    chunk (V4_VERSION / V6_VERSION) and the L4 checksum field right before a
    cut at payload_off: the filler and every neighbour's bytes are intact."""
    kinds = [("v4", cf.UDP), ("v6", cf.TCP), ("v4", cf.ICMP4), ("v6", cf.UDP), ("v4", cf.TCP),
             ("v6", cf.ICMP6)]
    frames = [cf.frame(*kinds[i % 6], bytes((i + 3 * j) & 0xFF for j in range(1 + i % 23)))
              for i in range(257)]
    arena, off, lens = cf.place(frames)
    recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    csum_model.fill(arena, off, lens, recs)
    packets = [cases.cut_at(f, [14, int(r["payload_off"])])
               for f, r in zip(cases.frames_of(arena, off, lens), recs)]
    edits = [(0, F.ETH_ETHERTYPE, XOR, 0xFFFF), (1, F.V4_VERSION, SET, 0xF),
             (1, F.V6_VERSION, SET, 0xF), (2, F.UDP_CHECKSUM, XOR, 0xFFFF),
             (2, F.TCP_CHECKSUM, ADD, 0x0101), (2, F.ICMP_CHECKSUM, SUB, 1),
             (1, F.V4_HOP_LIMIT, SUB, 1), (2, F.UDP_SOURCE, ADD, 1)]
    for first in (16, 21):
        tables = place_packed(packets, first=first)
        d = Device(ctx, torch, tables, Chain.GenericUlp)
        assert (d.parsed[0]["status"] == 0).all()
        for what in (0, BOTH):
            want = d.check(edits, what, f"neighbours@{first}")
            assert all(mc.logical(want, tables, i) != mc.logical(tables[0], tables, i)
                       for i in range(257))


# ---------------------------------------------------------------------------
# 5. batch edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_edges(ctx, torch, n):
    """Batches that end inside a wave, at its edge and just past it; 1-9
    chunks per packet, empty chunks after the headers and between payload
    pieces."""
    rng = np.random.default_rng(n)
    kinds = [("v4", cf.UDP), ("v6", cf.TCP), ("v4", cf.ICMP4), ("v6", cf.UDP), ("v4", cf.TCP),
             ("v6", cf.ICMP6)]
    frames = [cf.frame(*kinds[i % 6], rng.integers(0, 256, int(rng.integers(0, 200)),
                                                   dtype=np.uint8).tobytes()) for i in range(n)]
    arena, off, lens = cf.place(frames)
    recs = oracle.parse_batch(arena, off, lens, Chain.GenericUlp)
    csum_model.fill(arena, off, lens, recs)
    packets = []
    for i, f in enumerate(cases.frames_of(arena, off, lens)):
        p = cases.cut(f, recs[i], rng)
        pay = int(recs["payload_off"][i])
        holds = next(k for k in range(len(p)) if sum(len(c) for c in p[:k + 1]) >= pay)
        if i % 3 == 0:  # empty chunks between the payload pieces and at the end
            for at in sorted({int(x) for x in rng.integers(holds + 1, len(p) + 1, 2)}, reverse=True):
                p.insert(at, b"")
        packets.append(p[:9])
    if n == 257:
        assert {len(p) for p in packets} >= set(range(1, 8)) and any(b"" in p for p in packets)
    tables = cases.place(packets, misalign=list(range(16)) + [3, 9, 14], gap=2)
    edits, what = mc.nat_list(Chain.GenericUlp)
    d = Device(ctx, torch, tables, Chain.GenericUlp)
    for w in (what, 0):
        d.check(edits, w, f"n={n}")
    assert (d.parsed[0]["status"] == 0).sum() >= (n + 1) // 2


# ---------------------------------------------------------------------------
# 6. packets that are not Ok
# ---------------------------------------------------------------------------
def test_packets_that_are_not_ok_keep_every_byte(ctx, torch):
    from ingot_amd import ParseError

    arena, off, lens, packets = mc.cut_set("ADVERSARIAL", Chain.GenericUlp, "split", 5_000)
    g = cf.frame("v6", cf.UDP, bytes(range(33)), ext=((60, bytes(6)),))
    for i in range(7, len(packets), 50):
        packets[i] = []                      # no chunks
    packets[100] = cases.cut_at(g, [54])     # IPv6 cut after the fixed header: Unwanted
    packets[101] = cases.cut_at(g, [14, 62])  # the same frame, Ok
    tables = cases.place(packets, misalign=list(range(16)) + [1], gap=2)
    for chain in (Chain.GenericUlp, Chain.VlanUlp):
        d = Device(ctx, torch, tables, chain)
        recs = d.parsed[0]
        assert (recs["status"] == ParseError.StraddledHeader).sum() > 100
        assert int(recs["status"][100]) == ParseError.Unwanted and int(recs["status"][101]) == 0
        edits, what = mc.nat_list(chain)
        edits = edits + [(0, F.ETH_ETHERTYPE, XOR, 0x0101)]
        for w in (what, 0):
            want = d.check(edits, w, chain.name)
            for i in np.nonzero(recs["status"] != 0)[0]:
                assert mc.logical(want, tables, i) == mc.logical(tables[0], tables, i), i
            ok = np.nonzero(recs["status"] == 0)[0]
            assert len(ok) > 100
            assert all(mc.logical(want, tables, i) != mc.logical(tables[0], tables, i) for i in ok)


# ---------------------------------------------------------------------------
# 7. generator traffic
# ---------------------------------------------------------------------------
GEN_CASES = [("MIXED", Chain.GenericUlp), ("VLAN_V6EH", Chain.VlanUlp), ("GENEVE", TUN),
             ("MIXED", Chain.UdpParser)]


def _rows(t):
    return t.cpu().numpy().view(CSUM_DTYPE).reshape(-1)


@pytest.mark.parametrize("profile,chain", GEN_CASES, ids=[f"{p}-{c.name}" for p, c in GEN_CASES])
def test_generator_traffic_nat(ctx, torch, profile, chain):
    """5,000 generator frames with valid sums, cut by csum_read_cases.cut, the
    NAT list with the sums kept right: the model's arena, and
    checksum_verify_read afterwards reports OK for every layer that was OK
    before (the tunnel: the outer UDP sum too, under a UdpParser parse_read)."""
    n = 5_000
    arena, off, lens = gen_frames_host(GenProfile[profile], n, seed=4343, slack=64)
    arena = arena.copy()
    fill_chain = Chain.GenericUlp if chain == Chain.UdpParser else chain
    crecs = oracle.parse_batch(arena, off, lens, fill_chain)
    csum_model.fill(arena, off, lens, crecs)
    if chain == TUN:
        csum_model.fill(arena, off, lens, oracle.parse_batch(arena, off, lens, Chain.UdpParser),
                        what=CSUM_L4)
    rng = np.random.default_rng(17)
    packets = [cases.cut(f, crecs[i], rng)
               for i, f in enumerate(cases.frames_of(arena, off, lens))]
    tables = cases.place(packets, misalign=list(range(16)) + [5, 11, 2], gap=1)
    edits, what = mc.nat_list(chain)
    d = Device(ctx, torch, tables, chain)
    views = [(chain, BOTH)] + ([(Chain.UdpParser, CSUM_L4)] if chain == TUN else [])
    before = []
    for c, w in views:
        rec, _ = ctx.parse_read(d.pristine, *d.tab, c)
        before.append(_rows(ctx.checksum_verify_read(d.pristine, *d.tab, rec, w)))
    want = d.check(edits, what, profile)
    assert (want != tables[0]).sum() > n
    for (c, w), b in zip(views, before):
        rec, _ = ctx.parse_read(d.arena, *d.tab, c)
        after = _rows(ctx.checksum_verify_read(d.arena, *d.tab, rec, w))
        for k in ("l3_state", "l4_state"):
            was = b[k] == OK
            assert was.sum() > 500 or k == "l3_state"
            assert (after[k][was] == OK).all(), (c, k, np.nonzero(after[k][was] != OK)[0][:5])


# ---------------------------------------------------------------------------
# 8. one chunk per packet: device against device
# ---------------------------------------------------------------------------
@chains
def test_one_chunk_per_packet_equals_parse_modify(ctx, torch, chain):
    b = sc.batch(chain, "indexed")
    tables = mc.single_chunk_tables(b)
    d = Device(ctx, torch, tables, chain)
    d_off, d_len = _dev(torch, b.off), _dev(torch, b.lens)
    lists = [mc.nat_list(chain)[0], dict((n, e) for n, e, _ in sc.dependent_lists(chain))["16 nat"]]
    for edits in lists:
        for what in (0,) + tuple(sc.WHATS[chain]):
            want = d.check(edits, what, "one chunk")
            a = d.pristine.clone()
            recs = torch.zeros((b.n, 16), dtype=torch.uint8, device="cuda")
            ctx.parse_modify(a, d_off, d_len, chain, edits, out=recs, csum=what)
            assert a.cpu().numpy().tobytes() == want.tobytes(), (what, "parse_modify")
            assert recs.cpu().numpy().tobytes() == d.parsed[0].tobytes()
            assert (want != tables[0]).any()


# ---------------------------------------------------------------------------
# 9. the two-chunk encapsulation
# ---------------------------------------------------------------------------
def test_two_chunk_encapsulation_rewrite(ctx, torch):
    """emit_header_blocks writes the Geneve-over-IPv6 stack into slots; packet
    i is (slot i, source frame i), outer sums filled by checksum_fill_read.
    parse_read_modify on the tunnel chain: inner hop limit - 1, VNI SET, what
    = 7; a UdpParser parse_read + checksum_verify_read afterwards reports L4
    OK for every packet."""
    n = 2_000
    arena, off, lens = gen_frames_host(GenProfile.MIXED, n, seed=33, slack=64)
    arena = arena.copy()
    csum_model.fill(arena, off, lens, oracle.parse_batch(arena, off, lens, Chain.GenericUlp))
    hdr = (E.ethernet(bytes.fromhex("a84025777776"), bytes.fromhex("a84025777777"), 0x86DD)
           + E.ipv6(bytes.fromhex("fd000000f70101000000000000000002"),
                    bytes.fromhex("fd000000f70101000000000000000001"), 17, hop_limit=0xF0)
           + E.udp(0xC0DE, 6081, checksum=0) + E.geneve(0x123456, options=E.geneve_opt(0x0129, 0)))
    H, stride = len(hdr), 128
    sets = [(14, Field.V6_PAYLOAD_LEN, EmitSource.LENGTH, -40),
            (54, Field.UDP_LENGTH, EmitSource.LENGTH, 0)]
    base = n * stride
    d_all = torch.full((base + len(arena),), 0xA5, dtype=torch.uint8, device="cuda")
    d_all[base:] = _dev(torch, arena)
    ctx.emit_header_blocks(hdr, sets, _dev(torch, lens), d_all, stride=stride)
    seg_off = np.empty(2 * n + 1, dtype=np.uint64)
    seg_len = np.empty(2 * n + 1, dtype=np.uint16)
    seg_off[0:2 * n:2] = np.arange(n, dtype=np.uint64) * stride
    seg_off[1:2 * n:2] = off + np.uint64(base)
    seg_len[0:2 * n:2] = H
    seg_len[1:2 * n:2] = lens
    seg_off[-1], seg_len[-1] = 0, 0
    pkt_seg = (np.arange(n + 1) * 2).astype(np.uint32)
    d_tab = (_dev(torch, seg_off), _dev(torch, seg_len), _dev(torch, pkt_seg))
    o_rec, _ = ctx.parse_read(d_all, *d_tab, Chain.UdpParser)
    ctx.checksum_fill_read(d_all, *d_tab, o_rec, CSUM_L4)
    filled = _rows(ctx.checksum_verify_read(d_all, *d_tab, o_rec, CSUM_L4))
    assert (filled["l4_state"] == OK).all()
    tables = (d_all.cpu().numpy().copy(), seg_off, seg_len, pkt_seg)
    edits = [(5, F.V4_HOP_LIMIT, SUB, 1), (5, F.V6_HOP_LIMIT, SUB, 1), (3, F.GENEVE_VNI, SET, 0xABCDEF)]
    d = Device(ctx, torch, tables, TUN)
    assert (d.parsed[0]["status"] == 0).sum() > n // 2
    want = d.check(edits, 7, "encapsulation")
    assert (want[:base] != tables[0][:base]).any() and (want[base:] != tables[0][base:]).any()
    o_rec2, _ = ctx.parse_read(d.arena, *d.tab, Chain.UdpParser)
    assert o_rec2.cpu().numpy().tobytes() == o_rec.cpu().numpy().tobytes()
    after = _rows(ctx.checksum_verify_read(d.arena, *d.tab, o_rec2, CSUM_L4))
    assert (after["l4_state"] == OK).all(), np.nonzero(after["l4_state"] != OK)[0][:5]


# ---------------------------------------------------------------------------
# 10. arguments and streams
# ---------------------------------------------------------------------------
def test_argument_errors_write_nothing(ctx, torch):
    lib = ingot_amd._lib.load()
    packets = header_chunked(Chain.GenericUlp)
    tables = cases.place(packets, misalign=[2, 7], gap=1)
    d = Device(ctx, torch, tables, Chain.GenericUlp)
    n = d.n
    e = ingot_amd.abi.edits_array([(1, F.V4_HOP_LIMIT, SUB, 1), (1, F.V6_HOP_LIMIT, SUB, 1)])
    E_, NE = e.ctypes.data_as(ctypes.c_void_p), len(e)
    h, A = ctx._h, d.arena.data_ptr()
    SO, SL, PS = (t.data_ptr() for t in d.tab)
    R, C = d.out.data_ptr(), d.chunk.data_ptr()
    plain, csum = lib.ingot_gpu_parse_read_modify, lib.ingot_gpu_parse_read_modify_csum

    def both(args_plain, want, what=3):
        a = list(args_plain)
        assert plain(*a) == want, a
        assert csum(*a[:9], what, *a[9:]) == want, a

    ok = (h, A, SO, SL, PS, n, 1, E_, NE, R, C, None)

    def swap(**kw):
        names = "h A SO SL PS n chain E NE R C s".split()
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    both(swap(h=None), -1)
    both(swap(chain=99), -1)
    both(swap(chain=-1), -1)
    both(swap(NE=17), -1)
    both(swap(E=None), -1)
    for bad in ((1, 200, 0, 1), (1, int(F.V4_HOP_LIMIT), 9, 1), (3, int(F.V4_HOP_LIMIT), 0, 1)):
        x = ingot_amd.abi.edits_array([(bad[0], bad[1], bad[2], bad[3])])
        both(swap(E=x.ctypes.data_as(ctypes.c_void_p), NE=1), -1)
    for what in (0, 8, 4, 5):  # (4: OUTER_L4 is the tunnel chain's)
        assert csum(*ok[:9], what, *ok[9:]) == -1, what
    for f in sc.REFUSED:
        x = ingot_amd.abi.edits_array([(1, f, SET, 1)])
        assert csum(h, A, SO, SL, PS, n, 1, x.ctypes.data_as(ctypes.c_void_p), 1, 3, R, C,
                    None) == -1, f
        assert plain(h, A, SO, SL, PS, 0, 1, x.ctypes.data_as(ctypes.c_void_p), 1, R, C, None) == 0
    both(swap(A=None), -1)
    both(swap(SO=None), -1)
    both(swap(SL=None), -1)
    both(swap(PS=None), -1)
    both([h, None, None, None, None, 0, 1, E_, NE, None, None, None], 0)  # n == 0
    torch.cuda.synchronize()
    assert d.arena.cpu().numpy().tobytes() == tables[0].tobytes(), "a refused call wrote"
    with pytest.raises(ValueError):
        ctx.parse_read_modify(d.arena, d.tab[0], d.tab[1], d.tab[0], Chain.GenericUlp, [])
    with pytest.raises(ValueError):
        ctx.parse_read_modify(d.arena, d.tab[0], d.tab[1][:3], d.tab[2], Chain.GenericUlp, [])
    both(ok, 0)
    torch.cuda.synchronize()


def test_without_records_on_a_side_stream(ctx, torch):
    """d_out and d_chunk both NULL, on a side stream: the default stream's
    result."""
    arena, off, lens, packets = mc.cut_set("MIXED", Chain.GenericUlp, "cut", 3_000)
    tables = cases.place(packets, misalign=list(range(16)) + [5], gap=1)
    edits, what = mc.nat_list(Chain.GenericUlp)
    d = Device(ctx, torch, tables, Chain.GenericUlp)
    want = d.check(edits, what, "default stream")
    a1 = d.pristine.clone()
    torch.cuda.synchronize()
    lib = ingot_amd._lib.load()
    raw = ctypes.c_void_p()
    lib.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lib.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    assert lib.hipStreamCreateWithFlags(ctypes.byref(raw), 1) == 0  # hipStreamNonBlocking
    side = torch.cuda.ExternalStream(raw.value)
    with torch.cuda.stream(side):
        assert ctx.parse_read_modify(a1, *d.tab, Chain.GenericUlp, edits, csum=what,
                                     stream=side) == (None, None)
    side.synchronize()
    torch.cuda.synchronize()
    assert lib.hipStreamDestroy(raw) == 0
    assert a1.cpu().numpy().tobytes() == want.tobytes()
