"""ingot_gpu_parse_modify_rows on the device: per-packet operands, action
tables behind the row guard, MAC and IPv6 address setters and the fused
checksum update, against the definition (tests/modify_rows_model.py) bit for
bit — the whole arena (gaps and tail filled with 0xA5) and the records."""
import ctypes
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import ingot_amd
from ingot_amd import Chain, EditOp, Field, GenProfile, abi
from ingot_amd.abi import (CSUM_L3, CSUM_L4, CSUM_OUTER_L4, ROW_NONE, TUNE_MAX_BLOCKS,
                           TUNE_PIPELINE, EditBy, EditSource, WideField)
from ingot_amd.hostgen import gen_frames_host
from tests import csum_frames as cf
from tests import modify_rows_cases as cases
from tests import modify_rows_model as rows_model
from tests.modify_rows_cases import col_u16, col_u32

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TUN = Chain.GeneveOverV6Tunnel
SET, ADD, SUB, XOR, OR = EditOp.SET, EditOp.ADD, EditOp.SUB, EditOp.XOR, EditOp.OR
L3_LABEL = {Chain.UdpParser: 1, Chain.GenericUlp: 1, Chain.VlanUlp: 2, TUN: 5}
N_ROWS = 37


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return ingot_amd.Context(0)


def on_gpu(torch, c, arena, off, lens, chain, edits, rows=None, n_rows=0, what=0, stride=0,
           n=None):
    """-> (arena after the call, records), numpy."""
    d_arena = torch.from_numpy(np.array(arena)).cuda()  # (a copy: shared inputs are read-only)
    d_off = None if off is None else torch.from_numpy(off.view(np.int64)).cuda()
    d_len = None if lens is None else torch.from_numpy(lens.view(np.int16)).cuda()
    d_rows = None if rows is None else torch.from_numpy(rows.view(np.int32)).cuda()
    n = len(off) if n is None else n
    recs = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    c.parse_modify_rows(d_arena, d_off, d_len, chain, cases.device_edits(torch, edits),
                        rows=d_rows, n_rows=n_rows, stride=stride, n=n, out=recs, csum=what)
    torch.cuda.synchronize()
    return d_arena.cpu().numpy(), recs.cpu().numpy()


def check(torch, c, arena, off, lens, chain, edits, **kw):
    want, w_rec = rows_model.apply(arena, off, lens, chain, edits, **kw)
    got, recs = on_gpu(torch, c, arena, off, lens, chain, edits, **kw)
    assert recs.tobytes() == w_rec.tobytes()
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, (chain, diff[:10], got[diff[:10]], want[diff[:10]])
    return got, w_rec


@lru_cache(maxsize=None)
def placed(profile, n, seed=91, misalign=3):
    """Generated frames packed back to back from a misaligned start; gaps and
    tail 0xA5."""
    a, o, ln = gen_frames_host(profile, n, seed=seed, slack=64)
    frames = [a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, ln)]
    arena, off, lens = cf.place(frames, misalign=misalign)
    arena.setflags(write=False)
    return arena, off, lens


def mixed_rows(n, seed=5):
    """Valid rows, INGOT_ROW_NONE and n_rows itself."""
    rows = np.random.default_rng(seed).integers(0, N_ROWS, n).astype(np.uint32)
    rows[2::5] = ROW_NONE
    rows[3::11] = N_ROWS
    return rows


def mixed_edits(chain, n, seed=1):
    """VALUE, U16, U32 and BYTES operands, by packet (table `t`, 32-B rows)
    and by row (table `r`); ops other than SET on per-packet operands; UDP's
    source edited twice; a 32-bit operand into a 16-bit field; byte rows at
    odd addresses."""
    t, r = cases.nat_table(n, seed), cases.nat_table(N_ROWS, seed + 100)
    dense = (np.arange(n, dtype=np.uint16) * 3 + 1) % 7  # a dense array: pitch 0
    l3 = L3_LABEL[chain]
    l4 = l3 + 1
    e = [(l3, Field.V4_SOURCE, SET, col_u32(t)), (l4, Field.UDP_SOURCE, SET, col_u16(t)),
         (l4, Field.TCP_SEQUENCE, ADD, ("row", col_u32(r))), (l3, Field.V4_HOP_LIMIT, SUB, 1),
         (l3, Field.V6_HOP_LIMIT, SUB, dense), (l3, WideField.V6_SOURCE, SET, ("row", r[:, 16:32])),
         (l3, WideField.V6_DESTINATION, SET, t[:, 13:29]),
         (0, WideField.ETH_DESTINATION, SET, t[:, 8:14]),
         (0, WideField.ETH_SOURCE, SET, ("row", r[:, 1:7])),
         (l4, Field.UDP_SOURCE, XOR, ("row", col_u16(r, 4))),
         (l4, Field.TCP_DESTINATION, SET, col_u32(t, 20)), (l3, Field.V4_DSCP, OR, col_u16(t, 24)),
         (l4, Field.ICMP_CODE, ADD, col_u16(t, 26))]
    if chain == Chain.VlanUlp:
        e += [(1, Field.VLAN_VID, ADD, col_u16(t, 28), 1), (1, Field.VLAN_PRIORITY, XOR, dense, 0)]
    if chain == TUN:
        e = e[:11] + [(1, WideField.V6_SOURCE, SET, t[:, 16:32]),
                      (4, WideField.ETH_SOURCE, SET, ("row", r[:, 20:26])),
                      (3, Field.GENEVE_VNI, SET, col_u32(t, 0)),
                      (2, Field.UDP_SOURCE, XOR, col_u16(t, 30)),
                      (1, WideField.V6_DESTINATION, SET, ("row", r[:, 7:23]))]
    assert len(e) <= abi.MAX_EDITS
    return e


# ---------------------------------------------------------------------------
# Tile edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tile_edges(ctx, torch, n):
    arena, off, lens = placed(GenProfile.MIXED, n)
    got, _ = check(torch, ctx, arena, off, lens, Chain.GenericUlp, mixed_edits(Chain.GenericUlp, n),
                   rows=mixed_rows(n), n_rows=N_ROWS, what=CSUM_L3 | CSUM_L4)
    assert n == 1 or (got != arena).any()


def test_grid_stride_later_trips(torch):
    """4,099 frames on one block: every wave's tile loop takes later trips."""
    n = 4099
    c = ingot_amd.Context(0)
    c.set_tuning(TUNE_MAX_BLOCKS, 1)
    arena, off, lens = placed(GenProfile.MIXED, n)
    check(torch, c, arena, off, lens, Chain.GenericUlp, mixed_edits(Chain.GenericUlp, n),
          rows=mixed_rows(n), n_rows=N_ROWS, what=CSUM_L3 | CSUM_L4)


# ---------------------------------------------------------------------------
# Strided layouts: k_parse, whatever the pipeline knob says
# ---------------------------------------------------------------------------
@lru_cache(maxsize=None)
def slots(stride, with_lens):
    n = 64 * 3 + 5
    if stride == 64:
        arena, _, _ = gen_frames_host(GenProfile.V4UDP64, n, stride=64)
        arena = np.array(arena[:n * 64])
        lens = None
    else:
        pay6, pay4 = bytes(range(54)), bytes(range(86))
        frames = [cf.frame("v4", cf.UDP, pay4) if i % 3 == 2 else cf.frame("v6", cf.TCP, pay6)
                  for i in range(n)]
        arena = np.frombuffer(b"".join(frames), dtype=np.uint8).copy()
        lens = None
    if with_lens:  # shorter frames in the same slots: the bytes after them stay
        lens = (np.full(n, stride, np.uint16) - (np.arange(n) % 4).astype(np.uint16))
    arena.setflags(write=False)
    return arena, lens, n


@pytest.mark.parametrize("pipeline", [1, 0])
@pytest.mark.parametrize("stride,with_lens", [(64, False), (128, False), (128, True)])
def test_strided_slots(torch, stride, with_lens, pipeline):
    arena, lens, n = slots(stride, with_lens)
    c = ingot_amd.Context(0)
    c.set_tuning(TUNE_PIPELINE, pipeline)
    got, recs = check(torch, c, arena, None, lens, Chain.GenericUlp,
                      mixed_edits(Chain.GenericUlp, n), rows=mixed_rows(n), n_rows=N_ROWS,
                      what=CSUM_L3 | CSUM_L4, stride=stride, n=n)
    assert (recs["status"] == 0).sum() > n // 2 and (got != arena).any()


# ---------------------------------------------------------------------------
# Chains, profiles, sums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("profile", [GenProfile.MIXED, GenProfile.VLAN_V6EH, GenProfile.GENEVE,
                                     GenProfile.ADVERSARIAL, GenProfile.GENEVE_ADVERSARIAL])
@pytest.mark.parametrize("chain", list(Chain))
def test_chains_and_profiles(ctx, torch, chain, profile):
    """Fields inside the staged window, straddling its end and past it (the
    tunnel's inner IPv6 addresses, L4 behind EH chains)."""
    n = 700
    arena, off, lens = placed(profile, n)
    what = 7 if chain == TUN else CSUM_L3 | CSUM_L4
    check(torch, ctx, arena, off, lens, chain, mixed_edits(chain, n), rows=mixed_rows(n),
          n_rows=N_ROWS, what=what)


@pytest.mark.parametrize("chain,profile,what", [
    (Chain.GenericUlp, GenProfile.MIXED, 0), (Chain.GenericUlp, GenProfile.MIXED, CSUM_L3),
    (Chain.GenericUlp, GenProfile.MIXED, CSUM_L4), (Chain.VlanUlp, GenProfile.VLAN_V6EH, 3),
    (TUN, GenProfile.GENEVE, CSUM_OUTER_L4), (TUN, GenProfile.GENEVE, 7), (TUN, GenProfile.GENEVE, 0)])
def test_selected_sums(ctx, torch, chain, profile, what):
    n = 300
    arena, off, lens = placed(profile, n, seed=92, misalign=5)
    got, _ = check(torch, ctx, arena, off, lens, chain, mixed_edits(chain, n, seed=2), what=what,
                   rows=mixed_rows(n), n_rows=N_ROWS)
    assert (got != arena).any()


def test_no_row_array(ctx, torch):
    """d_row NULL: every Ok packet is edited, n_rows is ignored."""
    n = 200
    arena, off, lens = placed(GenProfile.MIXED, n)
    t = cases.nat_table(n, 3)
    check(torch, ctx, arena, off, lens, Chain.UdpParser, cases.nat_edits(t, 1), what=3)


# ---------------------------------------------------------------------------
# d_row
# ---------------------------------------------------------------------------
def test_guarded_packets_are_untouched_and_recorded(ctx, torch):
    n = 500
    arena, off, lens = placed(GenProfile.MIXED, n)
    rows = mixed_rows(n)
    got, recs = check(torch, ctx, arena, off, lens, Chain.GenericUlp,
                      mixed_edits(Chain.GenericUlp, n), rows=rows, n_rows=N_ROWS, what=3)
    skipped = np.nonzero(rows >= N_ROWS)[0]
    assert len(skipped) > 100
    for i in skipped:
        o, ln = int(off[i]), int(lens[i])
        assert got[o:o + ln].tobytes() == arena[o:o + ln].tobytes(), i
    assert (recs["status"][skipped] == 0).sum() > 50  # their records are still written


def test_flow_bins_drive_a_nat_table(ctx, torch):
    """flow_hist's d_flow, as it comes, is d_row for a table of `bins` rows."""
    n, bins = 1000, 1 << 10
    frames = []  # 700 well-formed frames, then 300 of which most are not counted
    for a, o, ln in (placed(GenProfile.MIXED, 700), placed(GenProfile.ADVERSARIAL, 300)):
        frames += [a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, ln)]
    arena, off, lens = cf.place(frames, misalign=3)
    d_arena = torch.from_numpy(np.array(arena)).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_len = torch.from_numpy(lens.view(np.int16)).cuda()
    flow = ctx.flow_hist(d_arena, d_off, d_len, Chain.GenericUlp, bins=bins)
    t = cases.nat_table(bins, 4)
    edits = [(1, Field.V4_SOURCE, SET, ("row", col_u32(t))),
             (2, Field.UDP_SOURCE, SET, ("row", col_u16(t))),
             (2, Field.TCP_SOURCE, SET, ("row", col_u16(t))),
             (1, WideField.V6_SOURCE, SET, ("row", t[:, 16:32]))]
    recs = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    ctx.parse_modify_rows(d_arena, d_off, d_len, Chain.GenericUlp,
                          cases.device_edits(torch, edits), rows=flow, n_rows=bins, out=recs,
                          csum=3)
    torch.cuda.synchronize()
    rows = flow.cpu().numpy().view(np.uint32)
    assert (rows == ROW_NONE).any() and (rows < bins).sum() > n // 2
    want, w_rec = rows_model.apply(arena, off, lens, Chain.GenericUlp, edits, rows=rows,
                                   n_rows=bins, what=3)
    assert recs.cpu().numpy().tobytes() == w_rec.tobytes()
    assert (d_arena.cpu().numpy() == want).all()


# ---------------------------------------------------------------------------
# End to end: the device's own verify after NAT66 + MAC
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tunnel", [False, True])
def test_right_sums_stay_right_on_the_device(ctx, torch, tunnel):
    arena, off, lens = cases.right_sum_tunnel_frames() if tunnel else cases.right_sum_frames()
    chain = TUN if tunnel else Chain.VlanUlp
    t = cases.nat_table(len(off), 11)
    edits = cases.tunnel_edits(t) if tunnel else cases.nat_edits(t, 2)
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_len = torch.from_numpy(lens.view(np.int16)).cuda()

    def verify(a):
        d = torch.from_numpy(np.array(a)).cuda()
        out = [ctx.checksum_verify(d, d_off, d_len, ctx.parse(d, d_off, d_len, chain))]
        if tunnel:  # the outer UDP sum: a UdpParser parse of the tunnel frame
            out.append(ctx.checksum_verify(d, d_off, d_len,
                                           ctx.parse(d, d_off, d_len, Chain.UdpParser),
                                           what=CSUM_L4))
        torch.cuda.synchronize()
        rows = [x.cpu().numpy().view(abi.CSUM_DTYPE).reshape(-1) for x in out]
        return np.stack([r[k] for r in rows for k in ("l3_state", "l4_state")], axis=1)

    before = verify(arena)
    assert (before[:, 1] == cases.OK).mean() >= 0.9
    got, _ = check(torch, ctx, arena, off, lens, chain, edits, what=7 if tunnel else 3)
    assert (verify(got) == before).all()
    assert (got != arena).any()


# ---------------------------------------------------------------------------
# The raw ABI: every EINVAL, n == 0
# ---------------------------------------------------------------------------
def test_every_einval_leaves_the_arena_alone(ctx, torch):
    arena, off, lens = placed(GenProfile.MIXED, 64)
    d_arena = torch.from_numpy(np.array(arena)).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_len = torch.from_numpy(lens.view(np.int16)).cuda()
    d_rows = torch.zeros(64, dtype=torch.int32, device="cuda")
    tab = torch.zeros((64, 32), dtype=torch.uint8, device="cuda")
    p = tab.data_ptr()
    G, lib = int(Chain.GenericUlp), ctx._lib
    V, U16, U32, B = (int(x) for x in EditSource)
    PKT, ROW = int(EditBy.PACKET), int(EditBy.ROW)
    MAC, V6 = int(WideField.ETH_SOURCE), int(WideField.V6_SOURCE)
    F = Field

    def call(edits, what=0, chain=G, rows=d_rows, n=64, arena_p=None, offp=None, lenp=None,
             stride=0, h=None, n_edits=None, null_list=False):
        e = abi.edit_rows_array(edits)
        return lib.ingot_gpu_parse_modify_rows(
            ctx._h if h is None else h, d_arena.data_ptr() if arena_p is None else arena_p,
            d_off.data_ptr() if offp is None else offp, d_len.data_ptr() if lenp is None else lenp,
            stride, n, chain, None if null_list else e.ctypes.data_as(ctypes.c_void_p),
            len(e) if n_edits is None else n_edits, None if rows is None else rows.data_ptr(),
            64, what, None, None)

    # (layer, field, op, index, value, source, by, pitch, d_values)
    good = (1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 32, p)
    assert call([good]) == 0
    torch.cuda.synchronize()
    after_good = d_arena.cpu().numpy().copy()
    assert (after_good != arena).any()
    bad = {
        "bad chain": dict(edits=[good], chain=99),
        "too many edits": dict(edits=[good] * 17),
        "NULL list": dict(edits=[good], null_list=True),
        "unknown narrow field": dict(edits=[(1, 48, SET, 0, 0, U32, PKT, 0, p)]),
        "field between the enums": dict(edits=[(1, 63, SET, 0, 0, B, PKT, 0, p)]),
        "field past the wide ones": dict(edits=[(1, 68, SET, 0, 0, B, PKT, 0, p)]),
        "unknown op": dict(edits=[(1, F.V4_SOURCE, 6, 0, 0, U32, PKT, 0, p)]),
        "layer out of range": dict(edits=[(3, F.V4_SOURCE, SET, 0, 0, U32, PKT, 0, p)]),
        "bad source": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, 4, PKT, 0, p)]),
        "bad by": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, 2, 0, p)]),
        "value with a table": dict(edits=[(1, F.V4_SOURCE, SET, 0, 9, U32, PKT, 0, p)]),
        "NULL table": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 0, 0)]),
        "BYTES on a narrow field": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, B, PKT, 0, p)]),
        "U32 on a wide field": dict(edits=[(0, MAC, SET, 0, 0, U32, PKT, 0, p)]),
        "VALUE on a wide field": dict(edits=[(0, MAC, SET, 0, 5, V, PKT, 0, 0)]),
        "wide field with ADD": dict(edits=[(1, V6, ADD, 0, 0, B, PKT, 0, p)]),
        "pitch below u32": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 2, p)]),
        "pitch below a MAC": dict(edits=[(0, MAC, SET, 0, 0, B, PKT, 5, p)]),
        "pitch below an address": dict(edits=[(1, V6, SET, 0, 0, B, PKT, 15, p)]),
        "odd u16 table": dict(edits=[(2, F.UDP_SOURCE, SET, 0, 0, U16, PKT, 0, p + 1)]),
        "odd u16 pitch": dict(edits=[(2, F.UDP_SOURCE, SET, 0, 0, U16, PKT, 3, p)]),
        "misaligned u32 table": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 0, p + 2)]),
        "misaligned u32 pitch": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, PKT, 6, p)]),
        "BY_ROW without d_row": dict(edits=[(1, F.V4_SOURCE, SET, 0, 0, U32, ROW, 0, p)],
                                     rows=None),
        "BY_ROW VALUE without d_row": dict(edits=[(1, F.V4_SOURCE, SET, 0, 7, V, ROW, 0, 0)],
                                           rows=None),
        "what above 7": dict(edits=[good], what=8),
        "OUTER_L4 outside the tunnel": dict(edits=[good], what=CSUM_OUTER_L4),
        "a refused field": dict(edits=[(1, F.V4_IHL, SET, 0, 5, V, PKT, 0, 0)], what=3),
        "d_off without d_len": dict(edits=[good], lenp=0),
    }
    for name, kw in bad.items():
        assert call(**kw) == -1, name
    e = abi.edit_rows_array([good])
    ep = e.ctypes.data_as(ctypes.c_void_p)
    rest = (ep, 1, None, 0, 0, None, None)
    assert lib.ingot_gpu_parse_modify_rows(None, p, None, None, 64, 1, G, *rest) == -1  # no ctx
    e["_pad"] = 1
    assert lib.ingot_gpu_parse_modify_rows(ctx._h, d_arena.data_ptr(), d_off.data_ptr(),
                                           d_len.data_ptr(), 0, 64, G, *rest) == -1  # _pad
    e["_pad"] = 0
    # n > 0: a NULL arena; slots at a stride that is no multiple of 16
    assert lib.ingot_gpu_parse_modify_rows(ctx._h, None, d_off.data_ptr(), d_len.data_ptr(), 0,
                                           64, G, *rest) == -1
    assert lib.ingot_gpu_parse_modify_rows(ctx._h, tab.data_ptr(), None, None, 24, 4, G,
                                           *rest) != 0
    # n == 0 succeeds whatever the device pointers are, after the list's checks
    assert lib.ingot_gpu_parse_modify_rows(ctx._h, None, None, None, 0, 0, G, *rest) == 0
    assert lib.ingot_gpu_parse_modify_rows(ctx._h, None, None, None, 0, 0, G, ep, 1, None, 0, 8,
                                           None, None) == -1
    torch.cuda.synchronize()
    assert d_arena.cpu().numpy().tobytes() == after_good.tobytes()  # no refused call wrote
    assert not tab.any()


def test_n_zero_through_the_wrapper(ctx, torch):
    arena = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = torch.zeros(0, dtype=torch.int64, device="cuda")
    lens = torch.zeros(0, dtype=torch.int16, device="cuda")
    assert ctx.parse_modify_rows(arena, off, lens, Chain.GenericUlp,
                                 [(1, Field.V4_HOP_LIMIT, SUB, 1)]) is None
    torch.cuda.synchronize()
    assert not arena.any()


# ---------------------------------------------------------------------------
# The C-ABI-only host
# ---------------------------------------------------------------------------
def test_cpp_nat_table_example_on_device(torch):
    """tests/cpp/example_nat_table.cpp, a fresh process: flow bins -> SNAT from
    a bins-row table with L3 | L4, then ingot_gpu_checksum_verify: every sum Ok."""
    exe = ROOT / "tests" / "cpp" / "build" / "example_nat_table"
    if not exe.exists():
        from ingot_amd.build import build_cpp_tests

        build_cpp_tests()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ", 0 not OK before, 0 not OK after, 0 not rewritten: OK" in r.stdout
