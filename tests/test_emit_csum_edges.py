"""ingot_gpu_emit_packets_csum on the device at the values where a checksum
goes wrong (tests/csum_sweep_cases.py): a computed 0 (UDP: written 0xffff;
IPv4: 00 00) and its neighbours, all-0xff and all-0x00 payloads up to the
longest datagram and one byte past it, header blocks near the 256-B limit with
every setter slot taken, IPv6 extension headers between `l3_at` and `at`.
As in tests/test_emit_csum.py the destination starts as 0xA5 and the whole
arena equals oracle.emit_batch + tests/emit_csum_model.py; crafted packets sit
among ordinary ones at packets 0, 63, 64, 255, 256 and the last of 600.
tests/test_csum_sweep_model.py holds the same cases to a byte-wise receiver.
Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import ingot_amd
from ingot_amd import EmitSum
from tests import csum_sweep_cases as sc
from tests import emit_csum_cases as cases
from tests.test_emit_csum import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return ingot_amd.Context(0)


def _device(ctx, torch, c: sc.EmitCase):
    """The whole arena equals the definition's; -> the device's arena."""
    return _check(ctx, torch, c.hdr, c.sets, c.sums, c.src, c.off, c.lens, c.dst_off, c.size,
                  c.name)


@pytest.mark.parametrize("name", cases.STACKS)
def test_computed_zero(ctx, torch, name):
    """Payload lengths 2, 3, 17 and 1025 whose first word makes the segment
    add up to 0xffff (field ff ff), 0xfffe (00 01) and 0x10000 (ff fe), at all
    16 destination misalignments: both parities, the field inside one 16-B
    chunk and across two."""
    seen = set()
    for dmis in range(16):
        for c in sc.computed_zero_cases(name, dmis):
            assert all(int(c.dst_off[k]) % 16 == dmis for k, *_ in c.checks)
            sc.held(c, sc.emit_model(c))  # the model's field is what the case was built for
            sc.held(c, _device(ctx, torch, c))
            seen |= {(k, want) for k, _, want, _ in c.checks}
    # every value at every crafted place
    assert seen == {(k, w) for k in sc.CRAFTED_AT for w in (b"\xff\xff", b"\x00\x01", b"\xff\xfe")}


@pytest.mark.parametrize("name", ["geneve_v4", "vlan_v4opt"])
def test_ipv4_header_sum_of_zero(ctx, torch, name):
    c = sc.ipv4_zero_case(name)
    assert sorted(w for _, _, w, _ in c.checks) == [b"\x00\x00"] * 2 + [b"\x00\x01"] * 2 + \
        [b"\xff\xfe"] * 2
    sc.held(c, sc.emit_model(c))
    sc.held(c, _device(ctx, torch, c))


@pytest.mark.parametrize("name", cases.STACKS)
def test_largest_sums(ctx, torch, name):
    """All-0xff payloads drive the accumulator and both folds to their largest
    values; S = 65,535 is the last datagram, S = 65,536 keeps its field."""
    for parity in (0, 1):
        for smis in (0, 5):
            c = sc.largest_sum_case(name, parity, smis)
            u_at = sc._udp_sum(c.sums)[1]
            S = len(c.hdr) - u_at + c.lens.astype(np.int64)
            assert {65534, 65535, 65536} <= set(S.tolist()) and len(c.checks) == 4
            sc.held(c, _device(ctx, torch, c))


@pytest.mark.parametrize("name", sc.BIG_STACKS)
def test_largest_header_blocks(ctx, torch, name):
    """254-B header blocks (about 90 KB of LDS per workgroup, the field's
    chunk up to the region's last) with all eight setters, one of them on a
    checksum field the named sum overrides; 257 packets, every edge length."""
    c = sc.big_header_case(name)
    got = _device(ctx, torch, c)
    if name == "v6_dstopts":
        return
    assert len(c.hdr) == 254 and len(c.sets) == ingot_amd.abi.MAX_EMIT_SETS
    # the setter's per-packet value did not survive in any datagram's field
    # (S > 65,535: the field is the setter's, as emitted)
    u = sc._udp_sum(c.sums)
    vals = next(s[4] for s in c.sets if s[1] == sc.F.UDP_CHECKSUM)
    field = np.array([(int(got[int(o) + u[1] + 6]) << 8) | int(got[int(o) + u[1] + 7])
                      for o in c.dst_off])
    datagram = len(c.hdr) - u[1] + c.lens.astype(np.int64) <= 65535
    assert (field[datagram] != vals[datagram]).sum() >= datagram.sum() - 2
    assert (field[~datagram] == vals[~datagram]).all() and (~datagram).sum() == 1
    if any(int(s[0]) == int(EmitSum.IPV4) for s in c.sums):
        v4 = next(s[4] for s in c.sets if s[1] == sc.F.V4_CHECKSUM)
        f4 = np.array([(int(got[int(o) + 24]) << 8) | int(got[int(o) + 25]) for o in c.dst_off])
        assert (f4 != v4).sum() >= len(v4) - 2
