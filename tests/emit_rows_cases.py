"""Header stacks, operand tables and batches shared by
tests/test_emit_rows_model.py, tests/test_emit_rows.py and tools/bigfuzz.py.
TEST INFRASTRUCTURE ONLY.

A case's sets are in the model's host form (tests/emit_rows_model.py): every
table is a numpy array, or a view into one backing array.  `backing` names the
arrays the views come from, so a device test can upload each backing array
once and rebuild the same views (same base alignment, same pitch) there.
"""
from __future__ import annotations

import numpy as np

from ingot_amd import EmitSource, Field, WideField
from tests import emit_csum_cases as cases

ROW_NONE = 0xFFFFFFFF
STACKS = ("opte", "geneve_v4", "v6_udp")
# dense: every table an array of its own, pitch = width (a MAC's 6-B pitch is
#        the byte path, an address's 16-B pitch the dword path);
# struct32: one (rows, 32) uint8 table, members passed as column views
#        (pitch 32; address at 0, MACs at 16 and 22, u32 at 28, u16 at 26);
# odd:   the wide tables start at an odd address (byte loads);
# aligned: every wide table 4-B aligned with a pitch that is a multiple of 4.
FORMS = ("dense", "struct32", "odd", "aligned")


class View:
    """A table as a view of backing array `name`: uint8 bytes [first, first +
    width) of rows `pitch` bytes apart, reinterpreted as `dtype`."""

    def __init__(self, name, first, width, pitch, rows, dtype=np.uint8):
        self.name, self.first, self.width, self.pitch = name, first, width, pitch
        self.rows, self.dtype = rows, np.dtype(dtype)

    def numpy(self, backing):
        b = backing[self.name]
        v = np.lib.stride_tricks.as_strided(b[self.first:], (self.rows, self.width),
                                            (self.pitch, 1), writeable=False)
        if self.dtype == np.uint8:
            return v
        return np.ascontiguousarray(v).view(self.dtype).reshape(-1)  # a copy: same values

    def torch(self, dev_backing):
        t = dev_backing[self.name]
        v = t[self.first:].as_strided((self.rows, self.width), (self.pitch, 1))
        if self.dtype == np.uint8:
            return v
        import torch

        return v.view({2: torch.int16, 4: torch.int32}[self.dtype.itemsize])  # (rows, 1)


def _tables(form, rows, members, rng):
    """members = [(key, width, dtype)] -> ({key: View}, backing).  Narrow
    members keep their natural alignment in every form."""
    backing, views = {}, {}
    if form == "struct32":
        at = {16: [0], 6: [16, 22], 4: [28], 2: [26]}
        backing["t"] = rng.integers(0, 256, rows * 32, dtype=np.uint8)
        for key, width, dt in members:
            views[key] = View("t", at[width].pop(0), width, 32, rows, dt)
        return views, backing
    for key, width, dt in members:
        wide = np.dtype(dt) == np.uint8
        lead = 1 if (form == "odd" and wide) else 0
        pitch = (width + 3) // 4 * 4 if (form == "aligned" and wide) else width
        backing[key] = rng.integers(0, 256, lead + rows * pitch + 8, dtype=np.uint8)
        views[key] = View(key, lead, width, pitch, rows, dt)
    return views, backing


class Case:
    def __init__(self, hdr, sets, sums, backing):
        self.hdr, self.sets, self.sums, self.backing = hdr, sets, sums, backing

    def host_sets(self):
        return [_host(s, self.backing) for s in self.sets]

    def device_sets(self, dev_backing):
        return [_dev(s, dev_backing) for s in self.sets]


def _host(s, backing):
    if len(s) == 4:
        return s
    t = s[4]
    if isinstance(t, tuple):
        return (*s[:4], ("row", t[1].numpy(backing)))
    return (*s[:4], t.numpy(backing))


def _dev(s, dev_backing):
    if len(s) == 4:
        return s
    t = s[4]
    if isinstance(t, tuple):
        return (*s[:4], ("row", t[1].torch(dev_backing)))
    return (*s[:4], t.torch(dev_backing))


def stack(name: str, form: str, n: int, n_rows: int, rng) -> Case:
    """The issue's three stacks.  BY_PACKET tables hold n rows, BY_ROW tables
    n_rows."""
    hdr, _, sums = cases.stack(name, 1, rng)
    if name == "opte":
        # per-row outer IPv6 destination, Ethernet addresses and VNI; a
        # per-packet entropy port
        row, b = _tables(form, n_rows, [("v6d", 16, np.uint8), ("macd", 6, np.uint8),
                                        ("macs", 6, np.uint8), ("vni", 4, np.uint32)], rng)
        pkt, b2 = _tables("dense", n, [("port", 2, np.uint16)], rng)
        sets = [(14, Field.V6_PAYLOAD_LEN, EmitSource.LENGTH, -40),
                (54, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
                (14, WideField.V6_DESTINATION, EmitSource.BYTES, 0, ("row", row["v6d"])),
                (0, WideField.ETH_DESTINATION, EmitSource.BYTES, 0, ("row", row["macd"])),
                (0, WideField.ETH_SOURCE, EmitSource.BYTES, 0, ("row", row["macs"])),
                (62, Field.GENEVE_VNI, EmitSource.U32, 0, ("row", row["vni"])),
                (54, Field.UDP_SOURCE, EmitSource.U16, 0, pkt["port"])]
        return Case(hdr, sets, sums, {**b, **b2})
    if name == "geneve_v4":
        row, b = _tables(form, n_rows, [("macs", 6, np.uint8), ("v4s", 4, np.uint32)], rng)
        sets = [(14, Field.V4_TOTAL_LEN, EmitSource.LENGTH, 0),
                (34, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
                (14, Field.V4_SOURCE, EmitSource.U32, 0x01020304, ("row", row["v4s"])),
                (0, WideField.ETH_SOURCE, EmitSource.BYTES, 0, ("row", row["macs"]))]
        return Case(hdr, sets, sums, b)
    if name == "v6_udp":
        # the whole pseudo-header per packet
        pkt, b = _tables(form, n, [("v6s", 16, np.uint8), ("port", 2, np.uint16)], rng)
        pkt2, b2 = _tables("odd" if form == "odd" else "dense", n, [("v6d", 16, np.uint8)], rng)
        sets = [(14, Field.V6_PAYLOAD_LEN, EmitSource.LENGTH, -40),
                (54, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
                (14, WideField.V6_SOURCE, EmitSource.BYTES, 0, pkt["v6s"]),
                (14, WideField.V6_DESTINATION, EmitSource.BYTES, 0, pkt2["v6d"]),
                (54, Field.UDP_SOURCE, EmitSource.U16, -1, pkt["port"])]
        return Case(hdr, sets, sums, {**b, **b2})
    raise KeyError(name)


def lengths(n: int, rng, live=None):
    """Payload lengths cycling through EDGE_LENGTHS without 65535, from a
    random phase, plus one 65535-B packet (no datagram: its field is left)
    among the emitted ones."""
    edge = np.asarray(cases.EDGE_LENGTHS[:-1], np.uint16)
    ln = edge[(np.arange(n) + int(rng.integers(0, len(edge)))) % len(edge)].copy()
    cand = np.arange(n) if live is None else np.nonzero(live)[0]
    if len(cand):
        ln[int(rng.choice(cand))] = 65535
    return ln


def row_indices(n: int, n_rows: int, rng, guarded=()):
    """n row indices below n_rows, the last row among them; the packets in
    `guarded` get n_rows and ROW_NONE in turn."""
    rows = rng.integers(0, n_rows, n, dtype=np.uint64).astype(np.uint32)
    free = np.setdiff1d(np.arange(n), np.asarray(list(guarded), np.int64))
    if len(free):
        rows[int(rng.choice(free))] = n_rows - 1
    for k, i in enumerate(guarded):
        rows[i] = n_rows if k % 2 == 0 else ROW_NONE
    return rows


def batch(n: int, hdr_len: int, rng, rows=None, n_rows: int = 0, poison: bool = True):
    """-> (src, off, lens, dst_off, size): random_source payloads, pack()
    destinations; the neighbours of a guarded packet are packed with gap 0 on
    both sides of it, and (poison) its own descriptors point far outside both
    arenas."""
    live = np.ones(n, bool) if rows is None else rows.astype(np.uint64) < n_rows
    ln = lengths(n, rng, live)
    src, off = cases.random_source(ln, rng)
    # destinations of the emitted packets only: a guarded packet owns no bytes
    tot = np.where(live, hdr_len + ln.astype(np.int64), 0)
    gaps = rng.integers(0, 4, n)
    gaps[~live] = 0
    gaps[np.r_[~live[1:], False]] = 0  # the packet before a guarded one: no gap either
    dst_off = (np.cumsum(np.r_[0, (tot + gaps)[:-1]]) + 5).astype(np.uint64)
    size = int(dst_off[-1] + tot[-1] + 64)
    if poison:
        off, ln = off.copy(), ln.copy()
        off[~live] = 1 << 40
        ln[~live] = 65535
        dst_off[~live] = 1 << 41
    return src, off, ln, dst_off, size
