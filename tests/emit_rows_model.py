"""The definition of ingot_gpu_emit_packets_rows (include/ingot_gpu.h), in
numpy / Python.  TEST INFRASTRUCTURE ONLY.

Written from the header's equivalence, on top of the definitions that exist:
`oracle.emit_batch` (the plain emit) and `tests/emit_csum_model.one` (the
sums).  For every emitted packet, alone:

  - the sets are walked in list order over a copy of `hdr`;
  - a BYTES set pastes its row's 6 / 16 bytes at the wide field's place;
  - a U16 / U32 table set becomes a VALUE set of the row's integer + add;
  - LENGTH / VALUE sets stay as they are;
  - narrow sets that come before a BYTES set are folded into the copy first
    (the plain emit's header-block form writes exactly the patched block), so
    a later paste overwrites them and a later narrow set overwrites a paste;
  - `oracle.emit_batch` emits that one packet, `emit_csum_model.one` fills its
    sums.

A packet whose row index is >= n_rows is not emitted: the arena keeps whatever
it held there (the tests' 0xA5 fill).

Host form of a set: (at, Field | WideField, EmitSource, add[, table]) with
`table` a numpy array (one row per packet) or ("row", array) (row rows[i]):
u16 / u32 of shape (rows,) or (rows, 1), or u8 of shape (rows, 6 | 16).  Views
with a row stride are fine; numpy indexes them as the device does.
"""
from __future__ import annotations

import numpy as np

import oracle
from ingot_amd.abi import WIDE_BYTES, EmitSource, Field, WideField
from tests import emit_csum_model

WIDE_AT = {WideField.ETH_DESTINATION: 0, WideField.ETH_SOURCE: 6, WideField.V6_SOURCE: 8,
           WideField.V6_DESTINATION: 24}
MAX_SETS = 8
N_FIELDS = len(Field)
# field -> (first bit, width): only what check_args needs, the covering bytes;
# taken from the oracle's own setter so the model carries no second table
_SPAN = {}


def is_wide(field) -> bool:
    return int(field) in WIDE_BYTES


def field_span(field) -> tuple[int, int]:
    """(first covering byte, covering bytes) of a narrow field in its header:
    found by setting the field to all ones in a zero header through the plain
    emit and looking at which bytes changed."""
    f = Field(int(field))
    if f not in _SPAN:
        out = np.zeros(64, np.uint8)
        oracle.emit_batch(bytes(64), [(0, f, EmitSource.VALUE, -1)], None, None,
                          np.zeros(1, np.uint16), out, np.zeros(1, np.uint64), copy=False)
        nz = np.nonzero(out)[0]
        _SPAN[f] = (int(nz[0]), int(nz[-1] - nz[0] + 1))
    return _SPAN[f]


def _table(e):
    """-> (by_row, array or None)"""
    t = e[4] if len(e) > 4 else None
    if isinstance(t, tuple):
        assert t[0] == "row"
        return True, t[1]
    return False, t


def emitted(n: int, rows, n_rows: int) -> np.ndarray:
    """Which packets the row guard lets through."""
    if rows is None:
        return np.ones(n, bool)
    return np.asarray(rows).astype(np.uint64) < np.uint64(n_rows)


def one(hdr: bytes, sets, sums, payload: np.ndarray, i: int, r: int) -> np.ndarray:
    """The bytes of packet i (row index r) -> u8 array of len(hdr) + len(payload)."""
    h = bytearray(hdr)
    L = len(payload)
    lens = np.array([L], np.uint16)
    zero = np.zeros(1, np.uint64)
    pending = []
    for e in sets:
        at, field, source, add = int(e[0]), e[1], EmitSource(int(e[2])), int(e[3])
        by_row, t = _table(e)
        row = r if by_row else i
        if source == EmitSource.BYTES:
            if pending:  # fold the narrow sets so far into the block
                blk = np.zeros(len(h), np.uint8)
                oracle.emit_batch(bytes(h), pending, None, None, lens, blk, zero, copy=False)
                h, pending = bytearray(blk.tobytes()), []
            w = WideField(int(field))
            p = at + WIDE_AT[w]
            h[p:p + WIDE_BYTES[w]] = bytes(np.asarray(t[row], np.uint8).reshape(-1))
        elif source in (EmitSource.U16, EmitSource.U32):
            v = int(np.asarray(t[row]).reshape(-1)[0])
            pending.append((at, field, EmitSource.VALUE, (v + add) & 0xFFFFFFFF))
        else:
            pending.append((at, field, source, add))
    out = np.zeros(len(h) + L, np.uint8)
    src = np.concatenate([np.asarray(payload, np.uint8), np.zeros(16, np.uint8)])
    oracle.emit_batch(bytes(h), pending, src, zero, lens, out, zero)
    if sums:
        # ihl and the IP version come from the host block, as the header says
        emit_csum_model.one(out, bytes(hdr), sums)
    return out


def apply(arena: np.ndarray, hdr: bytes, sets, sums, src, off, lens, dst_off, rows=None,
          n_rows: int = 0) -> np.ndarray:
    """In place on `arena` (numpy u8): the whole call."""
    hdr = bytes(hdr)
    n = len(lens)
    live = emitted(n, rows, n_rows)
    for i in np.nonzero(live)[0].tolist():
        o, ln, d = int(off[i]), int(lens[i]), int(dst_off[i])
        r = int(rows[i]) if rows is not None else i
        arena[d:d + len(hdr) + ln] = one(hdr, sets, sums or (), src[o:o + ln], i, r)
    return arena


def check_args(ctx_ok: bool, hdr, hdr_len: int, sets, n_sets: int, sums, have_row: bool, n: int,
               pointers_ok: bool) -> None:
    """The argument errors of the call, raised (ValueError naming the step) in
    the order the header gives.  `sets`: None (a NULL list) or records of
    abi.EMIT_SET_ROWS_DTYPE, the C structs themselves; `sums`: as
    emit_csum_model.check_args takes them."""
    if not ctx_ok:
        raise ValueError("1: ctx NULL")
    if hdr_len > 256 or (hdr_len and hdr is None) or n_sets > MAX_SETS or (n_sets and sets is None):
        raise ValueError("2: hdr / hdr_len / n_sets / NULL sets")
    hdr = bytes(hdr or b"")[:hdr_len]
    narrow = []
    for k in range(n_sets):
        e = sets[k]
        field, source, by = int(e["field"]), int(e["source"]), int(e["by"])
        pitch, values, add = int(e["pitch"]), int(e["d_values"]), int(e["add"])
        wide = is_wide(field)
        if not wide and field >= N_FIELDS:
            raise ValueError(f"3.{k}: unknown field")
        if source > int(EmitSource.BYTES):
            raise ValueError(f"3.{k}: unknown source")
        if any(int(b) for b in e["_pad"]):
            raise ValueError(f"3.{k}: padding")
        if by > 1:
            raise ValueError(f"3.{k}: unknown by")
        if (source == int(EmitSource.BYTES)) != wide:
            raise ValueError(f"3.{k}: BYTES and wide fields go together")
        table = source not in (int(EmitSource.LENGTH), int(EmitSource.VALUE))
        if not table and (by or pitch or values):
            raise ValueError(f"3.{k}: LENGTH / VALUE with by, pitch or d_values")
        if table and not values:
            raise ValueError(f"3.{k}: NULL table")
        if wide and add:
            raise ValueError(f"3.{k}: BYTES with add")
        width = {int(EmitSource.U16): 2, int(EmitSource.U32): 4}.get(
            source, WIDE_BYTES[WideField(field)] if wide else 0)
        if pitch and pitch < width:
            raise ValueError(f"3.{k}: pitch below the width")
        if source in (int(EmitSource.U16), int(EmitSource.U32)) and (values | pitch) % width:
            raise ValueError(f"3.{k}: misaligned table")
        if by == 1 and not have_row:
            raise ValueError(f"3.{k}: BY_ROW without d_row")
        if wide:
            first, nbytes = WIDE_AT[WideField(field)], width
        else:
            first, nbytes = field_span(field)
            narrow.append((int(e["at"]), Field(field)))
        if int(e["at"]) + first + nbytes > hdr_len:
            raise ValueError(f"3.{k}: field outside hdr")
    try:
        emit_csum_model.check_args(hdr, narrow, sums or ())
    except ValueError as err:
        raise ValueError(f"4: {err}") from None
    if n == 0:
        return
    if not pointers_ok:
        raise ValueError("6: NULL device pointer")
