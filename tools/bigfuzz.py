#!/usr/bin/env python3
"""Validation tool: a large one-off differential run, device vs oracle, beyond
the sizes the pytest suite uses.  For every chain: records and every getter
over N adversarial frames (every truncation / ihl / data_offset / EH / Geneve
defect path), in the packed layout and in 256-B slots; flow ids and hashes
for the VLAN chain.  Prints one JSON line with the mismatch counts (all must
be 0) and writes it to gpurun_out/bigfuzz.json.  Also parse_read over random
4-chunk splits (every staging plan kept, parse_read_first, lazy bounds),
flow bins from k_flows_bits and from k_parse's flows mode, the slot ring, and
the checksum calls (`csum`: verify, then fill + verify, against the Python
model of tests/csum_model.py, so on at most --csum-frames frames per case),
and the rewrite with the fused checksum update (`modify_csum`: against the
oracle's rewrite + the Python model of tests/csum_update_model.py, same cap),
and the emit with checksums (`emit_csum`: against the oracle's emit + the
Python model of tests/emit_csum_model.py, same cap), and the checksum calls
over chunked packets (`csum_read`, only with --only: verify, fill, verify again
over cut generator frames against tests/csum_read_model.py, same cap), and the
rewrite over chunked packets (`modify_read`, only with --only: random edit
lists over cut generator frames against tests/modify_read_model.py, same cap),
and the emit over chunked packets (`emit_read`, only with --only: every header
stack in front of cut generator frames with random from / take, whole arenas
against tests/emit_read_model.py, same cap), and the emit with per-row
operands (`emit_rows`, only with --only: every stack and table form of
tests/emit_rows_cases.py, rows from the flow bins, whole arenas against
tests/emit_rows_model.py, same cap), and the rewrite over chunked packets with
per-packet operands (`modify_read_rows`, only with --only: modify_read's five
sets with random mixed lists, tables, guards and every `what`, against
tests/modify_read_rows_model.py, same cap), and the emit over chunked packets
with per-row operands (`emit_read_rows`, only with --only: emit_rows' stacks,
table forms and rows over emit_read's cut frames with random from / take, the
guarded packets' chunk descriptors unusable, whole arenas and d_taken against
tests/emit_read_rows_model.py, same cap).

    python tools/bigfuzz.py [--frames 4000000] [--seed 1234]
                            [--only csum|modify_csum|emit_csum|csum_read|modify_read|emit_read|
                                    emit_rows|modify_read_rows|emit_read_rows]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def csum_cases(ctx, n, seed, res):
    """ingot_gpu_checksum_verify on generator frames (random checksums: BAD,
    SHORT, FRAGMENT, NONE rows), then _fill and a second verify (OK rows), each
    against the model; packed frames of every chain's profile and 256-B slots."""
    import torch

    import ingot_amd
    from ingot_amd import CSUM_DTYPE, Chain, GenProfile
    from tests import csum_model as model

    def rows(t):
        return t.cpu().numpy().view(CSUM_DTYPE).reshape(-1)

    cases = [(GenProfile.MIXED, Chain.UdpParser, None),
             (GenProfile.ADVERSARIAL, Chain.GenericUlp, None),
             (GenProfile.VLAN_V6EH, Chain.VlanUlp, None), (GenProfile.FLOWS, Chain.VlanUlp, 256),
             (GenProfile.GENEVE, Chain.GeneveOverV6Tunnel, None),
             (GenProfile.GENEVE_ADVERSARIAL, Chain.GeneveOverV6Tunnel, None)]
    for k, (prof, chain, stride) in enumerate(cases):
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=seed + 70 + k, stride=stride)
        st = stride or 0
        recs = (ctx.parse_strided(arena, stride, n, chain, lens=lens) if stride
                else ctx.parse(arena, off, lens, chain))
        got_v = rows(ctx.checksum_verify(arena, off, lens, recs, stride=st, n=n))
        a = arena.cpu().numpy().copy()
        o = None if off is None else off.cpu().numpy().view(np.uint64)
        ln = None if lens is None else lens.cpu().numpy()
        rec = ingot_amd.records_to_numpy(recs)
        want_v = model.verify(a, o, ln, rec, 3, st, n)
        out = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
        ctx.checksum_fill(arena, off, lens, recs, stride=st, n=n, out=out)
        want_f = model.fill(a, o, ln, rec, 3, st, n)
        got_a = rows(ctx.checksum_verify(arena, off, lens, recs, stride=st, n=n))
        torch.cuda.synchronize()
        key = f"csum/{prof.name}/{chain.name}" + (f"/slots{stride}" if stride else "")
        res[key] = {
            "verify_row_mismatches": int((got_v.view(np.uint64) != want_v.view(np.uint64)).sum()),
            "fill_row_mismatches": int((rows(out).view(np.uint64) != want_f.view(np.uint64)).sum()),
            "fill_byte_mismatches": int((arena.cpu().numpy() != a).sum()),
            "verify_after_fill_row_mismatches": int((got_a.view(np.uint64)
                                                     != want_f.view(np.uint64)).sum()),
            "l4_states_before": np.bincount(want_v["l4_state"], minlength=6).tolist(),
            "l4_states_after": np.bincount(want_f["l4_state"], minlength=6).tolist()}
        print(key, res[key], flush=True)
        del arena, off, lens, recs, out
        torch.cuda.empty_cache()


def modify_csum_cases(ctx, n, seed, res):
    """ingot_gpu_parse_modify_csum against the oracle's rewrite followed by the
    update model: the checksum cases' profiles x chains x layouts (packed
    frames, 256-B slots with lengths) and 64- and 128-B slot rings, on the
    generator's frames as they are (random sums stay wrong by the same
    amount) and, every other case, with their sums filled first."""
    import torch

    import ingot_amd
    import oracle
    from ingot_amd import CSUM_L3, CSUM_L4, CSUM_OUTER_L4, Chain, EditOp, Field, GenProfile
    from tests import csum_update_model as upd

    def edits(l3):
        l4 = l3 + 1
        return [(l3, Field.V4_HOP_LIMIT, EditOp.SUB, 1), (l3, Field.V4_SOURCE, EditOp.SET, 0x0A000001),
                (l3, Field.V4_DESTINATION, EditOp.XOR, 0x00FF00FF),
                (l4, Field.UDP_DESTINATION, EditOp.SUB, 1), (l4, Field.TCP_SOURCE, EditOp.SET, 0),
                (l4, Field.TCP_FLAGS, EditOp.OR, 0x10), (l3, Field.V4_DSCP, EditOp.SET, 0x2E),
                (l3, Field.V6_HOP_LIMIT, EditOp.SUB, 1), (l4, Field.ICMP_CODE, EditOp.ADD, 1),
                (l3, Field.V4_FRAGMENT_OFFSET, EditOp.AND, 0x1F00),
                (l4, Field.UDP_CHECKSUM, EditOp.XOR, 0x0100), (l4, Field.TCP_SEQUENCE, EditOp.ADD,
                                                               0x80000001)]

    tun = Chain.GeneveOverV6Tunnel
    l3_of = {Chain.UdpParser: 1, Chain.GenericUlp: 1, Chain.VlanUlp: 2, tun: 5}
    cases = [(GenProfile.MIXED, Chain.UdpParser, None, True),
             (GenProfile.ADVERSARIAL, Chain.GenericUlp, None, True),
             (GenProfile.VLAN_V6EH, Chain.VlanUlp, None, True),
             (GenProfile.FLOWS, Chain.VlanUlp, 256, True),
             (GenProfile.GENEVE, tun, None, True), (GenProfile.GENEVE_ADVERSARIAL, tun, None, True),
             (GenProfile.V4UDP64, Chain.UdpParser, 64, False),
             (GenProfile.ADVERSARIAL, Chain.GenericUlp, 64, False),
             (GenProfile.MIXED, Chain.GenericUlp, 128, False),
             (GenProfile.VLAN_V6EH, Chain.VlanUlp, 128, False)]
    for k, (prof, chain, stride, with_lens) in enumerate(cases):
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=seed + 90 + k, stride=stride)
        if not with_lens:
            lens = None  # whole slots: the ring kernel
        st = stride or 0
        if k % 2:
            recs = (ctx.parse_strided(arena, stride, n, chain, lens=lens) if stride
                    else ctx.parse(arena, off, lens, chain))
            ctx.checksum_fill(arena, off, lens, recs, stride=st, n=n)
            torch.cuda.synchronize()
        before = arena.cpu().numpy().copy()
        o = None if off is None else off.cpu().numpy().view(np.uint64)
        ln = None if lens is None else lens.cpu().numpy()
        e = edits(l3_of[chain])
        what = CSUM_L3 | CSUM_L4
        if chain == tun:
            what |= CSUM_OUTER_L4
            e += [(3, Field.GENEVE_VNI, EditOp.ADD, 1), (2, Field.UDP_SOURCE, EditOp.XOR, 0x0FF0)]
        got_rec = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
        ctx.parse_modify(arena, off, lens, chain, e, stride=st, n=n, out=got_rec, csum=what)
        torch.cuda.synchronize()
        want = before.copy()
        w_rec = oracle.parse_modify_batch(want, o, ln, chain, e, stride=st, n=n, nthreads=16)
        o_udp = (oracle.geneve_fields_batch(before, o, ln, stride=st, n=n)["outer"]["outer_udp_off"]
                 if chain == tun else None)
        rewritten = want.copy()
        upd.update(before, want, o, ln, w_rec, what, o_udp=o_udp, stride=st, n=n)
        key = f"modify_csum/{prof.name}/{chain.name}" + (
            f"/slots{stride}" + ("" if with_lens else "_ring") if stride else "")
        res[key] = {
            "byte_mismatches": int((arena.cpu().numpy() != want).sum()),
            "record_mismatches": int((got_rec.cpu().numpy().reshape(n, -1) !=
                                      w_rec.view(np.uint8).reshape(n, -1)).any(axis=1).sum()),
            "sums_filled_first": bool(k % 2),
            "checksum_bytes_moved": int((want != rewritten).sum())}
        print(key, res[key], flush=True)
        del arena, off, lens, got_rec
        torch.cuda.empty_cache()


def emit_csum_cases(ctx, n, seed, res):
    """ingot_gpu_emit_packets_csum against the oracle's emit followed by the
    model: every header stack of tests/emit_csum_cases.py in front of the
    frames of four generator profiles, packed with 0-3 B gaps; the whole
    destination arena is compared."""
    import torch

    import ingot_amd
    import oracle
    from ingot_amd import GenProfile
    from tests import emit_csum_cases as cases
    from tests import emit_csum_model as model

    def dev(a):
        a = np.ascontiguousarray(a)
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
                  np.dtype(np.uint64): np.int64}
        return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()

    rng = np.random.default_rng(seed)
    profiles = (GenProfile.MIXED, GenProfile.VLAN_V6EH, GenProfile.ADVERSARIAL, GenProfile.GENEVE)
    for k, prof in enumerate(profiles):
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=seed + 110 + k)
        a, o, ln = arena.cpu().numpy(), off.cpu().numpy().view(np.uint64), lens.cpu().numpy()
        for name in cases.STACKS:
            hdr, sets, sums = cases.stack(name, n, rng)
            dst_off, size = cases.pack(ln, len(hdr), rng)
            dst = dev(np.full(size, 0xA5, np.uint8))
            dsets = [s if len(s) == 4 else (*s[:4], dev(s[4])) for s in sets]
            ctx.emit_packets(hdr, dsets, arena, off, lens, dst, dev(dst_off), sums=sums)
            torch.cuda.synchronize()
            want = np.full(size, 0xA5, np.uint8)
            oracle.emit_batch(hdr, sets, a, o, ln, want, dst_off, nthreads=16)
            plain = want.copy()
            model.apply(want, hdr, sums, dst_off, ln, sets)
            key = f"emit_csum/{prof.name}/{name}"
            res[key] = {"byte_mismatches": int((dst.cpu().numpy() != want).sum()),
                        "checksum_bytes_moved": int((want != plain).sum()),
                        "arena_bytes": size}
            print(key, res[key], flush=True)
            del dst
        del arena, off, lens
        torch.cuda.empty_cache()


def csum_read_cases(ctx, n, seed, res):
    """ingot_gpu_checksum_verify_read, then _fill_read and a second verify, over
    generator frames cut into chunks (tests/csum_read_cases.py: header cuts at
    layer edges, payload cuts anywhere, empty chunks, every chunk at its own
    misalignment) with the device's own parse_read records, against the model
    of tests/csum_read_model.py.  Every other case has its sums filled first
    (OK rows), the others keep the generator's random sums (BAD rows)."""
    import torch

    import ingot_amd
    from ingot_amd import CSUM_DTYPE, Chain, GenProfile
    from tests import csum_read_cases as cases
    from tests import csum_read_model as model

    def rows(t):
        return t.cpu().numpy().view(CSUM_DTYPE).reshape(-1)

    def dev(a):
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
                  np.dtype(np.uint64): np.int64}
        return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()

    pairs = [(GenProfile.MIXED, Chain.GenericUlp), (GenProfile.VLAN_V6EH, Chain.VlanUlp),
             (GenProfile.GENEVE, Chain.GeneveOverV6Tunnel), (GenProfile.MIXED, Chain.UdpParser),
             (GenProfile.ADVERSARIAL, Chain.GenericUlp)]
    for k, (prof, chain) in enumerate(pairs):
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=seed + 130 + k)
        recs = ctx.parse(arena, off, lens, chain)
        if k % 2:
            ctx.checksum_fill(arena, off, lens, recs)
        torch.cuda.synchronize()
        rng = np.random.default_rng(seed + 130 + k)
        crec = ingot_amd.records_to_numpy(recs)
        frames = cases.frames_of(arena.cpu().numpy(), off.cpu().numpy().view(np.uint64),
                                 lens.cpu().numpy())
        packets = [cases.cut(f, crec[i], rng) for i, f in enumerate(frames)]
        a, so, sl, ps = cases.place(packets, misalign=list(range(16)) + [int(rng.integers(16))],
                                    gap=int(rng.integers(0, 4)))
        d_a, d_tab = dev(a), (dev(so), dev(sl), dev(ps))
        d_rec, _ = ctx.parse_read(d_a, *d_tab, chain)
        rec = ingot_amd.records_to_numpy(d_rec)
        got_v = rows(ctx.checksum_verify_read(d_a, *d_tab, d_rec))
        wrote = int((d_a.cpu().numpy() != a).sum())
        want_v = model.verify((a, so, sl, ps), rec)
        out = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
        ctx.checksum_fill_read(d_a, *d_tab, d_rec, out=out)
        want_f = model.fill((a, so, sl, ps), rec)
        got_a = rows(ctx.checksum_verify_read(d_a, *d_tab, d_rec))
        torch.cuda.synchronize()
        key = f"csum_read/{prof.name}/{chain.name}"
        res[key] = {
            "records_unlike_the_contiguous_parse": int((rec.view(np.uint8).reshape(n, -1) !=
                                                          crec.view(np.uint8).reshape(n, -1))
                                                         .any(axis=1).sum()),
            "verify_row_mismatches": int((got_v.view(np.uint64) != want_v.view(np.uint64)).sum()),
            "verify_byte_mismatches": wrote,
            "fill_row_mismatches": int((rows(out).view(np.uint64) != want_f.view(np.uint64)).sum()),
            "fill_byte_mismatches": int((d_a.cpu().numpy() != a).sum()),
            "verify_after_fill_row_mismatches": int((got_a.view(np.uint64)
                                                     != want_f.view(np.uint64)).sum()),
            "sums_filled_first": bool(k % 2),
            "chunks": int(ps[-1]), "chunks_per_packet_max": int(np.diff(ps.astype(np.int64)).max()),
            "l4_states_before": np.bincount(want_v["l4_state"], minlength=6).tolist(),
            "l4_states_after": np.bincount(want_f["l4_state"], minlength=6).tolist()}
        print(key, res[key], flush=True)
        del arena, off, lens, recs, out, d_a, d_tab, d_rec
        torch.cuda.empty_cache()


def modify_read_cases(ctx, n, seed, res):
    """ingot_gpu_parse_read_modify / _csum over csum_read's generator profiles x
    chains, cut by tests/csum_read_cases.py's `cut`, with random edit lists of
    tests/csum_sweep_cases.py (and every `what` of the chain in turn, 0
    included), against tests/modify_read_model.py: the whole arena, the
    records and the chunk indices.  Every other case has its sums filled
    first."""
    import torch

    import ingot_amd
    from ingot_amd import Chain, GenProfile
    from tests import csum_read_cases as cases
    from tests import csum_sweep_cases as sc
    from tests import modify_read_model as model

    def dev(a):
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
                  np.dtype(np.uint64): np.int64}
        return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()

    pairs = [(GenProfile.MIXED, Chain.GenericUlp), (GenProfile.VLAN_V6EH, Chain.VlanUlp),
             (GenProfile.GENEVE, Chain.GeneveOverV6Tunnel), (GenProfile.MIXED, Chain.UdpParser),
             (GenProfile.ADVERSARIAL, Chain.GenericUlp)]
    for k, (prof, chain) in enumerate(pairs):
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=seed + 160 + k)
        recs = ctx.parse(arena, off, lens, chain)
        if k % 2:
            ctx.checksum_fill(arena, off, lens, recs)
        torch.cuda.synchronize()
        rng = np.random.default_rng(seed + 160 + k)
        crec = ingot_amd.records_to_numpy(recs)
        frames = cases.frames_of(arena.cpu().numpy(), off.cpu().numpy().view(np.uint64),
                                 lens.cpu().numpy())
        packets = [cases.cut(f, crec[i], rng) for i, f in enumerate(frames)]
        tables = cases.place(packets, misalign=list(range(16)) + [int(rng.integers(16))],
                             gap=int(rng.integers(0, 4)))
        parsed = model.parse(tables, chain)
        pristine, d_tab = dev(tables[0]), [dev(x) for x in tables[1:]]
        out = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
        chunk = torch.zeros(n, dtype=torch.int16, device="cuda")
        whats = (0,) + tuple(sc.WHATS[chain])
        lists = sc.random_lists(chain, 6, seed=seed + k)
        bytes_bad = recs_bad = chunk_bad = edited = 0
        for j, edits in enumerate(lists):
            what = whats[j % len(whats)]
            want, w_rec, w_chunk = model.apply(tables, chain, edits, what, parsed=parsed)
            d_a = pristine.clone()
            ctx.parse_read_modify(d_a, *d_tab, chain, edits, csum=what, out=out, chunk=chunk)
            got = d_a.cpu().numpy()
            bytes_bad += int((got != want).sum())
            recs_bad += int((out.cpu().numpy() != w_rec.view(np.uint8).reshape(n, 16))
                            .any(axis=1).sum())
            chunk_bad += int((chunk.cpu().numpy().view(np.uint16) != w_chunk).sum())
            edited += int((want != tables[0]).sum())
        key = f"modify_read/{prof.name}/{chain.name}"
        res[key] = {"byte_mismatches": bytes_bad, "record_mismatches": recs_bad,
                    "chunk_mismatches": chunk_bad, "edit_lists": len(lists),
                    "bytes_edited": edited, "ok_packets": int((parsed[0]["status"] == 0).sum()),
                    "chunks": int(tables[3][-1]), "sums_filled_first": bool(k % 2)}
        print(key, res[key], flush=True)
        del arena, off, lens, recs, out, chunk, pristine, d_tab
        torch.cuda.empty_cache()


def modify_read_rows_cases(ctx, n, seed, res):
    """ingot_gpu_parse_read_modify_rows over modify_read's five sets (the same
    generator profiles x chains, cut by tests/csum_read_cases.py's `cut`), with
    the random mixed lists of tests/modify_read_rows_cases.py (wide and narrow
    fields, every op, VALUE / U16 / U32 / BYTES operands by packet and by row),
    random guards and every `what` of the chain in turn, 0 included, against
    tests/modify_read_rows_model.py: the whole arena, the records and the chunk
    indices.  Every other case has its sums filled first."""
    import torch

    import ingot_amd
    from ingot_amd import Chain, GenProfile
    from ingot_amd.abi import ROW_NONE
    from tests import csum_read_cases as cases
    from tests import modify_read_model as mrm
    from tests import modify_read_rows_cases as rc2
    from tests import modify_read_rows_model as model
    from tests import modify_rows_cases as rc

    def dev(a):
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
                  np.dtype(np.uint64): np.int64}
        return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()

    pairs = [(GenProfile.MIXED, Chain.GenericUlp), (GenProfile.VLAN_V6EH, Chain.VlanUlp),
             (GenProfile.GENEVE, Chain.GeneveOverV6Tunnel), (GenProfile.MIXED, Chain.UdpParser),
             (GenProfile.ADVERSARIAL, Chain.GenericUlp)]
    for k, (prof, chain) in enumerate(pairs):
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=seed + 210 + k)
        recs = ctx.parse(arena, off, lens, chain)
        if k % 2:
            ctx.checksum_fill(arena, off, lens, recs)
        torch.cuda.synchronize()
        rng = np.random.default_rng(seed + 210 + k)
        crec = ingot_amd.records_to_numpy(recs)
        frames = cases.frames_of(arena.cpu().numpy(), off.cpu().numpy().view(np.uint64),
                                 lens.cpu().numpy())
        packets = [cases.cut(f, crec[i], rng) for i, f in enumerate(frames)]
        tables = cases.place(packets, misalign=list(range(16)) + [int(rng.integers(16))],
                             gap=int(rng.integers(0, 4)))
        parsed = mrm.parse(tables, chain)
        pristine, d_tab = dev(tables[0]), [dev(x) for x in tables[1:]]
        out = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
        chunk = torch.zeros(n, dtype=torch.int16, device="cuda")
        whats = rc2.valid_whats(chain)
        lists = rc2.random_lists(chain, n, len(whats), seed=seed + k)
        bytes_bad = recs_bad = chunk_bad = edited = guarded = 0
        uploads = {}
        for j, edits in enumerate(lists):
            what = whats[j]
            rows = rng.integers(0, rc2.N_ROWS, n).astype(np.uint32)
            rows[rng.random(n) < 0.2] = ROW_NONE
            rows[rng.random(n) < 0.05] = rc2.N_ROWS
            want, w_rec, w_chunk = model.apply(tables, chain, edits, rows, rc2.N_ROWS, what,
                                               parsed=parsed)
            d_a = pristine.clone()
            out.fill_(0xEE)
            chunk.fill_(-1)
            ctx.parse_read_modify_rows(d_a, *d_tab, chain, rc.device_edits(torch, edits, uploads),
                                       rows=dev(rows), n_rows=rc2.N_ROWS, csum=what, out=out,
                                       chunk=chunk)
            got = d_a.cpu().numpy()
            bytes_bad += int((got != want).sum())
            recs_bad += int((out.cpu().numpy() != w_rec.view(np.uint8).reshape(n, 16))
                            .any(axis=1).sum())
            chunk_bad += int((chunk.cpu().numpy().view(np.uint16) != w_chunk).sum())
            edited += int((want != tables[0]).sum())
            guarded += int((rows >= rc2.N_ROWS).sum())
        key = f"modify_read_rows/{prof.name}/{chain.name}"
        res[key] = {"byte_mismatches": bytes_bad, "record_mismatches": recs_bad,
                    "chunk_mismatches": chunk_bad, "edit_lists": len(lists), "whats": list(whats),
                    "bytes_edited": edited, "guarded": guarded,
                    "ok_packets": int((parsed[0]["status"] == 0).sum()),
                    "chunks": int(tables[3][-1]), "sums_filled_first": bool(k % 2)}
        print(key, res[key], flush=True)
        del arena, off, lens, recs, out, chunk, pristine, d_tab
        torch.cuda.empty_cache()


def emit_read_cases(ctx, n, seed, res):
    """ingot_gpu_emit_packets_read against tests/emit_read_model.py: every
    header stack of tests/emit_csum_cases.py in front of the frames of four
    generator profiles cut by tests/csum_read_cases.py's `cut` (up to 9
    chunks, empty ones included, every chunk at its own misalignment), with
    random d_from / d_take (half of the packets whole); the whole destination
    arena and d_taken are compared."""
    import torch

    import ingot_amd
    from ingot_amd import Chain, GenProfile
    from tests import csum_read_cases as chunks
    from tests import emit_csum_cases as cases
    from tests import emit_read_model as model

    def dev(a):
        a = np.ascontiguousarray(a)
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
                  np.dtype(np.uint64): np.int64}
        return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()

    rng = np.random.default_rng(seed)
    pairs = ((GenProfile.MIXED, Chain.GenericUlp), (GenProfile.VLAN_V6EH, Chain.VlanUlp),
             (GenProfile.ADVERSARIAL, Chain.GenericUlp),
             (GenProfile.GENEVE, Chain.GeneveOverV6Tunnel))
    for k, (prof, chain) in enumerate(pairs):
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=seed + 150 + k)
        crec = ingot_amd.records_to_numpy(ctx.parse(arena, off, lens, chain))
        ln = lens.cpu().numpy()
        frames = chunks.frames_of(arena.cpu().numpy(), off.cpu().numpy().view(np.uint64), ln)
        packets = [chunks.cut(f, crec[i], rng) for i, f in enumerate(frames)]
        tables = chunks.place(packets, misalign=list(range(16)) + [int(rng.integers(16))],
                              gap=int(rng.integers(0, 4)))
        d_tab = [dev(x) for x in tables]
        del arena, off, lens
        for name in cases.STACKS:
            hdr, sets, sums = cases.stack(name, n, rng)
            whole = rng.random(n) < 0.5
            frm = np.where(whole, 0, rng.integers(0, ln.astype(np.int64) + 10)).astype(np.uint16)
            take = np.where(rng.random(n) < 0.5, 65535,
                            rng.integers(0, ln.astype(np.int64) + 10)).astype(np.uint16)
            t = model.linearise(*tables, frm, take)[2]
            dst_off, size = cases.pack(t, len(hdr), rng)
            want, lens_want = model.apply(np.full(size, 0xA5, np.uint8), hdr, sets, sums, *tables,
                                          dst_off, frm, take)
            dst = dev(np.full(size, 0xA5, np.uint8))
            taken = dev(np.full(n, 0xA5A5, np.uint16))
            dsets = [s if len(s) == 4 else (*s[:4], dev(s[4])) for s in sets]
            ctx.emit_packets_read(hdr, dsets, *d_tab, dst, dev(dst_off), frm=dev(frm),
                                  take=dev(take), taken=taken, sums=sums)
            torch.cuda.synchronize()
            key = f"emit_read/{prof.name}/{name}"
            res[key] = {"byte_mismatches": int((dst.cpu().numpy() != want).sum()),
                        "taken_mismatches": int((taken.cpu().numpy().view(np.uint16)
                                                 != lens_want).sum()),
                        "arena_bytes": size, "chunks": int(tables[3][-1]),
                        "chunks_per_packet_max": int(np.diff(tables[3].astype(np.int64)).max()),
                        "packets_cut_short": int((t < ln).sum())}
            print(key, res[key], flush=True)
            del dst, taken
        del d_tab
        torch.cuda.empty_cache()


def emit_rows_cases(ctx, n, seed, res):
    """ingot_gpu_emit_packets_rows against tests/emit_rows_model.py, from the
    generators of tests/emit_rows_cases.py: every stack with every table form
    in front of generator frames, the row of each packet its flow bin (the
    uncounted packets are not emitted) and, for 1 packet in 16, a row past
    the table; whole destination arenas are compared."""
    import torch

    import ingot_amd
    from ingot_amd import Chain, GenProfile
    from tests import emit_rows_cases as rc
    from tests import emit_rows_model as model

    def dev(a):
        a = np.ascontiguousarray(a)
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
                  np.dtype(np.uint64): np.int64}
        return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()

    rng = np.random.default_rng(seed)
    bins = 4096
    for k, prof in enumerate((GenProfile.MIXED, GenProfile.ADVERSARIAL)):
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=seed + 170 + k)
        flow = ctx.flow_hist(arena, off, lens, Chain.GenericUlp, bins=bins)
        rows = flow.cpu().numpy().view(np.uint32).copy()
        rows[rng.random(n) < 1 / 16] = bins
        live = rows < bins
        src, s_off, ln = arena.cpu().numpy(), off.cpu().numpy().view(np.uint64), lens.cpu().numpy()
        d_src, d_off, d_len, d_rows = arena, off, lens, dev(rows)
        for name in rc.STACKS:
            for form in rc.FORMS:
                case = rc.stack(name, form, n, bins, rng)
                tot = np.where(live, len(case.hdr) + ln.astype(np.int64), 0)
                gaps = np.where(live, rng.integers(0, 4, n), 0)
                dst_off = (np.cumsum(np.r_[0, (tot + gaps)[:-1]]) + 5).astype(np.uint64)
                size = int(dst_off[-1] + tot[-1] + 64)
                want = np.full(size, 0xA5, np.uint8)
                model.apply(want, case.hdr, case.host_sets(), case.sums, src, s_off, ln, dst_off,
                            rows, bins)
                dst = dev(np.full(size, 0xA5, np.uint8))
                backing = {key: dev(v) for key, v in case.backing.items()}
                ctx.emit_packets_rows(case.hdr, case.device_sets(backing), d_src, d_off, d_len, dst,
                                      dev(dst_off), rows=d_rows, n_rows=bins, sums=case.sums)
                torch.cuda.synchronize()
                key = f"emit_rows/{prof.name}/{name}/{form}"
                res[key] = {"byte_mismatches": int((dst.cpu().numpy() != want).sum()),
                            "arena_bytes": size, "emitted": int(live.sum()),
                            "not_emitted": int((~live).sum())}
                print(key, res[key], flush=True)
                del dst, backing
        torch.cuda.empty_cache()


def emit_read_rows_cases(ctx, n, seed, res):
    """ingot_gpu_emit_packets_read_rows against tests/emit_read_rows_model.py:
    emit_rows_cases' stacks, table forms and rows (the flow bin; 1 packet in
    16 a row past the table) over emit_read_cases' cut frames and random
    d_from / d_take.  A packet that is not emitted has chunk offsets of 2^60,
    chunk lengths of 65,535 and a destination outside the arena; the whole
    destination arena and d_taken are compared."""
    import torch

    import ingot_amd
    from ingot_amd import Chain, GenProfile
    from tests import csum_read_cases as chunks
    from tests import emit_read_model
    from tests import emit_read_rows_cases as rrc
    from tests import emit_read_rows_model as model
    from tests import emit_rows_cases as rc

    def dev(a):
        a = np.ascontiguousarray(a)
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
                  np.dtype(np.uint64): np.int64}
        return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()

    rng = np.random.default_rng(seed)
    bins = 4096
    for k, prof in enumerate((GenProfile.MIXED, GenProfile.ADVERSARIAL)):
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=seed + 190 + k)
        flow = ctx.flow_hist(arena, off, lens, Chain.GenericUlp, bins=bins)
        rows = flow.cpu().numpy().view(np.uint32).copy()
        rows[rng.random(n) < 1 / 16] = bins
        live = rows < bins
        crec = ingot_amd.records_to_numpy(ctx.parse(arena, off, lens, Chain.GenericUlp))
        ln = lens.cpu().numpy()
        frames = chunks.frames_of(arena.cpu().numpy(), off.cpu().numpy().view(np.uint64), ln)
        packets = [chunks.cut(f, crec[i], rng) for i, f in enumerate(frames)]
        src, seg_off, seg_len, pkt_seg = chunks.place(
            packets, misalign=list(range(16)) + [int(rng.integers(16))], gap=int(rng.integers(0, 4)))
        whole = rng.random(n) < 0.5
        frm = np.where(whole, 0, rng.integers(0, ln.astype(np.int64) + 10)).astype(np.uint16)
        take = np.where(rng.random(n) < 0.5, 65535,
                        rng.integers(0, ln.astype(np.int64) + 10)).astype(np.uint16)
        t = emit_read_model.linearise(src, seg_off, seg_len, pkt_seg, frm, take)[2]
        seg_off, seg_len = seg_off.copy(), seg_len.copy()
        for i in np.nonzero(~live)[0]:
            seg_off[int(pkt_seg[i]):int(pkt_seg[i + 1])] = rrc.POISON_OFF
            seg_len[int(pkt_seg[i]):int(pkt_seg[i + 1])] = 65535
        tables = (src, seg_off, seg_len, pkt_seg)
        d_tab, d_rows = [dev(x) for x in tables], dev(rows)
        del arena, off, lens
        for name in rc.STACKS:
            for form in rc.FORMS:
                case = rc.stack(name, form, n, bins, rng)
                dst_off, size = rrc.pack_live(len(case.hdr) + t.astype(np.int64), live, rng)
                dst_off[~live] = rrc.POISON_DST
                want, taken_want = model.apply(np.full(size, 0xA5, np.uint8), case.hdr,
                                               case.host_sets(), case.sums, *tables, dst_off,
                                               rows, bins, frm, take)
                dst = dev(np.full(size, 0xA5, np.uint8))
                taken = dev(np.full(n, 0xA5A5, np.uint16))
                backing = {key: dev(v) for key, v in case.backing.items()}
                ctx.emit_packets_read_rows(case.hdr, case.device_sets(backing), *d_tab, dst,
                                           dev(dst_off), rows=d_rows, n_rows=bins, frm=dev(frm),
                                           take=dev(take), taken=taken, sums=case.sums)
                torch.cuda.synchronize()
                key = f"emit_read_rows/{prof.name}/{name}/{form}"
                res[key] = {"byte_mismatches": int((dst.cpu().numpy() != want).sum()),
                            "taken_mismatches": int((taken.cpu().numpy().view(np.uint16)
                                                     != taken_want).sum()),
                            "arena_bytes": size, "chunks": int(pkt_seg[-1]),
                            "emitted": int(live.sum()), "not_emitted": int((~live).sum())}
                print(key, res[key], flush=True)
                del dst, taken, backing
        del d_tab
        torch.cuda.empty_cache()


def finish(n, seed, t0, res):
    out = {"frames_per_case": n, "seed": seed, "wall_s": round(time.time() - t0, 1),
           "cases": res,
           "all_zero": all(v == 0 for c in res.values() for k, v in c.items() if "mismatch" in k)}
    print(json.dumps(out))
    (ROOT / "gpurun_out").mkdir(exist_ok=True)
    (ROOT / "gpurun_out" / "bigfuzz.json").write_text(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4_000_000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--csum-frames", type=int, default=200_000,
                    help="frames per csum case (its reference is a Python model)")
    ap.add_argument("--only", default="",
                    help="'csum' / 'modify_csum' / 'emit_csum' / 'csum_read' / 'modify_read' / "
                         "'emit_read' / 'emit_rows' / 'modify_read_rows' / 'emit_read_rows': run "
                         "only that case group")
    args = ap.parse_args()
    if args.only in ("csum", "modify_csum", "emit_csum", "csum_read", "modify_read", "emit_read",
                     "emit_rows", "modify_read_rows", "emit_read_rows"):
        import ingot_amd

        res, t0 = {}, time.time()
        group = {"csum": csum_cases, "modify_csum": modify_csum_cases,
                 "emit_csum": emit_csum_cases, "csum_read": csum_read_cases,
                 "modify_read": modify_read_cases, "emit_read": emit_read_cases,
                 "emit_rows": emit_rows_cases,
                 "modify_read_rows": modify_read_rows_cases,
                 "emit_read_rows": emit_read_rows_cases}[args.only]
        group(ingot_amd.Context(0), min(args.frames, args.csum_frames), args.seed, res)
        return finish(min(args.frames, args.csum_frames), args.seed, t0, res)

    import torch

    import ingot_amd
    import oracle
    from ingot_amd import Chain, GenProfile

    ctx = ingot_amd.Context(0)
    n, res, t0 = args.frames, {}, time.time()
    for chain in Chain:
        prof = (GenProfile.GENEVE_ADVERSARIAL if chain == Chain.GeneveOverV6Tunnel
                else GenProfile.ADVERSARIAL)
        for layout in ("packed", "slots256"):
            stride = 256 if layout == "slots256" else None
            arena, off, lens = ingot_amd.gen_frames(prof, n, seed=args.seed + int(chain),
                                                    stride=stride)
            if stride:
                recs = ctx.parse_strided(arena, stride, n, chain, lens=lens)
            else:
                recs = ctx.parse(arena, off, lens, chain)
            if chain == Chain.GeneveOverV6Tunnel:
                flds = ctx.geneve_fields(arena, off, lens, stride=stride or 0, n=n)
            else:
                flds = ctx.fields(arena, off, lens, chain, stride=stride or 0, n=n)
            torch.cuda.synchronize()
            a = arena.cpu().numpy()
            o = None if off is None else off.cpu().numpy()
            ln = None if lens is None else lens.cpu().numpy()
            w_rec = oracle.parse_batch(a, o, ln, chain, stride=stride or 0, n=n, nthreads=16)
            if chain == Chain.GeneveOverV6Tunnel:
                w_fld = oracle.geneve_fields_batch(a, o, ln, stride=stride or 0, n=n)
            else:
                _, w_fld = oracle.parse_batch(a, o, ln, chain, stride=stride or 0, n=n,
                                              fields=True, nthreads=16)
            g_rec = recs.cpu().numpy().reshape(n, -1)
            g_fld = flds.cpu().numpy().reshape(n, -1)
            bad_r = int((g_rec != w_rec.view(np.uint8).reshape(n, -1)).any(axis=1).sum())
            bad_f = int((g_fld != w_fld.view(np.uint8).reshape(n, -1)).any(axis=1).sum())
            st = g_rec[:, 0]
            res[f"{chain.name}/{layout}"] = {"record_mismatches": bad_r, "field_mismatches": bad_f,
                                            "ok_fraction": round(float((st == 0).mean()), 4)}
            print(chain.name, layout, res[f"{chain.name}/{layout}"], flush=True)
            del arena, off, lens, recs, flds
            torch.cuda.empty_cache()
    # parse_read over random chunk splits with every staging plan
    from ingot_amd.abi import TUNE_READ_PLAN

    for chain in Chain:
        prof = (GenProfile.GENEVE_ADVERSARIAL if chain == Chain.GeneveOverV6Tunnel
                else GenProfile.ADVERSARIAL)
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=args.seed + 10 + int(chain))
        a, o, ln = arena.cpu().numpy(), off.cpu().numpy(), lens.cpu().numpy()
        # 4 chunks per packet at 3 sorted random cuts (empty chunks included)
        rng = np.random.default_rng(args.seed + int(chain))
        cuts = np.sort(rng.integers(0, ln.astype(np.int64)[:, None] + 1, size=(n, 3)), axis=1)
        bounds = np.concatenate([np.zeros((n, 1), np.int64), cuts,
                                 ln.astype(np.int64)[:, None]], axis=1)
        seg_off = (o.astype(np.int64)[:, None] + bounds[:, :4]).reshape(-1)
        seg_len = (bounds[:, 1:] - bounds[:, :4]).reshape(-1).astype(np.uint16)
        pkt_seg = (np.arange(n + 1, dtype=np.int64) * 4).astype(np.uint32)
        w_r, _, w_ch = oracle.parse_read_batch(a, seg_off.view(np.uint64), seg_len, pkt_seg,
                                                chain, nthreads=16)
        d_so = torch.from_numpy(seg_off).cuda()
        d_sl = torch.from_numpy(seg_len.view(np.int16)).cuda()
        d_ps = torch.from_numpy(pkt_seg.view(np.int32)).cuda()
        for plan in (0, 1):
            c2 = ingot_amd.Context(0)
            c2.set_tuning(TUNE_READ_PLAN, plan)
            r, ch = c2.parse_read(arena, d_so, d_sl, d_ps, chain)
            torch.cuda.synchronize()
            bad = int((r.cpu().numpy().reshape(n, -1) != w_r.view(np.uint8).reshape(n, -1))
                      .any(axis=1).sum())
            badc = int((ch.cpu().numpy().view(np.uint16) != w_ch).sum())
            res[f"{chain.name}/parse_read_plan{plan}"] = {"record_mismatches": bad,
                                                          "chunk_mismatches": badc}
            print(chain.name, f"parse_read plan {plan}", res[f"{chain.name}/parse_read_plan{plan}"],
                  flush=True)
        # round 3/4: chunk 0 per packet (parse_read_first), bounds per tile or
        # on demand (READ_PLAN 17)
        first = ingot_amd.first_chunks(d_so, d_sl, d_ps)
        for plan in (0, 17):
            c2 = ingot_amd.Context(0)
            c2.set_tuning(TUNE_READ_PLAN, plan)
            r, ch = c2.parse_read(arena, d_so, d_sl, d_ps, chain, first=first)
            torch.cuda.synchronize()
            bad = int((r.cpu().numpy().reshape(n, -1) != w_r.view(np.uint8).reshape(n, -1))
                      .any(axis=1).sum())
            badc = int((ch.cpu().numpy().view(np.uint16) != w_ch).sum())
            key = f"{chain.name}/parse_read_first" + ("_lazy" if plan else "")
            res[key] = {"record_mismatches": bad, "chunk_mismatches": badc}
            print(chain.name, key, res[key], flush=True)
        del arena, off, lens, d_so, d_sl, d_ps, first
        torch.cuda.empty_cache()
    # flows on the VLAN chain
    arena, off, lens = ingot_amd.gen_frames(GenProfile.FLOWS, n, seed=args.seed)
    flow16 = ctx.flow_hist(arena, off, lens, Chain.VlanUlp)  # no hashes: the 16-bit table
    hashes = torch.zeros(n, dtype=torch.int32, device="cuda")
    flow = ctx.flow_hist(arena, off, lens, Chain.VlanUlp, hashes=hashes)
    torch.cuda.synchronize()
    _, w_hash = oracle.flow_hist(arena.cpu().numpy(), off.cpu().numpy(), lens.cpu().numpy(),
                                 Chain.VlanUlp)
    w_flow = oracle.flow_hist.last_flows
    res["flows/VlanUlp"] = {
        "hash_mismatches": int((hashes.cpu().numpy().view(np.uint32) != w_hash).sum()),
        "flow_mismatches": int((flow.cpu().numpy().view(np.uint32) != w_flow).sum()),
        "flow16_mismatches": int((flow16.cpu().numpy().view(np.uint32) != w_flow).sum())}
    print("flows", res["flows/VlanUlp"], flush=True)
    # k_parse's flows mode (explicit windows) beside the default k_flows_bits,
    # on the FLOWS frames and on adversarial frames
    from ingot_amd.abi import TUNE_WINDOW_INDEXED

    for fk in (0, 1025, 1056):  # 0: k_flows_bits; else k_parse flows with that window
        c4 = ingot_amd.Context(0)
        c4.set_tuning(TUNE_WINDOW_INDEXED, fk)
        f4 = c4.flow_hist(arena, off, lens, Chain.VlanUlp)
        torch.cuda.synchronize()
        res[f"flows/VlanUlp/win{fk}"] = {
            "flow_mismatches": int((f4.cpu().numpy().view(np.uint32) != w_flow).sum())}
        print("flows", fk, res[f"flows/VlanUlp/win{fk}"], flush=True)
    del arena, off, lens
    torch.cuda.empty_cache()
    for chain in (Chain.GenericUlp, Chain.VlanUlp):
        arena, off, lens = ingot_amd.gen_frames(GenProfile.ADVERSARIAL, n,
                                                seed=args.seed + 40 + int(chain))
        oracle.flow_hist(arena.cpu().numpy(), off.cpu().numpy(), lens.cpu().numpy(), chain)
        w_adv = oracle.flow_hist.last_flows
        for fk in (0, 1025, 1056):
            c4 = ingot_amd.Context(0)
            c4.set_tuning(TUNE_WINDOW_INDEXED, fk)
            f4 = c4.flow_hist(arena, off, lens, chain)
            torch.cuda.synchronize()
            key = f"flows_adversarial/{chain.name}/win{fk}"
            res[key] = {"flow_mismatches": int((f4.cpu().numpy().view(np.uint32) != w_adv).sum())}
            print(key, res[key], flush=True)
        del arena, off, lens
        torch.cuda.empty_cache()
    # the C2 slot-ring kernel (64-B slots, no lengths) over adversarial
    # bytes, 16- and 8-B records
    for chain in (Chain.UdpParser, Chain.GenericUlp, Chain.VlanUlp):
        arena, _, _ = ingot_amd.gen_frames(GenProfile.ADVERSARIAL, n, seed=args.seed + 20 +
                                           int(chain), stride=64)
        w_rec = oracle.parse_batch(arena.cpu().numpy(), None, None, chain, stride=64, n=n,
                                   nthreads=16)
        g16 = ctx.parse_strided(arena, 64, n, chain)
        g8 = ctx.parse_strided_compact(arena, 64, n, chain)
        torch.cuda.synchronize()
        bad16 = int((g16.cpu().numpy().reshape(n, -1) != w_rec.view(np.uint8).reshape(n, -1))
                    .any(axis=1).sum())
        from ingot_amd.abi import rec16_to_rec8

        w8 = rec16_to_rec8(w_rec)
        r = {"record_mismatches": bad16,
             "rec8_mismatches": int((g8.cpu().numpy().reshape(n, -1) !=
                                     w8.view(np.uint8).reshape(n, -1)).any(axis=1).sum())}
        res[f"{chain.name}/ring64"] = r
        print(chain.name, "ring64", r, flush=True)
        # every LDS-image count of the ring kernel (0 = the default, a single
        # image restaged in place) at 1 to 4 blocks per CU
        from ingot_amd.abi import TUNE_PIPE_DEPTH, TUNE_RING_GRID

        for depth in (0, 2, 3, 4):
            for grid in (1, 2, 3, 4) if depth <= 2 else (0,):
                c5 = ingot_amd.Context(0)
                c5.set_tuning(TUNE_PIPE_DEPTH, depth)
                c5.set_tuning(TUNE_RING_GRID, grid)
                d16 = c5.parse_strided(arena, 64, n, chain)
                d8 = c5.parse_strided_compact(arena, 64, n, chain)
                torch.cuda.synchronize()
                key = f"{chain.name}/ring64/depth{depth}/grid{grid}"
                res[key] = {"record_mismatches": int((~(d16 == g16).all(dim=1)).sum().item()) + bad16,
                            "rec8_mismatches": int((~(d8 == g8).all(dim=1)).sum().item()) +
                            r["rec8_mismatches"]}
                print(key, res[key], flush=True)
                del d16, d8
        del arena, g16, g8
        torch.cuda.empty_cache()
    # batched Emit (ingot_gpu_emit_packets / _headers): random header blocks
    # (1-256 B) with random setters over generator frames, destinations packed
    # with random gaps (the bytes between packets must stay untouched)
    from ingot_amd import EmitSource, Field

    for case in range(3):
        rng = np.random.default_rng(args.seed + 50 + case)
        prof = (GenProfile.MIXED, GenProfile.ADVERSARIAL, GenProfile.GENEVE)[case]
        arena, off, lens = ingot_amd.gen_frames(prof, n, seed=args.seed + 60 + case)
        H = int(rng.integers(1, 257))
        hdr = rng.integers(0, 256, H, dtype=np.uint8).tobytes()
        u16 = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
        u32 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        host_sets, dev_sets = [], []
        fields = [f for f in Field]
        for _ in range(int(rng.integers(0, 9))):
            f = fields[int(rng.integers(0, len(fields)))]
            at = int(rng.integers(0, max(1, H - 3)))
            src = EmitSource(int(rng.integers(0, 4)))
            add = int(rng.integers(-(1 << 31), 1 << 31))
            vals = u16 if src == EmitSource.U16 else u32 if src == EmitSource.U32 else None
            host_sets.append((at, f, src, add) + ((vals,) if vals is not None else ()))
            dev_sets.append((at, f, src, add) + (
                (torch.from_numpy(vals.view(np.int16 if vals.dtype == np.uint16 else np.int32))
                 .cuda(),) if vals is not None else ()))
        # drop setters whose field would not lie inside the header block
        keep = []
        for hs, ds in zip(host_sets, dev_sets):
            try:
                oracle.emit_batch(hdr, [hs[:4] + hs[4:5]], np.zeros(16, np.uint8), [0], [0],
                                  np.zeros(H + 16, np.uint8), [0])
                keep.append((hs, ds))
            except ValueError:
                pass
        host_sets = [k[0] for k in keep]
        dev_sets = [k[1] for k in keep]
        ln = lens.cpu().numpy()
        tot = H + ln.astype(np.int64)
        gaps = rng.integers(0, 33, n)
        dst_off = np.cumsum(np.r_[0, (tot + gaps)[:-1]]) + int(rng.integers(0, 16))
        fill = rng.integers(0, 256, int(dst_off[-1] + tot[-1] + 64), dtype=np.uint8)
        dst = torch.from_numpy(fill).cuda()
        ctx.emit_packets(hdr, dev_sets, arena, off, lens, dst,
                         torch.from_numpy(dst_off.astype(np.int64)).cuda())
        # header blocks into each frame's headroom of a second copy
        hfill = rng.integers(0, 256, int(dst_off[-1] + tot[-1] + 64), dtype=np.uint8)
        hdst = torch.from_numpy(hfill).cuda()
        ctx.emit_header_blocks(hdr, dev_sets, lens, hdst,
                               out_off=torch.from_numpy(dst_off.astype(np.int64)).cuda())
        torch.cuda.synchronize()
        want = fill.copy()
        a = arena.cpu().numpy()
        oracle.emit_batch(hdr, host_sets, a, off.cpu().numpy(), ln, want, dst_off, nthreads=16)
        hwant = hfill.copy()
        oracle.emit_batch(hdr, host_sets, None, None, ln, hwant, dst_off, copy=False, nthreads=16)
        key = f"emit/{prof.name}/H{H}/sets{len(host_sets)}"
        res[key] = {"packet_byte_mismatches": int((dst.cpu().numpy() != want).sum()),
                    "header_block_byte_mismatches": int((hdst.cpu().numpy() != hwant).sum())}
        print(key, res[key], flush=True)
        del arena, off, lens, dst, hdst
        torch.cuda.empty_cache()
    csum_cases(ctx, min(n, args.csum_frames), args.seed, res)
    modify_csum_cases(ctx, min(n, args.csum_frames), args.seed, res)
    finish(n, args.seed, t0, res)


if __name__ == "__main__":
    main()
