#!/usr/bin/env python3
"""Measurement tool: emit with checksums against the plain emit and against the three-call path.

On 8,388,608 generator frames (MIXED, 64-1500 B) encapsulated as OPTE's
outbound path does (outer Ethernet / IPv6 / UDP / Geneve + one option = 74 B,
lengths, a per-packet UDP source port and VNI), times with HIP events (median
of interleaved rounds; destination arenas rotated so that no launch finds the
last one's lines in the 256 MiB Infinity Cache), in one process:

  a  emit        ingot_gpu_emit_packets;
  b  emit_csum   ingot_gpu_emit_packets_csum with the outer UDP sum;
  c  three_call  ingot_gpu_emit_packets + a UDP_PARSER parse of the emitted
                 arena + ingot_gpu_checksum_fill(L4);

checks once that b and c leave identical bytes, and reports the ratios b/a and
b/c with the rounds' spread ((max - min) / median of each run).  Then, each
in a child process of its own and interleaved, the plain emit (a) of this
library and of another build (`--against NAME`: tools/variants/NAME, e.g. the
parent commit from tools/build_tree_variant.sh), so that a change of the
plain kernel would show.

`--read` measures ingot_gpu_emit_packets_read instead: the
same frames cut in place at payload_off into two chunks (the whole frame and
an empty chunk where the record is not Ok), rows

  a  emit               as above;
  b  emit_csum          as above;
  c  two_launch         what the chunked caller had before: emit_packets(hdr,
                        chunk 0), then emit_packets(no header, chunk 1) behind
                        it (the two length fields as per-packet U16 values,
                        since LENGTH would count chunk 0 alone);
  d  read               ingot_gpu_emit_packets_read, the same tables, no sums;
  e  two_launch_fill    c + the UDP_PARSER parse + ingot_gpu_checksum_fill(L4);
  f  read_csum          ingot_gpu_emit_packets_read with the outer UDP sum;
  d1 / f1               d and f with every packet one chunk (what the tables
                        cost against a and b);

checks once that c and d, and e and f, leave identical bytes, and compares the
rounds' ranges: the new row's maximum against the old row's minimum.

`--rows` measures ingot_gpu_emit_packets_rows instead: the
same frames and stack, the outer IPv6 destination and Ethernet destination of
every packet taken from a table, rows

  a  emit_csum          as b above (the UDP sum);
  b  rows_no_table      the new call with the same narrow sets and no table
                        (what the new prologue costs by itself);
  c  rows_by_packet     b + the two wide sets BY_PACKET (n-row tables);
  d  rows_by_row        the same BY_ROW from a 65,536-row table indexed by
                        ingot_gpu_flow_hist's bins (uncounted packets take row
                        0, so that every row of this table emits every packet);
  dg rows_by_row_guard  d with the bins as they are: uncounted packets are not
                        emitted;
  e  emit_modify_rows   today's route to d's bytes: emit_packets_csum, then
                        ingot_gpu_parse_modify_rows (GENEVE_OVER_V6, the two
                        wide fields BY_ROW, OUTER_L4), which parses by itself;
  e3 emit_parse_modify_rows  e with the separate parse of the result between;

checks once that a and b, and c, d and e, leave identical bytes.

`--read-rows` measures ingot_gpu_emit_packets_read_rows instead (DESIGN.md
4.18): `--read`'s two-chunk tables and `--rows`' endpoint table, rows

  a  read_csum          ingot_gpu_emit_packets_read with the UDP sum;
  b  rr_no_table        the new call with the same narrow sets and no table
                        (the same walk: what the new prologue costs by itself);
  c  rr_by_packet       b + the IPv6 destination and Ethernet destination
                        BY_PACKET (n-row tables);
  d  rr_by_row          the same BY_ROW from a 65,536-row table indexed by the
                        flow bins (uncounted packets take row 0);
  dg rr_by_row_guard    d with the bins as they are: uncounted packets are not
                        emitted and their chunks not walked;
  e  read_modify_rows   today's route to d's bytes: emit_packets_read with the
                        UDP sum, then ingot_gpu_parse_modify_rows over the
                        output (GENEVE_OVER_V6, the two wide fields BY_ROW,
                        OUTER_L4), which parses by itself;

checks once that a and b, and d and e (and c), leave identical bytes and
d_taken, and says whether b's median lies inside a's min-max of rounds and d
below e's fastest round.

`--usage-only` compiles ingot_amd/csrc/emit.hip, emit_read.hip and csum.hip with
-Rpass-analysis=kernel-resource-usage and writes the kernels' figures (no GPU
needed); `--usage FILE` attaches such a file to the result.

    python tools/emit_csum_probe.py [--frames N] [--reps 5] [--rounds 5] [--read]
        [--rows] [--read-rows] [--against head] [--usage FILE] [--out profiles/r12_emit_csum_probe.json]
"""
from __future__ import annotations

import argparse
import json
import re
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def resource_usage() -> dict:
    """k_emit's and k_emit_read's instantiations and the two checksum kernels
    -> registers, scratch, occupancy, static LDS (from hipcc)."""
    err = ""
    for src in ("emit.hip", "emit_read.hip", "csum.hip"):
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
               f"-I{ROOT / 'include'}", "-Rpass-analysis=kernel-resource-usage", "-c",
               str(ROOT / "ingot_amd" / "csrc" / src), "-o", "/dev/null"]
        err += subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    names = {"k_emitILb1ELb1ELb1EE": "k_emit<copy, sums, rows>",
             "k_emitILb1ELb0ELb1EE": "k_emit<copy, rows>",
             "k_emitILb1ELb1ELb0EE": "k_emit<copy, sums>", "k_emitILb1ELb0ELb0EE": "k_emit<copy>",
             "k_emitILb0ELb0ELb0EE": "k_emit<headers>",
             "k_emit_readILb1ELb1EE": "k_emit_read<sums, rows>",
             "k_emit_readILb0ELb1EE": "k_emit_read<rows>",
             "k_emit_readILb1ELb0EE": "k_emit_read<sums>", "k_emit_readILb0ELb0EE": "k_emit_read",
             "6k_csumE": "k_csum", "11k_csum_readE": "k_csum_read"}
    for line in err.splitlines():
        m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = next((v for k, v in names.items() if k in val), val)
            out[cur] = {}
        elif cur and key in ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy",
                             "SGPRs Spill", "VGPRs Spill", "LDS Size"):
            out[cur][key] = int(val)
    return out


def setup(n: int, copies: int):
    import torch

    import ingot_amd
    from ingot_amd import EmitSource, EmitSum, Field, GenProfile
    from ingot_amd import emit as E

    ctx = ingot_amd.Context(0)
    arena, off, lens = ingot_amd.gen_frames(GenProfile.MIXED, n)
    hdr = (E.ethernet(bytes(6), bytes(6), 0x86DD)
           + E.ipv6(bytes.fromhex("fd000000f70101000000000000000002"),
                    bytes.fromhex("fd000000f70101000000000000000001"), 17, hop_limit=64)
           + E.udp(0, 6081) + E.geneve(0, options=E.geneve_opt(0x0129, 0)))
    H = len(hdr)
    g = torch.Generator(device="cuda").manual_seed(1)
    ports = torch.randint(0, 1 << 15, (n,), dtype=torch.int16, device="cuda", generator=g)
    vnis = torch.randint(0, 1 << 24, (n,), dtype=torch.int32, device="cuda", generator=g)
    sets = [(14, Field.V6_PAYLOAD_LEN, EmitSource.LENGTH, -40),
            (54, Field.UDP_LENGTH, EmitSource.LENGTH, 0),
            (54, Field.UDP_SOURCE, EmitSource.U16, 0, ports),
            (62, Field.GENEVE_VNI, EmitSource.U32, 0, vnis)]
    ln = lens.to(torch.int64)
    dst_off = torch.cumsum(ln + H, 0) - (ln + H)
    total = int((ln + H).sum().item())
    tl = (ln + H).to(torch.int32).to(torch.uint16)
    dsts = [torch.empty(total + 64, dtype=torch.uint8, device="cuda") for _ in range(copies)]
    turn = {"k": 0}

    def pick():
        turn["k"] += 1
        return dsts[turn["k"] % copies]

    d = dict(ctx=ctx, arena=arena, off=off, lens=lens, hdr=hdr, sets=sets, dst_off=dst_off,
             total=total, payload=int(ln.sum().item()), tl=tl, pick=pick, dsts=dsts, H=H,
             sums=[(EmitSum.UDP, 54, 14)])
    return d


def timed(runs: dict, reps: int, rounds: int) -> dict:
    import torch

    s = torch.cuda.current_stream()
    for f in runs.values():
        f()
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in runs}
    for _ in range(rounds):
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                f()
            e1.record(s)
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    out = {}
    for k, v in res.items():
        med = statistics.median(v)
        out[k] = {"us": round(med, 1), "rounds": [round(x, 1) for x in v],
                  "spread": round((max(v) - min(v)) / med, 4)}
    return out


def child_plain(lib: str, args) -> dict:
    """The plain emit alone, of the in-tree library or of a variant."""
    if lib != "default":
        from ingot_amd import _lib as L

        L.LIB_PATH = ROOT / "tools" / "variants" / lib / "libingot_gpu.so"
        # an older build lacks the newer entry points: bind only what it exports
        image = L.LIB_PATH.read_bytes()
        for name in [k for k in L.SIGNATURES if k.encode() + b"\0" not in image]:
            del L.SIGNATURES[name]
    d = setup(args.frames, args.copies)
    ctx = d["ctx"]
    r = timed({"emit": lambda: ctx.emit_packets(d["hdr"], d["sets"], d["arena"], d["off"],
                                                d["lens"], d["pick"](), d["dst_off"])},
              args.reps, args.rounds)
    return {"lib": lib, **r["emit"]}


def child_main(args) -> dict:
    import torch

    from ingot_amd import CSUM_L4, Chain

    d = setup(args.frames, args.copies)
    ctx, n = d["ctx"], args.frames
    recs = torch.empty((n, 16), dtype=torch.uint8, device="cuda")

    def emit(dst=None):
        ctx.emit_packets(d["hdr"], d["sets"], d["arena"], d["off"], d["lens"],
                         d["pick"]() if dst is None else dst, d["dst_off"])

    def emit_csum(dst=None):
        ctx.emit_packets(d["hdr"], d["sets"], d["arena"], d["off"], d["lens"],
                         d["pick"]() if dst is None else dst, d["dst_off"], sums=d["sums"])

    def three_call(dst=None):
        dst = d["pick"]() if dst is None else dst
        ctx.emit_packets(d["hdr"], d["sets"], d["arena"], d["off"], d["lens"], dst, d["dst_off"])
        ctx.parse(dst, d["dst_off"], d["tl"], Chain.UdpParser, out=recs)
        ctx.checksum_fill(dst, d["dst_off"], d["tl"], recs, CSUM_L4)

    # b and c leave identical bytes (and both differ from a)
    x, y = d["dsts"][0], d["dsts"][1 % len(d["dsts"])]
    x.fill_(0xA5)
    y.fill_(0xA5)
    emit_csum(x)
    three_call(y)
    torch.cuda.synchronize()
    same = bool(torch.equal(x, y)) if x is not y else None
    emit(y)
    torch.cuda.synchronize()
    moved = int((x != y).sum().item())
    runs = timed({"emit": emit, "emit_csum": emit_csum, "three_call": three_call}, args.reps,
                 args.rounds)
    a, b, c = (runs[k]["us"] for k in ("emit", "emit_csum", "three_call"))
    spread = max(r["spread"] for r in runs.values())
    return {"frames": n, "hdr_len": d["H"], "payload_bytes": d["payload"],
            "emitted_bytes": d["total"], "copies": args.copies, "reps": args.reps,
            "b_equals_c_bytes": same, "bytes_b_differs_from_a": moved, "runs": runs,
            "b_over_a": round(b / a, 4), "b_over_c": round(b / c, 4),
            "rounds_spread_max": spread,
            "b_beats_c_by_more_than_spread": bool(b < c * (1 - spread))}


def child_read(args) -> dict:
    import torch

    from ingot_amd import CSUM_L4, Chain, EmitSource, Field

    d = setup(args.frames, args.copies)
    ctx, n, H = d["ctx"], args.frames, d["H"]
    arena, off, lens, hdr, dst_off = d["arena"], d["off"], d["lens"], d["hdr"], d["dst_off"]
    recs = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    # the frames cut in place at payload_off (tools/csum_probe.py --read's tables)
    rc = ctx.parse(arena, off, lens, Chain.GenericUlp)
    L = lens.to(torch.int32) & 0xFFFF
    pay = rc[:, 12].to(torch.int32) | (rc[:, 13].to(torch.int32) << 8)
    pay = torch.where(rc[:, 0] == 0, torch.minimum(pay, L), L)
    o0, o1 = off.contiguous(), (off + pay.to(torch.int64)).contiguous()
    l0, l1 = pay.to(torch.int16).contiguous(), (L - pay).to(torch.int16).contiguous()
    so = torch.stack((o0, o1), dim=1).reshape(-1).contiguous()
    sl = torch.stack((l0, l1), dim=1).reshape(-1).contiguous()
    ps1 = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    ps2 = (ps1 * 2).contiguous()
    dst_off1 = (dst_off + H + pay.to(torch.int64)).contiguous()
    # the two-launch path cannot use LENGTH (it would count chunk 0 alone)
    sets_c = [(14, Field.V6_PAYLOAD_LEN, EmitSource.U16, 0, (L + (H - 54)).to(torch.int16)),
              (54, Field.UDP_LENGTH, EmitSource.U16, 0, (L + (H - 54)).to(torch.int16)),
              d["sets"][2], d["sets"][3]]

    def pick(dst):
        return d["pick"]() if dst is None else dst

    def emit(dst=None):
        ctx.emit_packets(hdr, d["sets"], arena, off, lens, pick(dst), dst_off)

    def emit_csum(dst=None):
        ctx.emit_packets(hdr, d["sets"], arena, off, lens, pick(dst), dst_off, sums=d["sums"])

    def two_launch(dst=None):
        dst = pick(dst)
        ctx.emit_packets(hdr, sets_c, arena, o0, l0, dst, dst_off)
        ctx.emit_packets(b"", [], arena, o1, l1, dst, dst_off1)
        return dst

    def two_launch_fill(dst=None):
        dst = two_launch(dst)
        ctx.parse(dst, dst_off, d["tl"], Chain.UdpParser, out=recs)
        ctx.checksum_fill(dst, dst_off, d["tl"], recs, CSUM_L4)

    def read(dst=None):
        ctx.emit_packets_read(hdr, d["sets"], arena, so, sl, ps2, pick(dst), dst_off)

    def read_csum(dst=None):
        ctx.emit_packets_read(hdr, d["sets"], arena, so, sl, ps2, pick(dst), dst_off,
                              sums=d["sums"])

    def read_1chunk(dst=None):
        ctx.emit_packets_read(hdr, d["sets"], arena, off, lens, ps1, pick(dst), dst_off)

    def read_csum_1chunk(dst=None):
        ctx.emit_packets_read(hdr, d["sets"], arena, off, lens, ps1, pick(dst), dst_off,
                              sums=d["sums"])

    x, y = d["dsts"][0], d["dsts"][1 % len(d["dsts"])]
    same = {}
    for name, old, new in (("c_equals_d", two_launch, read), ("e_equals_f", two_launch_fill, read_csum),
                           ("a_equals_d1", emit, read_1chunk), ("b_equals_f1", emit_csum, read_csum_1chunk)):
        x.fill_(0xA5)
        y.fill_(0xA5)
        old(x)
        new(y)
        torch.cuda.synchronize()
        same[name] = bool(torch.equal(x, y)) if x is not y else None
    runs = timed({"a_emit": emit, "b_emit_csum": emit_csum, "c_two_launch": two_launch,
                  "d_read": read, "e_two_launch_fill": two_launch_fill, "f_read_csum": read_csum,
                  "d1_read_1chunk": read_1chunk, "f1_read_csum_1chunk": read_csum_1chunk},
                 args.reps, args.rounds)
    for r in runs.values():
        r["min"], r["max"] = min(r["rounds"]), max(r["rounds"])
    return {"frames": n, "hdr_len": H, "payload_bytes": d["payload"], "emitted_bytes": d["total"],
            "chunks": {"two": 2 * n, "one": n}, "empty_second_chunks": int((l1 == 0).sum().item()),
            "copies": args.copies, "reps": args.reps, "same_bytes": same, "runs": runs,
            "d_max_le_c_min": bool(runs["d_read"]["max"] <= runs["c_two_launch"]["min"]),
            "f_max_le_e_min": bool(runs["f_read_csum"]["max"] <= runs["e_two_launch_fill"]["min"]),
            "d1_over_a": round(runs["d1_read_1chunk"]["us"] / runs["a_emit"]["us"], 4),
            "f1_over_b": round(runs["f1_read_csum_1chunk"]["us"] / runs["b_emit_csum"]["us"], 4)}


def child_rows(args) -> dict:
    import torch

    from ingot_amd import CSUM_OUTER_L4, Chain, EditOp, EmitSource, WideField

    d = setup(args.frames, args.copies)
    ctx, n, H = d["ctx"], args.frames, d["H"]
    arena, off, lens, hdr, dst_off = d["arena"], d["off"], d["lens"], d["hdr"], d["dst_off"]
    sets, sums, bins = d["sets"], d["sums"], 1 << 16
    g = torch.Generator(device="cuda").manual_seed(2)
    # one (bins, 32) table: underlay IPv6 at 0, next-hop MAC at 16
    table = torch.randint(0, 256, (bins, 32), dtype=torch.uint8, device="cuda", generator=g)
    v6_row, mac_row = table[:, 0:16], table[:, 16:22]
    flow = ctx.flow_hist(arena, off, lens, Chain.GenericUlp, bins=bins)
    counted = flow >= 0
    rows_all = torch.where(counted, flow, torch.zeros_like(flow)).contiguous()
    v6_pkt = v6_row[rows_all.to(torch.int64)].contiguous()
    mac_pkt = mac_row[rows_all.to(torch.int64)].contiguous()
    V6D, MACD, B = WideField.V6_DESTINATION, WideField.ETH_DESTINATION, EmitSource.BYTES
    by_packet = sets + [(14, V6D, B, 0, v6_pkt), (0, MACD, B, 0, mac_pkt)]
    by_row = sets + [(14, V6D, B, 0, ("row", v6_row)), (0, MACD, B, 0, ("row", mac_row))]
    edits = [(1, V6D, EditOp.SET, ("row", v6_row)), (0, MACD, EditOp.SET, ("row", mac_row))]
    recs = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    TUN = Chain.GeneveOverV6Tunnel

    def pick(dst):
        return d["pick"]() if dst is None else dst

    def emit_csum(dst=None):
        ctx.emit_packets(hdr, sets, arena, off, lens, pick(dst), dst_off, sums=sums)

    def rows_no_table(dst=None):
        ctx.emit_packets_rows(hdr, sets, arena, off, lens, pick(dst), dst_off, sums=sums)

    def rows_by_packet(dst=None):
        ctx.emit_packets_rows(hdr, by_packet, arena, off, lens, pick(dst), dst_off, sums=sums)

    def rows_by_row(dst=None):
        ctx.emit_packets_rows(hdr, by_row, arena, off, lens, pick(dst), dst_off, rows=rows_all,
                              n_rows=bins, sums=sums)

    def rows_by_row_guard(dst=None):
        ctx.emit_packets_rows(hdr, by_row, arena, off, lens, pick(dst), dst_off, rows=flow,
                              n_rows=bins, sums=sums)

    def emit_modify_rows(dst=None, parse=False):
        dst = pick(dst)
        ctx.emit_packets(hdr, sets, arena, off, lens, dst, dst_off, sums=sums)
        if parse:
            ctx.parse(dst, dst_off, d["tl"], TUN, out=recs)
        ctx.parse_modify_rows(dst, dst_off, d["tl"], TUN, edits, rows=rows_all, n_rows=bins,
                              csum=CSUM_OUTER_L4)

    def emit_parse_modify_rows(dst=None):
        emit_modify_rows(dst, parse=True)

    x, y = d["dsts"][0], d["dsts"][1 % len(d["dsts"])]
    same = {}
    for name, old, new in (("a_equals_b", emit_csum, rows_no_table),
                           ("c_equals_d", rows_by_packet, rows_by_row),
                           ("e_equals_d", emit_modify_rows, rows_by_row)):
        x.fill_(0xA5)
        y.fill_(0xA5)
        old(x)
        new(y)
        torch.cuda.synchronize()
        same[name] = bool(torch.equal(x, y)) if x is not y else None
        if same[name] is False:
            same[name + "_bytes_differ"] = int((x != y).sum().item())
    runs = timed({"a_emit_csum": emit_csum, "b_rows_no_table": rows_no_table,
                  "c_rows_by_packet": rows_by_packet, "d_rows_by_row": rows_by_row,
                  "dg_rows_by_row_guard": rows_by_row_guard, "e_emit_modify_rows": emit_modify_rows,
                  "e3_emit_parse_modify_rows": emit_parse_modify_rows}, args.reps, args.rounds)
    for r in runs.values():
        r["min"], r["max"] = min(r["rounds"]), max(r["rounds"])
    us = {k: r["us"] for k, r in runs.items()}
    return {"frames": n, "hdr_len": H, "payload_bytes": d["payload"], "emitted_bytes": d["total"],
            "table_rows": bins, "table_pitch": 32, "counted_packets": int(counted.sum().item()),
            "copies": args.copies, "reps": args.reps, "same_bytes": same, "runs": runs,
            "rounds_spread_max": max(r["spread"] for r in runs.values()),
            "b_over_a": round(us["b_rows_no_table"] / us["a_emit_csum"], 4),
            "c_over_b": round(us["c_rows_by_packet"] / us["b_rows_no_table"], 4),
            "d_over_c": round(us["d_rows_by_row"] / us["c_rows_by_packet"], 4),
            "d_over_e": round(us["d_rows_by_row"] / us["e_emit_modify_rows"], 4),
            "d_max_le_e_min": bool(runs["d_rows_by_row"]["max"] <= runs["e_emit_modify_rows"]["min"])}


def child_read_rows(args) -> dict:
    import torch

    from ingot_amd import CSUM_OUTER_L4, Chain, EditOp, EmitSource, WideField

    d = setup(args.frames, args.copies)
    ctx, n, H = d["ctx"], args.frames, d["H"]
    arena, off, lens, hdr, dst_off = d["arena"], d["off"], d["lens"], d["hdr"], d["dst_off"]
    sets, sums, bins = d["sets"], d["sums"], 1 << 16
    # --read's tables: the frames cut in place at payload_off
    rc = ctx.parse(arena, off, lens, Chain.GenericUlp)
    L = lens.to(torch.int32) & 0xFFFF
    pay = rc[:, 12].to(torch.int32) | (rc[:, 13].to(torch.int32) << 8)
    pay = torch.where(rc[:, 0] == 0, torch.minimum(pay, L), L)
    so = torch.stack((off, off + pay.to(torch.int64)), dim=1).reshape(-1).contiguous()
    sl = torch.stack((pay.to(torch.int16), (L - pay).to(torch.int16)), dim=1).reshape(-1).contiguous()
    ps = (torch.arange(n + 1, dtype=torch.int32, device="cuda") * 2).contiguous()
    del rc
    # --rows' table: one (bins, 32) table, underlay IPv6 at 0, next-hop MAC at 16
    g = torch.Generator(device="cuda").manual_seed(2)
    table = torch.randint(0, 256, (bins, 32), dtype=torch.uint8, device="cuda", generator=g)
    v6_row, mac_row = table[:, 0:16], table[:, 16:22]
    flow = ctx.flow_hist(arena, off, lens, Chain.GenericUlp, bins=bins)
    counted = flow >= 0
    rows_all = torch.where(counted, flow, torch.zeros_like(flow)).contiguous()
    v6_pkt = v6_row[rows_all.to(torch.int64)].contiguous()
    mac_pkt = mac_row[rows_all.to(torch.int64)].contiguous()
    V6D, MACD, B = WideField.V6_DESTINATION, WideField.ETH_DESTINATION, EmitSource.BYTES
    by_packet = sets + [(14, V6D, B, 0, v6_pkt), (0, MACD, B, 0, mac_pkt)]
    by_row = sets + [(14, V6D, B, 0, ("row", v6_row)), (0, MACD, B, 0, ("row", mac_row))]
    edits = [(1, V6D, EditOp.SET, ("row", v6_row)), (0, MACD, EditOp.SET, ("row", mac_row))]
    TUN = Chain.GeneveOverV6Tunnel
    taken = torch.empty(n, dtype=torch.int16, device="cuda")

    def pick(dst):
        return d["pick"]() if dst is None else dst

    def read_csum(dst=None, tk=None):
        ctx.emit_packets_read(hdr, sets, arena, so, sl, ps, pick(dst), dst_off, taken=tk,
                              sums=sums)

    def rr(the_sets, dst, tk, **kw):
        ctx.emit_packets_read_rows(hdr, the_sets, arena, so, sl, ps, pick(dst), dst_off,
                                   taken=tk, sums=sums, **kw)

    def rr_no_table(dst=None, tk=None):
        rr(sets, dst, tk)

    def rr_by_packet(dst=None, tk=None):
        rr(by_packet, dst, tk)

    def rr_by_row(dst=None, tk=None):
        rr(by_row, dst, tk, rows=rows_all, n_rows=bins)

    def rr_by_row_guard(dst=None, tk=None):
        rr(by_row, dst, tk, rows=flow, n_rows=bins)

    def read_modify_rows(dst=None, tk=None):
        dst = pick(dst)
        ctx.emit_packets_read(hdr, sets, arena, so, sl, ps, dst, dst_off, taken=tk, sums=sums)
        ctx.parse_modify_rows(dst, dst_off, d["tl"], TUN, edits, rows=rows_all, n_rows=bins,
                              csum=CSUM_OUTER_L4)

    x, y = d["dsts"][0], d["dsts"][1 % len(d["dsts"])]
    tx = torch.empty_like(taken)
    same = {}
    for name, old, new in (("a_equals_b", read_csum, rr_no_table),
                           ("c_equals_d", rr_by_packet, rr_by_row),
                           ("e_equals_d", read_modify_rows, rr_by_row)):
        for t in (x, y):
            t.fill_(0xA5)
        tx.fill_(0x5A5A)
        taken.fill_(0x5A5A)
        old(x, tx)
        new(y, taken)
        torch.cuda.synchronize()
        same[name] = bool(torch.equal(x, y) and torch.equal(tx, taken)) if x is not y else None
        if same[name] is False:
            same[name + "_bytes_differ"] = int((x != y).sum().item())
    runs = timed({"a_read_csum": read_csum, "b_rr_no_table": rr_no_table,
                  "c_rr_by_packet": rr_by_packet, "d_rr_by_row": rr_by_row,
                  "dg_rr_by_row_guard": rr_by_row_guard, "e_read_modify_rows": read_modify_rows},
                 args.reps, args.rounds)
    for r in runs.values():
        r["min"], r["max"] = min(r["rounds"]), max(r["rounds"])
    us = {k: r["us"] for k, r in runs.items()}
    a = runs["a_read_csum"]
    return {"frames": n, "hdr_len": H, "payload_bytes": d["payload"], "emitted_bytes": d["total"],
            "chunks": 2 * n, "table_rows": bins, "table_pitch": 32,
            "counted_packets": int(counted.sum().item()),
            "copies": args.copies, "reps": args.reps, "same_bytes": same, "runs": runs,
            "rounds_spread_max": max(r["spread"] for r in runs.values()),
            "b_over_a": round(us["b_rr_no_table"] / us["a_read_csum"], 4),
            "b_median_inside_a_rounds": bool(a["min"] <= us["b_rr_no_table"] <= a["max"]),
            "c_over_b": round(us["c_rr_by_packet"] / us["b_rr_no_table"], 4),
            "d_over_c": round(us["d_rr_by_row"] / us["c_rr_by_packet"], 4),
            "d_over_e": round(us["d_rr_by_row"] / us["e_read_modify_rows"], 4),
            "d_below_e_min": bool(us["d_rr_by_row"] < runs["e_read_modify_rows"]["min"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--copies", type=int, default=2, help="destination arenas rotated")
    ap.add_argument("--against", default=None, help="tools/variants/<name>: A/B of the plain emit")
    ap.add_argument("--ab-rounds", type=int, default=2, help="child processes per library")
    ap.add_argument("--usage", default=None)
    ap.add_argument("--usage-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--read", action="store_true", help="the chunked emit's rows (DESIGN 4.12)")
    ap.add_argument("--rows", action="store_true", help="emit_packets_rows' rows (DESIGN 4.15)")
    ap.add_argument("--read-rows", action="store_true",
                    help="emit_packets_read_rows' rows (DESIGN 4.18)")
    args = ap.parse_args()
    if args.usage_only:
        out = resource_usage()
    elif args.child:
        print(json.dumps(child_main(args) if args.child == "main"
                         else child_read(args) if args.child == "read"
                         else child_rows(args) if args.child == "rows"
                         else child_read_rows(args) if args.child == "read_rows"
                         else child_plain(args.child, args)), flush=True)
        return
    else:
        def run(which):
            p = subprocess.run([sys.executable, __file__, "--child", which, "--frames",
                                str(args.frames), "--reps", str(args.reps), "--rounds",
                                str(args.rounds), "--copies", str(args.copies)],
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                print(p.stdout, p.stderr, flush=True)
                sys.exit(p.returncode or 1)
            return json.loads(p.stdout.strip().splitlines()[-1])

        out = {"what": __doc__.split("\n\n")[0], **run("read_rows" if args.read_rows else "read" if args.read else "rows" if args.rows
                     else "main")}
        print(json.dumps(out), flush=True)
        if args.against:
            rows = []
            for _ in range(args.ab_rounds):
                for lib in ("default", args.against):
                    rows.append(run(lib))
                    print(json.dumps(rows[-1]), flush=True)
            best = {lib: min(r["us"] for r in rows if r["lib"] == lib)
                    for lib in ("default", args.against)}
            out["plain_emit_ab"] = {
                "rows": rows, "this_us": best["default"], "other": args.against,
                "other_us": best[args.against],
                "this_over_other": round(best["default"] / best[args.against], 4),
                "spread_max": max(r["spread"] for r in rows)}
        if args.usage:
            out["resource_usage"] = json.loads(Path(args.usage).read_text())
    print(json.dumps(out), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
