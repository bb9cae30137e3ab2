#!/usr/bin/env python3
"""Measurement tool: the rewrite with per-packet operands
(ingot_gpu_parse_modify_rows) against the existing rewrite with one constant
per batch (ingot_gpu_parse_modify_csum) on the same frames.

One child process, the in-tree library, every row interleaved in it; HIP
events, the rounds in order, arenas rotated so that no launch reads what the
one before it left in the 256 MiB Infinity Cache.  Operands alternate between
two values / two tables from launch to launch, so every launch changes its
bytes and moves its sums.  All rows update L3 | L4.

On 8,388,608 MIXED frames addressed by offset (the C3 profile), GenericUlp:

  a  ingot_gpu_parse_modify_csum, V4_SOURCE and UDP_SOURCE SET to one value
     each (the baseline: the existing call);
  b  ingot_gpu_parse_modify_rows, the same fields from dense per-packet u32 /
     u16 arrays (BY_PACKET): + 6 B read per packet;
  c  ingot_gpu_parse_modify_rows, the same fields BY_ROW from a 65,536-row
     table of 8-B rows indexed by ingot_gpu_flow_hist's d_flow: + 4 B read per
     packet (the row index) and a 6-B gather from a 512 KiB table.

On 8,388,608 VLAN_V6EH frames (the C4 profile), VlanUlp:

  d  ingot_gpu_parse_modify_csum, V6_FLOW_LABEL and V6_HOP_LIMIT SET (the
     baseline: the existing call on these frames);
  e  ingot_gpu_parse_modify_rows, NAT66: V6_SOURCE and V6_DESTINATION from
     per-packet 16-B rows (BY_PACKET): + 32 B read per packet, and 32 B
     instead of 4 B rewritten in each IPv6 header.

Ratios are to the existing call on the same frames (b / a, c / a, e / d),
never to the new one.

    python tools/modify_rows_probe.py [--frames N] [--reps 5] [--inner-rounds 5] [--out F]
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BINS = 1 << 16


def child(n: int, reps: int, rounds: int, copies: int) -> dict:
    import torch  # before the library: one HIP runtime per process (ingot_amd/_lib.py)

    import ingot_amd
    from ingot_amd import CSUM_L3, CSUM_L4, Chain, EditOp, Field, GenProfile, WideField

    ctx = ingot_amd.Context(0)
    s = torch.cuda.current_stream()
    what = CSUM_L3 | CSUM_L4
    SET = EditOp.SET
    g = torch.Generator(device="cuda").manual_seed(1)

    def rnd(shape, dtype):
        hi = {torch.int32: 1 << 31, torch.int16: 1 << 15, torch.uint8: 256}[dtype]
        return torch.randint(0, hi, shape, dtype=dtype, device="cuda", generator=g)

    def frames(prof, chain):
        sets = []
        for c in range(copies):
            arena, off, lens = ingot_amd.gen_frames(prof, n, seed=ingot_amd.GEN_SEED + c)
            recs = ctx.parse(arena, off, lens, chain)
            ctx.checksum_fill(arena, off, lens, recs, n=n)  # valid sums
            flow = ctx.flow_hist(arena, off, lens, chain, bins=BINS)
            sets.append((arena, off, lens, flow))
        return sets

    c3, c4 = frames(GenProfile.MIXED, Chain.GenericUlp), frames(GenProfile.VLAN_V6EH, Chain.VlanUlp)
    # two of every operand, alternated from launch to launch
    addr, port = [rnd((n,), torch.int32) for _ in range(2)], [rnd((n,), torch.int16)
                                                             for _ in range(2)]
    table = [rnd((BINS, 8), torch.uint8) for _ in range(2)]
    v6s, v6d = [rnd((n, 16), torch.uint8) for _ in range(2)], [rnd((n, 16), torch.uint8)
                                                               for _ in range(2)]
    turn = {"k": 0}

    def pick(sets):
        turn["k"] += 1
        return sets[turn["k"] % len(sets)], (turn["k"] // len(sets)) & 1

    def a():
        (ar, o, ln, _), p = pick(c3)
        ctx.parse_modify(ar, o, ln, Chain.GenericUlp,
                         [(1, Field.V4_SOURCE, SET, 0x0A000001 + p),
                          (2, Field.UDP_SOURCE, SET, 4000 + p)], n=n, csum=what)

    def b():
        (ar, o, ln, _), p = pick(c3)
        ctx.parse_modify_rows(ar, o, ln, Chain.GenericUlp,
                              [(1, Field.V4_SOURCE, SET, addr[p]),
                               (2, Field.UDP_SOURCE, SET, port[p])], n=n, csum=what)

    def c():
        (ar, o, ln, flow), p = pick(c3)
        t = table[p]
        ctx.parse_modify_rows(ar, o, ln, Chain.GenericUlp,
                              [(1, Field.V4_SOURCE, SET, ("row", t[:, 0:4].view(torch.int32))),
                               (2, Field.UDP_SOURCE, SET, ("row", t[:, 4:6].view(torch.int16)))],
                              rows=flow, n_rows=BINS, n=n, csum=what)

    def d():
        (ar, o, ln, _), p = pick(c4)
        ctx.parse_modify(ar, o, ln, Chain.VlanUlp,
                         [(2, Field.V6_FLOW_LABEL, SET, 0x12345 + p),
                          (2, Field.V6_HOP_LIMIT, SET, 63 + p)], n=n, csum=what)

    def e():
        (ar, o, ln, _), p = pick(c4)
        ctx.parse_modify_rows(ar, o, ln, Chain.VlanUlp,
                              [(2, WideField.V6_SOURCE, SET, v6s[p]),
                               (2, WideField.V6_DESTINATION, SET, v6d[p])], n=n, csum=what)

    runs = {"a_c3_parse_modify_csum_uniform": a, "b_c3_rows_by_packet_u32_u16": b,
            "c_c3_rows_by_row_flow_table": c, "d_c4_parse_modify_csum_uniform": d,
            "e_c4_rows_nat66_bytes": e}
    for f in runs.values():
        for _ in range(2 * copies):
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
            res[k].append(round(e0.elapsed_time(e1) * 1e3 / reps, 1))
    med = {k: statistics.median(v) for k, v in res.items()}
    base = {"a": "a_c3_parse_modify_csum_uniform", "b": "a_c3_parse_modify_csum_uniform",
            "c": "a_c3_parse_modify_csum_uniform", "d": "d_c4_parse_modify_csum_uniform",
            "e": "d_c4_parse_modify_csum_uniform"}
    extra = {"a": 0, "b": 6, "c": 4, "d": 0, "e": 32}
    rows = {k: {"min_us": min(v), "max_us": max(v), "median_us": round(med[k], 1), "rounds": v,
                "compared_with": base[k[0]], "over_baseline": round(med[k] / med[base[k[0]]], 3),
                "extra_streamed_bytes_read_per_packet": extra[k[0]]}
            for k, v in res.items()}
    rows["c_c3_rows_by_row_flow_table"]["gathered_bytes_per_packet"] = 6
    rows["c_c3_rows_by_row_flow_table"]["table_bytes"] = BINS * 8
    return {"what": __doc__.split("\n\n")[0], "frames": n, "reps": reps, "copies": copies,
            "sums": "L3 | L4", "unit": "us per call, interleaved rounds in one process",
            "runs": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner-rounds", type=int, default=5, help="interleaved rounds")
    ap.add_argument("--copies", type=int, default=2, help="arenas rotated per profile")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.frames, args.reps, args.inner_rounds, args.copies)),
              flush=True)
        return
    p = subprocess.run([sys.executable, __file__, "--child", "--frames", str(args.frames),
                        "--reps", str(args.reps), "--inner-rounds", str(args.inner_rounds),
                        "--copies", str(args.copies)], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
