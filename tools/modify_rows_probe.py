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

--read: the same comparison for the rewrite over chunked packets
(ingot_gpu_parse_read_modify_rows), every frame cut at payload_off into two
chunks:

  a  ingot_gpu_parse_read_modify_csum with constants (the existing call);
  b  the same fields from dense arrays, BY_PACKET;
  c  BY_ROW from the 65,536-row table;
  d  NAT66 on cut C4 frames;
  f  NAT66 on the same frames uncut through ingot_gpu_parse_modify_rows (what d
     is held against);
  e  (--lib NAME) row d with the library of tools/variants/NAME, built by
     SRC=read.hip tools/build_variants.sh NAME:-DINGOT_READ_ROWS_FAST_SET=0:
     children of the two libraries in turn, rows a and d in each.

    python tools/modify_rows_probe.py --read [--lib nofast] [--rounds 2] [--out F]
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


def child_read(n: int, reps: int, rounds: int, copies: int, lib, only_ad: bool) -> dict:
    """--read: the rewrite over chunked packets with per-packet operands
    (ingot_gpu_parse_read_modify_rows) on frames cut at payload_off (two chunks
    per packet), against the chunked rewrite with one constant per batch."""
    if lib:
        import ingot_amd._lib as L

        L.LIB_PATH = ROOT / "tools" / "variants" / lib / "libingot_gpu.so"
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
            L_ = lens.to(torch.int32) & 0xFFFF
            pay = recs[:, 12].to(torch.int32) | (recs[:, 13].to(torch.int32) << 8)
            pay = torch.where(recs[:, 0] == 0, torch.minimum(pay, L_), L_)
            so = torch.stack((off, off + pay.to(torch.int64)), dim=1).reshape(-1).contiguous()
            sl = torch.stack((pay, L_ - pay), dim=1).reshape(-1).to(torch.int16).contiguous()
            ps = torch.arange(n + 1, dtype=torch.int32, device="cuda") * 2
            sets.append((arena, off, lens, flow, so, sl, ps))
        return sets

    c3, c4 = frames(GenProfile.MIXED, Chain.GenericUlp), frames(GenProfile.VLAN_V6EH, Chain.VlanUlp)
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
        (ar, _, _, _, so, sl, ps), p = pick(c3)
        ctx.parse_read_modify(ar, so, sl, ps, Chain.GenericUlp,
                              [(1, Field.V4_SOURCE, SET, 0x0A000001 + p),
                               (2, Field.UDP_SOURCE, SET, 4000 + p)], csum=what)

    def b():
        (ar, _, _, _, so, sl, ps), p = pick(c3)
        ctx.parse_read_modify_rows(ar, so, sl, ps, Chain.GenericUlp,
                                   [(1, Field.V4_SOURCE, SET, addr[p]),
                                    (2, Field.UDP_SOURCE, SET, port[p])], csum=what)

    def c():
        (ar, _, _, flow, so, sl, ps), p = pick(c3)
        t = table[p]
        ctx.parse_read_modify_rows(
            ar, so, sl, ps, Chain.GenericUlp,
            [(1, Field.V4_SOURCE, SET, ("row", t[:, 0:4].view(torch.int32))),
             (2, Field.UDP_SOURCE, SET, ("row", t[:, 4:6].view(torch.int16)))],
            rows=flow, n_rows=BINS, csum=what)

    def d():
        (ar, _, _, _, so, sl, ps), p = pick(c4)
        ctx.parse_read_modify_rows(ar, so, sl, ps, Chain.VlanUlp,
                                   [(2, WideField.V6_SOURCE, SET, v6s[p]),
                                    (2, WideField.V6_DESTINATION, SET, v6d[p])], csum=what)

    def f():
        (ar, o, ln, *_), p = pick(c4)
        ctx.parse_modify_rows(ar, o, ln, Chain.VlanUlp,
                              [(2, WideField.V6_SOURCE, SET, v6s[p]),
                               (2, WideField.V6_DESTINATION, SET, v6d[p])], n=n, csum=what)

    runs = {"a_c3_read_modify_csum_uniform": a, "b_c3_read_rows_by_packet_u32_u16": b,
            "c_c3_read_rows_by_row_flow_table": c, "d_c4_read_rows_nat66_bytes": d,
            "f_c4_contiguous_rows_nat66_bytes": f}
    if only_ad:
        runs = {k: v for k, v in runs.items() if k[0] in "ad"}
    for fn in runs.values():
        for _ in range(2 * copies):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            res[k].append(round(e0.elapsed_time(e1) * 1e3 / reps, 1))
    rows = {k: {"min_us": min(v), "max_us": max(v), "median_us": round(statistics.median(v), 1),
                "rounds": v} for k, v in res.items()}
    return {"lib": lib or "in-tree", "runs": rows}


def main_read(args):
    """One child with the in-tree library and every row; with --lib NAME, then
    children of NAME and of the in-tree library in turn, rows a and d only: row
    e is NAME's d (the fast store path compiled out), beside the in-tree d of
    the same alternation."""
    def run(lib, only_ad):
        cmd = [sys.executable, __file__, "--child-read", "--frames", str(args.frames), "--reps",
               str(args.reps), "--inner-rounds", str(args.inner_rounds), "--copies",
               str(args.copies)]
        cmd += (["--lib", lib] if lib else []) + (["--only-ad"] if only_ad else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"child failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
        return json.loads(p.stdout.strip().splitlines()[-1])

    first = run(None, False)
    runs = first["runs"]
    med = {k: v["median_us"] for k, v in runs.items()}
    base = med["a_c3_read_modify_csum_uniform"]
    for k in ("b_c3_read_rows_by_packet_u32_u16", "c_c3_read_rows_by_row_flow_table"):
        runs[k]["over_a"] = round(med[k] / base, 3)
    runs["d_c4_read_rows_nat66_bytes"]["over_contiguous_nat66"] = round(
        med["d_c4_read_rows_nat66_bytes"] / med["f_c4_contiguous_rows_nat66_bytes"], 3)
    out = {"what": " ".join(child_read.__doc__.split("\n\n")[0].replace("--read: ", "").split()),
           "frames": args.frames, "chunks": 2 * args.frames, "reps": args.reps,
           "copies": args.copies, "sums": "L3 | L4",
           "unit": "us per call, interleaved rounds in one process", "runs": runs}
    if args.lib:
        ab = []
        for r in range(args.rounds):
            for lib in (args.lib, None):
                x = run(lib, True)
                ab.append({"lib": x["lib"], "round": r,
                           **{k: v["rounds"] for k, v in x["runs"].items()}})
        d_of = lambda lib: [u for x in ab if x["lib"] == lib  # noqa: E731
                            for u in x["d_c4_read_rows_nat66_bytes"]]
        e, d = d_of(args.lib), d_of("in-tree")
        out["e_c4_read_rows_nat66_fast_path_compiled_out"] = {
            "lib": args.lib, "children": ab,
            "e_median_us": round(statistics.median(e), 1), "e_min_us": min(e), "e_max_us": max(e),
            "d_median_us": round(statistics.median(d), 1), "d_min_us": min(d), "d_max_us": max(d),
            "e_over_d": round(statistics.median(e) / statistics.median(d), 3)}
    print(json.dumps(out), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--read", action="store_true",
                    help="ingot_gpu_parse_read_modify_rows over cut frames instead")
    ap.add_argument("--lib", default=None,
                    help="--read: tools/variants/<name>/libingot_gpu.so for row e")
    ap.add_argument("--rounds", type=int, default=2, help="--read --lib: children per library")
    ap.add_argument("--child-read", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only-ad", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--frames", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner-rounds", type=int, default=5, help="interleaved rounds")
    ap.add_argument("--copies", type=int, default=2, help="arenas rotated per profile")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_read:
        print(json.dumps(child_read(args.frames, args.reps, args.inner_rounds, args.copies,
                                    args.lib, args.only_ad)), flush=True)
        return
    if args.read:
        return main_read(args)
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
