#!/usr/bin/env python3
"""Measurement tool: the rewrite with the fused checksum update against the
plain rewrite and against rewrite + checksum fill.

Two layouts, HIP events, the median of interleaved rounds, arenas rotated so
that no launch reads what the one before it left in the 256 MiB Infinity
Cache:

  c2m    8,388,608 64-B V4UDP64 slots, UdpParser, UDP destination - 1;
  c3nat  8,388,608 MIXED frames addressed by offset, GenericUlp, a NAT edit
         list (IPv4 destination, UDP / TCP destination port, hop limit).

Calls timed on each:

  a  ingot_gpu_parse_modify;
  b  ingot_gpu_parse_modify_csum, L3 | L4;
  c  ingot_gpu_parse_modify, then ingot_gpu_checksum_fill, L3 | L4.

Every variant runs in a child process of its own (one library per process;
this process never touches the GPU), the variants alternated: "default" is
the in-tree library, any other name tools/variants/<name>/libingot_gpu.so
(tools/build_tree_variant.sh, e.g. the parent commit).  A library without the
fused call, and any variant named with the suffix @plain, is timed on (a)
alone, in a process that launches nothing else: `default default@plain
parentA parentB` gives (a), (b), (c) at head, and the plain rewrite at head
against the parent and the parent against itself (the spread), all three
under the same conditions.

    python tools/modify_csum_probe.py default default@plain parentA parentB \
        [--rounds 3] [--out F]

With --read, the rewrite over chunked packets instead (one child process, the
in-tree library, all rows interleaved in it): the c3nat frames cut in place at
payload_off (header-split: two chunks per packet) with the same edit list,

  a  ingot_gpu_parse_read on those tables (the floor: the new call parses the
     same way before it edits);
  b  ingot_gpu_parse_modify_csum, L3 | L4, on the same frames uncut;
  c  ingot_gpu_parse_read_modify on the tables;
  d  ingot_gpu_parse_read_modify_csum, L3 | L4, on the tables;

each row's min - max of the rounds and its ratios to (a) and (b).

    python tools/modify_csum_probe.py --read [--inner-rounds 5] [--out F]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def child(spec: str, n: int, reps: int, rounds: int, copies: int) -> dict:
    import ingot_amd._lib as L

    name, _, mode = spec.partition("@")
    if name != "default":
        L.LIB_PATH = ROOT / "tools" / "variants" / name / "libingot_gpu.so"
    import torch  # before the library: one HIP runtime per process (ingot_amd/_lib.py)

    fused = hasattr(ctypes.CDLL(str(L.LIB_PATH)), "ingot_gpu_parse_modify_csum")
    if not fused:
        L.SIGNATURES.pop("ingot_gpu_parse_modify_csum", None)
    fused = fused and mode != "plain"
    import ingot_amd
    from ingot_amd import CSUM_L3, CSUM_L4, Chain, EditOp, Field, GenProfile

    ctx = ingot_amd.Context(0)
    s = torch.cuda.current_stream()
    what = CSUM_L3 | CSUM_L4
    # edits that change their bytes on every launch (a SET would move no sum
    # from the second launch on)
    layouts = (
        ("c2m", GenProfile.V4UDP64, Chain.UdpParser, 64,
         [(2, Field.UDP_DESTINATION, EditOp.SUB, 1)]),
        ("c3nat", GenProfile.MIXED, Chain.GenericUlp, None,
         [(1, Field.V4_DESTINATION, EditOp.XOR, 0x00FF00FF),
          (2, Field.UDP_DESTINATION, EditOp.SUB, 1), (2, Field.TCP_DESTINATION, EditOp.SUB, 1),
          (1, Field.V4_HOP_LIMIT, EditOp.SUB, 1)]))
    runs = {}
    for lname, prof, chain, stride, edits in layouts:
        sets = []
        for c in range(copies):
            arena, off, lens = ingot_amd.gen_frames(prof, n, seed=ingot_amd.GEN_SEED + c,
                                                    stride=stride)
            recs = (ctx.parse_strided(arena, stride, n, chain) if stride
                    else ctx.parse(arena, off, lens, chain))
            ctx.checksum_fill(arena, off, lens, recs, stride=stride or 0, n=n)  # valid sums
            sets.append((arena, off, lens, recs))
        turn = {"k": 0}

        def pick(sets=sets, turn=turn):
            turn["k"] += 1
            return sets[turn["k"] % len(sets)]

        def a(pick=pick, chain=chain, edits=edits, st=stride or 0):
            ar, o, ln, _ = pick()
            ctx.parse_modify(ar, o, ln, chain, edits, stride=st, n=n)

        def b(pick=pick, chain=chain, edits=edits, st=stride or 0):
            ar, o, ln, _ = pick()
            ctx.parse_modify(ar, o, ln, chain, edits, stride=st, n=n, csum=what)

        def c(pick=pick, chain=chain, edits=edits, st=stride or 0):
            ar, o, ln, rc = pick()
            ctx.parse_modify(ar, o, ln, chain, edits, stride=st, n=n)
            ctx.checksum_fill(ar, o, ln, rc, what, stride=st, n=n)

        runs[f"{lname}_a"] = a
        if fused:
            runs[f"{lname}_b"], runs[f"{lname}_c"] = b, c
    for f in runs.values():
        for _ in range(copies):
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
    return {"variant": spec, "fused": fused, "us": res}


def child_read(n: int, reps: int, rounds: int, copies: int) -> dict:
    import torch  # before the library: one HIP runtime per process (ingot_amd/_lib.py)

    import ingot_amd
    from ingot_amd import CSUM_L3, CSUM_L4, Chain, EditOp, Field, GenProfile

    ctx = ingot_amd.Context(0)
    s = torch.cuda.current_stream()
    what = CSUM_L3 | CSUM_L4
    chain = Chain.GenericUlp
    edits = [(1, Field.V4_DESTINATION, EditOp.XOR, 0x00FF00FF),
             (2, Field.UDP_DESTINATION, EditOp.SUB, 1), (2, Field.TCP_DESTINATION, EditOp.SUB, 1),
             (1, Field.V4_HOP_LIMIT, EditOp.SUB, 1)]
    sets = []
    for c in range(copies):
        arena, off, lens = ingot_amd.gen_frames(GenProfile.MIXED, n, seed=ingot_amd.GEN_SEED + c)
        recs = ctx.parse(arena, off, lens, chain)
        ctx.checksum_fill(arena, off, lens, recs, n=n)  # valid sums
        L = lens.to(torch.int32) & 0xFFFF
        pay = recs[:, 12].to(torch.int32) | (recs[:, 13].to(torch.int32) << 8)
        pay = torch.where(recs[:, 0] == 0, torch.minimum(pay, L), L)
        so = torch.stack((off, off + pay.to(torch.int64)), dim=1).reshape(-1).contiguous()
        sl = torch.stack((pay, L - pay), dim=1).reshape(-1).to(torch.int16).contiguous()
        ps = torch.arange(n + 1, dtype=torch.int32, device="cuda") * 2
        out = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
        chunk = torch.empty(n, dtype=torch.int16, device="cuda")
        sets.append((arena, off, lens, so, sl, ps, out, chunk))
    turn = {"k": 0}

    def pick():
        turn["k"] += 1
        return sets[turn["k"] % len(sets)]

    def a():
        ar, _, _, so, sl, ps, out, ch = pick()
        ctx.parse_read(ar, so, sl, ps, chain, out=out, chunk=ch)

    def b():
        ar, o, ln, *_ = pick()
        ctx.parse_modify(ar, o, ln, chain, edits, n=n, csum=what)

    def c():
        ar, _, _, so, sl, ps, out, ch = pick()
        ctx.parse_read_modify(ar, so, sl, ps, chain, edits, out=out, chunk=ch)

    def d():
        ar, _, _, so, sl, ps, out, ch = pick()
        ctx.parse_read_modify(ar, so, sl, ps, chain, edits, csum=what, out=out, chunk=ch)

    runs = {"a_parse_read": a, "b_parse_modify_csum_uncut": b, "c_parse_read_modify": c,
            "d_parse_read_modify_csum": d}
    for f in runs.values():
        for _ in range(copies):
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
    rows = {k: {"min_us": min(v), "max_us": max(v), "median_us": round(med[k], 1), "rounds": v,
                "over_a": round(med[k] / med["a_parse_read"], 3),
                "over_b": round(med[k] / med["b_parse_modify_csum_uncut"], 3)}
            for k, v in res.items()}
    return {"what": "the rewrite over chunked packets: C3 frames cut at payload_off, NAT edits",
            "frames": n, "chunks": 2 * n, "reps": reps, "copies": copies,
            "unit": "us per call, interleaved rounds in one process", "runs": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="*", default=["default"])
    ap.add_argument("--frames", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner-rounds", type=int, default=5, help="interleaved rounds per child")
    ap.add_argument("--rounds", type=int, default=3, help="children per variant, alternated")
    ap.add_argument("--copies", type=int, default=2, help="arenas rotated per layout")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--read", action="store_true",
                    help="the rewrite over chunked packets (parse_read_modify) instead")
    ap.add_argument("--child-read", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_read:
        print(json.dumps(child_read(args.frames, args.reps, args.inner_rounds, args.copies)),
              flush=True)
        return
    if args.read:
        p = subprocess.run(
            [sys.executable, __file__, "--child-read", "--frames", str(args.frames), "--reps",
             str(args.reps), "--inner-rounds", str(args.inner_rounds), "--copies",
             str(args.copies)], capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise SystemExit(f"child failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
        out = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(out), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
        return
    if args.child is not None:
        print(json.dumps(child(args.child, args.frames, args.reps, args.inner_rounds,
                               args.copies)), flush=True)
        return
    got = {}
    for r in range(args.rounds):
        for k, v in enumerate(args.variants):
            p = subprocess.run(
                [sys.executable, __file__, "--child", v, "--frames", str(args.frames), "--reps",
                 str(args.reps), "--inner-rounds", str(args.inner_rounds), "--copies",
                 str(args.copies)], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"child {v} failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
            d = json.loads(p.stdout.strip().splitlines()[-1])
            slot = got.setdefault(f"{k}:{v}", {"variant": v, "fused": d["fused"], "us": {}})
            for key, us in d["us"].items():
                slot["us"].setdefault(key, []).append(us)
            print(f"round {r} {v}: " + " ".join(f"{key}={statistics.median(us):.1f}"
                                                for key, us in d["us"].items()), flush=True)
    out = {"what": __doc__.split("\n\n")[0], "frames": args.frames, "reps": args.reps,
           "unit": "us per call, per child the rounds in order", "variants": []}
    for slot in got.values():
        row = {"variant": slot["variant"], "fused": slot["fused"], "runs": {}}
        for key, per_child in slot["us"].items():
            flat = [x for ch in per_child for x in ch]
            row["runs"][key] = {"median_us": round(statistics.median(flat), 1),
                                "child_medians": [round(statistics.median(ch), 1)
                                                  for ch in per_child],
                                "rounds": per_child}
        for lay in ("c2m", "c3nat"):
            if f"{lay}_b" in slot["us"]:
                bs = [x for ch in slot["us"][f"{lay}_b"] for x in ch]
                cs = [x for ch in slot["us"][f"{lay}_c"] for x in ch]
                row[f"{lay}_b_below_c_in_every_round"] = all(x < y for x, y in zip(bs, cs))
                row[f"{lay}_b_over_a"] = round(row["runs"][f"{lay}_b"]["median_us"] /
                                               row["runs"][f"{lay}_a"]["median_us"], 3)
                row[f"{lay}_b_over_c"] = round(row["runs"][f"{lay}_b"]["median_us"] /
                                               row["runs"][f"{lay}_c"]["median_us"], 3)
        out["variants"].append(row)
    print(json.dumps(out), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
