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

`--usage-only` compiles ingot_amd/csrc/emit.hip with
-Rpass-analysis=kernel-resource-usage and writes the kernels' figures (no GPU
needed); `--usage FILE` attaches such a file to the result.

    python tools/emit_csum_probe.py [--frames N] [--reps 5] [--rounds 5]
        [--against head] [--usage FILE] [--out profiles/r12_emit_csum_probe.json]
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
    """k_emit's instantiations -> registers, scratch, occupancy (from hipcc)."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
           f"-I{ROOT / 'include'}", "-Rpass-analysis=kernel-resource-usage", "-c",
           str(ROOT / "ingot_amd" / "csrc" / "emit.hip"), "-o", "/dev/null"]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    names = {"ILb1ELb1EE": "k_emit<copy, sums>", "ILb1ELb0EE": "k_emit<copy>",
             "ILb0ELb0EE": "k_emit<headers>"}
    for line in err.splitlines():
        m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = next((v for k, v in names.items() if k in val), val)
            out[cur] = {}
        elif cur and key in ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy"):
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
    args = ap.parse_args()
    if args.usage_only:
        out = resource_usage()
    elif args.child:
        print(json.dumps(child_main(args) if args.child == "main"
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

        out = {"what": __doc__.split("\n\n")[0], **run("main")}
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
