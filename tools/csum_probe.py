#!/usr/bin/env python3
"""Measurement tool: the batched checksum kernel against the gather copy.

On the C3 frames (MIXED, 64-1500 B, packed, GenericUlp records) and on C2's
64-B slots (V4UDP64, no length array, UdpParser records), times with HIP events
(median of interleaved rounds, arenas rotated so that no launch reads what the
one before it left in the 256 MiB Infinity Cache):

  verify   ingot_gpu_checksum_verify, L3 | L4;
  fill     ingot_gpu_checksum_fill, L3 | L4, with rows;
  gather   ingot_gpu_emit_packets with hdr_len 0 over the same frames (the
           existing gather copy: reads about the same bytes and writes them all
           back, where the checksum writes 8 B per packet).

and reports algorithmic GB/s.  Checksum: the L4 segments that are summed + the
L3 headers read (20 / 40 B) + the descriptors (10 B per packed frame, none for
slots) + the 16-B record, 8 B written per packet.  Gather: the frames read and
written + 18 B of descriptors per packet.

With --read, the chunked calls (k_csum_read) on the C3 frames join the same
interleaved rounds, beside c3_verify as the yardstick:

  c3_read_1chunk_verify   ingot_gpu_checksum_verify_read, every packet one
                          chunk (the like-for-like case);
  c3_read_split_verify    header-split: two chunks cut at payload_off (the
                          whole frame and an empty chunk where the record is
                          not Ok), in place in the same arena;
  c3_read_split_fill      ingot_gpu_checksum_fill_read over the same tables.

Their algorithmic bytes are the checksum's with 10 B per chunk and 4 B per
packet of tables in place of the 10 B of packed descriptors.

`--lib NAME` measures tools/variants/NAME/libingot_gpu.so (another build, e.g.
the parent commit from tools/build_tree_variant.sh) instead of the in-tree one.

    python tools/csum_probe.py [--frames N] [--reps 5] [--rounds 5] [--read] [--lib NAME]
        [--out F]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--copies", type=int, default=2, help="arenas rotated per layout")
    ap.add_argument("--read", action="store_true",
                    help="add the chunked calls (checksum_verify_read / _fill_read) on c3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="tools/variants/<name>/libingot_gpu.so instead")
    args = ap.parse_args()
    if args.lib:
        from ingot_amd import _lib as L

        L.LIB_PATH = ROOT / "tools" / "variants" / args.lib / "libingot_gpu.so"

    import torch

    import ingot_amd
    from ingot_amd import CSUM_DTYPE, Chain, GenProfile

    ctx = ingot_amd.Context(0)
    n = args.frames
    s = torch.cuda.current_stream()
    runs, algo, meta = {}, {}, {}
    for name, prof, chain, stride in (("c3", GenProfile.MIXED, Chain.GenericUlp, None),
                                      ("c2", GenProfile.V4UDP64, Chain.UdpParser, 64)):
        sets = []
        for c in range(args.copies):
            arena, off, lens = ingot_amd.gen_frames(prof, n, seed=ingot_amd.GEN_SEED + c,
                                                    stride=stride)
            if stride:
                recs = ctx.parse_strided(arena, stride, n, chain)
                g_off = torch.arange(n, dtype=torch.int64, device="cuda") * stride
                g_len = torch.full((n,), stride, dtype=torch.int32, device="cuda").to(torch.uint16)
                frame_bytes = n * stride
            else:
                recs = ctx.parse(arena, off, lens, chain)
                g_off, g_len = off, lens
                frame_bytes = int(lens.to(torch.int64).sum().item())
            rows = torch.empty((n, 8), dtype=torch.uint8, device="cuda")
            dst = torch.empty(frame_bytes + 64, dtype=torch.uint8, device="cuda")
            d_off = torch.cumsum(g_len.to(torch.int64), 0) - g_len.to(torch.int64)
            sets.append((arena, off, lens, recs, rows, g_off, g_len, dst, d_off))
        arena, off, lens, recs, rows, *_ = sets[0]
        ctx.checksum_verify(arena, off, lens, recs, stride=stride or 0, n=n, out=rows)
        torch.cuda.synchronize()
        r = rows.cpu().numpy().view(CSUM_DTYPE).reshape(-1)
        rec = ingot_amd.records_to_numpy(recs)
        ok = rec["status"] == 0
        hdr = (int((ok & (rec["l3_kind"] == 1)).sum()) * 20 +
               int((ok & (rec["l3_kind"] == 2)).sum()) * 40)
        seg = int(r["l4_len"].astype("int64").sum())
        desc = 0 if stride else 10
        algo[f"{name}_verify"] = algo[f"{name}_fill"] = seg + hdr + n * (desc + 16 + 8)
        algo[f"{name}_gather"] = 2 * frame_bytes + 18 * n
        meta[name] = {"frames": n, "frame_bytes": frame_bytes, "segment_bytes": seg,
                      "l3_header_bytes": hdr, "copies": args.copies,
                      "l4_states": [int((r["l4_state"] == k).sum()) for k in range(6)]}
        turn = {"k": 0}

        def pick(sets=sets, turn=turn):
            turn["k"] += 1
            return sets[turn["k"] % len(sets)]

        def verify(pick=pick, st=stride or 0):
            a, o, ln, rc, rw, *_ = pick()
            ctx.checksum_verify(a, o, ln, rc, stride=st, n=n, out=rw)

        def fill(pick=pick, st=stride or 0):
            a, o, ln, rc, rw, *_ = pick()
            ctx.checksum_fill(a, o, ln, rc, stride=st, n=n, out=rw)

        def gather(pick=pick):
            a, _, _, _, _, go, gl, d, do = pick()
            ctx.emit_packets(b"", [], a, go, gl, d, do)

        runs[f"{name}_verify"], runs[f"{name}_gather"], runs[f"{name}_fill"] = verify, gather, fill
        if args.read and name == "c3":
            one, two = [], []
            for a, o, ln, rc, rw, *_ in sets:
                ps1 = torch.arange(n + 1, dtype=torch.int32, device="cuda")
                r1, _ = ctx.parse_read(a, o, ln, ps1, chain)
                one.append((a, o, ln, ps1, r1, rw))
                L = ln.to(torch.int32) & 0xFFFF
                pay = rc[:, 12].to(torch.int32) | (rc[:, 13].to(torch.int32) << 8)
                pay = torch.where(rc[:, 0] == 0, torch.minimum(pay, L), L)
                so = torch.stack((o, o + pay.to(torch.int64)), dim=1).reshape(-1).contiguous()
                sl = torch.stack((pay, L - pay), dim=1).reshape(-1).to(torch.int16).contiguous()
                ps2 = ps1 * 2
                r2, _ = ctx.parse_read(a, so, sl, ps2, chain)
                two.append((a, so, sl, ps2, r2, rw))
            ctx.checksum_verify_read(*two[0][:5], out=two[0][5])
            torch.cuda.synchronize()
            r2 = two[0][5].cpu().numpy().view(CSUM_DTYPE).reshape(-1)
            meta[name]["split_rows_unlike_contiguous"] = int((r2.view("uint64") !=
                                                              r.view("uint64")).sum())
            meta[name]["chunks"] = {"one": n, "split": 2 * n}
            base = seg + hdr + n * (16 + 8 + 4)
            algo["c3_read_1chunk_verify"] = base + 10 * n
            algo["c3_read_split_verify"] = algo["c3_read_split_fill"] = base + 20 * n
            rturn = {"k": 0}

            def rpick(which, rturn=rturn):
                rturn["k"] += 1
                return which[rturn["k"] % len(which)]

            def read1(rpick=rpick, one=one):
                a, so, sl, ps, rc, rw = rpick(one)
                ctx.checksum_verify_read(a, so, sl, ps, rc, out=rw)

            def read2(rpick=rpick, two=two):
                a, so, sl, ps, rc, rw = rpick(two)
                ctx.checksum_verify_read(a, so, sl, ps, rc, out=rw)

            def fill2(rpick=rpick, two=two):
                a, so, sl, ps, rc, rw = rpick(two)
                ctx.checksum_fill_read(a, so, sl, ps, rc, out=rw)

            runs["c3_read_1chunk_verify"], runs["c3_read_split_verify"] = read1, read2
            runs["c3_read_split_fill"] = fill2
    for f in runs.values():  # warm up every shape (fill also makes the sums valid: same work)
        for _ in range(args.copies):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(args.reps):
                f()
            e1.record(s)
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    out = {"what": __doc__.split("\n\n")[0], "lib": args.lib or "in-tree", "layouts": meta,
           "reps": args.reps, "runs": {}}
    for k, v in res.items():
        us = statistics.median(v)
        out["runs"][k] = {"us": round(us, 1), "rounds": [round(x, 1) for x in v],
                          "algorithmic_bytes": algo[k], "GB_s": round(algo[k] / us / 1e3, 1),
                          "frac_of_8TBs": round(algo[k] / us / 1e3 / 8000, 3),
                          "Mpkt_s": round(n / us, 1)}
    print(json.dumps(out), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
