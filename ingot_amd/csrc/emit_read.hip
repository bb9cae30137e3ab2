// emit_read.hip — batched Emit over chunked packets (ingot_gpu_emit_packets_read):
// pull-up, encapsulation and the outer checksums in one launch
// (ingot_gpu_emit_packets_read_rows: the ROWS instantiations, described at
// k_emit_read).
//
// The source of packet i is the chunk list of ingot_gpu_parse_read, cut at
// 65,535 logical bytes, of which the bytes [f, f + t) are the payload (d_from /
// d_take, clamped).  The destination side is k_emit's (emit.hip), through the
// steps both kernels call in emit_common.h: start_sums per packet (and
// build_region's body, see step 2), then per aligned 16-B destination block
// of the group's flat run merge_header, udp_share and store_chunk, and
// finish_parked behind the group's barrier.  Everything about the sum is in destination coordinates.
//
// What differs is where a block's payload bytes come from.  A *piece* is the
// part of one non-empty chunk that lies inside the payload; in payload
// coordinates (byte x of the payload is logical byte f + x) piece p is
// [start_p, end_p) and its bytes sit at address sbase_p + x.  The prologue
// lane of a packet walks the chunk lengths once (L, t, the chunk that holds f)
// and leaves the first PIECES pieces in LDS; a block that needs a later piece
// walks the chunk table in global memory from where the LDS table stops, with
// a cursor that only moves forward (a block's bytes are taken in order).  A
// block whose payload bytes lie in one piece is k_emit's load: the aligned
// 16-B source block and its neighbour (the next lane's when that lane loaded
// exactly that block, a second load otherwise), funnel-shifted by the piece's
// source-vs-destination misalignment.  A block that holds a chunk boundary
// does the same per piece and keeps each piece's bytes under a byte mask.
// Source reads stay inside the aligned 16-B blocks that hold a byte of a
// piece; an empty chunk's offset is never turned into an address.
#include <type_traits>

#include "emit_common.h"

namespace ingot_gpu {
namespace {

constexpr uint32_t W = 16;          // waves per group (k_emit<copy>'s shape)
constexpr uint32_t PW = 4;          // 64-packet subgroups, one prologue wave each
constexpr uint32_t NP = PW * WAVE;  // packets per group
constexpr uint32_t BLOCK = W * WAVE;
constexpr uint32_t NPOW = 256;      // search span
static_assert(NP == NPOW, "the prefix search spans the group");
// 64-block steps whose loads fly together.  2 keeps both instantiations at or
// under 64 VGPRs (two 1,024-thread groups per CU, as k_emit); 4 takes 81 / 91
// and leaves room for one.
#ifndef INGOT_EMIT_READ_UNROLL
#define INGOT_EMIT_READ_UNROLL 2
#endif
constexpr uint32_t UNROLL = INGOT_EMIT_READ_UNROLL;
constexpr uint32_t PIECES = 4;                       // pieces per packet kept in LDS

// Per-group LDS.  start[k][j], k < PIECES: the payload offset at which piece k
// of packet j starts (0xffffffff: no such piece); start[PIECES][j]: where the
// tabled pieces end (t when they are all of them).
struct ReadDesc {
    uint64_t dst[NP];            // destination address of packet j
    uint64_t sbase[PIECES][NP];  // address of payload byte 0 as piece k would have it
    uint32_t start[PIECES + 1][NP];
    uint32_t pfx[NP];            // inclusive prefix of block counts
    uint32_t len[NP];            // t: payload bytes
    uint32_t dmis[NP];           // destination address & 15
    uint32_t cur[NP];            // first chunk index after the tabled pieces
    uint32_t s1[NP];             // the packet's chunk bound
    uint32_t sub[4];             // blocks of each 64-packet subgroup
    uint32_t _pad[WAVE - 4];
};

struct Piece {
    uint64_t sbase;
    uint32_t start, end;
    bool ok;
};

// The piece that holds payload byte x < t of packet q.  (s, xs) is the lane's
// cursor into the chunk table past the LDS entries: chunk s starts at payload
// offset xs.
__device__ __forceinline__ Piece piece_at(const ReadDesc& wd, const EmitReadArgs& ar, uint32_t q,
                                          uint32_t x, uint32_t t, uint32_t& s, uint32_t& xs) {
    Piece p;
    if (x < wd.start[PIECES][q]) {
        uint32_t k = 0;
#pragma unroll
        for (uint32_t m = 1; m < PIECES; ++m) k += wd.start[m][q] <= x ? 1u : 0u;
        p.start = wd.start[k][q];
        p.end = min(wd.start[k + 1][q], t);
        p.sbase = wd.sbase[k][q];
        p.ok = true;
        return p;
    }
    const uint32_t s1 = wd.s1[q];
    uint32_t ln = 0;
    while (s < s1) {
        ln = gbl(ar.seg_len)[s];
        if (xs + ln > x) break;
        xs += ln;
        ++s;
    }
    p.ok = s < s1;
    p.start = xs;
    p.end = min(xs + ln, t);
    p.sbase = p.ok ? (uint64_t)(uintptr_t)ar.e.src + gbl(ar.seg_off)[s] - xs : 0u;
    return p;
}

// The 16 bytes at X (any alignment) of piece p, zero outside the aligned
// blocks that hold a byte of the piece.
__device__ __forceinline__ u32x4 piece_block(const Piece& p, uint64_t X) {
    const uint64_t B = X & ~(uint64_t)15, S0 = p.sbase + p.start, S1 = p.sbase + p.end;
    const uint32_t sh = (uint32_t)X & 15u;
    u32x4 lo = u32x4{0u, 0u, 0u, 0u}, hi = u32x4{0u, 0u, 0u, 0u};
    if (B + 16 > S0 && B < S1) lo = *(const __attribute__((address_space(1))) u32x4*)B;
    if (sh != 0 && B + 16 < S1 && B + 32 > S0)
        hi = *(const __attribute__((address_space(1))) u32x4*)(B + 16);
    return funnel(lo, hi, sh);
}

// The EmitReadArgs of either argument block.
__device__ __forceinline__ const EmitReadArgs& read_args_of(const EmitReadArgs& a) { return a; }
__device__ __forceinline__ const EmitReadArgs& read_args_of(const EmitReadRowsArgs& a) { return a.r; }

// ROWS (ingot_gpu_emit_packets_read_rows; its argument block is
// EmitReadRowsArgs): the prologue also loads the packet's row index, folds the
// row guard into `live` before the chunk-length walk and takes the setters'
// operands from the pieces of EmitReadRowsArgs, as k_emit's ROWS instantiations
// do.  A guarded packet has no chunks to walk, no pieces, no payload and no
// blocks: the block search never lands on it, d_taken gets 0 and step 5
// returns on it.  Everything from step 3 on is the same code.
template <bool SUMS, bool ROWS = false>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_num_sgpr(96))) void k_emit_read(
    std::conditional_t<ROWS, EmitReadRowsArgs, EmitReadArgs> args) {
    // by value (the compiler reads every field from the kernel arguments all
    // the same): bound as a reference it moved blocks of the instantiations
    // without ROWS out of line, 26 more instructions in each
    const EmitReadArgs ar = read_args_of(args);
    const EmitArgs& a = ar.e;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    u32x4* tmpl = reinterpret_cast<u32x4*>(smem);
    load_template(tmpl, a, BLOCK);
    const uint32_t H = a.hdr_len;
    const uint32_t RS = region_bytes(H);
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t wg = threadIdx.x / WAVE;  // this wave's turn in the group
    ReadDesc& wd = *reinterpret_cast<ReadDesc*>(smem + TB * 16);
    uint8_t* regions = smem + TB * 16 + sizeof(ReadDesc);
    // SUMS: after the regions, the parked blocks, then the accumulators
    u32x4* park = reinterpret_cast<u32x4*>(smem + TB * 16 + sizeof(ReadDesc) + NP * RS);
    uint32_t* acc = reinterpret_cast<uint32_t*>(park + 2u * NP);
    // ROWS: the pieces, after everything else
    EmitPiece* pieces = reinterpret_cast<EmitPiece*>(SUMS ? (void*)(acc + NP) : (void*)park);
    if constexpr (ROWS) load_pieces(pieces, args, BLOCK);
    const bool udp = SUMS && a.sums.udp;
    const uint32_t fpos = (uint32_t)a.sums.udp_at + 6u;  // the UDP checksum field in hdr
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * NP;
    if (wg < PW) {
        // 1. wave wg, lane j: packet base + 64 wg + j.  Its chunk bounds, from /
        //    take and destination; one walk of its chunk lengths gives L (cut
        //    at 65,535), t, and the first PIECES pieces from the chunk that
        //    holds logical byte `from` on
        const uint32_t j = wg * WAVE + lane;
        const uint64_t i = base + j;
        const bool in_batch = i < a.n;
        bool live = in_batch;
        uint32_t r = 0;  // ROWS: the packet's row index, loaded with its descriptors
        if constexpr (ROWS) {
            if (live && args.row) r = gbl(args.row)[i];
        }
        uint32_t s0 = 0, s1 = 0;
        if (live) {
            s0 = gbl(ar.pkt_seg)[i];
            s1 = gbl(ar.pkt_seg)[i + 1];
            s1 = s1 < s0 ? s0 : s1;  // reversed bounds: no chunks
        }
        uint32_t fr = (live && ar.from) ? (uint32_t)gbl(ar.from)[i] : 0u;
        const uint32_t tk = (live && ar.take) ? (uint32_t)gbl(ar.take)[i] : 0xffffu;
        uint64_t doff = live ? gbl(a.dst_off)[i] : 0u;
        if constexpr (ROWS) {
            // the row guard, before the walk: no chunk bounds, so no entry of
            // seg_len / seg_off is read; the descriptors loaded above are
            // dropped unused
            if (args.row && r >= args.n_rows) {
                live = false;
                s0 = s1 = 0u;
                fr = 0u;
                doff = 0u;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k <= PIECES; ++k) wd.start[k][j] = 0xffffffffu;
        uint32_t g = 0, cnt = 0, cur = s1, tabled_end = 0;
        for (uint32_t s = s0; s < s1 && g < 65535u; ++s) {
            const uint32_t ln = min((uint32_t)gbl(ar.seg_len)[s], 65535u - g);
            if (ln != 0 && g + ln > fr && cnt < PIECES) {
                wd.start[cnt][j] = g > fr ? g - fr : 0u;
                wd.sbase[cnt][j] = (uint64_t)(uintptr_t)a.src + gbl(ar.seg_off)[s] + fr - g;
                if (++cnt == PIECES) {
                    cur = s + 1;
                    tabled_end = g + ln - fr;
                }
            }
            g += ln;
        }
        const uint32_t f = min(fr, g);
        const uint32_t L = min(tk, g - f);  // t: the payload bytes of this packet
        wd.start[PIECES][j] = cnt == PIECES ? min(tabled_end, L) : L;
        // a guarded packet's walk was empty: L = 0 is what its d_taken gets
        if (in_batch && ar.taken) ar.taken[i] = (uint16_t)L;
        uint32_t v[INGOT_MAX_EMIT_SETS];
        if constexpr (!ROWS) {
#pragma unroll
            for (uint32_t s = 0; s < INGOT_MAX_EMIT_SETS; ++s)
                v[s] = (s < a.n_sets && live) ? set_value(a.sets[s], i, H + L) : 0u;
        }
        uint8_t* D = a.dst + doff;
        const uint32_t T = H + L;
        const uint32_t dmis = (uint32_t)((uintptr_t)D & 15u);
        const uint32_t nch = live ? (dmis + T + 15u) / 16u : 0u;

        // 2. the packet's header block in its region: build_region's body
        //    (emit_common.h), kept here with the set values loaded before the
        //    destination is: called as a function it is the only shared step
        //    that changes this kernel's code, and the two-chunk copy without
        //    sums then measured 0.3 % slower
        //    (profiles/r18_csum_emit_shared_ab.json).  (2b) its sums' start
        uint8_t* R = regions + j * RS;
        if constexpr (ROWS) {
            build_region_rows(R, RS, tmpl, pieces, args.n_pieces, H, i, r, live, dmis, T);
        } else if (H && live) {
            for (uint32_t m = 0; m < RS / 16u; ++m) {
                const uint32_t tb = 16u + 16u * m - dmis;
                reinterpret_cast<u32x4*>(R)[m] = funnel(tmpl[tb >> 4], tmpl[(tb >> 4) + 1], tb & 15u);
            }
#pragma unroll
            for (uint32_t s = 0; s < INGOT_MAX_EMIT_SETS; ++s) {
                if (s >= a.n_sets) break;
                const EmitSet& e = a.sets[s];
                const uint32_t fm = e.bits >= 32 ? 0xffffffffu : ((1u << e.bits) - 1u);
                const uint32_t m = fm << e.rshift, vb = (v[s] & fm) << e.rshift;
                for (uint32_t k = 0; k < e.nbytes; ++k) {
                    const uint32_t shb = 8u * (e.nbytes - 1u - k);
                    uint8_t& b = R[dmis + e.pos + k];
                    b = (uint8_t)((b & ~(m >> shb)) | ((vb >> shb) & (m >> shb)));
                }
            }
        }
        if constexpr (SUMS) start_sums(R, a, live, dmis, T, acc + j);

        // 3. block counts -> inclusive prefix over the wave
        const uint32_t P = wave_inclusive_sum(nch, lane);
        wd.dst[j] = (uint64_t)(uintptr_t)D;
        wd.pfx[j] = P;
        wd.len[j] = L;
        wd.dmis[j] = (ROWS && !live) ? GUARDED : dmis;
        wd.cur[j] = cur;
        wd.s1[j] = s1;
        const uint32_t wtotal = (uint32_t)__shfl((int)P, (int)WAVE - 1);
        if (lane == 0) wd.sub[wg] = wtotal;
    }  // wg < PW
    __syncthreads();
    // subgroups 1.. continue the prefix of the ones before them
    if (wg > 0 && wg < PW) {
        uint32_t before = 0;
        for (uint32_t t = 0; t < wg; ++t) before += wd.sub[t];
        wd.pfx[wg * WAVE + lane] += before;
    }
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (uint32_t t = 0; t < PW; ++t) total += wd.sub[t];

    // 4. the wave's blocks, 64 per step and UNROLL steps at a time: block k
    //    belongs to the first packet whose inclusive prefix exceeds k
    // ROWS keeps the UNROLL steps: 63 / 57 VGPRs as they are without it
    constexpr uint32_t U = UNROLL;
    for (uint32_t k0 = wg * WAVE * U; k0 < total; k0 += W * WAVE * U) {
        uint32_t q[U], c[U];
        uint32_t fl[U];  // shift | extra << 4 | last << 5
        u32x4 own[U], nb[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t k = k0 + u * WAVE + lane;
            const bool valid = k < total;
            uint32_t qq = 0;
#pragma unroll
            for (uint32_t step = NPOW / 2; step; step >>= 1)
                if (wd.pfx[qq + step - 1] <= k) qq += step;
            qq = valid ? qq : 0u;
            const uint32_t end = wd.pfx[qq];
            c[u] = valid ? k - (qq ? wd.pfx[qq - 1] : 0u) : 0xffffu;
            q[u] = qq;
            const bool last = SUMS && valid && (lane == WAVE - 1 || k + 1 >= end);
            own[u] = u32x4{0u, 0u, 0u, 0u};
            nb[u] = u32x4{0u, 0u, 0u, 0u};
            uint64_t B = 0;       // the aligned block this lane loaded as `own` (0: none)
            uint32_t sh = 0;
            bool second = false;  // the funnel also needs block B + 16
            if (valid) {
                const uint32_t t = wd.len[qq];
                const int32_t r0 = (int32_t)(16u * c[u]) - (int32_t)wd.dmis[qq];
                const int32_t x0 = r0 - (int32_t)H;  // payload offset of the block's byte 0
                const int32_t p0 = max(-x0, 0), p1 = min((int32_t)t - x0, 16);
                if (p0 < p1) {
                    const uint32_t xa = (uint32_t)(x0 + p0), xb = (uint32_t)(x0 + p1);
                    uint32_t cs = wd.cur[qq], cx = wd.start[PIECES][qq];
                    Piece p = piece_at(wd, ar, qq, xa, t, cs, cx);
                    if (p.ok && p.end >= xb) {
                        // one piece: k_emit's load path
                        const uint64_t X = p.sbase + (uint64_t)(int64_t)x0;
                        const uint64_t S0 = p.sbase + p.start, S1 = p.sbase + p.end;
                        const uint64_t A = X & ~(uint64_t)15;
                        sh = (uint32_t)X & 15u;
                        if (A + 16 > S0 && A < S1) {
                            own[u] = *(const __attribute__((address_space(1))) u32x4*)A;
                            B = A;
                        }
                        second = sh != 0 && A + 16 < S1 && A + 32 > S0;
                        if (second && B == 0) {  // only the second block holds bytes
                            nb[u] = *(const __attribute__((address_space(1))) u32x4*)(A + 16);
                            second = false;
                            sh |= 16u;
                        }
                    } else {
                        // a chunk boundary inside the block: piece by piece
                        u32x4 o = u32x4{0u, 0u, 0u, 0u};
                        uint32_t x = xa;
                        while (p.ok) {
                            const uint32_t e = min(p.end, xb);
                            const u32x4 pv = piece_block(p, p.sbase + (uint64_t)(int64_t)x0);
                            const int32_t b0 = (int32_t)x - x0, b1 = (int32_t)e - x0;
                            o.x |= pv.x & below(b1) & ~below(b0);
                            o.y |= pv.y & below(b1 - 4) & ~below(b0 - 4);
                            o.z |= pv.z & below(b1 - 8) & ~below(b0 - 8);
                            o.w |= pv.w & below(b1 - 12) & ~below(b0 - 12);
                            x = e;
                            if (x >= xb) break;
                            p = piece_at(wd, ar, qq, x, t, cs, cx);
                        }
                        own[u] = o;
                    }
                }
            }
            // the next lane holds block B + 16 only if it loaded exactly that
            const uint32_t nlo = from_next_lane((uint32_t)B), nhi = from_next_lane((uint32_t)(B >> 32));
            const uint64_t NB = ((uint64_t)nhi << 32) | nlo;
            if (second && NB != B + 16) {
                nb[u] = *(const __attribute__((address_space(1))) u32x4*)(B + 16);
                sh |= 16u;
            }
            fl[u] = sh | (last ? 32u : 0u);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const bool valid = c[u] != 0xffffu;
            const uint32_t qq = q[u];
            const uint32_t qd = wd.dmis[qq];
            uint8_t* QD = (uint8_t*)(uintptr_t)wd.dst[qq];
            const uint32_t QT = H + wd.len[qq];
            const int32_t r0 = (int32_t)(16u * c[u]) - (int32_t)qd;
            u32x4 n2;
            n2.x = from_next_lane(own[u].x);
            n2.y = from_next_lane(own[u].y);
            n2.z = from_next_lane(own[u].z);
            n2.w = from_next_lane(own[u].w);
            u32x4 out = funnel(own[u], (fl[u] & 16u) ? nb[u] : n2, fl[u] & 15u);
            if (H && valid && r0 < (int32_t)H)
                merge_header(out, *reinterpret_cast<const u32x4*>(regions + qq * RS + 16u * c[u]),
                             H, r0);
            bool parked = false;
            if constexpr (SUMS) {
                if (udp)
                    parked = udp_share(out, valid, fl[u] & 32u, c[u], qq, qd, H, QT, r0, fpos, lane,
                                       acc, park, NP);
            }
            if (valid && !parked) store_chunk(QD, r0, QT, out);
        }
    }
    if constexpr (SUMS) {
        if (!udp) return;
        // 5. the parked blocks, once the group has summed every block
        __syncthreads();
        const uint32_t slot = threadIdx.x / NP, j = threadIdx.x % NP;
        if (slot >= 2u || base + j >= a.n) return;
        if (ROWS && wd.dmis[j] == GUARDED) return;  // nothing parked, nothing to store
        finish_parked(a, fpos, slot, wd.dmis[j], H + wd.len[j], (uint8_t*)(uintptr_t)wd.dst[j],
                      park + slot * NP + j, acc + j);
    }
}

// Dynamic LDS of one k_emit_read block for a header block of H bytes.
template <bool SUMS>
constexpr size_t emit_read_smem(uint32_t H) {
    return (INGOT_MAX_EMIT_HDR / 16 + 4) * 16 + sizeof(ReadDesc) + NP * region_bytes(H) +
           (SUMS ? NP * SUM_LDS_PER_PACKET : 0u);
}
// gfx950: 160 KiB of LDS per workgroup.
static_assert(emit_read_smem<true>(INGOT_MAX_EMIT_HDR) <= 160u * 1024u, "k_emit_read LDS > 160 KiB");
static_assert(emit_read_smem<true>(INGOT_MAX_EMIT_HDR) + sizeof(EmitReadRowsArgs::p) <= 160u * 1024u,
              "k_emit_read<sums, rows> LDS > 160 KiB");
static_assert(BLOCK >= 2 * NP, "sums: one lane per parked block");

template <bool SUMS>
hipError_t go(const EmitReadArgs& a, hipStream_t s) {
    const uint64_t blocks = (a.e.n + NP - 1) / NP;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_emit_read<SUMS>), dim3((uint32_t)blocks), dim3(BLOCK),
                       emit_read_smem<SUMS>(a.e.hdr_len), s, a);
    return hipGetLastError();
}

}  // namespace

size_t emit_read_lds_bytes(const EmitReadArgs& a) {
    return (a.e.sums.v4 || a.e.sums.udp) ? emit_read_smem<true>(a.e.hdr_len)
                                         : emit_read_smem<false>(a.e.hdr_len);
}

hipError_t launch_emit_read(const EmitReadArgs& a, hipStream_t s) {
    if (a.e.n == 0) return hipSuccess;
    return (a.e.sums.v4 || a.e.sums.udp) ? go<true>(a, s) : go<false>(a, s);
}

// The rows kernels: k_emit_read's launch shape and LDS (sums or not), and the pieces.
size_t emit_read_rows_lds_bytes(const EmitReadRowsArgs& a) { return emit_read_lds_bytes(a.r) + sizeof(a.p); }

hipError_t launch_emit_read_rows(const EmitReadRowsArgs& a, hipStream_t s) {
    if (a.r.e.n == 0) return hipSuccess;
    const uint64_t blocks = (a.r.e.n + NP - 1) / NP;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t smem = emit_read_rows_lds_bytes(a);
    if (a.r.e.sums.v4 || a.r.e.sums.udp)
        hipLaunchKernelGGL((k_emit_read<true, true>), dim3((uint32_t)blocks), dim3(BLOCK), smem, s, a);
    else
        hipLaunchKernelGGL((k_emit_read<false, true>), dim3((uint32_t)blocks), dim3(BLOCK), smem, s, a);
    return hipGetLastError();
}

}  // namespace ingot_gpu
