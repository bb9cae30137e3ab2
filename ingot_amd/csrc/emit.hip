// emit.hip — batched Emit (ingot_gpu_emit_packets / ingot_gpu_emit_headers /
// ingot_gpu_emit_packets_csum: the SUMS instantiation, described where it starts /
// ingot_gpu_emit_packets_rows: the ROWS instantiations, described at k_emit).
//
// ingot's Emit (ingot-types/src/emit.rs:8-120) writes an owned header stack
// field by field (the generated emit_raw, ingot-macros/src/packet/mod.rs:
// 2097-2255), a tuple emits its members back to back and a `&[u8]` member is
// a plain copy.  Here one owned stack, serialised once on the host, goes in
// front of every packet of a batch with per-packet setters applied to it
// (bitfield.rs:188-315: the field's covering bytes read-modify-written
// big-endian) — OPTE's outbound Geneve encapsulation.
//
// The header block sits in LDS once per workgroup.  A group of 4 x 64
// packets: lane j of the group's wave w < 4 loads packet 64 w + j's
// descriptors and set values (coalesced) and patches the header block for it
// into an LDS region
// at its destination's 16-B alignment (template funnel-shifted, then the
// setters byte by byte: every covering byte's new value depends only on its
// own mask and value bits); a scan of the packets' chunk counts turns the
// group into one flat run of aligned 16-B destination chunks, which the
// group's 16 waves take in turns, 64 chunks per step.  A lane's chunk: its
// packet by binary search of the scan; the payload bytes as one aligned
// 16-B source block plus the next lane's (DPP), funnel-shifted by the
// packet's source-vs-destination misalignment; the header bytes from the
// region; a whole chunk leaves as one 16-B store, the two edge chunks a
// packet shares with its neighbours as predicated pieces (store_edge).
// HBM-bound copy: algorithmic bytes per packet = len + 24 B of descriptors
// and set values read, hdr_len + len written.
#include <type_traits>

#include "emit_common.h"

namespace ingot_gpu {
namespace {

#ifndef INGOT_EMIT_GROUP_WAVES
#define INGOT_EMIT_GROUP_WAVES 16
#endif
// Whole packets: the W waves of a workgroup share one group of packets and
// take turns over its chunks, so a group's span is written by W waves at once
// and the spans in flight sit closer together (a plain copy of this shape:
// 4.87 TB/s one wave per span, 5.40 four).  A group is PW subgroups of 64
// packets whose descriptors PW waves load and patch in parallel, so the
// walkers wait on one subgroup's prologue, not PW of them.  Measured with
// equal output checksums (profiles/r05_emit_probe_history.json, r05aj /
// r05am / r05an): one wave per 64 packets 2.91 ms, W = 4 2.78-2.81, W = 16
// over four subgroups 2.65-2.77 (the best of W in {4, 6, 8, 10, 12, 16} with
// 1, 2, 3, 4, 8 or 16 subgroups).
// Header blocks: two one-wave groups.
#ifndef INGOT_EMIT_GROUP_SUBS
#define INGOT_EMIT_GROUP_SUBS 4
#endif
template <bool COPY> struct Shape {
    static constexpr uint32_t W = COPY ? INGOT_EMIT_GROUP_WAVES : 1u;  // waves per group
    static constexpr uint32_t PW = COPY ? INGOT_EMIT_GROUP_SUBS : 1u;  // 64-packet subgroups
    static constexpr uint32_t NP = PW * WAVE;                          // packets per group
    static constexpr uint32_t BLOCK = COPY ? W * WAVE : 2u * WAVE;
    static constexpr uint32_t G = BLOCK / (W * WAVE);                 // groups per block
    static_assert(PW <= W && PW <= 4, "one prologue wave per subgroup");
};
#ifndef INGOT_EMIT_UNROLL
#define INGOT_EMIT_UNROLL 4
#endif
constexpr uint32_t UNROLL = INGOT_EMIT_UNROLL;  // 64-chunk steps whose loads fly together

// Per-wave LDS: the 64 packets' descriptors, the inclusive prefix of their
// chunk counts, and each packet's patched header block at its destination's
// 16-B alignment (RS bytes per packet).
template <uint32_t NP>
struct WaveDesc {
    uint64_t dst[NP];     // destination address of packet j
    uint64_t src[NP];     // source address of its payload
    uint32_t pfx[NP];     // inclusive prefix of chunk counts
    uint32_t len[NP];     // payload bytes
    uint32_t mis[NP];     // dmis | s_mis << 8
    uint32_t sub[4];      // chunks of each 64-packet subgroup
    uint32_t cp, cp_inv;  // header blocks: chunk slots per packet, its reciprocal
    uint32_t _pad[WAVE - 6];
};

// The EmitArgs of either argument block.
__device__ __forceinline__ const EmitArgs& emit_args_of(const EmitArgs& a) { return a; }
__device__ __forceinline__ const EmitArgs& emit_args_of(const EmitRowsArgs& a) { return a.e; }

// ROWS (ingot_gpu_emit_packets_rows, whole packets only; its argument block is
// EmitRowsArgs): the prologue also loads the packet's row index, folds the row
// guard into `live` and takes the setters' operands from the pieces of
// EmitRowsArgs; a guarded packet has no chunks, so the walk never meets it,
// and step 5 skips it.  Everything after the prologue is the same code.
template <bool COPY, bool SUMS = false, bool ROWS = false>
__global__ __launch_bounds__(Shape<COPY>::BLOCK) void k_emit(
    std::conditional_t<ROWS, EmitRowsArgs, EmitArgs> args) {
    static_assert(COPY || !SUMS, "sums need the payload: whole packets only");
    static_assert(COPY || !ROWS, "rows: whole packets only");
    const EmitArgs& a = emit_args_of(args);
    constexpr uint32_t BLOCK = Shape<COPY>::BLOCK, W = Shape<COPY>::W, G = Shape<COPY>::G;
    constexpr uint32_t PW = Shape<COPY>::PW, NP = Shape<COPY>::NP;
    constexpr uint32_t NPOW = NP <= 64 ? 64 : NP <= 128 ? 128 : 256;  // search span
    using Desc = WaveDesc<NP>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    u32x4* tmpl = reinterpret_cast<u32x4*>(smem);
    load_template(tmpl, a, BLOCK);
    const uint32_t H = a.hdr_len;
    const uint32_t RS = region_bytes(H);
    const uint32_t lane = threadIdx.x % WAVE, g = threadIdx.x / (W * WAVE);
    const uint32_t wg = (threadIdx.x / WAVE) % W;  // this wave's turn in its group
    Desc& wd = reinterpret_cast<Desc*>(smem + TB * 16)[g];
    uint8_t* regions = smem + TB * 16 + G * sizeof(Desc) + g * NP * RS;
    // SUMS (G == 1): after the regions, the parked chunks, then the accumulators
    u32x4* park = reinterpret_cast<u32x4*>(smem + TB * 16 + G * sizeof(Desc) + G * NP * RS);
    uint32_t* acc = reinterpret_cast<uint32_t*>(park + 2u * NP);
    // ROWS: the pieces, after everything else
    EmitPiece* pieces = reinterpret_cast<EmitPiece*>(SUMS ? (void*)(acc + NP) : (void*)park);
    if constexpr (ROWS) load_pieces(pieces, args, BLOCK);
    const bool udp = SUMS && a.sums.udp;
    const uint32_t fpos = (uint32_t)a.sums.udp_at + 6u;  // the UDP checksum field in hdr
    __syncthreads();
    const uint64_t base = ((uint64_t)blockIdx.x * G + g) * NP;
    if (wg < PW) {
        // 1. wave wg of the group, lane j: packet base + 64 wg + j (coalesced
        //    descriptor and set-value loads)
        const uint32_t j = wg * WAVE + lane;  // the packet's index in the group
        const uint64_t i = base + j;
        bool live = i < a.n;
        uint32_t r = 0;  // ROWS: the packet's row index, loaded with its descriptors
        if constexpr (ROWS) {
            if (live && args.row) r = gbl(args.row)[i];
        }
        uint32_t L = live ? (uint32_t)gbl(a.len)[i] : 0u;
        uint64_t doff = live ? (a.dst_off ? gbl(a.dst_off)[i] : i * (uint64_t)a.stride) : 0u;
        uint64_t soff = (COPY && live) ? gbl(a.off)[i] : 0u;
        if constexpr (ROWS) {
            // the row guard: the descriptors of a guarded packet are dropped unused
            if (args.row && r >= args.n_rows) {
                live = false;
                L = 0u;
                doff = soff = 0u;
            }
        }
        uint8_t* D = a.dst + doff;
        const uint8_t* S = COPY ? a.src + soff : nullptr;
        const uint32_t T = H + (COPY ? L : 0u);
        const uint32_t dmis = (uint32_t)((uintptr_t)D & 15u);
        const uint32_t s_mis = COPY ? (uint32_t)((uintptr_t)(S - H - dmis) & 15u) : 0u;
        const uint32_t nch = live ? (dmis + T + 15u) / 16u : 0u;

        // 2. the packet's header block in its region, and (2b) its sums' start
        uint8_t* R = regions + j * RS;
        if constexpr (ROWS)
            build_region_rows(R, RS, tmpl, pieces, args.n_pieces, H, i, r, live, dmis, H + L);
        else build_region(R, RS, tmpl, a, i, live, dmis, H + L);
        if constexpr (SUMS) start_sums(R, a, live, dmis, H + L, acc + j);

        // 3. chunk counts -> inclusive prefix over the wave
        const uint32_t P = wave_inclusive_sum(nch, lane);
        wd.dst[j] = (uint64_t)(uintptr_t)D;
        wd.src[j] = (uint64_t)(uintptr_t)S;
        wd.pfx[j] = P;
        wd.len[j] = L;
        wd.mis[j] = (ROWS && !live) ? GUARDED : dmis | (s_mis << 8);
        // header blocks: every packet takes CP chunk slots, the most any packet
        // of this wave needs (5 for 74 B at 16-B aligned slots, 6 unaligned)
        uint32_t CP = nch;
#pragma unroll
        for (uint32_t o = 1; o < WAVE; o <<= 1) CP = max(CP, (uint32_t)__shfl_xor((int)CP, (int)o));
        CP = max(CP, 1u);
        const uint32_t cp_inv = CP > 1u ? 0xffffffffu / CP + 1u : 0u;  // CP == 1: q = k
        const uint32_t wtotal = COPY ? (uint32_t)__shfl((int)P, (int)WAVE - 1)
                                     : (base < a.n ? (uint32_t)min<uint64_t>(WAVE, a.n - base) * CP : 0u);
        if (lane == 0) {
            wd.sub[wg] = wtotal;
            wd.cp = CP;
            wd.cp_inv = cp_inv;
        }
    }  // wg < PW
    __syncthreads();
    if (PW > 1) {
        // subgroups 1.. continue the prefix of the ones before them
        if (wg > 0 && wg < PW) {
            uint32_t before = 0;
            for (uint32_t t = 0; t < wg; ++t) before += wd.sub[t];
            wd.pfx[wg * WAVE + lane] += before;
        }
        __syncthreads();
    }
    uint32_t total = 0;
#pragma unroll
    for (uint32_t t = 0; t < PW; ++t) total += wd.sub[t];
    const uint32_t CP = wd.cp, cp_inv = wd.cp_inv;

    // 4. the wave's chunks, 64 per step and UNROLL steps at a time (all their
    //    loads are issued before the first store: bytes in flight): chunk k
    //    belongs to the first packet whose inclusive prefix exceeds k
    // header blocks: no loads to overlap.  ROWS: one step fewer in flight: with
    // UNROLL steps these instantiations took 68 / 66 VGPRs, one workgroup per CU
    // instead of two (5.11 ms where k_emit<copy, sums> takes 3.61; with one fewer,
    // 56 / 54 VGPRs and 3.62 ms: profiles/r19_emit_rows_probe.json)
    constexpr uint32_t U = !COPY ? 2u : ROWS ? UNROLL - 1u : UNROLL;
    for (uint32_t k0 = wg * WAVE * U; k0 < total; k0 += W * WAVE * U) {
        uint32_t q[U], c[U];
        u32x4 own[U], nb[U];
        bool extra[U];
        bool last[U];  // SUMS: the wave's last chunk of its packet in this step
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t k = k0 + u * WAVE + lane;
            const bool valid = k < total;
            uint32_t qq = 0, end = 0;
            if (COPY) {
#pragma unroll
                for (uint32_t step = NPOW / 2; step; step >>= 1)
                    if ((NP == NPOW || qq + step <= NP) && wd.pfx[qq + step - 1] <= k) qq += step;
                qq = valid ? qq : 0u;
                end = wd.pfx[qq];
                c[u] = valid ? k - (qq ? wd.pfx[qq - 1] : 0u) : 0xffffu;
            } else {
                // header blocks: CP chunks per packet (the most any packet of
                // the wave needs); the ones past a packet's own count write
                // nothing.  k / CP as a multiply-high by the wave's reciprocal
                // (exact: k < 64 * CP)
                qq = valid ? (CP == 1u ? k : __umulhi(k, cp_inv)) : 0u;
                c[u] = valid ? k - qq * CP : 0xffffu;
            }
            q[u] = qq;
            last[u] = SUMS && valid && (lane == WAVE - 1 || k + 1 >= end);
            own[u] = u32x4{0u, 0u, 0u, 0u};
            nb[u] = u32x4{0u, 0u, 0u, 0u};
            extra[u] = false;
            if (COPY && valid) {
                const uint32_t mis = wd.mis[qq];
                const uint32_t qd = mis & 0xffu, qs = mis >> 8;
                const uint8_t* QS = (const uint8_t*)(uintptr_t)wd.src[qq];
                const int32_t r0 = (int32_t)(16u * c[u]) - (int32_t)qd;
                const uintptr_t X = (uintptr_t)QS + (intptr_t)(r0 - (int32_t)H);
                const uintptr_t B = X & ~(uintptr_t)15;
                const uintptr_t S0 = (uintptr_t)QS, S1 = (uintptr_t)QS + wd.len[qq];
                if (B + 16 > S0 && B < S1) own[u] = *(const __attribute__((address_space(1))) u32x4*)B;
                // the next lane holds block B + 16 only if it has this packet's next chunk
                if (qs != 0 && (lane == WAVE - 1 || k + 1 >= end) && B + 16 < S1 && B + 32 > S0) {
                    nb[u] = *(const __attribute__((address_space(1))) u32x4*)(B + 16);
                    extra[u] = true;
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const bool valid = c[u] != 0xffffu;
            const uint32_t qq = q[u];
            const uint32_t mis = wd.mis[qq];
            const uint32_t qd = mis & 0xffu, qs = mis >> 8;
            uint8_t* QD = (uint8_t*)(uintptr_t)wd.dst[qq];
            const uint32_t QT = H + (COPY ? wd.len[qq] : 0u);
            const int32_t r0 = (int32_t)(16u * c[u]) - (int32_t)qd;
            u32x4 out = u32x4{0u, 0u, 0u, 0u};
            if (COPY) {
                u32x4 n2;
                n2.x = from_next_lane(own[u].x);
                n2.y = from_next_lane(own[u].y);
                n2.z = from_next_lane(own[u].z);
                n2.w = from_next_lane(own[u].w);
                out = funnel(own[u], extra[u] ? nb[u] : n2, qs);
            }
            if (H && valid && r0 < (int32_t)H)
                merge_header(out, *reinterpret_cast<const u32x4*>(regions + qq * RS + 16u * c[u]),
                             H, r0);
            bool parked = false;
            if constexpr (SUMS) {
                if (udp)
                    parked = udp_share(out, valid, last[u], c[u], qq, qd, H, QT, r0, fpos, lane,
                                       acc, park, NP);
            }
            if (valid && !parked) store_chunk(QD, r0, QT, out);
        }
    }
    if constexpr (SUMS) {
        if (!udp) return;
        // 5. the parked chunks, once the block has summed every chunk
        __syncthreads();
        const uint32_t slot = threadIdx.x / NP, j = threadIdx.x % NP;
        if (slot >= 2u || base + j >= a.n) return;
        if (ROWS && wd.mis[j] == GUARDED) return;  // nothing parked, nothing to store
        finish_parked(a, fpos, slot, wd.mis[j] & 0xffu, H + wd.len[j],
                      (uint8_t*)(uintptr_t)wd.dst[j],
                      park + slot * NP + j, acc + j);
    }
}

// Dynamic LDS of one k_emit block for a header block of H bytes.
template <bool COPY, bool SUMS = false>
constexpr size_t emit_smem(uint32_t H) {
    return (INGOT_MAX_EMIT_HDR / 16 + 4) * 16 +
           Shape<COPY>::G * (sizeof(WaveDesc<Shape<COPY>::NP>) + Shape<COPY>::NP * region_bytes(H)) +
           (SUMS ? Shape<COPY>::NP * SUM_LDS_PER_PACKET : 0u);
}
// gfx950: 160 KiB of LDS per workgroup.  A build with other group shapes
// (INGOT_EMIT_GROUP_SUBS / _WAVES) must still fit the largest header block.
static_assert(emit_smem<true>(INGOT_MAX_EMIT_HDR) <= 160u * 1024u, "k_emit<copy> LDS > 160 KiB");
static_assert(emit_smem<false>(INGOT_MAX_EMIT_HDR) <= 160u * 1024u, "k_emit LDS > 160 KiB");
static_assert(emit_smem<true, true>(INGOT_MAX_EMIT_HDR) <= 160u * 1024u,
              "k_emit<copy, sums> LDS > 160 KiB");
static_assert(emit_smem<true, true>(INGOT_MAX_EMIT_HDR) + sizeof(EmitRowsArgs::p) <= 160u * 1024u,
              "k_emit<copy, sums, rows> LDS > 160 KiB");
static_assert(Shape<true>::G == 1 && Shape<true>::BLOCK >= 2 * Shape<true>::NP,
              "sums: one group per block, one lane per parked chunk");

template <bool COPY, bool SUMS = false>
hipError_t go(const EmitArgs& a, hipStream_t s) {
    constexpr uint32_t G = Shape<COPY>::G, NP = Shape<COPY>::NP;
    const uint64_t groups = (a.n + NP - 1) / NP;
    const uint64_t blocks = (groups + G - 1) / G;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t smem = emit_smem<COPY, SUMS>(a.hdr_len);
    hipLaunchKernelGGL((k_emit<COPY, SUMS>), dim3((uint32_t)blocks), dim3(Shape<COPY>::BLOCK), smem, s, a);
    return hipGetLastError();
}

}  // namespace

size_t emit_lds_bytes(const EmitArgs& a) {
    if (a.sums.v4 || a.sums.udp) return emit_smem<true, true>(a.hdr_len);
    return a.src ? emit_smem<true>(a.hdr_len) : emit_smem<false>(a.hdr_len);
}

// The rows kernels: k_emit<copy>'s launch shape and LDS (sums or not).
size_t emit_rows_lds_bytes(const EmitRowsArgs& a) {
    return ((a.e.sums.v4 || a.e.sums.udp) ? emit_smem<true, true>(a.e.hdr_len)
                                          : emit_smem<true>(a.e.hdr_len)) +
           sizeof(a.p);
}

hipError_t launch_emit_rows(const EmitRowsArgs& a, hipStream_t s) {
    if (a.e.n == 0) return hipSuccess;
    if (!a.e.src) return hipErrorInvalidValue;
    constexpr uint32_t NP = Shape<true>::NP;
    const uint64_t blocks = (a.e.n + NP - 1) / NP;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t smem = emit_rows_lds_bytes(a);
    if (a.e.sums.v4 || a.e.sums.udp)
        hipLaunchKernelGGL((k_emit<true, true, true>), dim3((uint32_t)blocks), dim3(Shape<true>::BLOCK),
                           smem, s, a);
    else
        hipLaunchKernelGGL((k_emit<true, false, true>), dim3((uint32_t)blocks), dim3(Shape<true>::BLOCK),
                           smem, s, a);
    return hipGetLastError();
}

hipError_t launch_emit(const EmitArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    if (a.sums.v4 || a.sums.udp) return a.src ? go<true, true>(a, s) : hipErrorInvalidValue;
    return a.src ? go<true>(a, s) : go<false>(a, s);
}

}  // namespace ingot_gpu
