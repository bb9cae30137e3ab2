// csum.hip — batched Internet checksums (ingot_gpu_checksum_verify / _fill:
// k_csum, described here; over chunk lists, ingot_gpu_checksum_verify_read /
// _fill_read: k_csum_read, described where it stands, below).
//
// RFC 1071 sums of already parsed frames: the IPv4 header checksum and the
// TCP / UDP / ICMP checksum over the pseudo-header and the whole L4 segment.
// The first kernel here whose work is the payload, not the header lines: a
// streaming segmented reduction (include/ingot_gpu.h states the semantics,
// tests/csum_model.py defines them).
//
// A group of 4 x 64 packets per 256-thread workgroup, the read side of
// emit.hip.  Lane j of wave w loads packet 64 w + j's descriptors and record
// (coalesced) and reads the few header bytes it needs as unaligned dwords
// (header_sums, own_field).  A scan of the packets' 16-B chunk counts turns
// the group's L4 segments into one flat run of aligned 16-B chunks, which the
// four waves take in turns, 64 chunks per step (reduce_blocks): no global
// atomics, no LDS atomic per chunk.  The owning lane then turns the packet's
// accumulator into the checksum and writes the 8-B record and, in fill mode,
// the two field bytes (finish).  Both kernels share these four functions;
// what a kernel keeps is how it finds the header and cuts the segment.
// HBM-bound: algorithmic bytes per packet = the segment + the header dwords +
// 10 B of descriptors + the 16-B record read, 8 B written.
#include <hip/hip_runtime.h>

#include "../../include/ingot_gpu.h"
#include "kernels.h"
#include "sums.h"

namespace ingot_gpu {
namespace {

constexpr uint32_t W = 4;          // waves per workgroup = 64-packet subgroups per group
constexpr uint32_t NP = W * WAVE;  // packets per group
constexpr uint32_t BLOCK = NP;
constexpr uint32_t UNROLL = 4;     // 64-chunk steps whose loads fly together

typedef uint32_t u32u __attribute__((aligned(1)));  // a dword at any byte address

// The dword at p (any alignment), bytes in memory order from bit 0.
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
    return *(const __attribute__((address_space(1))) u32u*)p;
}
// Its two 16-bit words read big-endian, added.
__device__ __forceinline__ uint32_t be_words(uint32_t w) {
    const uint32_t b = __builtin_bswap32(w);
    return (b >> 16) + (b & 0xffffu);
}
__device__ __forceinline__ uint32_t be16_lo(uint32_t w) {  // bytes 0, 1 of w as a BE u16
    return ((w & 0xffu) << 8) | ((w >> 8) & 0xffu);
}
__device__ __forceinline__ uint32_t be16_hi(uint32_t w) {  // bytes 2, 3
    return ((w >> 8) & 0xff00u) | (w >> 24);
}

// What a lane keeps of its packet from the header decode to the finish.
struct Lane {
    uint32_t st3 = INGOT_CSUM_NONE, st4 = INGOT_CSUM_NONE, sum3 = 0, seg = 0;
    uint32_t pseudo = 0;    // the pseudo-header's words, big-endian, added
    uint8_t* A = nullptr;   // the segment's first byte, when it is summed
    uint8_t* P3 = nullptr;  // the IPv4 header, when its sum is wanted
    uint32_t foff = 0, fhi = 0, flo = 0;  // the L4 field: offset in the segment, its bytes
    bool udp = false;
};

// The header at H (logical offset l3_off; its bytes up to logical offset
// `lim` are readable there, and so is [l3_off, l4_off) when geo4): the IPv4
// header sum, the segment's end, the fragment test and the pseudo-header
// words.  Returns whether the segment [l4_off, l4_off + p.seg) is to be
// summed; L is the frame's length.
__device__ __forceinline__ bool header_sums(Lane& p, const uint8_t* H, bool v4, bool geo4,
                                            uint32_t l3_off, uint32_t l4_off,
                                            uint32_t payload_off, uint32_t n_v6ext,
                                            uint32_t l4_proto, uint32_t what, uint32_t fill,
                                            uint32_t lim, uint32_t L) {
    uint32_t end = 0;
    bool frag = false;
    if (v4) {
        const uint32_t w0 = ld32(H), w1 = ld32(H + 4), w2 = ld32(H + 8), w3 = ld32(H + 12),
                       w4 = ld32(H + 16);
        const uint32_t hl = max(20u, (w0 & 0xfu) * 4u);
        if ((what & INGOT_CSUM_L3) && l3_off + hl <= lim) {
            uint32_t s = be_words(w0) + be_words(w1) + be_words(w2) + be_words(w3) + be_words(w4);
            for (uint32_t k = 20; k < hl; k += 4) s += be_words(ld32(H + k));
            const uint32_t field = be16_hi(w2);
            p.sum3 = ~fold16(s - field) & 0xffffu;
            p.st3 = (fill || fold16(s) == 0xffffu) ? INGOT_CSUM_OK : INGOT_CSUM_BAD;
            p.P3 = const_cast<uint8_t*>(H);
        }
        end = l3_off + be16_hi(w0);
        frag = (be16_hi(w1) & 0x3fffu) != 0;  // MF or a fragment offset
        p.pseudo = be_words(w3) + be_words(w4) + ((w2 >> 8) & 0xffu);
    } else if (geo4) {
        const uint32_t w1 = ld32(H + 4);
        end = l3_off + 40u + be16_lo(w1);
#pragma unroll
        for (uint32_t k = 8; k < 40; k += 4) p.pseudo += be_words(ld32(H + k));
        p.pseudo += l4_proto;
        uint32_t pos = 40u, h = (w1 >> 16) & 0xffu;
        for (uint32_t e = 0; e < n_v6ext && l3_off + pos + 8u <= l4_off; ++e) {
            const uint32_t b = ld32(H + pos);
            if (h == 44u) {
                const uint32_t fo = be16_hi(b);  // offset (13 bits), res, M
                frag = frag || (fo & 0xfff9u) != 0;
                pos += 8u;
            } else {
                pos += 8u + ((b >> 8) & 0xffu) * 8u;
            }
            h = b & 0xffu;
        }
    }
    if (!geo4) return false;
    if (end > L || end < payload_off) {
        p.st4 = INGOT_CSUM_SHORT;
    } else if (frag) {
        p.st4 = INGOT_CSUM_FRAGMENT;
    } else {
        p.seg = end - l4_off;
        return true;
    }
    return false;
}

// The segment of p.seg bytes starts at A: its checksum field's place and own
// bytes (the finish takes them out again), the length into the pseudo-header.
__device__ __forceinline__ void own_field(Lane& p, uint8_t* A, uint32_t l4_kind) {
    p.A = A;
    p.udp = l4_kind == INGOT_L4_UDP;
    p.foff = l4_kind == INGOT_L4_TCP ? 16u : p.udp ? 6u : 2u;
    p.fhi = gbl(A)[p.foff];
    p.flo = gbl(A)[p.foff + 1];
    p.pseudo = l4_kind == INGOT_L4_ICMPV4 ? 0u : p.pseudo + p.seg;
    p.st4 = INGOT_CSUM_OK;  // decided in finish
}

// `total` aligned 16-B blocks, the flat run of SPAN owners' pieces: owner q
// has the blocks [pfx[q - 1], pfx[q]) from address base[q] on, of which the
// bytes from span[q] & 15 of the first block on, ((span[q] >> 4) & 0xffff) of
// them, count.  The workgroup's W waves take the run in turns, 64 blocks per
// step and UNROLL steps at a time (their loads are issued together).  A lane
// finds its block's owner by binary search of the prefix (block k belongs to
// the first owner whose inclusive prefix exceeds k), masks the bytes outside
// the piece and adds the eight 16-bit words as loaded (little-endian) into 32
// bits — 65,535 bytes of 0xff stay below 2^31, so nothing is folded on the
// way.  The lanes of one owner are contiguous: a segmented scan over the wave
// leaves each owner's share in its last lane, which alone calls
// add(q, span[q], share).
template <uint32_t SPAN, class Add>
__device__ __forceinline__ void reduce_blocks(const uint32_t* pfx, const uint64_t* base,
                                              const uint32_t* span, uint32_t total,
                                              uint32_t wave, uint32_t lane, Add add) {
    for (uint32_t k0 = wave * WAVE * UNROLL; k0 < total; k0 += W * WAVE * UNROLL) {
        uint32_t q[UNROLL], c[UNROLL];
        u32x4 v[UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) {
            const uint32_t k = k0 + u * WAVE + lane;
            const bool valid = k < total;
            uint32_t qq = 0;
#pragma unroll
            for (uint32_t step = SPAN / 2; step; step >>= 1)
                if (pfx[qq + step - 1] <= k) qq += step;
            qq = valid ? qq : 0u;
            q[u] = valid ? qq : 0xffffffffu;
            c[u] = k - (qq ? pfx[qq - 1] : 0u);
            v[u] = u32x4{0u, 0u, 0u, 0u};
            if (valid)
                v[u] = *(const __attribute__((address_space(1))) u32x4*)(uintptr_t)(
                    base[qq] + 16ull * c[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) {
            const bool valid = q[u] != 0xffffffffu;
            const uint32_t sp = span[valid ? q[u] : 0u];
            // the piece's bytes inside this block: [t0, t1)
            const int32_t first = (int32_t)(sp & 15u) - (int32_t)(16u * c[u]);
            const int32_t t0 = max(first, 0), t1 = min(first + (int32_t)((sp >> 4) & 0xffffu), 16);
            // Deliberate: both arms give the same sum, but only a piece's first and
            // last block have bytes to mask, and the constant arm lets every other
            // block skip the masks (a plain call costs 5 VGPRs and k_csum_read a wave).
            uint32_t s = (t0 != 0 || t1 != 16) ? chunk_words(v[u], t0, t1) : chunk_words(v[u], 0, 16);
            s = owner_inclusive_sum(s, q[u], lane);
            const uint32_t next = (uint32_t)__shfl_down((int)q[u], 1);
            if (valid && (lane == WAVE - 1 || next != q[u])) add(q[u], sp, s);
        }
    }
}

// The owning lane: the field's own bytes out of its class, fold, byte order,
// the pseudo-header; the row and, in fill mode, the field bytes.  a0 / a1 are
// the sums of the segment's 16-bit words as loaded, by class: the parity of a
// byte's address XOR the parity of its offset in the segment.  The field's
// bytes are in the class of the segment's first byte (foff is even).  Class 0
// has the big-endian high byte in the low lane, so its fold is swapped.
__device__ __forceinline__ void finish(const Lane& p, uint32_t a0, uint32_t a1, uint32_t fill,
                                       ingot_csum* row) {
    uint32_t sum4 = 0, st4 = p.st4;
    if (p.A) {
        const uint32_t odd = (uint32_t)(uintptr_t)p.A & 1u;
        const uint32_t own = (p.fhi << (8u * odd)) + (p.flo << (8u * (odd ^ 1u)));
        if (odd) a1 -= own; else a0 -= own;
        const uint32_t s0 = fold16(swap16(fold16(a0)) + fold16(a1) + p.pseudo);
        sum4 = ~s0 & 0xffffu;
        if (p.udp && sum4 == 0) sum4 = 0xffffu;
        const uint32_t field = (p.fhi << 8) | p.flo;
        if (fill) {
            gbl_mut(p.A)[p.foff] = (uint8_t)(sum4 >> 8);
            gbl_mut(p.A)[p.foff + 1] = (uint8_t)sum4;
        } else {
            st4 = (p.udp && field == 0) ? INGOT_CSUM_ZERO
                  : fold16(s0 + field) == 0xffffu ? INGOT_CSUM_OK
                                                  : INGOT_CSUM_BAD;
        }
    }
    if (fill && p.P3) {
        gbl_mut(p.P3)[10] = (uint8_t)(p.sum3 >> 8);
        gbl_mut(p.P3)[11] = (uint8_t)p.sum3;
    }
    if (row)
        *(__attribute__((address_space(1))) u32x2*)row =
            u32x2{p.st3 | (st4 << 8) | (p.sum3 << 16), sum4 | (p.seg << 16)};
}

struct Group {
    uint64_t base[NP];  // address of the 16-B block holding the segment's first byte
    uint32_t pfx[NP];   // inclusive prefix of the packets' chunk counts
    uint32_t span[NP];  // the segment inside its chunks: first byte (0..15) | bytes << 4
    uint32_t acc[NP];   // sum of the segment's 16-bit words as loaded
    uint32_t sub[W];    // chunks of each 64-packet subgroup
};

__global__ __launch_bounds__(BLOCK) void k_csum(CsumArgs a) {
    __shared__ Group g;
    const uint32_t t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
    const uint64_t i = (uint64_t)blockIdx.x * NP + t;
    const bool live = i < a.n;

    // 1. packet t of the group: record, descriptors, header bytes
    Lane p;
    uint32_t nch = 0;
    if (live) {
        const u32x4 r = *(const __attribute__((address_space(1))) u32x4*)(a.rec + i);
        const uint32_t status = r.x & 0xffu, l3_kind = (r.x >> 16) & 0xffu, l4_kind = r.x >> 24;
        const uint32_t n_v6ext = (r.y >> 8) & 0xffu, l4_proto = (r.y >> 16) & 0xffu;
        const uint32_t l3_off = r.z & 0xffffu, l4_off = r.z >> 16, payload_off = r.w & 0xffffu;
        const uint64_t off = a.off ? gbl(a.off)[i] : i * (uint64_t)a.stride;
        const uint32_t L = a.len ? (uint32_t)gbl(a.len)[i] : a.stride;
        uint8_t* F = a.arena + off;
        const bool v4 = l3_kind == INGOT_L3_IPV4, v6 = l3_kind == INGOT_L3_IPV6;
        const uint32_t fixed = v4 ? 20u : 40u;
        if (status == INGOT_OK && (v4 || v6) && l3_off + fixed <= L) {
            const uint32_t min4 = l4_kind == INGOT_L4_TCP ? 20u : 8u;
            const bool geo4 = (a.what & INGOT_CSUM_L4) && l4_kind >= INGOT_L4_TCP &&
                              l4_kind <= INGOT_L4_ICMPV6 && l3_off + fixed <= l4_off &&
                              l4_off + min4 <= payload_off && payload_off <= L;
            if (header_sums(p, F + l3_off, v4, geo4, l3_off, l4_off, payload_off, n_v6ext,
                            l4_proto, a.what, a.fill, /*lim=*/L, /*L=*/L)) {
                own_field(p, F + l4_off, l4_kind);
                nch = (((uint32_t)(uintptr_t)p.A & 15u) + p.seg + 15u) / 16u;
            }
        }
    }

    // 2. chunk counts -> inclusive prefix over the wave, then over the group
    const uint32_t P = wave_inclusive_sum(nch, lane);
    const uint32_t lo = (uint32_t)(uintptr_t)p.A & 15u;
    g.base[t] = (uint64_t)(uintptr_t)p.A - lo;
    g.pfx[t] = P;
    g.span[t] = lo | (p.seg << 4);
    g.acc[t] = 0;
    if (lane == WAVE - 1) g.sub[wave] = P;
    __syncthreads();
    if (wave > 0) {
        uint32_t before = 0;
        for (uint32_t w = 0; w < wave; ++w) before += g.sub[w];
        g.pfx[t] += before;
    }
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (uint32_t w = 0; w < W; ++w) total += g.sub[w];

    // 3. the group's chunks: a packet is one piece
    reduce_blocks<NP>(g.pfx, g.base, g.span, total, wave, lane,
                      [&](uint32_t q, uint32_t, uint32_t s) { atomicAdd(&g.acc[q], s); });
    __syncthreads();

    // 4. the one-piece case of finish: every byte's offset in the segment is
    //    its distance from A, so the whole sum is in the class of A's parity
    const uint32_t odd = (uint32_t)(uintptr_t)p.A & 1u, sum = g.acc[t];
    finish(p, odd ? 0u : sum, odd ? sum : 0u, a.fill, live && a.out ? a.out + i : nullptr);
}

}  // namespace

hipError_t launch_csum(const CsumArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint64_t blocks = (a.n + NP - 1) / NP;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_csum, dim3((uint32_t)blocks), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_csum_read — the same sums over the chunk tables of ingot_gpu_parse_read
// (ingot_gpu_checksum_verify_read / _fill_read; tests/csum_read_model.py is
// the definition).  k_csum's shape and functions, with the segment a list of
// pieces.
//
// Lane j of wave w owns packet 64 w + j: it walks the packet's chunk lengths
// once for the logical length L (cut at 65,535) and the chunks that hold
// l3_off and l4_off, applies the one-chunk rule (a header is read from one
// chunk) and reads the header bytes from that chunk.  The segment
// [l4_off, end) is then cut into pieces, the part of each chunk inside it:
// (address of the first byte, bytes, class), the class being finish's.  The
// workgroup keeps a table of PIECES = 256 x 4 pieces in LDS and fills it in
// rounds: every round a packet adds up to PER_ROUND pieces to its own slots,
// continuing its walk from registers (chunk index, logical start), so any
// number of pieces per packet is summed and a packet of 1-4 pieces takes one
// round.  A scan of the slots' 16-B block counts makes the round's pieces one
// flat run of aligned blocks for reduce_blocks, keyed by the slot.  A packet
// has two accumulators in LDS, one per class, that persist over the rounds:
// words added as loaded, each below 2^31 for 65,535 bytes of 0xff.  No global
// atomics, no device allocation.
namespace {

constexpr uint32_t PER_ROUND = 4;          // pieces a packet adds per round
constexpr uint32_t PIECES = NP * PER_ROUND;  // capacity of the piece table
constexpr uint32_t MAX_FRAME = 65535;      // parse_read sees no later byte

struct ReadGroup {
    uint64_t base[PIECES];  // address of the 16-B block holding the piece's first byte
    uint32_t pfx[PIECES];   // inclusive prefix of the slots' block counts
    uint32_t span[PIECES];  // first byte in its block (0..15) | bytes << 4 | class << 20
    uint32_t acc[2][NP];    // per class: the sum of the packet's 16-bit words as loaded
    uint32_t sub[W];        // blocks of each 64-packet subgroup, this round
    uint32_t more[W];       // a packet of the subgroup has pieces left
};

__global__ __launch_bounds__(BLOCK) void k_csum_read(CsumReadArgs a) {
    __shared__ ReadGroup g;
    const uint32_t t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
    const uint64_t i = (uint64_t)blockIdx.x * NP + t;
    const bool live = i < a.n;

    // 1. packet t of the group: record, chunk walk, the one-chunk rule, header bytes
    Lane p;
    // the piece walk: chunk `ck` (arena offset cat, logical bytes [cstart, cstart + clen)),
    // the next byte to take `pos`, the walk's end `wend`, the table's last chunk index
    uint32_t ck = 0, cstart = 0, clen = 0, pos = 0, wend = 0, l4 = 0, k_end = 0;
    uint64_t cat = 0;
    if (live) {
        const u32x4 r = *(const __attribute__((address_space(1))) u32x4*)(a.rec + i);
        const uint32_t status = r.x & 0xffu, l3_kind = (r.x >> 16) & 0xffu, l4_kind = r.x >> 24;
        const uint32_t n_v6ext = (r.y >> 8) & 0xffu, l4_proto = (r.y >> 16) & 0xffu;
        const uint32_t l3_off = r.z & 0xffffu, l4_off = r.z >> 16, payload_off = r.w & 0xffffu;
        const bool v4 = l3_kind == INGOT_L3_IPV4, v6 = l3_kind == INGOT_L3_IPV6;
        const uint32_t fixed = v4 ? 20u : 40u;
        if (status == INGOT_OK && (v4 || v6)) {
            const uint32_t k_lo = gbl(a.pkt_seg)[i];
            k_end = max(gbl(a.pkt_seg)[i + 1], k_lo);
            // logical starts: the chunks of l3_off and l4_off, and L
            uint32_t L = 0, k3 = 0, s3 = 0, n3 = 0, k4 = 0, s4 = 0, n4 = 0;
            for (uint32_t k = k_lo; k < k_end && L < MAX_FRAME; ++k) {
                const uint32_t ln = min((uint32_t)gbl(a.seg_len)[k], MAX_FRAME - L);
                if (l3_off - L < ln) k3 = k, s3 = L, n3 = ln;  // L <= l3_off < L + ln
                if (l4_off - L < ln) k4 = k, s4 = L, n4 = ln;
                L += ln;
            }
            // n3 != 0: l3_off lies in chunk k3; the fixed header must end in it too
            if (n3 && l3_off + fixed <= s3 + n3) {
                const uint64_t at3 = gbl(a.seg_off)[k3];
                const uint32_t e3 = s3 + n3;  // chunk k3 ends here
                const uint32_t min4 = l4_kind == INGOT_L4_TCP ? 20u : 8u;
                const bool geo4 = (a.what & INGOT_CSUM_L4) && l4_kind >= INGOT_L4_TCP &&
                                  l4_kind <= INGOT_L4_ICMPV6 && l3_off + fixed <= l4_off &&
                                  l4_off + min4 <= payload_off && payload_off <= L &&
                                  l4_off <= e3 &&                  // [l3_off, l4_off) in one chunk
                                  n4 && payload_off <= s4 + n4;    // [l4_off, payload_off) too
                if (header_sums(p, a.arena + at3 + (l3_off - s3), v4, geo4, l3_off, l4_off,
                                payload_off, n_v6ext, l4_proto, a.what, a.fill, /*lim=*/e3,
                                /*L=*/L)) {
                    cat = k4 == k3 ? at3 : gbl(a.seg_off)[k4];
                    ck = k4, cstart = s4, clen = n4;
                    pos = l4 = l4_off, wend = l4_off + p.seg;
                    own_field(p, a.arena + cat + (l4_off - s4), l4_kind);
                }
            }
        }
    }
    g.acc[0][t] = 0;
    g.acc[1][t] = 0;

    for (;;) {
        // 2. up to PER_ROUND pieces of this packet into its slots, their block
        //    counts scanned over the wave, then over the group
        uint32_t made = 0, mine = 0;
        while (made < PER_ROUND && pos < wend) {
            if (pos >= cstart + clen) {  // the next chunk (end <= L: there is one)
                if (++ck >= k_end) {
                    pos = wend;
                    break;
                }
                cstart += clen;
                clen = min((uint32_t)gbl(a.seg_len)[ck], MAX_FRAME - cstart);
                if (clen) cat = gbl(a.seg_off)[ck];  // an empty chunk's offset is not read
                continue;
            }
            const uint32_t nb = min(wend, cstart + clen) - pos;
            const uint64_t at = (uint64_t)(uintptr_t)a.arena + cat + (pos - cstart);
            const uint32_t lo = (uint32_t)at & 15u, cls = ((uint32_t)at ^ (pos - l4)) & 1u;
            const uint32_t nblk = (lo + nb + 15u) / 16u, s = PER_ROUND * t + made;
            g.base[s] = at - lo;
            g.span[s] = lo | (nb << 4) | (cls << 20);
            g.pfx[s] = nblk;
            mine += nblk;
            pos += nb;
            ++made;
        }
        for (uint32_t j = made; j < PER_ROUND; ++j) g.pfx[PER_ROUND * t + j] = 0;
        const uint32_t P = wave_inclusive_sum(mine, lane);
        const bool left = __ballot(pos < wend) != 0;
        if (lane == WAVE - 1) {
            g.sub[wave] = P;
            g.more[wave] = left ? 1u : 0u;
        }
        __syncthreads();
        uint32_t before = 0, total = 0, more = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; ++w) {
            before += w < wave ? g.sub[w] : 0u;
            total += g.sub[w];
            more |= g.more[w];
        }
        uint32_t run = before + P - mine;
#pragma unroll
        for (uint32_t j = 0; j < PER_ROUND; ++j) {
            run += g.pfx[PER_ROUND * t + j];
            g.pfx[PER_ROUND * t + j] = run;
        }
        __syncthreads();

        // 3. the round's blocks (a slot without a piece has none)
        reduce_blocks<PIECES>(g.pfx, g.base, g.span, total, wave, lane,
                              [&](uint32_t q, uint32_t span, uint32_t s) {
                                  atomicAdd(&g.acc[(span >> 20) & 1u][q / PER_ROUND], s);
                              });
        __syncthreads();  // the accumulators are whole; the table may be refilled
        if (!more) break;
    }

    // 4. both classes
    finish(p, g.acc[0][t], g.acc[1][t], a.fill, live && a.out ? a.out + i : nullptr);
}

}  // namespace

hipError_t launch_csum_read(const CsumReadArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint64_t blocks = (a.n + NP - 1) / NP;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_csum_read, dim3((uint32_t)blocks), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace ingot_gpu
