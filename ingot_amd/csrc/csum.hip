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
// (coalesced) and reads the few header bytes it needs as unaligned dwords:
// the lengths, the fragment test, the IPv4 header sum and the pseudo-header.
// A scan of the packets' 16-B chunk counts turns the group's L4 segments into
// one flat run of aligned 16-B chunks, which the four waves take in turns, 64
// chunks per step; a lane finds its chunk's packet by binary search of the
// scan, masks the bytes outside [l4_off, end) and adds the eight 16-bit words
// as loaded (little-endian) into 32 bits — 65,535 bytes of 0xff stay below
// 2^31, so nothing is folded on the way.  Lanes of one packet are contiguous:
// a segmented scan over the wave (shuffles) leaves each packet's share in its
// last lane, and only those lanes touch the packet's LDS accumulator (no
// global atomics, no LDS atomic per chunk).  The owning lane then takes the
// checksum field's own bytes out again (an exact integer subtraction: it read
// them itself), folds, swaps the bytes once — the ones'-complement sum is
// byte-order independent — unless the segment starts at an odd address (a
// second swap), adds the pseudo-header, and writes the 8-B record and, in
// fill mode, the two field bytes (byte stores: the field may sit at an odd
// address).  HBM-bound: algorithmic bytes per packet = the segment + the
// header dwords + 10 B of descriptors + the 16-B record read, 8 B written.
#include <hip/hip_runtime.h>

#include "../../include/ingot_gpu.h"
#include "kernels.h"

namespace ingot_gpu {
namespace {

constexpr uint32_t WAVE = 64;
constexpr uint32_t W = 4;          // waves per workgroup = 64-packet subgroups per group
constexpr uint32_t NP = W * WAVE;  // packets per group
constexpr uint32_t BLOCK = NP;
constexpr uint32_t UNROLL = 4;     // 64-chunk steps whose loads fly together

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32u __attribute__((aligned(1)));  // a dword at any byte address

template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* gbl(const T* p) {
    return (const __attribute__((address_space(1))) T*)p;
}
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T* gbl_mut(T* p) {
    return (__attribute__((address_space(1))) T*)p;
}

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
__device__ __forceinline__ uint32_t fold(uint32_t x) {
    x = (x & 0xffffu) + (x >> 16);
    return (x & 0xffffu) + (x >> 16);
}
// bytes [0, k) of a dword, k any integer
__device__ __forceinline__ uint32_t below(int32_t k) {
    return k >= 4 ? 0xffffffffu : k <= 0 ? 0u : ((1u << (8u * (uint32_t)k)) - 1u);
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
    uint32_t st3 = INGOT_CSUM_NONE, st4 = INGOT_CSUM_NONE, sum3 = 0, seg = 0, nch = 0;
    uint32_t pseudo = 0;          // the pseudo-header's words, big-endian, added
    uint8_t* A = nullptr;         // the segment's first byte
    uint8_t* P3 = nullptr;        // the IPv4 header, when its sum is wanted
    uint32_t foff = 0, fhi = 0, flo = 0;  // the L4 field: offset in the segment, its bytes
    bool udp = false;
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
            const uint8_t* H = F + l3_off;
            const uint32_t min4 = l4_kind == INGOT_L4_TCP ? 20u : 8u;
            const bool geo4 = (a.what & INGOT_CSUM_L4) && l4_kind >= INGOT_L4_TCP &&
                              l4_kind <= INGOT_L4_ICMPV6 && l3_off + fixed <= l4_off &&
                              l4_off + min4 <= payload_off && payload_off <= L;
            uint32_t end = 0;
            bool frag = false;
            if (v4) {
                const uint32_t w0 = ld32(H), w1 = ld32(H + 4), w2 = ld32(H + 8), w3 = ld32(H + 12),
                               w4 = ld32(H + 16);
                const uint32_t hl = max(20u, (w0 & 0xfu) * 4u);
                if ((a.what & INGOT_CSUM_L3) && l3_off + hl <= L) {
                    uint32_t s = be_words(w0) + be_words(w1) + be_words(w2) + be_words(w3) +
                                 be_words(w4);
                    for (uint32_t k = 20; k < hl; k += 4) s += be_words(ld32(H + k));
                    const uint32_t field = be16_hi(w2);
                    sum3 = ~fold(s - field) & 0xffffu;
                    st3 = (a.fill || fold(s) == 0xffffu) ? INGOT_CSUM_OK : INGOT_CSUM_BAD;
                    P3 = F + l3_off;
                }
                end = l3_off + be16_hi(w0);
                frag = (be16_hi(w1) & 0x3fffu) != 0;  // MF or a fragment offset
                pseudo = be_words(w3) + be_words(w4) + ((w2 >> 8) & 0xffu);
            } else if (geo4) {
                const uint32_t w1 = ld32(H + 4);
                end = l3_off + 40u + be16_lo(w1);
#pragma unroll
                for (uint32_t k = 8; k < 40; k += 4) pseudo += be_words(ld32(H + k));
                pseudo += l4_proto;
                uint32_t pos = l3_off + 40u, h = (w1 >> 16) & 0xffu;
                for (uint32_t e = 0; e < n_v6ext && pos + 8u <= l4_off; ++e) {
                    const uint32_t b = ld32(F + pos);
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
            if (geo4) {
                if (end > L || end < payload_off) {
                    st4 = INGOT_CSUM_SHORT;
                } else if (frag) {
                    st4 = INGOT_CSUM_FRAGMENT;
                } else {
                    seg = end - l4_off;
                    A = F + l4_off;
                    nch = (((uint32_t)(uintptr_t)A & 15u) + seg + 15u) / 16u;
                    udp = l4_kind == INGOT_L4_UDP;
                    foff = l4_kind == INGOT_L4_TCP ? 16u : udp ? 6u : 2u;
                    fhi = gbl(A)[foff];
                    flo = gbl(A)[foff + 1];
                    pseudo = l4_kind == INGOT_L4_ICMPV4 ? 0u : pseudo + seg;
                    st4 = INGOT_CSUM_OK;  // decided in step 4
                }
            }
        }
    }

    // 2. chunk counts -> inclusive prefix over the wave, then over the group
    uint32_t P = nch;
#pragma unroll
    for (uint32_t o = 1; o < WAVE; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)P, o);
        if (lane >= o) P += y;
    }
    const uint32_t lo = (uint32_t)(uintptr_t)A & 15u;
    g.base[t] = (uint64_t)(uintptr_t)A - lo;
    g.pfx[t] = P;
    g.span[t] = lo | (seg << 4);
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

    // 3. the wave's chunks, 64 per step and UNROLL steps at a time (their loads
    //    are issued together): chunk k belongs to the first packet whose
    //    inclusive prefix exceeds k
    for (uint32_t k0 = wave * WAVE * UNROLL; k0 < total; k0 += W * WAVE * UNROLL) {
        uint32_t q[UNROLL], c[UNROLL];
        u32x4 v[UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) {
            const uint32_t k = k0 + u * WAVE + lane;
            const bool valid = k < total;
            uint32_t qq = 0;
#pragma unroll
            for (uint32_t step = NP / 2; step; step >>= 1)
                if (g.pfx[qq + step - 1] <= k) qq += step;
            qq = valid ? qq : 0u;
            q[u] = valid ? qq : 0xffffffffu;
            c[u] = k - (qq ? g.pfx[qq - 1] : 0u);
            v[u] = u32x4{0u, 0u, 0u, 0u};
            if (valid)
                v[u] = *(const __attribute__((address_space(1))) u32x4*)(uintptr_t)(
                    g.base[qq] + 16ull * c[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) {
            const bool valid = q[u] != 0xffffffffu;
            const uint32_t span = g.span[valid ? q[u] : 0u];
            // the segment's bytes inside this chunk: [t0, t1)
            const int32_t first = (int32_t)(span & 15u) - (int32_t)(16u * c[u]);
            const int32_t t0 = max(first, 0), t1 = min(first + (int32_t)(span >> 4), 16);
            u32x4 x = v[u];
            if (t0 != 0 || t1 != 16) {
                x.x &= below(t1) & ~below(t0);
                x.y &= below(t1 - 4) & ~below(t0 - 4);
                x.z &= below(t1 - 8) & ~below(t0 - 8);
                x.w &= below(t1 - 12) & ~below(t0 - 12);
            }
            uint32_t s = (x.x & 0xffffu) + (x.x >> 16) + (x.y & 0xffffu) + (x.y >> 16) +
                         (x.z & 0xffffu) + (x.z >> 16) + (x.w & 0xffffu) + (x.w >> 16);
            // segmented inclusive scan: equal keys are contiguous
#pragma unroll
            for (uint32_t o = 1; o < WAVE; o <<= 1) {
                const uint32_t ys = (uint32_t)__shfl_up((int)s, o);
                const uint32_t yq = (uint32_t)__shfl_up((int)q[u], o);
                if (lane >= o && yq == q[u]) s += ys;
            }
            const uint32_t next = (uint32_t)__shfl_down((int)q[u], 1);
            if (valid && (lane == WAVE - 1 || next != q[u])) atomicAdd(&g.acc[q[u]], s);
        }
    }
    __syncthreads();

    // 4. the owning lane: the field's own bytes out, fold, byte order, the
    //    pseudo-header; the record and, in fill mode, the field bytes
    uint32_t sum4 = 0;
    if (nch) {
        const uint32_t odd = (uint32_t)(uintptr_t)A & 1u;
        const uint32_t fp = (odd + foff) & 1u;  // parity of the field's first byte's address
        const uint32_t T = g.acc[t] - (fhi << (8u * fp)) - (flo << (8u * (fp ^ 1u)));
        const uint32_t f = fold(T);
        const uint32_t be = odd ? f : (((f & 0xffu) << 8) | (f >> 8));
        const uint32_t s0 = fold(be + pseudo);
        sum4 = ~s0 & 0xffffu;
        if (udp && sum4 == 0) sum4 = 0xffffu;
        const uint32_t field = (fhi << 8) | flo;
        if (a.fill) {
            gbl_mut(A)[foff] = (uint8_t)(sum4 >> 8);
            gbl_mut(A)[foff + 1] = (uint8_t)sum4;
        } else {
            st4 = (udp && field == 0) ? INGOT_CSUM_ZERO
                  : fold(s0 + field) == 0xffffu ? INGOT_CSUM_OK
                                                : INGOT_CSUM_BAD;
        }
    }
    if (a.fill && P3) {
        gbl_mut(P3)[10] = (uint8_t)(sum3 >> 8);
        gbl_mut(P3)[11] = (uint8_t)sum3;
    }
    if (live && a.out)
        *(__attribute__((address_space(1))) u32x2*)(a.out + i) =
            u32x2{st3 | (st4 << 8) | (sum3 << 16), sum4 | (seg << 16)};
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
// the definition).  k_csum's shape, with the segment a list of pieces.
//
// Lane j of wave w owns packet 64 w + j: it walks the packet's chunk lengths
// once for the logical length L (cut at 65,535) and the chunks that hold
// l3_off and l4_off, applies the one-chunk rule (a header is read from one
// chunk) and reads the header bytes as unaligned dwords from that chunk.  The
// segment [l4_off, end) is then cut into pieces, the part of each chunk
// inside it: (address of the first byte, bytes, lane class), the class being
// the parity of the address XOR the parity of the byte's offset from l4_off.
// The workgroup keeps a table of PIECES = 256 x 4 pieces in LDS and fills it
// in rounds: every round a packet adds up to PER_ROUND pieces to its own
// slots, continuing its walk from registers (chunk index, logical start), so
// any number of pieces per packet is summed and a packet of 1-4 pieces takes
// one round.  A scan of the slots' 16-B block counts makes the round's pieces
// one flat run of aligned blocks, which the waves take as k_csum does (binary
// search of the scan, the bytes outside the piece masked in its first and
// last block, a segmented wave scan keyed by the slot).  A packet has two
// accumulators in LDS, one per class, that persist over the rounds: words
// added as loaded, each below 2^31 for 65,535 bytes of 0xff.  At the end the
// owning lane takes the field's bytes out of the first piece's class, folds
// both, swaps the bytes of class 0 (address and offset parity agree, so the
// big-endian high byte sits in the low lane) and adds them.  No global
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
    uint32_t st3 = INGOT_CSUM_NONE, st4 = INGOT_CSUM_NONE, sum3 = 0, seg = 0;
    uint32_t pseudo = 0;
    uint8_t* A = nullptr;   // the segment's first byte
    uint8_t* P3 = nullptr;  // the IPv4 header, when its sum is wanted
    uint32_t foff = 0, fhi = 0, flo = 0;
    bool udp = false, summed = false;
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
                const uint8_t* H = a.arena + at3 + (l3_off - s3);
                const uint32_t e3 = s3 + n3;  // chunk k3 ends here
                const uint32_t min4 = l4_kind == INGOT_L4_TCP ? 20u : 8u;
                const bool geo4 = (a.what & INGOT_CSUM_L4) && l4_kind >= INGOT_L4_TCP &&
                                  l4_kind <= INGOT_L4_ICMPV6 && l3_off + fixed <= l4_off &&
                                  l4_off + min4 <= payload_off && payload_off <= L &&
                                  l4_off <= e3 &&                  // [l3_off, l4_off) in one chunk
                                  n4 && payload_off <= s4 + n4;    // [l4_off, payload_off) too
                uint32_t end = 0;
                bool frag = false;
                if (v4) {
                    const uint32_t w0 = ld32(H), w1 = ld32(H + 4), w2 = ld32(H + 8),
                                   w3 = ld32(H + 12), w4 = ld32(H + 16);
                    const uint32_t hl = max(20u, (w0 & 0xfu) * 4u);
                    if ((a.what & INGOT_CSUM_L3) && l3_off + hl <= e3) {
                        uint32_t s = be_words(w0) + be_words(w1) + be_words(w2) + be_words(w3) +
                                     be_words(w4);
                        for (uint32_t k = 20; k < hl; k += 4) s += be_words(ld32(H + k));
                        const uint32_t field = be16_hi(w2);
                        sum3 = ~fold(s - field) & 0xffffu;
                        st3 = (a.fill || fold(s) == 0xffffu) ? INGOT_CSUM_OK : INGOT_CSUM_BAD;
                        P3 = const_cast<uint8_t*>(H);
                    }
                    end = l3_off + be16_hi(w0);
                    frag = (be16_hi(w1) & 0x3fffu) != 0;
                    pseudo = be_words(w3) + be_words(w4) + ((w2 >> 8) & 0xffu);
                } else if (geo4) {
                    const uint32_t w1 = ld32(H + 4);
                    end = l3_off + 40u + be16_lo(w1);
#pragma unroll
                    for (uint32_t k = 8; k < 40; k += 4) pseudo += be_words(ld32(H + k));
                    pseudo += l4_proto;
                    // the extension headers lie in chunk k3 with the fixed header (geo4)
                    uint32_t p = 40u, h = (w1 >> 16) & 0xffu;
                    for (uint32_t e = 0; e < n_v6ext && l3_off + p + 8u <= l4_off; ++e) {
                        const uint32_t b = ld32(H + p);
                        if (h == 44u) {
                            const uint32_t fo = be16_hi(b);
                            frag = frag || (fo & 0xfff9u) != 0;
                            p += 8u;
                        } else {
                            p += 8u + ((b >> 8) & 0xffu) * 8u;
                        }
                        h = b & 0xffu;
                    }
                }
                if (geo4) {
                    if (end > L || end < payload_off) {
                        st4 = INGOT_CSUM_SHORT;
                    } else if (frag) {
                        st4 = INGOT_CSUM_FRAGMENT;
                    } else {
                        seg = end - l4_off;
                        cat = k4 == k3 ? at3 : gbl(a.seg_off)[k4];
                        ck = k4, cstart = s4, clen = n4;
                        pos = l4 = l4_off, wend = end;
                        A = a.arena + cat + (l4_off - s4);
                        udp = l4_kind == INGOT_L4_UDP;
                        foff = l4_kind == INGOT_L4_TCP ? 16u : udp ? 6u : 2u;
                        fhi = gbl(A)[foff];
                        flo = gbl(A)[foff + 1];
                        pseudo = l4_kind == INGOT_L4_ICMPV4 ? 0u : pseudo + seg;
                        st4 = INGOT_CSUM_OK;  // decided in step 4
                        summed = true;
                    }
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
            const uint64_t p = (uint64_t)(uintptr_t)a.arena + cat + (pos - cstart);
            const uint32_t lo = (uint32_t)p & 15u, cls = ((uint32_t)p ^ (pos - l4)) & 1u;
            const uint32_t nblk = (lo + nb + 15u) / 16u, s = PER_ROUND * t + made;
            g.base[s] = p - lo;
            g.span[s] = lo | (nb << 4) | (cls << 20);
            g.pfx[s] = nblk;
            mine += nblk;
            pos += nb;
            ++made;
        }
        for (uint32_t j = made; j < PER_ROUND; ++j) g.pfx[PER_ROUND * t + j] = 0;
        uint32_t P = mine;
#pragma unroll
        for (uint32_t o = 1; o < WAVE; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)P, o);
            if (lane >= o) P += y;
        }
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

        // 3. the wave's blocks, as in k_csum: block k belongs to the first slot
        //    whose inclusive prefix exceeds k (a slot without a piece has none)
        for (uint32_t k0 = wave * WAVE * UNROLL; k0 < total; k0 += W * WAVE * UNROLL) {
            uint32_t q[UNROLL], c[UNROLL];
            u32x4 v[UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < UNROLL; ++u) {
                const uint32_t k = k0 + u * WAVE + lane;
                const bool valid = k < total;
                uint32_t qq = 0;
#pragma unroll
                for (uint32_t step = PIECES / 2; step; step >>= 1)
                    if (g.pfx[qq + step - 1] <= k) qq += step;
                qq = valid ? qq : 0u;
                q[u] = valid ? qq : 0xffffffffu;
                c[u] = k - (qq ? g.pfx[qq - 1] : 0u);
                v[u] = u32x4{0u, 0u, 0u, 0u};
                if (valid)
                    v[u] = *(const __attribute__((address_space(1))) u32x4*)(uintptr_t)(
                        g.base[qq] + 16ull * c[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < UNROLL; ++u) {
                const bool valid = q[u] != 0xffffffffu;
                const uint32_t span = g.span[valid ? q[u] : 0u];
                const int32_t first = (int32_t)(span & 15u) - (int32_t)(16u * c[u]);
                const int32_t t0 = max(first, 0),
                              t1 = min(first + (int32_t)((span >> 4) & 0xffffu), 16);
                u32x4 x = v[u];
                if (t0 != 0 || t1 != 16) {
                    x.x &= below(t1) & ~below(t0);
                    x.y &= below(t1 - 4) & ~below(t0 - 4);
                    x.z &= below(t1 - 8) & ~below(t0 - 8);
                    x.w &= below(t1 - 12) & ~below(t0 - 12);
                }
                uint32_t s = (x.x & 0xffffu) + (x.x >> 16) + (x.y & 0xffffu) + (x.y >> 16) +
                             (x.z & 0xffffu) + (x.z >> 16) + (x.w & 0xffffu) + (x.w >> 16);
#pragma unroll
                for (uint32_t o = 1; o < WAVE; o <<= 1) {
                    const uint32_t ys = (uint32_t)__shfl_up((int)s, o);
                    const uint32_t yq = (uint32_t)__shfl_up((int)q[u], o);
                    if (lane >= o && yq == q[u]) s += ys;
                }
                const uint32_t next = (uint32_t)__shfl_down((int)q[u], 1);
                if (valid && (lane == WAVE - 1 || next != q[u]))
                    atomicAdd(&g.acc[(span >> 20) & 1u][q[u] / PER_ROUND], s);
            }
        }
        __syncthreads();  // the accumulators are whole; the table may be refilled
        if (!more) break;
    }

    // 4. the owning lane: the field's own bytes out of the first piece's class,
    //    fold both classes, byte order, the pseudo-header; the row and, in fill
    //    mode, the field bytes
    uint32_t sum4 = 0;
    if (summed) {
        const uint32_t odd = (uint32_t)(uintptr_t)A & 1u;  // the first piece's class; foff is even
        uint32_t a0 = g.acc[0][t], a1 = g.acc[1][t];
        const uint32_t own = (fhi << (8u * odd)) + (flo << (8u * (odd ^ 1u)));
        if (odd) a1 -= own; else a0 -= own;
        const uint32_t f0 = fold(a0), f1 = fold(a1);
        const uint32_t be = (((f0 & 0xffu) << 8) | (f0 >> 8)) + f1;
        const uint32_t s0 = fold(be + pseudo);
        sum4 = ~s0 & 0xffffu;
        if (udp && sum4 == 0) sum4 = 0xffffu;
        const uint32_t field = (fhi << 8) | flo;
        if (a.fill) {
            gbl_mut(A)[foff] = (uint8_t)(sum4 >> 8);
            gbl_mut(A)[foff + 1] = (uint8_t)sum4;
        } else {
            st4 = (udp && field == 0) ? INGOT_CSUM_ZERO
                  : fold(s0 + field) == 0xffffu ? INGOT_CSUM_OK
                                                : INGOT_CSUM_BAD;
        }
    }
    if (a.fill && P3) {
        gbl_mut(P3)[10] = (uint8_t)(sum3 >> 8);
        gbl_mut(P3)[11] = (uint8_t)sum3;
    }
    if (live && a.out)
        *(__attribute__((address_space(1))) u32x2*)(a.out + i) =
            u32x2{st3 | (st4 << 8) | (sum3 << 16), sum4 | (seg << 16)};
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
