// csum.hip — batched Internet checksums (ingot_gpu_checksum_verify / _fill).
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

}  // namespace ingot_gpu
