// emit_common.h — device helpers shared by the emit kernels (emit.hip: k_emit;
// emit_read.hip: k_emit_read): the funnel shift and its DPP neighbour, the
// predicated edge store, the header / byte masks, the setters' values and the
// 16-bit word sums of the fused checksums.  One copy of each.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ingot_gpu.h"
#include "kernels.h"

namespace ingot_gpu {
namespace {

constexpr uint32_t WAVE = 64;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* gbl(const T* p) {
    return (const __attribute__((address_space(1))) T*)p;
}
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T* gbl_mut(T* p) {
    return (__attribute__((address_space(1))) T*)p;
}

// The 16 bytes at byte s (0..15, per lane) of the 32-B pair a ++ b: rotate
// by whole dwords in two select stages (2, then 1), then v_alignbyte.
__device__ __forceinline__ u32x4 funnel(const u32x4& a, const u32x4& b, uint32_t s) {
    const bool r2 = s & 8u, r1 = s & 4u;
    const uint32_t c0 = r2 ? a.z : a.x, c1 = r2 ? a.w : a.y, c2 = r2 ? b.x : a.z,
                   c3 = r2 ? b.y : a.w, c4 = r2 ? b.z : b.x, c5 = r2 ? b.w : b.y;
    const uint32_t d0 = r1 ? c1 : c0, d1 = r1 ? c2 : c1, d2 = r1 ? c3 : c2, d3 = r1 ? c4 : c3,
                   d4 = r1 ? c5 : c4;
    const uint32_t sh = s & 3u;
    return u32x4{__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                 __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh)};
}

// The value of the next lane (lane 63: 0): DPP wave_shl:1, no LDS traffic.
__device__ __forceinline__ uint32_t from_next_lane(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x130, 0xf, 0xf, true);
}

__device__ __forceinline__ uint32_t head_mask(int32_t hc, uint32_t d) {
    // bytes [4d, 4d+4) of a chunk whose first hc bytes are header bytes
    const int32_t k = hc - (int32_t)(4u * d);
    return k >= 4 ? 0xffffffffu : k <= 0 ? 0u : ((1u << (8u * (uint32_t)k)) - 1u);
}

__device__ __forceinline__ uint32_t set_value(const EmitSet& e, uint64_t i, uint32_t total) {
    switch (e.source) {
    case INGOT_EMIT_LENGTH: return total - e.at + (uint32_t)e.add;
    case INGOT_EMIT_U16: return (uint32_t)gbl((const uint16_t*)e.values)[i] + (uint32_t)e.add;
    case INGOT_EMIT_U32: return gbl((const uint32_t*)e.values)[i] + (uint32_t)e.add;
    default: return (uint32_t)e.add;
    }
}

__host__ __device__ constexpr uint32_t region_bytes(uint32_t H) { return (H + 15u + 15u) / 16u * 16u; }

__device__ __forceinline__ uint32_t dword_at(const u32x4& v, uint32_t d) {
    return d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w;
}

// Bytes [t0, t1) of the 16-B chunk v at p (16-B aligned; neighbouring packets
// own the rest).  An edge chunk is cut on one side: a packet's first chunk
// keeps [t0, 16), its last [0, t1).  The whole dwords go as predicated dword
// stores at constant offsets, the one cut dword as a byte / short piece at
// p + 4 * (its index); a chunk cut on both sides (a packet shorter than a
// chunk) takes the byte loop.
__device__ __forceinline__ void store_edge(uint8_t* p, const u32x4& v, int32_t t0, int32_t t1) {
    auto* g32 = (__attribute__((address_space(1))) uint32_t*)p;
    if (t0 >= t1) return;
    if (t0 > 0 && t1 < 16) {
        for (int32_t t = t0; t < t1; ++t)
            gbl_mut(p)[t] = (uint8_t)(dword_at(v, (uint32_t)t >> 2) >> (8 * (t & 3)));
        return;
    }
    // whole dwords inside [t0, t1)
    if (0 >= t0 && 4 <= t1) g32[0] = v.x;
    if (4 >= t0 && 8 <= t1) g32[1] = v.y;
    if (8 >= t0 && 12 <= t1) g32[2] = v.z;
    if (12 >= t0 && 16 <= t1) g32[3] = v.w;
    // the cut dword: bytes [t0 & 3, 4) of dword t0 >> 2, or [0, t1 & 3) of t1 >> 2
    const bool head = t0 > 0;
    const uint32_t cut = head ? (uint32_t)t0 & 3u : (uint32_t)t1 & 3u;
    if (cut == 0) return;
    const uint32_t d = head ? (uint32_t)t0 >> 2 : (uint32_t)t1 >> 2;
    const uint32_t w = dword_at(v, d);
    auto* q8 = gbl_mut(p + 4 * d);
    auto* q16 = (__attribute__((address_space(1))) uint16_t*)(p + 4 * d);
    if (head) {  // bytes cut..3
        if (cut == 1) q8[1] = (uint8_t)(w >> 8);
        if (cut <= 2) q16[1] = (uint16_t)(w >> 16);
        if (cut == 3) q8[3] = (uint8_t)(w >> 24);
    } else {     // bytes 0..cut-1
        if (cut >= 2) q16[0] = (uint16_t)w;
        if (cut != 2) q8[cut == 1 ? 0 : 2] = (uint8_t)(cut == 1 ? w : w >> 16);
    }
}

// --- ingot_gpu_emit_packets_csum (the SUMS instantiation) -------------------
// Sums are kept as the 16-bit words of aligned dwords added as loaded (the
// sum is byte-order independent); a segment's big-endian sum is the folded
// value, byte-swapped unless the segment starts at an odd address.
__device__ __forceinline__ uint32_t fold16(uint32_t x) {
    x = (x & 0xffffu) + (x >> 16);
    return (x & 0xffffu) + (x >> 16);
}
__device__ __forceinline__ uint32_t swap16(uint32_t x) { return ((x & 0xffu) << 8) | (x >> 8); }
__device__ __forceinline__ uint32_t below(int32_t k) {  // bytes [0, k) of a dword, k any integer
    return k >= 4 ? 0xffffffffu : k <= 0 ? 0u : ((1u << (8u * (uint32_t)k)) - 1u);
}
// Bytes [b0, b1) of a 16-B chunk: its 16-bit words as loaded, added.
__device__ __forceinline__ uint32_t chunk_words(const u32x4& v, int32_t b0, int32_t b1) {
    const uint32_t x = v.x & below(b1) & ~below(b0), y = v.y & below(b1 - 4) & ~below(b0 - 4),
                   z = v.z & below(b1 - 8) & ~below(b0 - 8), w = v.w & below(b1 - 12) & ~below(b0 - 12);
    return (x & 0xffffu) + (x >> 16) + (y & 0xffffu) + (y >> 16) + (z & 0xffffu) + (z >> 16) +
           (w & 0xffffu) + (w >> 16);
}
// The same over bytes [b0, b1) of a packet's region (LDS, 16-B aligned).
__device__ __forceinline__ uint32_t region_words(const uint8_t* R, uint32_t b0, uint32_t b1) {
    uint32_t s = 0;
    for (uint32_t d = b0 >> 2; 4u * d < b1; ++d) {
        const int32_t o = (int32_t)(4u * d);
        const uint32_t x = reinterpret_cast<const uint32_t*>(R)[d] & below((int32_t)b1 - o) &
                           ~below((int32_t)b0 - o);
        s += (x & 0xffffu) + (x >> 16);
    }
    return s;
}
// Byte `pos` of a chunk := val, when the chunk holds it (0 <= pos < 16).
__device__ __forceinline__ void put_byte(u32x4& v, int32_t pos, uint32_t val) {
    if (pos < 0 || pos > 15) return;
    const uint32_t d = (uint32_t)pos >> 2, sh = 8u * ((uint32_t)pos & 3u);
    const uint32_t m = 0xffu << sh, b = val << sh;
    v.x = d == 0 ? (v.x & ~m) | b : v.x;
    v.y = d == 1 ? (v.y & ~m) | b : v.y;
    v.z = d == 2 ? (v.z & ~m) | b : v.z;
    v.w = d == 3 ? (v.w & ~m) | b : v.w;
}

}  // namespace
}  // namespace ingot_gpu
