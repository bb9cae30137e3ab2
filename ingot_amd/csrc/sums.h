// sums.h — device helpers of 16-bit-word sums, shared by the checksum kernels
// (csum.hip) and the emit kernels (emit_common.h): the address-space casts,
// the vector types, fold / swap / byte masks, a chunk's words, and the two
// wave scans.  One copy of each.
//
// Sums are kept as the 16-bit words of aligned dwords added as loaded (the
// ones'-complement sum is byte-order independent); a run's big-endian sum is
// the folded value, byte-swapped unless the run starts at an odd address.
#pragma once
#include <hip/hip_runtime.h>

namespace ingot_gpu {
namespace {

constexpr uint32_t WAVE = 64;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* gbl(const T* p) {
    return (const __attribute__((address_space(1))) T*)p;
}
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T* gbl_mut(T* p) {
    return (__attribute__((address_space(1))) T*)p;
}

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

// Inclusive prefix sum of x over the wave.
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t x, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < WAVE; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o);
        if (lane >= o) x += y;
    }
    return x;
}
// The same within runs of equal `owner` (the lanes of one owner are
// contiguous): an owner's last lane ends up with its lanes' sum.
__device__ __forceinline__ uint32_t owner_inclusive_sum(uint32_t x, uint32_t owner, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < WAVE; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o);
        const uint32_t yo = (uint32_t)__shfl_up((int)owner, o);
        if (lane >= o && yo == owner) x += y;
    }
    return x;
}

}  // namespace
}  // namespace ingot_gpu
