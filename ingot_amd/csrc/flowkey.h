// flowkey.h — the exact-match flow table's hash and slot layout, shared by
// the host side (flowtable.cpp) and a device lookup to come.  Compiles
// for host and device alike; on the host path it includes no HIP header, so
// flowtable.cpp builds with a plain C++ compiler too.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define INGOT_FK_HD __host__ __device__ inline
#else
#define INGOT_FK_HD inline
#endif

namespace ingot_gpu {

// The table: a 64-B header, then `slots` 64-B slots.
//   header dwords: 0 magic, 1 slots, 2 count, 3..15 zero;
//   slot dwords:   0..9 the key words, 10 the row, 11..15 zero.
// An empty slot is all zero: w[9] == 0 belongs to no key (its l3_kind is 0).
constexpr uint32_t FLOW_TABLE_MAGIC = 0x74667569u;  // "iuft" in memory
constexpr uint32_t FLOW_SLOT_BYTES = 64u;
constexpr uint32_t FLOW_SLOT_DW = FLOW_SLOT_BYTES / 4u;
constexpr uint32_t FLOW_KEY_WORDS = 10u;
constexpr uint32_t FLOW_SLOT_ROW = 10u;  // the row's dword in a slot

// The hash of the ten key words: a multiply-rotate mix per word and a final
// avalanche (the MurmurHash3 x86_32 round and finaliser, a public-domain
// construction), six integer operations per word.  Not Toeplitz: it has to
// spread keys that differ in one low bit over the table's low slot bits.
INGOT_FK_HD uint32_t flow_key_mix(const uint32_t* w) {
    uint32_t h = 0x9747b28cu;
    for (uint32_t k = 0; k < FLOW_KEY_WORDS; ++k) {
        uint32_t x = w[k] * 0xcc9e2d51u;
        x = (x << 15) | (x >> 17);
        x *= 0x1b873593u;
        h ^= x;
        h = (h << 13) | (h >> 19);
        h = h * 5u + 0xe6546b64u;
    }
    h ^= 4u * FLOW_KEY_WORDS;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// slots from the buffer size: 64 * (2^k + 1) with 2^k in [min, max], else 0.
INGOT_FK_HD uint32_t flow_table_slots(uint64_t table_bytes, uint32_t min_slots,
                                      uint32_t max_slots) {
    if (table_bytes % FLOW_SLOT_BYTES) return 0u;
    const uint64_t s = table_bytes / FLOW_SLOT_BYTES;
    if (s < 2u) return 0u;
    const uint64_t slots = s - 1u;
    if (slots < min_slots || slots > max_slots || (slots & (slots - 1u))) return 0u;
    return (uint32_t)slots;
}

}  // namespace ingot_gpu
