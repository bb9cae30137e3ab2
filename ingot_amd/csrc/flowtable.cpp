// flowtable.cpp — the host side of the exact-match flow table
// (include/ingot_gpu.h: ingot_gpu_flow_table_*, ingot_gpu_flow_key_hash):
// build, insert and find over a caller-owned buffer, with the hash and slot
// layout a device lookup will read (flowkey.h).  No context, no GPU, no HIP
// header: the file also builds with a plain C++ compiler (the sanitizer run
// in DESIGN.md §4.14 does).
#include <string.h>

#include "../../include/ingot_gpu.h"
#include "flowkey.h"

namespace {

using namespace ingot_gpu;

uint32_t slots_of(size_t table_bytes) {
    return flow_table_slots(table_bytes, INGOT_FLOW_TABLE_MIN_SLOTS, INGOT_FLOW_TABLE_MAX_SLOTS);
}

// A key a packet can have: l3_kind 1 or 2, the reserved upper bits zero.
bool key_ok(const ingot_flow_key* key) {
    const uint32_t kind = key->w[9] >> 8;
    return kind == INGOT_L3_IPV4 || kind == INGOT_L3_IPV6;
}

// The header of a buffer _build made for exactly table_bytes.
bool header_ok(const uint32_t* t, uint32_t slots) {
    return slots && t[0] == FLOW_TABLE_MAGIC && t[1] == slots && t[2] <= slots / 2u;
}

bool same_key(const uint32_t* slot, const ingot_flow_key* key) {
    return memcmp(slot, key->w, sizeof(key->w)) == 0;
}

int insert(uint32_t* t, uint32_t slots, const ingot_flow_key* key, uint32_t row) {
    const uint32_t mask = slots - 1u;
    const uint32_t home = flow_key_mix(key->w);
    for (uint32_t p = 0; p < INGOT_FLOW_TABLE_MAX_PROBE && p < slots; ++p) {
        uint32_t* s = t + FLOW_SLOT_DW * (1u + (size_t)((home + p) & mask));
        if (s[FLOW_KEY_WORDS - 1u] == 0u) {
            if (t[2] + 1u > slots / 2u) return INGOT_GPU_ERANGE;
            memcpy(s, key->w, sizeof(key->w));
            s[FLOW_SLOT_ROW] = row;
            ++t[2];
            return INGOT_GPU_SUCCESS;
        }
        if (same_key(s, key)) {
            s[FLOW_SLOT_ROW] = row;  // the last one wins
            return INGOT_GPU_SUCCESS;
        }
    }
    return INGOT_GPU_ERANGE;
}

}  // namespace

extern "C" {

size_t ingot_gpu_flow_table_bytes(uint32_t slots) {
    const size_t bytes = (size_t)FLOW_SLOT_BYTES * ((size_t)slots + 1u);
    return slots_of(bytes) ? bytes : 0u;
}

uint32_t ingot_gpu_flow_key_hash(const ingot_flow_key* key) {
    return key ? flow_key_mix(key->w) : 0u;
}

int ingot_gpu_flow_table_build(const ingot_flow_key* keys, const uint32_t* rows, uint32_t n_keys,
                               uint32_t slots, void* table, size_t table_bytes) {
    if (!ingot_gpu_flow_table_bytes(slots) || table_bytes != ingot_gpu_flow_table_bytes(slots))
        return INGOT_GPU_EINVAL;
    if (!table || (n_keys && (!keys || !rows))) return INGOT_GPU_EINVAL;
    for (uint32_t i = 0; i < n_keys; ++i)
        if (!key_ok(&keys[i]) || rows[i] == INGOT_ROW_NONE) return INGOT_GPU_EINVAL;
    uint32_t* t = static_cast<uint32_t*>(table);
    memset(t, 0, table_bytes);
    t[0] = FLOW_TABLE_MAGIC;
    t[1] = slots;
    for (uint32_t i = 0; i < n_keys; ++i)
        if (int e = insert(t, slots, &keys[i], rows[i])) return e;
    return INGOT_GPU_SUCCESS;
}

int ingot_gpu_flow_table_insert(void* table, size_t table_bytes, const ingot_flow_key* key,
                                uint32_t row) {
    const uint32_t slots = slots_of(table_bytes);
    if (!slots || !table || !key) return INGOT_GPU_EINVAL;
    if (!key_ok(key) || row == INGOT_ROW_NONE) return INGOT_GPU_EINVAL;
    uint32_t* t = static_cast<uint32_t*>(table);
    if (!header_ok(t, slots)) return INGOT_GPU_EINVAL;
    return insert(t, slots, key, row);
}

uint32_t ingot_gpu_flow_table_find(const void* table, size_t table_bytes,
                                   const ingot_flow_key* key) {
    const uint32_t slots = slots_of(table_bytes);
    if (!slots || !table || !key || !key_ok(key)) return INGOT_ROW_NONE;
    const uint32_t* t = static_cast<const uint32_t*>(table);
    if (!header_ok(t, slots)) return INGOT_ROW_NONE;
    const uint32_t mask = slots - 1u;
    const uint32_t home = flow_key_mix(key->w);
    for (uint32_t p = 0; p < INGOT_FLOW_TABLE_MAX_PROBE && p < slots; ++p) {
        const uint32_t* s = t + FLOW_SLOT_DW * (1u + (size_t)((home + p) & mask));
        if (s[FLOW_KEY_WORDS - 1u] == 0u) break;
        if (same_key(s, key)) return s[FLOW_SLOT_ROW];
    }
    return INGOT_ROW_NONE;
}

}  // extern "C"
