// flowtable_selftest.cpp — the host side of the flow table as a stand-alone
// program, for a sanitizer run of ingot_amd/csrc/flowtable.cpp without HIP,
// Python or a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/flowtable_selftest.cpp -o tools/bin/flowtable_selftest && tools/bin/flowtable_selftest
//
// It runs the cases of tests/test_flow_table_host.py that walk the buffer's
// edges: a probe chain that wraps from the last slot to the first, the
// half-full limit, the MAX_PROBE limit, duplicates, a 2^16-key table, and the
// refused arguments.  Prints "flowtable selftest: OK" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ingot_amd/csrc/flowtable.cpp"

#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #x);      \
            return 1;                                             \
        }                                                         \
    } while (0)

static ingot_flow_key key4(uint32_t src, uint32_t dst, uint32_t ports, uint32_t proto = 17) {
    ingot_flow_key k{};
    k.w[0] = src;
    k.w[1] = dst;
    k.w[2] = ports;
    k.w[9] = (INGOT_L3_IPV4 << 8) | proto;
    return k;
}

// `count` keys whose home is slot `home` of a `slots`-slot table
static std::vector<ingot_flow_key> with_home(uint32_t slots, uint32_t home, uint32_t count) {
    std::vector<ingot_flow_key> out;
    for (uint32_t p = 0; out.size() < count; ++p) {
        const ingot_flow_key k = key4(0x0a000001u, 0x0a000002u, p);
        if ((ingot_gpu_flow_key_hash(&k) & (slots - 1u)) == home) out.push_back(k);
    }
    return out;
}

int main() {
    // exactly table_bytes on the heap: the sanitizer sees any byte past it
    {  // a chain from the last slot wraps to the first
        const uint32_t slots = 16;
        const size_t nb = ingot_gpu_flow_table_bytes(slots);
        CHECK(nb == 64u * 17u);
        std::vector<uint8_t> t(nb);
        const auto k = with_home(slots, slots - 1u, 9);
        std::vector<uint32_t> rows = {100, 101, 102, 103, 104, 105, 106, 107};
        CHECK(ingot_gpu_flow_table_build(k.data(), rows.data(), 8, slots, t.data(), nb) == 0);
        for (uint32_t i = 0; i < 8; ++i)
            CHECK(ingot_gpu_flow_table_find(t.data(), nb, &k[i]) == 100u + i);
        CHECK(ingot_gpu_flow_table_find(t.data(), nb, &k[8]) == INGOT_ROW_NONE);
        // half full: one more is ERANGE and changes nothing
        const std::vector<uint8_t> before = t;
        CHECK(ingot_gpu_flow_table_insert(t.data(), nb, &k[8], 1) == INGOT_GPU_ERANGE);
        CHECK(t == before);
        // a duplicate replaces its row on the full table
        CHECK(ingot_gpu_flow_table_insert(t.data(), nb, &k[3], 55) == 0);
        CHECK(ingot_gpu_flow_table_find(t.data(), nb, &k[3]) == 55u);
    }
    {  // MAX_PROBE keys with one home near the end of the table, one more is ERANGE
        const uint32_t slots = 1024;
        const size_t nb = ingot_gpu_flow_table_bytes(slots);
        std::vector<uint8_t> t(nb);
        const auto k = with_home(slots, slots - 3u, INGOT_FLOW_TABLE_MAX_PROBE + 1u);
        std::vector<uint32_t> rows(k.size());
        for (size_t i = 0; i < rows.size(); ++i) rows[i] = (uint32_t)i;
        CHECK(ingot_gpu_flow_table_build(k.data(), rows.data(), INGOT_FLOW_TABLE_MAX_PROBE, slots,
                                         t.data(), nb) == 0);
        const std::vector<uint8_t> before = t;
        CHECK(ingot_gpu_flow_table_insert(t.data(), nb, &k.back(), 7) == INGOT_GPU_ERANGE);
        CHECK(t == before);
        for (uint32_t i = 0; i < INGOT_FLOW_TABLE_MAX_PROBE; ++i)
            CHECK(ingot_gpu_flow_table_find(t.data(), nb, &k[i]) == i);
        CHECK(ingot_gpu_flow_table_find(t.data(), nb, &k.back()) == INGOT_ROW_NONE);
        CHECK(ingot_gpu_flow_table_build(k.data(), rows.data(), (uint32_t)k.size(), slots, t.data(),
                                         nb) == INGOT_GPU_ERANGE);
    }
    {  // 2^16 keys in 2^17 slots, then as many absent ones
        const uint32_t n = 1u << 16, slots = 1u << 17;
        const size_t nb = ingot_gpu_flow_table_bytes(slots);
        std::vector<uint8_t> t(nb);
        std::vector<ingot_flow_key> k(2u * n);
        std::vector<uint32_t> rows(n);
        uint32_t x = 12345u;
        for (uint32_t i = 0; i < 2u * n; ++i) {
            for (uint32_t w = 0; w < 9; ++w) k[i].w[w] = x = x * 1664525u + 1013904223u;
            k[i].w[0] = i;  // distinct
            k[i].w[9] = ((i & 1u ? INGOT_L3_IPV6 : INGOT_L3_IPV4) << 8) | (x >> 24);
        }
        for (uint32_t i = 0; i < n; ++i) rows[i] = i ^ 0x5a5au;
        CHECK(ingot_gpu_flow_table_build(k.data(), rows.data(), n, slots, t.data(), nb) == 0);
        for (uint32_t i = 0; i < n; ++i)
            CHECK(ingot_gpu_flow_table_find(t.data(), nb, &k[i]) == rows[i]);
        for (uint32_t i = n; i < 2u * n; ++i)
            CHECK(ingot_gpu_flow_table_find(t.data(), nb, &k[i]) == INGOT_ROW_NONE);
    }
    {  // refused arguments touch nothing
        const size_t nb = ingot_gpu_flow_table_bytes(16);
        std::vector<uint8_t> t(nb), raw(nb, 0xa5);
        ingot_flow_key k = key4(1, 2, 3);
        const uint32_t row = 5, none = INGOT_ROW_NONE;
        CHECK(ingot_gpu_flow_table_bytes(0) == 0 && ingot_gpu_flow_table_bytes(24) == 0);
        CHECK(ingot_gpu_flow_table_bytes(0xffffffffu) == 0);
        CHECK(ingot_gpu_flow_table_build(&k, &row, 1, 16, t.data(), nb - 1) == INGOT_GPU_EINVAL);
        CHECK(ingot_gpu_flow_table_build(&k, &none, 1, 16, t.data(), nb) == INGOT_GPU_EINVAL);
        CHECK(ingot_gpu_flow_table_build(&k, &row, 1, 16, nullptr, nb) == INGOT_GPU_EINVAL);
        CHECK(ingot_gpu_flow_table_insert(raw.data(), nb, &k, 1) == INGOT_GPU_EINVAL);
        CHECK(ingot_gpu_flow_table_find(raw.data(), nb, &k) == INGOT_ROW_NONE);
        CHECK(ingot_gpu_flow_table_build(&k, &row, 1, 16, t.data(), nb) == 0);
        k.w[9] |= 1u << 16;
        CHECK(ingot_gpu_flow_table_insert(t.data(), nb, &k, 1) == INGOT_GPU_EINVAL);
        CHECK(ingot_gpu_flow_table_find(t.data(), nb, &k) == INGOT_ROW_NONE);
        CHECK(ingot_gpu_flow_key_hash(nullptr) == 0);
    }
    std::printf("flowtable selftest: OK\n");
    return 0;
}
