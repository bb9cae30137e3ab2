// emit_read_rows_selftest.cpp — the argument checks of
// ingot_gpu_emit_packets_read_rows as a stand-alone program, for a sanitizer
// run of that host code (ingot_amd/csrc/api.cpp and resolve.cpp) without Python
// or a GPU: every path taken here returns before any device work.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//       tools/emit_read_rows_selftest.cpp -Lingot_amd/lib -lingot_gpu
//       -Wl,-rpath,$PWD/ingot_amd/lib -o tools/bin/emit_read_rows_selftest
//   && tools/bin/emit_read_rows_selftest
//
// Both sources are compiled into the program (so their code carries the checks); the
// kernels' launchers come from the library and are never reached.  The set
// list, the header block and the sums live in heap blocks of exactly their
// size, so a read past any of them is seen.  The header's EINVAL list is walked
// in its order, each step reached with the earlier ones satisfied and carrying
// the fault of a later step, which must not be what decides.  Prints
// "emit_read_rows selftest: OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ingot_amd/csrc/api.cpp"
#include "../ingot_amd/csrc/resolve.cpp"

#define CHECK(x)                                             \
    do {                                                     \
        if (!(x)) {                                          \
            std::printf("FAIL line %d: %s\n", __LINE__, #x); \
            return 1;                                        \
        }                                                    \
    } while (0)

using Set = ingot_emit_set_rows;

static Set mk(uint16_t at, uint8_t field, uint8_t source, int32_t add, uint8_t by, uint32_t pitch,
              const void* values) {
    Set s{};
    s.at = at;
    s.field = field;
    s.source = source;
    s.add = add;
    s.by = by;
    s.pitch = pitch;
    s.d_values = values;
    return s;
}

// which device pointers are NULL
enum : unsigned { SRC = 1, SEG_OFF = 2, SEG_LEN = 4, PKT_SEG = 8, DST = 16, DST_OFF = 32 };

// the call over exact-size heap copies of hdr, sets and sums; n = 4 unless given
static int call(ingot_gpu_ctx* ctx, const std::vector<uint8_t>& hdr, const std::vector<Set>& sets,
                const std::vector<ingot_emit_sum>& sums, bool have_row, uint64_t n = 4,
                unsigned null = 0) {
    uint8_t* h = (uint8_t*)std::malloc(hdr.size() ? hdr.size() : 1);
    Set* s = (Set*)std::malloc(sets.empty() ? 1 : sets.size() * sizeof(Set));
    ingot_emit_sum* c =
        (ingot_emit_sum*)std::malloc(sums.empty() ? 1 : sums.size() * sizeof(ingot_emit_sum));
    if (!hdr.empty()) std::memcpy(h, hdr.data(), hdr.size());
    if (!sets.empty()) std::memcpy((void*)s, sets.data(), sets.size() * sizeof(Set));
    if (!sums.empty()) std::memcpy((void*)c, sums.data(), sums.size() * sizeof(ingot_emit_sum));
    // never dereferenced on the host: any non-NULL value stands for device memory
    auto dev = [&](unsigned bit) { return (null & bit) ? (uintptr_t)0 : (uintptr_t)0x1000; };
    const int r = ingot_gpu_emit_packets_read_rows(
        ctx, h, (uint32_t)hdr.size(), s, (uint32_t)sets.size(), c, (uint32_t)sums.size(),
        have_row ? (const uint32_t*)0x2000 : nullptr, 7, (const uint8_t*)dev(SRC),
        (const uint64_t*)dev(SEG_OFF), (const uint16_t*)dev(SEG_LEN),
        (const uint32_t*)dev(PKT_SEG), nullptr, nullptr, n, (uint8_t*)dev(DST),
        (const uint64_t*)dev(DST_OFF), nullptr, nullptr);
    std::free(h);
    std::free(s);
    std::free(c);
    return r;
}

int main() {
    // Ethernet / IPv6 / UDP / Geneve, 70 bytes
    std::vector<uint8_t> hdr(70, 0);
    hdr[12] = 0x86;
    hdr[13] = 0xdd;
    hdr[14] = 0x60;
    hdr[20] = 17;
    const void* T = (const void*)0x4000;
    const uint8_t B = INGOT_EMIT_BYTES, U16 = INGOT_EMIT_U16, U32 = INGOT_EMIT_U32,
                  VALUE = INGOT_EMIT_VALUE, LENGTH = INGOT_EMIT_LENGTH;
    const Set ok = mk(14, INGOT_FW_V6_DESTINATION, B, 0, INGOT_BY_ROW, 32, T);
    const Set unknown = mk(14, 48, VALUE, 0, 0, 0, nullptr);
    const std::vector<ingot_emit_sum> udp = {{54, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}}};
    const std::vector<ingot_emit_sum> odd = {{55, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}}};
    const unsigned ALL = SRC | SEG_OFF | SEG_LEN | PKT_SEG | DST | DST_OFF;
    ingot_gpu_ctx ctx;  // api.cpp's own struct: no device is opened
    ctx.lds_bytes = 160u * 1024u;

    // 1. ctx NULL (with every later fault present)
    CHECK(call(nullptr, std::vector<uint8_t>(257, 0), {unknown}, odd, false, 4, ALL) ==
          INGOT_GPU_EINVAL);
    // 2. emit_args: hdr_len, n_sets (each with a faulty set, faulty sums and NULL pointers)
    CHECK(call(&ctx, std::vector<uint8_t>(257, 0), {ok}, {}, true) == INGOT_GPU_EINVAL);
    CHECK(call(&ctx, hdr, std::vector<Set>(9, ok), {}, true) == INGOT_GPU_EINVAL);
    CHECK(call(&ctx, hdr, std::vector<Set>(9, unknown), odd, true, 0, ALL) == INGOT_GPU_EINVAL);
    // accepted: every kind of set, the largest list (8 wide sets = 32 pieces), n == 0
    CHECK(call(&ctx, hdr, {ok}, udp, true, 0, ALL) == INGOT_GPU_SUCCESS);
    CHECK(call(&ctx, hdr, std::vector<Set>(8, ok), udp, true, 0) == INGOT_GPU_SUCCESS);
    CHECK(call(&ctx, hdr,
               {mk(14, INGOT_F_V6_PAYLOAD_LEN, LENGTH, -40, 0, 0, nullptr),
                mk(54, INGOT_F_UDP_LENGTH, LENGTH, 0, 0, 0, nullptr),
                mk(0, INGOT_FW_ETH_DESTINATION, B, 0, 0, 0, (const void*)0x4001),
                mk(0, INGOT_FW_ETH_SOURCE, B, 0, INGOT_BY_ROW, 8, T),
                mk(14, INGOT_FW_V6_SOURCE, B, 0, 0, 16, T),
                mk(62, INGOT_F_GENEVE_VNI, U32, 5, INGOT_BY_ROW, 32, T),
                mk(54, INGOT_F_UDP_SOURCE, U16, -1, 0, 0, T),
                mk(62, INGOT_F_GENEVE_VNI, VALUE, 77, 0, 0, nullptr)},
               udp, true, 0) == INGOT_GPU_SUCCESS);
    // hdr_len == 0, n_sets == 0 with a row array: the guarded pull-up
    CHECK(call(&ctx, {}, {}, {}, true, 0) == INGOT_GPU_SUCCESS);
    // fields that end exactly at the block's end
    CHECK(call(&ctx, hdr, {mk(70 - 40, INGOT_FW_V6_DESTINATION, B, 0, 0, 0, T)}, {}, false, 0) ==
          INGOT_GPU_SUCCESS);
    CHECK(call(&ctx, hdr, {mk(70 - 12, INGOT_FW_ETH_SOURCE, B, 0, 0, 0, T)}, {}, false, 0) ==
          INGOT_GPU_SUCCESS);
    // 2 (cont.): emit_rows_pieces, per set; the sums given are faulty too and n > 0
    // with NULL pointers, so only the set can be what is refused first
    const std::vector<Set> bad = {
        unknown,                                                  // unknown field
        mk(14, 68, B, 0, 0, 0, T),                                // past the wide fields
        mk(54, INGOT_F_UDP_SOURCE, 5, 0, 0, 0, T),                // unknown source
        mk(54, INGOT_F_UDP_SOURCE, U16, 0, 2, 0, T),              // unknown by
        mk(54, INGOT_F_UDP_SOURCE, B, 0, 0, 0, T),                // BYTES on a narrow field
        mk(14, INGOT_FW_V6_SOURCE, U32, 0, 0, 0, T),              // a wide field without BYTES
        mk(14, INGOT_FW_V6_SOURCE, VALUE, 0, 0, 0, nullptr),
        mk(54, INGOT_F_UDP_LENGTH, LENGTH, 0, INGOT_BY_ROW, 0, nullptr),
        mk(54, INGOT_F_UDP_LENGTH, LENGTH, 0, 0, 4, nullptr),
        mk(54, INGOT_F_UDP_SOURCE, VALUE, 0, 0, 0, T),
        mk(54, INGOT_F_UDP_SOURCE, U16, 0, 0, 0, nullptr),        // NULL table
        mk(14, INGOT_FW_V6_SOURCE, B, 1, 0, 0, T),                // BYTES with add
        mk(14, INGOT_FW_V6_SOURCE, B, 0, 0, 15, T),               // pitch below the width
        mk(0, INGOT_FW_ETH_SOURCE, B, 0, 0, 5, T),
        mk(54, INGOT_F_UDP_SOURCE, U16, 0, 0, 0, (const void*)0x4001),  // misaligned
        mk(62, INGOT_F_GENEVE_VNI, U32, 0, 0, 6, T),
        mk(70 - 39, INGOT_FW_V6_DESTINATION, B, 0, 0, 0, T),      // outside hdr
        mk(70 - 11, INGOT_FW_ETH_SOURCE, B, 0, 0, 0, T),
        mk(65535, INGOT_FW_V6_DESTINATION, B, 0, 0, 0, T),
        mk(65535, INGOT_F_GENEVE_VNI, VALUE, 0, 0, 0, nullptr),
        mk(69, INGOT_F_UDP_SOURCE, VALUE, 0, 0, 0, nullptr)};
    for (size_t k = 0; k < bad.size(); ++k) {
        CHECK(call(&ctx, hdr, {ok, bad[k]}, udp, true, 0) == INGOT_GPU_EINVAL);
        CHECK(call(&ctx, hdr, {bad[k]}, odd, true, 4, ALL) == INGOT_GPU_EINVAL);
    }
    Set pad = ok;
    pad._pad[2] = 1;
    CHECK(call(&ctx, hdr, {pad}, {}, true, 0) == INGOT_GPU_EINVAL);
    CHECK(call(&ctx, hdr, {ok}, {}, false, 0) == INGOT_GPU_EINVAL);  // BY_ROW without d_row
    // 2 (cont.): emit_sums, with the narrow sets' version rule; n == 0 and NULL
    // pointers do not excuse them
    CHECK(call(&ctx, hdr, {ok}, odd, true, 0, ALL) == INGOT_GPU_EINVAL);
    CHECK(call(&ctx, hdr, {ok}, {udp[0], udp[0]}, true, 0) == INGOT_GPU_EINVAL);
    CHECK(call(&ctx, hdr, {ok, mk(14, INGOT_F_V6_VERSION, VALUE, 6, 0, 0, nullptr)}, udp, true,
               0) == INGOT_GPU_EINVAL);
    CHECK(call(&ctx, hdr, {ok, mk(14, INGOT_F_V6_VERSION, VALUE, 6, 0, 0, nullptr)}, {}, true,
               0) == INGOT_GPU_SUCCESS);
    // 3. n == 0 succeeds whatever the device pointers are (and whatever the LDS is)
    ctx.lds_bytes = 1024;
    for (unsigned bit = 1; bit <= DST_OFF; bit <<= 1)
        CHECK(call(&ctx, hdr, {ok}, udp, true, 0, bit) == INGOT_GPU_SUCCESS);
    CHECK(call(&ctx, hdr, {ok}, udp, true, 0, ALL) == INGOT_GPU_SUCCESS);
    // 4. d_dst / d_dst_off NULL; 5. the chunk tables: each alone, with an LDS
    // that would not fit (6) behind them
    for (unsigned bit = 1; bit <= DST_OFF; bit <<= 1)
        CHECK(call(&ctx, hdr, {ok}, udp, true, 4, bit) == INGOT_GPU_EINVAL);
    CHECK(call(&ctx, hdr, {ok}, udp, true, 4, ALL) == INGOT_GPU_EINVAL);
    // 6. ERANGE from the LDS fit, before any device work, with and without sums
    CHECK(call(&ctx, hdr, {ok}, udp, true) == INGOT_GPU_ERANGE);
    CHECK(call(&ctx, hdr, {ok}, {}, true) == INGOT_GPU_ERANGE);
    CHECK(call(&ctx, {}, {}, {}, true) == INGOT_GPU_ERANGE);
    std::printf("emit_read_rows selftest: OK\n");
    return 0;
}
