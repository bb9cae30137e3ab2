// example_nat_rewrite.cpp — a destination NAT from a host that binds only the
// C ABI: a ring of 128-B slots holding IPv4 UDP and TCP frames with valid
// checksums is rewritten in place (IPv4 destination, UDP / TCP destination
// port, hop limit - 1) and its IPv4 and L4 checksums are updated in the same
// launch (ingot_gpu_parse_modify_csum, RFC 1624) — what OPTE does per packet on
// the CPU after its own rewrites.  ingot_gpu_checksum_verify then reads every
// byte and must find no BAD sum.  Run on the GPU by tests/test_modify_csum.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "ingot_gpu.h"

static int fail(const char* what) {
    std::printf("FAIL %s\n", what);
    return 1;
}

// RFC 1071 over `n` bytes starting on a word boundary, added to `acc`.
static uint32_t add_words(uint32_t acc, const uint8_t* p, size_t n) {
    for (size_t k = 0; k + 1 < n; k += 2) acc += (uint32_t)p[k] << 8 | p[k + 1];
    if (n & 1) acc += (uint32_t)p[n - 1] << 8;
    return acc;
}
static uint16_t fold_not(uint32_t acc) {
    while (acc >> 16) acc = (acc & 0xffffu) + (acc >> 16);
    return (uint16_t)~acc;
}

int main() {
    const uint32_t slot = 128, n = 100003;  // the frame fills its slot; the last tile is partial
    const uint32_t ip_len = slot - 14;
    std::vector<uint8_t> ring((size_t)slot * n);
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t* f = ring.data() + (size_t)i * slot;
        const bool tcp = i % 3 == 1;
        for (uint32_t k = 0; k < slot; ++k) f[k] = (uint8_t)(i * 31u + k * 7u);  // payload
        std::memset(f, 0x02, 12);
        f[12] = 0x08;
        f[13] = 0x00;
        uint8_t* ip = f + 14;
        const uint8_t v4[20] = {0x45, 0, (uint8_t)(ip_len >> 8), (uint8_t)ip_len, (uint8_t)(i >> 8),
                                (uint8_t)i, 0x40, 0, 64, (uint8_t)(tcp ? 6 : 17), 0, 0,
                                192, 168, (uint8_t)(i >> 16), (uint8_t)i, 10, 1, 2, 3};
        std::memcpy(ip, v4, 20);
        const uint16_t hc = fold_not(add_words(0, ip, 20));
        ip[10] = (uint8_t)(hc >> 8);
        ip[11] = (uint8_t)hc;
        uint8_t* l4 = ip + 20;
        const uint32_t seg = ip_len - 20;
        const uint32_t at = tcp ? 16 : 6;
        if (tcp) {
            l4[12] = 0x50;  // data offset 5
            l4[13] = 0x18;
        } else {
            l4[4] = (uint8_t)(seg >> 8);
            l4[5] = (uint8_t)seg;
        }
        l4[at] = l4[at + 1] = 0;
        uint32_t acc = add_words(0, ip + 12, 8) + ip[9] + seg;  // the pseudo-header
        uint16_t c = fold_not(add_words(acc, l4, seg));
        if (!tcp && c == 0) c = 0xffff;
        l4[at] = (uint8_t)(c >> 8);
        l4[at + 1] = (uint8_t)c;
    }
    ingot_gpu_ctx* ctx = nullptr;
    if (ingot_gpu_ctx_create(0, &ctx)) return fail("ctx_create");
    uint8_t* d_ring = nullptr;
    ingot_rec* d_rec = nullptr;
    ingot_csum* d_sum = nullptr;
    if (hipMalloc(&d_ring, ring.size()) != hipSuccess ||
        hipMalloc(&d_rec, n * sizeof(ingot_rec)) != hipSuccess ||
        hipMalloc(&d_sum, n * sizeof(ingot_csum)) != hipSuccess)
        return fail("hipMalloc");
    if (hipMemcpy(d_ring, ring.data(), ring.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail("H2D");
    const uint32_t what = INGOT_CSUM_L3 | INGOT_CSUM_L4;
    std::vector<ingot_csum> sums(n);
    // the frames as built verify; then the NAT, and they still do
    const ingot_edit nat[4] = {{1, INGOT_F_V4_DESTINATION, INGOT_OP_SET, 0, 0xc6336407u},
                               {2, INGOT_F_UDP_DESTINATION, INGOT_OP_SET, 0, 8080},
                               {2, INGOT_F_TCP_DESTINATION, INGOT_OP_SET, 0, 8443},
                               {1, INGOT_F_V4_HOP_LIMIT, INGOT_OP_SUB, 0, 1}};
    uint32_t not_ok[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) {
            if (ingot_gpu_parse_strided(ctx, d_ring, slot, nullptr, n, INGOT_CHAIN_GENERIC_ULP,
                                        d_rec, nullptr))
                return fail("parse_strided");
        } else if (ingot_gpu_parse_modify_csum(ctx, d_ring, nullptr, nullptr, slot, n,
                                               INGOT_CHAIN_GENERIC_ULP, nat, 4, what, d_rec,
                                               nullptr)) {
            return fail("parse_modify_csum");
        }
        if (ingot_gpu_checksum_verify(ctx, d_ring, nullptr, nullptr, slot, n, d_rec, what, d_sum,
                                      nullptr))
            return fail("checksum_verify");
        if (hipMemcpy(sums.data(), d_sum, n * sizeof(ingot_csum), hipMemcpyDeviceToHost) !=
            hipSuccess)
            return fail("D2H");
        for (uint32_t i = 0; i < n; ++i)
            not_ok[pass] += sums[i].l3_state != INGOT_CSUM_OK || sums[i].l4_state != INGOT_CSUM_OK;
    }
    std::vector<uint8_t> got(ring.size());
    if (hipMemcpy(got.data(), d_ring, got.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return fail("D2H");
    uint32_t wrong = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* f = got.data() + (size_t)i * slot;
        const uint32_t port = (uint32_t)f[36] << 8 | f[37];
        wrong += std::memcmp(f + 30, "\xc6\x33\x64\x07", 4) != 0 || f[22] != 63 ||
                 port != (i % 3 == 1 ? 8443u : 8080u);
    }
    (void)hipFree(d_ring);
    (void)hipFree(d_rec);
    (void)hipFree(d_sum);
    ingot_gpu_ctx_destroy(ctx);
    std::printf("nat rewrite: %u frames, %u not OK before, %u not OK after, %u not rewritten\n", n,
                not_ok[0], not_ok[1], wrong);
    return not_ok[0] || not_ok[1] || wrong ? 1 : 0;
}
