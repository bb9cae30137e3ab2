// example_nat_table.cpp — a per-flow source NAT from a host that binds only the
// C ABI: ingot_gpu_flow_hist leaves every packet's flow bin on the device, and
// that array, as it is, selects the packet's row of a `bins`-row NAT table
// (ingot_gpu_parse_modify_rows, INGOT_BY_ROW): the IPv4 source and the UDP /
// TCP source port of each flow are rewritten to the flow's own translation and
// the IPv4 and L4 checksums are updated in the same launch.
// ingot_gpu_checksum_verify then reads every byte and must find every sum Ok.
// Run on the GPU by tests/test_modify_rows.py.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ingot_amd.hpp"

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

// one row of the host's NAT table, as the device reads it
struct NatRow {
    uint32_t address;  // host-endian: INGOT_EDIT_U32
    uint16_t port;     // host-endian: INGOT_EDIT_U16
    uint16_t _pad;
};

int main() {
    const uint32_t slot = 128, n = 20003, bins = 4096;  // the last tile is partial
    const uint32_t ip_len = slot - 14;
    std::vector<uint8_t> ring((size_t)slot * n);
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t* f = ring.data() + (size_t)i * slot;
        const bool tcp = i % 3 == 1;
        for (uint32_t k = 0; k < slot; ++k) f[k] = (uint8_t)(i * 31u + k * 7u);  // ports, payload
        std::memset(f, 0x02, 12);
        f[12] = 0x08;
        f[13] = 0x00;
        uint8_t* ip = f + 14;
        const uint8_t v4[20] = {0x45, 0, (uint8_t)(ip_len >> 8), (uint8_t)ip_len, (uint8_t)(i >> 8),
                                (uint8_t)i, 0x40, 0, 64, (uint8_t)(tcp ? 6 : 17), 0, 0,
                                192, 168, (uint8_t)(i >> 9), (uint8_t)(i >> 1), 10, 1, 2, 3};
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
    std::vector<NatRow> table(bins);
    for (uint32_t b = 0; b < bins; ++b)
        table[b] = NatRow{0xc6336400u + (b & 0xffu) + ((b >> 8) << 16), (uint16_t)(20000u + b), 0};

    ingot::gpu::Context ctx(0);
    uint8_t* d_ring = nullptr;
    ingot_rec* d_rec = nullptr;
    ingot_csum* d_sum = nullptr;
    uint32_t* d_flow = nullptr;
    NatRow* d_table = nullptr;
    if (hipMalloc(&d_ring, ring.size()) != hipSuccess ||
        hipMalloc(&d_rec, n * sizeof(ingot_rec)) != hipSuccess ||
        hipMalloc(&d_sum, n * sizeof(ingot_csum)) != hipSuccess ||
        hipMalloc(&d_flow, n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&d_table, bins * sizeof(NatRow)) != hipSuccess)
        return fail("hipMalloc");
    if (hipMemcpy(d_ring, ring.data(), ring.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_table, table.data(), bins * sizeof(NatRow), hipMemcpyHostToDevice) !=
            hipSuccess)
        return fail("H2D");
    const uint32_t what = INGOT_CSUM_L3 | INGOT_CSUM_L4;
    const int chain = INGOT_CHAIN_GENERIC_ULP;
    // the flow bins: one launch, left on the device
    if (ingot_gpu_flow_hist(ctx.get(), d_ring, nullptr, nullptr, slot, n, chain, nullptr, bins,
                            d_flow, nullptr, nullptr, nullptr))
        return fail("flow_hist");
    // two members of one table: d_values = the member, pitch = the row
    const uint8_t* rows = reinterpret_cast<const uint8_t*>(d_table);
    const uint32_t pitch = sizeof(NatRow);
    const std::vector<ingot_edit_rows> nat = {
        ingot::gpu::edit_rows(1, INGOT_F_V4_SOURCE, INGOT_OP_SET, INGOT_EDIT_U32, INGOT_BY_ROW,
                              rows + offsetof(NatRow, address), pitch),
        ingot::gpu::edit_rows(2, INGOT_F_UDP_SOURCE, INGOT_OP_SET, INGOT_EDIT_U16, INGOT_BY_ROW,
                              rows + offsetof(NatRow, port), pitch),
        ingot::gpu::edit_rows(2, INGOT_F_TCP_SOURCE, INGOT_OP_SET, INGOT_EDIT_U16, INGOT_BY_ROW,
                              rows + offsetof(NatRow, port), pitch)};
    std::vector<ingot_csum> sums(n);
    uint32_t not_ok[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) {
            if (ingot_gpu_parse_strided(ctx.get(), d_ring, slot, nullptr, n, chain, d_rec, nullptr))
                return fail("parse_strided");
        } else {
            ingot::gpu::parse_modify_rows(ctx, d_ring, nullptr, nullptr, slot, n, chain, nat, d_flow,
                                          bins, what, d_rec);
        }
        if (ingot_gpu_checksum_verify(ctx.get(), d_ring, nullptr, nullptr, slot, n, d_rec, what,
                                      d_sum, nullptr))
            return fail("checksum_verify");
        if (hipMemcpy(sums.data(), d_sum, n * sizeof(ingot_csum), hipMemcpyDeviceToHost) !=
            hipSuccess)
            return fail("D2H");
        for (uint32_t i = 0; i < n; ++i)
            not_ok[pass] += sums[i].l3_state != INGOT_CSUM_OK || sums[i].l4_state != INGOT_CSUM_OK;
    }
    std::vector<uint8_t> got(ring.size());
    std::vector<uint32_t> flow(n);
    if (hipMemcpy(got.data(), d_ring, got.size(), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(flow.data(), d_flow, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return fail("D2H");
    uint32_t wrong = 0, translated = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* f = got.data() + (size_t)i * slot;
        const uint8_t* was = ring.data() + (size_t)i * slot;
        if (flow[i] >= bins) {  // not counted: not touched
            wrong += std::memcmp(f, was, slot) != 0;
            continue;
        }
        ++translated;
        const NatRow& r = table[flow[i]];
        const uint32_t src = (uint32_t)f[26] << 24 | (uint32_t)f[27] << 16 | (uint32_t)f[28] << 8 |
                             f[29];
        const uint32_t port = (uint32_t)f[34] << 8 | f[35];
        wrong += src != r.address || port != r.port || std::memcmp(f + 30, was + 30, 4) != 0;
    }
    for (void* p : {(void*)d_ring, (void*)d_rec, (void*)d_sum, (void*)d_flow, (void*)d_table})
        (void)hipFree(p);
    const bool ok = !not_ok[0] && !not_ok[1] && !wrong && translated == n;
    std::printf("nat table: %u frames, %u translated, %u not OK before, %u not OK after, "
                "%u not rewritten: %s\n", n, translated, not_ok[0], not_ok[1], wrong,
                ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
