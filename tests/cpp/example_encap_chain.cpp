// example_encap_chain.cpp — example_encap_table.cpp for a header-split ring,
// from a host that binds only the C ABI.  Every frame is two chunks: its
// Ethernet / IPv4 / UDP headers (42 B) in a slot of the header ring, the rest in
// a slot of the payload ring, at an odd address.  ingot_gpu_flow_hist over the
// header ring leaves every packet's flow bin on the device, and that array, as
// it is, selects the packet's row of a `bins`-row endpoint table {underlay
// IPv6, next-hop MAC, VNI} (ingot_gpu_emit_packets_read_rows, INGOT_BY_ROW).
// One launch pulls the two chunks up behind the outer Ethernet / IPv6 / UDP /
// Geneve stack with that flow's outer IPv6 destination, destination MAC and
// VNI, and fills the outer UDP sum over them; a frame flow_hist does not count
// (here: ARP) is not emitted, its chunks are not read (their offsets are
// unusable) and its d_taken is 0.  The result is parsed as GENEVE_OVER_V6 and
// ingot_gpu_checksum_verify must find every sum of every emitted packet Ok.
// Run on the GPU by tests/test_emit_read_rows.py.
#include <hip/hip_runtime.h>

#include <cstddef>
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

// one row of the host's endpoint table, as the device reads it
struct Endpoint {
    uint8_t underlay[16];  // wire order: INGOT_EMIT_BYTES
    uint8_t mac[6];        // wire order: INGOT_EMIT_BYTES
    uint16_t _pad;
    uint32_t vni;          // host-endian: INGOT_EMIT_U32
    uint32_t _pad2;
};
static_assert(sizeof(Endpoint) == 32, "Endpoint is 32 bytes");

int main() {
    const uint32_t slot = 128, n = 20003, bins = 64;  // the last group is partial
    const uint32_t H = 70, out_slot = 208;            // 14 + 40 + 8 + 8; H + slot <= out_slot
    const uint32_t ip_len = slot - 14;
    const uint32_t hsplit = 42, hslot = 64, pslot = 96;  // 14 + 20 + 8 | the other 86 B at + 3
    std::vector<uint8_t> ring((size_t)slot * n);
    uint32_t arps = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t* f = ring.data() + (size_t)i * slot;
        for (uint32_t k = 0; k < slot; ++k) f[k] = (uint8_t)(i * 31u + k * 7u);  // ports, payload
        std::memset(f, 0x02, 12);
        f[12] = 0x08;
        f[13] = 0x00;
        if (i % 7 == 3) {  // ARP: no flow, not counted
            f[13] = 0x06;
            ++arps;
            continue;
        }
        uint8_t* ip = f + 14;
        const uint8_t v4[20] = {0x45, 0, (uint8_t)(ip_len >> 8), (uint8_t)ip_len, (uint8_t)(i >> 8),
                                (uint8_t)i, 0x40, 0, 64, 17, 0, 0,
                                192, 168, (uint8_t)(i >> 9), (uint8_t)(i >> 1), 10, 1, 2, 3};
        std::memcpy(ip, v4, 20);
        const uint16_t hc = fold_not(add_words(0, ip, 20));
        ip[10] = (uint8_t)(hc >> 8);
        ip[11] = (uint8_t)hc;
        uint8_t* l4 = ip + 20;
        const uint32_t seg = ip_len - 20;
        l4[4] = (uint8_t)(seg >> 8);
        l4[5] = (uint8_t)seg;
        l4[6] = l4[7] = 0;
        uint16_t c = fold_not(add_words(add_words(0, ip + 12, 8) + 17u + seg, l4, seg));
        if (c == 0) c = 0xffff;
        l4[6] = (uint8_t)(c >> 8);
        l4[7] = (uint8_t)c;
    }
    std::vector<Endpoint> table(bins);
    for (uint32_t b = 0; b < bins; ++b) {
        Endpoint& e = table[b];
        std::memset(&e, 0, sizeof e);
        const uint8_t v6[16] = {0xfd, 0, 0, 0, 0xf7, 1, 1, 0, 0, 0, 0, 0, 0, 0, (uint8_t)(b >> 4),
                                (uint8_t)(b * 17u + 1u)};
        std::memcpy(e.underlay, v6, 16);
        const uint8_t mac[6] = {0xa8, 0x40, 0x25, 0x77, (uint8_t)b, (uint8_t)(b ^ 0x5a)};
        std::memcpy(e.mac, mac, 6);
        e.vni = 0x100000u + b * 257u;
    }
    // outer Ethernet / IPv6 / UDP / Geneve, serialised once
    uint8_t hdr[H];
    std::memset(hdr, 0, H);
    std::memset(hdr + 6, 0x0a, 6);
    hdr[12] = 0x86;
    hdr[13] = 0xdd;
    hdr[14] = 0x60;
    hdr[20] = 17;    // next header
    hdr[21] = 0xf0;  // hop limit
    hdr[22] = 0xfd;  // source fd00::2
    hdr[37] = 2;
    hdr[54] = 0xc0;  // UDP source port
    hdr[55] = 0xde;
    hdr[56] = 6081 >> 8;
    hdr[57] = 6081 & 0xff;
    hdr[64] = 0x65;  // Geneve protocol type: Ethernet
    hdr[65] = 0x58;

    ingot_gpu_ctx* ctx = nullptr;
    if (ingot_gpu_ctx_create(0, &ctx)) return fail("ctx_create");
    const size_t out_bytes = (size_t)out_slot * n;
    // one chunk arena: the header ring, then the payload ring
    const size_t pay_at = (size_t)hslot * n, arena_bytes = pay_at + (size_t)pslot * n;
    std::vector<uint8_t> arena(arena_bytes, 0xEE);
    std::vector<uint64_t> seg_off(2 * (size_t)n);
    std::vector<uint16_t> seg_len(2 * (size_t)n), hlen(n, (uint16_t)hsplit);
    std::vector<uint32_t> pkt_seg(n + 1);
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* f = ring.data() + (size_t)i * slot;
        const bool arp = f[13] == 0x06;
        std::memcpy(arena.data() + (size_t)i * hslot, f, hsplit);
        std::memcpy(arena.data() + pay_at + (size_t)i * pslot + 3, f + hsplit, slot - hsplit);
        // an uncounted frame's chunks: nothing that could be read
        seg_off[2 * i] = arp ? (1ull << 60) : (uint64_t)i * hslot;
        seg_off[2 * i + 1] = arp ? (1ull << 60) : pay_at + (uint64_t)i * pslot + 3;
        seg_len[2 * i] = arp ? 65535 : (uint16_t)hsplit;
        seg_len[2 * i + 1] = arp ? 65535 : (uint16_t)(slot - hsplit);
        pkt_seg[i] = 2 * i;
    }
    pkt_seg[n] = 2 * n;
    uint8_t *d_ring = nullptr, *d_out = nullptr;
    uint64_t* d_seg_off = nullptr;
    uint16_t *d_seg_len = nullptr, *d_hlen = nullptr, *d_taken = nullptr;
    uint32_t* d_pkt_seg = nullptr;
    ingot_rec* d_rec = nullptr;
    ingot_csum* d_sum = nullptr;
    uint32_t* d_flow = nullptr;
    Endpoint* d_table = nullptr;
    uint64_t* d_dst_off = nullptr;
    uint16_t* d_out_len = nullptr;
    if (hipMalloc(&d_ring, arena_bytes + 16) != hipSuccess ||
        hipMalloc(&d_seg_off, 2 * (size_t)n * 8) != hipSuccess ||
        hipMalloc(&d_seg_len, 2 * (size_t)n * 2) != hipSuccess ||
        hipMalloc(&d_hlen, n * 2) != hipSuccess || hipMalloc(&d_taken, n * 2) != hipSuccess ||
        hipMalloc(&d_pkt_seg, ((size_t)n + 1) * 4) != hipSuccess ||
        hipMalloc(&d_out, out_bytes) != hipSuccess ||
        hipMalloc(&d_rec, n * sizeof(ingot_rec)) != hipSuccess ||
        hipMalloc(&d_sum, n * sizeof(ingot_csum)) != hipSuccess ||
        hipMalloc(&d_flow, n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&d_table, bins * sizeof(Endpoint)) != hipSuccess ||
        hipMalloc(&d_dst_off, n * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&d_out_len, n * sizeof(uint16_t)) != hipSuccess)
        return fail("hipMalloc");
    std::vector<uint64_t> dst_off(n);
    std::vector<uint16_t> out_len(n, (uint16_t)(H + slot));
    for (uint32_t i = 0; i < n; ++i) dst_off[i] = (uint64_t)i * out_slot;
    if (hipMemcpy(d_ring, arena.data(), arena_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_seg_off, seg_off.data(), 2 * (size_t)n * 8, hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemcpy(d_seg_len, seg_len.data(), 2 * (size_t)n * 2, hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemcpy(d_hlen, hlen.data(), n * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_pkt_seg, pkt_seg.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemset(d_taken, 0xA5, n * 2) != hipSuccess ||
        hipMemcpy(d_table, table.data(), bins * sizeof(Endpoint), hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemcpy(d_dst_off, dst_off.data(), n * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_out_len, out_len.data(), n * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_out, 0xA5, out_bytes) != hipSuccess)
        return fail("H2D");
    // the flow bins from the header ring alone: one launch, left on the device
    if (ingot_gpu_flow_hist(ctx, d_ring, nullptr, d_hlen, hslot, n, INGOT_CHAIN_GENERIC_ULP, nullptr,
                            bins, d_flow, nullptr, nullptr, nullptr))
        return fail("flow_hist");
    // three members of one table: d_values = the member, pitch = the row
    const uint8_t* rows = reinterpret_cast<const uint8_t*>(d_table);
    const uint32_t pitch = sizeof(Endpoint);
    const ingot_emit_set_rows sets[] = {
        {14, INGOT_F_V6_PAYLOAD_LEN, INGOT_EMIT_LENGTH, -40, 0, {0, 0, 0}, 0, nullptr},
        {54, INGOT_F_UDP_LENGTH, INGOT_EMIT_LENGTH, 0, 0, {0, 0, 0}, 0, nullptr},
        {14, INGOT_FW_V6_DESTINATION, INGOT_EMIT_BYTES, 0, INGOT_BY_ROW, {0, 0, 0}, pitch,
         rows + offsetof(Endpoint, underlay)},
        {0, INGOT_FW_ETH_DESTINATION, INGOT_EMIT_BYTES, 0, INGOT_BY_ROW, {0, 0, 0}, pitch,
         rows + offsetof(Endpoint, mac)},
        {62, INGOT_F_GENEVE_VNI, INGOT_EMIT_U32, 0, INGOT_BY_ROW, {0, 0, 0}, pitch,
         rows + offsetof(Endpoint, vni)}};
    const ingot_emit_sum udp_sum = {54, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}};
    if (ingot_gpu_emit_packets_read_rows(ctx, hdr, H, sets, 5, &udp_sum, 1, d_flow, bins, d_ring,
                                         d_seg_off, d_seg_len, d_pkt_seg, nullptr, nullptr, n,
                                         d_out, d_dst_off, d_taken, nullptr))
        return fail("emit_packets_read_rows");

    std::vector<uint32_t> flow(n);
    std::vector<uint8_t> got(out_bytes);
    std::vector<ingot_rec> rec(n);
    std::vector<ingot_csum> sums(n);
    std::vector<uint16_t> taken(n);
    if (hipMemcpy(flow.data(), d_flow, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(taken.data(), d_taken, n * 2, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(got.data(), d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return fail("D2H");
    // the tunnel parse: inner sums; the outer stack as a UDP packet: the outer sum
    uint32_t emitted = 0, not_parsed = 0, not_ok[2] = {0, 0};
    const int chains[2] = {INGOT_CHAIN_GENEVE_OVER_V6, INGOT_CHAIN_UDP_PARSER};
    for (int pass = 0; pass < 2; ++pass) {
        if (ingot_gpu_parse_strided(ctx, d_out, out_slot, d_out_len, n, chains[pass], d_rec, nullptr))
            return fail("parse_strided");
        if (ingot_gpu_checksum_verify(ctx, d_out, nullptr, d_out_len, out_slot, n, d_rec,
                                      pass ? INGOT_CSUM_L4 : INGOT_CSUM_L3 | INGOT_CSUM_L4, d_sum,
                                      nullptr))
            return fail("checksum_verify");
        if (hipMemcpy(rec.data(), d_rec, n * sizeof(ingot_rec), hipMemcpyDeviceToHost) !=
                hipSuccess ||
            hipMemcpy(sums.data(), d_sum, n * sizeof(ingot_csum), hipMemcpyDeviceToHost) !=
                hipSuccess)
            return fail("D2H");
        for (uint32_t i = 0; i < n; ++i) {
            if (flow[i] >= bins) continue;
            not_parsed += rec[i].status != 0;
            not_ok[pass] += sums[i].l4_state != INGOT_CSUM_OK ||
                            (!pass && sums[i].l3_state != INGOT_CSUM_OK);
        }
    }
    uint32_t wrong = 0, touched = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* p = got.data() + (size_t)i * out_slot;
        if (flow[i] >= bins) {  // not counted: not emitted, no byte of its slot stored
            for (uint32_t k = 0; k < out_slot; ++k) touched += p[k] != 0xA5;
            wrong += taken[i] != 0;
            continue;
        }
        ++emitted;
        wrong += taken[i] != slot;
        const Endpoint& e = table[flow[i]];
        const uint32_t vni = (uint32_t)p[66] << 16 | (uint32_t)p[67] << 8 | p[68];
        wrong += std::memcmp(p + 38, e.underlay, 16) != 0 || std::memcmp(p, e.mac, 6) != 0 ||
                 vni != e.vni || std::memcmp(p + H, ring.data() + (size_t)i * slot, slot) != 0;
        for (uint32_t k = H + slot; k < out_slot; ++k) touched += p[k] != 0xA5;
    }
    for (void* p : {(void*)d_ring, (void*)d_out, (void*)d_rec, (void*)d_sum, (void*)d_flow,
                    (void*)d_table, (void*)d_dst_off, (void*)d_out_len,
                    (void*)d_seg_off, (void*)d_seg_len, (void*)d_hlen, (void*)d_taken,
                    (void*)d_pkt_seg})
        (void)hipFree(p);
    ingot_gpu_ctx_destroy(ctx);
    const bool ok = emitted == n - arps && !not_parsed && !not_ok[0] && !not_ok[1] && !wrong &&
                    !touched;
    std::printf("encap chain: %u frames, %u emitted, %u not emitted, %u not parsed, %u inner not OK, "
                "%u outer not OK, %u wrong fields, %u stray bytes: %s\n", n, emitted, n - emitted,
                not_parsed, not_ok[0], not_ok[1], wrong, touched, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
