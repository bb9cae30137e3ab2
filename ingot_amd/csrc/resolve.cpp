// resolve.cpp — the public edit, set and sum lists resolved to the kernels'
// argument blocks (resolve.h): field geometry, the operand-table rules, the
// sums an edit feeds.  No HIP runtime call.
#include "resolve.h"

#include <cstring>

namespace {

// ingot_field -> (header kind, first bit, width): the setters' BE geometry
// (ethernet.rs:46-65, ip.rs:63-93 / 159-182, tcp.rs:9-30, udp.rs:8-15,
// icmp.rs:42-50, geneve.rs:16-44; layout rules packet/mod.rs:547-821).
struct FieldGeo {
    uint8_t kind;
    uint16_t bit;
    uint8_t bits;
};
constexpr FieldGeo kFieldGeo[INGOT_F_COUNT] = {
    {ingot_gpu::HK_ETH, 96, 16},
    {ingot_gpu::HK_VLAN, 0, 3},    {ingot_gpu::HK_VLAN, 3, 1},
    {ingot_gpu::HK_VLAN, 4, 12},   {ingot_gpu::HK_VLAN, 16, 16},
    {ingot_gpu::HK_V4, 0, 4},      {ingot_gpu::HK_V4, 4, 4},     {ingot_gpu::HK_V4, 8, 6},
    {ingot_gpu::HK_V4, 14, 2},     {ingot_gpu::HK_V4, 16, 16},   {ingot_gpu::HK_V4, 32, 16},
    {ingot_gpu::HK_V4, 48, 3},     {ingot_gpu::HK_V4, 51, 13},   {ingot_gpu::HK_V4, 64, 8},
    {ingot_gpu::HK_V4, 72, 8},     {ingot_gpu::HK_V4, 80, 16},   {ingot_gpu::HK_V4, 96, 32},
    {ingot_gpu::HK_V4, 128, 32},
    {ingot_gpu::HK_V6, 0, 4},      {ingot_gpu::HK_V6, 4, 6},     {ingot_gpu::HK_V6, 10, 2},
    {ingot_gpu::HK_V6, 12, 20},    {ingot_gpu::HK_V6, 32, 16},   {ingot_gpu::HK_V6, 48, 8},
    {ingot_gpu::HK_V6, 56, 8},
    {ingot_gpu::HK_TCP, 0, 16},    {ingot_gpu::HK_TCP, 16, 16},  {ingot_gpu::HK_TCP, 32, 32},
    {ingot_gpu::HK_TCP, 64, 32},   {ingot_gpu::HK_TCP, 96, 4},   {ingot_gpu::HK_TCP, 100, 4},
    {ingot_gpu::HK_TCP, 104, 8},   {ingot_gpu::HK_TCP, 112, 16}, {ingot_gpu::HK_TCP, 128, 16},
    {ingot_gpu::HK_TCP, 144, 16},
    {ingot_gpu::HK_UDP, 0, 16},    {ingot_gpu::HK_UDP, 16, 16},  {ingot_gpu::HK_UDP, 32, 16},
    {ingot_gpu::HK_UDP, 48, 16},
    {ingot_gpu::HK_ICMP, 0, 8},    {ingot_gpu::HK_ICMP, 8, 8},   {ingot_gpu::HK_ICMP, 16, 16},
    {ingot_gpu::HK_GENEVE, 0, 2},  {ingot_gpu::HK_GENEVE, 2, 6}, {ingot_gpu::HK_GENEVE, 8, 8},
    {ingot_gpu::HK_GENEVE, 16, 16}, {ingot_gpu::HK_GENEVE, 32, 24},
    {ingot_gpu::HK_GENEVE, 56, 8},
};

// The bytes of its header that cover a field: [byte0, byte0 + nbytes), the
// field `rshift` bits above the last one's low end.
struct Cover {
    uint8_t byte0, nbytes, rshift, bits;
};
constexpr Cover cover(FieldGeo g) {
    return Cover{(uint8_t)(g.bit / 8u), (uint8_t)((g.bit % 8u + g.bits + 7u) / 8u),
                 (uint8_t)((8u - ((g.bit + g.bits) % 8u)) % 8u), g.bits};
}

ingot_gpu::Edit edit_of(uint8_t layer, uint8_t field, uint8_t op, uint8_t index, uint32_t value) {
    const Cover c = cover(kFieldGeo[field]);
    return ingot_gpu::Edit{layer, kFieldGeo[field].kind, op, index, c.byte0, c.nbytes, c.rshift,
                           c.bits, value};
}

// ingot_wide_field -> (header kind, byte offset in the header, width).
struct WideGeo {
    uint8_t kind, at, width;
};
bool is_wide(uint8_t field) {
    return field >= INGOT_FW_ETH_DESTINATION && field <= INGOT_FW_V6_DESTINATION;
}
WideGeo wide_geo(uint8_t field) {
    switch (field) {
    case INGOT_FW_ETH_DESTINATION: return {ingot_gpu::HK_ETH, 0, 6};
    case INGOT_FW_ETH_SOURCE: return {ingot_gpu::HK_ETH, 6, 6};
    case INGOT_FW_V6_SOURCE: return {ingot_gpu::HK_V6, 8, 16};
    default: return {ingot_gpu::HK_V6, 24, 16};
    }
}
// A wide field's big-endian pieces of 4 (and, a MAC's last, 2) bytes:
// f(byte offset in the field, bytes).
template <class F>
void wide_pieces(uint32_t width, F f) {
    for (uint32_t b = 0; b < width; b += 4u) f(b, width - b < 4u ? width - b : 4u);
}

// What an ingot_edit_rows and an ingot_emit_set_rows share: the field is a
// narrow or a wide one, BYTES if and only if wide, `by`, a row array for
// BY_ROW, the operand's width by source, the pitch (0: the width) not below
// it, U16 / U32 tables and pitches aligned.
struct Operand {
    bool wide;
    uint32_t pitch;
    const uint8_t* values;
};
bool operand_of(uint8_t field, bool u16, bool u32, bool bytes, uint8_t by, uint32_t pitch,
                const void* d_values, bool have_row, Operand& o) {
    o.wide = is_wide(field);
    if ((!o.wide && field >= INGOT_F_COUNT) || bytes != o.wide) return false;
    if (by > INGOT_BY_ROW || (by == INGOT_BY_ROW && !have_row)) return false;
    const uint32_t width = u16 ? 2u : u32 ? 4u : o.wide ? wide_geo(field).width : 0u;
    if (pitch && pitch < width) return false;
    if ((u16 || u32) && (((uintptr_t)d_values | pitch) & (width - 1u))) return false;
    o.pitch = pitch ? pitch : width;
    o.values = static_cast<const uint8_t*>(d_values);
    return true;
}

// Which sums the bytes of an edit of `field` at chain layer `layer` are covered
// by (ingot_gpu_parse_modify_csum), limited to the sums `what` selects; -1 for
// a field that moves a sum's extent or its pseudo-header's length or protocol.
// A checksum field is left out of its own sum; the tunnel's outer UDP sum
// covers everything from outer_udp (layer 2) on except its own field.
int csum_feeds(int chain, uint8_t layer, uint8_t field, uint32_t what) {
    using namespace ingot_gpu;
    switch (field) {
    case INGOT_F_V4_IHL: case INGOT_F_V4_TOTAL_LEN: case INGOT_F_V4_PROTOCOL:
    case INGOT_F_V6_PAYLOAD_LEN: case INGOT_F_V6_NEXT_HEADER:
        return -1;
    default: break;
    }
    const bool tun = chain == INGOT_CHAIN_GENEVE_OVER_V6;
    const uint8_t kind = kFieldGeo[field].kind;
    uint32_t f = 0;
    // (the tunnel's layer 2 is the outer UDP header, not the parsed L4 layer)
    const bool l4_layer = !tun || layer == 6;
    if (kind == HK_V4 && field != INGOT_F_V4_CHECKSUM && (what & INGOT_CSUM_L3)) f |= FEED_L3;
    if ((field == INGOT_F_V4_SOURCE || field == INGOT_F_V4_DESTINATION) && (what & INGOT_CSUM_L4))
        f |= FEED_PSEUDO4;
    if ((kind == HK_TCP || kind == HK_UDP || kind == HK_ICMP) && l4_layer &&
        field != INGOT_F_TCP_CHECKSUM && field != INGOT_F_UDP_CHECKSUM &&
        field != INGOT_F_ICMP_CHECKSUM && (what & INGOT_CSUM_L4))
        f |= FEED_L4;
    if (tun && layer >= 2 && !(layer == 2 && field == INGOT_F_UDP_CHECKSUM) &&
        (what & INGOT_CSUM_OUTER_L4))
        f |= FEED_OUTER;
    return (int)f;
}

// The sums a wide field's bytes feed.  IPv6 addresses: the L4 sum's
// pseudo-header at the parsed L3 layer (FEED_PSEUDO4's run-time condition, TCP
// / UDP / ICMPv6, is the IPv6 pseudo-header's too), the tunnel's outer sum as
// its pseudo-header (layer 1) or as covered bytes (layer 5).  MACs: the
// tunnel's inner Ethernet (layer 4) is covered by the outer sum; layer 0 feeds
// nothing.
int wide_feeds(int chain, uint8_t layer, uint8_t field, uint32_t what) {
    using namespace ingot_gpu;
    const bool tun = chain == INGOT_CHAIN_GENEVE_OVER_V6;
    const bool v6 = wide_geo(field).kind == HK_V6;
    uint32_t f = 0;
    if (v6 && (!tun || layer == 5) && (what & INGOT_CSUM_L4)) f |= FEED_PSEUDO4;
    if (tun && (what & INGOT_CSUM_OUTER_L4) && (v6 ? layer == 1 || layer == 5 : layer == 4))
        f |= FEED_OUTER;
    return (int)f;
}

// ctx, chain and the size of a rewrite's list; then per edit its op and layer.
bool edit_list_ok(const ingot_gpu_ctx* ctx, int chain, const void* edits, uint32_t n_edits) {
    return ctx && ingot_gpu::chain_ok(chain) && n_edits <= INGOT_MAX_EDITS && (!n_edits || edits);
}
bool op_layer_ok(int chain, uint8_t op, uint8_t layer) {
    return op <= INGOT_OP_XOR && (int)layer < ingot_chain_layer_count(chain);
}

// A field of the header at `at` inside the header block: its first byte.
bool inside(uint16_t at, uint32_t byte0, uint32_t nbytes, uint32_t hdr_len, uint32_t& pos) {
    pos = (uint32_t)at + byte0;  // 32 bits: no wrap before the check
    return pos + nbytes <= hdr_len;
}

}  // namespace

namespace ingot_gpu {

bool what_ok(uint32_t what, uint32_t allowed, bool zero_ok, int chain) {
    return (what != 0 || zero_ok) && !(what & ~allowed) &&
           (!(what & INGOT_CSUM_OUTER_L4) || chain == INGOT_CHAIN_GENEVE_OVER_V6);
}

int resolve_edits(const ingot_gpu_ctx* ctx, int chain, const ingot_edit* edits, uint32_t n_edits,
                  uint32_t what, ModifyCsumArgs& c) {
    if (!edit_list_ok(ctx, chain, edits, n_edits)) return INGOT_GPU_EINVAL;
    c.what = what;
    for (uint32_t k = 0; k < n_edits; ++k) {
        const ingot_edit& e = edits[k];
        if (e.field >= INGOT_F_COUNT || !op_layer_ok(chain, e.op, e.layer)) return INGOT_GPU_EINVAL;
        c.m.e[k] = edit_of(e.layer, e.field, e.op, e.index, e.value);
        if (what) {
            const int f = csum_feeds(chain, e.layer, e.field, what);
            if (f < 0) return INGOT_GPU_EINVAL;
            c.feeds[k] = (uint8_t)f;
        }
    }
    c.m.n_edits = n_edits;
    return INGOT_GPU_SUCCESS;
}

int resolve_edit_rows(const ingot_gpu_ctx* ctx, int chain, const ingot_edit_rows* edits,
                      uint32_t n_edits, const uint32_t* d_row, uint32_t n_rows, uint32_t what,
                      ModifyRowsArgs& a) {
    if (!edit_list_ok(ctx, chain, edits, n_edits) ||
        !what_ok(what, INGOT_CSUM_L3 | INGOT_CSUM_L4 | INGOT_CSUM_OUTER_L4, true, chain))
        return INGOT_GPU_EINVAL;
    uint32_t np = 0;
    for (uint32_t k = 0; k < n_edits; ++k) {
        const ingot_edit_rows& e = edits[k];
        Operand o;
        if (e.source > INGOT_EDIT_BYTES || e._pad || !op_layer_ok(chain, e.op, e.layer) ||
            !operand_of(e.field, e.source == INGOT_EDIT_U16, e.source == INGOT_EDIT_U32,
                        e.source == INGOT_EDIT_BYTES, e.by, e.pitch, e.d_values, d_row != nullptr,
                        o))
            return INGOT_GPU_EINVAL;
        // a table takes no value of its own; a wide field is only ever SET
        if (e.source != INGOT_EDIT_VALUE && (e.value || !e.d_values)) return INGOT_GPU_EINVAL;
        if (o.wide && e.op != INGOT_OP_SET) return INGOT_GPU_EINVAL;
        const int f = !what    ? 0
                      : o.wide ? wide_feeds(chain, e.layer, e.field, what)
                               : csum_feeds(chain, e.layer, e.field, what);
        if (f < 0) return INGOT_GPU_EINVAL;
        auto piece = [&](const Edit& d, uint8_t source, uint32_t at) {
            a.e[np++] = RowPiece{d, source, e.by, (uint8_t)f, 0, o.pitch, o.values + at};
        };
        if (!o.wide) {  // VALUE / U16 / U32 are RowSource's first three
            piece(edit_of(e.layer, e.field, e.op, e.index, e.value), e.source, 0);
            continue;
        }
        const WideGeo g = wide_geo(e.field);
        wide_pieces(g.width, [&](uint32_t b, uint32_t nb) {
            piece(Edit{e.layer, g.kind, INGOT_OP_SET, e.index, (uint8_t)(g.at + b), (uint8_t)nb, 0,
                       (uint8_t)(8u * nb), 0u},
                  nb == 4u ? ROWS_BE32 : ROWS_BE16, b);
        });
    }
    a.n_pieces = np;
    a.row = d_row;
    a.n_rows = n_rows;
    a.what = what;
    return INGOT_GPU_SUCCESS;
}

int emit_args(const uint8_t* hdr, uint32_t hdr_len, const ingot_emit_set* sets, uint32_t n_sets,
              EmitArgs& a) {
    if (hdr_len > INGOT_MAX_EMIT_HDR || (hdr_len && !hdr) || n_sets > INGOT_MAX_EMIT_SETS ||
        (n_sets && !sets))
        return INGOT_GPU_EINVAL;
    if (hdr_len) std::memcpy(a.hdr, hdr, hdr_len);  // the rest stays zero
    a.hdr_len = hdr_len;
    for (uint32_t k = 0; k < n_sets; ++k) {
        const ingot_emit_set& e = sets[k];
        if (e.field >= INGOT_F_COUNT || e.source > INGOT_EMIT_VALUE) return INGOT_GPU_EINVAL;
        if ((e.source == INGOT_EMIT_U16 || e.source == INGOT_EMIT_U32) && !e.d_values)
            return INGOT_GPU_EINVAL;
        const Cover c = cover(kFieldGeo[e.field]);
        uint32_t pos;
        if (!inside(e.at, c.byte0, c.nbytes, hdr_len, pos)) return INGOT_GPU_EINVAL;
        a.sets[k] = EmitSet{(uint16_t)pos, e.at, c.nbytes, c.rshift, c.bits, e.source, e.add,
                            e.d_values};
    }
    a.n_sets = n_sets;
    return INGOT_GPU_SUCCESS;
}

int emit_sums(const uint8_t* hdr, uint32_t hdr_len, const ingot_emit_set* sets, uint32_t n_sets,
              const ingot_emit_sum* sums, uint32_t n_sums, EmitArgs& a) {
    if (n_sums > INGOT_MAX_EMIT_SUMS || (n_sums && !sums)) return INGOT_GPU_EINVAL;
    for (uint32_t k = 0; k < n_sums; ++k) {
        const ingot_emit_sum& s = sums[k];
        if (s.kind > INGOT_EMIT_SUM_UDP || s._pad[0] || s._pad[1] || s._pad[2] || (s.at & 1u) ||
            (s.l3_at & 1u))
            return INGOT_GPU_EINVAL;
        const uint32_t at = s.at, l3 = s.l3_at;
        uint32_t named;  // the header whose version / ihl this sum takes from hdr
        if (s.kind == INGOT_EMIT_SUM_IPV4) {
            if (a.sums.v4 || l3 != 0 || at + 20u > hdr_len) return INGOT_GPU_EINVAL;
            const uint32_t ihl = hdr[at] & 0xfu;
            if ((hdr[at] >> 4) != 4 || ihl < 5 || at + 4u * ihl > hdr_len) return INGOT_GPU_EINVAL;
            a.sums.v4 = 1;
            a.sums.v4_at = s.at;
            a.sums.v4_len = (uint16_t)(4u * ihl);
            named = at;
        } else {
            if (a.sums.udp || at + 8u > hdr_len || l3 >= hdr_len) return INGOT_GPU_EINVAL;
            const uint32_t version = hdr[l3] >> 4;
            if (version != 4 && version != 6) return INGOT_GPU_EINVAL;
            if (l3 + (version == 4 ? 20u : 40u) > at) return INGOT_GPU_EINVAL;
            a.sums.udp = 1;
            a.sums.udp_v6 = version == 6;
            a.sums.udp_at = s.at;
            a.sums.udp_l3 = s.l3_at;
            named = l3;
        }
        for (uint32_t e = 0; e < n_sets; ++e)
            if (sets[e].at == named &&
                (sets[e].field == INGOT_F_V4_VERSION || sets[e].field == INGOT_F_V4_IHL ||
                 sets[e].field == INGOT_F_V6_VERSION))
                return INGOT_GPU_EINVAL;
    }
    return INGOT_GPU_SUCCESS;
}

int emit_rows_pieces(const ingot_emit_set_rows* sets, uint32_t n_sets, bool have_row,
                     uint32_t hdr_len, EmitRowsArgs& a, ingot_emit_set* narrow,
                     uint32_t& n_narrow) {
    n_narrow = 0;
    if (n_sets > INGOT_MAX_EMIT_SETS || (n_sets && !sets)) return INGOT_GPU_EINVAL;
    uint32_t np = 0;
    for (uint32_t k = 0; k < n_sets; ++k) {
        const ingot_emit_set_rows& e = sets[k];
        Operand o;
        if (e.source > INGOT_EMIT_BYTES || e._pad[0] || e._pad[1] || e._pad[2] ||
            !operand_of(e.field, e.source == INGOT_EMIT_U16, e.source == INGOT_EMIT_U32,
                        e.source == INGOT_EMIT_BYTES, e.by, e.pitch, e.d_values, have_row, o))
            return INGOT_GPU_EINVAL;
        // LENGTH and VALUE take no table; a wide field's bytes take no `add`
        const bool table = e.source != INGOT_EMIT_LENGTH && e.source != INGOT_EMIT_VALUE;
        if (table ? !e.d_values : (e.by || e.pitch || e.d_values)) return INGOT_GPU_EINVAL;
        if (o.wide && e.add != 0) return INGOT_GPU_EINVAL;
        uint32_t pos;
        if (!o.wide) {
            const Cover c = cover(kFieldGeo[e.field]);
            if (!inside(e.at, c.byte0, c.nbytes, hdr_len, pos)) return INGOT_GPU_EINVAL;
            a.p[np++] = EmitPiece{(uint16_t)pos, e.at, c.nbytes, c.rshift, c.bits,
                                  e.source,  // LENGTH .. VALUE are EmitPieceSource's first four
                                  e.by, {0, 0, 0}, e.add, o.pitch, o.values};
            narrow[n_narrow++] = ingot_emit_set{e.at, e.field, e.source, e.add, nullptr};
            continue;
        }
        const WideGeo g = wide_geo(e.field);
        if (!inside(e.at, g.at, g.width, hdr_len, pos)) return INGOT_GPU_EINVAL;
        wide_pieces(g.width, [&](uint32_t b, uint32_t nb) {
            const bool aligned = !(((uintptr_t)(o.values + b) | o.pitch) & (nb - 1u));
            a.p[np++] = EmitPiece{(uint16_t)(pos + b), 0, (uint8_t)nb, 0, (uint8_t)(8u * nb),
                                  (uint8_t)(nb == 4u ? (aligned ? EP_BE32A : EP_BE32)
                                                     : (aligned ? EP_BE16A : EP_BE16)),
                                  e.by, {0, 0, 0}, 0, o.pitch, o.values + b};
        });
    }
    a.n_pieces = np;
    return INGOT_GPU_SUCCESS;
}

}  // namespace ingot_gpu
