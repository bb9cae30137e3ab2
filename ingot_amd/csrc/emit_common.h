// emit_common.h — what the emit kernels share (emit.hip: k_emit; emit_read.hip:
// k_emit_read).  Helpers: the funnel shift and its DPP neighbour, the
// predicated edge store, the setters' values (and the per-row operands of the
// rows kernels), the 16-bit word sums of the fused checksums (sums.h).  Steps
// of the kernels, below them: the template load, a packet's region (from the
// sets, or from the rows kernels' pieces) and the start of its sums, and a destination
// chunk's way out (header merge, UDP share, store, the parked chunks' finish).
// One copy of each; the kernels keep their descriptors and how a chunk's
// payload bytes are loaded.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ingot_gpu.h"
#include "kernels.h"
#include "sums.h"

namespace ingot_gpu {
namespace {

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

// --- ingot_gpu_emit_packets_csum (the SUMS instantiations; sums.h has the words) ---
// The 16-bit words as loaded of bytes [b0, b1) of a packet's region (LDS, 16-B aligned), added.
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

// --- the kernels' shared steps ----------------------------------------------
// Per-packet LDS of the UDP sum: the packet's accumulator and the one or two
// chunks that hold the checksum field (two when its bytes straddle a 16-B
// destination boundary), parked until the sum is known.
constexpr uint32_t SUM_LDS_PER_PACKET = 4u + 2u * 16u;

// The header block between zero bytes, as TB 16-B blocks at the start of LDS.
constexpr uint32_t TB = INGOT_MAX_EMIT_HDR / 16 + 4;  // 16 B before, 48 B after
__device__ __forceinline__ void load_template(u32x4* tmpl, const EmitArgs& a, uint32_t block) {
    for (uint32_t k = threadIdx.x; k < TB; k += block) {
        const bool in = k >= 1 && k <= INGOT_MAX_EMIT_HDR / 16;
        tmpl[k] = in ? u32x4{a.hdr[4 * k - 4], a.hdr[4 * k - 3], a.hdr[4 * k - 2],
                             a.hdr[4 * k - 1]}
                     : u32x4{0u, 0u, 0u, 0u};
    }
}

// Step 2.  Packet i's header block in its region R (RS bytes of LDS): the
// template bytes shifted to the destination's alignment (region byte b =
// header byte b - dmis), then the setters byte by byte: every covering byte's
// new value depends only on its own mask and value bits (neighbouring bits
// kept).  `total` is what INGOT_EMIT_LENGTH counts from.
__device__ __forceinline__ void build_region(uint8_t* R, uint32_t RS, const u32x4* tmpl,
                                             const EmitArgs& a, uint64_t i, bool live,
                                             uint32_t dmis, uint32_t total) {
    uint32_t v[INGOT_MAX_EMIT_SETS];  // coalesced set-value loads
#pragma unroll
    for (uint32_t s = 0; s < INGOT_MAX_EMIT_SETS; ++s)
        v[s] = (s < a.n_sets && live) ? set_value(a.sets[s], i, total) : 0u;
    if (!a.hdr_len || !live) return;
    for (uint32_t m = 0; m < RS / 16u; ++m) {
        const uint32_t tb = 16u + 16u * m - dmis;  // template byte of region byte 16m (+16)
        reinterpret_cast<u32x4*>(R)[m] = funnel(tmpl[tb >> 4], tmpl[(tb >> 4) + 1], tb & 15u);
    }
#pragma unroll
    for (uint32_t s = 0; s < INGOT_MAX_EMIT_SETS; ++s) {
        if (s >= a.n_sets) break;
        const EmitSet& e = a.sets[s];
        const uint32_t fm = e.bits >= 32 ? 0xffffffffu : ((1u << e.bits) - 1u);
        const uint32_t m = fm << e.rshift, vb = (v[s] & fm) << e.rshift;
        for (uint32_t k = 0; k < e.nbytes; ++k) {
            const uint32_t shb = 8u * (e.nbytes - 1u - k);
            uint8_t& b = R[dmis + e.pos + k];
            b = (uint8_t)((b & ~(m >> shb)) | ((vb >> shb) & (m >> shb)));
        }
    }
}

// --- ingot_gpu_emit_packets_rows / _read_rows (the ROWS instantiations) ----
// What WaveDesc::mis / ReadDesc::dmis holds for a packet the row guard holds
// back (no packet's misalignment): step 5 returns on it.
constexpr uint32_t GUARDED = 0xffffffffu;

// The operand of piece e for packet i, whose row index is r.  `total` as in
// set_value.  A wire-order piece comes back as the big-endian number the setter loop
// takes: one load and a byte swap from an aligned table, byte loads otherwise.
__device__ __forceinline__ uint32_t piece_value(const EmitPiece& e, uint64_t i, uint32_t r,
                                                uint32_t total) {
    if (e.source == EP_LENGTH) return total - e.at + (uint32_t)e.add;
    if (e.source == EP_VALUE) return (uint32_t)e.add;
    const uint8_t* p = e.values + (e.by ? (uint64_t)r : i) * (uint64_t)e.pitch;
    switch (e.source) {
    case EP_U16: return (uint32_t)*gbl((const uint16_t*)p) + (uint32_t)e.add;
    case EP_U32: return *gbl((const uint32_t*)p) + (uint32_t)e.add;
    case EP_BE16A: return __builtin_bswap32((uint32_t)*gbl((const uint16_t*)p)) >> 16;
    case EP_BE32A: return __builtin_bswap32(*gbl((const uint32_t*)p));
    case EP_BE16: return (uint32_t)gbl(p)[0] << 8 | gbl(p)[1];
    default:
        return (uint32_t)gbl(p)[0] << 24 | (uint32_t)gbl(p)[1] << 16 | (uint32_t)gbl(p)[2] << 8 |
               gbl(p)[3];
    }
}

// The pieces into LDS, for every lane of the prologue waves to read at one
// address: 32 pieces' fields read from the argument block in two unrolled
// loops made the compiler keep a private copy of the whole block (scratch).
template <class RowsArgs>  // EmitRowsArgs or EmitReadRowsArgs
__device__ __forceinline__ void load_pieces(EmitPiece* P, const RowsArgs& a, uint32_t block) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a.p);
    for (uint32_t k = threadIdx.x; k < a.n_pieces * (uint32_t)(sizeof(EmitPiece) / 4u); k += block)
        reinterpret_cast<uint32_t*>(P)[k] = w[k];
}

// Piece s as every lane of the wave holds it: read from LDS at one address and
// made scalar, so that its fields sit in SGPRs and the branches on them are
// the wave's, as they are for the sets of the argument block.
__device__ __forceinline__ EmitPiece wave_piece(const EmitPiece* P, uint32_t s) {
    uint32_t w[sizeof(EmitPiece) / 4u];
#pragma unroll
    for (uint32_t k = 0; k < sizeof(EmitPiece) / 4u; ++k)
        w[k] = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)reinterpret_cast<const uint32_t*>(P + s)[k]);
    EmitPiece e;
    __builtin_memcpy(&e, w, sizeof e);
    return e;
}

// Step 2 of the rows kernels: build_region with the pieces P (LDS) in place of
// the sets; the region's two steps are build_region's.  The first piece's
// operand is loaded before the template funnel and piece s + 1's before piece
// s is applied (by packet: coalesced; by row: gathers), so a load's latency
// overlaps the funnel or the piece before it, in a loop that is not unrolled:
// no value array, and a prologue of build_region's size.  A packet that is
// not live (past the batch, or held back by the row guard) loads nothing.
__device__ __forceinline__ void build_region_rows(uint8_t* R, uint32_t RS, const u32x4* tmpl,
                                                  const EmitPiece* P, uint32_t n_pieces,
                                                  uint32_t hdr_len, uint64_t i, uint32_t r,
                                                  bool live, uint32_t dmis, uint32_t total) {
    if (!hdr_len || !live) return;
    uint32_t next = n_pieces ? piece_value(wave_piece(P, 0), i, r, total) : 0u;
    for (uint32_t m = 0; m < RS / 16u; ++m) {
        const uint32_t tb = 16u + 16u * m - dmis;  // template byte of region byte 16m (+16)
        reinterpret_cast<u32x4*>(R)[m] = funnel(tmpl[tb >> 4], tmpl[(tb >> 4) + 1], tb & 15u);
    }
#pragma unroll 1
    for (uint32_t s = 0; s < n_pieces; ++s) {
        const uint32_t v = next;
        if (s + 1 < n_pieces) next = piece_value(wave_piece(P, s + 1), i, r, total);
        const EmitPiece e = wave_piece(P, s);
        const uint32_t fm = e.bits >= 32 ? 0xffffffffu : ((1u << e.bits) - 1u);
        const uint32_t m = fm << e.rshift, vb = (v & fm) << e.rshift;
        for (uint32_t k = 0; k < e.nbytes; ++k) {
            const uint32_t shb = 8u * (e.nbytes - 1u - k);
            uint8_t& b = R[dmis + e.pos + k];
            b = (uint8_t)((b & ~(m >> shb)) | ((vb >> shb) & (m >> shb)));
        }
    }
}

// Step 2b.  The sums of the region its lane just patched (`total` = header +
// payload bytes).  IPv4: complete, and written into the region before
// anything reads it (so a UDP segment that covers the header sums the final
// bytes).  UDP: the header bytes of the segment [udp_at, H) without the
// field, and the pseudo-header, start the packet's accumulator *acc; the
// walkers add the payload.  All of it has the parity of the destination
// address (`at` and `l3_at` are even).
__device__ __forceinline__ void start_sums(uint8_t* R, const EmitArgs& a, bool live,
                                           uint32_t dmis, uint32_t total, uint32_t* acc) {
    const uint32_t odd = dmis & 1u;
    if (live && a.sums.v4) {
        const uint32_t b0 = dmis + a.sums.v4_at;
        R[b0 + 10] = 0;
        R[b0 + 11] = 0;
        const uint32_t f = fold16(region_words(R, b0, b0 + a.sums.v4_len));
        const uint32_t c = ~(odd ? f : swap16(f)) & 0xffffu;
        R[b0 + 10] = (uint8_t)(c >> 8);
        R[b0 + 11] = (uint8_t)c;
    }
    if (a.sums.udp) {
        uint32_t s = 0;
        if (live) {
            const uint32_t b0 = dmis + a.sums.udp_at, l3 = dmis + a.sums.udp_l3;
            const uint32_t seg = total - a.sums.udp_at;  // > 65535: never written
            const uint32_t tail = fold16(seg + 17u);     // length and next header / protocol
            s = region_words(R, b0, dmis + a.hdr_len) - ((uint32_t)R[b0 + 6] << (8u * odd)) -
                ((uint32_t)R[b0 + 7] << (8u * (odd ^ 1u))) +
                (a.sums.udp_v6 ? region_words(R, l3 + 8u, l3 + 40u)
                               : region_words(R, l3 + 12u, l3 + 20u)) +
                (odd ? tail : swap16(tail));
        }
        *acc = s;
    }
}

// A destination chunk whose byte 0 is packet byte r0: its first H - r0 bytes
// are header bytes and come from the packet's region (hb: the region's chunk,
// by value: a pointer here moved the kernels' LDS load).
__device__ __forceinline__ void merge_header(u32x4& out, const u32x4 hb, uint32_t H, int32_t r0) {
    const int32_t hc = (int32_t)H - r0;
    const uint32_t m0 = below(hc), m1 = below(hc - 4), m2 = below(hc - 8), m3 = below(hc - 12);
    out.x = (hb.x & m0) | (out.x & ~m0);
    out.y = (hb.y & m1) | (out.y & ~m1);
    out.z = (hb.z & m2) | (out.z & ~m2);
    out.w = (hb.w & m3) | (out.w & ~m3);
}

// The UDP share of chunk c of packet qq (destination misalignment qd, QT
// bytes, the checksum field at header byte fpos): the words as loaded of its
// payload bytes; a segmented inclusive scan over the wave (the lanes of a
// packet are contiguous, chunk c is c lanes after its packet's first) leaves
// the packet's share of this step in its last lane (`last`), which adds it in
// LDS.  The chunk(s) holding the field wait in `park` (two slots of np
// chunks) for the sum: returns whether this one does.
__device__ __forceinline__ bool udp_share(const u32x4& out, bool valid, bool last, uint32_t c,
                                          uint32_t qq, uint32_t qd, uint32_t H, uint32_t QT,
                                          int32_t r0, uint32_t fpos, uint32_t lane, uint32_t* acc,
                                          u32x4* park, uint32_t np) {
    const int32_t p0 = max((int32_t)H - r0, 0), p1 = min((int32_t)QT - r0, 16);
    uint32_t s = (valid && p0 < p1) ? chunk_words(out, p0, p1) : 0u;
#pragma unroll
    for (uint32_t o = 1; o < WAVE; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)s, o);
        if (lane >= o && o <= c) s += y;
    }
    if (last && s) atomicAdd(&acc[qq], s);
    const uint32_t cf = (qd + fpos) >> 4;
    const bool parked = valid && (c == cf || c == ((qd + fpos + 1u) >> 4));
    if (parked) park[(c - cf) * np + qq] = out;
    return parked;
}

// The chunk whose byte 0 is byte r0 of the QT-byte packet at QD: whole as one
// 16-B store, a packet's first or last chunk as predicated pieces.
__device__ __forceinline__ void store_chunk(uint8_t* QD, int32_t r0, uint32_t QT, const u32x4 out) {
    const int32_t t0 = r0 < 0 ? -r0 : 0;
    const int32_t t1 = (int32_t)QT - r0 < 16 ? (int32_t)QT - r0 : 16;
    if (t0 == 0 && t1 == 16) {
        *(__attribute__((address_space(1))) u32x4*)(QD + r0) = out;
    } else {
        store_edge(QD + r0, out, t0, t1);
    }
}

// Step 5, once every chunk of the group is summed: one lane per parked chunk
// (`slot` 0 / 1 of the packet at QD, misalignment qd, QT bytes) folds the
// packet's sum, puts the field's byte(s) that lie in this chunk, and issues
// the chunk's only store.
__device__ __forceinline__ void finish_parked(const EmitArgs& a, uint32_t fpos, uint32_t slot,
                                              uint32_t qd, uint32_t QT, uint8_t* QD,
                                              const u32x4* parked, const uint32_t* acc) {
    const uint32_t cf = (qd + fpos) >> 4;
    if (slot && ((qd + fpos + 1u) >> 4) == cf) return;  // the field sits in one chunk
    const uint32_t c = cf + slot;
    u32x4 out = *parked;
    if (QT - a.sums.udp_at <= 65535u) {
        const uint32_t f = fold16(*acc);
        uint32_t sum = ~((qd & 1u) ? f : swap16(f)) & 0xffffu;
        sum = sum ? sum : 0xffffu;
        const int32_t pos = (int32_t)(qd + fpos) - (int32_t)(16u * c);
        put_byte(out, pos, sum >> 8);
        put_byte(out, pos + 1, sum & 0xffu);
    }
    store_chunk(QD, (int32_t)(16u * c) - (int32_t)qd, QT, out);
}

}  // namespace
}  // namespace ingot_gpu
