// read.hip — parse_read over chunk lists (ingot_gpu_parse_read*,
// ingot-macros/src/parse.rs:511-537): the k_parse_read kernel with the header
// chunks staged in LDS (SegFrameP) and its launcher; DESIGN.md §1b.  And the
// rewrite over chunk lists (ingot_gpu_parse_read_modify*): k_parse_read_modify
// and its launchers; DESIGN.md §4.11, and §4.16 for per-packet operands
// (ingot_gpu_parse_read_modify_rows).
#include "walk.h"

namespace ingot_gpu {
namespace {

// parse_read over chunk lists with chunk 0 staged (SegFrameP): per tile, the
// packets' chunk bounds and the first four chunks' descriptors are loaded
// together (independent loads), chunk 0 is staged packet-major like a frame
// window (with any later non-final chunk that lies inside that window), then
// the walk — no dependent descriptor or byte load for headers inside staged
// pieces.  One 64-packet tile per wave.  (Staging later chunks in planes, a
// persistent grid with a descriptor lookahead and fewer prefetched
// descriptors all measured slower — DESIGN.md §1b; git history, round 4.)
//
// NPRE (0 or 3): descriptors of chunks 1..NPRE loaded with chunk 0's (when
// not the packet's last); later chunks are looked up when the walk reaches
// them.
//
// FIRST (ingot_gpu_parse_read_first): chunk 0's descriptor comes from the
// per-packet array a.first, indexed by the packet like pkt_seg, so it is
// loaded together with the chunk bounds — one HBM round trip before the
// staging instead of two (pkt_seg, then the chunk table at pkt_seg[i]).
//
// LAZY (with FIRST; INGOT_TUNE_READ_PLAN 17): the chunk bounds are not
// loaded per tile at all — chunk 0 comes from a.first — but by the walk, per
// lane, only when it needs them (SegFrameP::bounds): one descriptor stream
// (8 B per packet) instead of two for packets whose headers lie in chunk 0.
template <int CS0, int CHAIN, int MODE, bool DENSE = false, int NPRE = 3, bool FIRST = false,
          bool LAZY = false>
__global__ __launch_bounds__(BLOCK) void k_parse_read(ParseArgs a) {
    static_assert(!LAZY || (FIRST && NPRE == 0), "lazy bounds: chunk 0 per packet, no prefetch");
    using FR = SegFrameP<CS0, DENSE, NPRE, LAZY>;
    constexpr uint32_t WAVE_DW = WAVE * CS0 * 4u;
    constexpr bool TUN = CHAIN == INGOT_CHAIN_GENEVE_OVER_V6;
    // no slack past the last image: SegFrameP::be clamps the second dword of
    // a pair to the current chunk's staged pieces (a 5-piece image is then
    // exactly 20 KiB per block)
    __shared__ __attribute__((aligned(16))) uint32_t s_win[WAVES * WAVE_DW];
    const uint32_t lane = threadIdx.x & (WAVE - 1u);
    const uint32_t wave = threadIdx.x / WAVE;
    uint32_t* wimg = s_win + wave * WAVE_DW;
    const uint64_t ntiles = (a.n + WAVE - 1u) / WAVE;
    const uint64_t W = (uint64_t)gridDim.x * WAVES;
    uint64_t t = (uint64_t)blockIdx.x * WAVES + wave;
    if (t >= ntiles) return;

    // packet i's chunk bounds (clamped index: always one load pair); LAZY:
    // none yet (FR::kUnknown for a packet of the batch, 0 past its end)
    auto load_pkt = [&](uint64_t tt, uint32_t& s0, uint32_t& ns) {
        uint64_t i = tt * WAVE + lane;
        const bool v = i < a.n;
        if constexpr (LAZY) {
            s0 = 0;
            ns = v ? FR::kUnknown : 0u;
            return;
        }
        if (!v) i = a.n - 1u;
        const uint32_t b0 = a.pkt_seg[i], b1 = a.pkt_seg[i + 1];
        s0 = v ? b0 : 0u;
        ns = v ? b1 - b0 : 0u;
    };
    // chunk 0's descriptor (none for a packet without chunks)
    auto load_d0 = [&](uint32_t s0, uint32_t ns, uint64_t& o0, uint32_t& l0) {
        if constexpr (DENSE) {
            const uint64_t v = ns ? a.off[s0] : 0u;
            o0 = v >> 16;
            l0 = (uint32_t)(v & 0xffffu);
        } else {
            o0 = ns ? a.off[s0] : 0u;
            l0 = ns ? a.len[s0] : 0u;
        }
    };
    // FIRST: chunk 0's (offset << 16) | length of packet tt's lane, loaded
    // beside its bounds (clamped index: always one load)
    auto load_first = [&](uint64_t tt, uint32_t ns, uint64_t& o, uint32_t& l) {
        uint64_t i = tt * WAVE + lane;
        if (i >= a.n) i = a.n - 1u;
        const uint64_t v = a.first[i];
        o = ns ? v >> 16 : 0u;  // (LAZY: ns is kUnknown for every packet of the batch)
        l = ns ? (uint32_t)(v & 0xffffu) : 0u;
    };
    uint32_t s0, nseg;
    uint64_t o0;
    uint32_t l0;
    load_pkt(t, s0, nseg);
    if constexpr (FIRST) load_first(t, nseg, o0, l0);
    else load_d0(s0, nseg, o0, l0);

    for (;;) {
        const uint64_t i = t * WAVE + lane;
        const bool valid = i < a.n;
        FR fr;
        fr.o0 = o0;
        fr.l0 = l0;
        if constexpr (DENSE) {
            // one 8-B entry per chunk: (offset << 16) | length; chunks 1..3
            // only when not the packet's last (SegFrameP::advance)
            const uint64_t v1 = nseg > 2 ? a.off[s0 + 1] : 0u;
            const uint64_t v2 = nseg > 3 ? a.off[s0 + 2] : 0u;
            const uint64_t v3 = nseg > 4 ? a.off[s0 + 3] : 0u;
            fr.o1 = v1 >> 16;
            fr.o2 = v2 >> 16;
            fr.o3 = v3 >> 16;
            fr.l1 = (uint32_t)(v1 & 0xffffu);
            fr.l2 = (uint32_t)(v2 & 0xffffu);
            fr.l3 = (uint32_t)(v3 & 0xffffu);
        } else {
            fr.o1 = NPRE >= 1 && nseg > 2 ? a.off[s0 + 1] : 0u;
            fr.o2 = NPRE >= 2 && nseg > 3 ? a.off[s0 + 2] : 0u;
            fr.o3 = NPRE >= 3 && nseg > 4 ? a.off[s0 + 3] : 0u;
            fr.l1 = NPRE >= 1 && nseg > 2 ? a.len[s0 + 1] : 0u;
            fr.l2 = NPRE >= 2 && nseg > 3 ? a.len[s0 + 2] : 0u;
            fr.l3 = NPRE >= 3 && nseg > 4 ? a.len[s0 + 3] : 0u;
        }
        // chunk 0, packet-major: instruction k, lane L fills slot 64k + L =
        // packet q / CS0, piece (q mod CS0) ^ swz (walk.h's chunk_of, spelt
        // out below: through the helper three of the tunnel's field-mode
        // kernels come out with other registers; 16-B aligned absolute
        // addresses; pieces only below the chunk's end).  Records never read
        // the MAC addresses (the walk reads Ethernet's ethertype only), so, as
        // in k_parse, the window starts at the piece holding chunk 0's byte
        // SKIP = 12: a frame starting in the last 12 bytes of a 128-B line
        // does not fetch that line.  Staged byte sh0 + j is chunk-0 byte
        // SKIP + j.
        constexpr uint32_t SKIP = MODE == OUT_REC16 ? INGOT_REC_SKIP : 0u;
        const uint32_t sh0 = (uint32_t)((uintptr_t)(a.arena + fr.o0 + SKIP) & 15u);
        const int64_t base0 = (int64_t)fr.o0 + (int64_t)SKIP - (int64_t)sh0;
        // chunk 0's window: CS0 pieces, or (a.linewin = m) a line-completing
        // window — at least m pieces, then to the end of that 128-B line
        // (k_parse's windows), at most CS0
        uint32_t want = CS0;
        if (a.linewin) {
            const uint32_t lp = (uint32_t)((uintptr_t)(a.arena + base0) >> 4) & 7u;
            want = ((lp + a.linewin + 7u) & ~7u) - lp;
            if (want > (uint32_t)CS0) want = CS0;
        }
        const uint32_t wlim = 16u * want;
        // the window's end in staged bytes: chunk 0's end, or the window's
        // (nothing when chunk 0 ends before byte SKIP)
        const int64_t e0 = (int64_t)sh0 + (int64_t)fr.l0 - (int64_t)SKIP;
        uint32_t ext = nseg && e0 > 0 ? (e0 < (int64_t)wlim ? (uint32_t)e0 : wlim) : 0u;
        // a later non-last chunk that starts inside chunk 0's window: stage
        // the window's pieces up to its end (or the window's)
        auto widen = [&](uint32_t e, uint64_t o, uint32_t l) {
            const int64_t d = (int64_t)o - base0;
            if (e + 1 < nseg && d >= 0 && d < (int64_t)wlim) {
                const uint32_t end = (uint32_t)d + l < wlim ? (uint32_t)d + l : wlim;
                ext = end > ext ? end : ext;
            }
        };
        if constexpr (NPRE >= 1) widen(1, fr.o1, fr.l1);
        if constexpr (NPRE >= 2) widen(2, fr.o2, fr.l2);
        if constexpr (NPRE >= 3) widen(3, fr.o3, fr.l3);
        const uint32_t n0 = (ext + 15u) >> 4;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)CS0; ++k) {
            const uint32_t q = k * WAVE + lane;
            const uint32_t pp = q / CS0;
            const uint32_t c = (q - pp * CS0) ^ swz<CS0>(pp);
            const uint32_t np = (uint32_t)__shfl((int)n0, (int)pp);
            const int64_t bp = (int64_t)__shfl((long long)base0, (int)pp);
            if (c < np) stage16(a.arena + bp + 16u * c, wimg + k * WAVE * 4u, false);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

        fr.win = (const lds_u32*)wimg;
        fr.p = lane;
        fr.arena = a.arena;
        fr.seg_off = a.off;
        fr.seg_len = a.len;
        fr.s0 = s0;
        fr.k = 0;
        fr.nseg = nseg;
        fr.pkt_seg = a.pkt_seg;
        fr.pi = i;
        fr.L = 0;
        fr.b0 = base0;
        fr.span0 = 16u * n0;
        fr.enter(fr.o0, fr.l0, nseg ? want : 0u);
        if constexpr (SKIP != 0) {
            // chunk-0 byte i >= SKIP is staged byte i + sh0 - SKIP (mod 2^32);
            // bytes [0, avail) count as staged (those below SKIP are never read)
            fr.sh = sh0 - SKIP;
            const uint32_t w0 = 16u * want + SKIP - sh0;
            fr.avail = nseg ? (fr.l0 < w0 ? fr.l0 : w0) : 0u;
        }
        Rec r;
        if constexpr (MODE == OUT_FIELDS) {
            using OutT = typename std::conditional<TUN, ingot_geneve_fields, ingot_fields>::type;
            OutT* G = static_cast<OutT*>(a.out) + (valid ? i : 0);
            if (valid) {
                uint4* z = reinterpret_cast<uint4*>(G);
#pragma unroll
                for (int k = 0; k < (int)(sizeof(OutT) / 16); ++k) st_global(z + k, make_uint4(0, 0, 0, 0));
                ingot_fields* F;
                ingot_tunnel_fields* T = nullptr;
                if constexpr (TUN) {
                    F = &G->inner;
                    T = &G->outer;
                } else {
                    F = G;
                }
                walk<CHAIN, true>(fr, r, F, T);
                st_global(reinterpret_cast<uint4*>(F), pack(r));
            }
        } else {
            walk<CHAIN, false>(fr, r, nullptr, nullptr);
            if (valid) store_rec(static_cast<uint4*>(a.out) + i, pack(r), a.policy);
        }
        if (valid && a.chunk) a.chunk[i] = (uint16_t)fr.k;
        // the next tile's LDS-DMA overwrites this image: every lane's reads
        // above have returned (their values were consumed by the stores)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        t += W;
        if (t >= ntiles) break;
        load_pkt(t, s0, nseg);
        if constexpr (FIRST) load_first(t, nseg, o0, l0);
        else load_d0(s0, nseg, o0, l0);
    }
}

// The rewrite over chunk lists: the frame view the shared setters and checksum
// update (walk.h: apply_edit, csum_finish — unchanged, one copy) read through
// after the walk, and where their bytes go.
// Offsets are the record's logical offsets (the chunks concatenated); logical
// byte x lies in the chunk k with start_k <= x < start_k + len_k, start_k the
// sum of the earlier chunks' lengths (an empty chunk holds no byte and its
// offset is never used).  The chunk is found by walking the lengths from the
// one found last — chunks 0..3 from the walk's registers (1..3 only when not
// the packet's last, as prefetched), later ones from the table, never past the
// packet's last chunk — and from chunk 0 again when x lies before it.
// Every byte is read from and stored to global memory, so an edit sees what
// the earlier edits of its packet wrote; nothing is staged or written back in
// wider units, so no byte outside an edited field or checksum field is stored
// to.  A header parse_read accepted lies in one chunk; bytes that would
// reach past the chunk found (never the case for an Ok record) read as 0 and
// are not stored.
template <class SF>
struct ChunkView {
    const SF& f;  // the walk's view, after the walk
    mutable uint32_t ck = 0, cstart = 0, clen;
    mutable uint64_t coff;
    __device__ __forceinline__ explicit ChunkView(const SF& s) : f(s), clen(s.l0), coff(s.o0) {}

    // the chunk holding logical bytes [x, x + n); false: none does
    __device__ __forceinline__ bool locate(uint32_t x, uint32_t n) const {
        if (x < cstart) {
            ck = 0;
            cstart = 0;
            clen = f.l0;
            coff = f.o0;
        }
        while (x - cstart >= clen) {
            if (ck + 1u >= f.nseg) return false;
            cstart += clen;
            ++ck;
            const bool pre = ck + 1u < f.nseg;  // a prefetched descriptor is valid
            if (pre && ck == 1u) {
                coff = f.o1;
                clen = f.l1;
            } else if (pre && ck == 2u) {
                coff = f.o2;
                clen = f.l2;
            } else if (pre && ck == 3u) {
                coff = f.o3;
                clen = f.l3;
            } else {
                coff = gbl(f.seg_off)[f.s0 + ck];
                clen = gbl(f.seg_len)[f.s0 + ck];
            }
        }
        return x - cstart + n <= clen;
    }
    __device__ __forceinline__ uint32_t be(uint32_t i, uint32_t n) const {
        uint32_t v = 0;
        if (locate(i, n)) {
            const auto* gg = gbl(f.arena) + coff + (i - cstart);
            for (uint32_t j = 0; j < n; ++j) v = (v << 8) | gg[j];
        }
        return v;
    }
    __device__ __forceinline__ uint32_t be_edited(uint32_t i, uint32_t n) const { return be(i, n); }
    __device__ __forceinline__ uint32_t get_edited(uint32_t hdr, Field fl) const {
        return (be(hdr + fl.byte0(), fl.nbytes()) >> fl.rshift()) & fl.mask();
    }
};

// The edit sink of a chunked packet: walk.h's put_byte for this view (the more
// specialised overload, found by the shared apply_edit through its frame
// argument).  One byte store into the chunk that holds the byte; the
// EditSink, the contiguous kernels' write-back bookkeeping, is not used.
template <class SF>
__device__ __forceinline__ void put_byte(const ChunkView<SF>& f, EditSink&, uint32_t i,
                                         uint8_t v) {
    if (f.locate(i, 1u))
        gbl_mut(const_cast<uint8_t*>(f.f.arena))[f.coff + (i - f.cstart)] = v;
}

// The whole-byte SET of the rows kernel (ingot_gpu_parse_read_modify_rows): a
// piece with op SET, rshift 0 and bits = 8 * nbytes replaces its covering bytes
// outright — every piece of a MAC or IPv6 address, the 16- and 32-bit narrow
// SETs, the hop limit.  Through apply_edit such a piece costs nbytes located
// byte loads and nbytes located byte stores; here the chunk is located once
// (by the caller), the old bytes are loaded only when a selected sum covers
// them, and a piece whose address is a multiple of its size goes out as one
// store.  The loads and stores go through gbl / gbl_mut like the byte path's
// and their types may alias anything, so a later edit of the packet and
// csum_finish read what was stored here.  Returns apply_edit<true>'s term.
// INGOT_READ_ROWS_FAST_SET 0 compiles the path out (every piece through
// apply_edit: the A/B of DESIGN.md §4.16; not a tuning knob).
#ifndef INGOT_READ_ROWS_FAST_SET
#define INGOT_READ_ROWS_FAST_SET 1
#endif
typedef __attribute__((address_space(1), may_alias)) uint16_t g_u16;
typedef __attribute__((address_space(1), may_alias)) uint32_t g_u32;

__device__ __forceinline__ bool whole_byte_set(const Edit& e) {
    return e.op == INGOT_OP_SET && e.rshift == 0u && e.bits == 8u * e.nbytes;
}

// `f` has located logical bytes [at, at + e.nbytes) in one chunk.
template <class SF>
__device__ __forceinline__ uint32_t set_located(const ChunkView<SF>& f, uint32_t at,
                                                const Edit& e, bool fed) {
    const uint32_t n = e.nbytes;
    uint8_t* p = const_cast<uint8_t*>(f.f.arena) + f.coff + (at - f.cstart);
    const uint32_t w_new = n >= 4u ? e.value : e.value & ((1u << (8u * n)) - 1u);
    const bool whole = (n == 4u || n == 2u) && ((uintptr_t)p & (n - 1u)) == 0u;
    uint32_t w_old = 0;
    // (the wide types are put on after gbl / gbl_mut: a template argument
    // drops may_alias)
    if (whole && n == 4u) {
        if (fed) w_old = __builtin_bswap32(*reinterpret_cast<const g_u32*>(gbl(p)));
        *reinterpret_cast<g_u32*>(gbl_mut(p)) = __builtin_bswap32(w_new);
    } else if (whole) {
        if (fed) w_old = __builtin_bswap32(*reinterpret_cast<const g_u16*>(gbl(p))) >> 16;
        *reinterpret_cast<g_u16*>(gbl_mut(p)) = (uint16_t)(__builtin_bswap32(w_new) >> 16);
    } else {
        if (fed)
            for (uint32_t j = 0; j < n; ++j) w_old = (w_old << 8) | gbl(p)[j];
        for (uint32_t j = 0; j < n; ++j) gbl_mut(p)[j] = (uint8_t)(w_new >> (8u * (n - 1u - j)));
    }
    return fed ? csum_term(at, n, w_old, w_new) : 0u;
}

// One piece of the rows kernel: the located SET above, or the shared setter.
template <class SF>
__device__ __forceinline__ uint32_t rows_edit(const ChunkView<SF>& f, EditSink& sink, uint32_t h,
                                              const Edit& e, uint32_t feeds) {
#if INGOT_READ_ROWS_FAST_SET
    if (whole_byte_set(e) && f.locate(h + e.byte0, e.nbytes))
        return set_located(f, h + e.byte0, e, feeds != 0u);
#endif
    return apply_edit<true>(f, sink, h, e);
}

// The rewrite over chunk lists (ingot_gpu_parse_read_modify, ARGS = ModifyArgs;
// ingot_gpu_parse_read_modify_csum, ARGS = ModifyCsumArgs): k_parse_read's
// record path over the CSR tables (three prefetched descriptors, the window
// from byte 12), then ingot's setters at the record's logical offsets and,
// with ModifyCsumArgs, the RFC 1624 update of the selected sums.
//
// The staging is k_parse_read's, line for line, in a kernel of its own: a
// body shared through a helper (tried both with the LDS image declared in the
// kernels and in the helper) gave five of k_parse_read's dense-table kernels
// other registers, and those kernels keep the instructions they were measured
// with.
//
// After the walk nothing is read from the LDS image again.  The setters and
// the checksum update read and store the few bytes they touch in global
// memory through ChunkView (above) — the lines are in L2 from the staging —
// so an edit sees what earlier edits of the packet wrote (a field edited
// twice, a checksum field set by an edit and then updated), and every store
// is a byte store inside the one chunk that holds the header: no neighbouring
// byte, which may belong to a packet another lane is editing, is written.
//
// ARGS = ModifyRowsArgs (ingot_gpu_parse_read_modify_rows): each piece's
// operand from a device table, by packet or by the packet's row, behind the
// row guard, as in k_parse's rows mode; `what` is a run-time value (0: no sum
// is touched), so there is one kernel per window and chain.  Whole-byte SET
// pieces take rows_edit's located path (above): their stores are 1, 2 or 4
// bytes wide and still lie inside the field they write.
template <int CS0, int CHAIN, class ARGS>
__global__ __launch_bounds__(BLOCK) void k_parse_read_modify(ARGS args) {
    constexpr bool ROWS = std::is_same<ARGS, ModifyRowsArgs>::value;
    constexpr bool CSUM = std::is_same<ARGS, ModifyCsumArgs>::value;
    const ParseArgs& a = base_args(args);
    using FR = SegFrameP<CS0, false, 3, false>;
    constexpr uint32_t WAVE_DW = WAVE * CS0 * 4u;
    __shared__ __attribute__((aligned(16))) uint32_t s_win[WAVES * WAVE_DW];
    const uint32_t lane = threadIdx.x & (WAVE - 1u);
    const uint32_t wave = threadIdx.x / WAVE;
    uint32_t* wimg = s_win + wave * WAVE_DW;
    const uint64_t ntiles = (a.n + WAVE - 1u) / WAVE;
    const uint64_t W = (uint64_t)gridDim.x * WAVES;

    for (uint64_t t = (uint64_t)blockIdx.x * WAVES + wave; t < ntiles; t += W) {
        const uint64_t i = t * WAVE + lane;
        const bool valid = i < a.n;
        // the packet's chunk bounds (clamped index) and descriptors 0..3
        // (1..3 only when not the packet's last: SegFrameP::advance)
        const uint64_t ic = valid ? i : a.n - 1u;
        const uint32_t b0 = a.pkt_seg[ic], b1 = a.pkt_seg[ic + 1];
        const uint32_t s0 = valid ? b0 : 0u;
        const uint32_t nseg = valid && b1 > b0 ? b1 - b0 : 0u;
        FR fr;
        fr.o0 = nseg ? a.off[s0] : 0u;
        fr.l0 = nseg ? a.len[s0] : 0u;
        fr.o1 = nseg > 2 ? a.off[s0 + 1] : 0u;
        fr.o2 = nseg > 3 ? a.off[s0 + 2] : 0u;
        fr.o3 = nseg > 4 ? a.off[s0 + 3] : 0u;
        fr.l1 = nseg > 2 ? a.len[s0 + 1] : 0u;
        fr.l2 = nseg > 3 ? a.len[s0 + 2] : 0u;
        fr.l3 = nseg > 4 ? a.len[s0 + 3] : 0u;
        // ROWS: the packet's row, loaded with the descriptors so that the
        // gather of its table rows does not wait for two dependent round
        // trips; the row guard is part of "edit this packet" (k_parse's)
        [[maybe_unused]] uint32_t row = 0;
        [[maybe_unused]] bool edit = valid;
        if constexpr (ROWS) {
            if (valid && args.row) {
                row = args.row[i];
                edit = row < args.n_rows;  // INGOT_ROW_NONE too
            }
        }
        // chunk 0's window from the piece holding its byte SKIP, packet-major
        // (k_parse_read's staging)
        constexpr uint32_t SKIP = INGOT_REC_SKIP;
        const uint32_t sh0 = (uint32_t)((uintptr_t)(a.arena + fr.o0 + SKIP) & 15u);
        const int64_t base0 = (int64_t)fr.o0 + (int64_t)SKIP - (int64_t)sh0;
        uint32_t want = CS0;
        if (a.linewin) {
            const uint32_t lp = (uint32_t)((uintptr_t)(a.arena + base0) >> 4) & 7u;
            want = ((lp + a.linewin + 7u) & ~7u) - lp;
            if (want > (uint32_t)CS0) want = CS0;
        }
        const uint32_t wlim = 16u * want;
        const int64_t e0 = (int64_t)sh0 + (int64_t)fr.l0 - (int64_t)SKIP;
        uint32_t ext = nseg && e0 > 0 ? (e0 < (int64_t)wlim ? (uint32_t)e0 : wlim) : 0u;
        auto widen = [&](uint32_t e, uint64_t o, uint32_t l) {
            const int64_t d = (int64_t)o - base0;
            if (e + 1 < nseg && d >= 0 && d < (int64_t)wlim) {
                const uint32_t end = (uint32_t)d + l < wlim ? (uint32_t)d + l : wlim;
                ext = end > ext ? end : ext;
            }
        };
        widen(1, fr.o1, fr.l1);
        widen(2, fr.o2, fr.l2);
        widen(3, fr.o3, fr.l3);
        const uint32_t n0 = (ext + 15u) >> 4;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)CS0; ++k) {
            const auto [pp, c] = chunk_of<CS0>(k, lane);
            const uint32_t np = (uint32_t)__shfl((int)n0, (int)pp);
            const int64_t bp = (int64_t)__shfl((long long)base0, (int)pp);
            if (c < np) stage16(a.arena + bp + 16u * c, wimg + k * WAVE * 4u, false);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

        fr.win = (const lds_u32*)wimg;
        fr.p = lane;
        fr.arena = a.arena;
        fr.seg_off = a.off;
        fr.seg_len = a.len;
        fr.s0 = s0;
        fr.k = 0;
        fr.nseg = nseg;
        fr.pkt_seg = a.pkt_seg;
        fr.pi = i;
        fr.L = 0;
        fr.b0 = base0;
        fr.span0 = 16u * n0;
        fr.enter(fr.o0, fr.l0, nseg ? want : 0u);
        fr.sh = sh0 - SKIP;
        const uint32_t w0 = 16u * want + SKIP - sh0;
        fr.avail = nseg ? (fr.l0 < w0 ? fr.l0 : w0) : 0u;

        Rec r;
        walk<CHAIN, false>(fr, r, nullptr, nullptr);
        // the image is not read below: the next tile's LDS-DMA may overwrite
        // it once every lane's reads above have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (valid && a.out) store_rec(static_cast<uint4*>(a.out) + i, pack(r), a.policy);
        if (valid && a.chunk) a.chunk[i] = (uint16_t)fr.k;
        // the setters, in order, on packets parsed Ok (no store for any
        // other packet, nor for lanes past n)
        if (edit && r.status == INGOT_OK) {
            const ChunkView<FR> cv(fr);
            EditSink sink{};  // (unused by this view's put_byte)
            [[maybe_unused]] typename std::conditional<CSUM || ROWS, CsumAcc, NoCsum>::type acc;
            if constexpr (ROWS) {
                for (uint32_t k = 0; k < args.n_pieces; ++k) {
                    const RowPiece& pc = args.e[k];
                    Edit e = pc.e;
                    uint32_t h;
                    // (no table is read for a piece that is not applied)
                    if (header_at<CHAIN>(r, e.layer, e.kind, e.index, h)) {
                        e.value = row_operand(pc, pc.by == INGOT_BY_ROW ? (uint64_t)row : i);
                        csum_feed(acc, pc.feeds, r, rows_edit(cv, sink, h, e, pc.feeds));
                    }
                }
                if (args.what)
                    csum_finish<CHAIN>(cv, r, args.what, acc,
                                       [&](uint32_t at, uint8_t v) { put_byte(cv, sink, at, v); });
            } else {
                const ModifyArgs& m = edit_args(args);
                for (uint32_t k = 0; k < m.n_edits; ++k) {
                    const Edit e = m.e[k];
                    uint32_t h;
                    if (header_at<CHAIN>(r, e.layer, e.kind, e.index, h)) {
                        if constexpr (CSUM)
                            csum_feed(acc, args.feeds[k], r, apply_edit<true>(cv, sink, h, e));
                        else
                            apply_edit(cv, sink, h, e);
                    }
                }
                if constexpr (CSUM)
                    csum_finish<CHAIN>(cv, r, args.what, acc, [&](uint32_t at, uint8_t v) {
                        put_byte(cv, sink, at, v);
                    });
            }
        }
    }
}

// The rewrite's launcher: parse_read's chunk-0 window (launch_segmented below:
// INGOT_TUNE_READ_PLAN 1, or an arena in mapped host memory, = 4 pieces; else
// the line-completing 3 to 5), its record stores and its grid.
template <class ARGS>
ParseArgs& tables_of(ARGS& a) {
    return edit_args(a).p;
}
ParseArgs& tables_of(ModifyRowsArgs& a) { return a.p; }  // (no ModifyArgs inside)

template <class ARGS>
hipError_t launch_read_modify_as(const ARGS& args, int chain, const Tuning& t, hipStream_t s) {
    ARGS b = args;
    ParseArgs& p = tables_of(b);
    if (p.n == 0) return hipSuccess;
    p.policy = t.cache_policy == 0 ? 2u : (uint32_t)t.cache_policy & 0x1fbu;  // launch_parse's
    const uint32_t g = grid_for(p.n, t.max_blocks);
    const bool four = t.read_plan == 1 || (t.read_plan == 0 && t.host_arena);
    if (!four) p.linewin = 3u;
    with_chain<INGOT_CHAIN_GENEVE_OVER_V6>(chain, [&](auto c) {
        if (four)
            hipLaunchKernelGGL((k_parse_read_modify<4, decltype(c)::value, ARGS>), dim3(g),
                               dim3(BLOCK), 0, s, b);
        else
            hipLaunchKernelGGL((k_parse_read_modify<5, decltype(c)::value, ARGS>), dim3(g),
                               dim3(BLOCK), 0, s, b);
    });
    return hipGetLastError();
}

template <int CS0, int MODE, bool DENSE = false, int NPRE = 3, bool FIRST = false,
          bool LAZY = false>
hipError_t launch_read(const ParseArgs& a, int chain, uint32_t g, hipStream_t s) {
    // any other tag is the tunnel
    with_chain<INGOT_CHAIN_GENEVE_OVER_V6>(chain, [&](auto c) {
        hipLaunchKernelGGL((k_parse_read<CS0, decltype(c)::value, MODE, DENSE, NPRE, FIRST, LAZY>),
                           dim3(g), dim3(BLOCK), 0, s, a);
    });
    return hipGetLastError();
}

}  // namespace

hipError_t launch_read_modify(const ModifyArgs& a, int chain, const Tuning& t, hipStream_t s) {
    return launch_read_modify_as(a, chain, t, s);
}

hipError_t launch_read_modify_csum(const ModifyCsumArgs& a, int chain, const Tuning& t,
                                   hipStream_t s) {
    return launch_read_modify_as(a, chain, t, s);
}

hipError_t launch_read_modify_rows(const ModifyRowsArgs& a, int chain, const Tuning& t,
                                   hipStream_t s) {
    return launch_read_modify_as(a, chain, t, s);
}

// parse_read over chunk lists.  Measured (tools/abtune.py, us per launch,
// DESIGN.md §1b): the reference's one-header-per-chunk shape (c2r, 1 M) 33.3
// with descriptors and bytes on demand / 25.1 with chunk 0 in 4 pieces /
// 24.2 with later chunks in planes {2,2,2,0}; header + payload chunks (c3r,
// 16.7 M) 651 / 667 / 681 — extra planes cost occupancy on the
// gather-bound shape.  Default (round 2): chunk 0 in a line-completing window
// of 3 to 5 pieces (to the end of the 128-B line its third piece lies in;
// k_parse's windows): c3r 676 -> 651 us, c2r 23.05 -> 23.24.
// INGOT_TUNE_READ_PLAN 1 = the round-1 4-piece window (the default for chunk
// pools in mapped host memory, where every staged piece is a PCIe read).
hipError_t launch_segmented(const ParseArgs& a, int chain, int mode, const Tuning& t,
                            uint32_t g, hipStream_t s) {
    if (mode != OUT_FIELDS && mode != OUT_REC16) return hipErrorInvalidValue;
    // dense chunk table (ingot_gpu_parse_read_dense): no length array, one
    // (offset << 16) | length entry per chunk; 4 pieces of chunk 0 (the
    // knob does not apply)
    if (!a.len)
        return mode == OUT_FIELDS ? launch_read<4, OUT_FIELDS, true>(a, chain, g, s)
                                  : launch_read<4, OUT_REC16, true>(a, chain, g, s);
    // chunk 0's descriptor per packet (ingot_gpu_parse_read_first): loaded
    // beside the bounds; 17 = the bounds loaded lazily by the walk
    if (a.first) {
        if (mode == OUT_FIELDS)
            return launch_read<4, OUT_FIELDS, false, 3, true>(a, chain, g, s);
        if (t.host_arena || t.read_plan == 1)
            return launch_read<4, OUT_REC16, false, 3, true>(a, chain, g, s);
        ParseArgs b = a;
        b.linewin = 3u;
        if (t.read_plan == 17)
            return launch_read<5, OUT_REC16, false, 0, true, true>(b, chain, g, s);
        return launch_read<5, OUT_REC16, false, 3, true>(b, chain, g, s);
    }
    if (mode == OUT_FIELDS) return launch_read<4, OUT_FIELDS>(a, chain, g, s);
    if (t.read_plan == 1 || (t.read_plan == 0 && t.host_arena))
        return launch_read<4, OUT_REC16>(a, chain, g, s);
    ParseArgs b = a;  // 0 / 11 / 17 (17 applies to parse_read_first only)
    b.linewin = 3u;
    return launch_read<5, OUT_REC16>(b, chain, g, s);
}

}  // namespace ingot_gpu
