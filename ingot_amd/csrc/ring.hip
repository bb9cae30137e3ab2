// ring.hip — the slot-ring kernels: k_parse_pipe (one batch per launch,
// the next tile's LDS-DMA in flight while a wave parses one), k_parse_ring
// (the persistent ring consumer, ingot_gpu_parse_ring: many batches per
// launch behind an in-kernel doorbell) and k_modify_pipe (parse + setters in
// place); DESIGN.md §4, §1c.
#include "walk.h"

namespace ingot_gpu {
namespace {

// A wave-uniform 64-bit value the compiler computed in VGPRs (a 64-bit
// division has no scalar form), moved to an SGPR pair.
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    // (pinned: a readfirstlane of a value known to be uniform folds away and
    // leaves the VGPR pair)
    asm volatile("" : "+s"(lo), "+s"(hi));
    return ((uint64_t)hi << 32) | lo;
}

// Pipelined variant for fixed slots with no length array (C2-style rings):
// each wave walks several tiles and keeps the next DEPTH-1 tiles' LDS-DMA in
// flight while it parses the current one (DEPTH LDS images per wave, used
// round robin).  DEPTH 1: a single image, restaged once the walk has read it.
// Requires stride >= 16*NCH.
// POL != 0: the cache-policy word fixed at compile time (the launcher's
// defaults), so the staging loads and record stores carry their cache bits
// directly instead of the runtime policy switch around every instruction
// (a tree of scalar branches per chunk); 0 = a.policy at run time.
template <uint32_t NCH, uint32_t DEPTH, int CHAIN, int MODE, uint32_t POL = 0>
__global__ __launch_bounds__(BLOCK) void k_parse_pipe(ParseArgs a) {
    using Img = RingImg<NCH, DEPTH>;
    const uint32_t pol = POL ? POL : a.policy;
    __shared__ __attribute__((aligned(16))) uint32_t s_img[Img::DW];
    constexpr uint32_t REC_B = MODE == OUT_REC8 ? 8u : 16u;
    const uint32_t lane = threadIdx.x & (WAVE - 1u);
    // wave-uniform (readfirstlane, as in k_parse_ring): the tile cursor, the
    // tile's source and record bases and the loop control stay in SGPRs, and
    // the staging instructions' LDS destinations (M0) are loop constants
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    uint32_t* img0 = s_img + wave * Img::WAVE_DW;
    const uint64_t ntiles = (a.n + WAVE - 1u) / WAVE;
    // only the batch's last tile can hold slots >= n (none if 64 divides n)
    const uint64_t ttail = a.n % WAVE ? ntiles - 1u : ~0ull;
    const uint32_t tail_last = (uint32_t)((a.n - 1u) % WAVE);  // its last valid lane

    // Tile order (INGOT_TUNE_XCD_REMAP).  Bit 0: block b runs on XCD b % 8;
    // renumbered (b % 8) * G/8 + b / 8 ("XCD-major"), each XCD's blocks take
    // a contiguous eighth of every round of G x WAVES tiles instead of every
    // eighth block's tiles.  Bit 1: each wave walks a contiguous run of
    // tiles (wave w: tiles w*J .. w*J + J-1) instead of striding by the grid.
    uint32_t bid = blockIdx.x;
    if ((a.xcd_remap & 1u) && gridDim.x % 8u == 0u)
        bid = (bid % 8u) * (gridDim.x / 8u) + bid / 8u;
    const uint64_t gw = (uint64_t)bid * WAVES + wave;  // this wave's index in the grid
    const uint64_t nw = (uint64_t)gridDim.x * WAVES;
    uint64_t t, step, tend;
    if ((a.xcd_remap & 4u) && gridDim.x % 8u == 0u) {
        // bit 2: the batch in 8 contiguous regions, one per XCD, the XCD's
        // waves striding through its region
        const uint64_t x = blockIdx.x % 8u;
        const uint64_t nwx = (uint64_t)(gridDim.x / 8u) * WAVES;
        const uint64_t region = (ntiles + 7u) / 8u;
        t = x * region + (uint64_t)(blockIdx.x / 8u) * WAVES + wave;
        tend = (x + 1u) * region < ntiles ? (x + 1u) * region : ntiles;
        step = nwx;
    } else if (a.xcd_remap & 2u) {
        const uint64_t J = (ntiles + nw - 1u) / nw;
        t = gw * J;
        tend = t + J < ntiles ? t + J : ntiles;
        step = 1u;
    } else {
        t = gw;
        tend = ntiles;
        step = nw;
    }
    t = uniform64(t);
    step = uniform64(step);
    tend = uniform64(tend);
    if (t >= tend) return;
    // The tile loop, once for 64-B slots (S64) and once for every other
    // stride (a wave-uniform choice).  A tile's staging addresses are a
    // scalar base (arena + t * 64 * stride, advanced by a constant per tile)
    // plus a per-lane 32-bit offset that is the same in every tile: chunk
    // instruction k covers packets 16k .. 16k+15 of the tile, lane L chunk
    // (L % 4) ^ swz of packet 16k + L/4.  S64: swz(16k + L/4) = (L >> 4) & 3
    // for every k, so the four instructions differ by 16 * stride = 1 KiB in
    // the source and by 1 KiB in the image, which is the instruction's
    // immediate offset (added to both).  Otherwise: four offsets in VGPRs.
    auto run = [&](auto s64) {
        constexpr bool S64 = decltype(s64)::value;
        static_assert(!S64 || NCH == 4, "the immediate-offset form is NCH == 4's");
        const uint32_t stride = S64 ? 64u : a.stride;
        const uint32_t take = stride < Img::WIN ? stride : Img::WIN;
        uint32_t voff[NCH];
#pragma unroll
        for (uint32_t k = 0; k < NCH; ++k) {
            const ChunkOf m = chunk_of<NCH>(k, lane);
            voff[k] = m.pp * stride + 16u * m.c;
        }
        const uint32_t frame_off = lane * stride;  // the lane's frame in its tile
        const uint32_t rec_off = lane * REC_B;     // and its record
        const uint64_t tile_b = (uint64_t)WAVE * stride;
        const uint64_t dsrc = step * tile_b;  // per step of the tile cursor
        const uint64_t dout = step * (WAVE * REC_B);

        // Tile tt, its first slot at src, into img.  The empty asm keeps each
        // offset a 32-bit VGPR at the point of use: hoisted out of the loop
        // as a zero-extended pair, it costs a second register and the
        // instruction loses its scalar-base form (a 64-bit add per chunk).
        auto stage = [&](uint64_t tt, const uint8_t* src, uint32_t* img) {
            if (tt == ttail) {
                // slots >= n of the tail tile: a valid address (the last slot)
                uint32_t l = lane;
                asm volatile("" : "+v"(l));
                stage_clamped<NCH>(l, 0u, tail_last + 1u, [&](uint32_t k, uint32_t slot, uint32_t c) {
                    stage16p(src + (slot * stride + 16u * c), img + k * WAVE * 4u, pol);
                });
            } else if constexpr (S64) {
                uint32_t vo = voff[0];
                asm volatile("" : "+v"(vo));
                stage16p<0>(src + vo, img, pol);
                stage16p<1024>(src + vo, img, pol);
                stage16p<2048>(src + vo, img, pol);
                stage16p<3072>(src + vo, img, pol);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < NCH; ++k) {
                    uint32_t vo = voff[k];
                    asm volatile("" : "+v"(vo));
                    stage16p(src + vo, img + k * WAVE * 4u, pol);
                }
            }
        };
        // The lane's view of tile tt staged in img.  Bytes past the window
        // are read through fr.g; a 64-B slot has none (the window is the
        // whole slot, and every read is bounds-checked against len = 64), so
        // no pointer is formed for it.  A tail tile's lanes past n hold the
        // last slot's bytes and point at it.
        auto frame = [&](uint64_t tt, const uint8_t* src, const uint32_t* img) {
            const uint8_t* g = nullptr;
            if constexpr (!S64)
                g = src + (tt == ttail && lane > tail_last ? tail_last * stride : frame_off);
            return Frame<NCH>{(const lds_u32*)img, lane, 0u, take, stride, g};
        };
        // record of tile tt, whose first record is at dst
        auto emit = [&](uint64_t tt, uint8_t* dst, const Rec& r) {
            if (tt == ttail && lane > tail_last) return;
            if constexpr (MODE == OUT_REC8) store_rec(dst, rec_off, pack8(r), pol);
            else store_rec(dst, rec_off, pack(r), pol);
        };

        const uint8_t* src = a.arena + t * tile_b;  // tile t's first slot
        uint8_t* dst = static_cast<uint8_t*>(a.out) + t * (WAVE * REC_B);  // and record
        if constexpr (DEPTH == 1) {
            // One image per wave (16.4 KiB per block instead of 32.9): the
            // next tile is staged into the image just parsed, between the
            // walk and the record store, so its loads fly during the pack,
            // the store and the loop overhead only.  Alone on the device it
            // is the slower kernel; beside an overlapping launch on a second
            // stream it is the faster one, at half the LDS per block
            // (DESIGN.md §4.2).
            stage(t, src, img0);
            // the first tile's loads are the youngest vector-memory operations
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (;;) {
                Frame<NCH> fr = frame(t, src, img0);
                Rec r;
                walk<CHAIN, false>(fr, r, nullptr, nullptr);
                // every lane's LDS reads of the image have returned before it
                // is restaged (the walk of every chain reads it
                // data-dependently, so not before the walk is over; bytes
                // past the window come from fr.g and are unaffected) —
                // k_modify_pipe's rule
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                const uint64_t tn = t + step;
                const bool more = tn < tend;
                if (more) stage(tn, src + dsrc, img0);
                emit(t, dst, r);
                if (!more) break;
                t = tn;
                src += dsrc;
                dst += dout;
                // younger than the new tile's four loads is only the one
                // record store above (lane 0 of every tile is a valid slot,
                // so the store is always issued); operations retire in issue
                // order
                asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            }
            return;
        }
        // the staging cursor runs DEPTH-1 tiles ahead of the parse cursor
        uint64_t ts = t;
        const uint8_t* ssrc = src;
        // prologue: the first DEPTH-1 tiles
#pragma unroll
        for (uint32_t d = 0; d + 1u < DEPTH; ++d) {
            if (ts < tend) stage(ts, ssrc, img0 + d * Img::IMG_DW);
            ts += step;
            ssrc += dsrc;
        }
        for (uint32_t j = 0;; ++j) {
            if (ts < tend) {
                stage(ts, ssrc, img0 + ((j + DEPTH - 1u) % DEPTH) * Img::IMG_DW);
                // tile j's loads have landed
                pipe_wait<NCH, DEPTH>(j + 1u >= DEPTH);
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            ts += step;
            ssrc += dsrc;
            Frame<NCH> fr = frame(t, src, img0 + (j % DEPTH) * Img::IMG_DW);
            Rec r;
            walk<CHAIN, false>(fr, r, nullptr, nullptr);
            emit(t, dst, r);
            t += step;
            if (t >= tend) break;
            src += dsrc;
            dst += dout;
        }
    };
    if constexpr (NCH == 4) {
        if (a.stride == 64u) {
            run(std::true_type{});
            return;
        }
    }
    run(std::false_type{});
}

// One 32-bit word read past every cache (system scope: a doorbell in pinned
// host memory, written by the host while the kernel runs), made uniform.
// A vector load in asm: the compiler would turn a uniform plain load into a
// scalar one served from the scalar cache, and never see the new value.
__device__ __forceinline__ uint32_t load_system_u32(const uint32_t* p) {
    uint32_t v;
    asm volatile("global_load_dword %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=v"(v)
                 : "v"(p)
                 : "memory");
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// Persistent ring consumer (ingot_gpu_parse_ring): k_parse_pipe's staging and
// walk over the tiles of up to INGOT_RING_MAX_BATCHES batches in one launch.
// The batches' tiles are laid end to end and wave w of the W in the grid
// takes tiles w, w + W, w + 2W, ..., so every wave crosses the batch
// boundaries with its next tile's LDS-DMA already in flight: one grid ramp-up
// and one drain per launch instead of one per batch (the per-launch cost the
// two-stream schedule only half hides).  Tiles of batch b are
// staged only once b is published: b < a.published (known at launch), else
// the doorbell word >= db_first + b, polled by the wave that needs it.
template <uint32_t NCH, uint32_t DEPTH, int CHAIN, int MODE>
__global__ __launch_bounds__(BLOCK) void k_parse_ring(RingArgs a) {
    using Img = RingImg<NCH, DEPTH>;
    __shared__ __attribute__((aligned(16))) uint32_t s_img[Img::DW];
    const uint32_t lane = threadIdx.x & (WAVE - 1u);
    // wave-uniform (readfirstlane): the tile cursors, the batch index and
    // the batch table lookups stay scalar (SGPRs, s_load from the kernel
    // arguments) instead of a per-lane load of the batch pointers per tile
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    uint32_t* img0 = s_img + wave * Img::WAVE_DW;
    const uint32_t tpb = a.tiles_per_batch;
    // Batch groups (RingArgs::groups = G): the grid is cut into G groups of
    // blocks (8 consecutive blocks, one per XCD, per group in turn), group q
    // consuming batches q, q+G, q+2G, ... — G batches in flight at once, as G
    // streams of per-batch launches would have (launch_ring: G divides the
    // grid into whole 8-block rows).
    const uint32_t G = a.groups;
    const uint32_t grp = (blockIdx.x / 8u) % G;
    const uint32_t gblk = (blockIdx.x / (8u * G)) * 8u + blockIdx.x % 8u;
    const uint32_t W = (gridDim.x / G) * WAVES;  // waves of the group
    const uint32_t nbg = (a.nbatches - grp + G - 1u) / G;
    const uint32_t total = tpb * nbg;  // the group's tiles (< 2^32, api.cpp)
    const uint32_t g0 = gblk * WAVES + wave;
    if (g0 >= total) return;
    const uint32_t J = (total - g0 + W - 1u) / W;  // this wave's tiles
    // the fields the loop uses, held in SGPRs: left as kernel-argument
    // reads, the compiler re-loads them from the (4 KiB) argument block
    // inside the loop, each a scalar load and an lgkmcnt wait per tile
    uint64_t n = a.n;
    uint32_t stride = a.stride, policy = a.policy, nb = a.nbatches;
    asm volatile("" : "+s"(n), "+s"(stride), "+s"(policy), "+s"(nb));
    const uint32_t take = stride < Img::WIN ? stride : Img::WIN;
    uint32_t avail = a.published;  // batches [0, avail) are known published
    bool live = true;              // false once this wave gave up waiting

    // Batch b published?  Polls only past `avail`: one system-scope load of
    // the doorbell per wave (one request; every lane gets the word), with
    // backoff sleeps between polls, until the word reaches
    // db_first + b or the wave's wait exceeds timeout_ticks.  On success the
    // wave's caches are invalidated (system-scope acquire) before it stages
    // the new batch, so frames written after the launch started are seen.
    auto ready = [&](uint32_t b) -> bool {
        if (b < avail) return true;
        if (!a.doorbell) return false;
        const uint64_t t0 = wall_clock64();
        uint32_t naps = 1;  // exponential backoff: 1, 2, 4, 8 sleeps between polls
        for (;;) {
            const uint32_t v = load_system_u32(a.doorbell);
            if (v >= a.db_first + b) {
                const uint32_t pub = v - a.db_first + 1u;
                avail = pub < a.nbatches ? pub : a.nbatches;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                return true;
            }
            if (wall_clock64() - t0 > a.timeout_ticks) {
                if (a.status && lane == 0) atomicOr(a.status, 1u);
                return false;
            }
            // ~1 us per nap: a waiting wave polls the host word at most
            // every ~8 us once the wait is long, so thousands of waiting
            // waves do not flood PCIe while a producer publishes
            for (uint32_t z = 0; z < naps; ++z) __builtin_amdgcn_s_sleep(32);
            naps = naps < 8u ? 2u * naps : 8u;
        }
    };
    // Cursors of the next tile to stage and to parse: (batch, tile) and that
    // batch's buffers, reloaded from the kernel arguments only when the
    // cursor crosses into the next batch (scalar loads, once per batch).
    struct Cur {
        uint32_t b, t;
        const uint8_t* arena;
        void* out;
    };
    auto setb = [&](Cur& c) {
        if (c.b < nb) {
            c.arena = a.b[c.b].arena;
            c.out = a.b[c.b].out;
            asm volatile("" : "+s"(c.arena), "+s"(c.out));
        }
    };
    auto adv = [&](Cur& c) {
        c.t += W;
        if (c.t >= tpb) {
            do {
                c.t -= tpb;
                c.b += G;
            } while (c.t >= tpb);
            setb(c);
        }
    };
    Cur sc{grp + (g0 / tpb) * G, g0 % tpb, nullptr, nullptr};
    setb(sc);
    Cur pc = sc;
    auto stage = [&](const Cur& c, uint32_t* img) {
        stage_clamped<NCH>(lane, (uint64_t)c.t * WAVE, n, [&](uint32_t k, uint64_t slot, uint32_t ch) {
            stage16p(c.arena + slot * stride + 16u * ch, img + k * WAVE * 4u, policy);
        });
    };
    auto parse = [&](const Cur& c, const uint32_t* img) {
        const uint64_t i = (uint64_t)c.t * WAVE + lane;
        Frame<NCH> fr{(const lds_u32*)img, lane, 0u, take, stride, c.arena + i * stride};
        Rec r;
        walk<CHAIN, false>(fr, r, nullptr, nullptr);
        if (i < n) {
            if constexpr (MODE == OUT_REC8)
                store_rec(static_cast<uint2*>(c.out) + i, pack8(r), policy);
            else
                store_rec(static_cast<uint4*>(c.out) + i, pack(r), policy);
        }
    };
    // stage the next tile when there is one and its batch is published
    auto issue = [&](uint32_t& js) -> bool {
        if (!live || js >= J) return false;
        if (!ready(sc.b)) {
            live = false;
            return false;
        }
        stage(sc, img0 + (js % DEPTH) * Img::IMG_DW);
        ++js;
        adv(sc);
        return true;
    };

    uint32_t js = 0;  // tiles staged so far
#pragma unroll
    for (uint32_t d = 0; d + 1u < DEPTH; ++d) issue(js);
    for (uint32_t j = 0; j < js; ++j) {
        // tile j's loads have landed (a wave that stopped staging drains)
        if (issue(js) && js - j == DEPTH) {
            pipe_wait<NCH, DEPTH>(j + 1u >= DEPTH);
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        // the image is restaged only after every lane's reads of it have
        // returned: the record store consumes them (as in k_parse_pipe)
        parse(pc, img0 + (j % DEPTH) * Img::IMG_DW);
        adv(pc);
    }
}

// In-place rewrite on a slot ring (C2m: the reference's parse-and-decr-v4):
// k_parse_pipe's multi-tile staging, then the setters edit the staged copy
// (put_staged) and mark the write-back units they touch; the wave writes the
// dirty 16-B chunks back lane-linearly from its LDS image — the inverse of the
// staging map, so one store instruction covers 16 consecutive slots instead
// of 64 scattered ones.  Write-back unit `a.wb` bytes (16, 32 or 64, aligned
// within the slot); slots >= 64 B, the whole window inside every frame.
// ARGS = ModifyCsumArgs (ingot_gpu_parse_modify_csum): each applied edit's
// RFC 1624 term goes into the lane's accumulators, and after the edits the
// checksum fields are updated through the same staged-copy / dirty-unit /
// direct-store paths (walk.h: csum_finish) — no further LDS, no cross-lane work.
template <uint32_t NCH, uint32_t DEPTH, int CHAIN, class ARGS = ModifyArgs>
__global__ __launch_bounds__(BLOCK) void k_modify_pipe(ARGS args) {
    constexpr bool CSUM = std::is_same<ARGS, ModifyCsumArgs>::value;
    const ModifyArgs& m = edit_args(args);
    const ParseArgs& a = m.p;
    using Img = RingImg<NCH, DEPTH>;
    __shared__ __attribute__((aligned(16))) uint32_t s_img[Img::DW];
    const uint32_t lane = threadIdx.x & (WAVE - 1u);
    const uint32_t wave = threadIdx.x / WAVE;
    uint32_t* img0 = s_img + wave * Img::WAVE_DW;
    const uint64_t ntiles = (a.n + WAVE - 1u) / WAVE;
    const uint64_t step = (uint64_t)gridDim.x * WAVES;
    const bool nt_ld = a.policy & 1u;
    uint8_t* arena = const_cast<uint8_t*>(a.arena);
    const uint32_t unit_ch = m.wb / 16u;  // chunks per write-back unit

    // stage_clamped's loop spelt out (through the helper, the DEPTH 2
    // kernels' register allocation changed); plain stage16: no policy switch
    auto stage = [&](uint64_t tt, uint32_t* img) {
#pragma unroll
        for (uint32_t k = 0; k < NCH; ++k) {
            const auto [pp, c] = chunk_of<NCH>(k, lane);
            uint64_t slot = tt * WAVE + pp;
            if (slot >= a.n) slot = a.n - 1u;
            stage16(a.arena + slot * a.stride + 16u * c, img + k * WAVE * 4u, nt_ld);
        }
    };
    auto modify = [&](uint64_t tt, uint32_t* img) {
        const uint64_t i = tt * WAVE + lane;
        const bool valid = i < a.n;
        uint8_t* frame = arena + (valid ? i : 0) * a.stride;
        Frame<NCH> fr{(const lds_u32*)img, lane, 0u, Img::WIN, a.stride, frame};
        Rec r;
        walk<CHAIN, false>(fr, r, nullptr, nullptr);
        uint32_t dirty = 0;
        if (valid && r.status == INGOT_OK) {
            // (no accumulators in the plain kernel, whose code stays as it was)
            [[maybe_unused]] typename std::conditional<CSUM, CsumAcc, NoCsum>::type acc;
            for (uint32_t k = 0; k < m.n_edits; ++k) {
                const Edit& e = m.e[k];
                uint32_t h;
                if (!header_at<CHAIN>(r, e.layer, e.kind, e.index, h)) continue;
                // the setter (bitfield.rs:188-315): read-modify-write of the
                // covering bytes through the staged copy (a field across the
                // window's end: each byte from its side, see be_edited)
                uint64_t w = fr.be_edited(h + e.byte0, e.nbytes);
                [[maybe_unused]] const uint32_t w_old = CSUM ? (uint32_t)w : 0u;
                const uint32_t fm = e.bits >= 32 ? 0xffffffffu : ((1u << e.bits) - 1u);
                const uint32_t cur = (uint32_t)(w >> e.rshift) & fm;
                uint32_t v;
                switch (e.op) {
                case INGOT_OP_ADD: v = cur + e.value; break;
                case INGOT_OP_SUB: v = cur - e.value; break;
                case INGOT_OP_AND: v = cur & e.value; break;
                case INGOT_OP_OR: v = cur | e.value; break;
                case INGOT_OP_XOR: v = cur ^ e.value; break;
                default: v = e.value; break;
                }
                w = (w & ~((uint64_t)fm << e.rshift)) | ((uint64_t)(v & fm) << e.rshift);
                for (uint32_t b = 0; b < e.nbytes; ++b) {
                    const uint32_t at = h + e.byte0 + b;
                    const uint8_t x = (uint8_t)(w >> (8u * (e.nbytes - 1u - b)));
                    if (at < Img::WIN) {
                        fr.put_staged(at, x);
                        const uint32_t c0 = (at >> 4) & ~(unit_ch - 1u);
                        dirty |= ((1u << unit_ch) - 1u) << c0;
                    } else {
                        frame[at] = x;  // past the window (slots > 64 B)
                    }
                }
                if constexpr (CSUM)
                    csum_feed(acc, args.feeds[k], r,
                              csum_term(h + e.byte0, e.nbytes, w_old, (uint32_t)w));
            }
            if constexpr (CSUM)
                csum_finish<CHAIN>(fr, r, args.what, acc, [&](uint32_t at, uint8_t x) {
                    if (at < Img::WIN) {
                        fr.put_staged(at, x);
                        const uint32_t c0 = (at >> 4) & ~(unit_ch - 1u);
                        dirty |= ((1u << unit_ch) - 1u) << c0;
                    } else {
                        frame[at] = x;
                    }
                });
        }
        if (valid && a.out) store_rec(static_cast<uint4*>(a.out) + i, pack(r), a.policy);
        // every lane's staged edits are in LDS before any lane reads them back
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (uint32_t k = 0; k < NCH; ++k) {
            // chunk_of(k, lane), spelt out: through the helper the compiler
            // folds the unit's address differently (9 instructions fewer, not
            // measured)
            const uint32_t q = k * WAVE + lane;
            const uint32_t pp = q / NCH;
            const uint32_t c = (q - pp * NCH) ^ swz<NCH>(pp);
            const uint32_t d = (uint32_t)__shfl((int)dirty, (int)pp);
            if ((d >> c) & 1u) {
                const uint32_t* src = img + q * 4u;
                const uint4 v = make_uint4(src[0], src[1], src[2], src[3]);
                store_rec(reinterpret_cast<uint4*>(arena + (tt * WAVE + pp) * a.stride + 16u * c),
                          v, a.policy);
            }
        }
    };

    // XCD-major block order (a.xcd_remap bit 0), as in k_parse_pipe
    uint32_t bid = blockIdx.x;
    if ((a.xcd_remap & 1u) && gridDim.x % 8u == 0u)
        bid = (bid % 8u) * (gridDim.x / 8u) + bid / 8u;
    uint64_t t = (uint64_t)bid * WAVES + wave;
    if (t >= ntiles) return;
#pragma unroll
    for (uint32_t d = 0; d + 1u < DEPTH; ++d)
        if (t + d * step < ntiles) stage(t + d * step, img0 + d * Img::IMG_DW);
    for (uint32_t j = 0;; ++j) {
        const uint64_t tn = t + (DEPTH - 1u) * step;
        if (tn < ntiles) {
            stage(tn, img0 + ((j + DEPTH - 1u) % DEPTH) * Img::IMG_DW);
            // the write-back's stores vary per tile: waited out
            pipe_wait<NCH, DEPTH>(false);
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        modify(t, img0 + (j % DEPTH) * Img::IMG_DW);
        // the write-back's LDS reads are done before this image is restaged
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        t += step;
        if (t >= ntiles) break;
    }
}

// Launch f's kernel for the chain tag (f(integral_constant<int, CHAIN>)).
template <class F>
hipError_t launch_for_chain(int chain, F&& f) {
    return with_chain(chain, f) ? hipGetLastError() : hipErrorInvalidValue;
}

template <uint32_t DEPTH, class ARGS>
hipError_t launch_modify_pipe(const ARGS& a, int chain, uint32_t grid, hipStream_t s) {
    return launch_for_chain(chain, [&](auto c) {
        hipLaunchKernelGGL((k_modify_pipe<4, DEPTH, decltype(c)::value, ARGS>), dim3(grid),
                           dim3(BLOCK), 0, s, a);
    });
}

template <uint32_t DEPTH, int MODE, uint32_t POL = 0>
hipError_t launch_pipe(const ParseArgs& a, int chain, uint32_t grid, hipStream_t s) {
    return launch_for_chain(chain, [&](auto c) {
        hipLaunchKernelGGL((k_parse_pipe<4, DEPTH, decltype(c)::value, MODE, POL>), dim3(grid),
                           dim3(BLOCK), 0, s, a);
    });
}

template <uint32_t DEPTH, int MODE>
hipError_t launch_ring_chain(const RingArgs& a, int chain, uint32_t grid, hipStream_t s) {
    return launch_for_chain(chain, [&](auto c) {
        hipLaunchKernelGGL((k_parse_ring<4, DEPTH, decltype(c)::value, MODE>), dim3(grid),
                           dim3(BLOCK), 0, s, a);
    });
}

// The ring kernels' grid over `tiles` 64-slot tiles: INGOT_TUNE_PIPELINE = k
// > 1 gives every wave k tiles; otherwise a whole number of blocks per CU
// (`per_cu`: INGOT_TUNE_RING_GRID where the kernel follows it, default 2), so
// that the tiles spread evenly over the CUs, capped at one tile per wave.
uint32_t ring_blocks(uint64_t tiles, int pipeline, uint64_t per_cu, uint32_t cus) {
    uint64_t blocks;
    if (pipeline > 1) {
        const uint64_t waves = (tiles + (uint64_t)pipeline - 1) / (uint64_t)pipeline;
        blocks = (waves + WAVES - 1) / WAVES;
    } else {
        const uint64_t cap = per_cu * cus;
        blocks = (tiles + WAVES - 1) / WAVES;
        if (blocks > cap) blocks = cap;
    }
    return (uint32_t)(blocks ? blocks : 1);
}

// INGOT_TUNE_XCD_REMAP as the kernels' tile-order bits (k_parse_pipe), `mask`
// the bits the kernel implements: 0 = the default, XCD-major (bit 0; measured,
// 2 streams 12.22 -> 12.03 us/step at 20 steps, 11.91 -> 11.74
// at 2,000); 4 = hardware order; 5 = one region per XCD (bit 2, under which
// bit 0 changes nothing); 1-3 = the bits themselves.
uint32_t xcd_bits(int v, uint32_t mask) {
    return (v == 0 ? 1u : v == 4 ? 0u : (uint32_t)v) & mask;
}

// One depth of launch_slot_ring's ladder.  The default policies (launch_parse:
// 16-B records 11, 8-B records 3) have their cache bits compiled in at depths
// 1 and 2 (k_parse_pipe's POL); any other policy, and depths 3 and 4, take
// the runtime switch.
template <uint32_t DEPTH>
hipError_t launch_pipe_depth(const ParseArgs& a, int chain, int mode, uint32_t pg, hipStream_t s) {
    if constexpr (DEPTH <= 2) {
        if (mode == OUT_REC16 && a.policy == 11u) return launch_pipe<DEPTH, OUT_REC16, 11u>(a, chain, pg, s);
        if (mode == OUT_REC8 && a.policy == 3u) return launch_pipe<DEPTH, OUT_REC8, 3u>(a, chain, pg, s);
    }
    return mode == OUT_REC8 ? launch_pipe<DEPTH, OUT_REC8>(a, chain, pg, s)
                            : launch_pipe<DEPTH, OUT_REC16>(a, chain, pg, s);
}

}  // namespace

// Ring rewrite kernel defaults (k_modify_pipe; measured).
constexpr uint32_t kModifyRingWb = 64;
constexpr uint32_t kModifyRingPolicy = 3;  // nt staging loads + nt write-back

// C2-style rings (slots >= 64 B, no length array, record output): the
// multi-tile kernel k_parse_pipe on ring_blocks' grid (INGOT_TUNE_RING_GRID
// blocks per CU; 6 or 12 tiles per wave, uneven over the CUs, lose most of
// what the whole-blocks-per-CU grid gains).
// Default: one LDS image per wave (DEPTH 1), measured on the two-stream C2
// schedule against two images, alternated runs of the benchmark's default
// command: 11.59-11.64 vs 11.87-11.94 us/step
// (profiles/r07_c2_single_image_ab.json); with the scalar
// tile loop (round 8, profiles/r08_c2_lean_loop_ab.json) 11.41-11.47 against
// that parent's 11.61-11.68 us/step, one stream alone 14.00 against 14.9.
// INGOT_TUNE_PIPE_DEPTH = 2..4 selects that many images (the key's value 1
// stays EINVAL: the single image is what 0, the default, selects).
hipError_t launch_slot_ring(const ParseArgs& args, int chain, int mode, const Tuning& t,
                            hipStream_t s) {
    ParseArgs a = args;
    a.xcd_remap = xcd_bits(t.xcd_remap, 7u);
    const uint32_t pg = ring_blocks((a.n + WAVE - 1) / WAVE, t.pipeline,
                                    t.ring_grid ? (uint64_t)t.ring_grid : 2ull, t.cus);
    switch (t.pipe_depth) {
    case 0: return launch_pipe_depth<1>(a, chain, mode, pg, s);
    case 3: return launch_pipe_depth<3>(a, chain, mode, pg, s);
    case 4: return launch_pipe_depth<4>(a, chain, mode, pg, s);
    default: return launch_pipe_depth<2>(a, chain, mode, pg, s);
    }
}

// Slot rings (slots >= 64 B, no length array): the multi-tile kernel with
// lane-linear write-back (k_modify_pipe).  Defaults measured on MI355X
// (DESIGN.md §1c): write-back unit WB, plain staging loads.
template <class ARGS>
static hipError_t launch_modify_ring_as(const ARGS& args, int chain, const Tuning& t,
                                        hipStream_t s) {
    ARGS b = args;
    ModifyArgs& a = edit_args(b);
    a.p.xcd_remap = xcd_bits(t.xcd_remap, 1u);  // block order only
    a.wb = t.writeback ? (uint32_t)t.writeback : kModifyRingWb;
    a.p.policy = t.cache_policy ? (uint32_t)t.cache_policy & 0x3bu : kModifyRingPolicy;
    const uint32_t pg = ring_blocks((a.p.n + WAVE - 1) / WAVE, t.pipeline, 2, t.cus);
    return t.pipe_depth == 3 ? launch_modify_pipe<3>(b, chain, pg, s)
                             : launch_modify_pipe<2>(b, chain, pg, s);
}

hipError_t launch_modify_ring(const ModifyArgs& a, int chain, const Tuning& t, hipStream_t s) {
    return launch_modify_ring_as(a, chain, t, s);
}

hipError_t launch_modify_ring_csum(const ModifyCsumArgs& a, int chain, const Tuning& t,
                                   hipStream_t s) {
    return launch_modify_ring_as(a, chain, t, s);
}

// The ring consumer's grid is persistent: blocks per CU x CUs (default 2,
// like the single-batch ring kernel), capped at one tile per wave.  Cache
// policy as k_parse_pipe's (nt staging loads; 16-B records stored sc1).
hipError_t launch_ring(const RingArgs& args, int chain, int mode, const Tuning& t,
                       hipStream_t s) {
    RingArgs a = args;
    if (a.nbatches == 0 || a.n == 0) return hipSuccess;
    if (t.cache_policy == 0) a.policy = mode == OUT_REC16 ? 11u : 3u;
    else a.policy = (uint32_t)t.cache_policy & 0x1fbu;
    const uint32_t g = ring_blocks((uint64_t)a.tiles_per_batch * a.nbatches, 0,
                                   t.ring_grid ? (uint64_t)t.ring_grid : 2ull, t.cus);
    // batch groups only on a grid of whole 8-block rows per group
    a.groups = t.ring_groups > 1 ? (uint32_t)t.ring_groups : 1u;
    if (g % (8u * a.groups) != 0 || a.groups > a.nbatches) a.groups = 1;
    const bool r8 = mode == OUT_REC8;
    switch (t.pipe_depth) {
    case 3: return r8 ? launch_ring_chain<3, OUT_REC8>(a, chain, g, s)
                      : launch_ring_chain<3, OUT_REC16>(a, chain, g, s);
    case 4: return r8 ? launch_ring_chain<4, OUT_REC8>(a, chain, g, s)
                      : launch_ring_chain<4, OUT_REC16>(a, chain, g, s);
    default: return r8 ? launch_ring_chain<2, OUT_REC8>(a, chain, g, s)
                       : launch_ring_chain<2, OUT_REC16>(a, chain, g, s);
    }
}

}  // namespace ingot_gpu
