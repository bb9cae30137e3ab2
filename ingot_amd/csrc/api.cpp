// api.cpp — the C ABI (include/ingot_gpu.h) over the HIP kernels.
//
// Contexts, host mappings, the doorbell, tuning, where a call's packets lie
// and the string tables that mirror ingot's error surface:
// ParseError::as_cstr (ingot-types/src/error.rs:49-60) and the per-layer
// labels a generated chain attaches to PacketParseError
// (ingot-macros/src/parse.rs:36-50, field names from
// ingot-examples/src/packets.rs:18-40, 54-60).  The edit, set and sum lists
// become kernel argument blocks in resolve.cpp.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/ingot_gpu.h"
#include "kernels.h"
#include "resolve.h"

struct ingot_gpu_ctx {
    // One ingot_gpu_host_map of [host, host + bytes) by a context.  `owned`:
    // the bytes lie inside a registration this library made (g_regs below);
    // otherwise the memory was pinned and mapped by someone else (hipHostMalloc,
    // or the caller's own hipHostRegister) and unmapping it is a no-op.
    struct HostMapping {
        uintptr_t host, bytes, dev;
        bool owned;
    };
    int device = 0;
    ingot_gpu::Tuning tuning;
    uint32_t wall_khz = 0;  // the device's constant-rate wall clock (stream delays)
    size_t lds_bytes = 160u * 1024u;  // LDS per workgroup (the device's, at create)
    // live ingot_gpu_host_map mappings of this context (dropped on unmap)
    std::mutex mu;
    std::vector<HostMapping> host;
};

// Doorbell: one pinned, coherent host word the command processor polls
// (hipStreamWaitValue32).  Host stores to coherent memory are seen by the
// device without a flush.
struct ingot_gpu_doorbell {
    int device = 0;
    uint32_t* word;
    uint32_t* dword = nullptr;  // the word's device address (ingot_gpu_parse_ring polls it)
};

namespace {

using namespace ingot_gpu;
using HostMapping = ingot_gpu_ctx::HostMapping;

// Pageable host ranges this library page-locked (hipHostRegister, mapped).
// Registration state is per process, not per context, so the table is too.
// Each entry is the exact byte range registered; every ingot_gpu_host_map of
// bytes inside it (by any context) holds a reference, and the last
// ingot_gpu_host_unmap unregisters it.  Nothing else is ever unregistered.
struct Registration {
    uintptr_t host, bytes, dev;
    uint32_t refs;
};
std::mutex g_reg_mu;
std::vector<Registration> g_regs;

const char* const kParseErrorNames[] = {
    "Ok",           "Unwanted",       "NeedsHint", "TooSmall",    "StraddledHeader",
    "NoRemainingChunks", "CannotAccept", "Reject",    "IllegalValue",
};

const char* const kUdpParserLabels[] = {"eth", "l3", "l4"};
const char* const kGenericUlpLabels[] = {"inner_eth", "inner_l3", "inner_ulp"};
const char* const kVlanUlpLabels[] = {"eth", "vlan", "l3", "l4"};
// ingot-examples/src/packets.rs:27-40
const char* const kGeneveLabels[] = {"outer_eth", "outer_v6",  "outer_udp", "outer_encap",
                                     "inner_eth", "inner_l3", "inner_ulp"};

// INGOT_TUNE_* -> the Tuning member it sets and gets (max_blocks is the
// unsigned one).
struct TuneKey {
    int key;
    int Tuning::*i;
    uint32_t Tuning::*u;
};
constexpr TuneKey kTuneKeys[] = {
    {INGOT_TUNE_WINDOW_INDEXED, &Tuning::window_indexed, nullptr},
    {INGOT_TUNE_WINDOW_STRIDED, &Tuning::window_strided, nullptr},
    {INGOT_TUNE_MAX_BLOCKS, nullptr, &Tuning::max_blocks},
    {INGOT_TUNE_PIPELINE, &Tuning::pipeline, nullptr},
    {INGOT_TUNE_CACHE_POLICY, &Tuning::cache_policy, nullptr},
    {INGOT_TUNE_PIPE_DEPTH, &Tuning::pipe_depth, nullptr},
    {INGOT_TUNE_WRITEBACK, &Tuning::writeback, nullptr},
    {INGOT_TUNE_FLOW_TABLE, &Tuning::flow_table, nullptr},
    {INGOT_TUNE_SLOW_PATH, &Tuning::slow_path, nullptr},
    {INGOT_TUNE_READ_PLAN, &Tuning::read_plan, nullptr},
    {INGOT_TUNE_FLOW_KERNEL, &Tuning::flow_kernel, nullptr},
    {INGOT_TUNE_RING_GRID, &Tuning::ring_grid, nullptr},
    {INGOT_TUNE_RING_GROUPS, &Tuning::ring_groups, nullptr},
    {INGOT_TUNE_XCD_REMAP, &Tuning::xcd_remap, nullptr},
};
const TuneKey* tune_key(int key) {
    for (const TuneKey& k : kTuneKeys)
        if (k.key == key) return &k;
    return nullptr;
}

int from_hip(hipError_t e) { return e == hipSuccess ? INGOT_GPU_SUCCESS : INGOT_GPU_EHIP; }

// Make the context's device current for the launch (callers may juggle
// devices on one thread).
int enter(const ingot_gpu_ctx* ctx) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return INGOT_GPU_EHIP;
    if (cur != ctx->device && hipSetDevice(ctx->device) != hipSuccess) return INGOT_GPU_EHIP;
    return INGOT_GPU_SUCCESS;
}

// The context's tuning for a call over `arena`: frames in mapped host memory
// get the host-arena window defaults (launch_parse).
Tuning tuning_for(ingot_gpu_ctx* ctx, const void* arena) {
    Tuning t = ctx->tuning;
    const uintptr_t a = (uintptr_t)arena;
    std::lock_guard<std::mutex> g(ctx->mu);
    for (const auto& m : ctx->host)
        if (a >= m.dev && a < m.dev + m.bytes) t.host_arena = true;
    return t;
}

// Drop one reference to the library's registration holding [h, h + n); the
// last one unregisters it.  Caller holds g_reg_mu.
void release_registration(uintptr_t h, uintptr_t n) {
    for (size_t i = 0; i < g_regs.size(); ++i) {
        Registration& r = g_regs[i];
        if (h < r.host || h + n > r.host + r.bytes) continue;
        if (--r.refs == 0) {
            if (hipHostUnregister(reinterpret_cast<void*>(r.host)) != hipSuccess)
                (void)hipGetLastError();
            g_regs.erase(g_regs.begin() + (long)i);
        }
        return;
    }
}

int stride_ok(const uint8_t* d_arena, uint32_t stride) {
    if (stride == 0 || stride % 16u != 0 || stride > 65535u) return INGOT_GPU_ERANGE;
    if (((uintptr_t)d_arena & 15u) != 0) return INGOT_GPU_EINVAL;
    return INGOT_GPU_SUCCESS;
}

// Where a call's packets lie, as the kernels take it.
struct Frames {
    int layout;
    ParseArgs p;
};

// Frames in an arena: d_off NULL means slots of `stride` (stride_ok's rules,
// d_len optional); otherwise (d_off, d_len), both required.
int frames_of(const uint8_t* d_arena, const uint64_t* d_off, const uint16_t* d_len,
              uint32_t stride, uint64_t n, void* d_out, Frames& f) {
    if (!d_arena || (d_off && !d_len)) return INGOT_GPU_EINVAL;
    if (!d_off)
        if (int e = stride_ok(d_arena, stride)) return e;
    f.layout = d_off ? LAYOUT_INDEXED : LAYOUT_STRIDED;
    f.p = ParseArgs{d_arena, d_off, d_len, stride, n, d_out};
    return INGOT_GPU_SUCCESS;
}

// parse_read's CSR chunk tables: packet i is the chunks d_pkt_seg[i] ..
// d_pkt_seg[i + 1] of (d_seg_off, d_seg_len).  `dense`: one table of
// (offset << 16) | length, no d_seg_len (len == NULL selects it, launch_parse).
int chunks_of(const uint8_t* d_arena, const uint64_t* d_seg_off, const uint16_t* d_seg_len,
              const uint32_t* d_pkt_seg, uint64_t n, void* d_out, uint16_t* d_chunk, Frames& f,
              bool dense = false) {
    if (!d_arena || !d_seg_off || (!dense && !d_seg_len) || !d_pkt_seg) return INGOT_GPU_EINVAL;
    f.layout = LAYOUT_SEGMENTED;
    f.p = ParseArgs{d_arena, d_seg_off, dense ? nullptr : d_seg_len, 0, n, d_out, d_pkt_seg,
                    d_chunk};
    return INGOT_GPU_SUCCESS;
}

// The frames or the chunk tables of a call that has a form for each.
struct Packets {
    bool chunks;
    const uint64_t* off;  // d_off, or d_seg_off
    const uint16_t* len;  // d_len, or d_seg_len
    uint32_t stride;
    const uint32_t* pkt_seg;
    uint16_t* chunk;
};
int packets_of(const Packets& w, const uint8_t* d_arena, uint64_t n, void* d_out, Frames& f) {
    return w.chunks ? chunks_of(d_arena, w.off, w.len, w.pkt_seg, n, d_out, w.chunk, f)
                    : frames_of(d_arena, w.off, w.len, w.stride, n, d_out, f);
}

// The parse calls over frames; `need_off`: the call has no slot form.
int parse_frames(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                 const uint16_t* d_len, uint32_t stride, bool need_off, uint64_t n, int chain,
                 void* d_out, int mode, void* stream) {
    if (!ctx || !chain_ok(chain)) return INGOT_GPU_EINVAL;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_out || (need_off && !d_off)) return INGOT_GPU_EINVAL;
    Frames f;
    if (int e = frames_of(d_arena, d_off, d_len, d_off ? 0u : stride, n, d_out, f)) return e;
    if (int e = enter(ctx)) return e;
    return from_hip(launch_parse(f.p, f.layout, chain, mode, tuning_for(ctx, d_arena),
                                 (hipStream_t)stream));
}

// The parse calls over chunk tables; d_first: ingot_gpu_parse_read_first's.
int parse_chunks(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_seg_off,
                 const uint16_t* d_seg_len, const uint32_t* d_pkt_seg, bool dense,
                 const uint64_t* d_first, uint64_t n, int chain, void* d_out, uint16_t* d_chunk,
                 int mode, void* stream) {
    if (!ctx || !chain_ok(chain)) return INGOT_GPU_EINVAL;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_out) return INGOT_GPU_EINVAL;
    Frames f;
    if (int e = chunks_of(d_arena, d_seg_off, d_seg_len, d_pkt_seg, n, d_out, d_chunk, f, dense))
        return e;
    if (int e = enter(ctx)) return e;
    f.p.first = d_first;
    return from_hip(launch_parse(f.p, f.layout, chain, mode, tuning_for(ctx, d_arena),
                                 (hipStream_t)stream));
}

// The rewrites with one operand per edit (what == 0: no sums): every argument
// is checked before any device work.
int rewrite(ingot_gpu_ctx* ctx, uint8_t* d_arena, const Packets& w, uint64_t n, int chain,
            const ingot_edit* edits, uint32_t n_edits, uint32_t what, ingot_rec* d_out,
            void* stream) {
    ModifyCsumArgs c{};  // (the checksum update's extras: used when what != 0)
    if (int e = resolve_edits(ctx, chain, edits, n_edits, what, c)) return e;
    if (n == 0) return INGOT_GPU_SUCCESS;
    Frames f;
    if (int e = packets_of(w, d_arena, n, d_out, f)) return e;
    if (int e = enter(ctx)) return e;
    c.m.p = f.p;
    const Tuning t = tuning_for(ctx, d_arena);
    const hipStream_t s = (hipStream_t)stream;
    if (w.chunks)
        return from_hip(what ? launch_read_modify_csum(c, chain, t, s)
                             : launch_read_modify(c.m, chain, t, s));
    return from_hip(what ? launch_modify_csum(c, f.layout, chain, t, s)
                         : launch_modify(c.m, f.layout, chain, t, s));
}

// The rewrites with per-packet and per-row operands, checked in the order the
// header gives.
int rewrite_rows(ingot_gpu_ctx* ctx, uint8_t* d_arena, const Packets& w, uint64_t n, int chain,
                 const ingot_edit_rows* edits, uint32_t n_edits, const uint32_t* d_row,
                 uint32_t n_rows, uint32_t what, ingot_rec* d_out, void* stream) {
    ModifyRowsArgs a{};
    if (int e = resolve_edit_rows(ctx, chain, edits, n_edits, d_row, n_rows, what, a)) return e;
    if (n == 0) return INGOT_GPU_SUCCESS;
    Frames f;
    if (int e = packets_of(w, d_arena, n, d_out, f)) return e;
    if (int e = enter(ctx)) return e;
    a.p = f.p;
    const Tuning t = tuning_for(ctx, d_arena);
    const hipStream_t s = (hipStream_t)stream;
    return from_hip(w.chunks ? launch_read_modify_rows(a, chain, t, s)
                             : launch_modify_rows(a, f.layout, chain, t, s));
}

const uint32_t kRewriteSums = INGOT_CSUM_L3 | INGOT_CSUM_L4 | INGOT_CSUM_OUTER_L4;

// Both whole-packet calls (the plain one: no sums).
int emit_packets(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                 const ingot_emit_set* sets, uint32_t n_sets, const ingot_emit_sum* sums,
                 uint32_t n_sums, const uint8_t* d_src, const uint64_t* d_off,
                 const uint16_t* d_len, uint64_t n, uint8_t* d_dst, const uint64_t* d_dst_off,
                 void* stream) {
    if (!ctx) return INGOT_GPU_EINVAL;
    EmitArgs a{};
    if (int e = emit_args(hdr, hdr_len, sets, n_sets, a)) return e;
    if (int e = emit_sums(hdr, hdr_len, sets, n_sets, sums, n_sums, a)) return e;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_src || !d_off || !d_len || !d_dst || !d_dst_off) return INGOT_GPU_EINVAL;
    if (int e = enter(ctx)) return e;
    a.src = d_src;
    a.off = d_off;
    a.len = d_len;
    a.dst = d_dst;
    a.dst_off = d_dst_off;
    a.n = n;
    // the device's LDS per workgroup must hold one emit block's
    if (emit_lds_bytes(a) > ctx->lds_bytes) return INGOT_GPU_ERANGE;
    return from_hip(launch_emit(a, (hipStream_t)stream));
}

// The four checksum calls (verify: the kernel writes the arena only in fill
// mode): every argument is checked before any device work.
int checksum(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const Packets& w, uint64_t n,
             const ingot_rec* d_rec, uint32_t what, ingot_csum* d_out, bool fill, void* stream) {
    // (no chain: there is no outer sum to ask for)
    if (!ctx || !what_ok(what, INGOT_CSUM_L3 | INGOT_CSUM_L4, false, -1)) return INGOT_GPU_EINVAL;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_rec || (!d_out && !fill)) return INGOT_GPU_EINVAL;
    Frames f;
    if (int e = packets_of(w, d_arena, n, nullptr, f)) return e;
    if (int e = enter(ctx)) return e;
    uint8_t* arena = const_cast<uint8_t*>(d_arena);
    const hipStream_t s = (hipStream_t)stream;
    if (w.chunks)
        return from_hip(launch_csum_read(CsumReadArgs{arena, f.p.off, f.p.len, f.p.pkt_seg, n,
                                                      d_rec, d_out, what, fill ? 1u : 0u},
                                         s));
    return from_hip(launch_csum(CsumArgs{arena, f.p.off, f.p.len, w.off ? 0u : w.stride, what, n,
                                         d_rec, d_out, fill ? 1u : 0u},
                                s));
}

bool bins_ok(uint32_t bins) { return bins != 0 && (bins & (bins - 1)) == 0 && bins <= (1u << 24); }

}  // namespace

extern "C" {

int ingot_gpu_abi_version(void) { return INGOT_GPU_ABI_VERSION; }

const char* ingot_gpu_build_info(void) {
    return "ingot_gpu " __DATE__ " gfx950 (LDS-DMA staged wave-per-64-packet parse)";
}

int ingot_gpu_ctx_create(int device, ingot_gpu_ctx** out) {
    if (!out) return INGOT_GPU_EINVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
        return INGOT_GPU_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return INGOT_GPU_EHIP;
    // Code objects are built for gfx950 only.
    if (prop.gcnArchName[0] && std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return INGOT_GPU_ENODEV;
    ingot_gpu_ctx* c = new (std::nothrow) ingot_gpu_ctx();  // value-initialised
    if (!c) return INGOT_GPU_ENOMEM;
    c->device = device;
    if (prop.multiProcessorCount > 0) c->tuning.cus = (uint32_t)prop.multiProcessorCount;
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) ==
            hipSuccess &&
        lds > 0)
        c->lds_bytes = (size_t)lds;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess &&
        khz > 0)
        c->wall_khz = (uint32_t)khz;
    *out = c;
    return INGOT_GPU_SUCCESS;
}

void ingot_gpu_ctx_destroy(ingot_gpu_ctx* ctx) {
    if (!ctx) return;
    {  // the context's mappings still open release their registrations
        std::lock_guard<std::mutex> g(g_reg_mu);
        std::lock_guard<std::mutex> c(ctx->mu);
        for (const HostMapping& m : ctx->host)
            if (m.owned) release_registration(m.host, m.bytes);
        ctx->host.clear();
    }
    delete ctx;
}

int ingot_gpu_ctx_device(const ingot_gpu_ctx* ctx) { return ctx ? ctx->device : -1; }

int ingot_gpu_ctx_set_tuning(ingot_gpu_ctx* ctx, int key, int value) {
    const TuneKey* k = tune_key(key);
    if (!ctx || !k || !tuning_valid(key, value)) return INGOT_GPU_EINVAL;
    if (k->i)
        ctx->tuning.*(k->i) = value;
    else
        ctx->tuning.*(k->u) = (uint32_t)value;  // tuning_valid: not negative
    return INGOT_GPU_SUCCESS;
}

int ingot_gpu_ctx_get_tuning(const ingot_gpu_ctx* ctx, int key) {
    const TuneKey* k = tune_key(key);
    if (!ctx || !k) return INGOT_GPU_EINVAL;
    return k->i ? ctx->tuning.*(k->i) : (int)(ctx->tuning.*(k->u));
}

int ingot_gpu_host_map(ingot_gpu_ctx* ctx, void* host, size_t bytes, void** d_ptr) {
    if (!ctx || !host || !d_ptr || bytes == 0) return INGOT_GPU_EINVAL;
    *d_ptr = nullptr;
    const uintptr_t h = (uintptr_t)host;
    if (h + bytes < h) return INGOT_GPU_ERANGE;
    if (int e = enter(ctx)) return e;
    std::lock_guard<std::mutex> g(g_reg_mu);
    HostMapping m{h, bytes, 0, false};
    // 1. inside one of our registrations: one more reference to it
    for (Registration& r : g_regs) {
        if (h >= r.host && h + bytes <= r.host + r.bytes) {
            ++r.refs;
            m.dev = r.dev + (h - r.host);
            m.owned = true;
            break;
        }
        // partly overlapping bytes we registered: the rest is not ours to
        // register, and a second registration of the same bytes is refused
        if (h < r.host + r.bytes && r.host < h + bytes) return INGOT_GPU_EINVAL;
    }
    if (!m.owned) {
        // 2. pinned and mapped by someone else (hipHostMalloc, the caller's
        //    own hipHostRegister): used as it is, never unregistered here
        hipPointerAttribute_t attr;
        void* d = nullptr;
        if (hipPointerGetAttributes(&attr, host) == hipSuccess &&
            attr.type == hipMemoryTypeHost && hipHostGetDevicePointer(&d, host, 0) == hipSuccess) {
            m.dev = (uintptr_t)d;
        } else {
            // 3. pageable: page-lock and map exactly these bytes (pages
            //    shared with neighbours stay usable by them)
            (void)hipGetLastError();  // clear the probe's error
            if (hipHostRegister(host, bytes, hipHostRegisterMapped) != hipSuccess) {
                (void)hipGetLastError();
                return INGOT_GPU_EHIP;
            }
            if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess) {
                (void)hipHostUnregister(host);
                (void)hipGetLastError();
                return INGOT_GPU_EHIP;
            }
            m.dev = (uintptr_t)d;
            m.owned = true;
            g_regs.push_back(Registration{h, bytes, m.dev, 1u});
        }
    }
    {
        std::lock_guard<std::mutex> c(ctx->mu);
        ctx->host.push_back(m);
    }
    *d_ptr = reinterpret_cast<void*>(m.dev);
    return INGOT_GPU_SUCCESS;
}

int ingot_gpu_host_unmap(ingot_gpu_ctx* ctx, void* host) {
    if (!ctx || !host) return INGOT_GPU_EINVAL;
    const uintptr_t h = (uintptr_t)host;
    std::lock_guard<std::mutex> g(g_reg_mu);
    HostMapping m{};
    {
        std::lock_guard<std::mutex> c(ctx->mu);
        size_t i = ctx->host.size();
        while (i > 0 && ctx->host[i - 1].host != h) --i;  // the latest mapping of `host`
        if (i == 0) return INGOT_GPU_EINVAL;               // not mapped by this context
        m = ctx->host[i - 1];
        ctx->host.erase(ctx->host.begin() + (long)(i - 1));
    }
    if (m.owned) release_registration(m.host, m.bytes);  // registrations are per process
    return INGOT_GPU_SUCCESS;
}
int ingot_gpu_doorbell_create(ingot_gpu_ctx* ctx, ingot_gpu_doorbell** out,
                              volatile uint32_t** host_word) {
    if (!ctx || !out) return INGOT_GPU_EINVAL;
    *out = nullptr;
    if (host_word) *host_word = nullptr;
    if (int e = enter(ctx)) return e;
    int can = 0;
    if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, ctx->device) !=
            hipSuccess ||
        !can)
        return INGOT_GPU_ENODEV;
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
        return INGOT_GPU_EHIP;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess) {
        (void)hipHostFree(p);
        return INGOT_GPU_EHIP;
    }
    ingot_gpu_doorbell* d =
        new (std::nothrow) ingot_gpu_doorbell{ctx->device, (uint32_t*)p, (uint32_t*)dp};
    if (!d) {
        (void)hipHostFree(p);
        return INGOT_GPU_ENOMEM;
    }
    __atomic_store_n(d->word, 0u, __ATOMIC_SEQ_CST);
    *out = d;
    if (host_word) *host_word = d->word;
    return INGOT_GPU_SUCCESS;
}

int ingot_gpu_doorbell_wait(ingot_gpu_doorbell* db, uint32_t value, void* stream) {
    if (!db) return INGOT_GPU_EINVAL;
    return from_hip(hipStreamWaitValue32((hipStream_t)stream, db->word, value,
                                         hipStreamWaitValueGte, 0xffffffffu));
}

int ingot_gpu_doorbell_ring(ingot_gpu_doorbell* db, uint32_t value) {
    if (!db) return INGOT_GPU_EINVAL;
    __atomic_store_n(db->word, value, __ATOMIC_SEQ_CST);
    return INGOT_GPU_SUCCESS;
}

int ingot_gpu_stream_delay(ingot_gpu_ctx* ctx, uint32_t ns, void* stream) {
    if (!ctx) return INGOT_GPU_EINVAL;
    if (ns == 0) return INGOT_GPU_SUCCESS;
    if (!ctx->wall_khz) return INGOT_GPU_ENODEV;
    if (int e = enter(ctx)) return e;
    const uint64_t ticks = ((uint64_t)ns * ctx->wall_khz + 999999u) / 1000000u;
    return from_hip(ingot_gpu::launch_delay(ticks, (hipStream_t)stream));
}

void ingot_gpu_doorbell_destroy(ingot_gpu_doorbell* db) {
    if (!db) return;
    (void)hipHostFree(db->word);
    delete db;
}

size_t ingot_gpu_packed_workspace_size(uint64_t n) { return packed_workspace(n); }

int ingot_gpu_parse_packed(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint16_t* d_len,
                           uint64_t n, int chain, ingot_rec* d_out, uint64_t* d_off_out,
                           void* d_work, size_t work_bytes, void* stream) {
    if (!ctx || !chain_ok(chain)) return INGOT_GPU_EINVAL;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_arena || !d_len || !d_out || !d_work || ((uintptr_t)d_work & 7u))
        return INGOT_GPU_EINVAL;
    if (work_bytes < packed_workspace(n)) return INGOT_GPU_ERANGE;
    if (int e = enter(ctx)) return e;
    const hipStream_t s = (hipStream_t)stream;
    if (int e = from_hip(launch_tile_bases(d_len, n, d_work, s))) return e;
    const uint64_t ngroups = ((n + 63) / 64 + PACKED_GROUP - 1) / PACKED_GROUP;
    ParseArgs a{d_arena, static_cast<const uint64_t*>(d_work), d_len, 0, n, d_out};
    a.tile_local =
        reinterpret_cast<const uint32_t*>(static_cast<const uint64_t*>(d_work) + ngroups);
    a.off_out = d_off_out;
    return from_hip(launch_parse(a, LAYOUT_PACKED, chain, OUT_REC16, tuning_for(ctx, d_arena), s));
}

int ingot_gpu_parse_header(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                           const uint16_t* d_len, uint32_t stride, uint64_t n, int kind,
                           const uint32_t* d_hint, uint32_t hint, ingot_hdr* d_out,
                           void* stream) {
    const bool kind_ok = (kind >= INGOT_HDR_ETHERNET && kind <= INGOT_HDR_GENEVE) ||
                         (kind >= INGOT_HDR_L3 && kind <= INGOT_HDR_ULP);
    if (!ctx || !kind_ok) return INGOT_GPU_EINVAL;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_arena || !d_out) return INGOT_GPU_EINVAL;
    // single headers lie at any address: slots need no alignment here
    if (d_off) {
        if (!d_len) return INGOT_GPU_EINVAL;
        stride = 0;
    } else if (stride == 0 || stride > 65535u) {
        return INGOT_GPU_ERANGE;
    }
    if (int e = enter(ctx)) return e;
    HeaderArgs a{d_arena, d_off, d_len, stride, n, kind, d_hint, hint, d_out};
    return from_hip(launch_header(a, (hipStream_t)stream));
}

int ingot_gpu_parse(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                    const uint16_t* d_len, uint64_t n, int chain, ingot_rec* d_out,
                    void* stream) {
    return parse_frames(ctx, d_arena, d_off, d_len, 0, true, n, chain, d_out, OUT_REC16, stream);
}

int ingot_gpu_parse_strided(ingot_gpu_ctx* ctx, const uint8_t* d_arena, uint32_t stride,
                            const uint16_t* d_len, uint64_t n, int chain, ingot_rec* d_out,
                            void* stream) {
    return parse_frames(ctx, d_arena, nullptr, d_len, stride, false, n, chain, d_out, OUT_REC16,
                        stream);
}

int ingot_gpu_parse_ring(ingot_gpu_ctx* ctx, const ingot_ring_batch* batches, uint32_t nbatches,
                         uint32_t stride, uint64_t n, int chain, uint32_t record_bytes,
                         const ingot_gpu_doorbell* db, uint32_t db_first, uint32_t timeout_ms,
                         uint32_t* d_status, void* stream) {
    if (!ctx || !chain_ok(chain) || chain == INGOT_CHAIN_GENEVE_OVER_V6) return INGOT_GPU_EINVAL;
    if (record_bytes != 16 && record_bytes != 8) return INGOT_GPU_EINVAL;
    if (nbatches > INGOT_RING_MAX_BATCHES) return INGOT_GPU_ERANGE;
    if (stride < 64u || stride % 16u != 0 || stride > 65535u) return INGOT_GPU_ERANGE;
    if (db && (timeout_ms == 0 || timeout_ms > 60000u)) return INGOT_GPU_ERANGE;
    // the kernel compares the word with db_first + b (b < nbatches) in 32
    // bits: the largest, db_first + nbatches - 1, must not wrap
    if (db && nbatches && (uint64_t)db_first + nbatches - 1u > 0xffffffffull)
        return INGOT_GPU_ERANGE;
    if (db && db->device != ctx->device) return INGOT_GPU_EINVAL;
    if (nbatches == 0 || n == 0) return INGOT_GPU_SUCCESS;
    if (!batches) return INGOT_GPU_EINVAL;
    // the kernel's tile cursors are 32-bit
    const uint64_t tiles = (n + 63u) / 64u;
    if (tiles * nbatches >= (1ull << 31)) return INGOT_GPU_ERANGE;
    ingot_gpu::RingArgs a{};
    for (uint32_t b = 0; b < nbatches; ++b) {
        const ingot_ring_batch& x = batches[b];
        if (!x.d_arena || !x.d_out || ((uintptr_t)x.d_arena & 15u)) return INGOT_GPU_EINVAL;
        a.b[b] = ingot_gpu::RingBatch{x.d_arena, x.d_out};
    }
    if (db && !ctx->wall_khz) return INGOT_GPU_ENODEV;
    if (int e = enter(ctx)) return e;
    a.n = n;
    a.stride = stride;
    a.nbatches = nbatches;
    a.tiles_per_batch = (uint32_t)tiles;
    a.published = db ? 0u : nbatches;
    a.doorbell = db ? db->dword : nullptr;
    a.db_first = db_first;
    a.timeout_ticks = (uint64_t)timeout_ms * ctx->wall_khz;
    a.status = d_status;
    return from_hip(ingot_gpu::launch_ring(a, chain,
                                           record_bytes == 8 ? ingot_gpu::OUT_REC8
                                                             : ingot_gpu::OUT_REC16,
                                           tuning_for(ctx, batches[0].d_arena),
                                           (hipStream_t)stream));
}

int ingot_gpu_parse_compact(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                            const uint16_t* d_len, uint64_t n, int chain, ingot_rec8* d_out,
                            void* stream) {
    if (chain == INGOT_CHAIN_GENEVE_OVER_V6) return INGOT_GPU_EINVAL;
    return parse_frames(ctx, d_arena, d_off, d_len, 0, true, n, chain, d_out, OUT_REC8, stream);
}

int ingot_gpu_parse_strided_compact(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                                    uint32_t stride, const uint16_t* d_len, uint64_t n,
                                    int chain, ingot_rec8* d_out, void* stream) {
    if (chain == INGOT_CHAIN_GENEVE_OVER_V6) return INGOT_GPU_EINVAL;
    return parse_frames(ctx, d_arena, nullptr, d_len, stride, false, n, chain, d_out, OUT_REC8,
                        stream);
}

int ingot_gpu_fields(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                     const uint16_t* d_len, uint32_t stride, uint64_t n, int chain,
                     ingot_fields* d_out, void* stream) {
    if (chain == INGOT_CHAIN_GENEVE_OVER_V6) return INGOT_GPU_EINVAL;  // 384-B blocks
    return parse_frames(ctx, d_arena, d_off, d_len, stride, false, n, chain, d_out, OUT_FIELDS,
                        stream);
}

int ingot_gpu_geneve_fields(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                            const uint16_t* d_len, uint32_t stride, uint64_t n,
                            ingot_geneve_fields* d_out, void* stream) {
    return parse_frames(ctx, d_arena, d_off, d_len, stride, false, n, INGOT_CHAIN_GENEVE_OVER_V6,
                        d_out, OUT_FIELDS, stream);
}

int ingot_gpu_parse_read(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_seg_off,
                         const uint16_t* d_seg_len, const uint32_t* d_pkt_seg, uint64_t n,
                         int chain, ingot_rec* d_out, uint16_t* d_chunk, void* stream) {
    return parse_chunks(ctx, d_arena, d_seg_off, d_seg_len, d_pkt_seg, false, nullptr, n, chain,
                        d_out, d_chunk, OUT_REC16, stream);
}

int ingot_gpu_parse_read_first(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                               const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                               const uint32_t* d_pkt_seg, const uint64_t* d_first, uint64_t n,
                               int chain, ingot_rec* d_out, uint16_t* d_chunk, void* stream) {
    if (n != 0 && !d_first) return INGOT_GPU_EINVAL;
    return parse_chunks(ctx, d_arena, d_seg_off, d_seg_len, d_pkt_seg, false, d_first, n, chain,
                        d_out, d_chunk, OUT_REC16, stream);
}

int ingot_gpu_fields_read(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_seg_off,
                          const uint16_t* d_seg_len, const uint32_t* d_pkt_seg, uint64_t n,
                          int chain, ingot_fields* d_out, uint16_t* d_chunk, void* stream) {
    if (chain == INGOT_CHAIN_GENEVE_OVER_V6) return INGOT_GPU_EINVAL;  // 384-B blocks
    return parse_chunks(ctx, d_arena, d_seg_off, d_seg_len, d_pkt_seg, false, nullptr, n, chain,
                        d_out, d_chunk, OUT_FIELDS, stream);
}

int ingot_gpu_geneve_fields_read(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                                 const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                 const uint32_t* d_pkt_seg, uint64_t n,
                                 ingot_geneve_fields* d_out, uint16_t* d_chunk, void* stream) {
    return parse_chunks(ctx, d_arena, d_seg_off, d_seg_len, d_pkt_seg, false, nullptr, n,
                        INGOT_CHAIN_GENEVE_OVER_V6, d_out, d_chunk, OUT_FIELDS, stream);
}

int ingot_gpu_parse_read_dense(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_seg,
                               const uint32_t* d_pkt_seg, uint64_t n, int chain, int fields,
                               void* d_out, uint16_t* d_chunk, void* stream) {
    if (fields < 0 || fields > 2 || (fields == 1 && chain == INGOT_CHAIN_GENEVE_OVER_V6) ||
        (fields == 2 && chain != INGOT_CHAIN_GENEVE_OVER_V6))
        return INGOT_GPU_EINVAL;
    return parse_chunks(ctx, d_arena, d_seg, nullptr, d_pkt_seg, true, nullptr, n, chain, d_out,
                        d_chunk, fields ? OUT_FIELDS : OUT_REC16, stream);
}

int ingot_gpu_parse_modify(ingot_gpu_ctx* ctx, uint8_t* d_arena, const uint64_t* d_off,
                           const uint16_t* d_len, uint32_t stride, uint64_t n, int chain,
                           const ingot_edit* edits, uint32_t n_edits, ingot_rec* d_out,
                           void* stream) {
    return rewrite(ctx, d_arena, Packets{false, d_off, d_len, stride, nullptr, nullptr}, n, chain,
                   edits, n_edits, 0u, d_out, stream);
}

int ingot_gpu_parse_modify_csum(ingot_gpu_ctx* ctx, uint8_t* d_arena, const uint64_t* d_off,
                                const uint16_t* d_len, uint32_t stride, uint64_t n, int chain,
                                const ingot_edit* edits, uint32_t n_edits, uint32_t what,
                                ingot_rec* d_out, void* stream) {
    if (!what_ok(what, kRewriteSums, false, chain)) return INGOT_GPU_EINVAL;
    return rewrite(ctx, d_arena, Packets{false, d_off, d_len, stride, nullptr, nullptr}, n, chain,
                   edits, n_edits, what, d_out, stream);
}

int ingot_gpu_parse_modify_rows(ingot_gpu_ctx* ctx, uint8_t* d_arena, const uint64_t* d_off,
                                const uint16_t* d_len, uint32_t stride, uint64_t n, int chain,
                                const ingot_edit_rows* edits, uint32_t n_edits,
                                const uint32_t* d_row, uint32_t n_rows, uint32_t what,
                                ingot_rec* d_out, void* stream) {
    return rewrite_rows(ctx, d_arena, Packets{false, d_off, d_len, stride, nullptr, nullptr}, n,
                        chain, edits, n_edits, d_row, n_rows, what, d_out, stream);
}

int ingot_gpu_parse_read_modify(ingot_gpu_ctx* ctx, uint8_t* d_arena, const uint64_t* d_seg_off,
                                const uint16_t* d_seg_len, const uint32_t* d_pkt_seg, uint64_t n,
                                int chain, const ingot_edit* edits, uint32_t n_edits,
                                ingot_rec* d_out, uint16_t* d_chunk, void* stream) {
    return rewrite(ctx, d_arena, Packets{true, d_seg_off, d_seg_len, 0, d_pkt_seg, d_chunk}, n,
                   chain, edits, n_edits, 0u, d_out, stream);
}

int ingot_gpu_parse_read_modify_csum(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                                     const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                     const uint32_t* d_pkt_seg, uint64_t n, int chain,
                                     const ingot_edit* edits, uint32_t n_edits, uint32_t what,
                                     ingot_rec* d_out, uint16_t* d_chunk, void* stream) {
    if (!what_ok(what, kRewriteSums, false, chain)) return INGOT_GPU_EINVAL;
    return rewrite(ctx, d_arena, Packets{true, d_seg_off, d_seg_len, 0, d_pkt_seg, d_chunk}, n,
                   chain, edits, n_edits, what, d_out, stream);
}

int ingot_gpu_parse_read_modify_rows(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                                     const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                     const uint32_t* d_pkt_seg, uint64_t n, int chain,
                                     const ingot_edit_rows* edits, uint32_t n_edits,
                                     const uint32_t* d_row, uint32_t n_rows, uint32_t what,
                                     ingot_rec* d_out, uint16_t* d_chunk, void* stream) {
    return rewrite_rows(ctx, d_arena, Packets{true, d_seg_off, d_seg_len, 0, d_pkt_seg, d_chunk},
                        n, chain, edits, n_edits, d_row, n_rows, what, d_out, stream);
}

int ingot_gpu_emit_packets_rows(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                                const ingot_emit_set_rows* sets, uint32_t n_sets,
                                const ingot_emit_sum* sums, uint32_t n_sums,
                                const uint32_t* d_row, uint32_t n_rows, const uint8_t* d_src,
                                const uint64_t* d_off, const uint16_t* d_len, uint64_t n,
                                uint8_t* d_dst, const uint64_t* d_dst_off, void* stream) {
    if (!ctx) return INGOT_GPU_EINVAL;
    EmitRowsArgs a{};
    if (int e = emit_args(hdr, hdr_len, nullptr, 0, a.e)) return e;
    ingot_emit_set narrow[INGOT_MAX_EMIT_SETS];
    uint32_t n_narrow = 0;
    if (int e = emit_rows_pieces(sets, n_sets, d_row != nullptr, hdr_len, a, narrow, n_narrow))
        return e;
    if (int e = emit_sums(hdr, hdr_len, narrow, n_narrow, sums, n_sums, a.e)) return e;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_src || !d_off || !d_len || !d_dst || !d_dst_off) return INGOT_GPU_EINVAL;
    if (emit_rows_lds_bytes(a) > ctx->lds_bytes) return INGOT_GPU_ERANGE;
    if (int e = enter(ctx)) return e;
    a.e.src = d_src;
    a.e.off = d_off;
    a.e.len = d_len;
    a.e.dst = d_dst;
    a.e.dst_off = d_dst_off;
    a.e.n = n;
    a.row = d_row;
    a.n_rows = n_rows;
    return from_hip(launch_emit_rows(a, (hipStream_t)stream));
}

int ingot_gpu_emit_packets(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                           const ingot_emit_set* sets, uint32_t n_sets, const uint8_t* d_src,
                           const uint64_t* d_off, const uint16_t* d_len, uint64_t n,
                           uint8_t* d_dst, const uint64_t* d_dst_off, void* stream) {
    return emit_packets(ctx, hdr, hdr_len, sets, n_sets, nullptr, 0, d_src, d_off, d_len, n,
                        d_dst, d_dst_off, stream);
}

int ingot_gpu_emit_packets_csum(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                                const ingot_emit_set* sets, uint32_t n_sets,
                                const ingot_emit_sum* sums, uint32_t n_sums, const uint8_t* d_src,
                                const uint64_t* d_off, const uint16_t* d_len, uint64_t n,
                                uint8_t* d_dst, const uint64_t* d_dst_off, void* stream) {
    return emit_packets(ctx, hdr, hdr_len, sets, n_sets, sums, n_sums, d_src, d_off, d_len, n,
                        d_dst, d_dst_off, stream);
}

int ingot_gpu_emit_packets_read(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                                const ingot_emit_set* sets, uint32_t n_sets,
                                const ingot_emit_sum* sums, uint32_t n_sums, const uint8_t* d_src,
                                const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                const uint32_t* d_pkt_seg, const uint16_t* d_from,
                                const uint16_t* d_take, uint64_t n, uint8_t* d_dst,
                                const uint64_t* d_dst_off, uint16_t* d_taken, void* stream) {
    if (!ctx) return INGOT_GPU_EINVAL;
    EmitReadArgs a{};
    if (int e = emit_args(hdr, hdr_len, sets, n_sets, a.e)) return e;
    if (int e = emit_sums(hdr, hdr_len, sets, n_sets, sums, n_sums, a.e)) return e;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_dst || !d_dst_off) return INGOT_GPU_EINVAL;
    Frames f;
    if (int e = chunks_of(d_src, d_seg_off, d_seg_len, d_pkt_seg, n, nullptr, nullptr, f)) return e;
    if (int e = enter(ctx)) return e;
    a.e.src = d_src;
    a.e.dst = d_dst;
    a.e.dst_off = d_dst_off;
    a.e.n = n;
    a.seg_off = f.p.off;
    a.seg_len = f.p.len;
    a.pkt_seg = f.p.pkt_seg;
    a.from = d_from;
    a.take = d_take;
    a.taken = d_taken;
    if (emit_read_lds_bytes(a) > ctx->lds_bytes) return INGOT_GPU_ERANGE;
    return from_hip(launch_emit_read(a, (hipStream_t)stream));
}

int ingot_gpu_emit_packets_read_rows(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                                     const ingot_emit_set_rows* sets, uint32_t n_sets,
                                     const ingot_emit_sum* sums, uint32_t n_sums,
                                     const uint32_t* d_row, uint32_t n_rows,
                                     const uint8_t* d_src, const uint64_t* d_seg_off,
                                     const uint16_t* d_seg_len, const uint32_t* d_pkt_seg,
                                     const uint16_t* d_from, const uint16_t* d_take, uint64_t n,
                                     uint8_t* d_dst, const uint64_t* d_dst_off, uint16_t* d_taken,
                                     void* stream) {
    if (!ctx) return INGOT_GPU_EINVAL;
    // the header block, pieces and sums as ingot_gpu_emit_packets_rows makes
    // them, then moved behind the chunk tables' block
    EmitRowsArgs rows{};
    if (int e = emit_args(hdr, hdr_len, nullptr, 0, rows.e)) return e;
    ingot_emit_set narrow[INGOT_MAX_EMIT_SETS];
    uint32_t n_narrow = 0;
    if (int e = emit_rows_pieces(sets, n_sets, d_row != nullptr, hdr_len, rows, narrow, n_narrow))
        return e;
    if (int e = emit_sums(hdr, hdr_len, narrow, n_narrow, sums, n_sums, rows.e)) return e;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_dst || !d_dst_off) return INGOT_GPU_EINVAL;
    Frames f;
    if (int e = chunks_of(d_src, d_seg_off, d_seg_len, d_pkt_seg, n, nullptr, nullptr, f)) return e;
    EmitReadRowsArgs a{};
    a.r.e = rows.e;
    a.n_pieces = rows.n_pieces;
    std::memcpy(a.p, rows.p, sizeof a.p);
    if (emit_read_rows_lds_bytes(a) > ctx->lds_bytes) return INGOT_GPU_ERANGE;
    if (int e = enter(ctx)) return e;
    a.r.e.src = d_src;
    a.r.e.dst = d_dst;
    a.r.e.dst_off = d_dst_off;
    a.r.e.n = n;
    a.r.seg_off = f.p.off;
    a.r.seg_len = f.p.len;
    a.r.pkt_seg = f.p.pkt_seg;
    a.r.from = d_from;
    a.r.take = d_take;
    a.r.taken = d_taken;
    a.row = d_row;
    a.n_rows = n_rows;
    return from_hip(launch_emit_read_rows(a, (hipStream_t)stream));
}

int ingot_gpu_emit_headers(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                           const ingot_emit_set* sets, uint32_t n_sets, const uint16_t* d_len,
                           uint64_t n, uint8_t* d_out, const uint64_t* d_out_off,
                           uint32_t out_stride, void* stream) {
    if (!ctx) return INGOT_GPU_EINVAL;
    EmitArgs a{};
    if (int e = emit_args(hdr, hdr_len, sets, n_sets, a)) return e;
    if (!d_out_off && out_stride < hdr_len) return INGOT_GPU_ERANGE;  // blocks would overlap
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_len || !d_out || hdr_len == 0) return INGOT_GPU_EINVAL;
    if (int e = enter(ctx)) return e;
    a.len = d_len;
    a.dst = d_out;
    a.dst_off = d_out_off;
    a.stride = out_stride;
    a.n = n;
    if (emit_lds_bytes(a) > ctx->lds_bytes) return INGOT_GPU_ERANGE;
    return from_hip(launch_emit(a, (hipStream_t)stream));
}

int ingot_gpu_checksum_verify_read(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                                   const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                   const uint32_t* d_pkt_seg, uint64_t n, const ingot_rec* d_rec,
                                   uint32_t what, ingot_csum* d_out, void* stream) {
    return checksum(ctx, d_arena, Packets{true, d_seg_off, d_seg_len, 0, d_pkt_seg, nullptr}, n,
                    d_rec, what, d_out, false, stream);
}

int ingot_gpu_checksum_fill_read(ingot_gpu_ctx* ctx, uint8_t* d_arena, const uint64_t* d_seg_off,
                                 const uint16_t* d_seg_len, const uint32_t* d_pkt_seg, uint64_t n,
                                 const ingot_rec* d_rec, uint32_t what, ingot_csum* d_out,
                                 void* stream) {
    return checksum(ctx, d_arena, Packets{true, d_seg_off, d_seg_len, 0, d_pkt_seg, nullptr}, n,
                    d_rec, what, d_out, true, stream);
}

int ingot_gpu_checksum_verify(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                              const uint16_t* d_len, uint32_t stride, uint64_t n,
                              const ingot_rec* d_rec, uint32_t what, ingot_csum* d_out,
                              void* stream) {
    return checksum(ctx, d_arena, Packets{false, d_off, d_len, stride, nullptr, nullptr}, n, d_rec,
                    what, d_out, false, stream);
}

int ingot_gpu_checksum_fill(ingot_gpu_ctx* ctx, uint8_t* d_arena, const uint64_t* d_off,
                            const uint16_t* d_len, uint32_t stride, uint64_t n,
                            const ingot_rec* d_rec, uint32_t what, ingot_csum* d_out,
                            void* stream) {
    return checksum(ctx, d_arena, Packets{false, d_off, d_len, stride, nullptr, nullptr}, n, d_rec,
                    what, d_out, true, stream);
}

int ingot_gpu_flow_hist_ws(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                           const uint16_t* d_len, uint32_t stride, uint64_t n, int chain,
                           const uint8_t* key, uint32_t bins, uint32_t* d_flow, uint32_t* d_hash,
                           uint32_t* d_hist, void* d_work, size_t work_bytes, void* stream) {
    // The standard Microsoft RSS key (the one its published verification
    // vectors use; tests/test_flows.py).
    static const uint8_t kRssKey[INGOT_FLOW_KEY_BYTES] = {
        0x6d, 0x5a, 0x56, 0xda, 0x25, 0x5b, 0x0e, 0xc2, 0x41, 0x67, 0x25, 0x3d, 0x43, 0xa3,
        0x8f, 0xb0, 0xd0, 0xca, 0x2b, 0xcb, 0xae, 0x7b, 0x30, 0xb4, 0x77, 0xcb, 0x2d, 0xa3,
        0x80, 0x30, 0xf2, 0x0c, 0x6a, 0x42, 0xb7, 0x3b, 0xbe, 0xac, 0x01, 0xfa};
    if (!ctx || !chain_ok(chain)) return INGOT_GPU_EINVAL;
    if (!bins_ok(bins)) return INGOT_GPU_ERANGE;
    if (n == 0) return INGOT_GPU_SUCCESS;
    if (!d_flow) return INGOT_GPU_EINVAL;
    Frames f;
    if (int e = frames_of(d_arena, d_off, d_len, stride, n, nullptr, f)) return e;
    if (int e = enter(ctx)) return e;
    const int layout = f.layout;
    const uint8_t* k = key ? key : kRssKey;
    FlowArgs a{};
    a.p = f.p;
    a.flow = d_flow;
    a.bin_mask = bins - 1u;
    a.hash = d_hash;
    for (uint32_t b = 0; b < ingot_gpu::FLOW_INPUT_BITS; ++b) {
        uint32_t w = 0;
        for (uint32_t j = 0; j < 32; ++j) {
            const uint32_t bit = b + j;
            w = (w << 1) | ((k[bit >> 3] >> (7u - (bit & 7u))) & 1u);
        }
        a.w[b] = w;
    }
    // the 16-bit table: entry (p, v) = low 16 bits of the XOR of the windows
    // of v's set bits at nibble position p (bit 3 of v = input bit 4p)
    for (uint32_t e = 0; e < 2 * ingot_gpu::FLOW_TAB16_DW; ++e) {
        const uint32_t p = e / 16u, v = e & 15u;
        uint32_t acc = 0;
        for (uint32_t j = 0; j < 4; ++j)
            if ((v >> (3u - j)) & 1u) acc ^= a.w[4u * p + j];
        a.tab16[e / 2] |= (acc & 0xffffu) << (16u * (e & 1u));
    }
    const hipStream_t s = (hipStream_t)stream;
    if (int e = from_hip(ingot_gpu::launch_flows(a, layout, chain, tuning_for(ctx, d_arena), s)))
        return e;
    if (!d_hist) return INGOT_GPU_SUCCESS;
    return from_hip(ingot_gpu::launch_flow_hist(d_flow, n, d_hist, bins, d_work, work_bytes, s));
}

int ingot_gpu_flow_hist(ingot_gpu_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                        const uint16_t* d_len, uint32_t stride, uint64_t n, int chain,
                        const uint8_t* key, uint32_t bins, uint32_t* d_flow, uint32_t* d_hash,
                        uint32_t* d_hist, void* stream) {
    return ingot_gpu_flow_hist_ws(ctx, d_arena, d_off, d_len, stride, n, chain, key, bins, d_flow,
                                  d_hash, d_hist, nullptr, 0, stream);
}

size_t ingot_gpu_flow_hist_workspace_size(uint64_t n, uint32_t bins) {
    return bins_ok(bins) ? flow_hist_workspace(n, bins) : 0;
}

const char* ingot_gpu_strerror(int code) {
    switch (code) {
    case INGOT_GPU_SUCCESS: return "success";
    case INGOT_GPU_EINVAL: return "invalid argument";
    case INGOT_GPU_EHIP: return "HIP runtime error";
    case INGOT_GPU_ENOMEM: return "out of host memory";
    case INGOT_GPU_ENODEV: return "no such gfx950 device";
    case INGOT_GPU_ERANGE: return "size outside the supported range";
    case INGOT_GPU_ECOMM: return "collective (RCCL) call failed";
    default: return "unknown error";
    }
}

const char* ingot_parse_error_name(int status) {
    if (status < 0 || status > INGOT_ERR_ILLEGAL_VALUE) return nullptr;
    return kParseErrorNames[status];
}

int ingot_chain_layer_count(int chain) {
    switch (chain) {
    case INGOT_CHAIN_UDP_PARSER: return 3;
    case INGOT_CHAIN_GENERIC_ULP: return 3;
    case INGOT_CHAIN_VLAN_ULP: return 4;
    case INGOT_CHAIN_GENEVE_OVER_V6: return 7;
    default: return -1;
    }
}

const char* ingot_chain_layer_label(int chain, int layer) {
    if (layer < 0 || layer >= ingot_chain_layer_count(chain)) return nullptr;
    switch (chain) {
    case INGOT_CHAIN_UDP_PARSER: return kUdpParserLabels[layer];
    case INGOT_CHAIN_GENERIC_ULP: return kGenericUlpLabels[layer];
    case INGOT_CHAIN_VLAN_ULP: return kVlanUlpLabels[layer];
    default: return kGeneveLabels[layer];
    }
}

}  // extern "C"
