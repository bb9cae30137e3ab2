// api_args_selftest.cpp — the C API's host layer (ingot_amd/csrc/api.cpp and,
// where the tree has it, resolve.cpp) run as a stand-alone program with no GPU:
// for a fixed corpus of calls, the return code of every call, the launcher it
// reached and every field of the argument block it built.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -Iinclude
//       tools/api_args_selftest.cpp -o tools/bin/api_args_selftest
//   && tools/bin/api_args_selftest [--verbose]
//
// (for a sanitizer run add -g -Xarch_host -fsanitize=address,undefined
//  -Xarch_host -fno-sanitize-recover=all)
//
// The API sources are compiled into the program.  hipGetDevice / hipSetDevice
// and every launcher, LDS-size and workspace function of kernels.h are defined
// here as stubs that write what they were given into a log; the context is a
// stack ingot_gpu_ctx and the "device" pointers are fixed numbers that are
// never dereferenced.  One line per group: its name, the number of cases and a
// 64-bit FNV-1a digest over the text of each case (label, return code,
// launchers and their fields, printed field by field: padding never enters).
// --verbose prints the cases.  tests/golden/api_args.txt is this output;
// tests/test_api_args.py compares.  A change to the host layer that keeps every
// return code and every argument block keeps the output.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../ingot_amd/csrc/api.cpp"
#if __has_include("../ingot_amd/csrc/resolve.cpp")
#include "../ingot_amd/csrc/resolve.cpp"
#endif

namespace ig = ingot_gpu;

// ---------------------------------------------------------------- the log
static std::string g_log;           // what the stubs saw during the current case
static bool g_no_device = false;    // hipGetDevice fails
static bool g_fail_launch = false;  // every launcher fails
static int g_cur_device = 0;

static void put(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    const int k = std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_log.append(buf, (size_t)(k < (int)sizeof buf ? k : (int)sizeof buf - 1));
}

#define U(x) ((unsigned long long)(x))
#define A(x) ((unsigned long long)(uintptr_t)(x))

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
constexpr uint64_t kFnv0 = 0xcbf29ce484222325ull;

static uint64_t words(const uint32_t* w, size_t n) {  // a digest of n values (no padding in them)
    uint64_t h = kFnv0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t v = w[i];
        const unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8),
                                    (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
        h = fnv(h, b, 4);
    }
    return h;
}

extern "C" hipError_t hipGetDevice(int* d) {
    put("hipGetDevice ");
    if (g_no_device) return hipErrorNoDevice;
    *d = g_cur_device;
    return hipSuccess;
}
extern "C" hipError_t hipSetDevice(int d) {
    put("hipSetDevice(%d) ", d);
    g_cur_device = d;
    return hipSuccess;
}

static hipError_t done() {
    put("; ");
    return g_fail_launch ? hipErrorUnknown : hipSuccess;
}

static void put_parse(const ig::ParseArgs& a) {
    put("p{arena=%llx off=%llx len=%llx stride=%llu n=%llu out=%llx pkt_seg=%llx chunk=%llx "
        "off_out=%llx tile_local=%llx policy=%llu linewin=%llu first=%llx xcd=%llu} ",
        A(a.arena), A(a.off), A(a.len), U(a.stride), U(a.n), A(a.out), A(a.pkt_seg), A(a.chunk),
        A(a.off_out), A(a.tile_local), U(a.policy), U(a.linewin), A(a.first), U(a.xcd_remap));
}

static void put_tuning(const ig::Tuning& t) {
    put("t{wi=%d ws=%d mb=%llu pipe=%d depth=%d wb=%d cache=%d ft=%d slow=%d plan=%d fk=%d "
        "rg=%d rgr=%d xcd=%d cus=%llu host=%d} ",
        t.window_indexed, t.window_strided, U(t.max_blocks), t.pipeline, t.pipe_depth,
        t.writeback, t.cache_policy, t.flow_table, t.slow_path, t.read_plan, t.flow_kernel,
        t.ring_grid, t.ring_groups, t.xcd_remap, U(t.cus), (int)t.host_arena);
}

static void put_edit(const ig::Edit& e) {
    put("e{%u %u %u %u b0=%u nb=%u rs=%u bits=%u v=%llx} ", e.layer, e.kind, e.op, e.index,
        e.byte0, e.nbytes, e.rshift, e.bits, U(e.value));
}
static bool zero(const ig::Edit& e) {
    return !(e.layer | e.kind | e.op | e.index | e.byte0 | e.nbytes | e.rshift | e.bits | e.value);
}

static void put_modify(const ig::ModifyArgs& a) {
    put_parse(a.p);
    put("wb=%llu n_edits=%llu ", U(a.wb), U(a.n_edits));
    for (uint32_t k = 0; k < INGOT_MAX_EDITS; ++k)
        if (k < a.n_edits || !zero(a.e[k])) put("[%u]", k), put_edit(a.e[k]);
}

static void put_modify_csum(const ig::ModifyCsumArgs& a) {
    put_modify(a.m);
    put("what=%llu feeds=", U(a.what));
    for (uint32_t k = 0; k < INGOT_MAX_EDITS; ++k)
        if (k < a.m.n_edits || a.feeds[k]) put("%u:%u,", k, a.feeds[k]);
}

static void put_modify_rows(const ig::ModifyRowsArgs& a) {
    put_parse(a.p);
    put("row=%llx n_rows=%llu what=%llu n_pieces=%llu ", A(a.row), U(a.n_rows), U(a.what),
        U(a.n_pieces));
    for (uint32_t k = 0; k < ig::ROWS_MAX_PIECES; ++k) {
        const ig::RowPiece& r = a.e[k];
        const bool z = zero(r.e) && !(r.source | r.by | r.feeds | r._pad | r.pitch) && !r.values;
        if (k >= a.n_pieces && z) continue;
        put("[%u]", k);
        put_edit(r.e);
        put("src=%u by=%u feeds=%u pad=%u pitch=%llu values=%llx ", r.source, r.by, r.feeds,
            r._pad, U(r.pitch), A(r.values));
    }
}

static void put_emit(const ig::EmitArgs& a) {
    put("src=%llx off=%llx len=%llx dst=%llx dst_off=%llx stride=%llu hdr_len=%llu n=%llu "
        "n_sets=%llu ",
        A(a.src), A(a.off), A(a.len), A(a.dst), A(a.dst_off), U(a.stride), U(a.hdr_len), U(a.n),
        U(a.n_sets));
    for (uint32_t k = 0; k < INGOT_MAX_EMIT_SETS; ++k) {
        const ig::EmitSet& s = a.sets[k];
        const bool z =
            !(s.pos | s.at | s.nbytes | s.rshift | s.bits | s.source | s.add) && !s.values;
        if (k >= a.n_sets && z) continue;
        put("[%u]{pos=%u at=%u nb=%u rs=%u bits=%u src=%u add=%d values=%llx} ", k, s.pos, s.at,
            s.nbytes, s.rshift, s.bits, s.source, (int)s.add, A(s.values));
    }
    put("hdr=%016llx sums{%u %u %u %u v4=%u udp=%u v6=%u pad=%u} ",
        U(words(a.hdr, INGOT_MAX_EMIT_HDR / 4)), a.sums.v4_at, a.sums.v4_len, a.sums.udp_at,
        a.sums.udp_l3, a.sums.v4, a.sums.udp, a.sums.udp_v6, a.sums._pad);
}

static void put_emit_rows(const ig::EmitRowsArgs& a) {
    put_emit(a.e);
    put("row=%llx n_rows=%llu n_pieces=%llu ", A(a.row), U(a.n_rows), U(a.n_pieces));
    for (uint32_t k = 0; k < ig::EMIT_MAX_PIECES; ++k) {
        const ig::EmitPiece& p = a.p[k];
        const bool z = !(p.pos | p.at | p.nbytes | p.rshift | p.bits | p.source | p.by |
                         p._pad[0] | p._pad[1] | p._pad[2] | p.add | p.pitch) &&
                       !p.values;
        if (k >= a.n_pieces && z) continue;
        put("[%u]{pos=%u at=%u nb=%u rs=%u bits=%u src=%u by=%u pad=%u%u%u add=%d pitch=%llu "
            "values=%llx} ",
            k, p.pos, p.at, p.nbytes, p.rshift, p.bits, p.source, p.by, p._pad[0], p._pad[1],
            p._pad[2], (int)p.add, U(p.pitch), A(p.values));
    }
}

// ---------------------------------------------------------------- the stubs
namespace ingot_gpu {

hipError_t launch_parse(const ParseArgs& a, int layout, int chain, int mode, const Tuning& t,
                        hipStream_t s) {
    put("launch_parse(layout=%d chain=%d mode=%d s=%llx ", layout, chain, mode, A(s));
    put_parse(a);
    put_tuning(t);
    return done();
}
hipError_t launch_flows(const FlowArgs& a, int layout, int chain, const Tuning& t, hipStream_t s) {
    put("launch_flows(layout=%d chain=%d s=%llx ", layout, chain, A(s));
    put_parse(a.p);
    put("flow=%llx mask=%llx hash=%llx w=%016llx tab16=%016llx ", A(a.flow), U(a.bin_mask),
        A(a.hash), U(words(a.w, FLOW_INPUT_BITS)), U(words(a.tab16, FLOW_TAB16_DW)));
    put_tuning(t);
    return done();
}
hipError_t launch_ring(const RingArgs& a, int chain, int mode, const Tuning& t, hipStream_t s) {
    put("launch_ring(chain=%d mode=%d s=%llx n=%llu stride=%llu nb=%llu policy=%llu pub=%llu "
        "db=%llx first=%llu tpb=%llu ticks=%llu status=%llx groups=%llu ",
        chain, mode, A(s), U(a.n), U(a.stride), U(a.nbatches), U(a.policy), U(a.published),
        A(a.doorbell), U(a.db_first), U(a.tiles_per_batch), U(a.timeout_ticks), A(a.status),
        U(a.groups));
    for (uint32_t b = 0; b < INGOT_RING_MAX_BATCHES; ++b)
        if (b < a.nbatches || a.b[b].arena || a.b[b].out)
            put("[%u]%llx>%llx ", b, A(a.b[b].arena), A(a.b[b].out));
    put_tuning(t);
    return done();
}
hipError_t launch_flow_hist(const uint32_t* flow, uint64_t n, uint32_t* hist, uint32_t bins,
                            void* work, size_t work_bytes, hipStream_t s) {
    put("launch_flow_hist(flow=%llx n=%llu hist=%llx bins=%llu work=%llx bytes=%llu s=%llx ",
        A(flow), U(n), A(hist), U(bins), A(work), U(work_bytes), A(s));
    return done();
}
size_t flow_hist_workspace(uint64_t n, uint32_t bins) { return (size_t)(n + 4u * bins); }
hipError_t launch_header(const HeaderArgs& a, hipStream_t s) {
    put("launch_header(s=%llx arena=%llx off=%llx len=%llx stride=%llu n=%llu kind=%d "
        "hints=%llx hint=%llu out=%llx ",
        A(s), A(a.arena), A(a.off), A(a.len), U(a.stride), U(a.n), a.kind, A(a.hints), U(a.hint),
        A(a.out));
    return done();
}
size_t emit_lds_bytes(const EmitArgs& a) {
    put("emit_lds_bytes ");
    return 4096u + a.hdr_len + 64u * a.n_sets;
}
hipError_t launch_emit(const EmitArgs& a, hipStream_t s) {
    put("launch_emit(s=%llx ", A(s));
    put_emit(a);
    return done();
}
size_t emit_rows_lds_bytes(const EmitRowsArgs& a) {
    put("emit_rows_lds_bytes ");
    return 4096u + a.e.hdr_len + 32u * a.n_pieces;
}
hipError_t launch_emit_rows(const EmitRowsArgs& a, hipStream_t s) {
    put("launch_emit_rows(s=%llx ", A(s));
    put_emit_rows(a);
    return done();
}
size_t emit_read_lds_bytes(const EmitReadArgs& a) {
    put("emit_read_lds_bytes ");
    return 8192u + a.e.hdr_len + 64u * a.e.n_sets;
}
hipError_t launch_emit_read(const EmitReadArgs& a, hipStream_t s) {
    put("launch_emit_read(s=%llx ", A(s));
    put_emit(a.e);
    put("seg_off=%llx seg_len=%llx pkt_seg=%llx from=%llx take=%llx taken=%llx ", A(a.seg_off),
        A(a.seg_len), A(a.pkt_seg), A(a.from), A(a.take), A(a.taken));
    return done();
}
// ingot_gpu_emit_packets_read_rows: linked, and in no group of the corpus
// (tools/emit_read_rows_selftest.cpp has its argument checks)
size_t emit_read_rows_lds_bytes(const EmitReadRowsArgs& a) {
    put("emit_read_rows_lds_bytes ");
    return 8192u + a.r.e.hdr_len + 32u * a.n_pieces;
}
hipError_t launch_emit_read_rows(const EmitReadRowsArgs& a, hipStream_t s) {
    put("launch_emit_read_rows(s=%llx ", A(s));
    put_emit(a.r.e);
    return done();
}
hipError_t launch_csum(const CsumArgs& a, hipStream_t s) {
    put("launch_csum(s=%llx arena=%llx off=%llx len=%llx stride=%llu what=%llu n=%llu rec=%llx "
        "out=%llx fill=%llu ",
        A(s), A(a.arena), A(a.off), A(a.len), U(a.stride), U(a.what), U(a.n), A(a.rec), A(a.out),
        U(a.fill));
    return done();
}
hipError_t launch_csum_read(const CsumReadArgs& a, hipStream_t s) {
    put("launch_csum_read(s=%llx arena=%llx seg_off=%llx seg_len=%llx pkt_seg=%llx n=%llu "
        "rec=%llx out=%llx what=%llu fill=%llu ",
        A(s), A(a.arena), A(a.seg_off), A(a.seg_len), A(a.pkt_seg), U(a.n), A(a.rec), A(a.out),
        U(a.what), U(a.fill));
    return done();
}
size_t packed_workspace(uint64_t n) { return (size_t)(((n + 63) / 64) * 4 + 1024); }
hipError_t launch_tile_bases(const uint16_t* len, uint64_t n, void* work, hipStream_t s) {
    put("launch_tile_bases(len=%llx n=%llu work=%llx s=%llx ", A(len), U(n), A(work), A(s));
    return done();
}
hipError_t launch_delay(uint64_t ticks, hipStream_t s) {
    put("launch_delay(ticks=%llu s=%llx ", U(ticks), A(s));
    return done();
}
hipError_t launch_modify(const ModifyArgs& a, int layout, int chain, const Tuning& t,
                         hipStream_t s) {
    put("launch_modify(layout=%d chain=%d s=%llx ", layout, chain, A(s));
    put_modify(a);
    put_tuning(t);
    return done();
}
hipError_t launch_modify_csum(const ModifyCsumArgs& a, int layout, int chain, const Tuning& t,
                              hipStream_t s) {
    put("launch_modify_csum(layout=%d chain=%d s=%llx ", layout, chain, A(s));
    put_modify_csum(a);
    put_tuning(t);
    return done();
}
hipError_t launch_modify_rows(const ModifyRowsArgs& a, int layout, int chain, const Tuning& t,
                              hipStream_t s) {
    put("launch_modify_rows(layout=%d chain=%d s=%llx ", layout, chain, A(s));
    put_modify_rows(a);
    put_tuning(t);
    return done();
}
hipError_t launch_read_modify(const ModifyArgs& a, int chain, const Tuning& t, hipStream_t s) {
    put("launch_read_modify(chain=%d s=%llx ", chain, A(s));
    put_modify(a);
    put_tuning(t);
    return done();
}
hipError_t launch_read_modify_csum(const ModifyCsumArgs& a, int chain, const Tuning& t,
                                   hipStream_t s) {
    put("launch_read_modify_csum(chain=%d s=%llx ", chain, A(s));
    put_modify_csum(a);
    put_tuning(t);
    return done();
}
hipError_t launch_read_modify_rows(const ModifyRowsArgs& a, int chain, const Tuning& t,
                                   hipStream_t s) {
    put("launch_read_modify_rows(chain=%d s=%llx ", chain, A(s));
    put_modify_rows(a);
    put_tuning(t);
    return done();
}
bool tuning_valid(int key, int value) { return key >= 1 && key <= 14 && value >= 0; }

}  // namespace ingot_gpu

// ---------------------------------------------------------------- groups and cases
static bool g_verbose = false;
static const char* g_group = nullptr;
static uint64_t g_cases = 0, g_hash = kFnv0;

static void begin(const char* name) {
    g_group = name;
    g_cases = 0;
    g_hash = kFnv0;
}
static void end() {
    std::printf("%-22s %8llu %016llx\n", g_group, U(g_cases), U(g_hash));
}
// one case: its label, the return code, what the stubs logged
static void rec(int rc, const char* fmt, ...) {
    char label[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(label, sizeof label, fmt, ap);
    va_end(ap);
    char head[320];
    const int k = std::snprintf(head, sizeof head, "%s -> %d : ", label, rc);
    g_hash = fnv(g_hash, head, (size_t)k);
    g_hash = fnv(g_hash, g_log.data(), g_log.size());
    g_hash = fnv(g_hash, "\n", 1);
    ++g_cases;
    if (g_verbose) std::printf("%s/%s%s\n", g_group, head, g_log.c_str());
    g_log.clear();
}

// ---------------------------------------------------------------- fixed operands
// "Device" addresses: never dereferenced on the host.
constexpr uintptr_t kArena = 0x10000, kOff = 0x20000, kLen = 0x30000, kOut = 0x40000,
                    kSegOff = 0x50000, kSegLen = 0x60000, kPktSeg = 0x70000, kChunk = 0x80000,
                    kRow = 0x90000, kTab = 0xa0000, kRec = 0xb0000, kDst = 0xc0000,
                    kDstOff = 0xd0000, kWork = 0xe0000, kFlow = 0xf0000, kHash = 0x110000,
                    kHist = 0x120000, kFirst = 0x130000, kFrom = 0x140000, kTake = 0x150000,
                    kTaken = 0x160000, kHint = 0x170000, kStatus = 0x180000, kOffOut = 0x190000;
static void* const kStream = (void*)0x5000;

struct Env {
    ingot_gpu_ctx* ctx = nullptr;
    int chain = INGOT_CHAIN_GENERIC_ULP;
    uint64_t n = 100;
    uint32_t null = 0;  // bit k: the entry's pointer k is NULL
    uint32_t stride = 128;
    uintptr_t arena = kArena;
    template <class T>
    T* p(int k, uintptr_t v) const {
        return (null >> k) & 1u ? nullptr : reinterpret_cast<T*>(v);
    }
};

static const ingot_edit kEdits[2] = {{0, INGOT_F_ETH_ETHERTYPE, INGOT_OP_SET, 0, 0x0800},
                                     {2, INGOT_F_UDP_SOURCE, INGOT_OP_ADD, 0, 1}};

static ingot_edit_rows mk_edit(uint8_t layer, uint8_t field, uint8_t op, uint32_t value,
                               uint8_t source, uint8_t by, uint32_t pitch, const void* values) {
    ingot_edit_rows e{};
    e.layer = layer;
    e.field = field;
    e.op = op;
    e.value = value;
    e.source = source;
    e.by = by;
    e.pitch = pitch;
    e.d_values = values;
    return e;
}
static ingot_emit_set_rows mk_set(uint16_t at, uint8_t field, uint8_t source, int32_t add,
                                  uint8_t by, uint32_t pitch, const void* values) {
    ingot_emit_set_rows s{};
    s.at = at;
    s.field = field;
    s.source = source;
    s.add = add;
    s.by = by;
    s.pitch = pitch;
    s.d_values = values;
    return s;
}

static const ingot_edit_rows kEditRows[3] = {
    mk_edit(0, INGOT_F_ETH_ETHERTYPE, INGOT_OP_SET, 0x86dd, INGOT_EDIT_VALUE, 0, 0, nullptr),
    mk_edit(1, INGOT_FW_V6_SOURCE, INGOT_OP_SET, 0, INGOT_EDIT_BYTES, INGOT_BY_ROW, 32,
            (const void*)kTab),
    mk_edit(2, INGOT_F_UDP_SOURCE, INGOT_OP_XOR, 0, INGOT_EDIT_U16, INGOT_BY_PACKET, 0,
            (const void*)(kTab + 16))};

// Ethernet / IPv6 / UDP / Geneve, 70 bytes
static std::vector<uint8_t> opte_hdr() {
    std::vector<uint8_t> h(70, 0);
    h[12] = 0x86;
    h[13] = 0xdd;
    h[14] = 0x60;
    h[20] = 17;
    for (size_t i = 22; i < 70; ++i) h[i] = (uint8_t)(i * 7u);
    return h;
}
// Ethernet / IPv4 / UDP / Geneve, 50 bytes (the stack of tests/test_emit_csum.py's argument test)
static std::vector<uint8_t> v4_hdr() {
    std::vector<uint8_t> h(50, 0);
    h[0] = 0xa2;
    h[12] = 0x08;
    h[14] = 0x45;
    h[23] = 17;
    for (size_t i = 26; i < 50; ++i) h[i] = (uint8_t)(i * 5u);
    return h;
}
static const std::vector<uint8_t> kOpte = opte_hdr(), kV4 = v4_hdr();
static const ingot_emit_set kSets[3] = {
    {14, INGOT_F_V6_PAYLOAD_LEN, INGOT_EMIT_LENGTH, -40, nullptr},
    {54, INGOT_F_UDP_SOURCE, INGOT_EMIT_U16, 3, (const void*)kTab},
    {62, INGOT_F_GENEVE_VNI, INGOT_EMIT_VALUE, 77, nullptr}};
static const ingot_emit_set_rows kSetRows[3] = {
    mk_set(14, INGOT_F_V6_PAYLOAD_LEN, INGOT_EMIT_LENGTH, -40, 0, 0, nullptr),
    mk_set(14, INGOT_FW_V6_DESTINATION, INGOT_EMIT_BYTES, 0, INGOT_BY_ROW, 32, (const void*)kTab),
    mk_set(62, INGOT_F_GENEVE_VNI, INGOT_EMIT_U32, 5, INGOT_BY_PACKET, 0, (const void*)kTab)};
static const ingot_emit_sum kSumUdp6[1] = {{54, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}}};

// ---------------------------------------------------------------- the calls
// The six rewrites.  form: 0 plain, 1 with sums; bits 0.. of `null`: arena, the
// two or three tables, the list, d_out, (chunks) d_chunk, (rows) d_row.
static int rewrite(const Env& v, bool chunks, int form, const ingot_edit* e, uint32_t ne,
                   uint32_t what) {
    uint8_t* arena = v.p<uint8_t>(0, v.arena);
    if (!chunks) {
        const uint64_t* off = v.p<const uint64_t>(1, kOff);
        const uint16_t* len = v.p<const uint16_t>(2, kLen);
        ingot_rec* out = v.p<ingot_rec>(4, kOut);
        return form ? ingot_gpu_parse_modify_csum(v.ctx, arena, off, len, v.stride, v.n, v.chain,
                                                  e, ne, what, out, kStream)
                    : ingot_gpu_parse_modify(v.ctx, arena, off, len, v.stride, v.n, v.chain, e,
                                             ne, out, kStream);
    }
    const uint64_t* so = v.p<const uint64_t>(1, kSegOff);
    const uint16_t* sl = v.p<const uint16_t>(2, kSegLen);
    const uint32_t* ps = v.p<const uint32_t>(3, kPktSeg);
    ingot_rec* out = v.p<ingot_rec>(5, kOut);
    uint16_t* chunk = v.p<uint16_t>(6, kChunk);
    return form ? ingot_gpu_parse_read_modify_csum(v.ctx, arena, so, sl, ps, v.n, v.chain, e, ne,
                                                   what, out, chunk, kStream)
                : ingot_gpu_parse_read_modify(v.ctx, arena, so, sl, ps, v.n, v.chain, e, ne, out,
                                              chunk, kStream);
}
static int rewrite_rows(const Env& v, bool chunks, const ingot_edit_rows* e, uint32_t ne,
                        bool row, uint32_t what) {
    uint8_t* arena = v.p<uint8_t>(0, v.arena);
    const uint32_t* r = row ? v.p<const uint32_t>(7, kRow) : nullptr;
    if (!chunks)
        return ingot_gpu_parse_modify_rows(v.ctx, arena, v.p<const uint64_t>(1, kOff),
                                           v.p<const uint16_t>(2, kLen), v.stride, v.n, v.chain, e,
                                           ne, r, 9, what, v.p<ingot_rec>(4, kOut), kStream);
    return ingot_gpu_parse_read_modify_rows(
        v.ctx, arena, v.p<const uint64_t>(1, kSegOff), v.p<const uint16_t>(2, kSegLen),
        v.p<const uint32_t>(3, kPktSeg), v.n, v.chain, e, ne, r, 9, what, v.p<ingot_rec>(5, kOut),
        v.p<uint16_t>(6, kChunk), kStream);
}

// The five emits.  which: 0 packets, 1 packets_csum, 2 packets_read, 3 headers,
// 4 packets_rows (set list converted: `rows` given instead of `sets`).
struct EmitIn {
    const uint8_t* hdr = nullptr;
    uint32_t hdr_len = 0;
    const ingot_emit_set* sets = nullptr;
    const ingot_emit_set_rows* rows = nullptr;
    uint32_t n_sets = 0;
    const ingot_emit_sum* sums = nullptr;
    uint32_t n_sums = 0;
    bool row = true;
    uint32_t out_stride = 512;
};
static int emit(const Env& v, int which, const EmitIn& in) {
    // bits of `null`: 0 hdr, 1 sets, 2 sums, 3 src / d_len (headers), 4 .. per call
    const uint8_t* hdr = v.p<const uint8_t>(0, (uintptr_t)in.hdr);
    const ingot_emit_set* sets = v.p<const ingot_emit_set>(1, (uintptr_t)in.sets);
    const ingot_emit_sum* sums = v.p<const ingot_emit_sum>(2, (uintptr_t)in.sums);
    const uint8_t* src = v.p<const uint8_t>(3, v.arena);
    switch (which) {
    case 0:
        return ingot_gpu_emit_packets(v.ctx, hdr, in.hdr_len, sets, in.n_sets, src,
                                      v.p<const uint64_t>(4, kOff), v.p<const uint16_t>(5, kLen),
                                      v.n, v.p<uint8_t>(6, kDst), v.p<const uint64_t>(7, kDstOff),
                                      kStream);
    case 1:
        return ingot_gpu_emit_packets_csum(
            v.ctx, hdr, in.hdr_len, sets, in.n_sets, sums, in.n_sums, src,
            v.p<const uint64_t>(4, kOff), v.p<const uint16_t>(5, kLen), v.n, v.p<uint8_t>(6, kDst),
            v.p<const uint64_t>(7, kDstOff), kStream);
    case 2:
        return ingot_gpu_emit_packets_read(
            v.ctx, hdr, in.hdr_len, sets, in.n_sets, sums, in.n_sums, src,
            v.p<const uint64_t>(4, kSegOff), v.p<const uint16_t>(5, kSegLen),
            v.p<const uint32_t>(6, kPktSeg), v.p<const uint16_t>(7, kFrom),
            v.p<const uint16_t>(8, kTake), v.n, v.p<uint8_t>(9, kDst),
            v.p<const uint64_t>(10, kDstOff), v.p<uint16_t>(11, kTaken), kStream);
    case 3:
        return ingot_gpu_emit_headers(v.ctx, hdr, in.hdr_len, sets, in.n_sets,
                                      v.p<const uint16_t>(3, kLen), v.n, v.p<uint8_t>(4, kDst),
                                      v.p<const uint64_t>(5, kDstOff), in.out_stride, kStream);
    default:
        return ingot_gpu_emit_packets_rows(
            v.ctx, hdr, in.hdr_len, v.p<const ingot_emit_set_rows>(1, (uintptr_t)in.rows),
            in.n_sets, sums, in.n_sums, in.row ? v.p<const uint32_t>(8, kRow) : nullptr, 9, src,
            v.p<const uint64_t>(4, kOff), v.p<const uint16_t>(5, kLen), v.n,
            v.p<uint8_t>(6, kDst), v.p<const uint64_t>(7, kDstOff), kStream);
    }
}
static const char* const kEmitNames[5] = {"emit_packets", "emit_packets_csum", "emit_packets_read",
                                          "emit_headers", "emit_packets_rows"};
// a narrow list as the rows call takes it
static std::vector<ingot_emit_set_rows> as_rows(const ingot_emit_set* s, uint32_t n) {
    std::vector<ingot_emit_set_rows> r;
    for (uint32_t k = 0; k < n; ++k)
        r.push_back(mk_set(s[k].at, s[k].field, s[k].source, s[k].add, 0, 0, s[k].d_values));
    return r;
}
static int emit_any(const Env& v, int which, const std::vector<uint8_t>& hdr,
                    const std::vector<ingot_emit_set>& sets,
                    const std::vector<ingot_emit_sum>& sums) {
    const std::vector<ingot_emit_set_rows> rows = as_rows(sets.data(), (uint32_t)sets.size());
    EmitIn in;
    in.hdr = hdr.data();
    in.hdr_len = (uint32_t)hdr.size();
    in.sets = sets.data();
    in.rows = rows.data();
    in.n_sets = (uint32_t)sets.size();
    in.sums = sums.data();
    in.n_sums = (uint32_t)sums.size();
    return emit(v, which, in);
}

static ingot_ring_batch g_batches[INGOT_RING_MAX_BATCHES];
static ingot_gpu_doorbell g_db;

// Every entry point that takes frames, chunks or packets: its name, how many
// pointers it has, which of them is d_off (slots when NULL; -1: none).
struct Entry {
    const char* name;
    int pointers, off_bit;
    std::function<int(const Env&)> call;
};

static std::vector<Entry> entries() {
    std::vector<Entry> e;
    auto arena = [](const Env& v) { return v.p<const uint8_t>(0, v.arena); };
    e.push_back({"parse", 4, 1, [=](const Env& v) {
                     return ingot_gpu_parse(v.ctx, arena(v), v.p<const uint64_t>(1, kOff),
                                            v.p<const uint16_t>(2, kLen), v.n, v.chain,
                                            v.p<ingot_rec>(3, kOut), kStream);
                 }});
    e.push_back({"parse_strided", 3, -1, [=](const Env& v) {
                     return ingot_gpu_parse_strided(v.ctx, arena(v), v.stride,
                                                    v.p<const uint16_t>(1, kLen), v.n, v.chain,
                                                    v.p<ingot_rec>(2, kOut), kStream);
                 }});
    e.push_back({"parse_compact", 4, 1, [=](const Env& v) {
                     return ingot_gpu_parse_compact(v.ctx, arena(v), v.p<const uint64_t>(1, kOff),
                                                    v.p<const uint16_t>(2, kLen), v.n, v.chain,
                                                    v.p<ingot_rec8>(3, kOut), kStream);
                 }});
    e.push_back({"parse_strided_compact", 3, -1, [=](const Env& v) {
                     return ingot_gpu_parse_strided_compact(
                         v.ctx, arena(v), v.stride, v.p<const uint16_t>(1, kLen), v.n, v.chain,
                         v.p<ingot_rec8>(2, kOut), kStream);
                 }});
    e.push_back({"parse_packed", 5, -1, [=](const Env& v) {
                     return ingot_gpu_parse_packed(v.ctx, arena(v), v.p<const uint16_t>(1, kLen),
                                                   v.n, v.chain, v.p<ingot_rec>(2, kOut),
                                                   v.p<uint64_t>(3, kOffOut), v.p<void>(4, kWork),
                                                   1u << 20, kStream);
                 }});
    e.push_back({"parse_header", 5, 1, [=](const Env& v) {  // `chain` stands for the kind
                     return ingot_gpu_parse_header(
                         v.ctx, arena(v), v.p<const uint64_t>(1, kOff),
                         v.p<const uint16_t>(2, kLen),
                         v.stride, v.n, v.chain, v.p<const uint32_t>(3, kHint), 7,
                         v.p<ingot_hdr>(4, kOut), kStream);
                 }});
    e.push_back({"parse_ring", 3, -1, [=](const Env& v) {
                     return ingot_gpu_parse_ring(v.ctx,
                                                 v.p<const ingot_ring_batch>(0, (uintptr_t)g_batches),
                                                 2, v.stride, v.n, v.chain, 16,
                                                 v.p<const ingot_gpu_doorbell>(1, (uintptr_t)&g_db),
                                                 5, 100, v.p<uint32_t>(2, kStatus), kStream);
                 }});
    e.push_back({"fields", 4, 1, [=](const Env& v) {
                     return ingot_gpu_fields(v.ctx, arena(v), v.p<const uint64_t>(1, kOff),
                                             v.p<const uint16_t>(2, kLen), v.stride, v.n, v.chain,
                                             v.p<ingot_fields>(3, kOut), kStream);
                 }});
    e.push_back({"geneve_fields", 4, 1, [=](const Env& v) {
                     return ingot_gpu_geneve_fields(v.ctx, arena(v), v.p<const uint64_t>(1, kOff),
                                                    v.p<const uint16_t>(2, kLen), v.stride, v.n,
                                                    v.p<ingot_geneve_fields>(3, kOut), kStream);
                 }});
    e.push_back({"parse_read", 6, -1, [=](const Env& v) {
                     return ingot_gpu_parse_read(
                         v.ctx, arena(v), v.p<const uint64_t>(1, kSegOff),
                         v.p<const uint16_t>(2, kSegLen), v.p<const uint32_t>(3, kPktSeg), v.n,
                         v.chain, v.p<ingot_rec>(4, kOut), v.p<uint16_t>(5, kChunk), kStream);
                 }});
    e.push_back({"parse_read_first", 7, -1, [=](const Env& v) {
                     return ingot_gpu_parse_read_first(
                         v.ctx, arena(v), v.p<const uint64_t>(1, kSegOff),
                         v.p<const uint16_t>(2, kSegLen), v.p<const uint32_t>(3, kPktSeg),
                         v.p<const uint64_t>(6, kFirst), v.n, v.chain, v.p<ingot_rec>(4, kOut),
                         v.p<uint16_t>(5, kChunk), kStream);
                 }});
    e.push_back({"fields_read", 6, -1, [=](const Env& v) {
                     return ingot_gpu_fields_read(
                         v.ctx, arena(v), v.p<const uint64_t>(1, kSegOff),
                         v.p<const uint16_t>(2, kSegLen), v.p<const uint32_t>(3, kPktSeg), v.n,
                         v.chain, v.p<ingot_fields>(4, kOut), v.p<uint16_t>(5, kChunk), kStream);
                 }});
    e.push_back({"geneve_fields_read", 6, -1, [=](const Env& v) {
                     return ingot_gpu_geneve_fields_read(
                         v.ctx, arena(v), v.p<const uint64_t>(1, kSegOff),
                         v.p<const uint16_t>(2, kSegLen), v.p<const uint32_t>(3, kPktSeg), v.n,
                         v.p<ingot_geneve_fields>(4, kOut), v.p<uint16_t>(5, kChunk), kStream);
                 }});
    for (int fields = 0; fields < 3; ++fields)
        e.push_back({fields == 0   ? "parse_read_dense0"
                     : fields == 1 ? "parse_read_dense1"
                                   : "parse_read_dense2",
                     5, -1, [=](const Env& v) {
                         return ingot_gpu_parse_read_dense(
                             v.ctx, arena(v), v.p<const uint64_t>(1, kSegOff),
                             v.p<const uint32_t>(2, kPktSeg), v.n, v.chain, fields,
                             v.p<void>(3, kOut), v.p<uint16_t>(4, kChunk), kStream);
                     }});
    e.push_back({"parse_modify", 5, 1, [](const Env& v) {
                     return rewrite(v, false, 0, v.p<const ingot_edit>(3, (uintptr_t)kEdits), 2, 0);
                 }});
    e.push_back({"parse_modify_csum", 5, 1, [](const Env& v) {
                     return rewrite(v, false, 1, v.p<const ingot_edit>(3, (uintptr_t)kEdits), 2,
                                    INGOT_CSUM_L3 | INGOT_CSUM_L4);
                 }});
    e.push_back({"parse_modify_rows", 8, 1, [](const Env& v) {
                     return rewrite_rows(v, false,
                                         v.p<const ingot_edit_rows>(3, (uintptr_t)kEditRows), 3,
                                         true, INGOT_CSUM_L4);
                 }});
    e.push_back({"parse_read_modify", 7, -1, [](const Env& v) {
                     return rewrite(v, true, 0, v.p<const ingot_edit>(4, (uintptr_t)kEdits), 2, 0);
                 }});
    e.push_back({"parse_read_modify_csum", 7, -1, [](const Env& v) {
                     return rewrite(v, true, 1, v.p<const ingot_edit>(4, (uintptr_t)kEdits), 2,
                                    INGOT_CSUM_L3 | INGOT_CSUM_L4);
                 }});
    e.push_back({"parse_read_modify_rows", 8, -1, [](const Env& v) {
                     return rewrite_rows(v, true,
                                         v.p<const ingot_edit_rows>(4, (uintptr_t)kEditRows), 3,
                                         true, INGOT_CSUM_L4);
                 }});
    static const int kEmitPointers[5] = {8, 8, 12, 6, 9};
    for (int which = 0; which < 5; ++which)
        e.push_back({kEmitNames[which], kEmitPointers[which], -1, [=](const Env& v) {
                         EmitIn in;
                         in.hdr = kOpte.data();
                         in.hdr_len = (uint32_t)kOpte.size();
                         in.sets = kSets;
                         in.rows = kSetRows;
                         in.n_sets = 3;
                         in.sums = kSumUdp6;
                         in.n_sums = 1;
                         return emit(v, which, in);
                     }});
    for (int fill = 0; fill < 2; ++fill) {
        e.push_back({fill ? "checksum_fill" : "checksum_verify", 5, 1, [=](const Env& v) {
                         return fill ? ingot_gpu_checksum_fill(
                                           v.ctx, v.p<uint8_t>(0, v.arena),
                                           v.p<const uint64_t>(1, kOff),
                                           v.p<const uint16_t>(2, kLen), v.stride, v.n,
                                           v.p<const ingot_rec>(3, kRec),
                                           INGOT_CSUM_L3 | INGOT_CSUM_L4,
                                           v.p<ingot_csum>(4, kOut), kStream)
                                     : ingot_gpu_checksum_verify(
                                           v.ctx, arena(v), v.p<const uint64_t>(1, kOff),
                                           v.p<const uint16_t>(2, kLen), v.stride, v.n,
                                           v.p<const ingot_rec>(3, kRec), INGOT_CSUM_L4,
                                           v.p<ingot_csum>(4, kOut), kStream);
                     }});
        e.push_back({fill ? "checksum_fill_read" : "checksum_verify_read", 6, -1,
                     [=](const Env& v) {
                         return fill ? ingot_gpu_checksum_fill_read(
                                           v.ctx, v.p<uint8_t>(0, v.arena),
                                           v.p<const uint64_t>(1, kSegOff),
                                           v.p<const uint16_t>(2, kSegLen),
                                           v.p<const uint32_t>(3, kPktSeg), v.n,
                                           v.p<const ingot_rec>(4, kRec), INGOT_CSUM_L3,
                                           v.p<ingot_csum>(5, kOut), kStream)
                                     : ingot_gpu_checksum_verify_read(
                                           v.ctx, arena(v), v.p<const uint64_t>(1, kSegOff),
                                           v.p<const uint16_t>(2, kSegLen),
                                           v.p<const uint32_t>(3, kPktSeg), v.n,
                                           v.p<const ingot_rec>(4, kRec),
                                           INGOT_CSUM_L3 | INGOT_CSUM_L4, v.p<ingot_csum>(5, kOut),
                                           kStream);
                     }});
    }
    static uint8_t key[INGOT_FLOW_KEY_BYTES];
    for (int i = 0; i < INGOT_FLOW_KEY_BYTES; ++i) key[i] = (uint8_t)(i * 37 + 11);
    e.push_back({"flow_hist_ws", 8, 1, [=](const Env& v) {
                     return ingot_gpu_flow_hist_ws(
                         v.ctx, arena(v), v.p<const uint64_t>(1, kOff),
                         v.p<const uint16_t>(2, kLen),
                         v.stride, v.n, v.chain, v.p<const uint8_t>(3, (uintptr_t)key), 1024,
                         v.p<uint32_t>(4, kFlow), v.p<uint32_t>(5, kHash), v.p<uint32_t>(6, kHist),
                         v.p<void>(7, kWork), 4096, kStream);
                 }});
    e.push_back({"flow_hist", 7, 1, [=](const Env& v) {
                     return ingot_gpu_flow_hist(
                         v.ctx, arena(v), v.p<const uint64_t>(1, kOff),
                         v.p<const uint16_t>(2, kLen),
                         v.stride, v.n, v.chain, v.p<const uint8_t>(3, (uintptr_t)key), 1024,
                         v.p<uint32_t>(4, kFlow), v.p<uint32_t>(5, kHash), v.p<uint32_t>(6, kHist),
                         kStream);
                 }});
    e.push_back({"stream_delay", 0, -1, [](const Env& v) {  // n stands for the nanoseconds
                     return ingot_gpu_stream_delay(v.ctx, (uint32_t)v.n, kStream);
                 }});
    return e;
}

// NULL ctx, every chain and the two beside them, n == 0, each pointer and each
// pair of pointers NULL.
static void basics(ingot_gpu_ctx* ctx, const std::vector<Entry>& es) {
    for (const Entry& e : es) {
        Env v;
        v.ctx = ctx;
        rec(e.call(v), "%s", e.name);
        v.ctx = nullptr;
        rec(e.call(v), "%s ctx=NULL", e.name);
        v.ctx = ctx;
        for (int chain = -1; chain <= INGOT_CHAIN_COUNT; ++chain) {
            v.chain = chain;
            rec(e.call(v), "%s chain=%d", e.name, chain);
            v.n = 0;
            rec(e.call(v), "%s chain=%d n=0", e.name, chain);
            v.n = 100;
        }
        v.chain = INGOT_CHAIN_GENERIC_ULP;
        const uint32_t all = (1u << e.pointers) - 1u;
        v.n = 0;
        rec(e.call(v), "%s n=0", e.name);
        v.null = all;
        rec(e.call(v), "%s n=0 null=all", e.name);
        for (int a = 0; a < e.pointers; ++a) {
            v.null = 1u << a;
            rec(e.call(v), "%s n=0 null=%x", e.name, v.null);
        }
        v.n = 100;
        v.null = all;
        rec(e.call(v), "%s null=all", e.name);
        for (int a = 0; a < e.pointers; ++a)
            for (int b = a; b < e.pointers; ++b) {
                v.null = (1u << a) | (1u << b);
                rec(e.call(v), "%s null=%x", e.name, v.null);
            }
    }
}

static void slots(ingot_gpu_ctx* ctx, const std::vector<Entry>& es) {
    static const uint32_t strides[] = {0, 8, 16, 24, 48, 64, 72, 65520, 65535, 65536, 0x10010};
    static const uintptr_t arenas[] = {kArena, kArena + 8, kArena + 1};
    for (const Entry& e : es)
        for (uint32_t stride : strides)
            for (uintptr_t arena : arenas)
                for (int with_off = 0; with_off < 2; ++with_off)
                    for (uint64_t n : {(uint64_t)100, (uint64_t)0}) {
                        if (with_off && e.off_bit < 0) continue;
                        Env v;
                        v.ctx = ctx;
                        v.stride = stride;
                        v.arena = arena;
                        v.n = n;
                        v.null = with_off || e.off_bit < 0 ? 0u : 1u << e.off_bit;
                        rec(e.call(v), "%s stride=%u arena=%llx off=%d n=%llu", e.name, stride,
                            U(arena), with_off, U(n));
                        if (!with_off && e.off_bit >= 0) {  // slots without a length array
                            v.null |= 1u << (e.off_bit + 1);
                            rec(e.call(v), "%s stride=%u arena=%llx no len n=%llu", e.name, stride,
                                U(arena), U(n));
                        }
                    }
}

// Both rewrite lists over frames and chunks: every field (and one past), every
// op (and one past), every layer of every chain (and one past), what 0..8.
static void rewrite_sweep(ingot_gpu_ctx* ctx, bool rows) {
    Env v;
    v.ctx = ctx;
    v.n = 64;
    for (int chunks = 0; chunks < 2; ++chunks)
        for (int chain = 0; chain < INGOT_CHAIN_COUNT; ++chain)
            for (int layer = 0; layer <= ingot_chain_layer_count(chain); ++layer)
                for (int field = 0; field <= (rows ? 69 : (int)INGOT_F_COUNT); ++field) {
                    if (rows && field > INGOT_F_COUNT && field < 63) continue;
                    for (int op = 0; op <= INGOT_OP_XOR + 1; ++op)
                        for (uint32_t what = 0; what <= 8; ++what) {
                            v.chain = chain;
                            if (rows) {
                                const bool wide = field >= 64;
                                const ingot_edit_rows e = mk_edit(
                                    (uint8_t)layer, (uint8_t)field, (uint8_t)op,
                                    wide ? 0u : 0x12345u,
                                    wide ? INGOT_EDIT_BYTES : INGOT_EDIT_VALUE,
                                    0, 0, wide ? (const void*)(kTab + 1) : nullptr);
                                rec(rewrite_rows(v, chunks, &e, 1, true, what),
                                    "rows chunks=%d chain=%d layer=%d field=%d op=%d what=%u",
                                    chunks, chain, layer, field, op, what);
                                continue;
                            }
                            const ingot_edit e{(uint8_t)layer, (uint8_t)field, (uint8_t)op, 1,
                                               0x12345u};
                            if (what == 0)
                                rec(rewrite(v, chunks, 0, &e, 1, 0),
                                    "plain chunks=%d chain=%d layer=%d field=%d op=%d", chunks,
                                    chain, layer, field, op);
                            rec(rewrite(v, chunks, 1, &e, 1, what),
                                "csum chunks=%d chain=%d layer=%d field=%d op=%d what=%u", chunks,
                                chain, layer, field, op, what);
                        }
                }
}

// List sizes 0 / 1 / INGOT_MAX_EDITS / + 1, lists of several edits, NULL lists,
// and the list's checks against n == 0 and the frames' own.
static void rewrite_lists(ingot_gpu_ctx* ctx) {
    std::vector<ingot_edit> plain;
    std::vector<ingot_edit_rows> rows;
    for (uint32_t k = 0; k < INGOT_MAX_EDITS + 1; ++k) {
        plain.push_back(ingot_edit{(uint8_t)(k % 3), (uint8_t)((k * 5) % INGOT_F_COUNT),
                                   (uint8_t)(k % 6), 0, 0x1000u + k});
        const int kind = k % 4;
        rows.push_back(
            kind == 0   ? mk_edit(1, INGOT_FW_V6_DESTINATION, 0, 0, INGOT_EDIT_BYTES, INGOT_BY_ROW,
                                  40, (const void*)(kTab + k))
            : kind == 1 ? mk_edit(0, INGOT_FW_ETH_SOURCE, 0, 0, INGOT_EDIT_BYTES, 0, 0,
                                  (const void*)(kTab + 64 + k))
            : kind == 2 ? mk_edit(2, INGOT_F_TCP_SEQUENCE, INGOT_OP_ADD, 0, INGOT_EDIT_U32,
                                  INGOT_BY_ROW, 8, (const void*)(kTab + 128))
                        : mk_edit(1, INGOT_F_V4_HOP_LIMIT, INGOT_OP_SUB, 1, INGOT_EDIT_VALUE, 0, 0,
                                  nullptr));
    }
    std::vector<ingot_edit_rows> wide(INGOT_MAX_EDITS + 1, rows[0]);  // 4 pieces each
    static const uint32_t sizes[] = {0, 1, 2, 5, INGOT_MAX_EDITS, INGOT_MAX_EDITS + 1};
    for (int chunks = 0; chunks < 2; ++chunks)
        for (int chain : {INGOT_CHAIN_GENERIC_ULP, INGOT_CHAIN_GENEVE_OVER_V6})
            for (uint32_t ne : sizes)
                for (int null_list = 0; null_list < 2; ++null_list)
                    for (uint64_t n : {(uint64_t)100, (uint64_t)0})
                        for (uint32_t what : {0u, 2u, 3u, 7u}) {
                            Env v;
                            v.ctx = ctx;
                            v.chain = chain;
                            v.n = n;
                            const char* fmt = "%s chunks=%d chain=%d ne=%u null=%d n=%llu what=%u";
                            rec(rewrite(v, chunks, what != 0, null_list ? nullptr : plain.data(),
                                        ne, what),
                                fmt, "plain", chunks, chain, ne, null_list, U(n), what);
                            rec(rewrite_rows(v, chunks, null_list ? nullptr : rows.data(), ne,
                                             true, what),
                                fmt, "rows", chunks, chain, ne, null_list, U(n), what);
                            rec(rewrite_rows(v, chunks, null_list ? nullptr : wide.data(), ne,
                                             true, what),
                                fmt, "wide", chunks, chain, ne, null_list, U(n), what);
                            // a bad list against bad frames: which is seen first
                            v.null = 1u;  // arena
                            v.stride = 24;
                            rec(rewrite(v, chunks, what != 0, plain.data(), ne, what), fmt,
                                "plain-noarena", chunks, chain, ne, null_list, U(n), what);
                            rec(rewrite_rows(v, chunks, rows.data(), ne, false, what), fmt,
                                "rows-noarena-norow", chunks, chain, ne, null_list, U(n), what);
                        }
}

// Operand tables of ingot_edit_rows: every source (and one past) on narrow and
// wide fields, by-packet / by-row (and one past) with and without a row array,
// pitches around every width, d_values at each address mod 4 and NULL,
// non-zero value / _pad, SET and another op.
static void edit_tables(ingot_gpu_ctx* ctx) {
    static const uint8_t fields[] = {INGOT_F_UDP_SOURCE,       INGOT_F_V4_SOURCE,
                                     INGOT_FW_ETH_DESTINATION, INGOT_FW_ETH_SOURCE,
                                     INGOT_FW_V6_SOURCE,       INGOT_FW_V6_DESTINATION};
    static const uint32_t pitches[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 32};
    Env v;
    v.ctx = ctx;
    v.chain = INGOT_CHAIN_GENEVE_OVER_V6;
    for (int chunks = 0; chunks < 2; ++chunks)
        for (uint8_t field : fields)
            for (int source = 0; source <= INGOT_EDIT_BYTES + 1; ++source)
                for (int by = 0; by <= INGOT_BY_ROW + 1; ++by)
                    for (int row = 0; row < 2; ++row)
                        for (uint32_t pitch : pitches)
                            for (int at = -1; at < 4; ++at)
                                for (int bits = 0; bits < 8; ++bits) {
                                    ingot_edit_rows e = mk_edit(
                                        5, field, bits & 1 ? INGOT_OP_ADD : INGOT_OP_SET,
                                        bits & 2 ? 5u : 0u, (uint8_t)source, (uint8_t)by, pitch,
                                        at < 0 ? nullptr : (const void*)(kTab + (uintptr_t)at));
                                    e._pad = bits & 4 ? 0x100 : 0;
                                    rec(rewrite_rows(v, chunks, &e, 1, row, 6u),
                                        "chunks=%d field=%d source=%d by=%d row=%d pitch=%u "
                                        "at=%d bits=%d",
                                        chunks, field, source, by, row, pitch, at, bits);
                                }
}

// The same for ingot_emit_set_rows.
static void emit_tables(ingot_gpu_ctx* ctx) {
    static const struct {
        uint16_t at;
        uint8_t field;
    } fields[] = {{54, INGOT_F_UDP_SOURCE},       {62, INGOT_F_GENEVE_VNI},
                  {0, INGOT_FW_ETH_DESTINATION},  {0, INGOT_FW_ETH_SOURCE},
                  {14, INGOT_FW_V6_SOURCE},       {14, INGOT_FW_V6_DESTINATION}};
    static const uint32_t pitches[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 32};
    Env v;
    v.ctx = ctx;
    EmitIn in;
    in.hdr = kOpte.data();
    in.hdr_len = (uint32_t)kOpte.size();
    in.n_sets = 1;
    in.sums = kSumUdp6;
    in.n_sums = 1;
    for (const auto& f : fields)
        for (int source = 0; source <= INGOT_EMIT_BYTES + 1; ++source)
            for (int by = 0; by <= INGOT_BY_ROW + 1; ++by)
                for (int row = 0; row < 2; ++row)
                    for (uint32_t pitch : pitches)
                        for (int at = -1; at < 4; ++at)
                            for (int bits = 0; bits < 8; ++bits) {
                                ingot_emit_set_rows s = mk_set(
                                    f.at, f.field, (uint8_t)source, bits & 1 ? 3 : 0, (uint8_t)by,
                                    pitch, at < 0 ? nullptr : (const void*)(kTab + (uintptr_t)at));
                                s._pad[(bits >> 1) & 1] = bits & 4 ? 1 : 0;
                                in.rows = &s;
                                in.row = row;
                                rec(emit(v, 4, in),
                                    "field=%d source=%d by=%d row=%d pitch=%u at=%d bits=%d",
                                    f.field, source, by, row, pitch, at, bits);
                            }
}

// Every field at every `at` of a 64-byte block (so just inside and just outside
// it), and far outside, for every emit call and source.
static void emit_fields(ingot_gpu_ctx* ctx) {
    std::vector<uint8_t> hdr(64);
    for (size_t i = 0; i < hdr.size(); ++i) hdr[i] = (uint8_t)(i * 3u + 1u);
    Env v;
    v.ctx = ctx;
    v.n = 8;
    for (int which = 0; which < 5; ++which)
        for (int field = 0; field <= (which == 4 ? 69 : (int)INGOT_F_COUNT + 1); ++field) {
            if (field > INGOT_F_COUNT + 1 && field < 63) continue;
            for (int source = 0; source <= INGOT_EMIT_VALUE + 1; ++source)
                for (uint32_t at = 0; at <= 68; ++at) {
                    const uint16_t a =
                        at <= 64 ? (uint16_t)at : (uint16_t)(65535u - (at - 65u) * 20u);
                    const bool wide = field >= 64;
                    if (wide && source != 0) continue;
                    ingot_emit_set s{a, (uint8_t)field, (uint8_t)(wide ? INGOT_EMIT_BYTES : source),
                                     (int32_t)at - 7,
                                     wide || source == INGOT_EMIT_U16 || source == INGOT_EMIT_U32
                                         ? (const void*)kTab
                                         : nullptr};
                    if (wide) s.add = 0;
                    rec(emit_any(v, which, hdr, {s}, {}), "%s field=%d source=%d at=%u",
                        kEmitNames[which], field, source, a);
                }
        }
}

// The header block's and the lists' own limits, the sums of
// tests/test_emit_csum.py's argument test, emit_headers' stride rule, the LDS fit.
static void emit_args_group(ingot_gpu_ctx* ctx) {
    Env v;
    v.ctx = ctx;
    const std::vector<ingot_emit_set> sets(kSets, kSets + 3);
    const std::vector<ingot_emit_set> v4sets = {
        {14, INGOT_F_V4_TOTAL_LEN, INGOT_EMIT_LENGTH, 0, nullptr},
        {34, INGOT_F_UDP_LENGTH, INGOT_EMIT_LENGTH, 0, nullptr},
        {34, INGOT_F_UDP_SOURCE, INGOT_EMIT_U16, 0, (const void*)kTab}};
    for (int which = 0; which < 5; ++which) {
        const char* nm = kEmitNames[which];
        for (uint64_t n : {(uint64_t)100, (uint64_t)0}) {
            v.n = n;
            for (uint32_t len : {0u, 1u, 70u, 256u, 257u}) {
                std::vector<uint8_t> h(len, 0x61);
                rec(emit_any(v, which, h, {}, {}), "%s hdr_len=%u n=%llu", nm, len, U(n));
                Env w = v;
                w.null = 1u;
                rec(emit_any(w, which, h, {}, {}), "%s hdr_len=%u hdr=NULL n=%llu", nm, len, U(n));
            }
            for (uint32_t ns : {0u, 1u, 8u, 9u}) {
                std::vector<ingot_emit_set> many(ns, kSets[2]);
                rec(emit_any(v, which, kOpte, many, {}), "%s n_sets=%u n=%llu", nm, ns, U(n));
                Env w = v;
                w.null = 2u;
                rec(emit_any(w, which, kOpte, many, {}), "%s n_sets=%u sets=NULL n=%llu", nm, ns,
                    U(n));
            }
            // a set without its table; an unknown source
            rec(emit_any(v, which, kOpte, {{54, INGOT_F_UDP_SOURCE, INGOT_EMIT_U16, 0, nullptr}},
                         {}),
                "%s U16 no table n=%llu", nm, U(n));
            rec(emit_any(v, which, kOpte, {{54, INGOT_F_UDP_SOURCE, INGOT_EMIT_BYTES, 0, nullptr}},
                         {}),
                "%s BYTES narrow n=%llu", nm, U(n));
            using Sums = std::vector<ingot_emit_sum>;
            const ingot_emit_sum v4{14, 0, INGOT_EMIT_SUM_IPV4, {0, 0, 0}};
            const ingot_emit_sum udp{34, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}};
            auto sum = [&](const char* tag, const std::vector<uint8_t>& h,
                           const std::vector<ingot_emit_set>& se, const Sums& s) {
                rec(emit_any(v, which, h, se, s), "%s sums %s n=%llu", nm, tag, U(n));
            };
            sum("ok both", kV4, v4sets, {v4, udp});
            sum("ok udp first", kV4, v4sets, {udp, v4});
            sum("ok v4", kV4, v4sets, {v4});
            sum("ok udp", kV4, v4sets, {udp});
            sum("ok udp6", kOpte, sets, {kSumUdp6[0]});
            sum("three", kV4, v4sets, {v4, udp, v4});
            {
                Env w = v;
                w.null = 4u;
                rec(emit_any(w, which, kV4, v4sets, {v4}), "%s sums NULL n=%llu", nm, U(n));
            }
            sum("kind 2", kV4, v4sets, {{34, 14, 2, {0, 0, 0}}});
            for (int p = 0; p < 3; ++p) {
                ingot_emit_sum s = udp;
                s._pad[p] = 1;
                sum("pad", kV4, v4sets, {s});
            }
            sum("two udp", kV4, v4sets, {udp, udp});
            sum("two v4", kV4, v4sets, {v4, v4});
            sum("odd at", kV4, v4sets, {{35, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            sum("odd l3", kV4, v4sets, {{34, 13, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            sum("v4 odd at", kV4, v4sets, {{15, 0, INGOT_EMIT_SUM_IPV4, {0, 0, 0}}});
            sum("v4 l3_at", kV4, v4sets, {{14, 2, INGOT_EMIT_SUM_IPV4, {0, 0, 0}}});
            sum("v4 version", kV4, v4sets, {{34, 0, INGOT_EMIT_SUM_IPV4, {0, 0, 0}}});
            for (uint8_t b : {(uint8_t)0x44, (uint8_t)0x4f, (uint8_t)0x49, (uint8_t)0x4a}) {
                std::vector<uint8_t> h = kV4;  // ihl < 5; 4 ihl past / at / past hdr_len
                h[14] = b;
                sum("v4 ihl", h, v4sets, {v4});
            }
            sum("v4 at end", kV4, v4sets, {{32, 0, INGOT_EMIT_SUM_IPV4, {0, 0, 0}}});
            sum("udp at end", kV4, v4sets, {{44, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            sum("udp at end ok", kV4, v4sets, {{42, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            sum("udp l3 version", kV4, v4sets, {{34, 0, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            sum("udp l3 past", kV4, v4sets, {{34, 50, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            sum("udp l3 last", kV4, v4sets, {{34, 48, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            sum("v4 ends past at", kV4, v4sets, {{32, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            sum("v6 ends past at", kOpte, sets, {{52, 14, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            for (uint8_t f : {(uint8_t)INGOT_F_V4_VERSION, (uint8_t)INGOT_F_V4_IHL,
                              (uint8_t)INGOT_F_V6_VERSION, (uint8_t)INGOT_F_V4_DSCP})
                for (uint16_t at : {(uint16_t)14, (uint16_t)34}) {
                    std::vector<ingot_emit_set> extra = v4sets;
                    extra.push_back({at, f, INGOT_EMIT_VALUE, 4, nullptr});
                    sum("setter v4", kV4, extra, {v4});
                    sum("setter udp", kV4, extra, {udp});
                    sum("setter none", kV4, extra, {});
                }
            sum("no hdr", {}, {}, {{0, 0, INGOT_EMIT_SUM_UDP, {0, 0, 0}}});
            sum("hdr too long", std::vector<uint8_t>(300, 0), {}, {});
            // emit_headers: slots narrower than the block
            for (uint32_t os : {0u, 69u, 70u, 71u})
                for (uint32_t no_off = 0; no_off < 2; ++no_off) {
                    EmitIn in;
                    in.hdr = kOpte.data();
                    in.hdr_len = 70;
                    in.sets = kSets;
                    in.n_sets = 3;
                    in.out_stride = os;
                    Env w = v;
                    w.null = no_off ? 1u << 5 : 0u;
                    rec(emit(w, 3, in), "headers out_stride=%u no_off=%u n=%llu", os, no_off, U(n));
                }
        }
        // the LDS fit against device entry, the n == 0 exit and NULL pointers
        v.n = 100;
        const size_t lds = ctx->lds_bytes;
        for (size_t l : {(size_t)16, (size_t)4096 + 70 + 3 * 64 - 1, (size_t)4096 + 70 + 3 * 64,
                         (size_t)8192 + 70 + 3 * 64}) {
            ctx->lds_bytes = l;
            for (int nodev = 0; nodev < 2; ++nodev)
                for (uint32_t null : {0u, 8u}) {
                    g_no_device = nodev;
                    Env w = v;
                    w.null = null;
                    rec(emit_any(w, which, kOpte, sets, {kSumUdp6[0]}),
                        "%s lds=%llu nodev=%d null=%x", nm, U(l), nodev, null);
                    w.n = 0;
                    rec(emit_any(w, which, kOpte, sets, {kSumUdp6[0]}),
                        "%s lds=%llu nodev=%d null=%x n=0", nm, U(l), nodev, null);
                }
            g_no_device = false;
        }
        ctx->lds_bytes = lds;
    }
}

static void ring_and_packed(ingot_gpu_ctx* ctx) {
    auto ring = [&](const char* tag, ingot_gpu_ctx* c, const ingot_ring_batch* b, uint32_t nb,
                    uint32_t stride, uint64_t n, int chain, uint32_t rb,
                    const ingot_gpu_doorbell* db, uint32_t first, uint32_t ms) {
        rec(ingot_gpu_parse_ring(c, b, nb, stride, n, chain, rb, db, first, ms,
                                 (uint32_t*)kStatus, kStream),
            "ring %s nb=%u stride=%u n=%llu chain=%d rb=%u db=%d first=%u ms=%u", tag, nb, stride,
            U(n), chain, rb, db != nullptr, first, ms);
    };
    for (int chain = -1; chain <= INGOT_CHAIN_COUNT; ++chain)
        for (uint32_t rb : {0u, 8u, 16u, 24u})
            ring("chain", ctx, g_batches, 3, 128, 1000, chain, rb, nullptr, 0, 0);
    for (uint32_t nb : {0u, 1u, 2u, 63u, 64u, 65u})
        for (uint32_t stride : {0u, 48u, 64u, 72u, 80u, 65520u, 65535u, 65536u})
            for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)64, (uint64_t)65}) {
                ring("shape", ctx, g_batches, nb, stride, n, 0, 16, nullptr, 0, 0);
                ring("shape-null", ctx, nullptr, nb, stride, n, 0, 16, nullptr, 0, 0);
                ring("shape-db", ctx, g_batches, nb, stride, n, 0, 8, &g_db, 9, 250);
            }
    for (uint32_t ms : {0u, 1u, 60000u, 60001u})
        for (uint32_t first : {0u, 0xffffffffu, 0xffffffffu - 62u, 0xffffffffu - 63u})
            for (uint32_t nb : {0u, 1u, 64u})
                ring("db", ctx, g_batches, nb, 128, 100, 1, 16, &g_db, first, ms);
    // 32-bit tile cursors
    ring("tiles", ctx, g_batches, 1, 128, (1ull << 37) - 64, 0, 16, nullptr, 0, 0);
    ring("tiles", ctx, g_batches, 1, 128, (1ull << 37) - 63, 0, 16, nullptr, 0, 0);
    ring("tiles", ctx, g_batches, 64, 128, (1ull << 31) - 64, 0, 16, nullptr, 0, 0);
    ring("tiles", ctx, g_batches, 64, 128, (1ull << 31) - 63, 0, 16, nullptr, 0, 0);
    ring("tiles", ctx, g_batches, 64, 24, (1ull << 31), 0, 16, nullptr, 0, 0);
    // a doorbell of another device; no wall clock
    ingot_gpu_doorbell other = g_db;
    other.device = 1;
    ring("db-device", ctx, g_batches, 2, 128, 100, 0, 16, &other, 0, 10);
    ring("db-device n=0", ctx, g_batches, 2, 128, 0, 0, 16, &other, 0, 10);
    const uint32_t khz = ctx->wall_khz;
    ctx->wall_khz = 0;
    ring("no-clock", ctx, g_batches, 2, 128, 100, 0, 16, &g_db, 0, 10);
    ring("no-clock", ctx, g_batches, 2, 128, 100, 0, 16, nullptr, 0, 10);
    ring("no-clock n=0", ctx, g_batches, 2, 128, 0, 0, 16, &g_db, 0, 10);
    rec(ingot_gpu_stream_delay(ctx, 10, kStream), "delay no clock");
    rec(ingot_gpu_stream_delay(ctx, 0, kStream), "delay 0 no clock");
    ctx->wall_khz = khz;
    for (uint32_t ns : {0u, 1u, 999u, 1000u, 0xffffffffu})
        rec(ingot_gpu_stream_delay(ctx, ns, kStream), "delay %u", ns);
    // one bad batch, at either end
    for (uint32_t bad : {0u, 3u})
        for (int kind = 0; kind < 3; ++kind) {
            ingot_ring_batch b[4];
            for (uint32_t k = 0; k < 4; ++k) b[k] = g_batches[k];
            if (kind == 0) b[bad].d_arena = nullptr;
            if (kind == 1) b[bad].d_arena = (const uint8_t*)(kArena + 8);
            if (kind == 2) b[bad].d_out = nullptr;
            ring("bad-batch", ctx, b, 4, 128, 100, 0, 16, nullptr, 0, 0);
            ring("bad-batch-noclock", ctx, b, 4, 128, 100, 0, 16, &other, 0, 10);
        }
    g_no_device = true;
    ring("nodev", ctx, g_batches, 2, 128, 100, 0, 16, &g_db, 0, 10);
    g_no_device = false;

    for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)64, (uint64_t)65, (uint64_t)100000})
        for (uintptr_t work : {kWork, kWork + 4, kWork + 1})
            for (int d = -1; d <= 1; ++d) {
                const size_t bytes = ig::packed_workspace(n) + (size_t)d;
                rec(ingot_gpu_parse_packed(ctx, (const uint8_t*)kArena, (const uint16_t*)kLen, n, 1,
                                           (ingot_rec*)kOut, nullptr, (void*)work, bytes, kStream),
                    "packed n=%llu work=%llx bytes%+d", U(n), U(work), d);
                rec(ingot_gpu_parse_packed(ctx, (const uint8_t*)kArena, nullptr, n, 1,
                                           (ingot_rec*)kOut, nullptr, (void*)work, bytes, kStream),
                    "packed no len n=%llu work=%llx bytes%+d", U(n), U(work), d);
            }
    rec((int)ingot_gpu_packed_workspace_size(1000), "packed_workspace_size");
    g_fail_launch = true;
    rec(ingot_gpu_parse_packed(ctx, (const uint8_t*)kArena, (const uint16_t*)kLen, 100, 1,
                               (ingot_rec*)kOut, nullptr, (void*)kWork, 1u << 20, kStream),
        "packed launch fails");
    g_fail_launch = false;
}

static void flows_and_sums(ingot_gpu_ctx* ctx) {
    uint8_t key[INGOT_FLOW_KEY_BYTES];
    for (int i = 0; i < INGOT_FLOW_KEY_BYTES; ++i) key[i] = (uint8_t)(255 - i * 3);
    for (uint32_t bins : {0u, 1u, 2u, 3u, 1024u, 1u << 16, 1u << 17, 1u << 24, 1u << 25,
                          0x80000000u, 0xffffffffu})
        for (uint64_t n : {(uint64_t)100, (uint64_t)0})
            for (int chain : {-1, 0, 3, 4})
                for (int k = 0; k < 2; ++k)
                    for (int slots_bad = 0; slots_bad < 2; ++slots_bad) {
                        rec(ingot_gpu_flow_hist_ws(
                                ctx, (const uint8_t*)kArena,
                                slots_bad ? nullptr : (const uint64_t*)kOff,
                                (const uint16_t*)kLen, 24, n, chain, k ? key : nullptr, bins,
                                (uint32_t*)kFlow, k ? (uint32_t*)kHash : nullptr,
                                k ? nullptr : (uint32_t*)kHist, (void*)kWork, 64, kStream),
                            "flow bins=%u n=%llu chain=%d key=%d bad_stride=%d", bins, U(n), chain,
                            k, slots_bad);
                        rec((int)ingot_gpu_flow_hist_workspace_size(n, bins),
                            "flow workspace bins=%u n=%llu", bins, U(n));
                    }
    g_fail_launch = true;
    rec(ingot_gpu_flow_hist(ctx, (const uint8_t*)kArena, (const uint64_t*)kOff,
                            (const uint16_t*)kLen, 0, 100, 0, nullptr, 64, (uint32_t*)kFlow,
                            nullptr, (uint32_t*)kHist, kStream),
        "flow launch fails");
    g_fail_launch = false;
    // the checksum calls' `what`, their optional d_out, slots
    for (int which = 0; which < 4; ++which)
        for (uint32_t what = 0; what <= 8; ++what)
            for (int out = 0; out < 2; ++out)
                for (uint64_t n : {(uint64_t)100, (uint64_t)0})
                    for (int slots = 0; slots < 3; ++slots) {
                        ingot_csum* o = out ? (ingot_csum*)kOut : nullptr;
                        const uint64_t* off = slots ? nullptr : (const uint64_t*)kOff;
                        const uint16_t* len = slots == 2 ? nullptr : (const uint16_t*)kLen;
                        int r;
                        if (which == 0)
                            r = ingot_gpu_checksum_verify(ctx, (const uint8_t*)kArena, off, len,
                                                          256, n, (const ingot_rec*)kRec, what,
                                                          o, kStream);
                        else if (which == 1)
                            r = ingot_gpu_checksum_fill(ctx, (uint8_t*)kArena, off, len, 256, n,
                                                        (const ingot_rec*)kRec, what, o, kStream);
                        else if (which == 2)
                            r = ingot_gpu_checksum_verify_read(
                                ctx, (const uint8_t*)kArena, (const uint64_t*)kSegOff,
                                (const uint16_t*)kSegLen, (const uint32_t*)kPktSeg, n,
                                (const ingot_rec*)kRec, what, o, kStream);
                        else
                            r = ingot_gpu_checksum_fill_read(
                                ctx, (uint8_t*)kArena, (const uint64_t*)kSegOff,
                                (const uint16_t*)kSegLen, (const uint32_t*)kPktSeg, n,
                                (const ingot_rec*)kRec, what, o, kStream);
                        rec(r, "csum which=%d what=%u out=%d n=%llu slots=%d", which, what, out,
                            U(n), slots);
                    }
    // parse_header's kinds and its own slot rule
    for (int kind = -1; kind <= 20; ++kind)
        for (uint32_t stride : {0u, 1u, 24u, 65535u, 65536u})
            for (int off = 0; off < 2; ++off)
                for (int len = 0; len < 2; ++len)
                    rec(ingot_gpu_parse_header(ctx, (const uint8_t*)(kArena + 3),
                                               off ? (const uint64_t*)kOff : nullptr,
                                               len ? (const uint16_t*)kLen : nullptr, stride, 10,
                                               kind, nullptr, INGOT_HINT_NONE, (ingot_hdr*)kOut,
                                               kStream),
                        "header kind=%d stride=%u off=%d len=%d", kind, stride, off, len);
}

static void tuning_and_misc(ingot_gpu_ctx* ctx) {
    const ig::Tuning saved = ctx->tuning;
    for (int key = -1; key <= 16; ++key)
        for (int value : {0, 1, 7, -1, 65536, 0x7fffffff}) {
            rec(ingot_gpu_ctx_set_tuning(ctx, key, value), "set key=%d value=%d", key, value);
            rec(ingot_gpu_ctx_get_tuning(ctx, key), "get key=%d", key);
            rec(ingot_gpu_ctx_set_tuning(nullptr, key, value), "set NULL key=%d", key);
            rec(ingot_gpu_ctx_get_tuning(nullptr, key), "get NULL key=%d", key);
        }
    for (int key = 1; key <= 14; ++key) ingot_gpu_ctx_set_tuning(ctx, key, 100 + key);
    for (int key = 0; key <= 15; ++key) rec(ingot_gpu_ctx_get_tuning(ctx, key), "get2 key=%d", key);
    // every member reaches the launcher
    rec(ingot_gpu_parse(ctx, (const uint8_t*)kArena, (const uint64_t*)kOff, (const uint16_t*)kLen,
                        10, 0, (ingot_rec*)kOut, nullptr),
        "parse with tuning");
    ctx->tuning = saved;

    rec(ingot_gpu_abi_version(), "abi");
    rec(ingot_gpu_ctx_device(ctx), "device");
    rec(ingot_gpu_ctx_device(nullptr), "device NULL");
    rec(ingot_gpu_ctx_create(0, nullptr), "create out=NULL");
    for (int code = -8; code <= 1; ++code) rec(0, "strerror %d %s", code, ingot_gpu_strerror(code));
    for (int s = -1; s <= 10; ++s) {
        const char* nm = ingot_parse_error_name(s);
        rec(0, "parse_error_name %d %s", s, nm ? nm : "(null)");
    }
    for (int chain = -1; chain <= INGOT_CHAIN_COUNT; ++chain) {
        rec(ingot_chain_layer_count(chain), "layer_count %d", chain);
        for (int layer = -1; layer <= 7; ++layer) {
            const char* nm = ingot_chain_layer_label(chain, layer);
            rec(0, "layer_label %d %d %s", chain, layer, nm ? nm : "(null)");
        }
    }
    // host mappings and the doorbell: the argument checks and device entry only
    // (past them lies the HIP runtime)
    void* d = (void*)1;
    char here[16];
    rec(ingot_gpu_host_map(nullptr, here, 16, &d), "host_map ctx=NULL");
    rec(ingot_gpu_host_map(ctx, nullptr, 16, &d), "host_map host=NULL");
    rec(ingot_gpu_host_map(ctx, here, 16, nullptr), "host_map d_ptr=NULL");
    rec(ingot_gpu_host_map(ctx, here, 0, &d), "host_map bytes=0");
    rec(ingot_gpu_host_map(ctx, (void*)~(uintptr_t)15, 32, &d), "host_map wraps");
    rec(d == nullptr, "host_map cleared d_ptr");
    g_no_device = true;
    rec(ingot_gpu_host_map(ctx, here, 16, &d), "host_map nodev");
    ingot_gpu_doorbell* db = (ingot_gpu_doorbell*)1;
    volatile uint32_t* word = (volatile uint32_t*)1;
    rec(ingot_gpu_doorbell_create(ctx, &db, &word), "doorbell_create nodev");
    rec(db == nullptr && word == nullptr, "doorbell_create cleared");
    g_no_device = false;
    rec(ingot_gpu_doorbell_create(nullptr, &db, &word), "doorbell_create ctx=NULL");
    rec(ingot_gpu_doorbell_create(ctx, nullptr, &word), "doorbell_create out=NULL");
    rec(ingot_gpu_host_unmap(nullptr, here), "host_unmap ctx=NULL");
    rec(ingot_gpu_host_unmap(ctx, nullptr), "host_unmap host=NULL");
    rec(ingot_gpu_host_unmap(ctx, here), "host_unmap not mapped");
    rec(ingot_gpu_doorbell_wait(nullptr, 1, kStream), "doorbell_wait NULL");
    rec(ingot_gpu_doorbell_ring(nullptr, 1), "doorbell_ring NULL");
    uint32_t w = 0;
    ingot_gpu_doorbell local = g_db;
    local.word = &w;
    rec(ingot_gpu_doorbell_ring(&local, 41), "doorbell_ring");
    rec((int)w, "doorbell word");
    ingot_gpu_doorbell_destroy(nullptr);
    ingot_gpu_ctx_destroy(nullptr);
}

int main(int argc, char** argv) {
    g_verbose = argc > 1 && !std::strcmp(argv[1], "--verbose");
    for (uint32_t b = 0; b < INGOT_RING_MAX_BATCHES; ++b)
        g_batches[b] = ingot_ring_batch{(const uint8_t*)(kArena + 0x1000u * b),
                                        (void*)(kOut + 0x1000u * b)};
    g_db.device = 0;
    g_db.word = (uint32_t*)0x7000;
    g_db.dword = (uint32_t*)0x7100;
    ingot_gpu_ctx ctx;  // api.cpp's own struct: no device is opened
    ctx.wall_khz = 100000;
    ctx.tuning.cus = 256;
    const std::vector<Entry> es = entries();

    begin("basics");
    basics(&ctx, es);
    end();
    begin("basics_no_device");  // where device entry stands among the checks
    g_no_device = true;
    basics(&ctx, es);
    g_no_device = false;
    end();
    begin("basics_other_device");  // the context's device made current
    ctx.device = 1;
    for (const Entry& e : es) {
        Env v;
        v.ctx = &ctx;
        g_cur_device = 0;
        rec(e.call(v), "%s", e.name);
    }
    ctx.device = 0;
    g_cur_device = 0;
    end();
    begin("basics_host_arena");  // frames inside a host mapping: Tuning::host_arena
    ctx.host.push_back({0x7f0000, 0x1000, kArena - 0x100, false});
    for (const Entry& e : es)
        for (uintptr_t arena : {kArena, kArena + 0xf00 - 16, kArena + 0xf00, kArena - 0x110}) {
            Env v;
            v.ctx = &ctx;
            v.arena = arena;
            rec(e.call(v), "%s arena=%llx", e.name, U(arena));
        }
    ctx.host.clear();
    end();
    begin("basics_launch_fails");
    g_fail_launch = true;
    for (const Entry& e : es) {
        Env v;
        v.ctx = &ctx;
        rec(e.call(v), "%s", e.name);
    }
    g_fail_launch = false;
    end();
    begin("slots");
    slots(&ctx, es);
    end();
    begin("rewrite_sweep");
    rewrite_sweep(&ctx, false);
    end();
    begin("rewrite_rows_sweep");
    rewrite_sweep(&ctx, true);
    end();
    begin("rewrite_lists");
    rewrite_lists(&ctx);
    end();
    begin("edit_tables");
    edit_tables(&ctx);
    end();
    begin("emit_tables");
    emit_tables(&ctx);
    end();
    begin("emit_fields");
    emit_fields(&ctx);
    end();
    begin("emit_args");
    emit_args_group(&ctx);
    end();
    begin("ring_packed_delay");
    ring_and_packed(&ctx);
    end();
    begin("flows_sums_header");
    flows_and_sums(&ctx);
    end();
    begin("tuning_misc");
    tuning_and_misc(&ctx);
    end();
    return 0;
}
