// kernels.h — internal interface between the C ABI (api.cpp, resolve.cpp) and the HIP
// kernels: the argument blocks, the tuning record and the launchers of
// parse.hip, read.hip, ring.hip, tuple.hip, packed.hip, flow.hip, header.hip,
// emit.hip, emit_read.hip, csum.hip and stream.hip.  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ingot_gpu.h"

namespace ingot_gpu {

// STRIDED: frame i at i*stride; INDEXED: (off[i], len[i]); SEGMENTED: packet i
// is the chunks pkt_seg[i] .. pkt_seg[i+1] of (off, len) = (seg_off, seg_len),
// walked with parse_read's chunk semantics (read.hip).
// PACKED: frames back to back with only a length array; `off` holds one u64
// base per group of tiles and `tile_local` each tile's prefix in its group
// (packed.hip); the frame offsets come from a wavefront prefix scan of the
// tile's lengths.
enum LayoutKind { LAYOUT_STRIDED = 0, LAYOUT_INDEXED = 1, LAYOUT_SEGMENTED = 2, LAYOUT_PACKED = 3 };

// Output mode: 16-B ingot_rec, 8-B ingot_rec8, 256-B ingot_fields, or the
// flow hash + histogram (OUT_FLOWS16: only the hash's low 16 bits, enough for
// <= 65,536 bins when the full hash is not requested — half the LDS table).
enum OutMode {
    OUT_REC16 = 0,
    OUT_REC8 = 1,
    OUT_FIELDS = 2,
    OUT_FLOWS = 3,
    OUT_MODIFY = 4,
    OUT_FLOWS16 = 5
};

// Toeplitz key windows: w[b] = the 32 key bits starting at input bit b, for
// every bit of the longest input (IPv6 src|dst|ports = 36 bytes).
constexpr uint32_t FLOW_INPUT_BITS = 36 * 8;
// The 16-bit nibble table (OUT_FLOWS16), in dwords: 72 positions x 16 values
// x 2 B.  Computed once per call on the host (api.cpp) and passed with the
// kernel arguments, so a block loads it instead of building it.
constexpr uint32_t FLOW_TAB16_DW = FLOW_INPUT_BITS / 4 * 16 / 2;

struct ParseArgs {
    const uint8_t* arena;
    const uint64_t* off;   // LAYOUT_INDEXED (LAYOUT_SEGMENTED: per chunk)
    const uint16_t* len;   // optional for LAYOUT_STRIDED (LAYOUT_SEGMENTED: per chunk)
    uint32_t stride;       // LAYOUT_STRIDED
    uint64_t n;
    void* out;             // n records of the OutMode's type
    const uint32_t* pkt_seg = nullptr;  // LAYOUT_SEGMENTED: n+1 chunk-index bounds
    uint16_t* chunk = nullptr;          // LAYOUT_SEGMENTED, optional: remainder's chunk
    uint64_t* off_out = nullptr;        // LAYOUT_PACKED, optional: the computed offsets
    const uint32_t* tile_local = nullptr;  // LAYOUT_PACKED: tile prefix within its group
    uint32_t policy = 0;                // INGOT_TUNE_CACHE_POLICY bits (launch_parse sets it)
    uint32_t linewin = 0;  // windows from byte 12: >= linewin chunks, then to the line end
    // LAYOUT_SEGMENTED, optional (ingot_gpu_parse_read_first): per packet,
    // chunk 0's (offset << 16) | length, indexed like pkt_seg
    const uint64_t* first = nullptr;
    uint32_t xcd_remap = 0;  // ring kernels: tile-order bits (ring.hip: xcd_bits, k_parse_pipe)
};

struct FlowArgs {
    ParseArgs p;
    uint32_t* flow;  // per-packet bin or INGOT_FLOW_NONE
    uint32_t bin_mask;
    uint32_t* hash;  // optional
    uint32_t w[FLOW_INPUT_BITS];
    alignas(16) uint32_t tab16[FLOW_TAB16_DW];  // entry (p, v) at half-word 16p + v
};

// In-place rewrite (ingot_gpu_parse_modify): resolve.cpp resolves each ingot_edit's
// field to its header kind and BE bit geometry, so the kernel needs no tables.
enum HdrKind : uint8_t { HK_ETH, HK_VLAN, HK_V4, HK_V6, HK_TCP, HK_UDP, HK_ICMP, HK_GENEVE };
struct Edit {
    uint8_t layer, kind, op, index;
    uint8_t byte0, nbytes, rshift, bits;  // field bytes [byte0, byte0+nbytes) of the header
    uint32_t value;
};
struct ModifyArgs {
    ParseArgs p;
    uint32_t wb = 32;  // ring kernel: write-back unit in bytes (16, 32, 64)
    uint32_t n_edits;
    Edit e[INGOT_MAX_EDITS];
};
// ingot_gpu_parse_modify_csum: the rewrite's arguments and, after them (so
// the plain rewrite kernels keep their own argument block, byte for byte),
// which sums edit k's bytes feed, resolved by resolve.cpp from the edit's layer
// and field, and the sums the call selected.
struct ModifyCsumArgs {
    ModifyArgs m;
    uint8_t feeds[INGOT_MAX_EDITS];  // CsumFeed bits
    uint32_t what;                   // INGOT_CSUM_* bits
};
// An edit's bytes are covered by the IPv4 header sum, by its layer's L4 sum
// (the fixed L4 header), by the L4 sum's IPv4 pseudo-header (the addresses:
// fed only when the packet's L4 layer has one) or by the tunnel's outer UDP sum.
enum CsumFeed : uint8_t { FEED_L3 = 1, FEED_L4 = 2, FEED_OUTER = 4, FEED_PSEUDO4 = 8 };
// ingot_gpu_parse_modify_rows: per-packet operands.  resolve.cpp resolves each
// ingot_edit_rows to one piece (a narrow field) or to 4-byte SET pieces (an
// IPv6 address: 4; a MAC: a 4-byte and a 2-byte one), each an Edit of at most
// 4 bytes for the shared apply_edit, with where its operand comes from.  A
// block of its own, so the ModifyArgs / ModifyCsumArgs kernels keep theirs.
enum RowSource : uint8_t {
    ROWS_VALUE = 0,  // e.value
    ROWS_U16 = 1,    // host-endian u16 at the row (aligned)
    ROWS_U32 = 2,    // host-endian u32 at the row (aligned)
    ROWS_BE16 = 3,   // 2 bytes of the row, big-endian (any alignment)
    ROWS_BE32 = 4    // 4 bytes of the row, big-endian (any alignment)
};
struct RowPiece {
    Edit e;                 // e.value: the operand of a ROWS_VALUE piece
    uint8_t source;         // RowSource
    uint8_t by;             // INGOT_BY_PACKET / INGOT_BY_ROW
    uint8_t feeds;          // CsumFeed bits
    uint8_t _pad;
    uint32_t pitch;         // bytes between rows
    const uint8_t* values;  // the table + the piece's byte offset in its row
};
constexpr uint32_t ROWS_MAX_PIECES = 4 * INGOT_MAX_EDITS;
struct ModifyRowsArgs {
    ParseArgs p;
    const uint32_t* row;  // optional: per-packet row index (the row guard)
    uint32_t n_rows;
    uint32_t what;        // INGOT_CSUM_* bits, or 0
    uint32_t n_pieces;
    RowPiece e[ROWS_MAX_PIECES];
};
static_assert(sizeof(RowPiece) == 32, "RowPiece is 32 bytes");
static_assert(sizeof(ModifyRowsArgs) <= 4096,
              "ModifyRowsArgs exceeds the 4 KiB kernel-argument limit");
// 3,824 B today (ParseArgs + key windows + the 16-bit table): the kernarg
// segment is 4 KiB, and a larger FlowArgs would fail flow launches at run
// time, not here.
static_assert(sizeof(FlowArgs) <= 4096, "FlowArgs exceeds the 4 KiB kernel-argument limit");

// Persistent ring consumer (ingot_gpu_parse_ring): one launch parses up to
// INGOT_RING_MAX_BATCHES batches of n fixed slots, batch b from b.arena into
// b.out; tiles of batch b are staged only once b is published (b < published,
// or the doorbell word reaches db_first + b).
struct RingBatch {
    const uint8_t* arena;
    void* out;
};
struct RingArgs {
    uint64_t n;               // frames per batch
    uint32_t stride;          // slot bytes (>= 64, multiple of 16)
    uint32_t nbatches;
    uint32_t policy;          // INGOT_TUNE_CACHE_POLICY bits
    uint32_t published;       // batches known published at launch (no poll below)
    const uint32_t* doorbell; // device address of the doorbell word, or NULL
    uint32_t db_first;        // doorbell value that publishes batch 0
    uint32_t tiles_per_batch;
    uint64_t timeout_ticks;   // wall-clock ticks a wave waits for a batch
    uint32_t* status;         // optional: |= 1 when a wave gave up waiting
    uint32_t groups = 1;      // batch groups in flight at once (launch_ring)
    RingBatch b[INGOT_RING_MAX_BATCHES];
};
static_assert(sizeof(RingArgs) <= 4096, "RingArgs exceeds the 4 KiB kernel-argument limit");

// Histogram pass over flow bins (flow.hip).
hipError_t launch_flow_hist(const uint32_t* flow, uint64_t n, uint32_t* hist, uint32_t bins,
                            void* work, size_t work_bytes, hipStream_t s);
size_t flow_hist_workspace(uint64_t n, uint32_t bins);

// Single-header parse (ingot_gpu_parse_header, header.hip).
struct HeaderArgs {
    const uint8_t* arena;
    const uint64_t* off;  // NULL: slots of `stride`
    const uint16_t* len;
    uint32_t stride;
    uint64_t n;
    int kind;              // enum ingot_header_kind
    const uint32_t* hints;  // per-slice choice hints, or NULL: `hint`
    uint32_t hint;
    ingot_hdr* out;
};
hipError_t launch_header(const HeaderArgs& a, hipStream_t s);

// Batched Emit (ingot_gpu_emit_packets / _headers, emit.hip).  resolve.cpp
// resolves each ingot_emit_set to the covering bytes of its field in the
// header block, so the kernel needs no tables.
struct EmitSet {
    uint16_t pos;      // first covering byte of the field in the header block
    uint16_t at;       // INGOT_EMIT_LENGTH counts the packet's bytes from here
    uint8_t nbytes, rshift, bits, source;
    int32_t add;
    const void* values;  // U16 / U32 sources: n per-packet values
};
struct EmitArgs {
    const uint8_t* src;      // NULL: header blocks only
    const uint64_t* off;     // source offsets (whole packets)
    const uint16_t* len;     // payload bytes per packet
    uint8_t* dst;
    const uint64_t* dst_off; // NULL: i * stride
    uint32_t stride;
    uint32_t hdr_len;
    uint64_t n;
    uint32_t n_sets;
    EmitSet sets[INGOT_MAX_EMIT_SETS];
    uint32_t hdr[INGOT_MAX_EMIT_HDR / 4];  // the header block, zero-padded
    // ingot_gpu_emit_packets_csum: the validated sums, after everything else
    // so the plain emit kernels read their arguments where they always did.
    // Both absent: the plain kernels run.
    struct Sums {
        uint16_t v4_at, v4_len;    // IPV4: the header in hdr, its 4 * ihl bytes
        uint16_t udp_at, udp_l3;   // UDP: the UDP header, the IP header of the pseudo-header
        uint8_t v4, udp, udp_v6;   // which sums; the pseudo-header's IP version is 6
        uint8_t _pad;
    } sums;
};
static_assert(sizeof(EmitArgs) <= 4096, "EmitArgs exceeds the 4 KiB kernel-argument limit");
// bytes of dynamic LDS one emit block needs (checked against the device)
size_t emit_lds_bytes(const EmitArgs& a);
hipError_t launch_emit(const EmitArgs& a, hipStream_t s);

// Emit with per-packet and per-row operands (ingot_gpu_emit_packets_rows, k_emit's
// ROWS instantiations in emit.hip).  resolve.cpp resolves each
// ingot_emit_set_rows, in list order, to one piece (a narrow field: EmitSet's
// geometry) or to big-endian pieces of 4 and 2 bytes (an IPv6 address: 4; a
// MAC: a 4-byte and a 2-byte one), each with where its operand comes from.
// `e` is what emit_args / emit_sums made of the header block, with no sets of
// its own; a block of its own, so the EmitArgs kernels keep theirs.
enum EmitPieceSource : uint8_t {
    EP_LENGTH = 0,  // as INGOT_EMIT_LENGTH
    EP_U16 = 1,     // host-endian u16 at the row (aligned) + add
    EP_U32 = 2,     // host-endian u32 at the row (aligned) + add
    EP_VALUE = 3,   // add
    EP_BE16 = 4,    // 2 bytes of the row in wire order, byte loads
    EP_BE32 = 5,    // 4 bytes of the row in wire order, byte loads
    EP_BE16A = 6,   // the same from a 2-byte aligned row: one load
    EP_BE32A = 7    // the same from a 4-byte aligned row: one load
};
struct EmitPiece {
    uint16_t pos;           // first covering byte of the piece in the header block
    uint16_t at;            // EP_LENGTH counts the packet's bytes from here
    uint8_t nbytes, rshift, bits;
    uint8_t source;         // EmitPieceSource
    uint8_t by;             // INGOT_BY_PACKET / INGOT_BY_ROW
    uint8_t _pad[3];
    int32_t add;
    uint32_t pitch;         // bytes between rows
    const uint8_t* values;  // the table + the piece's byte offset in its row
};
constexpr uint32_t EMIT_MAX_PIECES = 4 * INGOT_MAX_EMIT_SETS;
struct EmitRowsArgs {
    EmitArgs e;
    const uint32_t* row;  // optional: per-packet row index (the row guard)
    uint32_t n_rows;
    uint32_t n_pieces;
    EmitPiece p[EMIT_MAX_PIECES];
};
static_assert(sizeof(EmitPiece) == 32, "EmitPiece is 32 bytes");
static_assert(sizeof(EmitRowsArgs) <= 4096, "EmitRowsArgs exceeds the 4 KiB kernel-argument limit");
size_t emit_rows_lds_bytes(const EmitRowsArgs& a);
hipError_t launch_emit_rows(const EmitRowsArgs& a, hipStream_t s);

// Emit over parse_read's chunk tables (ingot_gpu_emit_packets_read,
// k_emit_read in emit_read.hip).  `e` is what emit_args / emit_sums made of the
// header block; e.src is the chunk arena, e.off / e.len / e.stride are unused.
struct EmitReadArgs {
    EmitArgs e;
    const uint64_t* seg_off;   // per chunk
    const uint16_t* seg_len;   // per chunk
    const uint32_t* pkt_seg;   // n+1 chunk-index bounds
    const uint16_t* from;      // optional: first logical byte taken
    const uint16_t* take;      // optional: at most this many bytes
    uint16_t* taken;           // optional: payload bytes written
};
static_assert(sizeof(EmitReadArgs) <= 4096, "EmitReadArgs exceeds the 4 KiB kernel-argument limit");
size_t emit_read_lds_bytes(const EmitReadArgs& a);
hipError_t launch_emit_read(const EmitReadArgs& a, hipStream_t s);

// The two together (ingot_gpu_emit_packets_read_rows, k_emit_read's ROWS
// instantiations): EmitReadArgs with no sets of its own in r.e, then what
// EmitRowsArgs has behind its `e`.  A block of its own again, so the
// EmitReadArgs kernels keep theirs.
struct EmitReadRowsArgs {
    EmitReadArgs r;
    const uint32_t* row;  // optional: per-packet row index (the row guard)
    uint32_t n_rows;
    uint32_t n_pieces;
    EmitPiece p[EMIT_MAX_PIECES];
};
static_assert(sizeof(EmitReadRowsArgs) <= 4096,
              "EmitReadRowsArgs exceeds the 4 KiB kernel-argument limit");
size_t emit_read_rows_lds_bytes(const EmitReadRowsArgs& a);
hipError_t launch_emit_read_rows(const EmitReadRowsArgs& a, hipStream_t s);

// Batched Internet checksums (ingot_gpu_checksum_verify / _fill, csum.hip).
struct CsumArgs {
    uint8_t* arena;        // written only when `fill`
    const uint64_t* off;   // NULL: slots of `stride`
    const uint16_t* len;   // NULL (slots only): `stride`
    uint32_t stride;
    uint32_t what;         // INGOT_CSUM_L3 | INGOT_CSUM_L4
    uint64_t n;
    const ingot_rec* rec;
    ingot_csum* out;       // optional when `fill`
    uint32_t fill;
};
hipError_t launch_csum(const CsumArgs& a, hipStream_t s);

// The same sums over parse_read's chunk tables (ingot_gpu_checksum_verify_read /
// _fill_read, k_csum_read in csum.hip): packet i is the chunks pkt_seg[i] ..
// pkt_seg[i+1] of (seg_off, seg_len).
struct CsumReadArgs {
    uint8_t* arena;            // written only when `fill`
    const uint64_t* seg_off;   // per chunk
    const uint16_t* seg_len;   // per chunk
    const uint32_t* pkt_seg;   // n+1 chunk-index bounds
    uint64_t n;
    const ingot_rec* rec;
    ingot_csum* out;           // optional when `fill`
    uint32_t what;             // INGOT_CSUM_L3 | INGOT_CSUM_L4
    uint32_t fill;
};
hipError_t launch_csum_read(const CsumReadArgs& a, hipStream_t s);

// Lengths-only packed frames (packed.hip): tile base = u64 base of its group
// of PACKED_GROUP tiles (at the start of `work`, >= packed_workspace(n)
// bytes) + the tile's u32 prefix within the group (after the group bases).
constexpr uint32_t PACKED_GROUP = 128;
size_t packed_workspace(uint64_t n);
hipError_t launch_tile_bases(const uint16_t* len, uint64_t n, void* work, hipStream_t s);

// One wave that holds its stream for `ticks` of the device's constant-rate
// wall clock (ingot_gpu_stream_delay, stream.hip).
hipError_t launch_delay(uint64_t ticks, hipStream_t s);

// Per-context tuning (0 = measured default); see INGOT_TUNE_* in ingot_gpu.h.
struct Tuning {
    int window_indexed = 0;
    int window_strided = 0;
    uint32_t max_blocks = 0;
    int pipeline = 0;  // ring kernels: 0 = auto (ring_grid blocks per CU), 1 = off, k = k tiles
                       // per wave
    int pipe_depth = 0;    // ring kernels: LDS images per wave, 2..4 (rewrite: 2 or 3); 0 = the
                           // default: one image restaged in place (slot-ring parse), 2
                           // (consumer, rewrite)
    int writeback = 0;     // ring rewrite kernel: write-back unit (0 = measured default)
    int cache_policy = 0;  // bit 0: nt staging loads; bit 1: nt record stores
    int flow_table = 0;    // flows: 0 = auto (16-bit table when it suffices), 32 = 32-bit
    int slow_path = 0;     // bytes past the window: per-lane loads (0, the only value left)
    int read_plan = 0;     // parse_read: 0 / 11 line-completing chunk-0 window, 1 = 4 pieces,
                           // 17 = chunk bounds loaded lazily (parse_read_first)
    int flow_kernel = 0;   // flows: 0 / 15 = the measured default (k_flows_bits when it applies)
    int ring_grid = 0;     // ring consumer and slot-ring parse: blocks per CU (0 = default, 2;
                           // the rewrite kernel's grid is always 2 per CU)
    int ring_groups = 0;   // ring consumer: batches in flight at once (0 = measured default)
    int xcd_remap = 0;     // slot ring: 1 = each XCD's blocks take a contiguous share of tiles
    uint32_t cus = 256;  // compute units of the context's device (grid shaping)
    bool host_arena = false;  // per call: the arena is host memory (ingot_gpu_host_map)
};

hipError_t launch_parse(const ParseArgs& a, int layout_kind, int chain, int mode,
                        const Tuning& t, hipStream_t s);
hipError_t launch_flows(const FlowArgs& a, int layout_kind, int chain, const Tuning& t,
                        hipStream_t s);
hipError_t launch_ring(const RingArgs& a, int chain, int mode, const Tuning& t, hipStream_t s);
// Flow classification over the plain parse's window with the table-free
// Toeplitz hash (tuple.hip, k_flows_bits): offset-addressed device frames,
// 16-bit bins, not the tunnel chain.
hipError_t launch_flows_tuple(const FlowArgs& a, int chain, const Tuning& t, hipStream_t s);
// launch_parse's branches in their own files: parse_read over chunk lists
// (read.hip; `a` with its cache policy set, `g` the one-tile-per-wave grid)
// and the slot-ring kernels (ring.hip).
hipError_t launch_segmented(const ParseArgs& a, int chain, int mode, const Tuning& t, uint32_t g,
                            hipStream_t s);
hipError_t launch_slot_ring(const ParseArgs& a, int chain, int mode, const Tuning& t,
                            hipStream_t s);
hipError_t launch_modify_ring(const ModifyArgs& a, int chain, const Tuning& t, hipStream_t s);
hipError_t launch_modify(const ModifyArgs& a, int layout_kind, int chain, const Tuning& t,
                         hipStream_t s);
// The same two with the fused checksum update (the CSUM instantiations).
hipError_t launch_modify_ring_csum(const ModifyCsumArgs& a, int chain, const Tuning& t,
                                   hipStream_t s);
hipError_t launch_modify_csum(const ModifyCsumArgs& a, int layout_kind, int chain,
                              const Tuning& t, hipStream_t s);
// The rewrite with per-packet operands (ingot_gpu_parse_modify_rows): k_parse's
// OUT_MODIFY kernels only, never the slot-ring kernel.
hipError_t launch_modify_rows(const ModifyRowsArgs& a, int layout_kind, int chain,
                              const Tuning& t, hipStream_t s);
// The rewrite over parse_read's chunk tables (ingot_gpu_parse_read_modify[_csum],
// read.hip): `a.p` holds the CSR tables as LAYOUT_SEGMENTED does, out and chunk
// both optional.
hipError_t launch_read_modify(const ModifyArgs& a, int chain, const Tuning& t, hipStream_t s);
hipError_t launch_read_modify_csum(const ModifyCsumArgs& a, int chain, const Tuning& t,
                                   hipStream_t s);
// The same with per-packet operands (ingot_gpu_parse_read_modify_rows, read.hip).
hipError_t launch_read_modify_rows(const ModifyRowsArgs& a, int chain, const Tuning& t,
                                   hipStream_t s);
bool tuning_valid(int key, int value);

}  // namespace ingot_gpu
