/*
 * ingot_gpu.h — C ABI of the MI355X (gfx950) batched L2/L3/L4 header extractor.
 *
 * This is the drop-in boundary for ingot's per-packet parse path.  In ingot the
 * path sits behind Rust traits, not an FFI:
 *
 *   HeaderParse::parse / parse_choice      ingot-types/src/lib.rs:137-147
 *   Success<T, B> = (T, Option<Denom>, B)   ingot-types/src/lib.rs:208
 *   <Chain>::parse_slice(from)              ingot-macros/src/parse.rs:496-509
 *   PacketParseError { label, inner }       ingot-types/src/error.rs:119-171
 *   ParseError (8 kinds)                    ingot-types/src/error.rs:21-44
 *
 * and it is called once per packet by the caller's loop
 * (ingot-examples/benches/packet.rs:136-172).  The entry points below replace
 * that loop + the parse bodies for a whole batch at once: the caller owns a
 * packet arena in device memory (borrow semantics: nothing is copied, nothing
 * is allocated per call) and gets one fixed-size record per packet that says
 * what `parse_slice` would have returned — Ok with the layer views as
 * (offset, kind) pairs and the remainder offset, or the PacketParseError
 * (failing layer index == label, ParseError discriminant).
 *
 * Plain C, plain pointers and sizes; `stream` is a hipStream_t passed as void*
 * (NULL = the null stream).  Every call is asynchronous on `stream`.  API
 * errors are negative ints (see ingot_gpu_strerror); per-packet parse errors
 * live in the records and are never API errors — like ingot, malformed input
 * never fails the call.
 *
 * Threading: a context is bound to one device; calls on distinct contexts or
 * distinct streams may run concurrently.  The context holds no per-call state.
 */
#ifndef INGOT_GPU_H
#define INGOT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: ingot_gpu_checksum_verify / ingot_gpu_checksum_fill (ingot_csum);
 *    ingot_gpu_parse_modify_csum, ingot_gpu_checksum_verify_read / _fill_read,
 *    ingot_gpu_parse_read_modify / ingot_gpu_parse_read_modify_csum,
 *    ingot_gpu_parse_modify_rows, ingot_gpu_parse_read_modify_rows,
 *    ingot_gpu_flow_table_* /
 *    ingot_gpu_flow_key_hash (added calls: the number stays).
 * 3: ingot_gpu_comm_wrap (borrow the host's RCCL communicator).
 * 2: ingot_gpu_comm_* / ingot_gpu_flow_hist_allreduce (config 5's reduce);
 *    host mappings counted per map, ingot_gpu_host_unmap EINVAL for a pointer
 *    the context never mapped (1: any pointer, hipHostUnregister'd). */
#define INGOT_GPU_ABI_VERSION 4

/* ---------------------------------------------------------------------------
 * Per-packet status: 0 = Ok, else 1 + the ParseError discriminant in the
 * declaration order of ingot-types/src/error.rs:22-44.  Reachable: UNWANTED
 * and TOO_SMALL, STRADDLED_HEADER under ingot_gpu_parse_read;
 * the others are listed so the numbering is ingot's.
 * ------------------------------------------------------------------------- */
enum ingot_status {
    INGOT_OK = 0,
    INGOT_ERR_UNWANTED = 1,
    INGOT_ERR_NEEDS_HINT = 2,
    INGOT_ERR_TOO_SMALL = 3,
    INGOT_ERR_STRADDLED_HEADER = 4,
    INGOT_ERR_NO_REMAINING_CHUNKS = 5,
    INGOT_ERR_CANNOT_ACCEPT = 6,
    INGOT_ERR_REJECT = 7,
    INGOT_ERR_ILLEGAL_VALUE = 8
};

/* ---------------------------------------------------------------------------
 * Parse chains (the `#[derive(Parse)]` structs the batch is parsed as).
 *
 * UDP_PARSER   ingot-examples/src/packets.rs:18-24
 *              eth: Ethernet, l3: L3 (v4|v6), l4: from L4 (tcp|udp) -> Udp
 *              layer labels "eth", "l3", "l4"
 * GENERIC_ULP  ingot-examples/src/packets.rs:54-60  (control = exit_on_arp)
 *              inner_eth: Ethernet, inner_l3: Option<L3>, inner_ulp: Option<Ulp>
 *              layer labels "inner_eth", "inner_l3", "inner_ulp"
 * VLAN_ULP     build-defined (ingot declares VlanBody, ethernet.rs:57-65, but
 *              no chain uses it): eth, 0..2 x VlanBody while the ethertype is
 *              0x8100/0x9100, L3, Ulp; no control.  Labels "eth", "vlan",
 *              "l3", "l4".  Parity for this chain is unpinned by the reference.
 * GENEVE_OVER_V6  ingot-examples/src/packets.rs:27-40 (OPTE's inbound path)
 *              outer_eth: Ethernet, outer_v6: from L3 -> Ipv6 (+EHs),
 *              outer_udp: from L4 -> Udp, outer_encap: Geneve (+options,
 *              geneve.rs:16-44), then GenericUlp's three layers (control =
 *              exit_on_arp on inner_eth).  Labels "outer_eth", "outer_v6",
 *              "outer_udp", "outer_encap", "inner_eth", "inner_l3", "inner_ulp".
 * ------------------------------------------------------------------------- */
enum ingot_chain {
    INGOT_CHAIN_UDP_PARSER = 0,
    INGOT_CHAIN_GENERIC_ULP = 1,
    INGOT_CHAIN_VLAN_ULP = 2,
    INGOT_CHAIN_GENEVE_OVER_V6 = 3,
    INGOT_CHAIN_COUNT = 4
};

enum ingot_l3_kind { INGOT_L3_NONE = 0, INGOT_L3_IPV4 = 1, INGOT_L3_IPV6 = 2 };
enum ingot_l4_kind {
    INGOT_L4_NONE = 0,
    INGOT_L4_TCP = 1,
    INGOT_L4_UDP = 2,
    INGOT_L4_ICMPV4 = 3,
    INGOT_L4_ICMPV6 = 4
};

/* rec.flags */
#define INGOT_REC_ACCEPTED 0x01u /* a parse control accepted early (parse.rs:221-254) */
#define INGOT_REC_INNER 0x02u    /* tunnel chain: the walk reached inner_eth */

/* ---------------------------------------------------------------------------
 * ingot_rec — the 16-byte per-packet result.
 *
 * Fields are filled as the chain walks, so an error record still shows how
 * far the walk got:
 *   status/err_layer  Ok, or (1+ParseError, index of the failing layer label)
 *                     err_layer = 0xff when Ok.
 *   l3_kind/l4_kind   set when the L3 / L4 choice selects a variant (before
 *                     that variant is parsed).
 *   l3_off/l4_off     frame offset where the L3 / L4 layer starts (0 = never
 *                     reached).
 *   payload_off       offset of the remainder: bytes consumed by the headers
 *                     that parsed successfully (== remainder start on Ok).
 *   ethertype         the Ethertype hint handed to the L3 choice (after VLAN
 *                     tags); 0 if Ethernet did not parse.
 *   l4_proto          the IpProtocol hint handed to the L4 choice (IPv6: the
 *                     last extension header's next_header, ip.rs:180-181,
 *                     util.rs:189-228).
 *   n_vlan/n_v6ext    VLAN tags / IPv6 extension headers fully parsed.
 *
 * GENEVE_OVER_V6: the fields describe the innermost layers reached.  While
 * the walk is in the outer layers they describe outer_v6 / outer_udp; once
 * inner_eth parses, flags |= INGOT_REC_INNER and l3/l4 kind, offsets,
 * n_v6ext, l4_proto restart for the inner frame (ethertype = the inner one).
 * The inner frame then starts at l3_off - 14 (inner L3 reached) or
 * payload_off - 14 (walk ended at inner_eth); ingot_gpu_geneve_fields gives
 * every outer offset and getter.
 * ------------------------------------------------------------------------- */
typedef struct ingot_rec {
    uint8_t status;
    uint8_t err_layer;
    uint8_t l3_kind;
    uint8_t l4_kind;
    uint8_t n_vlan;
    uint8_t n_v6ext;
    uint8_t l4_proto;
    uint8_t flags;
    uint16_t l3_off;
    uint16_t l4_off;
    uint16_t payload_off;
    uint16_t ethertype;
} ingot_rec;

/* ---------------------------------------------------------------------------
 * ingot_rec8 — the same result in 8 bytes (for record-bandwidth-bound
 * callers).  Everything a caller needs to rebuild the layer views is kept;
 * the dropped rec16 fields are derivable from it and the frame:
 *   l3_off    = 14 + 4*n_vlan            (when l3_kind != NONE)
 *   ethertype = be16(frame, 12 + 4*n_vlan)
 *   err_layer = 0xff when status == Ok
 *
 *   b0: status (bits 0-3) | err_layer (bits 4-5, 0 when Ok) | l3_kind (bits 6-7)
 *   b1: l4_kind (bits 0-2) | n_vlan (bits 3-4) | accepted (bit 5)
 * ------------------------------------------------------------------------- */
typedef struct ingot_rec8 {
    uint8_t status_layer_l3;
    uint8_t l4_vlan_flags;
    uint8_t n_v6ext;
    uint8_t l4_proto;
    uint16_t l4_off;
    uint16_t payload_off;
} ingot_rec8;

/* One IPv6 extension header as ingot's getters see it
 * (IpV6ExtFragment ip.rs:190-200, IpV6Ext6564 ip.rs:202-211). */
#define INGOT_EH_FRAGMENT 1
#define INGOT_EH_RFC6564 2
#define INGOT_MAX_EH_FIELDS 4 /* first 4 EHs are materialised; count is exact */

typedef struct ingot_v6eh {
    uint32_t ident;         /* fragment: ident (u32be) */
    uint16_t frag_offset;   /* fragment: fragment_offset (u13be) */
    uint16_t off;           /* frame offset of this EH */
    uint8_t kind;           /* INGOT_EH_FRAGMENT / INGOT_EH_RFC6564 */
    uint8_t next_header;    /* both */
    uint8_t ext_len;        /* 6564: ext_len; fragment: reserved */
    uint8_t frag_res_more;  /* fragment: res << 1 | more_frags */
} ingot_v6eh;

/* ---------------------------------------------------------------------------
 * ingot_fields — every getter of every header on the chain, materialised
 * (parity mode).  Values are exactly what ingot's generated XRef getters
 * return (bitfield.rs:40-315 BE bit order; NetworkRepr conversions applied:
 * `*_ecn` is Ecn::from_network (3 -> Capable0 == 1, ip.rs:111-119), flags are
 * bitflags from_bits_truncate (identity on the stored bits)).  Variable-length
 * fields (options, EH data) are given as (offset, length) into the frame.
 * Headers that were not reached are all-zero.
 * ------------------------------------------------------------------------- */
typedef struct ingot_fields {
    ingot_rec rec;                      /*   0 */
    /* 32-bit */
    uint32_t v6_flow_label;             /*  16 */
    uint32_t tcp_sequence;              /*  20 */
    uint32_t tcp_acknowledgement;       /*  24 */
    /* 16-bit */
    uint16_t eth_ethertype;             /*  28 */
    uint16_t vlan_vid[2];               /*  30 */
    uint16_t vlan_ethertype[2];         /*  34 */
    uint16_t v4_total_len;              /*  38 */
    uint16_t v4_identification;         /*  40 */
    uint16_t v4_fragment_offset;        /*  42 */
    uint16_t v4_checksum;               /*  44 */
    uint16_t v4_options_off;            /*  46 */
    uint16_t v4_options_len;            /*  48 */
    uint16_t v6_payload_len;            /*  50 */
    uint16_t v6_ext_off;                /*  52  RepeatedView span start */
    uint16_t v6_ext_len;                /*  54  RepeatedView span bytes */
    uint16_t l4_source;                 /*  56  tcp/udp source */
    uint16_t l4_destination;            /*  58  tcp/udp destination */
    uint16_t tcp_window_size;           /*  60 */
    uint16_t tcp_checksum;              /*  62 */
    uint16_t tcp_urgent_ptr;            /*  64 */
    uint16_t tcp_options_off;           /*  66 */
    uint16_t tcp_options_len;           /*  68 */
    uint16_t udp_length;                /*  70 */
    uint16_t udp_checksum;              /*  72 */
    uint16_t icmp_checksum;             /*  74 */
    /* 8-bit */
    uint8_t eth_destination[6];         /*  76 */
    uint8_t eth_source[6];              /*  82 */
    uint8_t vlan_priority[2];           /*  88 */
    uint8_t vlan_dei[2];                /*  90 */
    uint8_t v4_version;                 /*  92 */
    uint8_t v4_ihl;                     /*  93 */
    uint8_t v4_dscp;                    /*  94 */
    uint8_t v4_ecn_raw;                 /*  95 */
    uint8_t v4_ecn;                     /*  96 */
    uint8_t v4_flags;                   /*  97 */
    uint8_t v4_hop_limit;               /*  98 */
    uint8_t v4_protocol;                /*  99 */
    uint8_t v4_source[4];               /* 100 */
    uint8_t v4_destination[4];          /* 104 */
    uint8_t v6_version;                 /* 108 */
    uint8_t v6_dscp;                    /* 109 */
    uint8_t v6_ecn_raw;                 /* 110 */
    uint8_t v6_ecn;                     /* 111 */
    uint8_t v6_next_header;             /* 112 */
    uint8_t v6_hop_limit;               /* 113 */
    uint8_t v6_source[16];              /* 114 */
    uint8_t v6_destination[16];         /* 130 */
    uint8_t tcp_data_offset;            /* 146 */
    uint8_t tcp_reserved;               /* 147 */
    uint8_t tcp_flags;                  /* 148 */
    uint8_t icmp_ty;                    /* 149 */
    uint8_t icmp_code;                  /* 150 */
    uint8_t icmp_rest_of_hdr[4];        /* 151 */
    uint8_t _pad0;                      /* 155 */
    ingot_v6eh v6_eh[INGOT_MAX_EH_FIELDS]; /* 156 (4 x 12) */
    uint8_t _pad1[52];                  /* 204 -> 256 */
} ingot_fields;

/* ---------------------------------------------------------------------------
 * GENEVE_OVER_V6 parity mode: the outer layers' getters (128 B) after the
 * inner frame's ingot_fields (whose eth_* / v4_* / v6_* / l4 fields are
 * inner_eth / inner_l3 / inner_ulp).  Geneve getters follow geneve.rs:16-44:
 * version u2, opt_len u6, flags = GeneveFlags::from_bits_truncate (bits 0xC0
 * kept), protocol_type u16be, vni [u8;3] as a 24-bit BE integer, reserved
 * u8.  Options (Repeated<GeneveOpt>, geneve.rs:80-102) are listed in order;
 * the first INGOT_MAX_GENEVE_OPT_FIELDS are materialised, the count is exact.
 * ------------------------------------------------------------------------- */
#define INGOT_MAX_GENEVE_OPT_FIELDS 4

typedef struct ingot_geneve_opt {
    uint16_t opt_class;     /* class (u16be) */
    uint16_t data_off;      /* frame offset of data (length*4 bytes) */
    uint8_t option_type;    /* GeneveOptionType (is_critical = bit 7) */
    uint8_t reserved;       /* u3 */
    uint8_t length;         /* u5, in 4-byte words */
    uint8_t _pad;
} ingot_geneve_opt;

typedef struct ingot_tunnel_fields {
    uint8_t outer_eth_destination[6];   /*   0 */
    uint8_t outer_eth_source[6];        /*   6 */
    uint16_t outer_eth_ethertype;       /*  12 */
    uint16_t outer_udp_off;             /*  14  frame offset of outer_udp */
    uint8_t outer_v6_source[16];        /*  16 */
    uint8_t outer_v6_destination[16];   /*  32 */
    uint32_t outer_v6_flow_label;       /*  48 */
    uint16_t outer_v6_payload_len;      /*  52 */
    uint16_t outer_v6_ext_len;          /*  54  EH span bytes (from offset 54) */
    uint8_t outer_v6_version;           /*  56 */
    uint8_t outer_v6_dscp;              /*  57 */
    uint8_t outer_v6_ecn_raw;           /*  58 */
    uint8_t outer_v6_ecn;               /*  59 */
    uint8_t outer_v6_next_header;       /*  60 */
    uint8_t outer_v6_hop_limit;         /*  61 */
    uint8_t outer_v6_n_ext;             /*  62 */
    uint8_t outer_l4_proto;             /*  63  hint handed to the outer L4 choice */
    uint16_t outer_udp_source;          /*  64 */
    uint16_t outer_udp_destination;     /*  66 */
    uint16_t outer_udp_length;          /*  68 */
    uint16_t outer_udp_checksum;        /*  70 */
    uint16_t geneve_off;                /*  72 */
    uint16_t inner_eth_off;             /*  74 */
    uint32_t geneve_vni;                /*  76 */
    uint16_t geneve_protocol_type;      /*  80 */
    uint8_t geneve_version;             /*  82 */
    uint8_t geneve_opt_len;             /*  83 */
    uint8_t geneve_flags;               /*  84 */
    uint8_t geneve_reserved;            /*  85 */
    uint8_t geneve_n_opts;              /*  86  (saturates at 255) */
    uint8_t geneve_critical;            /*  87  any option_type.is_critical() */
    ingot_geneve_opt geneve_opt[INGOT_MAX_GENEVE_OPT_FIELDS]; /* 88 (4 x 8) */
    uint8_t _pad[8];                    /* 120 -> 128 */
} ingot_tunnel_fields;

typedef struct ingot_geneve_fields {
    ingot_fields inner;                 /*   0  rec + inner layers */
    ingot_tunnel_fields outer;          /* 256 */
} ingot_geneve_fields;

#ifdef __cplusplus
static_assert(sizeof(ingot_rec) == 16, "ingot_rec is 16 bytes");
static_assert(sizeof(ingot_rec8) == 8, "ingot_rec8 is 8 bytes");
static_assert(sizeof(ingot_v6eh) == 12, "ingot_v6eh is 12 bytes");
static_assert(sizeof(ingot_fields) == 256, "ingot_fields is 256 bytes");
static_assert(sizeof(ingot_geneve_opt) == 8, "ingot_geneve_opt is 8 bytes");
static_assert(sizeof(ingot_tunnel_fields) == 128, "ingot_tunnel_fields is 128 bytes");
static_assert(sizeof(ingot_geneve_fields) == 384, "ingot_geneve_fields is 384 bytes");
#endif

/* API return codes (negative). */
#define INGOT_GPU_SUCCESS 0
#define INGOT_GPU_EINVAL (-1)   /* bad argument (null pointer, bad chain ...) */
#define INGOT_GPU_EHIP (-2)     /* a HIP runtime call failed */
#define INGOT_GPU_ENOMEM (-3)   /* context allocation failed */
#define INGOT_GPU_ENODEV (-4)   /* no such device / no gfx950 code object */
#define INGOT_GPU_ERANGE (-5)   /* size outside what the ABI supports */

typedef struct ingot_gpu_ctx ingot_gpu_ctx;

/* Library / ABI identification. */
int ingot_gpu_abi_version(void);
const char* ingot_gpu_build_info(void);

/* Context: binds a device.  Cheap; owns no per-call buffers. */
int ingot_gpu_ctx_create(int device, ingot_gpu_ctx** out);
void ingot_gpu_ctx_destroy(ingot_gpu_ctx* ctx);
int ingot_gpu_ctx_device(const ingot_gpu_ctx* ctx);

/*
 * Zero-copy host rings.  The path often starts and ends in host memory (a NIC
 * or loopback ring).  ingot_gpu_host_map makes host memory [host, host+bytes)
 * device-addressable — memory already pinned by hipHostMalloc is used as it
 * is, pageable memory is page-locked and mapped (hipHostRegister, mapped) —
 * and returns the device address of `host` in *d_ptr.  That address may be
 * passed as any device pointer of the calls below (d_arena, descriptors,
 * d_out ...): the kernels then read only the header bytes they touch across
 * PCIe (LDS-DMA staging from host memory) instead of a whole-frame
 * hipMemcpy, and can write records straight into host memory.  Results are
 * identical to a device-resident arena.
 *
 * Mappings are counted.  Every successful ingot_gpu_host_map is paired with
 * one ingot_gpu_host_unmap(ctx, host) by the same context and the same
 * `host` (INGOT_GPU_EINVAL if this context holds no mapping starting there).
 * The library unregisters only what it registered itself: pageable ranges it
 * page-locked, once the last mapping inside them is unmapped (by any context)
 * or its context is destroyed.  Memory pinned by someone else (hipHostMalloc,
 * the caller's own hipHostRegister) is never unregistered: unmapping it only
 * forgets the mapping.  A range inside one registered by an earlier map
 * shares that registration (e.g. a record buffer carved out of a mapped
 * ring); a range that partly overlaps one is refused (INGOT_GPU_EINVAL).
 * Two buffers whose bytes are disjoint but share a page are registered
 * separately and may be mapped at the same time.  The caller keeps the bytes
 * stable while a call that reads them runs, unmaps only after the calls that
 * use a mapping have completed, and frees (or munmaps) pageable memory only
 * after unmapping it: a registration whose pages were freed leaves a stale
 * device mapping behind.
 */
int ingot_gpu_host_map(ingot_gpu_ctx* ctx, void* host, size_t bytes, void** d_ptr);
int ingot_gpu_host_unmap(ingot_gpu_ctx* ctx, void* host);

/*
 * Doorbells.  A ring consumer that knows its next batches in advance (a NIC
 * or loopback ring: slot k of the ring is batch k) can enqueue their parse
 * launches before the frames arrive, each behind a doorbell wait; the
 * producer publishes batch k by writing k (or more) into the doorbell from
 * the host, and the GPU starts the queued launch with no host round trip
 * (no launch latency on the critical path).  The doorbell is one 32-bit word
 * of pinned host memory polled by the GPU's command processor
 * (hipStreamWaitValue32, compare >=).  *host_word may be written directly by
 * the producer (e.g. another thread) or through ingot_gpu_doorbell_ring.
 *   ingot_gpu_doorbell_wait: everything enqueued on `stream` after this call
 *     runs only once *doorbell >= value.  The caller must make sure the
 *     doorbell is eventually rung: a stream left waiting never drains.
 *   ingot_gpu_doorbell_destroy: only after every wait on it has been passed.
 * ENODEV when the device cannot wait on memory values.
 *
 * A doorbell wait holds a whole HARDWARE queue, not just its stream: HIP
 * maps streams round-robin onto GPU_MAX_HW_QUEUES hardware queues (4 by
 * default), and the command processor stops at the wait packet, so every
 * other stream mapped to that queue (a producer's copy stream, RCCL's
 * stream, torch's current stream) stalls behind it until the ring.  A
 * producer must therefore publish frames from the host, or from a stream
 * known to sit on another hardware queue; publishing with GPU work that
 * shares the held queue and ringing only after that work completes
 * deadlocks (tests/test_doorbell.py::test_held_queue_blocks_its_streams).
 * ingot_gpu_parse_ring's in-kernel doorbell has no such constraint.
 */
typedef struct ingot_gpu_doorbell ingot_gpu_doorbell;
int ingot_gpu_doorbell_create(ingot_gpu_ctx* ctx, ingot_gpu_doorbell** out,
                              volatile uint32_t** host_word);
int ingot_gpu_doorbell_wait(ingot_gpu_doorbell* db, uint32_t value, void* stream);
int ingot_gpu_doorbell_ring(ingot_gpu_doorbell* db, uint32_t value);
void ingot_gpu_doorbell_destroy(ingot_gpu_doorbell* db);

/*
 * Persistent ring consumer.  One launch parses `nbatches` (<=
 * INGOT_RING_MAX_BATCHES) batches of `n` frames in fixed slots of `stride`
 * bytes (>= 64, a multiple of 16; no length array, like
 * ingot_gpu_parse_strided with d_len NULL): batch b from batches[b].d_arena
 * into batches[b].d_out (n ingot_rec when record_bytes is 16, n ingot_rec8
 * when 8; not GENEVE_OVER_V6).  The records are exactly those of
 * ingot_gpu_parse_strided over each batch.  Instead of one launch per batch
 * (each paying a grid ramp-up and drain), every wave walks its share of all
 * the batches' tiles in order, keeping the next tile's LDS-DMA in flight
 * across batch boundaries.
 *
 *   db == NULL: every batch is resident when the launch starts.
 *   db != NULL: a wave stages tiles of batch b only once the doorbell word
 *     is >= db_first + b (the producer rings db_first + b after batch b's
 *     frames are in memory; rings may cover several batches at once).  The
 *     wave polls the word (one lane, with sleeps) only when it reaches a batch
 *     not yet known published, then invalidates its caches (system-scope
 *     acquire), so frames written by the host, a copy engine or another
 *     kernel after the launch started are seen.  A wave that waits more than
 *     `timeout_ms` (1..60000) for a batch stops, and *d_status (optional,
 *     device memory, caller-zeroed) gets bit 0 set.  Waves give up one by
 *     one: a wave that reaches the ring later may still see a batch published
 *     and parse its tiles.  So when bit 0 is set, the record buffers of
 *     EVERY batch from the first one not published at launch onward are
 *     undefined (some tiles written, some not); batches published before the
 *     launch are complete.  Every launch ends, rung or not.  Doorbell values
 *     must increase monotonically across ring launches, the last batch's
 *     value db_first + nbatches - 1 must fit in 32 bits (else
 *     INGOT_GPU_ERANGE), and `db` must belong to
 *     ctx's device (else INGOT_GPU_EINVAL).
 * The arenas are read-only for the launch; a batch buffer must not be
 * rewritten while the launch may still read it (a ring reuses a slot only
 * after the launch that consumes it has completed).  Unlike a
 * doorbell_wait, the polling kernel holds no hardware queue: other streams
 * (a producer's copies included) keep running beside it.
 */
#define INGOT_RING_MAX_BATCHES 64
typedef struct ingot_ring_batch {
    const uint8_t* d_arena; /* n slots of `stride` bytes, 16-B aligned */
    void* d_out;            /* n records */
} ingot_ring_batch;
int ingot_gpu_parse_ring(ingot_gpu_ctx* ctx, const ingot_ring_batch* batches,
                         uint32_t nbatches, uint32_t stride, uint64_t n, int chain,
                         uint32_t record_bytes, const ingot_gpu_doorbell* db,
                         uint32_t db_first, uint32_t timeout_ms, uint32_t* d_status,
                         void* stream);

/*
 * Staggered streams.  A consumer that alternates its batches over two (or
 * more) streams keeps one launch ramping up while another drains; started
 * together, the streams' launches ramp and drain in lockstep and that
 * overlap is lost until they drift apart.  ingot_gpu_stream_delay enqueues
 * on `stream` a one-wave wait of `ns` nanoseconds of the device's wall clock
 * (everything enqueued after it starts that much later); enqueued right after
 * a doorbell wait, it starts a second stream behind the first.
 * ENODEV when the device reports no wall-clock rate.
 */
int ingot_gpu_stream_delay(ingot_gpu_ctx* ctx, uint32_t ns, void* stream);

/*
 * Tuning knobs (results never depend on them).  Defaults are the measured
 * best on MI355X; value 0 restores the default.
 *   INGOT_TUNE_WINDOW_INDEXED  16-B chunks staged in LDS per packed frame:
 *                              2,3,4,5,6,8,9, or 100 = no staging; 20 + k:
 *                              record / flow modes, a window from byte 12's
 *                              chunk to the end of the 128-B line its second
 *                              chunk lies in, at most k chunks (packed
 *                              frames: k = 2, 3, 5 or 8); 1000 + 10 m + k:
 *                              the same from at least m chunks.  Defaults:
 *                              records 25 (the tunnel chain 1069; packed
 *                              tunnel frames 8), fields / rewrites 3 (tunnel
 *                              8), mapped host memory 5.  Flows: offset-
 *                              addressed device frames with 16-bit bins use
 *                              k_flows_bits over a 4-to-5-chunk window; any
 *                              explicit value here turns that kernel off and
 *                              runs the k_parse flows mode with the value
 *                              (its own default, for the full 32-bit hash,
 *                              the tunnel chain and host memory: 1056)
 *   INGOT_TUNE_WINDOW_STRIDED  16-B chunks staged per slot: 2,3,4,5,8 or 100
 *                              (default 4 for slots <= 64 B, else 3)
 *   INGOT_TUNE_MAX_BLOCKS      grid cap in 256-thread blocks (0 = one
 *                              64-packet tile per wave)
 *   INGOT_TUNE_PIPELINE        strided rings (slots >= 64 B) without a length
 *                              array, 16- or 8-B records: the multi-tile kernel
 *                              (several tiles per wave, staged by LDS-DMA;
 *                              INGOT_TUNE_PIPE_DEPTH).  0 = on, 2 blocks per CU
 *                              or INGOT_TUNE_RING_GRID's (default); 1 = off;
 *                              k >= 2 = k tiles per wave
 *   INGOT_TUNE_CACHE_POLICY    0 = measured default (non-temporal record
 *                              stores; the ring kernel: non-temporal staging
 *                              loads and, for 16-B records, device-scope
 *                              record stores); else bit 0: stage frame
 *                              bytes with non-temporal loads, bit 1:
 *                              non-temporal record stores (4 = neither);
 *                              bits 3-5, when non-zero, set the record
 *                              stores' cache bits instead of bit 1: 1 sc1,
 *                              2 sc1 nt, 3 sc0 sc1, 4 sc0 sc1 nt, 5 sc0;
 *                              bits 6-8, when non-zero, the staging loads'
 *                              instead of bit 0 (same codes, 6 sc0 nt)
 *   INGOT_TUNE_PIPE_DEPTH      the multi-tile ring kernel's LDS images per
 *                              wave: 0 (default) = a single image, restaged
 *                              once the walk has read it (16.4 KiB of LDS per
 *                              block; the faster one when launches overlap on
 *                              two streams); 2, 3 or 4 = that many tiles in
 *                              flight, the next ones staged while one is
 *                              parsed (2: 32.9 KiB per block; the faster one
 *                              for launches on a single stream).  The rewrite
 *                              ring kernel takes 2 (its default) or 3 and
 *                              ingot_gpu_parse_ring 2 (default) to 4; 4
 *                              means 2 for the rewrite.  Any other value,
 *                              1 included: EINVAL
 *   INGOT_TUNE_WRITEBACK       ingot_gpu_parse_modify on slot rings: bytes
 *                              written back per edited unit, 16, 32 or 64
 *                              (0 = measured default)
 *   INGOT_TUNE_FLOW_TABLE      ingot_gpu_flow_hist's Toeplitz lookup table:
 *                              0 / 16 = 16-bit entries when bins <= 65,536
 *                              and no full hash is requested (default), 32 =
 *                              always 32-bit entries (same flow bins)
 *   INGOT_TUNE_SLOW_PATH       bytes past the staged window: 0 = read per
 *                              lane from L2/HBM (the only value; the
 *                              compacted re-stage and resume-style variants
 *                              lost and were removed: EINVAL)
 *   INGOT_TUNE_READ_PLAN       ingot_gpu_parse_read / _read_first (16-B
 *                              records): 0 / 11 = chunk 0 staged in a
 *                              line-completing window of 3 to 5 16-B pieces
 *                              (to the end of the 128-B line its third piece
 *                              lies in; default); 1 = 4 pieces (the default
 *                              for chunk pools in mapped host memory,
 *                              ingot_gpu_host_map); 17 = the default window
 *                              with the chunk bounds loaded lazily, per lane,
 *                              only by a walk that leaves chunk 0 or fails
 *                              in it (ingot_gpu_parse_read_first only: one
 *                              descriptor stream for header-split packets;
 *                              elsewhere it means 0).  Field blocks stage 4
 *                              pieces, and ingot_gpu_parse_read_dense always
 *                              stages 4 pieces (the knob is ignored there).
 *                              Other values: EINVAL
 *   INGOT_TUNE_FLOW_KERNEL     ingot_gpu_flow_hist: 0 / 15 = the measured
 *                              default (the only values; EINVAL otherwise):
 *                              offset-addressed device frames with bins <=
 *                              65,536, no full hash, no explicit window and
 *                              not the tunnel chain run k_flows_bits (the
 *                              plain parse's 4-to-5-chunk window, the
 *                              Toeplitz hash bit by bit from the key windows,
 *                              no LDS table); everything else runs k_parse's
 *                              flows mode (LDS table: 16-bit entries one tile
 *                              per wave, 32-bit entries on a persistent grid)
 *   INGOT_TUNE_RING_GRID       ingot_gpu_parse_ring and the multi-tile ring
 *                              kernel (when INGOT_TUNE_PIPELINE is 0):
 *                              256-thread blocks per CU (1..8; 0 = measured
 *                              default, 2).  The tiles in flight per wave
 *                              follow INGOT_TUNE_PIPE_DEPTH
 *   INGOT_TUNE_XCD_REMAP       slot-ring kernels (parse, rewrite) tile order:
 *                              0 = measured default (= 1); 1 = blocks
 *                              renumbered XCD-major (block b runs on XCD b % 8;
 *                              logical block (b % 8) * G/8 + b / 8), so each
 *                              XCD walks a contiguous eighth of every round of
 *                              tiles; 2 = each wave walks a contiguous run of
 *                              tiles instead of striding by the grid; 3 = both;
 *                              4 = hardware order, grid stride; 5 = the batch
 *                              in 8 contiguous regions, one per XCD (parse ring
 *                              only; the rewrite ring takes 0/1/4)
 *   INGOT_TUNE_RING_GROUPS     ingot_gpu_parse_ring: batches in flight at
 *                              once (1, 2 or 4; 0 = measured default): the
 *                              grid is cut into that many block groups, group
 *                              q consuming batches q, q+G, ...
 */
#define INGOT_TUNE_WINDOW_INDEXED 1
#define INGOT_TUNE_WINDOW_STRIDED 2
#define INGOT_TUNE_MAX_BLOCKS 3
#define INGOT_TUNE_PIPELINE 4
#define INGOT_TUNE_CACHE_POLICY 5
#define INGOT_TUNE_PIPE_DEPTH 6
#define INGOT_TUNE_WRITEBACK 7
#define INGOT_TUNE_FLOW_TABLE 8
#define INGOT_TUNE_SLOW_PATH 9
#define INGOT_TUNE_READ_PLAN 10
#define INGOT_TUNE_FLOW_KERNEL 11
#define INGOT_TUNE_RING_GRID 12
#define INGOT_TUNE_RING_GROUPS 13
#define INGOT_TUNE_XCD_REMAP 14
int ingot_gpu_ctx_set_tuning(ingot_gpu_ctx* ctx, int key, int value);
int ingot_gpu_ctx_get_tuning(const ingot_gpu_ctx* ctx, int key);

/*
 * Batched `<Chain>::parse_slice` over frames in a device arena.
 *
 *   d_arena   device pointer to the packet bytes, any alignment (the
 *             kernels align the absolute addresses they stage; they may read
 *             up to 15 bytes before d_arena + d_off[i] and after a frame's
 *             end, never outside that frame's 16-byte blocks)
 *   d_off     per-packet byte offset into d_arena (u64)
 *   d_len     per-packet length in bytes (u16); the caller guarantees every
 *             [d_off[i], d_off[i] + d_len[i]) lies inside its allocation
 *             (ingot's borrowed-slice contract: the kernels read no byte of
 *             a frame past d_len[i] except within its last 16-byte block)
 *   n         number of packets
 *   chain     enum ingot_chain
 *   d_out     n records (device memory, 16 B each)
 *
 * Replaces the caller's per-packet loop over `parse_slice`
 * (ingot-examples/benches/packet.rs:136-172) for the whole batch.
 */
int ingot_gpu_parse(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                    const uint64_t* d_off, const uint16_t* d_len, uint64_t n,
                    int chain, ingot_rec* d_out, void* stream);

/*
 * Same, for fixed-stride arenas (ring buffers with one frame per slot):
 * frame i starts at d_arena + i*stride; its length is d_len[i], or `stride`
 * when d_len is NULL.  stride must be a multiple of 16 and <= 65535 and
 * d_arena 16-byte aligned.  No descriptor bytes are read when d_len is NULL.
 */
int ingot_gpu_parse_strided(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                            uint32_t stride, const uint16_t* d_len, uint64_t n,
                            int chain, ingot_rec* d_out, void* stream);

/* The two batch calls above with 8-byte ingot_rec8 records.  Not for
 * GENEVE_OVER_V6 (EINVAL): the inner offsets do not fit its derivation rules. */
int ingot_gpu_parse_compact(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                            const uint64_t* d_off, const uint16_t* d_len,
                            uint64_t n, int chain, ingot_rec8* d_out,
                            void* stream);
int ingot_gpu_parse_strided_compact(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                                    uint32_t stride, const uint16_t* d_len,
                                    uint64_t n, int chain, ingot_rec8* d_out,
                                    void* stream);

/*
 * Parity mode: every getter of every parsed header (ingot_fields, 256 B per
 * packet).  Same inputs as ingot_gpu_parse; d_off may be NULL to select the
 * strided layout with `stride` (ignored otherwise).
 */
int ingot_gpu_fields(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                     const uint64_t* d_off, const uint16_t* d_len,
                     uint32_t stride, uint64_t n, int chain,
                     ingot_fields* d_out, void* stream);
/* (chain GENEVE_OVER_V6 is EINVAL here: use ingot_gpu_geneve_fields.) */

/*
 * Parity mode for GeneveOverV6Tunnel (384 B per packet): the inner frame's
 * ingot_fields + the outer layers' ingot_tunnel_fields.  Same inputs as
 * ingot_gpu_fields, chain implied.
 */
int ingot_gpu_geneve_fields(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                            const uint64_t* d_off, const uint16_t* d_len,
                            uint32_t stride, uint64_t n,
                            ingot_geneve_fields* d_out, void* stream);

/*
 * Batched `<Chain>::parse_read` (ingot-macros/src/parse.rs:511-537) over
 * multi-chunk packets (mblk_t-style chains) — the `Read` input of
 * ingot-types/src/lib.rs:151-166 as a chunk list:
 *   d_seg_off / d_seg_len  every chunk's device offset into d_arena and length;
 *   d_pkt_seg              n+1 u32 bounds: packet i is chunks
 *                          [d_pkt_seg[i], d_pkt_seg[i+1]) in order.
 * Semantics are parse_read's: a header must lie inside one chunk; a layer
 * that ends its chunk makes the next chunk the slice (none left: TooSmall at
 * that layer, even if the rest was accepted); a header cut by its chunk's end
 * is StraddledHeader when another chunk follows, else TooSmall
 * (error.rs:65-72); no chunks at all is TooSmall at the first label.
 * Record offsets are logical (into the chunks concatenated; a packet's
 * chunks should total <= 65535 B: later bytes are not seen).  d_chunk
 * (optional, n x u16) = index within the packet of the chunk holding the
 * remainder: Parsed::last_chunk is that chunk from payload_off (None when
 * empty), Parsed::data the chunks after it.  No 8-B records or flow mode.
 */
int ingot_gpu_parse_read(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                         const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                         const uint32_t* d_pkt_seg, uint64_t n, int chain,
                         ingot_rec* d_out, uint16_t* d_chunk, void* stream);
/* Parity mode of the same (GENEVE_OVER_V6: EINVAL, use the geneve form). */
int ingot_gpu_fields_read(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                          const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                          const uint32_t* d_pkt_seg, uint64_t n, int chain,
                          ingot_fields* d_out, uint16_t* d_chunk, void* stream);
int ingot_gpu_geneve_fields_read(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                                 const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                 const uint32_t* d_pkt_seg, uint64_t n,
                                 ingot_geneve_fields* d_out, uint16_t* d_chunk,
                                 void* stream);
/*
 * ingot_gpu_parse_read with a dense chunk table: one 8-byte entry per chunk,
 * d_seg[k] = (offset << 16) | length (offset < 2^48), instead of the u64 and
 * u16 arrays — one load per chunk descriptor and no padding between them.
 * fields = 0: d_out holds ingot_rec records; 1: ingot_fields blocks (EINVAL
 * for GENEVE_OVER_V6); 2: ingot_geneve_fields blocks (GENEVE_OVER_V6 only).
 * Staging: chunk 0 in a fixed 4-piece (64-B) window, whatever
 * INGOT_TUNE_READ_PLAN says.
 */
int ingot_gpu_parse_read_dense(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                               const uint64_t* d_seg, const uint32_t* d_pkt_seg,
                               uint64_t n, int chain, int fields, void* d_out,
                               uint16_t* d_chunk, void* stream);

/*
 * ingot_gpu_parse_read with chunk 0 of every packet also given per packet:
 * d_first[i] = (seg_off[pkt_seg[i]] << 16) | seg_len[pkt_seg[i]] (0 for a
 * packet without chunks; offsets < 2^48).  An mblk chain's packet pointer is
 * its first chunk, so a ring of packets naturally carries this; the kernel
 * then loads chunk 0's descriptor beside the packet's chunk bounds instead of
 * after them (one HBM round trip before the staging, not two).  The chunk
 * table is still read for chunks >= 1.  Records and chunk indices are those
 * of ingot_gpu_parse_read over the same chunks (the caller keeps d_first
 * consistent with the table).  16-B records; chunk 0 in the default
 * line-completing 3-5-piece window (INGOT_TUNE_READ_PLAN 1: 4 pieces; 17:
 * the chunk bounds loaded only by walks that leave chunk 0 or fail in it —
 * set it for header-split producers).
 */
int ingot_gpu_parse_read_first(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                               const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                               const uint32_t* d_pkt_seg, const uint64_t* d_first, uint64_t n,
                               int chain, ingot_rec* d_out, uint16_t* d_chunk, void* stream);

/* ---------------------------------------------------------------------------
 * In-place header rewrite: ingot's generated setters (packet/mod.rs:2097-2255;
 * BE bitfield set paths, bitfield.rs:188-315) after the parse, e.g. the
 * reference's `parse-and-decr-v4` bench (ingot-examples/benches/packet.rs:
 * 139-145: l4.set_destination(l4.destination() - 1)).
 *
 * Every packet is parsed as `chain`; for packets that parse Ok the edits are
 * applied in order, each to the header at chain layer `layer` (the label
 * index: UdpParser 0 eth, 1 l3, 2 l4; GenericUlp 0-2; VlanUlp 0 eth, 1 vlan
 * (tag `index`), 2 l3, 3 l4; GeneveOverV6Tunnel 0-6) when that layer holds
 * the header kind the field belongs to (an IPv4 field on an IPv6 layer, or
 * on a layer skipped by an accepting control, is not applied).  Values are
 * the raw wire bits (NetworkRepr::to_network already applied, e.g. Ecn
 * Capable1 = 2); ADD/SUB wrap modulo 2^width; the neighbouring bits of a
 * bitfield are preserved.  Offsets come from the one parse: an edit never
 * re-parses (as in ingot, setting ihl does not move the L4 view).
 * ------------------------------------------------------------------------- */
enum ingot_field {
    INGOT_F_ETH_ETHERTYPE = 0,
    INGOT_F_VLAN_PRIORITY, INGOT_F_VLAN_DEI, INGOT_F_VLAN_VID, INGOT_F_VLAN_ETHERTYPE,
    INGOT_F_V4_VERSION, INGOT_F_V4_IHL, INGOT_F_V4_DSCP, INGOT_F_V4_ECN, INGOT_F_V4_TOTAL_LEN,
    INGOT_F_V4_IDENTIFICATION, INGOT_F_V4_FLAGS, INGOT_F_V4_FRAGMENT_OFFSET,
    INGOT_F_V4_HOP_LIMIT, INGOT_F_V4_PROTOCOL, INGOT_F_V4_CHECKSUM, INGOT_F_V4_SOURCE,
    INGOT_F_V4_DESTINATION,
    INGOT_F_V6_VERSION, INGOT_F_V6_DSCP, INGOT_F_V6_ECN, INGOT_F_V6_FLOW_LABEL,
    INGOT_F_V6_PAYLOAD_LEN, INGOT_F_V6_NEXT_HEADER, INGOT_F_V6_HOP_LIMIT,
    INGOT_F_TCP_SOURCE, INGOT_F_TCP_DESTINATION, INGOT_F_TCP_SEQUENCE,
    INGOT_F_TCP_ACKNOWLEDGEMENT, INGOT_F_TCP_DATA_OFFSET, INGOT_F_TCP_RESERVED,
    INGOT_F_TCP_FLAGS, INGOT_F_TCP_WINDOW_SIZE, INGOT_F_TCP_CHECKSUM, INGOT_F_TCP_URGENT_PTR,
    INGOT_F_UDP_SOURCE, INGOT_F_UDP_DESTINATION, INGOT_F_UDP_LENGTH, INGOT_F_UDP_CHECKSUM,
    INGOT_F_ICMP_TY, INGOT_F_ICMP_CODE, INGOT_F_ICMP_CHECKSUM,
    INGOT_F_GENEVE_VERSION, INGOT_F_GENEVE_OPT_LEN, INGOT_F_GENEVE_FLAGS,
    INGOT_F_GENEVE_PROTOCOL_TYPE, INGOT_F_GENEVE_VNI, INGOT_F_GENEVE_RESERVED,
    INGOT_F_COUNT
};
enum ingot_edit_op {
    INGOT_OP_SET = 0, INGOT_OP_ADD = 1, INGOT_OP_SUB = 2, INGOT_OP_AND = 3, INGOT_OP_OR = 4,
    INGOT_OP_XOR = 5
};
#define INGOT_MAX_EDITS 16

typedef struct ingot_edit {
    uint8_t layer;   /* chain layer index (label) */
    uint8_t field;   /* enum ingot_field */
    uint8_t op;      /* enum ingot_edit_op */
    uint8_t index;   /* VLAN tag (VLAN_ULP's vlan layer), else 0 */
    uint32_t value;  /* raw wire bits */
} ingot_edit;

#ifdef __cplusplus
static_assert(sizeof(ingot_edit) == 8, "ingot_edit is 8 bytes");
#endif

/* Parse + rewrite in place.  `edits` is host memory (<= INGOT_MAX_EDITS);
 * d_out (optional) receives the parse records.  d_off == NULL selects the
 * strided layout (as ingot_gpu_fields). */
int ingot_gpu_parse_modify(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                           const uint64_t* d_off, const uint16_t* d_len,
                           uint32_t stride, uint64_t n, int chain,
                           const ingot_edit* edits, uint32_t n_edits,
                           ingot_rec* d_out, void* stream);

/* ---------------------------------------------------------------------------
 * Batched Emit: ingot's `Emit` (ingot-types/src/emit.rs:8-120; the generated
 * owned `emit_raw`, ingot-macros/src/packet/mod.rs:2097-2255) of one owned
 * header stack per packet, followed by the packet's own bytes — the tuple
 * `(headers, &payload[..])` emitted for every packet of a batch, e.g. OPTE's
 * outbound Geneve encapsulation (outer Ethernet / IPv6 / UDP / Geneve + options
 * in front of the inner frame, ingot-examples/src/packets.rs:27-40).
 *
 * The owned headers are serialised ONCE, on the host, by the caller (ingot's
 * own `(eth, v6, udp, geneve).emit_vec()`, or ingot_amd.emit_headers in the
 * Python mirror): `hdr`, hdr_len <= INGOT_MAX_EMIT_HDR bytes of host memory.
 * The device then writes them in front of every packet and applies the
 * per-packet setters `sets` (<= INGOT_MAX_EMIT_SETS; host memory) to that
 * packet's copy, in order: the field `field` (enum ingot_field) of the header
 * that starts at byte `at` of `hdr` is set (bitfield.rs:188-315 set paths,
 * neighbouring bits kept, big-endian) to
 *   INGOT_EMIT_LENGTH  the packet's emitted bytes from `at` to its end, + add
 *                      (IPv6 payload_len: at = the IPv6 header, add = -40;
 *                      UDP / IPv4 length: add = 0);
 *   INGOT_EMIT_U16     ((const uint16_t*)d_values)[i] + add  (device array);
 *   INGOT_EMIT_U32     ((const uint32_t*)d_values)[i] + add  (device array);
 *   INGOT_EMIT_VALUE   add (the same value for every packet);
 * wrapping modulo 2^width.  The field must lie inside hdr (EINVAL).
 *
 * ingot_gpu_emit_packets: packet i (hdr_len + d_len[i] bytes) is written at
 * d_dst + d_dst_off[i]: the headers, then d_src[d_off[i] .. + d_len[i]).
 * hdr_len 0 is a plain gather-copy (decapsulation: the inner frames at their
 * parsed offsets).  Sources are read in aligned 16-B blocks (the arena must be
 * readable to the 16-B boundary past each packet); destinations are written
 * exactly (packets may be packed back to back); source and destination must
 * not overlap.
 *
 * ingot_gpu_emit_headers: only the header blocks, packet i's at d_out +
 * (d_out_off ? d_out_off[i] : i * out_stride); LENGTH counts hdr_len +
 * d_len[i] (the payload that will follow).  With d_out_off[i] = off[i] -
 * hdr_len into the frames' own arena this is `emit_suffix` into headroom (the
 * packet becomes contiguous in place); into separate slots it is the header
 * chunk of a two-chunk packet that ingot_gpu_parse_read parses as is.
 * hdr_len must be >= 1 here (EINVAL); slots narrower than the block
 * (d_out_off NULL, out_stride < hdr_len) are ERANGE.  Header blocks are
 * written exactly (neighbouring bytes untouched); destinations at any
 * alignment.
 * ------------------------------------------------------------------------- */
enum ingot_emit_source {
    INGOT_EMIT_LENGTH = 0,
    INGOT_EMIT_U16 = 1,
    INGOT_EMIT_U32 = 2,
    INGOT_EMIT_VALUE = 3,
    INGOT_EMIT_BYTES = 4   /* only valid in ingot_emit_set_rows (ingot_gpu_emit_packets_rows) */
};
#define INGOT_MAX_EMIT_SETS 8
#define INGOT_MAX_EMIT_HDR 256

typedef struct ingot_emit_set {
    uint16_t at;           /* byte offset in hdr of the header holding the field */
    uint8_t field;         /* enum ingot_field */
    uint8_t source;        /* enum ingot_emit_source */
    int32_t add;           /* added to the value (VALUE: the value) */
    const void* d_values;  /* U16 / U32: n per-packet values (device memory) */
} ingot_emit_set;

#ifdef __cplusplus
static_assert(sizeof(ingot_emit_set) == 16, "ingot_emit_set is 16 bytes");
#endif

int ingot_gpu_emit_packets(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                           const ingot_emit_set* sets, uint32_t n_sets,
                           const uint8_t* d_src, const uint64_t* d_off,
                           const uint16_t* d_len, uint64_t n, uint8_t* d_dst,
                           const uint64_t* d_dst_off, void* stream);
int ingot_gpu_emit_headers(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                           const ingot_emit_set* sets, uint32_t n_sets,
                           const uint16_t* d_len, uint64_t n, uint8_t* d_out,
                           const uint64_t* d_out_off, uint32_t out_stride, void* stream);

/* ---------------------------------------------------------------------------
 * Emit with checksums: ingot_gpu_emit_packets that also fills the outer IPv4
 * header checksum and / or the outer UDP checksum of every packet it writes,
 * in the same launch (the kernel holds every output byte in registers, so the
 * payload is not read a second time).  One call instead of emit_packets + a
 * UDP_PARSER parse of the result + ingot_gpu_checksum_fill.  Build-defined,
 * like the checksum calls; tests/emit_csum_model.py is the definition.
 *
 * In emit's spirit nothing is derived: the caller names each sum (`sums`,
 * n_sums <= INGOT_MAX_EMIT_SUMS, host memory, at most one of each kind).
 * The emitted bytes are exactly those of ingot_gpu_emit_packets with the same
 * arguments, except the two checksum-field bytes of each named sum, which are
 * computed after all setters of that packet have been applied (a setter that
 * targets a checksum field is overridden).  n_sums == 0 is byte-identical to
 * ingot_gpu_emit_packets.  The IPV4 sum is written before the UDP sum is
 * taken, so a UDP segment that covers the named IPv4 header sums its final
 * bytes.
 *
 *   INGOT_EMIT_SUM_IPV4  the field at `at + 10`: the RFC 1071 checksum of
 *       [at, at + 4 * ihl) of the packet's patched header block, the field
 *       taken as 0; ihl is read from the host block `hdr` at call time.
 *   INGOT_EMIT_SUM_UDP   the field at `at + 6`: the segment is every emitted
 *       byte from `at` to the packet's end, S = hdr_len + d_len[i] - at bytes
 *       (an odd last byte padded with 0, the field taken as 0), plus the
 *       pseudo-header taken from the packet's patched header at `l3_at`
 *       (per-packet address setters are honoured).  The IP version is
 *       hdr[l3_at] >> 4 of the host block: IPv4 = source, destination, 0, 17,
 *       S as 16 bits; IPv6 = source, destination, S as 32 bits, next header
 *       17 (the constant 17 even when extension headers sit between).  A
 *       result of 0 is written as 0xffff (RFC 768).  S > 65535: no such
 *       datagram exists, and the field keeps the bytes the header block and
 *       the setters gave it.
 *
 * EINVAL, besides ingot_gpu_emit_packets's own: n_sums too large or sums NULL
 * with n_sums > 0; an unknown kind, non-zero padding, two sums of one kind; an
 * odd `at` or `l3_at` (every stack ingot can serialise keeps its headers at
 * even offsets); IPV4: l3_at != 0, version nibble != 4, ihl < 5, at + 4 * ihl
 * > hdr_len; UDP: at + 8 > hdr_len, version nibble at l3_at not 4 or 6, the IP
 * header's fixed part (20 / 40 B) not ending at or before `at`; a setter on
 * V4_VERSION, V4_IHL or V6_VERSION of a header that a sum names (the IPV4
 * sum's `at`, the UDP sum's `l3_at`).  So hdr_len == 0 with sums is EINVAL.
 * ERANGE from the LDS-fit check as in ingot_gpu_emit_packets.
 *
 * Out of scope: sums in ingot_gpu_emit_headers (that kernel never sees the
 * payload; the header slot and the source frame are a two-chunk packet, and
 * ingot_gpu_checksum_fill_read fills its outer UDP sum in place); inner-frame checksums (ingot_gpu_checksum_fill on the source
 * arena before the emit); TCP and ICMP kinds.
 * ------------------------------------------------------------------------- */
enum ingot_emit_sum_kind { INGOT_EMIT_SUM_IPV4 = 0, INGOT_EMIT_SUM_UDP = 1 };
#define INGOT_MAX_EMIT_SUMS 2

typedef struct ingot_emit_sum {
    uint16_t at;     /* byte offset in hdr of the header that holds the checksum field */
    uint16_t l3_at;  /* UDP: byte offset in hdr of the IPv4 / IPv6 header whose addresses
                        form the pseudo-header; IPV4: must be 0 */
    uint8_t kind;    /* enum ingot_emit_sum_kind */
    uint8_t _pad[3]; /* must be 0 */
} ingot_emit_sum;

#ifdef __cplusplus
static_assert(sizeof(ingot_emit_sum) == 8, "ingot_emit_sum is 8 bytes");
#endif

int ingot_gpu_emit_packets_csum(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                                const ingot_emit_set* sets, uint32_t n_sets,
                                const ingot_emit_sum* sums, uint32_t n_sums,
                                const uint8_t* d_src, const uint64_t* d_off,
                                const uint16_t* d_len, uint64_t n, uint8_t* d_dst,
                                const uint64_t* d_dst_off, void* stream);

/* ---------------------------------------------------------------------------
 * Emit over chunked packets: ingot_gpu_emit_packets_csum whose source packets
 * are the chunk lists of ingot_gpu_parse_read (an mblk chain, a header-split
 * ring, an ingot_gpu_emit_headers slot in front of its frame).  One launch
 * pulls the chunks up into a contiguous frame (msgpullup), puts the header
 * block in front of it (encapsulation) or cuts the inner frame out of it
 * (decapsulation), and fills the outer sums.  Build-defined;
 * tests/emit_read_model.py is the definition.
 *
 * Payload.  The tables are those of ingot_gpu_parse_read: packet i is the
 * chunks d_pkt_seg[i] .. d_pkt_seg[i+1] of (d_seg_off, d_seg_len), in order,
 * at d_src + d_seg_off[k]; d_pkt_seg[i+1] < d_pkt_seg[i] counts as no chunks.
 * The logical frame is the chunks concatenated and cut at 65,535 bytes (the
 * rule of parse_read and of the _read checksum calls); L is its length.  With
 * f = min(d_from[i], L) and t = min(d_take[i], L - f) (d_from NULL: 0; d_take
 * NULL: L - f), the payload P_i is the logical bytes [f, f + t), and
 * d_taken[i] = t when d_taken is given.  A record's payload_off, or a
 * tunnel's inner Ethernet offset, goes straight into d_from: that is the
 * decapsulation of a chunked tunnel packet.
 *
 * Output.  The bytes written are exactly those ingot_gpu_emit_packets_csum
 * writes with the same hdr, sets, sums and d_dst_off when its source is a
 * linear copy of P_i and d_len[i] = t: the header block, then P_i; the setters
 * in order, INGOT_EMIT_LENGTH counting hdr_len + t; the IPV4 sum before the
 * UDP sum; a UDP result of 0 written as 0xffff; S > 65,535 leaves the field as
 * emitted.  n_sums == 0 is the plain emit, and with hdr_len == 0 the plain
 * pull-up.  Nothing outside [d_dst + d_dst_off[i], + hdr_len + t) is stored
 * to, and every destination byte is stored once (the two checksum-field bytes
 * included: the block that holds them leaves after the sum is known).
 *
 * Reads.  Source reads stay inside the aligned 16-B blocks of non-empty chunks
 * that hold a byte of P_i (the arena must be readable to the 16-B boundaries
 * around each such chunk); an empty chunk's offset is never dereferenced; the
 * chunk descriptors of the packet may all be read.  Source chunks may alias
 * between packets (one payload chunk emitted behind many header chunks).
 * Source and destination must not overlap; destination packets must not
 * overlap.  A packet may have any number of chunks; only the first few are
 * fast.
 *
 * EINVAL: ctx NULL; then ingot_gpu_emit_packets's and
 * ingot_gpu_emit_packets_csum's own checks of hdr, sets and sums, unchanged;
 * then, for n > 0, any of d_src, d_seg_off, d_seg_len, d_pkt_seg, d_dst,
 * d_dst_off NULL.  n == 0 succeeds whatever the device pointers are.  ERANGE
 * from the LDS-fit check as in ingot_gpu_emit_packets.  All of it before any
 * device work.
 *
 * Out of scope: scattering the output into chunks (the destination is
 * contiguous); the dense (offset << 16) | length table and d_first; chunk
 * pools in mapped host memory; TCP / ICMP sum kinds and inner-frame sums
 * (ingot_gpu_checksum_fill_read on the source chunks first).
 * ------------------------------------------------------------------------- */
int ingot_gpu_emit_packets_read(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                                const ingot_emit_set* sets, uint32_t n_sets,
                                const ingot_emit_sum* sums, uint32_t n_sums,
                                const uint8_t* d_src, const uint64_t* d_seg_off,
                                const uint16_t* d_seg_len, const uint32_t* d_pkt_seg,
                                const uint16_t* d_from, const uint16_t* d_take, uint64_t n,
                                uint8_t* d_dst, const uint64_t* d_dst_off, uint16_t* d_taken,
                                void* stream);

/* ---------------------------------------------------------------------------
 * Internet checksums (RFC 1071) of already parsed frames: verify or fill the
 * IPv4 header checksum and the TCP / UDP / ICMPv4 / ICMPv6 checksum of every
 * packet of a batch, on the device.  Build-defined, like the flow hash: ingot
 * has no checksum code and leaves the sums to its caller (OPTE computes them
 * on the CPU, per packet); tests/csum_model.py is the definition.
 *
 * Frames as in ingot_gpu_fields (d_off NULL selects slots of `stride`, a
 * multiple of 16 in a 16-B aligned arena, and d_len NULL then means `stride`;
 * with d_off the arena may have any alignment); reads stay inside each
 * frame's 16-byte blocks.  d_rec holds the 16-B records of an earlier parse
 * of the same frames, under any chain: the layers are taken from the record's
 * l3_kind, l4_kind, l3_off, l4_off, payload_off, l4_proto and n_v6ext (for a
 * GENEVE_OVER_V6 record these are the inner layers; the outer checksums of a
 * tunnel frame come from a UDP_PARSER parse of it).  `what` selects the layers
 * (INGOT_CSUM_L3 | INGOT_CSUM_L4; 0 or any other bit: EINVAL); a layer that
 * is not selected reports NONE and zeros.
 *
 * Only records with status Ok are processed; all others, and records whose
 * offsets do not fit their frame (l3_off + the fixed L3 header <= l4_off,
 * l4_off + the smallest L4 header (TCP 20, UDP 8, ICMP 8) <= payload_off <=
 * the frame length), give NONE / NONE and zeros.
 *   L3   IPv4 only (IPv6 has no header sum: NONE), over the bytes ingot parsed
 *        as the header, max(20, ihl * 4), which must end inside the frame
 *        (else NONE).  OK iff the folded ones'-complement sum including the
 *        field is 0xffff, else BAD; l3_sum is the complement of the sum with
 *        the field taken as 0.
 *   L4   the segment is [l4_off, end), end = l3_off + total_len (IPv4) or
 *        l3_off + 40 + payload_len (IPv6); frame bytes past `end` (Ethernet
 *        padding) are not summed.  In this order:
 *          SHORT     iff end > the frame length or end < payload_off;
 *          FRAGMENT  IPv4: MF set or fragment offset != 0; IPv6: one of the
 *                    n_v6ext extension headers, walked from l3_off + 40 (a
 *                    Fragment header, selected by the value 44, is 8 bytes, any
 *                    other 8 + 8 * its length byte), is a Fragment header with
 *                    offset != 0 or M = 1 (an atomic fragment is summed);
 *          ZERO      verify, UDP only (IPv4 and IPv6 alike): the field is 0.
 *                    l4_sum is still computed; whether a zero sum is allowed
 *                    (RFC 6935) is the caller's decision;
 *          OK / BAD  as for L3, over the pseudo-header and the segment (an odd
 *                    last byte padded with 0).
 *        Pseudo-header: ICMPv4 none; over IPv4 (TCP, UDP; also an ICMPv6
 *        layer) source, destination, 0, the header's protocol byte and the
 *        16-bit segment length; over IPv6 (TCP, UDP, ICMPv6) source,
 *        destination, the 32-bit segment length and rec.l4_proto (RFC 8200
 *        8.1).  l4_sum is the complement of the sum with the field taken as
 *        0, for UDP given as 0xffff when that is 0 (RFC 768); l4_len the
 *        segment's bytes.  SHORT and FRAGMENT rows carry zeros.
 *
 * ingot_gpu_checksum_fill writes exactly the two checksum bytes of every
 * layer that verify would report OK, BAD or ZERO (l3_sum / l4_sum, big-
 * endian) and nothing else, and reports the state after writing (OK) in
 * d_out, which may be NULL.  UDP is always computed.  A caller that fills
 * both levels of a tunnel frame runs the inner call first, then the outer, on
 * one stream.  Frames of one call must not overlap.
 * ------------------------------------------------------------------------- */
enum ingot_csum_state {
    INGOT_CSUM_NONE = 0,     /* nothing to check: record not Ok, no such layer, IPv6 (no header sum) */
    INGOT_CSUM_OK = 1,
    INGOT_CSUM_BAD = 2,
    INGOT_CSUM_ZERO = 3,     /* L4, UDP only: the field is 0, the sender computed none */
    INGOT_CSUM_SHORT = 4,    /* L4: the L3 header's length ends past the frame or inside the L4 header */
    INGOT_CSUM_FRAGMENT = 5  /* L4: the packet is a fragment; not summed */
};
#define INGOT_CSUM_L3 1u
#define INGOT_CSUM_L4 2u

typedef struct ingot_csum {
    uint8_t l3_state;  /* enum ingot_csum_state */
    uint8_t l4_state;
    uint16_t l3_sum;   /* the value the IPv4 checksum field must carry */
    uint16_t l4_sum;   /* the value the L4 checksum field must carry (UDP: 0 is given as 0xffff) */
    uint16_t l4_len;   /* bytes of the L4 segment that were summed */
} ingot_csum;

#ifdef __cplusplus
static_assert(sizeof(ingot_csum) == 8, "ingot_csum is 8 bytes");
#endif

int ingot_gpu_checksum_verify(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                              const uint64_t* d_off, const uint16_t* d_len,
                              uint32_t stride, uint64_t n, const ingot_rec* d_rec,
                              uint32_t what, ingot_csum* d_out, void* stream);
int ingot_gpu_checksum_fill(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                            const uint64_t* d_off, const uint16_t* d_len,
                            uint32_t stride, uint64_t n, const ingot_rec* d_rec,
                            uint32_t what, ingot_csum* d_out, void* stream);

/* ---------------------------------------------------------------------------
 * The two checksum calls over chunked packets: the chunk tables of
 * ingot_gpu_parse_read (packet i is the chunks d_pkt_seg[i] .. d_pkt_seg[i+1]
 * of (d_seg_off, d_seg_len), in order), driven by the 16-B records an earlier
 * ingot_gpu_parse_read (any of its forms) wrote over the same chunks, under
 * any chain.  For a header-split receive ring (headers in one buffer, the
 * payload in another), for the two-chunk packet ingot_gpu_emit_headers makes
 * (header slot + the untouched source frame: the outer UDP sum without
 * copying the payload), and for an inner frame that arrives as a chain.
 * Build-defined, like the contiguous pair; tests/csum_read_model.py is the
 * definition.  `what`, the ingot_csum rows, the states and which of d_out may
 * be NULL are those of ingot_gpu_checksum_verify / _fill.
 *
 * The logical frame is the chunks concatenated, cut at 65,535 bytes
 * (parse_read: later bytes are not seen); L is its length, and
 * d_pkt_seg[i+1] < d_pkt_seg[i] counts as no chunks (L = 0).  A packet's row
 * is the row ingot_gpu_checksum_verify gives for that logical frame with that
 * record, under one added rule: a header is read from one chunk.  "The span
 * [a, b) lies in one chunk" means that some chunk k of the packet has
 * start_k <= a and b <= start_k + len_k, start_k being the logical offset of
 * its first byte.
 *   - Where the contiguous definition requires l3_off + fixed <= L (fixed = 20
 *     for IPv4, 40 for IPv6), [l3_off, l3_off + fixed) must also lie in one
 *     chunk; otherwise the row is NONE / NONE.
 *   - L3: where it requires l3_off + max(20, ihl * 4) <= L, that span must
 *     also lie in one chunk; otherwise L3 is NONE.
 *   - L4: besides the contiguous geometry test, [l3_off, l4_off) (the L3
 *     header as parsed, IPv6 extension headers included: the fragment walk
 *     reads them) must lie in one chunk, and so must [l4_off, payload_off)
 *     (the L4 header as parsed); otherwise L4 is NONE.
 * Every record ingot_gpu_parse_read itself wrote satisfies the rule (ingot
 * parses a header from one slice); the rule decides only what a caller's own
 * or stale records get.  The segment [l4_off, end) itself may cross any
 * number of chunk boundaries, at odd and even offsets, through empty chunks;
 * chunks or bytes past `end` (Ethernet padding, a trailing chunk) are not
 * summed, and end > L is SHORT, as before.  For a GENEVE_OVER_V6 record the
 * layers are the inner ones; the outer UDP sum of a chunked tunnel packet
 * comes from a UDP_PARSER ingot_gpu_parse_read of the same chunks.
 *
 * ingot_gpu_checksum_fill_read writes exactly the two field bytes of every
 * layer verify would call OK, BAD or ZERO (the rule puts them inside one
 * chunk) and nothing else, neither the gaps between chunks nor a chunk's
 * other bytes, and reports the state after writing.  Chunks of different
 * packets may alias for verify; for fill, a chunk that holds a written field
 * must not be shared between packets of one call.  Reads stay inside each
 * non-empty chunk's 16-byte blocks (the contiguous calls' contract, per
 * chunk); an empty chunk's offset is never dereferenced.
 *
 * All argument checks happen before any device work.  EINVAL: a NULL context;
 * `what` 0 or with any other bit; for n > 0 a NULL d_arena, d_rec or any of
 * the three tables; d_out NULL in verify.  n == 0 succeeds.
 *
 * Out of scope: the dense (offset << 16) | length table and the d_first form
 * of parse_read; k_csum itself (the contiguous calls are unchanged).  The
 * chunked emit is ingot_gpu_emit_packets_read.
 * ------------------------------------------------------------------------- */
int ingot_gpu_checksum_verify_read(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                                   const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                   const uint32_t* d_pkt_seg, uint64_t n,
                                   const ingot_rec* d_rec, uint32_t what, ingot_csum* d_out,
                                   void* stream);
int ingot_gpu_checksum_fill_read(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                                 const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                 const uint32_t* d_pkt_seg, uint64_t n,
                                 const ingot_rec* d_rec, uint32_t what, ingot_csum* d_out,
                                 void* stream);

/* ---------------------------------------------------------------------------
 * Parse + rewrite + incremental checksum update (RFC 1624) in one launch: what
 * a forwarding caller does after decrementing a hop limit or translating an
 * address or a port (OPTE updates its sums this way per packet on the CPU).
 * Frames, edits, records and argument checks are exactly those of
 * ingot_gpu_parse_modify.  After the edits of a packet that parsed Ok, the
 * checksums selected by `what` (INGOT_CSUM_L3 | INGOT_CSUM_L4 |
 * INGOT_CSUM_OUTER_L4) are updated from the bytes the edits changed — no
 * payload byte is read.  Build-defined, like ingot_csum;
 * tests/csum_update_model.py is the definition.
 *
 * Words are the big-endian 16-bit words at even frame offsets (every header
 * of every chain starts at an even frame offset).  For a sum whose field holds
 * HC after the edits, D = the sum of (~m + m') mod 0xffff over its covered
 * words, m the word before the call and m' the word after the edits.
 * D == 0 (mod 0xffff): the field is not written (a sum that does not move
 * keeps its representation, also 0xffff).  Otherwise x = (~HC + D) mod 0xffff
 * taken in [1, 0xffff] and HC' = ~x (RFC 1624 eqn. 3).
 *   L3        IPv4 only; covered: the header except its checksum field (at
 *             l3_off + 10).
 *   L4        when l4_kind is TCP, UDP, ICMPv4 or ICMPv6; field at l4_off + 16
 *             (TCP), + 6 (UDP), + 2 (ICMP).  Covered: the fixed L4 header (TCP
 *             20 B, UDP 8 B, ICMP its first 4 B) except the field, and, where
 *             ingot_gpu_checksum_fill sums an IPv4 pseudo-header (not ICMPv4),
 *             the IPv4 source and destination.  Skipped when the IPv4
 *             fragment offset is non-zero after the edits (those bytes are no
 *             L4 header); a first fragment (MF set, offset 0) is updated.
 *             UDP: a field that is 0 after the edits stays 0, and a result of
 *             0 is written as 0xffff.
 *   OUTER_L4  GENEVE_OVER_V6 only (any other chain: EINVAL): outer_udp's
 *             checksum, at its offset + 6.  Covered: every byte from outer_udp
 *             to the frame's end except that field — the Geneve fields, the
 *             inner headers and the inner checksum fields this same call
 *             rewrote (the inner sums are updated first).  The UDP rules apply.
 * An edit whose target is a checksum field itself is applied as written and
 * is left out of that sum's D.  A frame whose sum was wrong stays wrong by the
 * same amount.
 *
 * EINVAL besides ingot_gpu_parse_modify's: what == 0 or any bit above 7, and
 * an edit list that names V4_IHL, V4_TOTAL_LEN, V4_PROTOCOL, V6_PAYLOAD_LEN or
 * V6_NEXT_HEADER: they move a sum's extent or its pseudo-header, so no
 * incremental update exists — rewrite, then ingot_gpu_checksum_fill.
 * ------------------------------------------------------------------------- */
#define INGOT_CSUM_OUTER_L4 4u   /* GENEVE_OVER_V6 only: outer_udp's checksum */
int ingot_gpu_parse_modify_csum(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                                const uint64_t* d_off, const uint16_t* d_len,
                                uint32_t stride, uint64_t n, int chain,
                                const ingot_edit* edits, uint32_t n_edits,
                                uint32_t what, ingot_rec* d_out, void* stream);

/* ---------------------------------------------------------------------------
 * The rewrite with per-packet operands: ingot_gpu_parse_modify (and, with
 * `what`, ingot_gpu_parse_modify_csum) whose edits take their operand from
 * device tables instead of one constant per batch, and which can set the
 * Ethernet and IPv6 addresses (ingot's `set_destination` / `set_source` on
 * Ethernet and Ipv6, ethernet.rs / ip.rs).  A NAT that maps each flow to its
 * own address and port, a next-hop MAC per packet, NAT66, a per-connection
 * TCP sequence offset.  Build-defined; tests/modify_rows_model.py is the
 * definition.
 *
 * Frames, parse, records.  The frames (d_off NULL selects the strided layout),
 * the parse, the records, the layer / kind matching and the order of the edits
 * are ingot_gpu_parse_modify's: only packets that parse Ok are edited, and a
 * later edit sees what earlier ones wrote.  `edits` is host memory
 * (<= INGOT_MAX_EDITS).
 *
 * Fields.  `field` is an ingot_field, or one of the wide fields of
 * ingot_wide_field, which exist only here: the Ethernet destination / source
 * (6 B at header + 0 / + 6; layer 0, and the tunnel chain's inner Ethernet at
 * layer 4) and the IPv6 source / destination (16 B at header + 8 / + 24; the
 * L3 layer when it is IPv6, and the tunnel chain's outer IPv6 at layer 1).
 *
 * Operand of edit k for packet i, by `source`:
 *   INGOT_EDIT_VALUE  `value`, for every packet (ingot_edit's meaning);
 *   otherwise the row index is r = i (INGOT_BY_PACKET) or d_row[i]
 *   (INGOT_BY_ROW) and the row is (const uint8_t*)d_values + r * pitch
 *   (pitch 0: the source's width, i.e. a dense array);
 *   INGOT_EDIT_U16 / _U32  the host-endian integer at the row, zero-extended,
 *       used exactly as `value` would be, with any op, wrapping modulo
 *       2^width;
 *   INGOT_EDIT_BYTES  the field's bytes in wire order (6 or 16) at the row.
 *       BYTES is valid only for wide fields, wide fields take only BYTES, and
 *       wide fields take only INGOT_OP_SET.
 * Several edits may point into one table at different offsets (d_values = the
 * table + the member's offset, pitch = the row size).
 *
 * Row guard.  With d_row given, a packet whose d_row[i] >= n_rows is not
 * touched at all: no edit is applied (not even a VALUE one), no checksum is
 * updated and no table is read for it; its record is still written.
 * INGOT_ROW_NONE is the largest such value, so the d_flow array of
 * ingot_gpu_flow_hist (INGOT_FLOW_NONE for packets that are not counted) can
 * be passed as d_row with a table of `bins` rows.  With d_row NULL no edit may
 * be BY_ROW (EINVAL) and n_rows is ignored.  Table reads are bounded by the
 * row guard alone: a BY_PACKET table holds n rows, a BY_ROW table n_rows.
 *
 * Bytes written: exactly what ingot_gpu_parse_modify writes for the same
 * fields (whole write-back sectors of the staged copy, as there), plus the two
 * bytes of each updated sum.  The tables and d_row are only read; they may be
 * shared between concurrent calls.
 *
 * Checksums.  what == 0: none.  Otherwise `what`, the three sums, RFC 1624
 * eqn. 3, the UDP rules, the later-fragment rule and the refused fields are
 * ingot_gpu_parse_modify_csum's, with these covered ranges in addition:
 *   - the IPv6 source and destination (l3_off + 8 .. + 40) feed the L4 sum
 *     where ingot_gpu_checksum_fill sums an IPv6 pseudo-header (TCP, UDP,
 *     ICMPv6; not ICMPv4);
 *   - in the tunnel chain, the outer IPv6 addresses (layer 1) feed OUTER_L4 as
 *     its pseudo-header, and the inner Ethernet addresses (layer 4) and the
 *     inner IPv6 addresses (layer 5) feed OUTER_L4 as covered bytes;
 *   - Ethernet addresses at layer 0 feed nothing.
 *
 * EINVAL, all checked before any device work, in this order:
 *   1. ingot_gpu_parse_modify's own checks (ctx, chain, n_edits >
 *      INGOT_MAX_EDITS, a NULL list);
 *   2. per edit: an unknown field or op, or a layer out of range; a bad
 *      `source` or `by`; non-zero `_pad`; non-zero `value` with a table
 *      source; NULL d_values with a table source; BYTES on a narrow field, or
 *      another source on a wide field; a wide field with an op other than SET;
 *      `pitch` non-zero and below the source's width; U16 / U32 with d_values
 *      or pitch not a multiple of 2 / 4; BY_ROW without d_row;
 *   3. `what`: bits above 7, or OUTER_L4 outside the tunnel chain; with
 *      what != 0, the refused fields;
 *   4. n == 0 succeeds;
 *   5. a NULL arena, the slots' stride / alignment rules, d_off without d_len.
 *
 * Out of scope: the slot-ring kernel (slots >= 64 B without a length array
 * run the plain per-tile kernel here, whatever INGOT_TUNE_PIPELINE says); ops
 * other than SET on wide fields; wide fields in ingot_edit (the emit takes them
 * in ingot_gpu_emit_packets_rows, the chunked rewrite in
 * ingot_gpu_parse_read_modify_rows, both below).
 * ------------------------------------------------------------------------- */
enum ingot_wide_field {            /* only valid in ingot_edit_rows.field */
    INGOT_FW_ETH_DESTINATION = 64, /* ethernet.rs, 6 B at +0  */
    INGOT_FW_ETH_SOURCE      = 65, /* 6 B at +6  */
    INGOT_FW_V6_SOURCE       = 66, /* ip.rs Ipv6, 16 B at +8  */
    INGOT_FW_V6_DESTINATION  = 67  /* 16 B at +24 */
};
enum ingot_edit_source {
    INGOT_EDIT_VALUE = 0, INGOT_EDIT_U16 = 1, INGOT_EDIT_U32 = 2, INGOT_EDIT_BYTES = 3
};
enum ingot_edit_by { INGOT_BY_PACKET = 0, INGOT_BY_ROW = 1 };
#define INGOT_ROW_NONE 0xffffffffu

typedef struct ingot_edit_rows {
    uint8_t layer;         /* as ingot_edit */
    uint8_t field;         /* enum ingot_field or enum ingot_wide_field */
    uint8_t op;            /* enum ingot_edit_op */
    uint8_t index;         /* as ingot_edit */
    uint32_t value;        /* VALUE: the operand; otherwise must be 0 */
    uint8_t source;        /* enum ingot_edit_source */
    uint8_t by;            /* enum ingot_edit_by */
    uint16_t _pad;         /* must be 0 */
    uint32_t pitch;        /* bytes between rows; 0 = the source's width */
    const void* d_values;  /* device memory; NULL only for VALUE */
} ingot_edit_rows;

#ifdef __cplusplus
static_assert(sizeof(ingot_edit_rows) == 24, "ingot_edit_rows is 24 bytes");
#endif

int ingot_gpu_parse_modify_rows(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                                const uint64_t* d_off, const uint16_t* d_len,
                                uint32_t stride, uint64_t n, int chain,
                                const ingot_edit_rows* edits, uint32_t n_edits,
                                const uint32_t* d_row, uint32_t n_rows,
                                uint32_t what, ingot_rec* d_out, void* stream);

/* ---------------------------------------------------------------------------
 * Emit with per-packet and per-row header operands: ingot_gpu_emit_packets_csum
 * whose setters take the operand forms of ingot_gpu_parse_modify_rows, the
 * Ethernet and IPv6 addresses included.  One launch encapsulates every packet
 * towards its own flow's endpoint (OPTE's outbound Geneve-over-IPv6: the outer
 * IPv6 destination, the next-hop MAC and the VNI of the mapping the flow
 * resolved to) and fills the outer sums over those per-packet bytes.
 * Build-defined; tests/emit_rows_model.py is the definition.
 *
 * Frames, header block, sums.  The frames, the header block `hdr`, the LENGTH
 * and VALUE sources, the sums (n_sums == 0: none), the source reads, the
 * destination writes, the alignment rules and the LDS-fit ERANGE are exactly
 * ingot_gpu_emit_packets_csum's.  `sets` is host memory
 * (<= INGOT_MAX_EMIT_SETS; a wide field counts as one).
 *
 * Fields.  `field` is an ingot_field, or one of ingot_wide_field: for the
 * header at `at`, the Ethernet destination / source (6 B at at + 0 / at + 6)
 * or the IPv6 source / destination (16 B at at + 8 / at + 24).  As for narrow
 * fields nothing is derived: the caller names `at`, and the field must lie
 * inside hdr.  Wide fields take only INGOT_EMIT_BYTES, and BYTES is valid only
 * for them.
 *
 * Operand of set k for packet i, by `source`:
 *   INGOT_EMIT_LENGTH / _VALUE  as in ingot_emit_set;
 *   otherwise the row index is r = i (INGOT_BY_PACKET) or d_row[i]
 *   (INGOT_BY_ROW) and the row is (const uint8_t*)d_values + r * pitch
 *   (pitch 0: the source's width, i.e. a dense array; the product is taken in
 *   64 bits);
 *   INGOT_EMIT_U16 / _U32  the host-endian integer at the row, + add, modulo
 *       2^width;
 *   INGOT_EMIT_BYTES  the field's 6 or 16 bytes in wire order at the row, at
 *       any address.
 * Several sets may point into one table at different offsets (d_values = the
 * table + the member's offset, pitch = the row size).
 *
 * Order.  The setters apply in list order to the packet's copy of the block: a
 * later set overwrites what an earlier one wrote, and a wide and a narrow set
 * may overlap.  The sums are taken after all setters, so the UDP pseudo-header
 * sees the per-packet addresses.
 *
 * Row guard.  With d_row given, a packet whose d_row[i] >= n_rows is not
 * emitted: no byte is stored at or around d_dst + d_dst_off[i], no source byte
 * and no table is read for it (INGOT_ROW_NONE is the largest such value, so the
 * d_flow array of ingot_gpu_flow_hist can be passed as d_row with a table of
 * `bins` rows).  This is the emit's form of the rewrite's "not touched at
 * all": a flow without a mapping goes to the slow path, it is not
 * encapsulated towards a made-up endpoint.  With d_row NULL no set may be
 * BY_ROW (EINVAL) and n_rows is ignored.  Table reads are bounded by the row
 * guard alone: a BY_PACKET table holds n rows, a BY_ROW table n_rows.
 *
 * Equivalence.  For every emitted packet the bytes are those
 * ingot_gpu_emit_packets_csum writes for that packet alone when each table set
 * is replaced by a VALUE set of the row's value and each BYTES set's row is
 * pasted into hdr at its place in list order.  With no BYTES set, no BY_ROW
 * set and d_row NULL, the output is byte-identical to
 * ingot_gpu_emit_packets_csum with the same sets and sums.
 *
 * EINVAL, all checked before any device work, in this order:
 *   1. ctx NULL;
 *   2. ingot_gpu_emit_packets's checks of hdr / hdr_len / n_sets / NULL sets;
 *   3. per set, in list order: a field that is neither an ingot_field nor a
 *      wide field; source > INGOT_EMIT_BYTES; non-zero `_pad`; by >
 *      INGOT_BY_ROW; BYTES on a narrow field, or another source on a wide
 *      field; LENGTH / VALUE with `by`, `pitch` or `d_values` non-zero; a table
 *      source with NULL d_values; BYTES with add != 0; `pitch` non-zero and
 *      below the source's width; U16 / U32 with d_values or pitch not a
 *      multiple of 2 / 4; BY_ROW without d_row; a field not inside hdr;
 *   4. ingot_gpu_emit_packets_csum's checks of `sums`, unchanged (the version /
 *      ihl setter rule applies to the narrow sets);
 *   5. n == 0 succeeds;
 *   6. any of d_src, d_off, d_len, d_dst, d_dst_off NULL;
 *   7. then ERANGE from the LDS-fit check.
 *
 * Out of scope: the header-block-only form (ingot_gpu_emit_headers) takes no
 * tables (the chunked form with tables is ingot_gpu_emit_packets_read_rows);
 * wide fields in ingot_emit_set and ingot_edit; a per-packet "emitted" flag
 * (the caller has d_row).
 * ------------------------------------------------------------------------- */
typedef struct ingot_emit_set_rows {
    uint16_t at;           /* as ingot_emit_set */
    uint8_t  field;        /* enum ingot_field or enum ingot_wide_field */
    uint8_t  source;       /* enum ingot_emit_source, incl. INGOT_EMIT_BYTES */
    int32_t  add;          /* as ingot_emit_set; must be 0 for BYTES */
    uint8_t  by;           /* enum ingot_edit_by; must be 0 for LENGTH / VALUE */
    uint8_t  _pad[3];      /* must be 0 */
    uint32_t pitch;        /* bytes between rows; 0 = the source's width */
    const void* d_values;  /* device memory; must be NULL for LENGTH / VALUE */
} ingot_emit_set_rows;

#ifdef __cplusplus
static_assert(sizeof(ingot_emit_set_rows) == 24, "ingot_emit_set_rows is 24 bytes");
#endif

int ingot_gpu_emit_packets_rows(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                                const ingot_emit_set_rows* sets, uint32_t n_sets,
                                const ingot_emit_sum* sums, uint32_t n_sums,
                                const uint32_t* d_row, uint32_t n_rows,
                                const uint8_t* d_src, const uint64_t* d_off,
                                const uint16_t* d_len, uint64_t n, uint8_t* d_dst,
                                const uint64_t* d_dst_off, void* stream);

/* ---------------------------------------------------------------------------
 * The rewrite over chunked packets: ingot_gpu_parse_read, then ingot's setters
 * in place over the chunk lists, and (_csum) the RFC 1624 update of the
 * selected sums in the same launch.  For packets held as an mblk chain or in
 * a header-split ring, and for the two-chunk packet ingot_gpu_emit_headers
 * makes (header slot + the untouched source frame): hop limit, NAT of an
 * address or a port, a VNI, with the sums kept right and no payload byte
 * read or copied.  tests/modify_read_model.py is the definition.
 *
 * Tables and records.  (d_seg_off, d_seg_len, d_pkt_seg) are the CSR tables of
 * ingot_gpu_parse_read.  d_out and d_chunk are both optional; whatever is
 * written to them is byte for byte what ingot_gpu_parse_read writes for the
 * same tables and bytes: the parse sees the bytes before the edits.
 *
 * Where edits land.  Only packets whose record is Ok are edited; every other
 * packet (StraddledHeader, TooSmall, no chunks, ...) has no byte written.  For
 * an Ok packet the edits are ingot_gpu_parse_modify's, in order: the same
 * layer / field / kind matching, ops wrapping modulo 2^width, neighbouring
 * bits preserved, raw wire values; a later edit sees what the earlier ones
 * wrote.  Offsets come from this one parse and are the record's logical
 * offsets (the chunks concatenated): the tunnel chain's outer offsets from
 * the walk, VLAN tag `index` at 14 + 4 * index.  Logical byte x of a packet
 * lives in the chunk k with start_k <= x < start_k + len_k, start_k the sum of
 * the earlier chunks' lengths; an empty chunk holds no byte and its offset is
 * never dereferenced.  Every header parse_read accepted lies in one chunk, so
 * each edited field and each checksum field lies in one chunk.
 *
 * Checksum update.  `what`, the sums, their covered bytes, the EINVAL rules
 * and the refused fields are ingot_gpu_parse_modify_csum's.  Its "even frame
 * offsets" are even logical offsets: a byte's place in its 16-bit word is the
 * parity of its logical offset, whatever the chunk's address.  Inner sums come
 * first, then OUTER_L4 (tunnel chain only).
 *
 * Bytes written: exactly the covering bytes of each applied edit and the two
 * bytes of each updated checksum field, each stored as a byte.  Gaps between
 * chunks, other packets' chunks and payload chunks are not stored to at all.
 *
 * Aliasing: a chunk that holds a header the call may write must not be shared
 * between packets of one call; chunks that are only parsed past (payload) may.
 *
 * All argument checks happen before any device work: ingot_gpu_parse_modify's
 * (_csum: and ingot_gpu_parse_modify_csum's) own, then n == 0 succeeds, then
 * for n > 0 a NULL d_arena or any NULL table is EINVAL.  Results never depend
 * on tuning knobs; INGOT_TUNE_READ_PLAN 1 is honoured as in
 * ingot_gpu_parse_read (17 means 0).
 *
 * Out of scope: the dense table and the d_first / lazy forms of parse_read.
 * ------------------------------------------------------------------------- */
int ingot_gpu_parse_read_modify(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                                const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                const uint32_t* d_pkt_seg, uint64_t n, int chain,
                                const ingot_edit* edits, uint32_t n_edits,
                                ingot_rec* d_out, uint16_t* d_chunk, void* stream);
int ingot_gpu_parse_read_modify_csum(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                                     const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                     const uint32_t* d_pkt_seg, uint64_t n, int chain,
                                     const ingot_edit* edits, uint32_t n_edits,
                                     uint32_t what, ingot_rec* d_out, uint16_t* d_chunk,
                                     void* stream);

/* ---------------------------------------------------------------------------
 * The rewrite over chunked packets with per-packet operands and the address
 * setters: ingot_gpu_parse_read_modify_csum's chunk lists with
 * ingot_gpu_parse_modify_rows' edits.  A NAT address, a next-hop MAC or a
 * tunnel endpoint per flow for packets held as an mblk chain or in a
 * header-split ring, without pulling them up; and, after
 * ingot_gpu_emit_headers, the outer IPv6 destination, MAC and VNI per row over
 * the header slot + the untouched source frame, with the outer UDP sum updated
 * in place.  No new struct or enum: ingot_edit_rows, ingot_wide_field,
 * ingot_edit_source, ingot_edit_by and INGOT_ROW_NONE are
 * ingot_gpu_parse_modify_rows'.  Build-defined;
 * tests/modify_read_rows_model.py is the definition.
 *
 * Tables, parse, records, d_chunk are ingot_gpu_parse_read_modify's: the CSR
 * tables of ingot_gpu_parse_read; d_out and d_chunk are both optional and get,
 * byte for byte, what ingot_gpu_parse_read writes; the parse sees the bytes
 * before the edits.
 *
 * Edits.  Fields (the wide ones too), sources, `by`, pitch, ops and order are
 * ingot_gpu_parse_modify_rows'; they are applied to packets whose record is Ok
 * at the record's logical offsets (the chunks concatenated), as
 * ingot_gpu_parse_read_modify applies them.  A wide field lies inside its
 * header and every header parse_read accepted lies in one chunk, so each wide
 * field lies in one chunk.
 *
 * Row guard.  With d_row given, a packet whose d_row[i] >= n_rows has no byte
 * written and no table read; its record and chunk index are still written.
 * With d_row NULL no edit may be BY_ROW (EINVAL) and n_rows is ignored.
 *
 * Checksums.  what == 0: none.  Otherwise the sums, their covered ranges (the
 * IPv6 pseudo-header and the tunnel chain's ranges included), the UDP rules
 * and the refused fields are ingot_gpu_parse_modify_rows'.  A byte's place in
 * its 16-bit word is the parity of its logical offset, and inner sums come
 * before OUTER_L4, as in ingot_gpu_parse_read_modify_csum.
 *
 * Bytes written: exactly the covering bytes of each applied edit and the two
 * bytes of each updated sum.  A store may be 1, 2 or 4 bytes wide and never
 * covers a byte outside the field it writes.  Gaps between chunks, other
 * packets' chunks and payload chunks are not stored to at all.
 *
 * Aliasing: ingot_gpu_parse_read_modify's rule.  The tables and d_row are only
 * read; they may be shared between concurrent calls.
 *
 * EINVAL, all checked before any device work, in this order:
 *   1. checks 1 to 3 of ingot_gpu_parse_modify_rows (ctx, chain, the list; per
 *      edit; `what`);
 *   2. n == 0 succeeds;
 *   3. a NULL d_arena or any NULL chunk table.
 *
 * Results never depend on tuning knobs; INGOT_TUNE_READ_PLAN 1 and an arena in
 * mapped host memory select the 4-piece window, as in
 * ingot_gpu_parse_read_modify.
 *
 * Out of scope: the dense (offset << 16) | length table; the d_first and lazy
 * forms of parse_read; ops other than SET on wide fields; the C++ mirror
 * (ingot_amd.hpp).
 * ------------------------------------------------------------------------- */
int ingot_gpu_parse_read_modify_rows(ingot_gpu_ctx* ctx, uint8_t* d_arena,
                                     const uint64_t* d_seg_off, const uint16_t* d_seg_len,
                                     const uint32_t* d_pkt_seg, uint64_t n, int chain,
                                     const ingot_edit_rows* edits, uint32_t n_edits,
                                     const uint32_t* d_row, uint32_t n_rows,
                                     uint32_t what, ingot_rec* d_out, uint16_t* d_chunk,
                                     void* stream);

/* ---------------------------------------------------------------------------
 * Emit over chunked packets with per-packet and per-row header operands:
 * ingot_gpu_emit_packets_read's chunk lists with ingot_gpu_emit_packets_rows'
 * setters.  One launch pulls an mblk chain or a header-split packet up,
 * encapsulates it towards its own flow's endpoint (outer IPv6 destination,
 * next-hop MAC and VNI from the row the flow resolved to), fills the outer
 * sums over those bytes, and leaves a packet whose flow has no mapping
 * un-emitted.  Inbound, with d_from the inner L3 offset of a chunked tunnel
 * packet and hdr a 14-byte Ethernet header whose MACs are BY_ROW, it cuts the
 * inner packet out and puts the flow's own Ethernet header in front of it.
 * No new struct or enum: ingot_emit_set_rows, ingot_emit_sum, ingot_wide_field,
 * ingot_edit_by and INGOT_ROW_NONE are ingot_gpu_emit_packets_rows'.
 * Build-defined; tests/emit_read_rows_model.py is the definition.
 *
 * Payload, reads, cut.  The tables (d_src, d_seg_off, d_seg_len, d_pkt_seg),
 * d_from / d_take and their clamps, the cut at 65,535 logical bytes, d_taken,
 * the 16-B read contract, the never-dereferenced offset of an empty chunk, the
 * aliasing and overlap rules are exactly ingot_gpu_emit_packets_read's; P_i
 * and t are its payload and its length.
 *
 * Setters, operands, order, sums, row guard.  `sets`, the fields (the wide ones
 * too), the operand of set k for packet i, `by`, pitch, the list order, the
 * sums taken after all setters and the bounds of the table reads are exactly
 * ingot_gpu_emit_packets_rows'.  INGOT_EMIT_LENGTH counts hdr_len + t.
 *
 * Equivalence, which is the definition.  For every emitted packet the bytes
 * are those ingot_gpu_emit_packets_rows writes with the same hdr, sets, sums,
 * d_row, n_rows and d_dst_off when its source is a linear copy of P_i and
 * d_len[i] = t.  With no BYTES set, no BY_ROW set and d_row NULL, the
 * destination and d_taken are byte-identical to ingot_gpu_emit_packets_read
 * with the same sets and sums.  Every destination byte is stored once, and
 * nothing outside [d_dst + d_dst_off[i], + hdr_len + t) is stored to.
 *
 * Guarded packet (d_row given and d_row[i] >= n_rows).  No byte at or around
 * d_dst + d_dst_off[i] is stored; no source byte, no table and no entry of
 * d_seg_off / d_seg_len is read for it (its chunk bounds may be garbage); its
 * d_pkt_seg, d_from, d_take and d_dst_off entries may be read;
 * d_taken[i] = 0 when d_taken is given.  With d_row NULL no set may be BY_ROW
 * (EINVAL) and n_rows is ignored.
 *
 * EINVAL, all checked before any device work, in this order:
 *   1. ctx NULL;
 *   2. checks 2 to 4 of ingot_gpu_emit_packets_rows (hdr / hdr_len / n_sets /
 *      NULL sets; per set, in list order; the sums), unchanged;
 *   3. n == 0 succeeds whatever the device pointers are;
 *   4. d_dst or d_dst_off NULL;
 *   5. any of d_src, d_seg_off, d_seg_len, d_pkt_seg NULL;
 *   6. then ERANGE from the LDS-fit check.
 *
 * Out of scope: tables in ingot_gpu_emit_headers; scattering the output into
 * chunks; the dense (offset << 16) | length table and d_first; TCP / ICMP sum
 * kinds and inner-frame sums; the C++ mirror (ingot_amd.hpp).
 * ------------------------------------------------------------------------- */
int ingot_gpu_emit_packets_read_rows(ingot_gpu_ctx* ctx, const uint8_t* hdr, uint32_t hdr_len,
                                     const ingot_emit_set_rows* sets, uint32_t n_sets,
                                     const ingot_emit_sum* sums, uint32_t n_sums,
                                     const uint32_t* d_row, uint32_t n_rows,
                                     const uint8_t* d_src, const uint64_t* d_seg_off,
                                     const uint16_t* d_seg_len, const uint32_t* d_pkt_seg,
                                     const uint16_t* d_from, const uint16_t* d_take, uint64_t n,
                                     uint8_t* d_dst, const uint64_t* d_dst_off, uint16_t* d_taken,
                                     void* stream);

/*
 * Flow classification + per-flow histogram (config 5; build-defined, ingot
 * has no flow hash).  For every packet that parses Ok as `chain` with an
 * IPv4/IPv6 layer, the RSS Toeplitz hash of
 *     source addr | destination addr | (source port | destination port)
 * (ports only when the L4 layer is TCP or UDP; network byte order, the
 * Microsoft RSS input order) with the 40-byte `key` (host memory; NULL =
 * the standard Microsoft RSS key).  Outputs:
 *   d_flow  (required, n x u32)  the packet's flow bin hash & (bins - 1), or
 *           INGOT_FLOW_NONE for packets that are not counted;
 *   d_hash  (optional, n x u32)  the full hash, 0 when not counted;
 *   d_hist  (optional, bins x u32) d_hist[bin] += 1 per counted packet —
 *           accumulated into (zero it to start a new histogram).
 * bins is a power of two <= 2^24.  d_off == NULL selects the strided layout
 * (as ingot_gpu_fields).  Two launches: parse + hash, then a contention-free
 * histogram pass over d_flow (LDS-privatised counters).
 *
 * ingot_gpu_flow_hist_ws: the same with a caller-owned device workspace
 * (d_work, work_bytes >= ingot_gpu_flow_hist_workspace_size(n, bins), e.g.
 * 16 MiB for 8 M packets x 65,536 bins): the histogram pass then stores
 * per-block counters there and reduces them without atomics (faster; see
 * DESIGN.md).  Size 0 = no workspace is used for (n, bins); a smaller or NULL
 * workspace falls back to the atomic pass.  Like the arena, the workspace is
 * borrowed for the call: calls that run concurrently need their own.
 */
#define INGOT_FLOW_KEY_BYTES 40
#define INGOT_FLOW_NONE 0xffffffffu
int ingot_gpu_flow_hist(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                        const uint64_t* d_off, const uint16_t* d_len,
                        uint32_t stride, uint64_t n, int chain,
                        const uint8_t* key, uint32_t bins, uint32_t* d_flow,
                        uint32_t* d_hash, uint32_t* d_hist, void* stream);
int ingot_gpu_flow_hist_ws(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                           const uint64_t* d_off, const uint16_t* d_len,
                           uint32_t stride, uint64_t n, int chain,
                           const uint8_t* key, uint32_t bins, uint32_t* d_flow,
                           uint32_t* d_hash, uint32_t* d_hist, void* d_work,
                           size_t work_bytes, void* stream);
size_t ingot_gpu_flow_hist_workspace_size(uint64_t n, uint32_t bins);

/* ---------------------------------------------------------------------------
 * Exact-match flow table, host side: the 40-byte per-packet flow key and a
 * table from keys to action-table rows (build-defined, like the flow hash:
 * ingot has no flow table; tests/flow_lookup_model.py is the definition of the
 * key and of the lookup).  ingot_gpu_flow_hist's bins collide, so two flows in
 * one bin share a row of a bins-row table; an exact-match table gives every
 * flow its own row for ingot_gpu_parse_modify_rows (d_row, n_rows = the action
 * table's size).  This is the host half: the key, the table's layout and hash,
 * build / insert / find.  The device calls that fill d_row from it are not in
 * the library yet.
 *
 * The key, 40 bytes.  w[0..8] are the nine words ingot_gpu_flow_hist hashes:
 * source address, destination address, then the L4 header's first word
 * (source port | destination port) when the L4 layer is TCP or UDP, else 0;
 * IPv4 fills words 0-2, IPv6 words 0-8, the rest are zero.  Each word is the
 * host-endian value of the big-endian read (10.0.0.1 is 0x0a000001).
 * w[9] = (l3_kind << 8) | l4_proto; its upper 16 bits are zero (reserved).
 * A packet has a key exactly when ingot_gpu_flow_hist counts it: its record
 * is Ok and l3_kind != NONE; the layers are the ones the record describes
 * (the tunnel chain's inner layers once INGOT_REC_INNER is set).  A packet
 * without a key has 40 zero bytes: w[9] == 0 belongs to no key, and marks an
 * empty slot of the table.
 *
 * The table (host side: no context, no GPU).  A caller-owned buffer of
 * ingot_gpu_flow_table_bytes(slots) = 64 * (slots + 1) bytes, `slots` a power
 * of two in [MIN_SLOTS, MAX_SLOTS] (0 for any other `slots`); the layout is
 * opaque.  Open addressing, linear probing from
 * ingot_gpu_flow_key_hash(key) & (slots - 1), wrapping.
 *   _build   zeroes the buffer, then inserts keys[i] -> rows[i] in order
 *            (n_keys may be 0; keys / rows may then be NULL).
 *   _insert  one key on a host copy: a key already present has its row
 *            replaced (the last one wins, the count stays).  INGOT_GPU_ERANGE,
 *            the table left as it was, when the count would exceed slots / 2
 *            or the key would land MAX_PROBE or more slots from its home:
 *            double `slots` and rebuild.  (_build stops at the first such key.)
 *   _find    the key's row, or INGOT_ROW_NONE (also for any bad argument); at
 *            most MAX_PROBE slots are probed, stopping at an empty one.
 *   _key_hash  the hash (0 for NULL), so hosts can reason about home slots.
 * INGOT_GPU_EINVAL: `slots` not a power of two in range; table_bytes !=
 * 64 * (slots + 1); a NULL table, or NULL key / keys / rows where one is
 * needed; a key whose w[9] >> 8 is not 1 or 2 (upper bits non-zero included);
 * a row equal to INGOT_ROW_NONE; _insert / _find on a buffer whose header
 * does not match table_bytes.
 * The buffer is made to be uploaded whole to 64-B-aligned device memory: one
 * slot is one aligned 64-B read.
 *
 * Out of scope: the device-side key extraction and lookup (see above);
 * removal (rebuild the table); a VNI-qualified key (w[9]'s upper bits are
 * reserved for it); the C++ mirror ingot_amd.hpp.
 * ------------------------------------------------------------------------- */
typedef struct ingot_flow_key { uint32_t w[10]; } ingot_flow_key;

#ifdef __cplusplus
static_assert(sizeof(ingot_flow_key) == 40, "ingot_flow_key is 40 bytes");
#endif

#define INGOT_FLOW_TABLE_MIN_SLOTS 16u
#define INGOT_FLOW_TABLE_MAX_SLOTS (1u << 26)
#define INGOT_FLOW_TABLE_MAX_PROBE 128u
size_t ingot_gpu_flow_table_bytes(uint32_t slots);
int ingot_gpu_flow_table_build(const ingot_flow_key* keys, const uint32_t* rows,
                               uint32_t n_keys, uint32_t slots, void* table,
                               size_t table_bytes);
int ingot_gpu_flow_table_insert(void* table, size_t table_bytes,
                                const ingot_flow_key* key, uint32_t row);
uint32_t ingot_gpu_flow_table_find(const void* table, size_t table_bytes,
                                   const ingot_flow_key* key);
uint32_t ingot_gpu_flow_key_hash(const ingot_flow_key* key);

/*
 * The multi-GPU reduce of config 5 (the only collective of the design).
 * Packets shard across GPUs by contiguous index ranges with no exchange;
 * each rank's ingot_gpu_flow_hist leaves a per-rank histogram, and the job's
 * histogram is their element-wise sum: RCCL all-reduce (sum, uint32) over
 * xGMI, 65,536 x u32 = 256 KiB at the default bins.
 *
 * One process (or thread) per GPU.  Rank 0 makes a communicator id with
 * ingot_gpu_comm_unique_id and the host sends its INGOT_COMM_ID_BYTES bytes to
 * every rank over its own control channel; every rank then calls
 * ingot_gpu_comm_create with the same id, nranks and its own rank (this
 * blocks until all ranks have joined).  The communicator is bound to ctx's
 * device.  RCCL is loaded at the first call of these functions (librccl.so.1,
 * the one already in the process if there is one); INGOT_GPU_ENODEV if it
 * cannot be loaded, INGOT_GPU_ECOMM if an RCCL call fails.
 *
 * ingot_gpu_flow_hist_allreduce enqueues the in-place sum of d_hist (bins x
 * u32, device memory of the communicator's device) across all ranks on
 * `stream`, ordered after the work already enqueued there (e.g. the
 * ingot_gpu_flow_hist that filled it) and before what follows; every rank
 * must enqueue the same sequence of reduces.  The counts wrap modulo 2^32.
 *
 * Release: ingot_gpu_comm_destroy on every rank flushes the reduces issued,
 * waits until the communicator is quiescent on all ranks (ncclCommFinalize)
 * and frees it; ingot_gpu_comm_abort frees it at once, locally, aborting any
 * reduce still in flight (error paths, or a process that is exiting after its
 * streams have drained).  Either way the handle is gone afterwards.
 *
 * A host that already holds an RCCL communicator over the same ranks (its
 * own, or PyTorch's ProcessGroupNCCL) hands it over with ingot_gpu_comm_wrap
 * instead of creating a second one: one RCCL communicator per process is the
 * layout that ran clean (with two per process the world-2
 * rehearsal stalled).  `nccl_comm` is an ncclComm_t of the process's
 * librccl.so.1; the handle borrows it: size and rank are the communicator's,
 * its device must be ctx's (else INGOT_GPU_EINVAL), and
 * ingot_gpu_comm_destroy / _abort free only the handle — the borrowed
 * communicator stays the host's and must outlive the handle.
 */
#define INGOT_GPU_ECOMM (-6)    /* a collective (RCCL) call failed */
#define INGOT_COMM_ID_BYTES 128
typedef struct ingot_gpu_comm ingot_gpu_comm;
int ingot_gpu_comm_unique_id(uint8_t id[INGOT_COMM_ID_BYTES]);
int ingot_gpu_comm_create(ingot_gpu_ctx* ctx, int nranks, int rank,
                          const uint8_t id[INGOT_COMM_ID_BYTES], ingot_gpu_comm** out);
int ingot_gpu_comm_wrap(ingot_gpu_ctx* ctx, void* nccl_comm, ingot_gpu_comm** out);
int ingot_gpu_comm_destroy(ingot_gpu_comm* comm);
int ingot_gpu_comm_abort(ingot_gpu_comm* comm);
int ingot_gpu_comm_size(const ingot_gpu_comm* comm);
int ingot_gpu_comm_rank(const ingot_gpu_comm* comm);
int ingot_gpu_flow_hist_allreduce(ingot_gpu_comm* comm, uint32_t* d_hist, uint32_t bins,
                                  void* stream);

/* ---------------------------------------------------------------------------
 * Frames stored back to back with only a length array (a capture buffer, a
 * ring without a descriptor table): frame i starts at d_arena + the sum of
 * d_len[0..i).  The offsets are derived on the device — a base per
 * 64-packet tile from a scan of tile sums (two small passes over the lengths,
 * into the caller's workspace d_work of >= ingot_gpu_packed_workspace_size(n)
 * bytes, 8-B aligned), then a wavefront prefix scan of each tile's lengths
 * inside the parse — and the batch is parsed as by ingot_gpu_parse.  2 B of
 * descriptor per packet instead of 10.  d_off_out (optional, n x u64)
 * receives the offsets.
 * ------------------------------------------------------------------------- */
size_t ingot_gpu_packed_workspace_size(uint64_t n);
int ingot_gpu_parse_packed(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                           const uint16_t* d_len, uint64_t n, int chain,
                           ingot_rec* d_out, uint64_t* d_off_out, void* d_work,
                           size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Single-header parse, batched: `HeaderParse::parse(slice)` of one header kind
 * at the start of every slice (ingot-types/src/lib.rs:137-147; the generated
 * bodies, packet/mod.rs:1831-2005) — ValidEthernet::parse, ValidIpv4::parse
 * ... as the reference's `ingot/benches/modify.rs:79-104` parse benches — or
 * a choice's `parse_choice(slice, hint)` (ingot-macros/src/choice.rs:231-246:
 * no hint -> NeedsHint, a hint no variant takes -> Unwanted), as
 * `ValidL3::parse_choice` in `ingot-examples/benches/choice.rs`.
 *
 * Per slice one 8-B ingot_hdr: status (0 Ok, else 1 + ParseError), the header
 * parsed (for a choice: the variant taken), `used` = its HeaderLen (the
 * remainder starts there) and `hint` = its NextLayer hint (ethertype /
 * IpProtocol; INGOT_HINT_NONE = None: TCP, UDP, ICMP, Geneve).  Choices take
 * d_hint[i] when d_hint is non-NULL, else `hint` for every slice
 * (INGOT_HINT_NONE = None).  Slices: (d_off[i], d_len[i]) or fixed slots of
 * `stride` bytes (d_off NULL; d_len optional).
 * ------------------------------------------------------------------------- */
enum ingot_header_kind {
    INGOT_HDR_ETHERNET = 0,  /* ethernet.rs:46-55 */
    INGOT_HDR_VLAN = 1,      /* ethernet.rs:57-65 (VlanBody) */
    INGOT_HDR_IPV4 = 2,      /* ip.rs:63-93 */
    INGOT_HDR_IPV6 = 3,      /* ip.rs:159-182, with its extension-header chain */
    INGOT_HDR_TCP = 4,       /* tcp.rs:9-30 */
    INGOT_HDR_UDP = 5,       /* udp.rs:8-15 */
    INGOT_HDR_ICMP = 6,      /* icmp.rs:42-50 (v4 and v6 share the layout) */
    INGOT_HDR_REPEATED_UDP = 7, /* Repeated<Udp> over the whole slice (util.rs:189-228) */
    INGOT_HDR_GENEVE = 8,    /* geneve.rs:16-44, options subparsed */
    INGOT_HDR_L3 = 16,       /* choice L3 (ingot-examples/src/choices.rs:17-21) */
    INGOT_HDR_L4 = 17,       /* choice L4 (choices.rs:25-29) */
    INGOT_HDR_ULP = 18       /* choice Ulp (choices.rs:32-38) */
};
#define INGOT_HINT_NONE 0xffffffffu

typedef struct ingot_hdr {
    uint8_t status;  /* 0 = Ok, else 1 + ParseError */
    uint8_t kind;    /* enum ingot_header_kind parsed (a choice's variant) */
    uint16_t used;   /* HeaderLen: bytes consumed from the slice start */
    uint32_t hint;   /* NextLayer hint, INGOT_HINT_NONE = None */
} ingot_hdr;

#ifdef __cplusplus
static_assert(sizeof(ingot_hdr) == 8, "ingot_hdr is 8 bytes");
#endif

int ingot_gpu_parse_header(ingot_gpu_ctx* ctx, const uint8_t* d_arena,
                           const uint64_t* d_off, const uint16_t* d_len,
                           uint32_t stride, uint64_t n, int kind,
                           const uint32_t* d_hint, uint32_t hint,
                           ingot_hdr* d_out, void* stream);

/* Error strings. */
const char* ingot_gpu_strerror(int api_code);
/* ParseError name as ingot prints it (error.rs:49-60): "Unwanted", ... ;
 * "Ok" for 0, NULL if out of range. */
const char* ingot_parse_error_name(int status);
/* Layer label of a chain (the PacketParseError label, parse.rs:36-50). */
const char* ingot_chain_layer_label(int chain, int layer);
int ingot_chain_layer_count(int chain);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* INGOT_GPU_H */
