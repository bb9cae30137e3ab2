// resolve.h — the public edit, set and sum lists (include/ingot_gpu.h) resolved
// to the kernels' argument blocks (kernels.h).  Pure host functions: no HIP
// runtime call, and the context only for its NULL test, so they run without a
// device (tools/api_args_selftest.cpp, tools/emit_rows_selftest.cpp,
// tools/emit_read_rows_selftest.cpp).  The C
// ABI's entry points (api.cpp) add the frames or chunk tables and launch.
#pragma once

#include "../../include/ingot_gpu.h"
#include "kernels.h"

namespace ingot_gpu {

inline bool chain_ok(int chain) { return chain >= 0 && chain < INGOT_CHAIN_COUNT; }

// A call's `what`: only bits of `allowed`, zero only where the call takes it,
// and the tunnel's outer sum only for the tunnel chain.
bool what_ok(uint32_t what, uint32_t allowed, bool zero_ok, int chain);

// The edit list of a rewrite call -> ModifyCsumArgs (c.m.p is the caller's to
// fill): each ingot_edit's field resolved to its header kind and covering
// bytes and, with `what`, to the sums its bytes feed.  EINVAL: NULL context,
// chain, the list's size, unknown field / op / layer, refused fields.
int resolve_edits(const ingot_gpu_ctx* ctx, int chain, const ingot_edit* edits, uint32_t n_edits,
                  uint32_t what, ModifyCsumArgs& c);

// The ingot_edit_rows list -> the kernels' pieces, each with the sums it
// feeds: checks 1 to 3 of ingot_gpu_parse_modify_rows.  `a` comes in zeroed;
// a.p is the caller's to fill.
int resolve_edit_rows(const ingot_gpu_ctx* ctx, int chain, const ingot_edit_rows* edits,
                      uint32_t n_edits, const uint32_t* d_row, uint32_t n_rows, uint32_t what,
                      ModifyRowsArgs& a);

// The header block and its setters -> EmitArgs (every emit call).
int emit_args(const uint8_t* hdr, uint32_t hdr_len, const ingot_emit_set* sets, uint32_t n_sets,
              EmitArgs& a);

// The sums, checked against the header block and the setters that emit_args
// has already accepted into `a`.
int emit_sums(const uint8_t* hdr, uint32_t hdr_len, const ingot_emit_set* sets, uint32_t n_sets,
              const ingot_emit_sum* sums, uint32_t n_sums, EmitArgs& a);

// ingot_gpu_emit_packets_rows: the set list -> the pieces of EmitRowsArgs.
// `narrow` (INGOT_MAX_EMIT_SETS entries) receives the (at, field) of the
// narrow sets, for emit_sums' version / ihl rule.
int emit_rows_pieces(const ingot_emit_set_rows* sets, uint32_t n_sets, bool have_row,
                     uint32_t hdr_len, EmitRowsArgs& a, ingot_emit_set* narrow,
                     uint32_t& n_narrow);

}  // namespace ingot_gpu
