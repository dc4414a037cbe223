// sb_encode_dev.h -- internals shared by the device writer's two translation
// units (sb_encode_gpu.hip: entry points and the no-sampling fast path;
// sb_encode_adapt.hip: the adaptive page encoders and their host drivers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/strawboat_gpu.h"
#include "sb_internal.h"

namespace sb {

// What the page encoders need to know of a physical type.  width: bytes of a
// value (Boolean: 1, its staged bits); offset_width: bytes of a Binary / Utf8
// offset.  Both 0: not a type the device writer encodes.
struct EncType {
  uint32_t width;
  bool is_float, is_signed, is_bool;
  uint32_t offset_width;
  constexpr bool supported() const { return width || offset_width; }
  constexpr uint32_t value_width() const { return is_bool ? 0 : width; }  // of a fixed-width number, else 0
};
constexpr EncType enc_type(int32_t t) {
  switch (t) {
    case SB_T_INT8: return {1, false, true, false, 0};
    case SB_T_INT16: return {2, false, true, false, 0};
    case SB_T_INT32: return {4, false, true, false, 0};
    case SB_T_INT64: return {8, false, true, false, 0};
    case SB_T_UINT8: return {1, false, false, false, 0};
    case SB_T_UINT16: return {2, false, false, false, 0};
    case SB_T_UINT32: return {4, false, false, false, 0};
    case SB_T_UINT64: return {8, false, false, false, 0};
    case SB_T_FLOAT32: return {4, true, false, false, 0};
    case SB_T_FLOAT64: return {8, true, false, false, 0};
    case SB_T_BOOLEAN: return {1, false, false, true, 0};
    case SB_T_BINARY: case SB_T_UTF8: return {0, false, false, false, 4};
    case SB_T_LARGE_BINARY: case SB_T_LARGE_UTF8: return {0, false, false, false, 8};
  }
  return {0, false, false, false, 0};
}

// Paging of a column chunk: page_size = max_page_size.unwrap_or(len).min(len)
// rows a page (write/common.rs:54-58).
struct PagePlan {
  uint64_t step, np;
  PagePlan(uint64_t n_rows, uint64_t max_page_rows)
      : step(max_page_rows ? std::min(max_page_rows, n_rows) : n_rows), np(step ? (n_rows + step - 1) / step : 0) {}
};
// The entry points' output protocol, after their argument checks: *n_pages,
// the room in h_metas, *out_len = 0, pages of at most max_step rows, the
// context's device.  The entry point returns its status unless that is SB_OK
// and there are pages (pl.np) to encode.
sb_status begin_pages(sb_ctx* ctx, const PagePlan& pl, uint64_t max_step, sb_page_meta* h_metas, uint64_t metas_cap,
                      uint64_t* n_pages, uint64_t* out_len);

// Pages that are leaf slices behind a level header (List and nested columns):
// page p holds the leaf values [rows_at[p], rows_at[p + 1]) and starts with
// head_len[p] bytes at heads + head_at[p] (its slot ends at head_at[p + 1])
// in place of a validity prefix.
struct ListPart {
  const uint64_t* rows_at;    // device [np + 1]
  const uint64_t* head_at;    // device [np + 1]
  const uint8_t* heads;       // device
  const uint32_t* head_len;   // device [np]
  const uint64_t* h_rows_at;  // host [np + 1]
  const uint64_t* h_head_at;  // host [np + 1]
  const uint64_t* h_levels;   // host [np]: PageMeta.num_values
};

uint64_t adaptive_slot_bytes(uint64_t P, uint32_t w, int nullable);
int encode_adaptive(sb_ctx* ctx, int phys, const uint8_t* d_values, const uint8_t* d_validity, uint64_t n_rows,
                    int nullable, const sb_write_options* opts, uint64_t P, uint8_t* d_out, uint64_t out_cap,
                    uint64_t* out_len, sb_page_meta* h_metas, uint64_t np, const ListPart* lp);
int encode_list_device(sb_ctx* ctx, int phys, const int64_t* d_offsets, const uint8_t* d_list_validity,
                       int list_nullable, const void* d_child, const uint8_t* d_child_validity, int item_nullable,
                       uint64_t n_rows, const sb_write_options* opts, uint64_t step, uint8_t* d_out, uint64_t out_cap,
                       uint64_t* out_len, sb_page_meta* h_metas, uint64_t np);

// ULEB128 of h: its length, and its bytes at out (any address space)
__device__ __forceinline__ uint32_t uleb_len(uint64_t h) {
  uint32_t l = 1;
  while (h >= 0x80) {
    h >>= 7;
    l++;
  }
  return l;
}
template <class Ptr>
__device__ __forceinline__ void put_uleb(Ptr out, uint64_t h) {
  for (; h >= 0x80; h >>= 7) *out++ = (uint8_t)(h | 0x80);
  *out = (uint8_t)h;
}

}  // namespace sb
