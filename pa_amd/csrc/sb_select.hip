// sb_select.hip -- row selection over decoded pages (selective reads).
//
// A selection is an LSB-first Arrow bitmap over a column's rows (a List
// column's top-level rows).  The host (sb_api.cpp, sb_plan_selected_column,
// sb_plan_selected_list_column) decodes the partially selected pages (Binary
// and List: every touched page) into plan-owned scratch with the ordinary
// page kernels; the kernels
// here turn "rows I want" into per-page work and dense Arrow buffers:
//
//   k_sel_count     selected rows of every page (popcount of its bit range)
//   k_sel_take<W>   compacts a page's scratch rows (values of W bytes, the
//                   validity bitmap, a Boolean values bitmap) to its output
//                   row base
//   k_sel_bin_size / k_sel_scan / k_sel_take_bin<OW>
//                   Binary / Utf8: selected bytes per tile, their scan into
//                   each tile's values base, then offsets + bytes + validity
//   k_sel_take_list<OW, W>
//                   List<primitive>: the same three passes with leaves of W
//                   bytes in place of bytes (the sizing pass and the scan are
//                   the Binary ones), plus the selected rows' leaf validity
//                   bits, a bit-range copy at arbitrary bit offsets
//   k_list_page_rows
//                   the row count every nested page starts with (a List
//                   selection is resolved against these, not the footer's
//                   level counts)
//
// Take grids are one 256-thread workgroup per (page, tile of kSelTileRows
// rows); each wave owns a quarter of the tile and walks it in 64-row groups:
// one lane per row, __ballot-style masks straight from the selection words,
// mbcnt ranks, a running base per wave.  Compacted bitmap bits are gathered
// in an LDS image of the tile's output words (same bit alignment as the
// output) and flushed once: whole words are plain stores, the edge words a
// tile shares with its neighbours go through atomicOr into a bitmap the host
// zeroed first (k_decode_staged's validity discipline).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sb_internal.h"

namespace sb {
namespace {

constexpr uint32_t kSelNT = 256;
constexpr uint32_t kSelWaveRows = kSelTileRows / 4;  // rows of a tile one wave owns
constexpr uint32_t kSelGroups = kSelWaveRows / 64;   // its 64-row groups (one mask per lane < kSelGroups)
constexpr uint32_t kSelLongRow = 256;                // Binary rows above this are copied by the whole wave
static_assert(kSelGroups <= 64, "a wave keeps one group mask per lane");

// This thread's share of the popcount of bitmap bits [b, e): the words are
// strided over nt threads, the first and last word masked.
__device__ __forceinline__ uint32_t bits_count_part(const uint32_t* bm, uint64_t b, uint64_t e, uint32_t tid,
                                                    uint32_t nt) {
  if (e <= b) return 0;
  const uint64_t fw = b >> 5, lw = (e - 1) >> 5;
  uint32_t c = 0;
  for (uint64_t w = fw + tid; w <= lw; w += nt) {
    uint32_t v = bm[w];
    if (w == fw) v &= 0xFFFFFFFFu << (b & 31);
    if (w == lw) v &= 0xFFFFFFFFu >> (31 - (uint32_t)((e - 1) & 31));
    c += (uint32_t)__popc(v);
  }
  return c;
}

// Sum over the workgroup's 256 threads (every thread calls it).
template <class T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // (red may still be read from an earlier sum)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// Bits [pos, pos + 64) of a bitmap whose bits at and past `end` do not exist
// (read as zero; no word past the one holding bit end - 1 is touched).
__device__ __forceinline__ uint64_t bits64(const uint32_t* bm, uint64_t pos, uint64_t end) {
  if (pos >= end) return 0;
  const uint64_t w = pos >> 5, lw = (end - 1) >> 5;
  const uint32_t s = (uint32_t)(pos & 31);
  const uint64_t lo = bm[w];
  const uint64_t mid = w + 1 <= lw ? bm[w + 1] : 0u;
  uint64_t v = (lo | (mid << 32)) >> s;
  if (s && w + 2 <= lw) v |= (uint64_t)bm[w + 2] << (64 - s);
  const uint64_t n = end - pos;
  if (n < 64) v &= (1ull << n) - 1;
  return v;
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// Position of the r-th set bit of m (r < popcount(m)).
__device__ __forceinline__ uint32_t select64(uint64_t m, uint32_t r) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t s = 32; s; s >>= 1) {
    const uint32_t c = (uint32_t)__popcll(m & ((1ull << s) - 1));
    if (r >= c) {
      r -= c;
      m >>= s;
      pos += s;
    }
  }
  return pos;
}

// The bits of `bits` at the set positions of `mask`, packed to the low end
// (one lane per output bit; the same value in every lane).
__device__ __forceinline__ uint64_t wave_compress(uint64_t bits, uint64_t mask, uint32_t cnt, uint32_t lane) {
  const uint32_t pos = lane < cnt ? select64(mask, lane) : 0u;
  return __ballot(lane < cnt && ((bits >> pos) & 1));
}

// OR the low cnt (<= 64) bits of v into the LDS image at bit position pos:
// three lanes, one word each (waves of one tile share words).
__device__ __forceinline__ void image_or(uint32_t* img, uint32_t pos, uint64_t v, uint32_t lane) {
  if (lane >= 3 || !v) return;
  const uint32_t s = pos & 31;
  const uint64_t lo = v << s;
  const uint32_t hi = s ? (uint32_t)(v >> (64 - s)) : 0u;
  const uint32_t w = lane == 0 ? (uint32_t)lo : lane == 1 ? (uint32_t)(lo >> 32) : hi;
  if (w) atomicOr(&img[(pos >> 5) + lane], w);
}

// The tile's image (its bits [bit0, bit0 + cnt) are output bits [out0,
// out0 + cnt), bit0 = out0 & 31) to the output bitmap.
__device__ __forceinline__ void image_flush(const uint32_t* img, uint64_t out0, uint32_t cnt, uint32_t* out,
                                            uint32_t tid) {
  if (!cnt) return;
  const uint32_t bit0 = (uint32_t)(out0 & 31), nw = (bit0 + cnt + 31) >> 5;
  uint32_t* o = out + (out0 >> 5);
  for (uint32_t i = tid; i < nw; i += kSelNT) {
    const uint32_t v = img[i];
    if (32 * i >= bit0 && 32 * (i + 1) <= bit0 + cnt) o[i] = v;
    else if (v) atomicOr(&o[i], v);
  }
}

constexpr uint32_t kImageWords = kSelTileRows / 32 + 3;

__global__ __launch_bounds__(kSelNT) void k_sel_count(const uint32_t* __restrict__ sel,
                                                      const uint64_t* __restrict__ row_offs, uint32_t n_pages,
                                                      uint64_t* __restrict__ counts) {
  __shared__ uint32_t red[4];
  for (uint32_t p = blockIdx.x; p < n_pages; p += gridDim.x) {
    const uint32_t c = block_sum(bits_count_part(sel, row_offs[p], row_offs[p + 1], threadIdx.x, kSelNT), red);
    if (threadIdx.x == 0) counts[p] = c;
  }
}

// What every take kernel starts with: the tile's place in the page and the
// selection masks of this wave's groups.
struct TileWalk {
  SelPage sp;
  uint64_t p0, te, w0;   // the page's first row, the tile's end, this wave's first row (column rows)
  uint64_t m;            // lane g < kSelGroups: the selection mask of group g
  uint32_t excl;         // lane g: selected rows of this wave before group g
  uint32_t tile_base;    // selected rows of the page before the tile
  uint32_t wave_base;    // selected rows of the tile before this wave
  uint32_t tile_cnt;     // selected rows of the tile
};

__device__ __forceinline__ TileWalk tile_walk(const uint32_t* sel, const SelPage* pages, const uint32_t* tiles,
                                              uint32_t* red, uint32_t* wtot) {
  TileWalk t;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t pg = tiles[2 * blockIdx.x], tile = tiles[2 * blockIdx.x + 1];
  t.sp = pages[pg];
  t.p0 = t.sp.sel_row;
  const uint64_t pe = t.p0 + t.sp.num_values, t0 = t.p0 + (uint64_t)tile * kSelTileRows;
  t.te = min(t0 + kSelTileRows, pe);
  t.tile_base = block_sum(bits_count_part(sel, t.p0, t0, tid, kSelNT), red);
  t.w0 = t0 + (uint64_t)wave * kSelWaveRows;
  t.m = lane < kSelGroups ? bits64(sel, t.w0 + 64ull * lane, t.te) : 0ull;
  const uint32_t c = (uint32_t)__popcll(t.m);
  uint32_t inc = c;
  for (uint32_t o = 1; o < kSelGroups; o <<= 1) {
    const uint32_t u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  t.excl = inc - c;
  const uint32_t wsum = __shfl(inc, kSelGroups - 1);
  if (lane == 0) wtot[wave] = wsum;
  __syncthreads();
  t.wave_base = 0;
  for (uint32_t w = 0; w < wave; w++) t.wave_base += wtot[w];
  t.tile_cnt = wtot[0] + wtot[1] + wtot[2] + wtot[3];
  return t;
}

template <int W> struct word_of { using type = uint8_t; };
template <> struct word_of<2> { using type = uint16_t; };
template <> struct word_of<4> { using type = uint32_t; };
template <> struct word_of<8> { using type = uint64_t; };

// W = 0: bitmaps only (a Boolean column: bits[1] is its values bitmap).
template <int W>
__global__ __launch_bounds__(kSelNT) void k_sel_take(SelTake a) {
  __shared__ uint32_t red[4], wtot[4];
  __shared__ uint32_t img[2][kImageWords];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  for (uint32_t i = tid; i < 2 * kImageWords; i += kSelNT) (&img[0][0])[i] = 0;
  const TileWalk t = tile_walk(a.sel, a.pages, a.tiles, red, wtot);  // (its barriers publish the zeroed image)
  if (!t.tile_cnt) return;
  const uint64_t out0 = t.sp.dst_row + t.tile_base;
  const uint32_t bit0 = (uint32_t)(out0 & 31);
  const uint64_t src_end = t.sp.src_row + t.sp.num_values;
  using T = typename word_of<W>::type;
  // the selected rows of all of the wave's groups, loaded before the first
  // store: the loop below would otherwise wait out one load latency a group
  T vals[kSelGroups];
  if (W) {
#pragma unroll
    for (uint32_t g = 0; g < kSelGroups; g++) {
      const uint64_t mg = __shfl(t.m, g);
      vals[g] = (mg >> lane) & 1 ? ((const T*)a.src_values)[t.sp.src_row + (t.w0 + 64ull * g - t.p0) + lane] : T(0);
    }
  }
#pragma unroll
  for (uint32_t g = 0; g < kSelGroups; g++) {
    const uint64_t mg = __shfl(t.m, g);
    if (!mg) continue;  // (uniform over the wave)
    const uint32_t cnt = (uint32_t)__popcll(mg);
    const uint32_t orel = t.wave_base + __shfl(t.excl, g);  // the group's first row in the tile's output
    const uint64_t s0 = t.sp.src_row + (t.w0 + 64ull * g - t.p0);  // its first scratch row
    if (W) {
      if ((mg >> lane) & 1) ((T*)a.dst_values)[out0 + orel + lane_rank(mg)] = vals[g];
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (!a.src_bits[k]) continue;
      const uint64_t c = wave_compress(bits64(a.src_bits[k], s0, src_end), mg, cnt, lane);
      image_or(img[k], bit0 + orel, c, lane);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; k++)
    if (a.src_bits[k]) image_flush(img[k], out0, t.tile_cnt, a.dst_bits[k], tid);
}

template <int OW> struct off_of { using type = uint32_t; };
template <> struct off_of<8> { using type = uint64_t; };

// Row s of the scratch column: its first byte and length.  Offsets a failed
// page left behind are not trusted: a row outside the scratch values is
// empty (the sizing pass and the take pass agree on that).
template <int OW>
__device__ __forceinline__ uint64_t row_len(const SelBin& a, uint64_t s, uint64_t* first) {
  using O = typename off_of<OW>::type;
  const uint64_t b = ((const O*)a.src_offsets)[s], e = ((const O*)a.src_offsets)[s + 1];
  *first = b;
  return (e < b || e > a.src_len) ? 0ull : e - b;
}

template <int OW>
__global__ __launch_bounds__(kSelNT) void k_sel_bin_size(SelBin a) {
  __shared__ uint64_t red[4];
  const uint32_t pg = a.tiles[2 * blockIdx.x], tile = a.tiles[2 * blockIdx.x + 1];
  const SelPage sp = a.pages[pg];
  const uint64_t t0 = sp.sel_row + (uint64_t)tile * kSelTileRows;
  const uint64_t te = min(t0 + kSelTileRows, sp.sel_row + sp.num_values);
  uint64_t sum = 0;
  for (uint64_t r = t0 + threadIdx.x; r < te; r += kSelNT) {
    if (!((a.sel[r >> 5] >> (r & 31)) & 1)) continue;
    uint64_t first;
    sum += row_len<OW>(a, sp.src_row + (r - sp.sel_row), &first);
  }
  sum = block_sum(sum, red);
  if (threadIdx.x == 0) a.tile_bytes[blockIdx.x] = sum;
}

// One wave: tile sizes -> exclusive bases in place, the total behind them, offsets[0] = 0.
template <int OW>
__global__ __launch_bounds__(64) void k_sel_scan(SelBin a) {
  using O = typename off_of<OW>::type;
  const uint32_t lane = threadIdx.x;
  uint64_t carry = 0;
  for (uint32_t b = 0; b < a.n_tiles; b += 64) {
    const uint32_t i = b + lane;
    const uint64_t v = i < a.n_tiles ? a.tile_bytes[i] : 0ull;
    uint64_t inc = v;
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint64_t u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    if (i < a.n_tiles) a.tile_bytes[i] = carry + inc - v;
    carry += __shfl(inc, 63);
  }
  if (lane == 0) {
    a.tile_bytes[a.n_tiles] = carry;
    ((O*)a.dst_offsets)[0] = 0;
  }
}

template <int OW>
__global__ __launch_bounds__(kSelNT) void k_sel_take_bin(SelBin a) {
  using O = typename off_of<OW>::type;
  __shared__ uint32_t red[4], wtot[4];
  __shared__ uint64_t wbytes[4];
  __shared__ uint32_t img[kImageWords];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t i = tid; i < kImageWords; i += kSelNT) img[i] = 0;
  const TileWalk t = tile_walk(a.sel, a.pages, a.tiles, red, wtot);
  if (!t.tile_cnt) return;
  const uint64_t out0 = t.sp.dst_row + t.tile_base;
  const uint32_t bit0 = (uint32_t)(out0 & 31);
  const uint64_t src_end = t.sp.src_row + t.sp.num_values;
  // selected bytes of this wave's rows -> its values base
  uint64_t wsum = 0;
  for (uint32_t g = 0; g < kSelGroups; g++) {
    const uint64_t mg = __shfl(t.m, g);
    uint64_t first;
    if ((mg >> lane) & 1) wsum += row_len<OW>(a, t.sp.src_row + (t.w0 + 64ull * g + lane - t.p0), &first);
  }
  for (int o = 32; o; o >>= 1) wsum += __shfl_xor(wsum, o);
  if (lane == 0) wbytes[wave] = wsum;
  __syncthreads();
  uint64_t base = a.tile_bytes[blockIdx.x];
  for (uint32_t w = 0; w < wave; w++) base += wbytes[w];
  for (uint32_t g = 0; g < kSelGroups; g++) {
    const uint64_t mg = __shfl(t.m, g);
    if (!mg) continue;
    const uint32_t cnt = (uint32_t)__popcll(mg);
    const uint32_t orel = t.wave_base + __shfl(t.excl, g);
    const uint64_t s0 = t.sp.src_row + (t.w0 + 64ull * g - t.p0);
    const bool on = (mg >> lane) & 1;
    uint64_t first = 0;
    const uint64_t len = on ? row_len<OW>(a, s0 + lane, &first) : 0ull;
    uint64_t inc = len;
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint64_t u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    const uint64_t dst = base + inc - len;  // this row's first output byte
    base += __shfl(inc, 63);
    if (on) ((O*)a.dst_offsets)[out0 + orel + lane_rank(mg) + 1] = (O)(dst + len);
    const bool fits = dst + len <= a.values_cap;
    // short rows, packed: output byte b of the group's short rows belongs to
    // the last lane whose prefix is <= b (empty rows share their successor's)
    const uint32_t plen = on && fits && len <= kSelLongRow ? (uint32_t)len : 0u;
    uint32_t pinc = plen;
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(pinc, o);
      if (lane >= o) pinc += u;
    }
    const uint32_t pex = pinc - plen, ptot = __shfl(pinc, 63);
    for (uint32_t b0 = 0; b0 < ptot; b0 += 64) {
      const uint32_t b = b0 + lane;
      uint32_t r = 0;
#pragma unroll
      for (uint32_t s = 32; s; s >>= 1) {
        const uint32_t cand = r + s;
        const uint32_t pv = __shfl(pex, cand & 63);
        if (cand < 64 && pv <= b) r = cand;
      }
      const uint64_t rs = __shfl(first, r), rd = __shfl(dst, r);
      const uint32_t rp = __shfl(pex, r);
      if (b < ptot) a.dst_values[rd + (b - rp)] = a.src_values[rs + (b - rp)];
    }
    // long rows: the whole wave copies one
    for (uint64_t big = __ballot(on && fits && len > kSelLongRow); big; big &= big - 1) {
      const uint32_t r = (uint32_t)__builtin_ctzll(big);
      const uint64_t rs = __shfl(first, r), rd = __shfl(dst, r), rl = __shfl(len, r);
      for (uint64_t i = lane; i < rl; i += 64) a.dst_values[rd + i] = a.src_values[rs + i];
    }
    if (a.src_validity) {
      const uint64_t c = wave_compress(bits64(a.src_validity, s0, src_end), mg, cnt, lane);
      image_or(img, bit0 + orel, c, lane);
    }
  }
  __syncthreads();
  if (a.src_validity) image_flush(img, out0, t.tile_cnt, a.dst_validity, tid);
}

// OR the low cnt (1..64) bits of v into a global bitmap at bit position pos:
// three lanes, one word each.  Every output bit has one writer, so a word all
// of whose bits this call owns has no other writer and is stored plainly; the
// rest are ORed into the bitmap the host zeroed.
__device__ __forceinline__ void bits_out(uint32_t* out, uint64_t pos, uint64_t v, uint32_t cnt, uint32_t lane) {
  if (lane >= 3 || !cnt) return;
  const uint32_t s = (uint32_t)(pos & 31);
  const uint64_t own = cnt >= 64 ? ~0ull : (1ull << cnt) - 1;
  v &= own;
  const uint64_t vlo = v << s, olo = own << s;
  const uint32_t vhi = s ? (uint32_t)(v >> (64 - s)) : 0u, ohi = s ? (uint32_t)(own >> (64 - s)) : 0u;
  const uint32_t w = lane == 0 ? (uint32_t)vlo : lane == 1 ? (uint32_t)(vlo >> 32) : vhi;
  const uint32_t o = lane == 0 ? (uint32_t)olo : lane == 1 ? (uint32_t)(olo >> 32) : ohi;
  uint32_t* p = out + (pos >> 5) + lane;
  if (o == 0xFFFFFFFFu) *p = w;
  else if (w) atomicOr(p, w);
}

// List<primitive>: k_sel_take_bin with leaves of W bytes in place of bytes
// (a.b counts leaves), and the leaf validity bits of the copied leaves.  A
// tile's leaves are unbounded, so their bits take no LDS image: each step of
// the two copy loops ballots the source bits of its (up to 64) leaves and
// writes them at their output bit position (bits_out).
template <int OW, int W>
__global__ __launch_bounds__(kSelNT) void k_sel_take_list(SelList l) {
  using O = typename off_of<OW>::type;
  using T = typename word_of<W>::type;
  const SelBin& a = l.b;
  __shared__ uint32_t red[4], wtot[4];
  __shared__ uint64_t wleaves[4];
  __shared__ uint32_t img[kImageWords];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t i = tid; i < kImageWords; i += kSelNT) img[i] = 0;
  const TileWalk t = tile_walk(a.sel, a.pages, a.tiles, red, wtot);
  if (!t.tile_cnt) return;
  const uint64_t out0 = t.sp.dst_row + t.tile_base;
  const uint32_t bit0 = (uint32_t)(out0 & 31);
  const uint64_t src_end = t.sp.src_row + t.sp.num_values;
  const T* sv = (const T*)a.src_values;
  T* dv = (T*)a.dst_values;
  const uint32_t* sbits = l.src_leaf_validity;
  // selected leaves of this wave's rows -> its values base
  uint64_t wsum = 0;
  for (uint32_t g = 0; g < kSelGroups; g++) {
    const uint64_t mg = __shfl(t.m, g);
    uint64_t first;
    if ((mg >> lane) & 1) wsum += row_len<OW>(a, t.sp.src_row + (t.w0 + 64ull * g + lane - t.p0), &first);
  }
  for (int o = 32; o; o >>= 1) wsum += __shfl_xor(wsum, o);
  if (lane == 0) wleaves[wave] = wsum;
  __syncthreads();
  uint64_t base = a.tile_bytes[blockIdx.x];
  for (uint32_t w = 0; w < wave; w++) base += wleaves[w];
  for (uint32_t g = 0; g < kSelGroups; g++) {
    const uint64_t mg = __shfl(t.m, g);
    if (!mg) continue;
    const uint32_t cnt = (uint32_t)__popcll(mg);
    const uint32_t orel = t.wave_base + __shfl(t.excl, g);
    const uint64_t s0 = t.sp.src_row + (t.w0 + 64ull * g - t.p0);
    const bool on = (mg >> lane) & 1;
    uint64_t first = 0;
    const uint64_t len = on ? row_len<OW>(a, s0 + lane, &first) : 0ull;
    uint64_t inc = len;
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint64_t u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    const uint64_t dst = base + inc - len;  // this row's first output leaf
    base += __shfl(inc, 63);
    if (on) ((O*)a.dst_offsets)[out0 + orel + lane_rank(mg) + 1] = (O)(dst + len);
    const bool fits = dst + len <= a.values_cap;
    // short rows, packed: output leaf b of the group's short rows belongs to
    // the last lane whose prefix is <= b (empty rows share their successor's)
    const uint32_t plen = on && fits && len <= kSelLongRow ? (uint32_t)len : 0u;
    uint32_t pinc = plen;
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(pinc, o);
      if (lane >= o) pinc += u;
    }
    const uint32_t pex = pinc - plen, ptot = __shfl(pinc, 63);
    for (uint32_t b0 = 0; b0 < ptot; b0 += 64) {
      const uint32_t b = b0 + lane;
      uint32_t r = 0;
#pragma unroll
      for (uint32_t s = 32; s; s >>= 1) {
        const uint32_t cand = r + s;
        const uint32_t pv = __shfl(pex, cand & 63);
        if (cand < 64 && pv <= b) r = cand;
      }
      const uint32_t k = b - __shfl(pex, r);
      const uint64_t src = __shfl(first, r) + k, d = __shfl(dst, r) + k;
      const bool act = b < ptot;
      if (act) dv[d] = sv[src];
      if (sbits) {
        // the step's output leaves are consecutive except where a long row
        // (or one that does not fit) lies between two short ones: one
        // bits_out per consecutive run
        const uint64_t vb = __ballot(act && ((sbits[src >> 5] >> (src & 31)) & 1));
        const uint64_t dprev = __shfl_up(d, 1);
        uint64_t starts = __ballot(act && (lane == 0 || d != dprev + 1));
        const uint32_t nact = min(64u, ptot - b0);
        while (starts) {
          const uint32_t s = (uint32_t)__builtin_ctzll(starts);
          starts &= starts - 1;
          const uint32_t e = starts ? (uint32_t)__builtin_ctzll(starts) : nact;
          bits_out(l.dst_leaf_validity, __shfl(d, s), vb >> s, e - s, lane);
        }
      }
    }
    // long rows: the whole wave copies one, 64 leaves a step
    for (uint64_t big = __ballot(on && fits && len > kSelLongRow); big; big &= big - 1) {
      const uint32_t r = (uint32_t)__builtin_ctzll(big);
      const uint64_t rs = __shfl(first, r), rd = __shfl(dst, r), rl = __shfl(len, r);
      for (uint64_t i0 = 0; i0 < rl; i0 += 64) {
        const uint64_t i = i0 + lane;
        const bool act = i < rl;
        if (act) dv[rd + i] = sv[rs + i];
        if (sbits) {
          const uint64_t vb = __ballot(act && ((sbits[(rs + i) >> 5] >> ((rs + i) & 31)) & 1));
          bits_out(l.dst_leaf_validity, rd + i0, vb, (uint32_t)min((uint64_t)64, rl - i0), lane);
        }
      }
    }
    if (a.src_validity) {
      const uint64_t c = wave_compress(bits64(a.src_validity, s0, src_end), mg, cnt, lane);
      image_or(img, bit0 + orel, c, lane);
    }
  }
  __syncthreads();
  if (a.src_validity) image_flush(img, out0, t.tile_cnt, a.dst_validity, tid);
}

// A nested page starts with its row count (pages start at any byte).
__global__ __launch_bounds__(256) void k_list_page_rows(const uint8_t* __restrict__ chunk,
                                                        const uint64_t* __restrict__ offs, uint32_t n_pages,
                                                        uint32_t* __restrict__ rows) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pages) return;
  const uint8_t* p = chunk + offs[i];
  rows[i] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

}  // namespace

int launch_sel_count(const uint32_t* sel, const uint64_t* row_offs, uint32_t n_pages, uint64_t* counts, void* stream) {
  if (!n_pages) return 0;
  const uint32_t grid = n_pages < 65535u ? n_pages : 65535u;
  hipLaunchKernelGGL(k_sel_count, dim3(grid), dim3(kSelNT), 0, (hipStream_t)stream, sel, row_offs, n_pages, counts);
  return hipGetLastError() != hipSuccess;
}

int launch_sel_take(int width, const SelTake& a, void* stream) {
  if (!a.n_tiles) return 0;
  const dim3 grid(a.n_tiles), block(kSelNT);
  hipStream_t s = (hipStream_t)stream;
  switch (width) {
    case 0: hipLaunchKernelGGL(k_sel_take<0>, grid, block, 0, s, a); break;
    case 1: hipLaunchKernelGGL(k_sel_take<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_sel_take<2>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(k_sel_take<4>, grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL(k_sel_take<8>, grid, block, 0, s, a); break;
    default: return 1;
  }
  return hipGetLastError() != hipSuccess;
}

template <int OW>
static int take_bin(const SelBin& a, hipStream_t s) {
  const dim3 grid(a.n_tiles), block(kSelNT);
  hipLaunchKernelGGL(k_sel_bin_size<OW>, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_sel_scan<OW>, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_sel_take_bin<OW>, grid, block, 0, s, a);
  return hipGetLastError() != hipSuccess;
}

int launch_sel_take_bin(int offset_width, const SelBin& a, void* stream) {
  if (!a.n_tiles) return 0;
  if (offset_width == 4) return take_bin<4>(a, (hipStream_t)stream);
  if (offset_width == 8) return take_bin<8>(a, (hipStream_t)stream);
  return 1;
}

// The sizing pass and the scan are the Binary ones (offsets count leaves).
template <int OW>
static int take_list(int width, const SelList& a, hipStream_t s) {
  const dim3 grid(a.b.n_tiles), block(kSelNT);
  hipLaunchKernelGGL(k_sel_bin_size<OW>, grid, block, 0, s, a.b);
  hipLaunchKernelGGL(k_sel_scan<OW>, dim3(1), dim3(64), 0, s, a.b);
  switch (width) {
    case 1: hipLaunchKernelGGL((k_sel_take_list<OW, 1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_sel_take_list<OW, 2>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_sel_take_list<OW, 4>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((k_sel_take_list<OW, 8>), grid, block, 0, s, a); break;
    default: return 1;
  }
  return hipGetLastError() != hipSuccess;
}

int launch_sel_take_list(int offset_width, int width, const SelList& a, void* stream) {
  if (!a.b.n_tiles) return 0;
  if (offset_width == 4) return take_list<4>(width, a, (hipStream_t)stream);
  if (offset_width == 8) return take_list<8>(width, a, (hipStream_t)stream);
  return 1;
}

int launch_list_page_rows(const uint8_t* chunk, const uint64_t* offs, uint32_t n_pages, uint32_t* rows, void* stream) {
  if (!n_pages) return 0;
  hipLaunchKernelGGL(k_list_page_rows, dim3((n_pages + 255) / 256), dim3(256), 0, (hipStream_t)stream, chunk, offs,
                     n_pages, rows);
  return hipGetLastError() != hipSuccess;
}

}  // namespace sb
