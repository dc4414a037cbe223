// sb_dev_core.h -- device code the decode units share: the build knobs, the
// byte sources (LDS / HBM), the per-workgroup Shared state, the scans and
// st_out.  Included by .hip units only; defines no kernel and no device
// variable.  (The codec parsers every page kernel uses are still in
// sb_decode.hip, their only user so far.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sb_internal.h"

namespace sbk {

using namespace sb;

#ifndef SB_BLOCK
#define SB_BLOCK 256
#endif
#ifndef SB_LOAD_NT
#define SB_LOAD_NT 1
#endif
#ifndef SB_STORE_NT
#define SB_STORE_NT 1
#endif
#ifndef SB_LDS_DMA
#define SB_LDS_DMA 1
#endif
constexpr int NT = SB_BLOCK;
constexpr int NW = NT / 64;
constexpr uint32_t kWinBlocks = 64;  // bitpack blocks per header walk window
constexpr uint32_t kMaxConts = 16;   // roaring containers handled per page
constexpr uint32_t kMaxBitmapConts = 4;  // of which bitmap containers (card > 4096)
constexpr uint32_t kRleFastRows = 8192;  // RLE pages up to this many rows use the run-start bitmap

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int W> struct VT { using T = uint32_t; };
template <> struct VT<8> { using T = uint64_t; };
// Int128 / Int256 (the storage of Decimal / Decimal256): L little-endian dwords
template <int L>
struct WideV {
  uint32_t d[L];
  __device__ __forceinline__ bool operator==(const WideV& o) const {
    bool e = true;
#pragma unroll
    for (int k = 0; k < L; k++) e &= d[k] == o.d[k];
    return e;
  }
};
template <> struct VT<16> { using T = WideV<4>; };
template <> struct VT<32> { using T = WideV<8>; };

// ---------------------------------------------------------------------------
// byte sources
// ---------------------------------------------------------------------------
// Page staged in LDS at byte `base` of the dynamic LDS words.  The staging
// buffer carries kStagePad bytes of slack so word-granular over-reads are safe.
struct LdsSrc {
  const uint32_t* w;
  uint32_t base;
  __device__ __forceinline__ uint32_t u8(uint32_t p) const {
    p += base;
    return (w[p >> 2] >> ((p & 3) * 8)) & 0xFFu;
  }
  __device__ __forceinline__ uint32_t u32(uint32_t p) const {
    p += base;
    uint32_t i = p >> 2;
    return __builtin_amdgcn_alignbyte(w[i + 1], w[i], p & 3);
  }
  __device__ __forceinline__ LdsSrc at(uint32_t o) const { return LdsSrc{w, base + o}; }
  __device__ __forceinline__ uint64_t u64(uint32_t p) const {
    p += base;
    uint32_t i = p >> 2, sh = p & 3;
    uint32_t a = w[i], b = w[i + 1], c = w[i + 2];
    return (uint64_t)__builtin_amdgcn_alignbyte(b, a, sh) |
           ((uint64_t)__builtin_amdgcn_alignbyte(c, b, sh) << 32);
  }
  // L dwords at any byte position (one dword of over-read, inside the pad)
  template <int L>
  __device__ __forceinline__ void words(uint32_t p, uint32_t* o) const {
    p += base;
    uint32_t i = p >> 2, sh = p & 3;
    uint32_t d[L + 1];
#pragma unroll
    for (int k = 0; k <= L; k++) d[k] = w[i + k];
#pragma unroll
    for (int k = 0; k < L; k++) o[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
  }
  // the 4 lane words at p and (if need_hi) the 4 at p + 16, unaligned
  __device__ __forceinline__ void quad_words(uint32_t p, bool need_hi, uint32_t* d8) const {
    p += base;
    uint32_t i = p >> 2, sh = p & 3;
    uint32_t d[9];
#pragma unroll
    for (int k = 0; k < 9; k++) d[k] = w[i + k];
#pragma unroll
    for (int k = 0; k < 8; k++) d8[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
  }
};

// Page read straight from HBM (pages larger than the LDS stage).  Unaligned
// words are assembled from the aligned dwords that contain them, so no read
// leaves the bytes the page owns.
struct GlbSrc {
  typedef const __attribute__((address_space(1))) uint8_t g8;
  typedef const __attribute__((address_space(1))) uint32_t g32;
  g8* p;  // global address space: global_load, not flat
  __device__ __forceinline__ GlbSrc() : p(nullptr) {}
  __device__ __forceinline__ GlbSrc(const uint8_t* q) : p((g8*)q) {}
  __device__ __forceinline__ GlbSrc(g8* q) : p(q) {}
  __device__ __forceinline__ GlbSrc at(uint32_t o) const { return GlbSrc{p + o}; }
  __device__ __forceinline__ uint32_t u8(uint32_t i) const { return p[i]; }
  __device__ __forceinline__ uint32_t u32(uint32_t i) const {
    const uintptr_t a = (uintptr_t)(p + i);
    g32* q = (g32*)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3);
    if (sh == 0) return q[0];
    return __builtin_amdgcn_alignbyte(q[1], q[0], sh);
  }
  __device__ __forceinline__ uint64_t u64(uint32_t i) const {
    return (uint64_t)u32(i) | ((uint64_t)u32(i + 4) << 32);
  }
  // L dwords at any byte position, from the aligned dwords that hold them
  template <int L>
  __device__ __forceinline__ void words(uint32_t i, uint32_t* o) const {
    const uintptr_t a = (uintptr_t)(p + i);
    g32* q = (g32*)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3);
    if (sh == 0) {
#pragma unroll
      for (int k = 0; k < L; k++) o[k] = q[k];
      return;
    }
    uint32_t d[L + 1];
#pragma unroll
    for (int k = 0; k <= L; k++) d[k] = q[k];
#pragma unroll
    for (int k = 0; k < L; k++) o[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
  }
  __device__ __forceinline__ void quad_words(uint32_t pos, bool need_hi, uint32_t* d8) const {
#pragma unroll
    for (int k = 0; k < 4; k++) d8[k] = u32(pos + 4 * k);
    if (need_hi) {
#pragma unroll
      for (int k = 0; k < 4; k++) d8[4 + k] = u32(pos + 16 + 4 * k);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) d8[4 + k] = 0;
    }
  }
};

template <int W, class Src>
__device__ __forceinline__ typename VT<W>::T ldv(const Src& s, uint32_t p) {
  if constexpr (W >= 16) {
    typename VT<W>::T v;
    s.template words<W / 4>(p, v.d);
    return v;
  } else if constexpr (W == 8) return s.u64(p);
  else if constexpr (W == 4) return s.u32(p);
  else if constexpr (W == 2) return s.u32(p) & 0xFFFFu;
  else return s.u8(p);
}

// ---------------------------------------------------------------------------
// per-workgroup shared state
// ---------------------------------------------------------------------------
struct Stream {
  uint32_t codec, body, csize, n;
};

struct Shared {
  uint32_t err;
  uint32_t walk_off;
  uint32_t blk_off[kWinBlocks];
  uint32_t blk_bits[kWinBlocks];
  uint64_t wsum[NW];
  uint32_t rle_start[NT + 1];
  uint32_t rle_c;
  uint32_t rle_R;
  uint32_t rle_flags;  // bit0 = a run ends exactly at n, bit1 = a run overshoots n, bit2 = zero-count run
  uint32_t rle_bits[kRleFastRows / 32];  // bit r set <=> a run starts at row r
  uint16_t rle_pref[kRleFastRows / 32];  // set bits before word w
  // page header
  uint32_t has_valid, vb_pos, vb_bytes;
  Stream top;
  Stream sub;  // the leaf stream at the bottom of the cascade
  uint32_t chain;
  uint32_t defer;
  // Dict
  uint32_t dict_k, dict_off;
  // Freq: the roaring bitmap's container tables (roaring_build), in the LDS
  // arrays below when they fit, else in the page's HBM region
  uint64_t freq_top;
  uint32_t n_conts;
  uint32_t roar_r, roar_bm, roar_pending;  // position and size of the portable bitmap; tables still to build
  uint32_t roar_lds, cp_lds;              // tables / checkpoints in the arrays below (else the region)
  uint32_t* rkey;                         // container keys
  uint32_t* rdata;                        // source position of each container's data
  uint32_t* rpre;                         // exceptions before each container (n_conts + 1)
  uint32_t* rbm;                          // bitmap container index into rcp, or ~0u for array containers
  uint16_t* rcp;                          // per bitmap container: set bits before each 16-word group (64)
  uint32_t cont_key[kMaxConts];
  uint32_t cont_data[kMaxConts];
  uint32_t cont_prefix[kMaxConts + 1];
  uint32_t cont_bm[kMaxConts];
  uint16_t cont_cp[kMaxBitmapConts][64];
};

__device__ __forceinline__ void set_err(Shared& sh, uint32_t code) { atomicMax(&sh.err, code); }

// Block-wide exclusive scan (sum) of one value per thread; *total = block sum.
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, Shared& sh, T* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    T y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) sh.wsum[wv] = (uint64_t)x;
  __syncthreads();
  T pre = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < NW; k++) {
    T s = (T)sh.wsum[k];
    if (k < wv) pre += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return pre + x - v;
}

// ---------------------------------------------------------------------------
// output sinks
// ---------------------------------------------------------------------------
template <class V>
__device__ __forceinline__ void st_out(V* p, V v) {
#if SB_STORE_NT
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {  // DPP: no LDS round trips
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);  // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false); // row_bcast:15
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false); // row_bcast:31
  return v;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ void bin_put_off(uint8_t* out, uint64_t row, uint64_t v, int ow) {
  if (ow == 8) ((uint64_t*)out)[row] = v;
  else ((uint32_t*)out)[row] = (uint32_t)v;
}

}  // namespace sbk
