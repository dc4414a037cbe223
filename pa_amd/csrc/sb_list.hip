// sb_list.hip -- List<primitive> pages and the general nest walk: the list
// sizing / scan / level kernels, k_nest_walk and their launchers.
#include <algorithm>

#include "sb_dev_core.h"

namespace sbk {

// ===========================================================================
// Nested List<primitive> pages: read_validity_nested (read/read_basic.rs:65-173)
// + create_list (read/array/list.rs:48), one list level over a primitive leaf.
// Page = [u32 rows][u32 rep_len][u32 def_len][rep hybrid][def hybrid][values].
// Per level: rep == 0 starts a row (list offset = leaves so far, list valid =
// def > 0); def >= cum_sum[1] = nl + 1 is a leaf (leaf valid = def > nl + 1);
// decoding stops before the level that would start row `rows + 1`
// (:158-162).  k_list_size counts each page's rows and leaves and fills the
// page's values-stream descriptor, k_list_bscan / k_list_bases turn counts
// into bases, k_list_levels writes offsets and both bitmaps; the values streams then go
// through the flat decode kernels (k_decode_staged / global / deferred /
// k_inflate) at their leaf bases.
// ===========================================================================
constexpr uint32_t kLvK = 32;                   // levels per thread per tile
constexpr uint32_t kMaxRuns = 64;               // hybrid runs per level stream

struct LvRuns {
  uint32_t n;
  uint32_t start[kMaxRuns + 1];  // first level of each run
  uint32_t arg[kMaxRuns];        // bit-packed: 0x80000000 | payload position; RLE: the value
};

struct ListShared {
  uint32_t rows, vpos, bw_def, region, fast;
  LvRuns rep, def;
};

__device__ __forceinline__ void put_err(uint32_t* err, uint32_t code) { *err = max(*err, code); }

// parquet2 HybridRleDecoder (hybrid_rle/decoder.rs) run headers of one level
// stream [p, end) covering L levels, bit width bw.  One lane.
template <class Src>
__device__ bool parse_runs(const Src& s, uint32_t* err, uint32_t p, uint32_t end, uint32_t L, uint32_t bw, LvRuns& R) {
  uint32_t covered = 0, n = 0;
  while (covered < L) {
    uint32_t h = 0, sft = 0;
    for (;;) {  // ULEB128 header
      if (p >= end || sft > 28) { put_err(err, ST_OUT_OF_SPEC); return false; }
      const uint32_t c = s.u8(p++);
      h |= (c & 0x7Fu) << sft;
      if (!(c & 0x80)) break;
      sft += 7;
    }
    if (n == kMaxRuns) { put_err(err, ST_NYI); return false; }
    R.start[n] = covered;
    if (h & 1) {  // bit-packed: h >> 1 groups of 8, clamped to the bytes present
      const uint64_t want = (uint64_t)(h >> 1) * bw;
      const uint32_t have = (uint32_t)min<uint64_t>(want, end - p);
      const uint32_t vals = (uint32_t)min<uint64_t>((uint64_t)(h >> 1) * 8, (uint64_t)have * 8 / bw);
      if (vals == 0) { put_err(err, ST_OUT_OF_SPEC); return false; }
      R.arg[n] = 0x80000000u | p;
      p += have;
      covered += vals;
    } else {  // RLE: h >> 1 repeats of a ceil(bw / 8)-byte value
      const uint32_t vb = (bw + 7) / 8;
      if (p + vb > end) { put_err(err, ST_OUT_OF_SPEC); return false; }
      uint32_t v = 0;
      for (uint32_t k = 0; k < vb; k++) v |= s.u8(p + k) << (8 * k);
      R.arg[n] = v;
      p += vb;
      covered += h >> 1;
    }
    n++;
  }
  R.start[n] = covered;
  R.n = n;
  return true;
}

template <class Src>
__device__ __forceinline__ uint32_t level_at(const Src& s, const LvRuns& R, uint32_t i, uint32_t bw) {
  uint32_t r = 0;
  if (R.n > 1) {  // last run starting at or before i
    uint32_t lo = 0, hi = R.n;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (R.start[mid] <= i) lo = mid; else hi = mid;
    }
    r = lo;
  }
  const uint32_t a = R.arg[r];
  if (!(a & 0x80000000u)) return a;
  const uint32_t bit = (i - R.start[r]) * bw;
  return (s.u32((a & 0x7FFFFFFFu) + (bit >> 3)) >> (bit & 7)) & ((1u << bw) - 1);
}

struct ListArgs {
  const uint8_t* chunk;
  const PageDesc* pages;  // num_values = the page's level count (PageMeta.num_values)
  uint32_t n_pages;
  uint32_t nl, ni, ow;    // list nullable, item nullable, offset width
  uint32_t width;         // leaf value width (the values header's usize / width = leaves)
  uint32_t peek;          // sizes from the page headers (verified at plan time) instead of the levels
  uint64_t* counts;       // [n_pages] rows << 32 | leaves
  uint64_t* local;        // [2 n_pages] row / leaf bases within the page's block of NT pages
  uint64_t* blk;          // [2 ceil(n_pages / NT)] row / leaf totals of each block
  uint64_t* totals;       // [2] rows, leaves
  uint4* lvdesc;          // [2 n_pages] per page: the parse results the levels pass reuses
  PageDesc* vpages;       // values stream of each page, as a flat page at its leaf base
  uint8_t* out_offsets;
  uint32_t* out_list_validity;
  uint32_t* out_leaf_validity;
  uint32_t* status;
  uint32_t epoch;             // k_list_bases: tag of this decode's block totals
};

// Header + run tables (one lane).
template <class Src>
__device__ bool list_parse(const Src& s, uint32_t* err, ListShared& ls, const PageDesc& pd, const ListArgs& a) {
  const uint32_t len = pd.byte_len, L = pd.num_values;
  if (len < 12) { put_err(err, ST_IO); return false; }
  const uint32_t rows = s.u32(0), rl = s.u32(4), dl = s.u32(8);
  if ((uint64_t)12 + rl + dl > len) { put_err(err, ST_IO); return false; }
  const uint32_t max_def = a.nl + 1 + a.ni;
  ls.rows = rows;
  ls.vpos = 12 + rl + dl;
  ls.region = 12 + rl + dl;
  ls.bw_def = 32 - __clz(max_def);
  if (!parse_runs(s, err, 12, 12 + rl, L, 1, ls.rep)) return false;
  if (!parse_runs(s, err, 12 + rl, 12 + rl + dl, L, ls.bw_def, ls.def)) return false;
  if (L > 0 && rows == 0) { put_err(err, ST_OUT_OF_SPEC); return false; }
  // the writer's shape: one bit-packed run per stream, def bit width <= 2
  ls.fast = ls.rep.n == 1 && (ls.rep.arg[0] & 0x80000000u) && ls.def.n == 1 && (ls.def.arg[0] & 0x80000000u) &&
            ls.bw_def <= 2;
  return true;
}

// Gathers the even bits of x (bit 2j -> bit j).
__device__ __forceinline__ uint32_t compact_even(uint64_t x) {
  x &= 0x5555555555555555ull;
  x = (x | (x >> 1)) & 0x3333333333333333ull;
  x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
  x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
  x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
  return (uint32_t)x;
}

// little-endian bytes [p, p + nb) of the page, nb <= 8, never past `end`
template <class Src>
__device__ __forceinline__ uint64_t ld_bytes(const Src& s, uint32_t p, uint32_t nb, uint32_t end) {
  if (p + 8 <= end) return s.u64(p) & (nb >= 8 ? ~0ull : ((1ull << (8 * nb)) - 1));
  uint64_t v = 0;
  for (uint32_t k = 0; k < nb && p + k < end; k++) v |= (uint64_t)s.u8(p + k) << (8 * k);
  return v;
}

// Level masks of 32 consecutive levels [i0, i0 + 32): rsm = row starts
// (rep 0), lfm = leaves (def >= nl + 1), lvm = def > 0, fvm = def > nl + 1.
struct LvMasks {
  uint32_t vm, rsm, lfm, lvm, fvm;
};

// Level masks of a page whose level streams are one bit-packed run each (the
// writer's shape): rep payload at rp, def payload at dp (the rep stream ends
// there), def bit width bw <= 2, level streams end at `region`.
template <class Src>
__device__ __forceinline__ LvMasks fast_level_masks(const Src& s, uint32_t rp, uint32_t dp, uint32_t region, uint32_t bw,
                                                    uint32_t i0, uint32_t L, uint32_t cs1) {
  LvMasks m{0, 0, 0, 0, 0};
  if (i0 >= L) return m;
  m.vm = L - i0 >= 32 ? 0xFFFFFFFFu : ((1u << (L - i0)) - 1);
  const uint32_t repw = (uint32_t)ld_bytes(s, rp + i0 / 8, 4, dp);
  m.rsm = ~repw & m.vm;
  const uint64_t dw = ld_bytes(s, dp + i0 * bw / 8, 4 * bw, region);
  auto ge = [&](uint32_t t) -> uint32_t {
    if (t == 0) return 0xFFFFFFFFu;
    if (bw == 1) return t == 1 ? (uint32_t)dw : 0u;
    const uint32_t lo = compact_even(dw), hi = compact_even(dw >> 1);
    return t == 1 ? (lo | hi) : t == 2 ? hi : (hi & lo);
  };
  m.lfm = ge(cs1) & m.vm;
  m.lvm = ge(1) & m.vm;
  m.fvm = ge(cs1 + 1) & m.vm;
  return m;
}

template <class Src>
__device__ __forceinline__ LvMasks level_masks(const Src& s, const ListShared& ls, uint32_t i0, uint32_t L,
                                               uint32_t cs1) {
  if (ls.fast)  // direct bit slices of the single bit-packed runs
    return fast_level_masks(s, ls.rep.arg[0] & 0x7FFFFFFFu, ls.def.arg[0] & 0x7FFFFFFFu, ls.region, ls.bw_def, i0, L, cs1);
  LvMasks m{0, 0, 0, 0, 0};
  if (i0 >= L) return m;
  m.vm = L - i0 >= 32 ? 0xFFFFFFFFu : ((1u << (L - i0)) - 1);
  const uint32_t bw = ls.bw_def;
  for (uint32_t k = 0; k < 32; k++) {
    const uint32_t i = i0 + k;
    if (i >= L) break;
    const uint32_t r = level_at(s, ls.rep, i, 1), d = level_at(s, ls.def, i, bw);
    if (r == 0) m.rsm |= 1u << k;
    if (r <= 1 && d >= cs1) m.lfm |= 1u << k;
    if (d > 0) m.lvm |= 1u << k;
    if (d > cs1) m.fvm |= 1u << k;
  }
  return m;
}

// OR `nbits` (<= 32) bits of v into the LDS bitmap at bit position pos
__device__ __forceinline__ void lds_or_bits(uint32_t* bm, uint32_t pos, uint64_t v, uint32_t nbits) {
  if (!nbits || !v) return;
  const uint32_t w = pos >> 5, sft = pos & 31;
  const uint64_t lo = v << sft;
  atomicOr(&bm[w], (uint32_t)lo);
  if ((uint32_t)(lo >> 32)) atomicOr(&bm[w + 1], (uint32_t)(lo >> 32));
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}


// n bits of an LDS bitmap (bit 0 at word 0, zero past n, one spare zero word
// before it at bm[-1]) to global bit position g0: the shift is uniform over
// the wave, so output word i is a funnel of bm[i - 1] and bm[i]; interior
// words are stored.  An edge word, shared with the neighbouring range, gets
// its own bits cleared (atomicAnd) and then set (atomicOr): the neighbour's
// bits are never touched, so the bitmap needs no zeroing first.
__device__ __forceinline__ void wave_put_bits(const uint32_t* bm, uint32_t n, uint64_t g0, uint32_t* out) {
  if (n == 0) return;
  const uint32_t sh = (uint32_t)(g0 & 31), nw = (sh + n + 31) >> 5, eb = (sh + n) & 31;
  uint32_t* o = out + (g0 >> 5);
  for (uint32_t i = threadIdx.x & 63; i < nw; i += 64) {
    const uint32_t v = sh ? __builtin_amdgcn_alignbit(bm[i], bm[(int)i - 1], 32 - sh) : bm[i];
    const bool lo_edge = i == 0 && sh, hi_edge = i == nw - 1 && eb;
    if (lo_edge || hi_edge) {
      uint32_t m = lo_edge ? ~0u << sh : ~0u;
      if (hi_edge) m &= (1u << eb) - 1;
      atomicAnd(&o[i], ~m);
      if (v) atomicOr(&o[i], v);
    } else {
      o[i] = v;
    }
  }
}

#ifndef SB_LV_STAGE
#define SB_LV_STAGE 4160
#endif
#ifndef SB_LV_STAGE_PAD
#define SB_LV_STAGE_PAD 16  // (>= 3 dwords: LdsSrc::u64 reads two words past the last staged one)
#endif
constexpr uint32_t kLvStage = SB_LV_STAGE;  // page bytes staged per wave (header + level streams)
constexpr uint32_t kLvStep = 64 * kLvK;  // levels per wave step (2048)

#ifndef SB_LV_ACC_BITS
#define SB_LV_ACC_BITS 8192
#endif
// The page's validity bits accumulate over its steps and go out once per
// kLvAccBits (a C4 page: once), as whole words with two edge merges,
// instead of a short partial-line write and two atomics every step.
constexpr uint32_t kLvAccBits = SB_LV_ACC_BITS;
constexpr uint32_t kLvBitsW = kLvAccBits / 32 + 2;

struct ListWave {
  ListShared ls;
  uint32_t err;
  alignas(16) uint16_t obuf[kLvStep + 8];  // step-relative leaf offset of each row start, at row + (g0 & 3)
  uint32_t lbits[kLvBitsW];   // [0] = 0, then the list-validity bits held (rows)
  uint32_t fbits[kLvBitsW];   // [0] = 0, then the leaf-validity bits held (leaves)
};

// Validity bits held in ListWave.lbits / fbits: r / l bits from global bit
// positions g0 / v0 (uniform over the wave).
struct LvAcc {
  uint32_t r, l;
  uint64_t g0, v0;
};

// Page bytes: the staged prefix from LDS, the rest from HBM.
struct StageSrc {
  LdsSrc l;
  GlbSrc g;
  uint32_t lim;  // staged page bytes
  __device__ __forceinline__ uint32_t u8(uint32_t i) const { return i < lim ? l.u8(i) : g.u8(i); }
  __device__ __forceinline__ uint32_t u32(uint32_t i) const { return i + 4 <= lim ? l.u32(i) : g.u32(i); }
  __device__ __forceinline__ uint64_t u64(uint32_t i) const { return i + 8 <= lim ? l.u64(i) : g.u64(i); }
};

// Hacker's Delight 7-4 compress: the bits of x at the set positions of m,
// packed to the low end (a branch-free pext).
__device__ __forceinline__ uint32_t compress32(uint32_t x, uint32_t m) {
  x &= m;
  uint32_t mk = ~m << 1;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    uint32_t mp = mk ^ (mk << 1);
    mp ^= mp << 2;
    mp ^= mp << 4;
    mp ^= mp << 8;
    mp ^= mp << 16;
    const uint32_t mv = mp & m;
    m = (m ^ mv) | (mv >> (1 << i));
    const uint32_t t = x & mv;
    x = (x ^ t) | (t >> (1 << i));
    mk &= ~mp;
  }
  return x;
}

// The held validity bits to the bitmaps; the buffers zeroed again.
__device__ __forceinline__ void lv_flush(ListWave& w, const ListArgs& a, LvAcc& acc) {
  const uint32_t lane = threadIdx.x & 63;
#ifndef SB_V_LV_NOBITS
  if (a.nl) wave_put_bits(w.lbits + 1, acc.r, acc.g0, a.out_list_validity);
  if (a.ni) wave_put_bits(w.fbits + 1, acc.l, acc.v0, a.out_leaf_validity);
#endif
  wave_sync();
  const uint32_t nw = (max(acc.r, acc.l) + 31) / 32 + 2;
  for (uint32_t i = lane; i < nw; i += 64) w.lbits[i] = w.fbits[i] = 0;
  wave_sync();
  acc.g0 += acc.r;
  acc.v0 += acc.l;
  acc.r = acc.l = 0;
}

// One step of kLvStep levels [t0, t0 + kLvStep) of a page, one wave, rows
// and leaves before it = (carry_r, carry_l).  *step_r / *step_l: the step's
// row starts and leaves (all levels); the return value: leaves consumed
// (levels whose inclusive row count stays <= rows, read_basic.rs:158-162).
// WRITE: offsets and bitmaps at (rbase, lbase).
// (m: this lane's masks of levels t0 + 32 lane ..; rows: the page's rows.)
template <bool WRITE, class WV>
__device__ uint32_t lv_step_m(const LvMasks m, WV& w, uint32_t rows, const ListArgs& a, uint32_t t0, uint64_t rbase,
                              uint64_t lbase, uint32_t carry_r, uint32_t carry_l, uint32_t* step_r, uint32_t* step_l,
                              LvAcc& acc) {
  const uint32_t lane = threadIdx.x & 63;
  if (t0 == 0 && lane == 0 && !(m.rsm & 1)) put_err(&w.err, ST_OUT_OF_SPEC);  // level 0 starts no row
  const uint32_t pk = ((uint32_t)__popc(m.rsm) << 16) | (uint32_t)__popc(m.lfm);
  const uint32_t incl = wave_incl_scan(pk), tot = __builtin_amdgcn_readlane(incl, 63), ex = incl - pk;
  const uint32_t rb = carry_r + (ex >> 16), lb = carry_l + (ex & 0xFFFFu);
  uint32_t cm = m.vm;
  if (rb + __popc(m.rsm) > rows) {
    if (rb >= rows + 1) cm = 0;
    else {  // cut at the (rows - rb + 1)-th row start
      uint32_t x = m.rsm;
      for (uint32_t k = rows - rb; k; k--) x &= x - 1;
      cm = (x & (0u - x)) - 1;
    }
  }
  const uint32_t rsm = m.rsm & cm, lfm = m.lfm & cm;
  if constexpr (WRITE) {
    const uint32_t s_r0 = carry_r, s_l0 = carry_l;
    const uint64_t g0 = rbase + s_r0, v0 = lbase + s_l0;
    const uint32_t al = a.ow == 4 ? (uint32_t)(g0 & 3) : (uint32_t)(g0 & 1);  // obuf index of row 0
    if (acc.r + (tot >> 16) > kLvAccBits || acc.l + (tot & 0xFFFFu) > kLvAccBits) lv_flush(w, a, acc);
    const uint32_t pr = acc.r + rb - s_r0, pf = acc.l + lb - s_l0;
    const uint32_t nr = __popc(rsm), nf = __popc(lfm);
    uint16_t* ob = w.obuf + al + (rb - s_r0);
    const uint32_t lrel = lb - s_l0;
    uint32_t j = 0;
#ifndef SB_V_LV_NOOB
    for (uint32_t x = rsm; x; x &= x - 1, j++) ob[j] = (uint16_t)(lrel + __popc(m.lfm & ((x & (0u - x)) - 1)));
#endif
    if (a.nl) lds_or_bits(w.lbits + 1, pr, compress32(m.lvm, rsm), nr);
    if (a.ni) lds_or_bits(w.fbits + 1, pf, compress32(m.fvm, lfm), nf);
    const uint32_t cpk = (nr << 16) | nf;
    const uint32_t ctot = __builtin_amdgcn_readlane(wave_incl_scan(cpk), 63);
    const uint32_t tr = ctot >> 16, tl = ctot & 0xFFFFu;
    wave_sync();
#ifdef SB_V_LV_NOOFF
    constexpr bool wr_off = false;
#else
    constexpr bool wr_off = true;
#endif
    if (!wr_off) {
    } else if (a.ow == 4) {  // quads of rows on 16-byte boundaries: obuf[4q .. 4q + 3] -> o[4q - al ..]
      uint32_t* o = (uint32_t*)a.out_offsets + (g0 - al);
      const uint32_t v32 = (uint32_t)v0, nq = (al + tr + 3) >> 2;
      for (uint32_t q = lane; q < nq; q += 64) {
        const uint32_t* pr = (const uint32_t*)(w.obuf + 4 * q);
        const uint32_t px = pr[0], py = pr[1];
        const uint32_t e0 = v32 + (px & 0xFFFFu), e1 = v32 + (px >> 16), e2 = v32 + (py & 0xFFFFu), e3 = v32 + (py >> 16);
        const uint32_t j0 = 4 * q;
        if (j0 >= al && j0 + 4 <= al + tr) {
          st_out((u32x4*)(o + j0), u32x4{e0, e1, e2, e3});
        } else {
          const uint32_t e[4] = {e0, e1, e2, e3};
#pragma unroll
          for (uint32_t k = 0; k < 4; k++)
            if (j0 + k >= al && j0 + k < al + tr) o[j0 + k] = e[k];
        }
      }
    } else {
      uint64_t* o = (uint64_t*)a.out_offsets + (g0 - al);
      const uint32_t nq = (al + tr + 1) >> 1;
      for (uint32_t q = lane; q < nq; q += 64) {
        const uint32_t j0 = 2 * q;
        const uint64_t x0 = v0 + w.obuf[j0], x1 = v0 + w.obuf[j0 + 1];
        if (j0 >= al && j0 + 2 <= al + tr) {
          st_out((u32x4*)(o + j0), u32x4{(uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32)});
        } else {
          if (j0 >= al && j0 < al + tr) o[j0] = x0;
          if (j0 + 1 >= al && j0 + 1 < al + tr) o[j0 + 1] = x1;
        }
      }
    }
    acc.r += tr;
    acc.l += tl;
    wave_sync();
  }
  *step_r = tot >> 16;
  *step_l = tot & 0xFFFFu;
  return __builtin_amdgcn_readlane(wave_incl_scan(__popc(lfm)), 63);  // DPP, not a permute chain
}

template <bool WRITE, class Src>
__device__ __forceinline__ uint32_t lv_step(const Src& s, ListWave& w, const ListShared& ls, const ListArgs& a,
                                            uint32_t t0, uint32_t L, uint64_t rbase, uint64_t lbase, uint32_t carry_r,
                                            uint32_t carry_l, uint32_t* step_r, uint32_t* step_l, LvAcc& acc) {
  const LvMasks m = level_masks(s, ls, t0 + (threadIdx.x & 63) * kLvK, L, a.nl + 1);
  return lv_step_m<WRITE>(m, w, ls.rows, a, t0, rbase, lbase, carry_r, carry_l, step_r, step_l, acc);
}

// One wave walks its page's levels a step at a time (the sizing pass).
template <bool WRITE, class Src>
__device__ void wave_levels(const Src& s, ListWave& w, const ListArgs& a, uint32_t L, uint64_t rbase, uint64_t lbase,
                            uint32_t* rows_c, uint32_t* leaves_c) {
  const uint32_t lane = threadIdx.x & 63, rows = w.ls.rows;
  uint32_t carry_r = 0, carry_l = 0, leaves = 0;
  LvAcc acc{0, 0, rbase, lbase};
  if constexpr (WRITE) {
    for (uint32_t i = lane; i < kLvBitsW; i += 64) w.lbits[i] = w.fbits[i] = 0;
    wave_sync();
  }
  for (uint32_t t0 = 0; t0 < L; t0 += kLvStep) {
    uint32_t sr, sl;
    leaves += lv_step<WRITE>(s, w, w.ls, a, t0, L, rbase, lbase, carry_r, carry_l, &sr, &sl, acc);
    carry_r += sr;
    carry_l += sl;
    if (carry_r > rows) break;  // uniform: every later level is past the last row
  }
  if constexpr (WRITE) lv_flush(w, a, acc);
  const uint32_t rc = min(carry_r, rows);
  if (lane == 0 && rc != rows) put_err(&w.err, ST_OUT_OF_SPEC);  // levels ended before `rows` rows
  *rows_c = rc;
  *leaves_c = leaves;
}

// Row starts and leaves of the step at t0 (all its levels), one wave.
template <class Src>
__device__ __forceinline__ uint32_t lv_count(const Src& s, const ListShared& ls, uint32_t t0, uint32_t L, uint32_t cs1) {
  const LvMasks m = level_masks(s, ls, t0 + (threadIdx.x & 63) * kLvK, L, cs1);
  const uint32_t pk = ((uint32_t)__popc(m.rsm) << 16) | (uint32_t)__popc(m.lfm);
  return __builtin_amdgcn_readlane(wave_incl_scan(pk), 63);  // rows < 2^16 per 2048-level step
}

// Per page setup of one wave: the page's first kLvStage bytes staged in LDS
// in one round of loads (the header and, for the writer's pages, both level
// streams), then the header parse -- or, on the levels pass of a fast page,
// the descriptor the sizing pass left.  *staged: the level streams lie in
// the staged prefix.  Returns false on a parse error.
__device__ bool wave_page_setup(ListWave& w, uint32_t* stage, const ListArgs& a, uint32_t page, const PageDesc& pd, bool reuse,
                                bool* staged, uint32_t* mis_out, uint32_t* lim_out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint8_t* pg = a.chunk + pd.byte_off;
  const uintptr_t a0 = (uintptr_t)pg & ~(uintptr_t)3;
  const uint32_t mis = (uint32_t)((uintptr_t)pg & 3);
  const uint32_t lim = stage ? min(pd.byte_len, kLvStage) : 0u;
  const uint32_t ndw = (mis + lim + 3) >> 2;
  uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
  if (reuse) {
    d0 = a.lvdesc[2 * page];
    d1 = a.lvdesc[2 * page + 1];
  }
  if (stage) {  // every load issued before the first LDS store (one round trip, not one per 64 dwords)
    typedef const __attribute__((address_space(1))) uint32_t g32;
    constexpr uint32_t kIt = (kLvStage / 4 + 2 + 63) / 64;
    uint32_t v[kIt];
#pragma unroll
    for (uint32_t k = 0; k < kIt; k++) {
      const uint32_t d = lane + 64 * k;
      v[k] = d < ndw ? __builtin_nontemporal_load((g32*)a0 + d) : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < kIt; k++)
      if (lane + 64 * k < ndw) stage[lane + 64 * k] = v[k];
  }
  if (lane == 0) w.err = 0;
  wave_sync();
  *mis_out = mis;
  *lim_out = lim;
  if (reuse && (d0.w & 1)) {  // fast page: one bit-packed run per stream
    if (lane == 0) {
      w.ls.rows = d0.x;
      w.ls.vpos = d0.y;
      w.ls.region = d0.y;
      w.ls.bw_def = d0.w >> 1;
      w.ls.fast = 1;
      w.ls.rep.n = w.ls.def.n = 1;
      w.ls.rep.start[0] = w.ls.def.start[0] = 0;
      w.ls.rep.arg[0] = 0x80000000u | d0.z;
      w.ls.def.arg[0] = 0x80000000u | d1.x;
    }
  } else if (lane == 0) {
    const StageSrc ss{LdsSrc{stage, mis}, GlbSrc{pg}, lim};
    list_parse(ss, &w.err, w.ls, pd, a);
  }
  wave_sync();
  if (w.err) return false;
  *staged = w.ls.region <= lim;
  return true;
}

// Exact sizing pass: one wave per page (4 per workgroup) walks the levels:
// consumed rows / leaves, and the parse results for the levels pass.
__global__ __launch_bounds__(NT) void k_list_size(ListArgs a) {
  __shared__ ListWave waves[NW];
  __shared__ uint32_t stages[NW][kLvStage / 4 + SB_LV_STAGE_PAD];  // the page's first bytes at byte `mis` (+ pad)
  const uint32_t lane = threadIdx.x & 63;
  ListWave& w = waves[threadIdx.x >> 6];
  uint32_t* stage = stages[threadIdx.x >> 6];
  for (uint32_t page = blockIdx.x * NW + (threadIdx.x >> 6); page < a.n_pages; page += gridDim.x * NW) {
    const PageDesc pd = a.pages[page];
    bool staged = false;
    uint32_t mis = 0, lim = 0, rows_c = 0, leaves_c = 0;
    if (wave_page_setup(w, stage, a, page, pd, false, &staged, &mis, &lim)) {
      if (staged) wave_levels<false>(LdsSrc{stage, mis}, w, a, pd.num_values, 0, 0, &rows_c, &leaves_c);
      else wave_levels<false>(GlbSrc{a.chunk + pd.byte_off}, w, a, pd.num_values, 0, 0, &rows_c, &leaves_c);
    }
    wave_sync();
    if (lane == 0) {
      const bool ok = w.err == 0;
      a.counts[page] = ok ? (((uint64_t)rows_c << 32) | leaves_c) : 0;
      const uint32_t fast = ok && w.ls.fast;
      a.lvdesc[2 * page] = make_uint4(w.ls.rows, w.ls.vpos, w.ls.rep.arg[0] & 0x7FFFFFFFu, fast | (w.ls.bw_def << 1));
      a.lvdesc[2 * page + 1] = make_uint4(w.ls.def.arg[0] & 0x7FFFFFFFu, ok, 0, 0);
      a.status[page] = w.err;
    }
    wave_sync();
  }
}

// Block bases: one workgroup per NT pages, one thread per page.  a.peek:
// the page's counts come straight from its headers -- rows from the nested
// header (read_basic.rs:71, `additional`), leaves from the values stream's
// usize = leaves * width (integer/mod.rs:62-63) -- two small reads per page
// instead of a walk over its levels; the plan only takes this path after
// checking it against the exact pass page by page.  Otherwise the counts of
// k_list_size.  Writes each page's bases within its block and the block totals.
__global__ __launch_bounds__(NT) void k_list_bscan(ListArgs a) {
  __shared__ Shared sh;
  const uint32_t p = blockIdx.x * NT + threadIdx.x;
  uint64_t c = 0;
  if (p < a.n_pages) {
    if (a.peek) {
      const PageDesc pd = a.pages[p];
      const GlbSrc g{a.chunk + pd.byte_off};
      if (pd.byte_len >= 12) {
        const uint64_t vpos = 12ull + g.u32(4) + g.u32(8);
        if (vpos + 9 <= pd.byte_len) c = ((uint64_t)g.u32(0) << 32) | (g.u32((uint32_t)vpos + 5) / a.width);
      }
      a.counts[p] = c;
    } else {
      c = a.counts[p];
    }
  }
  uint64_t tr, tl;
  const uint64_t er = block_excl_scan<uint64_t>(c >> 32, sh, &tr);
  const uint64_t el = block_excl_scan<uint64_t>(c & 0xFFFFFFFFull, sh, &tl);
  if (p < a.n_pages) {
    a.local[2 * p] = er;
    a.local[2 * p + 1] = el;
  }
  if (threadIdx.x == 0) {
    a.blk[2 * blockIdx.x] = tr;
    a.blk[2 * blockIdx.x + 1] = tl;
  }
}

// A decode's sizing in one launch: page counts (from the headers with
// a.peek, else the exact pass's), block scans and global bases, and each
// page's values-stream descriptor (a.peek), so the values decode needs
// nothing from k_list_levels.  Block b < nblk scans its NT pages' counts, publishes its
// row / leaf totals as two words of blk tagged with a.epoch (top 16 bits),
// and sums the totals of blocks 0..b-1 -- every predecessor's own total, no
// inclusive prefixes, so no block waits on another's wait: the lower blocks
// were dispatched first (workgroups launch in order on each XCD), each
// publishes as soon as its scan is done.  A stale word (an earlier decode's
// tag, or the plan's zeroed state) reads as not yet published.  The bitmaps
// need no zeroing (k_list_levels clears and sets only the bits it owns), but
// for the bits past the column's last row / leaf: the last page's thread
// zeroes the final word of each bitmap before k_list_levels runs.
__global__ __launch_bounds__(NT) void k_list_bases(ListArgs a) {
  __shared__ Shared sh;
  __shared__ uint64_t red[2][NW];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t p = blockIdx.x * NT + tid;
  uint64_t c = 0;
  uint64_t vpos = ~0ull;
  PageDesc pd{};
  if (p < a.n_pages) {
    if (a.peek) {
      pd = a.pages[p];
      const GlbSrc g{a.chunk + pd.byte_off};
      if (pd.byte_len >= 12) {
        vpos = 12ull + g.u32(4) + g.u32(8);
        if (vpos + 9 <= pd.byte_len) c = ((uint64_t)g.u32(0) << 32) | (g.u32((uint32_t)vpos + 5) / a.width);
      }
      a.counts[p] = c;
    } else {
      c = a.counts[p];
    }
  }
  uint64_t tr, tl;
  const uint64_t er = block_excl_scan<uint64_t>(c >> 32, sh, &tr);
  const uint64_t el = block_excl_scan<uint64_t>(c & 0xFFFFFFFFull, sh, &tl);
  constexpr uint64_t kVal = (1ull << 48) - 1;
  const uint64_t tag = (uint64_t)a.epoch << 48;
  if (tid == 0) {
    __hip_atomic_store(&a.blk[2 * blockIdx.x], tag | tr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.blk[2 * blockIdx.x + 1], tag | tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (wv == 0) {  // the totals of blocks 0..b-1, 64 blocks a probe
    uint64_t br = 0, bl = 0;
    for (uint32_t b0 = 0; b0 < blockIdx.x; b0 += 64) {
      const uint32_t b = b0 + lane;
      const bool need = b < blockIdx.x;
      uint64_t r = 0, l = 0;
      for (;;) {
        if (need) {
          r = __hip_atomic_load(&a.blk[2 * b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          l = __hip_atomic_load(&a.blk[2 * b + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!__ballot(need && ((r & ~kVal) != tag || (l & ~kVal) != tag))) break;
        __builtin_amdgcn_s_sleep(1);
      }
      if (need) {
        br += r & kVal;
        bl += l & kVal;
      }
    }
    br = wave_sum64(br);
    bl = wave_sum64(bl);
    if (lane == 0) {
      red[0][0] = br;
      red[1][0] = bl;
    }
  }
  __syncthreads();
  if (p < a.n_pages) {
    const uint64_t rbase = red[0][0] + er, lbase = red[1][0] + el;
    a.local[2 * p] = rbase;
    a.local[2 * p + 1] = lbase;
    if (p == a.n_pages - 1) {
      const uint64_t tr_all = rbase + (c >> 32), tl_all = lbase + (c & 0xFFFFFFFFull);
      if (a.nl && a.out_list_validity && (tr_all & 31)) a.out_list_validity[tr_all >> 5] = 0;
      if (a.ni && a.out_leaf_validity && (tl_all & 31)) a.out_leaf_validity[tl_all >> 5] = 0;
    }
    if (a.peek) {
      const bool ok = vpos + 9 <= pd.byte_len;
      a.vpages[p] = PageDesc{pd.byte_off + (ok ? vpos : 0), lbase, ok ? pd.byte_len - (uint32_t)vpos : 0,
                             ok ? (uint32_t)c : 0, a.vpages[p].reserved};
    }
  }
}

// Levels pass: one wave per page, at the global bases k_list_bases wrote.
// Writes offsets and both bitmaps, its status, and (unless the values
// descriptors came from the headers) the page's values-stream descriptor;
// the last page also the totals and the final offset.
__global__ __launch_bounds__(NT) void k_list_levels(ListArgs a) {
  __shared__ ListWave waves[NW];
  __shared__ uint32_t stages[NW][kLvStage / 4 + SB_LV_STAGE_PAD];  // the page's first bytes at byte `mis` (+ pad)
  const uint32_t lane = threadIdx.x & 63;
  ListWave& w = waves[threadIdx.x >> 6];
  uint32_t* stage = stages[threadIdx.x >> 6];
  for (uint32_t page = blockIdx.x * NW + (threadIdx.x >> 6); page < a.n_pages; page += gridDim.x * NW) {
    const PageDesc pd = a.pages[page];
    const uint64_t rbase = a.local[2 * page], lbase = a.local[2 * page + 1];
    const uint64_t cnt = a.counts[page];
    bool staged = false;
    uint32_t mis = 0, lim = 0, rows_c = 0, leaves_c = 0;
    const bool sized = a.lvdesc[2 * page + 1].y != 0;  // the exact pass parsed this page
    if (sized && wave_page_setup(w, stage, a, page, pd, true, &staged, &mis, &lim)) {
      if (staged) wave_levels<true>(LdsSrc{stage, mis}, w, a, pd.num_values, rbase, lbase, &rows_c, &leaves_c);
      else wave_levels<true>(GlbSrc{a.chunk + pd.byte_off}, w, a, pd.num_values, rbase, lbase, &rows_c, &leaves_c);
    } else if (lane == 0) {
      w.err = 0;
      if (!sized) {  // re-parse for the status the reference would give
        const StageSrc ss{LdsSrc{nullptr, 0}, GlbSrc{a.chunk + pd.byte_off}, 0};
        list_parse(ss, &w.err, w.ls, pd, a);
        if (!w.err) w.err = ST_OUT_OF_SPEC;
      }
    }
    wave_sync();
    if (lane == 0) {
      uint32_t err = w.err;
      if (!err && (rows_c != (uint32_t)(cnt >> 32) || leaves_c != (uint32_t)cnt)) err = ST_OUT_OF_SPEC;
      const bool ok = err == 0;
      // the page's values stream, decoded as a flat non-nullable page of `leaves` values
      if (!a.peek)
        a.vpages[page] = PageDesc{pd.byte_off + (ok ? w.ls.vpos : 0), lbase, ok ? pd.byte_len - w.ls.vpos : 0,
                                  ok ? leaves_c : 0, a.vpages[page].reserved};
      a.status[page] = err;
      if (page == a.n_pages - 1) {
        const uint64_t tr = rbase + (cnt >> 32), tl = lbase + (uint32_t)cnt;
        a.totals[0] = tr;
        a.totals[1] = tl;
        if (a.out_offsets) bin_put_off(a.out_offsets, tr, tl, a.ow);  // create_list appends values.len()
      }
    }
    wave_sync();
  }
}

// ===========================================================================
// General nesting: a leaf under `depth` nests (List / Map / Struct chains,
// the InitNested chain of read/deserialize.rs:140-233),
// read_validity_nested (read/read_basic.rs:95-164) level by level: nests
// 0..depth-1 are lists (repeated; nullable per level) or, where bit d of
// struct_mask is set, structs (not repeated; arrow2's NestedStruct /
// NestedStructValid are "required"), nest `depth` the primitive; cum_sum /
// cum_rep over (nullable + repeated) / repeated; a nest is pushed when
// rep <= cum_rep[d] && def >= cum_sum[d], or when the nest above is a struct
// that was pushed and is not valid (the is_required chain, :118-137: every
// child of a null struct gets a slot).  One wave per page, one level per
// lane per step: each lane runs the chain over its level, ballots give each
// nest's pushes and ranks; a list push's offset is its child's running
// count; validity bits are compacted to push order and OR-ed into the
// (zeroed) bitmaps.  A zero-width level stream (max level 0: a chain of
// required structs writes none) reads as all zeros, as parquet2's
// HybridRleDecoder does with num_bits 0.
// ===========================================================================
struct NestArgs {
  const uint8_t* chunk;
  const PageDesc* pages;
  uint32_t n_pages, depth, nullable, ow, smask;
  uint64_t* counts;
  const uint64_t* bases;
  const uint64_t* totals;
  PageDesc* vpages;
  uint8_t* out_offsets[kMaxNest];
  uint32_t* out_validity[kMaxNest];
  uint32_t* out_leaf_validity;
  uint32_t* status;
  uint32_t* vpos;
};

// A window of hybrid runs (parquet2 HybridRleDecoder) over the levels of the
// current 64-level step, parsed incrementally by one lane: the run holding
// the step's first level plus every run up to the step's end (each run
// covers >= 1 level, so <= 65 entries), so a stream may hold any number of
// runs (pyarrow's writer mixes many RLE and bit-packed runs).
struct RunWin {
  uint32_t n, p, end, covered, bw;
  uint32_t start[68];
  uint32_t arg[68];  // bit-packed: 0x80000000 | payload position; RLE: the value
};

// lane 0: make the window cover levels [l0, lend)
__device__ bool runwin_advance(const GlbSrc& s, RunWin& R, uint32_t l0, uint32_t lend, uint32_t* err) {
  if (R.bw == 0) {  // no stream: one RLE run of zeros over every level
    R.n = 1;
    R.start[0] = 0;
    R.arg[0] = 0;
    R.covered = 0xFFFFFFFFu;
    R.start[1] = R.covered;
    return true;
  }
  uint32_t k = R.n;
  while (k > 0 && R.start[k - 1] > l0) k--;
  if (k > 1) {  // keep the run holding l0
    for (uint32_t i = k - 1; i < R.n; i++) {
      R.start[i - (k - 1)] = R.start[i];
      R.arg[i - (k - 1)] = R.arg[i];
    }
    R.n -= k - 1;
  }
  while (R.covered < lend) {
    if (R.n >= 66) { put_err(err, ST_NYI); return false; }
    uint32_t h = 0, sft = 0;
    for (;;) {  // ULEB128 header
      if (R.p >= R.end || sft > 28) { put_err(err, ST_OUT_OF_SPEC); return false; }
      const uint32_t c = s.u8(R.p++);
      h |= (c & 0x7Fu) << sft;
      if (!(c & 0x80)) break;
      sft += 7;
    }
    uint32_t cnt, arg;
    if (h & 1) {  // bit-packed: h >> 1 groups of 8, clamped to the bytes present
      const uint64_t want = (uint64_t)(h >> 1) * R.bw;
      const uint32_t have = (uint32_t)min<uint64_t>(want, R.end - R.p);
      cnt = (uint32_t)min<uint64_t>((uint64_t)(h >> 1) * 8, (uint64_t)have * 8 / max(R.bw, 1u));
      arg = 0x80000000u | R.p;
      R.p += have;
    } else {  // RLE: h >> 1 repeats of a ceil(bw / 8)-byte value
      const uint32_t vb = (R.bw + 7) / 8;
      if (R.p + vb > R.end) { put_err(err, ST_OUT_OF_SPEC); return false; }
      arg = 0;
      for (uint32_t b = 0; b < vb; b++) arg |= s.u8(R.p + b) << (8 * b);
      R.p += vb;
      cnt = h >> 1;
    }
    if (cnt == 0) continue;  // an empty run yields no levels
    R.start[R.n] = R.covered;
    R.arg[R.n] = arg;
    R.n++;
    R.covered += cnt;
  }
  R.start[R.n] = R.covered;
  return true;
}

__device__ __forceinline__ uint32_t runwin_at(const GlbSrc& s, const RunWin& R, uint32_t i) {
  uint32_t lo = 0, hi = R.n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (R.start[mid] <= i) lo = mid; else hi = mid;
  }
  const uint32_t a = R.arg[lo];
  if (!(a & 0x80000000u)) return a;
  const uint32_t bit = (i - R.start[lo]) * R.bw;
  return (s.u32((a & 0x7FFFFFFFu) + (bit >> 3)) >> (bit & 7)) & ((1u << R.bw) - 1);
}

struct NestWave {
  RunWin rep, def;
  uint32_t err, rows, vpos;
};

__device__ __forceinline__ uint64_t compress64(uint64_t v, uint64_t m) {
  const uint32_t lo = compress32((uint32_t)v, (uint32_t)m), hi = compress32((uint32_t)(v >> 32), (uint32_t)(m >> 32));
  return (uint64_t)lo | ((uint64_t)hi << __popc((uint32_t)m));
}

// n (<= 64) bits at bit position pos of a zeroed bitmap, OR-ed (lanes 0..2)
__device__ __forceinline__ void put_bits64(uint32_t* bm, uint64_t pos, uint64_t v, uint32_t n) {
  const uint32_t lane = threadIdx.x & 63;
  if (!n || !v || lane > 2) return;
  const uint32_t sh = (uint32_t)(pos & 31);
  const uint64_t w0 = pos >> 5;
  const uint32_t word = lane == 0 ? (uint32_t)(v << sh)
                      : lane == 1 ? (uint32_t)(sh ? (v >> (32 - sh)) : (v >> 32))
                                  : (uint32_t)(sh ? (v >> (64 - sh)) : 0u);
  if (word) atomicOr(&bm[w0 + lane], word);
}

template <bool WRITE>
__global__ __launch_bounds__(NT) void k_nest_walk(NestArgs a) {
  __shared__ NestWave waves[NW];
  const uint32_t lane = threadIdx.x & 63, D = a.depth;
  NestWave& w = waves[threadIdx.x >> 6];
  uint32_t cum_sum[kMaxNest + 2], cum_rep[kMaxNest + 2];
  cum_sum[0] = cum_rep[0] = 0;
  for (uint32_t d = 0; d <= D; d++) {
    const uint32_t nl = (a.nullable >> d) & 1, rp = (d < D && !((a.smask >> d) & 1)) ? 1u : 0u;
    cum_sum[d + 1] = cum_sum[d] + nl + rp;
    cum_rep[d + 1] = cum_rep[d] + rp;
  }
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (uint32_t page = blockIdx.x * NW + (threadIdx.x >> 6); page < a.n_pages; page += gridDim.x * NW) {
    const PageDesc pd = a.pages[page];
    const GlbSrc s{a.chunk + pd.byte_off};
    const uint32_t L = pd.num_values;
    if (lane == 0) {
      w.err = 0;
      const uint32_t len = pd.byte_len;
      if (len < 12) {
        w.err = ST_IO;
      } else {
        const uint32_t rows = s.u32(0), rl = s.u32(4), dl = s.u32(8);
        if ((uint64_t)12 + rl + dl > len) {
          w.err = ST_IO;
        } else {
          w.rows = rows;
          w.vpos = 12 + rl + dl;
          w.rep = RunWin{0, 12, 12 + rl, 0, 32u - __clz(cum_rep[D + 1])};
          w.def = RunWin{0, 12 + rl, 12 + rl + dl, 0, 32u - __clz(cum_sum[D + 1])};
          if (L > 0 && rows == 0) w.err = ST_OUT_OF_SPEC;
        }
      }
    }
    wave_sync();
    uint64_t carry[kMaxNest + 1] = {0, 0, 0, 0, 0}, base[kMaxNest + 1] = {0, 0, 0, 0, 0};
    if (WRITE)
      for (uint32_t d = 0; d <= D; d++) base[d] = a.bases[(uint64_t)page * (D + 1) + d];
    uint32_t rows_seen = 0;
    const uint32_t rows = w.rows;
    if (!w.err) {
      for (uint32_t l0 = 0; l0 < L; l0 += 64) {
        if (lane == 0 && runwin_advance(s, w.rep, l0, min(l0 + 64, L), &w.err))
          runwin_advance(s, w.def, l0, min(l0 + 64, L), &w.err);
        wave_sync();
        if (w.err) break;
        const uint32_t l = l0 + lane;
        const bool in = l < L;
        const uint32_t r = in ? runwin_at(s, w.rep, l) : 0u, dv = in ? runwin_at(s, w.def, l) : 0u;
        if (l == 0 && r != 0) w.err = ST_OUT_OF_SPEC;  // the first level starts no row
        const uint64_t rs = __ballot(in && r == 0);
        // consumed: inclusive row count <= rows (read_basic.rs:150-162)
        const bool cons = in && rows_seen + (uint32_t)__popcll(rs & (below | (1ull << lane))) <= rows;
        uint64_t push[kMaxNest + 1];
        bool forced = false;  // the is_required chain: the nest above is a struct pushed invalid
        for (uint32_t d = 0; d <= D; d++) {
          const bool me = cons && (forced || (r <= cum_rep[d] && dv >= cum_sum[d]));
          push[d] = __ballot(me);
          forced = me && ((a.smask >> d) & 1) && !(((a.nullable >> d) & 1) && dv > cum_sum[d]);
        }
        if (WRITE) {
          for (uint32_t d = 0; d <= D; d++) {
            const bool me = (push[d] >> lane) & 1;
            const uint64_t pos = base[d] + carry[d] + (uint32_t)__popcll(push[d] & below);
            if (d < D && me && !((a.smask >> d) & 1)) {  // list offset = the child's count before this level
              const uint64_t v = base[d + 1] + carry[d + 1] + (uint32_t)__popcll(push[d + 1] & below);
              bin_put_off(a.out_offsets[d], pos, v, (int)a.ow);
            }
            if ((a.nullable >> d) & 1) {
              const uint64_t vm = __ballot(me && dv > cum_sum[d]);
              const uint32_t np = (uint32_t)__popcll(push[d]);
              uint32_t* bm = d < D ? a.out_validity[d] : a.out_leaf_validity;
              put_bits64(bm, base[d] + carry[d], compress64(vm, push[d]), np);
            }
            (void)pos;
          }
        }
        for (uint32_t d = 0; d <= D; d++) carry[d] += (uint32_t)__popcll(push[d]);
        rows_seen += (uint32_t)__popcll(rs);
        if (rows_seen > rows) break;  // every later level is past the last row
      }
      if (lane == 0 && min(rows_seen, rows) != rows) w.err = ST_OUT_OF_SPEC;  // levels ended early
    }
    wave_sync();
    if (lane == 0) {
      uint32_t err = w.err;
      if (!WRITE) {
        for (uint32_t d = 0; d <= D; d++) a.counts[(uint64_t)page * (D + 1) + d] = err ? 0 : carry[d];
        a.vpos[page] = err ? 0u : w.vpos;
      } else {
        for (uint32_t d = 0; d <= D; d++)
          if (!err && carry[d] != a.counts[(uint64_t)page * (D + 1) + d]) err = ST_OUT_OF_SPEC;
        const bool ok = err == 0;
        a.vpages[page] = PageDesc{pd.byte_off + (ok ? w.vpos : 0), base[D], ok ? pd.byte_len - w.vpos : 0,
                                  ok ? (uint32_t)carry[D] : 0u, a.vpages[page].reserved};
        if (page == a.n_pages - 1)  // create_list / create_map append each child's length
          for (uint32_t d = 0; d < D; d++)
            if (!((a.smask >> d) & 1)) bin_put_off(a.out_offsets[d], a.totals[d], a.totals[d + 1], (int)a.ow);
      }
      a.status[page] = err;
    }
    wave_sync();
  }
}

}  // namespace sbk

namespace sb {
int launch_list(int stage, const ListLaunch& L, void* stream) {
  sbk::ListArgs a{L.chunk, L.pages, L.n_pages, L.list_nullable, L.item_nullable, L.offset_width, L.width, L.peek,
                  L.counts, L.local, L.blk, L.totals, (uint4*)L.lvdesc, L.vpages, L.out_offsets, L.out_list_validity,
                  L.out_leaf_validity, L.status, L.epoch};
  if (L.n_pages == 0) return 0;
  const uint32_t grid = std::min<uint32_t>((L.n_pages + sbk::NW - 1) / sbk::NW, kListGrid);
  const uint32_t nblk = (L.n_pages + sbk::NT - 1) / sbk::NT;
  hipStream_t st = (hipStream_t)stream;
  if (stage == 0) {  // exact sizing
    hipLaunchKernelGGL(sbk::k_list_size, dim3(grid), dim3(sbk::NT), 0, st, a);
  } else if (stage == 1) {  // block bases (+ header sizing when peek)
    hipLaunchKernelGGL(sbk::k_list_bscan, dim3(nblk), dim3(sbk::NT), 0, st, a);
  } else if (stage == 4) {  // counts, global bases, values descriptors (peek)
    hipLaunchKernelGGL(sbk::k_list_bases, dim3(nblk), dim3(sbk::NT), 0, st, a);
  } else {
    hipLaunchKernelGGL(sbk::k_list_levels, dim3(grid), dim3(sbk::NT), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace sb

namespace sb {
int launch_nest(int stage, const NestLaunch& L, void* stream) {
  if (L.n_pages == 0) return 0;
  sbk::NestArgs a{L.chunk, L.pages, L.n_pages, L.depth, L.nullable, L.offset_width, L.struct_mask, L.counts, L.bases, L.totals,
                  L.vpages, {}, {}, L.out_leaf_validity, L.status, L.vpos};
  for (int d = 0; d < kMaxNest; d++) {
    a.out_offsets[d] = L.out_offsets[d];
    a.out_validity[d] = L.out_validity[d];
  }
  const uint32_t grid = std::min<uint32_t>((L.n_pages + sbk::NW - 1) / sbk::NW, kListGrid);
  if (stage == 0) hipLaunchKernelGGL(sbk::k_nest_walk<false>, dim3(grid), dim3(sbk::NT), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(sbk::k_nest_walk<true>, dim3(grid), dim3(sbk::NT), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace sb
