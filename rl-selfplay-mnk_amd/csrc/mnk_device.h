// mnk_device.h -- device-side building blocks shared by the MNK kernels (gfx950 only).
//
// One lane owns one env.  A board plane is a bit string in the guard-column layout of
// include/mnk_hip.h, held in registers as NW 32-bit words (9x9: 90 bits = 3 VGPRs per
// plane; in memory it stays u64[W], the unused top half-word is simply never loaded).
// The K-in-a-row test of the reference (env/torch_vector_mnk_env.py:106-119: three
// conv2d's with ones / eye stencils over the mover's whole plane, "> k - 0.1") becomes
// four shift-AND chains on that bit string -- shifts 1 (row), n+1 (column), n+2
// (diagonal), n (anti-diagonal) -- exact integer arithmetic, so it reproduces the f32
// sums of 0/1 values bit for bit.  Multi-word shifts are v_alignbit_b32 per word.
//
// Templates: NW = register words per plane; CN / CK = board width / run length when
// they are compile-time constants (0 = read them from MnkGeom at run time).  The
// specialised forms turn every shift amount into an immediate and unroll the run
// doubling; the generic forms keep wave-uniform loops.
#pragma once
#ifdef __HIPCC_RTC__
// compiled at run time by hiprtc (mnk_jit.hip): the HIP device API is built in, libc headers do not exist
typedef unsigned char uint8_t;
typedef unsigned short uint16_t;
typedef unsigned int uint32_t;
typedef unsigned long long uint64_t;
typedef signed char int8_t;
typedef int int32_t;
typedef long long int64_t;
typedef unsigned long long uintptr_t;
#include "mnk_hip.h"
#else
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mnk_hip.h"
#endif

#define MNK_MAX_W 16    // u64 words per plane in memory: boards of up to 1 024 bits m*(n+1) (25x25, 31x31)
#define MNK_MAX_NW 32   // u32 words per plane in registers

struct MnkGeom {
  int m, n, k;
  int C;        // m*n cells = number of actions
  int W;        // u64 words per plane in memory
  int NW;       // u32 words that actually hold board bits: ceil(m*(n+1)/32)
  int stride;   // n+1 bits per board row (guard column included)
  uint32_t magic_n;       // x / n      == __umulhi(x, magic_n)      for x*n      < 2^32
  uint32_t magic_stride;  // x / (n+1)
  uint32_t magic_C;       // x / C
  uint32_t magic_2C;      // x / (2C)
  uint32_t valid[MNK_MAX_NW];  // 1 on real cells, 0 on guard / padding bits
};

__device__ __forceinline__ uint32_t mnk_div(uint32_t x, uint32_t magic) { return __umulhi(x, magic); }

__host__ __device__ inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// A masked draw from a policy head's logits (mnk_sample_logits; the mnk_selfplay_*_logits entry points fold it into a
// step kernel): where the logits and the mask live, the sampler's Philox key and position, where the results go.
struct MnkSample {
  const void* logits;        // [N][C] f32 / bf16 bit patterns; NULL = all-zero logits (uniform over the mask)
  int logits_dtype;          // MNK_LOGITS_F32 / MNK_LOGITS_BF16
  const uint8_t* mask;       // [N][C]
  uint64_t seed;
  const uint64_t* seed_dev;  // optional device word that REPLACES seed (a captured graph's sampler can be re-keyed)
  uint64_t step;
  const uint64_t* step_dev;  // optional device word ADDED to step
  int64_t env_id0;           // Philox row id of row 0
  int deterministic;
  int64_t* actions;          // out [N]
  float* logp;               // out [N], optional
};

template <int CN>
__device__ __forceinline__ int geom_n(const MnkGeom& g) { return CN ? CN : g.n; }
template <int CK>
__device__ __forceinline__ int geom_k(const MnkGeom& g) { return CK ? CK : g.k; }

// guard-column bit index (row * (n + 1) + col) -> cell (row * n + col), and back
template <int CN>
__device__ __forceinline__ int mnk_bit_cell(const MnkGeom& g, uint32_t bit) {
  // CN known: x / (n + 1) as one v_mul_hi_u32 by ceil(2^32 / (n + 1)), exact for x * (magic * (n + 1) - 2^32) < 2^32 --
  // every board bit (x < 1 024, the error term < n + 1) -- where the compiler's general form adds a shift
  constexpr uint32_t magic = CN ? (uint32_t)((0x100000000ull + CN) / (uint32_t)(CN + 1)) : 0u;
  return (int)(bit - (CN ? __umulhi(bit, magic) : mnk_div(bit, g.magic_stride)));
}
template <int CN>
__device__ __forceinline__ uint32_t mnk_cell_bit(const MnkGeom& g, uint32_t cell) {
  return cell + (CN ? cell / (uint32_t)CN : mnk_div(cell, g.magic_n));
}

// ---------------------------------------------------------------- multi-word bit strings
// x >>= s for a wave-uniform s >= 0 (an immediate in the specialised kernels)
template <int NW>
__device__ __forceinline__ void bs_shr(uint32_t (&x)[NW], int s) {
  for (int q = s >> 5; q > 0; --q) {
#pragma unroll
    for (int w = 0; w < NW; ++w) x[w] = (w + 1 < NW) ? x[w + 1] : 0u;
  }
  const int r = s & 31;
  if (r) {
#pragma unroll
    for (int w = 0; w < NW; ++w) x[w] = __builtin_amdgcn_alignbit((w + 1 < NW) ? x[w + 1] : 0u, x[w], (uint32_t)r);
  }
}

// x <<= s for a wave-uniform s >= 0; bits shifted past word NW-1 are dropped
template <int NW>
__device__ __forceinline__ void bs_shl(uint32_t (&x)[NW], int s) {
  for (int q = s >> 5; q > 0; --q) {
#pragma unroll
    for (int w = NW - 1; w >= 0; --w) x[w] = w > 0 ? x[w - 1] : 0u;
  }
  const int r = s & 31;
  if (r) {
#pragma unroll
    for (int w = NW - 1; w >= 0; --w) x[w] = __builtin_amdgcn_alignbit(x[w], w > 0 ? x[w - 1] : 0u, (uint32_t)(32 - r));
  }
}

// does the bit string hold k set bits spaced d apart?  log2(k) doubling steps.
template <int NW>
__device__ __forceinline__ bool bs_has_run(const uint32_t (&b)[NW], int d, int k) {
  uint32_t x[NW], t[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) x[w] = b[w];
  int len = 1;  // x marks the starts of runs of >= len
  while (2 * len <= k) {
#pragma unroll
    for (int w = 0; w < NW; ++w) t[w] = x[w];
    bs_shr<NW>(t, len * d);
#pragma unroll
    for (int w = 0; w < NW; ++w) x[w] &= t[w];
    len *= 2;
  }
  if (len + 1 == k) {
    // one stone short (k = 3, 5, 9, ...): AND with the string itself, shifted by len*d.  Same result as the
    // general step below, but the large shift moves zeros into the top words, so the compiler drops
    // everything that only fed those words (9x9x5: 12 instead of 15 ops for each of the three long strides)
#pragma unroll
    for (int w = 0; w < NW; ++w) t[w] = b[w];
    bs_shr<NW>(t, len * d);
#pragma unroll
    for (int w = 0; w < NW; ++w) x[w] &= t[w];
  } else if (len < k) {
#pragma unroll
    for (int w = 0; w < NW; ++w) t[w] = x[w];
    bs_shr<NW>(t, (k - len) * d);
#pragma unroll
    for (int w = 0; w < NW; ++w) x[w] &= t[w];
  }
  uint32_t any = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) any |= x[w];
  return any != 0;
}

// env/torch_vector_mnk_env.py:106-119 on one plane
template <int NW, int CN, int CK>
__device__ __forceinline__ bool mnk_plane_wins(const MnkGeom& g, const uint32_t (&b)[NW]) {
  const int n = geom_n<CN>(g), k = geom_k<CK>(g);
  bool hit = bs_has_run<NW>(b, 1, k);      // rows
  hit |= bs_has_run<NW>(b, n + 1, k);      // columns
  hit |= bs_has_run<NW>(b, n + 2, k);      // diagonals
  hit |= bs_has_run<NW>(b, n, k);          // anti-diagonals
  return hit;
}

// The cells of `empty` where one more stone of `plane` leaves a run of >= k of its stones through that cell -- the win
// test of env_play after that ply, for every empty cell at once (an overline counts, as in the reference's "> k - 0.1").
// Along stride d: R_j = cells whose next j cells along +d are all stones, L_j = the same along -d; a cell completes a
// run when L_j & R_{k-1-j} holds for some j.  R_j = R_{j-1} & (plane >> j d): the prefixes are shared, so the j-loop
// below costs 2(k-1) shifts and ~3k AND / OR per stride and word once unrolled (CK known; the compiler merges the
// repeated prefixes).  Guard-column bits are never stones, so no run wraps a row.  `empty` already carries g.valid.
template <int NW, int CN, int CK>
__device__ __forceinline__ void mnk_plane_completions(const MnkGeom& g, const uint32_t (&plane)[NW],
                                                      const uint32_t (&empty)[NW], uint32_t (&out)[NW]) {
  const int n = geom_n<CN>(g), k = geom_k<CK>(g);
  constexpr int UK = CK ? CK : 1;  // the j / i loops unroll when k is known, stay loops when it is not
  uint32_t acc[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) acc[w] = 0u;
#pragma unroll
  for (int dir = 0; dir < 4; ++dir) {
    const int d = dir == 0 ? 1 : (dir == 1 ? n + 1 : (dir == 2 ? n + 2 : n));  // rows, columns, diagonals, anti-diagonals
    uint32_t lj[NW];  // L_j, grown one stone per j
#pragma unroll
    for (int w = 0; w < NW; ++w) lj[w] = ~0u;
#pragma unroll UK
    for (int j = 0; j < k; ++j) {
      if (j > 0) {
        uint32_t t[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) t[w] = plane[w];
        bs_shl<NW>(t, j * d);
#pragma unroll
        for (int w = 0; w < NW; ++w) lj[w] &= t[w];
      }
      uint32_t rj[NW];  // R_{k-1-j}
#pragma unroll
      for (int w = 0; w < NW; ++w) rj[w] = ~0u;
#pragma unroll UK
      for (int i = 1; i < k - j; ++i) {
        uint32_t t[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) t[w] = plane[w];
        bs_shr<NW>(t, i * d);
#pragma unroll
        for (int w = 0; w < NW; ++w) rj[w] &= t[w];
      }
#pragma unroll
      for (int w = 0; w < NW; ++w) acc[w] |= lj[w] & rj[w];
    }
  }
#pragma unroll
  for (int w = 0; w < NW; ++w) out[w] = acc[w] & empty[w];
}

// position of the r-th (0-based) set bit of x; r < popcount(x).
// A halving search in arithmetic only, as one block of gfx950 assembly: on a wave that is alone on its
// SIMD every instruction -- VALU, SALU or hazard s_nop -- costs one ~4-cycle issue slot
// (tools/exp_valu_rate.hip), and the v_cmp -> SGPR -> v_cndmask form the compiler makes of any C++
// spelling of this costs 8-9 slots per level.  Here a level is five:
//   t    = popcount(x[pos .. pos+S)) + nr      nr = -(r + 1), negative while bits remain
//   nr   = umax(nr, t)                         t < 0  <=>  the bit lies above the field: rank -= count
//   pos |= S & (t >> 31)                       ... and the position moves up
// The last level looks at one bit: the answer is pos + 1 unless r == 0 and that bit is set.
// select_bit32_nr takes the rank already negated (nr = ~r) and a start `base` whose low five bits are zero: the
// field offsets of v_bfe and the shift that makes the one-hot read only the low five bits of pos, so the word's
// bit offset in a multi-word string rides along in pos for free.
#define MNK_SELECT_LEVEL(S)                        \
  "v_bfe_u32 %[t], %[x], %[pos], " #S "\n\t"       \
  "v_bcnt_u32_b32 %[t], %[t], %[nr]\n\t"          \
  "v_max_u32 %[nr], %[nr], %[t]\n\t"              \
  "v_ashrrev_i32 %[t], 31, %[t]\n\t"              \
  "v_and_or_b32 %[pos], %[t], " #S ", %[pos]\n\t"
__device__ __forceinline__ uint32_t select_bit32_nr(uint32_t x, uint32_t nr, uint32_t base) {
  uint32_t pos, t;
  asm("v_and_b32 %[t], 0xffff, %[x]\n\t"
      "v_bcnt_u32_b32 %[t], %[t], %[nr]\n\t"
      "v_max_u32 %[nr], %[nr], %[t]\n\t"
      "v_ashrrev_i32 %[t], 31, %[t]\n\t"
      "v_and_or_b32 %[pos], %[t], 16, %[base]\n\t"
      MNK_SELECT_LEVEL(8) MNK_SELECT_LEVEL(4) MNK_SELECT_LEVEL(2)
      "v_bfe_u32 %[t], %[x], %[pos], 1\n\t"
      "v_bitop3_b32 %[t], %[nr], %[t], %[t] bitop3:0x3f\n\t"  // ~(nr & bit): bit 0 clear only if r == 0 and the bit is set
      "v_and_or_b32 %[pos], %[t], 1, %[pos]"
      : [pos] "=&v"(pos), [t] "=&v"(t), [nr] "+v"(nr)
      : [x] "v"(x), [base] "v"(base));
  return pos;
}
// The tail of the same search as one LDS byte read: the last three levels (8 -> 4 -> 2 -> 1, 13 slots) only answer
// "where is the r-th set bit of this byte, r < 8", a function of 11 bits.  MnkSelectTable is that function as a table,
// t[b][r] = position of the r-th (0-based) set bit of byte b, 0 where r >= popcount(b); mnk_select_table_fetch / _put copy it
// into 2 KB of a one-wave workgroup's LDS, and select_bit32_nr_tab runs the 16- and 8-level steps as above, then reads
// t[byte at pos][~nr].  The read is plain C++, not part of the assembly: the compiler counts it in its own s_waitcnt,
// which it puts before the first use -- behind the caller's cover(), see below.
struct MnkSelectTable {
  uint8_t t[256][8];
  constexpr MnkSelectTable() : t() {
    for (int b = 0; b < 256; ++b) {
      int r = 0;
      for (int p = 0; p < 8; ++p)
        if ((b >> p) & 1) t[b][r++] = (uint8_t)p;
    }
  }
};
#define MNK_SELECT_TABLE_BYTES 2048
static __device__ const MnkSelectTable mnk_select_table_rom = MnkSelectTable();

// all 64 threads of a one-wave workgroup: 32 bytes each, global -> LDS; the caller's __syncthreads() publishes it.
// In two halves, so that the caller can issue other loads of its own (the env's state) between the table's loads and
// the wait that the LDS writes need: one round trip to memory for both, not one after the other.
struct MnkSelectTableShare {
  uint4 lo, hi;
};
__device__ __forceinline__ MnkSelectTableShare mnk_select_table_fetch() {
  const uint4* src = (const uint4*)&mnk_select_table_rom.t[0][0];
  return {src[threadIdx.x], src[threadIdx.x + 64u]};
}
__device__ __forceinline__ void mnk_select_table_put(uint32_t* lds_table, const MnkSelectTableShare& s) {
  uint4* dst = (uint4*)lds_table;
  dst[threadIdx.x] = s.lo;
  dst[threadIdx.x + 64u] = s.hi;
}

// `cover()` stands between the read and the first use of what it returns: work of the caller's that does not hang on the
// pick, pinned there (the scheduler left to itself puts a few instructions behind the read and waits; a lone wave then
// sits out most of the read's ~50 cycles)
struct MnkNoCover {
  __device__ __forceinline__ void operator()() const {}
};
template <typename Cover>
__device__ __forceinline__ uint32_t select_bit32_nr_tab(uint32_t x, uint32_t nr, uint32_t base, const uint8_t* tab,
                                                        Cover&& cover) {
  uint32_t pos, t;
  asm("v_and_b32 %[t], 0xffff, %[x]\n\t"
      "v_bcnt_u32_b32 %[t], %[t], %[nr]\n\t"
      "v_max_u32 %[nr], %[nr], %[t]\n\t"
      "v_ashrrev_i32 %[t], 31, %[t]\n\t"
      "v_and_or_b32 %[pos], %[t], 16, %[base]\n\t"
      MNK_SELECT_LEVEL(8)
      "v_bfe_u32 %[t], %[x], %[pos], 8\n\t"     // the byte the bit lies in ...
      "v_not_b32 %[nr], %[nr]\n\t"               // ... its rank there, 0 .. 7 ...
      "v_lshl_add_u32 %[t], %[t], 3, %[nr]"      // ... and the table's index
      : [pos] "=&v"(pos), [t] "=&v"(t), [nr] "+v"(nr)
      : [x] "v"(x), [base] "v"(base));
  const uint32_t in_byte = tab[t];
  __builtin_amdgcn_sched_barrier(0);
  cover();
  __builtin_amdgcn_sched_barrier(0);
  return pos | in_byte;
}
#undef MNK_SELECT_LEVEL

// ---------------------------------------------------------------- the rollout statistics of a wave
// The five counters of `stats` (episodes, black wins, white wins, draws, summed lengths) from per-lane counts, without
// a pass over the lanes: an atomicAdd of a per-lane value on one LDS word makes the compiler scan the active lanes one
// by one (find the lane, v_readlane, add, branch: seven scalar-side instructions and a taken branch per lane and
// counter -- some 250 trips a wave at the headline).  mnk_wave_sum is gfx9's DPP add ladder instead: every lane of a
// row of 16 gets the sum of its row up to itself (row_shr 1 / 2 / 3 of the value, then row_shr 4 and 8 of the partial
// sums), row_bcast:15 carries a row's total into the next row, row_bcast:31 the first half's into the second: lane
// 63 ends with the wave's total.  Lanes that a shift leaves without a source add the `old` operand, zero.
// ALL 64 LANES MUST BE ACTIVE (a lane that is switched off sends nothing): callers zero the counts of lanes that carry
// no env and fold outside their `i < N` branch.
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
__device__ __forceinline__ uint32_t mnk_dpp_or_zero(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, BANK_MASK, false);
}
__device__ __forceinline__ uint32_t mnk_wave_sum(uint32_t v) {  // the total, in lane 63
  uint32_t s = v + mnk_dpp_or_zero<0x111>(v);  // row_shr:1
  s += mnk_dpp_or_zero<0x112>(v);              // row_shr:2
  s += mnk_dpp_or_zero<0x113>(v);              // row_shr:3 -- lanes hold v[l-3 .. l] of their row
  s += mnk_dpp_or_zero<0x114, 0xF, 0xE>(s);    // row_shr:4, not into lanes 0-3 of a row
  s += mnk_dpp_or_zero<0x118, 0xF, 0xC>(s);    // row_shr:8, into lanes 8-15 of a row: lane 15 has the row's sum
  s += mnk_dpp_or_zero<0x142, 0xA>(s);         // row_bcast:15 into rows 1 and 3
  s += mnk_dpp_or_zero<0x143, 0xC>(s);         // row_bcast:31 into rows 2 and 3
  return s;
}
// Lane c < MNK_STATS_COUNTERS of the wave gets the wave's total of counter c (every other lane 0).  The four sums fit
// 32 bits for every legal launch: 64 lanes x (C + 65 535) at the most.  Draws are episodes minus wins, of the totals.
__device__ __forceinline__ uint32_t mnk_stats_wave_totals(uint32_t done, uint32_t black, uint32_t white, uint32_t len) {
  const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)mnk_wave_sum(done), 63);
  const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)mnk_wave_sum(black), 63);
  const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)mnk_wave_sum(white), 63);
  const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)mnk_wave_sum(len), 63);
  uint32_t v = 0;  // (one v_writelane per counter: a chain of selects on the lane number became a tree of branches)
  asm("v_writelane_b32 %0, %1, 0\n\t"
      "v_writelane_b32 %0, %2, 1\n\t"
      "v_writelane_b32 %0, %3, 2\n\t"
      "v_writelane_b32 %0, %4, 3\n\t"
      "v_writelane_b32 %0, %5, 4"
      : "+v"(v)
      : "s"(d), "s"(b), "s"(w), "s"(d - b - w), "s"(l));
  return v;
}
// a one-wave workgroup's totals into its replica of `stats`: one global atomic per counter that is not zero (spread
// over MNK_STATS_REPLICAS cache lines: thousands of adds on five addresses would serialise at ~11 ns each -- measured:
// 56 us per launch)
__device__ __forceinline__ void mnk_stats_wave_commit(unsigned long long* stats, uint32_t total) {
  if (threadIdx.x < MNK_STATS_COUNTERS && total)
    atomicAdd(&stats[(size_t)(blockIdx.x % MNK_STATS_REPLICAS) * MNK_STATS_STRIDE + threadIdx.x], (unsigned long long)total);
}

__device__ __forceinline__ int select_bit32(uint32_t x, int r) { return (int)select_bit32_nr(x, ~(uint32_t)r, 0u); }

template <int NW>
__device__ __forceinline__ int bs_popcount(const uint32_t (&x)[NW]) {
  int c = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) c += __popc(x[w]);
  return c;
}

// bit index of the r-th set bit of the multi-word string (r < popcount), and the string with only
// that bit set in `hot`.  With nr = ~r = -(r + 1) and pre[w] = popcount of words 0 .. w-1, t[w] = pre[w] + nr is
// negative exactly when the bit lies in word w or above; prefix counts never decrease, so these tests are independent
// of each other and their sign masks m[w] = t[w] >> 31 are monotone (m[w + 1] implies m[w]).  The rank inside the
// chosen word is the largest t[w] as an unsigned number (a negative t[w] is larger than nr, a non-negative one is
// smaller), one v_max3 per two words; the word and its bit offset are bit-field inserts on the masks; and the one-hot
// is one & m[w] & ~m[w + 1] -- one logic op per word, no compare, no select.  (v_bitop3 truth tables are indexed by
// src0 * 4 + src1 * 2 + src2.  Spelled as plain C++ the masks went back to v_cmp + v_cndmask: 3 more slots per ply.)
// TAB: the search inside the chosen word ends with a read of `tab`, an LDS copy of MnkSelectTable, and `cover()` runs
// behind that read (select_bit32_nr_tab).
template <int NW, bool TAB = false, typename Cover = MnkNoCover>
__device__ __forceinline__ int bs_select_hot(const uint32_t (&x)[NW], int r_, uint32_t (&hot)[NW],
                                             const uint8_t* tab = nullptr, Cover&& cover = Cover()) {
  const uint32_t nr = ~(uint32_t)r_;
  uint32_t m[NW + 1], word = x[0], base = 0u, rank = nr, pre = 0u;
  m[0] = ~0u;
  m[NW] = 0u;
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    pre += (uint32_t)__popc(x[w - 1]);
    const uint32_t t = pre + nr;
    m[w] = (uint32_t)((int32_t)t >> 31);
    rank = rank > t ? rank : t;
    word = __builtin_amdgcn_bitop3_b32(m[w], x[w], word, 0xca);  // m ? x[w] : word
    base = __builtin_amdgcn_bitop3_b32(m[w], 32u * w, base, 0xca);    // m ? 32 w : base
  }
  uint32_t pos;
  if constexpr (TAB) pos = select_bit32_nr_tab(word, rank, base, tab, cover);
  else pos = select_bit32_nr(word, rank, base);
  const uint32_t one = 1u << (pos & 31u);
#pragma unroll
  for (int w = 0; w < NW; ++w) hot[w] = __builtin_amdgcn_bitop3_b32(one, m[w], m[w + 1], 0x40);  // one & m[w] & ~m[w + 1]
  return (int)pos;
}

template <int NW>
__device__ __forceinline__ int bs_select(const uint32_t (&x)[NW], int r) {
  uint32_t hot[NW];
  return bs_select_hot<NW>(x, r, hot);
}

// ---------------------------------------------------------------- Philox4x32-10
struct Philox4 { uint32_t v[4]; };

// 32 x 32 -> 64 in one instruction (the compiler spells it v_mul_lo_u32 + v_mul_hi_u32: two issue slots).
// Two spellings that differ only in where the (unused) carry-out goes: an SGPR pair of the compiler's choice, or vcc.
// After an inline-assembly statement the compiler wants one wait state before a VALU instruction that names any
// register the statement defines (it cannot see inside the statement, so it assumes a forwarding hazard), and fills
// it with an s_nop when nothing else is there.  A Philox round multiplies twice: with the two carry-outs apart the
// multiplies share no register and may stand back to back (philox4x32_10_from; and an assembly statement in between
// does not count as a wait state, so that form also keeps an xor away from the multiply it reads).
__device__ __forceinline__ uint64_t mnk_mul_wide(uint32_t a, uint32_t m) {
  uint64_t product, carry;
  asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(product), "=s"(carry) : "v"(a), "s"(m));
  return product;
}
__device__ __forceinline__ uint64_t mnk_mul_wide_vcc(uint32_t a, uint32_t m) {
  uint64_t product;
  asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(product) : "v"(a), "s"(m) : "vcc");
  return product;
}

#define MNK_PHILOX_M0 0xD2511F53u
#define MNK_PHILOX_M1 0xCD9E8D57u

// round 1's first product, c0 * M0.  The rollout's c0 is the low word of the lane's env id -- the same in every block
// of a launch -- so its loops compute this once and hand it to philox4x32_10_from.
__device__ __forceinline__ uint64_t philox_first_product(uint32_t c0) { return mnk_mul_wide_vcc(c0, MNK_PHILOX_M0); }

// the ten rounds, given round 1's first product p0_first = philox_first_product(c0).
// Round r multiplies twice, A[r] = c0 * M0 and B[r] = c2 * M1, and xors twice, n0[r] off B[r]'s high half and n2[r]
// off A[r]'s; A[r + 1] takes n0[r], B[r + 1] takes n2[r].  So the block is two chains that only exchange low halves
// a round late, and the statements below walk them half a round apart -- multiply of one chain, xor of the other --
// so that an xor never directly follows the multiply whose product it reads (see mnk_mul_wide).
// The words are those of philox4x32_10, bit for bit: tests/test_gpu_rollout_lean2.py holds the loops that use this
// form to the oracle's Philox (oracle/philox.py), the env id's low word wrapping inside a wave included.
// PhiloxSteps: the block as a list of its 39 statements, numbered in the order philox4x32_10_from below has them, so
// that a caller may run it in pieces (run<FROM, TO>(): the rollout's FAST loop makes the next trip's block a quarter
// per ply, behind the ply's table read).
struct PhiloxSteps {
  static constexpr int COUNT = 39;
  uint64_t A[11], B[11];
  uint32_t n0[11], n2[11];
  uint32_t c1, c2, c3, k0, k1;
  __device__ __forceinline__ PhiloxSteps(uint64_t p0_first, uint32_t c1_, uint32_t c2_, uint32_t c3_, uint32_t k0_,
                                         uint32_t k1_)
      : c1(c1_), c2(c2_), c3(c3_), k0(k0_), k1(k1_) {
    A[1] = p0_first;
  }
  // the xors of round r (keys of round r; c1 / c3 of round r are the low halves of round r - 1's products)
  __device__ __forceinline__ void xor_n0(int r) {
    n0[r] = __builtin_amdgcn_bitop3_b32((uint32_t)(B[r] >> 32), r == 1 ? c1 : (uint32_t)B[r - 1],
                                        k0 + (uint32_t)(r - 1) * 0x9E3779B9u, 0x96);
  }
  __device__ __forceinline__ void xor_n2(int r) {
    n2[r] = __builtin_amdgcn_bitop3_b32((uint32_t)(A[r] >> 32), r == 1 ? c3 : (uint32_t)A[r - 1],
                                        k1 + (uint32_t)(r - 1) * 0xBB67AE85u, 0x96);
  }
  // statement s (a compile-time constant once unrolled): 0 and 1 open, then eight per pair of rounds r - 1, r
  __device__ __forceinline__ void statement(int s) {
    if (s == 0) { B[1] = mnk_mul_wide(c2, MNK_PHILOX_M1); return; }
    if (s == 1) { xor_n2(1); return; }
    if (s == 38) { xor_n2(10); return; }
    const int r = 2 + 2 * ((s - 2) >> 3);
    switch ((s - 2) & 7) {
      case 0: B[r] = mnk_mul_wide(n2[r - 1], MNK_PHILOX_M1); break;
      case 1: xor_n0(r - 1); break;
      case 2: A[r] = mnk_mul_wide_vcc(n0[r - 1], MNK_PHILOX_M0); break;
      case 3: xor_n0(r); break;
      case 4: A[r + 1] = mnk_mul_wide_vcc(n0[r], MNK_PHILOX_M0); break;
      case 5: xor_n2(r); break;
      case 6: B[r + 1] = mnk_mul_wide(n2[r], MNK_PHILOX_M1); break;
      default: xor_n2(r + 1); break;
    }
  }
  template <int FROM, int TO>
  __device__ __forceinline__ void run() {
#pragma unroll
    for (int s = FROM; s < TO; ++s) statement(s);
  }
  __device__ __forceinline__ Philox4 words() const {
    Philox4 o;
    o.v[0] = n0[10]; o.v[1] = (uint32_t)B[10]; o.v[2] = n2[10]; o.v[3] = (uint32_t)A[10];
    return o;
  }
};

// the block in one piece, for every other user of this form (kept as its own text: spelled through PhiloxSteps the
// two-lane kernels came out with another register allocation, and they are to keep their code)
__device__ __forceinline__ Philox4 philox4x32_10_from(uint64_t p0_first, uint32_t c1, uint32_t c2, uint32_t c3,
                                                      uint32_t k0, uint32_t k1) {
  uint64_t A[11], B[11];
  uint32_t n0[11], n2[11];
#define MNK_PHILOX_N0(r) \
  n0[r] = __builtin_amdgcn_bitop3_b32((uint32_t)(B[r] >> 32), (r) == 1 ? c1 : (uint32_t)B[(r) - 1], k0 + ((r) - 1) * 0x9E3779B9u, 0x96)
#define MNK_PHILOX_N2(r) \
  n2[r] = __builtin_amdgcn_bitop3_b32((uint32_t)(A[r] >> 32), (r) == 1 ? c3 : (uint32_t)A[(r) - 1], k1 + ((r) - 1) * 0xBB67AE85u, 0x96)
  A[1] = p0_first;
  B[1] = mnk_mul_wide(c2, MNK_PHILOX_M1);
  MNK_PHILOX_N2(1);
#pragma unroll
  for (int r = 2; r <= 10; r += 2) {
    B[r] = mnk_mul_wide(n2[r - 1], MNK_PHILOX_M1);
    MNK_PHILOX_N0(r - 1);
    A[r] = mnk_mul_wide_vcc(n0[r - 1], MNK_PHILOX_M0);
    MNK_PHILOX_N0(r);
    if (r < 10) {
      A[r + 1] = mnk_mul_wide_vcc(n0[r], MNK_PHILOX_M0);
      MNK_PHILOX_N2(r);
      B[r + 1] = mnk_mul_wide(n2[r], MNK_PHILOX_M1);
      MNK_PHILOX_N2(r + 1);
    }
  }
  MNK_PHILOX_N2(10);
#undef MNK_PHILOX_N0
#undef MNK_PHILOX_N2
  Philox4 o;
  o.v[0] = n0[10]; o.v[1] = (uint32_t)B[10]; o.v[2] = n2[10]; o.v[3] = (uint32_t)A[10];
  return o;
}

// the block as every other kernel computes it: round after round, both multiplies with their carry-out in an SGPR
// pair.  Left as it was: where this form sits among a ply's record stores (19x19, two lanes per env) the skewed one
// measured 1 % slower, and elsewhere the waves of other envs cover the wait states.
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                 uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = mnk_mul_wide(c0, MNK_PHILOX_M0), p1 = mnk_mul_wide(c2, MNK_PHILOX_M1);
    // three-input xor in one slot (v_bitop3_b32, truth table 0x96); left alone the compiler emits two v_xor_b32
    const uint32_t n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, k0, 0x96);
    const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, k1, 0x96);
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}

// counter layout of oracle/philox.py: ctr = (env_lo, env_hi, q_lo, stream | q_hi24 << 8)
__device__ __forceinline__ Philox4 mnk_rng_block(uint64_t seed, uint64_t env, uint64_t q, uint32_t stream) {
  return philox4x32_10((uint32_t)env, (uint32_t)(env >> 32), (uint32_t)q,
                       stream | ((uint32_t)((q >> 32) & 0xFFFFFFu) << 8),
                       (uint32_t)seed, (uint32_t)(seed >> 32));
}

// the same block with env_p0 = philox_first_product((uint32_t)env) computed by the caller, once for many blocks
__device__ __forceinline__ Philox4 mnk_rng_block_from(uint64_t seed, uint64_t env_p0, uint64_t env, uint64_t q,
                                                      uint32_t stream) {
  return philox4x32_10_from(env_p0, (uint32_t)(env >> 32), (uint32_t)q,
                            stream | ((uint32_t)((q >> 32) & 0xFFFFFFu) << 8),
                            (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ... and the same block not yet run: the caller runs its statements where it wants them
__device__ __forceinline__ PhiloxSteps mnk_rng_steps_from(uint64_t seed, uint64_t env_p0, uint64_t env, uint64_t q,
                                                          uint32_t stream) {
  return PhiloxSteps(env_p0, (uint32_t)(env >> 32), (uint32_t)q, stream | ((uint32_t)((q >> 32) & 0xFFFFFFu) << 8),
                     (uint32_t)seed, (uint32_t)(seed >> 32));
}

__device__ __forceinline__ uint32_t philox_word(const Philox4& b, uint32_t i) {
  uint32_t lo = (i & 1u) ? b.v[1] : b.v[0];
  uint32_t hi = (i & 1u) ? b.v[3] : b.v[2];
  return (i & 2u) ? hi : lo;
}

// scalar streams: one u32 per (env, step)
__device__ __forceinline__ uint32_t mnk_rand_u32(uint64_t seed, uint64_t env, uint64_t step, uint32_t stream) {
  Philox4 b = mnk_rng_block(seed, env, step >> 2, stream);
  return philox_word(b, (uint32_t)(step & 3));
}

// ---------------------------------------------------------------- one env in registers
template <int NW>
struct MnkEnv {
  uint32_t p[2][NW];
  uint32_t meta;  // bit0 side to move, bits 1.. move count
};

// planes u64[2][W][N] in memory <-> NW u32 words per plane in registers
// EXACT: the plane has exactly (NW+1)/2 memory words (true for the specialised boards), so the
// wave-uniform "does this word exist" tests fold away
template <int NW, bool EXACT = false>
__device__ __forceinline__ void plane_load(uint32_t (&x)[NW], const uint64_t* plane, int64_t N, int W, int64_t i) {
#pragma unroll
  for (int q = 0; q < (NW + 1) / 2; ++q) {
    const uint64_t v = (EXACT || q < W) ? plane[(int64_t)q * N + i] : 0ull;
    x[2 * q] = (uint32_t)v;
    if (2 * q + 1 < NW) x[2 * q + 1] = (uint32_t)(v >> 32);
  }
}

template <int NW, bool EXACT = false>
__device__ __forceinline__ void plane_store(const uint32_t (&x)[NW], uint64_t* plane, int64_t N, int W, int64_t i) {
#pragma unroll
  for (int q = 0; q < (NW + 1) / 2; ++q) {
    const uint64_t hi = (2 * q + 1 < NW) ? (uint64_t)x[2 * q + 1] : 0ull;
    if (EXACT || q < W) plane[(int64_t)q * N + i] = (uint64_t)x[2 * q] | (hi << 32);
  }
}

// ---------------------------------------------------------------- rollout records
// One recorded position is NW u64 rows of stride N: row w = first plane's word w | second plane's word w << 32
// (the 32-bit words of two planes, interleaved; the rollout records the mover's plane first).  No padding at any board size -- 9x9 takes 3 rows =
// 24 B where the state layout's two u64 planes take 32 -- and the rollout is bound by exactly these
// stores.  nw = the board's word count (MnkGeom::NW), used when NW is only an upper bound.
template <int NW, bool EXACT = false>
__device__ __forceinline__ void rec_store(const uint32_t (&p0)[NW], const uint32_t (&p1)[NW], uint64_t* rows, int64_t N,
                                          int nw, int64_t i) {
#pragma unroll
  for (int w = 0; w < NW; ++w)
    if (EXACT || w < nw) rows[(int64_t)w * N + i] = (uint64_t)p0[w] | ((uint64_t)p1[w] << 32);
}

template <int NW, bool EXACT = false>
__device__ __forceinline__ void rec_load(uint32_t (&p0)[NW], uint32_t (&p1)[NW], const uint64_t* rows, int64_t N, int nw,
                                         int64_t i) {
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const uint64_t v = (EXACT || w < nw) ? rows[(int64_t)w * N + i] : 0ull;
    p0[w] = (uint32_t)v;
    p1[w] = (uint32_t)(v >> 32);
  }
}

template <int NW, bool EXACT = false>
__device__ __forceinline__ void env_load(MnkEnv<NW>& e, const uint64_t* planes, const uint32_t* meta, int64_t N,
                                         int W, int64_t i) {
  plane_load<NW, EXACT>(e.p[0], planes, N, W, i);
  plane_load<NW, EXACT>(e.p[1], planes + (int64_t)W * N, N, W, i);
  e.meta = meta[i];
}

template <int NW, bool EXACT = false>
__device__ __forceinline__ void env_store(const MnkEnv<NW>& e, uint64_t* planes, uint32_t* meta, int64_t N, int W,
                                          int64_t i) {
  plane_store<NW, EXACT>(e.p[0], planes, N, W, i);
  plane_store<NW, EXACT>(e.p[1], planes + (int64_t)W * N, N, W, i);
  meta[i] = e.meta;
}

template <int NW>
__device__ __forceinline__ void env_clear(MnkEnv<NW>& e) {
#pragma unroll
  for (int pl = 0; pl < 2; ++pl)
#pragma unroll
    for (int w = 0; w < NW; ++w) e.p[pl][w] = 0u;
  e.meta = 0u;
}

template <int NW>
__device__ __forceinline__ void env_legal(const MnkGeom& g, const MnkEnv<NW>& e, uint32_t (&legal)[NW]) {
#pragma unroll
  for (int w = 0; w < NW; ++w) legal[w] = ~(e.p[0][w] | e.p[1][w]) & g.valid[w];
}

// the r-th cell of `set` in action order with r = mulhi32(x, |set|) (oracle/philox.py pick_legal over the set's mask).
// An empty set draws over all C cells like RandomPolicy's 1e-8 guard (policy.py:21-24): `set` is replaced by the
// valid-cell string, whose r-th set bit is cell r -- on return `set` holds what was drawn from.
template <int NW, int CN>
__device__ __forceinline__ int bs_pick_cell(const MnkGeom& g, uint32_t (&set)[NW], uint32_t x) {
  const int nl = bs_popcount<NW>(set);
#pragma unroll
  for (int w = 0; w < NW; ++w) set[w] = nl ? set[w] : g.valid[w];
  const int r = (int)__umulhi(x, (uint32_t)(nl ? nl : g.C));
  const uint32_t bit = (uint32_t)bs_select<NW>(set, r);
  return mnk_bit_cell<CN>(g, bit);
}

// uniform legal cell from one u32 (oracle/philox.py pick_legal; selfplay/policy.py:18-29)
template <int NW, int CN>
__device__ __forceinline__ int env_pick_legal(const MnkGeom& g, const MnkEnv<NW>& e, uint32_t x) {
  uint32_t legal[NW];
  env_legal<NW>(g, e, legal);
  // (a full board -- poked states only -- draws over all C cells)
  return bs_pick_cell<NW, CN>(g, legal, x);
}

// The candidate set of the one-ply tactical player for the side whose stones are `mine` (the other side's: `theirs`):
// the legal cells that win now if there are any, else the legal cells where the other side would win next ply, else
// the legal cells.  (Empty only on a full board; bs_pick_cell then draws over all C cells.)
template <int NW, int CN, int CK>
__device__ __forceinline__ void mnk_tactical_set(const MnkGeom& g, const uint32_t (&mine)[NW], const uint32_t (&theirs)[NW],
                                                 uint32_t (&set)[NW]) {
  uint32_t legal[NW], win[NW], block[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) legal[w] = ~(mine[w] | theirs[w]) & g.valid[w];
  mnk_plane_completions<NW, CN, CK>(g, mine, legal, win);
  mnk_plane_completions<NW, CN, CK>(g, theirs, legal, block);
  uint32_t any_win = 0, any_block = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    any_win |= win[w];
    any_block |= block[w];
  }
#pragma unroll
  for (int w = 0; w < NW; ++w) set[w] = any_win ? win[w] : (any_block ? block[w] : legal[w]);
}

// the tactical reply of the side to move from one u32 (x = 0: the first cell of the set, deterministic=True)
template <int NW, int CN, int CK>
__device__ __forceinline__ int env_pick_tactical(const MnkGeom& g, const MnkEnv<NW>& e, uint32_t x) {
  const uint32_t side = e.meta & 1u;
  uint32_t mine[NW], theirs[NW], set[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    mine[w] = side ? e.p[1][w] : e.p[0][w];
    theirs[w] = side ? e.p[0][w] : e.p[1][w];
  }
  mnk_tactical_set<NW, CN, CK>(g, mine, theirs, set);
  return bs_pick_cell<NW, CN>(g, set, x);
}

struct MnkPly {
  bool win, done;
  int err;  // MNK_ERR_* (0 = fine); on error the env is left untouched
};

// env/torch_vector_mnk_env.py:60-84 for one env.
// TRUSTED: the action comes from our own legal-move sampler (always in [0, C)), so the range
// check -- a divergent branch around the whole ply -- is compiled out.
template <int NW, int CN, int CK, bool TRUSTED = false>
__device__ __forceinline__ MnkPly env_play(const MnkGeom& g, MnkEnv<NW>& e, int64_t action, bool strict) {
  MnkPly out;
  out.win = false; out.done = false; out.err = 0;
  const int C = g.C;
  uint32_t a;
  if (TRUSTED) {
    a = (uint32_t)action;
  } else {
    const int64_t a64 = action < 0 ? action + C : action;  // torch indexing wraps negatives (:68)
    if (a64 < 0 || a64 >= C) { out.err = 1; return out; }
    a = (uint32_t)a64;
  }
  const uint32_t bit = mnk_cell_bit<CN>(g, a);
  const int wsel = (int)(bit >> 5);
  const uint32_t one = 1u << (bit & 31u);
  const uint32_t side = e.meta & 1u;
  if (strict) {
    uint32_t occ = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) occ |= (w == wsel) ? ((e.p[0][w] | e.p[1][w]) & one) : 0u;
    if (occ) { out.err = 2; return out; }
  }
  uint32_t mine[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const uint32_t add = (w == wsel) ? one : 0u;
    e.p[0][w] |= side ? 0u : add;   // :68 boards[idx, player, r, c] = 1
    e.p[1][w] |= side ? add : 0u;
    mine[w] = side ? e.p[1][w] : e.p[0][w];
  }
  const uint32_t moves = (e.meta >> 1) + 1u;                 // :69
  out.win = mnk_plane_wins<NW, CN, CK>(g, mine);              // :71
  const bool draw = (moves >= (uint32_t)C) && !out.win;       // :72
  out.done = out.win || draw;                                 // :73
  e.meta = (moves << 1) | (side ^ 1u);                        // :82 toggles even when finished
  return out;
}

__device__ __forceinline__ void mnk_report(int32_t* err, int code, int64_t env) {
  if (err && atomicCAS(&err[0], 0, code) == 0) err[1] = (int32_t)env;
}
