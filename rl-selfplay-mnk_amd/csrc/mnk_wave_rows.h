// mnk_wave_rows.h -- device code shared by the kernels that run one wave64 per row (the PUCT player, mnk_puct.hip, and
// the search self-play step, mnk_search_selfplay.hip): the wave's LDS fence, a stone test on guard-column planes in LDS,
// the canonical view of a position, and the move choice from root visit counts.
#pragma once
#include "mnk_device.h"
#include "mnk_emit.h"

// the wave's own LDS traffic: make this wave's stores (LDS and global) visible to its other lanes
__device__ __forceinline__ void row_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int CN>
__device__ __forceinline__ bool row_stone(const MnkGeom& g, const uint32_t* plane, int cell) {
  const uint32_t bit = mnk_cell_bit<CN>(g, (uint32_t)cell);
  return (plane[bit >> 5] >> (bit & 31u)) & 1u;
}

// the canonical observation (channel 0 = plane `flip` of pos) and legal mask of a position in LDS, row i (MASK_OPT: the
// mask may be NULL)
template <int NW, int CN, bool MASK_OPT = false>
__device__ __forceinline__ void row_write_view(const MnkGeom& g, const uint32_t* pos, int flip, int64_t i, void* obs,
                                               int obs_dtype, uint8_t* mask, int lane) {
  const int C = g.C;
  for (int q = lane; q < 2 * C; q += 64) {
    const int ch = q >= C, cell = q - (ch ? C : 0);
    const bool s = row_stone<CN>(g, pos + (ch ^ flip) * NW, cell);
    const int64_t o = i * 2 * C + q;
    if (obs_dtype == MNK_OBS_F32) ((float*)obs)[o] = s ? 1.0f : 0.0f;
    else if (obs_dtype == MNK_OBS_BF16) ((uint16_t*)obs)[o] = s ? (uint16_t)0x3F80 : (uint16_t)0;
    else ((uint8_t*)obs)[o] = s ? 1 : 0;
  }
  if (MASK_OPT && !mask) return;
  for (int a = lane; a < C; a += 64) mask[i * C + a] = !(row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a));
}

// The move from root visit counts n_a = na_of(a) (wave-uniform result), given maxn = max n_a > 0 and tot = sum n_a:
//   by_count (temperature 1): the cell at which the counts, accumulated in action order, first exceed r = mulhi32(x, tot);
//   otherwise (temperature 0): S = the cells of n_a = maxn, the r-th cell of S in action order, r = mulhi32(x, |S|).
// `move` is left as it is only when maxn is not the maximum (no cell hit).  na_of(a) must return 0 for a >= C.
template <class NA>
__device__ __forceinline__ void mnk_pick_by_visits(int C, uint32_t x, bool by_count, uint32_t maxn, uint32_t tot, int lane,
                                                   NA na_of, int& move) {
  uint32_t r = 0u;
  if (by_count) {
    r = __umulhi(x, tot);
  } else {
    uint32_t ns = 0u;
    for (int a0 = 0; a0 < C; a0 += 64) {
      const int a = a0 + lane;
      const bool in = na_of(a) == maxn;
      ns += (uint32_t)__popcll(__ballot(in));
    }
    r = __umulhi(x, ns);
  }
  uint32_t before = 0u;  // (by_count: the visits of the chunks before; else: the members of S before)
  for (int a0 = 0; a0 < C; a0 += 64) {
    const int a = a0 + lane;
    const uint32_t na = na_of(a);
    uint64_t hit;
    if (by_count) {
      uint32_t cum = na;  // inclusive scan over the chunk
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)cum, off, 64);
        if (lane >= off) cum += o;
      }
      hit = __ballot(before + cum > r);
      before += (uint32_t)__shfl((int)cum, 63, 64);
    } else {
      const uint64_t in = __ballot(na == maxn && na != 0u);
      const uint32_t cnt = (uint32_t)__popcll(in);
      if (r < before + cnt) {
        uint64_t b = in;
        for (uint32_t s = before; s < r; ++s) b &= b - 1;  // drop the members before the r-th
        hit = b;
      } else {
        hit = 0;
      }
      before += cnt;
    }
    if (hit) {
      move = a0 + (int)__ffsll((unsigned long long)hit) - 1;
      break;
    }
  }
}
