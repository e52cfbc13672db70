// mnk_search_selfplay_advance.h -- what the launches of search self-play with per-row budgets share (gfx950 / MI355X
// only): the argument block, the host's check of it and the launch shape, and the self-play steps of a row as device
// functions that every advance kernel inlines -- k_search_selfplay_advance, _opts and _keep
// (mnk_search_selfplay_async.hip), _leaves (mnk_search_selfplay_async_leaves.hip) and _gumbel
// (mnk_search_selfplay_async_gumbel.hip): the budget draw, the root's noise and visit counts, the end of a ply, the fresh
// root, the error row.  What a row does as a PUCT tree -- its view of the workspace, the clamped header, the stage's
// planes, a selection's write-out -- is mnk_puct_tree.h's, shared with the lockstep player (mnk_puct.hip).  A kernel body
// is a short composition of these pieces around what is its own; a change to the outcome labels, the error row or the
// budget draw is made here, once.  The rule: include/mnk_hip.h, mnk_search_selfplay_advance.
//
// The shape of every kernel: one wave per row, MNK_PUCT_ROWS rows per workgroup, no workgroup barrier (which branch a row
// takes is wave-uniform; the rows of a workgroup diverge), `pos` the wave's own LDS stage of 2 * NW words
// (mnk_puct_tree.h).  A piece that writes or reads pos says which row_wave_sync() its caller owes.
#pragma once
#include "mnk_puct_noise.h"
#include "mnk_puct_tree.h"

// ================================================================== the argument block
// What every advance kernel takes, as its first parameter; a kernel's own parameters follow it.  I: the full budget (and,
// but for the keep kernel, the workspace's layout parameter).  temp_plies: unused by the Gumbel kernel (0).
struct MnkAdvanceArgs {
  MnkGeom g;
  unsigned char* ws;
  uint64_t* planes;
  uint32_t* meta;
  int64_t N;
  int I, I_fast;
  uint64_t full_threshold;
  const void* priors;
  int priors_dtype;
  const void* values;
  int values_dtype;
  float c;
  int temp_plies;
  uint64_t seed;
  const uint64_t* seed_dev;
  int64_t env_id0;
  unsigned long long* row_plies;
  int64_t T;
  uint64_t* ring_planes;
  uint16_t* ring_visits;
  int8_t* ring_z;
  void* leaf_obs;
  int leaf_dtype;
  uint8_t* leaf_mask;
  uint8_t* fresh;
  unsigned long long* plies_max;
  unsigned long long* stats;
  int32_t* err;
};

// ================================================================== the host side
// the common arguments of a C entry point, under the names the public header gives them in every one, for
// mnk_advance_check; TEMP_PLIES: the entry point's temp_plies, or 0 where it has none
#define MNK_ADVANCE_COMMON(TEMP_PLIES)                                                                                  \
  workspace, planes, meta, N, m, n, k, iterations, fast_iterations, full_threshold, priors, priors_dtype, values,       \
      values_dtype, c, TEMP_PLIES, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits, ring_z, leaf_obs,   \
      leaf_dtype, leaf_mask, fresh, plies_max, stats, err

// What every entry point refuses: the board's code, else MNK_EINVAL.  MNK_OK: `a` is filled.
inline int mnk_advance_check(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                             int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                             int priors_dtype, const void* values, int values_dtype, float c, int temp_plies, uint64_t seed,
                             const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies, int64_t T,
                             uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype,
                             uint8_t* leaf_mask, uint8_t* fresh, uint64_t* plies_max, int64_t* stats, int32_t* err,
                             MnkAdvanceArgs* a) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  const bool dt_ok = (priors_dtype == MNK_LOGITS_F32 || priors_dtype == MNK_LOGITS_BF16) &&
                     (values_dtype == MNK_LOGITS_F32 || values_dtype == MNK_LOGITS_BF16);
  if (!workspace || !planes || !meta || !priors || !values || !row_plies || !ring_planes || !ring_visits || !ring_z ||
      !leaf_obs || !leaf_mask || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_ROWS || !dt_ok ||
      !mnk_obs_dtype_ok(leaf_dtype) || fast_iterations < 1 || fast_iterations > iterations ||
      iterations > MNK_PUCT_ITERS_MAX || full_threshold > (1ull << 32) || !(c >= 0.0f && c <= 3.0e38f) || T < g.C ||
      temp_plies < 0)
    return MNK_EINVAL;
  *a = MnkAdvanceArgs{g, (unsigned char*)workspace, planes, meta, N, iterations, fast_iterations, full_threshold, priors,
                      priors_dtype, values, values_dtype, c, temp_plies, seed, seed_dev, env_id0,
                      (unsigned long long*)row_plies, T, ring_planes, ring_visits, ring_z, leaf_obs, leaf_dtype, leaf_mask,
                      fresh, (unsigned long long*)plies_max, (unsigned long long*)stats, err};
  return MNK_OK;
}

// the option group of the opts, keep and leaves entry points
inline int mnk_advance_options_check(const MnkGeom& g, int solver, float noise_alpha, float noise_eps, int noise_fast) {
  if ((solver != 0 && solver != 1) || !(noise_alpha == 0.0f || (noise_alpha > 0.0f && noise_alpha <= 3.0e38f)) ||
      !(noise_eps >= 0.0f && noise_eps <= 1.0f) || (noise_fast != 0 && noise_fast != 1) ||
      g.C > MNK_PUCT_NOISE_CELLS_MAX)
    return MNK_EINVAL;
  return MNK_OK;
}
inline bool mnk_advance_fpu_ok(float fpu, float fpu_root) {
  return fpu >= 0.0f && fpu <= 3.0e38f && fpu_root >= 0.0f && fpu_root <= 3.0e38f;
}
inline MnkPuctNoise mnk_advance_noise(float noise_alpha) {
  return noise_alpha > 0.0f ? mnk_puct_noise_params(noise_alpha) : MnkPuctNoise{0.0, 0.0, 0.0};
}
// the noise's dynamic LDS: a root's log-gammas, [MNK_PUCT_ROWS][C] doubles
inline size_t mnk_advance_noise_lds(const MnkGeom& g, float noise_alpha) {
  return noise_alpha > 0.0f ? (size_t)MNK_PUCT_ROWS * g.C * sizeof(double) : 0;
}

// the one launch shape (a.N > 0): the block, then the kernel's own parameters
template <typename... P, typename... A>
inline void mnk_advance_launch(void (*kernel)(MnkAdvanceArgs, P...), const MnkAdvanceArgs& a, size_t lds, void* stream,
                               const A&... own) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((a.N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), dim3(64 * MNK_PUCT_ROWS), lds,
                     (hipStream_t)stream, a, own...);
}

// ================================================================== the wave's stage
// the canonical position of e (plane 0 = the side to move) into pos, by lane 0.  The caller owes a row_wave_sync() before
// it (every lane is done with what the stage held) and one after it.
template <int NW>
__device__ __forceinline__ void stage_env(uint32_t* pos, const MnkEnv<NW>& e, int lane) {
  if (lane == 0) {
    const uint32_t s = e.meta & 1u;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      pos[w] = s ? e.p[1][w] : e.p[0][w];
      pos[NW + w] = s ? e.p[0][w] : e.p[1][w];
    }
  }
}

// ================================================================== the budget of the row's ply
// a function of (seed, row id, the row's ply) alone.  seed: the launch's, seed_dev's when there is one.
struct MnkAdvanceBudget {
  uint64_t seed, p;
  bool full;
};
__device__ __forceinline__ MnkAdvanceBudget advance_budget(const MnkAdvanceArgs& a, int64_t i) {
  MnkAdvanceBudget b;
  b.seed = a.seed_dev ? *a.seed_dev : a.seed;
  b.p = a.row_plies[i];
  const uint32_t u = mnk_rand_u32(b.seed, (uint64_t)(a.env_id0 + i), b.p, MNK_STREAM_BUDGET);
  b.full = (uint64_t)u < a.full_threshold;
  return b;
}

// ================================================================== the root's noise
// After the backup of evaluation 0 (eval0: the caller's test of the slot's state; what puct_row_fresh, the carry and
// mnk_puct_begin leave pending), the root in pos: the root's prior row -- node 0's -- takes the noised priors on its free
// cells, and root_priors what the root then holds.  br: the evaluation's batch row of priors.  gamma: the wave's C doubles
// of dynamic LDS.  A lane rewrites the cells it wrote in the backup and reads in the selection: no sync of its own.
template <int NW, int CN>
__device__ __forceinline__ void advance_root_noise(const MnkAdvanceArgs& a, const MnkAdvanceBudget& bg, bool eval0,
                                                   const uint32_t* pos, float* prior, int64_t i, int64_t br,
                                                   const MnkPuctNoise& nz, float noise_eps, int noise_fast,
                                                   float* root_priors, double* gamma, int lane) {
  if (!eval0 || !(nz.alpha > 0.0 || root_priors)) return;
  const int C = a.g.C;
  auto is_free = [&](int q) { return !(row_stone<CN>(a.g, pos, q) || row_stone<CN>(a.g, pos + NW, q)); };
  auto prior_of = [&](int q) { return puct_read(a.priors, a.priors_dtype, br * C + q); };
  auto store = [&](int q, float pa) {
    if (is_free(q)) prior[q] = pa;
    if (root_priors) root_priors[i * C + q] = pa;
  };
  if (nz.alpha > 0.0 && (bg.full || noise_fast))
    puct_noise_row(C, is_free, prior_of, store, bg.seed, (uint64_t)(a.env_id0 + i), bg.p, nz.alpha, nz.d, nz.c, noise_eps,
                   gamma, lane);
  else if (root_priors)
    for (int q = lane; q < C; q += 64) root_priors[i * C + q] = prior_of(q);
}

// ================================================================== the root's visit counts
// visits_of(cell): the visits of the root's child through a cell of a row whose position is in pos, 0 on an occupied cell
// and for a cell >= C.  SOLVER: the count under `keep` (puct_root_keep), which advance_root_visits sets.
template <int NW, int CN, bool SOLVER>
struct MnkAdvanceVisits {
  const MnkGeom& g;
  const uint32_t* pos;
  const MnkPuctNode* node;
  const uint16_t* child;
  int nodes;
  int keep;
  __device__ __forceinline__ uint32_t operator()(int q) const {
    if (q >= g.C || row_stone<CN>(g, pos, q) || row_stone<CN>(g, pos + NW, q)) return 0u;
    if constexpr (SOLVER) {
      return min(puct_kept_count(puct_root_kid(g.C, node, child, nodes, true, q), keep), 65535u);
    } else {
      const uint32_t ch = child[q];
      return (ch != 0u && ch != MNK_PUCT_NONE) ? min(node[min((int)ch, nodes - 1)].n, 65535u) : 0u;
    }
  }
};
// their maximum (the same in every lane: a scalar branch) and their sum, the position before the ply staged in pos
template <int NW, int CN, bool SOLVER>
__device__ __forceinline__ void advance_root_visits(MnkAdvanceVisits<NW, CN, SOLVER>& visits_of, int lane, uint32_t& maxn,
                                                    uint32_t& tot) {
  if constexpr (SOLVER)
    visits_of.keep = puct_root_keep(visits_of.g.C, visits_of.node, visits_of.child, visits_of.nodes, true, lane, maxn, tot);
  maxn = 0u;
  tot = 0u;
  for (int q = lane; q < visits_of.g.C; q += 64) {
    const uint32_t na = visits_of(q);
    maxn = max(maxn, na);
    tot += na;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
    tot += (uint32_t)__shfl_xor((int)tot, off, 64);
  }
  maxn = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxn);
}

// ================================================================== the end of a ply
// The row plays `move` at its ply p, ring row t = p mod T: the ring's planes (the canonical position before the ply, in
// pos), the move, ring_z of the ply, the labels of a game that ends, the statistics, the reset, the env's store, the
// row's ply count, plies_max, fresh.  Returns the ply, e the position reached (cleared after a game's end).  The caller
// has stored the ring's visit row; it owes a row_wave_sync() before pos is written again.
template <int NW, int CN, int CK>
__device__ __forceinline__ MnkPly advance_finish_ply(const MnkAdvanceArgs& a, MnkEnv<NW>& e, const uint32_t* pos, int move,
                                                     uint64_t p, int64_t t, int64_t i, int lane) {
  const int64_t N = a.N, T = a.T;
  const int W = a.g.W;
  const uint32_t side = e.meta & 1u, moves = e.meta >> 1;
  if (lane == 0) {
    uint64_t* rp = a.ring_planes + t * 2 * W * N;
    uint32_t pl[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) pl[w] = pos[w];
    plane_store<NW>(pl, rp, N, W, i);
#pragma unroll
    for (int w = 0; w < NW; ++w) pl[w] = pos[NW + w];
    plane_store<NW>(pl, rp + (int64_t)W * N, N, W, i);
  }
  const MnkPly ply = env_play<NW, CN, CK, true>(a.g, e, move, false);
  if (lane == 0) a.ring_z[t * N + i] = ply.done ? (int8_t)(ply.win ? 1 : 0) : (int8_t)MNK_Z_UNKNOWN;
  if (ply.done) {
    // records t - d (mod T), d = 1 .. L - 1, of this game: the view of the side to move there; T >= C >= L
    const int64_t Lg = min((int64_t)moves + 1, T);
    const int8_t zw = ply.win ? 1 : 0;
    for (int64_t d = 1 + lane; d < Lg; d += 64) {
      const int64_t r = t >= d ? t - d : t + T - d;
      a.ring_z[r * N + i] = (d & 1) ? (int8_t)-zw : zw;
    }
    if (a.stats && lane == 0) {
      unsigned long long* s = a.stats + (size_t)(blockIdx.x % MNK_STATS_REPLICAS) * MNK_STATS_STRIDE;
      atomicAdd(&s[0], 1ull);
      atomicAdd(&s[ply.win ? 1 + side : 3], 1ull);
      atomicAdd(&s[4], (unsigned long long)moves + 1ull);
    }
    env_clear<NW>(e);
  }
  if (lane == 0) {
    env_store<NW>(e, a.planes, a.meta, N, W, i);
    a.row_plies[i] = p + 1ull;
    if (a.plies_max) atomicMax(a.plies_max, (unsigned long long)(p + 1ull));
    if (a.fresh) a.fresh[i] = 1;
  }
  return ply;
}

// the search of the position reached, e: a fresh tree, its root the pending leaf, shown as batch row b.  The syncs around
// the staging are inside.
template <int NW, int CN>
__device__ __forceinline__ void advance_fresh_root(const MnkAdvanceArgs& a, const MnkPuctRow& r, uint32_t* pos,
                                                   const MnkEnv<NW>& e, int64_t b, int lane) {
  row_wave_sync();  // (every lane is done with the position before this ply)
  stage_env<NW>(pos, e, lane);
  row_wave_sync();
  puct_row_fresh<NW>(r.row, r.L, pos, a.g.NW, (int)(e.meta >> 1) < a.g.C, lane);
  row_write_view<NW, CN>(a.g, pos, 0, b, a.leaf_obs, a.leaf_dtype, a.leaf_mask, lane);
}

// ================================================================== the error row
// a root without a legal cell (or, of a workspace that is not this position's, without a move on a free cell): reported,
// left alone, the root shown again in `count` batch rows from b.  The syncs around the staging are inside.
template <int NW, int CN>
__device__ __forceinline__ void advance_error_row(const MnkAdvanceArgs& a, const MnkPuctRow& r, uint32_t* pos, int64_t i,
                                                  int64_t b, int count, int lane) {
  if (lane == 0) {
    mnk_report(a.err, MNK_ERR_VISITS, i);
    if (a.fresh) a.fresh[i] = 0;
  }
  row_wave_sync();
  puct_stage_planes<NW>(pos, r.root, a.g.NW, lane);
  row_wave_sync();
  for (int j = 0; j < count; ++j)
    row_write_view<NW, CN>(a.g, pos, 0, b + j, a.leaf_obs, a.leaf_dtype, a.leaf_mask, lane);
}
