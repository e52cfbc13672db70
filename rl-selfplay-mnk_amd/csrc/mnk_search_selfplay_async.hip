// mnk_search_selfplay_async.hip -- search self-play with per-row search budgets (gfx950 / MI355X only): ONE launch per
// evaluator call.  Row i backs up its pending evaluation (mnk_puct_step's backup), and then either selects its next leaf
// (mnk_puct_step's selection) or, when the budget of its current ply is spent, plays the ply in the same launch
// (mnk_search_selfplay_step's rule with the row's own ply count in the place of the global one) and starts the search of
// the position it reached.  Rows finish their searches at different times and go on at once; the budget of a ply is a
// function of (seed, row id, the row's ply) alone, so nothing but the tree and the ply count is kept.  The rule:
// include/mnk_hip.h, mnk_search_selfplay_advance.
//
// mnk_search_selfplay_advance_opts is the same launch with two of the lockstep player's options built in: Dirichlet noise
// on the roots (mnk_puct_root_noise's draw, at the backup of a fresh tree's root) and the solver (mnk_puct_step_solver's
// backup and selection; a ply ends as soon as its root is proven).  It has a kernel of its own,
// k_search_selfplay_advance_opts, so that the plain launch above it keeps its code.
//
// mnk_search_selfplay_advance_keep is the launch with the options for rows that keep the played move's subtree from ply
// to ply (the lockstep player's mnk_puct_rebase, inside the launch that plays the ply): again a kernel of its own,
// k_search_selfplay_advance_keep, and the two above keep their code.
#include "mnk_host.h"
#include "mnk_puct_noise.h"
#include "mnk_puct_tree.h"

// One wave per row, MNK_PUCT_ROWS rows per workgroup.  Which branch a row takes is wave-uniform; the rows of a workgroup
// diverge, so the kernel has no workgroup barrier: a row's LDS stage and its workspace are its own wave's alone.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int I, int I_fast,
                          uint64_t full_threshold, const void* priors, int priors_dtype, const void* values,
                          int values_dtype, float c, int temp_plies, uint64_t seed, const uint64_t* seed_dev,
                          int64_t env_id0, unsigned long long* row_plies, int64_t T, uint64_t* ring_planes,
                          uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask,
                          uint8_t* fresh, unsigned long long* plies_max, unsigned long long* stats, int32_t* err) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW, W = g.W;
  const MnkPuctLayout L = mnk_puct_layout(NWg, C, I);
  unsigned char* row = ws + i * L.row;
  uint32_t* hdr = (uint32_t*)row;
  const uint32_t* root = (const uint32_t*)(row + L.root);
  uint32_t* leafp = (uint32_t*)(row + L.leaf);
  uint16_t* path = (uint16_t*)(row + L.path);
  MnkPuctNode* node = (MnkPuctNode*)(row + L.node);
  float* prior = (float*)(row + L.prior);
  uint16_t* child = (uint16_t*)(row + L.child);
  uint32_t* pos = lds_pos[wave];
  // (clamped, as in k_puct_step: whatever the workspace holds, no id leaves the row)
  int nodes = (int)min(max(hdr[0], 1u), (uint32_t)(I + 1));
  const int depth = (int)min(hdr[1], (uint32_t)I);
  const uint32_t state = hdr[2];
  const bool live = hdr[3] != 0u;
  for (int q = lane; q < 2 * NW; q += 64) {
    const int pl = q >= NW, w = q - (pl ? NW : 0);
    pos[q] = w < NWg ? leafp[pl * NWg + w] : 0u;
  }
  row_wave_sync();

  // ---- backup of the pending evaluation
  if (live && (state & 1u))
    puct_backup<NW, CN>(g, pos, path, node, prior, child, nodes, depth, state, priors, priors_dtype, values, values_dtype,
                        i, lane);

  // ---- the budget of the row's ply, and whether it is spent
  if (seed_dev) seed = *seed_dev;
  const uint64_t p = row_plies[i];
  const uint32_t u = mnk_rand_u32(seed, (uint64_t)(env_id0 + i), p, MNK_STREAM_BUDGET);
  const bool full = (uint64_t)u < full_threshold;
  const uint32_t n_root = node[0].n;
  const bool spent = n_root != 0u && n_root - 1u >= (uint32_t)(full ? I : I_fast);

  uint32_t maxn = 0u, tot = 0u;
  // the visits of the root's child through cell a of a row whose position is in pos: 0 on an occupied cell
  auto visits_of = [&](int a) {
    if (a >= C || row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a)) return 0u;
    const uint32_t ch = child[a];
    return (ch != 0u && ch != MNK_PUCT_NONE) ? min(node[min((int)ch, nodes - 1)].n, 65535u) : 0u;
  };
  MnkEnv<NW> e;
  if (__builtin_amdgcn_readfirstlane((int)(live && spent))) {
    // the position before the ply: in registers, and canonical (plane 0 = the side to move) in LDS
    env_load<NW>(e, planes, meta, N, W, i);
    row_wave_sync();  // (every lane is done with the leaf's planes)
    if (lane == 0) {
      const uint32_t s = e.meta & 1u;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = s ? e.p[1][w] : e.p[0][w];
        pos[NW + w] = s ? e.p[0][w] : e.p[1][w];
      }
    }
    row_wave_sync();
    for (int a = lane; a < C; a += 64) {
      const uint32_t na = visits_of(a);
      maxn = max(maxn, na);
      tot += na;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
      tot += (uint32_t)__shfl_xor((int)tot, off, 64);
    }
    maxn = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxn);  // (the same in every lane: a scalar branch)
  }

  if (maxn) {
    // ---- the ply ends in this launch: ring row t = p mod T, the move, the outcome labels, the reset
    const int64_t t = (int64_t)(p % (uint64_t)T);
    const uint32_t x = mnk_rand_u32(seed, (uint64_t)(env_id0 + i), p, MNK_STREAM_SELFPLAY);
    const uint32_t side = e.meta & 1u, moves = e.meta >> 1;
    uint16_t* rv = ring_visits + (t * N + i) * C;
    for (int a = lane; a < C; a += 64) rv[a] = full ? (uint16_t)visits_of(a) : (uint16_t)0;  // a fast ply: no policy target
    if (lane == 0) {  // (the canonical planes are in LDS already)
      uint64_t* rp = ring_planes + t * 2 * W * N;
      uint32_t pl[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) pl[w] = pos[w];
      plane_store<NW>(pl, rp, N, W, i);
#pragma unroll
      for (int w = 0; w < NW; ++w) pl[w] = pos[NW + w];
      plane_store<NW>(pl, rp + (int64_t)W * N, N, W, i);
    }
    int move = 0;
    mnk_pick_by_visits(C, x, (int64_t)moves < (int64_t)temp_plies, maxn, tot, lane, visits_of, move);
    const MnkPly ply = env_play<NW, CN, CK, true>(g, e, move, false);
    if (lane == 0) ring_z[t * N + i] = ply.done ? (int8_t)(ply.win ? 1 : 0) : (int8_t)MNK_Z_UNKNOWN;
    if (ply.done) {
      // records t - d (mod T), d = 1 .. L - 1, of this game: the view of the side to move there; T >= C >= L
      const int64_t Lg = min((int64_t)moves + 1, T);
      const int8_t zw = ply.win ? 1 : 0;
      for (int64_t d = 1 + lane; d < Lg; d += 64) {
        const int64_t r = t >= d ? t - d : t + T - d;
        ring_z[r * N + i] = (d & 1) ? (int8_t)-zw : zw;
      }
      if (stats && lane == 0) {
        unsigned long long* s = stats + (size_t)(blockIdx.x % MNK_STATS_REPLICAS) * MNK_STATS_STRIDE;
        atomicAdd(&s[0], 1ull);
        atomicAdd(&s[ply.win ? 1 + side : 3], 1ull);
        atomicAdd(&s[4], (unsigned long long)moves + 1ull);
      }
      env_clear<NW>(e);
    }
    if (lane == 0) {
      env_store<NW>(e, planes, meta, N, W, i);
      row_plies[i] = p + 1ull;
      if (plies_max) atomicMax(plies_max, (unsigned long long)(p + 1ull));
      if (fresh) fresh[i] = 1;
    }
    // ---- the search of the position reached: a fresh tree, its root the pending leaf
    row_wave_sync();  // (every lane is done with the position before this ply)
    if (lane == 0) {
      const uint32_t ns = e.meta & 1u;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = ns ? e.p[1][w] : e.p[0][w];
        pos[NW + w] = ns ? e.p[0][w] : e.p[1][w];
      }
    }
    row_wave_sync();
    puct_row_fresh<NW>(row, L, pos, NWg, (int)(e.meta >> 1) < C, lane);
    row_write_view<NW, CN>(g, pos, 0, i, leaf_obs, leaf_dtype, leaf_mask, lane);
    return;
  }

  if (!live || spent) {
    // ---- a root without a legal cell (or, of a workspace that is not this position's, without a visit on a free cell):
    // reported, left alone, shown again
    if (lane == 0) {
      mnk_report(err, MNK_ERR_VISITS, i);
      if (fresh) fresh[i] = 0;
    }
    row_wave_sync();
    for (int q = lane; q < 2 * NW; q += 64) {
      const int pl = q >= NW, w = q - (pl ? NW : 0);
      pos[q] = w < NWg ? root[pl * NWg + w] : 0u;
    }
    row_wave_sync();
    row_write_view<NW, CN>(g, pos, 0, i, leaf_obs, leaf_dtype, leaf_mask, lane);
    return;
  }

  // ---- selection: k_puct_step's
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a full tree shows its root again (it cannot happen: nodes <= n_root <= I)
  if (nodes <= I) {
    puct_env_root<NW>(e, root, NWg);
    nstate = puct_walk<NW, CN, CK, false>(g, e, I, c, node, prior, child, path, nodes, d, lane);
    if (nstate == 0u) d = 0;
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = nstate ? e.p[0][w] : (w < NWg ? root[w] : 0u);
        pos[NW + w] = nstate ? e.p[1][w] : (w < NWg ? root[NWg + w] : 0u);
      }
    }
  } else if (lane == 0) {
    for (int q = 0; q < 2 * NW; ++q) {
      const int pl = q >= NW, w = q - (pl ? NW : 0);
      pos[q] = w < NWg ? root[pl * NWg + w] : 0u;
    }
  }
  if (lane == 0) {
    path[0] = 0;
    hdr[0] = (uint32_t)nodes;
    hdr[1] = (uint32_t)d;
    hdr[2] = nstate;
    if (fresh) fresh[i] = 0;
    // no leaf: nothing is pending, so n_root cannot advance and the row would show its root for ever.  It cannot happen
    // in a workspace that mnk_puct_begin set up (nodes <= n_root <= I while the budget is unspent): reported, not silent
    if (nstate == 0u) mnk_report(err, MNK_ERR_VISITS, i);
  }
  row_wave_sync();
  for (int q = lane; q < 2 * NWg; q += 64) leafp[q] = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
  row_write_view<NW, CN>(g, pos, d & 1, i, leaf_obs, leaf_dtype, leaf_mask, lane);
}

// k_search_selfplay_advance with the options (the rule: include/mnk_hip.h, mnk_search_selfplay_advance_opts).  The same
// shape: one wave per row, no workgroup barrier, every id clamped to the row.  SOLVER is a template flag (it changes
// puct_walk's inner loop); the noise is a wave-uniform run-time branch that only a wave whose pending leaf is the root of
// a fresh tree takes, once per ply.  nz.alpha = 0: no noise, and then the launch has no dynamic LDS.
// The launch's row is a device function, search_selfplay_advance_opts_row, so that the kernel with first-play urgency
// (FPU: puct_walk's, the rule: include/mnk_hip.h, mnk_puct_step_fpu) is the same text; k_search_selfplay_advance_opts
// below is its FPU = false form behind the parameter list it always had.
template <int NW, int CN, int CK, bool SOLVER, bool FPU>
__device__ __forceinline__ void
search_selfplay_advance_opts_row(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int I,
                               int I_fast, uint64_t full_threshold, const void* priors, int priors_dtype,
                               const void* values, int values_dtype, float c, int temp_plies, uint64_t seed,
                               const uint64_t* seed_dev, int64_t env_id0, unsigned long long* row_plies, int64_t T,
                               uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype,
                               uint8_t* leaf_mask, uint8_t* fresh, unsigned long long* plies_max, unsigned long long* stats,
                               int32_t* err, MnkPuctNoise nz, float noise_eps, int noise_fast, float* root_priors, float fpu,
                               float fpu_root) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  extern __shared__ double lds_gamma[];  // with noise: [MNK_PUCT_ROWS][C], a root's log-gammas between the two passes
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW, W = g.W;
  const MnkPuctLayout L = mnk_puct_layout(NWg, C, I);
  unsigned char* row = ws + i * L.row;
  uint32_t* hdr = (uint32_t*)row;
  const uint32_t* root = (const uint32_t*)(row + L.root);
  uint32_t* leafp = (uint32_t*)(row + L.leaf);
  uint16_t* path = (uint16_t*)(row + L.path);
  MnkPuctNode* node = (MnkPuctNode*)(row + L.node);
  float* prior = (float*)(row + L.prior);
  uint16_t* child = (uint16_t*)(row + L.child);
  uint32_t* pos = lds_pos[wave];
  // (clamped, as in k_puct_step: whatever the workspace holds, no id leaves the row)
  int nodes = (int)min(max(hdr[0], 1u), (uint32_t)(I + 1));
  const int depth = (int)min(hdr[1], (uint32_t)I);
  const uint32_t state = hdr[2];
  const bool live = hdr[3] != 0u;
  for (int q = lane; q < 2 * NW; q += 64) {
    const int pl = q >= NW, w = q - (pl ? NW : 0);
    pos[q] = w < NWg ? leafp[pl * NWg + w] : 0u;
  }
  row_wave_sync();

  // ---- the budget of the row's ply (before the backup: whether a root is noised depends on it)
  if (seed_dev) seed = *seed_dev;
  const uint64_t p = row_plies[i];
  const uint32_t u = mnk_rand_u32(seed, (uint64_t)(env_id0 + i), p, MNK_STREAM_BUDGET);
  const bool full = (uint64_t)u < full_threshold;

  // ---- backup of the pending evaluation
  if (live && (state & 1u))
    puct_backup<NW, CN, SOLVER>(g, pos, path, node, prior, child, nodes, depth, state, priors, priors_dtype, values,
                                values_dtype, i, lane);
  // evaluation 0 (what puct_row_fresh and mnk_puct_begin leave pending): the root's prior row -- node 0's -- takes the
  // noised priors on its free cells, and root_priors what the root then holds.  A lane rewrites the cells it wrote in the
  // backup and reads in the selection: no further sync.
  if (live && state == 1u && depth == 0 && (nz.alpha > 0.0 || root_priors)) {
    auto is_free = [&](int a) { return !(row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a)); };
    auto prior_of = [&](int a) { return puct_read(priors, priors_dtype, i * C + a); };
    auto store = [&](int a, float pa) {
      if (is_free(a)) prior[a] = pa;
      if (root_priors) root_priors[i * C + a] = pa;
    };
    if (nz.alpha > 0.0 && (full || noise_fast))
      puct_noise_row(C, is_free, prior_of, store, seed, (uint64_t)(env_id0 + i), p, nz.alpha, nz.d, nz.c, noise_eps,
                     lds_gamma + wave * C, lane);
    else if (root_priors)
      for (int a = lane; a < C; a += 64) root_priors[i * C + a] = prior_of(a);
  }

  // ---- whether the ply ends: the budget is spent, or (SOLVER) the root has a proof
  const uint32_t n_root = node[0].n;
  bool spent = n_root != 0u && n_root - 1u >= (uint32_t)(full ? I : I_fast);
  if constexpr (SOLVER) spent |= n_root != 0u && MNK_PUCT_PROOF(node[0].info) != 0u;

  uint32_t maxn = 0u, tot = 0u;
  [[maybe_unused]] int keep = 0;  // SOLVER: which of the root's children count (puct_root_keep)
  // the visits of the root's child through cell a of a row whose position is in pos: 0 on an occupied cell
  auto visits_of = [&](int a) -> uint32_t {
    if (a >= C || row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a)) return 0u;
    if constexpr (SOLVER) {
      return min(puct_kept_count(puct_root_kid(C, node, child, nodes, true, a), keep), 65535u);
    } else {
      const uint32_t ch = child[a];
      return (ch != 0u && ch != MNK_PUCT_NONE) ? min(node[min((int)ch, nodes - 1)].n, 65535u) : 0u;
    }
  };
  MnkEnv<NW> e;
  if (__builtin_amdgcn_readfirstlane((int)(live && spent))) {
    // the position before the ply: in registers, and canonical (plane 0 = the side to move) in LDS
    env_load<NW>(e, planes, meta, N, W, i);
    row_wave_sync();  // (every lane is done with the leaf's planes)
    if (lane == 0) {
      const uint32_t s = e.meta & 1u;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = s ? e.p[1][w] : e.p[0][w];
        pos[NW + w] = s ? e.p[0][w] : e.p[1][w];
      }
    }
    row_wave_sync();
    if constexpr (SOLVER) keep = puct_root_keep(C, node, child, nodes, true, lane, maxn, tot);
    maxn = 0u;
    tot = 0u;
    for (int a = lane; a < C; a += 64) {
      const uint32_t na = visits_of(a);
      maxn = max(maxn, na);
      tot += na;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
      tot += (uint32_t)__shfl_xor((int)tot, off, 64);
    }
    maxn = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxn);  // (the same in every lane: a scalar branch)
  }

  if (maxn) {
    // ---- the ply ends in this launch: ring row t = p mod T, the move, the outcome labels, the reset
    const int64_t t = (int64_t)(p % (uint64_t)T);
    const uint32_t x = mnk_rand_u32(seed, (uint64_t)(env_id0 + i), p, MNK_STREAM_SELFPLAY);
    const uint32_t side = e.meta & 1u, moves = e.meta >> 1;
    uint16_t* rv = ring_visits + (t * N + i) * C;
    for (int a = lane; a < C; a += 64) rv[a] = full ? (uint16_t)visits_of(a) : (uint16_t)0;  // a fast ply: no policy target
    if (lane == 0) {  // (the canonical planes are in LDS already)
      uint64_t* rp = ring_planes + t * 2 * W * N;
      uint32_t pl[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) pl[w] = pos[w];
      plane_store<NW>(pl, rp, N, W, i);
#pragma unroll
      for (int w = 0; w < NW; ++w) pl[w] = pos[NW + w];
      plane_store<NW>(pl, rp + (int64_t)W * N, N, W, i);
    }
    int move = 0;
    mnk_pick_by_visits(C, x, (int64_t)moves < (int64_t)temp_plies, maxn, tot, lane, visits_of, move);
    const MnkPly ply = env_play<NW, CN, CK, true>(g, e, move, false);
    if (lane == 0) ring_z[t * N + i] = ply.done ? (int8_t)(ply.win ? 1 : 0) : (int8_t)MNK_Z_UNKNOWN;
    if (ply.done) {
      // records t - d (mod T), d = 1 .. L - 1, of this game: the view of the side to move there; T >= C >= L
      const int64_t Lg = min((int64_t)moves + 1, T);
      const int8_t zw = ply.win ? 1 : 0;
      for (int64_t d = 1 + lane; d < Lg; d += 64) {
        const int64_t r = t >= d ? t - d : t + T - d;
        ring_z[r * N + i] = (d & 1) ? (int8_t)-zw : zw;
      }
      if (stats && lane == 0) {
        unsigned long long* s = stats + (size_t)(blockIdx.x % MNK_STATS_REPLICAS) * MNK_STATS_STRIDE;
        atomicAdd(&s[0], 1ull);
        atomicAdd(&s[ply.win ? 1 + side : 3], 1ull);
        atomicAdd(&s[4], (unsigned long long)moves + 1ull);
      }
      env_clear<NW>(e);
    }
    if (lane == 0) {
      env_store<NW>(e, planes, meta, N, W, i);
      row_plies[i] = p + 1ull;
      if (plies_max) atomicMax(plies_max, (unsigned long long)(p + 1ull));
      if (fresh) fresh[i] = 1;
    }
    // ---- the search of the position reached: a fresh tree (no proof), its root the pending leaf
    row_wave_sync();  // (every lane is done with the position before this ply)
    if (lane == 0) {
      const uint32_t ns = e.meta & 1u;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = ns ? e.p[1][w] : e.p[0][w];
        pos[NW + w] = ns ? e.p[0][w] : e.p[1][w];
      }
    }
    row_wave_sync();
    puct_row_fresh<NW>(row, L, pos, NWg, (int)(e.meta >> 1) < C, lane);
    row_write_view<NW, CN>(g, pos, 0, i, leaf_obs, leaf_dtype, leaf_mask, lane);
    return;
  }

  if (!live || spent) {
    // ---- a root without a legal cell (or, of a workspace that is not this position's, without a visit on a free cell):
    // reported, left alone, shown again
    if (lane == 0) {
      mnk_report(err, MNK_ERR_VISITS, i);
      if (fresh) fresh[i] = 0;
    }
    row_wave_sync();
    for (int q = lane; q < 2 * NW; q += 64) {
      const int pl = q >= NW, w = q - (pl ? NW : 0);
      pos[q] = w < NWg ? root[pl * NWg + w] : 0u;
    }
    row_wave_sync();
    row_write_view<NW, CN>(g, pos, 0, i, leaf_obs, leaf_dtype, leaf_mask, lane);
    return;
  }

  // ---- selection: k_puct_step's (SOLVER: k_puct_step_solver's at one leaf per row; the root has no proof here)
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a full tree shows its root again (it cannot happen: nodes <= n_root <= I)
  if (nodes <= I) {
    puct_env_root<NW>(e, root, NWg);
    nstate = puct_walk<NW, CN, CK, false, SOLVER, false, FPU>(g, e, I, c, node, prior, child, path, nodes, d, lane, 0, 0u,
                                                              nullptr, 0, nullptr, fpu, fpu_root);
    if (nstate == 0u) d = 0;
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = nstate ? e.p[0][w] : (w < NWg ? root[w] : 0u);
        pos[NW + w] = nstate ? e.p[1][w] : (w < NWg ? root[NWg + w] : 0u);
      }
    }
  } else if (lane == 0) {
    for (int q = 0; q < 2 * NW; ++q) {
      const int pl = q >= NW, w = q - (pl ? NW : 0);
      pos[q] = w < NWg ? root[pl * NWg + w] : 0u;
    }
  }
  if (lane == 0) {
    path[0] = 0;
    hdr[0] = (uint32_t)nodes;
    hdr[1] = (uint32_t)d;
    hdr[2] = nstate;
    if (fresh) fresh[i] = 0;
    // no leaf: nothing is pending, so n_root cannot advance and the row would show its root for ever: reported, not silent
    if (nstate == 0u) mnk_report(err, MNK_ERR_VISITS, i);
  }
  row_wave_sync();
  for (int q = lane; q < 2 * NWg; q += 64) leafp[q] = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
  row_write_view<NW, CN>(g, pos, d & 1, i, leaf_obs, leaf_dtype, leaf_mask, lane);
}

template <int NW, int CN, int CK, bool SOLVER>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_opts(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int I,
                               int I_fast, uint64_t full_threshold, const void* priors, int priors_dtype,
                               const void* values, int values_dtype, float c, int temp_plies, uint64_t seed,
                               const uint64_t* seed_dev, int64_t env_id0, unsigned long long* row_plies, int64_t T,
                               uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype,
                               uint8_t* leaf_mask, uint8_t* fresh, unsigned long long* plies_max, unsigned long long* stats,
                               int32_t* err, MnkPuctNoise nz, float noise_eps, int noise_fast, float* root_priors) {
  search_selfplay_advance_opts_row<NW, CN, CK, SOLVER, false>(
      g, ws, planes, meta, N, I, I_fast, full_threshold, priors, priors_dtype, values,
      values_dtype, c, temp_plies, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits, ring_z, leaf_obs,
      leaf_dtype, leaf_mask, fresh, plies_max, stats, err, nz, noise_eps, noise_fast, root_priors, 0.0f, 0.0f);
}
template <int NW, int CN, int CK, bool SOLVER>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_opts_fpu(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int I,
                                   int I_fast, uint64_t full_threshold, const void* priors, int priors_dtype,
                                   const void* values, int values_dtype, float c, int temp_plies, uint64_t seed,
                                   const uint64_t* seed_dev, int64_t env_id0, unsigned long long* row_plies, int64_t T,
                                   uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype,
                                   uint8_t* leaf_mask, uint8_t* fresh, unsigned long long* plies_max, unsigned long long* stats,
                                   int32_t* err, MnkPuctNoise nz, float noise_eps, int noise_fast, float* root_priors,
                                   float fpu, float fpu_root) {
  search_selfplay_advance_opts_row<NW, CN, CK, SOLVER, true>(
      g, ws, planes, meta, N, I, I_fast, full_threshold, priors, priors_dtype, values,
      values_dtype, c, temp_plies, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits, ring_z, leaf_obs,
      leaf_dtype, leaf_mask, fresh, plies_max, stats, err, nz, noise_eps, noise_fast, root_priors, fpu, fpu_root);
}

// k_search_selfplay_advance_opts for rows that keep the played move's subtree (the rule: include/mnk_hip.h,
// mnk_search_selfplay_advance_keep).  The same shape: one wave per row, no workgroup barrier, every id clamped to the row
// -- by TI = tree_iterations, the workspace's layout parameter; I stays the full budget.  The end of a ply calls
// puct_carry_subtree (mnk_puct_tree.h) on the root's child through the move, the position reached still in the wave's LDS
// stage.  Dynamic LDS: with noise [MNK_PUCT_ROWS][C] doubles, then the carry's two maps, [MNK_PUCT_ROWS][2][MS] u16 with
// MS = TI + 2 rounded up to even; the host sizes it (mnk_search_selfplay_advance_keep).
#ifndef MNK_KEEP_CARRY_B
#define MNK_KEEP_CARRY_B 8  // nodes in flight in the carry's copy loop (an experiment's knob: DESIGN section 5, row 34)
#endif
// (a device function for the same reason as search_selfplay_advance_opts_row)
template <int NW, int CN, int CK, bool SOLVER, bool FPU>
__device__ __forceinline__ void
search_selfplay_advance_keep_row(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int I,
                               int I_fast, uint64_t full_threshold, const void* priors, int priors_dtype,
                               const void* values, int values_dtype, float c, int temp_plies, uint64_t seed,
                               const uint64_t* seed_dev, int64_t env_id0, unsigned long long* row_plies, int64_t T,
                               uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype,
                               uint8_t* leaf_mask, uint8_t* fresh, unsigned long long* plies_max, unsigned long long* stats,
                               int32_t* err, MnkPuctNoise nz, float noise_eps, int noise_fast, float* root_priors, int TI,
                               int keep_nodes, int32_t* carried, float fpu, float fpu_root) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  extern __shared__ double lds_gamma[];  // with noise: [MNK_PUCT_ROWS][C], a root's log-gammas between the two passes;
                                         // behind them (or first) the carry's maps
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW, W = g.W;
  const MnkPuctLayout L = mnk_puct_layout(NWg, C, TI);
  unsigned char* row = ws + i * L.row;
  uint32_t* hdr = (uint32_t*)row;
  const uint32_t* root = (const uint32_t*)(row + L.root);
  uint32_t* leafp = (uint32_t*)(row + L.leaf);
  uint16_t* path = (uint16_t*)(row + L.path);
  MnkPuctNode* node = (MnkPuctNode*)(row + L.node);
  float* prior = (float*)(row + L.prior);
  uint16_t* child = (uint16_t*)(row + L.child);
  uint32_t* pos = lds_pos[wave];
  const int MS = (TI + 3) & ~1;
  uint16_t* map = (uint16_t*)(lds_gamma + (nz.alpha > 0.0 ? MNK_PUCT_ROWS * C : 0)) + (int64_t)wave * 2 * MS;
  uint16_t* inv = map + MS;
  // (clamped, as in k_puct_step: whatever the workspace holds, no id leaves the row)
  int nodes = (int)min(max(hdr[0], 1u), (uint32_t)(TI + 1));
  const int depth = (int)min(hdr[1], (uint32_t)TI);
  const uint32_t state = hdr[2];
  const bool live = hdr[3] != 0u;
  for (int q = lane; q < 2 * NW; q += 64) {
    const int pl = q >= NW, w = q - (pl ? NW : 0);
    pos[q] = w < NWg ? leafp[pl * NWg + w] : 0u;
  }
  row_wave_sync();

  // ---- the budget of the row's ply (before the backup: whether a root is noised depends on it)
  if (seed_dev) seed = *seed_dev;
  const uint64_t p = row_plies[i];
  const uint32_t u = mnk_rand_u32(seed, (uint64_t)(env_id0 + i), p, MNK_STREAM_BUDGET);
  const bool full = (uint64_t)u < full_threshold;

  // ---- backup of the pending evaluation
  if (live && (state & 1u))
    puct_backup<NW, CN, SOLVER>(g, pos, path, node, prior, child, nodes, depth, state, priors, priors_dtype, values,
                                values_dtype, i, lane);
  // evaluation 0 (what puct_row_fresh, the carry and mnk_puct_begin leave pending; bit 3, "renew", is not looked at): the
  // root's prior row -- node 0's -- takes the noised priors on its free cells, and root_priors what the root then holds.
  // A lane rewrites the cells it wrote in the backup and reads in the selection: no further sync.
  if (live && (state & ~8u) == 1u && depth == 0 && (nz.alpha > 0.0 || root_priors)) {
    auto is_free = [&](int a) { return !(row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a)); };
    auto prior_of = [&](int a) { return puct_read(priors, priors_dtype, i * C + a); };
    auto store = [&](int a, float pa) {
      if (is_free(a)) prior[a] = pa;
      if (root_priors) root_priors[i * C + a] = pa;
    };
    if (nz.alpha > 0.0 && (full || noise_fast))
      puct_noise_row(C, is_free, prior_of, store, seed, (uint64_t)(env_id0 + i), p, nz.alpha, nz.d, nz.c, noise_eps,
                     lds_gamma + wave * C, lane);
    else if (root_priors)
      for (int a = lane; a < C; a += 64) root_priors[i * C + a] = prior_of(a);
  }

  // ---- whether the ply ends: the budget is spent, or (SOLVER) the root has a proof
  // it = the iterations of this ply: the root's visits above those it was carried with (saturating)
  const uint32_t n_root = node[0].n;
  const uint32_t n0 = (uint32_t)max(carried[2 * i + 1], 1);
  bool spent = n_root != 0u && (n_root > n0 ? n_root - n0 : 0u) >= (uint32_t)(full ? I : I_fast);
  if constexpr (SOLVER) spent |= n_root != 0u && MNK_PUCT_PROOF(node[0].info) != 0u;

  uint32_t maxn = 0u, tot = 0u;
  [[maybe_unused]] int keep = 0;  // SOLVER: which of the root's children count (puct_root_keep)
  // the visits of the root's child through cell a of a row whose position is in pos: 0 on an occupied cell
  auto visits_of = [&](int a) -> uint32_t {
    if (a >= C || row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a)) return 0u;
    if constexpr (SOLVER) {
      return min(puct_kept_count(puct_root_kid(C, node, child, nodes, true, a), keep), 65535u);
    } else {
      const uint32_t ch = child[a];
      return (ch != 0u && ch != MNK_PUCT_NONE) ? min(node[min((int)ch, nodes - 1)].n, 65535u) : 0u;
    }
  };
  MnkEnv<NW> e;
  if (__builtin_amdgcn_readfirstlane((int)(live && spent))) {
    // the position before the ply: in registers, and canonical (plane 0 = the side to move) in LDS
    env_load<NW>(e, planes, meta, N, W, i);
    row_wave_sync();  // (every lane is done with the leaf's planes)
    if (lane == 0) {
      const uint32_t s = e.meta & 1u;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = s ? e.p[1][w] : e.p[0][w];
        pos[NW + w] = s ? e.p[0][w] : e.p[1][w];
      }
    }
    row_wave_sync();
    if constexpr (SOLVER) keep = puct_root_keep(C, node, child, nodes, true, lane, maxn, tot);
    maxn = 0u;
    tot = 0u;
    for (int a = lane; a < C; a += 64) {
      const uint32_t na = visits_of(a);
      maxn = max(maxn, na);
      tot += na;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
      tot += (uint32_t)__shfl_xor((int)tot, off, 64);
    }
    maxn = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxn);  // (the same in every lane: a scalar branch)
  }

  if (maxn) {
    // ---- the ply ends in this launch: ring row t = p mod T, the move, the outcome labels, the reset
    const int64_t t = (int64_t)(p % (uint64_t)T);
    const uint32_t x = mnk_rand_u32(seed, (uint64_t)(env_id0 + i), p, MNK_STREAM_SELFPLAY);
    const uint32_t side = e.meta & 1u, moves = e.meta >> 1;
    uint16_t* rv = ring_visits + (t * N + i) * C;
    for (int a = lane; a < C; a += 64) rv[a] = full ? (uint16_t)visits_of(a) : (uint16_t)0;  // a fast ply: no policy target
    if (lane == 0) {  // (the canonical planes are in LDS already)
      uint64_t* rp = ring_planes + t * 2 * W * N;
      uint32_t pl[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) pl[w] = pos[w];
      plane_store<NW>(pl, rp, N, W, i);
#pragma unroll
      for (int w = 0; w < NW; ++w) pl[w] = pos[NW + w];
      plane_store<NW>(pl, rp + (int64_t)W * N, N, W, i);
    }
    int move = 0;
    mnk_pick_by_visits(C, x, (int64_t)moves < (int64_t)temp_plies, maxn, tot, lane, visits_of, move);
    const MnkPly ply = env_play<NW, CN, CK, true>(g, e, move, false);
    if (lane == 0) ring_z[t * N + i] = ply.done ? (int8_t)(ply.win ? 1 : 0) : (int8_t)MNK_Z_UNKNOWN;
    if (ply.done) {
      // records t - d (mod T), d = 1 .. L - 1, of this game: the view of the side to move there; T >= C >= L
      const int64_t Lg = min((int64_t)moves + 1, T);
      const int8_t zw = ply.win ? 1 : 0;
      for (int64_t d = 1 + lane; d < Lg; d += 64) {
        const int64_t r = t >= d ? t - d : t + T - d;
        ring_z[r * N + i] = (d & 1) ? (int8_t)-zw : zw;
      }
      if (stats && lane == 0) {
        unsigned long long* s = stats + (size_t)(blockIdx.x % MNK_STATS_REPLICAS) * MNK_STATS_STRIDE;
        atomicAdd(&s[0], 1ull);
        atomicAdd(&s[ply.win ? 1 + side : 3], 1ull);
        atomicAdd(&s[4], (unsigned long long)moves + 1ull);
      }
      env_clear<NW>(e);
    }
    if (lane == 0) {
      env_store<NW>(e, planes, meta, N, W, i);
      row_plies[i] = p + 1ull;
      if (plies_max) atomicMax(plies_max, (unsigned long long)(p + 1ull));
      if (fresh) fresh[i] = 1;
    }
    // ---- the search of the position reached: on the subtree of the move when there is one, else a fresh tree
    // (before pos changes: the root's child through the move; a game that ended keeps nothing)
    const uint32_t mch = child[move];
    int v = 0;
    [[maybe_unused]] uint32_t vproof = 0u;
    if (!ply.done && mch != 0u && mch != MNK_PUCT_NONE) {
      v = min((int)mch, nodes - 1);
      const uint32_t vinfo = node[v].info;
      if (MNK_PUCT_TERM(vinfo)) v = 0;
      vproof = MNK_PUCT_PROOF(vinfo);
    }
    row_wave_sync();  // (every lane is done with the position before this ply)
    if (lane == 0) {
      const uint32_t ns = e.meta & 1u;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = ns ? e.p[1][w] : e.p[0][w];
        pos[NW + w] = ns ? e.p[0][w] : e.p[1][w];
      }
    }
    row_wave_sync();
    if (v > 0) {
      const int kept = puct_carry_subtree<NW, MNK_KEEP_CARRY_B>(C, NWg, row, L, pos, nodes, v, keep_nodes, i, carried, map, inv,
                                                                      lane);
      // SOLVER: the new root keeps the proof it had as a child, so that it plays in the launch that renews it -- when the
      // children that were kept still justify it (the truncation keeps the oldest nodes: the child that proved the root
      // may be gone): a root proven won for its side to move (3) needs a kept WIN child, a drawn one (2) a kept DRAW
      // child, a lost one (1) any kept child (kept > 1: node 1's parent can only be the root).  One scan of the root's
      // child row in the backup's access shape.
      if constexpr (SOLVER) {
        if (vproof && kept > 1) {
          row_wave_sync();  // (the carry's stores of the child row and the node records)
          bool win = false, draw = false;
          for (int a = lane; a < C; a += 64) {
            const uint32_t ch = child[a];
            if (ch == 0u || ch == MNK_PUCT_NONE) continue;
            const uint32_t pf = MNK_PUCT_PROOF(node[min((int)ch, kept - 1)].info);
            win |= pf == 1u;
            draw |= pf == 2u;
          }
          const bool ok = vproof == 1u || (vproof == 3u ? __ballot(win) != 0 : __ballot(draw) != 0);
          if (lane == 0 && ok) node[0].info = vproof << 12;
        }
      }
    } else {
      puct_row_fresh<NW>(row, L, pos, NWg, (int)(e.meta >> 1) < C, lane);
      if (lane == 0) {
        carried[2 * i] = 0;
        carried[2 * i + 1] = 0;
      }
    }
    row_write_view<NW, CN>(g, pos, 0, i, leaf_obs, leaf_dtype, leaf_mask, lane);
    return;
  }

  if (!live || spent) {
    // ---- a root without a legal cell (or, of a workspace that is not this position's, without a visit on a free cell):
    // reported, left alone, shown again
    if (lane == 0) {
      mnk_report(err, MNK_ERR_VISITS, i);
      if (fresh) fresh[i] = 0;
    }
    row_wave_sync();
    for (int q = lane; q < 2 * NW; q += 64) {
      const int pl = q >= NW, w = q - (pl ? NW : 0);
      pos[q] = w < NWg ? root[pl * NWg + w] : 0u;
    }
    row_wave_sync();
    row_write_view<NW, CN>(g, pos, 0, i, leaf_obs, leaf_dtype, leaf_mask, lane);
    return;
  }

  // ---- selection: k_puct_step's (SOLVER: k_puct_step_solver's at one leaf per row; the root has no proof here)
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a full tree shows its root again (it cannot happen: nodes <= keep_nodes + it)
  if (nodes <= TI) {
    puct_env_root<NW>(e, root, NWg);
    nstate = puct_walk<NW, CN, CK, false, SOLVER, false, FPU>(g, e, TI, c, node, prior, child, path, nodes, d, lane, 0, 0u,
                                                              nullptr, 0, nullptr, fpu, fpu_root);
    if (nstate == 0u) d = 0;
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = nstate ? e.p[0][w] : (w < NWg ? root[w] : 0u);
        pos[NW + w] = nstate ? e.p[1][w] : (w < NWg ? root[NWg + w] : 0u);
      }
    }
  } else if (lane == 0) {
    for (int q = 0; q < 2 * NW; ++q) {
      const int pl = q >= NW, w = q - (pl ? NW : 0);
      pos[q] = w < NWg ? root[pl * NWg + w] : 0u;
    }
  }
  if (lane == 0) {
    path[0] = 0;
    hdr[0] = (uint32_t)nodes;
    hdr[1] = (uint32_t)d;
    hdr[2] = nstate;
    if (fresh) fresh[i] = 0;
    // no leaf: nothing is pending, so n_root cannot advance and the row would show its root for ever: reported, not silent
    if (nstate == 0u) mnk_report(err, MNK_ERR_VISITS, i);
  }
  row_wave_sync();
  for (int q = lane; q < 2 * NWg; q += 64) leafp[q] = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
  row_write_view<NW, CN>(g, pos, d & 1, i, leaf_obs, leaf_dtype, leaf_mask, lane);
}

template <int NW, int CN, int CK, bool SOLVER>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_keep(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int I,
                               int I_fast, uint64_t full_threshold, const void* priors, int priors_dtype,
                               const void* values, int values_dtype, float c, int temp_plies, uint64_t seed,
                               const uint64_t* seed_dev, int64_t env_id0, unsigned long long* row_plies, int64_t T,
                               uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype,
                               uint8_t* leaf_mask, uint8_t* fresh, unsigned long long* plies_max, unsigned long long* stats,
                               int32_t* err, MnkPuctNoise nz, float noise_eps, int noise_fast, float* root_priors, int TI,
                               int keep_nodes, int32_t* carried) {
  search_selfplay_advance_keep_row<NW, CN, CK, SOLVER, false>(
      g, ws, planes, meta, N, I, I_fast, full_threshold, priors, priors_dtype, values,
      values_dtype, c, temp_plies, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits, ring_z, leaf_obs,
      leaf_dtype, leaf_mask, fresh, plies_max, stats, err, nz, noise_eps, noise_fast, root_priors, TI, keep_nodes, carried,
      0.0f, 0.0f);
}
template <int NW, int CN, int CK, bool SOLVER>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_keep_fpu(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int I,
                                   int I_fast, uint64_t full_threshold, const void* priors, int priors_dtype,
                                   const void* values, int values_dtype, float c, int temp_plies, uint64_t seed,
                                   const uint64_t* seed_dev, int64_t env_id0, unsigned long long* row_plies, int64_t T,
                                   uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype,
                                   uint8_t* leaf_mask, uint8_t* fresh, unsigned long long* plies_max, unsigned long long* stats,
                                   int32_t* err, MnkPuctNoise nz, float noise_eps, int noise_fast, float* root_priors, int TI,
                                   int keep_nodes, int32_t* carried, float fpu, float fpu_root) {
  search_selfplay_advance_keep_row<NW, CN, CK, SOLVER, true>(
      g, ws, planes, meta, N, I, I_fast, full_threshold, priors, priors_dtype, values,
      values_dtype, c, temp_plies, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits, ring_z, leaf_obs,
      leaf_dtype, leaf_mask, fresh, plies_max, stats, err, nz, noise_eps, noise_fast, root_priors, TI, keep_nodes, carried,
      fpu, fpu_root);
}

extern "C" {

int mnk_search_selfplay_advance(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies, int64_t T,
                                uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs,
                                int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh, uint64_t* plies_max, int64_t* stats,
                                int32_t* err, void* stream) {
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
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_search_selfplay_advance), grid, block, 0, (hipStream_t)stream, g,
                                     (unsigned char*)workspace, planes, meta, N, iterations, fast_iterations,
                                     full_threshold, priors, priors_dtype, values, values_dtype, c, temp_plies, seed,
                                     seed_dev, env_id0, (unsigned long long*)row_plies, T, ring_planes, ring_visits, ring_z,
                                     leaf_obs, leaf_dtype, leaf_mask, fresh, (unsigned long long*)plies_max,
                                     (unsigned long long*)stats, err));
  return mnk_launch_status("search_selfplay_advance");
}

// (what mnk_search_selfplay_advance_opts and its _fpu form share: every host check, then the launch)
static int advance_opts(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                     int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                     int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                     uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                     int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                     uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                     float noise_eps, int noise_fast, float* root_priors, bool with_fpu, float fpu,
                                     float fpu_root, void* stream) {
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
  if ((solver != 0 && solver != 1) || !(noise_alpha == 0.0f || (noise_alpha > 0.0f && noise_alpha <= 3.0e38f)) ||
      !(noise_eps >= 0.0f && noise_eps <= 1.0f) || (noise_fast != 0 && noise_fast != 1) ||
      g.C > MNK_PUCT_NOISE_CELLS_MAX)
    return MNK_EINVAL;
  if (with_fpu && (!(fpu >= 0.0f && fpu <= 3.0e38f) || !(fpu_root >= 0.0f && fpu_root <= 3.0e38f))) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  const MnkPuctNoise nz = noise_alpha > 0.0f ? mnk_puct_noise_params(noise_alpha) : MnkPuctNoise{0.0, 0.0, 0.0};
  const size_t lds = noise_alpha > 0.0f ? (size_t)MNK_PUCT_ROWS * g.C * sizeof(double) : 0;
#define MNK_ADVANCE_OPTS_FPU(SOLVER)                                                                                      \
  MNK_DISPATCH(g, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_search_selfplay_advance_opts_fpu<NW, CN, CK, SOLVER>), grid,      \
                                     block, lds, (hipStream_t)stream, g, (unsigned char*)workspace, planes, meta, N,      \
                                     iterations, fast_iterations, full_threshold, priors, priors_dtype, values,           \
                                     values_dtype, c, temp_plies, seed, seed_dev, env_id0, (unsigned long long*)row_plies, \
                                     T, ring_planes, ring_visits, ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh,         \
                                     (unsigned long long*)plies_max, (unsigned long long*)stats, err, nz, noise_eps,      \
                                     noise_fast, root_priors, fpu, fpu_root))
  if (with_fpu) {
    if (solver) MNK_ADVANCE_OPTS_FPU(true);
    else MNK_ADVANCE_OPTS_FPU(false);
    return mnk_launch_status("search_selfplay_advance_opts_fpu");
  }
#undef MNK_ADVANCE_OPTS_FPU
#define MNK_ADVANCE_OPTS(SOLVER)                                                                                          \
  MNK_DISPATCH(g, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_search_selfplay_advance_opts<NW, CN, CK, SOLVER>), grid, block,   \
                                     lds, (hipStream_t)stream, g, (unsigned char*)workspace, planes, meta, N, iterations, \
                                     fast_iterations, full_threshold, priors, priors_dtype, values, values_dtype, c,      \
                                     temp_plies, seed, seed_dev, env_id0, (unsigned long long*)row_plies, T, ring_planes, \
                                     ring_visits, ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh,                         \
                                     (unsigned long long*)plies_max, (unsigned long long*)stats, err, nz, noise_eps,      \
                                     noise_fast, root_priors))
  if (solver) MNK_ADVANCE_OPTS(true);
  else MNK_ADVANCE_OPTS(false);
#undef MNK_ADVANCE_OPTS
  return mnk_launch_status("search_selfplay_advance_opts");
}
int mnk_search_selfplay_advance_opts(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                     int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                     int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                     uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                     int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                     uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                     float noise_eps, int noise_fast, float* root_priors, void* stream) {
  return advance_opts(workspace, planes, meta, N, m, n, k, iterations, fast_iterations, full_threshold, priors, priors_dtype,
                      values, values_dtype, c, temp_plies, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits,
                      ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh, plies_max, stats, err, solver, noise_alpha, noise_eps,
                      noise_fast, root_priors, false, 0.0f, 0.0f, stream);
}
int mnk_search_selfplay_advance_opts_fpu(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                     int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                     int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                     uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                     int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                     uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                     float noise_eps, int noise_fast, float* root_priors, float fpu, float fpu_root,
                                     void* stream) {
  return advance_opts(workspace, planes, meta, N, m, n, k, iterations, fast_iterations, full_threshold, priors, priors_dtype,
                      values, values_dtype, c, temp_plies, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits,
                      ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh, plies_max, stats, err, solver, noise_alpha, noise_eps,
                      noise_fast, root_priors, true, fpu, fpu_root, stream);
}

// the LDS one workgroup of a plain launch may hold on the current device, read once (64 KiB where no device answers: the
// checks below run on a host without one)
static size_t advance_keep_lds_limit() {
  static const size_t limit = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) {
      (void)hipGetLastError();
      return (size_t)64 * 1024;
    }
    return (size_t)v;
  }();
  return limit;
}

// (what mnk_search_selfplay_advance_keep and its _fpu form share)
static int advance_keep(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                     int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                     int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                     uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                     int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                     uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                     float noise_eps, int noise_fast, float* root_priors, int tree_iterations,
                                     int keep_nodes, int32_t* carried, bool with_fpu, float fpu, float fpu_root,
                                     void* stream) {
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
  if ((solver != 0 && solver != 1) || !(noise_alpha == 0.0f || (noise_alpha > 0.0f && noise_alpha <= 3.0e38f)) ||
      !(noise_eps >= 0.0f && noise_eps <= 1.0f) || (noise_fast != 0 && noise_fast != 1) ||
      g.C > MNK_PUCT_NOISE_CELLS_MAX)
    return MNK_EINVAL;
  if (!carried || tree_iterations < iterations || tree_iterations > MNK_PUCT_ITERS_MAX || keep_nodes < 1 ||
      keep_nodes > tree_iterations + 1 - iterations)
    return MNK_EINVAL;
  // the launch's LDS: the kernel's static stage (NW = the variant's words per plane), the noise's doubles, the two maps
  const size_t map_stride = (size_t)((tree_iterations + 3) & ~1);
  const size_t lds = (noise_alpha > 0.0f ? (size_t)MNK_PUCT_ROWS * g.C * sizeof(double) : 0) +
                     (size_t)MNK_PUCT_ROWS * 2 * map_stride * sizeof(uint16_t);
  size_t lds_static = 0;
  MNK_DISPATCH(g, lds_static = sizeof(uint32_t) * MNK_PUCT_ROWS * 2 * NW);
  if (lds_static + lds > advance_keep_lds_limit()) return MNK_EINVAL;
  if (with_fpu && (!(fpu >= 0.0f && fpu <= 3.0e38f) || !(fpu_root >= 0.0f && fpu_root <= 3.0e38f))) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  const MnkPuctNoise nz = noise_alpha > 0.0f ? mnk_puct_noise_params(noise_alpha) : MnkPuctNoise{0.0, 0.0, 0.0};
#define MNK_ADVANCE_KEEP_FPU(SOLVER)                                                                                      \
  MNK_DISPATCH(g, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_search_selfplay_advance_keep_fpu<NW, CN, CK, SOLVER>), grid,      \
                                     block, lds, (hipStream_t)stream, g, (unsigned char*)workspace, planes, meta, N,      \
                                     iterations, fast_iterations, full_threshold, priors, priors_dtype, values,           \
                                     values_dtype, c, temp_plies, seed, seed_dev, env_id0, (unsigned long long*)row_plies, \
                                     T, ring_planes, ring_visits, ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh,         \
                                     (unsigned long long*)plies_max, (unsigned long long*)stats, err, nz, noise_eps,      \
                                     noise_fast, root_priors, tree_iterations, keep_nodes, carried, fpu, fpu_root))
  if (with_fpu) {
    if (solver) MNK_ADVANCE_KEEP_FPU(true);
    else MNK_ADVANCE_KEEP_FPU(false);
    return mnk_launch_status("search_selfplay_advance_keep_fpu");
  }
#undef MNK_ADVANCE_KEEP_FPU
#define MNK_ADVANCE_KEEP(SOLVER)                                                                                          \
  MNK_DISPATCH(g, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_search_selfplay_advance_keep<NW, CN, CK, SOLVER>), grid, block,   \
                                     lds, (hipStream_t)stream, g, (unsigned char*)workspace, planes, meta, N, iterations, \
                                     fast_iterations, full_threshold, priors, priors_dtype, values, values_dtype, c,      \
                                     temp_plies, seed, seed_dev, env_id0, (unsigned long long*)row_plies, T, ring_planes, \
                                     ring_visits, ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh,                         \
                                     (unsigned long long*)plies_max, (unsigned long long*)stats, err, nz, noise_eps,      \
                                     noise_fast, root_priors, tree_iterations, keep_nodes, carried))
  if (solver) MNK_ADVANCE_KEEP(true);
  else MNK_ADVANCE_KEEP(false);
#undef MNK_ADVANCE_KEEP
  return mnk_launch_status("search_selfplay_advance_keep");
}
int mnk_search_selfplay_advance_keep(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                     int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                     int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                     uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                     int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                     uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                     float noise_eps, int noise_fast, float* root_priors, int tree_iterations,
                                     int keep_nodes, int32_t* carried, void* stream) {
  return advance_keep(workspace, planes, meta, N, m, n, k, iterations, fast_iterations, full_threshold, priors, priors_dtype,
                      values, values_dtype, c, temp_plies, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits,
                      ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh, plies_max, stats, err, solver, noise_alpha, noise_eps,
                      noise_fast, root_priors, tree_iterations, keep_nodes, carried, false, 0.0f, 0.0f, stream);
}
int mnk_search_selfplay_advance_keep_fpu(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                     int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                     int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                     uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                     int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                     uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                     float noise_eps, int noise_fast, float* root_priors, int tree_iterations,
                                     int keep_nodes, int32_t* carried, float fpu, float fpu_root, void* stream) {
  return advance_keep(workspace, planes, meta, N, m, n, k, iterations, fast_iterations, full_threshold, priors, priors_dtype,
                      values, values_dtype, c, temp_plies, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits,
                      ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh, plies_max, stats, err, solver, noise_alpha, noise_eps,
                      noise_fast, root_priors, tree_iterations, keep_nodes, carried, true, fpu, fpu_root, stream);
}

}  // extern "C"
