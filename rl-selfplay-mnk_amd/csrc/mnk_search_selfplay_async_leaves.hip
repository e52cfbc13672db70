// mnk_search_selfplay_async_leaves.hip -- search self-play with per-row search budgets and several leaves per evaluator
// call (gfx950 / MI355X only): mnk_search_selfplay_advance_opts (mnk_search_selfplay_async.hip) for rows that search with
// L slots per row and call -- the lockstep player's mnk_puct_step_leaves / mnk_puct_step_solver: L backups, then up to L
// selections under virtual visits -- with a ply's budget counted in the simulations it has been offered.  The rule:
// include/mnk_hip.h, mnk_search_selfplay_advance_leaves.
//
// A translation unit of its own: compiled beside its three siblings the kernel changes the code the compiler makes of
// them (every function here is inlined, but the module's passes see other call sites), and those keep their code objects.
#include "mnk_host.h"
#include "mnk_puct_noise.h"
#include "mnk_puct_tree.h"

// The backup loop and the selection loop of k_puct_step_leaves / k_puct_step_solver (mnk_puct.hip) around the end-of-ply
// block of k_search_selfplay_advance_opts.  The siblings' shape: one wave per row, MNK_PUCT_ROWS rows per workgroup, no
// workgroup barrier, every id read from the workspace clamped to the row.  Slot j of row i is batch row i * leaves + j; the
// slots' paths stay in the workspace.  Whether the ply ends is decided by row_sims, the simulations the ply has been
// offered, not by the root's visits: a slot that the walk makes void is a simulation spent.  The three branches after the
// backups -- the ply ends, an error row, the selections -- are disjoint and wave-uniform, so the one MnkEnv serves the ply
// and the walks.  nz.alpha = 0: no noise, and then the launch has no dynamic LDS.
template <int NW, int CN, int CK, bool SOLVER>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_leaves(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int I,
                                 int I_fast, int leaves, uint64_t full_threshold, const void* priors, int priors_dtype,
                                 const void* values, int values_dtype, float c, int temp_plies, uint64_t seed,
                                 const uint64_t* seed_dev, int64_t env_id0, unsigned long long* row_plies, int64_t T,
                                 uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs,
                                 int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh, unsigned long long* plies_max,
                                 unsigned long long* stats, int32_t* err, MnkPuctNoise nz, float noise_eps, int noise_fast,
                                 float* root_priors, uint32_t* row_sims) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  extern __shared__ double lds_gamma[];  // with noise: [MNK_PUCT_ROWS][C], a root's log-gammas between the two passes
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW, W = g.W;
  const MnkPuctLayout L = mnk_puct_layout(NWg, C, I, leaves);
  unsigned char* row = ws + i * L.row;
  uint32_t* hdr = (uint32_t*)row;
  const uint32_t* root = (const uint32_t*)(row + L.root);
  MnkPuctNode* node = (MnkPuctNode*)(row + L.node);
  float* prior = (float*)(row + L.prior);
  uint16_t* child = (uint16_t*)(row + L.child);
  uint32_t* pos = lds_pos[wave];
  // slot j's {depth, state}, leaf planes and path (slot 0: the header's, `leaf`, `path`)
  auto slot_ds = [&](int j) { return j ? (uint32_t*)(row + L.xhdr) + 2 * (j - 1) : hdr + 1; };
  auto slot_leaf = [&](int j) { return (uint32_t*)(row + (j ? L.xleaf + 8 * (int64_t)NWg * (j - 1) : L.leaf)); };
  auto slot_path = [&](int j) { return (uint16_t*)(row + (j ? L.xpath + L.pstride * (j - 1) : L.path)); };
  // the root's planes into the wave's stage
  auto stage_root = [&]() {
    for (int q = lane; q < 2 * NW; q += 64) {
      const int pl = q >= NW, w = q - (pl ? NW : 0);
      pos[q] = w < NWg ? root[pl * NWg + w] : 0u;
    }
  };
  // (clamped, as in k_puct_step_leaves: whatever the workspace holds, no id leaves the row)
  int nodes = (int)min(max(hdr[0], 1u), (uint32_t)(I + 1));
  const bool live = hdr[3] != 0u;

  // ---- the budget of the row's ply (before the backups: whether a root is noised depends on it)
  if (seed_dev) seed = *seed_dev;
  const uint64_t p = row_plies[i];
  const uint32_t u = mnk_rand_u32(seed, (uint64_t)(env_id0 + i), p, MNK_STREAM_BUDGET);
  const bool full = (uint64_t)u < full_threshold;
  const uint32_t sims = row_sims[i];
  const uint32_t budget = (uint32_t)(full ? I : I_fast);

  // ---- the backups of the pending evaluations, in slot order
  for (int j = 0; j < leaves && live; ++j) {
    const uint32_t* ds = slot_ds(j);
    const int depth = (int)min(ds[0], (uint32_t)I);
    const uint32_t state = ds[1];
    if (!(state & 1u)) continue;
    const uint32_t* leafp = slot_leaf(j);
    for (int q = lane; q < 2 * NW; q += 64) {
      const int pl = q >= NW, w = q - (pl ? NW : 0);
      pos[q] = w < NWg ? leafp[pl * NWg + w] : 0u;
    }
    row_wave_sync();
    puct_backup<NW, CN, SOLVER>(g, pos, slot_path(j), node, prior, child, nodes, depth, state, priors, priors_dtype, values,
                                values_dtype, i * leaves + j, lane);
    // evaluation 0 (what puct_row_fresh and mnk_puct_begin_leaves leave pending in slot 0): the root's prior row -- node
    // 0's -- takes the noised priors on its free cells, and root_priors what the root then holds.  A lane rewrites the
    // cells it wrote in the backup; the sync is for the stage, which the next slot's planes overwrite.
    if (j == 0 && state == 1u && depth == 0 && (nz.alpha > 0.0 || root_priors)) {
      const int64_t b = i * leaves;
      auto is_free = [&](int a) { return !(row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a)); };
      auto prior_of = [&](int a) { return puct_read(priors, priors_dtype, b * C + a); };
      auto store = [&](int a, float pa) {
        if (is_free(a)) prior[a] = pa;
        if (root_priors) root_priors[i * C + a] = pa;
      };
      if (nz.alpha > 0.0 && (full || noise_fast))
        puct_noise_row(C, is_free, prior_of, store, seed, (uint64_t)(env_id0 + i), p, nz.alpha, nz.d, nz.c, noise_eps,
                       lds_gamma + wave * C, lane);
      else if (root_priors)
        for (int a = lane; a < C; a += 64) root_priors[i * C + a] = prior_of(a);
      row_wave_sync();
    }
  }

  // ---- whether the ply ends: it has been offered its budget, or (SOLVER) the root has a proof
  bool spent = sims >= budget;
  if constexpr (SOLVER) spent |= node[0].n != 0u && MNK_PUCT_PROOF(node[0].info) != 0u;

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
    row_wave_sync();  // (every lane is done with the last leaf's planes)
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
      row_sims[i] = 0u;
    }
    // ---- the search of the position reached: a fresh tree (no proof) as mnk_puct_begin_leaves leaves it -- slot 0 the
    // root, pending; the other slots void, showing it
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
    row_write_view<NW, CN>(g, pos, 0, i * leaves, leaf_obs, leaf_dtype, leaf_mask, lane);
    puct_row_void_slots<NW, CN>(g, row, L, pos, i, leaves, leaf_obs, leaf_dtype, leaf_mask, lane);
    return;
  }

  if (!live || spent) {
    // ---- a root without a legal cell (or, of a workspace that is not this position's, without a visit on a free cell):
    // reported, left alone -- row_sims too --, the root shown in all of the row's batch rows
    if (lane == 0) {
      mnk_report(err, MNK_ERR_VISITS, i);
      if (fresh) fresh[i] = 0;
    }
    row_wave_sync();
    stage_root();
    row_wave_sync();
    for (int j = 0; j < leaves; ++j) row_write_view<NW, CN>(g, pos, 0, i * leaves + j, leaf_obs, leaf_dtype, leaf_mask, lane);
    return;
  }

  // ---- the selections: k_puct_step_leaves's (SOLVER: k_puct_step_solver's; the root has no proof here), slots 0 .. s - 1;
  // the slots from s on are void, so that the ply is offered its budget exactly
  const int s = (int)min((uint32_t)leaves, budget - sims);
  const int nodes0 = nodes;
  const uint16_t* epath = slot_path(min(lane, leaves - 1));  // lane l < leaves: slot l's path
  int edepth = 0;                                            // and, once it has selected, its leaf's depth
  uint32_t active = 0u;                                      // the slots of this round that have a leaf
  bool open = true;                                          // no slot was void yet
  for (int j = 0; j < leaves; ++j) {
    int d = 0;
    uint32_t nstate = 0u;
    uint16_t* path = slot_path(j);
    if (open && j < s && nodes <= I) {
      puct_env_root<NW>(e, root, NWg);
      nstate = puct_walk<NW, CN, CK, true, SOLVER>(g, e, I, c, node, prior, child, path, nodes, d, lane, nodes0, active,
                                                   epath, edepth);
    }
    if (nstate) {
      active |= 1u << j;
      if (lane == j) edepth = d;
    } else {
      d = 0;
      open = false;
    }
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pos[w] = nstate ? e.p[0][w] : (w < NWg ? root[w] : 0u);
        pos[NW + w] = nstate ? e.p[1][w] : (w < NWg ? root[NWg + w] : 0u);
      }
      path[0] = 0;
      uint32_t* ds = slot_ds(j);
      ds[0] = (uint32_t)d;
      ds[1] = nstate;
    }
    row_wave_sync();
    uint32_t* leafp = slot_leaf(j);
    for (int q = lane; q < 2 * NWg; q += 64) leafp[q] = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
    row_write_view<NW, CN>(g, pos, d & 1, i * leaves + j, leaf_obs, leaf_dtype, leaf_mask, lane);
    row_wave_sync();  // (the next slot's walk reads this one's node, child entry and path; its write-out reuses pos)
  }
  if (lane == 0) {
    hdr[0] = (uint32_t)nodes;
    if (fresh) fresh[i] = 0;
    // no leaf at all: nothing is pending, so the row would show its root for ever (a full tree: it cannot happen in a
    // workspace that mnk_puct_begin_leaves set up): reported, not silent, and the counter stays
    if (active == 0u) mnk_report(err, MNK_ERR_VISITS, i);
    else row_sims[i] = sims + (uint32_t)s;
  }
}

extern "C" {

int mnk_search_selfplay_advance_leaves(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                       int iterations, int fast_iterations, int leaves, uint64_t full_threshold,
                                       const void* priors, int priors_dtype, const void* values, int values_dtype, float c,
                                       int temp_plies, uint64_t seed, const uint64_t* seed_dev, int64_t env_id0,
                                       uint64_t* row_plies, int64_t T, uint64_t* ring_planes, uint16_t* ring_visits,
                                       int8_t* ring_z, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                       uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                       float noise_eps, int noise_fast, float* root_priors, uint32_t* row_sims,
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
  // (the workspace's condition: mnk_puct_begin_leaves takes no other pair)
  if (leaves < 1 || leaves > MNK_PUCT_LEAVES_MAX || iterations % leaves != 0 || !row_sims) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  const MnkPuctNoise nz = noise_alpha > 0.0f ? mnk_puct_noise_params(noise_alpha) : MnkPuctNoise{0.0, 0.0, 0.0};
  const size_t lds = noise_alpha > 0.0f ? (size_t)MNK_PUCT_ROWS * g.C * sizeof(double) : 0;
#define MNK_ADVANCE_LEAVES(SOLVER)                                                                                         \
  MNK_DISPATCH(g, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_search_selfplay_advance_leaves<NW, CN, CK, SOLVER>), grid, block,  \
                                     lds, (hipStream_t)stream, g, (unsigned char*)workspace, planes, meta, N, iterations, \
                                     fast_iterations, leaves, full_threshold, priors, priors_dtype, values, values_dtype, \
                                     c, temp_plies, seed, seed_dev, env_id0, (unsigned long long*)row_plies, T,           \
                                     ring_planes, ring_visits, ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh,            \
                                     (unsigned long long*)plies_max, (unsigned long long*)stats, err, nz, noise_eps,      \
                                     noise_fast, root_priors, row_sims))
  if (solver) MNK_ADVANCE_LEAVES(true);
  else MNK_ADVANCE_LEAVES(false);
#undef MNK_ADVANCE_LEAVES
  return mnk_launch_status("search_selfplay_advance_leaves");
}

}  // extern "C"
