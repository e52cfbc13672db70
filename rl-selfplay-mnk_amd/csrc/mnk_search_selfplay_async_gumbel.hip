// mnk_search_selfplay_async_gumbel.hip -- search self-play with per-row search budgets and a Gumbel root (gfx950 / MI355X
// only): mnk_search_selfplay_advance (mnk_search_selfplay_async.hip) for rows whose root is the lockstep player's Gumbel
// root -- mnk_puct_gumbel_root's draw at the backup of a fresh tree's root, mnk_puct_step_gumbel's selection with the
// schedule table of the ply's budget, its move and its improved policy at the end of the ply -- all inside the one launch.
// The rule: include/mnk_hip.h, mnk_search_selfplay_advance_gumbel.
//
// A translation unit of its own: compiled beside its siblings a kernel changes the code the compiler makes of them
// (profiles/exp_search_selfplay_async_leaves_kernels.md), and those keep their code objects.
//
// Floating point: the draw and the policy are f64 with the full-precision log and exp of the device library; the
// roundings to f32 are the ones the rule names.  The library is built with -ffp-contract=off and without any fast-math
// option, and nothing here may change that for this file.  There is no f32 transcendental in this translation unit.
#include "mnk_host.h"
#include "mnk_puct_tree.h"

#define MNK_ADVANCE_GUMBEL_CELLS_MAX 1024  // 64 * MNK_MAX_W: no supported board has more cells than a plane has bits
static_assert(MNK_ADVANCE_GUMBEL_CELLS_MAX == 64 * MNK_MAX_W, "the cell range follows the packed planes");

// a sum over the wave, the same value in every lane
__device__ __forceinline__ double advance_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// The improved policy of a Gumbel root after its last backup: the policy part of puct_move_gumbel (mnk_puct.hip; the
// rule: include/mnk_hip.h, mnk_puct_step_gumbel), operation for operation, without that function's `actions` / `visits`
// outputs.  This unit's own copy: moving the function into mnk_puct_tree.h, called from both, changed the code objects of
// k_puct_step_gumbel (profiles/exp_search_selfplay_async_gumbel_kernels.md), so the original stays where it is and any
// change to the rule is made in both.  The move is puct_gumbel_pick<true> (mnk_puct_tree.h), which also gives maxn.
// f64: five passes over the root's cells (the sum of the clamped priors; the visited cells' sums for v_mix; the maximum
// of y; the sum of exp(y - max); the store), every pass recomputing a cell's terms from the tree -- the same operations on
// the same inputs give the same y each time -- and reduced over the wave.  pr = the root's stored priors (node 0's row),
// cl its child row.  store(a, policy_a) is called once for every cell a < C by the lane that owns it (a = lane,
// lane + 64, ...), with 0 for an occupied cell.
template <class Store>
__device__ __forceinline__ void advance_gumbel_policy(int C, const MnkPuctNode* node, const float* pr, const uint16_t* cl,
                                                      int nodes, const MnkPuctGumbel& gm, float vroot, uint32_t maxn,
                                                      int lane, Store store) {
  // a free cell's clamped prior, visit count and q (0 where it has no visit)
  auto cell = [&](int a, double& p, uint32_t& na, double& q) {
    const uint32_t ch = cl[a];
    if (ch == MNK_PUCT_NONE) return false;
    const float pa = pr[a];
    p = (double)(pa > 0x1p-126f ? pa : 0x1p-126f);
    na = 0u;
    q = 0.0;
    if (ch) {
      const MnkPuctNode k = node[min((int)ch, nodes - 1)];
      na = k.n;
      if (na) q = (double)__fdiv_rn(k.w, (float)na);
    }
    return true;
  };
  double p, q, sp = 0.0;
  uint32_t na, ns = 0u;
  for (int a = lane; a < C; a += 64)
    if (cell(a, p, na, q)) {
      sp += p;
      ns += na;
    }
  sp = advance_wave_sum(sp);
#pragma unroll
  for (int off = 32; off; off >>= 1) ns += (uint32_t)__shfl_xor((int)ns, off, 64);
  double sv = 0.0, sq = 0.0;
  for (int a = lane; a < C; a += 64)
    if (cell(a, p, na, q) && na) {
      sv += p / sp;
      sq += p / sp * q;
    }
  sv = advance_wave_sum(sv);
  sq = advance_wave_sum(sq);
  const double vmix = sv > 0.0 ? ((double)vroot + (double)ns * sq / sv) / (1.0 + (double)ns) : (double)vroot;
  const double K = ((double)gm.c_visit + (double)maxn) * (double)gm.c_scale;
  auto y_of = [&](int a, double& y) {
    if (!cell(a, p, na, q)) return false;
    y = log(p) + K * (na ? q : vmix);
    return true;
  };
  double y, my = -INFINITY;
  for (int a = lane; a < C; a += 64)
    if (y_of(a, y)) my = fmax(my, y);
#pragma unroll
  for (int off = 32; off; off >>= 1) my = fmax(my, __shfl_xor(my, off, 64));
  double se = 0.0;
  for (int a = lane; a < C; a += 64)
    if (y_of(a, y)) se += exp(y - my);
  se = advance_wave_sum(se);
  for (int a = lane; a < C; a += 64) store(a, y_of(a, y) ? (float)(exp(y - my) / se) : 0.0f);
}

// k_search_selfplay_advance with the Gumbel root.  The same shape: one wave per row, MNK_PUCT_ROWS rows per workgroup, no
// workgroup barrier (which branch a row takes is wave-uniform; the rows of a workgroup diverge), every id read from the
// workspace clamped to the row.  B, the budget of the row's ply, is also the row stride of the ply's schedule table, so it
// is what the walk and the root's pick are given as their iteration count: the pick's read stays inside the table of B
// columns, and the walk's depth guard (d >= B) is as unreachable as it is with I -- an existing node lies at depth <= it < B.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_gumbel(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int I,
                                 int I_fast, uint64_t full_threshold, const void* priors, int priors_dtype,
                                 const void* values, int values_dtype, float c, uint64_t seed, const uint64_t* seed_dev,
                                 int64_t env_id0, unsigned long long* row_plies, int64_t T, uint64_t* ring_planes,
                                 uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask,
                                 uint8_t* fresh, unsigned long long* plies_max, unsigned long long* stats, int32_t* err,
                                 int considered, float c_visit, float c_scale, double gscale, const uint16_t* table_full,
                                 const uint16_t* table_fast, float* gscore, float* vroot) {
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

  // ---- the budget of the row's ply: B, and the schedule table that goes with it
  if (seed_dev) seed = *seed_dev;
  const uint64_t p = row_plies[i];
  const uint32_t u = mnk_rand_u32(seed, (uint64_t)(env_id0 + i), p, MNK_STREAM_BUDGET);
  const bool full = (uint64_t)u < full_threshold;
  const int B = full ? I : I_fast;
  MnkPuctGumbel gm;
  gm.gs = gscore + i * C;
  gm.table = full ? table_full : table_fast;
  gm.considered = considered;
  gm.c_visit = c_visit;
  gm.c_scale = c_scale;

  // ---- backup of the pending evaluation
  if (live && (state & 1u))
    puct_backup<NW, CN>(g, pos, path, node, prior, child, nodes, depth, state, priors, priors_dtype, values, values_dtype,
                        i, lane);
  // evaluation 0 (what puct_row_fresh and mnk_puct_begin leave pending): the root's Gumbel scores and its value, by
  // k_puct_gumbel_root's text with step = the row's ply and the free cells those of the root's planes (pos: at depth 0 the
  // leaf is the root).  A cell's gscore is written here and read, in the selections and at the end of the ply, by the same
  // lane -- cells are strided over the lanes the same way in every loop -- so no synchronisation is needed, as with the
  // noised priors of k_search_selfplay_advance_opts.  vroot[i] is lane 0's store; it is read when the ply ends, which is
  // never this launch (n_root = 1 here and B >= 1).
  if (live && state == 1u && depth == 0) {
    const int64_t base = i * C;
    const uint64_t env = (uint64_t)(env_id0 + i);
    const uint64_t s_row = p * (uint64_t)((C + 3) & ~3);  // word a of the row: block s_row / 4 + (a >> 2), word a & 3
    for (int a = lane; a < C; a += 64) {
      float gs = -INFINITY;
      if (!(row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a))) {
        const float pa = puct_read(priors, priors_dtype, base + a);
        const double l = log((double)(pa > 0x1p-126f ? pa : 0x1p-126f));
        const double uu = ((double)mnk_rand_u32(seed, env, s_row + (uint64_t)a, MNK_STREAM_GUMBEL) + 0.5) * 0x1p-32;
        const double gv = -log(-log(uu));  // (uu is never 0 or 1: gv is finite)
        gs = (float)(gscale * gv + l);
      }
      gscore[base + a] = gs;
    }
    if (lane == 0) vroot[i] = puct_read(values, values_dtype, i);
  }

  // ---- whether the ply ends, and then its move: mnk_puct_step_gumbel's, which must be a free cell of the env's position
  const uint32_t n_root = node[0].n;
  const bool spent = n_root != 0u && n_root - 1u >= (uint32_t)B;
  MnkEnv<NW> e;
  int move = 0x7fffffff;
  uint32_t maxn = 0u;
  bool playable = false;
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
    move = puct_gumbel_pick<true>(C, B, node, child, nodes, gm, lane, &maxn);  // (wave-uniform; 0x7fffffff: no free cell)
    playable = move >= 0 && move < C && !(row_stone<CN>(g, pos, move) || row_stone<CN>(g, pos + NW, move));
  }

  if (playable) {
    // ---- the ply ends in this launch: ring row t = p mod T, the improved policy, the outcome labels, the reset
    const int64_t t = (int64_t)(p % (uint64_t)T);
    const uint32_t side = e.meta & 1u, moves = e.meta >> 1;
    uint16_t* rv = ring_visits + (t * N + i) * C;
    if (full) {
      // k_search_selfplay_step_moves's quantisation of puct_move_gumbel's policy, a cell at a time
      advance_gumbel_policy(C, node, prior, child, nodes, gm, vroot[i], maxn, lane, [&](int a, float pa) {
        const bool occ = row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a);
        const float v = rintf(__fmul_rn(pa, 65535.0f));
        rv[a] = (occ || !(v > 0.0f)) ? (uint16_t)0 : (uint16_t)fminf(v, 65535.0f);
      });
    } else {
      for (int a = lane; a < C; a += 64) rv[a] = (uint16_t)0;  // a fast ply: no policy target
    }
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
    // ---- a root without a legal cell (or, of a workspace that is not this position's, a move that is no free cell):
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

  // ---- selection: k_puct_step_gumbel's (the root's cell by puct_gumbel_pick with the table of B columns)
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a full tree shows its root again (it cannot happen: nodes <= n_root <= B)
  if (nodes <= I) {
    puct_env_root<NW>(e, root, NWg);
    nstate = puct_walk<NW, CN, CK, false, false, true>(g, e, B, c, node, prior, child, path, nodes, d, lane, 0, 0u, nullptr,
                                                       0, &gm);
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
    // in a workspace that mnk_puct_begin set up (nodes <= n_root <= B while the budget is unspent): reported, not silent
    if (nstate == 0u) mnk_report(err, MNK_ERR_VISITS, i);
  }
  row_wave_sync();
  for (int q = lane; q < 2 * NWg; q += 64) leafp[q] = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
  row_write_view<NW, CN>(g, pos, d & 1, i, leaf_obs, leaf_dtype, leaf_mask, lane);
}

extern "C" {

int mnk_search_selfplay_advance_gumbel(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                       int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                       int priors_dtype, const void* values, int values_dtype, float c, uint64_t seed,
                                       const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies, int64_t T,
                                       uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs,
                                       int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh, uint64_t* plies_max,
                                       int64_t* stats, int32_t* err, int considered, float c_visit, float c_scale,
                                       float gumbel_scale, const uint16_t* table_full, const uint16_t* table_fast,
                                       float* gscore, float* vroot, void* stream) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  const bool dt_ok = (priors_dtype == MNK_LOGITS_F32 || priors_dtype == MNK_LOGITS_BF16) &&
                     (values_dtype == MNK_LOGITS_F32 || values_dtype == MNK_LOGITS_BF16);
  if (!workspace || !planes || !meta || !priors || !values || !row_plies || !ring_planes || !ring_visits || !ring_z ||
      !leaf_obs || !leaf_mask || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_ROWS || !dt_ok ||
      !mnk_obs_dtype_ok(leaf_dtype) || fast_iterations < 1 || fast_iterations > iterations ||
      iterations > MNK_PUCT_ITERS_MAX || full_threshold > (1ull << 32) || !(c >= 0.0f && c <= 3.0e38f) || T < g.C)
    return MNK_EINVAL;
  if (considered < 1 || considered > MNK_PUCT_CONSIDERED_MAX || !(c_visit >= 0.0f && c_visit <= 3.0e38f) ||
      !(c_scale >= 0.0f && c_scale <= 3.0e38f) || !(gumbel_scale >= 0.0f && gumbel_scale <= 3.0e38f) || !table_full ||
      !table_fast || !gscore || !vroot || g.C > MNK_ADVANCE_GUMBEL_CELLS_MAX)
    return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_search_selfplay_advance_gumbel), grid, block, 0, (hipStream_t)stream, g,
                                     (unsigned char*)workspace, planes, meta, N, iterations, fast_iterations,
                                     full_threshold, priors, priors_dtype, values, values_dtype, c, seed, seed_dev, env_id0,
                                     (unsigned long long*)row_plies, T, ring_planes, ring_visits, ring_z, leaf_obs,
                                     leaf_dtype, leaf_mask, fresh, (unsigned long long*)plies_max,
                                     (unsigned long long*)stats, err, considered, c_visit, c_scale, (double)gumbel_scale,
                                     table_full, table_fast, gscore, vroot));
  return mnk_launch_status("search_selfplay_advance_gumbel");
}

}  // extern "C"
