// mnk_puct.hip -- the PUCT search player (gfx950 / MI355X only): AlphaZero-style search guided by a caller's evaluator
// (normally a policy/value network), batched over rows.  The tree lives in a device workspace between launches; each
// launch backs up the previous evaluation and selects the next leaf (mnk_puct_step), so an act() is mnk_puct_begin,
// I + 1 evaluator calls and I + 1 steps with no host synchronisation.  mnk_puct_rebase in the place of mnk_puct_begin
// carries the subtree of the position that was reached into the next search.  The *_leaves entry points run the same
// search with L leaves per row and evaluation (a round = L backups, then L selections under virtual visits), so the
// evaluator sees I / L + 1 batches of N * L rows.  mnk_puct_step_solver is mnk_puct_step_leaves with exact proofs of wins,
// draws and losses in the backup (a 2-bit proof per node, propagated up the leaf's path).  The rule: include/mnk_hip.h.
#include "mnk_host.h"
#include "mnk_wave_rows.h"
#include "mnk_puct_tree.h"

// ------------------------------------------------------------------ evaluation 0: the roots
// row i of obs into guard-column bit planes in LDS (pos[2 * NW], the wave's own); returns its stone count
template <int NW, int CN>
__device__ __forceinline__ int puct_row_planes(const MnkGeom& g, const void* obs, int obs_dtype, int64_t i, uint32_t* pos,
                                               int lane) {
  const int C = g.C;
  for (int q = lane; q < 2 * NW; q += 64) pos[q] = 0u;
  row_wave_sync();
  const size_t eb = (size_t)mnk_obs_bytes(obs_dtype);
  const unsigned char* src = (const unsigned char*)obs + (size_t)i * 2 * C * eb;
  for (int q = lane; q < 2 * C; q += 64) {
    uint32_t v;
    if (obs_dtype == MNK_OBS_F32) v = ((const uint32_t*)src)[q] << 1;  // (+0.0 and -0.0 are empty)
    else if (obs_dtype == MNK_OBS_BF16) v = (uint32_t)((const uint16_t*)src)[q] << 17;
    else v = src[q];
    if (v) {
      const int pl = q >= C;
      const uint32_t bit = mnk_cell_bit<CN>(g, (uint32_t)(q - (pl ? C : 0)));
      atomicOr(&pos[pl * NW + (bit >> 5)], 1u << (bit & 31u));
    }
  }
  row_wave_sync();
  int stones = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) stones += __popc(pos[w] | pos[NW + w]);
  return stones;
}

// One wave per row: the row into bit planes (LDS, pos), the root node, the roots as the first leaves (slot 0 of `leaves`).
template <int NW, int CN>
__device__ __forceinline__ void puct_begin_row(const MnkGeom& g, const void* obs, int obs_dtype, int64_t i, int I, int leaves,
                                               unsigned char* ws, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask,
                                               uint32_t* pos, int lane) {
  const int C = g.C, NWg = g.NW;
  const int stones = puct_row_planes<NW, CN>(g, obs, obs_dtype, i, pos, lane);
  const MnkPuctLayout L = mnk_puct_layout(NWg, C, I, leaves);
  puct_row_fresh<NW>(ws + i * L.row, L, pos, NWg, stones < C, lane);
  row_write_view<NW, CN>(g, pos, 0, i * leaves, leaf_obs, leaf_dtype, leaf_mask, lane);
  puct_row_void_slots<NW, CN>(g, ws + i * L.row, L, pos, i, leaves, leaf_obs, leaf_dtype, leaf_mask, lane);
}

template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_begin(MnkGeom g, const void* obs, int obs_dtype, int64_t N, int I, unsigned char* ws, void* leaf_obs,
             int leaf_dtype, uint8_t* leaf_mask) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  puct_begin_row<NW, CN>(g, obs, obs_dtype, i, I, 1, ws, leaf_obs, leaf_dtype, leaf_mask, lds_pos[wave], lane);
}

template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_begin_leaves(MnkGeom g, const void* obs, int obs_dtype, int64_t N, int I, int leaves, unsigned char* ws,
                    void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  puct_begin_row<NW, CN>(g, obs, obs_dtype, i, I, leaves, ws, leaf_obs, leaf_dtype, leaf_mask, lds_pos[wave], lane);
}

// ------------------------------------------------------------------ evaluation 0 of a search that keeps its tree
// One wave per row.  The row is matched against the stored root (the rule: include/mnk_hip.h, mnk_puct_rebase); a row
// that continues it keeps the subtree of the node it reached, compacted in place to ids 0 .. kept - 1 in creation order
// (puct_carry_subtree, mnk_puct_tree.h: the marking and the compaction, eight nodes of the prior and child rows in flight).
template <int NW, int CN>
__device__ __forceinline__ void puct_rebase_row(const MnkGeom& g, const void* obs, int obs_dtype, int64_t i, int I, int keep,
                                                int leaves, unsigned char* ws, void* leaf_obs, int leaf_dtype,
                                                uint8_t* leaf_mask, int32_t* carried, uint32_t* pos, uint32_t* ext,
                                                uint16_t* map, uint16_t* inv, int lane) {
  const int C = g.C, NWg = g.NW;
  const int stones = puct_row_planes<NW, CN>(g, obs, obs_dtype, i, pos, lane);
  const MnkPuctLayout L = mnk_puct_layout(NWg, C, I, leaves);
  unsigned char* row = ws + i * L.row;
  uint32_t* hdr = (uint32_t*)row;
  const uint32_t* root = (const uint32_t*)(row + L.root);
  MnkPuctNode* node = (MnkPuctNode*)(row + L.node);
  uint16_t* child = (uint16_t*)(row + L.child);
  // (clamped, as in k_puct_step: whatever the workspace holds, no id leaves the row)
  const int nodes = (int)min(hdr[0], (uint32_t)(I + 1));
  const bool live = hdr[3] != 0u;

  // ---- the match (wave-uniform): same[x][y] = the row's plane x is the stored plane y; more[x][y] = it is that plane and
  // one cell more
  bool same00 = true, same11 = true, same01 = true, sup00 = true, sup11 = true, sup10 = true;
  int n00 = 0, n11 = 0, n10 = 0;
  for (int w = 0; w < NWg; ++w) {
    const uint32_t r0 = root[w], r1 = root[NWg + w], o0 = pos[w], o1 = pos[NW + w];
    same00 &= o0 == r0;
    same11 &= o1 == r1;
    same01 &= o0 == r1;
    sup00 &= (r0 & ~o0) == 0u;
    sup11 &= (r1 & ~o1) == 0u;
    sup10 &= (r0 & ~o1) == 0u;
    n00 += __popc(o0 & ~r0);
    n11 += __popc(o1 & ~r1);
    n10 += __popc(o1 & ~r0);
  }
  int plies = -1;  // the length of the path from the stored root, -1: the row does not continue it
  if (nodes >= 1 && live) {
    if (same00 && same11) plies = 0;
    else if (same01 && sup10 && n10 == 1) plies = 1;
    else if (sup00 && n00 == 1 && sup11 && n11 == 1) plies = 2;
  }
  if (plies > 0) {  // the new stones as planes: [0] the first ply's, [1] the second's
    for (int q = lane; q < NWg; q += 64) {
      const uint32_t r0 = root[q], r1 = root[NWg + q], o0 = pos[q], o1 = pos[NW + q];
      ext[q] = plies == 1 ? (o1 & ~r0) : (o0 & ~r0);
      ext[NW + q] = plies == 1 ? 0u : (o1 & ~r1);
    }
    row_wave_sync();
  }
  int v = 0;  // the node the path ends in
  for (int s = 0; s < plies; ++s) {
    int a = -1;
    for (int a0 = 0; a0 < C && a < 0; a0 += 64) {
      const uint64_t hit = __ballot(a0 + lane < C && row_stone<CN>(g, ext + s * NW, a0 + lane));
      if (hit) a = a0 + (int)__ffsll((unsigned long long)hit) - 1;
    }
    const uint32_t ch = a >= 0 ? child[(int64_t)v * C + a] : 0u;
    if (ch == 0u || ch == MNK_PUCT_NONE) {
      plies = -1;
      break;
    }
    v = min((int)ch, nodes - 1);
    if (MNK_PUCT_TERM(node[v].info)) {
      plies = -1;
      break;
    }
  }

  if (plies < 0) {  // exactly what k_puct_begin writes
    puct_row_fresh<NW>(row, L, pos, NWg, stones < C, lane);
    if (carried && lane == 0) {
      carried[2 * i] = 0;
      carried[2 * i + 1] = 0;
    }
    row_write_view<NW, CN>(g, pos, 0, i * leaves, leaf_obs, leaf_dtype, leaf_mask, lane);
    puct_row_void_slots<NW, CN>(g, row, L, pos, i, leaves, leaf_obs, leaf_dtype, leaf_mask, lane);
    return;
  }
  // ---- the subtree of node v, carried over (mnk_puct_tree.h)
  puct_carry_subtree<NW>(C, NWg, row, L, pos, nodes, v, keep, i, carried, map, inv, lane);
  row_write_view<NW, CN>(g, pos, 0, i * leaves, leaf_obs, leaf_dtype, leaf_mask, lane);
  puct_row_void_slots<NW, CN>(g, row, L, pos, i, leaves, leaf_obs, leaf_dtype, leaf_mask, lane);
}

#define MNK_PUCT_REBASE_LDS                                                                                      \
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];                                                            \
  __shared__ uint32_t lds_new[MNK_PUCT_ROWS][2 * NW]; /* the stones the row has and the stored root has not */ \
  __shared__ uint16_t lds_map[MNK_PUCT_ROWS][MNK_PUCT_ITERS_MAX + 2];                                            \
  __shared__ uint16_t lds_inv[MNK_PUCT_ROWS][MNK_PUCT_ITERS_MAX + 2];

template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_rebase(MnkGeom g, const void* obs, int obs_dtype, int64_t N, int I, int keep, unsigned char* ws, void* leaf_obs,
              int leaf_dtype, uint8_t* leaf_mask, int32_t* carried) {
  MNK_PUCT_REBASE_LDS
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  puct_rebase_row<NW, CN>(g, obs, obs_dtype, i, I, keep, 1, ws, leaf_obs, leaf_dtype, leaf_mask, carried, lds_pos[wave],
                          lds_new[wave], lds_map[wave], lds_inv[wave], lane);
}

template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_rebase_leaves(MnkGeom g, const void* obs, int obs_dtype, int64_t N, int I, int keep, int leaves, unsigned char* ws,
                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int32_t* carried) {
  MNK_PUCT_REBASE_LDS
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  puct_rebase_row<NW, CN>(g, obs, obs_dtype, i, I, keep, leaves, ws, leaf_obs, leaf_dtype, leaf_mask, carried,
                          lds_pos[wave], lds_new[wave], lds_map[wave], lds_inv[wave], lane);
}

// ------------------------------------------------------------------ one backup, then one selection (or the move)

// The move, the visits, the root value of row i, after its last backup.
// SOLVER: the counts are the adjusted ones (`keep`: 0 = every child's n, 1 = the WIN children's, 2 = all but the LOSS
// children's), a proven root's value is exact, and `proof` takes the root's proof for its side to move.
template <bool SOLVER = false>
__device__ __forceinline__ void puct_move(int C, const MnkPuctNode* node, const uint16_t* child, int nodes, bool live,
                                          int temperature, uint64_t seed, const uint64_t* seed_dev, uint64_t step,
                                          const uint64_t* step_dev, int64_t env_id0, int deterministic, int64_t i,
                                          int64_t* actions, int32_t* visits, float* root_value, int lane,
                                          int8_t* proof = nullptr) {
  if (step_dev) step += *step_dev;
  if (seed_dev) seed = *seed_dev;
  const uint32_t x = deterministic ? 0u : mnk_rand_u32(seed, (uint64_t)(env_id0 + i), step, MNK_STREAM_SAMPLE);
  if constexpr (SOLVER) {
    auto count = [&](int a, int keep) { return puct_kept_count(puct_root_kid(C, node, child, nodes, live, a), keep); };
    uint32_t maxn = 0u, tot = 0u;
    const int keep = puct_root_keep(C, node, child, nodes, live, lane, maxn, tot);
    if (visits)
      for (int a = lane; a < C; a += 64) visits[i * C + a] = (int32_t)count(a, keep);
    int move = (int)__umulhi(x, (uint32_t)C);  // no legal cell: a draw over all C cells
    if (maxn)
      mnk_pick_by_visits(C, x, temperature == 1 && !deterministic, maxn, tot, lane, [&](int a) { return count(a, keep); },
                         move);
    if (lane == 0) {
      const uint32_t pf = MNK_PUCT_PROOF(node[0].info);  // from the view of the side that is NOT to move
      actions[i] = move;
      if (root_value) root_value[i] = pf ? (float)((int)pf - 2) : __fdiv_rn(-node[0].w, (float)node[0].n);
      if (proof) proof[i] = pf ? (int8_t)((int)pf - 2) : (int8_t)MNK_PROOF_UNKNOWN;
    }
    return;
  }
  uint32_t maxn = 0u, tot = 0u;
  for (int a = lane; a < C; a += 64) {
    const uint32_t ch = live ? child[a] : MNK_PUCT_NONE;
    const uint32_t na = (ch != 0u && ch != MNK_PUCT_NONE) ? node[min((int)ch, nodes - 1)].n : 0u;
    if (visits) visits[i * C + a] = (int32_t)na;
    maxn = max(maxn, na);
    tot += na;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
    tot += (uint32_t)__shfl_xor((int)tot, off, 64);
  }
  int move = (int)__umulhi(x, (uint32_t)C);  // no legal cell: a draw over all C cells
  if (maxn)
    mnk_pick_by_visits(C, x, temperature == 1 && !deterministic, maxn, tot, lane, [&](int a) {
      const uint32_t ch = a < C ? child[a] : 0u;
      return (ch != 0u && ch != MNK_PUCT_NONE) ? node[min((int)ch, nodes - 1)].n : 0u;
    }, move);
  if (lane == 0) {
    actions[i] = move;
    if (root_value) root_value[i] = __fdiv_rn(-node[0].w, (float)node[0].n);
  }
}

// a sum over the wave, the same value in every lane
__device__ __forceinline__ double puct_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// The move, the visits, the root value and the improved policy of row i, after its last backup (the rule:
// include/mnk_hip.h, mnk_puct_step_gumbel).  The policy is f64: five passes over the root's cells (the sum of the clamped
// priors; the visited cells' sums for v_mix; the maximum of y; the sum of exp(y - max); the store), every pass
// recomputing a cell's terms from the tree -- the same operations on the same inputs give the same y each time -- and
// reduced over the wave.  pr = the root's stored priors (node 0's row).
__device__ __forceinline__ void puct_move_gumbel(int C, int I, const MnkPuctNode* node, const float* pr, const uint16_t* cl,
                                                 int nodes, bool live, const MnkPuctGumbel& gm, float vroot, uint64_t seed,
                                                 const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev,
                                                 int64_t env_id0, int deterministic, int64_t i, int64_t* actions,
                                                 int32_t* visits, float* root_value, float* policy, int lane) {
  if (!live) {  // no legal cell: the draw over all C cells of mnk_puct_step, no visits, no policy
    if (step_dev) step += *step_dev;
    if (seed_dev) seed = *seed_dev;
    const uint32_t x = deterministic ? 0u : mnk_rand_u32(seed, (uint64_t)(env_id0 + i), step, MNK_STREAM_SAMPLE);
    for (int a = lane; a < C; a += 64) {
      if (visits) visits[i * C + a] = 0;
      if (policy) policy[i * C + a] = 0.0f;
    }
    if (lane == 0) {
      actions[i] = (int)__umulhi(x, (uint32_t)C);
      if (root_value) root_value[i] = __fdiv_rn(-node[0].w, (float)node[0].n);
    }
    return;
  }
  uint32_t maxn = 0u;
  const int move = puct_gumbel_pick<true>(C, I, node, cl, nodes, gm, lane, &maxn);
  if (lane == 0) {
    actions[i] = move == 0x7fffffff ? 0 : move;
    if (root_value) root_value[i] = __fdiv_rn(-node[0].w, (float)node[0].n);
  }
  if (!visits && !policy) return;
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
  for (int a = lane; a < C; a += 64) {
    const bool fr = cell(a, p, na, q);
    if (visits) visits[i * C + a] = fr ? (int32_t)na : 0;
    if (fr) {
      sp += p;
      ns += na;
    }
  }
  if (!policy) return;
  sp = puct_wave_sum(sp);
#pragma unroll
  for (int off = 32; off; off >>= 1) ns += (uint32_t)__shfl_xor((int)ns, off, 64);
  double sv = 0.0, sq = 0.0;
  for (int a = lane; a < C; a += 64)
    if (cell(a, p, na, q) && na) {
      sv += p / sp;
      sq += p / sp * q;
    }
  sv = puct_wave_sum(sv);
  sq = puct_wave_sum(sq);
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
  se = puct_wave_sum(se);
  for (int a = lane; a < C; a += 64) policy[i * C + a] = y_of(a, y) ? (float)(exp(y - my) / se) : 0.0f;
}

// One wave per row, MNK_PUCT_ROWS rows per workgroup.  Selection is wave-uniform: the position in registers, the scores
// of a node's C cells spread over the lanes and reduced to the maximum, ties to the lowest cell.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_step(MnkGeom g, unsigned char* ws, int64_t N, int I, const void* priors, int priors_dtype, const void* values,
            int values_dtype, float c, int last, int temperature, uint64_t seed, const uint64_t* seed_dev, uint64_t step,
            const uint64_t* step_dev, int64_t env_id0, int deterministic, void* leaf_obs, int leaf_dtype,
            uint8_t* leaf_mask, int64_t* actions, int32_t* visits, float* root_value) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW;
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
  // (clamped: a workspace that mnk_puct_begin did not set up cannot send a store outside the row)
  int nodes = (int)min(hdr[0], (uint32_t)(I + 1));
  const int depth = (int)min(hdr[1], (uint32_t)I);
  const uint32_t state = hdr[2];
  const bool live = hdr[3] != 0u;
  for (int q = lane; q < 2 * NW; q += 64) {
    const int pl = q >= NW, w = q - (pl ? NW : 0);
    pos[q] = w < NWg ? leafp[pl * NWg + w] : 0u;
  }
  row_wave_sync();

  // ---- backup of the pending evaluation
  if (state & 1u)
    puct_backup<NW, CN>(g, pos, path, node, prior, child, nodes, depth, state, priors, priors_dtype, values, values_dtype,
                        i, lane);

  if (last) {
    puct_move(C, node, child, nodes, live, temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, i, actions,
              visits, root_value, lane);
    return;
  }

  // ---- selection
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a row without a legal cell (or a full tree) shows its root again
  if (live && nodes <= I) {
    MnkEnv<NW> e;
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
  }
  row_wave_sync();
  for (int q = lane; q < 2 * NWg; q += 64) leafp[q] = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
  row_write_view<NW, CN>(g, pos, d & 1, i, leaf_obs, leaf_dtype, leaf_mask, lane);
}

// ------------------------------------------------------------------ a round: `leaves` backups, then `leaves` selections
// One wave per row as above.  Slot j of row i is batch row i * leaves + j.  The backups run in slot order with a wave
// sync between them (paths share nodes), each lane-parallel over its path.  Then the slots select one after the other,
// each under the virtual visits of the slots before it (puct_walk<VL>), and every slot's leaf is written out as soon as
// it is known: planes through the wave's LDS stage, the one part of a slot that every lane reads.  The paths stay in the
// workspace (at the maxima 4 rows x 16 slots x 2 050 u16 exceed the CU's LDS); a walk reads one entry per earlier slot and
// node.  A slot without a leaf is void (state 0, the root's view), and so is every slot after it: nothing has changed
// that its walk could see.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_step_leaves(MnkGeom g, unsigned char* ws, int64_t N, int I, int leaves, const void* priors, int priors_dtype,
                   const void* values, int values_dtype, float c, int last, int temperature, uint64_t seed,
                   const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic,
                   void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions, int32_t* visits,
                   float* root_value) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW;
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
  // (clamped: a workspace that mnk_puct_begin_leaves did not set up cannot send a store outside the row)
  int nodes = (int)min(hdr[0], (uint32_t)(I + 1));
  const bool live = hdr[3] != 0u;

  // ---- the backups of the pending evaluations, in slot order
  for (int j = 0; j < leaves; ++j) {
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
    puct_backup<NW, CN>(g, pos, slot_path(j), node, prior, child, nodes, depth, state, priors, priors_dtype, values,
                        values_dtype, i * leaves + j, lane);
  }

  if (last) {
    puct_move(C, node, child, nodes, live, temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, i, actions,
              visits, root_value, lane);
    return;
  }

  // ---- the selections
  const int nodes0 = nodes;
  const uint16_t* epath = slot_path(min(lane, leaves - 1));  // lane l < leaves: slot l's path
  int edepth = 0;                                            // and, once it has selected, its leaf's depth
  uint32_t active = 0u;                                      // the slots of this round that have a leaf
  bool open = live;                                          // no slot was void yet
  for (int j = 0; j < leaves; ++j) {
    int d = 0;
    uint32_t nstate = 0u;
    uint16_t* path = slot_path(j);
    MnkEnv<NW> e;
    if (open && nodes <= I) {
      puct_env_root<NW>(e, root, NWg);
      nstate = puct_walk<NW, CN, CK, true>(g, e, I, c, node, prior, child, path, nodes, d, lane, nodes0, active, epath,
                                           edepth);
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
  if (lane == 0) hdr[0] = (uint32_t)nodes;
}

// ------------------------------------------------------------------ a round that proves wins, draws and losses
// k_puct_step_leaves (for any number of leaves, 1 included) with the solver's parts of puct_backup, puct_walk and
// puct_move compiled in: the backups prove what they can along their paths, a root that is proven selects nothing (its
// slots are void, as those of a full tree), and the move is made from the adjusted counts.  The rule: include/mnk_hip.h,
// mnk_puct_step_solver.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_step_solver(MnkGeom g, unsigned char* ws, int64_t N, int I, int leaves, const void* priors, int priors_dtype,
                   const void* values, int values_dtype, float c, int last, int temperature, uint64_t seed,
                   const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic,
                   void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions, int32_t* visits,
                   float* root_value, int8_t* proof) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW;
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
  // (clamped: a workspace that mnk_puct_begin_leaves did not set up cannot send a store outside the row)
  int nodes = (int)min(hdr[0], (uint32_t)(I + 1));
  const bool live = hdr[3] != 0u;

  // ---- the backups of the pending evaluations, in slot order
  for (int j = 0; j < leaves; ++j) {
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
    puct_backup<NW, CN, true>(g, pos, slot_path(j), node, prior, child, nodes, depth, state, priors, priors_dtype, values,
                              values_dtype, i * leaves + j, lane);
  }

  if (last) {
    puct_move<true>(C, node, child, nodes, live, temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, i,
                    actions, visits, root_value, lane, proof);
    return;
  }

  // ---- the selections
  const int nodes0 = nodes;
  const uint16_t* epath = slot_path(min(lane, leaves - 1));  // lane l < leaves: slot l's path
  int edepth = 0;                                            // and, once it has selected, its leaf's depth
  uint32_t active = 0u;                                      // the slots of this round that have a leaf
  bool open = live;                                          // no slot was void yet
  if (MNK_PUCT_PROOF(node[0].info)) open = false;            // a proven root: nothing left to search
  for (int j = 0; j < leaves; ++j) {
    int d = 0;
    uint32_t nstate = 0u;
    uint16_t* path = slot_path(j);
    MnkEnv<NW> e;
    if (open && nodes <= I) {
      puct_env_root<NW>(e, root, NWg);
      nstate = puct_walk<NW, CN, CK, true, true>(g, e, I, c, node, prior, child, path, nodes, d, lane, nodes0, active,
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
  if (lane == 0) hdr[0] = (uint32_t)nodes;
}

// ------------------------------------------------------------------ a round with first-play urgency
// k_puct_step_leaves (SOLVER: k_puct_step_solver) with the first-play urgency of puct_walk compiled in: a free cell
// without a visit scores from its parent's own mean value, less a reduction that grows with the prior mass already
// visited, in the place of q = 0.  The backups, the move and the slots are those kernels'; proof is read with SOLVER
// only.  The rule: include/mnk_hip.h, mnk_puct_step_fpu.
template <int NW, int CN, int CK, bool SOLVER>
__global__ void __launch_bounds__(256)
k_puct_step_fpu(MnkGeom g, unsigned char* ws, int64_t N, int I, int leaves, const void* priors, int priors_dtype,
                const void* values, int values_dtype, float c, int last, int temperature, uint64_t seed,
                const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic,
                void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions, int32_t* visits, float* root_value,
                int8_t* proof, float fpu, float fpu_root) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW;
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
  // (clamped: a workspace that mnk_puct_begin_leaves did not set up cannot send a store outside the row)
  int nodes = (int)min(hdr[0], (uint32_t)(I + 1));
  const bool live = hdr[3] != 0u;

  // ---- the backups of the pending evaluations, in slot order
  for (int j = 0; j < leaves; ++j) {
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
  }

  if (last) {
    puct_move<SOLVER>(C, node, child, nodes, live, temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, i,
                      actions, visits, root_value, lane, proof);
    return;
  }

  // ---- the selections
  const int nodes0 = nodes;
  const uint16_t* epath = slot_path(min(lane, leaves - 1));  // lane l < leaves: slot l's path
  int edepth = 0;                                            // and, once it has selected, its leaf's depth
  uint32_t active = 0u;                                      // the slots of this round that have a leaf
  bool open = live;                                          // no slot was void yet
  if constexpr (SOLVER)
    if (MNK_PUCT_PROOF(node[0].info)) open = false;  // a proven root: nothing left to search
  for (int j = 0; j < leaves; ++j) {
    int d = 0;
    uint32_t nstate = 0u;
    uint16_t* path = slot_path(j);
    MnkEnv<NW> e;
    if (open && nodes <= I) {
      puct_env_root<NW>(e, root, NWg);
      nstate = puct_walk<NW, CN, CK, true, SOLVER, false, true>(g, e, I, c, node, prior, child, path, nodes, d, lane, nodes0,
                                                                active, epath, edepth, nullptr, fpu, fpu_root);
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
  if (lane == 0) hdr[0] = (uint32_t)nodes;
}

// ------------------------------------------------------------------ a step whose root is a Gumbel root
// k_puct_step (one leaf per row and evaluation, the same workspace) with the root's part of puct_walk replaced by
// puct_gumbel_pick and puct_move by puct_move_gumbel; below the root the walk and the backup are k_puct_step's.  The
// rule: include/mnk_hip.h, mnk_puct_step_gumbel.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_step_gumbel(MnkGeom g, unsigned char* ws, int64_t N, int I, const void* priors, int priors_dtype, const void* values,
                   int values_dtype, float c, int last, int considered, float c_visit, float c_scale,
                   const uint16_t* table, const float* gscore, const float* vroot, uint64_t seed, const uint64_t* seed_dev,
                   uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic, void* leaf_obs,
                   int leaf_dtype, uint8_t* leaf_mask, int64_t* actions, int32_t* visits, float* root_value,
                   float* policy) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW;
  const MnkPuctLayout L = mnk_puct_layout(NWg, C, I, 1);
  unsigned char* row = ws + i * L.row;
  uint32_t* hdr = (uint32_t*)row;
  const uint32_t* root = (const uint32_t*)(row + L.root);
  uint32_t* leafp = (uint32_t*)(row + L.leaf);
  uint16_t* path = (uint16_t*)(row + L.path);
  MnkPuctNode* node = (MnkPuctNode*)(row + L.node);
  float* prior = (float*)(row + L.prior);
  uint16_t* child = (uint16_t*)(row + L.child);
  uint32_t* pos = lds_pos[wave];
  // (clamped: a workspace that mnk_puct_begin_leaves did not set up cannot send a store outside the row)
  int nodes = (int)min(hdr[0], (uint32_t)(I + 1));
  const int depth = (int)min(hdr[1], (uint32_t)I);
  const uint32_t state = hdr[2];
  const bool live = hdr[3] != 0u;
  for (int q = lane; q < 2 * NW; q += 64) {
    const int pl = q >= NW, w = q - (pl ? NW : 0);
    pos[q] = w < NWg ? leafp[pl * NWg + w] : 0u;
  }
  row_wave_sync();
  MnkPuctGumbel gm;
  gm.gs = gscore + i * C;
  gm.table = table;
  gm.considered = considered;
  gm.c_visit = c_visit;
  gm.c_scale = c_scale;

  // ---- backup of the pending evaluation
  if (state & 1u)
    puct_backup<NW, CN>(g, pos, path, node, prior, child, nodes, depth, state, priors, priors_dtype, values, values_dtype,
                        i, lane);

  if (last) {
    puct_move_gumbel(C, I, node, prior, child, nodes, live, gm, policy ? vroot[i] : 0.0f, seed, seed_dev, step, step_dev,
                     env_id0, deterministic, i, actions, visits, root_value, policy, lane);
    return;
  }

  // ---- selection
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a row without a legal cell (or a full tree) shows its root again
  if (live && nodes <= I) {
    MnkEnv<NW> e;
    puct_env_root<NW>(e, root, NWg);
    nstate = puct_walk<NW, CN, CK, false, false, true>(g, e, I, c, node, prior, child, path, nodes, d, lane, 0, 0u, nullptr,
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
  }
  row_wave_sync();
  for (int q = lane; q < 2 * NWg; q += 64) leafp[q] = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
  row_write_view<NW, CN>(g, pos, d & 1, i, leaf_obs, leaf_dtype, leaf_mask, lane);
}

// ------------------------------------------------------------------ the entry points
// what the four pairs of entry points share: the host checks (before anything is enqueued) and the launch.  leaves = 0
// stands for the entry point without the argument: today's kernels, one leaf.
static bool puct_leaves_ok(int iterations, int leaves) {
  return leaves == 0 || (leaves >= 1 && leaves <= MNK_PUCT_LEAVES_MAX && iterations % leaves == 0);
}

static int64_t puct_workspace_bytes(int64_t N, int m, int n, int iterations, int leaves) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, 1, &g);
  if (rc != MNK_OK) return rc;
  if (N < 0 || iterations < 1 || iterations > MNK_PUCT_ITERS_MAX || !puct_leaves_ok(iterations, leaves)) return MNK_EINVAL;
  return N * mnk_puct_layout(g.NW, g.C, iterations, leaves ? leaves : 1).row;
}

static int puct_begin(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, int leaves,
                      void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, void* stream) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  if (!obs || !workspace || !leaf_obs || !leaf_mask || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_ROWS || !mnk_obs_dtype_ok(obs_dtype) ||
      !mnk_obs_dtype_ok(leaf_dtype) || iterations < 1 || iterations > MNK_PUCT_ITERS_MAX || !puct_leaves_ok(iterations, leaves))
    return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  hipStream_t s = (hipStream_t)stream;
  if (leaves)
    MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_begin_leaves), grid, block, 0, s, g, obs, obs_dtype, N, iterations,
                                       leaves, (unsigned char*)workspace, leaf_obs, leaf_dtype, leaf_mask));
  else
    MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_begin), grid, block, 0, s, g, obs, obs_dtype, N, iterations,
                                       (unsigned char*)workspace, leaf_obs, leaf_dtype, leaf_mask));
  return mnk_launch_status(leaves ? "puct_begin_leaves" : "puct_begin");
}

static int puct_rebase(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int tree_iterations, int keep_nodes,
                       int leaves, void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int32_t* carried,
                       void* stream) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  // (at least one round's room: keep_nodes <= tree_iterations + 1 - J, J >= leaves)
  if (!obs || !workspace || !leaf_obs || !leaf_mask || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_ROWS || !mnk_obs_dtype_ok(obs_dtype) ||
      !mnk_obs_dtype_ok(leaf_dtype) || tree_iterations < 1 || tree_iterations > MNK_PUCT_ITERS_MAX ||
      !puct_leaves_ok(tree_iterations, leaves) || keep_nodes < 1 || keep_nodes > tree_iterations + 1 - (leaves ? leaves : 1))
    return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  hipStream_t s = (hipStream_t)stream;
  if (leaves)
    MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_rebase_leaves), grid, block, 0, s, g, obs, obs_dtype, N, tree_iterations,
                                       keep_nodes, leaves, (unsigned char*)workspace, leaf_obs, leaf_dtype, leaf_mask,
                                       carried));
  else
    MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_rebase), grid, block, 0, s, g, obs, obs_dtype, N, tree_iterations,
                                       keep_nodes, (unsigned char*)workspace, leaf_obs, leaf_dtype, leaf_mask, carried));
  return mnk_launch_status(leaves ? "puct_rebase_leaves" : "puct_rebase");
}

static int puct_step(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                     int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                     uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                     int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                     int32_t* visits, float* root_value, void* stream, bool solver = false, int8_t* proof = nullptr,
                     bool with_fpu = false, float fpu = 0.0f, float fpu_root = 0.0f) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  const bool dt_ok = (priors_dtype == MNK_LOGITS_F32 || priors_dtype == MNK_LOGITS_BF16) &&
                     (values_dtype == MNK_LOGITS_F32 || values_dtype == MNK_LOGITS_BF16);
  if (!workspace || !priors || !values || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_ROWS || !dt_ok || iterations < 1 ||
      iterations > MNK_PUCT_ITERS_MAX || !(c >= 0.0f && c <= 3.0e38f) || (last != 0 && last != 1) ||
      (temperature != 0 && temperature != 1) || !puct_leaves_ok(iterations, leaves))
    return MNK_EINVAL;
  if (last ? !actions : (!leaf_obs || !leaf_mask || !mnk_obs_dtype_ok(leaf_dtype))) return MNK_EINVAL;
  if (with_fpu && (!(fpu >= 0.0f && fpu <= 3.0e38f) || !(fpu_root >= 0.0f && fpu_root <= 3.0e38f))) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  hipStream_t s = (hipStream_t)stream;
#define MNK_PUCT_STEP_FPU(SOLVER)                                                                                        \
  MNK_DISPATCH(g, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_puct_step_fpu<NW, CN, CK, SOLVER>), grid, block, 0, s, g,         \
                                     (unsigned char*)workspace, N, iterations, leaves, priors, priors_dtype, values,     \
                                     values_dtype, c, last, temperature, seed, seed_dev, step, step_dev, env_id0,        \
                                     deterministic, leaf_obs, leaf_dtype, leaf_mask, actions, visits, root_value, proof, \
                                     fpu, fpu_root))
  if (with_fpu) {
    if (solver) MNK_PUCT_STEP_FPU(true);
    else MNK_PUCT_STEP_FPU(false);
    return mnk_launch_status("puct_step_fpu");
  }
#undef MNK_PUCT_STEP_FPU
  if (solver)
    MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_step_solver), grid, block, 0, s, g, (unsigned char*)workspace, N,
                                       iterations, leaves, priors, priors_dtype, values, values_dtype, c, last,
                                       temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, leaf_obs,
                                       leaf_dtype, leaf_mask, actions, visits, root_value, proof));
  else if (leaves)
    MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_step_leaves), grid, block, 0, s, g, (unsigned char*)workspace, N,
                                       iterations, leaves, priors, priors_dtype, values, values_dtype, c, last,
                                       temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, leaf_obs,
                                       leaf_dtype, leaf_mask, actions, visits, root_value));
  else
    MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_step), grid, block, 0, s, g, (unsigned char*)workspace, N, iterations,
                                       priors, priors_dtype, values, values_dtype, c, last, temperature, seed, seed_dev,
                                       step, step_dev, env_id0, deterministic, leaf_obs, leaf_dtype, leaf_mask, actions,
                                       visits, root_value));
  return mnk_launch_status(solver ? "puct_step_solver" : leaves ? "puct_step_leaves" : "puct_step");
}

extern "C" {

int64_t mnk_puct_workspace_bytes(int64_t N, int m, int n, int iterations) {
  return puct_workspace_bytes(N, m, n, iterations, 0);
}
int64_t mnk_puct_workspace_bytes_leaves(int64_t N, int m, int n, int iterations, int leaves) {
  return leaves ? puct_workspace_bytes(N, m, n, iterations, leaves) : MNK_EINVAL;
}

int mnk_puct_begin(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, void* workspace,
                   void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, void* stream) {
  return puct_begin(obs, obs_dtype, N, m, n, k, iterations, 0, workspace, leaf_obs, leaf_dtype, leaf_mask, stream);
}
int mnk_puct_begin_leaves(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, int leaves,
                          void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, void* stream) {
  if (!leaves) return MNK_EINVAL;
  return puct_begin(obs, obs_dtype, N, m, n, k, iterations, leaves, workspace, leaf_obs, leaf_dtype, leaf_mask, stream);
}

int mnk_puct_rebase(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int tree_iterations, int keep_nodes,
                    void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int32_t* carried, void* stream) {
  return puct_rebase(obs, obs_dtype, N, m, n, k, tree_iterations, keep_nodes, 0, workspace, leaf_obs, leaf_dtype, leaf_mask,
                     carried, stream);
}
int mnk_puct_rebase_leaves(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int tree_iterations,
                           int keep_nodes, int leaves, void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask,
                           int32_t* carried, void* stream) {
  if (!leaves) return MNK_EINVAL;
  return puct_rebase(obs, obs_dtype, N, m, n, k, tree_iterations, keep_nodes, leaves, workspace, leaf_obs, leaf_dtype,
                     leaf_mask, carried, stream);
}

int mnk_puct_step(void* workspace, int64_t N, int m, int n, int k, int iterations, const void* priors, int priors_dtype,
                  const void* values, int values_dtype, float c, int last, int temperature, uint64_t seed,
                  const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic,
                  void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions, int32_t* visits,
                  float* root_value, void* stream) {
  return puct_step(workspace, N, m, n, k, iterations, 0, priors, priors_dtype, values, values_dtype, c, last, temperature,
                   seed, seed_dev, step, step_dev, env_id0, deterministic, leaf_obs, leaf_dtype, leaf_mask, actions, visits,
                   root_value, stream);
}
int mnk_puct_step_leaves(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, void* stream) {
  if (!leaves) return MNK_EINVAL;
  return puct_step(workspace, N, m, n, k, iterations, leaves, priors, priors_dtype, values, values_dtype, c, last,
                   temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, leaf_obs, leaf_dtype, leaf_mask,
                   actions, visits, root_value, stream);
}
int mnk_puct_step_solver(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, int8_t* proof, void* stream) {
  if (!leaves) return MNK_EINVAL;
  return puct_step(workspace, N, m, n, k, iterations, leaves, priors, priors_dtype, values, values_dtype, c, last,
                   temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, leaf_obs, leaf_dtype, leaf_mask,
                   actions, visits, root_value, stream, true, proof);
}

int mnk_puct_step_fpu(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                      int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                      uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                      int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                      int32_t* visits, float* root_value, int8_t* proof, int solver, float fpu, float fpu_root,
                      void* stream) {
  if (!leaves || (solver != 0 && solver != 1)) return MNK_EINVAL;
  return puct_step(workspace, N, m, n, k, iterations, leaves, priors, priors_dtype, values, values_dtype, c, last,
                   temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, leaf_obs, leaf_dtype, leaf_mask,
                   actions, visits, root_value, stream, solver != 0, solver ? proof : nullptr, true, fpu, fpu_root);
}

int mnk_puct_step_gumbel(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int considered,
                         float c_visit, float c_scale, const uint16_t* table, const float* gscore, const float* vroot,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, float* policy, void* stream) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  const bool dt_ok = (priors_dtype == MNK_LOGITS_F32 || priors_dtype == MNK_LOGITS_BF16) &&
                     (values_dtype == MNK_LOGITS_F32 || values_dtype == MNK_LOGITS_BF16);
  if (!workspace || !priors || !values || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_ROWS || !dt_ok || iterations < 1 ||
      iterations > MNK_PUCT_ITERS_MAX || !(c >= 0.0f && c <= 3.0e38f) || (last != 0 && last != 1) || leaves != 1 ||
      considered < 1 || considered > MNK_PUCT_CONSIDERED_MAX || !(c_visit >= 0.0f && c_visit <= 3.0e38f) ||
      !(c_scale >= 0.0f && c_scale <= 3.0e38f) || !table || !gscore)
    return MNK_EINVAL;
  if (last ? (!actions || (policy && !vroot)) : (!leaf_obs || !leaf_mask || !mnk_obs_dtype_ok(leaf_dtype)))
    return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_step_gumbel), grid, block, 0, (hipStream_t)stream, g,
                                     (unsigned char*)workspace, N, iterations, priors, priors_dtype, values, values_dtype, c,
                                     last, considered, c_visit, c_scale, table, gscore, vroot, seed, seed_dev, step,
                                     step_dev, env_id0, deterministic, leaf_obs, leaf_dtype, leaf_mask, actions, visits,
                                     root_value, policy));
  return mnk_launch_status("puct_step_gumbel");
}

}  // extern "C"
