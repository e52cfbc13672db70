// mnk_puct.hip -- the PUCT search player (gfx950 / MI355X only): AlphaZero-style search guided by a caller's evaluator
// (normally a policy/value network), batched over rows.  The tree lives in a device workspace between launches; each
// launch backs up the previous evaluation and selects the next leaf (mnk_puct_step), so an act() is mnk_puct_begin,
// I + 1 evaluator calls and I + 1 steps with no host synchronisation.  mnk_puct_rebase in the place of mnk_puct_begin
// carries the subtree of the position that was reached into the next search.  The *_leaves entry points run the same
// search with L leaves per row and evaluation (a round = L backups, then L selections under virtual visits), so the
// evaluator sees I / L + 1 batches of N * L rows.  mnk_puct_step_solver is mnk_puct_step_leaves with exact proofs of wins,
// draws and losses in the backup (a 2-bit proof per node, propagated up the leaf's path), mnk_puct_step_fpu either of them
// with first-play urgency, mnk_puct_step_forced any of those with forced playouts and policy target pruning,
// mnk_puct_step_gumbel mnk_puct_step with a Gumbel root.  The rule: include/mnk_hip.h.
//
// What is here: one begin kernel and one rebase kernel (an entry point without `leaves` launches them with 1: the layout of
// one leaf is the layout without the argument); the moves; ONE body of a step, puct_step_row, which the ten step kernels
// instantiate -- k_puct_step and k_puct_step_gumbel with one leaf and the walk without virtual visits,
// k_puct_step_leaves<SOLVER, FPU, FORCED> as the round -- around the pieces of mnk_puct_tree.h; and the host side: one
// argument block, one check of it, one launch shape.
#include "mnk_host.h"
#include "mnk_wave_rows.h"
#include "mnk_puct_tree.h"

// what every kernel here begins with: one wave per row, MNK_PUCT_ROWS rows per workgroup; row i, the wave's stage `pos`
#define MNK_PUCT_WAVE_ROW(N)                                       \
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];              \
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;      \
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;    \
  if (i >= (N)) return;                                            \
  uint32_t* pos = lds_pos[wave];

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
k_puct_begin_leaves(MnkGeom g, const void* obs, int obs_dtype, int64_t N, int I, int leaves, unsigned char* ws,
                    void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask) {
  MNK_PUCT_WAVE_ROW(N)
  puct_begin_row<NW, CN>(g, obs, obs_dtype, i, I, leaves, ws, leaf_obs, leaf_dtype, leaf_mask, pos, lane);
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
  // (clamped, as in puct_header: whatever the workspace holds, no id leaves the row)
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

  if (plies < 0) {  // exactly what k_puct_begin_leaves writes
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

template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_rebase_leaves(MnkGeom g, const void* obs, int obs_dtype, int64_t N, int I, int keep, int leaves, unsigned char* ws,
                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int32_t* carried) {
  MNK_PUCT_WAVE_ROW(N)
  __shared__ uint32_t lds_new[MNK_PUCT_ROWS][2 * NW];  // the stones the row has and the stored root has not
  __shared__ uint16_t lds_map[MNK_PUCT_ROWS][MNK_PUCT_ITERS_MAX + 2];
  __shared__ uint16_t lds_inv[MNK_PUCT_ROWS][MNK_PUCT_ITERS_MAX + 2];
  puct_rebase_row<NW, CN>(g, obs, obs_dtype, i, I, keep, leaves, ws, leaf_obs, leaf_dtype, leaf_mask, carried, pos,
                          lds_new[wave], lds_map[wave], lds_inv[wave], lane);
}

// ------------------------------------------------------------------ a step: the argument block
// What every step kernel takes, as its first parameter; a kernel's own parameters follow it.  leaves: 1 from an entry
// point without the argument.  temperature: 0 from mnk_puct_step_gumbel, which has none.
struct MnkPuctStepArgs {
  MnkGeom g;
  unsigned char* ws;
  int64_t N;
  int I, leaves;
  const void* priors;
  int priors_dtype;
  const void* values;
  int values_dtype;
  float c;
  int last, temperature;
  uint64_t seed;
  const uint64_t* seed_dev;
  uint64_t step;
  const uint64_t* step_dev;
  int64_t env_id0;
  int deterministic;
  void* leaf_obs;
  int leaf_dtype;
  uint8_t* leaf_mask;
  int64_t* actions;
  int32_t* visits;
  float* root_value;
};

// ------------------------------------------------------------------ the move
// the draw of row i's move (0: deterministic)
__device__ __forceinline__ uint32_t puct_move_draw(const MnkPuctStepArgs& a, int64_t i) {
  const uint64_t step = a.step_dev ? a.step + *a.step_dev : a.step, seed = a.seed_dev ? *a.seed_dev : a.seed;
  return a.deterministic ? 0u : mnk_rand_u32(seed, (uint64_t)(a.env_id0 + i), step, MNK_STREAM_SAMPLE);
}

// The move, the visits, the root value of row i, after its last backup.
// SOLVER: the counts are the adjusted ones (`keep`: 0 = every child's n, 1 = the WIN children's, 2 = all but the LOSS
// children's), a proven root's value is exact, and `proof` takes the root's proof for its side to move.
template <bool SOLVER>
__device__ __forceinline__ void puct_move(const MnkPuctStepArgs& a, const MnkPuctNode* node, const uint16_t* child,
                                          int nodes, bool live, int64_t i, int lane, int8_t* proof) {
  const int C = a.g.C;
  const bool sample = a.temperature == 1 && !a.deterministic;
  const uint32_t x = puct_move_draw(a, i);
  int move = (int)__umulhi(x, (uint32_t)C);  // no legal cell: a draw over all C cells
  uint32_t maxn = 0u, tot = 0u;
  if constexpr (SOLVER) {
    auto count = [&](int q, int keep) { return puct_kept_count(puct_root_kid(C, node, child, nodes, live, q), keep); };
    const int keep = puct_root_keep(C, node, child, nodes, live, lane, maxn, tot);
    if (a.visits)
      for (int q = lane; q < C; q += 64) a.visits[i * C + q] = (int32_t)count(q, keep);
    if (maxn) mnk_pick_by_visits(C, x, sample, maxn, tot, lane, [&](int q) { return count(q, keep); }, move);
    if (lane == 0) {
      const uint32_t pf = MNK_PUCT_PROOF(node[0].info);  // from the view of the side that is NOT to move
      a.actions[i] = move;
      if (a.root_value) a.root_value[i] = pf ? (float)((int)pf - 2) : __fdiv_rn(-node[0].w, (float)node[0].n);
      if (proof) proof[i] = pf ? (int8_t)((int)pf - 2) : (int8_t)MNK_PROOF_UNKNOWN;
    }
    return;
  }
  for (int q = lane; q < C; q += 64) {
    const uint32_t ch = live ? child[q] : MNK_PUCT_NONE;
    const uint32_t na = (ch != 0u && ch != MNK_PUCT_NONE) ? node[min((int)ch, nodes - 1)].n : 0u;
    if (a.visits) a.visits[i * C + q] = (int32_t)na;
    maxn = max(maxn, na);
    tot += na;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
    tot += (uint32_t)__shfl_xor((int)tot, off, 64);
  }
  if (maxn)
    mnk_pick_by_visits(C, x, sample, maxn, tot, lane, [&](int q) {
      const uint32_t ch = q < C ? child[q] : 0u;
      return (ch != 0u && ch != MNK_PUCT_NONE) ? node[min((int)ch, nodes - 1)].n : 0u;
    }, move);
  if (lane == 0) {
    a.actions[i] = move;
    if (a.root_value) a.root_value[i] = __fdiv_rn(-node[0].w, (float)node[0].n);
  }
}

// puct_move<SOLVER> of a search with forced playouts (the rule: include/mnk_hip.h, mnk_puct_step_forced): the counts n' of
// puct_move go to raw_visits, and visits and the move take the pruned counts n'' (puct_prune_root, puct_pruned_count;
// nothing is pruned when the solver keeps the WIN children alone).  pr = the root's stored priors.  A cell's n'' is
// computed again wherever it is read -- the store, the sum, the pick -- from the same inputs: no scratch.
template <bool SOLVER>
__device__ __forceinline__ void puct_move_forced(const MnkPuctStepArgs& a, const MnkPuctNode* node, const float* pr,
                                                 const uint16_t* child, int nodes, bool live, int64_t i, int lane,
                                                 int8_t* proof, float forced_k, int32_t* raw_visits) {
  const int C = a.g.C;
  const bool sample = a.temperature == 1 && !a.deterministic;
  const uint32_t x = puct_move_draw(a, i);
  int move = (int)__umulhi(x, (uint32_t)C);  // no legal cell: a draw over all C cells
  uint32_t maxn = 0u, tot = 0u;
  int keep = 0;
  if constexpr (SOLVER) keep = puct_root_keep(C, node, child, nodes, live, lane, maxn, tot);
  auto kid = [&](int q) { return puct_root_kid(C, node, child, nodes, live, q); };  // (n = 0 for q >= C)
  auto count = [&](int q) { return puct_kept_count(kid(q), keep); };
  MnkPuctPrune pp = puct_prune_root(C, forced_k, a.c, node, pr, child, nodes, live, count, lane);
  if (keep == 1) pp.on = false;
  auto pruned = [&](int q) { return puct_pruned_count(pp, q, count(q), kid(q), q < C ? pr[q] : 0.0f); };
  maxn = 0u;
  tot = 0u;
  for (int q = lane; q < C; q += 64) {
    const uint32_t na = pruned(q);
    if (raw_visits) raw_visits[i * C + q] = (int32_t)count(q);
    if (a.visits) a.visits[i * C + q] = (int32_t)na;
    maxn = max(maxn, na);
    tot += na;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
    tot += (uint32_t)__shfl_xor((int)tot, off, 64);
  }
  if (maxn) mnk_pick_by_visits(C, x, sample, maxn, tot, lane, pruned, move);
  if (lane == 0) {
    a.actions[i] = move;
    if constexpr (SOLVER) {
      const uint32_t pf = MNK_PUCT_PROOF(node[0].info);  // from the view of the side that is NOT to move
      if (a.root_value) a.root_value[i] = pf ? (float)((int)pf - 2) : __fdiv_rn(-node[0].w, (float)node[0].n);
      if (proof) proof[i] = pf ? (int8_t)((int)pf - 2) : (int8_t)MNK_PROOF_UNKNOWN;
    } else {
      if (a.root_value) a.root_value[i] = __fdiv_rn(-node[0].w, (float)node[0].n);
    }
  }
}

// The move, the visits, the root value and the improved policy (puct_gumbel_policy, mnk_puct_tree.h) of row i, after its
// last backup (the rule: include/mnk_hip.h, mnk_puct_step_gumbel).  pr = the root's stored priors (node 0's row), cl its
// child row.
__device__ __forceinline__ void puct_move_gumbel(const MnkPuctStepArgs& a, const MnkPuctNode* node, const float* pr,
                                                 const uint16_t* cl, int nodes, bool live, const MnkPuctGumbel& gm,
                                                 const float* vroot, float* policy, int64_t i, int lane) {
  const int C = a.g.C;
  uint32_t maxn = 0u;
  // no legal cell: the draw over all C cells of mnk_puct_step, no visits, no policy
  const int move = live ? puct_gumbel_pick<true>(C, a.I, node, cl, nodes, gm, lane, &maxn)
                        : (int)__umulhi(puct_move_draw(a, i), (uint32_t)C);
  if (lane == 0) {
    a.actions[i] = move == 0x7fffffff ? 0 : move;
    if (a.root_value) a.root_value[i] = __fdiv_rn(-node[0].w, (float)node[0].n);
  }
  if (a.visits)
    for (int q = lane; q < C; q += 64) {
      const uint32_t ch = live ? cl[q] : MNK_PUCT_NONE;
      a.visits[i * C + q] = (ch != 0u && ch != MNK_PUCT_NONE) ? (int32_t)node[min((int)ch, nodes - 1)].n : 0;
    }
  if (!policy) return;
  if (live)
    puct_gumbel_policy(C, node, pr, cl, nodes, gm, vroot[i], maxn, lane, [&](int q, float p) { policy[i * C + q] = p; });
  else
    for (int q = lane; q < C; q += 64) policy[i * C + q] = 0.0f;
}

// ------------------------------------------------------------------ a step of row i
// One wave per row.  `leaves` backups, then the move (a.last) or `leaves` selections; slot j of row i is batch row
// i * leaves + j.  The backups run in slot order with a wave sync between them (paths share nodes), each lane-parallel
// over its path.  Selection is wave-uniform: the position in registers, the scores of a node's C cells spread over the
// lanes and reduced to the maximum, ties to the lowest cell.  The slots select one after the other, each (VL) under the
// virtual visits of the slots before it, and every slot's leaf is written out as soon as it is known: planes through the
// wave's LDS stage, the one part of a slot that every lane reads.  The paths stay in the workspace (at the maxima 4 rows x
// 16 slots x 2 050 u16 exceed the CU's LDS); a walk reads one entry per earlier slot and node.  A slot without a leaf -- a
// row without a legal cell, a full tree, a walk that ends in a node of this round -- is void (state 0, the root's view),
// and so is every slot after it: nothing has changed that its walk could see.
// The flags are puct_walk's, puct_backup's and the move's:
//   VL      the round.  Without it `leaves` is the constant 1 and the walk is the one without virtual visits.
//   SOLVER  the backups prove what they can along their paths, and a root that is proven selects nothing (its slots are
//           void, as those of a full tree).  The rule: mnk_puct_step_solver.
//   FPU     a free cell without a visit scores from its parent's own mean value (fpu below the root, fpu_root at it).  The
//           rule: mnk_puct_step_fpu.
//   GUMBEL  the root's part of the walk is puct_gumbel_pick (gm: the row's Gumbel inputs).  The rule: mnk_puct_step_gumbel.
//   FORCED  forced playouts: at the root a visited child short of its floor of visits is selected before any other
//           (forced_k; the kernel's move prunes them again).  The rule: mnk_puct_step_forced.
// move(r, nodes, live): the kernel's move on a.last.
template <int NW, int CN, int CK, bool VL, bool SOLVER, bool FPU, bool GUMBEL, class Move, bool FORCED = false>
__device__ __forceinline__ void puct_step_row(const MnkPuctStepArgs& a, int leaves, int64_t i, uint32_t* pos, int lane,
                                              Move move, float fpu = 0.0f, float fpu_root = 0.0f,
                                              const MnkPuctGumbel* gm = nullptr, float forced_k = 0.0f) {
  const int C = a.g.C, NWg = a.g.NW, I = a.I;
  const MnkPuctRow r = puct_row(a.ws, i, NWg, C, I, leaves);
  const MnkPuctHeader h = puct_header(r.hdr, I);  // (nodes and live; depth and state are a slot's)
  int nodes = h.nodes;

  // ---- the backups of the pending evaluations, in slot order
  for (int j = 0; j < leaves; ++j) {
    const uint32_t* ds = puct_slot_ds(r, j);
    const int depth = (int)min(ds[0], (uint32_t)I);
    const uint32_t state = ds[1];
    if (!(state & 1u)) continue;
    puct_stage_planes<NW>(pos, puct_slot_leaf(r, j, NWg), NWg, lane);
    row_wave_sync();
    puct_backup<NW, CN, SOLVER>(a.g, pos, puct_slot_path(r, j), r.node, r.prior, r.child, nodes, depth, state, a.priors,
                                a.priors_dtype, a.values, a.values_dtype, i * leaves + j, lane);
  }

  if (a.last) {
    move(r, nodes, h.live);
    return;
  }

  // ---- the selections
  const int nodes0 = nodes;
  const uint16_t* epath = puct_slot_path(r, min(lane, leaves - 1));  // lane l < leaves: slot l's path
  int edepth = 0;                                                    // and, once it has selected, its leaf's depth
  uint32_t active = 0u;                                              // the slots of this round that have a leaf
  bool open = h.live;                                                // no slot was void yet
  if constexpr (SOLVER)
    if (MNK_PUCT_PROOF(r.node[0].info)) open = false;  // a proven root: nothing left to search
  for (int j = 0; j < leaves; ++j) {
    int d = 0;
    uint32_t nstate = 0u;
    uint16_t* path = puct_slot_path(r, j);
    MnkEnv<NW> e;
    if (open && nodes <= I) {
      puct_env_root<NW>(e, r.root, NWg);
      nstate = puct_walk<NW, CN, CK, VL, SOLVER, GUMBEL, FPU, FORCED>(a.g, e, I, a.c, r.node, r.prior, r.child, path,
                                                                      nodes, d, lane, nodes0, active, epath, edepth, gm,
                                                                      fpu, fpu_root, forced_k, true);
    }
    if (nstate) {
      active |= 1u << j;
      if (lane == j) edepth = d;
      puct_stage_selection<NW>(pos, e, nstate, r.root, NWg, lane);
    } else {
      d = 0;
      open = false;
      puct_stage_planes<NW>(pos, r.root, NWg, lane);  // (a void slot shows the root)
    }
    puct_store_selection<NW, CN>(a.g, pos, nstate, d, path, puct_slot_ds(r, j), puct_slot_leaf(r, j, NWg), i * leaves + j,
                                 a.leaf_obs, a.leaf_dtype, a.leaf_mask, lane);
    // (the next slot's walk reads this one's node, child entry and path; its write-out reuses pos)
    if constexpr (VL) row_wave_sync();
  }
  if (lane == 0) r.hdr[0] = (uint32_t)nodes;
}

// one leaf per row and evaluation
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256) k_puct_step(MnkPuctStepArgs a) {
  MNK_PUCT_WAVE_ROW(a.N)
  puct_step_row<NW, CN, CK, false, false, false, false>(a, 1, i, pos, lane, [&](const MnkPuctRow& r, int nodes, bool live) {
    puct_move<false>(a, r.node, r.child, nodes, live, i, lane, nullptr);
  });
}

// the round; proof is read with SOLVER only, fpu and fpu_root with FPU, forced_k and raw_visits with FORCED
template <int NW, int CN, int CK, bool SOLVER, bool FPU, bool FORCED = false>
__global__ void __launch_bounds__(256)
k_puct_step_leaves(MnkPuctStepArgs a, int8_t* proof, float fpu, float fpu_root, float forced_k, int32_t* raw_visits) {
  MNK_PUCT_WAVE_ROW(a.N)
  auto move = [&](const MnkPuctRow& r, int nodes, bool live) {
    if constexpr (FORCED) puct_move_forced<SOLVER>(a, r.node, r.prior, r.child, nodes, live, i, lane, proof, forced_k, raw_visits);
    else puct_move<SOLVER>(a, r.node, r.child, nodes, live, i, lane, proof);
  };
  puct_step_row<NW, CN, CK, true, SOLVER, FPU, false, decltype(move), FORCED>(a, a.leaves, i, pos, lane, move, fpu, fpu_root,
                                                                              nullptr, forced_k);
}

// one leaf, the root a Gumbel root (the same workspace as k_puct_step's)
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_step_gumbel(MnkPuctStepArgs a, int considered, float c_visit, float c_scale, const uint16_t* table,
                   const float* gscore, const float* vroot, float* policy) {
  MNK_PUCT_WAVE_ROW(a.N)
  const MnkPuctGumbel gm{gscore + i * a.g.C, table, considered, c_visit, c_scale};
  puct_step_row<NW, CN, CK, false, false, false, true>(a, 1, i, pos, lane, [&](const MnkPuctRow& r, int nodes, bool live) {
    puct_move_gumbel(a, r.node, r.prior, r.child, nodes, live, gm, vroot, policy, i, lane);
  }, 0.0f, 0.0f, &gm);
}

// ------------------------------------------------------------------ the entry points
// what the pairs of entry points share: the host checks (before anything is enqueued) and the launch.  leaves = 0 stands
// for the entry point without the argument: one leaf.
static bool puct_leaves_ok(int iterations, int leaves) {
  return leaves == 0 || (leaves >= 1 && leaves <= MNK_PUCT_LEAVES_MAX && iterations % leaves == 0);
}

// the one launch shape (N > 0): one wave per row, MNK_PUCT_ROWS rows per workgroup
template <typename... P, typename... A>
static void puct_launch(void (*kernel)(P...), int64_t N, void* stream, const A&... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), dim3(64 * MNK_PUCT_ROWS), 0,
                     (hipStream_t)stream, args...);
}

static int64_t puct_workspace_bytes(int64_t N, int m, int n, int iterations, int leaves) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, 1, &g);
  if (rc != MNK_OK) return rc;
  if (N < 0 || iterations < 1 || iterations > MNK_PUCT_ITERS_MAX || !puct_leaves_ok(iterations, leaves)) return MNK_EINVAL;
  return N * mnk_puct_layout(g.NW, g.C, iterations, leaves ? leaves : 1).row;
}

// what mnk_puct_begin* and mnk_puct_rebase* refuse alike: the board's code, else MNK_EINVAL
static int puct_roots_check(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, int leaves,
                            void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, MnkGeom* g) {
  const int rc = mnk_check_geom(m, n, k, g);
  if (rc != MNK_OK) return rc;
  if (!obs || !workspace || !leaf_obs || !leaf_mask || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_ROWS ||
      !mnk_obs_dtype_ok(obs_dtype) || !mnk_obs_dtype_ok(leaf_dtype) || iterations < 1 || iterations > MNK_PUCT_ITERS_MAX ||
      !puct_leaves_ok(iterations, leaves))
    return MNK_EINVAL;
  return MNK_OK;
}

static int puct_begin(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, int leaves,
                      void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, void* stream) {
  MnkGeom g;
  const int rc =
      puct_roots_check(obs, obs_dtype, N, m, n, k, iterations, leaves, workspace, leaf_obs, leaf_dtype, leaf_mask, &g);
  if (rc != MNK_OK) return rc;
  if (N == 0) return MNK_OK;
  MNK_DISPATCH(g, puct_launch(MNK_K(k_puct_begin_leaves), N, stream, g, obs, obs_dtype, N, iterations, leaves ? leaves : 1,
                              (unsigned char*)workspace, leaf_obs, leaf_dtype, leaf_mask));
  return mnk_launch_status(leaves ? "puct_begin_leaves" : "puct_begin");
}

static int puct_rebase(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int tree_iterations, int keep_nodes,
                       int leaves, void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int32_t* carried,
                       void* stream) {
  MnkGeom g;
  const int rc = puct_roots_check(obs, obs_dtype, N, m, n, k, tree_iterations, leaves, workspace, leaf_obs, leaf_dtype,
                                  leaf_mask, &g);
  if (rc != MNK_OK) return rc;
  // (at least one round's room: keep_nodes <= tree_iterations + 1 - J, J >= leaves)
  if (keep_nodes < 1 || keep_nodes > tree_iterations + 1 - (leaves ? leaves : 1)) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  MNK_DISPATCH(g, puct_launch(MNK_K(k_puct_rebase_leaves), N, stream, g, obs, obs_dtype, N, tree_iterations, keep_nodes,
                              leaves ? leaves : 1, (unsigned char*)workspace, leaf_obs, leaf_dtype, leaf_mask, carried));
  return mnk_launch_status(leaves ? "puct_rebase_leaves" : "puct_rebase");
}

// the common arguments of a step's C entry point, under the names the public header gives them in every one, for
// puct_step_check; LEAVES / TEMPERATURE: the entry point's, or 0 where it has none
#define MNK_PUCT_STEP_COMMON(LEAVES, TEMPERATURE)                                                                          \
  workspace, N, m, n, k, iterations, LEAVES, priors, priors_dtype, values, values_dtype, c, last, TEMPERATURE, seed,       \
      seed_dev, step, step_dev, env_id0, deterministic, leaf_obs, leaf_dtype, leaf_mask, actions, visits, root_value

// What every step entry point refuses: the board's code, else MNK_EINVAL.  MNK_OK: `a` is filled.
static int puct_step_check(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                           int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                           uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev,
                           int64_t env_id0, int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask,
                           int64_t* actions, int32_t* visits, float* root_value, MnkPuctStepArgs* a) {
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
  *a = MnkPuctStepArgs{g, (unsigned char*)workspace, N, iterations, leaves ? leaves : 1, priors, priors_dtype, values,
                       values_dtype, c, last, temperature, seed, seed_dev, step, step_dev, env_id0, deterministic, leaf_obs,
                       leaf_dtype, leaf_mask, actions, visits, root_value};
  return MNK_OK;
}

// the round's launch: which of the eight instantiations (forced: forced_k is read, finite and > 0)
static int puct_step_round(const MnkPuctStepArgs& a, bool solver, bool with_fpu, int8_t* proof, float fpu, float fpu_root,
                           void* stream, const char* what, bool forced = false, float forced_k = 0.0f,
                           int32_t* raw_visits = nullptr) {
  if (with_fpu && (!(fpu >= 0.0f && fpu <= 3.0e38f) || !(fpu_root >= 0.0f && fpu_root <= 3.0e38f))) return MNK_EINVAL;
  if (forced && !(forced_k > 0.0f && forced_k <= 3.0e38f)) return MNK_EINVAL;
  if (a.N == 0) return MNK_OK;
#define MNK_PUCT_ROUND(SOLVER, FPU, FORCED)                                                                          \
  MNK_DISPATCH(a.g, puct_launch(k_puct_step_leaves<NW, CN, CK, SOLVER, FPU, FORCED>, a.N, stream, a, proof, fpu, fpu_root, \
                                forced_k, raw_visits))
  if (forced) {
    if (solver && with_fpu) MNK_PUCT_ROUND(true, true, true);
    else if (with_fpu) MNK_PUCT_ROUND(false, true, true);
    else if (solver) MNK_PUCT_ROUND(true, false, true);
    else MNK_PUCT_ROUND(false, false, true);
  } else if (solver && with_fpu) MNK_PUCT_ROUND(true, true, false);
  else if (with_fpu) MNK_PUCT_ROUND(false, true, false);
  else if (solver) MNK_PUCT_ROUND(true, false, false);
  else MNK_PUCT_ROUND(false, false, false);
#undef MNK_PUCT_ROUND
  return mnk_launch_status(what);
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
  MnkPuctStepArgs a;
  const int rc = puct_step_check(MNK_PUCT_STEP_COMMON(0, temperature), &a);
  if (rc != MNK_OK || N == 0) return rc;
  MNK_DISPATCH(a.g, puct_launch(MNK_K(k_puct_step), N, stream, a));
  return mnk_launch_status("puct_step");
}
int mnk_puct_step_leaves(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, void* stream) {
  MnkPuctStepArgs a;
  const int rc = leaves ? puct_step_check(MNK_PUCT_STEP_COMMON(leaves, temperature), &a) : MNK_EINVAL;
  return rc != MNK_OK ? rc : puct_step_round(a, false, false, nullptr, 0.0f, 0.0f, stream, "puct_step_leaves");
}
int mnk_puct_step_solver(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, int8_t* proof, void* stream) {
  MnkPuctStepArgs a;
  const int rc = leaves ? puct_step_check(MNK_PUCT_STEP_COMMON(leaves, temperature), &a) : MNK_EINVAL;
  return rc != MNK_OK ? rc : puct_step_round(a, true, false, proof, 0.0f, 0.0f, stream, "puct_step_solver");
}

int mnk_puct_step_fpu(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                      int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                      uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                      int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                      int32_t* visits, float* root_value, int8_t* proof, int solver, float fpu, float fpu_root,
                      void* stream) {
  MnkPuctStepArgs a;
  const int rc = leaves && (solver == 0 || solver == 1) ? puct_step_check(MNK_PUCT_STEP_COMMON(leaves, temperature), &a)
                                                        : MNK_EINVAL;
  if (rc != MNK_OK) return rc;
  return puct_step_round(a, solver != 0, true, solver ? proof : nullptr, fpu, fpu_root, stream, "puct_step_fpu");
}

int mnk_puct_step_forced(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, int8_t* proof, int solver, float fpu, float fpu_root,
                         int fpu_on, float forced_k, int32_t* raw_visits, void* stream) {
  MnkPuctStepArgs a;
  const int rc = leaves && (solver == 0 || solver == 1) && (fpu_on == 0 || fpu_on == 1)
                     ? puct_step_check(MNK_PUCT_STEP_COMMON(leaves, temperature), &a)
                     : MNK_EINVAL;
  if (rc != MNK_OK) return rc;
  return puct_step_round(a, solver != 0, fpu_on != 0, solver ? proof : nullptr, fpu, fpu_root, stream, "puct_step_forced",
                         true, forced_k, raw_visits);
}

int mnk_puct_step_gumbel(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int considered,
                         float c_visit, float c_scale, const uint16_t* table, const float* gscore, const float* vroot,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, float* policy, void* stream) {
  MnkPuctStepArgs a;
  const int rc = puct_step_check(MNK_PUCT_STEP_COMMON(leaves, 0), &a);  // (the Gumbel root has no temperature)
  if (rc != MNK_OK) return rc;
  if (leaves != 1 || considered < 1 || considered > MNK_PUCT_CONSIDERED_MAX || !(c_visit >= 0.0f && c_visit <= 3.0e38f) ||
      !(c_scale >= 0.0f && c_scale <= 3.0e38f) || !table || !gscore || (last && policy && !vroot))
    return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  MNK_DISPATCH(a.g, puct_launch(MNK_K(k_puct_step_gumbel), N, stream, a, considered, c_visit, c_scale, table, gscore, vroot,
                                policy));
  return mnk_launch_status("puct_step_gumbel");
}

}  // extern "C"
