// mnk_search_selfplay_async_gumbel.hip -- search self-play with per-row search budgets and a Gumbel root (gfx950 / MI355X
// only): mnk_search_selfplay_advance (mnk_search_selfplay_async.hip) for rows whose root is the lockstep player's Gumbel
// root -- mnk_puct_gumbel_root's draw at the backup of a fresh tree's root, mnk_puct_step_gumbel's selection with the
// schedule table of the ply's budget, its move and its improved policy at the end of the ply -- all inside the one launch.
// The rule: include/mnk_hip.h, mnk_search_selfplay_advance_gumbel.
//
// What a row does in every advance kernel -- the budget draw, the end of a ply, the error row -- and the host's common
// check are mnk_search_selfplay_advance.h's; the row's view, the selection's write-out, the root's pick and the improved
// policy (puct_gumbel_policy, the one the lockstep player's move calls) are mnk_puct_tree.h's; the root's draw and the
// policy's quantisation are this kernel's own.  So are, for the registers of one variant (15x15: 127 VGPRs, four waves
// per SIMD), its parameter list -- the kernel puts the argument block together itself -- and the start of the next search
// (profiles/exp_search_selfplay_advance_pieces_kernels.md).  A translation unit of its own all the same: compiled beside its
// siblings a kernel changes the code the compiler makes of them (profiles/exp_search_selfplay_async_leaves_kernels.md).
//
// Floating point: the draw and the policy are f64 with the full-precision log and exp of the device library; the
// roundings to f32 are the ones the rule names.  The library is built with -ffp-contract=off and without any fast-math
// option, and nothing here may change that for this file.  There is no f32 transcendental in this translation unit.
#include "mnk_search_selfplay_advance.h"

#define MNK_ADVANCE_GUMBEL_CELLS_MAX 1024  // 64 * MNK_MAX_W: no supported board has more cells than a plane has bits
static_assert(MNK_ADVANCE_GUMBEL_CELLS_MAX == 64 * MNK_MAX_W, "the cell range follows the packed planes");

// k_search_selfplay_advance with the Gumbel root.  The same shape: one wave per row, MNK_PUCT_ROWS rows per workgroup, no
// workgroup barrier (which branch a row takes is wave-uniform; the rows of a workgroup diverge), every id read from the
// workspace clamped to the row.  B, the budget of the row's ply, is also the row stride of the ply's schedule table, so it
// is what the walk and the root's pick are given as their iteration count: the pick's read stays inside the table of B
// columns, and the walk's depth guard (d >= B) is as unreachable as it is with I -- an existing node lies at depth <= it < B.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_gumbel(MnkGeom g, unsigned char* ws, uint64_t* planes, uint32_t* meta, int64_t N, int iterations,
                                 int I_fast, uint64_t full_threshold, const void* priors, int priors_dtype,
                                 const void* values, int values_dtype, float c, uint64_t seed, const uint64_t* seed_dev,
                                 int64_t env_id0, unsigned long long* row_plies, int64_t T, uint64_t* ring_planes,
                                 uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask,
                                 uint8_t* fresh, unsigned long long* plies_max, unsigned long long* stats, int32_t* err,
                                 int considered, float c_visit, float c_scale, double gscale, const uint16_t* table_full,
                                 const uint16_t* table_fast, float* gscore, float* vroot) {
  // (the block put together here, for the shared pieces: as the kernel's argument it costs the 15x15 variant a wave)
  const MnkAdvanceArgs a{g, ws, planes, meta, N, iterations, I_fast, full_threshold, priors, priors_dtype, values,
                         values_dtype, c, 0, seed, seed_dev, env_id0, row_plies, T, ring_planes, ring_visits, ring_z,
                         leaf_obs, leaf_dtype, leaf_mask, fresh, plies_max, stats, err};
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= a.N) return;
  const int C = a.g.C, NWg = a.g.NW, I = a.I;
  const MnkPuctRow r = puct_row(a.ws, i, NWg, C, I);
  const MnkPuctHeader h = puct_header(r.hdr, I);
  int nodes = h.nodes;
  uint32_t* pos = lds_pos[wave];
  puct_stage_planes<NW>(pos, r.leaf, NWg, lane);
  row_wave_sync();

  // ---- the budget of the row's ply: B, and the schedule table that goes with it
  const MnkAdvanceBudget bg = advance_budget(a, i);
  const int B = bg.full ? I : a.I_fast;
  const MnkPuctGumbel gm{gscore + i * C, bg.full ? table_full : table_fast, considered, c_visit, c_scale};

  // ---- backup of the pending evaluation
  if (h.live && (h.state & 1u))
    puct_backup<NW, CN>(a.g, pos, r.path, r.node, r.prior, r.child, nodes, h.depth, h.state, a.priors, a.priors_dtype,
                        a.values, a.values_dtype, i, lane);
  // evaluation 0 (what puct_row_fresh and mnk_puct_begin leave pending): the root's Gumbel scores and its value, by
  // k_puct_gumbel_root's text with step = the row's ply and the free cells those of the root's planes (pos: at depth 0 the
  // leaf is the root).  A cell's gscore is written here and read, in the selections and at the end of the ply, by the same
  // lane -- cells are strided over the lanes the same way in every loop -- so no synchronisation is needed, as with the
  // noised priors of k_search_selfplay_advance_opts.  vroot[i] is lane 0's store; it is read when the ply ends, which is
  // never this launch (n_root = 1 here and B >= 1).
  if (h.live && h.state == 1u && h.depth == 0) {
    const int64_t base = i * C;
    const uint64_t env = (uint64_t)(a.env_id0 + i);
    const uint64_t s_row = bg.p * (uint64_t)((C + 3) & ~3);  // word q of the row: block s_row / 4 + (q >> 2), word q & 3
    for (int q = lane; q < C; q += 64) {
      float gs = -INFINITY;
      if (!(row_stone<CN>(a.g, pos, q) || row_stone<CN>(a.g, pos + NW, q))) {
        const float pa = puct_read(a.priors, a.priors_dtype, base + q);
        const double l = log((double)(pa > 0x1p-126f ? pa : 0x1p-126f));
        const double uu = ((double)mnk_rand_u32(bg.seed, env, s_row + (uint64_t)q, MNK_STREAM_GUMBEL) + 0.5) * 0x1p-32;
        const double gv = -log(-log(uu));  // (uu is never 0 or 1: gv is finite)
        gs = (float)(gscale * gv + l);
      }
      gscore[base + q] = gs;
    }
    if (lane == 0) vroot[i] = puct_read(a.values, a.values_dtype, i);
  }

  // ---- whether the ply ends, and then its move: mnk_puct_step_gumbel's, which must be a free cell of the env's position
  const uint32_t n_root = r.node[0].n;
  const bool spent = n_root != 0u && n_root - 1u >= (uint32_t)B;
  MnkEnv<NW> e;
  int move = 0x7fffffff;
  uint32_t maxn = 0u;
  bool playable = false;
  if (__builtin_amdgcn_readfirstlane((int)(h.live && spent))) {
    // the position before the ply: in registers, and canonical (plane 0 = the side to move) in LDS
    env_load<NW>(e, a.planes, a.meta, a.N, a.g.W, i);
    row_wave_sync();  // (every lane is done with the leaf's planes)
    stage_env<NW>(pos, e, lane);
    row_wave_sync();
    move = puct_gumbel_pick<true>(C, B, r.node, r.child, nodes, gm, lane, &maxn);  // (wave-uniform; 0x7fffffff: no free cell)
    playable = move >= 0 && move < C && !(row_stone<CN>(a.g, pos, move) || row_stone<CN>(a.g, pos + NW, move));
  }

  if (playable) {
    // ---- the ply ends in this launch: ring row t = p mod T, the improved policy, the outcome labels, the reset
    const int64_t t = (int64_t)(bg.p % (uint64_t)a.T);
    uint16_t* rv = a.ring_visits + (t * a.N + i) * C;
    if (bg.full) {
      // k_search_selfplay_step_moves's quantisation of the improved policy, a cell at a time
      puct_gumbel_policy(C, r.node, r.prior, r.child, nodes, gm, vroot[i], maxn, lane, [&](int q, float pa) {
        const bool occ = row_stone<CN>(a.g, pos, q) || row_stone<CN>(a.g, pos + NW, q);
        const float v = rintf(__fmul_rn(pa, 65535.0f));
        rv[q] = (occ || !(v > 0.0f)) ? (uint16_t)0 : (uint16_t)fminf(v, 65535.0f);
      });
    } else {
      for (int q = lane; q < C; q += 64) rv[q] = (uint16_t)0;  // a fast ply: no policy target
    }
    advance_finish_ply<NW, CN, CK>(a, e, pos, move, bg.p, t, i, lane);
    // ---- the search of the position reached: a fresh tree, its root the pending leaf (advance_fresh_root's steps in
    // this kernel's own text: through the piece, or stage_env here, the 15x15 variant takes 129-130 VGPRs and loses a wave)
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
    puct_row_fresh<NW>(r.row, r.L, pos, NWg, (int)(e.meta >> 1) < C, lane);
    row_write_view<NW, CN>(a.g, pos, 0, i, a.leaf_obs, a.leaf_dtype, a.leaf_mask, lane);
    return;
  }

  if (!h.live || spent) {
    advance_error_row<NW, CN>(a, r, pos, i, i, 1, lane);
    return;
  }

  // ---- selection: k_puct_step_gumbel's (the root's cell by puct_gumbel_pick with the table of B columns)
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a full tree shows its root again (it cannot happen: nodes <= n_root <= B)
  if (nodes <= I) {
    puct_env_root<NW>(e, r.root, NWg);
    // (B, not I, is the walk's iteration count: the schedule table's row stride)
    nstate = puct_walk<NW, CN, CK, false, false, true>(a.g, e, B, a.c, r.node, r.prior, r.child, r.path, nodes, d, lane, 0,
                                                       0u, nullptr, 0, &gm);
    if (nstate == 0u) d = 0;
    puct_stage_selection<NW>(pos, e, nstate, r.root, NWg, lane);
  } else {
    puct_stage_planes<NW>(pos, r.root, NWg, lane);  // (a full tree: no walk, the root again)
  }
  puct_store_selection<NW, CN>(a.g, pos, nstate, d, r.path, r.hdr + 1, r.leaf, i, a.leaf_obs, a.leaf_dtype,
                               a.leaf_mask, lane);
  if (lane == 0) {
    r.hdr[0] = (uint32_t)nodes;
    if (a.fresh) a.fresh[i] = 0;
    // no leaf: nothing is pending and the row would show its root for ever (it cannot happen, as above): reported
    if (nstate == 0u) mnk_report(a.err, MNK_ERR_VISITS, i);
  }
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
  MnkAdvanceArgs a;
  const int rc = mnk_advance_check(MNK_ADVANCE_COMMON(0), &a);  // (the Gumbel root has no temperature)
  if (rc != MNK_OK) return rc;
  if (considered < 1 || considered > MNK_PUCT_CONSIDERED_MAX || !(c_visit >= 0.0f && c_visit <= 3.0e38f) ||
      !(c_scale >= 0.0f && c_scale <= 3.0e38f) || !(gumbel_scale >= 0.0f && gumbel_scale <= 3.0e38f) || !table_full ||
      !table_fast || !gscore || !vroot || a.g.C > MNK_ADVANCE_GUMBEL_CELLS_MAX)
    return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  MNK_DISPATCH(a.g, hipLaunchKernelGGL(MNK_K(k_search_selfplay_advance_gumbel), grid, block, 0, (hipStream_t)stream, a.g, a.ws,
                                       planes, meta, N, iterations, fast_iterations, full_threshold, priors, priors_dtype,
                                       values, values_dtype, c, seed, seed_dev, env_id0, a.row_plies, T, ring_planes,
                                       ring_visits, ring_z, leaf_obs, leaf_dtype, leaf_mask, fresh, a.plies_max, a.stats, err,
                                       considered, c_visit, c_scale, (double)gumbel_scale, table_full, table_fast, gscore,
                                       vroot));
  return mnk_launch_status("search_selfplay_advance_gumbel");
}

}  // extern "C"
