// mnk_search_selfplay_async_leaves.hip -- search self-play with per-row search budgets and several leaves per evaluator
// call (gfx950 / MI355X only): mnk_search_selfplay_advance_opts (mnk_search_selfplay_async.hip) for rows that search with
// L slots per row and call -- the lockstep player's mnk_puct_step_leaves / mnk_puct_step_solver: L backups, then up to L
// selections under virtual visits -- with a ply's budget counted in the simulations it has been offered.  The rule:
// include/mnk_hip.h, mnk_search_selfplay_advance_leaves.
//
// What a row does in every advance kernel -- the budget draw, the root's noise and visit counts, the end of a ply, the
// error row -- and the host's common checks are mnk_search_selfplay_advance.h's; the row's view, its slots and a slot's
// write-out are mnk_puct_tree.h's; the slot loops, row_sims and the virtual visits are this kernel's own.  A translation
// unit of its own all the same: every function here is inlined, but the module's passes see sibling call sites, and
// compiled beside its siblings the kernel changes the code the compiler makes of them
// (profiles/exp_search_selfplay_async_leaves_kernels.md).
#include "mnk_search_selfplay_advance.h"

// The backup loop and the selection loop of the lockstep player's round (puct_step_row, mnk_puct.hip) around the shared
// end of a ply.  The siblings' shape: one wave per row, MNK_PUCT_ROWS rows per workgroup, no workgroup barrier, every id
// read from the workspace clamped to the row.  Slot j of row i is batch row i * leaves + j; the slots' paths stay in the
// workspace.  Whether the ply ends is decided by row_sims, the simulations the ply has been offered, not by the root's
// visits: a slot that the walk makes void is a simulation spent.  The three branches after the backups -- the ply ends, an
// error row, the selections -- are disjoint and wave-uniform, so the one MnkEnv serves the ply and the walks.
// nz.alpha = 0: no noise, and then the launch has no dynamic LDS.
template <int NW, int CN, int CK, bool SOLVER>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_leaves(MnkAdvanceArgs a, int leaves, MnkPuctNoise nz, float noise_eps, int noise_fast,
                                 float* root_priors, uint32_t* row_sims) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  extern __shared__ double lds_gamma[];  // with noise: [MNK_PUCT_ROWS][C], a root's log-gammas between the two passes
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= a.N) return;
  const int C = a.g.C, NWg = a.g.NW, I = a.I;
  const MnkPuctRow r = puct_row(a.ws, i, NWg, C, I, leaves);
  const MnkPuctHeader h = puct_header(r.hdr, I);  // (nodes and live; depth and state are a slot's)
  int nodes = h.nodes;
  uint32_t* pos = lds_pos[wave];

  // ---- the budget of the row's ply (before the backups: whether a root is noised depends on it)
  const MnkAdvanceBudget bg = advance_budget(a, i);
  const uint32_t sims = row_sims[i];
  const uint32_t budget = (uint32_t)(bg.full ? I : a.I_fast);

  // ---- the backups of the pending evaluations, in slot order
  for (int j = 0; j < leaves && h.live; ++j) {
    const uint32_t* ds = puct_slot_ds(r, j);
    const int depth = (int)min(ds[0], (uint32_t)I);
    const uint32_t state = ds[1];
    if (!(state & 1u)) continue;
    puct_stage_planes<NW>(pos, puct_slot_leaf(r, j, NWg), NWg, lane);
    row_wave_sync();
    puct_backup<NW, CN, SOLVER>(a.g, pos, puct_slot_path(r, j), r.node, r.prior, r.child, nodes, depth, state, a.priors,
                                a.priors_dtype, a.values, a.values_dtype, i * leaves + j, lane);
    // evaluation 0 (pending in slot 0) is batch row i * leaves.  The sync is this kernel's: the next slot's planes
    // overwrite the stage the noise reads
    if (j == 0 && state == 1u && depth == 0 && (nz.alpha > 0.0 || root_priors)) {
      advance_root_noise<NW, CN>(a, bg, true, pos, r.prior, i, i * leaves, nz, noise_eps, noise_fast, root_priors,
                                 lds_gamma + wave * C, lane);
      row_wave_sync();
    }
  }

  // ---- whether the ply ends: it has been offered its budget, or (SOLVER) the root has a proof
  bool spent = sims >= budget;
  if constexpr (SOLVER) spent |= r.node[0].n != 0u && MNK_PUCT_PROOF(r.node[0].info) != 0u;

  uint32_t maxn = 0u, tot = 0u;
  MnkAdvanceVisits<NW, CN, SOLVER> visits_of{a.g, pos, r.node, r.child, nodes, 0};
  MnkEnv<NW> e;
  if (__builtin_amdgcn_readfirstlane((int)(h.live && spent))) {
    // the position before the ply: in registers, and canonical (plane 0 = the side to move) in LDS
    env_load<NW>(e, a.planes, a.meta, a.N, a.g.W, i);
    row_wave_sync();  // (every lane is done with the last leaf's planes)
    stage_env<NW>(pos, e, lane);
    row_wave_sync();
    advance_root_visits(visits_of, lane, maxn, tot);
  }

  if (maxn) {
    // ---- the ply ends in this launch: ring row t = p mod T, the move, the outcome labels, the reset
    const int64_t t = (int64_t)(bg.p % (uint64_t)a.T);
    const uint32_t x = mnk_rand_u32(bg.seed, (uint64_t)(a.env_id0 + i), bg.p, MNK_STREAM_SELFPLAY);
    uint16_t* rv = a.ring_visits + (t * a.N + i) * C;
    for (int q = lane; q < C; q += 64) rv[q] = bg.full ? (uint16_t)visits_of(q) : (uint16_t)0;  // a fast ply: no policy target
    int move = 0;
    mnk_pick_by_visits(C, x, (int64_t)(e.meta >> 1) < (int64_t)a.temp_plies, maxn, tot, lane, visits_of, move);
    advance_finish_ply<NW, CN, CK>(a, e, pos, move, bg.p, t, i, lane);
    if (lane == 0) row_sims[i] = 0u;
    // ---- the search of the position reached: a fresh tree (no proof) as mnk_puct_begin_leaves leaves it -- slot 0 the
    // root, pending; the other slots void, showing it
    advance_fresh_root<NW, CN>(a, r, pos, e, i * leaves, lane);
    puct_row_void_slots<NW, CN>(a.g, r.row, r.L, pos, i, leaves, a.leaf_obs, a.leaf_dtype, a.leaf_mask, lane);
    return;
  }

  if (!h.live || spent) {
    advance_error_row<NW, CN>(a, r, pos, i, i * leaves, leaves, lane);  // (every batch row of the row; row_sims stays)
    return;
  }

  // ---- the selections: puct_step_row's with VL (the root has no proof here), slots 0 .. s - 1;
  // the slots from s on are void, so that the ply is offered its budget exactly
  const int s = (int)min((uint32_t)leaves, budget - sims);
  const int nodes0 = nodes;
  const uint16_t* epath = puct_slot_path(r, min(lane, leaves - 1));  // lane l < leaves: slot l's path
  int edepth = 0;                                            // and, once it has selected, its leaf's depth
  uint32_t active = 0u;                                      // the slots of this round that have a leaf
  bool open = true;                                          // no slot was void yet
  for (int j = 0; j < leaves; ++j) {
    int d = 0;
    uint32_t nstate = 0u;
    uint16_t* path = puct_slot_path(r, j);
    if (open && j < s && nodes <= I) {
      puct_env_root<NW>(e, r.root, NWg);
      nstate = puct_walk<NW, CN, CK, true, SOLVER>(a.g, e, I, a.c, r.node, r.prior, r.child, path, nodes, d, lane, nodes0,
                                                   active, epath, edepth);
    }
    if (nstate) {
      active |= 1u << j;
      if (lane == j) edepth = d;
    } else {
      d = 0;
      open = false;
    }
    if (nstate) puct_stage_selection<NW>(pos, e, nstate, r.root, NWg, lane);
    else puct_stage_planes<NW>(pos, r.root, NWg, lane);  // (a void slot shows the root)
    puct_store_selection<NW, CN>(a.g, pos, nstate, d, path, puct_slot_ds(r, j), puct_slot_leaf(r, j, NWg), i * leaves + j,
                                 a.leaf_obs, a.leaf_dtype, a.leaf_mask, lane);
    row_wave_sync();  // (the next slot's walk reads this one's node, child entry and path; its write-out reuses pos)
  }
  if (lane == 0) {
    r.hdr[0] = (uint32_t)nodes;
    if (a.fresh) a.fresh[i] = 0;
    // no leaf at all: nothing is pending, so the row would show its root for ever (a full tree: it cannot happen in a
    // workspace that mnk_puct_begin_leaves set up): reported, not silent, and the counter stays
    if (active == 0u) mnk_report(a.err, MNK_ERR_VISITS, i);
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
  MnkAdvanceArgs a;
  const int rc = mnk_advance_check(MNK_ADVANCE_COMMON(temp_plies), &a);
  if (rc != MNK_OK) return rc;
  if (mnk_advance_options_check(a.g, solver, noise_alpha, noise_eps, noise_fast) != MNK_OK) return MNK_EINVAL;
  // (the workspace's condition: mnk_puct_begin_leaves takes no other pair)
  if (leaves < 1 || leaves > MNK_PUCT_LEAVES_MAX || iterations % leaves != 0 || !row_sims) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const MnkPuctNoise nz = mnk_advance_noise(noise_alpha);
  const size_t lds = mnk_advance_noise_lds(a.g, noise_alpha);
#define MNK_ADVANCE_LEAVES(SOLVER)                                                                                     \
  MNK_DISPATCH(a.g, mnk_advance_launch(k_search_selfplay_advance_leaves<NW, CN, CK, SOLVER>, a, lds, stream, leaves, nz, \
                                       noise_eps, noise_fast, root_priors, row_sims))
  if (solver) MNK_ADVANCE_LEAVES(true);
  else MNK_ADVANCE_LEAVES(false);
#undef MNK_ADVANCE_LEAVES
  return mnk_launch_status("search_selfplay_advance_leaves");
}

}  // extern "C"
