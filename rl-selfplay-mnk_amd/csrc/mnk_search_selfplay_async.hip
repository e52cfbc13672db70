// mnk_search_selfplay_async.hip -- search self-play with per-row search budgets (gfx950 / MI355X only): ONE launch per
// evaluator call.  Row i backs up its pending evaluation (mnk_puct_step's backup), and then either selects its next leaf
// (mnk_puct_step's selection) or, when the budget of its current ply is spent, plays the ply in the same launch
// (mnk_search_selfplay_step's rule with the row's own ply count in the place of the global one) and starts the search of
// the position it reached.  Rows finish their searches at different times and go on at once; the budget of a ply is a
// function of (seed, row id, the row's ply) alone, so nothing but the tree and the ply count is kept.  The rule:
// include/mnk_hip.h, mnk_search_selfplay_advance.
//
// Three kernels live here: the plain launch; mnk_search_selfplay_advance_opts, the launch with two of the lockstep
// player's options built in -- Dirichlet noise on the roots (mnk_puct_root_noise's draw, at the backup of a fresh tree's
// root) and the solver (mnk_puct_step_solver's backup and selection; a ply ends as soon as its root is proven), and behind
// template flags first-play urgency and forced playouts with policy target pruning (mnk_puct_step_forced's); and
// mnk_search_selfplay_advance_keep, the launch with the options for rows that keep the played move's subtree from ply to
// ply (the lockstep player's mnk_puct_rebase, inside the launch that plays the ply).  The steps they share with each other
// and with the leaves and Gumbel kernels -- the row's prologue, the budget draw, the root's noise and visit counts, the end
// of a ply, the error row, the selection's write-out -- and the host's common check are mnk_search_selfplay_advance.h's;
// a body below spells out only what is its own.
#include "mnk_search_selfplay_advance.h"

// One wave per row, MNK_PUCT_ROWS rows per workgroup.  Which branch a row takes is wave-uniform; the rows of a workgroup
// diverge, so the kernel has no workgroup barrier: a row's LDS stage and its workspace are its own wave's alone.
// Its own: the budget is drawn after the backup.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256) k_search_selfplay_advance(MnkAdvanceArgs a) {
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

  // ---- backup of the pending evaluation
  if (h.live && (h.state & 1u))
    puct_backup<NW, CN>(a.g, pos, r.path, r.node, r.prior, r.child, nodes, h.depth, h.state, a.priors, a.priors_dtype,
                        a.values, a.values_dtype, i, lane);

  // ---- the budget of the row's ply, and whether it is spent
  const MnkAdvanceBudget bg = advance_budget(a, i);
  const uint32_t n_root = r.node[0].n;
  const bool spent = n_root != 0u && n_root - 1u >= (uint32_t)(bg.full ? I : a.I_fast);

  uint32_t maxn = 0u, tot = 0u;
  MnkAdvanceVisits<NW, CN, false> visits_of{a.g, pos, r.node, r.child, nodes, 0};
  MnkEnv<NW> e;
  if (__builtin_amdgcn_readfirstlane((int)(h.live && spent))) {
    // the position before the ply: in registers, and canonical (plane 0 = the side to move) in LDS
    env_load<NW>(e, a.planes, a.meta, a.N, a.g.W, i);
    row_wave_sync();  // (every lane is done with the leaf's planes)
    stage_env<NW>(pos, e, lane);
    row_wave_sync();
    advance_root_visits(visits_of, lane, maxn, tot);  // (the plain form: no puct_root_keep, maxn and tot were 0 already)
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
    // ---- the search of the position reached: a fresh tree, its root the pending leaf
    advance_fresh_root<NW, CN>(a, r, pos, e, i, lane);
    return;
  }

  if (!h.live || spent) {
    advance_error_row<NW, CN>(a, r, pos, i, i, 1, lane);
    return;
  }

  // ---- selection: k_puct_step's
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a full tree shows its root again (it cannot happen: nodes <= n_root <= I)
  if (nodes <= I) {
    puct_env_root<NW>(e, r.root, NWg);
    nstate = puct_walk<NW, CN, CK, false>(a.g, e, I, a.c, r.node, r.prior, r.child, r.path, nodes, d, lane);
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
    // no leaf: nothing is pending, so n_root cannot advance and the row would show its root for ever.  It cannot happen
    // in a workspace that mnk_puct_begin set up (nodes <= n_root <= I while the budget is unspent): reported, not silent
    if (nstate == 0u) mnk_report(a.err, MNK_ERR_VISITS, i);
  }
}

// k_search_selfplay_advance with the options (the rule: include/mnk_hip.h, mnk_search_selfplay_advance_opts).  The same
// shape: one wave per row, no workgroup barrier, every id clamped to the row.  SOLVER is a template flag (it changes
// puct_walk's inner loop), and so is FPU, first-play urgency (puct_walk's, the rule: include/mnk_hip.h,
// mnk_puct_step_fpu; fpu and fpu_root are read by the FPU form alone); the noise is a wave-uniform run-time branch that
// only a wave whose pending leaf is the root of a fresh tree takes, once per ply.  nz.alpha = 0: no noise, and then the
// launch has no dynamic LDS.  FORCED: forced playouts and policy target pruning (the rule: include/mnk_hip.h,
// mnk_puct_step_forced) on the plies the noise applies to -- `force`, wave-uniform: the ply is full, or noise_fast is set
// -- in puct_walk's per-cell loop and, where the ply is played, over the counts the move is drawn from and the ring records
// (puct_prune_root, puct_pruned_count); forced_k is read by the FORCED form alone.
template <int NW, int CN, int CK, bool SOLVER, bool FPU, bool FORCED = false>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_opts(MnkAdvanceArgs a, MnkPuctNoise nz, float noise_eps, int noise_fast, float* root_priors,
                               float fpu, float fpu_root, float forced_k) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  extern __shared__ double lds_gamma[];  // with noise: [MNK_PUCT_ROWS][C], a root's log-gammas between the two passes
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

  // ---- the budget of the row's ply (before the backup: whether a root is noised depends on it)
  const MnkAdvanceBudget bg = advance_budget(a, i);

  // ---- backup of the pending evaluation, and the noise of a fresh tree's root
  if (h.live && (h.state & 1u))
    puct_backup<NW, CN, SOLVER>(a.g, pos, r.path, r.node, r.prior, r.child, nodes, h.depth, h.state, a.priors,
                                a.priors_dtype, a.values, a.values_dtype, i, lane);
  advance_root_noise<NW, CN>(a, bg, h.live && h.state == 1u && h.depth == 0, pos, r.prior, i, i, nz, noise_eps, noise_fast,
                             root_priors, lds_gamma + wave * C, lane);

  // ---- whether the ply ends: the budget is spent, or (SOLVER) the root has a proof
  const uint32_t n_root = r.node[0].n;
  bool spent = n_root != 0u && n_root - 1u >= (uint32_t)(bg.full ? I : a.I_fast);
  if constexpr (SOLVER) spent |= n_root != 0u && MNK_PUCT_PROOF(r.node[0].info) != 0u;

  uint32_t maxn = 0u, tot = 0u;
  MnkAdvanceVisits<NW, CN, SOLVER> visits_of{a.g, pos, r.node, r.child, nodes, 0};
  MnkEnv<NW> e;
  if (__builtin_amdgcn_readfirstlane((int)(h.live && spent))) {
    // the position before the ply: in registers, and canonical (plane 0 = the side to move) in LDS
    env_load<NW>(e, a.planes, a.meta, a.N, a.g.W, i);
    row_wave_sync();  // (every lane is done with the leaf's planes)
    stage_env<NW>(pos, e, lane);
    row_wave_sync();
    advance_root_visits(visits_of, lane, maxn, tot);
  }

  if (maxn) {
    // ---- the ply ends in this launch: ring row t = p mod T, the move, the outcome labels, the reset
    const int64_t t = (int64_t)(bg.p % (uint64_t)a.T);
    const uint32_t x = mnk_rand_u32(bg.seed, (uint64_t)(a.env_id0 + i), bg.p, MNK_STREAM_SELFPLAY);
    uint16_t* rv = a.ring_visits + (t * a.N + i) * C;
    int move = 0;
    if constexpr (FORCED) {
      // the pruned counts n'' in the place of n' = visits_of, on a ply that forces (else pp.on is false: n'' = n'); a
      // cell's n'' is computed again wherever it is read -- the store, the sum, the pick -- from the same inputs
      MnkPuctPrune pp;
      pp.on = false;
      if (bg.full || noise_fast) {
        pp = puct_prune_root(C, forced_k, a.c, r.node, r.prior, r.child, nodes, true, visits_of, lane);
        if (visits_of.keep == 1) pp.on = false;  // (the solver keeps the WIN children alone: nothing is pruned)
      }
      auto pruned = [&](int q) {
        return puct_pruned_count(pp, q, visits_of(q), puct_root_kid(C, r.node, r.child, nodes, true, q),
                                 q < C ? r.prior[q] : 0.0f);
      };
      tot = 0u;  // (the maximum is c*'s count, which is kept)
      for (int q = lane; q < C; q += 64) {
        const uint32_t na = pruned(q);
        rv[q] = bg.full ? (uint16_t)na : (uint16_t)0;  // a fast ply: no policy target
        tot += na;
      }
#pragma unroll
      for (int off = 32; off; off >>= 1) tot += (uint32_t)__shfl_xor((int)tot, off, 64);
      mnk_pick_by_visits(C, x, (int64_t)(e.meta >> 1) < (int64_t)a.temp_plies, maxn, tot, lane, pruned, move);
    } else {
      for (int q = lane; q < C; q += 64) rv[q] = bg.full ? (uint16_t)visits_of(q) : (uint16_t)0;  // a fast ply: no policy target
      mnk_pick_by_visits(C, x, (int64_t)(e.meta >> 1) < (int64_t)a.temp_plies, maxn, tot, lane, visits_of, move);
    }
    advance_finish_ply<NW, CN, CK>(a, e, pos, move, bg.p, t, i, lane);
    // ---- the search of the position reached: a fresh tree (no proof), its root the pending leaf
    advance_fresh_root<NW, CN>(a, r, pos, e, i, lane);
    return;
  }

  if (!h.live || spent) {
    advance_error_row<NW, CN>(a, r, pos, i, i, 1, lane);
    return;
  }

  // ---- selection: k_puct_step's (SOLVER: k_puct_step_leaves<true>'s at one leaf per row; the root has no proof here)
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a full tree shows its root again (it cannot happen: nodes <= n_root <= I)
  if (nodes <= I) {
    puct_env_root<NW>(e, r.root, NWg);
    nstate = puct_walk<NW, CN, CK, false, SOLVER, false, FPU, FORCED>(a.g, e, I, a.c, r.node, r.prior, r.child, r.path,
                                                                      nodes, d, lane, 0, 0u, nullptr, 0, nullptr, fpu,
                                                                      fpu_root, forced_k, bg.full || noise_fast);
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
    // no leaf: nothing is pending, so n_root cannot advance and the row would show its root for ever: reported, not silent
    if (nstate == 0u) mnk_report(a.err, MNK_ERR_VISITS, i);
  }
}

// k_search_selfplay_advance_opts for rows that keep the played move's subtree (the rule: include/mnk_hip.h,
// mnk_search_selfplay_advance_keep).  The same shape: one wave per row, no workgroup barrier, every id clamped to the row
// -- by TI = tree_iterations, the workspace's layout parameter; a.I stays the full budget.  Its own: the iterations of a
// ply are counted above the visits the root was carried with; the end of a ply calls puct_carry_subtree (mnk_puct_tree.h)
// on the root's child through the move, the position reached still in the wave's LDS stage; a carried root keeps its
// proof.  Dynamic LDS: with noise [MNK_PUCT_ROWS][C] doubles, then the carry's two maps, [MNK_PUCT_ROWS][2][MS] u16 with
// MS = TI + 2 rounded up to even; the host sizes it (mnk_search_selfplay_advance_keep).
#ifndef MNK_KEEP_CARRY_B
#define MNK_KEEP_CARRY_B 8  // nodes in flight in the carry's copy loop (an experiment's knob: DESIGN section 5, row 34)
#endif
template <int NW, int CN, int CK, bool SOLVER, bool FPU>
__global__ void __launch_bounds__(256)
k_search_selfplay_advance_keep(MnkAdvanceArgs a, MnkPuctNoise nz, float noise_eps, int noise_fast, float* root_priors,
                               int TI, int keep_nodes, int32_t* carried, float fpu, float fpu_root) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  extern __shared__ double lds_gamma[];  // with noise: [MNK_PUCT_ROWS][C], a root's log-gammas between the two passes;
                                         // behind them (or first) the carry's maps
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= a.N) return;
  const int C = a.g.C, NWg = a.g.NW, I = a.I;
  const MnkPuctRow r = puct_row(a.ws, i, NWg, C, TI);  // (the layout and the clamps are TI's)
  const MnkPuctHeader h = puct_header(r.hdr, TI);
  int nodes = h.nodes;
  uint32_t* pos = lds_pos[wave];
  const int MS = (TI + 3) & ~1;
  uint16_t* map = (uint16_t*)(lds_gamma + (nz.alpha > 0.0 ? MNK_PUCT_ROWS * C : 0)) + (int64_t)wave * 2 * MS;
  uint16_t* inv = map + MS;
  puct_stage_planes<NW>(pos, r.leaf, NWg, lane);
  row_wave_sync();

  // ---- the budget of the row's ply (before the backup: whether a root is noised depends on it)
  const MnkAdvanceBudget bg = advance_budget(a, i);

  // ---- backup of the pending evaluation, and the noise of a root's first evaluation
  if (h.live && (h.state & 1u))
    puct_backup<NW, CN, SOLVER>(a.g, pos, r.path, r.node, r.prior, r.child, nodes, h.depth, h.state, a.priors,
                                a.priors_dtype, a.values, a.values_dtype, i, lane);
  // (evaluation 0 with bit 3, "renew", masked: a carried root's renewal is noised like a fresh root's evaluation)
  advance_root_noise<NW, CN>(a, bg, h.live && (h.state & ~8u) == 1u && h.depth == 0, pos, r.prior, i, i, nz, noise_eps,
                             noise_fast, root_priors, lds_gamma + wave * C, lane);

  // ---- whether the ply ends: the budget is spent, or (SOLVER) the root has a proof
  // it = the iterations of this ply: the root's visits above those it was carried with (saturating)
  const uint32_t n_root = r.node[0].n;
  const uint32_t n0 = (uint32_t)max(carried[2 * i + 1], 1);
  bool spent = n_root != 0u && (n_root > n0 ? n_root - n0 : 0u) >= (uint32_t)(bg.full ? I : a.I_fast);
  if constexpr (SOLVER) spent |= n_root != 0u && MNK_PUCT_PROOF(r.node[0].info) != 0u;

  uint32_t maxn = 0u, tot = 0u;
  MnkAdvanceVisits<NW, CN, SOLVER> visits_of{a.g, pos, r.node, r.child, nodes, 0};
  MnkEnv<NW> e;
  if (__builtin_amdgcn_readfirstlane((int)(h.live && spent))) {
    // the position before the ply: in registers, and canonical (plane 0 = the side to move) in LDS
    env_load<NW>(e, a.planes, a.meta, a.N, a.g.W, i);
    row_wave_sync();  // (every lane is done with the leaf's planes)
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
    const MnkPly ply = advance_finish_ply<NW, CN, CK>(a, e, pos, move, bg.p, t, i, lane);
    // ---- the search of the position reached: on the subtree of the move when there is one, else a fresh tree
    // (before pos changes: the root's child through the move; a game that ended keeps nothing)
    const uint32_t mch = r.child[move];
    int v = 0;
    [[maybe_unused]] uint32_t vproof = 0u;
    if (!ply.done && mch != 0u && mch != MNK_PUCT_NONE) {
      v = min((int)mch, nodes - 1);
      const uint32_t vinfo = r.node[v].info;
      if (MNK_PUCT_TERM(vinfo)) v = 0;
      vproof = MNK_PUCT_PROOF(vinfo);
    }
    // (this kernel's own text for advance_fresh_root's steps: the position is staged once, ahead of the choice -- staged
    // inside either branch the unrolled stores stand twice, 3 to 4 % more instructions in every variant)
    row_wave_sync();  // (every lane is done with the position before this ply)
    stage_env<NW>(pos, e, lane);
    row_wave_sync();
    if (v > 0) {
      const int kept = puct_carry_subtree<NW, MNK_KEEP_CARRY_B>(C, NWg, r.row, r.L, pos, nodes, v, keep_nodes, i, carried, map,
                                                                inv, lane);
      // SOLVER: the new root keeps the proof it had as a child, so that it plays in the launch that renews it -- when the
      // children that were kept still justify it (the truncation keeps the oldest nodes: the child that proved the root
      // may be gone): a root proven won for its side to move (3) needs a kept WIN child, a drawn one (2) a kept DRAW
      // child, a lost one (1) any kept child (kept > 1: node 1's parent can only be the root).  One scan of the root's
      // child row in the backup's access shape.
      if constexpr (SOLVER) {
        if (vproof && kept > 1) {
          row_wave_sync();  // (the carry's stores of the child row and the node records)
          bool win = false, draw = false;
          for (int q = lane; q < C; q += 64) {
            const uint32_t ch = r.child[q];
            if (ch == 0u || ch == MNK_PUCT_NONE) continue;
            const uint32_t pf = MNK_PUCT_PROOF(r.node[min((int)ch, kept - 1)].info);
            win |= pf == 1u;
            draw |= pf == 2u;
          }
          const bool ok = vproof == 1u || (vproof == 3u ? __ballot(win) != 0 : __ballot(draw) != 0);
          if (lane == 0 && ok) r.node[0].info = vproof << 12;
        }
      }
    } else {
      puct_row_fresh<NW>(r.row, r.L, pos, NWg, (int)(e.meta >> 1) < C, lane);
      if (lane == 0) {
        carried[2 * i] = 0;
        carried[2 * i + 1] = 0;
      }
    }
    row_write_view<NW, CN>(a.g, pos, 0, i, a.leaf_obs, a.leaf_dtype, a.leaf_mask, lane);
    return;
  }

  if (!h.live || spent) {
    advance_error_row<NW, CN>(a, r, pos, i, i, 1, lane);
    return;
  }

  // ---- selection: k_puct_step's (SOLVER: k_puct_step_leaves<true>'s at one leaf per row; the root has no proof here)
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a full tree shows its root again (it cannot happen: nodes <= keep_nodes + it)
  if (nodes <= TI) {
    puct_env_root<NW>(e, r.root, NWg);
    nstate = puct_walk<NW, CN, CK, false, SOLVER, false, FPU>(a.g, e, TI, a.c, r.node, r.prior, r.child, r.path, nodes, d,
                                                              lane, 0, 0u, nullptr, 0, nullptr, fpu, fpu_root);
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
    // no leaf: nothing is pending, so n_root cannot advance and the row would show its root for ever: reported, not silent
    if (nstate == 0u) mnk_report(a.err, MNK_ERR_VISITS, i);
  }
}

extern "C" {

int mnk_search_selfplay_advance(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies, int64_t T,
                                uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs,
                                int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh, uint64_t* plies_max, int64_t* stats,
                                int32_t* err, void* stream) {
  MnkAdvanceArgs a;
  const int rc = mnk_advance_check(MNK_ADVANCE_COMMON(temp_plies), &a);
  if (rc != MNK_OK) return rc;
  if (N == 0) return MNK_OK;
  MNK_DISPATCH(a.g, mnk_advance_launch(k_search_selfplay_advance<NW, CN, CK>, a, 0, stream));
  return mnk_launch_status("search_selfplay_advance");
}

// (what mnk_search_selfplay_advance_opts and its _fpu and _forced forms share: the option checks, then the launch)
static int advance_opts(const MnkAdvanceArgs& a, int solver, float noise_alpha, float noise_eps, int noise_fast,
                        float* root_priors, bool with_fpu, float fpu, float fpu_root, void* stream, bool forced = false,
                        float forced_k = 0.0f) {
  if (mnk_advance_options_check(a.g, solver, noise_alpha, noise_eps, noise_fast) != MNK_OK) return MNK_EINVAL;
  if (with_fpu && !mnk_advance_fpu_ok(fpu, fpu_root)) return MNK_EINVAL;
  if (forced && !(forced_k > 0.0f && forced_k <= 3.0e38f)) return MNK_EINVAL;
  if (a.N == 0) return MNK_OK;
  const MnkPuctNoise nz = mnk_advance_noise(noise_alpha);
  const size_t lds = mnk_advance_noise_lds(a.g, noise_alpha);
#define MNK_ADVANCE_OPTS(SOLVER, FPU, FORCED)                                                                    \
  MNK_DISPATCH(a.g, mnk_advance_launch(k_search_selfplay_advance_opts<NW, CN, CK, SOLVER, FPU, FORCED>, a, lds, \
                                       stream, nz, noise_eps, noise_fast, root_priors, fpu, fpu_root, forced_k))
  if (forced) {
    if (solver && with_fpu) MNK_ADVANCE_OPTS(true, true, true);
    else if (with_fpu) MNK_ADVANCE_OPTS(false, true, true);
    else if (solver) MNK_ADVANCE_OPTS(true, false, true);
    else MNK_ADVANCE_OPTS(false, false, true);
    return mnk_launch_status("search_selfplay_advance_opts_forced");
  }
  if (with_fpu) {
    if (solver) MNK_ADVANCE_OPTS(true, true, false);
    else MNK_ADVANCE_OPTS(false, true, false);
    return mnk_launch_status("search_selfplay_advance_opts_fpu");
  }
  if (solver) MNK_ADVANCE_OPTS(true, false, false);
  else MNK_ADVANCE_OPTS(false, false, false);
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
  MnkAdvanceArgs a;
  const int rc = mnk_advance_check(MNK_ADVANCE_COMMON(temp_plies), &a);
  if (rc != MNK_OK) return rc;
  return advance_opts(a, solver, noise_alpha, noise_eps, noise_fast, root_priors, false, 0.0f, 0.0f, stream);
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
  MnkAdvanceArgs a;
  const int rc = mnk_advance_check(MNK_ADVANCE_COMMON(temp_plies), &a);
  if (rc != MNK_OK) return rc;
  return advance_opts(a, solver, noise_alpha, noise_eps, noise_fast, root_priors, true, fpu, fpu_root, stream);
}
int mnk_search_selfplay_advance_opts_forced(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n,
                                            int k, int iterations, int fast_iterations, uint64_t full_threshold,
                                            const void* priors, int priors_dtype, const void* values, int values_dtype,
                                            float c, int temp_plies, uint64_t seed, const uint64_t* seed_dev,
                                            int64_t env_id0, uint64_t* row_plies, int64_t T, uint64_t* ring_planes,
                                            uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype,
                                            uint8_t* leaf_mask, uint8_t* fresh, uint64_t* plies_max, int64_t* stats,
                                            int32_t* err, int solver, float noise_alpha, float noise_eps, int noise_fast,
                                            float* root_priors, float fpu, float fpu_root, int fpu_on, float forced_k,
                                            void* stream) {
  MnkAdvanceArgs a;
  const int rc = mnk_advance_check(MNK_ADVANCE_COMMON(temp_plies), &a);
  if (rc != MNK_OK) return rc;
  if (fpu_on != 0 && fpu_on != 1) return MNK_EINVAL;
  return advance_opts(a, solver, noise_alpha, noise_eps, noise_fast, root_priors, fpu_on != 0, fpu, fpu_root, stream, true,
                      forced_k);
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
static int advance_keep(const MnkAdvanceArgs& a, int solver, float noise_alpha, float noise_eps, int noise_fast,
                        float* root_priors, int tree_iterations, int keep_nodes, int32_t* carried, bool with_fpu, float fpu,
                        float fpu_root, void* stream) {
  if (mnk_advance_options_check(a.g, solver, noise_alpha, noise_eps, noise_fast) != MNK_OK) return MNK_EINVAL;
  if (!carried || tree_iterations < a.I || tree_iterations > MNK_PUCT_ITERS_MAX || keep_nodes < 1 ||
      keep_nodes > tree_iterations + 1 - a.I)
    return MNK_EINVAL;
  // the launch's LDS: the kernel's static stage (NW = the variant's words per plane), the noise's doubles, the two maps
  const size_t map_stride = (size_t)((tree_iterations + 3) & ~1);
  const size_t lds = mnk_advance_noise_lds(a.g, noise_alpha) + (size_t)MNK_PUCT_ROWS * 2 * map_stride * sizeof(uint16_t);
  size_t lds_static = 0;
  MNK_DISPATCH(a.g, lds_static = sizeof(uint32_t) * MNK_PUCT_ROWS * 2 * NW);
  if (lds_static + lds > advance_keep_lds_limit()) return MNK_EINVAL;
  if (with_fpu && !mnk_advance_fpu_ok(fpu, fpu_root)) return MNK_EINVAL;
  if (a.N == 0) return MNK_OK;
  const MnkPuctNoise nz = mnk_advance_noise(noise_alpha);
#define MNK_ADVANCE_KEEP(SOLVER, FPU)                                                                                \
  MNK_DISPATCH(a.g, mnk_advance_launch(k_search_selfplay_advance_keep<NW, CN, CK, SOLVER, FPU>, a, lds, stream, nz, \
                                       noise_eps, noise_fast, root_priors, tree_iterations, keep_nodes, carried, fpu, \
                                       fpu_root))
  if (with_fpu) {
    if (solver) MNK_ADVANCE_KEEP(true, true);
    else MNK_ADVANCE_KEEP(false, true);
    return mnk_launch_status("search_selfplay_advance_keep_fpu");
  }
  if (solver) MNK_ADVANCE_KEEP(true, false);
  else MNK_ADVANCE_KEEP(false, false);
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
  MnkAdvanceArgs a;
  const int rc = mnk_advance_check(MNK_ADVANCE_COMMON(temp_plies), &a);
  if (rc != MNK_OK) return rc;
  return advance_keep(a, solver, noise_alpha, noise_eps, noise_fast, root_priors, tree_iterations, keep_nodes, carried,
                      false, 0.0f, 0.0f, stream);
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
  MnkAdvanceArgs a;
  const int rc = mnk_advance_check(MNK_ADVANCE_COMMON(temp_plies), &a);
  if (rc != MNK_OK) return rc;
  return advance_keep(a, solver, noise_alpha, noise_eps, noise_fast, root_priors, tree_iterations, keep_nodes, carried,
                      true, fpu, fpu_root, stream);
}

}  // extern "C"
