// mnk_puct_tree.h -- the PUCT tree as device code shared by the kernels that search it (the PUCT player,
// mnk_puct.hip, and search self-play with per-row budgets, mnk_search_selfplay_async*.hip): the node record and the
// workspace layout; a row's view of its workspace, its slots and its clamped header; the wave's LDS stage (packed planes
// in, a selection's planes in, a selected slot out); a fresh row, the backup of one evaluation, the solver's root counts,
// the Gumbel root's pick and improved policy, first-play urgency, the walk that selects the next leaf and the carry of a
// subtree into the next search.  The rule: include/mnk_hip.h, mnk_puct_step and mnk_puct_rebase.
#pragma once
#include "mnk_wave_rows.h"

// One tree node (12 B).  w is from the view of the player who moved into the node.
struct MnkPuctNode {
  uint32_t n;
  float w;
  uint32_t info;  // the move into the node | proof << 12 (the SOLVER kernels only; from w's point of view, 0: unknown,
                  // 1: WIN, 2: DRAW, 3: LOSS) | term << 16 (0: not terminal; 1: the move won; 2: it filled the board) |
                  // the parent's id << 18 (what k_puct_rebase_leaves marks a subtree by; the root's is 0)
};
#define MNK_PUCT_PROOF(info) (((info) >> 12) & 3u)
#define MNK_PUCT_TERM(info) (((info) >> 16) & 3u)
#define MNK_PUCT_PARENT(info) ((info) >> 18)
static_assert(sizeof(MnkPuctNode) == 12, "node record");

// The workspace of one row, at row * L.row bytes (every part 16-byte aligned, the row 256-byte aligned):
//   header   u32[4]          nodes created, leaf depth, state (bit 0: a backup is pending; bits 1-2: the leaf's term, with
//                            the solver its proof;
//                            bit 3: the pending evaluation is of a root that k_puct_rebase_leaves carried over -- it only
//                            renews the root's priors), live (the root has a legal cell)
//   root     u32[2][NWg]     the root's guard-column bit planes (plane 0 = the root's side to move), NWg = MnkGeom::NW
//   leaf     u32[2][NWg]     the pending leaf's planes
//   path     u16[I + 2]      node ids root .. leaf
//   node     MnkPuctNode[I + 1]
//   prior    f32[I + 1][C]   the evaluator's prior of each legal cell of node v, at v * C (slot = node id)
//   child    u16[I + 1][C]   the child of node v through each cell: 0 = none yet (node 0, the root, is never a child),
//                            0xFFFF = an occupied cell
// and, with Lv > 1 leaves per evaluation, behind all of that the state of slots 1 .. Lv - 1 (slot 0's is the header's
// depth and state, `leaf` and `path`):
//   xhdr     u32[Lv - 1][2]       leaf depth, state
//   xleaf    u32[Lv - 1][2][NWg]  the slot's pending leaf's planes
//   xpath    u16[Lv - 1][..]      its path, `pstride` bytes apart
// About (I + 1) * 6 * C bytes per row.  The host (mnk_puct_workspace_bytes) and the kernels share this one function.
struct MnkPuctLayout {
  int64_t root, leaf, path, node, prior, child, xhdr, xleaf, xpath, pstride, row;
};
__host__ __device__ inline int64_t mnk_puct_al(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
__host__ __device__ inline MnkPuctLayout mnk_puct_layout(int NWg, int C, int I, int Lv = 1) {
  MnkPuctLayout L;
  L.root = 16;
  L.leaf = L.root + 8 * NWg;
  L.path = mnk_puct_al(L.leaf + 8 * NWg, 16);
  L.node = mnk_puct_al(L.path + 2 * (int64_t)(I + 2), 16);
  L.prior = mnk_puct_al(L.node + 12 * (int64_t)(I + 1), 16);
  L.child = mnk_puct_al(L.prior + 4 * (int64_t)(I + 1) * C, 16);
  L.row = mnk_puct_al(L.child + 2 * (int64_t)(I + 1) * C, 256);
  L.pstride = mnk_puct_al(2 * (int64_t)(I + 2), 16);
  L.xhdr = mnk_puct_al(L.child + 2 * (int64_t)(I + 1) * C, 16);
  L.xleaf = mnk_puct_al(L.xhdr + 8 * (int64_t)(Lv - 1), 16);
  L.xpath = mnk_puct_al(L.xleaf + 8 * (int64_t)NWg * (Lv - 1), 16);
  if (Lv > 1) L.row = mnk_puct_al(L.xpath + L.pstride * (Lv - 1), 256);  // (Lv = 1: nothing behind `child`)
  return L;
}

#define MNK_PUCT_ROWS 4  // rows (waves) per 256-lane workgroup
#define MNK_PUCT_NONE 0xFFFFu

// fsqrt((float)n) correctly rounded for a visit count n < 2^24.  The compiler lowers the square root of a converted
// integer to a bare v_sqrt_f32, which may be an ulp off; sqrt(n) is compared with the midpoints around that result
// exactly in f64 (a midpoint has 25 significant bits, its square 50) and the result moved by an ulp when it lies
// outside.  (No midpoint is the square root of an integer below 2^48: there are no ties.)
__device__ __forceinline__ float puct_sqrt_rn(uint32_t n) {
  float r = __fsqrt_rn((float)n);
  const uint32_t b = __float_as_uint(r);
  const double dr = (double)r, dn = (double)n;
  const double lo = (dr + (double)__uint_as_float(b ? b - 1u : 0u)) * 0.5;
  const double hi = (dr + (double)__uint_as_float(b + 1u)) * 0.5;
  if (__dmul_rn(lo, lo) > dn) r = __uint_as_float(b - 1u);
  else if (__dmul_rn(hi, hi) < dn) r = __uint_as_float(b + 1u);
  return r;
}

__device__ __forceinline__ float puct_read(const void* p, int dtype, int64_t q) {
  return dtype == MNK_LOGITS_BF16 ? __uint_as_float((uint32_t)((const uint16_t*)p)[q] << 16) : ((const float*)p)[q];
}

// pos as the row's root planes and as its pending leaf's
template <int NW>
__device__ __forceinline__ void puct_row_root(unsigned char* row, const MnkPuctLayout& L, const uint32_t* pos, int NWg,
                                              int lane) {
  uint32_t* root = (uint32_t*)(row + L.root);
  uint32_t* leaf = (uint32_t*)(row + L.leaf);
  for (int q = lane; q < 2 * NWg; q += 64) {
    const uint32_t v = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
    root[q] = v;
    leaf[q] = v;
  }
}

// a fresh tree: the root node alone, its evaluation pending
template <int NW>
__device__ __forceinline__ void puct_row_fresh(unsigned char* row, const MnkPuctLayout& L, const uint32_t* pos, int NWg,
                                               bool legal, int lane) {
  puct_row_root<NW>(row, L, pos, NWg, lane);
  if (lane == 0) {
    uint32_t* hdr = (uint32_t*)row;
    hdr[0] = 1u;                     // the root
    hdr[1] = 0u;                     // the leaf is the root
    hdr[2] = 1u;                     // its evaluation is pending, not terminal
    hdr[3] = legal ? 1u : 0u;        // a legal cell
    ((uint16_t*)(row + L.path))[0] = 0;
    MnkPuctNode r;
    r.n = 0u; r.w = 0.0f; r.info = 0u;
    *(MnkPuctNode*)(row + L.node) = r;
  }
}

// slots 1 .. leaves - 1 of evaluation 0 are void: nothing pending, the root's view (pos) as batch rows i * leaves + j
template <int NW, int CN>
__device__ __forceinline__ void puct_row_void_slots(const MnkGeom& g, unsigned char* row, const MnkPuctLayout& L,
                                                    const uint32_t* pos, int64_t i, int leaves, void* leaf_obs,
                                                    int leaf_dtype, uint8_t* leaf_mask, int lane) {
  for (int j = 1; j < leaves; ++j) {
    if (lane == 0) {
      uint32_t* ds = (uint32_t*)(row + L.xhdr) + 2 * (j - 1);
      ds[0] = 0u;
      ds[1] = 0u;
    }
    row_write_view<NW, CN>(g, pos, 0, i * leaves + j, leaf_obs, leaf_dtype, leaf_mask, lane);
  }
}

// ------------------------------------------------------------------ a row's view of its workspace
// (what every kernel that steps a tree begins with; TI: the layout's iterations, the caller's)
struct MnkPuctRow {
  MnkPuctLayout L;
  unsigned char* row;
  uint32_t* hdr;
  const uint32_t* root;
  uint32_t* leaf;  // (slot 0's, as `path`)
  uint16_t* path;
  MnkPuctNode* node;
  float* prior;
  uint16_t* child;
};
__device__ __forceinline__ MnkPuctRow puct_row(unsigned char* ws, int64_t i, int NWg, int C, int TI, int leaves = 1) {
  MnkPuctRow r;
  r.L = mnk_puct_layout(NWg, C, TI, leaves);
  r.row = ws + i * r.L.row;
  r.hdr = (uint32_t*)r.row;
  r.root = (const uint32_t*)(r.row + r.L.root);
  r.leaf = (uint32_t*)(r.row + r.L.leaf);
  r.path = (uint16_t*)(r.row + r.L.path);
  r.node = (MnkPuctNode*)(r.row + r.L.node);
  r.prior = (float*)(r.row + r.L.prior);
  r.child = (uint16_t*)(r.row + r.L.child);
  return r;
}
// slot j's {depth, state}, leaf planes and path (slot 0: the header's, `leaf`, `path`)
__device__ __forceinline__ uint32_t* puct_slot_ds(const MnkPuctRow& r, int j) {
  return j ? (uint32_t*)(r.row + r.L.xhdr) + 2 * (j - 1) : r.hdr + 1;
}
__device__ __forceinline__ uint32_t* puct_slot_leaf(const MnkPuctRow& r, int j, int NWg) {
  return (uint32_t*)(r.row + (j ? r.L.xleaf + 8 * (int64_t)NWg * (j - 1) : r.L.leaf));
}
__device__ __forceinline__ uint16_t* puct_slot_path(const MnkPuctRow& r, int j) {
  return (uint16_t*)(r.row + (j ? r.L.xpath + r.L.pstride * (j - 1) : r.L.path));
}

// The header, clamped by the layout's iterations: whatever the workspace holds, no id leaves the row and nodes - 1 is a
// node.  (nodes >= 1 changes nothing for a workspace that mnk_puct_begin* / mnk_puct_rebase* set up -- the root is created
// there and nodes never falls; it keeps `min(id, nodes - 1)` from going negative in one that nobody set up.)
struct MnkPuctHeader {
  int nodes, depth;
  uint32_t state;
  bool live;
};
__device__ __forceinline__ MnkPuctHeader puct_header(const uint32_t* hdr, int TI) {
  MnkPuctHeader h;
  h.nodes = (int)min(max(hdr[0], 1u), (uint32_t)(TI + 1));
  h.depth = (int)min(hdr[1], (uint32_t)TI);
  h.state = hdr[2];
  h.live = hdr[3] != 0u;
  return h;
}

// ------------------------------------------------------------------ the wave's stage
// (pos: the wave's own 2 * NW words of LDS.  A piece that writes or reads pos says which row_wave_sync() its caller owes.)
// packed planes of the workspace (a leaf's, the root's: u32[2][NWg]) into pos, padded to NW words a plane; every lane
// calls it.  The caller owes a row_wave_sync() after it, and one before it when lanes may still read the stage.
template <int NW>
__device__ __forceinline__ void puct_stage_planes(uint32_t* pos, const uint32_t* src, int NWg, int lane) {
  for (int q = lane; q < 2 * NW; q += 64) {
    const int pl = q >= NW, w = q - (pl ? NW : 0);
    pos[q] = w < NWg ? src[pl * NWg + w] : 0u;
  }
}

// The planes a slot shows after a walk that started from e (so e is set up), by lane 0 into the stage: the walk's leaf, e,
// when nstate != 0; else nothing is pending and the slot shows the root.  (A slot that no walk entered stages the root
// with puct_stage_planes.)  e's words are read ahead of the choice: written as `nstate ? e.p[..] : root[..]` on a reference
// the compiler selects between the two addresses, which costs the 19x19 kernels 5 VGPRs and 9 % more instructions.  The
// caller owes a row_wave_sync() before it, when lanes may still read the stage; the one after it is
// puct_store_selection's.
template <int NW>
__device__ __forceinline__ void puct_stage_selection(uint32_t* pos, const MnkEnv<NW>& e, uint32_t nstate,
                                                     const uint32_t* root, int NWg, int lane) {
  if (lane == 0) {
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const uint32_t l0 = e.p[0][w], l1 = e.p[1][w];
      pos[w] = nstate ? l0 : (w < NWg ? root[w] : 0u);
      pos[NW + w] = nstate ? l1 : (w < NWg ? root[NWg + w] : 0u);
    }
  }
}

// The slot's planes are staged (puct_stage_selection, or puct_stage_planes of the root): path[0] and the slot's {depth,
// state} (ds) by lane 0, the sync, the planes to the workspace (leafp), the view as batch row b with parity d & 1.
template <int NW, int CN>
__device__ __forceinline__ void puct_store_selection(const MnkGeom& g, const uint32_t* pos, uint32_t nstate, int d,
                                                     uint16_t* path, uint32_t* ds, uint32_t* leafp, int64_t b,
                                                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int lane) {
  const int NWg = g.NW;
  if (lane == 0) {
    path[0] = 0;
    ds[0] = (uint32_t)d;
    ds[1] = nstate;
  }
  row_wave_sync();
  for (int q = lane; q < 2 * NWg; q += 64) leafp[q] = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
  row_write_view<NW, CN>(g, pos, d & 1, b, leaf_obs, leaf_dtype, leaf_mask, lane);
}

// The backup of one pending evaluation (state bit 0 set): batch row b of priors / values, the leaf's planes in pos (LDS).
// SOLVER: the leaf's term is its proof (3: a proven loss of its mover, +1 for its side to move), and a proven leaf's
// backup ends with the proofs of its path, leaf side first: one scan of a node's child row per level (the selection's
// access shape, the children's info gathered, reduced over the wave), at most `depth` levels, over as soon as a node
// stays unknown or was proven before.
template <int NW, int CN, bool SOLVER = false>
__device__ __forceinline__ void puct_backup(const MnkGeom& g, const uint32_t* pos, const uint16_t* path, MnkPuctNode* node,
                                            float* prior, uint16_t* child, int nodes, int depth, uint32_t state,
                                            const void* priors, int priors_dtype, const void* values, int values_dtype,
                                            int64_t b, int lane) {
  const int C = g.C;
  const int lf = min((int)path[depth], nodes - 1);
  const uint32_t term = (state >> 1) & 3u;
  const bool renew = (state & 8u) != 0u;  // a carried root (k_puct_rebase_leaves): its priors again and nothing else
  float v;
  if (term) {
    v = term == 1u ? -1.0f : 0.0f;  // the mover into the leaf won: a loss for its side to move
    if constexpr (SOLVER)
      if (term == 3u) v = 1.0f;
  } else {
    v = puct_read(values, values_dtype, b);
    float* pr = prior + (int64_t)lf * C;
    uint16_t* cl = child + (int64_t)lf * C;
    for (int a = lane; a < C; a += 64) {
      const bool occ = row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a);
      if (!renew) cl[a] = occ ? (uint16_t)MNK_PUCT_NONE : (uint16_t)0;
      if (!occ) pr[a] = puct_read(priors, priors_dtype, b * C + a);
    }
  }
  for (int p = lane; p <= depth && !renew; p += 64) {  // depth - p odd: the mover into path[p] is the leaf's side to move
    MnkPuctNode* k = &node[min((int)path[p], nodes - 1)];
    k->n += 1u;
    k->w = __fadd_rn(k->w, ((depth - p) & 1) ? v : -v);
  }
  row_wave_sync();
  if constexpr (SOLVER) {
    for (int p = depth - 1; p >= 0 && term; --p) {
      const int x = min((int)path[p], nodes - 1);
      const uint32_t info = node[x].info;
      if (MNK_PUCT_PROOF(info)) break;
      const uint16_t* cl = child + (int64_t)x * C;
      bool win = false, open = false, held = false;  // a child that is WIN / missing or unknown / not LOSS
      for (int a = lane; a < C; a += 64) {
        const uint32_t ch = cl[a];
        if (ch == MNK_PUCT_NONE) continue;
        const uint32_t pf = ch ? MNK_PUCT_PROOF(node[min((int)ch, nodes - 1)].info) : 0u;
        win |= pf == 1u;
        open |= pf == 0u;
        held |= pf != 3u;
      }
      uint32_t pf = 3u;  // a move that wins: the mover into x has lost
      if (!__ballot(win)) {
        if (__ballot(open)) break;
        pf = __ballot(held) ? 2u : 1u;
      }
      if (lane == 0) node[x].info = info | (pf << 12);
      row_wave_sync();  // (the next level gathers this proof)
    }
  }
}

template <int NW>
__device__ __forceinline__ void puct_env_root(MnkEnv<NW>& e, const uint32_t* root, int NWg) {
  int stones = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    e.p[0][w] = w < NWg ? root[w] : 0u;
    e.p[1][w] = w < NWg ? root[NWg + w] : 0u;
    stones += __popc(e.p[0][w] | e.p[1][w]);
  }
  e.meta = (uint32_t)stones << 1;
}

// ------------------------------------------------------------------ the solver's adjusted root counts
// What a search that proves moves plays from and records (mnk_puct_step_solver): shared by its move, puct_move<true>,
// and by the ply of search self-play with per-row budgets.
// The root's child through cell a (child = the root's child row); n = 0 where there is none.
__device__ __forceinline__ MnkPuctNode puct_root_kid(int C, const MnkPuctNode* node, const uint16_t* child, int nodes,
                                                     bool live, int a) {
  MnkPuctNode k;
  k.n = 0u; k.w = 0.0f; k.info = 0u;
  const uint32_t ch = live && a < C ? child[a] : MNK_PUCT_NONE;
  if (ch != 0u && ch != MNK_PUCT_NONE) k = node[min((int)ch, nodes - 1)];
  return k;
}
// child k's count under `keep`: 0 = every child's n, 1 = the WIN children's, 2 = all but the LOSS children's
__device__ __forceinline__ uint32_t puct_kept_count(const MnkPuctNode& k, int keep) {
  const uint32_t pf = MNK_PUCT_PROOF(k.info);
  return (keep == 1 && pf != 1u) || (keep == 2 && pf == 3u) ? 0u : k.n;
}
// The root's `keep` (wave-uniform): 1 if some child is WIN, else 2; were those counts all zero, 0, the raw ones.  maxn and
// tot: the maximum and the sum of the counts kept.
__device__ __forceinline__ int puct_root_keep(int C, const MnkPuctNode* node, const uint16_t* child, int nodes, bool live,
                                              int lane, uint32_t& maxn, uint32_t& tot) {
  bool win = false;
  for (int a = lane; a < C; a += 64) win |= MNK_PUCT_PROOF(puct_root_kid(C, node, child, nodes, live, a).info) == 1u;
  int keep = __ballot(win) ? 1 : 2;
  maxn = 0u;
  tot = 0u;
  for (int t = 0; t < 2 && !maxn; ++t) {  // the adjusted counts; were they all zero, the raw ones
    if (t) keep = 0;
    tot = 0u;
    for (int a = lane; a < C; a += 64) {
      const uint32_t na = puct_kept_count(puct_root_kid(C, node, child, nodes, live, a), keep);
      maxn = max(maxn, na);
      tot += na;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
      tot += (uint32_t)__shfl_xor((int)tot, off, 64);
    }
  }
  return keep;
}

// ------------------------------------------------------------------ policy target pruning
// What a search with forced playouts plays from and records (the rule: include/mnk_hip.h, mnk_puct_step_forced): shared by
// its move, puct_move_forced, and by the ply of search self-play with per-row budgets.  One wave per row, a cell per lane.
// The root's constants and the cell of most visits with its score (wave-uniform); on = false: nothing is pruned.
struct MnkPuctPrune {
  bool on;
  int cstar;
  float k, c, sq, t1, sstar;  // k; c; fsqrt((float)n_0); (float)(n_0 - 1); s*
};
// s_a(j): the score of the root's child `kid` through a cell of prior p, had it j visits
__device__ __forceinline__ float puct_prune_score(const MnkPuctPrune& pp, const MnkPuctNode& kid, float p, uint32_t j) {
  return __fadd_rn(__fdiv_rn(kid.w, (float)kid.n), __fdiv_rn(__fmul_rn(__fmul_rn(pp.c, p), pp.sq), (float)(1u + j)));
}
// count(q): n' of cell q, 0 for q >= C and where there is no child.  pr = the root's stored priors, `child` its child row.
// The arg-max (ties to the lowest cell) by one pass and one __shfl_xor reduction; s* from the winner's record.
template <class Count>
__device__ __forceinline__ MnkPuctPrune puct_prune_root(int C, float k, float c, const MnkPuctNode* node, const float* pr,
                                                        const uint16_t* child, int nodes, bool live, Count count,
                                                        int lane) {
  uint32_t bn = 0u;
  int ba = 0x7fffffff;
  for (int a = lane; a < C; a += 64) {
    const uint32_t na = count(a);
    if (na > bn) {  // (a rises: ">" keeps the lowest cell of a tie)
      bn = na;
      ba = a;
    }
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const uint32_t on = (uint32_t)__shfl_xor((int)bn, off, 64);
    const int oa = __shfl_xor(ba, off, 64);
    if (on > bn || (on == bn && oa < ba)) {
      bn = on;
      ba = oa;
    }
  }
  MnkPuctPrune pp;
  pp.on = bn != 0u;
  pp.cstar = min(ba, C - 1);  // (bn = 0: no cell; nothing is read through it then)
  pp.c = c;
  pp.k = k;
  const uint32_t n0 = max(node[0].n, 1u);
  pp.sq = puct_sqrt_rn(n0);
  pp.t1 = (float)(n0 - 1u);
  pp.sstar = 0.0f;
  if (pp.on) pp.sstar = puct_prune_score(pp, puct_root_kid(C, node, child, nodes, live, pp.cstar), pr[pp.cstar], bn);
  return pp;
}
// n'' of cell a from its n' = na, its child's record and its prior.  The rule walks j upwards; s_a(j) does not increase
// with j for p > 0 (a correctly rounded quotient by a growing divisor, then a correctly rounded sum), and neither does
// "F * F >= t" turn false again as F grows, so both searches bisect: at most 2 * 24 probes a cell, no memory.
__device__ __forceinline__ uint32_t puct_pruned_count(const MnkPuctPrune& pp, int a, uint32_t na, const MnkPuctNode& kid,
                                                      float p) {
  if (!pp.on || a == pp.cstar || na == 0u || p <= 0.0f) return na;
  const float t = __fmul_rn(__fmul_rn(pp.k, p), pp.t1);
  uint32_t lo = 0u, hi = na;  // min(n', F_a): the least F in [0, n') with F * F >= t, n' when there is none
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (__fmul_rn((float)mid, (float)mid) >= t) hi = mid;
    else lo = mid + 1u;
  }
  uint32_t jl = na - lo, jh = na;  // the least j in [n' - min(n', F_a), n') with s_a(j) < s*, n' when there is none
  while (jl < jh) {
    const uint32_t mid = (jl + jh) >> 1;
    if (puct_prune_score(pp, kid, p, mid) < pp.sstar) jh = mid;
    else jl = mid + 1u;
  }
  return jl == 1u && na > 1u ? 0u : jl;
}

// ------------------------------------------------------------------ the Gumbel root
// (k_puct_step_gumbel and k_search_selfplay_advance_gumbel)
// What the root of row i reads besides the tree: its row of gscore (mnk_puct_gumbel_root), the table of considered visits
// (mnk_puct_gumbel_schedule, [considered + 1][I]; the I that puct_gumbel_pick and puct_walk are given is its row stride)
// and the constants of sigma.
struct MnkPuctGumbel {
  const float* gs;
  const uint16_t* table;
  int considered;
  float c_visit, c_scale;
};

// The root's child of maximal key among the free cells of `want` visits -- LAST: of the most visits; else of
// table[min(considered, F)][n_root - 1] visits -- or, when no free cell has that count, among all free cells; ties to the
// lowest cell, 0x7fffffff for a root without a free cell.  Wave-uniform.  Two scans of the root's child row in the access
// shape of the scoring loop (cells over the lanes, a child's record gathered): the first for F and the most visits, the
// second for the two maxima, each reduced by __shfl_xor.
template <bool LAST>
__device__ __forceinline__ int puct_gumbel_pick(int C, int I, const MnkPuctNode* node, const uint16_t* cl, int nodes,
                                                const MnkPuctGumbel& gm, int lane, uint32_t* maxn_out = nullptr) {
  uint32_t F = 0u, maxn = 0u;
  for (int a = lane; a < C; a += 64) {
    const uint32_t ch = cl[a];
    if (ch == MNK_PUCT_NONE) continue;
    ++F;
    if (ch) maxn = max(maxn, node[min((int)ch, nodes - 1)].n);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    F += (uint32_t)__shfl_xor((int)F, off, 64);
    maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
  }
  if (maxn_out) *maxn_out = maxn;
  uint32_t want = maxn;
  if (!LAST) {  // (clamped: whatever the workspace holds, the read stays inside the table)
    const int t = min((int)max(node[0].n, 1u) - 1, I - 1);
    want = gm.table[(int64_t)min((uint32_t)gm.considered, F) * I + t];
  }
  const float sigma = __fmul_rn(__fadd_rn(gm.c_visit, (float)maxn), gm.c_scale);
  float bk = 0.0f, ak = 0.0f;  // the best key among the cells of `want` visits / among all free cells
  int ba = 0x7fffffff, aa = 0x7fffffff;
  for (int a = lane; a < C; a += 64) {
    const uint32_t ch = cl[a];
    if (ch == MNK_PUCT_NONE) continue;
    float key = gm.gs[a];
    uint32_t na = 0u;
    if (ch) {
      const MnkPuctNode k = node[min((int)ch, nodes - 1)];
      na = k.n;
      if (na) key = __fadd_rn(key, __fmul_rn(sigma, __fdiv_rn(k.w, (float)na)));
    }
    if (na == want && (ba == 0x7fffffff || key > bk)) {  // (a rises: ">" keeps the lowest cell of a tie)
      bk = key;
      ba = a;
    }
    if (aa == 0x7fffffff || key > ak) {
      ak = key;
      aa = a;
    }
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const float ob = __shfl_xor(bk, off, 64), oa = __shfl_xor(ak, off, 64);
    const int obc = __shfl_xor(ba, off, 64), oac = __shfl_xor(aa, off, 64);
    if (obc != 0x7fffffff && (ba == 0x7fffffff || ob > bk || (ob == bk && obc < ba))) {
      bk = ob;
      ba = obc;
    }
    if (oac != 0x7fffffff && (aa == 0x7fffffff || oa > ak || (oa == ak && oac < aa))) {
      ak = oa;
      aa = oac;
    }
  }
  return __builtin_amdgcn_readfirstlane(ba != 0x7fffffff ? ba : aa);
}

// a sum over the wave, the same value in every lane
__device__ __forceinline__ double puct_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// The improved policy of a Gumbel root after its last backup (the rule: include/mnk_hip.h, mnk_puct_step_gumbel); maxn is
// puct_gumbel_pick<true>'s.  f64: five passes over the root's cells (the sum of the clamped priors; the visited cells'
// sums for v_mix; the maximum of y; the sum of exp(y - max); the store), every pass recomputing a cell's terms from the
// tree -- the same operations on the same inputs give the same y each time -- and reduced over the wave.  pr = the root's
// stored priors (node 0's row), cl its child row.  store(a, policy_a) is called once for every cell a < C by the lane that
// owns it (a = lane, lane + 64, ...), with 0 for an occupied cell.
template <class Store>
__device__ __forceinline__ void puct_gumbel_policy(int C, const MnkPuctNode* node, const float* pr, const uint16_t* cl,
                                                   int nodes, const MnkPuctGumbel& gm, float vroot, uint32_t maxn, int lane,
                                                   Store store) {
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
  for (int a = lane; a < C; a += 64) store(a, y_of(a, y) ? (float)(exp(y - my) / se) : 0.0f);
}

// ------------------------------------------------------------------ first-play urgency
// A visited cell's share of the visited prior mass: the prior clipped to [0, 1] as a 32-bit fixed-point number (truncated;
// 2^32 for a prior of 1 or more).  Integers, so that the order of the sum over the lanes cannot matter.
__device__ __forceinline__ uint64_t puct_fpu_term(float p) {
  const float pc = fminf(fmaxf(p, 0.0f), 1.0f);
  return pc >= 1.0f ? 1ull << 32 : (uint64_t)(uint32_t)__fmul_rn(pc, 0x1p32f);  // (pc < 1: the product is exact, < 2^32)
}
// The q of node k's free cells without a visit from the lanes' partial sums T of puct_fpu_term (reduced here; the result
// is the same in every lane): mass = fl32(sqrt(T * 2^-32)), the f64 square root correctly rounded (T < 2^43: the
// conversion and the scaling are exact), q_v = -w / n from the stored record, q = max(q_v - r * mass, -1).
__device__ __forceinline__ float puct_fpu_q(uint64_t T, const MnkPuctNode& k, float r) {
#pragma unroll
  for (int off = 32; off; off >>= 1) T += (uint64_t)__shfl_xor((unsigned long long)T, off, 64);
  const float mass = (float)__dsqrt_rn(__dmul_rn((double)T, 0x1p-32));
  const float qv = __fdiv_rn(-k.w, (float)k.n);
  return fmaxf(__fsub_rn(qv, __fmul_rn(r, mass)), -1.0f);
}

// One walk from the root (e = the root's position on entry, the leaf's on return; wave-uniform): the new pending state
// (0: no leaf), the leaf's depth in d, its path in path[1 .. d].  A new leaf becomes node `nodes`.
// VL: the walk of a slot under the virtual visits of the round's earlier slots.  vl(x) is counted from their stored paths
// (the tree has one path to a node: slot l's path holds x, a node at depth t, iff its entry t is x): `share` = the
// earlier slots whose path runs through the walk's node v, slot l's path and depth are lane l's epath / edepth, and a
// child's vl = how many slots of `share` go on to it.  nodes0 = the node count when the round began: a node of a higher
// id that is not terminal has no evaluation yet, and reaching it ends the walk without a leaf.
// SOLVER: a child that is proven LOSS (a move proven to lose for the player making it) is a candidate only when every
// child is -- `bc`, the class of the best cell so far (1: not such a child), orders before the score -- and the walk ends
// in a child with a proof as it ends in a terminal one; the new pending state carries the proof in the term's bits.
// GUMBEL: at the root the cell is puct_gumbel_pick's (gm: the row's Gumbel inputs); from the chosen child on, the walk
// below.
// FPU: first-play urgency (the rule: include/mnk_hip.h, mnk_puct_step_fpu).  A free cell without a visit scores with
// q = max(q_v - r * mass, -1) in the place of 0, r = fpu_root at the root and fpu below it: puct_fpu_q, one more pass over
// the node's child row and priors before the scoring loop, in its access shape.
// FORCED: forced playouts at the root (the rule: include/mnk_hip.h, mnk_puct_step_forced), when `force` (wave-uniform: the
// per-row loop's "this ply forces") is set.  A root cell whose child has a stored visit, is not proven LOSS and has
// n'^2 < k * P * S' is of class 2, above SOLVER's two: the test stands beside the score in the per-cell loop (S' = nv - 1,
// the nv the loop already has), and `bc` orders the candidates as it does for SOLVER -- no pass and no reduction more.
template <int NW, int CN, int CK, bool VL, bool SOLVER = false, bool GUMBEL = false, bool FPU = false,
          bool FORCED = false>
__device__ __forceinline__ uint32_t puct_walk(const MnkGeom& g, MnkEnv<NW>& e, int I, float c, MnkPuctNode* node,
                                              const float* prior, uint16_t* child, uint16_t* path, int& nodes, int& d,
                                              int lane, int nodes0 = 0, uint32_t share = 0u,
                                              const uint16_t* epath = nullptr, int edepth = 0,
                                              const MnkPuctGumbel* gm = nullptr, float fpu = 0.0f,
                                              float fpu_root = 0.0f, float forced_k = 0.0f, bool force = false) {
  const int C = g.C;
  constexpr bool CLS = SOLVER || FORCED;  // the candidates have classes: `bc` orders before the score
  int v = 0;
  for (;;) {
    uint32_t nxt = 0u;  // VL: where lane l's slot goes from v (0: not through v, or its leaf is v)
    uint32_t nv = node[v].n;
    if (VL) {
      if (lane < MNK_PUCT_LEAVES_MAX && ((share >> lane) & 1u) && edepth > d) nxt = epath[d + 1];
      nv += (uint32_t)__popc(share);
    }
    // the slots' next nodes as wave-uniform values, read here where every lane is active (the per-cell loop below is not)
    uint32_t nx[MNK_PUCT_LEAVES_MAX];
    if (VL) {
#pragma unroll
      for (int l = 0; l < MNK_PUCT_LEAVES_MAX; ++l) nx[l] = (uint32_t)__builtin_amdgcn_readlane((int)nxt, l);
    }
    const float sq = puct_sqrt_rn(nv);
    const float* pr = prior + (int64_t)v * C;
    const uint16_t* cl = child + (int64_t)v * C;
    float best = 0.0f;
    int ba = 0x7fffffff;
    [[maybe_unused]] int bc = 0;
    [[maybe_unused]] bool picked = false;  // GUMBEL, at the root: ba is the cell already, the same in every lane
    if constexpr (GUMBEL) {
      if (v == 0) {
        ba = puct_gumbel_pick<false>(C, I, node, cl, nodes, *gm, lane);
        picked = true;
      }
    }
    [[maybe_unused]] float qu = 0.0f;  // FPU: the q of a free cell without a visit, the same in every lane
    if constexpr (FPU) {
      uint64_t T = 0ull;
      for (int a = lane; a < C; a += 64) {
        const uint32_t ch = cl[a];
        if (ch == MNK_PUCT_NONE || ch == 0u) continue;
        const int kk = min((int)ch, nodes - 1);
        uint32_t na = node[kk].n;
        if (VL && share) {
#pragma unroll
          for (int l = 0; l < MNK_PUCT_LEAVES_MAX; ++l) na += nx[l] == (uint32_t)kk;
        }
        if (na) T += puct_fpu_term(pr[a]);
      }
      qu = puct_fpu_q(T, node[v], v == 0 ? fpu_root : fpu);
    }
    if (!picked)  // (the loop keeps its indentation: below this line the scoring is the text it was)
    for (int a = lane; a < C; a += 64) {
      const uint32_t ch = cl[a];
      if (ch == MNK_PUCT_NONE) continue;
      uint32_t na = 0u;
      float wa = 0.0f;
      [[maybe_unused]] int cls = 1;
      [[maybe_unused]] uint32_t stored = 0u;  // FORCED: the child's n without the round's virtual visits
      if (ch) {
        const int kk = min((int)ch, nodes - 1);
        const MnkPuctNode k = node[kk];
        na = k.n;
        wa = k.w;
        if constexpr (SOLVER) cls = MNK_PUCT_PROOF(k.info) != 3u;
        if constexpr (FORCED) stored = na;
        if (VL && share) {
          uint32_t vl = 0u;  // (nx is 0, never a child's id, for a slot that is not in `share`)
#pragma unroll
          for (int l = 0; l < MNK_PUCT_LEAVES_MAX; ++l) vl += nx[l] == (uint32_t)kk;
          na += vl;
          wa = __fadd_rn(wa, -(float)vl);
        }
      }
      const float q = na ? __fdiv_rn(wa, (float)na) : (FPU ? qu : 0.0f);
      const float s = __fadd_rn(q, __fdiv_rn(__fmul_rn(__fmul_rn(c, pr[a]), sq), (float)(1u + na)));
      if constexpr (FORCED) {  // (a child of this round has no stored visit: never forced)
        if (v == 0 && force && stored && cls == 1 &&
            __fmul_rn((float)na, (float)na) < __fmul_rn(__fmul_rn(forced_k, pr[a]), (float)(nv - 1u)))
          cls = 2;
      }
      if constexpr (CLS) {
        if (ba == 0x7fffffff || cls > bc || (cls == bc && s > best)) {
          best = s;
          ba = a;
          bc = cls;
        }
      } else if (ba == 0x7fffffff || s > best) {  // (a rises: ">" keeps the lowest cell of a tie)
        best = s;
        ba = a;
      }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const float ob = __shfl_xor(best, off, 64);
      const int oa = __shfl_xor(ba, off, 64);
      if constexpr (CLS) {
        const int oc = __shfl_xor(bc, off, 64);
        if (oa != 0x7fffffff &&
            (ba == 0x7fffffff || oc > bc || (oc == bc && (ob > best || (ob == best && oa < ba))))) {
          best = ob;
          ba = oa;
          bc = oc;
        }
      } else if (oa != 0x7fffffff && (ba == 0x7fffffff || ob > best || (ob == best && oa < ba))) {
        best = ob;
        ba = oa;
      }
    }
    const int a = __builtin_amdgcn_readfirstlane(ba);
    if (a == 0x7fffffff) return 0u;  // (an evaluated non-terminal node always has a legal cell)
    const uint32_t ch = cl[a];
    const MnkPly ply = env_play<NW, CN, CK, true>(g, e, a, false);
    ++d;
    if (ch == 0u) {  // a new node: the leaf
      const uint32_t term = ply.win ? 1u : (ply.done ? 2u : 0u);
      if (lane == 0) {
        MnkPuctNode k;
        k.n = 0u; k.w = 0.0f; k.info = (uint32_t)a | (term << 16) | ((uint32_t)v << 18);
        if constexpr (SOLVER) k.info |= term << 12;
        node[nodes] = k;
        child[(int64_t)v * C + a] = (uint16_t)nodes;
        path[d] = (uint16_t)nodes;
      }
      ++nodes;
      return 1u | (term << 1);
    }
    const int k = min((int)ch, nodes - 1);
    if (lane == 0) path[d] = (uint16_t)k;
    const uint32_t term = SOLVER ? MNK_PUCT_PROOF(node[k].info) : MNK_PUCT_TERM(node[k].info);  // (a constant choice)
    if (term) return 1u | (term << 1);  // an existing terminal child (SOLVER: a proven one): the leaf again
    if (VL) {
      if (k >= nodes0) return 0u;  // created in this round: not evaluated yet
      share = (uint32_t)__ballot(nxt == (uint32_t)k);
    }
    v = k;
    if (d >= I) return 0u;  // (cannot happen: a path holds at most one new node per iteration)
  }
}

// ------------------------------------------------------------------ carry the subtree of node v
// What a search that keeps its tree does to a row whose new root is node v of the stored tree (the rule: include/mnk_hip.h,
// mnk_puct_rebase): the subtree of v stays, compacted in place to ids 0 .. kept - 1 in creation order, the first `keep` of
// its nodes; pos (LDS) = the new root's planes; the header says "pending, renew"; carried (optional) gets {kept, v's n}.
//   1. marking: a pass over the node records in chunks of 64.  A node is in the subtree when it is the new root or its
//      parent (info >> 18, always a lower id) is: parents of earlier chunks are read from the LDS table, parents inside
//      the chunk by pointer jumping over the lanes (at most 6 rounds).  The first `keep` marked nodes get new ids by a
//      ballot rank; map[old] = new id or NONE, inv[new] = old id, both in LDS (nodes + 1 entries each at the most).
//   2. the node records move in chunks of 64 new ids (every load of a chunk before its stores: lane j's destination j may
//      be a lower lane's source), the prior and child rows B nodes at a time, a cell per lane.  new <= old, and a
//      destination slot was itself moved or dropped before, so no second workspace is needed; a cell's column of the
//      prior and child rows is only ever touched by the one lane that owns the cell.
// Wave-uniform; returns kept (>= 1).  Shared by k_puct_rebase_leaves (v = where the match ended) and
// k_search_selfplay_advance_keep (v = the root's child through the move just played).
template <int NW, int B = 8>
__device__ __forceinline__ int puct_carry_subtree(int C, int NWg, unsigned char* row, const MnkPuctLayout& L,
                                                  const uint32_t* pos, int nodes, int v, int keep, int64_t i,
                                                  int32_t* carried, uint16_t* map, uint16_t* inv, int lane) {
  uint32_t* hdr = (uint32_t*)row;
  MnkPuctNode* node = (MnkPuctNode*)(row + L.node);
  float* prior = (float*)(row + L.prior);
  uint16_t* child = (uint16_t*)(row + L.child);
  const uint32_t root_n = node[v].n;

  // ---- 1. marking
  int cnt = 0;
  for (int base = 0; base < nodes; base += 64) {
    const int id = base + lane;
    const bool valid = id < nodes;
    int p = valid && id > 0 ? min((int)MNK_PUCT_PARENT(node[id].info), id - 1) : 0;
    bool in = id == v;
    bool known = !valid || id <= v;  // (a lower id is never in the subtree)
    if (!known && p < base) {
      in = map[p] != MNK_PUCT_NONE;
      known = true;
    }
    for (int r = 0; r < 6 && __ballot(!known); ++r) {
      const int from = known ? lane : p - base;
      const int fknown = __shfl((int)known, from, 64), fin = __shfl((int)in, from, 64), fp = __shfl(p, from, 64);
      if (!known) {
        if (fknown) {
          in = fin != 0;
          known = true;
        } else {
          p = fp;  // (the parent is neither the new root nor decided: the same answer as its own parent, in the chunk too)
        }
      }
    }
    in = in && known;
    const uint64_t marked = __ballot(in);
    const int rank = cnt + (int)__popcll(marked & ((1ull << lane) - 1ull));
    const bool kept = in && rank < keep;  // (a dropped node's descendants have higher ranks: dropped as well)
    if (valid) map[id] = kept ? (uint16_t)rank : (uint16_t)MNK_PUCT_NONE;
    if (kept) inv[rank] = (uint16_t)id;
    cnt += (int)__popcll(marked);
    row_wave_sync();
  }
  const int kept = min(cnt, keep);  // >= 1: the new root

  // ---- 2. compaction in place
  for (int base = 0; base < kept; base += 64) {
    const int j = base + lane;
    MnkPuctNode k;
    k.n = 0u; k.w = 0.0f; k.info = 0u;
    if (j < kept) k = node[inv[j]];
    row_wave_sync();
    if (j < kept) {
      const uint32_t up = map[min((int)MNK_PUCT_PARENT(k.info), nodes - 1)];  // (kept: the node is in the subtree)
      k.info = j ? ((k.info & 0x3FFFFu) | ((up == MNK_PUCT_NONE ? 0u : up) << 18)) : 0u;  // (the root: as a fresh one's)
      node[j] = k;
    }
  }
  for (int j0 = 0; j0 < kept; j0 += B) {
    for (int a = lane; a < C; a += 64) {
      float pr[B];
      uint32_t cl[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const int64_t o = (int64_t)inv[min(j0 + b, kept - 1)] * C + a;
        pr[b] = prior[o];
        cl[b] = child[o];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (j0 + b < kept) {
          uint32_t ch = cl[b];
          if (ch != 0u && ch != MNK_PUCT_NONE) {
            ch = map[min((int)ch, nodes - 1)];
            if (ch == MNK_PUCT_NONE) ch = 0u;  // a dropped child: none yet
          }
          const int64_t o = (int64_t)(j0 + b) * C + a;
          prior[o] = pr[b];
          child[o] = (uint16_t)ch;
        }
      }
    }
  }

  // ---- the new root as evaluation 0
  puct_row_root<NW>(row, L, pos, NWg, lane);
  if (lane == 0) {
    hdr[0] = (uint32_t)kept;
    hdr[1] = 0u;
    hdr[2] = 1u | 8u;  // pending, and only the priors of it are used
    hdr[3] = 1u;       // (a node that is not terminal has a legal cell)
    ((uint16_t*)(row + L.path))[0] = 0;
    if (carried) {
      carried[2 * i] = kept;
      carried[2 * i + 1] = (int32_t)root_n;
    }
  }
  return kept;
}
