// mnk_search.hip -- the tree-search player (gfx950 / MI355X only): UCT over a canonical observation, I iterations of
// selection, expansion, B random playouts from the leaf and backup, inside one launch, one workgroup per row; the move
// is a root child of maximal visit count (mnk_sample_search).  The rule: include/mnk_hip.h.  The playouts reuse the
// rollout's building blocks: env_play (whole-plane win test) and env_pick_legal (mnk_device.h), Philox stream
// MNK_STREAM_SEARCH.
#include "mnk_host.h"

// One tree node in LDS (24 B).  Children of a node form a singly linked list in DESCENDING action order (a new child is
// expanded at a higher action index than its siblings and is prepended), so a scan with ">=" keeps the lowest index.
struct MnkSearchNode {
  uint16_t move;   // the cell played into this node (root: unused)
  uint16_t first;  // first child (0 = none: node 0 is the root, never a child)
  uint16_t next;   // next sibling
  uint16_t nexp;   // children expanded so far: the next one is the nexp-th legal cell of this node's position
  uint32_t n, w, lo;  // visits; wins and losses from the view of the player who moved into this node
  uint32_t term;   // 0: not terminal; 1: the move won for its mover; 2: the move filled the board without a win
};
static_assert(sizeof(MnkSearchNode) == 24, "node record");

// ------------------------------------------------------------------ the kernel
// One workgroup per row, 64 * ceil(B / 64) lanes.
//   setup:     the row into the guard-column bit planes in LDS, the root node;
//   iteration: wave 0 walks from the root with the position in (wave-uniform) registers, expands the first untried
//              cell of the first node that has one, or descends to the child of maximal UCT score; writes the path
//              (node ids) and the leaf's depth to LDS.                                                 -- barrier 1
//              lanes j < B rebuild the leaf position from the root planes plus the path's moves and play one random
//              game each; the two win counts are reduced by ballot, one LDS atomic per wave.           -- barrier 2
//              wave 0 backs the counts up along the path, lane p taking path nodes p, p + 64, ...  The next
//              selection runs on the same wave, so a wave-scope fence replaces a third barrier.
//   the move:  lane 0 walks the root's children (max n, |S|, the r-th of S) and writes the stats.
// Dynamic LDS: MnkSearchNode node[I + 1], then uint16_t path[min(I, C) + 2].
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_sample_search(MnkGeom g, const void* obs, int obs_dtype, int64_t N, int I, int B, float c, uint64_t seed,
                const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic,
                int64_t* actions, int32_t* stats) {
  extern __shared__ __align__(16) unsigned char lds_dyn[];
  MnkSearchNode* node = (MnkSearchNode*)lds_dyn;
  uint16_t* path = (uint16_t*)(node + I + 1);
  __shared__ uint32_t lds_plane[2][NW];
  __shared__ uint32_t lds_won[2];  // playouts won by "me" (plane 0), by the other side (plane 1)
  __shared__ int lds_depth;        // the leaf's depth (path[0..depth]); -1 - depth when the leaf is terminal
  const int64_t i = blockIdx.x;
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
  if (step_dev) step += *step_dev;
  if (seed_dev) seed = *seed_dev;
  const int n = geom_n<CN>(g), C = g.C;
  const uint64_t env = (uint64_t)(env_id0 + i);

  // ---- setup
  if (tid < 2 * NW) lds_plane[tid / NW][tid % NW] = 0u;
  if (tid < 2) lds_won[tid] = 0u;
  if (tid == 0) {
    MnkSearchNode r;
    r.move = 0; r.first = 0; r.next = 0; r.nexp = 0;
    r.n = 0u; r.w = 0u; r.lo = 0u; r.term = 0u;
    node[0] = r;
  }
  __syncthreads();
  {
    const size_t eb = (size_t)mnk_obs_bytes(obs_dtype);
    const unsigned char* row = (const unsigned char*)obs + (size_t)i * 2 * C * eb;
    for (int q = tid; q < 2 * C; q += NT) {
      uint32_t v;
      if (obs_dtype == MNK_OBS_F32) v = ((const uint32_t*)row)[q] << 1;  // (+0.0 and -0.0 are empty)
      else if (obs_dtype == MNK_OBS_BF16) v = (uint32_t)((const uint16_t*)row)[q] << 17;
      else v = row[q];
      if (v) {
        const int pl = q >= C, cell = q - (pl ? C : 0);
        const int bit = cell + cell / n;  // row * (n + 1) + col
        atomicOr(&lds_plane[pl][bit >> 5], 1u << (bit & 31));
      }
    }
  }
  __syncthreads();
  int stones = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) stones += __popc(lds_plane[0][w] | lds_plane[1][w]);
  const int C4 = (C + 3) & ~3;
  const uint32_t ub = (uint32_t)B;

  // ---- the iterations (none on a full board: the move is then drawn over all C cells)
  int nodes = 1;  // (wave 0 only)
  for (int it = 0; stones < C && it < I; ++it) {
    if (tid < 64) {
      // selection / expansion, wave-uniform
      MnkEnv<NW> e;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        e.p[0][w] = lds_plane[0][w];
        e.p[1][w] = lds_plane[1][w];
      }
      e.meta = (uint32_t)stones << 1;
      int v = 0, d = 0;
      bool terminal = false;
      for (;;) {
        const MnkSearchNode nv = node[v];
        if (nv.term) {
          terminal = true;
          break;
        }
        if ((int)nv.nexp < C - stones - d) {  // an untried legal cell: expand it
          uint32_t legal[NW];
          env_legal<NW>(g, e, legal);
          const uint32_t bit = (uint32_t)bs_select<NW>(legal, (int)nv.nexp);
          const int cell = mnk_bit_cell<CN>(g, bit);
          const MnkPly ply = env_play<NW, CN, CK, true>(g, e, cell, false);
          const int ch = nodes++;
          if (lane == 0) {
            MnkSearchNode k;
            k.move = (uint16_t)cell; k.first = 0; k.next = nv.first; k.nexp = 0;
            k.n = 0u; k.w = 0u; k.lo = 0u; k.term = ply.win ? 1u : (ply.done ? 2u : 0u);
            node[ch] = k;
            node[v].first = (uint16_t)ch;
            node[v].nexp = (uint16_t)(nv.nexp + 1);
            path[d + 1] = (uint16_t)ch;
          }
          ++d;
          terminal = ply.done;
          break;
        }
        // every legal cell is a child: the child of maximal q + c * sqrt(n_v / n_child), ties to the lowest cell
        const float fnv = (float)nv.n;
        float best = 0.0f;
        int bc = 0;
        bool any = false;
        for (int ch = nv.first; ch; ) {
          const MnkSearchNode k = node[ch];
          const float fn = (float)k.n;
          const float q = __fdiv_rn((float)((int)k.w - (int)k.lo), fn);
          const float s = __fadd_rn(q, __fmul_rn(c, __fsqrt_rn(__fdiv_rn(fnv, fn))));
          if (!any || s >= best) {
            best = s;
            bc = ch;
            any = true;
          }
          ch = k.next;
        }
        v = bc;
        env_play<NW, CN, CK, true>(g, e, node[v].move, false);
        ++d;
        if (lane == 0) path[d] = (uint16_t)v;
      }
      if (lane == 0) {
        path[0] = 0;
        lds_depth = terminal ? -1 - d : d;
      }
    }
    __syncthreads();  // barrier 1: the path is published

    const int dd = lds_depth;
    const int depth = dd < 0 ? -1 - dd : dd;
    if (dd >= 0 && tid < B) {
      // one random game from the leaf
      MnkEnv<NW> e;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        e.p[0][w] = lds_plane[0][w];
        e.p[1][w] = lds_plane[1][w];
      }
      for (int p = 1; p <= depth; ++p) {  // depth p odd: "me" (plane 0) moved into path[p]
        const int cell = node[path[p]].move;
        const uint32_t bit = mnk_cell_bit<CN>(g, (uint32_t)cell);
        const uint32_t one = 1u << (bit & 31u);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const uint32_t add = (w == (int)(bit >> 5)) ? one : 0u;
          e.p[0][w] |= (p & 1) ? add : 0u;
          e.p[1][w] |= (p & 1) ? 0u : add;
        }
      }
      e.meta = ((uint32_t)(stones + depth) << 1) | (uint32_t)(depth & 1);
      const uint64_t q0 = ((((uint64_t)step * (uint64_t)I + (uint64_t)it) * (uint64_t)B + (uint64_t)tid) *
                           (uint64_t)C4) >> 2;
      Philox4 blk;
      blk.v[0] = blk.v[1] = blk.v[2] = blk.v[3] = 0u;
      int outcome = 0;  // 1: "me" won, 2: the other side won, 0: a draw
      for (int t = 0;; ++t) {
        if ((t & 3) == 0) blk = mnk_rng_block(seed, env, q0 + (uint64_t)(t >> 2), MNK_STREAM_SEARCH);
        const int pick = env_pick_legal<NW, CN>(g, e, philox_word(blk, (uint32_t)t & 3u));
        const int mover = (int)(e.meta & 1u);
        const MnkPly ply = env_play<NW, CN, CK, true>(g, e, pick, false);
        if (ply.done) {
          outcome = ply.win ? 1 + mover : 0;
          break;
        }
      }
      const uint64_t won_me = __ballot(outcome == 1), won_other = __ballot(outcome == 2);
      if (lane == 0) {
        if (won_me) atomicAdd(&lds_won[0], (uint32_t)__popcll(won_me));
        if (won_other) atomicAdd(&lds_won[1], (uint32_t)__popcll(won_other));
      }
    }
    __syncthreads();  // barrier 2: the counts are in

    if (tid < 64) {
      uint32_t wm, wo;  // the B outcomes: wins of "me", wins of the other side
      if (dd >= 0) {
        wm = lds_won[0];
        wo = lds_won[1];
      } else {           // a terminal leaf: its outcome B times
        const uint32_t won = node[path[depth]].term == 1u ? ub : 0u;
        wm = (depth & 1) ? won : 0u;
        wo = (depth & 1) ? 0u : won;
      }
      for (int p = lane; p <= depth; p += 64) {  // the mover into a node of odd depth is "me"
        MnkSearchNode* k = &node[path[p]];
        k->n += ub;
        k->w += (p & 1) ? wm : wo;
        k->lo += (p & 1) ? wo : wm;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (lane == 0) lds_won[0] = lds_won[1] = 0u;  // (read above by this wave only; the next adds follow barrier 1)
    }
  }

  // ---- the move, and the stats
  int32_t* out = stats ? stats + i * 3 * C : nullptr;
  if (out)
    for (int q = tid; q < 3 * C; q += NT) out[q] = 0;
  __syncthreads();
  if (tid == 0) {
    uint32_t maxn = 0u;
    int ns = 0;
    for (int ch = node[0].first; ch; ch = node[ch].next) {
      const uint32_t nc = node[ch].n;
      ns = nc > maxn ? 1 : ns + (nc == maxn);
      maxn = nc > maxn ? nc : maxn;
    }
    const uint32_t x = deterministic ? 0u : mnk_rand_u32(seed, env, step, MNK_STREAM_SAMPLE);
    const int r = (int)__umulhi(x, (uint32_t)(ns ? ns : C));
    if (ns == 0) actions[i] = r;  // no legal cell: the draw is over all C cells
    int from_top = ns - 1 - r;    // (the list runs in descending action order)
    for (int ch = node[0].first; ch; ch = node[ch].next) {
      const MnkSearchNode k = node[ch];
      if (k.n == maxn && from_top-- == 0) actions[i] = k.move;
      if (out) {
        out[k.move] = (int32_t)k.n;
        out[C + k.move] = (int32_t)k.w;
        out[2 * C + k.move] = (int32_t)k.lo;
      }
    }
  }
}

// ------------------------------------------------------------------ the entry point
extern "C" {

int mnk_sample_search(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, int playouts,
                      float c, uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev,
                      int64_t env_id0, int deterministic, int64_t* actions, int32_t* stats, void* stream) {
  MnkGeom g;
  int rc = mnk_sample_check(obs, obs_dtype, N, m, n, k, actions, &g);
  if (rc != MNK_OK) return rc;
  if (iterations < 1 || iterations > MNK_SEARCH_ITERS_MAX) return MNK_EINVAL;
  if (playouts < 1 || playouts > MNK_SEARCH_PLAYOUTS_MAX) return MNK_EINVAL;
  if (!(c >= 0.0f && c <= 3.0e38f)) return MNK_EINVAL;  // (finite and not negative; NaN fails both)
  rc = mnk_rows_games_check(step, (uint64_t)iterations * (uint64_t)playouts, g.C, N);  // (I * B games)
  if (rc != MNK_OK || N == 0) return rc;
  const dim3 grid((unsigned)N), block((unsigned)(64 * ((playouts + 63) / 64)));
  const int depth_max = iterations < g.C ? iterations : g.C;
  const size_t lds = (size_t)(iterations + 1) * sizeof(MnkSearchNode) + (size_t)(depth_max + 2) * sizeof(uint16_t);
  hipStream_t s = (hipStream_t)stream;
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_sample_search), grid, block, lds, s, g, obs, obs_dtype, N, iterations,
                                     playouts, c, seed, seed_dev, step, step_dev, env_id0, deterministic, actions, stats));
  return mnk_launch_status("sample_search");
}

}  // extern "C"
