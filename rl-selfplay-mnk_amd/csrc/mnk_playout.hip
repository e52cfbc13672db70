// mnk_playout.hip -- the flat Monte Carlo player (gfx950 / MI355X only): for every legal cell of a canonical observation,
// P uniformly random playouts to the end of the game, and the move among the cells of best win-minus-loss count
// (mnk_sample_playouts).  The rule: include/mnk_hip.h.  The playouts reuse the rollout's building blocks: env_play
// (whole-plane win test) and env_pick_legal (mnk_device.h), Philox stream MNK_STREAM_PLAYOUT.
#include "mnk_host.h"

// ------------------------------------------------------------------ the kernel
// One workgroup per row.
//   phase 1: the row is packed into the guard-column bit planes in LDS (one element load per cell, atomicOr per stone);
//   phase 2: the lanes share the |L| * P playouts, item e = (cell L[e / P], playout e % P).  A lane holds one game in
//            registers and plays one ply per loop iteration; a lane whose game has ended takes its next item at the next
//            iteration that is a multiple of 4, so every live lane is at the same t mod 4 and the Philox block of four
//            plies (every 4th ply) is drawn by the whole wave at once.  Results go to per-cell LDS counters (LDS atomics);
//   phase 3: wave 0 reduces the maximal score over the legal cells, counts S and picks its r-th cell with ballots.
// Dynamic LDS: u32 wins[C], losses[C].
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_sample_playouts(MnkGeom g, const void* obs, int obs_dtype, int64_t N, int P, uint64_t seed, const uint64_t* seed_dev,
                  uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic, int64_t* actions,
                  int32_t* counts) {
  extern __shared__ uint32_t lds_cnt[];  // [2][C]
  __shared__ uint32_t lds_plane[2][NW];
  const int64_t i = blockIdx.x;
  const int tid = threadIdx.x, NT = blockDim.x;
  if (step_dev) step += *step_dev;
  if (seed_dev) seed = *seed_dev;
  const int n = geom_n<CN>(g), C = g.C;
  const uint64_t env = (uint64_t)(env_id0 + i);

  // ---- phase 1: counters to zero, the row into bit planes
  for (int c = tid; c < 2 * C; c += NT) lds_cnt[c] = 0u;
  if (tid < 2 * NW) lds_plane[tid / NW][tid % NW] = 0u;
  __syncthreads();
  {
    const size_t eb = (size_t)mnk_obs_bytes(obs_dtype);
    const unsigned char* row = (const unsigned char*)obs + (size_t)i * 2 * C * eb;
    for (int c = tid; c < 2 * C; c += NT) {
      uint32_t v;
      if (obs_dtype == MNK_OBS_F32) v = ((const uint32_t*)row)[c] << 1;  // (+0.0 and -0.0 are empty)
      else if (obs_dtype == MNK_OBS_BF16) v = (uint32_t)((const uint16_t*)row)[c] << 17;
      else v = row[c];
      if (v) {
        const int pl = c >= C, cell = c - (pl ? C : 0);
        const int bit = cell + cell / n;  // row * (n + 1) + col
        atomicOr(&lds_plane[pl][bit >> 5], 1u << (bit & 31));
      }
    }
  }
  __syncthreads();

  // ---- phase 2: the playouts
  int stones = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) stones += __popc(lds_plane[0][w] | lds_plane[1][w]);
  const int total = (C - stones) * P;  // |L| * P
  const int C4 = (C + 3) & ~3;
  int item = tid, cell = 0, t = 0;
  bool live = false;
  uint64_t q0 = 0;
  MnkEnv<NW> e;
  env_clear<NW>(e);
  Philox4 blk;
  blk.v[0] = blk.v[1] = blk.v[2] = blk.v[3] = 0u;
  for (int it = 0;; ++it) {
    if ((it & 3) == 0) {
      if (!live && item < total) {  // the next item: the root position, "me" (plane 0, side bit 0) to move
        const int li = item / P, j = item - li * P;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          e.p[0][w] = lds_plane[0][w];
          e.p[1][w] = lds_plane[1][w];
        }
        e.meta = (uint32_t)stones << 1;
        uint32_t legal[NW];  // (rebuilt per item from the root rather than held across the loop: NW fewer VGPRs)
        env_legal<NW>(g, e, legal);
        const uint32_t bit = (uint32_t)bs_select<NW>(legal, li);
        cell = mnk_bit_cell<CN>(g, bit);
        q0 = ((((uint64_t)step * (uint64_t)C + (uint64_t)cell) * (uint64_t)P + (uint64_t)j) * (uint64_t)C4) >> 2;
        t = -1;  // ply -1: "me" plays the cell
        live = true;
        item += NT;
      }
      if (!__any(live)) break;  // (a lane that is not live here has no item left)
    }
    if (live) {
      if ((t & 3) == 0) blk = mnk_rng_block(seed, env, q0 + (uint64_t)(t >> 2), MNK_STREAM_PLAYOUT);  // (wave-uniform)
      const int pick = env_pick_legal<NW, CN>(g, e, philox_word(blk, (uint32_t)t & 3u));
      const MnkPly ply = env_play<NW, CN, CK, true>(g, e, t < 0 ? cell : pick, false);
      if (ply.done) {
        // the mover of ply t: "me" for t = -1 and odd t, the other side for even t
        if (ply.win) atomicAdd(&lds_cnt[(t & 1) ? cell : C + cell], 1u);
        live = false;
      }
      ++t;
    }
  }
  __syncthreads();

  // ---- phase 3: the move, and the counts
  if (tid < 64) {
    const int lane = tid;
    // (from the LDS planes: a lane's `legal` words cannot be indexed by a run-time word number without scratch)
    auto empty = [&](int c) {
      const int bit = c + c / n;
      return ((~(lds_plane[0][bit >> 5] | lds_plane[1][bit >> 5]) >> (bit & 31)) & 1u) != 0u;
    };
    int best = -0x7fffffff;
    for (int c = lane; c < C; c += 64) {
      if (empty(c)) {
        const int s = (int)lds_cnt[c] - (int)lds_cnt[C + c];
        best = s > best ? s : best;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(best, off, 64);
      best = o > best ? o : best;
    }
    // |S|, then its r-th cell in action order, 64 cells per ballot
    int ns = 0;
    for (int c0 = 0; c0 < C; c0 += 64) {
      const int c = c0 + lane;
      const bool in = c < C && empty(c) && (int)lds_cnt[c] - (int)lds_cnt[C + c] == best;
      ns += __popcll(__ballot(in));
    }
    const uint32_t x = deterministic ? 0u : mnk_rand_u32(seed, env, step, MNK_STREAM_SAMPLE);
    int r = (int)__umulhi(x, (uint32_t)(ns ? ns : C));
    if (ns == 0) {
      if (lane == 0) actions[i] = r;  // no legal cell: the draw is over all C cells
    } else {
      const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
      for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < C && empty(c) && (int)lds_cnt[c] - (int)lds_cnt[C + c] == best;
        const uint64_t mask = __ballot(in);
        const int cnt = __popcll(mask);
        if (r < cnt) {
          if (in && __popcll(mask & below) == r) actions[i] = c;
          break;
        }
        r -= cnt;
      }
    }
  }
  if (counts) {
    int32_t* out = counts + i * 2 * C;
    for (int c = tid; c < 2 * C; c += NT) out[c] = (int32_t)lds_cnt[c];
  }
}

// ------------------------------------------------------------------ the entry point
extern "C" {

int mnk_sample_playouts(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int playouts, uint64_t seed,
                        const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                        int deterministic, int64_t* actions, int32_t* counts, void* stream) {
  MnkGeom g;
  int rc = mnk_sample_check(obs, obs_dtype, N, m, n, k, actions, &g);
  if (rc != MNK_OK) return rc;
  if (playouts < 1 || playouts > MNK_PLAYOUTS_MAX) return MNK_EINVAL;
  rc = mnk_rows_games_check(step, (uint64_t)g.C * (uint64_t)playouts, g.C, N);  // (C * P games)
  if (rc != MNK_OK || N == 0) return rc;
  const dim3 grid((unsigned)N), block(256);
  const size_t lds = (size_t)2 * g.C * sizeof(uint32_t);
  hipStream_t s = (hipStream_t)stream;
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_sample_playouts), grid, block, lds, s, g, obs, obs_dtype, N, playouts, seed,
                                     seed_dev, step, step_dev, env_id0, deterministic, actions, counts));
  return mnk_launch_status("sample_playouts");
}

}  // extern "C"
