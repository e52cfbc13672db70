// mnk_search_selfplay.hip -- search self-play (gfx950 / MI355X only): the env side of an AlphaZero loop.  One launch per
// ply turns the root visit counts of a search (PUCTSearchPolicy.act(visits=...)) into a move, records the position and the
// visits in a ring, labels every record of a finished game with its outcome, resets finished games and writes the next
// roots (mnk_search_selfplay_step); a second kernel expands a minibatch of ring records into network inputs and targets
// under the board's symmetries (mnk_search_gather).  The rules: include/mnk_hip.h.
#include "mnk_host.h"
#include "mnk_wave_rows.h"

#define MNK_SSP_ROWS 4  // rows (waves) per 256-lane workgroup of the step
#define MNK_SSP_GATHER_MAX_ENVS 128  // the largest samples-per-workgroup mnk_block_envs hands out

// ------------------------------------------------------------------ one ply of every row
// One wave per row: the position in registers and (canonical, channel 0 = the side to move) in LDS, the C-wide reads of
// the row's visits and writes of its ring visits row-contiguous over the lanes.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_search_selfplay_step(MnkGeom g, uint64_t* planes, uint32_t* meta, int64_t N, const int32_t* visits, int temp_plies,
                       uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                       int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* obs, int obs_dtype,
                       uint8_t* legal_mask, unsigned long long* stats, int32_t* err) {
  __shared__ uint32_t lds_pos[MNK_SSP_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_SSP_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, W = g.W;
  uint32_t* pos = lds_pos[wave];
  MnkEnv<NW> e;
  env_load<NW>(e, planes, meta, N, W, i);
  if (step_dev) step += *step_dev;
  if (seed_dev) seed = *seed_dev;
  const int64_t t = (int64_t)(step % (uint64_t)T);
  const uint32_t x = mnk_rand_u32(seed, (uint64_t)(env_id0 + i), step, MNK_STREAM_SELFPLAY);
  const uint32_t side = e.meta & 1u, moves = e.meta >> 1;
  uint32_t mine[NW], theirs[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    mine[w] = side ? e.p[1][w] : e.p[0][w];
    theirs[w] = side ? e.p[0][w] : e.p[1][w];
  }
  if (lane == 0) {
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      pos[w] = mine[w];
      pos[NW + w] = theirs[w];
    }
  }
  row_wave_sync();

  // ---- the visits of the free cells (clamped to [0, 65535]) into ring row t, their maximum and sum
  const int32_t* vrow = visits + i * C;
  uint16_t* rv = ring_visits + (t * N + i) * C;
  uint32_t maxn = 0u, tot = 0u;
  for (int a = lane; a < C; a += 64) {
    const bool occ = row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a);
    const int32_t v = vrow[a];
    const uint32_t na = (occ || v <= 0) ? 0u : min((uint32_t)v, 65535u);
    rv[a] = (uint16_t)na;
    maxn = max(maxn, na);
    tot += na;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, off, 64));
    tot += (uint32_t)__shfl_xor((int)tot, off, 64);
  }
  if (lane == 0) {
    uint64_t* rp = ring_planes + t * 2 * W * N;
    plane_store<NW>(mine, rp, N, W, i);
    plane_store<NW>(theirs, rp + (int64_t)W * N, N, W, i);
  }

  // ---- the move (a lane reads back only the ring visits it wrote itself), the ply, the outcome labels
  MnkPly ply;
  ply.win = false; ply.done = false; ply.err = 0;
  if (maxn) {
    int move = 0;
    mnk_pick_by_visits(C, x, (int64_t)moves < (int64_t)temp_plies, maxn, tot, lane,
                       [&](int a) { return a < C ? (uint32_t)rv[a] : 0u; }, move);
    ply = env_play<NW, CN, CK, true>(g, e, move, false);
  } else if (lane == 0) {
    mnk_report(err, MNK_ERR_VISITS, i);  // the env is left as it is; its record carries no outcome
  }
  if (lane == 0) ring_z[t * N + i] = ply.done ? (int8_t)(ply.win ? 1 : 0) : (int8_t)MNK_Z_UNKNOWN;
  if (ply.done) {
    // records t - d (mod T), d = 1 .. L - 1, of this game: the view of the side to move there; T >= C >= L
    const int64_t L = min((int64_t)moves + 1, T);
    const int8_t zw = ply.win ? 1 : 0;
    for (int64_t d = 1 + lane; d < L; d += 64) {
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
  if (maxn && lane == 0) env_store<NW>(e, planes, meta, N, W, i);

  // ---- the next root
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
  row_write_view<NW, CN, true>(g, pos, 0, i, obs, obs_dtype, legal_mask, lane);
}

// mnk_search_selfplay_step with the move given and the improved policy as the ring's visits (the rule: include/mnk_hip.h,
// mnk_search_selfplay_step_moves).  A kernel of its own, not a flag on the one above: what follows the move -- the ply, the
// outcome labels, the statistics, the reset, the next root -- is that kernel's text, kept apart so that its code objects
// stay what they were.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_search_selfplay_step_moves(MnkGeom g, uint64_t* planes, uint32_t* meta, int64_t N, const float* policy,
                             const int64_t* actions, uint64_t step, const uint64_t* step_dev, int64_t T,
                             uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* obs, int obs_dtype,
                             uint8_t* legal_mask, unsigned long long* stats, int32_t* err) {
  __shared__ uint32_t lds_pos[MNK_SSP_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_SSP_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, W = g.W;
  uint32_t* pos = lds_pos[wave];
  MnkEnv<NW> e;
  env_load<NW>(e, planes, meta, N, W, i);
  if (step_dev) step += *step_dev;
  const int64_t t = (int64_t)(step % (uint64_t)T);
  const uint32_t side = e.meta & 1u, moves = e.meta >> 1;
  uint32_t mine[NW], theirs[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    mine[w] = side ? e.p[1][w] : e.p[0][w];
    theirs[w] = side ? e.p[0][w] : e.p[1][w];
  }
  if (lane == 0) {
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      pos[w] = mine[w];
      pos[NW + w] = theirs[w];
    }
  }
  row_wave_sync();

  // ---- the policy of the free cells, scaled to 65535, into ring row t; is the action a free cell?
  const float* prow = policy + i * C;
  uint16_t* rv = ring_visits + (t * N + i) * C;
  for (int a = lane; a < C; a += 64) {
    const bool occ = row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a);
    const float v = rintf(__fmul_rn(prow[a], 65535.0f));
    rv[a] = (occ || !(v > 0.0f)) ? (uint16_t)0 : (uint16_t)fminf(v, 65535.0f);
  }
  const int64_t act = actions[i];
  const bool in_range = act >= 0 && act < C;
  const int move = in_range ? (int)act : 0;
  const bool playable = in_range && !(row_stone<CN>(g, pos, move) || row_stone<CN>(g, pos + NW, move));
  if (lane == 0) {
    uint64_t* rp = ring_planes + t * 2 * W * N;
    plane_store<NW>(mine, rp, N, W, i);
    plane_store<NW>(theirs, rp + (int64_t)W * N, N, W, i);
  }

  // ---- the ply, the outcome labels
  MnkPly ply;
  ply.win = false; ply.done = false; ply.err = 0;
  if (playable) {
    ply = env_play<NW, CN, CK, true>(g, e, move, false);
  } else if (lane == 0) {  // the env is left as it is; its record carries no outcome
    mnk_report(err, in_range ? MNK_ERR_ILLEGAL_MOVE : MNK_ERR_ACTION_RANGE, i);
  }
  if (lane == 0) ring_z[t * N + i] = ply.done ? (int8_t)(ply.win ? 1 : 0) : (int8_t)MNK_Z_UNKNOWN;
  if (ply.done) {
    // records t - d (mod T), d = 1 .. L - 1, of this game: the view of the side to move there; T >= C >= L
    const int64_t L = min((int64_t)moves + 1, T);
    const int8_t zw = ply.win ? 1 : 0;
    for (int64_t d = 1 + lane; d < L; d += 64) {
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
  if (playable && lane == 0) env_store<NW>(e, planes, meta, N, W, i);

  // ---- the next root
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
  row_write_view<NW, CN, true>(g, pos, 0, i, obs, obs_dtype, legal_mask, lane);
}

// ------------------------------------------------------------------ a minibatch of ring records under symmetries
// symmetry s of a board of m rows, n columns: the source cell of output cell (r, c)
__device__ __forceinline__ void mnk_sym_src(int s, int m, int n, int& r, int& c) {
  if (s & 4) {
    const int q = r;
    r = c;
    c = q;
  }
  if (s & 1) r = m - 1 - r;
  if (s & 2) c = n - 1 - c;
}

// k_gather_obs with a symmetry per sample and the search targets: one lane per sample fetches its planes into the LDS
// stage, maps them through its symmetry there (a bit at a time, the output words in registers), and the workgroup writes
// its slab of observations and masks with the write-out of the env's kernels (mnk_write_out), then its slab of policy
// targets.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_search_gather(MnkGeom g, const uint64_t* ring_planes, const uint16_t* ring_visits, const int8_t* ring_z, int64_t T,
                int64_t N, const int64_t* idx, const int8_t* sym, int64_t B_total, void* obs, int obs_dtype,
                uint8_t* legal_mask, float* policy, float* value, float* weight, int32_t* err, int vec_ok,
                int envs_per_block) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ int64_t lds_src[MNK_SSP_GATHER_MAX_ENVS];
  __shared__ uint32_t lds_sum[MNK_SSP_GATHER_MAX_ENVS];
  __shared__ int lds_sym[MNK_SSP_GATHER_MAX_ENVS];
  const int B = envs_per_block, NT = blockDim.x, tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * B;
  const int64_t j = row0 + tid;
  const bool mine = tid < B && j < B_total;
  const bool emit = obs || legal_mask;
  MnkStage st = mnk_stage_carve(lds_raw, g, B);
  if (emit) mnk_stage_tables<CN>(st, g, B, tid, NT);
  uint32_t p0[NW], p1[NW];
  int s = 0;
  if (mine) {
    int64_t flat = idx[j];
    if (flat < 0) flat += T * N;
    const bool in_range = flat >= 0 && flat < T * N;
    const int sj = sym ? (int)sym[j] : 0;
    const bool sym_ok = sj >= 0 && sj < 8 && (sj < 4 || g.m == g.n);
    s = sym_ok ? sj : 0;
    float v = 0.0f, wt = 0.0f;
    uint32_t sum = 0u;
    if (!in_range) {
      mnk_report(err, MNK_ERR_ACTION_RANGE, idx[j]);
#pragma unroll
      for (int w = 0; w < NW; ++w) p0[w] = p1[w] = 0u;
    } else {
      if (!sym_ok) mnk_report(err, MNK_ERR_SYMMETRY, j);
      const int64_t t = flat / N, i = flat - t * N;
      const uint64_t* base = ring_planes + t * 2 * g.W * N;
      plane_load<NW>(p0, base, N, g.W, i);
      plane_load<NW>(p1, base + (int64_t)g.W * N, N, g.W, i);
      if (policy) {
        const uint16_t* rv = ring_visits + flat * g.C;
        for (int a = 0; a < g.C; ++a) sum += rv[a];
      }
      const int z = ring_z[flat];
      if (z != MNK_Z_UNKNOWN) {
        v = (float)z;
        wt = sym_ok ? 1.0f : 0.0f;
      }
    }
    if (value) value[j] = v;
    if (weight) weight[j] = wt;
    lds_src[tid] = in_range ? flat : -1;
    lds_sum[tid] = sum;
    lds_sym[tid] = s;
  }
  if (emit) {
    if (mine) mnk_stage_put<NW>(st, g, B, tid, p0, p1, false);
    __syncthreads();  // the source planes are staged
    if (mine && s) {
      const int S = mnk_stage_stride(B), m = g.m, n = geom_n<CN>(g);
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        uint32_t o0 = 0u, o1 = 0u;
        if (w < g.NW) {
          for (int b = 0; b < 32; ++b) {
            const uint32_t bit = (uint32_t)(32 * w + b);
            int r = (int)mnk_div(bit, g.magic_stride), c = (int)bit - r * (n + 1);
            if (c >= n || r >= m) continue;
            mnk_sym_src(s, m, n, r, c);
            const uint32_t sb = (uint32_t)(r * (n + 1) + c);
            o0 |= ((st.words[(sb >> 5) * S + tid] >> (sb & 31u)) & 1u) << b;
            o1 |= ((st.words[(g.NW + (sb >> 5)) * S + tid] >> (sb & 31u)) & 1u) << b;
          }
        }
        p0[w] = o0;
        p1[w] = o1;
      }
    }
    __syncthreads();  // every lane has read its source
    if (mine && s) mnk_stage_put<NW>(st, g, B, tid, p0, p1, false);
    const int64_t left = B_total - row0;
    const int nb = left < B ? (int)left : B;
    mnk_write_out<NW, CN, CK>(st, g, B, nb, mnk_obs_slab(obs, obs_dtype, row0, g.C), obs_dtype,
                              legal_mask ? legal_mask + row0 * g.C : nullptr, vec_ok, tid, NT);
  }
  if (!policy) return;  // (workgroup-uniform)
  __syncthreads();
  const int64_t left = B_total - row0;
  const uint32_t C = (uint32_t)g.C, n = (uint32_t)geom_n<CN>(g);
  const uint32_t total = (uint32_t)(left < B ? left : B) * C;
  float* out = policy + row0 * g.C;
  for (uint32_t q = tid; q < total; q += NT) {
    const uint32_t el = mnk_div(q, g.magic_C), a = q - el * C;
    const int64_t src = lds_src[el];
    const uint32_t sum = lds_sum[el];
    float v = 0.0f;
    if (src >= 0 && sum) {
      int r = (int)mnk_div(a, g.magic_n), c = (int)(a - (uint32_t)r * n);
      mnk_sym_src(lds_sym[el], g.m, (int)n, r, c);
      v = __fdiv_rn((float)ring_visits[src * g.C + r * (int)n + c], (float)sum);
    }
    out[q] = v;
  }
}

// ------------------------------------------------------------------ the entry points
extern "C" {

int mnk_search_selfplay_step(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, const int32_t* visits,
                             int temp_plies, uint64_t seed, const uint64_t* seed_dev, uint64_t step,
                             const uint64_t* step_dev, int64_t env_id0, int64_t T, uint64_t* ring_planes,
                             uint16_t* ring_visits, int8_t* ring_z, void* obs, int obs_dtype, uint8_t* legal_mask,
                             int64_t* stats, int32_t* err, void* stream) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  if (!planes || !meta || !visits || !ring_planes || !ring_visits || !ring_z || !obs || N < 0 ||
      N > (int64_t)0x7fffffff * MNK_SSP_ROWS || T < g.C || temp_plies < 0 || !mnk_obs_dtype_ok(obs_dtype))
    return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_SSP_ROWS - 1) / MNK_SSP_ROWS)), block(64 * MNK_SSP_ROWS);
  hipStream_t s = (hipStream_t)stream;
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_search_selfplay_step), grid, block, 0, s, g, planes, meta, N, visits,
                                     temp_plies, seed, seed_dev, step, step_dev, env_id0, T, ring_planes, ring_visits,
                                     ring_z, obs, obs_dtype, legal_mask, (unsigned long long*)stats, err));
  return mnk_launch_status("search_selfplay_step");
}

int mnk_search_selfplay_step_moves(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, const float* policy,
                                   const int64_t* actions, uint64_t step, const uint64_t* step_dev, int64_t T,
                                   uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* obs, int obs_dtype,
                                   uint8_t* legal_mask, int64_t* stats, int32_t* err, void* stream) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  if (!planes || !meta || !policy || !actions || !ring_planes || !ring_visits || !ring_z || !obs || N < 0 ||
      N > (int64_t)0x7fffffff * MNK_SSP_ROWS || T < g.C || !mnk_obs_dtype_ok(obs_dtype))
    return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_SSP_ROWS - 1) / MNK_SSP_ROWS)), block(64 * MNK_SSP_ROWS);
  hipStream_t s = (hipStream_t)stream;
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_search_selfplay_step_moves), grid, block, 0, s, g, planes, meta, N, policy,
                                     actions, step, step_dev, T, ring_planes, ring_visits, ring_z, obs, obs_dtype,
                                     legal_mask, (unsigned long long*)stats, err));
  return mnk_launch_status("search_selfplay_step_moves");
}

int mnk_search_gather(const uint64_t* ring_planes, const uint16_t* ring_visits, const int8_t* ring_z, int64_t T,
                      int64_t N, int m, int n, const int64_t* idx, const int8_t* sym, int64_t B, void* obs, int obs_dtype,
                      uint8_t* legal_mask, float* policy, float* value, float* weight, int32_t* err, void* stream) {
  MnkGeom g;
  const int rc = mnk_geom_any_k(m, n, &g);
  if (rc != MNK_OK) return rc;
  if (!ring_planes || !ring_visits || !ring_z || T < 0 || N < 0 || B < 0 || B > 0x7fffffff || (B > 0 && !idx) ||
      !mnk_obs_dtype_ok(obs_dtype))
    return MNK_EINVAL;
  if (B == 0) return MNK_OK;
  const int E = mnk_block_envs(B);
  if (E > MNK_SSP_GATHER_MAX_ENVS) return MNK_EINVAL;
  const int vec_ok = (aligned16(obs) ? 1 : 0) | (aligned16(legal_mask) ? 2 : 0);
  const dim3 grid((unsigned)((B + E - 1) / E));
  const size_t lds = mnk_stage_bytes(g.NW, g.C, E, g.n, mnk_geom_packed(g.n, g.k, g.NW, g.C));
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_search_gather), grid, dim3(mnk_block_threads()), lds, (hipStream_t)stream, g,
                                     ring_planes, ring_visits, ring_z, T, N, idx, sym, B, obs, obs_dtype, legal_mask,
                                     policy, value, weight, err, vec_ok, E));
  return mnk_launch_status("search_gather");
}

}  // extern "C"
