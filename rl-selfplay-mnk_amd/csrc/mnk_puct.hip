// mnk_puct.hip -- the PUCT search player (gfx950 / MI355X only): AlphaZero-style search guided by a caller's evaluator
// (normally a policy/value network), batched over rows.  The tree lives in a device workspace between launches; each
// launch backs up the previous evaluation and selects the next leaf (mnk_puct_step), so an act() is mnk_puct_begin,
// I + 1 evaluator calls and I + 1 steps with no host synchronisation.  The rule: include/mnk_hip.h.
#include "mnk_host.h"
#include "mnk_wave_rows.h"

// One tree node (12 B).  w is from the view of the player who moved into the node.
struct MnkPuctNode {
  uint32_t n;
  float w;
  uint32_t info;  // the move into the node | term << 16 (0: not terminal; 1: the move won; 2: it filled the board)
};
static_assert(sizeof(MnkPuctNode) == 12, "node record");

// The workspace of one row, at row * L.row bytes (every part 16-byte aligned, the row 256-byte aligned):
//   header   u32[4]          nodes created, leaf depth, state (bit 0: a backup is pending; bits 1-2: the leaf's term),
//                            live (the root has a legal cell)
//   root     u32[2][NWg]     the root's guard-column bit planes (plane 0 = the root's side to move), NWg = MnkGeom::NW
//   leaf     u32[2][NWg]     the pending leaf's planes
//   path     u16[I + 2]      node ids root .. leaf
//   node     MnkPuctNode[I + 1]
//   prior    f32[I + 1][C]   the evaluator's prior of each legal cell of node v, at v * C (slot = node id)
//   child    u16[I + 1][C]   the child of node v through each cell: 0 = none yet (node 0, the root, is never a child),
//                            0xFFFF = an occupied cell
// About (I + 1) * 6 * C bytes per row.  The host (mnk_puct_workspace_bytes) and the kernels share this one function.
struct MnkPuctLayout {
  int64_t root, leaf, path, node, prior, child, row;
};
__host__ __device__ inline int64_t mnk_puct_al(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
__host__ __device__ inline MnkPuctLayout mnk_puct_layout(int NWg, int C, int I) {
  MnkPuctLayout L;
  L.root = 16;
  L.leaf = L.root + 8 * NWg;
  L.path = mnk_puct_al(L.leaf + 8 * NWg, 16);
  L.node = mnk_puct_al(L.path + 2 * (int64_t)(I + 2), 16);
  L.prior = mnk_puct_al(L.node + 12 * (int64_t)(I + 1), 16);
  L.child = mnk_puct_al(L.prior + 4 * (int64_t)(I + 1) * C, 16);
  L.row = mnk_puct_al(L.child + 2 * (int64_t)(I + 1) * C, 256);
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

// ------------------------------------------------------------------ evaluation 0: the roots
// One wave per row: the row into bit planes (LDS), the root node, the roots as the first leaves.
template <int NW, int CN, int CK>
__global__ void __launch_bounds__(256)
k_puct_begin(MnkGeom g, const void* obs, int obs_dtype, int64_t N, int I, unsigned char* ws, void* leaf_obs,
             int leaf_dtype, uint8_t* leaf_mask) {
  __shared__ uint32_t lds_pos[MNK_PUCT_ROWS][2 * NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_ROWS + wave;
  if (i >= N) return;
  const int C = g.C, NWg = g.NW;
  uint32_t* pos = lds_pos[wave];
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
  const MnkPuctLayout L = mnk_puct_layout(NWg, C, I);
  unsigned char* row = ws + i * L.row;
  uint32_t* root = (uint32_t*)(row + L.root);
  uint32_t* leaf = (uint32_t*)(row + L.leaf);
  for (int q = lane; q < 2 * NWg; q += 64) {
    const uint32_t v = pos[(q >= NWg) * NW + q - (q >= NWg ? NWg : 0)];
    root[q] = v;
    leaf[q] = v;
  }
  if (lane == 0) {
    uint32_t* hdr = (uint32_t*)row;
    hdr[0] = 1u;                     // the root
    hdr[1] = 0u;                     // the leaf is the root
    hdr[2] = 1u;                     // its evaluation is pending, not terminal
    hdr[3] = stones < C ? 1u : 0u;   // a legal cell
    ((uint16_t*)(row + L.path))[0] = 0;
    MnkPuctNode r;
    r.n = 0u; r.w = 0.0f; r.info = 0u;
    *(MnkPuctNode*)(row + L.node) = r;
  }
  row_write_view<NW, CN>(g, pos, 0, i, leaf_obs, leaf_dtype, leaf_mask, lane);
}

// ------------------------------------------------------------------ one backup, then one selection (or the move)
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
  if (state & 1u) {
    const int lf = min((int)path[depth], nodes - 1);
    const uint32_t term = (state >> 1) & 3u;
    float v;
    if (term) {
      v = term == 1u ? -1.0f : 0.0f;  // the mover into the leaf won: a loss for its side to move
    } else {
      v = puct_read(values, values_dtype, i);
      float* pr = prior + (int64_t)lf * C;
      uint16_t* cl = child + (int64_t)lf * C;
      for (int a = lane; a < C; a += 64) {
        const bool occ = row_stone<CN>(g, pos, a) || row_stone<CN>(g, pos + NW, a);
        cl[a] = occ ? (uint16_t)MNK_PUCT_NONE : (uint16_t)0;
        if (!occ) pr[a] = puct_read(priors, priors_dtype, i * C + a);
      }
    }
    for (int p = lane; p <= depth; p += 64) {  // depth - p odd: the mover into path[p] is the leaf's side to move
      MnkPuctNode* k = &node[min((int)path[p], nodes - 1)];
      k->n += 1u;
      k->w = __fadd_rn(k->w, ((depth - p) & 1) ? v : -v);
    }
    row_wave_sync();
  }

  if (last) {
    // ---- the move, the visits, the root value
    if (step_dev) step += *step_dev;
    if (seed_dev) seed = *seed_dev;
    const uint32_t x = deterministic ? 0u : mnk_rand_u32(seed, (uint64_t)(env_id0 + i), step, MNK_STREAM_SAMPLE);
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
    return;
  }

  // ---- selection
  int d = 0;
  uint32_t nstate = 0u;  // nothing pending: a row without a legal cell (or a full tree) shows its root again
  if (live && nodes <= I) {
    MnkEnv<NW> e;
    int stones = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      e.p[0][w] = w < NWg ? root[w] : 0u;
      e.p[1][w] = w < NWg ? root[NWg + w] : 0u;
      stones += __popc(e.p[0][w] | e.p[1][w]);
    }
    e.meta = (uint32_t)stones << 1;
    int v = 0;
    for (;;) {
      const float sq = puct_sqrt_rn(node[v].n);
      const float* pr = prior + (int64_t)v * C;
      const uint16_t* cl = child + (int64_t)v * C;
      float best = 0.0f;
      int ba = 0x7fffffff;
      for (int a = lane; a < C; a += 64) {
        const uint32_t ch = cl[a];
        if (ch == MNK_PUCT_NONE) continue;
        uint32_t na = 0u;
        float wa = 0.0f;
        if (ch) {
          const MnkPuctNode k = node[min((int)ch, nodes - 1)];
          na = k.n;
          wa = k.w;
        }
        const float q = na ? __fdiv_rn(wa, (float)na) : 0.0f;
        const float s = __fadd_rn(q, __fdiv_rn(__fmul_rn(__fmul_rn(c, pr[a]), sq), (float)(1u + na)));
        if (ba == 0x7fffffff || s > best) {  // (a rises: ">" keeps the lowest cell of a tie)
          best = s;
          ba = a;
        }
      }
#pragma unroll
      for (int off = 32; off; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(ba, off, 64);
        if (oa != 0x7fffffff && (ba == 0x7fffffff || ob > best || (ob == best && oa < ba))) {
          best = ob;
          ba = oa;
        }
      }
      const int a = __builtin_amdgcn_readfirstlane(ba);
      if (a == 0x7fffffff) break;  // (an evaluated non-terminal node always has a legal cell)
      const uint32_t ch = cl[a];
      const MnkPly ply = env_play<NW, CN, CK, true>(g, e, a, false);
      ++d;
      if (ch == 0u) {  // a new node: the leaf
        const uint32_t term = ply.win ? 1u : (ply.done ? 2u : 0u);
        if (lane == 0) {
          MnkPuctNode k;
          k.n = 0u; k.w = 0.0f; k.info = (uint32_t)a | (term << 16);
          node[nodes] = k;
          child[(int64_t)v * C + a] = (uint16_t)nodes;
          path[d] = (uint16_t)nodes;
        }
        ++nodes;
        nstate = 1u | (term << 1);
        break;
      }
      const int k = min((int)ch, nodes - 1);
      if (lane == 0) path[d] = (uint16_t)k;
      const uint32_t term = node[k].info >> 16;
      if (term) {  // an existing terminal child: the leaf again
        nstate = 1u | (term << 1);
        break;
      }
      v = k;
      if (d >= I) break;  // (cannot happen: a path holds at most one new node per iteration)
    }
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
extern "C" {

int64_t mnk_puct_workspace_bytes(int64_t N, int m, int n, int iterations) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, 1, &g);
  if (rc != MNK_OK) return rc;
  if (N < 0 || iterations < 1 || iterations > MNK_PUCT_ITERS_MAX) return MNK_EINVAL;
  return N * mnk_puct_layout(g.NW, g.C, iterations).row;
}

int mnk_puct_begin(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, void* workspace,
                   void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, void* stream) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  if (!obs || !workspace || !leaf_obs || !leaf_mask || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_ROWS || !mnk_obs_dtype_ok(obs_dtype) ||
      !mnk_obs_dtype_ok(leaf_dtype) || iterations < 1 || iterations > MNK_PUCT_ITERS_MAX)
    return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  hipStream_t s = (hipStream_t)stream;
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_begin), grid, block, 0, s, g, obs, obs_dtype, N, iterations,
                                     (unsigned char*)workspace, leaf_obs, leaf_dtype, leaf_mask));
  return mnk_launch_status("puct_begin");
}

int mnk_puct_step(void* workspace, int64_t N, int m, int n, int k, int iterations, const void* priors, int priors_dtype,
                  const void* values, int values_dtype, float c, int last, int temperature, uint64_t seed,
                  const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic,
                  void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions, int32_t* visits,
                  float* root_value, void* stream) {
  MnkGeom g;
  const int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  const bool dt_ok = (priors_dtype == MNK_LOGITS_F32 || priors_dtype == MNK_LOGITS_BF16) &&
                     (values_dtype == MNK_LOGITS_F32 || values_dtype == MNK_LOGITS_BF16);
  if (!workspace || !priors || !values || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_ROWS || !dt_ok || iterations < 1 ||
      iterations > MNK_PUCT_ITERS_MAX || !(c >= 0.0f && c <= 3.0e38f) || (last != 0 && last != 1) ||
      (temperature != 0 && temperature != 1))
    return MNK_EINVAL;
  if (last ? !actions : (!leaf_obs || !leaf_mask || !mnk_obs_dtype_ok(leaf_dtype))) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_ROWS - 1) / MNK_PUCT_ROWS)), block(64 * MNK_PUCT_ROWS);
  hipStream_t s = (hipStream_t)stream;
  MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_puct_step), grid, block, 0, s, g, (unsigned char*)workspace, N, iterations,
                                     priors, priors_dtype, values, values_dtype, c, last, temperature, seed, seed_dev,
                                     step, step_dev, env_id0, deterministic, leaf_obs, leaf_dtype, leaf_mask, actions,
                                     visits, root_value));
  return mnk_launch_status("puct_step");
}

}  // extern "C"
