// mnk_puct_gumbel.hip -- the Gumbel root of the PUCT search player (gfx950 / MI355X only): the table of considered visits
// that Sequential Halving follows (host only, no GPU), and one launch between evaluation 0 and the first
// mnk_puct_step_gumbel that draws one Philox-keyed Gumbel variable per free root cell and adds the cell's log prior.
// The rule: include/mnk_hip.h, mnk_puct_step_gumbel.
//
// One wave64 per row, four rows per 256-lane workgroup, cells strided over the lanes -- the shape of the kernels in
// mnk_puct.hip and of k_puct_root_noise.  The kernel needs C and the mask only, no board geometry, so there is one
// generic kernel (no MNK_DISPATCH variants, no hiprtc kind).  A cell is one Philox word, three logarithms and one store:
// no LDS, no reduction, no scratch.
//
// Floating point: f64 throughout with the full-precision log of the device library; the one rounding to f32 is the
// store.  The library is built with -ffp-contract=off and without any fast-math option, and nothing here may change that
// for this file.  There is no f32 transcendental in this translation unit.
#include "mnk_host.h"

#define MNK_PUCT_GUMBEL_ROWS 4          // rows (waves) per 256-lane workgroup
#define MNK_PUCT_GUMBEL_CELLS_MAX 1024  // 64 * MNK_MAX_W: no supported board has more cells than a plane has bits
static_assert(MNK_PUCT_GUMBEL_CELLS_MAX == 64 * MNK_MAX_W, "the cell range follows the packed planes");
static_assert(MNK_PUCT_CONSIDERED_MAX == MNK_PUCT_GUMBEL_CELLS_MAX, "a root never considers more moves than it has cells");

__device__ __forceinline__ float gumbel_read(const void* p, int dtype, int64_t q) {
  return dtype == MNK_LOGITS_BF16 ? __uint_as_float((uint32_t)((const uint16_t*)p)[q] << 16) : ((const float*)p)[q];
}

__global__ __launch_bounds__(64 * MNK_PUCT_GUMBEL_ROWS) void k_puct_gumbel_root(
    const void* priors, int priors_dtype, const uint8_t* mask, const void* values, int values_dtype, int64_t N, int C,
    double scale, uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
    float* gscore, float* vroot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_GUMBEL_ROWS + wave;
  if (i >= N) return;
  if (seed_dev) seed = *seed_dev;
  if (step_dev) step += *step_dev;
  const int64_t base = i * C;
  const uint64_t env = (uint64_t)(env_id0 + i);
  const uint64_t s_row = step * (uint64_t)((C + 3) & ~3);  // word a of the row: block s_row / 4 + (a >> 2), word a & 3
  for (int a = lane; a < C; a += 64) {
    float gs = -INFINITY;
    if (mask[base + a]) {
      const float p = gumbel_read(priors, priors_dtype, base + a);
      const double l = log((double)(p > 0x1p-126f ? p : 0x1p-126f));
      const double u = ((double)mnk_rand_u32(seed, env, s_row + (uint64_t)a, MNK_STREAM_GUMBEL) + 0.5) * 0x1p-32;
      const double g = -log(-log(u));  // (u is never 0 or 1: g is finite)
      gs = (float)(scale * g + l);
    }
    gscore[base + a] = gs;
  }
  if (lane == 0) vroot[i] = gumbel_read(values, values_dtype, i);
}

extern "C" {

int mnk_puct_gumbel_schedule(int considered, int iterations, uint16_t* out) {
  if (!out || considered < 1 || considered > MNK_PUCT_CONSIDERED_MAX || iterations < 1 || iterations > MNK_PUCT_ITERS_MAX)
    return MNK_EINVAL;
  const int I = iterations;
  uint16_t visits[MNK_PUCT_CONSIDERED_MAX];
  for (int mp = 0; mp <= considered; ++mp) {
    uint16_t* row = out + (size_t)mp * I;
    if (mp <= 1) {
      for (int t = 0; t < I; ++t) row[t] = (uint16_t)t;
      continue;
    }
    int l2 = 0;  // ceil(log2 mp)
    while ((1 << l2) < mp) ++l2;
    for (int j = 0; j < mp; ++j) visits[j] = 0;
    int len = 0;
    for (int nc = mp; len < I; nc = nc / 2 > 2 ? nc / 2 : 2) {
      const int extra = I / (l2 * nc) > 1 ? I / (l2 * nc) : 1;
      for (int e = 0; e < extra && len < I; ++e) {
        for (int j = 0; j < nc && len < I; ++j) row[len++] = visits[j];
        for (int j = 0; j < nc; ++j) ++visits[j];  // (at most once per nc entries appended: below I)
      }
    }
  }
  return MNK_OK;
}

int mnk_puct_gumbel_root(const void* priors, int priors_dtype, const void* mask, const void* values, int values_dtype,
                         int64_t N, int C, float gumbel_scale, uint64_t seed, const uint64_t* seed_dev, uint64_t step,
                         const uint64_t* step_dev, int64_t env_id0, float* gscore, float* vroot, void* stream) {
  const bool dt_ok = (priors_dtype == MNK_LOGITS_F32 || priors_dtype == MNK_LOGITS_BF16) &&
                     (values_dtype == MNK_LOGITS_F32 || values_dtype == MNK_LOGITS_BF16);
  if (!priors || !mask || !values || !gscore || !vroot || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_GUMBEL_ROWS ||
      C < 1 || C > MNK_PUCT_GUMBEL_CELLS_MAX || !(gumbel_scale >= 0.0f && gumbel_scale <= 3.0e38f) || !dt_ok)
    return MNK_EINVAL;
  // the last Philox position of the call, (step + 1) * C4 / 4, must fit in the counter's 56 bits
  if (step >= (1ull << 56) / (uint64_t)((C + 3) & ~3) - 1) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const dim3 grid((unsigned)((N + MNK_PUCT_GUMBEL_ROWS - 1) / MNK_PUCT_GUMBEL_ROWS)), block(64 * MNK_PUCT_GUMBEL_ROWS);
  hipLaunchKernelGGL(k_puct_gumbel_root, grid, block, 0, (hipStream_t)stream, priors, priors_dtype, (const uint8_t*)mask,
                     values, values_dtype, N, C, (double)gumbel_scale, seed, seed_dev, step, step_dev, env_id0, gscore,
                     vroot);
  return mnk_launch_status("puct_gumbel_root");
}

}  // extern "C"
