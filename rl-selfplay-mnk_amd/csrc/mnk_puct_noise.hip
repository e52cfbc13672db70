// mnk_puct_noise.hip -- Dirichlet root noise for the PUCT search player (gfx950 / MI355X only): one launch between
// evaluation 0 and the first mnk_puct_step that mixes a Philox-keyed Dirichlet(alpha) draw over each root's free cells
// into a private f32 copy of the root's priors.  The rule: include/mnk_hip.h, mnk_puct_root_noise.
//
// One wave64 per row, four rows per 256-lane workgroup, cells strided over the lanes -- the shape of the kernels in
// mnk_puct.hip.  The kernel needs C and the mask only, no board geometry, so there is one generic kernel (no
// MNK_DISPATCH variants, no hiprtc kind).  The draw and the mix are puct_noise_row (mnk_puct_noise.h, where the notes on
// floating point are), shared with search self-play's per-row launch; a cell's log-gamma stays in the wave's own part of
// LDS between its two passes.  No scratch.
#include "mnk_puct_noise.h"

#define MNK_PUCT_NOISE_ROWS 4          // rows (waves) per 256-lane workgroup

__global__ __launch_bounds__(64 * MNK_PUCT_NOISE_ROWS) void k_puct_root_noise(
    const void* priors, int priors_dtype, const uint8_t* mask, int64_t N, int C, int leaves, double alpha, double d,
    double c, float eps, uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
    float* out) {
  extern __shared__ double noise_lds[];  // [MNK_PUCT_NOISE_ROWS][C]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * MNK_PUCT_NOISE_ROWS + wave;
  if (i >= N) return;
  if (seed_dev) seed = *seed_dev;
  if (step_dev) step += *step_dev;
  const int64_t base = i * leaves * C;  // the row's root: batch row i * leaves
  puct_noise_row(
      C, [&](int a) { return mask[base + a] != 0; }, [&](int a) { return noise_read(priors, priors_dtype, base + a); },
      [&](int a, float p) { out[base + a] = p; }, seed, (uint64_t)(env_id0 + i), step, alpha, d, c, eps,
      noise_lds + wave * C, lane);
}

extern "C" int mnk_puct_root_noise(const void* priors, int priors_dtype, const void* mask, int64_t N, int C, int leaves,
                                   float alpha, float eps, uint64_t seed, const uint64_t* seed_dev, uint64_t step,
                                   const uint64_t* step_dev, int64_t env_id0, float* out, void* stream) {
  if (!priors || !mask || !out || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_NOISE_ROWS || C < 1 ||
      C > MNK_PUCT_NOISE_CELLS_MAX || leaves < 1 || leaves > MNK_PUCT_LEAVES_MAX || !(alpha > 0.0f && alpha <= 3.0e38f) ||
      !(eps >= 0.0f && eps <= 1.0f) || (priors_dtype != MNK_LOGITS_F32 && priors_dtype != MNK_LOGITS_BF16))
    return MNK_EINVAL;
  if (!mnk_puct_noise_step_ok(step, C)) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const MnkPuctNoise q = mnk_puct_noise_params(alpha);
  const dim3 grid((unsigned)((N + MNK_PUCT_NOISE_ROWS - 1) / MNK_PUCT_NOISE_ROWS)), block(64 * MNK_PUCT_NOISE_ROWS);
  const size_t lds = (size_t)MNK_PUCT_NOISE_ROWS * C * sizeof(double);
  hipLaunchKernelGGL(k_puct_root_noise, grid, block, lds, (hipStream_t)stream, priors, priors_dtype, (const uint8_t*)mask,
                     N, C, leaves, q.alpha, q.d, q.c, eps, seed, seed_dev, step, step_dev, env_id0, out);
  return mnk_launch_status("puct_root_noise");
}
