// mnk_puct_noise.hip -- Dirichlet root noise for the PUCT search player (gfx950 / MI355X only): one launch between
// evaluation 0 and the first mnk_puct_step that mixes a Philox-keyed Dirichlet(alpha) draw over each root's free cells
// into a private f32 copy of the root's priors.  The rule: include/mnk_hip.h, mnk_puct_root_noise.
//
// One wave64 per row, four rows per 256-lane workgroup, cells strided over the lanes -- the shape of the kernels in
// mnk_puct.hip.  The kernel needs C and the mask only, no board geometry, so there is one generic kernel (no
// MNK_DISPATCH variants, no hiprtc kind).  A cell's log-gamma stays in the wave's own part of LDS between the pass that
// draws it and the pass that normalises (each lane reads back only what it wrote: no barrier); maximum and sum are
// __shfl_xor reductions.  No scratch.
//
// Floating point: f64 throughout up to eta, with the full-precision log / exp / cos / sqrt of the device library.  The
// library is built with -ffp-contract=off and without any fast-math option, and nothing here may change that for this
// file: an accept / reject comparison is only as reproducible as the logarithms on its two sides.
#include "mnk_host.h"

#define MNK_PUCT_NOISE_ROWS 4          // rows (waves) per 256-lane workgroup
#define MNK_PUCT_NOISE_CELLS_MAX 1024  // 64 * MNK_MAX_W: no supported board has more cells than a plane has bits
static_assert(MNK_PUCT_NOISE_CELLS_MAX == 64 * MNK_MAX_W, "the cell range follows the packed planes");

__device__ __forceinline__ float noise_read(const void* p, int dtype, int64_t q) {
  return dtype == MNK_LOGITS_BF16 ? __uint_as_float((uint32_t)((const uint16_t*)p)[q] << 16) : ((const float*)p)[q];
}

__device__ __forceinline__ double noise_u01(uint32_t x) { return ((double)x + 0.5) * 0x1p-32; }  // never 0 or 1

// ln of a Gamma(alpha) variate for cell `a`: Marsaglia-Tsang at shape alpha + 1 (d = alpha + 1 - 1/3, c = 1 / sqrt(9 d)),
// at most MNK_PUCT_NOISE_TRIES candidates of one Philox block each, then the boost U^(1 / alpha) in log space
__device__ __forceinline__ double noise_log_gamma(uint64_t seed, uint64_t env, uint64_t u0, double alpha, double d,
                                                  double c) {
  double l = 0.0;
  for (int t = 0; t < MNK_PUCT_NOISE_TRIES; ++t) {
    const Philox4 b = mnk_rng_block(seed, env, u0 + (uint64_t)t, MNK_STREAM_NOISE);
    const double U0 = noise_u01(b.v[0]), U1 = noise_u01(b.v[1]), U2 = noise_u01(b.v[2]), U3 = noise_u01(b.v[3]);
    const double z = sqrt(-2.0 * log(U0)) * cos(6.283185307179586 * U1);
    const double s = 1.0 + c * z;
    const double v = s * s * s;
    if (v > 0.0 && log(U2) < 0.5 * z * z + d - d * v + d * log(v)) {
      l = log(d * v) + log(U3) / alpha;
      break;
    }
    if (t == MNK_PUCT_NOISE_TRIES - 1) l = log(d) + log(U3) / alpha;  // (acceptance is above 0.95 per try: unreachable)
  }
  return l;
}

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
  const uint64_t env = (uint64_t)(env_id0 + i);
  const uint64_t u_row = step * (uint64_t)((C + 3) & ~3);
  double* ls = noise_lds + wave * C;

  double mx = -INFINITY;
  bool any = false;
  for (int a = lane; a < C; a += 64) {
    if (mask[base + a]) {
      const double l = noise_log_gamma(seed, env, (u_row + (uint64_t)a) * MNK_PUCT_NOISE_TRIES, alpha, d, c);
      ls[a] = l;
      mx = fmax(mx, l);
      any = true;
    }
  }
  if (!__any(any)) {  // no free cell: a plain copy
    for (int a = lane; a < C; a += 64) out[base + a] = noise_read(priors, priors_dtype, base + a);
    return;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  double sum = 0.0;
  for (int a = lane; a < C; a += 64)
    if (mask[base + a]) {
      const double e = exp(ls[a] - mx);
      ls[a] = e;
      sum += e;
    }
#pragma unroll
  for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off, 64);
  const float w = __fsub_rn(1.0f, eps);
  for (int a = lane; a < C; a += 64) {
    float p = noise_read(priors, priors_dtype, base + a);
    if (mask[base + a]) p = __fadd_rn(__fmul_rn(w, p), __fmul_rn(eps, (float)(ls[a] / sum)));
    out[base + a] = p;
  }
}

extern "C" int mnk_puct_root_noise(const void* priors, int priors_dtype, const void* mask, int64_t N, int C, int leaves,
                                   float alpha, float eps, uint64_t seed, const uint64_t* seed_dev, uint64_t step,
                                   const uint64_t* step_dev, int64_t env_id0, float* out, void* stream) {
  if (!priors || !mask || !out || N < 0 || N > (int64_t)0x7fffffff * MNK_PUCT_NOISE_ROWS || C < 1 ||
      C > MNK_PUCT_NOISE_CELLS_MAX || leaves < 1 || leaves > MNK_PUCT_LEAVES_MAX || !(alpha > 0.0f && alpha <= 3.0e38f) ||
      !(eps >= 0.0f && eps <= 1.0f) || (priors_dtype != MNK_LOGITS_F32 && priors_dtype != MNK_LOGITS_BF16))
    return MNK_EINVAL;
  // the last Philox position of the call, ((step + 1) * C4) * 16, must fit in the counter's 56 bits
  if (step >= (1ull << 52) / (uint64_t)((C + 3) & ~3) - 1) return MNK_EINVAL;
  if (N == 0) return MNK_OK;
  const double a64 = (double)alpha, d = a64 + 1.0 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  const dim3 grid((unsigned)((N + MNK_PUCT_NOISE_ROWS - 1) / MNK_PUCT_NOISE_ROWS)), block(64 * MNK_PUCT_NOISE_ROWS);
  const size_t lds = (size_t)MNK_PUCT_NOISE_ROWS * C * sizeof(double);
  hipLaunchKernelGGL(k_puct_root_noise, grid, block, lds, (hipStream_t)stream, priors, priors_dtype, (const uint8_t*)mask,
                     N, C, leaves, a64, d, c, eps, seed, seed_dev, step, step_dev, env_id0, out);
  return mnk_launch_status("puct_root_noise");
}
