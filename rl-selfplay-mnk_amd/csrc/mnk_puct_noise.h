// mnk_puct_noise.h -- the Dirichlet root noise of the PUCT search as device code shared by the kernels that draw it (the
// stand-alone launch, mnk_puct_noise.hip, and search self-play with per-row budgets, mnk_search_selfplay_async.hip): one
// wave draws one root's noise and mixes it into the root's priors.  The rule: include/mnk_hip.h, mnk_puct_root_noise.
//
// Floating point: f64 throughout up to eta, with the full-precision log / exp / cos / sqrt of the device library.  The
// library is built with -ffp-contract=off and without any fast-math option, and nothing may change that for a file that
// includes this one: an accept / reject comparison is only as reproducible as the logarithms on its two sides.
#pragma once
#include "mnk_host.h"

#define MNK_PUCT_NOISE_CELLS_MAX 1024  // 64 * MNK_MAX_W: no supported board has more cells than a plane has bits
static_assert(MNK_PUCT_NOISE_CELLS_MAX == 64 * MNK_MAX_W, "the cell range follows the packed planes");

// alpha widened to f64 and Marsaglia and Tsang's constants of shape alpha + 1: computed once on the host, so every
// kernel that draws gets the same three doubles
struct MnkPuctNoise {
  double alpha, d, c;
};
inline MnkPuctNoise mnk_puct_noise_params(float alpha) {
  MnkPuctNoise q;
  q.alpha = (double)alpha;
  q.d = q.alpha + 1.0 - 1.0 / 3.0;
  q.c = 1.0 / sqrt(9.0 * q.d);
  return q;
}
// the last Philox position of a draw at `step`, ((step + 1) * C4) * 16, must fit in the counter's 56 bits
inline bool mnk_puct_noise_step_ok(uint64_t step, int C) { return step < (1ull << 52) / (uint64_t)((C + 3) & ~3) - 1; }

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

// One root's noise, by one wave (cells strided over the lanes; every lane of the wave calls it): out(a, P'_a) for every
// cell a < C, where P'_a is the mix on the cells with is_free(a) and prior_of(a) elsewhere -- a root without a free cell
// is a plain copy.  Keyed by (seed, env, step).  ls: C doubles of the wave's own, in LDS: a cell's log-gamma stays there
// between the pass that draws it and the pass that normalises (each lane reads back only what it wrote: no barrier);
// maximum and sum are __shfl_xor reductions.
template <class Free, class Prior, class Out>
__device__ __forceinline__ void puct_noise_row(int C, Free is_free, Prior prior_of, Out out, uint64_t seed, uint64_t env,
                                               uint64_t step, double alpha, double d, double c, float eps, double* ls,
                                               int lane) {
  const uint64_t u_row = step * (uint64_t)((C + 3) & ~3);
  double mx = -INFINITY;
  bool any = false;
  for (int a = lane; a < C; a += 64) {
    if (is_free(a)) {
      const double l = noise_log_gamma(seed, env, (u_row + (uint64_t)a) * MNK_PUCT_NOISE_TRIES, alpha, d, c);
      ls[a] = l;
      mx = fmax(mx, l);
      any = true;
    }
  }
  if (!__any(any)) {  // no free cell: a plain copy
    for (int a = lane; a < C; a += 64) out(a, prior_of(a));
    return;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  double sum = 0.0;
  for (int a = lane; a < C; a += 64)
    if (is_free(a)) {
      const double e = exp(ls[a] - mx);
      ls[a] = e;
      sum += e;
    }
#pragma unroll
  for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off, 64);
  const float w = __fsub_rn(1.0f, eps);
  for (int a = lane; a < C; a += 64) {
    float p = prior_of(a);
    if (is_free(a)) p = __fadd_rn(__fmul_rn(w, p), __fmul_rn(eps, (float)(ls[a] / sum)));
    out(a, p);
  }
}
