// mnk_rollout_log.hip -- the fused random rollout with the action log switched on (gfx950 / MI355X only):
// the variants the multi-GPU exchange uses.  Its own translation unit so it compiles beside mnk_rollout.hip.
#include "mnk_host.h"
#include "mnk_rollout_lane.h"

void mnk_launch_rollout_log(const MnkGeom& g, uint64_t* planes, uint32_t* meta, int64_t N, int T, uint64_t seed,
                            uint64_t step0, int64_t env_id0, uint64_t* rec_planes, uint32_t* rec_meta, int64_t* stats,
                            void* act_log, int act_bytes, void* stream) {
  const int B = 64;
  const dim3 grid((unsigned)((N + B - 1) / B));
  const bool rec = rec_planes && rec_meta;
  // compile-time boards, records on, one wave per SIMD: 32-bit lane offsets for the record stores (see mnk_rollout.hip)
  // (each board has the log widths mnk_act_format_ok allows for its cell count: 9x9 and 3x3 the 7-bit stream, 19x19 U8P1)
  if (rec && mnk_rollout_saddr_ok(g, N, T)) {
#define MNK_SADDR(ACTB)                                                                                                  \
  if constexpr (mnk_act_format_ok(ACTB, MnkRow_::C))                                                                     \
    if (act_bytes == ACTB)                                                                                               \
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rollout_random<NW, CN, CK, true, ACTB, true>), grid, dim3(B), 0,              \
                         (hipStream_t)stream, g, planes, meta, N, T, seed, step0, env_id0, rec_planes, rec_meta,         \
                         (unsigned long long*)stats, act_log);
    const bool fixed = MNK_BUILTIN(g, true, MNK_SADDR(1) MNK_SADDR(2) MNK_SADDR(3) MNK_SADDR(4));
#undef MNK_SADDR
    if (fixed) return;
  }
  // U8P1: boards of more than 256 cells (19x19 and the generic 16-word form); the 7-bit stream: boards of at most 128 cells
  // (9x9, 3x3 and generic boards of up to 8 register words, e.g. 11x11 = 121 cells, NW 5)
#define MNK_ROLLOUT(DISPATCH, REC, ACTB)                                                                           \
  DISPATCH(g, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rollout_random<NW, CN, CK, REC, ACTB>), grid, dim3(B), 0,       \
                                 (hipStream_t)stream, g, planes, meta, N, T, seed, step0, env_id0, rec_planes,     \
                                 rec_meta, (unsigned long long*)stats, act_log))
  if (act_bytes == MNK_ACT_U8P1) {
    if (rec) MNK_ROLLOUT(MNK_DISPATCH16_LARGE, true, 4);
    else MNK_ROLLOUT(MNK_DISPATCH16_LARGE, false, 4);
  } else if (act_bytes == MNK_ACT_BITS7) {
    if (rec) MNK_ROLLOUT(MNK_DISPATCH_SMALL, true, 3);
    else MNK_ROLLOUT(MNK_DISPATCH_SMALL, false, 3);
  } else if (rec && act_bytes == 1) MNK_ROLLOUT(MNK_DISPATCH16, true, 1);
  else if (rec) MNK_ROLLOUT(MNK_DISPATCH16, true, 2);
  else if (act_bytes == 1) MNK_ROLLOUT(MNK_DISPATCH16, false, 1);
  else MNK_ROLLOUT(MNK_DISPATCH16, false, 2);
#undef MNK_ROLLOUT
}
