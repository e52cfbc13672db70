// mnk_tactical.hip -- the one-ply tactical player (take a win, else block one, else play at random; gfx950 / MI355X only):
// the self-play step with it as the opponent in one launch (mnk_selfplay_step_tactical) and the player as a policy on a
// canonical observation (mnk_sample_tactical).  The rule: include/mnk_hip.h; the device code: mnk_plane_completions /
// env_pick_tactical (mnk_device.h), k_selfplay_step_tactical / k_sample_tactical (mnk_selfplay_kernels.h).
#include "mnk_selfplay_host.h"

extern "C" {

int mnk_selfplay_step_tactical(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, const int64_t* actions,
                               uint8_t* pending, int64_t* agent_side, const int64_t* forced_side, uint64_t seed,
                               uint64_t step, const uint64_t* step_dev, int64_t env_id0, float* rewards,
                               uint8_t* terminated, void* obs, int obs_dtype, uint8_t* legal_mask, uint64_t* packed_obs,
                               int32_t* err, float* ep_return, int32_t* ep_length, int64_t* ep_stats, uint32_t flags,
                               void* stream) {
  MnkSpArgs a;
  const int rc = mnk_sp_args_step(&a, planes, meta, N, m, n, k, pending, agent_side, forced_side, seed, step, step_dev,
                                  env_id0, rewards, terminated, obs, obs_dtype, legal_mask, packed_obs, err, ep_return,
                                  ep_length, ep_stats, flags);
  return mnk_sp_step<MNK_SP_STEP_TACTICAL>(rc, a, actions, stream, "selfplay_step_tactical");
}

int mnk_sample_tactical(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, uint64_t seed,
                        const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic,
                        int64_t* actions, uint8_t* candidates, void* stream) {
  MnkGeom g;
  const int rc = mnk_sample_check(obs, obs_dtype, N, m, n, k, actions, &g);
  if (rc != MNK_OK) return rc;
  if (N == 0) return MNK_OK;
  const int B = 64;
  const dim3 grid((unsigned)((N + B - 1) / B));
  hipStream_t s = (hipStream_t)stream;
  if (hipFunction_t fn = mnk_jit_api_function(g, MNK_JK_SAMPLE_TACTICAL, N, s))
    mnk_module_launch(&k_sample_tactical<2, 0, 0>, fn, grid, dim3(B), 0, s, g, obs, obs_dtype, N, seed, seed_dev, step, step_dev,
                      env_id0, deterministic, actions, candidates);
  else
    MNK_DISPATCH(g, hipLaunchKernelGGL(MNK_K(k_sample_tactical), grid, dim3(B), 0, s, g, obs, obs_dtype, N, seed, seed_dev, step,
                                       step_dev, env_id0, deterministic, actions, candidates));
  return mnk_launch_status("sample_tactical");
}

}  // extern "C"
