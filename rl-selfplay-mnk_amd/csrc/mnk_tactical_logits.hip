// mnk_tactical_logits.hip -- mnk_selfplay_step_tactical with the AGENT's masked draw folded in (gfx950 / MI355X only): a
// network agent against the one-ply tactical opponent is ONE launch per agent-step after the forward, as against the
// uniformly random one (mnk_selfplay_step_logits.hip).  A unit of its own so that its 15 kernel variants -- five boards x
// {f32, bf16, no logits} -- compile in parallel with the rest of the library.
#include "mnk_selfplay_draw.h"

extern "C" int mnk_selfplay_step_tactical_logits(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                                 const void* logits, int logits_dtype, const uint8_t* mask, uint64_t sample_seed,
                                                 const uint64_t* sample_seed_dev, uint64_t sample_step,
                                                 const uint64_t* sample_step_dev, int64_t sample_env_id0, int deterministic,
                                                 int64_t* actions, float* logp, uint8_t* pending, int64_t* agent_side,
                                                 const int64_t* forced_side, uint64_t seed, uint64_t step,
                                                 const uint64_t* step_dev, int64_t env_id0, float* rewards, uint8_t* terminated,
                                                 void* obs, int obs_dtype, uint8_t* legal_mask, uint64_t* packed_obs,
                                                 int32_t* err, float* ep_return, int32_t* ep_length, int64_t* ep_stats,
                                                 uint32_t flags, void* stream) {
  MnkSpArgs a;
  const int rc = mnk_sp_args_step(&a, planes, meta, N, m, n, k, pending, agent_side, forced_side, seed, step, step_dev,
                                  env_id0, rewards, terminated, obs, obs_dtype, legal_mask, packed_obs, err, ep_return,
                                  ep_length, ep_stats, flags);
  const MnkSample sa = {logits, logits_dtype, mask, sample_seed, sample_seed_dev, sample_step, sample_step_dev, sample_env_id0,
                        deterministic, actions, logp};
  return mnk_sp_step_logits<MNK_SP_STEP_TACTICAL>(rc, a, sa, stream, "selfplay_step_tactical_logits", [&] {
    return mnk_selfplay_step_tactical(planes, meta, N, m, n, k, actions, pending, agent_side, forced_side, seed, step, step_dev,
                                      env_id0, rewards, terminated, obs, obs_dtype, legal_mask, packed_obs, err, ep_return,
                                      ep_length, ep_stats, flags, stream);
  });
}
