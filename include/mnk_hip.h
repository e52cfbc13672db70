/*
 * mnk_hip.h -- C ABI of libmnk_hip.so, the MI355X (gfx950) implementation of the
 * vectorized MNK self-play rollout path.
 *
 * The reference (michal-szadkowski/rl-selfplay-mnk) has no FFI layer: its boundary
 * is the duck-typed Python surface of TorchVectorMnkEnv / TorchSelfPlayWrapper.
 * The Python classes in rl-selfplay-mnk_amd/{env,selfplay}/ keep that surface and
 * call the functions below through ctypes; every entry point cites the reference
 * code it replaces (paths relative to the reference's src/).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name says host; buffers are owned
 *     by the caller (torch tensors on the Python side) and must be contiguous;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every function only enqueues work on it: no allocation, no synchronisation,
 *     no host<->device copy, so all of them may be captured into a hipGraph;
 *   - return value: MNK_OK (0) or a negative MNK_E* code for an argument error that
 *     was detected on the host (nothing is enqueued then);
 *   - data-dependent errors (action out of range, illegal move in strict mode) are
 *     recorded on the device in `err` = int32[2] {code, global env id}; first error
 *     wins, the word is sticky until the caller clears it.  The offending env is
 *     left untouched, all other envs proceed;
 *   - single writer per state buffer: calls that touch the same state must be
 *     ordered on one stream (or by events).  No global mutable state in the library.
 *
 * Packed state:
 *   planes  u64[2][W][N]   plane 0 = black, 1 = white; cell (r,c) is bit r*(n+1)+c of the
 *                          W-word little-endian bit string; column n of each row is a
 *                          guard column that is always 0;  W = mnk_state_words(m, n)
 *   meta    u32[N]         bit 0 = side to move (0 black, 1 white), bits 1..31 = move count
 *
 * Rollout record of one position (what mnk_rollout_random / mnk_replay_actions write per ply):
 *   rows    u64[R][N]      row w = (32-bit word w of the MOVER's plane) | (word w of the other side's plane) << 32,
 *                          same bit numbering as above; R = mnk_record_words(m, n) = ceil(m*(n+1)/32).
 *                          Which colour the mover is says MNK_REC_SIDE_BIT of the ply's meta word (0 = black).
 *                          This is the view the policy sees (channel 0 = own stones, wrapper.py:99-106).
 *                          No padding at any board size: 24 B at 9x9 where two state planes take 32 B --
 *                          the rollout is bound by these stores.
 */
#ifndef MNK_HIP_H
#define MNK_HIP_H

#ifndef __HIPCC_RTC__ /* hiprtc (the run-time specialisation of the rollout kernel) has no libc headers */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MNK_ABI_VERSION 6

/* status codes (host-side argument checks) */
#define MNK_OK 0
#define MNK_EINVAL -1   /* null pointer / negative size */
#define MNK_EGEOM -2    /* unsupported board geometry (see mnk_geometry_supported) */
#define MNK_ELAUNCH -3  /* hipLaunchKernel failed (hipGetLastError text via mnk_last_launch_error) */
#define MNK_ECOMM -4    /* an RCCL call failed or librccl could not be resolved (text via mnk_comm_last_error) */

/* device-side error codes written to err[0] */
#define MNK_ERR_NONE 0
#define MNK_ERR_ACTION_RANGE 1 /* action outside [-m*n, m*n): the reference raises IndexError (env/torch_vector_mnk_env.py:68) */
#define MNK_ERR_ILLEGAL_MOVE 2 /* strict mode only: occupied cell, message of env/torch_vector_mnk_env.py:102-104 */
#define MNK_ERR_SYMMETRY 3     /* mnk_search_gather: a symmetry id outside [0, 8), or >= 4 on a board that is not square */
#define MNK_ERR_VISITS 4       /* mnk_search_selfplay_step: a row without a positive visit count on a free cell */

/* flags for mnk_step and the mnk_selfplay_* functions */
#define MNK_STEP_STRICT 1u /* refuse moves onto occupied cells (the behaviour tests/test_mnk_integration.py:68-81 expects) */
#define MNK_STEP_AUTORESET 2u /* mnk_step, full batch only: an env whose game this ply finished is reset in the same launch
                               * (env.reset(nonzero(done)), env/torch_vector_mnk_env.py:34-44) and the legal mask / observation
                               * written are those of the fresh board -- the raw loop "step; reset(done); observe" in one launch */

/* element type of the observations a kernel writes (`obs_dtype` next to every `obs` pointer).  A cell is exactly
 * 0 or 1, so every narrowing is lossless: obs.float() of a narrow observation equals the f32 one bit for bit.
 * F32 is what the reference hands out (env/torch_vector_mnk_env.py:17, :52); BF16 is what its first convolution
 * computes in under alg/ppo.py:194 autocast (utils/hardware.py:38-41) -- the cast the caller does today is a separate
 * elementwise kernel over 648 B/env; U8 is 0/1 bytes.  Halves / quarters the dominant bytes of every API kernel. */
#define MNK_OBS_F32 0
#define MNK_OBS_BF16 1
#define MNK_OBS_U8 2

/* element type of the logits handed to mnk_sample_logits */
#define MNK_LOGITS_F32 0
#define MNK_LOGITS_BF16 1 /* what the reference's networks emit under alg/ppo.py:194 autocast on Ampere+ (utils/hardware.py:38-41) */

/* format of the action log (`act_bytes` of mnk_rollout_random / mnk_replay_actions / mnk_jit_compile_rollout) */
#define MNK_ACT_U8 1    /* one byte per action, boards of at most 256 cells: u32[ceil(T/4)][N] */
#define MNK_ACT_U16 2   /* 16 bits per action: u64[ceil(T/4)][N] */
#define MNK_ACT_BITS7 3 /* 7 bits per action, boards of at most 128 cells: a bit stream, ply p at bit 7p, in u32 words
                         * [mnk_action_log_words(MNK_ACT_BITS7, T)][N] -- 0.875 B per env-step, what the ranks of
                         * BASELINE.json configs 2-4 (9x9: 81 cells) put on xGMI */

#define MNK_ACT_U8P1 4  /* 9 bits per action, boards of 257 to 512 cells (19x19: 361; larger boards take MNK_ACT_U16): the low bytes as in MNK_ACT_U8,
                         * u32[ceil(T/4)][N], followed by a bit plane of bit 8 of every action, ply p at bit p % 32 of
                         * word [ceil(T/4) + p / 32][i], u32[ceil(T/32)][N] -- 1.125 B per env-step where MNK_ACT_U16 takes 2
                         * (BASELINE.json config 5's exchange) */

/* bytes of the opaque communicator id exchanged between ranks (= NCCL_UNIQUE_ID_BYTES) */
#define MNK_COMM_ID_BYTES 128

/* flags written by mnk_selfplay_pre for mnk_selfplay_post (u8 per env) */
#define MNK_SP_NEED_OPP 1u
#define MNK_SP_WAS_RESET 2u

/* rollout record meta word (u32 per env-step) */
#define MNK_REC_ACTION_MASK 0xFFFFu
#define MNK_REC_REWARD_SHIFT 16 /* i8 */
#define MNK_REC_DONE_BIT 24
#define MNK_REC_SIDE_BIT 25

/* rollout statistics: int64[MNK_STATS_REPLICAS][MNK_STATS_STRIDE]; a counter's value is the sum of
 * its replicas (column j of every row).  Replication keeps thousands of waves from serialising
 * their atomic adds on one address. */
#define MNK_STATS_REPLICAS 64
#define MNK_STATS_STRIDE 8
#define MNK_STATS_COUNTERS 5 /* episodes finished, black wins, white wins, draws, sum of episode lengths */

/* Philox streams (oracle/philox.py restates the generator) */
#define MNK_STREAM_MOVE 0
#define MNK_STREAM_OPP 1
#define MNK_STREAM_SIDE 2
#define MNK_STREAM_SAMPLE 3
#define MNK_STREAM_PLAYOUT 4 /* the random plies of the Monte Carlo player's playouts (mnk_sample_playouts) */
#define MNK_STREAM_SEARCH 5  /* the random plies of the tree-search player's playouts (mnk_sample_search) */
#define MNK_STREAM_SELFPLAY 6 /* the move of a search self-play ply (mnk_search_selfplay_step) */
#define MNK_STREAM_NOISE 7    /* the Dirichlet noise on the PUCT player's root priors (mnk_puct_root_noise) */
#define MNK_STREAM_GUMBEL 8   /* the Gumbel variables of the PUCT player's Gumbel root (mnk_puct_gumbel_root) */
#define MNK_STREAM_BUDGET 9   /* is a self-play ply searched with the full budget? (mnk_search_selfplay_advance) */

int mnk_abi_version(void);
/* Developer knobs (MNK_ROLLOUT_PAIR, MNK_ROLLOUT_FORM, MNK_JIT, MNK_ROLLOUT_SADDR, MNK_EMIT_ENVS, MNK_EMIT_THREADS: A/B
 * timing and parity tests of every kernel form) are read from the environment once, at the first call that needs them;
 * this reads them again.  Not meant to race with launches from other threads. */
int mnk_reload_config(void);
/* W = ceil(m*(n+1)/64), or 0 when the geometry is unsupported */
int mnk_state_words(int m, int n);
/* R = ceil(m*(n+1)/32), rows of one rollout record; 0 when the geometry is unsupported */
int mnk_record_words(int m, int n);
/* 1 when 1 <= k <= min(m,n), 2 <= n <= 61 and W <= 16 (planes of up to 1 024 bits m*(n+1): 22x22, 25x25, 31x31, 16x61) */
int mnk_geometry_supported(int m, int n, int k);
const char* mnk_last_launch_error(void);

/* ---- env/torch_vector_mnk_env.py:34-44  reset(env_indices=None) ------------------- */
int mnk_reset_all(uint64_t* planes, uint32_t* meta, int64_t N, int W, void* stream);
/* idx: R int64 env indices (negative indices wrap like torch indexing); out-of-range -> err */
int mnk_reset_idx(uint64_t* planes, uint32_t* meta, int64_t N, int W, const int64_t* idx, int64_t R,
                  int32_t* err, void* stream);
/* mask: u8[N], non-zero = reset (fixed-shape form used by the fused paths) */
int mnk_reset_mask(uint64_t* planes, uint32_t* meta, int64_t N, int W, const uint8_t* mask, void* stream);

/* ---- env/torch_vector_mnk_env.py:55-84 + 106-119  step / step_subset / _check_wins ---
 * actions: int64[A]; active_idx: int64[A] ascending unique env ids, or NULL for the full
 * batch (then A must equal N).  rewards f32[N] / dones u8[N] are FULL-SIZE as in the
 * reference (:75-80): zero outside the active set.  legal_mask u8[N][m*n] and
 * obs f32[N][2][m][n] (absolute planes, env/torch_vector_mnk_env.py:46-53) are optional
 * (NULL = skip) and always cover all N envs. */
int mnk_step(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
             const int64_t* actions, const int64_t* active_idx, int64_t A,
             float* rewards, uint8_t* dones, uint8_t* legal_mask, void* obs, int obs_dtype,
             int32_t* err, uint32_t flags, void* stream);

/* ---- BASELINE.json config 2 in ONE launch per ply: RandomPolicy.act (selfplay/policy.py:18-29) -> env.step
 * (env/torch_vector_mnk_env.py:55-84, win scan :106-119) -> env.reset(nonzero(done)) (:34-44) -> observe (:46-53).
 * Every env draws its own uniformly random legal move -- Philox(seed, env_id0 + i, step [+ *step_dev], stream_id),
 * the draw of mnk_sample_legal -- plays it, and (flags & MNK_STEP_AUTORESET) restarts if the game ended; rewards /
 * dones / legal_mask / obs as in mnk_step; actions_out (optional) int64[N] receives the moves played.
 * T such launches with step = s .. s+T-1 and MNK_STEP_AUTORESET play the plies of mnk_rollout_random(T, step0 = s). */
int mnk_step_random(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                    uint64_t seed, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int stream_id,
                    int64_t* actions_out, float* rewards, uint8_t* dones, uint8_t* legal_mask, void* obs, int obs_dtype,
                    uint32_t flags, void* stream);

/* ---- env/torch_vector_mnk_env.py:46-53 observe() and
 *      selfplay/torch_self_play_wrapper.py:99-112 _get_canonical_obs() --------------------
 * flip_side: NULL -> absolute planes; else int64[N], envs with flip_side==1 get the two
 * planes swapped (the agent sees itself in channel 0).  fix_empty_mask != 0 sets
 * mask[i][0] = 1 for rows without a legal cell (wrapper:108-110). obs or mask may be NULL. */
int mnk_observe(const uint64_t* planes, const uint32_t* meta, int64_t N, int m, int n,
                const int64_t* flip_side, void* obs, int obs_dtype, uint8_t* legal_mask, int fix_empty_mask,
                uint64_t* packed_obs, void* stream);
/* packed_obs (optional, here and in mnk_selfplay_post / mnk_selfplay_step_random): the same view as `obs` as packed
 * planes u64[2][W][N], channel 0 = the viewer's stones -- 16*W B per env (32 B at 9x9) instead of the 8C + C B of
 * observation + mask; what alg.packed_rollout_buffer.PackedRolloutBuffer stores and mnk_gather_obs expands. */

/* dense (N,2,m,n) f32 <-> packed planes: backs the writable `env.boards` view
 * (tests/test_mnk_integration.py:57-58 pokes stones in).  A cell is a stone when != 0. */
int mnk_pack_boards(const float* boards, uint64_t* planes, int64_t N, int m, int n, void* stream);
int mnk_unpack_boards(const uint64_t* planes, float* boards, int64_t N, int m, int n, void* stream);

/* `step_dev` (functions that draw random numbers): optional device pointer to a u64 that is ADDED to `step`.
 * A captured hipGraph replays its kernel arguments verbatim; keeping the advancing part of the Philox step
 * counter in device memory (bumped by one more node of the graph) lets a captured agent-step be replayed.
 * NULL = the step is `step`. */

/* ---- selfplay/policy.py:13-29 RandomPolicy.act -------------------------------------------
 * One uniformly drawn legal cell per env, from Philox(seed, env_id0 + i, step, stream_id).
 * Rows without a legal cell draw uniformly over all cells (the 1e-8 guard of policy.py:21-24). */
int mnk_sample_legal(const uint64_t* planes, int64_t N, int m, int n, uint64_t seed, uint64_t step,
                     const uint64_t* step_dev, int64_t env_id0, int stream_id, int64_t* actions, void* stream);

/* ---- alg/architectures/cnn.py:69-79 (= resnet.py:84-95, transformer.py:80-91) + policy.py:46-52 + ppo.py:96-97
 * Masked categorical head fused with the draw: logits [N][C] of type `logits_dtype` (MNK_LOGITS_F32: float,
 * MNK_LOGITS_BF16: bf16 bit patterns; any additive normalisation), mask u8[N][C], C <= 1024.
 * logits == NULL: every logit is 0 -- a uniform draw over the legal cells (RandomPolicy, policy.py:13-29) that
 * reads only the mask.  deterministic != 0 -> argmax over legal cells (policy.py:48-49); else an inverse-CDF draw
 * from softmax(masked logits) with one Philox uniform per row (stream MNK_STREAM_SAMPLE).
 * All-masked row -> uniform over C (cnn.py:76-77).
 * logp (optional) = log-probability of the chosen action under the masked softmax (f32 arithmetic).
 * For finite logits of any magnitude the drawn cell is legal and logp is finite, within f32 rounding of the
 * differences logit - max (no error term in the size of the logits themselves); non-finite logits (+-inf, NaN) are
 * unspecified.  The row's uniform is (top 24 bits of the Philox word + 0.5) * 2^-24 rounded to f32, so the top word
 * gives exactly 1.0: that point is the end of the walk and takes the last cell with weight.
 * seed_dev (optional): device pointer to a u64 that REPLACES `seed` -- the sampler's Philox key in device memory, so a
 * sampler captured into a hipGraph can be re-keyed without a new capture (a fresh opponent before every rollout,
 * train.py:106-114).  Row i draws from Philox(seed, env_id0 + i, step [+ *step_dev], MNK_STREAM_SAMPLE). */
int mnk_sample_logits(const void* logits, int logits_dtype, const uint8_t* mask, int64_t N, int C, uint64_t seed,
                      const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic,
                      int64_t* actions, float* logp, void* stream);

/* ---- selfplay/torch_self_play_wrapper.py:32-67 step(), split around the opponent forward ----
 * pre : envs with pending != 0 are reset instead of stepped (their action is ignored), get a
 *       fresh side (forced_side[i] if given, else the top bit of Philox(seed, env, step, SIDE));
 *       the others play the agent's ply.  Writes partial rewards / terminated, the per-env
 *       flags for `post`, and the opponent's view (itself in channel 0, wrapper:83-89) for
 *       every env; rows that need no reply carry their current position and are ignored later.
 * post: envs flagged NEED_OPP play opp_actions; zero-sum merge (wrapper:59-63: reward -= r_opp,
 *       terminated = done_opp, both skipped for freshly reset envs :46); pending = terminated;
 *       writes the agent's canonical observation and mask (wrapper:99-112). */
int mnk_selfplay_pre(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                     const int64_t* actions, const uint8_t* pending, int64_t* agent_side,
                     const int64_t* forced_side, uint64_t seed, uint64_t step, const uint64_t* step_dev,
                     int64_t env_id0, float* rewards, uint8_t* terminated, uint8_t* sp_flags,
                     void* opp_obs, int obs_dtype, uint8_t* opp_mask, int32_t* err, uint32_t flags, void* stream);
int mnk_selfplay_post(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                      const int64_t* opp_actions, const uint8_t* sp_flags, const int64_t* agent_side,
                      float* rewards, uint8_t* terminated, uint8_t* pending,
                      void* obs, int obs_dtype, uint8_t* legal_mask, uint64_t* packed_obs, int32_t* err,
                      float* ep_return, int32_t* ep_length, int64_t* ep_stats, uint32_t flags, void* stream);
/* Every output is caller-owned and may point INTO the rollout sink: obs / legal_mask at row t+1 of the
 * RolloutBuffer's observations / action_masks (alg/rollout_buffer.py:14-44), rewards / terminated at row t of its
 * rewards / dones -- the step then writes each agent-step once, where the reference writes it, reads it back and
 * writes it again in RolloutBuffer.add (alg/rollout_buffer.py:47-58: 7 copy_ per step). */
/* flags: MNK_STEP_STRICT makes an agent / opponent move onto an occupied cell an MNK_ERR_ILLEGAL_MOVE (the env is
 * left untouched) instead of the reference's silent overwrite (env/torch_vector_mnk_env.py:67-69).
 * ep_* (all three or none; NULL = off): device-side episode accounting replacing the host loop of
 * alg/ppo.py:110-120 (dones.any() + nonzero + tolist, two synchronisations per step).  ep_return f32[N] /
 * ep_length i32[N] carry the running return and length (agent-steps) of each env's current episode; when
 * an env terminates its episode is added to ep_stats = int64[MNK_STATS_REPLICAS][MNK_STATS_STRIDE]
 * {episodes, wins (return > 0), losses (< 0), draws, sum of lengths} and the two running values restart. */
/* Whole wrapper.step in ONE launch for a uniformly random opponent (RandomPolicy, policy.py:13-29):
 * pre + Philox legal draw (stream OPP) + post. */
int mnk_selfplay_step_random(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                             const int64_t* actions, uint8_t* pending, int64_t* agent_side,
                             const int64_t* forced_side, uint64_t seed, uint64_t step, const uint64_t* step_dev,
                             int64_t env_id0, float* rewards, uint8_t* terminated, void* obs, int obs_dtype,
                             uint8_t* legal_mask, uint64_t* packed_obs,
                             int32_t* err, float* ep_return, int32_t* ep_length, int64_t* ep_stats,
                             uint32_t flags, void* stream);

/* ---- the step kernels with the masked draw folded in ("[masked sample + opp ply + zero-sum
 * merge + canonical obs]" in one launch).  Each takes, in place of the int64 moves of its plain form, what
 * mnk_sample_logits takes -- logits [N][C] (NULL = uniform over the mask), logits_dtype, mask u8[N][C], the SAMPLER's
 * Philox key and position (sample_seed / sample_seed_dev / sample_step / sample_step_dev / sample_env_id0: independent of
 * the wrapper's own seed / step / env_id0 that follow), deterministic -- draws every row's move in the kernel and plays it:
 *   mnk_selfplay_pre_logits          the AGENT's move from its policy head (selfplay/policy.py:46-52, cnn.py:69-79) with its
 *                                    log-probability (alg/ppo.py:96-97), then wrapper:39-59;
 *   mnk_selfplay_post_logits         the OPPONENT's reply from its head on the view `pre` wrote (wrapper:83-96), then the
 *                                    merge and the agent's canonical view (wrapper:59-65, :99-112);
 *   mnk_selfplay_step_random_logits  the agent's move as in pre, the uniformly random opponent, everything else: one launch
 *                                    per agent-step.
 * `actions` (required) / `logp` (optional) receive the drawn moves and their log-probabilities for ALL N rows (rows whose
 * move is not played -- pending resets, no reply needed -- still draw: the rollout buffer stores them, alg/ppo.py:104).
 * Bit-identical to mnk_sample_logits followed by the plain form.  One launch on 3x3x3, 9x9x5, 13x13x5, 15x15x5 and 19x19x5;
 * other boards take the two launches inside the call until the kernel is hot, then one launch of the board's own run-time
 * compiled variant (ABI 6, below).  A network-vs-network agent-step is 2 env-side launches (was 4). */
int mnk_selfplay_pre_logits(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, const void* logits,
                            int logits_dtype, const uint8_t* mask, uint64_t sample_seed, const uint64_t* sample_seed_dev,
                            uint64_t sample_step, const uint64_t* sample_step_dev, int64_t sample_env_id0, int deterministic,
                            int64_t* actions, float* logp, const uint8_t* pending, int64_t* agent_side,
                            const int64_t* forced_side, uint64_t seed, uint64_t step, const uint64_t* step_dev,
                            int64_t env_id0, float* rewards, uint8_t* terminated, uint8_t* sp_flags, void* opp_obs,
                            int obs_dtype, uint8_t* opp_mask, int32_t* err, uint32_t flags, void* stream);
int mnk_selfplay_post_logits(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, const void* opp_logits,
                             int logits_dtype, const uint8_t* opp_mask, uint64_t sample_seed, const uint64_t* sample_seed_dev,
                             uint64_t sample_step, const uint64_t* sample_step_dev, int64_t sample_env_id0, int deterministic,
                             int64_t* opp_actions, float* opp_logp, const uint8_t* sp_flags, const int64_t* agent_side,
                             float* rewards, uint8_t* terminated, uint8_t* pending, void* obs, int obs_dtype,
                             uint8_t* legal_mask, uint64_t* packed_obs, int32_t* err, float* ep_return, int32_t* ep_length,
                             int64_t* ep_stats, uint32_t flags, void* stream);
int mnk_selfplay_step_random_logits(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, const void* logits,
                                    int logits_dtype, const uint8_t* mask, uint64_t sample_seed,
                                    const uint64_t* sample_seed_dev, uint64_t sample_step, const uint64_t* sample_step_dev,
                                    int64_t sample_env_id0, int deterministic, int64_t* actions, float* logp,
                                    uint8_t* pending, int64_t* agent_side, const int64_t* forced_side, uint64_t seed,
                                    uint64_t step, const uint64_t* step_dev, int64_t env_id0, float* rewards,
                                    uint8_t* terminated, void* obs, int obs_dtype, uint8_t* legal_mask, uint64_t* packed_obs,
                                    int32_t* err, float* ep_return, int32_t* ep_length, int64_t* ep_stats, uint32_t flags,
                                    void* stream);

/* ---- the one-ply tactical player: a fixed-strength opponent (take a win, else block one, else play at random).
 * For the side to move, with C = m*n cells in action order: W = the legal cells where its stone leaves a run of >= k of
 * its stones through that cell (the win test of env/torch_vector_mnk_env.py:106-119 after that ply: an overline counts),
 * B = the same for the other side (where it would win next ply); S = W if W is not empty, else B if that is not empty,
 * else the legal cells (all C cells on a full board).  The move is the r-th cell of S in action order, r = mulhi32(x, |S|)
 * for one Philox u32 x -- oracle/philox.py pick_legal over the mask of S; deterministic: r = 0.  Where neither side can
 * complete a run S is the legal set, so the move equals the uniformly random one drawn from the same x.
 * mnk_selfplay_step_tactical: the arguments of mnk_selfplay_step_random, the same step in ONE launch with this player as
 * the opponent, drawing x = Philox(seed, env_id0 + i, step [+ *step_dev], MNK_STREAM_OPP) -- the random opponent's u32. */
int mnk_selfplay_step_tactical(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                               const int64_t* actions, uint8_t* pending, int64_t* agent_side,
                               const int64_t* forced_side, uint64_t seed, uint64_t step, const uint64_t* step_dev,
                               int64_t env_id0, float* rewards, uint8_t* terminated, void* obs, int obs_dtype,
                               uint8_t* legal_mask, uint64_t* packed_obs,
                               int32_t* err, float* ep_return, int32_t* ep_length, int64_t* ep_stats,
                               uint32_t flags, void* stream);
/* the same with the agent's masked draw folded in: the arguments of mnk_selfplay_step_random_logits */
int mnk_selfplay_step_tactical_logits(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, const void* logits,
                                      int logits_dtype, const uint8_t* mask, uint64_t sample_seed,
                                      const uint64_t* sample_seed_dev, uint64_t sample_step, const uint64_t* sample_step_dev,
                                      int64_t sample_env_id0, int deterministic, int64_t* actions, float* logp,
                                      uint8_t* pending, int64_t* agent_side, const int64_t* forced_side, uint64_t seed,
                                      uint64_t step, const uint64_t* step_dev, int64_t env_id0, float* rewards,
                                      uint8_t* terminated, void* obs, int obs_dtype, uint8_t* legal_mask, uint64_t* packed_obs,
                                      int32_t* err, float* ep_return, int32_t* ep_length, int64_t* ep_stats, uint32_t flags,
                                      void* stream);
/* The player as a policy (selfplay.policy.TacticalPolicy.act): obs = a canonical view [N][2][m][n] of element type
 * `obs_dtype` (channel 0 = the side to move; a cell is a stone when its element is non-zero); row i draws with
 * x = Philox(seed, env_id0 + i, step [+ *step_dev], MNK_STREAM_SAMPLE), seed_dev (optional) REPLACES seed.  actions
 * int64[N]; candidates (optional, NULL = off) u8[N][C] = the mask of S -- a threat map for features, too. */
int mnk_sample_tactical(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, uint64_t seed,
                        const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                        int deterministic, int64_t* actions, uint8_t* candidates, void* stream);

/* ---- the flat Monte Carlo player: a fixed-strength opponent whose strength is set by the playout count P.
 * Row i of obs is a canonical view [N][2][m][n] of element type `obs_dtype` (channel 0 = the side to move, "me"; a cell
 * is a stone when its element is non-zero, as in mnk_sample_tactical).  L = the legal cells in action order, C = m*n.
 * For every a in L and j in [0, P) one playout: "me" plays a, then the sides alternate starting with the other side,
 * each playing a uniformly random legal cell (pick_legal: r = mulhi32(x, |legal|), the r-th legal cell).  The game ends
 * at the first ply that leaves a run of >= k stones of its mover anywhere on its plane (the env's win test: an overline
 * counts, a run already on the board counts) or when the board is full; the outcome is a win, a loss or a draw for "me".
 * Playout j of cell a in row i, on call `step`, draws its t-th random ply (t = 0: the other side's first reply) from
 *   x = Philox(seed, env_id0 + i, u, MNK_STREAM_PLAYOUT),  u = (((step * C + a) * P + j) * C4) + t,
 * C4 = C rounded up to a multiple of 4 (one Philox block serves four consecutive plies of a playout).  The counter is keyed
 * by the global env id: the counts do not depend on the launch layout.  Range: q = u >> 2 must fit in 56 bits, i.e.
 * (step + 1) * C * P * C4 <= 2^58; a host `step` that breaks it is rejected (*step_dev is added on the device, unchecked).
 * W[a] = wins, Lo[a] = losses (draws = P - W - Lo), score s[a] = W[a] - Lo[a]; S = the legal cells of maximal score.  The
 * move is the r-th cell of S in action order, r = mulhi32(x, |S|), x = Philox(seed, env_id0 + i, step [+ *step_dev],
 * MNK_STREAM_SAMPLE) -- TacticalPolicy's u32; deterministic: r = 0; no legal cell: the draw is over all C cells.  A cell
 * that wins at once has W = P, Lo = 0 and so always lies in S: the player never misses a win in one ply.
 * seed_dev (optional) REPLACES seed, step_dev (optional) is ADDED to step.  actions int64[N]; counts (optional, NULL = off)
 * int32[N][2][C] = W then Lo per cell, 0 on occupied cells.  playouts in [1, 4096].  One launch, one workgroup per row. */
int mnk_sample_playouts(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int playouts, uint64_t seed,
                        const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                        int deterministic, int64_t* actions, int32_t* counts, void* stream);
#define MNK_PLAYOUTS_MAX 4096

/* ---- the tree-search player (UCT): a fixed-strength opponent whose strength is set by an iteration budget I, with B
 * random playouts per leaf.  Row i of obs is a canonical view as for mnk_sample_playouts (channel 0 = the side to move,
 * "me"; f32 / bf16 / u8, a cell is a stone when its element is non-zero); C = m*n.  The root is the row's position; a node
 * is the position after one more move.  Per node: visits n, and wins W and losses Lo counted from the view of the player
 * who made the move into the node.  A node is terminal when its move leaves a run of >= k of its mover anywhere on that
 * mover's plane (the env's whole-plane test: an overline counts, a run already on the board counts) or fills the board;
 * a terminal node is never expanded.  Iteration it = 0 .. I-1:
 *   selection: from the root, at a non-terminal node v: if v has a legal cell that is not yet a child, the first such
 *     cell in action order is expanded and the new child is the leaf; otherwise go to the child of maximal
 *     s = q + c * sqrt(n_v / n_child), q = (W - Lo) / n_child, evaluated in f32 with correctly rounded operations and no
 *     contraction: s = fadd(fdiv(W - Lo, n_child), fmul(c, fsqrt(fdiv(n_v, n_child)))); ties go to the lowest cell.  A
 *     terminal node reached this way is the leaf.
 *   evaluation: a terminal leaf counts its own outcome B times and draws no random numbers.  Otherwise B playouts start
 *     from the leaf with the Monte Carlo player's ply rule (pick_legal over the legal cells; the game ends at the first
 *     ply that leaves a run of its mover, or on a full board).  Ply t of playout j draws
 *       x = Philox(seed, env_id0 + i, u, MNK_STREAM_SEARCH),  u = (((step * I + it) * B + j) * C4) + t,  C4 = C rounded
 *     up to a multiple of 4.  Range: q = u >> 2 must fit in 56 bits, i.e. (step + 1) * I * B * C4 <= 2^58; a host `step`
 *     that breaks it is rejected (*step_dev is added on the device, unchecked).
 *   backup: every node on the path from the root to the leaf gets n += B, and the wins and losses of the B outcomes, each
 *     from that node's mover's view.
 * All counts stay below 2^24 and so convert to f32 exactly.  The move: S = the root children of maximal n; the r-th cell
 * of S in action order, r = mulhi32(x, |S|), x = Philox(seed, env_id0 + i, step [+ *step_dev], MNK_STREAM_SAMPLE) --
 * TacticalPolicy's u32; deterministic: r = 0; no legal cell: the draw is over all C cells (no iterations run).  A cell
 * that wins at once is a terminal child with W = n; the first |L| iterations expand every root child once (B visits
 * each), so with I < |L| a winning cell may stay unexpanded and is not guaranteed to be played.  With I >= |L| every
 * root child exists; a winning child keeps q = 1, the best value any child can have, but UCT may still spend more visits
 * on another child, so even then the rule guarantees only that the win is in the tree (in practice, at c = 1 and
 * I >= 2 |L|, it draws most of the visits).
 * seed_dev (optional) REPLACES seed, step_dev (optional) is ADDED to step.  c: finite, >= 0.  actions int64[N]; stats
 * (optional, NULL = off) int32[N][3][C] = the root children's n, then W, then Lo per cell, 0 on occupied cells and on
 * cells never expanded.  iterations in [1, 2048], playouts in [1, 256].  One launch, one workgroup per row, the tree in
 * LDS. */
int mnk_sample_search(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, int playouts,
                      float c, uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev,
                      int64_t env_id0, int deterministic, int64_t* actions, int32_t* stats, void* stream);
#define MNK_SEARCH_ITERS_MAX 2048
#define MNK_SEARCH_PLAYOUTS_MAX 256

/* ---- the PUCT search player: AlphaZero-style search guided by the caller's evaluator (normally a policy/value net),
 * batched over rows, one env-side launch per evaluation.  Row i of obs is a canonical view [N][2][m][n] (f32 / bf16 / u8,
 * channel 0 = the side to move, a cell is a stone when its element is non-zero); C = m*n; I = iterations in [1, 2048].
 * Nodes: a node is a position with a visit count n (u32) and a value sum w (f32) from the view of the player who moved
 * into it.  A node is terminal when its move leaves a run of >= k of its mover anywhere on that mover's plane (the env's
 * whole-plane test, as in mnk_sample_search) or fills the board.  An evaluated node keeps the prior P[a] of each of its
 * legal cells a exactly as the evaluator returned it (not renormalised; the priors of occupied cells are never read).
 * Evaluation 0: the leaf is the root (the row itself, its legal cells as the mask).  Iterations it = 1 .. I, each a
 * backup of the previous leaf, then a selection:
 *   backup: v = the leaf's value from the view of its side to move -- the evaluator's value for that row when the leaf
 *     is not terminal, -1 when the move into it won, 0 when it filled the board.  Every node on the path root .. leaf
 *     (leaf at depth d) gets n += 1 and, at depth j, w += v when d - j is odd, w += -v when it is even: one add per node
 *     and iteration, in iteration order, each a correctly rounded f32 add.
 *   selection: from the root, at an evaluated node v take the legal cell a of maximal
 *       s = fadd(q, fdiv(fmul(fmul(c, P[a]), fsqrt((float)n_v)), (float)(1 + n_a))),  q = n_a ? fdiv(w_a, n_a) : 0,
 *     every operation correctly rounded, no contraction, ties to the lowest cell; n_a, w_a are the child's through a
 *     (0 when it does not exist).  A child that does not exist yet is created and is the leaf; an existing terminal
 *     child is the leaf; otherwise descend into it.
 *   leaf output: the leaf's canonical observation (channel 0 = its side to move) into leaf_obs [N][2][m][n] of
 *     leaf_dtype, its legal cells into leaf_mask u8 [N][C], for every row, terminal leaves included (the evaluator's
 *     outputs for a terminal leaf are not read).
 * A row creates at most one node per iteration (at most I + 1 nodes).  A row whose root has no legal cell runs no
 * iterations (its leaf stays the root) and draws its move over all C cells, as the other players do.  The move, after
 * the last backup: S = the root children of maximal n; temperature 0: the r-th cell of S in action order, r = mulhi32(x,
 * |S|); temperature 1: the cell at which the root children's visits, accumulated in action order, first exceed r =
 * mulhi32(x, sum n_a); deterministic: the first cell of S.  x = Philox(seed, env_id0 + i, step [+ *step_dev],
 * MNK_STREAM_SAMPLE) -- TacticalPolicy's u32; seed_dev (optional) REPLACES seed, step_dev (optional) is ADDED to step.
 * Outputs (optional, NULL = off): visits int32 [N][C] = the root children's n (0 elsewhere; they sum to I on a row with a
 * legal cell whose tree mnk_puct_begin set up, to n_root - 1 = the carried visits + the iterations run on a tree that
 * mnk_puct_rebase carried over whole); root_value f32 [N] = -w_root / n_root, the root's mean value for its side to
 * move.  priors: f32 or bf16 [N][C], values f32 or bf16 [N] (MNK_LOGITS_*; a bf16 element is read as its exact f32).  Non-finite priors or values
 * give an unspecified result (not checked: a check would cost a synchronisation).  c: finite, >= 0.
 * The tree lives in `workspace` (mnk_puct_workspace_bytes(N, m, n, I) bytes, about (I + 1) * 6 * C per row; its layout is
 * private to the library) from mnk_puct_begin to the step with `last` set, and on to the next mnk_puct_rebase.  One
 * act() = mnk_puct_begin, then I steps with last = 0 and one with last = 1 (I + 2 launches, I + 1 evaluations), all
 * stream-ordered, no host synchronisation.  Every host check runs before anything is enqueued. */
int64_t mnk_puct_workspace_bytes(int64_t N, int m, int n, int iterations);  /* < 0: MNK_EINVAL / MNK_EGEOM */
/* the roots into the tree; writes them as evaluation 0 (leaf_obs, leaf_mask) */
int mnk_puct_begin(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, void* workspace,
                   void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, void* stream);
/* one backup of the evaluation (priors, values) of the pending leaves, then one selection that writes the next leaves;
 * with last = 1 the backup, then the move (actions int64[N]), visits and root_value, and no new leaf (leaf_obs /
 * leaf_mask may then be NULL) */
int mnk_puct_step(void* workspace, int64_t N, int m, int n, int k, int iterations, const void* priors, int priors_dtype,
                  const void* values, int values_dtype, float c, int last, int temperature, uint64_t seed,
                  const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0, int deterministic,
                  void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions, int32_t* visits,
                  float* root_value, void* stream);
#define MNK_PUCT_ITERS_MAX 2048
/* mnk_puct_begin for a search that keeps the subtree of the position that was reached (optional; a workspace that only
 * ever sees mnk_puct_begin behaves as above).  The workspace is that of tree_iterations (tree_iterations + 1 nodes; the
 * same number goes to mnk_puct_workspace_bytes and to every mnk_puct_step) and must start out as zeros.  An act() that
 * runs J iterations = mnk_puct_rebase, J steps with last = 0, one with last = 1; the host keeps
 * 1 <= keep_nodes <= tree_iterations + 1 - J, so the tree cannot fill during the act.
 * The rule is by position.  R0, R1 = the stored root's planes (R0 = its side to move), O0, O1 = the channels of row i of
 * obs.  The row CONTINUES the stored tree iff the row's tree is live (it has a node, its root had a legal cell) and
 * exactly one of
 *   O0 = R0 and O1 = R1                                                  (the same position: the path is empty),
 *   O1 = R0 + one cell a1 and O0 = R1                                    (one ply on: the path is [a1]),
 *   O0 = R0 + one cell a1 and O1 = R1 + one cell a2                      (two plies on: the path is [a1, a2])
 * holds, and every step of the path leads to a child that exists and is not terminal.  Any other row -- a workspace of
 * zeros, a game that was reset, an unrelated position -- is FRESH: it gets exactly what mnk_puct_begin writes.
 * A row that continues keeps the subtree of the node the path ends in: its nodes in their order of creation (the new
 * root is node 0), the first keep_nodes of them when there are more; a kept node keeps n, w, its move, its terminal kind,
 * its priors and its children, and a child that was dropped becomes "none yet".  w stays the view of the mover into the
 * node.  Evaluation 0 is the roots for every row (leaf_obs, leaf_mask as mnk_puct_begin writes them).  The step that
 * follows backs it up as ever on a fresh row; on a row that continues it only replaces the root's priors on its free
 * cells -- no n or w changes, no child is touched -- so an evaluator that perturbs the priors of evaluation 0 still acts on
 * every root.  The visits of such a row sum to n_root - 1 when nothing of the root's children was dropped.
 * carried (optional) int32 [N][2] = {nodes kept, the new root's n}, {0, 0} on a fresh row. */
int mnk_puct_rebase(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int tree_iterations, int keep_nodes,
                    void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int32_t* carried, void* stream);
/* The same search with L = leaves in [1, MNK_PUCT_LEAVES_MAX] leaves per row and evaluation, so that the evaluator sees
 * I / L + 1 batches of N * L rows instead of I + 1 batches of N.  Everything above holds, with a ROUND in the place of an
 * iteration: a round backs up the L pending SLOTS of the row, then selects L new ones.  An act of I simulations is I / L
 * rounds (the host requires I % L = 0, of the workspace's `iterations` too); the node capacity stays I + 1 (tree_iterations
 * + 1 with mnk_puct_rebase_leaves).  leaves = 1 is the search above, bit for bit, in the same workspace.
 *   batch layout: slot j of row i is batch row i * L + j of leaf_obs [N*L][2][m][n], leaf_mask [N*L][C], priors
 *     [N*L][C] and values [N*L] -- an evaluator sees a larger batch and nothing else.
 *   evaluation 0: slot 0 is the root, exactly as mnk_puct_begin / mnk_puct_rebase write it (on a carried root it only
 *     renews the priors); slots 1 .. L-1 are void.
 *   void slots: a void slot shows the root's view and the root's legal cells; the evaluator's outputs for it are never
 *     read and nothing is backed up for it.  A row whose root has no legal cell has only void slots.
 *   selection: slots 0 .. L-1 of a round select one after the other.  Slot j walks from the root by the score above under
 *     VIRTUAL VISITS: with vl(x) = the number of earlier non-void slots of this round whose path contains node x, at node
 *     v the child through cell a counts as
 *       n'_a = n_a + vl(a),  w'_a = fadd(w_a, -(float)vl(a)),  q = n'_a ? fdiv(w'_a, (float)n'_a) : 0,
 *       s = fadd(q, fdiv(fmul(fmul(c, P[a]), fsqrt((float)(n_v + vl(v)))), (float)(1 + n'_a))),
 *     every operation correctly rounded, no contraction, ties to the lowest cell (vl = 0: the score above, bit for bit).
 *     A child that does not exist yet is created and is the slot's leaf.  An existing terminal child is the leaf again,
 *     as often as the round's slots reach it (one created earlier in the same round too: it needs no evaluation).  A walk
 *     that reaches a node that is not terminal and was created earlier in this round makes the slot void: that node has no
 *     evaluation yet.  A void slot changes nothing, so every later slot of the round is void as well.  A full tree makes
 *     a slot void (it cannot happen within the budgets the host allows).
 *   backup: the round's non-void slots are backed up in slot order, each exactly as above (n += 1 and one correctly
 *     rounded f32 add per node of its path; slot 0's adds to a node come before slot 1's).  Virtual visits never touch n
 *     or w: they exist only while a round selects.
 *   visits: on a fresh row they sum to I minus the row's void slots after evaluation 0, on a carried row to the carried
 *     visits plus that.  The move, root_value, both temperatures, the key words and `deterministic` are as above.
 * One act() = mnk_puct_begin_leaves (or mnk_puct_rebase_leaves with keep_nodes <= tree_iterations + 1 - leaves), I / L
 * steps with last = 0 and one with last = 1; every call of an act gets the same `leaves`.  mnk_puct_workspace_bytes_leaves
 * (.., 1) = mnk_puct_workspace_bytes(..): the slots' own state (L paths, L leaves, L x {depth, state}) lies behind the
 * tree.  Every host check runs before anything is enqueued. */
#define MNK_PUCT_LEAVES_MAX 16
int64_t mnk_puct_workspace_bytes_leaves(int64_t N, int m, int n, int iterations, int leaves);
int mnk_puct_begin_leaves(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int iterations, int leaves,
                          void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, void* stream);
int mnk_puct_rebase_leaves(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, int tree_iterations,
                           int keep_nodes, int leaves, void* workspace, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask,
                           int32_t* carried, void* stream);
int mnk_puct_step_leaves(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, void* stream);
/* mnk_puct_step_leaves with exact game-theoretic proofs in the backup ("MCTS-Solver"; optional: a search that never calls
 * it is the search above).  The workspace is that of mnk_puct_begin_leaves / mnk_puct_rebase_leaves, leaves in [1,
 * MNK_PUCT_LEAVES_MAX]; every step of an act is this entry point (and with mnk_puct_rebase_leaves every act on the tree).
 * Every node has a PROOF from the same point of view as its w, the player who moved into it: 0 unknown, 1 WIN, 2 DRAW,
 * 3 LOSS; the root's point of view is the opponent of its side to move.  A proven node is worth, for its own side to
 * move, -1 (WIN), 0 (DRAW), +1 (LOSS).  Proofs are kept with the node, so a kept subtree keeps them; the node that
 * becomes the new root starts unknown again.
 *   creation: a new node whose move won is WIN, one whose move filled the board is DRAW, any other is unknown.
 *   selection at an evaluated, unproven node v: the candidates are the free cells whose child is not proven LOSS (a move
 *     proven to lose for the player making it); if that leaves none, all free cells.  The candidates are scored exactly
 *     as above (virtual visits included), the maximal score wins, ties to the lowest cell.  A child that does not exist
 *     is created and is the leaf.  A child with a proof is the leaf and needs no evaluation, as a terminal child above
 *     (as often as the round's slots reach it); its backup's v is -1 (WIN), 0 (DRAW), +1 (LOSS).  Otherwise descend.
 *     A root with a proof selects nothing: its slots are void, as those of a row whose tree is full.
 *   backup: n and w along the path exactly as above.  When the leaf has a proof, then for p = depth - 1 down to 0, x =
 *     the path's node at depth p:  (1) x has a proof: stop;  (2) some child of x is WIN: x is LOSS;  (3) else some free
 *     cell of x has no child or an unknown one: x stays unknown, stop;  (4) else every child is LOSS: x is WIN;  (5) else
 *     x is DRAW.  At most `depth` levels.  It runs on every backup of a proven leaf, so a carried root is proven again by
 *     the first visit to its deciding child.  w is not rewritten when a node becomes proven.
 *   the move: adjusted counts n' over the root's free cells -- some root child is WIN: n' = n on the WIN children and 0
 *     elsewhere; else n' = 0 on the LOSS children and n elsewhere; if that is all zero, n' = n.  visits = n', and the move
 *     is drawn from n' by the rules above (both temperatures, deterministic).  WITH THE SOLVER visits NO LONGER SUM TO THE
 *     NUMBER OF ITERATIONS: a proven root stops searching, and counts are dropped from n'.
 *   root_value = +1, 0 or -1 exactly when the root is proven (LOSS, DRAW, WIN), -w_root / n_root otherwise.
 *   proof (optional, NULL = off) int8 [N] = the root's proof for its side to move: +1 a proven win, 0 a proven draw, -1 a
 *     proven loss, MNK_PROOF_UNKNOWN otherwise (and on a row without a legal cell).
 * leaves outside [1, MNK_PUCT_LEAVES_MAX] is MNK_EINVAL; every host check runs before anything is enqueued. */
#define MNK_PROOF_UNKNOWN (-128)
int mnk_puct_step_solver(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, int8_t* proof, void* stream);
/* mnk_puct_step_leaves (solver = 0) or mnk_puct_step_solver (solver = 1) with FIRST-PLAY URGENCY (optional: a search
 * that never calls it is the search above).  Above, a free cell without a visit scores with q = 0: with values in [-1, 1],
 * "an untried move is a draw", so a node whose visited moves all look lost tries every other cell once before it returns
 * to one, and a node whose first move looks won never tries a second.  Here such a cell is valued at the node's own mean
 * value, less a reduction that grows with the prior mass already visited (KataGo's and Leela's rule).  The workspace is
 * that of mnk_puct_begin_leaves / mnk_puct_rebase_leaves, leaves in [1, MNK_PUCT_LEAVES_MAX]; every step of an act is this
 * entry point.  fpu_root is the reduction at the root (node 0), fpu the one below it: f32, finite, >= 0.
 *   At an evaluated node v, with n'_a, w'_a the child's counts through cell a under the round's virtual visits as above:
 *     q_v  = fdiv(-w_v, (float)n_v), from the stored n_v >= 1 and w_v, WITHOUT virtual visits: the node's mean value for
 *            its own side to move (root_value's formula);
 *     t_a  = (uint64_t)(min(max(P_v[a], 0), 1) * 2^32), truncated, for every free cell a of v with n'_a > 0 (every such
 *            cell, the children proven LOSS included), and T = the sum of the t_a: integers, so the order of the sum
 *            cannot matter (a prior of 1 or more is 2^32; T < 2^43);
 *     mass = fl32(sqrt((double)T * 2^-32)), the f64 square root correctly rounded, then rounded to f32;
 *     r    = fpu_root at v = node 0, fpu elsewhere;
 *     a free cell with n'_a = 0 scores with  q = fmax(fsub(q_v, fmul(r, mass)), -1);
 *     a free cell with n'_a > 0 keeps        q = fdiv(w'_a, (float)n'_a).
 *   Every operation correctly rounded, no contraction.  Everything else is unchanged: s, the tie rule, the solver's
 *   classes of candidates, where a walk ends, the backup, the move, visits, root_value, the proofs.  fpu = fpu_root = 0 is
 *   NOT the search above: an untried move then scores with q_v, not with 0.
 * proof may be NULL, and is not written, when solver = 0.  solver outside {0, 1}, leaves outside [1,
 * MNK_PUCT_LEAVES_MAX], a NaN, infinite or negative fpu or fpu_root are MNK_EINVAL; every host check runs before anything
 * is enqueued; N = 0 returns MNK_OK after them. */
int mnk_puct_step_fpu(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                      int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                      uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                      int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                      int32_t* visits, float* root_value, int8_t* proof, int solver, float fpu, float fpu_root,
                      void* stream);
/* mnk_puct_step_leaves, mnk_puct_step_solver (solver = 1) or mnk_puct_step_fpu (fpu_on = 1) with FORCED PLAYOUTS AND POLICY
 * TARGET PRUNING (Wu, "Accelerating self-play learning in Go", 2019, section 3.2; optional: a search that never calls it
 * is the search above).  With noise on the root's priors and a small budget, a move the noise promotes gets one visit,
 * looks mediocre and is never tried again, and that one visit goes into the policy target as noise.  Forced playouts give
 * every visited root child a floor of visits that grows with its prior and the root's total; pruning takes those visits
 * back out of the counts that are handed out and played from, wherever PUCT alone would not have spent them.  The
 * workspace is that of mnk_puct_begin_leaves / mnk_puct_rebase_leaves, leaves in [1, MNK_PUCT_LEAVES_MAX]; every step of an
 * act is this entry point.  forced_k = k: f32, finite, > 0 (KataGo's 2).  fpu_on in {0, 1}: 0 = no first-play urgency, fpu
 * and fpu_root are not read (fpu = 0 is not "off", hence the flag).
 * Notation: node 0 is the root, P_0[a] its stored prior of cell a (after mnk_puct_root_noise, if any), n_a and w_a the
 * stored counts of the root's child through cell a, vl(.) the round's virtual visits, c the exploration constant.  Every
 * float operation is a correctly rounded f32 operation, no contraction; priors are taken to be finite.
 *   selection, at the root only (below it the walk is unchanged): S' = n_0 + vl(0) - 1.  A free cell a is FORCED iff
 *     (1) its child exists with stored n_a > 0 -- a child created earlier in the same round has no evaluation and is never
 *     forced: with leaves > 1 a new child of high prior would otherwise pull the round's next slot into an unevaluated
 *     node and void the rest of the round; (2) with the solver, the child is not proven LOSS; (3) with n'_a = n_a + vl(a),
 *     fmul((float)n'_a, (float)n'_a) < fmul(fmul(k, P_0[a]), (float)S').  If any cell is FORCED, the candidates are the
 *     FORCED cells alone, scored by the unchanged s (first-play urgency cannot matter: n'_a > 0), the maximum wins, ties
 *     to the lowest cell.  If none is, the selection is the one above.
 *   pruning, on last = 1: n' = the counts the move would be drawn from above (the children's n; with the solver the
 *     adjusted counts).  If the solver keeps the WIN children alone, nothing is pruned: n'' = n'.  Otherwise
 *       c* = the cell of maximal n', ties to the lowest cell (all n' zero: nothing is pruned);
 *       s_a(j) = fadd(fdiv(w_a, (float)n_a), fdiv(fmul(fmul(c, P_0[a]), fsqrt((float)n_0)), (float)(1 + j)));
 *       s* = s_{c*}(n'_{c*});
 *       c* keeps its count; a cell with n'_a = 0 or P_0[a] <= 0 keeps its count; for every other cell
 *         t_a = fmul(fmul(k, P_0[a]), (float)(n_0 - 1)),
 *         F_a = the least integer F >= 0 with fmul((float)F, (float)F) >= t_a,
 *         lo = n'_a - min(n'_a, F_a),
 *         n''_a = the least j in [lo, n'_a] with s_a(j) < s*, and n'_a if there is none;
 *         if that leaves n''_a = 1 where n'_a > 1, then n''_a = 0.
 *     For P_0[a] > 0, s_a(j) does not increase with j (a correctly rounded quotient by a growing divisor, then a correctly
 *     rounded sum), and fmul((float)F, (float)F) does not decrease with F: the kernel bisects where this text walks, and
 *     finds the same j and the same min(n'_a, F_a).
 *   visits = n''; the move is drawn from n'' by the unchanged rules (both temperatures, deterministic).  root_value and
 *   proof are unchanged.  raw_visits (optional, int32 [N][C], NULL = off) takes n'.  WITH PRUNING visits NO LONGER SUM TO THE
 *   NUMBER OF ITERATIONS.
 * Everything else is unchanged: the backup, the proofs, where a walk ends.  proof may be NULL, and is not written, when
 * solver = 0.  solver or fpu_on outside {0, 1}, leaves outside [1, MNK_PUCT_LEAVES_MAX], a NaN, infinite or negative fpu or
 * fpu_root with fpu_on = 1, a forced_k that is NaN, infinite or <= 0 are MNK_EINVAL; every host check runs before anything
 * is enqueued; N = 0 returns MNK_OK after them. */
int mnk_puct_step_forced(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int temperature,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, int8_t* proof, int solver, float fpu, float fpu_root,
                         int fpu_on, float forced_k, int32_t* raw_visits, void* stream);
/* The search above with a GUMBEL ROOT ("Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022;
 * optional: a search that never calls these is the search above).  One Gumbel variable per root move, the budget spent on
 * the `considered` best moves by Sequential Halving, the survivor played -- an exact sample from the improved policy --
 * and that policy, pi' = softmax(ln P + sigma(completed q)), handed out as the training target.  Gumbel applies at the
 * root only: below the root the walk is mnk_puct_step's, backup included, bit for bit ("Gumbel root, PUCT elsewhere").
 * The workspace is that of mnk_puct_begin_leaves with leaves = 1 (any other `leaves` is MNK_EINVAL).  One act() =
 * mnk_puct_begin_leaves, evaluation 0, mnk_puct_gumbel_root, I times mnk_puct_step_gumbel with last = 0 and one with
 * last = 1, an evaluation before each; the table is uploaded once per (considered, I).
 * Parameters: considered = m in [1, MNK_PUCT_CONSIDERED_MAX]; c_visit (f32, >= 0; the paper's 50); c_scale (f32, >= 0;
 * 0.5 here where the paper has 1.0: the paper's q lies in [0, 1], this q in [-1, 1] = 2 q_paper - 1, and the constant
 * shift cancels in every argmax and softmax below, so 0.5 * q is the paper's 1.0 * q_paper); gumbel_scale (f32, >= 0;
 * 1: the sample, 0: the whole act is deterministic).
 *   the schedule (host only, no GPU): mnk_puct_gumbel_schedule fills out u16 [considered + 1][iterations].  Row m' is the
 *     sequence of considered visits of a root with m' moves to consider.  m' <= 1: 0, 1, 2, ...  Otherwise, with L2 =
 *     ceil(log2 m'), visits[0 .. m') = 0 and nc = m', repeat until the row holds I entries: extra = max(1, floor(I /
 *     (L2 * nc))); `extra` times over, append visits[0 .. nc) and then add 1 to each of them; nc = max(2, nc / 2).  The row
 *     is truncated to I entries.  (m' = 4, I = 8: 0 0 0 0 1 1 2 2.)
 *   the prep launch: mnk_puct_gumbel_root reads evaluation 0's priors [N][C] (f32 / bf16), mask (u8, non-zero = free) and
 *     values [N] and writes the caller-owned gscore f32 [N][C] and vroot f32 [N]; the evaluator's tensors are never
 *     written.  For a free cell a of row i, C4 = C rounded up to a multiple of 4, all arithmetic f64 with the full-
 *     precision logarithm:  P~_a = max(P_a, 2^-126),  l_a = ln((double)P~_a),  x_a = word a & 3 of the Philox block
 *     (step [+ *step_dev]) * (C4 / 4) + (a >> 2) of stream MNK_STREAM_GUMBEL keyed by (seed [or *seed_dev], env_id0 + i),
 *     U_a = (x_a + 0.5) * 2^-32,  g_a = -ln(-ln U_a),  gscore[a] = fl32(gumbel_scale * g_a + l_a)  (the product rounded,
 *     then the sum).  An occupied cell gets -inf.  vroot[i] = the root's value, widened to f32 exactly.
 *   root selection in simulation t = n_root - 1: F = the root's free cells, m' = min(m, F), v* = table[m'][t].  A root
 *     child has q_a = fdiv(w_a, (float)n_a), and maxn = the largest n_a.  The candidates are the free cells with
 *     n_a = v*; if there is none (it cannot happen on a fresh tree), all free cells.  A cell's key is gscore[a] when
 *     n_a = 0, else fadd(gscore[a], fmul(fmul(fadd(c_visit, (float)maxn), c_scale), q_a)), every operation correctly
 *     rounded, no contraction.  The maximal key wins, ties to the lowest cell.  From the chosen child on, the walk above.
 *   the move, after the last backup: the free cell of maximal key among those with n_a = maxn, ties to the lowest cell.
 *     A row without a legal cell draws as mnk_puct_step does.  visits (the raw n_a) and root_value are as above.
 *   policy (optional) f32 [N][C], the improved policy, in f64 (q_a above, widened):  pi_a = P~_a / sum over F of P~;  over
 *     the visited free cells Sv = sum pi_a, Sq = sum pi_a * q_a, Ns = sum n_a;  v_mix = (vroot + Ns * Sq / Sv) / (1 + Ns),
 *     or vroot when Sv = 0;  qhat_a = q_a if n_a > 0, else v_mix;  K = ((double)c_visit + maxn) * (double)c_scale;
 *     y_a = l_a + K * qhat_a;  policy_a = fl32(exp(y_a - max y) / sum exp(y - max y)).  An occupied cell gets 0, a row
 *     without a free cell is all zeros.  P~ is the root's prior as the backup of evaluation 0 stored it.
 * Every host check runs before anything is enqueued. */
#define MNK_PUCT_CONSIDERED_MAX 1024
int mnk_puct_gumbel_schedule(int considered, int iterations, uint16_t* out);
int mnk_puct_gumbel_root(const void* priors, int priors_dtype, const void* mask, const void* values, int values_dtype,
                         int64_t N, int C, float gumbel_scale, uint64_t seed, const uint64_t* seed_dev, uint64_t step,
                         const uint64_t* step_dev, int64_t env_id0, float* gscore, float* vroot, void* stream);
int mnk_puct_step_gumbel(void* workspace, int64_t N, int m, int n, int k, int iterations, int leaves, const void* priors,
                         int priors_dtype, const void* values, int values_dtype, float c, int last, int considered,
                         float c_visit, float c_scale, const uint16_t* table, const float* gscore, const float* vroot,
                         uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev, int64_t env_id0,
                         int deterministic, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, int64_t* actions,
                         int32_t* visits, float* root_value, float* policy, void* stream);
/* Dirichlet root noise for the search above (optional): one launch between evaluation 0 and the first mnk_puct_step[_leaves]
 * that mixes eta ~ Dirichlet(alpha) over each root's free cells into a copy of the root's priors.  priors (f32 / bf16,
 * MNK_LOGITS_*) and mask (u8, non-zero = free) are evaluation 0's [N * leaves][C] tensors; row i's root is batch row
 * i * leaves.  out is a caller-owned f32 [N * leaves][C] buffer of which only the rows i * leaves are written -- the step
 * reads no other row of evaluation 0 -- and which the first step then takes as its f32 priors.  priors is never written
 * (an evaluator may hand back the same tensor every call).  The rule for row i, F = its free cells, C4 = C rounded up to a
 * multiple of 4, alpha and eps widened to f64, all arithmetic f64 unless marked:
 *   draws: cell a and try t = 0 .. MNK_PUCT_NOISE_TRIES - 1 own u = ((step [+ *step_dev]) * C4 + a) * 16 + t and
 *     x_j = Philox(seed [or *seed_dev], env_id0 + i, 4 * u + j, MNK_STREAM_NOISE), j = 0 .. 3 -- the four words of one
 *     Philox block; U_j = (x_j + 0.5) * 2^-32, never 0 or 1.
 *   Gamma(alpha + 1) by Marsaglia and Tsang: d = alpha + 1 - 1/3, c = 1 / sqrt(9 d), z = sqrt(-2 ln U_0) * cos(2 pi U_1),
 *     v = (1 + c z)^3; the try is accepted iff v > 0 and ln U_2 < 0.5 z^2 + d - d v + d ln v.
 *   the first accepted try gives l_a = ln(d v) + ln(U_3) / alpha (the boost to shape alpha, U^(1 / alpha), in log space);
 *     if none of the 16 is accepted (acceptance is above 0.95 per try), l_a = ln d + ln(U_3) / alpha with try 15's U_3.
 *   normalisation: M = max of l_a over F, e_a = exp(l_a - M), eta_a = e_a / sum of e over F (at alpha = 0.03 the gammas
 *     of a 19x19 root span hundreds of decades: their plain sum can be 0).
 *   the mix, in correctly rounded f32 operations: w = fl32(1 - eps), P'_a = fl32(fl32(w * P_a) + fl32(eps * fl32(eta_a)))
 *     on free cells, P'_a = P_a elsewhere (a bf16 prior widened exactly).  A row with no free cell is a plain copy.
 *     Priors are not renormalised, as they are not without noise.
 * C in [1, 1024], leaves in [1, MNK_PUCT_LEAVES_MAX], alpha finite and > 0, eps in [0, 1]; every host check runs before
 * anything is enqueued.  One wave per row; the kernel needs C and the mask only, no board geometry. */
#define MNK_PUCT_NOISE_TRIES 16
int mnk_puct_root_noise(const void* priors, int priors_dtype, const void* mask, int64_t N, int C, int leaves, float alpha,
                        float eps, uint64_t seed, const uint64_t* seed_dev, uint64_t step, const uint64_t* step_dev,
                        int64_t env_id0, float* out, void* stream);

/* ---- search self-play: the env side of an AlphaZero loop.  A ply = a search that writes every row's root visit counts
 * (PUCTSearchPolicy.act(visits=...), mnk_puct_step), then ONE mnk_search_selfplay_step launch that plays every row's move
 * from those counts, records the position in a ring of T plies, labels the records of every game that ends with its
 * outcome, resets the finished games and writes the next roots.  No host synchronisation per ply.
 * Ring (T plies of N rows; T >= C = m*n, so a game never wraps onto its own records):
 *   ring_planes u64[T][2][W][N]  the position BEFORE the ply as packed planes, channel 0 = the side to move there
 *                                (PackedRolloutBuffer's layout: 16*W B per record)
 *   ring_visits u16[T][N][C]     the visits of the ply's search, min(max(v, 0), 65535) on free cells, 0 on occupied ones
 *   ring_z      i8[T][N]         the outcome from the view of the record's side to move: +1 win, -1 loss, 0 draw,
 *                                MNK_Z_UNKNOWN while the game is running
 * Row i of the launch: p = step [+ *step_dev], t = p mod T, x = Philox(seed [or *seed_dev], env_id0 + i, p,
 * MNK_STREAM_SELFPLAY), g = the row's move count, n_a = its ring visits above (in action order):
 *   the move: with maxn = max n_a > 0, if g < temp_plies the cell at which the n_a, accumulated in action order, first
 *     exceed mulhi32(x, sum n_a) (temperature 1), else the mulhi32(x, |S|)-th cell of S = the cells of n_a = maxn
 *     (temperature 0) -- mnk_puct_step's two rules.  maxn = 0: MNK_ERR_VISITS, the env is not played (its ring row t is
 *     still written, with z unknown, and its next root is its unchanged position).
 *   ring row t: the planes, the visits, z = MNK_Z_UNKNOWN; then the ply (the env's win test).  When it ends the game (L =
 *     g + 1 plies, the records t - d mod T for d = 0 .. L-1): a win writes z = +1 for even d and -1 for odd d, a draw 0;
 *     stats (optional, the rollout's int64[MNK_STATS_REPLICAS][MNK_STATS_STRIDE]) gain {1 game, a black win / a white
 *     win / a draw, L}; the env is reset.
 *   the next root: the canonical view (channel 0 = the side to move) of the row's position after the ply (a fresh board
 *   after a reset) into obs [N][2][m][n] of obs_dtype and (optional) legal_mask u8[N][C].
 * visits int32 [N][C]; temp_plies >= 0.  One wave per row.  Every host check runs before anything is enqueued. */
#define MNK_Z_UNKNOWN (-128)
int mnk_search_selfplay_step(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, const int32_t* visits,
                             int temp_plies, uint64_t seed, const uint64_t* seed_dev, uint64_t step,
                             const uint64_t* step_dev, int64_t env_id0, int64_t T, uint64_t* ring_planes,
                             uint16_t* ring_visits, int8_t* ring_z, void* obs, int obs_dtype, uint8_t* legal_mask,
                             int64_t* stats, int32_t* err, void* stream);
/* mnk_search_selfplay_step for a search that hands out its move and a policy target (mnk_puct_step_gumbel): the same
 * launch with two differences.  The move of row i is actions[i] (int64 [N]) instead of a draw from the visits -- no Philox
 * word is used, so there is no seed or env_id0: an action outside [0, C) sets MNK_ERR_ACTION_RANGE, one on an occupied
 * cell MNK_ERR_ILLEGAL_MOVE, and the env is then not played, exactly as a row of MNK_ERR_VISITS above.  The ring's u16
 * visits of a free cell are min(65535, rint(fl32(policy_a * 65535))) (policy f32 [N][C]; ties to even; 0 for anything
 * not above 0), so the ring format and mnk_search_gather stay as they are: the gather's n / sum n gives the target back
 * to 1.5e-5.  Outcome labels, resets, stats, the next root and every other argument are as above. */
int mnk_search_selfplay_step_moves(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, const float* policy,
                                   const int64_t* actions, uint64_t step, const uint64_t* step_dev, int64_t T,
                                   uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* obs, int obs_dtype,
                                   uint8_t* legal_mask, int64_t* stats, int32_t* err, void* stream);
/* Search self-play with a search budget per row and ply: ONE launch per evaluator call, in the place of mnk_puct_step and
 * mnk_search_selfplay_step.  A row that has spent the budget of its ply plays it in this launch and starts the search of
 * the position it reached at once, so rows finish their searches at different times ("playout cap randomisation": most
 * plies get a small budget and only move the game on, a random fraction get the full one and become policy targets).
 * The workspace is that of mnk_puct_begin with iterations (leaves = 1), set up by mnk_puct_begin on the current roots (the
 * canonical views of planes / meta); priors [N][C] and values [N] (f32 or bf16) are the evaluator's outputs for the
 * leaves of the call before (of mnk_puct_begin first).  row_plies u64 [N], in and out: p_i = the plies row i has played.
 * 1 <= fast_iterations <= iterations <= MNK_PUCT_ITERS_MAX; full_threshold in [0, 2^32].  Row i of a launch:
 *   1. backup: a pending evaluation is backed up by mnk_puct_step's rule, bit for bit, from batch row i.
 *   2. budget: u = Philox(seed [or *seed_dev], env_id0 + i, p_i, MNK_STREAM_BUDGET); the ply is FULL iff (uint64)u <
 *      full_threshold (0: never, 2^32: always); B = iterations when FULL, else fast_iterations.  Nothing is stored: the
 *      budget of a ply is a function of (seed, row id, p_i) alone.
 *   3. it = n_root - 1, the iterations backed up since the row's evaluation 0.
 *      it < B: mnk_puct_step's selection; the new leaf's view goes to row i of leaf_obs / leaf_mask; fresh[i] = 0.
 *      it >= B: the ply ends in this launch by mnk_search_selfplay_step's rule with p_i in the place of the global ply:
 *        t = p_i mod T, x = Philox(seed, env_id0 + i, p_i, MNK_STREAM_SELFPLAY), n_a = the root children's visits
 *        clamped to [0, 65535] on free cells, the move from n_a (temperature 1 while the game's move count g <
 *        temp_plies, else 0).  Ring row (t, i): the planes before the ply, z unknown, and the visits -- n_a on a FULL ply,
 *        all zero on a fast one (a value target only: mnk_search_gather gives a zero policy for a zero sum).  Then the
 *        ply, the outcome labels of a game that ends (t - d mod T, d < L), stats and the reset, as there.  Then p_i += 1,
 *        plies_max (optional device u64) = max(plies_max, p_i) -- the plies the most advanced row has written -- and
 *        the row's tree is set up afresh on the position reached (what mnk_puct_begin writes: the root alone, its
 *        evaluation pending), that root is the leaf, fresh[i] = 1.
 *   4. a root without a legal cell (only a state handed in has one): MNK_ERR_VISITS, err[1] = i; nothing of the row
 *      changes -- no backup, no ring record, p_i stays -- and it shows its root again, fresh[i] = 0, in every launch.  The
 *      same holds for a row whose root has no visit on a free cell of planes when its budget is spent (a workspace that
 *      was not set up on this position).  A selection that finds no leaf (a full tree: impossible in a workspace that
 *      mnk_puct_begin set up, where nodes <= n_root <= iterations while the budget is unspent) leaves nothing pending, so
 *      the row's n_root cannot advance: it shows its root again and reports MNK_ERR_VISITS in every launch as well.
 * So with full_threshold = 2^32 and rows that start together, iterations + 1 launches are one ply of mnk_puct_begin,
 * iterations + 1 mnk_puct_step and mnk_search_selfplay_step, bit for bit, without the two launches around the search.
 * fresh (optional u8 [N]) tells the caller which rows of the next evaluator call are roots.  Rows are not in step: ring
 * slot (t, i) is written when row i gets there, so a slot that a row has not reached yet holds whatever it held (z
 * unknown in a new ring: weight 0).  T >= C; temp_plies >= 0; c as in mnk_puct_step.  One wave per row; every id read
 * from the workspace is clamped to the row.  Every host check runs before anything is enqueued. */
int mnk_search_selfplay_advance(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies, int64_t T,
                                uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs,
                                int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh, uint64_t* plies_max, int64_t* stats,
                                int32_t* err, void* stream);
/* mnk_search_selfplay_advance with two of the lockstep player's options built in: Dirichlet noise on the roots and the
 * solver.  Every argument up to err, and every rule not named here, is mnk_search_selfplay_advance's.
 *   options off: with solver = 0 and noise_alpha = 0 the launch is mnk_search_selfplay_advance, bit for bit (root_priors,
 *     when given, still receives the roots' plain priors as below).
 *   noise: noise_alpha = 0 means off; otherwise alpha is finite and > 0 and noise_eps lies in [0, 1].  It applies to the
 *     backup of a row's evaluation 0 -- the pending leaf that is the root of a fresh tree (what mnk_puct_begin and the
 *     end of a ply leave pending).  The root is NOISED iff its ply p_i is FULL (step 2 above) or noise_fast != 0.  On a
 *     NOISED root the priors stored on the root's free cells are mnk_puct_root_noise's P', by that rule word for word
 *     (draws, Marsaglia and Tsang, the boost in log space, the maximum taken out before the sum, the three correctly
 *     rounded f32 operations of the mix), with step = p_i, row id = env_id0 + i, seed [or *seed_dev], leaves = 1 and the
 *     free cells those of the root's planes.  Nothing but the tree's own prior row is written: the evaluator's tensor is
 *     not.  A root that is not NOISED stores the plain priors.  noise_fast = 0 is KataGo's rule: the fast searches only
 *     move the game on and play at full strength; noise_fast = 1 noises every root.  So the noise of a ply is a function
 *     of (seed, row id, p_i) alone, like its budget.  Precondition (the host cannot see row_plies): p_i < 2^52 / C4 - 1,
 *     mnk_puct_root_noise's bound on step; no row reaches it.
 *   root_priors (optional, f32 [N][C]): row i is written in exactly those launches that back up row i's evaluation 0,
 *     NOISED or not, with the C values the root then holds; on occupied cells the evaluator's prior as given (a bf16
 *     prior widened exactly), like `out` of mnk_puct_root_noise.
 *   solver: with solver != 0 the backup and the selection are mnk_puct_step_solver's at leaves = 1.  In step 3 the ply of
 *     row i ends in this launch iff it >= B or the root has a proof.  The n_a of the move and of the ring record are the
 *     adjusted counts of mnk_puct_step_solver (if some root child is WIN, only the WIN children count; otherwise the
 *     LOSS children are dropped; if that leaves nothing, the raw counts), clamped to [0, 65535] on free cells as before.
 *     A FULL ply that ends by proof is a policy target like any FULL ply; a fast ply still records zero visits.  The
 *     fresh tree of the position reached starts with no proof.  Ring slot, the Philox word of the move, outcome labels,
 *     stats, the reset, plies_max, fresh and the rows that report MNK_ERR_VISITS are unchanged.
 * So with full_threshold = 2^32 and rows that start together, iterations + 1 launches with noise are one ply of the
 * lockstep player with mnk_puct_root_noise at step = the ply, bit for bit; with the solver the games are the lockstep
 * solver's, played without the launches in which a proven root would idle.
 * solver and noise_fast in {0, 1}; noise_alpha 0, or finite and > 0; noise_eps in [0, 1] (whether or not alpha is 0);
 * C <= 1024; every host check, the old entry point's included, runs before anything is enqueued. */
int mnk_search_selfplay_advance_opts(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                     int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                     int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                     uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                     int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                     uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                     float noise_eps, int noise_fast, float* root_priors, void* stream);
/* mnk_search_selfplay_advance_opts for rows that keep the played move's subtree from ply to ply (the lockstep player's
 * mnk_puct_rebase, inside the one launch).  Every argument up to root_priors, and every rule not named here, is
 * mnk_search_selfplay_advance_opts's; iterations stays the full budget I.
 *   tree_iterations: the workspace's layout parameter, node capacity - 1: the number given to mnk_puct_workspace_bytes and
 *     to mnk_puct_begin, which sets the workspace up.  iterations <= tree_iterations <= MNK_PUCT_ITERS_MAX; every id read
 *     from the workspace is clamped by it.
 *   keep_nodes: the most nodes a row carries over a ply, 1 <= keep_nodes <= tree_iterations + 1 - iterations, so that the
 *     tree cannot fill within a ply.
 *   carried (int32 [N][2], required, caller-owned): an output and the row's state -- {the nodes kept, the new root's n} of
 *     row i's current search, {0, 0} when it began afresh.  Zero it when mnk_puct_begin sets the workspace up.
 *   end of a ply: after the move, the ring record, the labels and the reset, exactly as before -- if the game did not end
 *     and the root's child through the move exists and is not terminal, the row keeps that child's subtree: what
 *     mnk_puct_rebase does for a path of one ply (the nodes stay in creation order, the first keep_nodes of them; a kept
 *     node keeps n, w, its move, its terminal kind, its proof, its priors and its children; a dropped child becomes "none
 *     yet"; the kept child is node 0 with info 0), the header says "pending, renew" (state 1 | 8), and carried[i] = {nodes
 *     kept, the new root's n}.  With the solver the new root keeps one thing more: the proof it had as a child, when the
 *     kept children still justify it -- a root proven a win for its side to move has a kept WIN child, a drawn one a kept
 *     DRAW child, a lost one any kept child (the truncation keeps the oldest nodes, so the child that proved the root may
 *     be gone: the root is then unknown, as in mnk_puct_rebase, and searches on).  Otherwise -- a game that
 *     ended, a missing child -- the row's tree is set up afresh as before and carried[i] = {0, 0}.  fresh[i] = 1 either
 *     way: it means "this row of the next batch is a root".
 *   budget: n0 = max(carried[i][1], 1); it = n_root - n0, the iterations run in the row's ply (a saturating subtraction:
 *     whatever carried holds, nothing leaves the row).  The ply ends iff it >= B or, with the solver, the root has a proof;
 *     B is I or fast_iterations by the same Philox word.  On a fresh row this is n_root - 1 as before.  The backup of a
 *     carried root's evaluation only renews its priors (mnk_puct_rebase's evaluation 0), so it = 0 in that launch; with the
 *     solver a carried root that has a proof plays in that launch.  The budget counts the iterations of this ply, not the
 *     root's total visits: the lockstep player's rule.
 *   noise and root_priors act on "the pending leaf is the row's root, depth 0", carried or not: the noised priors replace
 *     a carried root's priors on its free cells.
 * So with full_threshold = 2^32 and rows that start together, iterations + 1 launches are one ply of mnk_puct_rebase (with
 *   tree_iterations and keep_nodes), iterations + 1 mnk_puct_step and mnk_search_selfplay_step, bit for bit -- without
 *   the solver: with it a ply ends as soon as its root is proven, and a carried root starts with its proof where the
 *   lockstep solver's starts unknown, so the games are not the lockstep solver's launch for launch.
 * LDS: a workgroup holds, besides its static stage, 4 * C doubles when noise_alpha > 0 and the carry's two id maps,
 *   4 * 2 * (tree_iterations + 2, rounded up to even) u16, all dynamic.  The host computes the total and returns MNK_EINVAL
 *   before anything is enqueued when it exceeds what a plain launch may ask for on the current device (the device's
 *   limit, read once; 64 KiB where no device answers): at 64 KiB, 32 x 31 with noise and tree_iterations = 2048 is the
 *   one kind of case (4 * 992 * 8 + 4 * 2 * 2050 * 2 + 1024 static = 65 568 B); 19 x 19 at tree_iterations = 512 asks for
 *   8 608 B without noise and 20 160 B with it.  The limit is that of the device current at the first call, kept for the
 *   process.  A device that reports more than 64 KiB is taken at its word; no launch above 64 KiB has been run (it would
 *   fail through the launch status, MNK_ELAUNCH, not fault).
 * Every host check -- those of mnk_search_selfplay_advance_opts, the two ranges, carried != NULL, the LDS total -- runs
 * before anything is enqueued; N = 0 returns MNK_OK after them. */
int mnk_search_selfplay_advance_keep(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                     int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                     int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                     uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                     int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                     void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                     uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                     float noise_eps, int noise_fast, float* root_priors, int tree_iterations,
                                     int keep_nodes, int32_t* carried, void* stream);
/* mnk_search_selfplay_advance_opts and mnk_search_selfplay_advance_keep with FIRST-PLAY URGENCY in the selection (the
 * rule: mnk_puct_step_fpu at leaves = 1, with or without the solver): their arguments, then fpu and fpu_root before the
 * stream, and nothing else differs -- the backup, the budget, the end of a ply, the noise, the carry.  With full_threshold
 * = 2^32 and rows that start together the launches are the lockstep player's with mnk_puct_step_fpu in the place of its
 * step, bit for bit, with the exceptions their siblings state for the solver.  fpu, fpu_root: finite, >= 0 (else
 * MNK_EINVAL); every host check runs before anything is enqueued; N = 0 returns MNK_OK after them. */
int mnk_search_selfplay_advance_opts_fpu(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                         int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                         int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                         uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                         int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                         void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                         uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                         float noise_eps, int noise_fast, float* root_priors, float fpu, float fpu_root,
                                         void* stream);
int mnk_search_selfplay_advance_keep_fpu(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                         int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                         int priors_dtype, const void* values, int values_dtype, float c, int temp_plies,
                                         uint64_t seed, const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies,
                                         int64_t T, uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z,
                                         void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                         uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                         float noise_eps, int noise_fast, float* root_priors, int tree_iterations,
                                         int keep_nodes, int32_t* carried, float fpu, float fpu_root, void* stream);
/* mnk_search_selfplay_advance_opts (fpu_on = 0) or mnk_search_selfplay_advance_opts_fpu (fpu_on = 1) with FORCED PLAYOUTS
 * AND POLICY TARGET PRUNING (the rule: mnk_puct_step_forced at leaves = 1, with or without the solver): their arguments,
 * then fpu_on and forced_k before the stream.  Row i's ply p_i FORCES iff its root is NOISED by the rule above -- the ply
 * is FULL, or noise_fast != 0 -- whether or not noise_alpha is 0.  On a ply that FORCES the selection at the root is
 * mnk_puct_step_forced's, and in the launch that ends the ply n' = the clamped counts the move would be drawn from above,
 * n'' = their pruned counts by mnk_puct_step_forced's rule; the move is drawn from n'', and a FULL ply records n'' in the
 * ring (a fast ply zero visits, as before).  A ply that does not force is searched, played and recorded exactly as by
 * mnk_search_selfplay_advance_opts[_fpu].  Nothing else differs: the backup, the budget, the noise, ring slot, the Philox
 * word of the move, labels, stats, the reset.  With full_threshold = 2^32 and rows that start together the launches are
 * the lockstep player's with mnk_puct_step_forced in the place of its step, bit for bit, with the exceptions
 * mnk_search_selfplay_advance_opts states for the solver.  forced_k: finite, > 0; fpu_on in {0, 1}; fpu and fpu_root are
 * checked when fpu_on = 1 (else MNK_EINVAL); every host check runs before anything is enqueued; N = 0 returns MNK_OK after
 * them. */
int mnk_search_selfplay_advance_opts_forced(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n,
                                            int k, int iterations, int fast_iterations, uint64_t full_threshold,
                                            const void* priors, int priors_dtype, const void* values, int values_dtype,
                                            float c, int temp_plies, uint64_t seed, const uint64_t* seed_dev,
                                            int64_t env_id0, uint64_t* row_plies, int64_t T, uint64_t* ring_planes,
                                            uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs, int leaf_dtype,
                                            uint8_t* leaf_mask, uint8_t* fresh, uint64_t* plies_max, int64_t* stats,
                                            int32_t* err, int solver, float noise_alpha, float noise_eps, int noise_fast,
                                            float* root_priors, float fpu, float fpu_root, int fpu_on, float forced_k,
                                            void* stream);
/* mnk_search_selfplay_advance_opts for rows that search with L = leaves slots per row and evaluator call (the lockstep
 * player's mnk_puct_step_leaves / mnk_puct_step_solver inside the one launch).  Every argument but leaves and row_sims,
 * and every rule not named here, is mnk_search_selfplay_advance_opts's.
 *   workspace: that of mnk_puct_begin_leaves(.., iterations, leaves, ..), set up by it on the current roots.
 *   batch layout: mnk_puct_step_leaves's -- slot j of row i is batch row i * L + j of leaf_obs [N*L][2][m][n], leaf_mask
 *     [N*L][C], priors [N*L][C] and values [N*L].  root_priors stays [N][C] and fresh [N]: fresh[i] = 1 means "slot 0 of
 *     row i is a root".
 *   row_sims (u32 [N], in and out, required, caller-owned): the simulations row i's current ply has been offered.  Zero it
 *     whenever mnk_puct_begin_leaves sets the workspace up.
 *   1. backup: the row's pending slots are backed up in slot order by mnk_puct_step_leaves's rule (with solver != 0,
 *      mnk_puct_step_solver's).  The noise and root_priors act on slot 0 when it is evaluation 0 (state 1, depth 0),
 *      exactly as above, with the evaluator's row i * L.
 *   2. budget: unchanged -- the Philox word of (seed, row id, p_i) decides between B = iterations and B = fast_iterations.
 *   3. the ply ends iff row_sims[i] >= B or, with the solver, the root has a proof.
 *      It ends by the rule above word for word: ring slot, the move from the (adjusted) counts, labels, stats, the reset,
 *        p_i += 1, plies_max.  Then the row's tree is set up afresh on the position reached, as mnk_puct_begin_leaves
 *        leaves it: slot 0 is the root, pending; slots 1 .. L-1 are void and show the root's view.  row_sims[i] = 0,
 *        fresh[i] = 1.
 *      It goes on with s = min(L, B - row_sims[i]): slots 0 .. s-1 select one after the other under virtual visits --
 *        mnk_puct_step_leaves's selection, the slots that the walk makes void included -- and slots s .. L-1 are void.
 *        row_sims[i] += s, fresh[i] = 0.  So a budget is met exactly, whatever B mod L is.
 *      The counter, not n_root - 1: a slot that the walk makes void is a simulation the lockstep player loses as well, and
 *        a row that counted visits would search longer than the lockstep player's.  With the counter a ply of budget B
 *        takes exactly ceil(B / L) + 1 launches unless a proof ends it sooner.
 *   4. the rows that report MNK_ERR_VISITS are those of mnk_search_selfplay_advance's step 4 (a selection that finds no
 *      leaf: one whose slot 0 finds none); nothing of such a row changes, row_sims[i] stays, and all L batch rows of the
 *      row show its root.
 * So (a) with leaves = 1 the launch is mnk_search_selfplay_advance_opts, bit for bit, on every row that reports no error,
 * and row_sims[i] = n_root - 1 whenever the launch reads it; (b) with full_threshold = 2^32 and rows that start together,
 * iterations / L + 1 launches are one ply of the lockstep player with leaves = L (mnk_puct_begin_leaves, the steps,
 * mnk_search_selfplay_step), with noise mnk_puct_root_noise at step = the ply, bit for bit.
 * leaves in [1, MNK_PUCT_LEAVES_MAX]; iterations % leaves = 0 (the workspace's condition; fast_iterations is free in [1,
 * iterations]); row_sims != NULL.  LDS and the kernel's shape are as above; the slots' paths stay in the workspace.  Every
 * host check, those of mnk_search_selfplay_advance_opts included, runs before anything is enqueued; N = 0 returns MNK_OK
 * after them. */
int mnk_search_selfplay_advance_leaves(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                       int iterations, int fast_iterations, int leaves, uint64_t full_threshold,
                                       const void* priors, int priors_dtype, const void* values, int values_dtype, float c,
                                       int temp_plies, uint64_t seed, const uint64_t* seed_dev, int64_t env_id0,
                                       uint64_t* row_plies, int64_t T, uint64_t* ring_planes, uint16_t* ring_visits,
                                       int8_t* ring_z, void* leaf_obs, int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh,
                                       uint64_t* plies_max, int64_t* stats, int32_t* err, int solver, float noise_alpha,
                                       float noise_eps, int noise_fast, float* root_priors, uint32_t* row_sims,
                                       void* stream);
/* mnk_search_selfplay_advance for rows whose root is a GUMBEL ROOT (the lockstep player's mnk_puct_gumbel_root,
 * mnk_puct_step_gumbel and mnk_search_selfplay_step_moves inside the one launch).  The arguments are those of
 * mnk_search_selfplay_advance up to err without temp_plies -- the Gumbel draw is the exploration at every ply -- and every
 * rule not named here is mnk_search_selfplay_advance's.  A round stays one evaluator call and one launch.
 *   considered, c_visit, c_scale, gumbel_scale: those of mnk_puct_step_gumbel / mnk_puct_gumbel_root, with their ranges.
 *   table_full (u16 [considered + 1][iterations]) and table_fast (u16 [considered + 1][fast_iterations]): what
 *     mnk_puct_gumbel_schedule fills for the two budgets; they may be the same pointer when the budgets are equal.
 *   gscore (f32 [N][C]) and vroot (f32 [N]): caller-owned, the rows' state between launches.
 *   workspace: that of mnk_puct_begin with iterations, one leaf per row -- the workspace mnk_puct_begin_leaves(leaves = 1)
 *     sets up.
 * Row i of a launch, p_i its ply count:
 *   1. backup: mnk_puct_step's rule from batch row i, bit for bit.  When the pending leaf is evaluation 0 of a fresh tree
 *      (state 1, depth 0), the same launch writes gscore row i and vroot[i] by mnk_puct_gumbel_root's rule word for word
 *      (f64 arithmetic with the full-precision logarithm, the clamp at 2^-126, the Philox layout over C4, the product
 *      rounded, then the sum, then the one rounding to f32 -- fl32(gumbel_scale * g_a + l_a) -- and -inf on occupied
 *      cells) with step =
 *      p_i, row id = env_id0 + i, seed [or *seed_dev]; the free cells are those of the root's planes, the priors and the
 *      value the evaluator's batch row i.  So the Gumbel draw of a ply is a function of (seed, row id, p_i) alone, as its
 *      budget is.  The evaluator's tensors are never written; gscore row i and vroot[i] are written in no other launch.
 *      Precondition (the host cannot see row_plies): p_i < 2^56 / C4 - 1, mnk_puct_gumbel_root's bound on step.
 *   2. budget: unchanged -- the MNK_STREAM_BUDGET word of (seed, row id, p_i) decides between B = iterations with
 *      table_full (row stride iterations) and B = fast_iterations with table_fast (row stride fast_iterations).
 *   3. it = n_root - 1.
 *      it < B: mnk_puct_step_gumbel's selection -- F = the root's free cells, v* = table_B[min(considered, F)][it], the
 *        root's cell of maximal key among those with n_a = v* (all free cells if there is none), ties to the lowest cell,
 *        and below the root mnk_puct_step's walk; fresh[i] = 0.
 *      it >= B: the ply ends in this launch; fresh[i] = 1.  The move is mnk_puct_step_gumbel's: the free cell of maximal
 *        key among those of the most visits, ties to the lowest cell.  Ring slot (p_i mod T, i) takes the planes before
 *        the ply and z unknown.  On a FULL ply the visits are the improved policy of mnk_puct_step_gumbel (from vroot[i]
 *        and the root's stored priors) quantised by mnk_search_selfplay_step_moves's rule, min(65535, rint(fl32(policy_a *
 *        65535))) on free cells; on a fast ply they are all zero and no policy is computed.  No MNK_STREAM_SELFPLAY word
 *        is used.  Then mnk_search_selfplay_advance's end of a ply: the ply, the outcome labels, stats, the reset,
 *        p_i += 1, plies_max, and a fresh tree on the position reached, whose root is the next leaf.
 *   4. the rows that report MNK_ERR_VISITS are mnk_search_selfplay_advance's: a root without a legal cell; a selection
 *      that finds no leaf; a spent row whose move is not a free cell of planes (a workspace that is not this position's).
 *      Nothing of such a row changes and it shows its root again.
 * So with full_threshold = 2^32 and rows that start together, iterations + 1 launches are one ply of the lockstep Gumbel
 * player -- mnk_puct_begin_leaves(leaves = 1), mnk_puct_gumbel_root at step = the ply, iterations + 1 mnk_puct_step_gumbel,
 * mnk_search_selfplay_step_moves -- bit for bit, with two launches per ply fewer and the prep launch saved.
 * Every host check -- those of mnk_search_selfplay_advance, the ranges of considered, c_visit, c_scale and gumbel_scale,
 * non-NULL tables, gscore and vroot, C <= 1024 -- runs before anything is enqueued; N = 0 returns MNK_OK after them.  One
 * wave per row; every id read from the workspace is clamped to the row. */
int mnk_search_selfplay_advance_gumbel(void* workspace, uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k,
                                       int iterations, int fast_iterations, uint64_t full_threshold, const void* priors,
                                       int priors_dtype, const void* values, int values_dtype, float c, uint64_t seed,
                                       const uint64_t* seed_dev, int64_t env_id0, uint64_t* row_plies, int64_t T,
                                       uint64_t* ring_planes, uint16_t* ring_visits, int8_t* ring_z, void* leaf_obs,
                                       int leaf_dtype, uint8_t* leaf_mask, uint8_t* fresh, uint64_t* plies_max,
                                       int64_t* stats, int32_t* err, int considered, float c_visit, float c_scale,
                                       float gumbel_scale, const uint16_t* table_full, const uint16_t* table_fast,
                                       float* gscore, float* vroot, void* stream);
/* A minibatch of ring records: sample b is the flat id idx[b] = t*N + i (negative ids wrap, an id outside [0, T*N) sets
 * MNK_ERR_ACTION_RANGE as in mnk_gather_obs and gives zero planes, policy, value and weight) under symmetry s = sym[b]
 * (sym int8 [B] or NULL = the identity).  Output cell (r, c) reads source cell (r', c'): start from (r, c); if s & 4,
 * (r, c) <- (c, r) (square boards only); if s & 1, r <- m-1-r; if s & 2, c <- n-1-c.  An id s outside [0, 8), or >= 4 on
 * a board that is not square, sets MNK_ERR_SYMMETRY (err[1] = b), is read as the identity and gets weight 0.
 *   obs [B][2][m][n] (obs_dtype) and legal_mask u8[B][C]: the record's planes under the map (what mnk_gather_obs writes
 *     for s = 0);
 *   policy f32[B][C]: fdiv((float)n_src, (float)sum n) over the record's ring visits (one correctly rounded division;
 *     0 when the sum is 0);
 *   value f32[B] = z, weight f32[B] = 1; value = weight = 0 where z = MNK_Z_UNKNOWN.
 * Every output may be NULL. */
int mnk_search_gather(const uint64_t* ring_planes, const uint16_t* ring_visits, const int8_t* ring_z, int64_t T,
                      int64_t N, int m, int n, const int64_t* idx, const int8_t* sym, int64_t B, void* obs, int obs_dtype,
                      uint8_t* legal_mask, float* policy, float* value, float* weight, int32_t* err, void* stream);

/* ---- the random-policy rollout of BASELINE.json (RandomPolicy.act -> env.step -> env.reset(done)),
 * T plies per env in one launch with the state held in registers.
 * rec_planes u64[T][R][N]: the position BEFORE each ply (record rows, see the top of this file);
 * rec_meta u32[T][N]: MNK_REC_* word;
 * stats (optional) int64[MNK_STATS_REPLICAS][MNK_STATS_STRIDE] += {episodes finished, black wins,
 * white wins, draws, sum of episode lengths} spread over the replicas (sum the rows to read a counter).
 * rec_planes / rec_meta may be NULL together (state-only rollout); act_log may be NULL. */
int mnk_rollout_random(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, int T,
                       uint64_t seed, uint64_t step0, int64_t env_id0,
                       uint64_t* rec_planes, uint32_t* rec_meta, int64_t* stats,
                       void* act_log, int act_bytes, void* stream);
/* Which kernel mnk_rollout_random runs for a launch: every form computes the same bits, so this query is the only
 * place the choice shows.  Needs no GPU; uses the configuration the launcher uses (mnk_reload_config re-reads it).
 * `records` / `act_bytes`: whether the launch has record pointers / its log format (0: no log); `jit_failed`: the
 * answer once the board's run-time compiled kernel has failed to compile.  Returns one of the forms below ORed with
 * the flags, 0 when nothing would be launched (N or T is 0), or the negative status mnk_rollout_random gives for the
 * same arguments (MNK_ELAUNCH: the board's only kernel is the compiled one, and it failed).
 * The rules, first match wins.  builtin: one of the five boards with ahead-of-time variants; fits32: (T * R + 1) * N * 8
 * < 2^32, the record rows of the launch fit 32-bit byte offsets; small: MNK_ROLLOUT_PAIR if set, else N <= 32 768.
 *  1. MNK_ROLLOUT_FORM=ws2|ws4 on 9x9x5 / 19x19x5 without a log: that form, at any N (other launches ignore the knob).
 *  2. not builtin, and the compiled kernel is wanted (R > 16: always, it is the only one -- else MNK_JIT if set, else
 *     N * T >= 2^20) and has not failed: MNK_ROLLOUT_JIT, as PAIR when fits32, small, the log is none / U8 / U16 and
 *     MNK_ROLLOUT_FORM is not `lane`, else as LANE; SADDR (of the LANE kernel, which is also the next try after a PAIR
 *     kernel that does not compile) iff records, N <= 65 536, fits32 and not MNK_ROLLOUT_SADDR=0.
 *  3. PAIRW on the five-in-a-row builtin boards when fits32, the log is none / U8 / U16 / U8P1, and either
 *     MNK_ROLLOUT_FORM=pairw (any N) or small and n >= 13 -- unless MNK_ROLLOUT_FORM=pair and the log is not U8P1.
 *  4. PAIR on builtin boards when fits32, small and the log is none / U8 / U16.
 *  5. LANE otherwise; SADDR as in 2, on builtin boards only.  MNK_ROLLOUT_FORM=lane gets here only where 3 and 4 do
 *     not apply: by itself it does NOT select the one-lane kernel on a builtin board at a small batch
 *     (MNK_ROLLOUT_PAIR=0 does). */
#define MNK_ROLLOUT_LANE 1   /* one lane per env */
#define MNK_ROLLOUT_PAIR 2   /* two lanes per env, the scan directions split */
#define MNK_ROLLOUT_PAIRW 3  /* two lanes per env, the board's words split */
#define MNK_ROLLOUT_WS2 4    /* two / four waves per group of 64 envs */
#define MNK_ROLLOUT_WS4 5
#define MNK_ROLLOUT_FORM_MASK 0xF
#define MNK_ROLLOUT_SADDR 0x10     /* the one-lane kernel's record stores use 32-bit offsets */
#define MNK_ROLLOUT_JIT 0x20       /* the board's run-time compiled kernel is tried first */
#define MNK_ROLLOUT_JIT_ONLY 0x40  /* (with MNK_ROLLOUT_JIT) and there is no ahead-of-time kernel behind it */
int mnk_rollout_form(int64_t N, int m, int n, int k, int T, int records, int act_bytes, int jit_failed);

/* Boards other than 3x3x3, 9x9x5, 13x13x5, 15x15x5 and 19x19x5 have no ahead-of-time specialisation of the rollout
 * kernel; mnk_rollout_random compiles one with hiprtc (about a second, once per board / record / log-width
 * combination and process) when a launch covers at least 2^20 env-steps -- environment MNK_JIT=1: always, MNK_JIT=0:
 * never (the kernels with run-time geometry then run, 3-5x slower).  Results are identical either way.  The first
 * such launch compiles and loads a code object: make it outside a hipGraph capture (later launches only enqueue).
 * mnk_jit_compile_rollout only compiles (no GPU needed): code object bytes, or a negative status with the
 * compiler's log in mnk_jit_last_error(). */
int64_t mnk_jit_compile_rollout(int m, int n, int k, int record, int act_bytes);
/* Round 4: two more kernels exist as run-time specialisations -- the replay of an action log (mnk_replay_actions) and the
 * two-lanes-per-env form of the rollout (batches of up to 32 768 envs).  Boards whose planes take more than 512 bits
 * (25x25, 31x31 ...) have NO ahead-of-time rollout / replay kernel: theirs are always compiled at run time (~2 s).
 * mnk_jit_compile_kernel is mnk_jit_compile_rollout for any of the three (kind below; act_bytes of a replay = the log
 * format it reads). */
#define MNK_JIT_ROLLOUT 0
#define MNK_JIT_REPLAY 1
#define MNK_JIT_ROLLOUT_PAIR 2
int64_t mnk_jit_compile_kernel(int m, int n, int k, int record, int act_bytes, int kind);
const char* mnk_jit_last_error(void);
/* ABI 6: the API-level kernels are specialised at run time too.  On a board without a built-in variant the kernels behind
 * mnk_step / mnk_step_random / mnk_observe / mnk_sample_legal / mnk_unpack_records / mnk_gather_obs / mnk_selfplay_* start
 * on generic code (run-time shift amounts, table write-out) and switch to the board's own variant -- compile-time
 * geometry, the packed write-out, and for mnk_selfplay_*_logits the draw folded into the step kernel for any row width --
 * once they are hot: 1 024 launches or 2^26 items of that kernel on that board in this process (about a second of hiprtc per
 * kernel, then a code object load).  MNK_JIT_API=1 (or MNK_JIT=1): at the first launch; =0: never.  Results are identical
 * either way.  Nothing is compiled while the launch's stream is being captured into a hipGraph: call mnk_jit_prepare
 * before the capture.  `kind` / the bits of `kinds`: */
#define MNK_JIT_API_STEP 0            /* mnk_step, full batch */
#define MNK_JIT_API_STEP_DRAW 1       /* mnk_step_random */
#define MNK_JIT_API_STEP_SUBSET 2     /* mnk_step with active_idx */
#define MNK_JIT_API_OBSERVE 3         /* mnk_observe, mnk_unpack_boards */
#define MNK_JIT_API_SAMPLE_LEGAL 4    /* mnk_sample_legal */
#define MNK_JIT_API_UNPACK_RECORDS 5  /* mnk_unpack_records */
#define MNK_JIT_API_GATHER_OBS 6      /* mnk_gather_obs */
#define MNK_JIT_API_SP_PRE 7          /* mnk_selfplay_pre */
#define MNK_JIT_API_SP_POST 8         /* mnk_selfplay_post */
#define MNK_JIT_API_SP_STEP 9         /* mnk_selfplay_step_random */
#define MNK_JIT_API_SP_DRAW 10        /* + 3 * logits form (0 f32, 1 bf16, 2 none) + (0 pre, 1 post, 2 step_random):
                                         mnk_selfplay_pre_logits / _post_logits / _step_random_logits */
#define MNK_JIT_API_SP_TACTICAL 19      /* mnk_selfplay_step_tactical */
#define MNK_JIT_API_SP_TACTICAL_DRAW 20 /* + logits form (0 f32, 1 bf16, 2 none): mnk_selfplay_step_tactical_logits */
#define MNK_JIT_API_SAMPLE_TACTICAL 23  /* mnk_sample_tactical */
#define MNK_JIT_API_COUNT 24
/* compiles only (no GPU needed): code object bytes, or a negative status with the log in mnk_jit_last_error() */
int64_t mnk_jit_compile_api(int m, int n, int k, int kind);
/* compiles and loads, on the current device, the variants named by the bits of `kinds` NOW (kinds == 0: of every kernel
 * launched on this board so far -- after a warm-up run, exactly what a capture is going to launch): the number ready, 0
 * for a board with a built-in variant or with MNK_JIT_API / MNK_JIT = 0, or a negative status */
int mnk_jit_prepare(int m, int n, int k, int64_t kinds);
/* Compiled code objects are kept on disk and reused by later processes: directory $MNK_JIT_CACHE (default
 * $XDG_CACHE_HOME/mnk_hip or ~/.cache/mnk_hip; "0" or "off": no cache), one file per (this build's embedded sources, hiprtc
 * version, options, kernel), checksummed, written by rename.  mnk_jit_stats: out4 = {programs compiled by hiprtc, code
 * objects read from the cache instead, written to it, failed compilations} of this process. */
int mnk_jit_stats(int64_t* out4);
/* 1 when the board's own variant of `kind` is loaded on the current device (what the next launch will run), else 0 */
int mnk_jit_api_ready(int m, int n, int k, int kind);

/* The multi-GPU exchange format.  A shard's rollout is a pure function of its chunk-start state and
 * its actions, so the action log, optionally written by mnk_rollout_random, is what ranks all-gather
 * (1-2 B per env-step instead of the 28 B packed record or the reference's 750 B RolloutBuffer row).
 * Layout: four plies per word, act_log u32[ceil(T/4)][N] (act_bytes MNK_ACT_U8: one byte per action, boards with
 * <= 256 cells) or u64[ceil(T/4)][N] (MNK_ACT_U16: 16 bits per action); the action of ply 4q+j is field j
 * (little-endian) of word [q][i]; fields past T are 0.  MNK_ACT_BITS7 (boards with <= 128 cells): 7 bits per action
 * as one bit stream per env, see above.  With a log, step0 must be a multiple of 4 (every chunk but the last a
 * multiple of 4 plies).  A receiver that replays every chunk of a shard in order holds that shard's chunk-start state
 * itself, so after the first chunk the log alone is the message (selfplay/random_rollout.py).
 * mnk_replay_actions re-plays a log from `planes`/`meta` (updated in place, like the rollout) and
 * rebuilds rec_planes / rec_meta bit-identical to what the sender recorded (both may be NULL to only
 * advance the state).  An action >= m*n in the log is reported through err. */
/* 32-bit words per env of a T-ply log in format `act_bytes` (0 for an unknown format): U8 ceil(T/4), U16 2 ceil(T/4),
 * BITS7 ceil(7 ceil(T/4) / 8), U8P1 ceil(T/4) + ceil(T/32) */
int mnk_action_log_words(int act_bytes, int T);
int mnk_replay_actions(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, int T,
                       const void* act_log, int act_bytes, uint64_t* rec_planes, uint32_t* rec_meta,
                       int32_t* err, void* stream);

/* Unpack gathered records into the reference's RolloutBuffer layout (alg/rollout_buffer.py:14-44):
 * obs f32[T][N][2][m][n] from the mover's point of view, masks u8[T][N][C], actions i64[T][N],
 * rewards f32[T][N], dones u8[T][N].  Any output may be NULL. */
int mnk_unpack_records(const uint64_t* rec_planes, const uint32_t* rec_meta, int64_t N, int T, int m, int n,
                       void* obs, int obs_dtype, uint8_t* masks, int64_t* actions, float* rewards, uint8_t* dones,
                       void* stream);

/* ---- alg/rollout_buffer.py:82-113 get_data_loader: a shuffled minibatch straight from PACKED observations.
 * planes u64[T][2][W][N] (channel 0 = the viewer's stones, as the wrapper hands them out); idx int64[B] flat
 * sample ids t*N + i (negative ids wrap, out-of-range -> err).  Writes the network inputs of the B samples:
 * obs f32[B][2][m][n] and legal mask u8[B][m*n] (free cells; fix_empty_mask as in wrapper:108-110). */
int mnk_gather_obs(const uint64_t* planes, int64_t T, int64_t N, int m, int n, const int64_t* idx, int64_t B,
                   void* obs, int obs_dtype, uint8_t* legal_mask, int fix_empty_mask, int32_t* err, void* stream);

/* ---- alg/rollout_buffer.py:60-80 compute_advantages_and_returns (GAE), one lane per env ---- */
int mnk_gae(const float* rewards, const float* values, const uint8_t* dones, const float* last_values,
            int64_t N, int T, float gamma, float gamma_lambda, float* advantages, float* returns,
            void* stream);

/* ---- the exchange step of the sharded rollout: RCCL all-gather over xGMI ------------
 * The reference has no distributed code; what ranks exchange is the content of its RolloutBuffer
 * (alg/rollout_buffer.py:14-44) in the packed forms above -- either the records themselves or the message
 * "chunk-start planes | action log | chunk-start meta" that mnk_replay_actions expands on the receiver.
 * One process per GPU.  mnk_comm_unique_id (one rank, HOST buffer of MNK_COMM_ID_BYTES) -> the id travels to
 * the other ranks by any host channel (torch.distributed store, a file, MPI) -> every rank calls mnk_comm_init
 * with its rank on its current HIP device -> mnk_allgather_records enqueues ONE all-gather of `bytes` bytes per
 * rank on `stream` (recv holds nranks * bytes; rank r's message lands at recv + r * bytes; in-place allowed
 * when send == recv + rank * bytes) -> mnk_comm_destroy.  Only enqueues: ordering against the rollout kernel
 * is by stream / events, as for every other entry point.  RCCL is resolved from the librccl.so.1 the process
 * has already loaded (PyTorch-ROCm's), not linked.  Errors: MNK_ECOMM + mnk_comm_last_error(). */
int mnk_comm_unique_id(void* id_out_host);
int mnk_comm_init(void** comm_out, const void* id_host, int nranks, int rank);
int mnk_comm_destroy(void* comm);
int mnk_allgather_records(void* comm, const void* send, void* recv, int64_t bytes, void* stream);
/* The same exchange as one send and one receive per peer (ncclSend / ncclRecv in one group, peers in rotated order):
 * on the fully connected xGMI mesh every rank's message then travels once over each of its own links, where a ring
 * all-gather forwards it hop by hop.  Same arguments and result layout; send and recv must not overlap. */
int mnk_allgather_records_direct(void* comm, const void* send, void* recv, int64_t bytes, void* stream);
const char* mnk_comm_last_error(void);
/* NCCL_VERSION_CODE of the resolved library, 0 when none could be resolved */
int mnk_comm_version(void);

/* Measurement aid (bench.py: `roofline.measured_write_ceiling_GBps`): fills rec u64[T][rows][N] with a write-only
 * kernel that has the store pattern of the rollout records and no game logic -- the write rate the device sustains
 * for the access pattern mnk_rollout_random is bound by. */
int mnk_probe_record_writes(uint64_t* rec, int64_t N, int T, int rows, void* stream);

/* Test aid: the r-th-set-bit select of the rollout kernels (bs_select_hot in csrc/mnk_device.h) on `count` strings of
 * nw = 1, 3 or 12 u32 words (words u32[count][nw], ranks i32[count], each rank < the string's popcount): the bit index
 * to bits i32[count] and the one-hot string to hot u32[count][nw]. */
int mnk_probe_select_bits(const uint32_t* words, int nw, int64_t count, const int32_t* ranks, int32_t* bits, uint32_t* hot,
                          void* stream);

/* Test aid: the byte table that ends that select in the rollout kernels which have a FAST loop (MnkSelectTable in
 * csrc/mnk_device.h), as its generator makes it, to out u8[256][8] in HOST memory: out[b][r] = position of the r-th
 * set bit of byte b, 0 where r >= popcount(b).  Needs no device. */
int mnk_probe_select_table(uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MNK_HIP_H */
