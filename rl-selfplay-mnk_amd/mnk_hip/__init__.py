"""ctypes binding of ``libmnk_hip.so`` (C ABI in ``include/mnk_hip.h``).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There
is no fallback: if the shared object is missing or a call fails, an exception is
raised -- the product path never computes on the CPU.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MNK_HIP_LIB: another build of the same library (A/B experiments with compile-time options); default: the in-tree build
LIB_PATH = os.environ.get("MNK_HIP_LIB") or os.path.join(_HERE, "libmnk_hip.so")
ABI_VERSION = 6

MNK_OK = 0
ERR_NONE, ERR_ACTION_RANGE, ERR_ILLEGAL_MOVE, ERR_SYMMETRY, ERR_VISITS = 0, 1, 2, 3, 4
STEP_STRICT, STEP_AUTORESET = 1, 2
LOGITS_F32, LOGITS_BF16 = 0, 1
OBS_F32, OBS_BF16, OBS_U8 = 0, 1, 2
ACT_U8, ACT_U16, ACT_BITS7, ACT_U8P1 = 1, 2, 3, 4
COMM_ID_BYTES = 128
SP_NEED_OPP, SP_WAS_RESET = 1, 2
STREAM_MOVE, STREAM_OPP, STREAM_SIDE, STREAM_SAMPLE, STREAM_PLAYOUT, STREAM_SEARCH, STREAM_SELFPLAY = 0, 1, 2, 3, 4, 5, 6
STREAM_NOISE = 7  # MNK_STREAM_NOISE: the Dirichlet noise on the PUCT player's root priors (mnk_puct_root_noise)
Z_UNKNOWN = -128  # MNK_Z_UNKNOWN: the outcome of a ring record whose game is still running
PROOF_UNKNOWN = -128  # MNK_PROOF_UNKNOWN: the `proof` of a root that mnk_puct_step_solver has not proven
PLAYOUTS_MAX = 4096  # MNK_PLAYOUTS_MAX: the largest playout count of mnk_sample_playouts
SEARCH_ITERS_MAX = 2048  # MNK_SEARCH_ITERS_MAX: the largest iteration budget of mnk_sample_search
SEARCH_PLAYOUTS_MAX = 256  # MNK_SEARCH_PLAYOUTS_MAX: the largest playout count per leaf of mnk_sample_search
PUCT_ITERS_MAX = 2048  # MNK_PUCT_ITERS_MAX: the largest iteration budget of mnk_puct_begin / mnk_puct_step
PUCT_LEAVES_MAX = 16  # MNK_PUCT_LEAVES_MAX: the most leaves per row and evaluation of the mnk_puct_*_leaves entry points
STREAM_GUMBEL = 8  # MNK_STREAM_GUMBEL: the Gumbel variables of the PUCT player's Gumbel root (mnk_puct_gumbel_root)
STREAM_BUDGET = 9  # MNK_STREAM_BUDGET: is a self-play ply searched with the full budget? (mnk_search_selfplay_advance)
PUCT_CONSIDERED_MAX = 1024  # MNK_PUCT_CONSIDERED_MAX: the most root moves mnk_puct_step_gumbel considers
PUCT_NOISE_TRIES = 16  # MNK_PUCT_NOISE_TRIES: the most Marsaglia-Tsang candidates per cell of mnk_puct_root_noise
STATS_REPLICAS, STATS_STRIDE, STATS_COUNTERS = 64, 8, 5
# run-time specialised API kernels (MNK_JIT_API_* of include/mnk_hip.h): bit numbers for jit_prepare()
(JIT_API_STEP, JIT_API_STEP_DRAW, JIT_API_STEP_SUBSET, JIT_API_OBSERVE, JIT_API_SAMPLE_LEGAL, JIT_API_UNPACK_RECORDS,
 JIT_API_GATHER_OBS, JIT_API_SP_PRE, JIT_API_SP_POST, JIT_API_SP_STEP, JIT_API_SP_DRAW) = range(11)
JIT_API_SP_TACTICAL, JIT_API_SP_TACTICAL_DRAW, JIT_API_SAMPLE_TACTICAL = 19, 20, 23  # (TACTICAL_DRAW + logits form)
JIT_API_COUNT = 24
REC_ACTION_MASK, REC_REWARD_SHIFT, REC_DONE_BIT, REC_SIDE_BIT = 0xFFFF, 16, 24, 25
# what rollout_form() returns: one of the kernel forms (MNK_ROLLOUT_* of include/mnk_hip.h), ORed with the flags
ROLLOUT_LANE, ROLLOUT_PAIR, ROLLOUT_PAIRW, ROLLOUT_WS2, ROLLOUT_WS4 = 1, 2, 3, 4, 5
ROLLOUT_SADDR, ROLLOUT_JIT, ROLLOUT_JIT_ONLY = 0x10, 0x20, 0x40

_vp, _i, _i64, _u64, _u32, _f = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32,
                                 ctypes.c_float)

# name -> argtypes; restype is int unless noted.  Kept in step with include/mnk_hip.h
# (tests/test_abi.py parses the header and compares).
SIGNATURES = {
    "mnk_abi_version": [],
    "mnk_reload_config": [],
    "mnk_state_words": [_i, _i],
    "mnk_record_words": [_i, _i],
    "mnk_geometry_supported": [_i, _i, _i],
    "mnk_last_launch_error": [],
    "mnk_reset_all": [_vp, _vp, _i64, _i, _vp],
    "mnk_reset_idx": [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp],
    "mnk_reset_mask": [_vp, _vp, _i64, _i, _vp, _vp],
    "mnk_step": [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _u32, _vp],
    "mnk_step_random": [_vp, _vp, _i64, _i, _i, _i, _u64, _u64, _vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _i, _u32, _vp],
    "mnk_observe": [_vp, _vp, _i64, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp],
    "mnk_pack_boards": [_vp, _vp, _i64, _i, _i, _vp],
    "mnk_unpack_boards": [_vp, _vp, _i64, _i, _i, _vp],
    "mnk_sample_legal": [_vp, _i64, _i, _i, _u64, _u64, _vp, _i64, _i, _vp, _vp],
    "mnk_sample_logits": [_vp, _i, _vp, _i64, _i, _u64, _vp, _u64, _vp, _i64, _i, _vp, _vp, _vp],
    "mnk_selfplay_pre": [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _i64, _vp, _vp, _vp, _vp,
                         _i, _vp, _vp, _u32, _vp],
    "mnk_selfplay_post": [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                          _vp, _u32, _vp],
    "mnk_selfplay_step_random": [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _i64, _vp, _vp,
                                 _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
    # the sampler block of the *_logits forms: logits, dtype, mask, seed, seed_dev, step, step_dev, env_id0, deterministic,
    # actions (out), logp (out)
    "mnk_selfplay_pre_logits": [_vp, _vp, _i64, _i, _i, _i] + [_vp, _i, _vp, _u64, _vp, _u64, _vp, _i64, _i, _vp, _vp] +
                               [_vp, _vp, _vp, _u64, _u64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _u32, _vp],
    "mnk_selfplay_post_logits": [_vp, _vp, _i64, _i, _i, _i] + [_vp, _i, _vp, _u64, _vp, _u64, _vp, _i64, _i, _vp, _vp] +
                                [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
    "mnk_selfplay_step_random_logits": [_vp, _vp, _i64, _i, _i, _i] + [_vp, _i, _vp, _u64, _vp, _u64, _vp, _i64, _i, _vp, _vp] +
                                       [_vp, _vp, _vp, _u64, _u64, _vp, _i64, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _u32, _vp],
    "mnk_selfplay_step_tactical": [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _i64, _vp, _vp,
                                   _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
    "mnk_selfplay_step_tactical_logits": [_vp, _vp, _i64, _i, _i, _i] + [_vp, _i, _vp, _u64, _vp, _u64, _vp, _i64, _i, _vp,
                                                                         _vp] +
                                         [_vp, _vp, _vp, _u64, _u64, _vp, _i64, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _u32, _vp],
    # obs, obs dtype, N, m, n, k, then the sampler block (seed, seed_dev, step, step_dev, env_id0, deterministic), actions,
    # candidates, stream
    "mnk_sample_tactical": [_vp, _i, _i64, _i, _i, _i, _u64, _vp, _u64, _vp, _i64, _i, _vp, _vp, _vp],
    # obs, obs dtype, N, m, n, k, playouts, then the sampler block, actions, counts (int32 [N][2][C]), stream
    "mnk_sample_playouts": [_vp, _i, _i64, _i, _i, _i, _i, _u64, _vp, _u64, _vp, _i64, _i, _vp, _vp, _vp],
    # obs, obs dtype, N, m, n, k, iterations, playouts, c, then the sampler block, actions, stats (int32 [N][3][C]), stream
    "mnk_sample_search": [_vp, _i, _i64, _i, _i, _i, _i, _i, _f, _u64, _vp, _u64, _vp, _i64, _i, _vp, _vp, _vp],
    # N, m, n, iterations -> bytes of the PUCT tree workspace (int64; < 0: an error code)
    "mnk_puct_workspace_bytes": [_i64, _i, _i, _i],
    # obs, obs dtype, N, m, n, k, iterations, workspace, leaf obs, leaf dtype, leaf mask, stream
    "mnk_puct_begin": [_vp, _i, _i64, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp],
    # obs, obs dtype, N, m, n, k, tree iterations, keep nodes, workspace, leaf obs, leaf dtype, leaf mask, carried (int32
    # [N][2]), stream
    "mnk_puct_rebase": [_vp, _i, _i64, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp],
    # workspace, N, m, n, k, iterations, priors, priors dtype, values, values dtype, c, last, temperature, then the
    # sampler block, leaf obs, leaf dtype, leaf mask, actions, visits (int32 [N][C]), root value (f32 [N]), stream
    "mnk_puct_step": [_vp, _i64, _i, _i, _i, _i, _vp, _i, _vp, _i, _f, _i, _i, _u64, _vp, _u64, _vp, _i64, _i, _vp, _i,
                      _vp, _vp, _vp, _vp, _vp],
    # the four above with `leaves` (after iterations; after keep nodes for the rebase): L leaves per row and evaluation
    "mnk_puct_workspace_bytes_leaves": [_i64, _i, _i, _i, _i],
    "mnk_puct_begin_leaves": [_vp, _i, _i64, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp],
    "mnk_puct_rebase_leaves": [_vp, _i, _i64, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp],
    "mnk_puct_step_leaves": [_vp, _i64, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _f, _i, _i, _u64, _vp, _u64, _vp, _i64, _i,
                             _vp, _i, _vp, _vp, _vp, _vp, _vp],
    # mnk_puct_step_leaves with proofs of wins, draws and losses: its arguments, then proof (int8 [N]) before the stream
    "mnk_puct_step_solver": [_vp, _i64, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _f, _i, _i, _u64, _vp, _u64, _vp, _i64, _i,
                             _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    # mnk_puct_step_solver's arguments, then solver, fpu, fpu root before the stream: first-play urgency
    "mnk_puct_step_fpu": [_vp, _i64, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _f, _i, _i, _u64, _vp, _u64, _vp, _i64, _i,
                          _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _vp],
    # mnk_puct_step_fpu's arguments, then fpu on, forced k, raw visits (int32 [N][C]) before the stream: forced playouts
    # and policy target pruning
    "mnk_puct_step_forced": [_vp, _i64, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _f, _i, _i, _u64, _vp, _u64, _vp, _i64, _i,
                             _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _i, _f, _vp, _vp],
    # priors, priors dtype, mask, N, C, leaves, alpha, eps, then seed, seed_dev, step, step_dev, env_id0, out (f32
    # [N * leaves][C]), stream
    "mnk_puct_root_noise": [_vp, _i, _vp, _i64, _i, _i, _f, _f, _u64, _vp, _u64, _vp, _i64, _vp, _vp],
    # considered, iterations, out (HOST u16 [considered + 1][iterations]): the Gumbel root's table of considered visits
    "mnk_puct_gumbel_schedule": [_i, _i, _vp],
    # priors, priors dtype, mask, values, values dtype, N, C, gumbel scale, then seed, seed_dev, step, step_dev, env_id0,
    # gscore (f32 [N][C]), vroot (f32 [N]), stream
    "mnk_puct_gumbel_root": [_vp, _i, _vp, _vp, _i, _i64, _i, _f, _u64, _vp, _u64, _vp, _i64, _vp, _vp, _vp],
    # mnk_puct_step_leaves with considered, c_visit, c_scale, table, gscore, vroot in the place of the temperature, and
    # policy (f32 [N][C]) before the stream
    "mnk_puct_step_gumbel": [_vp, _i64, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _f, _i, _i, _f, _f, _vp, _vp, _vp, _u64, _vp,
                             _u64, _vp, _i64, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    # planes, meta, N, m, n, k, policy (f32 [N][C]), actions (int64 [N]), step, step_dev, T, ring planes, ring visits, ring
    # z, obs, obs dtype, legal mask, stats, err, stream
    "mnk_search_selfplay_step_moves": [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _u64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp,
                                       _vp, _vp, _vp],
    # planes, meta, N, m, n, k, visits (int32 [N][C]), temp_plies, then seed, seed_dev, step, step_dev, env_id0, T, ring
    # planes, ring visits, ring z, obs, obs dtype, legal mask, stats, err, stream
    "mnk_search_selfplay_step": [_vp, _vp, _i64, _i, _i, _i, _vp, _i, _u64, _vp, _u64, _vp, _i64, _i64, _vp, _vp, _vp, _vp,
                                 _i, _vp, _vp, _vp, _vp],
    # workspace, planes, meta, N, m, n, k, iterations, fast iterations, full threshold, priors, priors dtype, values, values
    # dtype, c, temp_plies, seed, seed_dev, env_id0, row plies (u64 [N]), T, ring planes, ring visits, ring z, leaf obs, leaf
    # dtype, leaf mask, fresh (u8 [N]), plies max (u64 [1]), stats, err, stream
    "mnk_search_selfplay_advance": [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _u64, _vp, _i, _vp, _i, _f, _i, _u64, _vp, _i64,
                                    _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    # mnk_search_selfplay_advance's arguments up to err, then solver, noise alpha, noise eps, noise on fast plies, root
    # priors (f32 [N][C], optional), stream
    "mnk_search_selfplay_advance_opts": [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _u64, _vp, _i, _vp, _i, _f, _i, _u64, _vp,
                                         _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _i,
                                         _vp, _vp],
    # mnk_search_selfplay_advance_opts's arguments up to root priors, then tree iterations, keep nodes, carried (int32
    # [N][2]), stream
    "mnk_search_selfplay_advance_keep": [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _u64, _vp, _i, _vp, _i, _f, _i, _u64, _vp,
                                         _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _i,
                                         _vp, _i, _i, _vp, _vp],
    # the two above with fpu, fpu root before the stream: first-play urgency in the selection
    "mnk_search_selfplay_advance_opts_fpu": [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _u64, _vp, _i, _vp, _i, _f, _i, _u64,
                                             _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f,
                                             _f, _i, _vp, _f, _f, _vp],
    "mnk_search_selfplay_advance_keep_fpu": [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _u64, _vp, _i, _vp, _i, _f, _i, _u64,
                                             _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f,
                                             _f, _i, _vp, _i, _i, _vp, _f, _f, _vp],
    # mnk_search_selfplay_advance_opts_fpu's arguments, then fpu on, forced k before the stream
    "mnk_search_selfplay_advance_opts_forced": [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _u64, _vp, _i, _vp, _i, _f, _i,
                                                _u64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                                _i, _f, _f, _i, _vp, _f, _f, _i, _f, _vp],
    # mnk_search_selfplay_advance_opts's arguments with leaves behind the fast iterations and row sims (u32 [N]) before the
    # stream
    "mnk_search_selfplay_advance_leaves": [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _u64, _vp, _i, _vp, _i, _f, _i, _u64,
                                           _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f,
                                           _i, _vp, _vp, _vp],
    # mnk_search_selfplay_advance's arguments up to err without temp_plies, then considered, c_visit, c_scale, gumbel scale,
    # table for the full budget (u16 [considered + 1][iterations]), table for the fast one, gscore (f32 [N][C]), vroot (f32
    # [N]), stream
    "mnk_search_selfplay_advance_gumbel": [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _u64, _vp, _i, _vp, _i, _f, _u64, _vp,
                                           _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f,
                                           _vp, _vp, _vp, _vp, _vp],
    # ring planes, ring visits, ring z, T, N, m, n, idx, sym, B, obs, obs dtype, legal mask, policy, value, weight, err, stream
    "mnk_search_gather": [_vp, _vp, _vp, _i64, _i64, _i, _i, _vp, _vp, _i64, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "mnk_rollout_random": [_vp, _vp, _i64, _i, _i, _i, _i, _u64, _u64, _i64, _vp, _vp, _vp, _vp, _i, _vp],
    "mnk_rollout_form": [_i64, _i, _i, _i, _i, _i, _i, _i],
    "mnk_action_log_words": [_i, _i],
    "mnk_replay_actions": [_vp, _vp, _i64, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp],
    "mnk_unpack_records": [_vp, _vp, _i64, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp],
    "mnk_gather_obs": [_vp, _i64, _i64, _i, _i, _vp, _i64, _vp, _i, _vp, _i, _vp, _vp],
    "mnk_gae": [_vp, _vp, _vp, _vp, _i64, _i, _f, _f, _vp, _vp, _vp],
    "mnk_jit_compile_rollout": [_i, _i, _i, _i, _i],
    "mnk_jit_compile_kernel": [_i, _i, _i, _i, _i, _i],
    "mnk_jit_last_error": [],
    "mnk_jit_compile_api": [_i, _i, _i, _i],
    "mnk_jit_prepare": [_i, _i, _i, _i64],
    "mnk_jit_api_ready": [_i, _i, _i, _i],
    "mnk_jit_stats": [_vp],
    "mnk_comm_unique_id": [_vp],
    "mnk_comm_init": [_vp, _vp, _i, _i],
    "mnk_comm_destroy": [_vp],
    "mnk_allgather_records": [_vp, _vp, _vp, _i64, _vp],
    "mnk_allgather_records_direct": [_vp, _vp, _vp, _i64, _vp],
    "mnk_comm_last_error": [],
    "mnk_comm_version": [],
    "mnk_probe_record_writes": [_vp, _i64, _i, _i, _vp],
    "mnk_probe_select_bits": [_vp, _i, _i64, _vp, _vp, _vp, _vp],
    "mnk_probe_select_table": [_vp],
}

_STATUS = {-1: "invalid argument (null pointer / negative size)", -2: "unsupported board geometry",
           -3: "kernel launch failed", -4: "RCCL call failed"}


class MnkHipError(RuntimeError):
    pass


_lib = None


def load():
    """Returns the loaded library; raises MnkHipError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MnkHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for this path."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)  # AttributeError here = header / library mismatch
        except AttributeError:
            if os.environ.get("MNK_HIP_LIB"):  # an older build loaded for an A/B run: entry points added since are absent
                continue
            raise
        fn.argtypes = argtypes
        if name in ("mnk_last_launch_error", "mnk_comm_last_error", "mnk_jit_last_error"):
            fn.restype = ctypes.c_char_p
        elif name in ("mnk_jit_compile_rollout", "mnk_jit_compile_kernel", "mnk_jit_compile_api",
                      "mnk_puct_workspace_bytes", "mnk_puct_workspace_bytes_leaves"):
            fn.restype = ctypes.c_int64
        else:
            fn.restype = ctypes.c_int
    if lib.mnk_abi_version() != ABI_VERSION:
        raise MnkHipError(f"libmnk_hip.so ABI {lib.mnk_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def ptr(t):
    """Device pointer of a contiguous tensor (or NULL for None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "mnk_hip: tensors handed to the C ABI must be contiguous"
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device):
    """hipStream_t of torch's current stream on ``device`` -- through the raw accessor where this torch has it (one C
    call, ~0.3 us) instead of building a ``torch.cuda.Stream`` object per launch (~4 us of the ~18 us a step costs on
    the host)"""
    if _raw_stream is not None:
        idx = device.index if isinstance(device, torch.device) else torch.device(device).index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(device).cuda_stream


_bound = {}


def call(name, *args):
    fn = _bound.get(name)
    if fn is None:
        fn = _bound[name] = getattr(load(), name)
    lib = _lib
    rc = fn(*args)
    if rc != MNK_OK:
        detail = _STATUS.get(rc, f"status {rc}")
        if rc == -3:
            detail += ": " + (lib.mnk_last_launch_error() or b"").decode()
        if rc == -4:
            detail += ": " + (lib.mnk_comm_last_error() or b"").decode()
        raise MnkHipError(f"{name}: {detail}")
    return rc


_OBS_DTYPES = {torch.float32: OBS_F32, torch.bfloat16: OBS_BF16, torch.uint8: OBS_U8}


def obs_dtype_code(dtype) -> int:
    """MNK_OBS_* code of a torch dtype an observation may be written in (float32 = the reference's; bfloat16 and
    uint8 are the opt-in narrow forms: cells are exactly 0 / 1, so ``obs.float()`` is the same tensor)."""
    try:
        return _OBS_DTYPES[dtype]
    except KeyError:
        raise TypeError(f"observations can be written as float32, bfloat16 or uint8, not {dtype}") from None


def obs_code(t) -> int:
    """MNK_OBS_* code of an observation tensor (None -> F32: the pointer is NULL and the code is not looked at)"""
    return OBS_F32 if t is None else obs_dtype_code(t.dtype)


def reload_config() -> None:
    """The library reads its developer knobs (MNK_ROLLOUT_PAIR / _FORM / _SADDR, MNK_JIT, MNK_EMIT_ENVS / _THREADS) from
    the environment once; call this after changing ``os.environ`` to make it read them again."""
    call("mnk_reload_config")


def rollout_form(N: int, m: int, n: int, k: int, T: int, records: bool = True, act_bytes: int = 0,
                 jit_failed: bool = False) -> int:
    """Which kernel ``mnk_rollout_random`` runs for such a launch under the current knobs: ROLLOUT_LANE / _PAIR / _PAIRW /
    _WS2 / _WS4, ORed with ROLLOUT_SADDR / _JIT / _JIT_ONLY; 0 when nothing would be launched, a negative status for
    arguments the launch rejects.  Needs no GPU (the rules: include/mnk_hip.h, mnk_rollout_form)."""
    return load().mnk_rollout_form(N, m, n, k, T, int(bool(records)), act_bytes, int(bool(jit_failed)))


def jit_api_draw_kind(which: int, logits_dtype=None) -> int:
    """MNK_JIT_API_* number of a self-play step kernel with the draw folded in: ``which`` 0 pre / 1 post / 2
    step_random; ``logits_dtype`` torch.float32, torch.bfloat16 or None (no logits: uniform over the mask)"""
    lt = 2 if logits_dtype is None else (1 if logits_dtype == torch.bfloat16 else 0)
    return JIT_API_SP_DRAW + 3 * lt + which


def jit_api_tactical_draw_kind(logits_dtype=None) -> int:
    """MNK_JIT_API_* number of the tactical step kernel with the agent's draw folded in (``logits_dtype`` as in
    ``jit_api_draw_kind``)"""
    return JIT_API_SP_TACTICAL_DRAW + (2 if logits_dtype is None else (1 if logits_dtype == torch.bfloat16 else 0))


def jit_prepare(m: int, n: int, k: int, kinds=None) -> int:
    """Compile and load NOW the board's own variants of the API kernels in ``kinds`` (iterable of JIT_API_* numbers;
    None: of every kernel launched on this board so far) instead of when they get hot -- before a hipGraph capture,
    where nothing can be compiled: warm up, ``jit_prepare(m, n, k)``, capture.  Returns how many are ready; 0 for
    boards with a built-in variant (3x3x3, 9x9x5, 13x13x5, 15x15x5, 19x19x5) or with MNK_JIT_API / MNK_JIT = 0."""
    mask = 0
    for kind in (kinds if kinds is not None else ()):
        mask |= 1 << int(kind)
    if kinds is not None and mask == 0:
        return 0
    lib = load()
    rc = lib.mnk_jit_prepare(m, n, k, mask)
    if rc < 0:
        raise MnkHipError(f"mnk_jit_prepare({m}, {n}, {k}): {_STATUS.get(rc, rc)}: " + (lib.mnk_jit_last_error() or b"").decode())
    return rc


def jit_stats() -> dict:
    """what the run-time compiler did in this process: programs compiled by hiprtc, code objects read from the cache on
    disk instead (``$MNK_JIT_CACHE``, default ``~/.cache/mnk_hip``; "0": off), written to it, failed compilations"""
    out = (ctypes.c_int64 * 4)()
    load().mnk_jit_stats(out)
    return dict(zip(("compiled", "cache_hits", "cache_stores", "failed"), (int(v) for v in out)))


def jit_api_ready(m: int, n: int, k: int, kind: int) -> bool:
    """is the board's own variant of API kernel ``kind`` (JIT_API_*) loaded on the current device?"""
    return bool(load().mnk_jit_api_ready(m, n, k, int(kind)))


def state_words(m, n):
    return load().mnk_state_words(m, n)


def puct_workspace_bytes(N: int, m: int, n: int, iterations: int, leaves: int = None) -> int:
    """bytes of the PUCT tree workspace of N rows (mnk_puct_workspace_bytes; with ``leaves``,
    mnk_puct_workspace_bytes_leaves); MnkHipError on a bad board, budget or number of leaves"""
    if leaves is None:
        name, size = "mnk_puct_workspace_bytes", load().mnk_puct_workspace_bytes(N, m, n, iterations)
    else:
        name, size = "mnk_puct_workspace_bytes_leaves", load().mnk_puct_workspace_bytes_leaves(N, m, n, iterations, leaves)
    if size < 0:
        raise MnkHipError(f"{name}: {_STATUS.get(size, f'status {size}')}")
    return size


def puct_gumbel_schedule(considered: int, iterations: int):
    """the Gumbel root's table of considered visits (mnk_puct_gumbel_schedule; needs no GPU): a numpy uint16 array
    ``[considered + 1, iterations]`` whose row m' is the sequence a root with m' moves to consider follows"""
    import numpy as np

    out = np.zeros((max(int(considered), 0) + 1, max(int(iterations), 0)), np.uint16)
    call("mnk_puct_gumbel_schedule", considered, iterations, out.ctypes.data)
    return out


def record_words(m: int, n: int) -> int:
    return load().mnk_record_words(m, n)


def geometry_supported(m, n, k):
    return bool(load().mnk_geometry_supported(m, n, k))
