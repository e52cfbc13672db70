// mnk_rollout.hip -- the fused random-policy rollout and the replay of its action log
// (gfx950 / MI355X only).  Separate translation unit: these kernels come in many variants
// (board specialisation x record / action-log forms) and compile in parallel with the rest.
#include "mnk_host.h"
#include "mnk_rollout_lane.h"

namespace {

// the argument checks of mnk_rollout_random (and of the query of its plan, which has no pointers to check): MNK_OK with
// the geometry and the log format a launch would use (0 without a log)
int rollout_check(int64_t N, int m, int n, int k, int T, bool log, int act_bytes, uint64_t step0, MnkGeom* g, int* act) {
  const int rc = mnk_check_geom(m, n, k, g);
  if (rc != MNK_OK) return rc;
  if (N < 0 || T < 0 || T > 65535) return MNK_EINVAL;
  if (log && (act_bytes == 0 || !mnk_act_format_ok(act_bytes, g->C))) return MNK_EINVAL;
  if (log && (step0 & 3)) return MNK_EINVAL;  // log words hold plies 4q..4q+3 of the Philox step counter
  *act = log ? act_bytes : 0;
  return MNK_OK;
}

// launches what the plan says; false: the plan's run-time compiled kernel did not compile, nothing was launched
bool rollout_launch(const MnkRolloutArgs& a, const MnkRolloutPlan& p) {
  if (p.jit != MNK_PLAN_AOT) {
    // (the module functions take their parameter list from the kernel templates; decltype instantiates no kernel here)
    hipFunction_t fn = nullptr;
    if (p.form == MNK_ROLLOUT_PAIR && (fn = mnk_jit_rollout_function(a.g, MNK_JIT_ROLLOUT_PAIR, a.rec(), a.act, false)))
      mnk_rollout_launch(decltype(&k_rollout_random_pair<2, 0, 0, true, 0>)(nullptr), fn, a.grid(32), dim3(64), a);
    else if ((fn = mnk_jit_rollout_function(a.g, MNK_JIT_ROLLOUT, a.rec(), a.act, p.saddr)))
      mnk_rollout_launch(decltype(&k_rollout_random<2, 0, 0, true, 0>)(nullptr), fn, a.grid(64), dim3(64), a);
    return fn != nullptr;
  }
  if (p.form == MNK_ROLLOUT_WS2 || p.form == MNK_ROLLOUT_WS4) mnk_launch_rollout_ws(a, p.form == MNK_ROLLOUT_WS4 ? 4 : 2);
  else if (p.form == MNK_ROLLOUT_PAIRW) mnk_launch_rollout_pairw(a);
  else if (p.form == MNK_ROLLOUT_PAIR) mnk_launch_rollout_pair(a);
  else if (a.act) mnk_launch_rollout_log(a, p.saddr);
  else mnk_launch_rollout_lane(a, p.saddr);
  return true;
}

}  // namespace

// one lane per env, no log
void mnk_launch_rollout_lane(const MnkRolloutArgs& a, bool saddr) {
  mnk_rollout_board(a.g, [&](auto row) {
    using Row = decltype(row);
    const auto launch = [&](auto kernel) { mnk_rollout_launch(kernel, nullptr, a.grid(64), dim3(64), a); };
    if constexpr (Row::CN != 0)  // (the plan asks for 32-bit record offsets on the built-in boards only)
      if (saddr) return launch(k_rollout_random<Row::NW, Row::CN, Row::CK, true, 0, true>);
    if (a.rec()) launch(k_rollout_random<Row::NW, Row::CN, Row::CK, true, 0>);
    else launch(k_rollout_random<Row::NW, Row::CN, Row::CK, false, 0>);
  });
}

// ================================================================== C ABI
extern "C" {

int mnk_rollout_random(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, int T, uint64_t seed,
                       uint64_t step0, int64_t env_id0, uint64_t* rec_planes, uint32_t* rec_meta, int64_t* stats,
                       void* act_log, int act_bytes, void* stream) {
  MnkRolloutArgs a{};
  const int rc = rollout_check(N, m, n, k, T, act_log != nullptr, act_bytes, step0, &a.g, &a.act);
  if (rc != MNK_OK) return rc;
  if (!planes || !meta || (!rec_planes != !rec_meta)) return MNK_EINVAL;
  if (N == 0 || T == 0) return MNK_OK;
  a.planes = planes, a.meta = meta, a.N = N, a.T = T, a.seed = seed, a.step0 = step0, a.env_id0 = env_id0;
  a.rec_planes = rec_planes, a.rec_meta = rec_meta, a.stats = stats, a.act_log = act_log, a.stream = (hipStream_t)stream;
  const MnkConfig& cfg = mnk_config();  // environment knobs, read once (mnk_reload_config() re-reads them)
  MnkRolloutPlan plan = mnk_rollout_plan(a.g, N, T, a.rec(), a.act, cfg, false);
  if (!rollout_launch(a, plan)) {  // if the compile fails the ahead-of-time kernel still runs, where there is one
    plan = mnk_rollout_plan(a.g, N, T, a.rec(), a.act, cfg, true);
    if (plan.status != MNK_OK) {
      snprintf(g_launch_err, sizeof(g_launch_err), "rollout_random: no kernel for this board: %.200s", mnk_jit_last_error());
      return plan.status;
    }
    rollout_launch(a, plan);
  }
  static const char* const what[] = {"", "rollout_random", "rollout_random_pair", "rollout_random_pairw", "rollout_random_ws",
                                     "rollout_random_ws"};
  return mnk_launch_status(plan.jit != MNK_PLAN_AOT ? "rollout_random (run-time specialised)" : what[plan.form]);
}

int mnk_rollout_form(int64_t N, int m, int n, int k, int T, int records, int act_bytes, int jit_failed) {
  MnkGeom g;
  int act;
  const int rc = rollout_check(N, m, n, k, T, act_bytes != 0, act_bytes, 0, &g, &act);
  if (rc != MNK_OK) return rc;
  if (N == 0 || T == 0) return 0;
  const MnkRolloutPlan p = mnk_rollout_plan(g, N, T, records != 0, act, mnk_config(), jit_failed != 0);
  if (p.status != MNK_OK) return p.status;
  return p.form | (p.saddr ? MNK_ROLLOUT_SADDR : 0) | (p.jit != MNK_PLAN_AOT ? MNK_ROLLOUT_JIT : 0) |
         (p.jit == MNK_PLAN_JIT_ONLY ? MNK_ROLLOUT_JIT_ONLY : 0);
}

int mnk_action_log_words(int act_bytes, int T) {
  if (T < 0) return 0;
  const int q = (T + 3) >> 2;
  if (act_bytes == MNK_ACT_U8) return q;
  if (act_bytes == MNK_ACT_U16) return 2 * q;
  if (act_bytes == MNK_ACT_BITS7) return (7 * q + 7) >> 3;
  if (act_bytes == MNK_ACT_U8P1) return q + ((T + 31) >> 5);
  return 0;
}

int mnk_replay_actions(uint64_t* planes, uint32_t* meta, int64_t N, int m, int n, int k, int T, const void* act_log,
                       int act_bytes, uint64_t* rec_planes, uint32_t* rec_meta, int32_t* err, void* stream) {
  MnkGeom g;
  int rc = mnk_check_geom(m, n, k, &g);
  if (rc != MNK_OK) return rc;
  if (!planes || !meta || !act_log || N < 0 || T < 0 || (!rec_planes != !rec_meta)) return MNK_EINVAL;
  if (act_bytes == 0 || !mnk_act_format_ok(act_bytes, g.C)) return MNK_EINVAL;
  if (N == 0 || T == 0) return MNK_OK;
  const bool rec = rec_planes && rec_meta;
  const auto launch = [&](auto kernel, hipFunction_t fn) {
    mnk_launch(kernel, fn, dim3((unsigned)((N + 63) / 64)), dim3(64), (hipStream_t)stream, g, planes, meta, N, T, act_log,
               rec_planes, rec_meta, err);
  };
  if (g.NW > 16) {  // planes of more than 512 bits: the run-time specialised kernel is the only one (mnk_rollout_board)
    if (hipFunction_t fn = mnk_jit_rollout_function(g, MNK_JIT_REPLAY, rec, act_bytes, false)) {
      launch(decltype(&k_replay_actions<2, 0, 0, true, 1>)(nullptr), fn);
      return mnk_launch_status("replay_actions (run-time specialised)");
    }
    snprintf(g_launch_err, sizeof(g_launch_err), "replay_actions: no kernel for this board: %.200s", mnk_jit_last_error());
    return MNK_ELAUNCH;
  }
  mnk_rollout_board(g, [&](auto row) {
    using Row = decltype(row);
    mnk_rec_act(rec, act_bytes, [](bool, int act) { return act != 0 && mnk_lane_built<Row>(act); }, [&](auto r, auto act) {
      launch(k_replay_actions<Row::NW, Row::CN, Row::CK, decltype(r)::value, decltype(act)::value>, nullptr);
    });
  });
  return mnk_launch_status("replay_actions");
}

}  // extern "C"
