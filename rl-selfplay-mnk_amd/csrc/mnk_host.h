// mnk_host.h -- host-side helpers shared by the translation units of libmnk_hip.so:
// geometry construction, kernel-variant dispatch, launch-status bookkeeping.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <tuple>
#include <utility>

#include "mnk_device.h"
#include "mnk_emit.h"

// ------------------------------------------------------------------ host helpers
inline thread_local char g_launch_err[256] = "";

inline int mnk_make_geom(int m, int n, int k, MnkGeom* g) {
  if (m < 1 || n < 1 || k < 1 || k > m || k > n || n > 61) return MNK_EGEOM;
  const int bits = m * (n + 1);
  const int W = (bits + 63) / 64;
  if (W > MNK_MAX_W) return MNK_EGEOM;
  memset(g, 0, sizeof(*g));
  g->m = m; g->n = n; g->k = k;
  g->C = m * n; g->W = W; g->NW = (bits + 31) / 32; g->stride = n + 1;
  auto magic = [](uint32_t d) { return (uint32_t)((1ull << 32) / d + 1ull); };
  g->magic_n = n == 1 ? 0u : magic((uint32_t)n);  // n == 1: x / 1 handled below
  g->magic_stride = magic((uint32_t)(n + 1));
  g->magic_C = g->C == 1 ? 0u : magic((uint32_t)g->C);
  g->magic_2C = magic((uint32_t)(2 * g->C));
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < n; ++c) {
      const int b = r * (n + 1) + c;
      g->valid[b >> 5] |= 1u << (b & 31);
    }
  return MNK_OK;
}

// division by 1 cannot use the 32-bit magic (2^32 + 1 overflows); boards with n == 1 or a
// single cell are degenerate and rejected instead of carrying a special case in every kernel
inline int mnk_check_geom(int m, int n, int k, MnkGeom* g) {
  int rc = mnk_make_geom(m, n, k, g);
  if (rc != MNK_OK) return rc;
  if (n < 2) return MNK_EGEOM;
  return MNK_OK;
}

// kernels that never look at k (observe, samplers, unpack): hand the dispatcher the k of the
// specialised variant of that board width so they take the compile-time-geometry path too
inline int mnk_geom_any_k(int m, int n, MnkGeom* g) {
  int rc = mnk_check_geom(m, n, 1, g);
  if (rc != MNK_OK) return rc;
#define MNK_ANY_K_ROW(NWv, CNv, CKv, Cv) if (n == CNv) g->k = CKv;
  MNK_BUILTIN_BOARDS(MNK_ANY_K_ROW)
#undef MNK_ANY_K_ROW
  return MNK_OK;
}

// the opening checks of the mnk_sample_* players on a canonical observation: the board, then obs / actions / N / dtype
inline int mnk_sample_check(const void* obs, int obs_dtype, int64_t N, int m, int n, int k, const int64_t* actions,
                            MnkGeom* g) {
  const int rc = mnk_check_geom(m, n, k, g);
  if (rc != MNK_OK) return rc;
  return !obs || !actions || N < 0 || !mnk_obs_dtype_ok(obs_dtype) ? MNK_EINVAL : MNK_OK;
}

// the players that run a workgroup per row and play `games` random games per call and row on C cells, C4 = C rounded
// up to a multiple of 4 Philox counters each: the position q = u >> 2 of the call's last ply must fit in 56 bits,
// (step + 1) * games * C4 <= 2^58, and N in the grid's x dimension
inline int mnk_rows_games_check(uint64_t step, uint64_t games, int C, int64_t N) {
  if (step >= (1ull << 58) / (games * (uint64_t)((C + 3) & ~3))) return MNK_EINVAL;
  return N > 0x7fffffff ? MNK_EINVAL : MNK_OK;
}

inline int mnk_launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MNK_OK;
  snprintf(g_launch_err, sizeof(g_launch_err), "%s: %s", what, hipGetErrorString(e));
  return MNK_ELAUNCH;
}

// Developer knobs from the environment (A/B timing, parity tests of every kernel form), read ONCE -- a launch used to
// cost four or five getenv() calls, which is nothing beside a 90 us rollout launch but not beside a 5 us step.
// mnk_reload_config() (C ABI; mnk_hip.reload_config() in Python) reads them again after the environment has changed.
struct MnkConfig {
  int pair_override = -1;  // MNK_ROLLOUT_PAIR=0/1: never / always two lanes per env (unset: by batch size)
  int form = 0;            // MNK_ROLLOUT_FORM=lane|pair|pairw|ws2|ws4 -> MNK_ROLLOUT_LANE .. _WS4 (unset / unknown: 0)
  int jit = -1;            // MNK_JIT=0/1 (unset: run-time specialisation from 2^20 env-steps per launch)
  int jit_api = -1;        // MNK_JIT_API=0/1: the same for the API-level kernels alone (unset: what MNK_JIT says; both unset:
                           // a board's own variant is compiled once the kernel is hot, mnk_jit_api_function)
  bool saddr_off = false;  // MNK_ROLLOUT_SADDR=0: no 32-bit-offset record stores
  int emit_envs = 0;       // MNK_EMIT_ENVS=16|32|64|128: envs per workgroup of the write-out kernels (0: by batch size)
  int emit_threads = 0;    // MNK_EMIT_THREADS=64|128|256 (the kernels are __launch_bounds__(256); 0: by output set)
  int gae_depth = 0;       // MNK_GAE_DEPTH=8|16|32: steps of loads mnk_gae keeps in flight per batch (0: the default)
};

inline MnkConfig mnk_read_config() {
  MnkConfig c;
  if (const char* v = getenv("MNK_ROLLOUT_PAIR")) c.pair_override = atoi(v) != 0 ? 1 : 0;
  if (const char* v = getenv("MNK_ROLLOUT_FORM")) {
    static const char* names[] = {"", "lane", "pair", "pairw", "ws2", "ws4"};
    for (int f = MNK_ROLLOUT_LANE; f <= MNK_ROLLOUT_WS4; ++f)
      if (!strcmp(v, names[f])) c.form = f;
  }
  if (const char* v = getenv("MNK_JIT")) c.jit = atoi(v) != 0 ? 1 : 0;
  c.jit_api = c.jit;
  if (const char* v = getenv("MNK_JIT_API")) c.jit_api = atoi(v) != 0 ? 1 : 0;
  if (const char* v = getenv("MNK_ROLLOUT_SADDR")) c.saddr_off = atoi(v) == 0;
  if (const char* v = getenv("MNK_EMIT_ENVS")) {
    const int t = atoi(v);
    c.emit_envs = (t == 16 || t == 32 || t == 64 || t == 128) ? t : 0;
  }
  if (const char* v = getenv("MNK_GAE_DEPTH")) {
    const int t = atoi(v);
    c.gae_depth = (t == 8 || t == 16 || t == 32) ? t : 0;
  }
  if (const char* v = getenv("MNK_EMIT_THREADS")) {
    const int t = atoi(v);
    c.emit_threads = (t == 64 || t == 128 || t == 256) ? t : 0;  // anything else would break the launch bounds
  }
  return c;
}

// (the first call initialises the function-local static: thread-safe; a reload is the caller's to serialise)
inline const MnkConfig& mnk_config(bool reload = false) {
  static MnkConfig cfg = mnk_read_config();
  if (reload) cfg = mnk_read_config();
  return cfg;
}

// envs per workgroup of the kernels with a write-out stage; `items` = envs (x plies for mnk_unpack_records) of the launch.
// 64 by default; 32 while that still leaves fewer than 1 024 workgroups (19x19x5 x 32 768 envs: 25.5 vs 26.9 us for
// the fused self-play step, tools/exp_kernels.py).  MNK_EMIT_ENVS=16|32|64 forces one (read once per process).
inline int mnk_block_envs(int64_t items) {
  if (const int forced = mnk_config().emit_envs) return forced;
  return items <= 32768 ? 32 : 64;
}

// threads per workgroup of those kernels: the first 64 lanes play their envs, then all waves of
// the workgroup sweep its output slab (more waves per SIMD to hide the LDS / store latency)
// 256 when an observation is written (1.3-1.7x faster than 64, tools/exp_emit.py); 128 when only the legal mask leaves
// (an eighth of the bytes: two waves sweep it as fast as four and start sooner -- mnk_step_random at 65 536 envs 4.77 ->
// 4.68 us per ply, at 262 144 envs 11.0 -> 9.5, tools/exp_one_launch.py)
// Never fewer threads than envs per workgroup: lane tid plays env env0 + tid, so with MNK_EMIT_ENVS=128 a 64-thread
// workgroup would leave envs 64..127 of every workgroup unplayed and emit them from an unfilled stage.
inline int mnk_block_threads(bool writes_obs = true) {
  const int envs = mnk_config().emit_envs;  // 0 unless forced; the default 32 / 64 never exceeds the defaults below
  int threads = writes_obs ? 256 : 128;
  if (const int forced = mnk_config().emit_threads) threads = forced;
  return threads < envs ? envs : threads;
}

// Kernel variants: NW = u32 register words per plane; CN / CK = compile-time board width and
// run length (0 = run time).  The boards people actually train on (MNK_BUILTIN_BOARDS, mnk_emit.h) get fully specialised
// code (immediate shift amounts, unrolled run doubling); everything else takes the generic form.
template <int NWv, int CNv, int CKv, int Cv>
struct MnkBoard {  // one row of MNK_BUILTIN_BOARDS as a type
  static constexpr int NW = NWv, CN = CNv, CK = CKv, C = Cv;
};

// f(MnkBoard<row>{}) for the row of MNK_BUILTIN_BOARDS that is g's board; f returns whether it launched (false: the row is
// outside the subset f has variants for).  false when no row is g's board.
template <typename F>
inline bool mnk_builtin_board(const MnkGeom& g, F&& f) {
#define MNK_BOARD_ROW(NWv, CNv, CKv, Cv) \
  if (g.n == CNv && g.k == CKv && g.NW == NWv) return f(MnkBoard<NWv, CNv, CKv, Cv>{});
  MNK_BUILTIN_BOARDS(MNK_BOARD_ROW)
#undef MNK_BOARD_ROW
  return false;
}

// __VA_ARGS__ with constexpr NW / CN / CK of g's row of MNK_BUILTIN_BOARDS, if there is one and it satisfies KEEP (a
// constant expression in the row's type MnkRow_, e.g. MnkRow_::C <= 128); false = nothing launched.  (`if constexpr` in
// the generic lambda: a row outside KEEP instantiates no kernel.)
#define MNK_BUILTIN(g, KEEP, ...)                                           \
  mnk_builtin_board(g, [&](auto row_) {                                     \
    using MnkRow_ = decltype(row_);                                         \
    if constexpr (KEEP) {                                                   \
      constexpr int NW = MnkRow_::NW, CN = MnkRow_::CN, CK = MnkRow_::CK;   \
      __VA_ARGS__;                                                          \
    }                                                                       \
    return bool(KEEP);                                                      \
  })
#define MNK_CASE(NWv, CNv, CKv, ...)                              \
  {                                                               \
    constexpr int NW = NWv, CN = CNv, CK = CKv;                   \
    __VA_ARGS__;                                                  \
  }
#define MNK_DISPATCH(g, ...)                                      \
  do {                                                            \
    if (MNK_BUILTIN(g, true, __VA_ARGS__)) break;                 \
    if ((g).NW <= 2) MNK_CASE(2, 0, 0, __VA_ARGS__)               \
    else if ((g).NW <= 4) MNK_CASE(4, 0, 0, __VA_ARGS__)          \
    else if ((g).NW <= 8) MNK_CASE(8, 0, 0, __VA_ARGS__)          \
    else if ((g).NW <= 16) MNK_CASE(16, 0, 0, __VA_ARGS__)        \
    else MNK_CASE(32, 0, 0, __VA_ARGS__)                          \
  } while (0)
#define MNK_K(name) HIP_KERNEL_NAME(name<NW, CN, CK>)
// is `act` a log format this board can use?  (0 = no log)
constexpr bool mnk_act_format_ok(int act, int C) {
  return act == 0 || act == MNK_ACT_U16 || (act == MNK_ACT_U8 && C <= 256) || (act == MNK_ACT_BITS7 && C <= 128) ||
         (act == MNK_ACT_U8P1 && C > 256 && C <= 512);  // (9 bits per action; only the boards that need it have kernel variants)
}

// the draw as a launch of its own (mnk_sample.hip)
int mnk_launch_sample(const MnkSample& sa, int64_t N, int C, hipStream_t s);

// dynamic LDS a launch may ask for without raising the function's limit (the packed write-out stage of a run-time
// specialised kernel is larger than the table form's: launches that would not fit stay on the ahead-of-time kernels)
#define MNK_MAX_DYNAMIC_LDS ((size_t)64 * 1024 - 256)  /* (the kernels also hold a few static words) */

// ------------------------------------------------------------------ run-time specialised API-level kernels (mnk_jit.hip)
// The kernels of mnk_api_kernels.h / mnk_selfplay_kernels.h, compiled by hiprtc with the board's NW / n / k (and, for the
// forms with a folded-in draw, its cell count) as template arguments.  Boards with a built-in variant never get here.
enum MnkJitApiKind {  // (the public names: MNK_JIT_API_* of include/mnk_hip.h)
  MNK_JK_STEP = MNK_JIT_API_STEP,                      // k_step_full<NW, CN, CK, false>
  MNK_JK_STEP_DRAW = MNK_JIT_API_STEP_DRAW,            // k_step_full<NW, CN, CK, true>
  MNK_JK_STEP_SUBSET = MNK_JIT_API_STEP_SUBSET,        // k_step_subset
  MNK_JK_OBSERVE = MNK_JIT_API_OBSERVE,                // k_observe          (never looks at k: compiled with CK = 0)
  MNK_JK_SAMPLE_LEGAL = MNK_JIT_API_SAMPLE_LEGAL,      // k_sample_legal     (CK = 0)
  MNK_JK_UNPACK_RECORDS = MNK_JIT_API_UNPACK_RECORDS,  // k_unpack_records   (CK = 0)
  MNK_JK_GATHER_OBS = MNK_JIT_API_GATHER_OBS,          // k_gather_obs       (CK = 0)
  MNK_JK_SP_PRE = MNK_JIT_API_SP_PRE,                  // k_selfplay_pre / _post / _step_random <NW, CN, CK, NoDraw>
  MNK_JK_SP_POST = MNK_JIT_API_SP_POST,
  MNK_JK_SP_STEP = MNK_JIT_API_SP_STEP,
  MNK_JK_SP_DRAW = MNK_JIT_API_SP_DRAW,  // + 3 * lt + which: <NW, CN, CK, Draw<LT, C>>, lt 0 f32 / 1 bf16 / 2 no logits
  MNK_JK_SP_TACTICAL = MNK_JIT_API_SP_TACTICAL,            // k_selfplay_step_tactical <NW, CN, CK, NoDraw>
  MNK_JK_SP_TACTICAL_DRAW = MNK_JIT_API_SP_TACTICAL_DRAW,  // + lt: k_selfplay_step_tactical <NW, CN, CK, Draw<LT, C>>
  MNK_JK_SAMPLE_TACTICAL = MNK_JIT_API_SAMPLE_TACTICAL,    // k_sample_tactical (needs k)
  MNK_JK_COUNT = MNK_JIT_API_COUNT
};
inline bool mnk_jit_kind_any_k(int kind) { return kind >= MNK_JK_OBSERVE && kind <= MNK_JK_GATHER_OBS; }

// The board's own variant of API kernel `kind`, or nullptr = launch the ahead-of-time kernel: the board has a built-in
// variant, MNK_JIT_API / MNK_JIT = 0, the kernel is not hot yet (fewer than 1 024 launches and 2^26 items on this board in
// this process; MNK_JIT_API / MNK_JIT = 1: compile at the first launch), `stream` is being captured and the variant does
// not exist yet (nothing is compiled or loaded under a capture), or the compilation failed (mnk_jit_last_error).
#define MNK_JIT_HOT_LAUNCHES 1024u
#define MNK_JIT_HOT_ITEMS (1ull << 26)
hipFunction_t mnk_jit_api_function(const MnkGeom& g, int kind, int64_t items, hipStream_t stream);

template <typename... P, size_t... I>
inline hipError_t mnk_module_launch_impl(hipFunction_t fn, dim3 grid, dim3 block, size_t lds, hipStream_t s,
                                         std::tuple<P...>& params, std::index_sequence<I...>) {
  void* ptrs[] = {(void*)&std::get<I>(params)...};
  return hipModuleLaunchKernel(fn, grid.x, grid.y, grid.z, block.x, block.y, block.z, (unsigned)lds, s, ptrs, nullptr);
}

// Launches a run-time compiled kernel.  `signature`: any ahead-of-time instantiation of the same kernel template -- its
// parameter list is the module function's, so every argument is converted to the exact parameter type here and a
// mismatch in the number of arguments does not compile.
template <typename... P, typename... A>
inline void mnk_module_launch(void (*signature)(P...), hipFunction_t fn, dim3 grid, dim3 block, size_t lds, hipStream_t s,
                              A&&... a) {
  (void)signature;
  static_assert(sizeof...(P) == sizeof...(A), "argument list differs from the kernel's parameter list");
  std::tuple<P...> params{static_cast<P>(a)...};
  (void)mnk_module_launch_impl(fn, grid, block, lds, s, params, std::index_sequence_for<P...>{});  // (mnk_launch_status reads the error)
}

// an ahead-of-time kernel or, with `fn`, the run-time compiled function of the same kernel template
template <typename... P, typename... A>
inline void mnk_launch(void (*kernel)(P...), hipFunction_t fn, dim3 grid, dim3 block, hipStream_t s, const A&... a) {
  if (fn) mnk_module_launch(kernel, fn, grid, block, 0, s, a...);
  else hipLaunchKernelGGL(kernel, grid, block, 0, s, a...);
}

// ================================================================== the random rollout and the replay of its log
// (mnk_rollout*.hip).  Every rollout kernel takes one parameter list, MnkRolloutArgs; what each kernel form can do is
// mnk_rollout_form_ok and which one a launch gets is mnk_rollout_plan -- pure functions, stated here once.
struct MnkRolloutArgs {
  MnkGeom g;
  uint64_t* planes; uint32_t* meta;  // the state, updated in place
  int64_t N; int T;
  uint64_t seed, step0; int64_t env_id0;
  uint64_t* rec_planes; uint32_t* rec_meta;  // records: both pointers or neither
  int64_t* stats;
  void* act_log; int act;  // the log and its format (MNK_ACT_*), 0 without a log
  hipStream_t stream;
  bool rec() const { return rec_planes != nullptr; }
  dim3 grid(int envs_per_block) const { return dim3((unsigned)((N + envs_per_block - 1) / envs_per_block)); }
};

// (`kernel` alone: the ahead-of-time kernel; with `fn`: the module function, `kernel` any instantiation of its template)
template <typename K>
inline void mnk_rollout_launch(K kernel, hipFunction_t fn, dim3 grid, dim3 block, const MnkRolloutArgs& a) {
  mnk_launch(kernel, fn, grid, block, a.stream, a.g, a.planes, a.meta, a.N, a.T, a.seed, a.step0, a.env_id0, a.rec_planes,
             a.rec_meta, (unsigned long long*)a.stats, a.act_log);
}

// The (rec, act) ladder: f(std::bool_constant<REC>{}, std::integral_constant<int, ACT>{}) for the run-time (rec, act).
// `keep(REC, ACT)`, a captureless lambda, names the combinations the caller has kernels for: f is instantiated for no
// other, and false comes back when the run-time pair is not among them.
template <bool REC, int ACT, typename Keep, typename F>
inline bool mnk_rec_act_case(bool rec, int act, Keep keep, F& f) {
  if constexpr (keep(REC, ACT)) {
    if (rec == REC && act == ACT) {
      f(std::bool_constant<REC>{}, std::integral_constant<int, ACT>{});
      return true;
    }
  }
  return false;
}
template <typename Keep, typename F, int... ACT>
inline bool mnk_rec_act_cases(bool rec, int act, Keep keep, F& f, std::integer_sequence<int, ACT...>) {
  return ((mnk_rec_act_case<true, ACT>(rec, act, keep, f) || mnk_rec_act_case<false, ACT>(rec, act, keep, f)) || ...);
}
template <typename Keep, typename F>
inline bool mnk_rec_act(bool rec, int act, Keep keep, F&& f) {
  return mnk_rec_act_cases(rec, act, keep, f, std::make_integer_sequence<int, MNK_ACT_U8P1 + 1>{});
}

// f(MnkBoard{}) for the ahead-of-time one-lane rollout / replay variant of g's board: its row of MNK_BUILTIN_BOARDS, else
// the generic form of its word count (CN = CK = C = 0).  Boards with more than 16 register words per plane (planes of
// more than 512 bits) have these kernels as run-time specialisations only: their generic ahead-of-time forms took 20
// minutes to compile for kernels nobody's default board runs.  The API-level kernels keep a generic 32-word variant.
template <typename F>
inline void mnk_rollout_board(const MnkGeom& g, F&& f) {
  if (mnk_builtin_board(g, [&](auto row) { f(row); return true; })) return;
  if (g.NW <= 2) f(MnkBoard<2, 0, 0, 0>{});
  else if (g.NW <= 4) f(MnkBoard<4, 0, 0, 0>{});
  else if (g.NW <= 8) f(MnkBoard<8, 0, 0, 0>{});
  else f(MnkBoard<16, 0, 0, 0>{});
}
// is that variant built with log format `act`?  The bit-packed logs only where a board that takes the variant can use
// them: U8P1 (more than 256 cells) on 19x19 and the generic 16-word form, the 7-bit stream (at most 128 cells) on 9x9, 3x3
// and the generic forms of up to 8 words (e.g. 11x11 = 121 cells, NW 5); bytes and 16 bits everywhere.
template <typename Row>
constexpr bool mnk_lane_built(int act) {
  if (act == MNK_ACT_U8P1) return Row::CN ? Row::C > 256 : Row::NW == 16;
  if (act == MNK_ACT_BITS7) return Row::CN ? Row::C <= 128 : Row::NW <= 8;
  return true;
}

// ---- what each kernel form can do.  `form`: MNK_ROLLOUT_* of mnk_hip.h, or the run-time compiled pair kernel:
enum { MNK_ROLLOUT_PAIR_JIT = MNK_ROLLOUT_WS4 + 1 };
constexpr bool mnk_rollout_form_ok(int form, int n, int k, int NW, int C, int act) {
  const bool builtin = mnk_geom_builtin(n, k, NW), bytes = act == 0 || act == MNK_ACT_U8 || act == MNK_ACT_U16;
  switch (form) {
    case MNK_ROLLOUT_LANE: return mnk_act_format_ok(act, C);
    // (the direction split writes byte / 16-bit logs only; every row has them, 19x19's byte log included, which no launch
    // asks for -- 361 cells -- but which stays built)
    case MNK_ROLLOUT_PAIR: return builtin && bytes;
    case MNK_ROLLOUT_PAIR_JIT: return bytes;
    // the five-in-a-row rows: 9x9, 13x13, 15x15, 19x19.  Boards up to 256 cells log a byte per action; 19x19 = 361 needs
    // two, or a byte and a bit
    case MNK_ROLLOUT_PAIRW: return builtin && k == 5 && (bytes || (act == MNK_ACT_U8P1 && C > 256));
    case MNK_ROLLOUT_WS2:
    case MNK_ROLLOUT_WS4: return builtin && (n == 9 || n == 19) && act == 0;
  }
  return false;
}
template <typename Row>
constexpr bool mnk_rollout_row_ok(int form, int act) {
  return mnk_rollout_form_ok(form, Row::CN, Row::CK, Row::NW, Row::C, act);
}

// do the record rows of one launch fit 32-bit byte offsets?  (what the two-lane forms and the SADDR stores address with)
constexpr bool mnk_rollout_fits32(int NW, int64_t N, int T) { return ((int64_t)T * NW + 1) * N * 8 < (1ll << 32); }

// ---- which kernel a launch gets
enum { MNK_PLAN_AOT = 0, MNK_PLAN_JIT_TRY, MNK_PLAN_JIT_ONLY };
struct MnkRolloutPlan {
  int form;    // MNK_ROLLOUT_LANE .. _WS4; 0: nothing to launch, `status` says why
  bool saddr;  // the one-lane kernel stores its records as `uniform base + 32-bit lane offset` (mnk_rollout_lane.h)
  int jit;     // MNK_PLAN_*: the ahead-of-time kernel / the board's run-time compiled one, with / without one behind it
  int status = MNK_OK;
};

// The rules of mnk_hip.h (mnk_rollout_form), in their order.  No HIP call, no environment, no allocation.
inline MnkRolloutPlan mnk_rollout_plan(const MnkGeom& g, int64_t N, int T, bool rec, int act, const MnkConfig& cfg,
                                       bool jit_failed) {
  const auto ok = [&](int form) { return mnk_rollout_form_ok(form, g.n, g.k, g.NW, g.C, act); };
  const bool fits32 = mnk_rollout_fits32(g.NW, N, T);
  // two lanes per env only while both lanes of every env still fit one wave per SIMD (2N <= 65 536 lanes: 9x9x5 106 vs
  // 135 us per 256 plies at 32 768 envs, 164 vs 135 at 36 864; tools/exp_pair_threshold.py)
  const bool small = cfg.pair_override >= 0 ? cfg.pair_override != 0 : N <= 32768;
  // 32-bit record offsets while a wave is alone on its SIMD (N <= 65 536: the kernel is bound by its instruction count and
  // this saves ~4 of ~150 per ply: 92.0 -> 88.5 us at the headline size); from 131 072 envs up the kernel is bound by the
  // HBM write rate and the 64-bit form measured faster (157 vs 166-184 us), so it stays there
  const bool saddr = rec && !cfg.saddr_off && N <= 65536 && fits32;
  // 1. a forced waves-per-group form (A/B timing, parity tests), where the board has it
  if ((cfg.form == MNK_ROLLOUT_WS2 || cfg.form == MNK_ROLLOUT_WS4) && ok(cfg.form)) return {cfg.form, false, MNK_PLAN_AOT};
  // 2. a board without ahead-of-time variants gets its own at run time (mnk_jit.hip) once a launch is large enough to pay
  // for the ~1 s of compilation: 2^20 env-steps (4 096 envs x 256 plies).  Two lanes per env for small batches, like the
  // built-in boards; the compiled one-lane kernel is also the next try after a pair kernel that does not compile.
  if (!mnk_geom_builtin(g.n, g.k, g.NW)) {
    const bool only = g.NW > 16;  // (mnk_rollout_board)
    const bool want = only || (cfg.jit >= 0 ? cfg.jit != 0 : N * (int64_t)T >= (1ll << 20));
    if (want && !jit_failed) {
      const bool pair = ok(MNK_ROLLOUT_PAIR_JIT) && fits32 && small && cfg.form != MNK_ROLLOUT_LANE;
      return {pair ? MNK_ROLLOUT_PAIR : MNK_ROLLOUT_LANE, saddr, only ? MNK_PLAN_JIT_ONLY : MNK_PLAN_JIT_TRY};
    }
    if (only) return {0, false, MNK_PLAN_AOT, MNK_ELAUNCH};
  }
  // 3. two lanes per env split by WORDS on the boards where that measured faster (us per 256 plies at 32 768 envs, by
  // directions / by words: 19x19 216 / 164, 15x15 155 / 135, 13x13 127 / 117; 9x9 86 / 98 stays split by directions).
  // A forced `pair` yields to it for the log only the word split writes.
  if (ok(MNK_ROLLOUT_PAIRW) && fits32 &&
      (cfg.form == MNK_ROLLOUT_PAIRW || (small && g.n >= 13 && !(cfg.form == MNK_ROLLOUT_PAIR && ok(MNK_ROLLOUT_PAIR)))))
    return {MNK_ROLLOUT_PAIRW, false, MNK_PLAN_AOT};
  // 4. split by directions
  if (ok(MNK_ROLLOUT_PAIR) && fits32 && small) return {MNK_ROLLOUT_PAIR, false, MNK_PLAN_AOT};
  // 5. one lane per env (the 7-bit log exists in this form only); generic boards address records with 64-bit pointers
  return {MNK_ROLLOUT_LANE, saddr && mnk_geom_builtin(g.n, g.k, g.NW), MNK_PLAN_AOT};
}

// the launchers of the forms, one translation unit each (they compile in parallel); the plan has checked mnk_rollout_form_ok
void mnk_launch_rollout_lane(const MnkRolloutArgs& a, bool saddr);  // without a log (mnk_rollout.hip)
void mnk_launch_rollout_log(const MnkRolloutArgs& a, bool saddr);   // one lane, with one (mnk_rollout_log.hip)
void mnk_launch_rollout_pair(const MnkRolloutArgs& a);
void mnk_launch_rollout_pairw(const MnkRolloutArgs& a);
void mnk_launch_rollout_ws(const MnkRolloutArgs& a, int ws);  // ws = 2 or 4

// run-time specialised rollout kernels (mnk_jit.hip, hiprtc): kind MNK_JIT_ROLLOUT / _REPLAY / _ROLLOUT_PAIR; nullptr when
// the compile failed.  Launched with mnk_launch.
hipFunction_t mnk_jit_rollout_function(const MnkGeom& g, int kind, bool rec, int act, bool saddr);
