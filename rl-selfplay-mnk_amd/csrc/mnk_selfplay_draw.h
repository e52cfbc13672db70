// mnk_selfplay_draw.h -- host side of the step kernels that draw their moves from logits (mnk_selfplay_*_logits of the
// C ABI).  One translation unit per entry point (mnk_selfplay_{pre,post,step}_logits.hip) so that the 15 kernel variants of
// each -- five boards x {f32, bf16, no logits} -- compile in parallel.
#pragma once
#include "mnk_selfplay_host.h"

inline int mnk_sample_args_ok(const MnkSample& sa, int64_t N, int C) {
  if (!sa.mask || !sa.actions || C < 1 || C > 1024 || N > 0x7fffffffLL) return MNK_EINVAL;
  if (sa.logits_dtype != MNK_LOGITS_F32 && sa.logits_dtype != MNK_LOGITS_BF16) return MNK_EINVAL;
  return MNK_OK;
}

// Launches kernel WHICH with the draw folded in when the board has a compile-time draw shape (the square boards of
// MNK_BUILTIN_BOARDS: the boards the reference trains on and the usual Gomoku sizes) or a run-time compiled variant of its
// own (mnk_jit.hip: any other board, any row width); false = the caller takes two launches.
template <int WHICH>
inline bool mnk_launch_sp_fused(const MnkSpArgs& a, const MnkSample& sa, hipStream_t s) {
  if (mnk_launch_sp_jit<WHICH>(a, nullptr, sa, s)) return true;  // a board without a built-in variant, once it is hot
  if (a.g.m != a.g.n) return false;
  const int lt = !sa.logits ? 2 : (sa.logits_dtype == MNK_LOGITS_BF16 ? 1 : 0);
  return MNK_BUILTIN(a.g, true,
                     if (lt == 0) mnk_launch_sp<WHICH, NW, CN, CK, Draw<float, MnkRow_::C>>(a, nullptr, sa, s);
                     else if (lt == 1) mnk_launch_sp<WHICH, NW, CN, CK, Draw<uint16_t, MnkRow_::C>>(a, nullptr, sa, s);
                     else mnk_launch_sp<WHICH, NW, CN, CK, Draw<void, MnkRow_::C>>(a, nullptr, sa, s));
}

// The body of the four logits forms of the step entry points: `rc` is the result of the argument builder that filled `a`;
// a board without a compile-time draw shape takes the draw as a launch of its own, then `actions_form` (the actions form
// of the same entry point, with sa.actions as its moves).
template <int WHICH, typename F>
inline int mnk_sp_step_logits(int rc, const MnkSpArgs& a, const MnkSample& sa, void* stream, const char* what,
                              F&& actions_form) {
  if (rc != MNK_OK) return rc;
  if ((rc = mnk_sample_args_ok(sa, a.N, a.g.C)) != MNK_OK) return rc;
  if (a.N == 0) return MNK_OK;
  if (mnk_launch_sp_fused<WHICH>(a, sa, (hipStream_t)stream)) return mnk_launch_status(what);
  if ((rc = mnk_launch_sample(sa, a.N, a.g.C, (hipStream_t)stream)) != MNK_OK) return rc;
  return actions_form();
}
