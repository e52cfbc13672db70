// mnk_rollout_pair.hip -- the two-lanes-per-env form of the fused random rollout (gfx950 / MI355X only).
// Its own translation unit so the many variants compile in parallel with the one-lane kernels.
#include "mnk_host.h"
#include "mnk_rollout_lane.h"

// ------------------------------------------------------------------ two lanes per env
// For SMALL batches.  With at most 32 envs per SIMD of the chip (<= 32 768 envs) the one-lane kernel leaves
// SIMDs empty.  This variant gives every env to a PAIR of adjacent lanes -- 32 envs per wave, twice the
// waves -- and splits what splits cleanly: lane 0 scans rows + columns, lane 1 diagonals + anti-diagonals (the
// shift amount is a per-lane VGPR; one DPP swap ORs the verdicts); lane r writes half r of every record row;
// each lane computes every other Philox block and hands its four words to its partner by DPP.  Move selection
// and the state update are done redundantly by both lanes (cheaper than exchanging them).  Results are
// bit-identical to the one-lane kernel (all compile-time board geometries).  The pair form executes 1.6x the
// instructions per env, so it wins exactly while both lanes of every env fit one wave per SIMD (2N <= 65 536
// lanes): the batch-size rule of mnk_rollout_plan (mnk_host.h).

// (the kernel and its body live in mnk_rollout_lane.h: boards without an ahead-of-time variant get this form compiled
// at run time too, mnk_jit.hip)

void mnk_launch_rollout_pair(const MnkRolloutArgs& a) {
  mnk_builtin_board(a.g, [&](auto row) {
    using Row = decltype(row);
    return mnk_rec_act(a.rec(), a.act, [](bool, int act) { return mnk_rollout_row_ok<Row>(MNK_ROLLOUT_PAIR, act); },
                       [&](auto rec, auto act) {
                         mnk_rollout_launch(k_rollout_random_pair<Row::NW, Row::CN, Row::CK, decltype(rec)::value, decltype(act)::value>,
                                            nullptr, a.grid(32), dim3(64), a);
                       });
  });
}
