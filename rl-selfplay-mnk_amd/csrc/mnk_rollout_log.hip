// mnk_rollout_log.hip -- the fused random rollout with the action log switched on (gfx950 / MI355X only):
// the variants the multi-GPU exchange uses.  Its own translation unit so it compiles beside mnk_rollout.hip.
#include "mnk_host.h"
#include "mnk_rollout_lane.h"

void mnk_launch_rollout_log(const MnkRolloutArgs& a, bool saddr) {
  mnk_rollout_board(a.g, [&](auto row) {
    using Row = decltype(row);
    const auto launch = [&](auto kernel) { mnk_rollout_launch(kernel, nullptr, a.grid(64), dim3(64), a); };
    // built-in boards, records on: 32-bit lane offsets for the record stores when the plan says so, with the log
    // formats each board can use (9x9 and 3x3 the 7-bit stream, 19x19 U8P1)
    if constexpr (Row::CN != 0)
      if (saddr && mnk_rec_act(true, a.act, [](bool rec, int act) { return rec && act && mnk_act_format_ok(act, Row::C); },
                               [&](auto, auto act) {
                                 launch(k_rollout_random<Row::NW, Row::CN, Row::CK, true, decltype(act)::value, true>);
                               }))
        return;
    mnk_rec_act(a.rec(), a.act, [](bool, int act) { return act != 0 && mnk_lane_built<Row>(act); }, [&](auto rec, auto act) {
      launch(k_rollout_random<Row::NW, Row::CN, Row::CK, decltype(rec)::value, decltype(act)::value>);
    });
  });
}
