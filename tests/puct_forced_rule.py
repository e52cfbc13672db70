"""numpy restatement of the PUCT player with forced playouts and policy target pruning (test helper; the rule is stated
in include/mnk_hip.h, mnk_puct_step_forced): ``puct_search_rule.PuctSearch`` with ``forced`` -- None or k.  The FORCED class
of the root's candidates (an argument of its one walk), the pruning (``prune``) and the one draw of the move from the
pruned counts are stated there; here is the per-row rule's record of its plies."""
import numpy as np

from oracle import philox
from puct_search_rule import PuctSearch, floor_of, prune, root_counts, score  # noqa: F401 (the names the tests know)
from search_selfplay_async_opts_rule import AsyncOptsRule
from search_selfplay_rule import STREAM_SELFPLAY, pick_by_visits

ForcedPuct = PuctSearch  # (``act`` returns the pruned ``visits`` and the move drawn from them; ``raw_visits`` keeps n')


class AsyncOptsForcedRule(AsyncOptsRule):
    """``AsyncOptsRule(fpu=..., forced=...)``, whose plies that force (``forces``) select with the FORCED class, with the
    pruning at the end of such a ply.  ``plies`` records, per ply played, (row, ply, full, forces, the root bool [2, C], n'
    int64 [C], the counts played from, the move)"""

    def __init__(self, *args, **kw):
        self.plies = []
        super().__init__(*args, **kw)

    def _ply(self, i, visits, full):
        raw = np.asarray(visits, np.int64).copy()
        forces = self.forces(i)  # (before the ply: its count is the row's still)
        if forces:
            _, wins_only = root_counts(self.trees[i], self.C, self.solver)
            if not wins_only and raw.max() > 0:
                visits = prune(self.trees[i], raw, self.c, self.forced)
        root, p, g = self.roots[i].copy(), int(self.row_plies[i]), int(self.moves[i])
        played = super()._ply(i, visits, full)
        if played:
            counts = np.where(root[0] | root[1], 0, np.clip(visits, 0, 65535))
            x = philox.rand_u32(self.seed, np.array([self.env_id0 + i], np.uint64), p, STREAM_SELFPLAY)[0]
            self.plies.append((i, p, full, forces, root, raw, counts, pick_by_visits(counts, x, g < self.temp_plies)))
        return played
