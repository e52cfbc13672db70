"""numpy restatement of the PUCT player with several leaves per row and evaluation (test helper; the rule is stated in
include/mnk_hip.h, mnk_puct_step_leaves): ``puct_search_rule.PuctSearch`` with L slots a round and no further option --
the rounds, their virtual visits, the void slots and the per-row ``trace`` are stated there."""
from puct_search_rule import PuctSearch


class LeavesPuct(PuctSearch):
    """``act(obs, step=0, deterministic=False) -> (actions, visits, root_value, carried)``; ``L`` has no default"""

    def __init__(self, k, iterations, c, evaluator, L, reuse=False, tree_nodes=None, seed=0, env_id0=0, temperature=0,
                 leaves=None):
        super().__init__(k, iterations, c, evaluator, L, reuse, tree_nodes, seed, env_id0, temperature, leaves)

    def act(self, obs, step=0, deterministic=False):
        return super().act(obs, step=step, deterministic=deterministic)[:4]


def puct_leaves(obs, k, iterations, c, evaluator, L, seed=0, step=0, env_id0=0, temperature=0, deterministic=False,
                leaves=None, trace=None):
    """one act of a fresh ``LeavesPuct``: (actions, visits, root_value); ``trace``: an optional list that receives the
    per-row trace"""
    rule = LeavesPuct(k, iterations, c, evaluator, L, seed=seed, env_id0=env_id0, temperature=temperature, leaves=leaves)
    out = rule.act(obs, step=step, deterministic=deterministic)
    if trace is not None:
        trace.extend(rule.trace)
    return out[:3]
