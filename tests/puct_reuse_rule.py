"""numpy restatement of the PUCT player that keeps its tree between calls (test helper; the rule is stated in
include/mnk_hip.h, mnk_puct_rebase): ``puct_search_rule.PuctSearch`` with one leaf per evaluation and ``reuse`` -- the match
of a new observation against the stored root, the carried subtree and the root's renewed priors are stated there
(``match``, ``descend``, ``rebase``)."""
from puct_search_rule import PuctSearch, descend, match, rebase  # noqa: F401 (the names the tests know)


class ReusePuct(PuctSearch):
    """``act(obs, step=0, deterministic=False) -> (actions, visits, root_value, carried)``"""

    def __init__(self, k, iterations, c, evaluator, tree_nodes=None, seed=0, env_id0=0, temperature=0, leaves=None):
        super().__init__(k, iterations, c, evaluator, 1, True, tree_nodes, seed, env_id0, temperature, leaves)

    def act(self, obs, step=0, deterministic=False):
        return super().act(obs, step=step, deterministic=deterministic)[:4]
