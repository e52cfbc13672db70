"""numpy restatement of the PUCT player with first-play urgency (test helper; the rule is stated in include/mnk_hip.h,
mnk_puct_step_fpu): ``puct_search_rule.PuctSearch`` with ``fpu`` -- None, a number or (fpu, fpu_root); the q of a free cell
without a visit (``untried_q``, ``mass_of``) is stated there, as an argument of its one walk.  The per-row self-play rules
take the same argument: ``AsyncOptsRule(fpu=...)`` and ``AsyncKeepRule(fpu=...)``."""
from puct_search_rule import PuctSearch, as_pair, mass_of, untried_q  # noqa: F401 (the names the tests know)
from search_selfplay_async_keep_rule import AsyncKeepRule
from search_selfplay_async_opts_rule import AsyncOptsRule

FpuPuct = PuctSearch  # (``solver`` is off unless asked for)
AsyncOptsFpuRule = AsyncOptsRule
AsyncKeepFpuRule = AsyncKeepRule
