"""The float operations of the PUCT rules that include/mnk_hip.h pins down to the single rounding, each written once
(test helper).  The rules (tests/puct_rule.py, puct_search_rule.py, puct_gumbel_rule.py) call them as ``puct_ops.NAME``,
so that a test can put a defect a kernel could have in the place of one of them (tests/test_near_tie_cpu.py) and see
whether its inputs notice.  Every operation is a numpy float32 operation, rounded on its own."""
import numpy as np

f32 = np.float32


def sqrt(x):
    """fl32(sqrt(x)) of a visit count"""
    return np.sqrt(f32(x))


def score(q, c, prior, sq, na):
    """s = q + ((c * prior) * sq) / (1 + na): q, prior float32 arrays, c, sq float32, na integers"""
    u = (c * prior) * sq / (1 + na).astype(f32)
    return (q + u.astype(f32)).astype(f32)


def fpu_q(qv, r, mass):
    """q_v - r * mass of first-play urgency, the product rounded before the difference"""
    return f32(qv - f32(r * mass))


def forcing_bound(k_forced, prior, S):
    """the right side of the forcing test n'^2 < k * P * S'"""
    return f32(f32(f32(k_forced) * prior) * S)


def floor_bound(k_forced, prior, S):
    """t_a = k * P * (n_0 - 1) of the pruning's floor"""
    return f32(f32(f32(k_forced) * prior) * S)


def backup_order(L):
    """the order in which a round backs its L slots up"""
    return range(L)
