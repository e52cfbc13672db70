"""CPU: the rule of the PUCT player's built-in Dirichlet root noise (tests/puct_noise_rule.py, the numpy restatement the
GPU test holds the kernel to) -- the moments of its draws against Dirichlet(alpha)'s, rows that sum to 1 and stay finite
where a plain sum of gammas underflows, the degenerate rows, eps = 0, and that row i is a function of env_id0 + i."""
import numpy as np

import puct_noise_rule as rule


def test_moments_are_dirichlets():
    eta = rule.eta(np.ones((4096, 9), bool), 0.3, seed=11, step=3)
    rule.check_moments(eta, 9, float(np.float32(0.3)))
    assert np.allclose(eta.sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_rows_sum_to_one_and_stay_finite_at_a_small_alpha():
    rng = np.random.default_rng(0)
    mask = rng.random((6, 361)) < 0.7
    mask[0] = True
    eta = rule.eta(mask, 0.03, seed=5, step=1)
    assert np.isfinite(eta).all() and (eta >= 0).all()
    assert np.allclose(eta.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert (eta[~mask] == 0).all()
    # the gammas span more than forty decades here: they are kept as logarithms until the row's maximum is known
    l, tries = rule.log_gammas(361, 6, 0.03, seed=5, step=1)
    assert l.min() < -100 and np.isfinite(l).all() and tries.max() < rule.TRIES


def test_one_free_cell_a_full_board_and_eps_zero():
    rng = np.random.default_rng(1)
    C = 24
    priors = rng.random((4, C)).astype(np.float32)
    mask = rng.random((4, C)) < 0.5
    mask[1] = False
    mask[1, 7] = True      # one free cell
    mask[2] = False        # a full board
    eta = rule.eta(mask, 0.3, seed=2)
    assert eta[1, 7] == 1.0 and eta[1].sum() == 1.0 and (eta[2] == 0).all()
    out = rule.root_noise(priors, mask, 0.3, 0.25, seed=2)
    assert np.array_equal(out[2].view(np.uint32), priors[2].view(np.uint32))
    assert np.array_equal(out[~mask].view(np.uint32), priors[~mask].view(np.uint32))
    assert out[1, 7] == np.float32(np.float32(0.75) * priors[1, 7]) + np.float32(0.25)
    assert (out[mask] != priors[mask]).any()
    zero = rule.root_noise(priors, mask, 0.3, 0.0, seed=2)
    assert np.array_equal(zero.view(np.uint32), priors.view(np.uint32))
    one = rule.root_noise(priors, mask, 0.3, 1.0, seed=2)
    assert np.array_equal(one[mask], eta.astype(np.float32)[mask])


def test_a_row_depends_on_its_own_id_only():
    rng = np.random.default_rng(2)
    mask = rng.random((8, 81)) < 0.8
    whole = rule.eta(mask, 0.3, seed=9, step=4)
    part = rule.eta(mask[4:], 0.3, seed=9, step=4, env_id0=4)
    assert np.array_equal(whole[4:], part)
    assert not np.array_equal(whole[:4], part)
    assert not np.array_equal(whole, rule.eta(mask, 0.3, seed=9, step=5))


def test_leaves_read_the_root_rows_only():
    rng = np.random.default_rng(3)
    priors = rng.random((12, 9)).astype(np.float32)
    mask = rng.random((12, 9)) < 0.7
    out = rule.root_noise(priors, mask, 0.3, 0.25, seed=1, step=2, env_id0=3, leaves=4)
    assert np.array_equal(out, rule.root_noise(priors[::4], mask[::4], 0.3, 0.25, seed=1, step=2, env_id0=3))
