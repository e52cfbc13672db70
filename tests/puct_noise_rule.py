"""numpy restatement of the PUCT player's built-in Dirichlet root noise (test helper; the rule is stated in
include/mnk_hip.h, mnk_puct_root_noise).

Row i, free cells F = the root's mask, C cells, C4 = C rounded up to a multiple of 4; alpha and eps are float32 values
widened to float64.  Cell a and try t = 0 .. 15 own the Philox block u = ((step) * C4 + a) * 16 + t of stream
MNK_STREAM_NOISE, keyed by (seed, env_id0 + i); its four words give U_j = (x_j + 0.5) * 2^-32.  A try is one
Marsaglia-Tsang candidate of Gamma(alpha + 1); the first accepted one gives the cell's log-gamma of shape alpha,
l_a = ln(d v) + ln(U_3) / alpha.  eta = softmax of l over F (the maximum taken out first); the mix
P' = fl32(fl32(w P) + fl32(eps fl32(eta))), w = fl32(1 - eps), is float32 arithmetic.  Everything else is float64.
"""
import numpy as np

from oracle import philox

STREAM_NOISE = 7
TRIES = 16


def log_gammas(C, n_rows, alpha, seed=0, step=0, env_id0=0):
    """l [n_rows, C] float64 of every cell (free or not), and the number of tries each cell used (16 = the fallback)"""
    alpha = float(np.float32(alpha))
    C4 = (C + 3) & ~3
    d = alpha + 1.0 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    env = (np.uint64(env_id0) + np.arange(n_rows, dtype=np.uint64))[:, None, None]
    a = np.arange(C, dtype=np.uint64)[None, :, None]
    t = np.arange(TRIES, dtype=np.uint64)[None, None, :]
    u = (np.uint64(step) * np.uint64(C4) + a) * np.uint64(TRIES) + t
    env, u = np.broadcast_arrays(env, u)
    x = philox._block(seed, env, u, STREAM_NOISE)
    U = [(w.astype(np.float64) + 0.5) * 2.0 ** -32 for w in x]
    z = np.sqrt(-2.0 * np.log(U[0])) * np.cos((2.0 * np.pi) * U[1])
    s = 1.0 + c * z
    v = s * s * s
    with np.errstate(invalid="ignore", divide="ignore"):
        bound = 0.5 * z * z + d - d * v + d * np.log(v)
        ok = (v > 0) & (np.log(U[2]) < bound)
        cand = np.log(d * v) + np.log(U[3]) / alpha
    first = np.argmax(ok, axis=2)
    any_ok = ok.any(axis=2)
    take = np.take_along_axis(cand, first[:, :, None], axis=2)[:, :, 0]
    fallback = np.log(d) + np.log(U[3][:, :, TRIES - 1]) / alpha
    return np.where(any_ok, take, fallback), np.where(any_ok, first + 1, TRIES)


def eta(mask, alpha, seed=0, step=0, env_id0=0):
    """eta [N, C] float64: the Dirichlet(alpha) draw of every row over its free cells (``mask`` bool [N, C]); 0 elsewhere"""
    mask = np.asarray(mask).astype(bool)
    N, C = mask.shape
    l, _ = log_gammas(C, N, alpha, seed, step, env_id0)
    out = np.zeros((N, C), np.float64)
    for i in range(N):
        F = mask[i]
        if F.any():
            e = np.exp(l[i, F] - l[i, F].max())
            out[i, F] = e / e.sum()
    return out


def mix(priors, mask, noise, eps):
    """P' float32 [N, C] from float32 priors, the bool mask and eta (float64)"""
    priors = np.asarray(priors, np.float32)
    eps = np.float32(eps)
    w = np.float32(np.float32(1) - eps)
    mixed = (w * priors).astype(np.float32) + (eps * noise.astype(np.float32)).astype(np.float32)
    return np.where(np.asarray(mask).astype(bool), mixed.astype(np.float32), priors)


def root_noise(priors, mask, alpha, eps, seed=0, step=0, env_id0=0, leaves=1):
    """what mnk_puct_root_noise writes into rows i * leaves of ``out``: float32 [N, C].  ``priors`` float32 [N * leaves, C]
    (a bfloat16 tensor widened by the caller), ``mask`` [N * leaves, C]; only the rows i * leaves are read."""
    priors = np.asarray(priors, np.float32)[::leaves]
    mask = np.asarray(mask).astype(bool)[::leaves]
    return mix(priors, mask, eta(mask, alpha, seed, step, env_id0), eps)


def check_moments(noise, F, alpha):
    """every cell's mean within 5 standard errors of 1 / F and its variance within 20 % of Dirichlet(alpha)'s
    m (1 - m) / (F alpha + 1), over the rows of ``noise`` [rows, F]"""
    noise = np.asarray(noise, np.float64)
    m = 1.0 / F
    var = m * (1 - m) / (F * alpha + 1)
    se = np.sqrt(var / len(noise))
    dev = (noise.mean(axis=0) - m) / se
    ratio = noise.var(axis=0) / var
    print("moments: mean deviations in standard errors", np.round(dev, 2), "variance ratios", np.round(ratio, 3))
    assert np.all(np.abs(dev) < 5), dev
    assert np.all((ratio > 0.8) & (ratio < 1.2)), ratio


def noisy_roots(evaluator, period, noised):
    """an evaluator that answers like ``evaluator`` but for the rows i * leaves of every call 0 (mod ``period``), the
    roots', whose priors are ``noised(call // period)`` (float32 [N, C]): what a search with built-in noise sees"""
    calls = [0]

    def evaluate(leaf_obs, leaf_mask):
        priors, values = evaluator(leaf_obs, leaf_mask)
        act, first = divmod(calls[0], period)
        calls[0] += 1
        if first == 0:
            rows = noised(act)
            priors = np.asarray(priors, np.float32).copy()
            priors[::len(priors) // len(rows)] = rows
        return priors, values

    return evaluate
