"""A near-tie evaluator, the same bits in numpy and in torch (test helper).

The evaluators of the older PUCT tests are dyadic: on them ``c * p``, ``r * mass`` and ``k * P * S'`` round nothing, so a
kernel that associates a product another way, fuses a multiply-add or takes a square root an ulp low gives their bits all
the same.  This one puts sibling scores an ulp or two apart all the way down the tree: the priors lie within ``ulps`` of
1 / C, the values within ``ulps`` of one of four levels, and both are looked up by an integer hash of the position, so that
any rounding other than the rule's picks another cell within a few iterations.

    h         = sum of wa[a] over the cells of plane 0 that hold a stone + sum of wb[a] over those of plane 1   (int64)
    priors[a] = ptab[(h + 7919 * a) % P] * mask[a]      ptab: the float32 pattern of 1 / C plus 0 .. ulps
    value     = vtab[h % V]                             vtab: the pattern of -0.3, -0.1, 0.1 or 0.3 plus 0 .. ulps

The tables are made once, in numpy, and copied to the device; the torch side is integer arithmetic, a gather and a product
with a 0 / 1 mask -- no float operation whose rounding could differ from numpy's.  With ``bf16`` the patterns keep their
low 16 bits zero and the perturbations count bfloat16 ulps, so that ``.to(torch.bfloat16)`` is exact."""
import functools

import numpy as np

P, V, STRIDE = 4093, 4099, 7919  # the table sizes: primes near 4096
LEVELS = (-0.3, -0.1, 0.1, 0.3)


@functools.lru_cache(maxsize=None)
def tables(C, ulps, seed, bf16=False):
    """(wa int64 [C], wb int64 [C], ptab f32 [P], vtab f32 [V])"""
    rng = np.random.default_rng([C, ulps, seed, int(bf16)])
    wa, wb = (rng.integers(1, 2 ** 31, size=C, dtype=np.int64) for _ in range(2))
    shift = 16 if bf16 else 0
    keep = np.uint32(0xFFFF0000 if bf16 else 0xFFFFFFFF)
    base = np.float32(1.0 / C).view(np.uint32) & keep
    ptab = (base + (rng.integers(0, ulps + 1, size=P).astype(np.uint32) << shift)).astype(np.uint32).view(np.float32)
    levels = np.array(LEVELS, np.float32).view(np.uint32) & keep
    vtab = (levels[rng.integers(0, len(LEVELS), size=V)]
            + (rng.integers(0, ulps + 1, size=V).astype(np.uint32) << shift)).astype(np.uint32).view(np.float32)
    for t in (wa, wb, ptab, vtab):
        t.setflags(write=False)
    return wa, wb, ptab, vtab


def near_np(C, ulps, seed, bf16=False):
    """``evaluate(leaf_obs [B, 2, m, n] (a cell holds a stone when non-zero), leaf_mask bool [B, C]) -> (priors f32 [B, C],
    values f32 [B])``"""
    wa, wb, ptab, vtab = tables(C, ulps, seed, bf16)
    cells = STRIDE * np.arange(C, dtype=np.int64)

    def evaluate(leaf_obs, leaf_mask):
        o = (np.asarray(leaf_obs).reshape(len(leaf_obs), 2, C) != 0).astype(np.int64)
        h = (o[:, 0] * wa).sum(axis=1) + (o[:, 1] * wb).sum(axis=1)
        priors = ptab[(h[:, None] + cells) % P] * np.asarray(leaf_mask).reshape(len(o), C).astype(np.float32)
        return priors.astype(np.float32), vtab[h % V]

    return evaluate


def near_torch(C, ulps, seed, out_dtype=None, record=None, device="cpu", bf16=False):
    """the same function in torch on ``device``, for float32, bfloat16 and uint8 leaves; priors and values come in
    ``out_dtype`` (float32 by default).  ``record``: a list that receives (leaf_obs f32, leaf_mask) of every call as
    numpy; without it the evaluator is capturable"""
    import torch

    wa, wb, ptab, vtab = (torch.from_numpy(t.copy()).to(device) for t in tables(C, ulps, seed, bf16))
    cells = STRIDE * torch.arange(C, dtype=torch.int64, device=device)
    out_dtype = torch.float32 if out_dtype is None else out_dtype

    def evaluate(leaf_obs, leaf_mask):
        if record is not None:
            record.append((leaf_obs.float().cpu().numpy(), leaf_mask.cpu().numpy()))
        o = (leaf_obs.reshape(len(leaf_obs), 2, C) != 0).to(torch.int64)
        h = (o[:, 0] * wa).sum(dim=1) + (o[:, 1] * wb).sum(dim=1)
        priors = ptab[torch.remainder(h[:, None] + cells, P)] * leaf_mask.reshape(len(o), C).to(torch.float32)
        return priors.to(out_dtype), vtab[torch.remainder(h, V)].to(out_dtype)

    return evaluate
