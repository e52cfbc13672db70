"""GPU: the r-th-set-bit select of the rollout kernels (bs_select_hot, csrc/mnk_device.h) against a plain loop --
random strings of 1, 3 and 12 words, every rank below each string's popcount, the bit index and the one-hot."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build_hip()
    entry._ensure_path()
    import mnk_hip

    mnk_hip.load()
    assert torch.cuda.is_available()
    return mnk_hip


def strings(nw, rng):
    """random words of every density, plus the edge cases: single bits at each end of every word, all ones"""
    dens = rng.random((512, 1))
    bits = rng.random((512, nw * 32)) < dens
    x = np.packbits(bits.reshape(512, nw, 32)[:, :, ::-1], axis=-1, bitorder="big").view(">u4").astype(np.uint32)
    x = x.reshape(512, nw)
    edge = [np.full(nw, 0xFFFFFFFF, np.uint32)]
    for w in range(nw):
        for b in (0, 1, 15, 16, 30, 31):
            e = np.zeros(nw, np.uint32)
            e[w] = np.uint32(1 << b)
            edge.append(e)
            edge.append(e | np.uint32(1))
    x = np.concatenate([x, np.stack(edge)])
    return x[np.array([int(sum(bin(int(v)).count("1") for v in row)) for row in x]) > 0]


@pytest.mark.parametrize("nw", [1, 3, 12])
def test_select_matches_a_plain_loop(lib, nw):
    rng = np.random.default_rng(nw)
    xs = strings(nw, rng)
    words, ranks, want_bits = [], [], []
    for row in xs:
        set_bits = [32 * w + b for w in range(nw) for b in range(32) if (int(row[w]) >> b) & 1]
        for r, bit in enumerate(set_bits):  # every r < popcount
            words.append(row)
            ranks.append(r)
            want_bits.append(bit)
    words = np.stack(words).astype(np.uint32)
    want_bits = np.array(want_bits, np.int32)
    want_hot = np.zeros_like(words)
    want_hot[np.arange(len(want_bits)), want_bits // 32] = (np.uint32(1) << (want_bits % 32).astype(np.uint32))
    count = len(ranks)
    d_words = torch.from_numpy(words.view(np.int32)).to(DEV)
    d_ranks = torch.from_numpy(np.array(ranks, np.int32)).to(DEV)
    d_bits = torch.full((count,), -1, dtype=torch.int32, device=DEV)
    d_hot = torch.full((count, nw), -1, dtype=torch.int32, device=DEV)
    rc = lib.call("mnk_probe_select_bits", lib.ptr(d_words), nw, count, lib.ptr(d_ranks), lib.ptr(d_bits), lib.ptr(d_hot),
                  lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_bits.cpu().numpy(), want_bits)
    assert np.array_equal(d_hot.cpu().numpy().view(np.uint32), want_hot)
