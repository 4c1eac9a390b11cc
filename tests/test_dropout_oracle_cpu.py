"""tests/dropout_oracle.py - the numpy restatement of the kernels' dropout mask - against a scalar version in plain Python
integers, its statistics, and the seed sequence of cotr_amd/train_ops.py.  CPU only."""
import math

import numpy as np
import pytest

from tests import dropout_oracle as D

M32 = 0xFFFFFFFF


def _thresh_scalar(p):
    p = float(np.float32(p))
    if not p > 0.0:
        return 0
    t = p * 4294967296.0
    return M32 if t >= 4294967295.0 else int(t)


def _keep_scalar(seed, idx, p, salt=None):
    """train_keep / train_salted / train_thresh of cotr_amd/csrc/train.h, one element, Python integers."""
    if salt is not None:
        seed ^= salt
    x = (idx & M32) ^ ((seed * 0x9E3779B9) & M32)
    hi = ((idx >> 32) & M32) ^ seed
    x ^= (hi * 0x85EBCA6B + 0xC2B2AE35) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x >= _thresh_scalar(p)


def test_threshold_rule():
    assert D.thresh(0.0) == 0 and D.thresh(-0.5) == 0 and D.thresh(float('nan')) == 0
    assert D.thresh(0.5) == 1 << 31 and D.thresh(0.25) == 1 << 30
    assert D.thresh(1.0) == M32 and D.thresh(2.0) == M32
    # p goes through float32: 0.1f = 0.100000001490116..., floor(0.1f * 2^32) = 429496736 (0.1 in double gives ...729)
    assert D.thresh(0.1) == int(float(np.float32(0.1)) * 4294967296.0) == 429496736
    assert int(0.1 * 4294967296.0) == 429496729
    assert D.inv_keep(0.0) == 1.0 and D.inv_keep(0.5) == 2.0 and D.inv_keep(0.25) == float(np.float32(1.0) / np.float32(0.75))
    assert D.inv_keep(0.1) == float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)))


@pytest.mark.parametrize('p', [0.1, 0.25, 0.5, 0.999])
def test_vectorised_keep_equals_the_scalar_one(p):
    rng = np.random.default_rng(int(p * 1000))
    idx = np.concatenate([rng.integers(0, 1 << 63, 2000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 2000, dtype=np.uint64),
                          rng.integers(0, 1 << 32, 2000, dtype=np.uint64),
                          np.array([0, 1, 511, 512, M32 - 1, M32, M32 + 1, M32 + 2, (1 << 33) - 1, 1 << 33, (1 << 64) - 1], dtype=np.uint64),
                          np.uint64(1 << 32) + np.arange(-600, 600, dtype=np.int64).astype(np.uint64)])
    assert int((idx > np.uint64(M32)).sum()) > 2000 and int((idx <= np.uint64(M32)).sum()) > 2000
    for seed, salt in ((0, None), (1234567, None), (M32, None), (0x9E3779B9, 0x5bd1e995), (77, M32)):
        got = D.keep(seed, idx, p, salt)
        want = np.array([_keep_scalar(seed, int(i), p, salt) for i in idx])
        assert got.dtype == np.bool_ and np.array_equal(got, want), (seed, salt)
    # shape is kept, a Python list works too
    assert D.keep(5, idx[:12].reshape(3, 4), p).shape == (3, 4)
    assert np.array_equal(D.keep(5, [int(i) for i in idx[:12]], p), D.keep(5, idx[:12], p))


def test_p_zero_keeps_everything():
    idx = np.arange(1 << 16, dtype=np.uint64) * np.uint64(0x10001)
    assert D.keep(3, idx, 0.0).all() and D.keep(3, idx, 0.0, salt=9).all() and D.keep(3, idx, -1.0).all()


@pytest.mark.parametrize('p', [0.1, 0.25, 0.5])
def test_kept_share(p):
    n = 1 << 22
    for seed, start in ((777, 0), (99, (1 << 32) - (n >> 1))):      # the second run straddles 2^32
        kept = D.keep(seed, np.uint64(start) + np.arange(n, dtype=np.uint64), p)
        want = 1.0 - D.thresh(p) / 4294967296.0
        assert abs(kept.mean() - want) < 4 * math.sqrt(want * (1 - want) / n), (p, seed, kept.mean())


def test_seed_and_salt_change_the_mask():
    idx = np.arange(1 << 14, dtype=np.uint64)
    base = D.keep(11, idx, 0.25)
    for other in (D.keep(12, idx, 0.25), D.keep(11, idx, 0.25, salt=1), D.keep(11, idx, 0.25, salt=0x5bd1e995)):
        frac = float((other != base).mean())
        assert 0.3 < frac < 0.45, frac                       # two independent masks at p = 0.25 differ in 2 * 0.25 * 0.75
    assert np.array_equal(D.keep(11, idx, 0.25, salt=0), base)
    assert np.array_equal(D.keep(11 ^ 0x5bd1e995, idx, 0.25), D.keep(11, idx, 0.25, salt=0x5bd1e995))     # the salt is an XOR
    assert not np.array_equal(D.keep(11, idx + np.uint64(1 << 32), 0.25), base)                      # the high word takes part


def test_index_conventions():
    f = D.flat_index(3, 256)
    assert f.shape == (3, 256) and f.dtype == np.uint64 and int(f[2, 5]) == 2 * 256 + 5
    assert int(D.flat_index(2, 1024, row0=7)[1, 3]) == 8 * 1024 + 3
    assert np.array_equal(D.flat_mask(5, 4, 256, 0.1, row0=2), D.flat_mask(5, 6, 256, 0.1)[2:])
    a = D.attention_index(2, 33)
    assert a.shape == (2, 8, 33, 512) and int(a[1, 3, 32, 511]) == ((1 * 8 + 3) * 33 + 32) * 512 + 511
    assert np.array_equal(D.attention_index(1, 33, pair0=1), a[1:])
    assert np.array_equal(D.attention_index(2, 33, queries=[4, 32]), a[:, :, [4, 32]])
    # past 2^32: pair 1, head 7 of 525000 queries crosses at query 513608
    big = D.attention_index(1, 525000, pair0=1, queries=[513607, 513608])
    assert int(big[0, 7, 0, 511]) < 1 << 32 <= int(big[0, 7, 1, 0])
    m = D.attention_mask(9, 2, 33, 0.1, salt=3)
    assert m.shape == (2, 8, 33, 512) and np.array_equal(m, D.keep(9, a, 0.1, 3))


def test_seed_sequence_is_the_librarys():
    from cotr_amd import train_ops
    saved = dict(train_ops._seed)
    try:
        for base in (0, 1234, 99, M32, (1 << 40) + 17):
            train_ops.reseed(base)
            want = [train_ops.next_seed() for _ in range(80)]
            assert D.seeds(base, 80) == want
            assert all(0 <= s <= M32 for s in want) and len(set(want)) == 80
        assert D.seeds(5, 3) == D.seeds(5, 80)[:3] and D.seeds(5, 0) == []
    finally:
        train_ops._seed.update(saved)
