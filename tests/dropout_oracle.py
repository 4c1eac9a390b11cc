"""Host restatement of the training kernels' counter-based dropout mask (cotr_amd/csrc/train.h, attention_train.hip) and of
the seed sequence of cotr_amd/train_ops.py, in plain numpy: nothing is imported from the library and nothing is called in it.

With it every dropout path has an exact-mask fp64 reference (tests/test_train_dropout_fp64_gpu.py,
tests/test_train_step_dropout_fp64_gpu.py).  The contract it restates is written down in DESIGN.md ("The dropout mask
contract"): a change to the hash, the threshold rule, the salt XOR, an index convention or the seed sequence must change this
file with it.

    keep(element) = hash(seed ^ salt, index) >= thresh(p)          kept elements are scaled by 1 / (1 - p)
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
ATT_KEYS = 512
ATT_HEADS = 8


def thresh(p):
    """train_thresh: p goes through float32; p <= 0 (or NaN) -> 0; floor(p * 2^32), clamped at 2^32 - 1."""
    p = float(np.float32(p))
    if not p > 0.0:
        return 0
    t = p * 4294967296.0
    return 4294967295 if t >= 4294967295.0 else int(t)


def inv_keep(p):
    """The factor of a kept element as the kernels' callers compute it: 1.f / (1.f - p) in float32."""
    p = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p)) if p > 0 else 1.0


def _mul32(a, c):
    return (a * np.uint64(c)) & _M32


def hash32(seed, idx):
    """The 64 -> 32 bit mixer of train_keep on an array of uint64 indices -> uint64 array of 32-bit values.  (32-bit
    arithmetic is done in uint64 and masked: numpy's uint64 products wrap modulo 2^64, which keeps the low 32 bits exact.)"""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = np.uint64(int(seed) & 0xFFFFFFFF)
    x = (idx & _M32) ^ _mul32(seed, 0x9E3779B9)
    hi = (idx >> np.uint64(32)) ^ seed
    x = x ^ ((_mul32(hi, 0x85EBCA6B) + np.uint64(0xC2B2AE35)) & _M32)
    x = x ^ (x >> np.uint64(16))
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> np.uint64(15))
    x = _mul32(x, 0x846CA68B)
    x = x ^ (x >> np.uint64(16))
    return x


def keep(seed, idx, p, salt=None):
    """train_keep(train_salted(seed, salt), idx, train_thresh(p)) -> bool array of idx's shape."""
    seed = int(seed) & 0xFFFFFFFF
    if salt is not None:
        seed ^= int(salt) & 0xFFFFFFFF
    return hash32(seed, idx) >= np.uint64(thresh(p))


def flat_index(rows, n, row0=0):
    """Element offsets of a row-major [rows, n] block that starts at row ``row0`` of its tensor -> uint64 [rows, n]:
    AddDropLN (n = 256: the dropout on ``a`` and its backward) and Proj with ReLU and p (cotr_train_dropout_fwd on y)."""
    r = np.arange(row0, row0 + rows, dtype=np.uint64)[:, None]
    return r * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :]


def flat_mask(seed, rows, n, p, salt=None, row0=0):
    return keep(seed, flat_index(rows, n, row0), p, salt)


def attention_index(nb, nq, pair0=0, queries=None):
    """mask_index of attention_train.hip: ((pair * 8 + head) * nq + qi) * 512 + key for pairs pair0 .. pair0 + nb - 1 and the
    given queries (default all nq) -> uint64 [nb, 8, len(queries), 512].  The index does not depend on the number of pairs."""
    qi = np.arange(nq, dtype=np.uint64) if queries is None else np.asarray(queries, dtype=np.uint64)
    pair = np.arange(pair0, pair0 + nb, dtype=np.uint64)[:, None, None, None]
    head = np.arange(ATT_HEADS, dtype=np.uint64)[None, :, None, None]
    key = np.arange(ATT_KEYS, dtype=np.uint64)[None, None, None, :]
    return ((pair * np.uint64(ATT_HEADS) + head) * np.uint64(nq) + qi[None, None, :, None]) * np.uint64(ATT_KEYS) + key


def attention_mask(seed, nb, nq, p, salt=None, pair0=0, queries=None):
    """The mask on the attention probabilities -> bool [nb, 8, nq (or len(queries)), 512]."""
    return keep(seed, attention_index(nb, nq, pair0, queries), p, salt)


def seeds(base, n):
    """The first n values of train_ops.next_seed() after train_ops.reseed(base)."""
    base = int(base) & 0xFFFFFFFF
    out = []
    for count in range(1, n + 1):
        x = (base * 0x9E3779B1 + count * 0x85EBCA77) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
        x ^= x >> 12
        out.append(x)
    return out
