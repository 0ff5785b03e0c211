"""TEST-ONLY numpy restatement of the two keyed draws of sda_amd/csrc/dataset.hip on top of tests/philox_ref.py: the per-epoch
permutation of the trajectories (four-round balanced Feistel network over 2h-bit words, 4^h the smallest power of four >= N, cycle
walking; round function = word 0 of Philox at {v, e_lo, 0x80000000 | e_hi, 'SHU0' + round}) and the first frame of every row
((u (L - W + 1)) >> 32, u = word 0 at {b, s_lo, 0x80000000 | s_hi, 'WSTA'}); key = seed."""
import numpy as np

from tests import philox_ref as P

TAG_START, TAG_SHUFFLE = 0x57535441, 0x53485530
U = np.uint64


def _keys(seed):
    return seed & 0xffffffff, (seed >> 32) & 0xffffffff


def half_bits(n):
    h = 0
    while 4 ** h < n:
        h += 1
    return h


def _feistel(x, e, h, seed):
    mask = U((1 << h) - 1)
    l, r = x >> U(h), x & mask
    for rd in range(4):
        w = P.philox4x32_10(r, e & P.MASK, U(0x80000000) | (e >> U(32)), TAG_SHUFFLE + rd, *_keys(seed))[0].astype(U)
        l, r = r, l ^ (w & mask)
    return (l << U(h)) | r


def perm(p, n, e, seed):
    """perm_e(p) for broadcastable integer arrays p in [0, n) and e >= 0 -> int64 array."""
    p, e = np.broadcast_arrays(np.asarray(p, dtype=U), np.asarray(e, dtype=U))
    h = half_bits(n)
    x = _feistel(p, e, h, seed).copy()
    while True:
        bad = x >= U(n)
        if not bad.any():
            return x.astype(np.int64)
        x[bad] = _feistel(x[bad], e[bad], h, seed)


def starts(length, window, s, b, seed):
    """start of row b of global batch s (broadcastable integer arrays) -> int64 array."""
    s, b = np.broadcast_arrays(np.asarray(s, dtype=U), np.asarray(b, dtype=U))
    u = P.philox4x32_10(b, s & P.MASK, U(0x80000000) | (s >> U(32)), TAG_START, *_keys(seed))[0].astype(U)
    return ((u * U(length - window + 1)) >> U(32)).astype(np.int64)


def plan(n, length, window, batch, seed, s, rows):
    """(src_row, start) of the `rows` rows of global batch s: what sda_window_batch_plan writes."""
    spe = -(-n // batch)
    e, i = divmod(s, spe)
    b = np.arange(rows)
    return perm(i * batch + b, n, e, seed), starts(length, window, s, b, seed)
