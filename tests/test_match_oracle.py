"""The NumPy stand-in (tests/_bfmatcher_numpy.py) against exact integer arithmetic (no GPU).  The GPU matching tests
compare the kernels with the stand-in bit for bit, so the stand-in itself is pinned here: correct rounding of
sqrt_rn_f32, injectivity below 2^22 (the identity range of the kernel's canon_s), integer L2 and Hamming distances
against pure-Python brute force, and the (distance, index) order of neighbours and the column-best."""
import math
from fractions import Fraction

import numpy as np

import _bfmatcher_numpy as bfm


def _f32(x):
    return np.float32(x)


def exact_sqrt_f32(s):
    """float32(sqrt(s)), correctly rounded, for a non-negative Python int s, by exact rational comparisons."""
    if s == 0:
        return _f32(0.0)
    c = _f32(math.sqrt(s))
    for _ in range(4):
        lo, hi = np.nextafter(c, _f32(0)), np.nextafter(c, _f32(np.inf))
        mlo, mhi = (Fraction(float(lo)) + Fraction(float(c))) / 2, (Fraction(float(c)) + Fraction(float(hi))) / 2
        if s < mlo * mlo:
            c = lo
        elif s > mhi * mhi:
            c = hi
        else:
            assert s != mlo * mlo and s != mhi * mhi          # float midpoints are never square roots of integers
            return c
    raise AssertionError("no convergence for %d" % s)


def test_sqrt_strictly_increasing_below_2p22():
    s = np.arange(0, (1 << 22) + 1, dtype=np.int64)
    d = bfm.sqrt_rn_f32(s)
    assert d[0] == 0 and (np.diff(d.view(np.uint32).astype(np.int64)) > 0).all()
    # ... and no longer injective just above 2^22: the reason canon_s exists
    s = np.arange(1 << 22, (1 << 22) + 200000, dtype=np.int64)
    assert (np.diff(bfm.sqrt_rn_f32(s)) == 0).any()


def test_sqrt_correctly_rounded_above_2p22():
    rng = np.random.default_rng(20)
    s = np.concatenate((rng.integers(1 << 22, 1 << 25, 100000),
                        np.arange((1 << 23) - 2000, (1 << 23) + 2001), np.arange((1 << 24) - 2000, (1 << 24) + 2001),
                        [1 << 22, (1 << 25) - 1])).astype(np.int64)
    d = bfm.sqrt_rn_f32(s)
    assert ((d >= 2048) & (d < 8192)).all()
    # here ulp(d) is 2^-12 or 2^-11, so d, its neighbours and the midpoints m are integers in units of 2^-13;
    # 2m * 2^13 = (x + y) * 2^13 with x, y adjacent floats, and m < sqrt(s) <=> (2m)^2 < 4 s, in Python ints
    cand = {}
    for k, name in ((0, "d"), (-1, "pred"), (1, "succ")):
        cand[name] = (d.view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(np.float32)
    sc = [(cand[n].astype(np.float64) * 8192.0).astype(np.int64) for n in ("pred", "d", "succ")]
    assert all(np.array_equal(x.astype(np.float64) / 8192.0, cand[n].astype(np.float64)) for x, n in zip(sc, ("pred", "d", "succ")))
    for i in range(s.shape[0]):
        si, p, c, n = int(s[i]), int(sc[0][i]), int(sc[1][i]), int(sc[2][i])
        lo2, hi2, four_s = (p + c) ** 2, (c + n) ** 2, 4 * si * (1 << 26)
        assert lo2 < four_s < hi2, (si, float(d[i]))


def test_sqrt_matches_exact_reference_on_a_sample():
    rng = np.random.default_rng(21)
    s = np.concatenate((np.arange(0, 300), rng.integers(0, 1 << 31, 300), [(1 << 31) - 1, 255 * 255 * 256]))
    got = bfm.sqrt_rn_f32(s)
    for v, g in zip(s.tolist(), got.tolist()):
        assert np.float32(g).view(np.uint32) == exact_sqrt_f32(int(v)).view(np.uint32), v


def _l2_brute(q, t):
    return [[exact_sqrt_f32(sum((int(a) - int(b)) ** 2 for a, b in zip(qr, tr))) for tr in t] for qr in q]


def _hamming_brute(q, t):
    qi = [int.from_bytes(bytes(r.tolist()), "little") for r in q]
    ti = [int.from_bytes(bytes(r.tolist()), "little") for r in t]
    return [[_f32((a ^ b).bit_count()) for b in ti] for a in qi]


def test_distances_integer_l2_against_python():
    rng = np.random.default_rng(22)
    for dim in (1, 5, 128, 256):
        q = rng.integers(0, 256, (6, dim)).astype(np.uint8)
        t = rng.integers(0, 256, (7, dim)).astype(np.uint8)
        q[0] = 0; q[1] = 255; t[0] = 255; t[1] = 0; t[2] = 254; t[3] = q[2]
        t[4] = 255; t[4, :: 3] = 254
        for qq, tt in ((q, t), (q.astype(np.float32), t.astype(np.float32))):
            got = bfm.distances(bfm.NORM_L2, qq, tt)
            want = np.array(_l2_brute(q, t), dtype=np.float32)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        if dim == 256:
            assert bfm.distances(bfm.NORM_L2, q[:1], t[:1])[0, 0] == np.float32(4080.0)      # s = 256 * 255^2


def test_distances_hamming_against_python():
    rng = np.random.default_rng(23)
    for width in (1, 3, 32, 61, 256):
        q = rng.integers(0, 256, (5, width)).astype(np.uint8)
        t = rng.integers(0, 256, (6, width)).astype(np.uint8)
        q[0] = 0; t[0] = 255; t[1] = q[1]
        got = bfm.distances(bfm.NORM_HAMMING, q, t)
        np.testing.assert_array_equal(got, np.array(_hamming_brute(q, t), dtype=np.float32))
        assert got[0, 0] == 8 * width


def test_neighbours_order_and_column_best_against_sorted():
    rng = np.random.default_rng(24)
    for trial in range(40):
        norm = (bfm.NORM_L2, bfm.NORM_HAMMING)[trial % 2]
        nq, nt, dim = int(rng.integers(1, 9)), int(rng.integers(1, 9)), int(rng.integers(1, 6))
        q = rng.integers(0, 3, (nq, dim)).astype(np.uint8)           # few values: many equal distances
        t = rng.integers(0, 3, (nt, dim)).astype(np.uint8)
        if nt > 2:
            t[nt - 1] = t[0]                                          # an exact duplicate row, higher index
        d = (_l2_brute if norm == bfm.NORM_L2 else _hamming_brute)(q, t)
        idx, dist, cb = bfm.neighbours(norm, q, t, k=2, col_best=True)
        for i in range(nq):
            order = sorted(range(nt), key=lambda j: (float(d[i][j]), j))[:2]
            order += [-1] * (2 - len(order))
            assert idx[i].tolist() == order, (trial, i)
            for k, j in enumerate(order):
                assert (dist[i, k] == d[i][j]) if j >= 0 else np.isinf(dist[i, k])
        for j in range(nt):
            assert cb[j] == min(range(nq), key=lambda i: (float(d[i][j]), i)), (trial, j)
