"""The matching kernels (csrc/sfm_match.hip) against the NumPy stand-in of the contract: bitwise-equal indices and
float32 distances for integer L2 and Hamming, a float64 oracle with a tolerance for general float L2."""
import numpy as np
import pytest

import _bfmatcher_numpy as bfm

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 31, 32, 33, 127, 128, 129, 1000, 8191)


def sift_like(rng, n):
    d = rng.gamma(0.6, 1.0, (n, 128))
    return np.clip(np.rint(d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9) * 512.0), 0, 255).astype(np.uint8)


def check(native, metric, query, refs, mode):
    norm = bfm.NORM_L2 if metric == native.MATCH_L2 else bfm.NORM_HAMMING
    q = native.DescriptorSet(metric, query)
    rs = [native.DescriptorSet(metric, r) for r in refs]
    try:
        bi, bd, si, sd, mu = native.match(q, rs, mode)
    finally:
        for r in rs:
            r.close()
        q.close()
    for k, r in enumerate(refs):
        idx, dist, cb = bfm.neighbours(norm, query, r, k=2, col_best=True)
        np.testing.assert_array_equal(bi[k], idx[:, 0])
        np.testing.assert_array_equal(bd[k].view(np.uint32), dist[:, 0].view(np.uint32))
        if mode == native.MATCH_KNN2:
            np.testing.assert_array_equal(si[k], idx[:, 1])
            np.testing.assert_array_equal(sd[k].view(np.uint32), dist[:, 1].view(np.uint32))
        if mode == native.MATCH_MUTUAL:
            want = (idx[:, 0] >= 0) & (cb[np.maximum(idx[:, 0], 0)] == np.arange(query.shape[0]))
            np.testing.assert_array_equal(mu[k], want)
    return bi, bd, si, sd, mu


@pytest.mark.parametrize("nq", SIZES)
def test_l2_sizes_query(hip, nq):
    rng = np.random.default_rng(nq)
    check(hip, hip.MATCH_L2, sift_like(rng, nq), [sift_like(rng, 129), sift_like(rng, 2)], hip.MATCH_KNN2)


@pytest.mark.parametrize("nt", SIZES)
def test_l2_sizes_train(hip, nt):
    rng = np.random.default_rng(100 + nt)
    mode = hip.MATCH_KNN2 if nt > 1 else hip.MATCH_NN1
    check(hip, hip.MATCH_L2, sift_like(rng, 129), [sift_like(rng, nt)], mode)


@pytest.mark.parametrize("nt", (1, 2, 33, 1000, 8191))
def test_hamming_sizes(hip, nt):
    rng = np.random.default_rng(200 + nt)
    q = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    check(hip, hip.MATCH_HAMMING, q, [rng.integers(0, 256, (nt, 32), dtype=np.uint8)], hip.MATCH_KNN2 if nt > 1 else hip.MATCH_NN1)


def test_hamming_odd_width_and_mutual(hip):
    rng = np.random.default_rng(7)
    q = rng.integers(0, 256, (500, 13), dtype=np.uint8)
    refs = [rng.integers(0, 256, (n, 13), dtype=np.uint8) for n in (2, 700, 1500)]
    refs[1][:500] = q ^ (rng.random(q.shape) < 0.05).astype(np.uint8)        # near matches
    check(hip, hip.MATCH_HAMMING, q, refs, hip.MATCH_MUTUAL)


def test_several_views_one_launch_with_ties(hip):
    rng = np.random.default_rng(8)
    q = sift_like(rng, 1000)
    refs = [sift_like(rng, n) for n in (2, 500, 3000, 1025)]
    refs[2][100:200] = refs[2][50]              # many exact duplicate train rows: the lower index wins
    refs[2][2000:2500] = q[:500]                # exact matches (d = 0) ...
    refs[2][2500:3000] = q[:500]                # ... twice: ties at distance 0
    refs[3][1024] = refs[3][3]                  # a duplicate across the chunk border
    for mode in (hip.MATCH_KNN2, hip.MATCH_NN1, hip.MATCH_MUTUAL):
        check(hip, hip.MATCH_L2, q, refs, mode)


def test_large_s_ties_in_reverse_index_order(hip):
    # two train rows whose s differ (s >= 2^22) but round to the same float32 distance, the larger s at the LOWER
    # index: the contract orders by (d, index), so the lower index wins although its s is larger
    dim = 256
    q = np.zeros((1, dim), dtype=np.uint8)
    found = None
    for s_hi in range(255 * 255 * 70, 255 * 255 * 70 + 200000):
        d = bfm.sqrt_rn_f32(np.array([s_hi]))[0]
        d2 = bfm.sqrt_rn_f32(np.array([s_hi - 1]))[0]
        if d == d2:
            found = s_hi
            break
    assert found is not None and found >= (1 << 22)

    def row_with_s(s):
        r = np.zeros(dim, dtype=np.int64)
        i = 0
        while s > 0:
            v = min(255, int(np.floor(np.sqrt(s))))
            r[i] = v
            s -= v * v
            i += 1
        return r.astype(np.uint8)
    t = np.stack([row_with_s(found), row_with_s(found - 1), row_with_s(found + 5000)])
    assert ((t.astype(np.int64) ** 2).sum(1)[:2] == [found, found - 1]).all()
    bi, bd, si, sd, _ = check(hip, hip.MATCH_L2, q, [t], hip.MATCH_KNN2)
    assert bi[0, 0] == 0 and si[0, 0] == 1 and bd[0, 0] == sd[0, 0]


def test_crosscheck_and_nn1_large(hip):
    rng = np.random.default_rng(9)
    q = sift_like(rng, 3000)
    t = sift_like(rng, 5000)
    t[:3000] = np.clip(q.astype(np.int64) + rng.integers(-2, 3, q.shape), 0, 255)
    for mode in (hip.MATCH_MUTUAL, hip.MATCH_NN1):
        check(hip, hip.MATCH_L2, q, [t, t[:1500]], mode)


def test_two_runs_identical_bytes(hip):
    rng = np.random.default_rng(10)
    q = sift_like(rng, 2000)
    refs = [sift_like(rng, n) for n in (3000, 2048)]
    a = check(hip, hip.MATCH_L2, q, refs, hip.MATCH_MUTUAL)
    b = check(hip, hip.MATCH_L2, q, refs, hip.MATCH_MUTUAL)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_general_float_l2_against_float64(hip):
    rng = np.random.default_rng(11)
    q = rng.normal(size=(400, 64)).astype(np.float32)
    t = rng.normal(size=(1500, 64)).astype(np.float32)
    qs, ts = hip.DescriptorSet(hip.MATCH_L2, q), hip.DescriptorSet(hip.MATCH_L2, t)
    assert not qs.exact and not ts.exact
    bi, bd, si, sd, _ = hip.match(qs, [ts], hip.MATCH_KNN2)
    qs.close(); ts.close()
    d = np.sqrt(((q.astype(np.float64)[:, None, :] - t.astype(np.float64)[None]) ** 2).sum(-1))
    order = np.argsort(d, axis=1, kind="stable")
    d_sorted = np.take_along_axis(d, order, 1)
    clear = (d_sorted[:, 1] - d_sorted[:, 0] > 1e-4 * d_sorted[:, 1]) & (d_sorted[:, 2] - d_sorted[:, 1] > 1e-4 * d_sorted[:, 2])
    assert clear.sum() > 300
    np.testing.assert_array_equal(bi[0][clear], order[clear, 0])
    np.testing.assert_array_equal(si[0][clear], order[clear, 1])
    np.testing.assert_allclose(bd[0], d_sorted[:, 0], rtol=1e-5)
    np.testing.assert_allclose(sd[0], d_sorted[:, 1], rtol=1e-5)


def test_float_rows_with_integer_values_take_the_exact_path(hip):
    rng = np.random.default_rng(12)
    q = sift_like(rng, 200)
    t = sift_like(rng, 300)
    qs = hip.DescriptorSet(hip.MATCH_L2, q.astype(np.float32))
    ts = hip.DescriptorSet(hip.MATCH_L2, t)
    assert qs.exact and ts.exact
    assert qs.upload_bytes == 200 * 128 * 4 and ts.upload_bytes == 300 * 128
    qs.close(); ts.close()
    check(hip, hip.MATCH_L2, q.astype(np.float32), [t.astype(np.float32)], hip.MATCH_KNN2)


def test_bad_input_is_refused(hip):
    rng = np.random.default_rng(13)
    q = hip.DescriptorSet(hip.MATCH_L2, sift_like(rng, 10))
    t64 = hip.DescriptorSet(hip.MATCH_L2, rng.integers(0, 256, (10, 64), dtype=np.uint8))
    h = hip.DescriptorSet(hip.MATCH_HAMMING, rng.integers(0, 256, (10, 128), dtype=np.uint8))
    empty = hip.DescriptorSet(hip.MATCH_L2, np.zeros((0, 128), dtype=np.uint8))
    for refs in ([t64], [h], [empty]):
        with pytest.raises(ValueError):
            hip.match(q, refs, hip.MATCH_KNN2)
    with pytest.raises(ValueError):
        hip.DescriptorSet(hip.MATCH_HAMMING, np.zeros((3, 8), dtype=np.float32))
    for s in (q, t64, h, empty):
        s.close()
