"""Every dispatch path of csrc/sfm_match.hip against exact references.

Which kernel instance each case reaches (dispatch in sfm_match_dev, sfm_match.hip:509-532; the f32 images of a mixed
launch: ensure_f32 calls at :469-471, bf16_to_f32_kernel and ensure_f32 at :350-364).  Every case runs KNN2, NN1 and
MUTUAL on the same resident sets (KNN2 and NN1 take the <..., false> instance, MUTUAL the <..., true> one):

| instance                            | band                         | cases                                                   |
|-------------------------------------|------------------------------|---------------------------------------------------------|
| match_l2_mfma_kernel<4, *>  (:509)  | exact L2, dim <= 128         | exact_l2_dims[1..128], exact_l2_size_sweep[64],         |
|                                     |                              | exact_l2_dot_product_bound[128], canonical_ties_*[128], |
|                                     |                              | many_references_one_launch[l2], match_dev_*,            |
|                                     |                              | negative_zero_rows_match_bitwise[64]                    |
| match_l2_mfma_kernel<8, *>  (:513)  | exact L2, dim 129-256        | exact_l2_dims[129..256], exact_l2_size_sweep[200],      |
|                                     |                              | exact_l2_dot_product_bound[256], canonical_ties_*[256], |
|                                     |                              | negative_zero_rows_match_bitwise[200]                   |
| match_simt_kernel<HAMMING, 8, *>    | Hamming <= 32 bytes (:526)   | hamming_widths[1,3,4,5,31,32], hamming_size_sweep[16]   |
| match_simt_kernel<HAMMING, 16, *>   | 33-64 bytes (:527)           | hamming_widths[33,61,64], hamming_size_sweep[61],       |
|                                     |                              | many_references_one_launch[hamming]                     |
| match_simt_kernel<HAMMING, 64, *>   | 65-256 bytes (:528)          | hamming_widths[65,128,255,256], hamming_size_sweep[130] |
| match_simt_kernel<FLOAT, 32, *>     | non-exact L2, dim <= 32      | float_dyadic[1,2,31,32], float_normal_bound[1,31,32]    |
|                                     | (:530)                       |                                                         |
| match_simt_kernel<FLOAT, 128, *>    | dim 33-128 (:531)            | float_dyadic[33,64,127,128], float_normal_bound[33,128],|
|                                     |                              | mixed_kind_launch[64,128]                               |
| match_simt_kernel<FLOAT, 256, *>    | dim 129-256 (:532)           | float_dyadic[129,200,256], float_normal_bound[129,256], |
|                                     |                              | mixed_kind_launch[200]                                  |
| ensure_f32 + bf16_to_f32_kernel     | exact sets in a mixed launch | mixed_kind_launch (dims 64, 200: stride dim != dp)      |
| sfm_match_dev                       | caller's stream, NULL outputs| match_dev_on_torch_stream, match_dev_empty_query        |

References: the NumPy stand-in (_bfmatcher_numpy) bit for bit for integer L2 and Hamming; for dyadic float data the
exact sqrt_rn_f32(S) / 8 (every fp32 operation of the kernel is exact there); for random float data a float64
reference with a proven error bound.  NaN and inf inputs are outside the contract and not tested."""
import math

import numpy as np
import pytest

import _bfmatcher_numpy as bfm

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)                      # MATCH_KNN2, MATCH_NN1, MATCH_MUTUAL
U = 2.0 ** -24                         # unit roundoff of float32
NQ = (1, 127, 128, 129, 257)           # around the 128-row query tile
NT = (1, 15, 16, 17, 1023, 1024, 1025, 2049)     # around the 16-column tile and the 1 024-column chunk


def int_rows(rng, n, dim):
    """Integer rows in [0, 255]: per row uniform, 0/255 (large s, the canon_s branch) or 0..2 (many equal
    distances), with some rows duplicated."""
    kind = rng.integers(0, 3, n)[:, None]
    out = np.where(kind == 0, rng.integers(0, 256, (n, dim)),
                   np.where(kind == 1, 255 * rng.integers(0, 2, (n, dim)), rng.integers(0, 3, (n, dim))))
    if n >= 8:
        out[rng.integers(0, n, n // 8)] = out[rng.integers(0, n, n // 8)]
    return out.astype(np.uint8)


def make_sets(hip, metric, arrays):
    return [hip.DescriptorSet(metric, a) for a in arrays]


def close(*groups):
    for g in groups:
        for s in (g if isinstance(g, (list, tuple)) else [g]):
            s.close()


def stand_in(norm, query, refs):
    return [bfm.neighbours(norm, query, r, k=2, col_best=True) for r in refs]


def mutual_of(idx, cb):
    return (idx[:, 0] >= 0) & (cb[np.maximum(idx[:, 0], 0)] == np.arange(idx.shape[0]))


def assert_bitwise(got, want, mode, what=""):
    """got = native.match output; want = per reference (idx, dist, col_best) of the stand-in."""
    bi, bd, si, sd, mu = got
    for k, (idx, dist, cb) in enumerate(want):
        msg = "%s ref %d mode %d" % (what, k, mode)
        np.testing.assert_array_equal(bi[k], idx[:, 0], err_msg=msg)
        np.testing.assert_array_equal(bd[k].view(np.uint32), dist[:, 0].view(np.uint32), err_msg=msg)
        if mode == 0:
            np.testing.assert_array_equal(si[k], idx[:, 1], err_msg=msg)
            np.testing.assert_array_equal(sd[k].view(np.uint32), dist[:, 1].view(np.uint32), err_msg=msg)
        if mode == 2:
            np.testing.assert_array_equal(mu[k], mutual_of(idx, cb), err_msg=msg)
        else:
            assert not mu[k].any(), msg


def match_all_modes(hip, metric, query, refs, want, what=""):
    norm = bfm.NORM_L2 if metric == hip.MATCH_L2 else bfm.NORM_HAMMING
    if want is None:
        want = stand_in(norm, query, refs)
    qs = hip.DescriptorSet(metric, query)
    rs = make_sets(hip, metric, refs)
    try:
        out = {}
        for mode in MODES:
            out[mode] = hip.match(qs, rs, mode)
            assert_bitwise(out[mode], want, mode, what)
        return out, want
    finally:
        close(rs, qs)


# ---- (a) exact L2 on the MFMA kernel ------------------------------------------------------------------------------
EXACT_DIMS = (1, 2, 31, 32, 33, 64, 127, 128, 129, 160, 255, 256)


@pytest.mark.parametrize("dtype", ("u8", "f32"))
@pytest.mark.parametrize("dim", EXACT_DIMS)
def test_exact_l2_dims(hip, dim, dtype):
    i = EXACT_DIMS.index(dim)
    rng = np.random.default_rng(1000 + dim + (dtype == "f32"))
    refs = [int_rows(rng, NT[(i + j) % len(NT)], dim) for j in (0, 3, 6)]
    q = int_rows(rng, NQ[i % len(NQ)], dim)
    m = min(q.shape[0], refs[1].shape[0], 3)
    q[:m] = refs[1][:m]                          # d = 0, twice when refs[1] has a duplicate
    if dtype == "f32":
        q, refs = q.astype(np.float32), [r.astype(np.float32) for r in refs]
    with hip.DescriptorSet(hip.MATCH_L2, q) as qs:
        assert qs.exact
    match_all_modes(hip, hip.MATCH_L2, q, refs, None, "dim %d %s" % (dim, dtype))


@pytest.mark.parametrize("nq", NQ)
@pytest.mark.parametrize("dim", (64, 200))
def test_exact_l2_size_sweep(hip, dim, nq):
    rng = np.random.default_rng(2000 + dim + nq)
    refs = [int_rows(rng, nt, dim) for nt in NT]
    refs[6][1024] = refs[6][1000]                # a duplicate across the chunk border, the higher index in chunk 1
    q = int_rows(rng, nq, dim)
    q[0] = refs[6][1000]
    match_all_modes(hip, hip.MATCH_L2, q, refs, None, "dim %d nq %d" % (dim, nq))


# ---- (b) the exactness bound of the bf16 MFMA: every dot product below 2^24 -------------------------------------
@pytest.mark.parametrize("dim", (128, 256))
def test_exact_l2_dot_product_bound(hip, dim):
    # all-255 rows have a . b = dim * 255^2 (8 323 200 at dim 128, 16 646 400 at 256, just under 2^24 = 16 777 216);
    # near-255 rows keep the dot products there while s is small, so a lost low bit of a . b changes d
    rng = np.random.default_rng(3000 + dim)
    full = np.full(dim, 255, dtype=np.int64)
    rows = [full, np.zeros(dim, dtype=np.int64)]
    for k in (1, 2, 7, dim // 2, dim - 1, dim):
        for off in (0, dim - k):
            r = full.copy()
            r[off:off + k] -= 1                      # 255 - 1 in k elements: s = k against all-255
            rows.append(r)
    rows += [255 - rng.integers(0, 4, dim) for _ in range(6)] + [255 - rng.integers(0, 2, dim) for _ in range(6)]
    rows = np.array(rows).astype(np.uint8)
    # one single-row reference per row: best_dist is then the whole distance matrix; plus all rows in one reference
    refs = [rows[j:j + 1] for j in range(rows.shape[0])] + [rows]
    out, _ = match_all_modes(hip, hip.MATCH_L2, rows, refs, None, "bound dim %d" % dim)
    bd = out[0][1]
    assert bd[0, 0] == 0.0                                                   # all-255 vs all-255: s = 0
    assert bd[0, 1] == bfm.sqrt_rn_f32(np.array([dim * 255 * 255]))[0]      # all-0 vs all-255: the canon_s branch
    for j in range(2, 14):
        k = int((rows[j] == 254).sum())
        assert bd[0, j] == bfm.sqrt_rn_f32(np.array([k]))[0] == bd[j, 0], (j, k)      # s = k: any error in a . b shows
    # many pairs of near-255 rows across tiles and a chunk border: s is small, the dot products are near 2^24
    q = (255 - rng.integers(0, 3, (300, dim))).astype(np.uint8)
    t = (255 - rng.integers(0, 3, (1100, dim))).astype(np.uint8)
    t[1030] = q[5]; t[1050] = q[5]
    match_all_modes(hip, hip.MATCH_L2, q, [t], None, "near-255 dim %d" % dim)


# ---- (c) canonical ties: distinct s >= 2^22 with the same float32 distance ---------------------------------------
def collision_pairs(lo, hi):
    """Pairs (s, s + 1) in [lo, hi) whose float32 square roots are equal.  Below 2^24 no three integers share one
    distance (the spacing of s between adjacent float distances is 2 d ulp(d) < 2), so a group is a pair."""
    s = np.arange(lo, hi, dtype=np.int64)
    d = bfm.sqrt_rn_f32(s)
    k = np.flatnonzero(d[1:] == d[:-1])
    assert k.size and not (d[k[k + 2 < s.size] + 2] == d[k[k + 2 < s.size]]).any()
    return s[k]


def displaced(row, s, cols):
    """`row` (0/255 values) with elements of `cols` moved toward the other end of [0, 255] by v, sum of v^2 = s."""
    t = row.astype(np.int64).copy()
    for c in cols:
        if s == 0:
            break
        v = min(255, math.isqrt(s))
        t[c] = v if row[c] == 0 else 255 - v
        s -= v * v
    assert s == 0
    return t


def tagged_rows(rng, n, dim, move):
    """n rows of 0/255 that agree on the `move` leading elements and differ pairwise in the tail: a row displaced
    inside the leading elements by s stays >= 255^2 + s away from every other row."""
    common = 255 * rng.integers(0, 2, move)
    tail = 255 * rng.integers(0, 2, (n, dim - move))
    assert np.unique(tail, axis=0).shape[0] == n
    return np.hstack((np.broadcast_to(common, (n, move)), tail)).astype(np.int64)


BAND = 60000                                # < 255^2: a displaced row's own group stays closest
TIE_CASES = [(128, 5_000_000, 90), (256, 5_000_000, 90), (256, 12_000_000, 200)]


@pytest.mark.parametrize("dim,lo,move", TIE_CASES)
def test_canonical_ties_row_side(hip, dim, lo, move):
    rng = np.random.default_rng(4000 + dim + lo // 1000)
    nq, n_fill = 300, 800
    pairs = collision_pairs(lo, lo + BAND)
    q = tagged_rows(rng, nq, dim, move)
    rows, s_of = [None] * (2 * nq + n_fill), {}
    pos = rng.permutation(2 * nq + n_fill)
    # groups on a chunk border, on both sides of it, and inside one 16-column tile
    for g, (a, b) in enumerate(((1023, 1024), (1022, 1025), (32, 33), (1040, 100))):
        ia = int(np.flatnonzero(pos == a)[0])
        pos[[2 * g, ia]] = pos[[ia, 2 * g]]
        ib = int(np.flatnonzero(pos == b)[0])
        pos[[2 * g + 1, ib]] = pos[[ib, 2 * g + 1]]
    cols = np.arange(move)
    for g in range(nq):
        s = int(pairs[rng.integers(0, pairs.size)])
        lo_pos, hi_pos = sorted((int(pos[2 * g]), int(pos[2 * g + 1])))
        big_first = g % 2 == 0                   # half the groups: the larger s at the lower index
        s_of[lo_pos], s_of[hi_pos] = (s + 1, s) if big_first else (s, s + 1)
        for p in (lo_pos, hi_pos):
            rows[p] = displaced(q[g], s_of[p], rng.permutation(cols))
    for p in pos[2 * nq:]:
        r = q[int(rng.integers(0, nq))].copy()
        r[:move] = 255 - r[:move]                # s >= move * 255^2 from every query
        rows[int(p)] = r
    t = np.array(rows).astype(np.uint8)
    q = q.astype(np.uint8)
    want = stand_in(bfm.NORM_L2, q, [t])
    idx, dist, _ = want[0]
    # the data does what it is meant to: each query's two nearest are its own pair, tied, the lower index first
    grp = np.sort(pos[: 2 * nq].reshape(nq, 2), axis=1)
    np.testing.assert_array_equal(idx, grp)
    assert (dist[:, 0] == dist[:, 1]).all() and (dist[:, 0] >= 2048).all()
    assert [s_of[int(p)] > s_of[int(r)] for p, r in grp[:4]] == [True, False, True, False]
    match_all_modes(hip, hip.MATCH_L2, q, [t], want, "row ties dim %d" % dim)


@pytest.mark.parametrize("dim,lo,move", TIE_CASES)
def test_canonical_ties_column_best(hip, dim, lo, move):
    # one train row per group, three queries: two whose s collide, one a pair further; the column-best (and so the
    # mutual flag) must go to the lower query index of the tied two, whichever has the larger s
    rng = np.random.default_rng(5000 + dim + lo // 1000)
    ng, n_fill = 100, 1000
    pairs = collision_pairs(lo, lo + BAND // 2)
    tr = tagged_rows(rng, ng + n_fill, dim, move)     # rows past ng: fillers, >= s + 255^2 from every query
    qpos = rng.permutation(3 * ng)
    qrows = [None] * (3 * ng)
    cols = np.arange(move)
    lower_big = []
    for g in range(ng):
        s = int(pairs[rng.integers(0, pairs.size)])
        a, b, c = (int(x) for x in qpos[3 * g: 3 * g + 3])
        lo_q, hi_q = min(a, b), max(a, b)
        big_first = g % 2 == 0
        qrows[lo_q] = displaced(tr[g], s + 1 if big_first else s, rng.permutation(cols))
        qrows[hi_q] = displaced(tr[g], s if big_first else s + 1, rng.permutation(cols))
        qrows[c] = displaced(tr[g], s + BAND // 2 + 7, rng.permutation(cols))
        lower_big.append(big_first)
    perm = rng.permutation(tr.shape[0])
    t = tr[perm].astype(np.uint8)
    q = np.array(qrows).astype(np.uint8)
    want = stand_in(bfm.NORM_L2, q, [t])
    idx, dist, cb = want[0]
    where = np.argsort(perm)                       # new position of train row g
    for g in range(ng):
        a, b = sorted(int(x) for x in qpos[3 * g: 3 * g + 2])
        assert idx[a, 0] == idx[b, 0] == where[g] and dist[a, 0] == dist[b, 0]
        assert cb[where[g]] == a
    match_all_modes(hip, hip.MATCH_L2, q, [t], want, "column ties dim %d" % dim)


# ---- (d) Hamming, all three MAXW ------------------------------------------------------------------------------------
HAMMING_WIDTHS = (1, 3, 4, 5, 31, 32, 33, 61, 64, 65, 128, 255, 256)


def byte_rows(rng, n, width):
    kind = rng.integers(0, 2, n)[:, None]
    out = np.where(kind == 0, rng.integers(0, 256, (n, width)), rng.choice(np.array([0, 1, 255]), (n, width)))
    if n >= 8:
        out[rng.integers(0, n, n // 8)] = out[rng.integers(0, n, n // 8)]
    return out.astype(np.uint8)


@pytest.mark.parametrize("width", HAMMING_WIDTHS)
def test_hamming_widths(hip, width):
    rng = np.random.default_rng(6000 + width)
    big = byte_rows(rng, 1025, width)
    big[1024] = big[3]; big[100:110] = big[50]
    ones = np.full((3, width), 0xFF, dtype=np.uint8)
    refs = [big, ones, byte_rows(rng, 17, width), byte_rows(rng, 1, width)]
    q = byte_rows(rng, 300, width)
    q[0] = 0
    q[1] = big[3]; q[2] = big[50]
    out, _ = match_all_modes(hip, hip.MATCH_HAMMING, q, refs, None, "width %d" % width)
    bi, bd, si, sd, _ = out[0]
    assert bd[1, 0] == sd[1, 0] == 8 * width and bi[1, 0] == 0 and si[1, 0] == 1      # all-0x00 vs all-0xFF
    assert bd[0, 1] == sd[0, 1] == 0


@pytest.mark.parametrize("nq", (1, 129, 257))
@pytest.mark.parametrize("width", (16, 61, 130))
def test_hamming_size_sweep(hip, width, nq):
    rng = np.random.default_rng(7000 + width + nq)
    refs = [byte_rows(rng, nt, width) for nt in NT]
    refs[7][2048] = refs[7][1024]
    q = byte_rows(rng, nq, width)
    q[0] = refs[7][1024]
    match_all_modes(hip, hip.MATCH_HAMMING, q, refs, None, "width %d nq %d" % (width, nq))


# ---- (e) general float L2, all three MAXW ---------------------------------------------------------------------------
FLOAT_DIMS = (1, 2, 31, 32, 33, 64, 127, 128, 129, 200, 256)


def dyadic_numerators(rng, n, dim):
    kind = rng.integers(0, 2, n)[:, None]
    k = np.where(kind == 0, rng.integers(-127, 128, (n, dim)), rng.integers(-2, 3, (n, dim)))
    if n >= 8:
        k[rng.integers(0, n, n // 8)] = k[rng.integers(0, n, n // 8)]
    k[0, 0] = 1                                   # 1/8: the set is not integer-valued
    return k.astype(np.int64)


@pytest.mark.parametrize("dim", FLOAT_DIMS)
def test_float_dyadic(hip, dim):
    # values k/8, |k| <= 127: a - b = m/8 with |m| <= 254 and (a - b)^2 = m^2/64 are exact in fp32, and so is the
    # running sum, S = sum m^2 <= 256 * 254^2 < 2^24.  The kernel's distance is then sqrt_rn_f32(S) / 8 exactly, in
    # any summation order; the stand-in's integer branch on the numerators k computes sqrt_rn_f32(S) from an exact S.
    i = FLOAT_DIMS.index(dim)
    rng = np.random.default_rng(8000 + dim)
    kq = dyadic_numerators(rng, NQ[i % len(NQ)], dim)
    kr = [dyadic_numerators(rng, n, dim) for n in (1, 1025, 300)]
    kr[1][1024] = kr[1][7]
    if kq.shape[0] > 1:
        kq[-1] = kr[1][7]
    want = [(idx, (dist / np.float32(8)).astype(np.float32), cb) for idx, dist, cb in stand_in(bfm.NORM_L2, kq, kr)]
    q, refs = (kq / 8).astype(np.float32), [(k / 8).astype(np.float32) for k in kr]
    with hip.DescriptorSet(hip.MATCH_L2, q) as qs:
        assert not qs.exact
    match_all_modes(hip, hip.MATCH_L2, q, refs, want, "dyadic dim %d" % dim)


def f64_distances(q, t):
    q, t = q.astype(np.float64), t.astype(np.float64)
    out = np.empty((q.shape[0], t.shape[0]))
    for i in range(0, q.shape[0], 32):
        out[i:i + 32] = np.sqrt(((q[i:i + 32, None, :] - t[None]) ** 2).sum(-1))
    return out


def assert_within_bound(got, q, refs, mode, dim):
    """Float L2 against float64.  The kernel computes e_i = fl(a_i - b_i) = (a_i - b_i)(1 + d_i), |d_i| <= u, then
    S^ = fma chain of e_i^2: one rounding per term, S^ = sum e_i^2 (1 + t), |t| <= gamma_dim = dim u / (1 - dim u),
    so S^ = S (1 + h) with |h| <= (1 + gamma_dim)(1 + u)^2 - 1; d^ = sqrt(S^)(1 + r), |r| <= u.  Hence
    |d^ - d| <= ((dim + 2) u / 2 + u + O(u^2)) d <= eps d with eps = (dim + 4) u.  The float64 reference adds
    under 2^-44 relative.  A returned index j then has d_j (1 - eps) <= d^_j <= d^_best <= d_best (1 + eps)."""
    eps = (dim + 4) * U + 2.0 ** -44
    widen = (1 + eps) / (1 - eps)
    bi, bd, si, sd, mu = got
    for k, t in enumerate(refs):
        d = f64_distances(q, t)
        srt = np.sort(d, axis=1)
        rows = np.arange(q.shape[0])
        d1 = srt[:, 0]
        assert (np.abs(bd[k] - d1) <= eps * d1).all()
        assert (d[rows, bi[k]] <= d1 * widen).all()
        clear1 = srt[:, 1] > d1 * widen if t.shape[0] > 1 else np.ones(q.shape[0], dtype=bool)
        np.testing.assert_array_equal(bi[k][clear1], d.argmin(1)[clear1])
        if mode == 0 and t.shape[0] > 1:
            d2 = srt[:, 1]
            assert (np.abs(sd[k] - d2) <= eps * d2).all()
            assert (si[k] != bi[k]).all()
            assert (d[rows, si[k]] <= d2 * widen).all() and (d[rows, si[k]] >= d2 / widen).all()
            if t.shape[0] > 2:
                clear2 = clear1 & (srt[:, 2] > d2 * widen)
                np.testing.assert_array_equal(si[k][clear2], np.argsort(d, axis=1)[clear2, 1])
        if mode == 0 and t.shape[0] == 1:
            assert (si[k] == -1).all() and np.isinf(sd[k]).all()
        if mode == 2:
            csrt = np.sort(d, axis=0)
            col_clear = csrt[1] > csrt[0] * widen if q.shape[0] > 1 else np.ones(t.shape[0], dtype=bool)
            ok = clear1 & col_clear[bi[k]]
            want = d.argmin(0)[bi[k]] == rows
            assert ok.sum() > 0.5 * q.shape[0]
            np.testing.assert_array_equal(mu[k][ok], want[ok])
        else:
            assert not mu[k].any()


@pytest.mark.parametrize("dim", (1, 31, 32, 33, 128, 129, 256))
def test_float_normal_bound(hip, dim):
    rng = np.random.default_rng(9000 + dim)
    q = rng.normal(size=(300, dim)).astype(np.float32)
    refs = [rng.normal(size=(n, dim)).astype(np.float32) for n in (1100, 1)]
    qs = hip.DescriptorSet(hip.MATCH_L2, q)
    rs = make_sets(hip, hip.MATCH_L2, refs)
    try:
        for mode in MODES:
            assert_within_bound(hip.match(qs, rs, mode), q, refs, mode, dim)
    finally:
        close(rs, qs)


# ---- (f) an exact query with exact and non-exact references: the float kernel on bf16 -> f32 images --------------
@pytest.mark.parametrize("dim", (64, 128, 200))
def test_mixed_kind_launch(hip, dim):
    rng = np.random.default_rng(10000 + dim)
    q = int_rows(rng, 257, dim)
    a = int_rows(rng, 1030, dim)
    a[1025] = q[9]; a[3] = q[9]
    b = (rng.integers(0, 255, (300, dim)) + rng.random((300, dim))).astype(np.float32)
    c = int_rows(rng, 40, dim).astype(np.float32)
    qs = hip.DescriptorSet(hip.MATCH_L2, q)
    sa, sb, sc = make_sets(hip, hip.MATCH_L2, (a, b, c))
    try:
        assert qs.exact and sa.exact and sc.exact and not sb.exact
        want = stand_in(bfm.NORM_L2, q, [a, c])
        first = {}
        for mode in MODES:
            got = hip.match(qs, [sa, sb, sc], mode)
            first[mode] = got
            # integer references: s < 2^24 is exact in the fp32 sum, so the float kernel agrees bit for bit
            assert_bitwise([x[[0, 2]] for x in got], want, mode, "mixed dim %d" % dim)
            assert_within_bound([x[1:2] for x in got], q, [b], mode, dim)
        for mode in MODES:                       # the same resident sets, all exact: the MFMA kernel again
            assert_bitwise(hip.match(qs, [sa, sc], mode), want, mode, "exact again dim %d" % dim)
        for mode in MODES:
            again = hip.match(qs, [sa, sb, sc], mode)
            for x, y in zip(first[mode], again):
                assert x.tobytes() == y.tobytes()
    finally:
        close([sa, sb, sc], qs)


# ---- (g) many references in one launch --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ("l2", "hamming"))
def test_many_references_one_launch(hip, metric):
    rng = np.random.default_rng(11000 + (metric == "hamming"))
    sizes = [1, 2, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 2048, 2049, 2100]
    sizes += [int(x) for x in rng.integers(1, 2101, 40 - len(sizes))]
    if metric == "l2":
        m, refs, q = hip.MATCH_L2, [int_rows(rng, n, 128) for n in sizes], int_rows(rng, 300, 128)
    else:
        m, refs, q = hip.MATCH_HAMMING, [byte_rows(rng, n, 64) for n in sizes], byte_rows(rng, 300, 64)
    q[:5] = refs[12][2044:2049]
    out, _ = match_all_modes(hip, m, q, refs, None, "many refs %s" % metric)
    bi, bd, si, sd, _ = out[0]
    assert (si[0] == -1).all() and np.isinf(sd[0]).all() and (bi[0] == 0).all()


# ---- (h) sfm_match_dev on the caller's stream, device outputs, NULL outputs ----------------------------------------
SENTINEL = (np.int32(-7), np.uint32(0x7FC0DEAD).view(np.float32), np.int32(-9), np.uint32(0x7FC0BEEF).view(np.float32),
            np.uint8(0xFF))


def sentinel_outputs(torch, shape):
    outs = []
    for v in SENTINEL:
        a = np.full(shape, v, dtype=v.dtype)
        outs.append(torch.from_numpy(a).cuda())
    return outs


def test_match_dev_on_torch_stream(hip):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(12000)
    q = int_rows(rng, 300, 128)
    refs = [int_rows(rng, n, 128) for n in (1, 1025, 200)]
    qs = hip.DescriptorSet(hip.MATCH_L2, q)
    rs = make_sets(hip, hip.MATCH_L2, refs)
    shape = (len(refs), q.shape[0])
    try:
        for mode in MODES:
            want = hip.match(qs, rs, mode)
            want = [w.astype(np.uint8) if w.dtype == bool else w for w in want]
            for mask in ((1, 1, 1, 1, 1), (1, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 0, 1, 0, 1), (1, 1, 1, 1, 0), (0, 0, 0, 0, 1),
                         (0, 0, 0, 0, 0)):
                outs = sentinel_outputs(torch, shape)
                ptrs = [o.data_ptr() if use else 0 for o, use in zip(outs, mask)]
                hip.match_dev(qs, rs, mode, *ptrs, stream=stream)
                torch.cuda.synchronize()
                for k, (o, use, w) in enumerate(zip(outs, mask, want)):
                    got = o.cpu().numpy()
                    if use:
                        assert got.tobytes() == w.tobytes(), (mode, mask, k)
                        if k == 4 and mode != 2:
                            assert not got.any()          # the 0xFF fill is cleared outside MUTUAL
                    else:
                        assert (got.view(np.uint8) == np.full(shape, SENTINEL[k], dtype=SENTINEL[k].dtype).view(np.uint8)).all()
    finally:
        close(rs, qs)


def test_match_dev_empty_query(hip):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(12001)
    q0 = hip.DescriptorSet(hip.MATCH_L2, np.zeros((0, 128), dtype=np.uint8))
    rs = make_sets(hip, hip.MATCH_L2, [int_rows(rng, 5, 128), int_rows(rng, 1500, 128)])
    try:
        for mode in MODES:
            outs = sentinel_outputs(torch, (2, 16))
            hip.match_dev(q0, rs, mode, *[o.data_ptr() for o in outs], stream=stream)
            torch.cuda.synchronize()
            for k, o in enumerate(outs):
                assert (o.cpu().numpy().view(np.uint8) == np.full((2, 16), SENTINEL[k], dtype=SENTINEL[k].dtype).view(np.uint8)).all()
            bi, bd, si, sd, mu = hip.match(q0, rs, mode)
            assert bi.shape == (2, 0) and mu.shape == (2, 0)
    finally:
        close(rs, q0)


# ---- (i) creation and limits ----------------------------------------------------------------------------------------
def test_exact_flag_and_limits(hip):
    base = np.tile(np.arange(8, dtype=np.float32) * 30, (3, 1))
    for v, exact in ((-0.0, True), (0.0, True), (255.0, True), (255.5, False), (256.0, False), (-1.0, False), (1e-30, False)):
        rows = base.copy()
        rows[1, 3] = v
        with hip.DescriptorSet(hip.MATCH_L2, rows) as s:
            assert s.exact == exact, v
    for bad in (np.zeros((2, 257), dtype=np.uint8), np.zeros((2, 257), dtype=np.float32)):
        with pytest.raises(ValueError):
            hip.DescriptorSet(hip.MATCH_L2, bad)
    with pytest.raises(ValueError):
        hip.DescriptorSet(hip.MATCH_HAMMING, np.zeros((2, 257), dtype=np.uint8))
    for s in (hip.DescriptorSet(hip.MATCH_L2, np.zeros((2, 256), dtype=np.uint8)),
              hip.DescriptorSet(hip.MATCH_L2, np.zeros((2, 256), dtype=np.float32)),
              hip.DescriptorSet(hip.MATCH_HAMMING, np.zeros((2, 256), dtype=np.uint8))):
        s.close()


@pytest.mark.parametrize("dim", (64, 200))
def test_negative_zero_rows_match_bitwise(hip, dim):
    rng = np.random.default_rng(13000 + dim)
    q = int_rows(rng, 200, dim).astype(np.float32)
    t = int_rows(rng, 1100, dim).astype(np.float32)
    q[q == 0] = -0.0
    t[: 550][t[: 550] == 0] = -0.0
    assert np.signbit(q).any() and np.signbit(t).any()
    with hip.DescriptorSet(hip.MATCH_L2, q) as qs, hip.DescriptorSet(hip.MATCH_L2, t) as ts:
        assert qs.exact and ts.exact
    match_all_modes(hip, hip.MATCH_L2, q, [t], None, "-0.0 dim %d" % dim)
