"""The view-pair selection on the device against tests/_retrieve_reference.py: every output EXACTLY (scores as bits), at the
smallest shapes at which each kernel can go wrong, under compute-unit limits of none, 1 and 32, and from run to run.  The
references are computed once per case and shared."""
import ctypes
import functools

import numpy as np
import pytest

import _retrieve_reference as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1, 32], ids=["cus_all", "cus_1", "cus_32"])
def limit(hip, request):
    hip.set_cu_limit(request.param)
    yield request.param
    hip.set_cu_limit(0)


class _Sets:
    """DescriptorSets of a list of uint8 arrays, closed on exit."""

    def __init__(self, hip, views):
        self.hip, self.views = hip, views

    def __enter__(self):
        self.sets = [self.hip.DescriptorSet(self.hip.MATCH_L2, v) for v in self.views]
        return self.sets

    def __exit__(self, *exc):
        for s in self.sets:
            s.close()


def _rows(seed, n, D, n_pool=40, spread=20):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (n_pool, D))
    return np.clip(pool[rng.integers(0, n_pool, n)] + rng.integers(-spread, spread + 1, (n, D)), 0, 255).astype(np.uint8)


# ---- training ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train_case(name):
    """(views, K, iters, seed, train_cap)"""
    if name.startswith("own_word_"):                          # T = K: every row is its own word
        return [np.unique(_rows(1, 40, 8), axis=0)[:17]], 17, int(name[9:]), 3, 0
    if name.startswith("duplicates_"):                        # 3 distinct rows ten times: words without a row keep their bytes
        return [np.tile(_rows(2, 3, 8), (10, 1))], 8, int(name[11:]), 1, 0
    if name == "half":                                        # both means fall on exactly .5
        return [np.array([[0, 10, 0, 0, 0, 0, 0, 0], [1, 11, 0, 0, 0, 0, 0, 0]], dtype=np.uint8),
                np.array([[1, 200, 0, 0, 0, 0, 0, 0], [2, 201, 0, 0, 0, 0, 0, 0]], dtype=np.uint8)], 2, 1, 0, 0
    if name == "capped":                                      # N > train_cap: 1 000 of 2 500 rows, three sets, one empty
        x = _rows(3, 2500, 8)
        return [x[:1000], x[:0], x[1000:]], 15, 4, 5, 1000
    if name == "K_global":                                    # (K D + K) * 4 bytes pass 64 KiB: the global-atomic route
        return [_rows(6, 1100, 128, n_pool=300)], 1024, 1, 2, 0
    if name.startswith("K_"):
        K = int(name[2:])
        return [_rows(4, 900, 8), _rows(5, 600, 8)], K, 1 if K == 1024 else 4, 7, 0
    if name.startswith("far_"):                               # all-255 rows against an all-0 word or the reverse: s = 255^2 D
        D = int(name[4:])
        return [np.zeros((40, D), dtype=np.uint8), np.full((41, D), 255, dtype=np.uint8)], 1, 1, 9, 0
    if name.startswith("seed_"):
        return [_rows(4, 900, 8), _rows(5, 600, 8)], 15, 2, int(name[5:]), 0
    if name == "wide":                                        # D = 256, not a multiple-of-tile row count
        return [_rows(8, 333, 256)], 17, 2, 1, 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _train_ref(name):
    views, K, iters, seed, cap = _train_case(name)
    return rr.train(np.concatenate(views), K, iters, seed, cap)


TRAIN = (["own_word_0", "own_word_1", "own_word_4", "duplicates_1", "duplicates_4", "half", "capped"]
         + ["K_%d" % K for K in (1, 2, 15, 16, 17, 64, 1024)] + ["K_global", "far_8", "far_128", "far_256", "seed_0", "seed_%d" % 2 ** 63, "wide"])


@pytest.mark.parametrize("name", TRAIN)
def test_training_equals_the_reference(hip, limit, name):
    views, K, iters, seed, cap = _train_case(name)
    want_words, want_log = _train_ref(name)
    with _Sets(hip, views) as sets:
        words, log = hip.vocab_train(sets, K, iters, seed, cap)
        assert np.array_equal(words, want_words) and np.array_equal(log, want_log), (log, want_log)
        if limit == 0:                                        # run to run
            again = hip.vocab_train(sets, K, iters, seed, cap)
            assert np.array_equal(again[0], words) and np.array_equal(again[1], log)
    x = np.concatenate(views)
    assert np.array_equal(hip.vocab_init_rows(x.shape[0], K, seed, cap), rr.init_rows(x.shape[0], K, seed, cap))


def test_the_training_cases_reach_what_they_are_there_for():
    w, log = _train_ref("own_word_4")
    assert np.all(log == 0) and np.array_equal(np.sort(w, axis=0), np.sort(_train_case("own_word_4")[0][0], axis=0))
    w, log = _train_ref("duplicates_1")
    x = _train_case("duplicates_1")[0][0]
    start = x[rr.init_rows(30, 8, 1)]
    distinct = np.unique(start, axis=0).shape[0]                            # 8 words on 3 distinct rows: ties go to the lower word
    later = [i for i in range(8) if any(np.array_equal(start[i], start[j]) for j in range(i))]
    assert distinct < 8 and log[0, 1] == 8 - distinct == len(later) and not np.isin(rr.assign(x, start)[0], later).any()
    assert np.array_equal(w[later], start[later]) and log[0, 2] >= 1        # the words without a row keep their bytes, another one moves
    assert _train_ref("half")[0].tolist() == [[1, 11, 0, 0, 0, 0, 0, 0], [2, 201, 0, 0, 0, 0, 0, 0]]
    for D in (8, 128, 256):
        assert _train_ref("far_%d" % D)[1][0, 0] in (40 * 255 * 255 * D, 41 * 255 * 255 * D)
    assert 255 * 255 * 256 < 2 ** 24
    assert (1024 * 128 + 1024) * 4 > 64 * 1024 >= (1024 * 8 + 1024) * 4     # the two accumulation routes
    assert _train_ref("capped")[1][0, 0] > 0 and not np.array_equal(_train_ref("seed_0")[0], _train_ref("seed_%d" % 2 ** 63)[0])


# ---- describing ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _describe_case(name):
    """(words, views)"""
    if name == "sizes":                                       # 0, 1, 127, 128, 129 and 1 025 rows in one call
        views = [_rows(10 + i, n, 128, n_pool=30) for i, n in enumerate((0, 1, 127, 128, 129, 1025))]
        return rr.train(np.concatenate(views), 16, 2, 1)[0], views
    if name == "one_word":                                    # every row of the view in one word: one accumulator per dimension
        return _rows(20, 1, 128), [_rows(21, 1025, 128)]
    if name == "one_of_five":
        words = np.array([[0] * 8, [60] * 8, [120] * 8, [180] * 8, [250] * 8], dtype=np.uint8)
        return words, [np.clip(180 + np.random.default_rng(3).integers(-9, 10, (700, 8)), 0, 255).astype(np.uint8)]
    if name == "clamp":                                       # 70 rows 255 away: |r| = 17 850, isqrt = 133, q = +-127
        return np.zeros((1, 8), dtype=np.uint8), [np.full((70, 8), 255, dtype=np.uint8), np.full((69, 8), 255, dtype=np.uint8)]
    if name == "clamp_negative":
        return np.full((1, 8), 255, dtype=np.uint8), [np.zeros((70, 8), dtype=np.uint8)]
    if name == "signs":                                       # r of both signs and r = 0 (rows 90 and 110 around 100), ties between words
        words = np.array([[100] * 8, [100] * 8, [30] * 8], dtype=np.uint8)
        return words, [np.array([[90] * 8, [110] * 8, [101, 99, 100, 100, 140, 60, 100, 100], [29] * 8], dtype=np.uint8)]
    if name.startswith("far_"):
        D = int(name[4:])
        return np.zeros((1, D), dtype=np.uint8), [np.full((3, D), 255, dtype=np.uint8)]
    if name == "wide":
        views = [_rows(30 + i, n, 256) for i, n in enumerate((200, 77))]
        return rr.train(np.concatenate(views), 20, 1, 1)[0], views
    if name == "global_route":                                # K D = 131 072: the limit, and the global-atomic route
        views = [_rows(40, 300, 128, n_pool=100), _rows(41, 150, 128, n_pool=100)]
        return _rows(42, 1024, 128, n_pool=1024, spread=0), views
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _describe_ref(name):
    words, views = _describe_case(name)
    return rr.describe(words, views)


DESCRIBE = ["sizes", "one_word", "one_of_five", "clamp", "clamp_negative", "signs", "far_8", "far_128", "far_256", "wide", "global_route"]


@pytest.mark.parametrize("name", DESCRIBE)
def test_describing_equals_the_reference(hip, limit, name):
    words, views = _describe_case(name)
    want = _describe_ref(name)
    with _Sets(hip, views + [words]) as sets:
        got = hip.view_describe(sets[-1], sets[:-1])
        for key in hip.DESCRIBE_OUTPUTS:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
        if limit == 0:
            again = hip.view_describe(sets[-1], sets[:-1])
            assert all(np.array_equal(again[key], got[key]) for key in hip.DESCRIBE_OUTPUTS)


def test_the_describing_cases_reach_what_they_are_there_for():
    assert np.all(_describe_ref("clamp")["desc"][0] == 127) and np.all(_describe_ref("clamp")["residual"][0] == 17850)
    assert np.all(_describe_ref("clamp")["desc"][1] == 127) and rr.isqrt(69 * 255) == 132
    assert np.all(_describe_ref("clamp_negative")["desc"] == -127)
    s = _describe_ref("signs")
    assert s["assign"].tolist() == [0, 0, 0, 2] and s["residual"][0, :8].tolist() == [1, -1, 0, 0, 40, -40, 0, 0] and s["word_count"].tolist() == [[3, 0, 1]]
    assert _describe_ref("one_of_five")["word_count"].tolist() == [[0, 0, 0, 700, 0]]
    z = _describe_ref("sizes")
    assert z["norm2"][0] == 0 and not z["desc"][0].any() and z["word_count"].sum(1).tolist() == [0, 1, 127, 128, 129, 1025]
    assert (z["desc"] > 0).any() and (z["desc"] < 0).any() and (z["desc"] == 0).any()


def test_every_optional_output_absent_in_turn_and_the_device_form(hip):
    import torch
    words, views = _describe_case("sizes")
    want = _describe_ref("sizes")
    with _Sets(hip, views + [words]) as sets:
        for absent in hip.DESCRIBE_OUTPUTS:
            got = hip.view_describe(sets[-1], sets[:-1], outputs=tuple(n for n in hip.DESCRIBE_OUTPUTS if n != absent))
            assert got[absent] is None and all(np.array_equal(got[n], want[n]) for n in hip.DESCRIBE_OUTPUTS if n != absent), absent
        for only in hip.DESCRIBE_OUTPUTS:
            assert np.array_equal(hip.view_describe(sets[-1], sets[:-1], outputs=(only,))[only], want[only]), only
        dev = {n: torch.full(want[n].shape, 7, dtype=getattr(torch, str(want[n].dtype)), device="cuda") for n in hip.DESCRIBE_OUTPUTS}
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            hip.view_describe_dev(sets[-1], sets[:-1], *(dev[n].data_ptr() for n in hip.DESCRIBE_OUTPUTS), stream=stream.cuda_stream)
            for n in hip.DESCRIBE_OUTPUTS:
                assert np.array_equal(dev[n].cpu().numpy(), want[n]), n
            only = torch.full(want["norm2"].shape, 7, dtype=torch.int64, device="cuda")
            hip.view_describe_dev(sets[-1], sets[:-1], d_norm2=only.data_ptr(), stream=stream.cuda_stream)
            assert np.array_equal(only.cpu().numpy(), want["norm2"])


def test_the_library_refuses_real_sets_it_cannot_describe(hip):
    rng = np.random.default_rng(1)
    exact, other_dim = rng.integers(0, 256, (40, 16)).astype(np.uint8), rng.integers(0, 256, (40, 32)).astype(np.uint8)
    with hip.DescriptorSet(hip.MATCH_L2, exact) as a, hip.DescriptorSet(hip.MATCH_L2, other_dim) as b, \
            hip.DescriptorSet(hip.MATCH_HAMMING, exact) as ham, hip.DescriptorSet(hip.MATCH_L2, rng.random((40, 16)).astype(np.float32)) as flt:
        assert a.exact and not flt.exact
        for sets, word in (([a, ham], "set 1 is not an exact"), ([flt], "set 0 is not an exact"), ([a, b], "set 1 has dim 32")):
            with pytest.raises(ValueError, match=word):
                hip.vocab_train(sets, 4)
            with pytest.raises(ValueError, match=word.replace("set", "view")):
                hip.view_describe(a, sets)
        with pytest.raises(ValueError, match="T = 40 training rows for K = 41"):
            hip.vocab_train([a], 41)
        lib, words = hip.load(), np.full((64, 16), 7, dtype=np.uint8)             # the library itself, past the Python checks
        for sets, K, word in (([a, ham], 4, "set 1 is not an exact"), ([flt, a], 4, "set 0 is not an exact"), ([a, b], 4, "set 1 has dim 32"),
                              ([a], 41, "T = 40 training rows")):
            assert lib.sfm_vocab_train(len(sets), hip._set_handles(sets), K, 1, ctypes.c_uint64(1), 0, hip._u8ptr(words), None) == hip.E_SHAPE
            assert word in hip.last_error() and np.all(words == 7)
            if K == 4:
                assert lib.sfm_view_describe(a._h, len(sets), hip._set_handles(sets), None, None, None, None, None) == hip.E_SHAPE
                assert word.replace("set", "view") in hip.last_error()
        with pytest.raises(ValueError, match="vocabulary 0 is not an exact"):
            hip.view_describe(ham, [a])


# ---- pairs -------------------------------------------------------------------------------------------------------------------------
def _norms(desc):
    return (desc.astype(np.int64) ** 2).sum(1)


@functools.lru_cache(maxsize=None)
def _pairs_case(name):
    """(desc int8 (V, len), norm2 int64 (V,))"""
    if name.startswith("V_"):                                 # random descriptors; len 40 is padded to 64, len 192 is not
        V, length = (int(x) for x in name[2:].split("_"))
        desc = np.random.default_rng(V).integers(-127, 128, (V, length)).astype(np.int8)
        return desc, _norms(desc)
    if name == "many":                                        # 1 025 views of two keys through K = 1, D = 8
        rng = np.random.default_rng(9)
        d = rr.describe(np.full((1, 8), 128, dtype=np.uint8), [rng.integers(0, 256, (2, 8)).astype(np.uint8) for _ in range(1025)])
        return d["desc"], d["norm2"]
    if name.startswith("bound_"):                             # every entry +-127: |dot| reaches 127^2 len, the int32 bound at 131 072
        length = int(name[6:])
        rng = np.random.default_rng(length)
        desc = np.full((5, length), 127, dtype=np.int8)
        desc[1] = -127
        desc[2, rng.random(length) < 0.5] = -127
        desc[3] = desc[2]
        desc[4, ::3] = -127
        return desc, _norms(desc)
    if name == "asymmetric":                                  # desc[a][j] depends on a and j differently: a swapped lane map shows
        a, j = np.arange(33)[:, None], np.arange(192)[None, :]
        desc = ((a * 7 + j * 13 + a * j * 3 + (j // 16) * a) % 255 - 127).astype(np.int8)
        return desc, _norms(desc)
    if name == "duplicates":                                  # equal views: equal scores, the lower index first
        desc = np.random.default_rng(4).integers(-20, 21, (17, 40)).astype(np.int8)
        desc[5], desc[11], desc[16] = desc[2], desc[2], desc[2]
        return desc, _norms(desc)
    if name == "zero_norm":                                   # views without a norm: nobody's neighbour, listed only as sequential
        desc = np.random.default_rng(5).integers(-50, 51, (16, 64)).astype(np.int8)
        desc[[0, 7, 15]] = 0
        return desc, _norms(desc)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _pairs_ref(name, k, min_score, mutual, sequential):
    desc, norm2 = _pairs_case(name)
    return rr.pairs(desc, norm2, k, min_score, mutual, sequential)


def _assert_pairs(got, want, cap=None):
    n = want["n_pairs"] if cap is None else min(cap, want["n_pairs"])
    assert got["n_pairs"] == want["n_pairs"]
    assert np.array_equal(got["nbr"], want["nbr"]) and np.array_equal(rr.bits(got["nbr_score"]), rr.bits(want["nbr_score"]))
    assert np.array_equal(got["pairs"], want["pairs"][:n]) and np.array_equal(got["how"], want["how"][:n])
    assert np.array_equal(rr.bits(got["pair_score"]), rr.bits(want["pair_score"][:n]))
    if got.get("dot") is not None:
        assert np.array_equal(got["dot"], want["dot"])


NEG = float("-inf")
PAIRS = ([("V_%d_%d" % (V, length), 3, NEG, m, s) for V in (1, 2, 15, 16, 17, 33) for length in (40, 192) for m, s in ((0, 0), (1, 2))]
         + [("V_33_40", 3, NEG, 1, 0), ("V_33_40", 3, NEG, 0, 2), ("V_17_192", 64, NEG, 0, 0), ("V_16_40", 15, NEG, 1, 0), ("V_33_192", 1, 0.02, 0, 0),
            ("many", 4, NEG, 0, 1), ("many", 2, 0.5, 1, 0), ("bound_8", 2, NEG, 0, 0), ("bound_131072", 2, NEG, 0, 1), ("bound_131072", 4, -0.5, 1, 0),
            ("asymmetric", 5, NEG, 0, 0), ("asymmetric", 5, NEG, 1, 3), ("duplicates", 3, NEG, 0, 0), ("duplicates", 16, NEG, 1, 0),
            ("zero_norm", 4, NEG, 0, 0), ("zero_norm", 4, NEG, 1, 2), ("zero_norm", 20, 0.0, 0, 16)])


@pytest.mark.parametrize("name,k,min_score,mutual,sequential", PAIRS)
def test_pairs_equal_the_reference(hip, limit, name, k, min_score, mutual, sequential):
    desc, norm2 = _pairs_case(name)
    want = _pairs_ref(name, k, min_score, mutual, sequential)
    outputs = hip.PAIRS_OUTPUTS if desc.shape[0] <= 33 else hip.PAIRS_OUTPUTS[:5]
    got = hip.view_pairs(desc, norm2, k, min_score, mutual, sequential, outputs=outputs)
    _assert_pairs(got, want)
    if limit == 0:
        again = hip.view_pairs(desc, norm2, k, min_score, mutual, sequential)       # run to run, and without `dot`: the strip route
        _assert_pairs(again, want)


def test_the_pair_cases_reach_what_they_are_there_for():
    b = _pairs_ref("bound_131072", 2, NEG, 0, 1)
    assert abs(int(b["dot"][0, 1])) == 127 * 127 * 131072 < 2 ** 31 and b["nbr_score"][0, 0] < 1.0 and b["nbr"][2, 0] == 3 and b["nbr_score"][2, 0] == 1.0
    d = _pairs_ref("duplicates", 3, NEG, 0, 0)
    assert d["nbr"][2].tolist() == [5, 11, 16] and d["nbr"][16].tolist() == [2, 5, 11] and np.all(d["nbr_score"][2] == 1.0)
    z = _pairs_ref("zero_norm", 4, NEG, 1, 2)
    assert np.all(z["nbr"][[0, 7, 15]] == -1) and not np.isin(z["nbr"], [0, 7, 15]).any()
    assert all(h == 4 and s == NEG for (a, c), h, s in zip(z["pairs"], z["how"], z["pair_score"]) if a in (0, 7, 15) or c in (0, 7, 15))
    assert (z["how"] == 4).any() and (z["how"] == 7).any() and (z["how"] == 3).any()
    pad = _pairs_ref("V_17_192", 64, NEG, 0, 0)
    assert np.all(pad["nbr"][:, 16:] == -1) and np.all(pad["nbr"][:, :16] >= 0) and np.all(np.isneginf(pad["nbr_score"][:, 16:]))
    asym = _pairs_ref("asymmetric", 5, NEG, 0, 0)["dot"]
    assert np.unique(asym[np.triu_indices(33, 1)]).shape[0] > 500              # no two rows or columns alike
    many = _pairs_ref("many", 4, NEG, 0, 1)
    assert many["n_pairs"] > 1024 and ((many["how"] & 4) != 0).sum() == 1024


def test_min_score_one_ulp_either_side_of_an_occurring_score(hip):
    desc, norm2 = _pairs_case("V_17_192")
    base = _pairs_ref("V_17_192", 3, NEG, 0, 0)
    s = float(base["nbr_score"][4, 1])                                          # the second neighbour of view 4
    for thr, kept in ((s, True), (np.nextafter(s, -np.inf), True), (np.nextafter(s, np.inf), False)):
        want = rr.pairs(desc, norm2, 3, thr, 0, 0)
        got = hip.view_pairs(desc, norm2, 3, thr)
        _assert_pairs(got, want)
        assert (got["nbr"][4, 1] == base["nbr"][4, 1]) == kept and (got["nbr"][4, 1] >= 0) == kept


def test_a_cap_below_the_count_leaves_the_rest_untouched(hip):
    desc, norm2 = _pairs_case("V_33_40")
    want = _pairs_ref("V_33_40", 3, NEG, 0, 2)
    lib, n = hip.load(), want["n_pairs"]
    for cap in (0, 1, n - 1, n, n + 5):
        pairs, how, score, count = np.full((n + 5, 2), -7, dtype=np.int32), np.full(n + 5, -7, dtype=np.int32), np.full(n + 5, -7.0), np.zeros(1, dtype=np.int64)
        hip.check(lib.sfm_view_pairs(33, 40, desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), hip._lptr(norm2), 3, NEG, 0, 2, cap, None, None,
                                     hip.iptr(pairs), hip.iptr(how), hip.dptr(score), None, hip._lptr(count)))
        w = min(cap, n)
        assert count[0] == n and np.array_equal(pairs[:w], want["pairs"][:w]) and np.array_equal(how[:w], want["how"][:w])
        assert np.array_equal(rr.bits(score[:w]), rr.bits(want["pair_score"][:w]))
        assert np.all(pairs[w:] == -7) and np.all(how[w:] == -7) and np.all(score[w:] == -7.0)
        got = hip.view_pairs(desc, norm2, 3, NEG, 0, 2, cap=cap)
        _assert_pairs(got, want, cap)
    assert hip.view_pairs(desc, norm2, 3, NEG, 0, 2, outputs=("nbr",))["n_pairs"] == n


def test_a_permutation_of_the_views_permutes_the_result(hip):
    desc, norm2 = _pairs_case("V_33_192")
    base = hip.view_pairs(desc, norm2, 4, -0.05, 0, 0)
    perm = np.random.default_rng(6).permutation(33)                             # new view i is old view perm[i]
    got = hip.view_pairs(desc[perm], norm2[perm], 4, -0.05, 0, 0)
    inv = np.argsort(perm)
    for i in range(33):
        mine, theirs = got["nbr"][i], base["nbr"][perm[i]]
        assert sorted(perm[mine[mine >= 0]].tolist()) == sorted(theirs[theirs >= 0].tolist())
        assert np.array_equal(np.sort(got["nbr_score"][i]), np.sort(base["nbr_score"][perm[i]]))
    mapped = {tuple(sorted((int(inv[a]), int(inv[b])))) for a, b in base["pairs"]}
    assert mapped == set(map(tuple, got["pairs"].tolist())) and got["n_pairs"] == base["n_pairs"]


def test_the_device_form_of_the_pairs(hip):
    import torch
    desc, norm2 = _pairs_case("asymmetric")
    want = _pairs_ref("asymmetric", 5, NEG, 1, 3)
    V, length, n = desc.shape[0], desc.shape[1], want["n_pairs"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_desc, d_norm = torch.from_numpy(desc).cuda(), torch.from_numpy(norm2).cuda()
        nbr = torch.full((V, 5), 7, dtype=torch.int32, device="cuda")
        sc = torch.full((V, 5), 7.0, dtype=torch.float64, device="cuda")
        pairs = torch.full((n + 3, 2), -7, dtype=torch.int32, device="cuda")
        how = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
        ps = torch.full((n + 3,), -7.0, dtype=torch.float64, device="cuda")
        dot = torch.zeros((V, V), dtype=torch.int32, device="cuda")
        count = hip.view_pairs_dev(V, length, d_desc.data_ptr(), d_norm.data_ptr(), 5, NEG, 1, 3, n + 3, nbr.data_ptr(), sc.data_ptr(),
                                   pairs.data_ptr(), how.data_ptr(), ps.data_ptr(), dot.data_ptr(), stream=stream.cuda_stream)
        got = dict(nbr=nbr.cpu().numpy(), nbr_score=sc.cpu().numpy(), pairs=pairs.cpu().numpy()[:n], how=how.cpu().numpy()[:n],
                   pair_score=ps.cpu().numpy()[:n], dot=dot.cpu().numpy(), n_pairs=count)
        _assert_pairs(got, want)
        assert np.all(pairs.cpu().numpy()[n:] == -7) and np.all(ps.cpu().numpy()[n:] == -7.0)
        # an odd byte offset: the library reads from its own aligned copy
        shifted = torch.zeros(V * length + 1, dtype=torch.int8, device="cuda")
        shifted[1:] = d_desc.reshape(-1)
        assert hip.view_pairs_dev(V, length, shifted.data_ptr() + 1, d_norm.data_ptr(), 5, NEG, 1, 3, 0, d_nbr=nbr.data_ptr(),
                                  stream=stream.cuda_stream) == n
        assert np.array_equal(nbr.cpu().numpy(), want["nbr"])


# ---- through the layers ----------------------------------------------------------------------------------------------------------
class _View:
    def __init__(self, sfm, xy, descriptors):
        self.key_pts = [sfm.processors.HipKeyPoint(float(x), float(y)) for x, y in xy]
        self.key_xy = xy
        self.key_descriptors = descriptors


def _planted_views(sfm, seed=3, n_views=7):
    """Views on a line, each seeing a window of 150 to 300 of the landmarks of a pool; a key is a noisy copy of its landmark's
    descriptor at the landmark's projection."""
    rng = np.random.default_rng(seed)
    n_land = 900
    X = np.stack((rng.uniform(-3, 9, n_land), rng.uniform(-2, 2, n_land), rng.uniform(6, 12, n_land)), axis=1)
    X = X[np.argsort(X[:, 0])]                                # the windows slide along x, as the cameras do
    pool = rr._landmark_descriptors(rng, n_land, 128)
    K = np.array([[800.0, 0, 400], [0, 800.0, 300], [0, 0, 1]])
    views = []
    for a in range(n_views):
        first, count = 90 * a, int(rng.integers(150, 301))
        idx = rng.permutation(np.arange(first, min(first + count, n_land)))
        cam = X[idx] - np.array([1.0 * a, 0.0, 0.0])
        xy = (cam[:, :2] / cam[:, 2:3]) * 800.0 + np.array([400.0, 300.0])
        d = np.clip(np.rint(pool[idx] + rng.normal(0.0, 6.0, (idx.shape[0], 128))), 0, 255).astype(np.uint8)
        views.append(_View(sfm, np.ascontiguousarray(xy), d))
    return views, K


def test_through_the_layers(hip, sfm):
    P = sfm.processors
    views, K = _planted_views(sfm)
    assert all(150 <= len(v.key_pts) <= 300 for v in views)
    full = P.HipDeviceKeyTracker("sift", False, True, False, None)
    part = P.HipDeviceKeyTracker("sift", False, True, False, None)
    try:
        for v in range(len(views)):
            full.add_new_view(views[v], views[:v])
        assert part._register_views(views) == len(views) and part._register_views(views) == 0
        pairs, verdict = P.select_pairs(part, K=8, iters=3, seed=2, k=2, sequential=1)
        words, log, d, p = rr.select([v.key_descriptors for v in views], 8, 3, 2, 2, sequential=1)
        assert pairs == [tuple(x) for x in p["pairs"].tolist()] and 6 <= len(pairs) < 21
        assert np.array_equal(verdict["words"], words) and np.array_equal(verdict["log"], log) and np.array_equal(verdict["word_count"], d["word_count"])
        assert np.array_equal(verdict["nbr"], p["nbr"]) and np.array_equal(rr.bits(verdict["nbr_score"]), rr.bits(p["nbr_score"]))
        assert np.array_equal(verdict["how"], p["how"]) and np.array_equal(rr.bits(verdict["pair_score"]), rr.bits(p["pair_score"]))
        again, v2 = P.select_pairs(full, k=2, sequential=1, vocab=words)             # a given vocabulary, another tracker
        assert again == pairs and v2["log"] is None
        assert P.match_pairs(part, views, pairs) == len(pairs)
        listed = set(pairs)
        for ref in range(len(views)):
            got, want = part.track_list[ref].table, full.track_list[ref].table
            assert got.shape == want.shape and got.dtype == want.dtype
            for que in range(len(views)):
                if que == ref:
                    continue
                if (min(ref, que), max(ref, que)) in listed:
                    assert np.array_equal(got[que], want[que]), (ref, que)
                    assert abs(ref - que) > 1 or (got[que] >= 0).sum() > 20, (ref, que)        # neighbours on the line share 60 landmarks or more
                else:
                    assert np.all(got[que] == -1), (ref, que)
        ref, que = pairs[0]
        r_idx, q_idx, inlier = P.verify_pairs(part, ref, que)
        r_full, q_full, inlier_full = P.verify_pairs(full, ref, que)
        assert np.array_equal(r_idx, r_full) and np.array_equal(q_idx, q_full) and np.array_equal(inlier, inlier_full) and inlier.sum() > 20
        with pytest.raises(ValueError, match="pair"):
            P.match_pairs(part, views, [(0, 7)])
        fund = P.HipDeviceKeyTracker("sift", False, True, True, None)
        with pytest.raises(ValueError, match="Q15"):
            P.match_pairs(fund, views, pairs)
    finally:
        full.kt_release()
        part.kt_release()
