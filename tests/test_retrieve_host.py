"""Host-side checks of the view-pair selection (no GPU): the NumPy reference of tests/_retrieve_reference.py against its
brute-force twins, sfm_view_score and sfm_vocab_init_rows against NumPy, every argument the library and the ``check_*``
functions refuse (before a device is looked for, outputs untouched), the exported names, and the quality record on the band
scene."""
import ctypes
import math

import numpy as np
import pytest

import _retrieve_reference as rr


# ---- the reference against brute force -----------------------------------------------------------------------------------------
def _small_views(seed, sizes=(0, 1, 7, 23, 40), D=6, hi=256):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, hi, (9, D))
    return [np.clip(pool[rng.integers(0, 9, n)] + rng.integers(-12, 13, (n, D)), 0, 255).astype(np.uint8) for n in sizes]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_reference_against_brute_force(seed):
    views = _small_views(seed)
    X = np.concatenate(views)
    for K, iters, cap in ((1, 2, 0), (5, 0, 0), (5, 3, 0), (9, 2, 40)):
        w, log = rr.train(X, K, iters, seed, cap)
        wb, logb = rr.train(X, K, iters, seed, cap, brute=True)
        assert np.array_equal(w, wb) and np.array_equal(log, logb) and log[-1, 2] == 0
        assert np.all(np.diff(log[:, 0]) <= 0) or cap                # inertia never rises on the rows it is trained on
    words, _ = rr.train(X, 5, 3, seed)
    d, db = rr.describe(words, views), rr.describe(words, views, brute=True)
    for name in d:
        assert np.array_equal(d[name], db[name]), name
    assert d["norm2"][0] == 0 and not d["desc"][0].any() and d["word_count"].sum(1).tolist() == [v.shape[0] for v in views]
    for k, min_score, mutual, sequential in ((1, -np.inf, 0, 0), (2, -np.inf, 1, 0), (3, 0.1, 0, 2), (8, -np.inf, 0, 1), (2, 0.0, 1, 9)):
        p = rr.pairs(d["desc"], d["norm2"], k, min_score, mutual, sequential)
        pb = rr.pairs(d["desc"], d["norm2"], k, min_score, mutual, sequential, brute=True)
        for name in ("nbr", "how", "pairs", "dot"):
            assert np.array_equal(p[name], pb[name]), (name, k)
        assert np.array_equal(rr.bits(p["nbr_score"]), rr.bits(pb["nbr_score"])) and np.array_equal(rr.bits(p["pair_score"]), rr.bits(pb["pair_score"]))
        assert np.all(p["nbr"][0] == -1) and not np.any(p["nbr"] == 0)       # the empty view is nobody's neighbour
        assert p["pairs"].tolist() == sorted(p["pairs"].tolist())


def test_the_integer_square_root():
    roots = np.array([0, 1, 2, 3, 11, 126, 127, 128, 133, 4095, 32767, 46340], dtype=np.int64)
    v = np.concatenate((roots * roots, roots * roots + 1, np.maximum(roots * roots - 1, 0), [17850, 2 ** 31 - 1]))
    assert rr.isqrt(v).tolist() == [math.isqrt(int(x)) for x in v]
    assert rr.isqrt(17850) == 133                                              # 70 rows 255 away: the clamp case of the GPU test


def test_a_mean_on_one_half_rounds_up():
    X = np.array([[0, 10], [1, 11], [1, 200], [2, 201]], dtype=np.uint8)       # two words: means (0.5, 10.5) and (1.5, 200.5)
    w, log = rr.train(X, 2, 1, 0)
    assert sorted(map(tuple, w.tolist())) == [(1, 11), (2, 201)]


# ---- the host entry points against NumPy ---------------------------------------------------------------------------------------
def test_the_score_against_numpy(sfm):
    native = sfm.native
    rng = np.random.default_rng(5)
    big = 2 ** 31 - 1
    cases = [(1, 1, 1), (-1, 1, 1), (0, 5, 7), (3, 9, 16), (-3, 10, 17), (big, big, big), (-big, big, big - 1), (1, big, big), (127 * 127 * 8, 127 * 127 * 8, 127 * 127 * 8),
             (-(127 * 127 * 131072), 127 * 127 * 131072, 127 * 127 * 131072)]
    cases += [(int(rng.integers(-big, big)), int(rng.integers(1, big)), int(rng.integers(1, big))) for _ in range(500)]
    cases += [(int(rng.integers(-500, 500)), int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(500)]
    for dot, na, nb in cases:
        got, want = native.view_score(dot, na, nb), rr.score(dot, na, nb)
        assert rr.bits(got) == rr.bits(want), (dot, na, nb, got, want)
    assert native.view_score(7, 49, 1) == 1.0 and native.view_score(-7, 7, 7) == -1.0 and native.view_score(0, 3, 3) == 0.0
    assert native.load().sfm_view_score(1, 1, 1, None) == native.E_SHAPE


def test_the_start_rows_against_numpy(sfm):
    native = sfm.native
    for N, K, seed, cap in ((1, 1, 0, 0), (17, 17, 3, 0), (1000, 15, 0, 0), (1000, 16, 2 ** 63, 0), (2500, 64, 1, 1000), (2500, 1000, 2 ** 64 - 1, 1000),
                            (3 * 2 ** 20 + 5, 1024, 7, 0), (2 ** 38, 1024, 11, 2 ** 22), (2 ** 22 + 1, 3, 5, 2 ** 22)):
        if N > 2 ** 24:                                                       # the reference enumerates the training rows: by formula here
            T = cap if cap else rr.CAP_DEFAULT
            want = []
            for w in range(K):
                lo, hi = w * T // K, (w + 1) * T // K
                want.append((lo + rr.mix((seed * K + w) & rr.M64) % (hi - lo)) * N // T)
        else:
            want = rr.init_rows(N, K, seed, cap).tolist()
        got = native.vocab_init_rows(N, K, seed, cap)
        assert got.tolist() == want, (N, K, seed, cap)
        assert len(set(want)) == K and want == sorted(want) and 0 <= want[0] and want[-1] < N
    lib = native.load()
    rows = np.full(8, -7, dtype=np.int64)
    for N, K, cap in ((3, 4, 0), (100, 0, 0), (100, 1025, 0), (100, 4, -1), (100, 4, 2 ** 22 + 1), (-1, 1, 0), (5000, 1001, 1000)):
        assert lib.sfm_vocab_init_rows(N, K, ctypes.c_uint64(1), cap, native._lptr(rows)) == native.E_SHAPE and np.all(rows == -7), (N, K, cap)


def test_the_version_and_the_exports(sfm):
    native = sfm.native
    assert native.load().sfm_version() >= 112
    names = ("sfm_vocab_train", "sfm_vocab_init_rows", "sfm_view_describe", "sfm_view_describe_dev", "sfm_view_pairs", "sfm_view_pairs_dev",
             "sfm_view_score")
    for name in names:
        assert name in native.EXPORTS and hasattr(native.load(), name)
    assert not any(name.startswith("sfm_track_") for name in names)
    for name in ("vocab_train", "vocab_init_rows", "view_describe", "view_describe_dev", "view_pairs", "view_pairs_dev", "view_score",
                 "check_view_pairs", "check_vocab_train"):
        assert callable(getattr(native, name))
    assert (native.RETRIEVE_MAX_WORDS, native.RETRIEVE_MAX_LEN, native.RETRIEVE_MAX_K) == (rr.MAX_WORDS, rr.MAX_LEN, rr.MAX_K)
    assert callable(sfm.processors.select_pairs) and callable(sfm.processors.match_pairs)


# ---- arguments -------------------------------------------------------------------------------------------------------------------
class _FakeSet(ctypes.Structure):
    """The layout of struct sfm_desc_set (csrc/sfm_desc.h) with no device memory behind it: every call below is refused before
    a pointer of it is read."""
    _fields_ = [("metric", ctypes.c_int), ("n", ctypes.c_int), ("dim", ctypes.c_int), ("dtype", ctypes.c_int), ("kind", ctypes.c_int),
                ("n_pad", ctypes.c_int), ("dp", ctypes.c_int), ("bf", ctypes.c_void_p), ("norm", ctypes.c_void_p), ("f32", ctypes.c_void_p),
                ("words", ctypes.c_void_p), ("upload_bytes", ctypes.c_int64)]


def _fake(n, dim, metric=0, kind=0):
    return _FakeSet(metric, n, dim, 0, kind, (n + 127) // 128 * 128 or 128, 128 if dim <= 128 else 256, None, None, None, None, 0)


def _handles(sets):
    return (ctypes.c_void_p * max(len(sets), 1))(*[ctypes.addressof(s) if s is not None else None for s in sets])


def _facts(sets):
    return [None if s is None else (s.n, s.dim, s.metric, s.kind == 0) for s in sets]


def test_training_refuses_bad_arguments_before_a_device_is_looked_for(sfm):
    native = sfm.native
    lib = native.load()
    good = [_fake(300, 128), _fake(0, 128), _fake(200, 128)]
    cases = [(good, 0, 4, 0, "K = 0"), (good, 1025, 4, 0, "K = 1025"), (good, 8, -1, 0, "iters"), (good, 8, 65, 0, "iters"),
             (good, 8, 4, -1, "train_cap"), (good, 8, 4, 2 ** 22 + 1, "train_cap"), ([], 8, 4, 0, "0 sets"),
             ([good[0], _fake(10, 128, metric=1, kind=1)], 8, 4, 0, "set 1 is not an exact L2 set"),
             ([_fake(10, 128, kind=2), good[0]], 8, 4, 0, "set 0 is not an exact L2 set"),
             ([good[0], _fake(10, 64)], 8, 4, 0, "set 1 has dim 64"), ([good[0], None], 8, 4, 0, "set 1 is null"),
             ([_fake(2000, 256)], 513, 4, 0, "K * D = 131328"), (good, 501, 4, 0, "T = 500 training rows for K = 501"),
             (good, 300, 4, 299, "T = 299 training rows for K = 300"), ([_fake(2 ** 22 + 1, 128)], 8, 4, 0, "at most 2^22")]
    for sets, K, iters, cap, word in cases:
        words = np.full((1024, 256), 7, dtype=np.uint8)
        log = np.full((66, 3), -7, dtype=np.int64)
        st = lib.sfm_vocab_train(len(sets), _handles(sets), K, iters, ctypes.c_uint64(1), cap, native._u8ptr(words), native._lptr(log))
        assert st == native.E_SHAPE and word in native.last_error() and np.all(words == 7) and np.all(log == -7), (word, native.last_error())
        with pytest.raises(ValueError) as err:
            native.check_vocab_train(_facts(sets), K, iters, 1, cap)
        assert word in str(err.value), (word, str(err.value))
    assert lib.sfm_vocab_train(3, _handles(good), 8, 4, ctypes.c_uint64(1), 0, None, None) == native.E_SHAPE
    with pytest.raises(ValueError, match="seed"):
        native.check_vocab_train(_facts(good), 8, 4, -1, 0)
    with pytest.raises(ValueError, match="integer"):
        native.check_vocab_train(_facts(good), 8.5, 4, 1, 0)
    sets, K, iters, seed, cap, D, N, T = native.check_vocab_train(_facts(good), 8, 0, 2 ** 63, 100)
    assert (K, iters, seed, cap, D, N, T) == (8, 0, 2 ** 63, 100, 128, 500, 100)


def test_describing_refuses_bad_arguments_before_a_device_is_looked_for(sfm):
    native = sfm.native
    lib = native.load()
    vocab, views = _fake(64, 128), [_fake(300, 128), _fake(0, 128)]
    cases = [(None, views, "vocabulary is null"), (_fake(64, 128, metric=1, kind=1), views, "vocabulary 0 is not an exact L2 set"),
             (_fake(0, 128), views, "K = 0"), (_fake(1025, 8), views, "K = 1025"), (_fake(1024, 129), views, "K * D = 132096"),
             (vocab, [], "0 views"), (vocab, [views[0], _fake(5, 128, kind=2)], "view 1 is not an exact L2 set"),
             (vocab, [views[0], _fake(5, 96)], "view 1 has dim 96"), (vocab, [_fake(5, 64)], "the views have dim 64, the vocabulary 128"),
             (vocab, [views[0], None], "view 1 is null")]
    for voc, vs, word in cases:
        desc = np.full(64 * 128 * 2, 7, dtype=np.int8)
        norm2 = np.full(2, -7, dtype=np.int64)
        st = lib.sfm_view_describe(None if voc is None else ctypes.addressof(voc), len(vs), _handles(vs), desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)),
                                   native._lptr(norm2), None, None, None)
        assert st == native.E_SHAPE and word in native.last_error() and np.all(desc == 7) and np.all(norm2 == -7), (word, native.last_error())
        st = lib.sfm_view_describe_dev(None if voc is None else ctypes.addressof(voc), len(vs), _handles(vs), None, None, None, None, None, None)
        assert st == native.E_SHAPE and word in native.last_error()
        with pytest.raises(ValueError) as err:
            native.check_view_describe(None if voc is None else _facts([voc])[0], _facts(vs))
        assert word in str(err.value), (word, str(err.value))


def test_pairs_refuse_bad_arguments_before_a_device_is_looked_for(sfm):
    native = sfm.native
    lib = native.load()
    V, length = 5, 16
    desc, norm2 = np.ones((V, length), dtype=np.int8), np.full(V, length, dtype=np.int64)
    good = dict(V=V, len=length, desc=desc, norm2=norm2, k=2, min_score=-np.inf, mutual=0, sequential=0, cap=10)
    bad = [("V", 0, "V = 0"), ("V", 65537, "V = 65537"), ("len", 0, "len = 0"), ("len", 131073, "len = 131073"), ("desc", None, "null"),
           ("norm2", None, "null"), ("k", 0, "k = 0"), ("k", 65, "k = 65"), ("min_score", float("nan"), "NaN"), ("mutual", 2, "mutual"),
           ("mutual", -1, "mutual"), ("sequential", -1, "sequential"), ("cap", -1, "cap")]
    i8 = ctypes.POINTER(ctypes.c_int8)
    for name, value, word in bad:
        kw = dict(good)
        kw[name] = value
        outs = dict(nbr=np.full((V, 64), -7, dtype=np.int32), nbr_score=np.full((V, 64), -7.0), pairs=np.full((10, 2), -7, dtype=np.int32),
                    how=np.full(10, -7, dtype=np.int32), pair_score=np.full(10, -7.0), n_pairs=np.full(1, -7, dtype=np.int64))
        for dev in (False, True):
            fn = lib.sfm_view_pairs_dev if dev else lib.sfm_view_pairs
            args = [kw["V"], kw["len"], None if kw["desc"] is None else kw["desc"].ctypes.data_as(ctypes.c_void_p if dev else i8),
                    None if kw["norm2"] is None else (kw["norm2"].ctypes.data_as(ctypes.c_void_p) if dev else native._lptr(kw["norm2"])),
                    kw["k"], kw["min_score"], kw["mutual"], kw["sequential"], kw["cap"]]
            if dev:
                args += [None] * 6 + [native._lptr(outs["n_pairs"]), None]
            else:
                args += [native.iptr(outs["nbr"]), native.dptr(outs["nbr_score"]), native.iptr(outs["pairs"]), native.iptr(outs["how"]),
                         native.dptr(outs["pair_score"]), None, native._lptr(outs["n_pairs"])]
            assert fn(*args) == native.E_SHAPE and word in native.last_error(), (name, value, native.last_error())
            assert all(np.all(v == -7) for v in outs.values())
        if value is None:
            continue
        with pytest.raises(ValueError) as err:
            native.check_view_pairs(kw["V"], kw["len"], kw["k"], kw["min_score"], kw["mutual"], kw["sequential"], kw["cap"])
        assert word in str(err.value)
    assert lib.sfm_view_pairs(V, length, desc.ctypes.data_as(i8), native._lptr(norm2), 2, 0.0, 0, 0, 10, None, None, None,
                              np.zeros(10, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None, None) == native.E_SHAPE
    assert "without pairs" in native.last_error()
    assert native.check_view_pairs(V, length, 64, -1.5, True, 2 ** 31 - 1, 0) == (V, length, 64, -1.5, 1, 2 ** 31 - 1, 0)
    with pytest.raises(ValueError, match="2\\^31 pairs"):
        native.check_view_pairs(65536, 8, 64, 0.0, 0, 65536, 0)


# ---- the quality record ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_the_band_scene_lists_its_neighbours_and_little_else(seed):
    """40 views on a band, about 2 100 keys per view, K = 32, 4 rounds, k = 4 (the scene of the issue's record, this file's
    generator).  Recorded (seeds 11, 12, 13): 83, 84, 83 of the 780 pairs are listed, all 77 pairs of views at most two apart
    among them; the largest |q| is 41, far from the clamp; no word is ever without a row."""
    V = 40
    views = rr.band_scene(V, seed)
    words, log, d, p = rr.select(views, 32, 4, seed, 4)
    listed = set(map(tuple, p["pairs"].tolist()))
    near = {(a, b) for a in range(V) for b in range(a + 1, V) if b - a <= 2}
    print("seed %d: %.0f keys per view, %d of %d pairs listed, %d of %d near pairs, max |q| %d" % (
        seed, np.mean([v.shape[0] for v in views]), len(listed), V * (V - 1) // 2, len(near & listed), len(near), np.abs(d["desc"]).max()))
    assert near <= listed
    assert 100 * len(listed) <= 15 * (V * (V - 1) // 2)
    assert np.abs(d["desc"]).max() < 127 and not log[:, 1].any() and np.all(np.diff(log[:, 0]) <= 0)
