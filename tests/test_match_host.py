"""Host side of the KeyTracker drop-in (no GPU): matching.py driven by the NumPy stand-in's neighbours reproduces the
reference's tables (tests/golden/g12_keytracker_*.npz), the closed form of quirk Q14 equals the reference's loop, the
reference's exceptions (Q16) are raised, and the mixin fits in front of the reference class."""
import inspect
import json
import os

import numpy as np
import pytest

import _bfmatcher_numpy as bfm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NON_FUND = ("sift_knn", "sift_cross", "sift_match", "orb_knn")


def standin_neighbours(norm, query, train, mode_cross):
    idx, dist, cb = bfm.neighbours(norm, query, train, k=2, col_best=mode_cross)
    mutual = np.zeros(idx.shape[0], dtype=bool)
    if mode_cross:
        mutual = (idx[:, 0] >= 0) & (cb[np.maximum(idx[:, 0], 0)] == np.arange(idx.shape[0]))
    return idx[:, 0], dist[:, 0], idx[:, 1], dist[:, 1], mutual


def replay(sfm, g):
    key_type = str(g["key_type"]); cross, knn, _fund = (bool(x) for x in g["flags"])
    norm = bfm.NORM_L2 if key_type in ("sift", "surf") else bfm.NORM_HAMMING
    nv = int(g["n_views"])
    desc = [g["desc_%d" % v] for v in range(nv)]
    tables = [np.full((1, desc[0].shape[0]), -1, dtype=np.int64)]
    for v in range(1, nv):
        tables = [np.vstack((t, np.full((1, t.shape[1]), -1))) for t in tables]
        new = np.full((v + 1, desc[v].shape[0]), -1, dtype=np.int64)
        for r in range(v):
            nn = standin_neighbours(norm, desc[v], desc[r], cross)
            q, t, d = sfm.matching.filter_matches(*nn, knn, cross)
            wq, wt = sfm.matching.table_writes(q, t, d)
            tables[r][v, wt] = wq
            new[r, wq] = wt
        tables.append(new)
    return tables


@pytest.mark.parametrize("case", NON_FUND)
def test_matching_reproduces_reference_tables(sfm, case):
    g = np.load(os.path.join(GOLDEN, "g12_keytracker_%s.npz" % case))
    tables = replay(sfm, g)
    for v, t in enumerate(tables):
        np.testing.assert_array_equal(t, g["table_%d" % v], err_msg="%s view %d" % (case, v))


def reference_dedup(train, dist):
    """key_tracker.py:276-291, step by step."""
    kept, seen = [], []
    for i in range(len(train)):
        try:
            p = seen.index(train[i])
            if dist[i] < dist[p]:
                seen[p] = train[i]
                kept[p] = i
        except ValueError:
            kept.append(i)
            seen.append(train[i])
    return kept


def test_q14_closed_form_equals_reference_loop(sfm):
    rng = np.random.default_rng(3)
    for trial in range(300):
        n = int(rng.integers(0, 60))
        train = rng.integers(0, max(1, n // 3 + 1), n)
        dist = rng.integers(0, 6, n).astype(np.float32)        # many equal distances
        want = reference_dedup(train.tolist(), dist.tolist())
        got = sfm.matching.dedup_kept(train, dist)
        assert got.tolist() == want, (trial, train, dist)


def _reference_knn_filter(matches):
    return [item[0] for item in matches if (item[0].distance / item[1].distance) < 0.7]     # key_tracker.py:342


def _exc_type(fn):
    try:
        fn()
    except Exception as e:        # noqa: BLE001
        return type(e)
    return None


def test_q16_exceptions_match_reference(sfm):
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, (4, 128)).astype(np.uint8)
    one = rng.integers(0, 256, (1, 128)).astype(np.uint8)
    m = bfm.BFMatcher(bfm.NORM_L2)
    # a single-descriptor reference in k = 2 mode: IndexError (item[1])
    want = _exc_type(lambda: _reference_knn_filter(m.knnMatch(q, one, k=2)))
    got = _exc_type(lambda: sfm.matching.filter_matches(*standin_neighbours(bfm.NORM_L2, q, one, False), True, False))
    assert want is IndexError and got is IndexError
    # d1 == 0: two exact copies of a query row in the reference view: ZeroDivisionError
    two = np.vstack((q[1:2], q[1:2], one))
    want = _exc_type(lambda: _reference_knn_filter(m.knnMatch(q, two, k=2)))
    got = _exc_type(lambda: sfm.matching.filter_matches(*standin_neighbours(bfm.NORM_L2, q, two, False), True, False))
    assert want is ZeroDivisionError and got is ZeroDivisionError


def test_q16_fundamental_needs_eight_matches(sfm):
    ep = sfm.processors.HipEpipolarProcessor(None)
    with pytest.raises(ValueError):
        ep.determine_fundamental_mat([np.ones((3, 7)), np.ones((3, 7))], object())


def test_ratio_test_in_python_floats(sfm):
    # d0 / d1 evaluated in float64 on float32 distances: 0.7 * d1 rounded to float32 may land on either side
    d1 = np.float32(10.0)
    d0 = np.float32(7.0)                       # 7/10 == 0.7 in float64 -> not < RATIO
    q, _t, _d = sfm.matching.filter_matches(np.array([0]), np.array([d0]), np.array([1]), np.array([d1]),
                                            np.array([False]), True, False)
    assert q.shape[0] == 0
    d0 = np.nextafter(np.float32(7.0), np.float32(0))
    q, _t, _d = sfm.matching.filter_matches(np.array([0]), np.array([d0]), np.array([1]), np.array([d1]),
                                            np.array([False]), True, False)
    assert q.tolist() == [0]


def _api():
    with open(os.path.join(GOLDEN, "g12_keytracker_api.json")) as f:
        return json.load(f)


def test_mixin_fits_in_front_of_the_reference_class(sfm):
    api = _api()
    P = sfm.processors
    assert "_KeyTracker__extend_list" in api["mangled"]
    assert any("self.__extend_list(" in ln for ln in api["add_new_view_calls"])

    # a stand-in base class built from the recorded API
    def method(params):
        ns = {}
        exec("def f(%s):\n    raise AssertionError('reference body called')" % ", ".join(params), ns)
        return ns["f"]

    body = {name: method(p) for name, p in api["KeyTracker"].items() if name != "__init__"}
    RefKeyTracker = type("KeyTracker", (), body)
    Drop = type("KeyTracker", (P.HipKeyTrackerMixin, RefKeyTracker), {})
    assert Drop.__mro__[1] is P.HipKeyTrackerMixin
    assert Drop._KeyTracker__extend_list is P.HipKeyTrackerMixin._KeyTracker__extend_list
    got = list(inspect.signature(P.HipKeyTrackerMixin._KeyTracker__extend_list).parameters)
    assert got == api["KeyTracker"]["_KeyTracker__extend_list"]
    # the standalone classes carry the reference's public signatures
    for name, params in api["KeyTracker"].items():
        if name.startswith("_KeyTracker__") and name != "_KeyTracker__extend_list":
            continue
        assert list(inspect.signature(getattr(P.HipKeyTracker, name)).parameters) == params, name
    for name, params in api["KeyTrack"].items():
        assert list(inspect.signature(getattr(P.HipKeyTrack, name)).parameters) == params, name


def test_keytrack_mirror_semantics(sfm):
    t = sfm.processors.HipKeyTrack(2, 6, 1)
    t.expand_table()
    assert t.table.shape == (3, 6) and (t.table == -1).all()
    t.update_usage(np.array([[4, 1, 4]]), np.array([[7, 8, 9]]))
    assert t.table[1].tolist() == [-1, 8, -1, -1, 9, -1]
    idx, vals = t.extract_constructed_points()
    assert idx.tolist() == [[1, 4]] and vals.tolist() == [[8, 9]]
    assert t.extract_unconstructed_points().tolist() == [[0, 2, 3, 5]]


def test_falsy_flags_fall_back_to_the_object(sfm, monkeypatch):
    kt = sfm.processors.HipKeyTracker("sift", False, True, True, "cfg")
    seen = []
    monkeypatch.setattr(kt, "_KeyTracker__extend_list", lambda *a: seen.append(a[2:]))

    class V:
        key_pts = [None] * 3
    kt.add_new_view(V(), [])
    kt.add_new_view(V(), [V()], False, False, None)          # Q17: False -> the object's setting
    assert seen == [(True, True, "cfg")]


def test_standin_sqrt_is_correctly_rounded():
    s = np.concatenate((np.arange(0, 5000), np.arange((1 << 22) - 3000, (1 << 22) + 3000), [2 ** 31 - 1]))
    got = bfm.sqrt_rn_f32(s)
    import decimal
    decimal.getcontext().prec = 50
    for v in s[:: 97].tolist():
        exact = decimal.Decimal(v).sqrt()
        cand = [np.float32(got[s.tolist().index(v)])]
        c = cand[0]
        lo, hi = np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(np.inf))
        err = abs(decimal.Decimal(float(c)) - exact)
        assert err <= abs(decimal.Decimal(float(lo)) - exact) and err <= abs(decimal.Decimal(float(hi)) - exact), v
