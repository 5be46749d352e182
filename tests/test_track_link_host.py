"""Host-side checks of the track linking (no GPU): every case of tests/test_gpu_track_link.py is SETTLED -- the two label
routes of tests/_track_link_reference.py agree in every output, so the GPU tests compare exactly and leave nothing out --
and says what it is there for; every argument the library and ``check_track_link`` refuse (before a device is looked for,
outputs untouched); the launch plan under ``sfm_set_cu_limit``; the mask scatter of ``link_views`` against a hand-written
table."""
import ctypes
import re

import numpy as np
import pytest

import _track_link_reference as ref


# ---- the cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_every_case_is_settled_and_says_what_it_is_for(name):
    purpose = ref.CASES[name][0]
    assert isinstance(purpose, str) and len(purpose) > 10
    case, want = ref.settled(name)              # AssertionError if the union-find and the propagation disagree anywhere
    K = int(case["key_ptr"][-1])
    assert want["key_track"].shape == (K,) and want["label"].shape == (K,)
    n_tracks, n_obs = int(want["summary"][2]), int(want["summary"][5])
    assert want["pt_ptr"].shape == (n_tracks + 1,) and want["cam_idx"].shape == (n_obs,) and n_tracks <= K // 2
    # a kept track has one key per view, ascending
    for t in range(min(n_tracks, 50)):
        cams = want["cam_idx"][want["pt_ptr"][t]:want["pt_ptr"][t + 1]]
        assert np.all(np.diff(cams) > 0) and cams.size >= case["min_len"]


def test_the_cases_reach_what_they_are_there_for():
    s = {name: ref.settled(name)[1]["summary"] for name in ref.CASES}
    assert s["no_views"].tolist() == [0] * 8 and s["no_pairs"].tolist() == [0] * 8 and s["all_masked"].tolist() == [0] * 8
    assert s["one_match"].tolist() == [1, 1, 1, 0, 0, 2, 2, 2]
    assert s["view_without_keys"][2] == 2
    assert s["conflict_small"].tolist() == [5, 2, 1, 1, 0, 3, 3, 4]
    assert s["conflict_by_counting"].tolist() == [5000, 1, 0, 1, 0, 0, 0, 5000]
    assert s["triangle"].tolist() == [3, 1, 1, 0, 0, 3, 3, 3]
    assert s["mask_split"].tolist() == [2, 2, 2, 0, 0, 4, 2, 2]
    assert s["duplicates"][0] == 8 and s["duplicates"][3] == 0
    for v in (63, 64, 65, 1023, 1025, 1100):
        assert s["through_%d" % v][6] == v and s["through_%d" % v][3] == 0
    for name in ("chain_descending", "chain_interleaved"):
        assert s[name][6] == 300 and np.array_equal(ref.settled(name)[1]["label"], ref.settled("chain_descending")[1]["label"])
    for n in (1023, 1024, 1025, 2049):
        assert s["tracks_%d" % n][2] == n and int(ref.settled("keys_%d" % n)[0]["key_ptr"][-1]) == n
    for m in (1023, 1025, 65537):
        assert int(ref.settled("m_%d" % m)[0]["pair_ptr"][-1]) == m
    for size in ("12", "70"):
        assert s["scene_%s_0" % size][3] == 0 < min(s["scene_%s_2" % size][3], s["scene_%s_10" % size][3])      # false matches make the conflicts
        assert s["scene_%s_10" % size][7] > 1024                    # ... and at 10 % they merge into a giant component
    assert s["scene_70_2"][7] > 70                                  # a conflict by counting next to conflicts found by the ordering
    assert s["min_len_2"][4] == 0 < s["min_len_3"][4] < s["min_len_6"][4] and s["min_len_6"][2] > 0
    assert s["min_len_2"][3] == s["min_len_6"][3] > 0               # conflict takes precedence over short


def test_a_permuted_listing_has_the_same_reference():
    case, want = ref.settled("scene_12_2")
    for seed in (1, 2):
        assert ref.same(ref.settle(ref.permuted(case, seed)), want)


# ---- the arguments -------------------------------------------------------------------------------------------------------
def _library_call(native, key_ptr, pair_views, pair_ptr, a, b, mask, min_len, group, scan):
    V, P, K = len(key_ptr) - 1, len(pair_ptr) - 1, 64
    outs = dict(key_track=np.full(K, -7, dtype=np.int32), pt_ptr=np.full(K, -7, dtype=np.int32), cam_idx=np.full(K, -7, dtype=np.int32),
                key_idx=np.full(K, -7, dtype=np.int32), summary=np.full(8, -7, dtype=np.int64), label=np.full(K, -7, dtype=np.int32))
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    key_ptr, pair_views, a, b = i32(key_ptr), i32(pair_views), i32(a), i32(b)
    pair_ptr = np.ascontiguousarray(pair_ptr, dtype=np.int64)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    st = native.load().sfm_link_tracks(V, native.iptr(key_ptr), P, native.iptr(pair_views), native._lptr(pair_ptr), native.iptr(a), native.iptr(b),
                                      None if mask is None else mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), min_len, group, scan,
                                      native.iptr(outs["key_track"]), native.iptr(outs["pt_ptr"]), native.iptr(outs["cam_idx"]),
                                      native.iptr(outs["key_idx"]), native._lptr(outs["summary"]), native.iptr(outs["label"]))
    return st, outs


def test_every_bad_argument_is_refused_before_a_device_is_looked_for(sfm):
    native = sfm.native
    good = dict(key_ptr=[0, 4, 7, 12], pair_views=[[0, 1], [2, 1], [0, 2]], pair_ptr=[0, 2, 3, 5], a=[0, 3, 4, 1, 2], b=[1, 2, 0, 4, 3],
                mask=None, min_len=2, group=0, scan=0)
    bad = [("key_ptr", [1, 4, 7, 12], r"key_ptr\[0\]"), ("key_ptr", [0, 4, 3, 12], "decreases at view 1"),
           ("pair_views", [[0, 1], [2, 3], [0, 2]], "pair 1 "), ("pair_views", [[0, 1], [2, 1], [-1, 2]], "pair 2 "),
           ("pair_views", [[1, 1], [2, 1], [0, 2]], "pair 0 "), ("pair_ptr", [1, 2, 3, 5], r"pair_ptr\[0\]"),
           ("pair_ptr", [0, 3, 2, 5], "decreases at pair 1"), ("min_len", 1, "min_len"), ("min_len", 0, "min_len"), ("group", 2, "group"),
           ("group", 128, "group"), ("scan", 3, "scan"), ("scan", -1, "scan"),
           ("a", [0, 4, 4, 1, 2], "match 1 "), ("a", [0, 3, 5, 1, 2], "match 2 "), ("b", [1, 2, 0, 5, 3], "match 3 "),
           ("b", [1, 2, 0, 4, -1], "match 4 "), ("a", [-1, 3, 4, 1, 7], "match 0 ")]
    for name, value, word in bad:
        kw = dict(good)
        kw[name] = value
        st, outs = _library_call(native, **kw)
        assert st == native.E_SHAPE, (name, value)
        assert re.search(word, native.last_error()), (name, value, native.last_error())
        assert all(np.all(v == -7) for v in outs.values()), (name, value)
        with pytest.raises(ValueError, match=word):
            native.check_track_link(**kw)
    # a masked match is checked like a used one
    st, outs = _library_call(native, **dict(good, a=[0, 9, 4, 1, 2], mask=[1, 0, 1, 1, 1]))
    assert st == native.E_SHAPE and "match 1 " in native.last_error() and all(np.all(v == -7) for v in outs.values())
    for kw in (dict(a=[0, 3, 4, 1]), dict(mask=[1, 1]), dict(pair_ptr=[0, 2, 5]), dict(key_ptr=[]), dict(min_len=2.5), dict(key_ptr=[0, 4, 7.5, 12])):
        with pytest.raises(ValueError, match="must"):
            native.check_track_link(**dict(good, **kw))
    with pytest.raises(ValueError, match="2\\^31"):
        native.check_track_link([0, 2 ** 31], np.zeros((0, 2)), [0], [], [])
    # what passes comes back converted
    key_ptr, pair_views, pair_ptr, a, b, mask, min_len, group, scan = native.check_track_link(
        good["key_ptr"], good["pair_views"], good["pair_ptr"], good["a"], [1.0, 2.0, 0.0, 4.0, 3.0], [2, 0, 0, 1, 1], 3, 64, 2)
    assert key_ptr.dtype == np.int32 and pair_views.shape == (3, 2) and pair_ptr.dtype == np.int64 and a.dtype == b.dtype == np.int32
    assert mask.dtype == np.uint8 and mask.tolist() == [1, 0, 0, 1, 1] and (min_len, group, scan) == (3, 64, 2)


def test_the_version(sfm):
    assert sfm.native.load().sfm_version() >= 110


# ---- the plan ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cu_limit(sfm):
    yield sfm.native.set_cu_limit
    sfm.native.set_cu_limit(0)


def test_the_plan_follows_the_cu_limit(sfm, cu_limit):
    native = sfm.native
    V, K, M = 1000, 8_000_000, 40_000_000
    free = native.track_link_plan(V, K, M)
    assert set(free) == set(native.LINK_PLAN)
    cus, _ = native.cu_count()
    assert free["union_grid"] == 16 * cus and free["order_grid"] == 32 * cus and free["big_grid"] == 4 * cus
    assert free["scan_keys"] == native.LINK_SCAN_DEVICE and free["tiles_keys"] == (K + 1023) // 1024
    assert free["scan_components"] == native.LINK_SCAN_DEVICE and free["tiles_components"] == (K // 2 + 1023) // 1024
    for limit in (1, 32):
        cu_limit(limit)
        p = native.track_link_plan(V, K, M)
        assert (p["union_grid"], p["order_grid"], p["big_grid"]) == (16 * limit, 32 * limit, 4 * limit)
        assert {k: p[k] for k in p if "grid" not in k and k != "group"} == {k: free[k] for k in free if "grid" not in k and k != "group"}
        assert p["group"] in native.TRACK_GROUPS[1:]
    cu_limit(0)
    assert native.track_link_plan(V, K, M) == free
    # small inputs: grids no larger than the work, one workgroup scans; the routes can be forced either way
    small = native.track_link_plan(3, 10, 4)
    assert (small["union_grid"], small["big_grid"], small["scan_keys"], small["tiles_keys"]) == (1, 1, 1, 1)
    assert small["group"] == 64 and small["order_grid"] == 2        # five components at the most, widened to a wave each: 320 lanes
    assert native.track_link_plan(3, 10, 0)["union_grid"] == 1 and native.track_link_plan(0, 0, 0)["tiles_keys"] == 1
    forced = native.track_link_plan(10, 5000, 100, scan=native.LINK_SCAN_DEVICE)
    assert (forced["scan_keys"], forced["tiles_keys"], forced["scan_components"], forced["tiles_components"]) == (2, 5, 2, 3)
    forced = native.track_link_plan(1000, K, M, scan=native.LINK_SCAN_ONE_BLOCK)
    assert (forced["scan_keys"], forced["scan_components"]) == (1, 1)
    assert native.track_link_plan(10, 1024, 100, scan=native.LINK_SCAN_DEVICE)["scan_keys"] == 1          # one tile is one workgroup
    assert native.track_link_plan(10, 5000, 100, group=16)["group"] == 16
    narrow = native.track_link_plan(3, 10 ** 7, 100)["group"]
    assert narrow == 4 and native.track_link_plan(1000, 10 ** 7, 100)["group"] == 8                   # min(V, 8) keys per typical track
    for bad in (dict(n_keys=-1), dict(n_keys=2 ** 31), dict(n_matches=-1), dict(group=3), dict(scan=5)):
        kw = dict(n_views=3, n_keys=10, n_matches=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            native.track_link_plan(**kw)


# ---- the mask of link_views ----------------------------------------------------------------------------------------------
def test_the_mask_scatter_of_link_views_against_a_hand_written_table(sfm):
    scatter = sfm.processors.link_key_mask
    # pair 0: reference view of 6 keys, matches at keys 1, 3, 4 (inliers: first and last); pair 1: 4 keys, dropped by the pair
    # verdict; pair 2: 3 keys, no inlier list: every match used; pair 3: 5 keys, matches at 0 and 2, none an inlier
    inliers = [(np.array([1, 3, 4]), np.array([True, False, True])), (np.array([0, 1]), np.array([1, 1])), None,
               (np.array([[0, 2]]), np.array([0, 0], dtype=np.uint8))]
    got = scatter([6, 4, 3, 5], inliers, [True, False, True, 1])
    want = [0, 1, 0, 0, 1, 0,   0, 0, 0, 0,   1, 1, 1,   0, 0, 0, 0, 0]
    assert got.dtype == np.uint8 and got.tolist() == want
    assert scatter([2, 3], None, [0, 1]).tolist() == [0, 0, 1, 1, 1]
    assert scatter([2, 3], [None, (np.zeros(0, dtype=int), np.zeros(0, dtype=bool))]).tolist() == [1, 1, 0, 0, 0]
    assert scatter([], None, None).size == 0
    for bad in (dict(inliers=[None]), dict(pair_mask=[1, 1, 1]), dict(inliers=[(np.array([0, 1]), np.array([1])), None]),
                dict(inliers=[(np.array([2]), np.array([1])), None]), dict(inliers=[None, (np.array([-1]), np.array([1]))])):
        with pytest.raises(ValueError, match="link"):
            scatter([2, 3], **bad)
