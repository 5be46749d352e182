"""Host-side checks of the relative pose of a verified pair (no GPU): the test of one match (sfm_twoview_pose_test) against
the rule in exact fused multiply-adds, bit for bit in both flags; the argument checks, which launch nothing; the NumPy
reference of tests/_twoview_pose_reference.py on the scenes the GPU tests use -- EVERY set of every scene
tests/test_gpu_twoview_pose.py uses is settled, so the GPU tests compare decisions exactly and leave nothing out; and the
decisions of the reference against the planted poses."""
import math

import numpy as np
import pytest

import _twoview_pose_reference as tp


def _edge_inputs():
    I = np.identity(3)
    R = tp.rodrigues([0.05, -0.1, 0.03])
    t = np.array([1.0, 0.0, 0.0])
    a = np.array([0.1, -0.2])
    big, tiny = 1e200, 1e-200
    yield I, t, a, a, tp.COS2_MIN                                   # parallel rays: d is the rounding of p q - r r
    yield I, np.zeros(3), a, a + 1e-3, tp.COS2_MIN                  # no translation: m1 = m2 = 0
    yield I, t, a, a + np.array([-1e-3, 0.0]), tp.COS2_MIN          # in front, narrow
    yield I, t, a, a + np.array([1e-3, 0.0]), tp.COS2_MIN           # the rays diverge: behind
    yield I, t, a, a + np.array([-0.5, 0.0]), tp.COS2_MIN           # in front, wide
    yield I, t, a, a + np.array([-0.5, 0.0]), 0.0                   # cos2_min = 0: only an obtuse pair has parallax
    yield I, t, a, a + np.array([-0.5, 0.0]), 1.0
    yield I, t, np.array([3.0, 0.0]), np.array([-3.0, 0.0]), 0.0    # r < 0: parallax whatever cos2_min
    yield R, t, np.array([np.nan, 0.0]), a, tp.COS2_MIN
    yield R, t, a, np.array([0.0, np.inf]), tp.COS2_MIN
    yield R, np.array([np.nan, 0.0, 0.0]), a, a, tp.COS2_MIN
    yield R * np.nan, t, a, a, tp.COS2_MIN
    yield R, t, np.array([big, big]), np.array([big, -big]), tp.COS2_MIN      # p q overflows
    yield R, t, np.array([tiny, tiny]), np.array([-tiny, tiny]), tp.COS2_MIN
    yield R, t * big, a, a + 0.1, tp.COS2_MIN
    yield np.zeros((3, 3)), t, a, a, tp.COS2_MIN
    for k in range(40):                                            # rays a rounding apart, both ways
        b = a.copy()
        b[k % 2] = np.nextafter(b[k % 2], (-1.0) ** k * np.inf)
        yield I, t * (-1.0) ** (k // 2), a, b, tp.COS2_MIN
    # on the parallax bound: r^2 against cos2_min p q with exactly representable numbers (a' = (0, 0, 1), b = (x, 0, 1))
    for x in (0.5, 1.0, 2.0):
        cos2 = 1.0 / (1.0 + x * x)
        for c in (cos2, np.nextafter(cos2, 0.0), np.nextafter(cos2, 1.0)):
            yield I, np.array([-1.0, 0.0, 0.0]), np.zeros(2), np.array([x, 0.0]), c


def test_the_hook_is_the_rule_bit_for_bit(sfm):
    native = sfm.native
    rng = np.random.default_rng(7)
    cases = list(_edge_inputs())
    for _ in range(1500):
        R = tp.rodrigues(rng.normal(size=3) * rng.choice([0.05, 1.0]))
        t = tp._unit(rng.normal(size=3))
        a = rng.uniform(-1.0, 1.0, size=2)
        X = np.array([a[0], a[1], 1.0]) * rng.uniform(0.5, 20.0) * rng.choice([-1.0, 1.0, 1.0])
        Y = R @ X + t * rng.choice([1.0, 1.0, 1e-3])
        b = Y[:2] / Y[2] + rng.choice([0.0, 1e-3]) * rng.normal(size=2)
        cases.append((R, t, a, b, rng.choice([tp.COS2_MIN, 0.0, 1.0, 0.9, 0.5])))
    seen = np.zeros((2, 2), dtype=int)
    for k, (R, t, a, b, cos2) in enumerate(cases):
        want = tp.pose_test_exact(R, t, a, b, cos2)
        got = native.twoview_pose_test(R, t, a, b, cos2)
        assert got == want, (k, R, t, a, b, cos2, got, want)
        seen[got] += 1
    assert seen[0, 0] > 100 and seen[1, 0] > 100 and seen[1, 1] > 100 and seen[0, 1] == 0       # parallax only where in front


def test_the_exact_fma_is_a_fused_multiply_add():
    assert tp.fma(1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0) == -2.0 ** -60        # the product alone rounds to 1
    assert tp.fma(3.0, 4.0, 5.0) == 17.0 and math.isnan(tp.fma(math.nan, 1.0, 1.0)) and tp.fma(1e300, 1e300, 0.0) == math.inf


def _lib_status(native, n_sets, set_ptr, M, kind, Kl, Kr, cos2, min_par):
    """The status of the library's entry point itself, every array given."""
    lib = native.load()
    set_ptr = None if set_ptr is None else np.ascontiguousarray(set_ptr, dtype=np.int32)
    kind = np.ascontiguousarray(kind, dtype=np.int32)
    Kl, Kr = np.ascontiguousarray(Kl, dtype=np.float64).reshape(9), np.ascontiguousarray(Kr, dtype=np.float64).reshape(9)
    m = max(int(M), 1)
    left, right, model = np.zeros((2, m)), np.zeros((2, m)), np.zeros((max(n_sets, 1), 9))
    R, t = np.zeros((max(n_sets, 1), 9)), np.zeros((max(n_sets, 1), 3))
    return lib.sfm_twoview_pose(n_sets, native.iptr(set_ptr), M, native.dptr(left), native.dptr(right), None, native.dptr(model),
                                native.iptr(kind), native.dptr(Kl), native.dptr(Kr), cos2, min_par, native.dptr(R), native.dptr(t),
                                None, None, None, None, None, None, None, None, None)


BAD_K = [np.array([[800.0, 0, 320], [1e-3, 800, 240], [0, 0, 1]]), np.array([[800.0, 0, 320], [0, 800, 240], [1e-9, 0, 1]]),
         np.array([[800.0, 0, 320], [0, 800, 240], [0, 1.0, 1]]), np.array([[800.0, 0, 320], [0, 800, 240], [0, 0, 2.0]]),
         np.array([[np.nan, 0, 320], [0, 800, 240], [0, 0, 1.0]])]


def bad_arguments():
    """(n_sets, set_ptr, M, kind, K_left, K_right, cos2_min, min_parallax) the library refuses, each for one reason."""
    ok = dict(n_sets=2, set_ptr=[0, 3, 5], M=5, kind=[0, 1], Kl=tp.K_LEFT, Kr=tp.K_RIGHT, cos2=tp.COS2_MIN, min_par=8)
    for change in ([dict(set_ptr=p) for p in ([1, 3, 5], [0, 3, 4], [0, 6, 5], None)] + [dict(M=-1), dict(n_sets=-1)] +
                   [dict(cos2=c) for c in (math.nan, -1e-9, 1.0 + 1e-9, math.inf)] + [dict(min_par=-1)] +
                   [dict(kind=k) for k in ([0, 2], [-1, 0])] + [dict(Kl=K) for K in BAD_K] + [dict(Kr=K) for K in BAD_K]):
        args = dict(ok)
        args.update(change)
        yield args


def test_the_library_refuses_bad_arguments_before_it_needs_a_device(sfm):
    native = sfm.native
    n = 0
    for args in bad_arguments():                   # the entry point returns before it initialises anything
        assert _lib_status(native, **args) == native.E_SHAPE, args
        assert "sfm_twoview_pose" in native.last_error()
        n += 1
    assert n == 23


def test_the_python_layer_refuses_the_same(sfm):
    native = sfm.native
    left = np.zeros((2, 5))
    good = dict(set_ptr=[0, 3, 5], left=left, right=left, models=np.zeros((2, 3, 3)), kinds=[0, 1], K_left=tp.K_LEFT, K_right=tp.K_RIGHT,
                cos2_min=tp.COS2_MIN, min_parallax=8)
    bad = [dict(set_ptr=[1, 3, 5]), dict(set_ptr=[0, 3, 4]), dict(set_ptr=[]), dict(cos2_min=math.nan), dict(cos2_min=-0.1),
           dict(cos2_min=1.1), dict(min_parallax=-1), dict(min_parallax=1.5), dict(kinds=[0, 2]), dict(kinds=[0]), dict(kinds=["fundamental", "affine"]),
           dict(models=np.zeros((3, 3, 3))), dict(K_left=BAD_K[0]), dict(K_right=BAD_K[3]), dict(K_left=np.zeros((3, 4))),
           dict(right=np.zeros((2, 4))), dict(mask=np.zeros(4)), dict(outputs=("mask",))]
    for change in bad:
        args = dict(good)
        args.update(change)
        with pytest.raises(ValueError):
            native.twoview_pose(**args)
    for change in bad[:14]:
        args = dict(good)
        args.update(change)
        for name in ("left", "right"):
            args.pop(name)
        with pytest.raises(ValueError):
            native.twoview_pose_dev(args.pop("set_ptr"), 5, 0, 0, **args)
    assert (native.POSE_EMPTY, native.POSE_NO_MODEL, native.POSE_NO_POSE, native.POSE_TIED, native.POSE_NO_PARALLAX) == \
        (tp.EMPTY, tp.NO_MODEL, tp.NO_POSE, tp.TIED, tp.NO_PARALLAX)
    assert (native.POSE_FROM_F, native.POSE_FROM_H, native.POSE_CANDIDATES) == (tp.FROM_F, tp.FROM_H, 4)
    assert native.POSE_KINDS == {"fundamental": 0, "homography": 1} and len(native.POSE_SUMMARY) == 6
    for name in ("sfm_twoview_pose", "sfm_twoview_pose_dev", "sfm_twoview_pose_test", "sfm_twoview_pose_pairs"):
        assert name in native.EXPORTS
    assert native.load().sfm_version() >= 103


@pytest.mark.parametrize("name", tp.CASES)
def test_every_set_of_every_scene_is_settled(name, capsys):
    sc, ref = tp.scene_and_reference(name)
    with capsys.disabled():
        print("\n%s: %d sets, %d unsettled, worst d_P %.3e, summary %s, statuses %s"
              % (name, sc.counts.size, int((~ref.settled).sum()), ref.d_P.max(initial=0.0), ref.summary.tolist(),
                 np.flatnonzero(np.bincount(ref.status, minlength=32)).tolist()))
    assert ref.settled.all(), np.flatnonzero(~ref.settled)
    assert ref.d_P.max(initial=0.0) < 1e-9                 # the two routes agree far inside the bound the GPU tests use
    # ... and the points they triangulate agree within the bound the GPU tests apply to X_out, in every set
    assert np.all(ref.d_X <= np.maximum(1e-9, 100.0 * ref.d_P)), float((ref.d_X / np.maximum(1e-9, 100.0 * ref.d_P)).max())
    assert ref.summary[0] + ref.summary[1] + ref.summary[2] == sc.counts.size
    assert ref.summary[4] == (ref.obs > 0).sum() == ref.n_front.sum()
    assert np.array_equal(np.isnan(ref.X).any(axis=0), ref.obs == 0)


def test_the_other_settings_are_settled_too():
    sc = tp.scene(tp.NO_MASK_CASE)
    ref = tp.reference(sc.set_ptr, sc.left, sc.right, None, sc.models, sc.kinds)
    assert ref.settled.all() and ref.summary[5] > 0
    sc = tp.scene(tp.OPTION_SCENE)
    for cos2, min_par in tp.OPTION_CASES:
        ref = tp.reference(sc.set_ptr, sc.left, sc.right, sc.mask, sc.models, sc.kinds, cos2_min=cos2, min_parallax=min_par)
        assert ref.settled.all(), (cos2, min_par)
        assert bool((ref.status & tp.NO_PARALLAX).any()) == (min_par == 1000)
    # the scenes of the Python entry points (tests/test_gpu_twoview_pose.py)
    l, r, displaced, F, kind = tp.family_part("general", 300, 21, 0.0, Kr=tp.K_LEFT)
    q = tp.solve_set(l, r, ~displaced, F, kind, tp.K_LEFT, tp.K_LEFT)
    assert q.settled and q.n_front == 300 and (q.cand_front == 300).sum() == 1


def test_the_scenes_are_what_they_say():
    sc = tp.scene("sizes")
    assert sc.counts.tolist() == list(tp.SIZES) and set(sc.kinds.tolist()) == {tp.FROM_F, tp.FROM_H}
    sc, ref = tp.scene_and_reference("many")
    assert sc.counts.size == 259 and set(sc.counts.tolist()) == set(tp.MANY_SIZES) and set(sc.kinds.tolist()) == {0, 1}
    assert set(sc.names) == set(tp.FAMILIES) and sc.displaced.any()
    assert ref.summary[0] > 100 and ref.summary[2] > 0 and ref.summary[3] > 0          # posed, empty and tied sets occur
    sc, ref = tp.scene_and_reference("special")
    by = {name: s for s, name in enumerate(sc.names)}
    assert ref.status[by["masked_out"]] == tp.EMPTY | tp.NO_POSE and ref.best[by["masked_out"]] == -1
    for name in ("rank1_F", "singular_H", "nan_F", "nan_H", "zero_H"):
        assert ref.status[by[name]] == tp.NO_MODEL | tp.NO_POSE and np.all(ref.cand_front[by[name]] == -1), name
    # a NaN coordinate: that match is not selected, the rest is unchanged
    nan_set, clean = by["nan_coordinate"], by["clean_general"]
    lo, lo2 = sc.set_ptr[nan_set], sc.set_ptr[clean]
    keep = np.ones(70, dtype=bool)
    keep[[17, 40]] = False
    assert np.isnan(sc.left[:, lo:lo + 70]).sum() == 1 and np.isnan(sc.right[:, lo:lo + 70]).sum() == 1
    assert np.array_equal(ref.obs[lo:lo + 70][keep], ref.obs[lo2:lo2 + 70][keep]) and not ref.obs[lo:lo + 70][~keep].any()
    assert ref.n_front[nan_set] == ref.n_front[clean] - 2 and np.array_equal(ref.R[nan_set], ref.R[clean])


@pytest.mark.parametrize("name", ["general", "general_displaced", "forward", "forward_displaced", "behind"])
def test_the_winner_is_the_candidate_nearest_the_planted_pose(name):
    sc, ref = tp.scene_and_reference(name)
    R0, t0 = tp.planted(name.split("_")[0])
    for s, q in enumerate(ref.sets):
        dist = [tp.pose_distance(q.cands.R[k], q.cands.t[k], R0, t0) if q.cands.ok[k] else np.inf for k in range(4)]
        lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
        if name == "behind":            # the points lie behind both cameras: the vote takes the pose that puts them in front
            assert q.best >= 0 and q.best != int(np.argmin(dist)) and np.allclose(q.R, R0, atol=1e-9) and np.allclose(q.t, -t0, atol=1e-9)
            continue
        assert q.best == int(np.argmin(dist)) and dist[q.best] < 1e-9, (s, dist)
        if name.startswith("general"):  # every clean match is in front
            assert np.all(ref.obs[lo:hi][sc.mask[lo:hi]] > 0) and not ref.obs[lo:hi][~sc.mask[lo:hi]].any()
            assert q.n_front == sc.mask[lo:hi].sum() and not q.status


@pytest.mark.parametrize("name", ["plane", "plane_displaced", "sizes"])
def test_on_a_plane_the_winner_has_the_count_of_the_planted_pose(name):
    sc, ref = tp.scene_and_reference(name)
    R0, t0 = tp.planted("plane")
    tied = 0
    for s, q in enumerate(ref.sets):
        if sc.names[s] != "plane" or sc.counts[s] == 0:
            continue
        lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
        a, b = tp.rays(tp.K_LEFT, sc.left[:, lo:hi]), tp.rays(tp.K_RIGHT, sc.right[:, lo:hi])
        front = tp.front_of(tp.front_terms(R0, t0, a, b), sc.mask[lo:hi], tp.COS2_MIN, 0.0)[0]
        assert q.n_front == front.sum() == q.cand_front.max()
        others = [k for k in range(4) if k != q.best and q.cands.ok[k] and q.cand_front[k] == q.n_front]
        assert bool(q.status & tp.TIED) == bool(others)
        tied += bool(others)
        if not others:                  # ... and where nothing ties, it is the planted pose up to the noise of the matches
            assert tp.pose_distance(q.R, q.t, R0, t0) < 1e-9
            assert np.allclose(np.abs(q.n @ tp.PLANE_N), 1.0, atol=1e-9)
    assert tied > 0 or name != "sizes"  # the single match of "sizes" cannot tell the two solutions apart


def test_a_camera_that_only_rotated_has_no_parallax():
    sc, ref = tp.scene_and_reference("rotation")
    assert np.all(ref.status & tp.NO_PARALLAX) and not ref.n_parallax.any() and np.all(ref.best >= 0)
    # noise-free matches and K R K^-1 itself: whichever candidate wins, the rotation is the planted one
    R0, _ = tp.planted("rotation")
    for n, seed in zip(tp.FAMILY_COUNTS, (1, 2, 3)):
        l, r, displaced, model, kind = tp.family_part("rotation", n, seed, noise=0.0)
        q = tp.solve_set(l, r, ~displaced, model, kind, cos2_min=math.cos(math.radians(2.0)) ** 2)
        assert kind == tp.FROM_H and q.best >= 0 and q.status & tp.NO_PARALLAX and q.n_parallax == 0
        assert np.abs(q.R - R0).max() <= max(1e-9, 100 * q.d_P)


def test_the_conversion_to_the_reference_convention():
    R, t = tp.planted("general")
    rot, centre = tp.to_reference_convention(R, t)
    X = np.array([0.3, -0.2, 5.0])
    assert np.allclose(rot.T @ (X - centre[:, 0]), R @ X + t)      # K [rot^T | -rot^T centre] projects what K [R | t] projects
