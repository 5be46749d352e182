"""Host-side checks of the refinement of a relative pose (no GPU): the residual and Jacobian row of one match
(sfm_twoview_refine_test) against the NumPy rule and against central differences of it; the argument checks, which launch
nothing; the NumPy reference of tests/_twoview_refine_reference.py on the scenes the GPU tests use -- EVERY set of every parity
case of tests/test_gpu_twoview_refine.py is settled, so the GPU tests compare decisions exactly and leave nothing out; and what
the reference's iteration achieves against the planted poses."""
import math

import numpy as np
import pytest

import _twoview_pose_reference as tp
import _twoview_refine_reference as rr


# ---- the hook ------------------------------------------------------------------------------------------------------------
def _random_case(rng):
    R = tp.rodrigues(rng.normal(size=3) * rng.choice([0.05, 0.5]))
    t = tp._unit(rng.normal(size=3))
    X = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(4, 8)])
    Y = R @ X + t
    l = (rr.K_LEFT @ (X / X[2]))[:2] + rng.choice([0.0, 0.5, 30.0]) * rng.normal(size=2)
    r = (rr.K_RIGHT @ (Y / Y[2]))[:2] + rng.choice([0.0, 0.5, 30.0]) * rng.normal(size=2)
    return R, t, l, r


def _terms_scale(F, l, r):
    """The size of the terms the residual is the sum of, over sqrt(s): what a relative error of the arithmetic is relative to."""
    x, y = np.array([l[0], l[1], 1.0]), np.array([r[0], r[1], 1.0])
    a, b = F @ x, F.T @ y
    return float(np.abs(y * a).sum() / math.sqrt(a[0] ** 2 + a[1] ** 2 + b[0] ** 2 + b[1] ** 2))


def test_the_hook_is_the_rule(sfm):
    """Residual and Jacobian row within 1e-12, relative to the size of the terms they are sums of (the residual of a good match
    is a difference of numbers a thousand times its size; its own magnitude is no scale for a rounding error)."""
    native = sfm.native
    rng = np.random.default_rng(11)
    worst = [0.0, 0.0]
    for _ in range(1500):
        R, t, l, r = _random_case(rng)
        F, dF, _b1, _b2 = rr.model(R, t)
        want_r, want_J = rr.residuals(F, dF, l[:, None], r[:, None])
        got_r, got_J = native.twoview_refine_test(R, t, rr.K_LEFT, rr.K_RIGHT, l[0], l[1], r[0], r[1])
        scale = _terms_scale(F, l, r)
        worst[0] = max(worst[0], abs(got_r - want_r[0]) / scale)
        worst[1] = max(worst[1], float(np.abs(got_J - want_J[:, 0]).max() / np.abs(want_J[:, 0]).max()))
    print("hook against the reference: residual %.2e, Jacobian %.2e (relative)" % tuple(worst))
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12, worst


def test_the_jacobian_is_the_derivative_of_the_reference():
    """The hook's Jacobian row against central differences of the REFERENCE's residual along the chart.  With h = 1e-6 the
    truncation is h^2 times a third derivative and the rounding eps / h times the terms of the residual: both some 1e-10
    of the row, and the bound is 1e-6 of its largest entry."""
    import importlib
    native = importlib.import_module("structure-from-motion_amd.native")
    rng = np.random.default_rng(12)
    h = 1e-6
    worst = 0.0
    for _ in range(200):
        R, t, l, r = _random_case(rng)
        _F, _dF, b1, b2 = rr.model(R, t)
        _r, J = native.twoview_refine_test(R, t, rr.K_LEFT, rr.K_RIGHT, l[0], l[1], r[0], r[1])
        num = np.zeros(5)
        for j in range(5):
            d = np.zeros(5)
            d[j] = h
            vals = []
            for sign in (1.0, -1.0):
                Rp, tpl = rr.move(R, t, b1, b2, sign * d)
                Fp = rr.model(Rp, tpl)[0]
                vals.append(rr.residuals(Fp, np.zeros((5, 3, 3)), l[:, None], r[:, None])[0][0])
            num[j] = (vals[0] - vals[1]) / (2.0 * h)
        worst = max(worst, float(np.abs(num - J).max() / np.abs(J).max()))
    print("Jacobian against central differences: %.2e of the row" % worst)
    assert worst <= 1e-6


def test_the_hook_on_edge_matches(sfm):
    native = sfm.native
    I, K1 = np.identity(3), np.identity(3)
    R, t = tp.planted("general")
    for l, r in (((np.nan, 1.0), (2.0, 3.0)), ((1.0, 1.0), (2.0, np.inf))):
        res, J = native.twoview_refine_test(R, t, rr.K_LEFT, rr.K_RIGHT, l[0], l[1], r[0], r[1])
        assert math.isnan(res) and np.isnan(J).all()
    # forward motion with identity intrinsics: F = [e2]x, both epipoles at the origin
    forward = np.array([0.0, 0.0, 1.0])
    res, J = native.twoview_refine_test(I, forward, K1, K1, 0.0, 0.0, 0.0, 0.0)            # both keys on their epipoles: s = 0
    assert math.isnan(res) and np.isnan(J).all()
    res, J = native.twoview_refine_test(I, forward, K1, K1, 0.0, 0.0, 0.5, -0.25)          # the left key on its epipole: a = 0
    F, dF, _b1, _b2 = rr.model(I, forward, K1, K1)
    want_r, want_J = rr.residuals(F, dF, np.zeros((2, 1)), np.array([[0.5], [-0.25]]))
    assert res == 0.0 == want_r[0] and np.allclose(J, want_J[:, 0], rtol=1e-12, atol=0.0) and np.isfinite(J).all()
    # the chart: the smallest |t_k| picks e_k, the lowest on a tie
    for t3, k in (((0.6, 0.0, 0.8), 1), ((0.0, 0.0, 1.0), 0), ((1.0, 0.0, 0.0), 1), ((-0.5, 0.5, math.sqrt(0.5)), 0)):
        b1, b2 = rr.basis(np.array(t3))
        e = np.zeros(3)
        e[k] = 1.0
        assert np.allclose(b1, np.cross(t3, e) / np.linalg.norm(np.cross(t3, e))) and abs(b1 @ np.array(t3)) < 1e-15 and abs(b2 @ b1) < 1e-15
        got = native.twoview_refine_test(I, np.array(t3), rr.K_LEFT, rr.K_RIGHT, 100.0, 50.0, 120.0, 40.0)[1]
        Fm, dFm, _1, _2 = rr.model(I, np.array(t3))
        want = rr.residuals(Fm, dFm, np.array([[100.0], [50.0]]), np.array([[120.0], [40.0]]))[1][:, 0]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (t3, got, want)
    bad_k = np.array([[800.0, 0, 320], [1e-3, 800, 240], [0, 0, 1]])
    with pytest.raises(ValueError):
        native.twoview_refine_test(R, t, bad_k, rr.K_RIGHT, 1.0, 1.0, 1.0, 1.0)


# ---- arguments -------------------------------------------------------------------------------------------------------------
def _lib_status(native, n_sets, set_ptr, M, Kl, Kr, lam, iters, max_err2, cos2, dev=False):
    """The status of the library's entry point itself, every array given."""
    lib = native.load()
    set_ptr = None if set_ptr is None else np.ascontiguousarray(set_ptr, dtype=np.int32)
    Kl, Kr = np.ascontiguousarray(Kl, dtype=np.float64).reshape(9), np.ascontiguousarray(Kr, dtype=np.float64).reshape(9)
    m, v = max(int(M), 1), max(n_sets, 1)
    left, right, R, t = np.zeros((2, m)), np.zeros((2, m)), np.zeros((v, 9)), np.ones((v, 3))
    Ro, to = np.zeros((v, 9)), np.zeros((v, 3))
    if dev:                                     # host addresses stand in for device pointers: the call must return before it uses one
        args = [left.ctypes.data, right.ctypes.data, None, R.ctypes.data, t.ctypes.data]
    else:
        args = [native.dptr(left), native.dptr(right), None, native.dptr(R), native.dptr(t)]
    fn = lib.sfm_twoview_refine_dev if dev else lib.sfm_twoview_refine
    outs = [Ro.ctypes.data, to.ctypes.data] if dev else [native.dptr(Ro), native.dptr(to)]
    rc = fn(n_sets, native.iptr(set_ptr), M, *args, native.dptr(Kl), native.dptr(Kr), lam, iters, max_err2, cos2, *outs,
            *([None] * (14 if dev else 13)))
    assert not Ro.any() and not to.any()
    return rc


BAD_K = [np.array([[800.0, 0, 320], [1e-3, 800, 240], [0, 0, 1]]), np.array([[800.0, 0, 320], [0, 800, 240], [1e-9, 0, 1]]),
         np.array([[800.0, 0, 320], [0, 800, 240], [0, 1.0, 1]]), np.array([[800.0, 0, 320], [0, 800, 240], [0, 0, 2.0]]),
         np.array([[np.nan, 0, 320], [0, 800, 240], [0, 0, 1.0]])]


def bad_arguments():
    """(n_sets, set_ptr, M, K_left, K_right, lambda, iters, max_err2, cos2_min) the library refuses, each for one reason."""
    ok = dict(n_sets=2, set_ptr=[0, 3, 5], M=5, Kl=rr.K_LEFT, Kr=rr.K_RIGHT, lam=0.0, iters=6, max_err2=4.0, cos2=rr.COS2_MIN)
    for change in ([dict(set_ptr=p) for p in ([1, 3, 5], [0, 3, 4], [0, 6, 5], None)] + [dict(M=-1), dict(n_sets=-1)] +
                   [dict(cos2=c) for c in (math.nan, -1e-9, 1.0 + 1e-9, math.inf)] + [dict(lam=v) for v in (-1e-9, math.nan)] +
                   [dict(iters=-1)] + [dict(max_err2=v) for v in (-1.0, math.nan)] + [dict(Kl=K) for K in BAD_K] + [dict(Kr=K) for K in BAD_K]):
        args = dict(ok)
        args.update(change)
        yield args


def test_the_library_refuses_bad_arguments_before_it_needs_a_device(sfm):
    native = sfm.native
    n = 0
    for args in bad_arguments():                   # the entry points return before they initialise anything
        for dev in (False, True):
            assert _lib_status(native, dev=dev, **args) == native.E_SHAPE, (dev, args)
            assert "sfm_twoview_refine" in native.last_error()
        n += 1
    assert n == 25
    lib = native.load()
    ptr, K = np.array([0, 0], dtype=np.int32), rr.K_LEFT.reshape(9).copy()
    none = [None] * 13
    assert lib.sfm_twoview_refine(1, native.iptr(ptr), 0, None, None, None, None, None, native.dptr(K), native.dptr(K), 0.0, 6, 4.0, 1.0, None,
                                  None, *none) == native.E_SHAPE                              # R_in, t_in, R_out and t_out are not optional


def test_the_python_layer_refuses_the_same(sfm):
    native = sfm.native
    left = np.zeros((2, 5))
    good = dict(set_ptr=[0, 3, 5], left=left, right=left, R_in=np.zeros((2, 3, 3)), t_in=np.ones((2, 3)), K_left=rr.K_LEFT, K_right=rr.K_RIGHT,
                lam=0.0, iters=6, max_err2=4.0, cos2_min=rr.COS2_MIN)
    bad = [dict(lam=-1.0), dict(lam=math.nan), dict(iters=-1), dict(iters=1.5), dict(max_err2=-1.0), dict(max_err2=math.nan),
           dict(cos2_min=math.nan), dict(cos2_min=-0.1), dict(cos2_min=1.1), dict(K_left=BAD_K[0]), dict(K_right=BAD_K[3]),
           dict(K_left=np.zeros((3, 4))), dict(set_ptr=[1, 3, 5]), dict(set_ptr=[0, 3, 4]), dict(set_ptr=[]), dict(R_in=np.zeros((3, 3, 3))),
           dict(t_in=np.ones((1, 3))), dict(right=np.zeros((2, 4))), dict(mask=np.zeros(4)), dict(outputs=("mask",))]
    for change in bad:
        args = dict(good)
        args.update(change)
        with pytest.raises(ValueError):
            native.twoview_refine(**args)
    for change in bad[:12]:
        args = dict(n_sets=2, R_in=good["R_in"], t_in=good["t_in"], K_left=rr.K_LEFT, K_right=rr.K_RIGHT, lam=0.0, iters=6, max_err2=4.0,
                    cos2_min=rr.COS2_MIN)
        args.update(change)
        with pytest.raises(ValueError):
            native.check_refine(**args)
        args.pop("n_sets"), args.pop("R_in"), args.pop("t_in")
        with pytest.raises(ValueError):
            native.twoview_refine_dev([0, 3, 5], 5, 0, 0, 0, 0, **args)
    assert (native.REFINE_EMPTY, native.REFINE_TOO_FEW, native.REFINE_BAD_POSE, native.REFINE_SINGULAR, native.REFINE_NONFINITE,
            native.REFINE_KEPT_INPUT) == (rr.EMPTY, rr.TOO_FEW, rr.BAD_POSE, rr.SINGULAR, rr.NONFINITE, rr.KEPT_INPUT)
    assert native.REFINE_MIN_USED == rr.MIN_USED and len(native.REFINE_SUMMARY) == 6 and len(native.REFINE_OUTPUTS) == 13
    for name in ("sfm_twoview_refine", "sfm_twoview_refine_dev", "sfm_twoview_refine_test", "sfm_twoview_refine_pairs"):
        assert name in native.EXPORTS
    assert native.load().sfm_version() >= 104
    U = native.info_matrix(np.arange(15.0))
    assert np.array_equal(U, U.T) and np.array_equal(U[0], [0, 1, 2, 3, 4]) and U[1, 1] == 5 and U[4, 4] == 14 and U[2, 3] == 10


# ---- the reference on the scenes of the GPU tests ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,iters,lam", rr.PARITY_CASES)
def test_every_set_of_every_parity_case_is_settled(name, iters, lam, capsys):
    sc, ref = rr.scene_and_reference(name, iters, lam)
    with capsys.disabled():
        print("\n%s, %d iterations, lambda %g: %d sets, %d unsettled, worst d_P %.3e, summary %s, statuses %s"
              % (name, iters, lam, sc.counts.size, int((~ref.settled).sum()), ref.d_P.max(initial=0.0), ref.summary.tolist(),
                 np.flatnonzero(np.bincount(ref.status, minlength=64)).tolist()))
    assert ref.settled.all(), np.flatnonzero(~ref.settled)
    assert np.all(100.0 * ref.d_P <= 1e-6), float(ref.d_P.max())
    assert np.all(ref.d_cost <= 1e-9)
    for s, q in enumerate(ref.sets):
        if not q.status & rr.BAD_POSE and not q.status & rr.KEPT_INPUT:
            assert abs(np.linalg.norm(q.t) - 1.0) <= 1e-15 and abs(np.linalg.norm(q.other.t) - 1.0) <= 1e-15
        if sc.names[s] != "rotation":       # the points of a camera that only rotated are not determined (see _twoview_pose_reference)
            assert q.d_X <= max(1e-9, 100.0 * q.d_P), (s, q.d_X)
    assert ref.summary[0] + ref.summary[1] + ref.summary[2] == sc.counts.size
    assert ref.summary[4] + ref.summary[5] == ref.n_used[(ref.status & (rr.BAD_POSE | rr.EMPTY | rr.TOO_FEW)) == 0].sum()


def test_the_scenes_are_what_they_say():
    sc, ref = rr.scene_and_reference("sizes")
    assert sc.counts.tolist() == list(rr.SIZES)
    few = ref.n_used < rr.MIN_USED
    assert np.array_equal(few, sc.counts < 8) and np.all(ref.status[few] & rr.TOO_FEW) and np.all(ref.status[few] & rr.KEPT_INPUT)
    assert ref.n_used[sc.counts.tolist().index(8)] == 8 and ref.status[sc.counts.tolist().index(8)] == 0    # eight matches are enough
    assert ref.status[0] == rr.EMPTY | rr.TOO_FEW | rr.KEPT_INPUT and not ref.cost[:, few].any() and not ref.info[few].any()
    sc, ref = rr.scene_and_reference("many")
    assert sc.counts.size == 259 and set(sc.names) == set(tp.FAMILIES) and sc.displaced.any()
    assert ref.summary[0] > 100 and ref.summary[2] > 100 and ref.summary[3] >= 1        # a small set whose iteration the guard rejects occurs
    kept = [s for s in range(259) if ref.status[s] == rr.KEPT_INPUT]
    assert kept and all(ref.sets[s].ratio > 1.0 + 1e-3 for s in kept)
    assert all(np.array_equal(ref.R[s], sc.R_in[s]) and np.array_equal(ref.t[s], sc.t_in[s]) and ref.cost[0, s] == ref.cost[1, s] for s in kept)
    sc, ref = rr.scene_and_reference("special")
    by = {name: s for s, name in enumerate(sc.names)}
    assert ref.status[by["masked_out"]] == rr.EMPTY | rr.TOO_FEW | rr.KEPT_INPUT
    for name in ("zero_pose", "nan_pose", "no_winner"):
        s = by[name]
        lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
        assert ref.status[s] == rr.BAD_POSE | rr.KEPT_INPUT and not ref.F[s].any() and np.isnan(ref.res[lo:hi]).all(), name
        assert not ref.inlier[lo:hi].any() and not ref.front[lo:hi].any() and ref.n_used[s] == 70
    # a NaN coordinate: that match is not selected and has no residual, the rest of the set is refined
    s, clean = by["nan_coordinate"], by["clean_general"]
    lo = sc.set_ptr[s]
    assert ref.n_used[s] == 68 and ref.status[s] == 0 and np.flatnonzero(np.isnan(ref.res[lo:lo + 70])).tolist() == [17, 40]
    assert ref.n_used[clean] == 70 and tp.pose_distance(ref.R[s], ref.t[s], ref.R[clean], ref.t[clean]) < 1e-2
    # the masked matches of a displaced scene are judged all the same: they are no inliers
    sc, ref = rr.scene_and_reference("general_displaced")
    assert not ref.inlier[sc.displaced].any() and ref.inlier[~sc.displaced].all() and np.isfinite(ref.res).all()
    sc, ref = rr.scene_and_reference("behind")
    assert not ref.front.any() and ref.summary[0] == 3 and ref.inlier.all()
    # iters = 0 is a pure evaluation
    sc, ref = rr.scene_and_reference("general_displaced", 0, 0.0)
    assert np.array_equal(ref.R, sc.R_in) and np.array_equal(ref.t, sc.t_in) and np.array_equal(ref.cost[0], ref.cost[1])
    assert np.all(ref.status == rr.KEPT_INPUT) and ref.info.any()


@pytest.mark.parametrize("name", ["general", "general_displaced", "forward", "forward_displaced", "plane", "plane_displaced"])
def test_six_steps_reach_the_minimum(name):
    """The reference's gradient at its output is at most 1e-6 of its gradient at the start, and the cost falls to the key noise."""
    sc, ref = rr.scene_and_reference(name)
    for s, q in enumerate(ref.sets):
        assert q.status == 0 and q.grad[1] <= 1e-6 * q.grad[0], (s, q.grad)
        rms = math.sqrt(q.cost[1] / q.n_used)
        assert 0.5 * tp.NOISE_PX < rms < 1.5 * tp.NOISE_PX and q.cost[1] < 0.07 * q.cost[0], (s, rms)   # the Sampson distance of a noisy match has the deviation of one key coordinate


@pytest.mark.parametrize("name", ["general_displaced", "plane", "forward", "sizes"])
def test_twenty_steps_reach_a_fixed_point(name):
    """What tests/test_gpu_twoview_refine.py asks of a second refinement holds for the rule itself: after twenty steps six more
    move the pose by less than 1e-12 and the guard lets it stand; after six steps forward motion is still 1e-7 away."""
    sc = rr.scene(name)
    first = rr.reference(sc.set_ptr, sc.left, sc.right, sc.mask, sc.R_in, sc.t_in, iters=20)
    again = rr.reference(sc.set_ptr, sc.left, sc.right, sc.mask, first.R, first.t)
    done = (first.status & (rr.TOO_FEW | rr.BAD_POSE)) == 0
    assert done.any() and not first.status[done].any() and not again.status[done].any()
    assert max(np.abs(again.R - first.R).max(), np.abs(again.t - first.t).max()) < 1e-12
    if name == "forward":
        six = rr.scene_and_reference(name)[1]
        more = rr.reference(sc.set_ptr, sc.left, sc.right, sc.mask, six.R, six.t)
        assert 1e-9 < max(np.abs(more.R - six.R).max(), np.abs(more.t - six.t).max()) < 1e-5


def test_the_baseline_direction_improves():
    """Against the planted pose the median error of the baseline direction over the general sets is lower after than before."""
    before, after = [], []
    for name in ("general", "general_displaced", "sizes", "many"):
        sc, ref = rr.scene_and_reference(name)
        for s, q in enumerate(ref.sets):
            if sc.names[s] == "general" and q.status == 0:
                t0 = tp.planted("general")[1]
                before.append(rr.baseline_angle_deg(sc.t_in[s], t0))
                after.append(rr.baseline_angle_deg(q.t, t0))
    print("baseline direction over %d general sets: median %.3f deg before, %.3f deg after" % (len(before), np.median(before), np.median(after)))
    assert len(before) > 30 and np.median(after) < np.median(before)


def test_a_camera_that_only_rotated_has_no_baseline_to_find():
    """Without a baseline the translation is not determined: the iteration lowers the cost and ends far from where it began in t,
    which is why initialise_pairs leaves such a set unrefined."""
    sc, ref = rr.scene_and_reference("rotation")
    for s, q in enumerate(ref.sets):
        assert q.status == 0 and q.cost[1] < q.cost[0] and abs(np.linalg.norm(q.t) - 1.0) <= 1e-15
    assert max(rr.baseline_angle_deg(q.t, sc.t_in[s]) for s, q in enumerate(ref.sets)) > 10.0
