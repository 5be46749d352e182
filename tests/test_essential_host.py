"""Host tests of the robust essential matrix (no GPU): the sampler and the minimal solver of the library on the host
(sfm_essential_sample, sfm_essential_solve: the function the hypothesis kernel runs) against tests/_essential_reference.py,
the argument checks of the library and of native.check_essential, the condition that every set of every parity case of
tests/test_gpu_essential.py is settled, and what the five-point hypotheses buy against the eight-point ones.

The canonical sign of step 5 (the entry of largest magnitude positive) is a tie for the planted motions of `forward`
(|E01| = |E10| = cos 0.05) and `sideways` (|E12| = |E21| = 1): rounding decides it, so the planted matrix is compared up to
sign, and the ORDER of the solutions is compared on the samples whose reference is itself settled (both routes agree on
number and order, keys at least 1e-6 apart) -- every family but those two has such samples, which the test checks."""
import math

import numpy as np
import pytest

import _essential_reference as er
import _twoview_ransac_reference as tv

SOLVE_SAMPLES = [(name, 40 + 7 * k, seed) for name in er.FAMILIES for k, seed in enumerate((1, 2, 3, 4))]


def _routes(a, b):
    return er.solve_one(a, b, 0), er.solve_one(a, b, 1)


def _route_difference(r0, r1):
    """The reference's own two-route difference of one sample's solutions, matched by nearest (up to sign)."""
    if len(r0) != len(r1) or len(r0) == 0:
        return math.inf
    return max(min(min(np.abs(e - f).max(), np.abs(e + f).max()) for f in r1) for e in r0)


# ---- the sampler -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 7, 64, 5000])
@pytest.mark.parametrize("max_hyp", [1, 1000])
def test_the_sampler_is_the_rule(sfm, n, max_hyp):
    native = sfm.native
    want = er.sample_indices(n, max_hyp)
    for h in range(max_hyp):
        H, idx = native.essential_sample(n, max_hyp, h)
        assert H == max_hyp and list(idx) == want[h].tolist(), (n, h)
        lo, hi = np.arange(5) * n // 5, np.arange(1, 6) * n // 5
        assert all(lo[k] <= idx[k] < hi[k] for k in range(5))
    assert native.essential_sample(n, max_hyp, max_hyp) == (max_hyp, (-1,) * 5) and native.essential_sample(n, max_hyp, -1)[1] == (-1,) * 5


def test_the_sampler_refuses(sfm):
    native = sfm.native
    assert native.essential_sample(5, 128, 0) == (0, (-1,) * 5) and native.essential_sample(64, 65537, 0)[0] == 0
    assert native.essential_sample(64, -1, 0)[0] == 0 and native.essential_sample(64, 0, 127)[0] == er.HYP_DEFAULT == 128
    assert er.hypothesis_count(5, 128) == 0 and er.hypothesis_count(6, 0) == 128


# ---- the solver --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,seed", SOLVE_SAMPLES)
def test_the_solver_on_noise_free_samples(sfm, name, n, seed):
    a, b, E_true = er.sample_of(name, n, seed)
    E = sfm.native.essential_solve(a, b)
    r0, r1 = _routes(a, b)
    d = _route_difference(r0, r1)
    bound = max(1e-9, 100.0 * d)
    assert math.isfinite(d) and 1 <= len(E) <= er.MAX_SOL and len(E) == len(r0) == len(r1)
    found = min(min(np.abs(e - E_true).max(), np.abs(e + E_true).max()) for e in E)
    print("%s n=%d seed=%d: %d solutions, planted within %.2e, routes %.2e apart" % (name, n, seed, len(E), found, d))
    assert found <= bound
    A, B = np.hstack((a, np.ones((5, 1)))), np.hstack((b, np.ones((5, 1))))
    for e in E:
        sv = np.linalg.svd(e)[1]
        assert abs(np.linalg.norm(e) - 1.0) < 1e-14 and e.max() >= np.abs(e).max() * (1.0 - 4e-16)
        assert abs(sv[0] - sv[1]) <= bound and sv[2] <= bound and np.abs(np.einsum("ki,ij,kj->k", B, e, A)).max() <= bound
    assert np.all(np.diff(E[:, 0, 0]) >= 0)
    if name not in ("forward", "sideways"):      # (see the module's docstring)
        keys = r0[:, 0, 0]
        settled = np.abs(r0 - r1).max() <= 1e-6 and (len(keys) < 2 or np.diff(keys).min() >= er.KEY_GAP)
        assert settled, "choose another sample: the reference's routes do not agree on the order of this one"
        assert np.abs(E - r0).max() <= bound


def test_degenerate_samples(sfm):
    native = sfm.native
    rng = np.random.default_rng(3)
    same = np.tile([[0.1, -0.2]], (5, 1))
    assert native.essential_solve(same, np.tile([[0.3, 0.05]], (5, 1))).shape == (0, 3, 3)       # five identical matches: a rank-1 system
    a = rng.uniform(-0.4, 0.4, (5, 2))
    Ra = (tv._rot_y(0.1) @ np.vstack((a.T, np.ones(5)))).T
    t = np.linspace(-0.4, 0.4, 5)
    line_a, line_b = np.stack((t, 0.5 * t + 0.1), axis=1), np.stack((t + 0.05, 0.5 * t + 0.12), axis=1)
    with_inf = a.copy()
    with_inf[1, 1] = np.inf
    for name, x, y in (("pure rotation", a, Ra[:, :2] / Ra[:, 2:3]), ("collinear", line_a, line_b), ("nan", a * np.nan, a),
                       ("inf", a, with_inf)):
        E = native.essential_solve(x, y)
        A, B = np.hstack((x, np.ones((5, 1)))), np.hstack((y, np.ones((5, 1))))
        assert E.shape[1:] == (3, 3) and len(E) <= er.MAX_SOL and np.isfinite(E).all(), name
        for e in E:                                  # whatever is returned is a canonical matrix that explains the five matches
            assert abs(np.linalg.norm(e) - 1.0) < 1e-14 and e.max() >= np.abs(e).max() * (1.0 - 4e-16), name
            assert np.abs(np.einsum("ki,ij,kj->k", B, e, A)).max() < 1e-6, name
        assert np.all(np.diff(E[:, 0, 0]) >= 0), name
    with pytest.raises(ValueError):
        native.essential_solve(np.zeros((4, 2)), np.zeros((5, 2)))
    lib = native.load()
    assert lib.sfm_essential_solve(None, None, None, None) == native.E_SHAPE and "sfm_essential_solve" in native.last_error()


# ---- arguments ---------------------------------------------------------------------------------------------------------------
BAD_K = [np.array([[800.0, 0, 320], [1e-3, 800, 240], [0, 0, 1]]), np.array([[800.0, 0, 320], [0, 800, 240], [0, 1e-9, 1]]),
         np.array([[800.0, 0, 320], [0, 800, 240], [0, 0, 2]]), np.array([[np.nan, 0, 320], [0, 800, 240], [0, 0, 1]]),
         np.array([[800.0, 0, np.inf], [0, 800, 240], [0, 0, 1]])]


def bad_arguments():
    ok = dict(ptr=[0, 3, 6], n_sets=2, M=6, max_err2=4.0, max_hyp=128, Kl=er.K, Kr=er.K)
    for change in ([dict(max_err2=v) for v in (-1.0, math.nan)] + [dict(max_hyp=v) for v in (-1, 65537)] +
                   [dict(ptr=[1, 3, 6]), dict(ptr=[0, 4, 3, 6], n_sets=3), dict(ptr=[0, 3, 5]), dict(n_sets=-1), dict(M=-1), dict(M=1 << 31)] +
                   [dict(Kl=Km) for Km in BAD_K] + [dict(Kr=Km) for Km in BAD_K]):
        args = dict(ok)
        args.update(change)
        yield args


def _lib_status(native, dev, ptr, n_sets, M, max_err2, max_hyp, Kl, Kr):
    lib = native.load()
    ptr = np.ascontiguousarray(ptr, dtype=np.int32)
    Kl, Kr = np.ascontiguousarray(Kl, dtype=np.float64).reshape(9), np.ascontiguousarray(Kr, dtype=np.float64).reshape(9)
    pts, E = np.zeros((2, 6)), np.full(9, 7.0)
    if dev:       # the pointers are never followed: the call returns before it needs a device
        status = lib.sfm_essential_ransac_dev(n_sets, native.iptr(ptr), M, None, None, native.dptr(Kl), native.dptr(Kr), max_err2, max_hyp,
                                              None, None, None, None, None, None, None, None, None, None)
    else:
        status = lib.sfm_essential_ransac(n_sets, native.iptr(ptr), M, native.dptr(pts), native.dptr(pts), native.dptr(Kl), native.dptr(Kr),
                                          max_err2, max_hyp, native.dptr(E), None, None, None, None, None, None, None, None)
    assert np.all(E == 7.0)
    return status


def test_the_library_refuses_bad_arguments_before_it_needs_a_device(sfm):
    native = sfm.native
    n = 0
    for args in bad_arguments():
        for dev in (False, True):
            assert _lib_status(native, dev, **args) == native.E_SHAPE, (dev, args)
            assert "sfm_essential_ransac" in native.last_error()
        n += 1
    assert n == 20


def test_the_python_layer_refuses_the_same(sfm):
    native = sfm.native
    pts = np.zeros((2, 6))
    good = dict(set_ptr=[0, 3, 6], left=pts, right=pts, K_left=er.K, K_right=er.K, max_err2=4.0, max_hyp=128)
    bad = [dict(max_err2=-1.0), dict(max_err2=math.nan), dict(max_hyp=-1), dict(max_hyp=65537), dict(max_hyp=1.5), dict(K_left=BAD_K[0]),
           dict(K_right=BAD_K[2]), dict(K_left=BAD_K[3]), dict(K_right=np.zeros((3, 4))), dict(set_ptr=[1, 3, 6]), dict(set_ptr=[0, 4, 3, 6]),
           dict(set_ptr=[0, 3, 5]), dict(set_ptr=[]), dict(right=np.zeros((2, 5))), dict(left=np.zeros((3, 6)))]
    for change in bad:
        args = dict(good)
        args.update(change)
        with pytest.raises(ValueError):
            native.check_essential(**args)
        with pytest.raises(ValueError):
            native.essential_ransac(**args)
    for change in bad[:9]:
        args = dict(K_left=er.K, K_right=er.K, max_err2=4.0, max_hyp=128)
        args.update(change)
        with pytest.raises(ValueError):
            native.essential_ransac_dev([0, 3, 6], 6, 0, 0, **args)
    with pytest.raises(ValueError):
        native.essential_ransac(outputs=("mask",), **good)
    set_ptr, left, right, Kl, Kr, max_err2, max_hyp = native.check_essential(**good)
    assert set_ptr.dtype == np.int32 and Kl.shape == Kr.shape == (9,) and (max_err2, max_hyp) == (4.0, 128)
    assert (native.ESSENTIAL_TOO_FEW, native.ESSENTIAL_NO_MODEL) == (er.TOO_FEW, er.NO_MODEL)
    assert (native.ESSENTIAL_MIN_MATCHES, native.ESSENTIAL_MAX_SOLUTIONS, native.ESSENTIAL_DEFAULT_HYP) == (er.MIN_MATCHES, er.MAX_SOL, er.HYP_DEFAULT)
    assert len(native.ESSENTIAL_SUMMARY) == 6 and len(native.ESSENTIAL_OUTPUTS) == 8
    for name in ("sfm_essential_ransac", "sfm_essential_ransac_dev", "sfm_essential_sample", "sfm_essential_solve"):
        assert name in native.EXPORTS
    assert native.load().sfm_version() >= 105


# ---- the reference on the scenes of the GPU tests ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.CASES, ids=lambda c: "%s-%g-%d" % c)
def test_every_set_of_every_parity_case_is_settled(case, capsys):
    sc, Km, ref = er.case_reference(case)
    with capsys.disabled():
        print("\n%s/%g/%d: %d sets, %d solved, %d without a model, %d too few; d_E <= %.2e, d_G <= %.2e"
              % (case + (sc.counts.size,) + tuple(ref.summary[:3]) + (ref.d_E.max(initial=0.0), ref.d_G.max(initial=0.0))))
    assert ref.settled.all(), np.flatnonzero(~ref.settled)
    assert ref.summary[2] == (sc.counts < er.MIN_MATCHES).sum() and ref.summary[:3].sum() == sc.counts.size


def test_the_scenes_are_what_they_say():
    sc, Km, ref = er.case_reference(("paths", er.MAX_ERR2, 128))
    assert sc.counts.tolist() == list(er.PATHS_COUNTS) and (ref.status[sc.counts >= 15] == 0).all()
    many = er.scene("many_sets")
    assert many.counts.size == 259 and many.counts[0] == 0 and many.counts[-1] == 5
    sc, Km, ref = er.case_reference(("ties", er.EVERYONE, er.TIES_HYP))
    assert ref.inlier.all() and (ref.best_root == 0).all() and (ref.status == 0).all()
    for name in er.FAMILIES:                   # every family is solved at every size
        sc, Km, ref = er.case_reference((name, er.family_err2(name), 128))
        assert (ref.status == 0).all() and sc.counts.tolist() == list(er.FAMILY_COUNTS), name


# ---- what five points buy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.5, 0.6])
def test_outlier_tolerance_against_the_eight_point_reference(frac):
    """At 128 hypotheses, 2 px and no refit: a clean sample of five has probability (1 - frac)^5 = 3.1 % / 1.0 %, one of eight
    0.4 % / 0.07 %.  The five-point reference keeps at least 0.95 of the clean matches where the eight-point one keeps at most
    half."""
    l, r, bad = tv.two_views(2000, 1, frac=frac)
    five = er.solve_set(l, r, er.K, er.K, er.MAX_ERR2, 128)
    eight = tv.solve_set(l, r, tv.MAX_ERR2, 128, 0)
    clean = int((~bad).sum())
    kept5, kept8 = int((five.mask & ~bad).sum()), int((eight.mask & ~bad).sum())
    print("frac %.1f: five-point keeps %d of %d clean matches, eight-point %d" % (frac, kept5, clean, kept8))
    assert five.status == 0 and kept5 >= 0.95 * clean and kept8 <= 0.5 * clean
