"""The robust-loss reference and the argument checks of the loss, without a device."""
import numpy as np
import pytest

import _robust_reference as rr


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _scene(sfm):
    """3 cameras, 20 points, every fourth observation displaced by about ten times the noise of the initial state."""
    sc = sfm.scenes.make_scene(3, 20, 1.0, seed=33)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic).copy()
    rng = np.random.default_rng(2)
    hit = np.arange(0, uvn.shape[1], 4)
    uvn[:, hit] += rng.normal(0.0, 0.05, (2, hit.shape[0]))
    cams = sc.cams_init.copy()
    cams[:, 3:7] /= np.linalg.norm(cams[:, 3:7], axis=1)[:, None]
    return sc, uvn, cams


def test_no_loss_is_the_oracle(sfm, oracle):
    sc, uvn, cams = _scene(sfm)
    trace = []
    got_c, got_p, costs = rr.ba_robust(cams, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 0.5, 4, rr.LOSS_NONE, 1.0, trace)
    want = []
    want_c, want_p = oracle.ba_sparse(cams, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 0.5, 4, trace=want)
    assert rel(got_c, want_c) < 1e-14 and rel(got_p, want_p) < 1e-14
    assert all(rel(a[0], b[0]) < 1e-14 and rel(a[1], b[1]) < 1e-14 for a, b in zip(trace, want))
    r = oracle.obs_terms_vec(cams, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn)[0]
    assert abs(costs[0] - np.sum(r * r)) <= 1e-14 * np.sum(r * r)


def test_loss_terms_values():
    r = np.array([[0.0, 0.0], [0.3, 0.4], [3.0, 4.0], [0.6, 0.8]])          # |r|^2 = 0, 0.25, 25, 1
    s, w, rho = rr.loss_terms(rr.LOSS_HUBER, 1.0, r)
    assert np.allclose(s, [0, 0.25, 25, 1], rtol=1e-15) and np.allclose(w, [1, 1, 0.2, 1], rtol=1e-15)
    assert np.allclose(rho, [0, 0.25, 9, 1], rtol=1e-15)
    s, w, rho = rr.loss_terms(rr.LOSS_CAUCHY, 0.5, r)
    assert np.allclose(s, [0, 1, 100, 4], rtol=1e-15) and np.allclose(w, [1, 0.5, 1 / 101, 0.2], rtol=1e-15)
    assert np.allclose(rho, np.log1p([0, 1, 100, 4]), rtol=1e-15)
    s, w, rho = rr.loss_terms(rr.LOSS_NONE, 7.0, r)
    assert np.array_equal(s, rho) and np.all(w == 1.0) and np.allclose(s, [0, 0.25, 25, 1], rtol=1e-15)


@pytest.mark.parametrize("kind", [rr.LOSS_HUBER, rr.LOSS_CAUCHY])
def test_weighted_rhs_is_the_gradient_of_the_robust_cost(sfm, oracle, kind):
    """-1/2 dC/dtheta = sum_o w_o J_o^T r_o for C = delta^2 sum rho(s): the right-hand sides of the reweighted normal
    equations (``ep`` per camera, ``ex`` per point) against a central difference of the cost, 1e-6 relative to the largest
    entry.  Taken with the Jacobian the code documents as the true one (no quirk bits; Q2 is a sign error of the
    reference's) and over the parameters the cost is a plain function of: the camera centres and the points.  (The
    quaternion columns differentiate through the re-derived canonical quaternion, not through the stored one.)"""
    sc, uvn, cams = _scene(sfm)
    pts = sc.pts_init.copy()
    r0 = oracle.obs_terms_vec(cams, pts, sc.cam_idx, sc.pt_idx, uvn, 0)[0]
    delta = float(np.sqrt(np.median(np.sum(r0 * r0, axis=1))))
    s = rr.loss_terms(kind, delta, r0)[0]
    assert np.count_nonzero(s > 1.0) >= 10 and np.count_nonzero(s < 1.0) >= 10      # both zones of the loss are exercised
    t = rr.reduced_system(cams, pts, sc.cam_idx, sc.pt_idx, uvn, 0.5, kind, delta, quirks=0)

    def c(cams_, pts_):
        return rr.cost(kind, delta, oracle.obs_terms_vec(cams_, pts_, sc.cam_idx, sc.pt_idx, uvn, 0)[0])

    h = 1e-6
    g_cam = np.zeros((sc.n_cams, 3))
    for v in range(sc.n_cams):
        for k in range(3):
            a, b = cams.copy(), cams.copy()
            a[v, k] += h; b[v, k] -= h
            g_cam[v, k] = (c(a, pts) - c(b, pts)) / (2 * h)
    g_pt = np.zeros((sc.n_pts, 3))
    for p in range(sc.n_pts):
        for k in range(3):
            a, b = pts.copy(), pts.copy()
            a[k, p] += h; b[k, p] -= h
            g_pt[p, k] = (c(cams, a) - c(cams, b)) / (2 * h)
    assert rel(t["ep"][:, 0:3], -0.5 * g_cam) < 1e-6
    assert rel(t["ex"], -0.5 * g_pt) < 1e-6


def test_check_loss_rejects_bad_arguments(sfm):
    native = sfm.native
    for kind in (-1, 3, 7, 1.5, "tukey", True):
        with pytest.raises(ValueError):
            native.check_loss(kind, 1.0)
    for delta in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        for kind in (native.LOSS_HUBER, native.LOSS_CAUCHY):
            with pytest.raises(ValueError):
                native.check_loss(kind, delta)
    assert native.check_loss(native.LOSS_NONE, float("nan")) == (native.LOSS_NONE, 1.0)      # delta is ignored
    assert native.check_loss(native.LOSS_HUBER, 0.25) == (native.LOSS_HUBER, 0.25)
    assert native.check_loss("cauchy", 2) == (native.LOSS_CAUCHY, 2.0)
    assert (native.LOSS_NONE, native.LOSS_HUBER, native.LOSS_CAUCHY) == (0, 1, 2)


class _Holder:
    pass


class _View:
    def __init__(self, k):
        self.k = k


def _processor(sfm, ks):
    vp, kt, tp = _Holder(), _Holder(), _Holder()
    vp.view_list = [_View(k) for k in ks]
    return sfm.processors.HipBaProcessor(vp, kt, None, tp, None, iteration=10, damping_factor=0.5)


def test_ba_loss_needs_one_focal_scale(sfm):
    k = np.array([[500.0, 0.0, 320.0], [0.0, 720.0, 240.0], [0.0, 0.0, 1.0]])
    bp = _processor(sfm, [k, k.copy(), k.copy()])
    assert bp.ba_loss is None and bp.ba_loss_native() is None
    bp.ba_loss = ("huber", 5.0)
    kind, delta = bp.ba_loss_native()
    assert kind == sfm.native.LOSS_HUBER and delta == 5.0 / np.sqrt(500.0 * 720.0)
    bp.ba_loss = ("cauchy", 10.0)
    assert bp.ba_loss_native() == (sfm.native.LOSS_CAUCHY, 10.0 / np.sqrt(500.0 * 720.0))
    k2 = k.copy()
    k2[0, 0] *= 1.0 + 1e-9
    bp = _processor(sfm, [k, k2, k])
    bp.ba_loss = ("huber", 5.0)
    with pytest.raises(ValueError):
        bp.ba_loss_native()
    with pytest.raises(ValueError):
        bp.execute_bundle_adjustment()          # refused before anything is read or uploaded
    for bad in (("tukey", 5.0), ("huber", 0.0), ("huber", float("nan")), "huber", ("huber",), (1, 5.0)):
        bp = _processor(sfm, [k, k])
        bp.ba_loss = bad
        with pytest.raises(ValueError):
            bp.ba_loss_native()
    bp = _processor(sfm, [k, k])
    bp.ba_loss, bp.ba_resident = ("huber", 5.0), False
    with pytest.raises(TypeError):
        bp.ba_loss_native()
