"""Robust losses of the resident bundle adjustment (sfm_ba_set_loss) against the NumPy reference of
tests/_robust_reference.py: per-observation terms, the reduced system on every linearisation path, whole iterations in
every launch configuration, the life of the setting across growth and culls, and the drop-in's ``ba_loss``.

Bounds: 1e-9 relative to the largest entry of the reference, the bound of the plain-loss parity tests -- the loss adds a
square root, a division and (Cauchy) a log1p per observation, each correct to a few ulp, in front of the same sums."""
import numpy as np
import pytest

import _robust_reference as rr
import _screen_reference as sr
import _tracks_reference as tr

pytestmark = pytest.mark.gpu

LAM = 0.5
_CACHE = {}


def rel(a, b):
    b = np.asarray(b)
    scale = np.max(np.abs(b)) if b.size else 1.0
    return float(np.max(np.abs(np.asarray(a) - b)) / (scale if scale > 0 else 1.0)) if b.size else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _outlier(sfm):
    """The outlier scene with normalised keys, the start state of the issue's measurement (cams_init with unit
    quaternions, pts_init), the focal scale and the two deltas (Huber 5 px, Cauchy 10 px)."""
    if "outlier" not in _CACHE:
        o = sr.outlier_scene(sfm)
        sc = o.scene
        uvn = sfm.geometry.normalise_pixels(o.uv_pix, sc.intrinsic)
        cams0 = sc.cams_init.copy()
        cams0[:, 3:7] /= np.linalg.norm(cams0[:, 3:7], axis=1)[:, None]
        scale = float(np.sqrt(abs(sc.intrinsic[0, 0] * sc.intrinsic[1, 1])))
        for a in (uvn, cams0):
            a.setflags(write=False)
        _CACHE["outlier"] = (o, sc, uvn, cams0, scale, {rr.LOSS_HUBER: 5.0 / scale, rr.LOSS_CAUCHY: 10.0 / scale})
    return _CACHE["outlier"]


def _outlier_run(sfm, kind):
    """20 reference iterations on the outlier scene, once per loss: (trace of states, costs)."""
    key = ("outlier_run", kind)
    if key not in _CACHE:
        _o, sc, uvn, cams0, _scale, deltas = _outlier(sfm)
        trace = []
        _c, _p, costs = rr.ba_robust(cams0, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, LAM, 20, kind, deltas.get(kind, 1.0), trace)
        _CACHE[key] = (trace, costs)
    return _CACHE[key]


def _ragged(sfm, oracle):
    """The ragged scene at (cams_true, x_init), its point index per observation, the squared residuals there and a delta
    in the widest gap around their median."""
    if "ragged" not in _CACHE:
        rs = tr.ragged_scene(sfm)
        pt_of = np.repeat(np.arange(rs.n_pts), np.diff(rs.pt_ptr)).astype(np.int32)
        r = oracle.obs_terms_vec(rs.scene.cams_true, rs.x_init[0:3], rs.cam_idx, pt_of, rs.uv)[0]
        err2 = np.sum(r * r, axis=1)
        delta = float(np.sqrt(sr.threshold_in_gap(err2, 0.5)))
        _CACHE["ragged"] = (rs, pt_of, r, delta)
    return _CACHE["ragged"]


def _ragged_run(sfm, oracle, kind):
    key = ("ragged_run", kind)
    if key not in _CACHE:
        rs, pt_of, _r, delta = _ragged(sfm, oracle)
        _CACHE[key] = rr.ba_robust(rs.scene.cams_true, rs.x_init[0:3], rs.cam_idx, pt_of, rs.uv, LAM, 3, kind, delta)
    return _CACHE[key]


LOSSES = [rr.LOSS_HUBER, rr.LOSS_CAUCHY]


# ---- 1 ------------------------------------------------------------------------------------------------------------
def test_terms_against_the_reference(hip, sfm, oracle):
    rs, _pt_of, r, delta = _ragged(sfm, oracle)
    s_ref = rr.loss_terms(rr.LOSS_HUBER, delta, r)[0]
    m = s_ref.shape[0]
    assert m == 2667 and np.count_nonzero(s_ref > 1.0) >= 0.2 * m and np.count_nonzero(s_ref < 1.0) >= 0.2 * m
    with hip.BaProblem(rs.scene.n_cams, rs.pt_ptr, rs.cam_idx, rs.uv) as prob:
        prob.set_state(rs.scene.cams_true, rs.x_init[0:3])
        assert prob.loss()[0] == hip.LOSS_NONE
        s, w, rho = prob.loss_terms()
        e = np.sum(r * r, axis=1)
        assert np.all(w == 1.0) and rel(s, e) < 1e-9 and same_bits(s, rho)
        for kind in LOSSES:
            prob.set_loss(kind, delta)
            assert prob.loss() == (kind, delta)
            want = rr.loss_terms(kind, delta, r)
            got = prob.loss_terms()
            for g, t, name in zip(got, want, "swr"):
                assert rel(g, t) < 1e-9, (kind, name, rel(g, t))
        inside = s_ref < 1.0 - 1e-9
        prob.set_loss(hip.LOSS_HUBER, delta)
        assert np.all(prob.loss_terms()[1][inside] == 1.0)          # the quadratic zone is exactly unweighted
        state = prob.get_state()
        prob.loss_terms()
        assert all(same_bits(a, b) for a, b in zip(prob.get_state(), state))


# ---- 2 ------------------------------------------------------------------------------------------------------------
def test_zero_residual(hip):
    cams = np.array([[0.0, 0, 0, 1, 0, 0, 0], [1.0, 0, 0, 1, 0, 0, 0]])
    pts = np.array([[0.0], [0.0], [5.0]])
    uv = np.array([[0.0, -0.19], [0.0, 0.01]])          # camera 0 sees the point exactly where it is
    for kind in LOSSES:
        with hip.BaProblem(2, np.array([0, 2]), np.array([0, 1]), uv) as prob:
            prob.set_state(cams, pts)
            prob.set_loss(kind, 0.01)
            s, w, rho = prob.loss_terms()
            assert s[0] == 0.0 and w[0] == 1.0 and rho[0] == 0.0
            assert s[1] > 1.0 and 0.0 < w[1] < 1.0 and rho[1] > 0.0
            prob.iterate(LAM, 2)
            c, p = prob.get_state()
            assert np.all(np.isfinite(c)) and np.all(np.isfinite(p)) and np.all(np.isfinite(prob.get_stats()))
            assert all(np.all(np.isfinite(t)) for t in prob.loss_terms())


# ---- 3 ------------------------------------------------------------------------------------------------------------
def _check_reduced(hip, sc, uvn, cams, pts, kind, delta, mode):
    want = rr.reduced_system(cams, pts, sc.cam_idx, sc.pt_idx, uvn, LAM, kind, delta)
    S, rhs = hip.ba_reduced_system(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn, cams, pts, LAM, schur_mode=mode, loss=(kind, delta))
    assert rel(S, want["S"]) < 1e-9 and rel(rhs, want["rhs"]) < 1e-9, (kind, mode, rel(S, want["S"]), rel(rhs, want["rhs"]))


@pytest.mark.parametrize("kind", LOSSES)
def test_reduced_system_on_the_outlier_scene(hip, sfm, kind):
    _o, sc, uvn, cams0, _scale, deltas = _outlier(sfm)
    assert 8 * sc.n_cams * (19 + 35) <= 64 * 1024          # cameras and accumulators in LDS (mode 2)
    for mode in (hip.SCHUR_PAIRS, hip.SCHUR_MFMA, hip.SCHUR_ROWS):
        _check_reduced(hip, sc, uvn, cams0, sc.pts_init, kind, deltas[kind], mode)
    # ... and it is the plain system when no loss is given
    plain = hip.ba_reduced_system(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn, cams0, sc.pts_init, LAM)
    none = hip.ba_reduced_system(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn, cams0, sc.pts_init, LAM, loss=(hip.LOSS_NONE, 1.0))
    assert rel(none[0], plain[0]) < 1e-12 and rel(none[1], plain[1]) < 1e-12


@pytest.mark.parametrize("n_cams,lds_mode", [(160, 1), (240, 0)])
def test_reduced_system_without_cameras_in_lds(hip, sfm, oracle, n_cams, lds_mode):
    """160 cameras: the accumulators alone fit LDS (mode 1); 240: neither does (mode 0, global atomics)."""
    fits2, fits1 = 8 * n_cams * (19 + 35) <= 64 * 1024, 8 * n_cams * 35 <= 64 * 1024
    assert (2 if fits2 else (1 if fits1 else 0)) == lds_mode
    sc = sfm.scenes.make_scene(n_cams, 40, 0.2, seed=3)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    r = oracle.obs_terms_vec(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn)[0]
    delta = float(np.sqrt(np.median(np.sum(r * r, axis=1))))
    for kind in LOSSES:
        for mode in (hip.SCHUR_PAIRS, hip.SCHUR_MFMA):          # sparse and dense Z
            _check_reduced(hip, sc, uvn, sc.cams_init, sc.pts_init, kind, delta, mode)


# ---- 4 ------------------------------------------------------------------------------------------------------------
CONFIGS = ("fused", "separate", "graph", "deterministic", "split")


def _run_config(hip, prob, config, iters):
    """``iters`` iterations in one launch configuration; returns what the configuration has to show."""
    if config == "separate":
        prob.set_option(hip.OPT_DEBUG, 16)
    elif config == "graph":
        prob.set_option(hip.OPT_GRAPH, 1)
    elif config == "deterministic":
        prob.set_option(hip.OPT_DETERMINISTIC, 1)
    if config == "split":
        for _ in range(iters):
            prob.linearize_reduce(LAM)
            prob.solve_update(LAM)
        prob.flush()
    else:
        prob.iterate(LAM, iters)
    return prob.info(hip.INFO_GRAPH_REPLAYS)


@pytest.mark.parametrize("kind", LOSSES)
def test_iterations_on_the_outlier_scene(hip, sfm, kind):
    _o, sc, uvn, cams0, _scale, deltas = _outlier(sfm)
    trace, costs = _outlier_run(sfm, kind)
    want_c, want_p = trace[9]
    bits = []
    for config in CONFIGS + ("deterministic",):
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_loss(kind, deltas[kind])
            prob.set_state(cams0, sc.pts_init)
            replays = _run_config(hip, prob, config, 10)
            cams, pts = prob.get_state()
            stats = prob.get_stats()
        assert (replays > 0) == (config == "graph"), config
        assert rel(cams, want_c) < 1e-9 and rel(pts, want_p) < 1e-9, (config, rel(cams, want_c), rel(pts, want_p))
        assert stats.shape == (10,) and rel(stats, costs[:10]) < 1e-9, (config, rel(stats, costs[:10]))
        if config == "deterministic":
            bits.append((cams, pts, stats))
    assert all(same_bits(a, b) for a, b in zip(*bits))


@pytest.mark.parametrize("kind", LOSSES)
def test_iterations_on_the_ragged_scene(hip, sfm, oracle, kind):
    """130 cameras: beyond the fused kernel (and with it the graph); tracks of 0 to 130 observations."""
    rs, _pt_of, _r, delta = _ragged(sfm, oracle)
    want_c, want_p, costs = _ragged_run(sfm, oracle, kind)
    assert (rs.lengths == 0).any() and rs.lengths.max() == 130
    for config in CONFIGS:
        with hip.BaProblem(rs.scene.n_cams, rs.pt_ptr, rs.cam_idx, rs.uv) as prob:
            prob.set_loss(kind, delta)
            prob.set_state(rs.scene.cams_true, rs.x_init[0:3])
            replays = _run_config(hip, prob, config, 3)
            cams, pts = prob.get_state()
            stats = prob.get_stats()
        assert replays == 0
        assert rel(cams, want_c) < 1e-9 and rel(pts, want_p) < 1e-9, (config, rel(cams, want_c), rel(pts, want_p))
        assert rel(stats, costs) < 1e-9, (config, rel(stats, costs))
        empty = rs.lengths == 0
        assert same_bits(pts[:, empty], rs.x_init[0:3][:, empty])


# ---- 5 ------------------------------------------------------------------------------------------------------------
def test_nothing_changes_when_off(hip, sfm):
    _o, sc, uvn, cams0, _scale, deltas = _outlier(sfm)

    def run(prepare):
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_option(hip.OPT_DETERMINISTIC, 1)
            prepare(prob)
            prob.set_state(cams0, sc.pts_init)
            prob.iterate(LAM, 5)
            return prob.get_state() + (prob.get_stats(),)

    def on_then_off(prob):
        prob.set_loss(hip.LOSS_HUBER, deltas[rr.LOSS_HUBER])
        prob.set_state(cams0, sc.pts_init)
        prob.iterate(LAM, 2)
        prob.set_loss(hip.LOSS_NONE)
        assert prob.loss()[0] == hip.LOSS_NONE

    fresh = run(lambda prob: None)
    back = run(on_then_off)
    assert all(same_bits(a, b) for a, b in zip(fresh, back))
    # a delta beyond every residual: Huber is the plain problem
    wide = run(lambda prob: prob.set_loss(hip.LOSS_HUBER, 1e3))
    assert rel(wide[0], fresh[0]) < 1e-12 and rel(wide[1], fresh[1]) < 1e-12
    assert np.max(np.abs(wide[2] - fresh[2]) / fresh[2]) < 1e-12


# ---- 6 ------------------------------------------------------------------------------------------------------------
def _clean_rmse_px(sfm, cams, pts):
    o, sc, uvn, _cams0, scale, _deltas = _outlier(sfm)
    r = rr._oracle().obs_terms_vec(np.asarray(cams), np.asarray(pts), sc.cam_idx, sc.pt_idx, uvn)[0]
    return float(scale * np.sqrt(np.mean(np.sum(r * r, axis=1)[~o.displaced])))


def test_it_does_its_job(hip, sfm, oracle):
    o, sc, uvn, cams0, _scale, deltas = _outlier(sfm)
    delta = deltas[rr.LOSS_HUBER]
    trace, costs = _outlier_run(sfm, rr.LOSS_HUBER)
    want_c, want_p = trace[19]
    # conditions on the reference alone
    final_cost = rr.state_cost(want_c, want_p, sc.cam_idx, sc.pt_idx, uvn, rr.LOSS_HUBER, delta)
    assert np.all(np.diff(np.append(costs, final_cost)) <= 0)
    r = oracle.obs_terms_vec(want_c, want_p, sc.cam_idx, sc.pt_idx, uvn)[0]
    _s, w_ref, _rho = rr.loss_terms(rr.LOSS_HUBER, delta, r)
    assert o.displaced.sum() == 37 and np.all(w_ref[o.displaced] < 0.5)
    assert np.count_nonzero(w_ref[~o.displaced] == 1.0) >= 0.99 * (~o.displaced).sum()
    plain_trace, _plain_costs = _outlier_run(sfm, rr.LOSS_NONE)
    assert _clean_rmse_px(sfm, want_c, want_p) <= 0.5 * _clean_rmse_px(sfm, *plain_trace[19])
    # the device equals it
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_loss(hip.LOSS_HUBER, delta)
        prob.set_state(cams0, sc.pts_init)
        prob.iterate(LAM, 20)
        cams, pts = prob.get_state()
        stats = prob.get_stats()
        w = prob.loss_terms()[1]
    assert rel(cams, want_c) < 1e-9 and rel(pts, want_p) < 1e-9
    assert rel(stats, costs) < 1e-9 and rel(w, w_ref) < 1e-9
    assert np.all(w[o.displaced] < 0.5)


# ---- 7 ------------------------------------------------------------------------------------------------------------
def test_the_loss_survives_append_and_cull(hip, sfm):
    o, sc, uvn, cams0, scale, deltas = _outlier(sfm)
    kind, delta = hip.LOSS_CAUCHY, deltas[rr.LOSS_CAUCHY]
    n0 = 250                                                    # the first 250 points, then the other 50 with their tracks
    m0 = int(sc.pt_ptr[n0])
    with hip.BaProblem(sc.n_cams, sc.pt_ptr[:n0 + 1], sc.cam_idx[:m0], uvn[:, :m0]) as prob:
        prob.set_option(hip.OPT_GRAPH, 1)
        prob.set_loss(kind, delta)
        prob.set_state(cams0, sc.pts_init[:, :n0])
        prob.iterate(LAM, 3)
        cams1, pts1 = prob.get_state()
        prob.append(np.zeros((0, 7)), sc.pts_init[:, n0:], sc.cam_idx[m0:], sc.pt_idx[m0:], uvn[:, m0:])
        assert prob.loss() == (kind, delta)
        pt_ptr, cam_idx, uv = prob.structure()
        assert np.array_equal(pt_ptr, sc.pt_ptr) and np.array_equal(cam_idx, sc.cam_idx)
        prob.iterate(LAM, 3)
        cams2, pts2 = prob.get_state()
        start = np.hstack((pts1, sc.pts_init[:, n0:]))
        want_c, want_p, costs = rr.ba_robust(cams1, start, sc.cam_idx, sc.pt_idx, uv, LAM, 3, kind, delta)
        assert rel(cams2, want_c) < 1e-9 and rel(pts2, want_p) < 1e-9 and rel(prob.get_stats(), costs) < 1e-9
        # cull at 20 px: the loss stays, the iterations are those of the culled lists
        want = sr.screen_reference(sc.pt_ptr, sc.cam_idx, uv, cams2, pts2, (20.0 / scale) ** 2, 1.0, 2)
        assert np.min(np.abs(np.sqrt(want.err2) * scale - 20.0)) > 1e-3 and 0 < np.count_nonzero(want.obs_flags) < 200
        got = prob.cull((20.0 / scale) ** 2, 1.0, 2)
        assert np.array_equal(got.obs_flags, want.obs_flags)
        assert prob.loss() == (kind, delta)
        new_ptr, new_cam, new_uv = prob.structure()
        pt_of = np.repeat(np.arange(sc.n_pts), np.diff(new_ptr)).astype(np.int32)
        prob.iterate(LAM, 3)
        cams3, pts3 = prob.get_state()
        want_c, want_p, costs = rr.ba_robust(cams2, pts2, new_cam, pt_of, new_uv, LAM, 3, kind, delta)
        assert rel(cams3, want_c) < 1e-9 and rel(pts3, want_p) < 1e-9 and rel(prob.get_stats(), costs) < 1e-9


def test_set_loss_completes_the_pending_step_with_the_old_loss(hip, sfm):
    _o, sc, uvn, cams0, _scale, deltas = _outlier(sfm)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_loss(hip.LOSS_HUBER, deltas[rr.LOSS_HUBER])
        prob.set_state(cams0, sc.pts_init)
        prob.linearize_reduce(LAM)
        prob.solve_update(LAM)                                  # 6 cameras: the back substitution is deferred
        up = prob.upload_bytes
        prob.set_loss(hip.LOSS_CAUCHY, deltas[rr.LOSS_CAUCHY])
        assert prob.upload_bytes == up
        prob.iterate(LAM, 1)
        cams, pts = prob.get_state()
        stats = prob.get_stats()
    c1, p1, _ = rr.ba_robust(cams0, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, LAM, 1, rr.LOSS_HUBER, deltas[rr.LOSS_HUBER])
    c2, p2, costs = rr.ba_robust(c1, p1, sc.cam_idx, sc.pt_idx, uvn, LAM, 1, rr.LOSS_CAUCHY, deltas[rr.LOSS_CAUCHY])
    assert rel(cams, c2) < 1e-9 and rel(pts, p2) < 1e-9
    assert stats.shape == (1,) and rel(stats, costs) < 1e-9      # set_loss restarted the cost history
    # the step completed with the NEW loss would have ended elsewhere
    t = rr.reduced_system(cams0, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, LAM, rr.LOSS_CAUCHY, deltas[rr.LOSS_CAUCHY])
    assert rel(t["ex"], rr.reduced_system(cams0, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, LAM, rr.LOSS_HUBER,
                                          deltas[rr.LOSS_HUBER])["ex"]) > 1e-3


def test_bad_arguments_and_an_empty_problem(hip, sfm):
    sc = sfm.scenes.make_scene(3, 10, 1.0, seed=4)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(sc.cams_init, sc.pts_init)
        prob.set_loss(hip.LOSS_HUBER, 0.25)
        lib = prob._lib
        for kind, delta in ((-1, 1.0), (3, 1.0), (hip.LOSS_HUBER, 0.0), (hip.LOSS_CAUCHY, -1.0),
                            (hip.LOSS_HUBER, float("nan")), (hip.LOSS_CAUCHY, float("inf"))):
            assert lib.sfm_ba_set_loss(prob._h, kind, delta) == hip.E_SHAPE, (kind, delta)
            assert prob.loss() == (hip.LOSS_HUBER, 0.25)
        with pytest.raises(ValueError):
            prob.set_loss(hip.LOSS_HUBER, 0.0)
        assert lib.sfm_ba_set_loss(prob._h, hip.LOSS_NONE, float("nan")) == hip.OK      # delta is ignored
        assert prob.loss()[0] == hip.LOSS_NONE
        # nothing left to fit: the loss is accepted and the step is zero
        prob.cull(0.0, 1.0, 0)
        assert prob.info(hip.INFO_N_OBS) == 0
        state = prob.get_state()
        prob.set_loss(hip.LOSS_CAUCHY, 0.5)
        prob.iterate(LAM, 2)
        cams, pts = prob.get_state()
        assert same_bits(pts, state[1]) and rel(cams, state[0]) < 1e-12
        assert all(t.shape == (0,) for t in prob.loss_terms()) and prob.loss() == (hip.LOSS_CAUCHY, 0.5)


# ---- 8 ------------------------------------------------------------------------------------------------------------
class _KP:
    def __init__(self, x, y):
        self.pt = (float(x), float(y))


class _View:
    def __init__(self, rot, loc, k, key_pts):
        self.rot, self.loc, self.k, self.key_pts = rot, loc, k, key_pts

    def update_cam_pose(self, rot, loc):
        self.rot, self.loc = rot, loc


class _Holder:
    pass


class _DropIn:
    """The host-track harness of the screening tests (tests/test_gpu_screen.py) with 20 iterations per adjustment."""

    def __init__(self, sfm, sc, uv_pix, max_views):
        self.sfm, self.sc, self.max_views = sfm, sc, max_views
        self.vp, self.kt = _Holder(), _Holder()
        self.vp.view_list, self.kt.track_list = [], []
        self.tp = sfm.processors.HipTriangulationProcessor(0.5, 30)
        self.tp.tri_pts = np.vstack((sc.pts_init, np.ones((1, sc.n_pts))))
        self.bp = sfm.processors.HipBaProcessor(self.vp, self.kt, None, self.tp, None, iteration=20, damping_factor=0.5)
        self.bp.ba_verbose = False
        for c in range(sc.n_cams):
            sel = sc.cam_idx == c
            q = sc.cams_init[c, 3:7] / np.linalg.norm(sc.cams_init[c, 3:7])
            self.add_view(sfm.geometry.quaternion_to_rotation(q), sc.cams_init[c, 0:3].reshape(3, 1).copy(), uv_pix[:, sel], sc.pt_idx[sel])

    def add_view(self, rot, loc, pix, pts):
        c = len(self.vp.view_list)
        self.vp.view_list.append(_View(rot, loc, self.sc.intrinsic.copy(), [_KP(-1.0, -1.0)] + [_KP(x, y) for x, y in pix.T]))
        track = _Holder()
        track.table = np.full((self.max_views, pix.shape[1] + 1), -1, dtype=int)
        track.table[c, 1:] = pts
        self.kt.track_list.append(track)

    def cams(self):
        return np.stack([self.sfm.geometry.pack_camera(v.rot, v.loc) for v in self.vp.view_list])


def test_drop_in(hip, sfm):
    o, sc, uvn, _cams0, scale, deltas = _outlier(sfm)
    run, plain = _DropIn(sfm, sc, o.uv_pix, 6), _DropIn(sfm, sc, o.uv_pix, 6)
    try:
        bp = run.bp
        bp.ba_loss = ("huber", 5.0)
        cams0, pts0 = run.cams(), run.tp.tri_pts[0:3].copy()
        bp.execute_bundle_adjustment()
        assert bp.ba_last_action == "create"
        assert bp._hip_scene.prob.loss() == (hip.LOSS_HUBER, 5.0 / scale)
        want_c, want_p, _costs = rr.ba_robust(cams0, pts0, sc.cam_idx, sc.pt_idx, uvn, 0.5, 20, rr.LOSS_HUBER, deltas[rr.LOSS_HUBER])
        assert rel(run.cams(), want_c) < 1e-9 and rel(run.tp.tri_pts[0:3], want_p) < 1e-9

        plain.bp.execute_bundle_adjustment()
        assert plain.bp.ba_loss is None and plain.bp._hip_scene.prob.loss()[0] == hip.LOSS_NONE
        assert _clean_rmse_px(sfm, run.cams(), run.tp.tri_pts[0:3]) <= 0.5 * _clean_rmse_px(sfm, plain.cams(), plain.tp.tri_pts[0:3])

        # the attribute set on a live scene reaches the resident problem with the next call, and moves no bytes
        up = plain.bp.ba_upload_bytes
        plain.bp.ba_loss = ("cauchy", 10.0)
        plain.bp.iteration = 1
        plain.bp.execute_bundle_adjustment()
        assert plain.bp.ba_last_action == "reuse" and plain.bp.ba_upload_bytes == up
        assert plain.bp._hip_scene.prob.loss() == (hip.LOSS_CAUCHY, 10.0 / scale)
        plain.bp.ba_loss = None
        plain.bp.execute_bundle_adjustment()
        assert plain.bp._hip_scene.prob.loss()[0] == hip.LOSS_NONE and plain.bp.ba_upload_bytes == up

        # the screening after the robust adjustment still finds every displaced observation
        scales = np.full(6, scale)
        want = sr.screen_reference(sc.pt_ptr, sc.cam_idx, uvn, want_c, want_p, 20.0 ** 2, 1.0, 2, scales)
        assert o.displaced.sum() == 37 and np.all(want.obs_flags[o.displaced] != 0)
        assert np.min(np.abs(np.sqrt(want.err2) - 20.0)) > 1e-3
        report = bp.filter_structure(max_reproj_px=20.0, min_angle_deg=None)
        assert np.array_equal(report.obs_flags, want.obs_flags) and np.all(report.obs_flags[o.displaced] != 0)
        assert bp._hip_scene.prob.loss() == (hip.LOSS_HUBER, 5.0 / scale)      # ... and the culled scene keeps the loss
    finally:
        run.bp.ba_release()
        plain.bp.ba_release()
