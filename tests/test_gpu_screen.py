"""GPU tests of the screening and culling of the resident bundle-adjustment scene (sfm_ba_screen / sfm_ba_cull,
``BaProblem.screen`` / ``cull``, ``HipBaMixin.screen_structure`` / ``filter_structure``) against the float64 reference of
tests/_screen_reference.py.  Values at the suite's bar of 1e-9 relative; flags, counts and the culled structure exactly,
with every threshold placed in a gap of the reference's values (``threshold_in_gap``) so that only a real error can flip
a flag."""
import numpy as np
import pytest

import _screen_reference as sr
import _tracks_reference as tr

pytestmark = pytest.mark.gpu

GROUPS = tr.GROUPS
FIELDS = ("err2", "depth", "obs_flags", "min_cos", "pt_flags", "summary")
_CACHE = {}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _problem(hip, sfm):
    """ragged_scene as a BaProblem at (cams_true, x_init[0:3]): 130 cameras, 66 points, M = 2 667."""
    rs = tr.ragged_scene(sfm)
    prob = hip.BaProblem(rs.scene.n_cams, rs.pt_ptr, rs.cam_idx, rs.uv)
    prob.set_state(rs.scene.cams_true, rs.x_init[0:3])
    return rs, prob


def _ref(sfm, max_err2=np.inf, cos_min_angle=1.0, min_obs=2, scaled=False, pts=None):
    """screen_reference on the ragged scene, computed once per argument set."""
    rs = tr.ragged_scene(sfm)
    key = (float(max_err2), float(cos_min_angle), int(min_obs), bool(scaled), None if pts is None else pts.tobytes())
    if key not in _CACHE:
        _CACHE[key] = sr.screen_reference(rs.pt_ptr, rs.cam_idx, rs.uv, rs.scene.cams_true, rs.x_init[0:3] if pts is None else pts,
                                          max_err2, cos_min_angle, min_obs, _scales(rs) if scaled else None)
    return _CACHE[key]


def _scales(rs):
    return 1.0 + np.arange(rs.scene.n_cams) / 7.0           # a distinct value per camera


def _thresholds(sfm):
    """(err2 thresholds at the 0.5 and 0.9 quantiles, cos of an angle threshold in the widest gap near 8 degrees)."""
    rs = tr.ragged_scene(sfm)
    base = _ref(sfm)
    t50, t90 = sr.threshold_in_gap(base.err2, 0.5), sr.threshold_in_gap(base.err2, 0.9)
    one_minus = np.sort(1.0 - base.min_cos[rs.lengths >= 2])
    near = one_minus[(one_minus > 1.0 - np.cos(np.radians(6.0))) & (one_minus < 1.0 - np.cos(np.radians(10.0)))]
    g = int(np.argmax(np.diff(near)))                          # the widest gap between 6 and 10 degrees
    assert near[g + 1] - near[g] >= 1e-4 * near[g + 1]
    cos_t = 1.0 - 0.5 * (near[g] + near[g + 1])
    return t50, t90, cos_t


def _check_values(got, want):
    assert got.err2.shape == want.err2.shape and got.min_cos.shape == want.min_cos.shape
    assert np.max(np.abs(got.err2 - want.err2) / want.err2) < 1e-9
    assert np.max(np.abs(got.depth - want.depth) / np.abs(want.depth)) < 1e-9
    wide = 1.0 - want.min_cos > 1e-6
    assert np.max(np.abs((1.0 - got.min_cos[wide]) - (1.0 - want.min_cos[wide])) / (1.0 - want.min_cos[wide])) < 1e-9
    assert np.all(np.abs(got.min_cos[~wide] - want.min_cos[~wide]) <= 1e-12)


def _check_flags(got, want, what=None):
    assert np.array_equal(got.obs_flags, want.obs_flags), what
    assert np.array_equal(got.pt_flags, want.pt_flags), what
    assert got.summary.tolist() == want.summary.tolist(), what
    assert got.obs_flags.dtype == np.uint8 and got.pt_flags.dtype == np.int32 and got.summary.dtype == np.int64


# ---- 1 ------------------------------------------------------------------------------------------------------------
def test_values_against_the_reference(hip, sfm):
    rs, prob = _problem(hip, sfm)
    with prob:
        before = prob.upload_bytes
        got = prob.screen()
        assert prob.upload_bytes == before                                       # nothing goes up without cam_scale
        _check_values(got, _ref(sfm))
        _check_flags(got, _ref(sfm))
        scaled = prob.screen(cam_scale=_scales(rs))
        assert prob.upload_bytes == before + 8 * rs.scene.n_cams
        _check_values(scaled, _ref(sfm, scaled=True))
        assert same_bits(scaled.depth, got.depth) and same_bits(scaled.min_cos, got.min_cos)
        # the residuals are the linearisation's: per point they add up to refine_points' cost at the same state
        per_point = np.array([got.err2[rs.pt_ptr[p]:rs.pt_ptr[p + 1]].sum() for p in range(rs.n_pts)])
        cost, _status = prob.refine_points(0.5, 0)
        some = rs.lengths > 0
        assert np.max(np.abs(per_point[some] - cost[0, some]) / cost[0, some]) < 1e-9
        assert np.all(per_point[~some] == 0) and np.all(cost[0, ~some] == 0)
        # the summary alone
        only = prob.screen(want_outputs=False)
        assert only.err2 is None and only.obs_flags is None and only.summary.tolist() == got.summary.tolist()


# ---- 2 ------------------------------------------------------------------------------------------------------------
def test_flags_and_counts_equal_the_reference(hip, sfm):
    t50, t90, cos_t = _thresholds(sfm)
    rs, prob = _problem(hip, sfm)
    with prob:
        for max_err2, cos_min in ((t50, 1.0), (t90, 1.0), (np.inf, cos_t), (t50, cos_t), (t90, cos_t)):
            for min_obs in (0, 1, 2, 3, 5):
                got = prob.screen(max_err2, cos_min, min_obs)
                want = _ref(sfm, max_err2, cos_min, min_obs)
                _check_flags(got, want, (max_err2, cos_min, min_obs))
        # every kind of flag has been seen
        want = _ref(sfm, t50, cos_t, 5)
        assert want.summary[2] > 1000 and want.summary[5] > 0 and want.summary[6] > 0 and want.summary[7] > 0
        assert _ref(sfm, np.inf, cos_t, 0).summary[7] > 3
        assert set(np.unique(want.pt_flags).tolist()) >= {0, sr.PT_TOO_FEW, sr.PT_EMPTY}


# ---- 3 ------------------------------------------------------------------------------------------------------------
def test_depth_and_nonfinite_points(hip, sfm):
    rs = tr.ragged_scene(sfm)
    pts = rs.x_init[0:3].copy()
    moved = []
    for length, k in ((5, 2), (17, 9), (64, 30)):
        p = int(np.flatnonzero(rs.lengths == length)[0])
        c = int(rs.cam_idx[rs.pt_ptr[p] + k])
        pts[:, p] = 2.0 * rs.scene.cams_true[c, 0:3] - pts[:, p]                 # mirrored through the centre of camera c
        moved.append((p, rs.pt_ptr[p] + k))
    p_nan = int(np.flatnonzero(rs.lengths == 9)[1])
    pts[1, p_nan] = np.nan
    t90 = _thresholds(sfm)[1]
    want = _ref(sfm, t90, 1.0, 2, pts=pts)
    for p, o in moved:
        assert want.obs_flags[o] & sr.OBS_BEHIND
    assert want.summary[3] >= 3 and want.summary[4] == 9
    with hip.BaProblem(rs.scene.n_cams, rs.pt_ptr, rs.cam_idx, rs.uv) as prob:
        prob.set_state(rs.scene.cams_true, pts)
        for g in (0, 1, 8, 64):
            got = prob.screen(t90, 1.0, 2, group=g)
            _check_flags(got, want, g)
            ok = want.obs_flags & sr.OBS_NONFINITE == 0
            assert np.max(np.abs(got.depth[ok] - want.depth[ok]) / np.abs(want.depth[ok])) < 1e-9
            own = slice(rs.pt_ptr[p_nan], rs.pt_ptr[p_nan + 1])
            assert np.all(got.obs_flags[own] == sr.OBS_NONFINITE) and got.pt_flags[p_nan] == sr.PT_TOO_FEW
            assert np.all(np.isnan(got.err2[own]))


# ---- 4 ------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_group_width(hip, sfm):
    t50, _t90, cos_t = _thresholds(sfm)
    rs, prob = _problem(hip, sfm)
    with prob:
        auto = prob.screen(t50, cos_t, 3, cam_scale=None)
        for g in GROUPS:
            runs = [prob.screen(t50, cos_t, 3, group=g) for _ in range(2)]
            for f in FIELDS:
                assert same_bits(getattr(runs[0], f), getattr(runs[1], f)), (g, f)
                assert same_bits(getattr(runs[0], f), getattr(auto, f)), (g, f)
        with pytest.raises(ValueError, match="group"):
            prob.screen(group=2)


# ---- 5 ------------------------------------------------------------------------------------------------------------
def test_cull_leaves_the_reference_structure_and_the_state(hip, sfm):
    _t50, t90, cos_t = _thresholds(sfm)
    rs, prob = _problem(hip, sfm)
    with prob:
        cams0, pts0 = prob.get_state()
        before = prob.upload_bytes
        want = _ref(sfm, t90, cos_t, 2)
        want_struct = sr.compact(rs.pt_ptr, rs.cam_idx, rs.uv, want.obs_flags)
        got = prob.cull(t90, cos_t, 2)
        _check_flags(got, want)
        _check_values(got, want)
        m2 = int(want.summary[1])
        assert 0 < m2 < rs.cam_idx.shape[0]
        pt_ptr, cam_idx, uv = prob.structure()
        assert np.array_equal(pt_ptr, want_struct[0]) and np.array_equal(cam_idx, want_struct[1]) and same_bits(uv, want_struct[2])
        assert prob.info(hip.INFO_N_OBS) == m2 == prob.n_obs and prob.info(hip.INFO_N_PTS) == rs.n_pts
        assert prob.info(hip.INFO_N_CAMS) == rs.scene.n_cams
        cams1, pts1 = prob.get_state()
        assert same_bits(cams1, cams0) and same_bits(pts1, pts0)
        assert prob.upload_bytes == before                                       # nothing is uploaded
        assert prob.get_stats().shape[0] == 0
        # a second identical cull drops nothing and leaves the scene in place
        again = prob.cull(t90, cos_t, 2)
        assert again.summary[0] == again.summary[1] == m2 and not again.summary[2:].any()
        assert not again.obs_flags.any() and again.obs_flags.shape[0] == m2
        second = prob.structure()
        assert all(same_bits(a, b) for a, b in zip(second, (pt_ptr, cam_idx, uv)))
        # with cam_scale only its bytes go up
        before = prob.upload_bytes
        prob.cull(cam_scale=_scales(rs))
        assert prob.upload_bytes - before == 8 * rs.scene.n_cams


# ---- 6 ------------------------------------------------------------------------------------------------------------
def test_culled_problem_behaves_as_a_problem_of_the_culled_lists(hip, sfm, oracle):
    _t50, t90, cos_t = _thresholds(sfm)
    rs, prob = _problem(hip, sfm)
    want = _ref(sfm, t90, cos_t, 2)
    new_ptr, new_cam, new_uv = sr.compact(rs.pt_ptr, rs.cam_idx, rs.uv, want.obs_flags)
    pts0 = rs.x_init[0:3]
    with prob, hip.BaProblem(rs.scene.n_cams, new_ptr, new_cam, new_uv) as fresh:
        prob.cull(t90, cos_t, 2)
        prob.iterate(0.5, 5)
        cams_a, pts_a = prob.get_state()
        fresh.set_state(rs.scene.cams_true, pts0)
        fresh.iterate(0.5, 5)
        cams_b, pts_b = fresh.get_state()
        assert prob.get_stats().shape[0] == 5
        assert rel(prob.get_stats(), fresh.get_stats()) < 1e-9
    assert rel(cams_a, cams_b) < 1e-9 and rel(pts_a, pts_b) < 1e-9
    pt_of = np.repeat(np.arange(rs.n_pts), np.diff(new_ptr)).astype(np.int32)
    ocams, opts = oracle.ba_sparse(rs.scene.cams_true, pts0, new_cam, pt_of, new_uv, 0.5, 5)
    assert rel(cams_a, ocams) < 1e-9 and rel(pts_a, opts) < 1e-9
    assert rel(cams_b, ocams) < 1e-9 and rel(pts_b, opts) < 1e-9
    emptied = np.diff(new_ptr) == 0
    assert emptied.sum() > (rs.lengths == 0).sum()
    assert same_bits(pts_a[:, emptied], pts0[:, emptied]) and same_bits(pts_b[:, emptied], pts0[:, emptied])


# ---- 7 ------------------------------------------------------------------------------------------------------------
def test_thresholds_that_drop_nothing_and_everything(hip, sfm):
    rs, prob = _problem(hip, sfm)
    with prob:
        m = rs.cam_idx.shape[0]
        prob.iterate(0.5, 1)
        state = prob.get_state()
        structure = prob.structure()
        got = prob.cull(np.inf, 1.0, 0)
        assert got.summary.tolist() == [m, m, 0, 0, 0, 0, 0, 0] and not got.obs_flags.any()
        assert all(same_bits(a, b) for a, b in zip(prob.structure(), structure))
        assert prob.get_stats().shape[0] == 1                                    # the untouched problem keeps its cost history
        got = prob.cull(0.0, 1.0, 0)                                             # every residual exceeds 0
        assert got.summary.tolist() == [m, 0, m, 0, 0, 0, 0, 0]
        assert np.all(got.obs_flags == sr.OBS_HIGH_ERROR) and not got.pt_flags[rs.lengths > 0].any()
        pt_ptr, cam_idx, uv = prob.structure()
        assert not pt_ptr.any() and cam_idx.shape == (0,) and uv.shape == (2, 0) and prob.info(hip.INFO_N_OBS) == 0
        assert all(same_bits(a, b) for a, b in zip(prob.get_state(), state))
        prob.iterate(0.5, 2)                                                     # nothing to fit: the step is zero
        cams, pts = prob.get_state()
        assert same_bits(pts, state[1]) and rel(cams, state[0]) < 1e-12
        empty = prob.screen()
        assert empty.summary.tolist() == [0] * 8 and np.all(empty.pt_flags == sr.PT_EMPTY) and np.all(empty.min_cos == 1.0)


def test_a_camera_left_without_observations(hip, sfm):
    rs, prob = _problem(hip, sfm)
    scale = np.ones(rs.scene.n_cams)
    scale[7] = 1e6
    want = sr.screen_reference(rs.pt_ptr, rs.cam_idx, rs.uv, rs.scene.cams_true, rs.x_init[0:3], 1.0, 1.0, 0, scale)
    assert np.array_equal(want.obs_flags != 0, rs.cam_idx == 7) and (rs.cam_idx == 7).sum() > 5
    new_ptr, new_cam, new_uv = sr.compact(rs.pt_ptr, rs.cam_idx, rs.uv, want.obs_flags)
    with prob, hip.BaProblem(rs.scene.n_cams, new_ptr, new_cam, new_uv) as fresh:
        got = prob.cull(1.0, 1.0, 0, cam_scale=scale)
        _check_flags(got, want)
        pt_ptr, cam_idx, uv = prob.structure()
        assert np.array_equal(pt_ptr, new_ptr) and np.array_equal(cam_idx, new_cam) and same_bits(uv, new_uv)
        assert not (cam_idx == 7).any()
        prob.iterate(0.5, 3)
        fresh.set_state(rs.scene.cams_true, rs.x_init[0:3])
        fresh.iterate(0.5, 3)
        (cams_a, pts_a), (cams_b, pts_b) = prob.get_state(), fresh.get_state()
        assert rel(cams_a, cams_b) < 1e-9 and rel(pts_a, pts_b) < 1e-9
        assert rel(cams_a[7], rs.scene.cams_true[7]) < 1e-12                     # the camera nothing observes stays


def test_cull_under_a_captured_graph(hip, sfm):
    """On a 6-camera scene: the ragged scene's 130 cameras are beyond what the fused iteration, and with it the graph,
    supports (102)."""
    sc = sfm.scenes.make_scene(6, 120, 0.6, seed=12)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    results = []
    for graph in (1, 0):
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.set_option(hip.OPT_GRAPH, graph)
            prob.iterate(5.0, 6)
            replays = prob.info(hip.INFO_GRAPH_REPLAYS)
            assert (replays > 0) == bool(graph)
            mid = prob.get_state()
            t80 = sr.threshold_in_gap(sr.screen_reference(sc.pt_ptr, sc.cam_idx, uvn, mid[0], mid[1]).err2, 0.8)
            want = sr.screen_reference(sc.pt_ptr, sc.cam_idx, uvn, mid[0], mid[1], t80, 1.0, 2)
            got = prob.cull(t80, 1.0, 2)
            _check_flags(got, want, graph)
            assert got.summary[1] < got.summary[0]
            prob.iterate(5.0, 6)                                                 # the graph is captured again for the new scene
            assert (prob.info(hip.INFO_GRAPH_REPLAYS) > replays) == bool(graph)
            results.append((mid, got, prob.get_state(), prob.structure()))
    (mid_g, got_g, end_g, str_g), (mid_e, got_e, end_e, str_e) = results
    assert rel(mid_g[0], mid_e[0]) < 1e-9 and rel(mid_g[1], mid_e[1]) < 1e-9
    assert np.array_equal(got_g.obs_flags, got_e.obs_flags) and all(same_bits(a, b) for a, b in zip(str_g, str_e))
    assert rel(end_g[0], end_e[0]) < 1e-9 and rel(end_g[1], end_e[1]) < 1e-9
    # ... and the culled, graphed problem equals a fresh one of the culled lists
    with hip.BaProblem(sc.n_cams, *str_e) as fresh:
        fresh.set_state(*mid_e)
        fresh.iterate(5.0, 6)
        cams, pts = fresh.get_state()
    assert rel(end_g[0], cams) < 1e-9 and rel(end_g[1], pts) < 1e-9


# ---- 8 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pts", [1, 1023, 1024, 1025, 2049])
def test_scan_boundaries(hip, sfm, n_pts):
    sc = sfm.scenes.make_scene(5, n_pts, 0.6, seed=60 + n_pts % 7)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    base = sr.screen_reference(sc.pt_ptr, sc.cam_idx, uvn, sc.cams_init, sc.pts_init)
    t80 = sr.threshold_in_gap(base.err2, 0.8)
    want = sr.screen_reference(sc.pt_ptr, sc.cam_idx, uvn, sc.cams_init, sc.pts_init, t80, 1.0, 2)
    new_ptr, new_cam, new_uv = sr.compact(sc.pt_ptr, sc.cam_idx, uvn, want.obs_flags)
    assert want.summary[1] < want.summary[0]
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(sc.cams_init, sc.pts_init)
        got = prob.cull(t80, 1.0, 2)
        _check_flags(got, want)
        pt_ptr, cam_idx, uv = prob.structure()
        assert np.array_equal(pt_ptr, new_ptr) and np.array_equal(cam_idx, new_cam) and same_bits(uv, new_uv)


# ---- 9 ------------------------------------------------------------------------------------------------------------
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
    """The host-track harness of the incremental tests: views with key lists, one track table per view whose self row
    maps key -> point (key 0 is a dummy), ``tri_pts``; all points are known from the start."""

    def __init__(self, sfm, sc, uv_pix, max_views):
        self.sfm, self.sc, self.max_views = sfm, sc, max_views
        self.vp, self.kt = _Holder(), _Holder()
        self.vp.view_list, self.kt.track_list = [], []
        self.tp = sfm.processors.HipTriangulationProcessor(0.5, 30)
        self.tp.tri_pts = np.vstack((sc.pts_init, np.ones((1, sc.n_pts))))
        self.bp = sfm.processors.HipBaProcessor(self.vp, self.kt, None, self.tp, None, iteration=10, damping_factor=0.5)
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

    def pairs(self):
        pt_ptr, cam_idx, _uv = self.bp._hip_scene.prob.structure()
        pt_of = np.repeat(np.arange(pt_ptr.shape[0] - 1), np.diff(pt_ptr))
        return set(zip(pt_of.tolist(), cam_idx.tolist()))


def test_filter_structure_end_to_end(hip, sfm, oracle):
    """Measured on the CPU for this scene (oracle, 10 iterations at lambda = 0.5, then a screen at 20 px): all 37 displaced
    observations and none of the 1 212 others are caught, the nearest errors are 19.7 and 24.0 px; ten more iterations leave
    the kept clean observations at 2.4 px RMSE on the culled scene against 5.4 px on the uncut one."""
    o = sr.outlier_scene(sfm)
    sc, displaced = o.scene, o.displaced
    uvn = sfm.geometry.normalise_pixels(o.uv_pix, sc.intrinsic)
    m = sc.cam_idx.shape[0]
    run = _DropIn(sfm, sc, o.uv_pix, 7)
    bp, tp = run.bp, run.tp
    try:
        bp.execute_bundle_adjustment()
        assert bp.ba_last_action == "create"
        cams1, pts1 = run.cams(), tp.tri_pts[0:3].copy()
        tables = [t.table.copy() for t in run.kt.track_list]
        up = bp.ba_upload_bytes
        report = bp.filter_structure(max_reproj_px=20.0, min_angle_deg=None)
        assert bp.ba_last_action == "reuse" and bp.ba_upload_bytes - up == 8 * 6       # cam_scale alone
        k = sc.intrinsic
        scale = np.full(6, np.sqrt(abs(k[0, 0] * k[1, 1])))
        want = sr.screen_reference(sc.pt_ptr, sc.cam_idx, uvn, cams1, pts1, 20.0 ** 2, 1.0, 2, scale)
        # conditions on the reference: the screen separates the displaced observations from the others
        assert np.all(want.obs_flags[displaced] != 0) and displaced.sum() == 37
        assert np.count_nonzero(want.obs_flags[~displaced]) <= 0.01 * (m - 37)
        assert np.min(np.abs(np.sqrt(want.err2) - 20.0)) > 0.1
        # the device drops exactly that
        assert np.array_equal(report.obs_flags, want.obs_flags) and np.array_equal(report.pt_flags, want.pt_flags)
        assert report.summary.tolist() == want.summary.tolist()
        assert rel(report.err_px, np.sqrt(want.err2)) < 1e-9
        assert np.all(report.min_angle_deg[want.min_cos < 1.0] > 0)
        new_ptr, new_cam, new_uv = sr.compact(sc.pt_ptr, sc.cam_idx, uvn, want.obs_flags)
        pt_ptr, cam_idx, uv = bp._hip_scene.prob.structure()
        assert np.array_equal(pt_ptr, new_ptr) and np.array_equal(cam_idx, new_cam) and same_bits(uv, new_uv)
        # the host's objects are untouched
        assert same_bits(tp.tri_pts[0:3], pts1) and same_bits(run.cams(), cams1)
        assert all(np.array_equal(t.table, old) for t, old in zip(run.kt.track_list, tables))
        gone = report.obs_flags != 0
        culled = set(zip(sc.pt_idx[gone].tolist(), sc.cam_idx[gone].tolist()))
        assert len(culled) == int(want.summary[0] - want.summary[1]) and not culled & run.pairs()

        # the next adjustment finds the culled scene in place and equals the oracle on the culled lists
        bp.execute_bundle_adjustment()
        assert bp.ba_last_action == "reuse"
        pt_of = np.repeat(np.arange(sc.n_pts), np.diff(new_ptr)).astype(np.int32)
        ocams, opts = oracle.ba_sparse(cams1, pts1, new_cam, pt_of, new_uv, 0.5, 10)
        assert rel(run.cams(), ocams) < 1e-9 and rel(tp.tri_pts[0:3], opts) < 1e-9
        ucams, upts = oracle.ba_sparse(cams1, pts1, sc.cam_idx, sc.pt_idx, uvn, 0.5, 10)
        clean = ~gone & ~displaced

        def rmse(cams, pts):
            return float(np.sqrt(np.mean(sr.screen_reference(sc.pt_ptr, sc.cam_idx, uvn, cams, pts, np.inf, 1.0, 0, scale).err2[clean])))
        assert rmse(ocams, opts) < rmse(ucams, upts)

        # one more view: pure growth is still an append onto the culled scene
        rot = sfm.geometry.quaternion_to_rotation(sc.cams_true[5, 3:7] / np.linalg.norm(sc.cams_true[5, 3:7]))
        loc = sc.cams_true[5, 0:3].reshape(3, 1) + np.array([[0.3], [0.1], [0.0]])
        seen = np.arange(0, sc.n_pts, 2)
        cam = rot.T @ (sc.pts_true[:, seen] - loc)
        assert np.all(cam[2] > 0)
        pix = (k @ cam)[0:2] / cam[2]
        run.add_view(rot, loc, pix, seen)
        bp.execute_bundle_adjustment()
        assert bp.ba_last_action == "append"
        pairs = run.pairs()
        assert not culled & pairs and len(pairs) == int(want.summary[1]) + seen.shape[0]
        assert {(int(p), 6) for p in seen} <= pairs

        # a changed table entry forces a rebuild, which leaves the culled pairs out as well
        row = run.kt.track_list[2].table[2]
        key = next(j for j in range(1, row.shape[0]) if (int(row[j]), 2) in pairs)
        lost = (int(row[key]), 2)
        run.kt.track_list[2].table[2, key] = -1
        bp.execute_bundle_adjustment()
        assert bp.ba_last_action == "create"
        rebuilt = run.pairs()
        assert not culled & rebuilt and rebuilt == pairs - {lost}
        # ba_release forgets the record: the next scene is the uncut one
        bp.ba_release()
        bp.screen_structure()
        assert bp.ba_last_action == "create" and culled - {lost} <= run.pairs()
    finally:
        bp.ba_release()


def test_screen_structure_changes_nothing(hip, sfm):
    o = sr.outlier_scene(sfm)
    sc = o.scene
    uvn = sfm.geometry.normalise_pixels(o.uv_pix, sc.intrinsic)
    run = _DropIn(sfm, sc, o.uv_pix, 6)
    bp, tp = run.bp, run.tp
    try:
        report = bp.screen_structure()                                           # creates the resident scene itself
        assert bp.ba_last_action == "create"
        k = sc.intrinsic
        scale = np.full(6, np.sqrt(abs(k[0, 0] * k[1, 1])))
        want = sr.screen_reference(sc.pt_ptr, sc.cam_idx, uvn, run.cams(), tp.tri_pts[0:3], np.inf, 1.0, 2, scale)
        assert rel(report.err_px, np.sqrt(want.err2)) < 1e-9 and np.array_equal(report.obs_flags, want.obs_flags)
        assert rel(report.min_angle_deg, np.degrees(np.arccos(want.min_cos))) < 1e-9
        structure = bp._hip_scene.prob.structure()
        state = bp._hip_scene.prob.get_state()
        up = bp.ba_upload_bytes
        strict = bp.screen_structure(max_reproj_px=5.0, min_angle_deg=3.0, min_obs=3)
        want = sr.screen_reference(sc.pt_ptr, sc.cam_idx, uvn, run.cams(), tp.tri_pts[0:3], 25.0, np.cos(np.radians(3.0)), 3, scale)
        assert strict.summary[1] < strict.summary[0] and bp.ba_last_action == "reuse"
        # 5 px and 3 degrees are not placed in gaps: a flag may differ where the reference's value is within 1e-9 of them
        near = (np.abs(want.err2 / 25.0 - 1.0) < 1e-9)
        assert np.array_equal(strict.obs_flags[~near] & 7, want.obs_flags[~near] & 7)
        assert bp.ba_upload_bytes - up == 8 * 6
        assert all(same_bits(a, b) for a, b in zip(bp._hip_scene.prob.structure(), structure))
        assert all(same_bits(a, b) for a, b in zip(bp._hip_scene.prob.get_state(), state))
    finally:
        bp.ba_release()
