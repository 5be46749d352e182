"""GPU tests of triangulation and structure-only refinement over ragged multi-view tracks: sfm_tri_tracks,
sfm_ba_refine_points and their drop-in methods, against the per-point float64 references of tests/_tracks_reference.py
(parity bars of the suite: 1e-9 relative for refined points and costs, 1e-10 for the DLT)."""
import numpy as np
import pytest

import _tracks_reference as tr

pytestmark = pytest.mark.gpu

GROUPS = tr.GROUPS


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views", [2, 3, 4, 5])
def test_rectangular_tracks_equal_the_rectangular_kernels(hip, sfm, n_views, capsys):
    sc = sfm.scenes.make_scene(n_views, 301, 1.0, seed=40 + n_views)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    projs = tr.camera_projections(sfm, sc.cams_true)
    uv_rect = np.stack([uvn[:, sc.cam_idx == c] for c in range(n_views)])
    x_init = np.vstack((sc.pts_init, np.ones((1, sc.n_pts))))
    want = hip.tri_nonlinear(projs, uv_rect, x_init, 0.5, 20)
    for g in (0,) + GROUPS:
        got, _cost, status = hip.tri_tracks(sc.pt_ptr, sc.cam_idx, uvn, projs, x_init, hip.TRACKS_NONLINEAR, 0.5, 20, g)
        assert rel(got, want) < 1e-9, g
        assert not status.any()
    lin_want = hip.tri_linear(projs, uv_rect)
    lin, _cost, status = hip.tri_tracks(sc.pt_ptr, sc.cam_idx, uvn, projs, None, hip.TRACKS_LINEAR, 0.5, 0)
    with capsys.disabled():
        print("\nDLT over rectangular tracks against tri_linear, %d views: %s (largest relative difference %.3e)"
              % (n_views, "equal bits" if same_bits(lin, lin_want) else "bits differ", rel(lin, lin_want)))
    assert rel(lin, lin_want) < 1e-10
    assert not status.any() and np.all(lin[3] == 1.0)


# ---- 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,iters", [(0.5, 100), (5.0, 3), (0.5, 1)])
def test_ragged_scene_against_the_per_point_reference(hip, sfm, lam, iters):
    rs = tr.ragged_scene(sfm)
    want, want_cost = tr.ragged_reference(sfm, lam, iters)
    many = rs.lengths >= 2
    assert np.all(want_cost[1, many] < want_cost[0, many])                    # the reference itself improves every such point
    for g in (0,) + GROUPS:
        got, cost, status = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, hip.TRACKS_NONLINEAR, lam, iters, g)
        assert rel(got, want) < 1e-9, g
        assert same_bits(got[3], rs.x_init[3])
        for row in (0, 1):
            big = want_cost[row] > 1e-20
            assert np.max(np.abs(cost[row, big] - want_cost[row, big]) / want_cost[row, big]) < 1e-9, (g, row)
            assert np.all(np.abs(cost[row, ~big]) <= 1e-20), (g, row)
        assert not (status & (hip.TRACK_TOO_FEW | hip.TRACK_NONFINITE)).any(), g
        assert same_bits(got[:, rs.lengths == 0], rs.x_init[:, rs.lengths == 0])


# ---- 3 ------------------------------------------------------------------------------------------------------------
def test_linear_plus_nonlinear_in_one_call_equals_two_calls(hip, sfm):
    rs = tr.ragged_scene(sfm)
    both = hip.TRACKS_LINEAR | hip.TRACKS_NONLINEAR
    lin, lin_cost, lin_status = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, hip.TRACKS_LINEAR, 0.5, 0)
    want_lin, solved = tr.dlt_tracks_reference(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init)
    assert rel(lin, want_lin) < 1e-10
    few = rs.lengths < 2
    assert few.sum() == 6 and np.array_equal(few, ~solved)
    assert np.all(lin_status[few] == hip.TRACK_TOO_FEW) and not (lin_status[~few] & hip.TRACK_TOO_FEW).any()
    assert same_bits(lin[:, few], rs.x_init[:, few])
    assert np.all(lin[3, ~few] == 1.0)
    for g in (0, 1, 8, 64):
        one, cost1, st1 = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, both, 0.5, 10, g)
        two, cost2, st2 = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, lin, hip.TRACKS_NONLINEAR, 0.5, 10, g)
        assert same_bits(one, two) and same_bits(cost1, cost2), g
        assert np.array_equal(st1, st2 | lin_status), g
        assert np.all((st1[few] & hip.TRACK_TOO_FEW) != 0)
        # the three empty tracks keep their input through both passes; the three single observations are refined
        assert same_bits(one[:, rs.lengths == 0], rs.x_init[:, rs.lengths == 0])
    # without X_init the unsolved points start at (0, 0, 0, 1)
    free, _c, st = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, None, hip.TRACKS_LINEAR, 0.5, 0)
    assert same_bits(free[:, ~few], lin[:, ~few]) and np.array_equal(st, lin_status)
    assert np.array_equal(free[:, few], np.tile([[0.0], [0.0], [0.0], [1.0]], (1, 6)))


# ---- 4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_two_identical_calls_give_equal_bits(hip, sfm, group):
    rs = tr.ragged_scene(sfm)
    runs = [hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, hip.TRACKS_LINEAR | hip.TRACKS_NONLINEAR, 0.5, 7, group)
            for _ in range(2)]
    for a, b in zip(*runs):
        assert same_bits(a, b)


# ---- 5 ------------------------------------------------------------------------------------------------------------
def _slice_call(hip, rs, order, lo, hi, group, lam=0.5, iters=5):
    """tri_tracks over points order[lo:hi] of the scene, pt_ptr rebased."""
    pts = order[lo:hi]
    lens = rs.lengths[pts]
    pt_ptr = np.zeros(pts.shape[0] + 1, dtype=np.int32)
    np.cumsum(lens, out=pt_ptr[1:])
    obs = np.concatenate([np.arange(rs.pt_ptr[p], rs.pt_ptr[p + 1]) for p in pts] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return hip.tri_tracks(pt_ptr, rs.cam_idx[obs], rs.uv[:, obs], rs.projs, rs.x_init[:, pts], hip.TRACKS_NONLINEAR, lam, iters, group)


@pytest.mark.parametrize("group", GROUPS)
def test_a_point_does_not_depend_on_the_rest_of_the_batch(hip, sfm, group):
    rs = tr.ragged_scene(sfm)
    n = rs.n_pts
    for order in (np.arange(n), np.random.default_rng(11).permutation(n)):
        whole = _slice_call(hip, rs, order, 0, n, group)
        # two slices (the first a single point), then three (the middle one empty); the short slices hold short tracks
        # only, so they run the register-cached kernels where the whole call re-reads
        for cuts in ((0, 1, n), (0, 20, 20, n)):
            parts = [_slice_call(hip, rs, order, lo, hi, group) for lo, hi in zip(cuts[:-1], cuts[1:])]
            assert [p[0].shape[1] for p in parts] == [hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])]
            assert same_bits(np.hstack([p[0] for p in parts]), whole[0]), cuts
            assert same_bits(np.hstack([p[1] for p in parts]), whole[1]), cuts
            assert same_bits(np.concatenate([p[2] for p in parts]), whole[2]), cuts
    # ... and the permuted call holds the same bits per point as the ordered one
    ordered = _slice_call(hip, rs, np.arange(n), 0, n, group)
    perm = np.random.default_rng(11).permutation(n)
    assert same_bits(whole[0], ordered[0][:, perm]) and same_bits(whole[1], ordered[1][:, perm])


# ---- 6 ------------------------------------------------------------------------------------------------------------
def test_pure_evaluation_returns_the_input(hip, sfm):
    rs = tr.ragged_scene(sfm)
    for g in (0,) + GROUPS:
        got, cost, status = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, hip.TRACKS_NONLINEAR, 0.5, 0, g)
        assert same_bits(got, rs.x_init), g
        assert same_bits(cost[0], cost[1]) and not status.any(), g
        assert rel(cost[0], tr.ragged_reference(sfm, 0.5, 1)[1][0]) < 1e-9


def test_point_on_a_camera_centre_is_returned_unchanged(hip, sfm):
    rs = tr.ragged_scene(sfm)
    # camera 0 of the scene is [I | 0]: the origin projects to s = (0, 0, 0) exactly
    assert np.array_equal(rs.projs[0], np.hstack((np.eye(3), np.zeros((3, 1)))))
    with_cam0 = [p for p in range(rs.n_pts) if rs.lengths[p] >= 2 and rs.cam_idx[rs.pt_ptr[p]] == 0]
    assert with_cam0
    p = with_cam0[0]
    x = rs.x_init.copy()
    x[0:3, p] = 0.0
    for g in (0,) + GROUPS:
        clean = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, hip.TRACKS_NONLINEAR, 0.5, 4, g)
        got, cost, status = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, x, hip.TRACKS_NONLINEAR, 0.5, 4, g)
        assert status[p] & hip.TRACK_NONFINITE, g
        assert same_bits(got[:, p], x[:, p]), g
        others = np.arange(rs.n_pts) != p
        assert same_bits(got[:, others], clean[0][:, others]) and same_bits(cost[:, others], clean[1][:, others]), g
        assert np.array_equal(status[others], clean[2][others]), g


def test_point_behind_a_camera_is_flagged(hip, sfm):
    rs = tr.ragged_scene(sfm)
    sc = rs.scene
    p = int(np.flatnonzero(rs.lengths == 5)[0])
    c = int(rs.cam_idx[rs.pt_ptr[p] + 2])
    rot = sfm.geometry.quaternion_to_rotation_unchecked(sc.cams_true[c, 3:7])
    loc = sc.cams_true[c, 0:3]
    x = rs.x_init.copy()
    x[0:3, p] = loc + rot @ (np.diag([1.0, 1.0, -1.0]) @ (rot.T @ (rs.x_init[0:3, p] - loc)))     # mirrored in the camera's image plane
    assert (rs.projs[c] @ x[:, p])[2] < 0
    for g in (0,) + GROUPS:
        got, _cost, status = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, x, hip.TRACKS_NONLINEAR, 0.5, 0, g)
        assert status[p] & hip.TRACK_BEHIND, g
        assert not (np.delete(status, p) & hip.TRACK_BEHIND).any(), g
        assert same_bits(got, x)


def test_empty_calls_return_ok(hip, sfm):
    rs = tr.ragged_scene(sfm)
    x, cost, status = hip.tri_tracks(np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((2, 0)), rs.projs,
                                     np.zeros((4, 0)), hip.TRACKS_NONLINEAR, 0.5, 3)
    assert x.shape == (4, 0) and cost.shape == (2, 0) and status.shape == (0,)
    x0 = np.ascontiguousarray(rs.x_init[:, :5])
    for mode in (hip.TRACKS_NONLINEAR, hip.TRACKS_LINEAR | hip.TRACKS_NONLINEAR):
        x, cost, status = hip.tri_tracks(np.zeros(6, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((2, 0)), rs.projs,
                                         x0, mode, 0.5, 3)
        assert same_bits(x, x0) and not cost.any()
        assert np.all(status == (hip.TRACK_TOO_FEW if mode & hip.TRACKS_LINEAR else 0))


def test_bad_structure_is_reported_and_nothing_is_written(hip, sfm):
    rs = tr.ragged_scene(sfm)
    lib = hip.load()
    n, m = rs.n_pts, rs.cam_idx.shape[0]
    x_init = np.ascontiguousarray(rs.x_init); uv = np.ascontiguousarray(rs.uv); projs = np.ascontiguousarray(rs.projs)

    def call(pt_ptr, cam_idx):
        out = np.full((4, n), -7.25); cost = np.full((2, n), -7.25); status = np.full(n, -7, dtype=np.int32)
        st = lib.sfm_tri_tracks(n, projs.shape[0], m, hip.iptr(pt_ptr), hip.iptr(cam_idx), hip.dptr(uv), hip.dptr(projs),
                                hip.TRACKS_NONLINEAR, 0.5, 3, 0, hip.dptr(x_init), hip.dptr(out), hip.dptr(cost), hip.iptr(status))
        assert np.all(out == -7.25) and np.all(cost == -7.25) and np.all(status == -7)
        return st, hip.last_error()

    bad_cam = rs.cam_idx.copy()
    bad_cam[100] = projs.shape[0]
    st, msg = call(np.ascontiguousarray(rs.pt_ptr), bad_cam)
    assert st == hip.E_SHAPE and "cam_idx[100]" in msg
    bad_cam[100] = -1
    st, msg = call(np.ascontiguousarray(rs.pt_ptr), bad_cam)
    assert st == hip.E_SHAPE and "cam_idx[100]" in msg
    bad_ptr = rs.pt_ptr.copy()
    bad_ptr[30] = bad_ptr[29] - 1                                               # decreasing at point 29
    st, msg = call(bad_ptr, np.ascontiguousarray(rs.cam_idx))
    assert st == hip.E_SHAPE and "pt_ptr" in msg and "29" in msg
    with pytest.raises(ValueError, match="pt_ptr"):
        hip.tri_tracks(bad_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init)
    # the library is as usable afterwards as before
    got, _c, _s = hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, hip.TRACKS_NONLINEAR, 5.0, 3)
    assert rel(got, tr.ragged_reference(sfm, 5.0, 3)[0]) < 1e-9


# ---- 7 ------------------------------------------------------------------------------------------------------------
def _resident_scenes(sfm):
    return {"bernoulli": sfm.scenes.make_scene(6, 120, 0.6, seed=12),
            "tracks": sfm.scenes.make_scene(9, 150, seed=13, structure=sfm.scenes.Structure(mean_track=3.0, heavy=0.1, single=0.05))}


@pytest.mark.parametrize("kind", ["bernoulli", "tracks"])
def test_refine_points_on_the_resident_scene(hip, sfm, kind):
    sc = _resident_scenes(sfm)[kind]
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob, hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as twin:
        prob.set_state(sc.cams_init, sc.pts_init)
        prob.iterate(5.0, 1)
        cams0, pts0 = prob.get_state()
        before = prob.upload_bytes
        cost, status = prob.refine_points(0.5, 10)
        assert prob.upload_bytes == before                                       # nothing goes up
        cams1, pts1 = prob.get_state()
        assert same_bits(cams1, cams0)
        assert prob.get_stats().shape[0] == 0                                    # the cost history restarts, as after set_points
        pt_ptr, cam_idx, uv = prob.structure()
        x0 = np.vstack((pts0, np.ones((1, sc.n_pts))))
        want, want_cost, want_status = hip.tri_tracks(pt_ptr, cam_idx, uv, tr.camera_projections(sfm, cams0), x0,
                                                      hip.TRACKS_NONLINEAR, 0.5, 10)
        assert rel(pts1, want[0:3]) < 1e-9 and rel(cost, want_cost) < 1e-9 and np.array_equal(status, want_status)
        assert np.all(cost[1] <= cost[0])
        # cost row 0 is the bundle adjustment's cost at the same state
        twin.set_state(cams0, pts0)
        twin.iterate(5.0, 1)
        ba_cost = twin.get_stats()[0]
        assert abs(cost[0].sum() - ba_cost) < 1e-12 * ba_cost
        # DLT first, in place
        prob.set_state(cams0, pts0)
        cost_l, status_l = prob.refine_points(0.5, 10, hip.TRACKS_LINEAR | hip.TRACKS_NONLINEAR)
        want_l, want_cost_l, want_status_l = hip.tri_tracks(pt_ptr, cam_idx, uv, tr.camera_projections(sfm, cams0), x0,
                                                            hip.TRACKS_LINEAR | hip.TRACKS_NONLINEAR, 0.5, 10)
        assert rel(prob.get_state()[1], want_l[0:3]) < 1e-9 and rel(cost_l, want_cost_l) < 1e-9
        assert np.array_equal(status_l, want_status_l)
        assert prob.refine_points(0.5, 2, want_outputs=False) is None


@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("graph", [0, 1])
def test_refine_points_leaves_no_stale_state_behind(hip, sfm, graph, pending):
    """iterate, refine_points, iterate under SFM_OPT_DETERMINISTIC ends in the bits of a fresh problem started from the
    state refine_points left.  ``pending``: the first phase is spelled linearize_reduce / solve_update, so the back
    substitution of its last iteration is still owed when refine_points is called."""
    sc = _resident_scenes(sfm)["bernoulli"]
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)

    def fresh():
        p = hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn)
        p.set_option(hip.OPT_DETERMINISTIC, 1)
        p.set_option(hip.OPT_GRAPH, graph)
        return p

    with fresh() as prob, fresh() as other:
        prob.set_state(sc.cams_init, sc.pts_init)
        if pending:
            for _ in range(2):
                prob.linearize_reduce(5.0)
                prob.solve_update(5.0)
        else:
            prob.iterate(5.0, 2)
        cost, _status = prob.refine_points(0.5, 5)
        assert np.all(cost[1] <= cost[0])
        cams_mid, pts_mid = prob.get_state()
        prob.iterate(5.0, 2)
        assert prob.get_stats().shape[0] == 2
        cams_end, pts_end = prob.get_state()
        other.set_state(cams_mid, pts_mid)
        other.iterate(5.0, 2)
        cams_want, pts_want = other.get_state()
        assert same_bits(cams_end, cams_want) and same_bits(pts_end, pts_want)
        assert same_bits(prob.get_stats(), other.get_stats())


def test_refine_points_on_an_empty_problem(hip):
    with hip.BaProblem(2, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((2, 0))) as prob:
        cost, status = prob.refine_points(0.5, 3)
        assert cost.shape == (2, 0) and status.shape == (0,)
    with pytest.raises(ValueError, match="group"):
        with hip.BaProblem(2, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((2, 0))) as prob:
            prob.refine_points(0.5, 3, group=3)


# ---- 8 ------------------------------------------------------------------------------------------------------------
class _View:
    def __init__(self, rot, loc, k, xy, key_pts, descriptors):
        self.rot, self.loc, self.k = rot, loc, k
        self.key_xy, self.key_pts, self.key_descriptors = xy, key_pts, descriptors

    def update_cam_pose(self, rot, loc):
        self.rot, self.loc = rot, loc


class _Holder:
    pass


class _Loop:
    """A small incremental run through HipDeviceKeyTracker and HipBaProcessor: key 0 of a view is a dummy, key p + 1
    observes point p; view c brings PER_VIEW new points, seen by the two views before it and by itself, and sees the
    older points whose index plus c is even -- tracks of different lengths."""
    PER_VIEW = 40

    def __init__(self, sfm, sc, device_tracks):
        P = sfm.processors
        self.sfm, self.sc = sfm, sc
        self.vp = _Holder()
        self.vp.view_list = []
        self.tp = P.HipTriangulationProcessor(0.5, 12)
        self.tp.tri_pts = np.zeros((4, 0))
        self.kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
        self.bp = P.HipBaProcessor(self.vp, self.kt, None, self.tp, None, iteration=3, damping_factor=5)
        self.bp.ba_verbose = False
        self.bp.ba_device_tracks = device_tracks
        self.rng = np.random.default_rng(5)

    def close(self):
        self.bp.ba_release()
        self.kt.kt_release()

    def register(self, c):
        sc, g = self.sc, self.sfm.geometry
        pix = sc.uv_pix[:, sc.cam_idx == c].T
        xy = np.vstack(([[-1.0, -1.0]], pix)).astype(np.float32).astype(np.float64)
        rot = g.quaternion_to_rotation(sc.cams_init[c, 3:7] / np.linalg.norm(sc.cams_init[c, 3:7]))
        view = _View(rot, sc.cams_init[c, 0:3].reshape(3, 1).copy(), sc.intrinsic.copy(), xy,
                     [self.sfm.scenes.KeyPoint(x, y) for x, y in xy], self.rng.integers(0, 256, (xy.shape[0], 128)).astype(np.uint8))
        self.kt.add_new_view(view, self.vp.view_list)
        self.vp.view_list.append(view)
        if c == 0:
            return
        n_old = self.tp.tri_pts.shape[1]
        new = np.arange(n_old, n_old + self.PER_VIEW)
        self.tp.tri_pts = np.hstack((self.tp.tri_pts, np.vstack((sc.pts_init[:, new], np.ones((1, new.size))))))
        for v in range(max(0, c - 2), c):
            self.kt.track_list[v].update_usage((new + 1)[np.newaxis, :], new[np.newaxis, :])
        old = np.arange(n_old)
        seen = np.concatenate((old[(old + c) % 2 == 0], new))
        self.kt.track_list[c].update_usage((seen + 1)[np.newaxis, :], seen[np.newaxis, :])

    def poses(self):
        return np.stack([self.sfm.geometry.pack_camera(v.rot, v.loc) for v in self.vp.view_list])


@pytest.mark.parametrize("device_tracks", [False, True])
def test_refine_structure_on_a_small_incremental_run(hip, sfm, device_tracks):
    sc = sfm.scenes.make_scene(5, 4 * _Loop.PER_VIEW, 1.0, seed=53, pixel_noise=0.3)
    run = _Loop(sfm, sc, device_tracks)
    try:
        run.register(0)
        for c in range(1, 5):
            run.register(c)
            run.bp._BaProcessor__execute_bundle_adjustment()
        bp, tp = run.bp, run.tp
        prob = bp._hip_scene.prob
        pt_ptr, cam_idx, uv = prob.structure()
        assert len(set(np.diff(pt_ptr).tolist())) > 1                           # a ragged structure
        poses = run.poses()
        views_before = [(v.rot.copy(), v.loc.copy()) for v in run.vp.view_list]
        x0 = tp.tri_pts.copy()
        up = bp.ba_upload_bytes
        cost, status = bp.refine_structure()
        assert bp.ba_last_action == "reuse" and bp.ba_upload_bytes == up
        want, want_cost = tr.refine_tracks_reference(pt_ptr, cam_idx, uv, tr.camera_projections(sfm, poses), x0, 0.5, 12)
        assert rel(tp.tri_pts[0:3], want[0:3]) < 1e-9 and rel(cost, want_cost) < 1e-9
        assert same_bits(tp.tri_pts[3], x0[3]) and not status.any()
        for v, (r, l) in zip(run.vp.view_list, views_before):
            assert same_bits(v.rot, r) and same_bits(v.loc, l)
        # a second call: nothing goes up; explicit arguments and the DLT start
        x1 = tp.tri_pts.copy()
        cost2, _st = bp.refine_structure(damping_factor=5, iteration=3)
        assert bp.ba_upload_bytes == up
        want2, want_cost2 = tr.refine_tracks_reference(pt_ptr, cam_idx, uv, tr.camera_projections(sfm, poses), x1, 5, 3)
        assert rel(tp.tri_pts[0:3], want2[0:3]) < 1e-9 and rel(cost2, want_cost2) < 1e-9
        bp.refine_structure(relinearize=True)
        assert bp.ba_upload_bytes == up
        lin = tr.dlt_tracks_reference(pt_ptr, cam_idx, uv, tr.camera_projections(sfm, poses), tp.tri_pts)[0]
        want3 = tr.refine_tracks_reference(pt_ptr, cam_idx, uv, tr.camera_projections(sfm, poses), lin, 0.5, 12)[0]
        assert rel(tp.tri_pts[0:3], want3[0:3]) < 1e-9
        # the next bundle adjustment finds everything in place
        x3 = tp.tri_pts.copy()
        bp._BaProcessor__execute_bundle_adjustment()
        assert bp.ba_last_action == "reuse" and bp.ba_upload_bytes == up
        with hip.BaProblem(5, pt_ptr, cam_idx, uv) as ref:
            ref.set_state(poses, x3[0:3])
            ref.iterate(5, 3)
            cams_want, pts_want = ref.get_state()
        assert rel(run.poses(), cams_want) < 1e-9 and rel(tp.tri_pts[0:3], pts_want) < 1e-9
    finally:
        run.close()


def test_triangulate_tracks_equals_native(hip, sfm):
    rs = tr.ragged_scene(sfm)
    tp = sfm.processors.HipTriangulationProcessor(0.5, 9)
    projs = [p for p in rs.projs]
    got = tp.triangulate_tracks(projs, rs.pt_ptr, rs.cam_idx, rs.uv, rs.x_init)
    assert same_bits(got, hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, hip.TRACKS_NONLINEAR, 0.5, 9)[0])
    got = tp.triangulate_tracks(projs, rs.pt_ptr, rs.cam_idx, rs.uv)
    assert same_bits(got, hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, None, hip.TRACKS_LINEAR | hip.TRACKS_NONLINEAR, 0.5, 9)[0])
    got = tp.triangulate_tracks(projs, rs.pt_ptr, rs.cam_idx, rs.uv, rs.x_init, damping_factor=5, iteration=2)
    assert same_bits(got, hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, hip.TRACKS_NONLINEAR, 5, 2)[0])
    # falsy arguments fall back to the instance's values, as in the reference's methods
    got = tp.triangulate_tracks(projs, rs.pt_ptr, rs.cam_idx, rs.uv, rs.x_init, damping_factor=0, iteration=0)
    assert same_bits(got, hip.tri_tracks(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, hip.TRACKS_NONLINEAR, 0.5, 9)[0])
