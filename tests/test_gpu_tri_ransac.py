"""GPU tests of the robust triangulation of ragged tracks: sfm_tri_tracks_ransac, its _dev form, sfm_ba_retriangulate and
the drop-in methods, against the float64 NumPy reference of tests/_tri_ransac_reference.py.

Decisions (best_hyp, masks, counts, status, summary) are compared EXACTLY on the points the reference calls settled --
those whose decisions do not change when the threshold moves by 1e-6 relative and whose winner leads its best
equal-count rival by more than 1e-9 in the cosine; points are compared at the suite's parity bound, 1e-9 relative (the
angle gate at 1.5 degrees keeps the conditioning of a two-ray solve near 1 / sin^2(1.5 deg) = 1.5e3).

The winner's inlier count BEFORE the refit is not an output of the C-ABI; it is a function of best_hyp and the track
alone (one lane, integers), so the group-independence test checks best_hyp and the status bits, which determine it."""
import numpy as np
import pytest

import _tracks_reference as tr
import _tri_ransac_reference as rr

pytestmark = pytest.mark.gpu

GROUPS = rr.GROUPS


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b)))) if a.size else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(hip, sc, group=0, x_init=None, cos_min=rr.COS_MIN, max_hyp=128, lam=0.5, iters=3):
    return hip.tri_tracks_ransac(sc.pt_ptr, sc.cam_idx, sc.uv, sc.projs, rr.MAX_ERR2, cos_min, max_hyp, lam, iters, sc.cam_scale,
                                 x_init, group)


def obs_mask(sc, pts):
    """Boolean (M,) mask of the observations of the points flagged in pts (n_pts,)."""
    return np.repeat(np.asarray(pts, dtype=bool), sc.lengths)


def subset(sc, pts):
    """The scene restricted to the points `pts` (in that order), as a namespace with the fields `run` reads."""
    from types import SimpleNamespace
    pts = np.asarray(pts, dtype=np.int64)
    obs = np.concatenate([np.arange(sc.pt_ptr[p], sc.pt_ptr[p + 1]) for p in pts] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    pt_ptr = np.zeros(pts.shape[0] + 1, dtype=np.int32)
    np.cumsum(sc.lengths[pts], out=pt_ptr[1:])
    return SimpleNamespace(pt_ptr=pt_ptr, cam_idx=np.ascontiguousarray(sc.cam_idx[obs]), uv=np.ascontiguousarray(sc.uv[:, obs]),
                           projs=sc.projs, cam_scale=sc.cam_scale, lengths=sc.lengths[pts], obs=obs)


def err2_at(sc, X):
    """err2 (M,) and s2 (M,) of every observation at its point's column of X (4, n_pts)."""
    P = sc.projs[sc.cam_idx]
    s = np.einsum("mrc,mc->mr", P[:, :, 0:3], X[0:3, sc.pt_idx].T) + P[:, :, 3]
    with np.errstate(all="ignore"):
        e = sc.cam_scale[sc.cam_idx] ** 2 * ((s[:, 0] / s[:, 2] - sc.uv[0]) ** 2 + (s[:, 1] / s[:, 2] - sc.uv[1]) ** 2)
    return e, s[:, 2]


# ---- 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["proto0", "proto1", "proto2", "paths"])
def test_parity_with_the_reference(hip, name):
    sc, ref = rr.scene_and_reference(name)
    ok = ref.settled
    assert (~ok).sum() <= 0.02 * sc.n_pts
    ok_obs = obs_mask(sc, ok)
    solved = ok & (ref.best_hyp >= 0)
    for g in GROUPS:
        X, inlier, n_in, best, status, summary = run(hip, sc, g)
        assert np.array_equal(best[ok], ref.best_hyp[ok]), g
        assert np.array_equal(n_in[ok], ref.n_inliers[ok]), g
        assert np.array_equal(inlier[ok_obs], ref.inlier[ok_obs]), g
        assert np.array_equal(status[ok], ref.status[ok]), g
        if ok.all():
            assert np.array_equal(summary, ref.summary), g
        assert rel(X[:, solved], ref.X[:, solved]) < 1e-9, g
        assert same_bits(X[:, ok & ~solved], ref.X[:, ok & ~solved]), g
        # whatever was decided on an unsettled point is consistent with the point that came back
        counts = np.add.reduceat(np.concatenate((inlier, [0])).astype(np.int64), np.minimum(sc.pt_ptr[:-1], inlier.shape[0]))
        counts[sc.lengths == 0] = 0
        assert np.array_equal(counts, n_in), g
        e, s2 = err2_at(sc, X)
        flagged = inlier.astype(bool)
        assert np.all(e[flagged] <= rr.MAX_ERR2 * (1.0 + 1e-6)) and np.all(s2[flagged] > 0.0), g
        assert summary[0] + summary[1] + summary[2] == sc.n_pts and summary[4] == inlier.sum(), g


# ---- 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["proto2", "paths"])
def test_the_winner_does_not_depend_on_the_group_width(hip, name):
    sc, _ref = rr.scene_and_reference(name)
    bits = hip.RANSAC_NO_MODEL | hip.RANSAC_TOO_FEW | hip.RANSAC_SAMPLED
    for kw in (dict(), dict(max_hyp=7), dict(cos_min=1.0, iters=0)):
        runs = {g: run(hip, sc, g, **kw) for g in GROUPS}
        for g in GROUPS[1:]:
            assert np.array_equal(runs[g][3], runs[GROUPS[0]][3]), (g, kw)
            assert np.array_equal(runs[g][4] & bits, runs[GROUPS[0]][4] & bits), (g, kw)
            # where the hypothesis itself stands, the final count is the winner's: equal as well
            kept = (runs[g][4] & runs[GROUPS[0]][4] & hip.RANSAC_KEPT_HYPOTHESIS) != 0
            assert np.array_equal(runs[g][2][kept], runs[GROUPS[0]][2][kept]), (g, kw)
    sampled = (runs[0][4] & hip.RANSAC_SAMPLED) != 0
    assert np.array_equal(sampled, sc.lengths * (sc.lengths - 1) // 2 > 128)


# ---- 3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS[1:])
def test_a_point_does_not_depend_on_the_rest_of_the_batch(hip, group):
    sc, _ref = rr.scene_and_reference("paths")
    n = sc.n_pts
    whole = run(hip, sc, group)

    def check(pts, got):
        sub_obs = np.concatenate([np.arange(sc.pt_ptr[p], sc.pt_ptr[p + 1]) for p in pts] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        assert same_bits(got[0], whole[0][:, pts]) and same_bits(got[1], whole[1][sub_obs])
        for k in (2, 3, 4):
            assert np.array_equal(got[k], whole[k][pts])

    perm = np.random.default_rng(3).permutation(n)
    check(perm, run(hip, subset(sc, perm), group))
    # without the tracks that are staged tile by tile at this width, and next to them
    short = np.flatnonzero(sc.lengths <= 6 * group)
    assert 0 < short.shape[0] < n
    check(short, run(hip, subset(sc, short), group))
    # alone: one point of every path
    for length in (2, 3, 17, 25, 385, 700):
        p = np.flatnonzero(sc.lengths == length)[0:1]
        check(p, run(hip, subset(sc, p), group))


# ---- 4 ------------------------------------------------------------------------------------------------------------
def test_points_without_a_model_come_out_as_they_went_in(hip):
    sc, ref = rr.scene_and_reference("paths")
    rng = np.random.default_rng(8)
    x_init = np.vstack((sc.pts_true + 0.1 * rng.standard_normal(sc.pts_true.shape), rng.uniform(0.5, 2.0, (1, sc.n_pts))))
    few = sc.lengths < 2
    for g in GROUPS:
        # the gate at -1 refuses every hypothesis
        X, inlier, n_in, best, status, summary = run(hip, sc, g, x_init, cos_min=-1.0)
        assert same_bits(X, x_init), g
        assert not inlier.any() and not n_in.any() and np.all(best == -1), g
        assert np.all(status[few] == hip.RANSAC_TOO_FEW) and np.all((status[~few] & ~hip.RANSAC_SAMPLED) == hip.RANSAC_NO_MODEL), g
        assert summary.tolist() == [0, int((~few).sum()), int(few.sum()), 0, 0, 0], g
        # the usual gate: the tracks of 0 and 1 keep their input, everything else is solved
        X, inlier, n_in, best, status, summary = run(hip, sc, g, x_init)
        assert same_bits(X[:, few], x_init[:, few]) and np.all(status[few] == hip.RANSAC_TOO_FEW), g
        assert np.all(X[3, ~few] == 1.0) and np.array_equal(best, ref.best_hyp), g
        # ... and without X_init they are (0, 0, 0, 1)
        X = run(hip, sc, g)[0]
        assert np.array_equal(X[:, few], np.tile([[0.0], [0.0], [0.0], [1.0]], (1, int(few.sum())))), g


def test_a_track_behind_its_cameras_has_no_model(hip):
    """Views V .. 2V - 1 are the negated projections of views 0 .. V - 1: the same keys and the same pair solutions, but
    s2 < 0 for every observation, so no observation is an inlier of anything."""
    from types import SimpleNamespace
    sc, ref = rr.scene_and_reference("proto0")
    V = sc.n_views
    p = int(np.flatnonzero(sc.lengths == 5)[0])
    cam = sc.cam_idx.copy()
    cam[sc.pt_ptr[p]:sc.pt_ptr[p + 1]] += V
    both = SimpleNamespace(pt_ptr=sc.pt_ptr, cam_idx=cam, uv=sc.uv, projs=np.concatenate((sc.projs, -sc.projs)),
                           cam_scale=np.concatenate((sc.cam_scale, sc.cam_scale)))
    x_init = np.vstack((sc.pts_true, np.ones((1, sc.n_pts))))
    others = np.arange(sc.n_pts) != p
    for g in GROUPS:
        X, inlier, n_in, best, status, _summary = run(hip, both, g, x_init)
        assert status[p] == hip.RANSAC_NO_MODEL and best[p] == -1 and n_in[p] == 0, g
        assert same_bits(X[:, p], x_init[:, p]) and not inlier[sc.pt_ptr[p]:sc.pt_ptr[p + 1]].any(), g
        assert np.array_equal(best[others], ref.best_hyp[others]), g


# ---- 5 ------------------------------------------------------------------------------------------------------------
def test_displaced_observations_are_found(hip, capsys):
    """A displacement of 30 px at f = 800 and a depth of 6 moves a ray by 0.22 units; shared among at most 6 observations
    the least-squares point moves by more than 0.03, where the noise of 0.5 px moves it by 4e-3 / sqrt(n).  So the plain
    triangulation of a contaminated track is expected at least ten times farther from the triangulation of its clean
    observations than the robust one."""
    sc, ref = rr.scene_and_reference("proto0")
    clean = ~sc.displaced
    n_clean = np.add.reduceat(np.concatenate((clean, [False])).astype(np.int64), np.minimum(sc.pt_ptr[:-1], clean.shape[0]))
    n_clean[sc.lengths == 0] = 0
    dirty = np.flatnonzero((n_clean >= 3) & (n_clean < sc.lengths))
    assert dirty.shape[0] > 50
    both = hip.TRACKS_LINEAR | hip.TRACKS_NONLINEAR
    plain = hip.tri_tracks(sc.pt_ptr, sc.cam_idx, sc.uv, sc.projs, None, both, 0.5, 3)[0]
    keep = np.flatnonzero(clean)
    ptr_clean = np.concatenate(([0], np.cumsum(n_clean))).astype(np.int32)
    want = hip.tri_tracks(ptr_clean, sc.cam_idx[keep], np.ascontiguousarray(sc.uv[:, keep]), sc.projs, None, both, 0.5, 3)[0]
    X, inlier, _n, best, _status, _summary = run(hip, sc)

    def rms(a):
        return float(np.sqrt(np.mean(np.sum((a[0:3, dirty] / a[3, dirty] - want[0:3, dirty] / want[3, dirty]) ** 2, axis=0))))

    with capsys.disabled():
        print("\n%d contaminated tracks: RMS distance from the clean-only triangulation %.3e plain, %.3e robust"
              % (dirty.shape[0], rms(plain), rms(X)))
    assert rms(plain) > 0.03 and rms(X) < 0.1 * rms(plain)
    ok = ref.settled & (ref.best_hyp >= 0)
    assert rel(X[:, ok], ref.X[:, ok]) < 1e-9
    assert np.array_equal(inlier[obs_mask(sc, ref.settled)], ref.inlier[obs_mask(sc, ref.settled)])
    assert np.array_equal(inlier[obs_mask(sc, dirty_mask(sc, dirty))].astype(bool), clean[obs_mask(sc, dirty_mask(sc, dirty))])


def dirty_mask(sc, idx):
    m = np.zeros(sc.n_pts, dtype=bool)
    m[idx] = True
    return m


# ---- 6 ------------------------------------------------------------------------------------------------------------
def _resident(sfm, name="proto0"):
    sc, ref = rr.scene_and_reference(name)
    cams = np.stack([sfm.geometry.pack_camera(sc.rots[c], sc.centres[c]) for c in range(sc.n_views)])
    pts0 = sc.pts_true + 0.05 * np.random.default_rng(21).standard_normal(sc.pts_true.shape)
    return sc, ref, cams, pts0


def test_retriangulate_equals_the_free_form(hip, sfm):
    sc, ref, cams, pts0 = _resident(sfm)
    with hip.BaProblem(sc.n_views, sc.pt_ptr, sc.cam_idx, sc.uv) as prob:
        prob.set_state(cams, pts0)
        prob.iterate(5.0, 1)
        cams0, pts_before = prob.get_state()
        before = prob.upload_bytes
        out = prob.retriangulate(rr.MAX_ERR2, rr.COS_MIN, 128, 0.5, 3, sc.cam_scale)
        assert prob.upload_bytes == before + 8 * sc.n_views                       # the scales, nothing else
        cams1, pts1 = prob.get_state()
        assert same_bits(cams1, cams0)
        assert prob.get_stats().shape[0] == 0                                     # the cost history restarts, as after set_points
        pt_ptr, cam_idx, uv = prob.structure()
        x0 = np.vstack((pts_before, np.ones((1, sc.n_pts))))
        X, inlier, n_in, best, status, summary = hip.tri_tracks_ransac(pt_ptr, cam_idx, uv, tr.camera_projections(sfm, cams0),
                                                                       rr.MAX_ERR2, rr.COS_MIN, 128, 0.5, 3, sc.cam_scale, x0)
        assert rel(pts1, X[0:3]) < 1e-9
        assert np.array_equal(out.inlier, inlier) and np.array_equal(out.n_inliers, n_in)
        assert np.array_equal(out.best_hyp, best) and np.array_equal(out.status, status) and np.array_equal(out.summary, summary)
        unsolved = best < 0
        assert unsolved.any() and same_bits(pts1[:, unsolved], pts_before[:, unsolved])
        assert prob.retriangulate(rr.MAX_ERR2, want_outputs=False) is None
        with pytest.raises(ValueError, match="group"):
            prob.retriangulate(rr.MAX_ERR2, group=3)
        with pytest.raises(ValueError, match="max_hyp"):
            hip.check(hip.load().sfm_ba_retriangulate(prob._h, 16.0, 1.0, 65537, 0.5, 3, 0, None, None, None, None, None, None))


@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("graph", [0, 1])
def test_retriangulate_leaves_no_stale_state_behind(hip, sfm, graph, pending):
    """iterate, retriangulate, iterate under SFM_OPT_DETERMINISTIC ends in the bits of a fresh problem started from the
    state retriangulate left.  ``pending``: the first phase is spelled linearize_reduce / solve_update, so the back
    substitution of its last iteration is still owed when retriangulate is called."""
    sc, _ref, cams, pts0 = _resident(sfm)

    def fresh():
        p = hip.BaProblem(sc.n_views, sc.pt_ptr, sc.cam_idx, sc.uv)
        p.set_option(hip.OPT_DETERMINISTIC, 1)
        p.set_option(hip.OPT_GRAPH, graph)
        return p

    with fresh() as prob, fresh() as other:
        prob.set_state(cams, pts0)
        if pending:
            for _ in range(2):
                prob.linearize_reduce(5.0)
                prob.solve_update(5.0)
        else:
            prob.iterate(5.0, 2)
        out = prob.retriangulate(rr.MAX_ERR2, rr.COS_MIN, 128, 0.5, 3, sc.cam_scale)
        assert out.summary[0] > 0.9 * sc.n_pts
        cams_mid, pts_mid = prob.get_state()
        prob.iterate(5.0, 2)
        assert prob.get_stats().shape[0] == 2
        cams_end, pts_end = prob.get_state()
        other.set_state(cams_mid, pts_mid)
        other.iterate(5.0, 2)
        cams_want, pts_want = other.get_state()
        assert same_bits(cams_end, cams_want) and same_bits(pts_end, pts_want)
        assert same_bits(prob.get_stats(), other.get_stats())


def test_retriangulate_then_cull_removes_what_was_flagged(hip, sfm):
    sc, _ref, cams, pts0 = _resident(sfm)
    with hip.BaProblem(sc.n_views, sc.pt_ptr, sc.cam_idx, sc.uv) as prob:
        prob.set_state(cams, pts0)
        out = prob.retriangulate(rr.MAX_ERR2, rr.COS_MIN, 128, 0.5, 3, sc.cam_scale)
        solved = out.best_hyp >= 0
        report = prob.cull(rr.MAX_ERR2, 1.0, 2, sc.cam_scale)
        of_solved = obs_mask(sc, solved)
        assert np.array_equal(report.obs_flags[of_solved] == 0, out.inlier[of_solved] != 0)
        pt_ptr, cam_idx, _uv = prob.structure(want_uv=False)
        assert np.array_equal(np.diff(pt_ptr)[solved], out.n_inliers[solved])
        kept_of_solved = np.flatnonzero(of_solved & (out.inlier != 0))
        new_of_solved = obs_mask(SimpleLengths(np.diff(pt_ptr)), solved)
        assert np.array_equal(cam_idx[new_of_solved], sc.cam_idx[kept_of_solved])
        assert out.summary[5] > 0 and (report.obs_flags[of_solved] != 0).sum() == out.summary[5]


class SimpleLengths:
    def __init__(self, lengths):
        self.lengths = lengths


def test_retriangulate_on_an_empty_problem(hip):
    with hip.BaProblem(2, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((2, 0))) as prob:
        out = prob.retriangulate(16.0)
        assert out.inlier.shape == (0,) and out.status.shape == (0,) and not out.summary.any()
    X, inlier, n_in, best, status, summary = hip.tri_tracks_ransac(np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32),
                                                                   np.zeros((2, 0)), np.zeros((1, 3, 4)), 16.0)
    assert X.shape == (4, 0) and inlier.shape == (0,) and not summary.any()
    # points, but no observation at all
    X, inlier, n_in, best, status, summary = hip.tri_tracks_ransac(np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32),
                                                                   np.zeros((2, 0)), np.zeros((1, 3, 4)), 16.0)
    assert np.array_equal(X, np.tile([[0.0], [0.0], [0.0], [1.0]], (1, 3))) and np.all(status == hip.RANSAC_TOO_FEW)
    assert summary.tolist() == [0, 0, 3, 0, 0, 0] and np.all(best == -1)


def test_bad_arguments_launch_nothing(hip):
    sc, _ref = rr.scene_and_reference("proto0")
    lib = hip.load()
    n, m = sc.n_pts, sc.cam_idx.shape[0]
    uv = np.ascontiguousarray(sc.uv); projs = np.ascontiguousarray(sc.projs)

    def call(max_err2=16.0, cos_min=0.9, max_hyp=128, lam=0.5, iters=3, group=0, cam_idx=sc.cam_idx):
        out = np.full((4, n), -7.25); status = np.full(n, -7, dtype=np.int32)
        st = lib.sfm_tri_tracks_ransac(n, projs.shape[0], m, hip.iptr(sc.pt_ptr), hip.iptr(cam_idx), hip.dptr(uv), hip.dptr(projs),
                                       None, max_err2, cos_min, max_hyp, lam, iters, group, None, hip.dptr(out), None, None, None,
                                       hip.iptr(status), None)
        assert np.all(out == -7.25) and np.all(status == -7)
        return st, hip.last_error()

    for kw in (dict(max_err2=float("nan")), dict(max_err2=-1.0), dict(cos_min=-1.5), dict(cos_min=float("nan")), dict(max_hyp=-1),
               dict(max_hyp=65537), dict(iters=-1), dict(lam=-1.0), dict(lam=float("nan"))):
        st, msg = call(**kw)
        assert st == hip.E_SHAPE and list(kw)[0].replace("cos_min", "cos_min_angle").replace("lam", "lambda") in msg, kw
    st, msg = call(group=3)
    assert st == hip.E_SHAPE and "group 3 is not one of 0, 1, 4, 8, 16, 32, 64" in msg
    bad_cam = sc.cam_idx.copy()
    bad_cam[100] = projs.shape[0]
    st, msg = call(cam_idx=bad_cam)
    assert st == hip.E_SHAPE and "cam_idx[100]" in msg


# ---- 7 ------------------------------------------------------------------------------------------------------------
def test_dev_form_in_place_on_a_callers_stream(hip):
    import torch
    sc, ref = rr.scene_and_reference("paths")
    x_init = np.vstack((sc.pts_true + 0.1, np.ones((1, sc.n_pts))))
    want = run(hip, sc, 8, x_init)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_ptr = torch.from_numpy(sc.pt_ptr).to(dev); d_cam = torch.from_numpy(sc.cam_idx).to(dev)
        d_uv = torch.from_numpy(sc.uv).to(dev); d_projs = torch.from_numpy(np.ascontiguousarray(sc.projs)).to(dev)
        d_scale = torch.from_numpy(sc.cam_scale).to(dev)
        d_x = torch.from_numpy(x_init).to(dev)
        d_in = torch.zeros(sc.cam_idx.shape[0], dtype=torch.uint8, device=dev)
        d_n = torch.zeros(sc.n_pts, dtype=torch.int32, device=dev); d_best = torch.zeros_like(d_n); d_st = torch.zeros_like(d_n)
        d_sum = torch.zeros(6, dtype=torch.int64, device=dev)
        stream.synchronize()
        hip.tri_tracks_ransac_dev(sc.n_pts, sc.n_views, sc.cam_idx.shape[0], d_ptr.data_ptr(), d_cam.data_ptr(), d_uv.data_ptr(),
                                  d_projs.data_ptr(), rr.MAX_ERR2, rr.COS_MIN, 128, 0.5, 3, 8, d_scale.data_ptr(), d_x.data_ptr(),
                                  d_x.data_ptr(), d_in.data_ptr(), d_n.data_ptr(), d_best.data_ptr(), d_st.data_ptr(),
                                  d_sum.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    got = (d_x.cpu().numpy(), d_in.cpu().numpy(), d_n.cpu().numpy(), d_best.cpu().numpy(), d_st.cpu().numpy(), d_sum.cpu().numpy())
    for a, b in zip(got, want):
        assert same_bits(a, b)
    # without the optional arrays
    d_y = torch.zeros_like(d_x)
    hip.tri_tracks_ransac_dev(sc.n_pts, sc.n_views, sc.cam_idx.shape[0], d_ptr.data_ptr(), d_cam.data_ptr(), d_uv.data_ptr(),
                              d_projs.data_ptr(), rr.MAX_ERR2, rr.COS_MIN, 128, 0.5, 3, 8, d_scale.data_ptr(), 0, d_y.data_ptr())
    torch.cuda.synchronize()
    assert same_bits(d_y.cpu().numpy(), run(hip, sc, 8)[0])


# ---- 8 ------------------------------------------------------------------------------------------------------------
def _subset_scene():
    """14 cameras, 70 points, track lengths cycling through 0, 1, 2, 3, 5, 7, 13: an empty track, one too short, tracks a
    lane keeps in registers and, at group 1, tracks beyond 6 G (the re-reading kernel, the tile-by-tile scoring)."""
    rng = np.random.default_rng(105)
    rots, C = rr._cameras(14, 120.0)
    lengths = np.resize(np.array([0, 1, 2, 3, 5, 7, 13]), 70)
    pts = rng.uniform(-rr.CUBE / 2.0, rr.CUBE / 2.0, (3, 70))
    pt_ptr = np.concatenate(([0], np.cumsum(lengths)))
    cam_idx = np.concatenate([np.sort(rng.choice(14, n, replace=False)) for n in lengths]).astype(np.int64)
    return rr._finish(rots, C, pts, pt_ptr, cam_idx, rng, rng.random(cam_idx.shape[0]) < rr.BAD_SHARE)


@pytest.mark.parametrize("group", [1, 8])
def test_any_subset_of_the_outputs_gives_the_same_bytes(hip, group):
    """Through the raw C calls: what a call computes does not depend on which optional outputs it was asked for."""
    sc = _subset_scene()
    lib = hip.load()
    n, m = sc.n_pts, sc.cam_idx.shape[0]
    projs = np.ascontiguousarray(sc.projs)
    names = ("inlier", "n_inliers", "best_hyp", "status", "summary")

    def ransac(wanted):
        o = hip._ransac_outputs(n, m)
        X = np.full((4, n), -7.25)
        ptrs = [p if k in wanted else None for k, p in zip(names, hip._ransac_pointers(o))]
        hip.check(lib.sfm_tri_tracks_ransac(n, 14, m, hip.iptr(sc.pt_ptr), hip.iptr(sc.cam_idx), hip.dptr(sc.uv), hip.dptr(projs),
                                            hip.dptr(sc.cam_scale), rr.MAX_ERR2, rr.COS_MIN, 128, 0.5, 3, group, None, hip.dptr(X),
                                            *ptrs))
        return X, o

    X_all, o_all = ransac(names)
    assert o_all.summary[0] > 0 and o_all.summary[2] == 20 and o_all.inlier.any()      # the call did solve something
    for wanted in [()] + [(k,) for k in names]:
        X, o = ransac(wanted)
        assert same_bits(X, X_all), wanted
        for k in names:
            got = getattr(o, k)
            assert same_bits(got, getattr(o_all, k)) if k in wanted else not got.any(), (wanted, k)

    def tracks(want_cost, want_status):
        X = np.full((4, n), -7.25); cost = np.full((2, n), -7.25); status = np.full(n, -7, dtype=np.int32)
        hip.check(lib.sfm_tri_tracks(n, 14, m, hip.iptr(sc.pt_ptr), hip.iptr(sc.cam_idx), hip.dptr(sc.uv), hip.dptr(projs),
                                     hip.TRACKS_LINEAR | hip.TRACKS_NONLINEAR, 0.5, 5, group, None, hip.dptr(X),
                                     hip.dptr(cost) if want_cost else None, hip.iptr(status) if want_status else None))
        return X, cost, status

    T_all = tracks(True, True)
    assert np.all(T_all[0] != -7.25) and np.all(T_all[2] >= 0)
    for want_cost, want_status in ((False, False), (True, False), (False, True)):
        X, cost, status = tracks(want_cost, want_status)
        assert same_bits(X, T_all[0]), (want_cost, want_status)
        assert same_bits(cost, T_all[1]) if want_cost else np.all(cost == -7.25)
        assert same_bits(status, T_all[2]) if want_status else np.all(status == -7)


# ---- drop-in methods -----------------------------------------------------------------------------------------------------
def test_triangulate_tracks_robust_equals_native(hip, sfm):
    sc, _ref = rr.scene_and_reference("proto1")
    tp = sfm.processors.HipTriangulationProcessor(0.5, 9)
    got, inlier, status = tp.triangulate_tracks_robust([p for p in sc.projs], sc.pt_ptr, sc.cam_idx, sc.uv, rr.MAX_PX, rr.MIN_ANGLE_DEG,
                                                       cam_scale=sc.cam_scale)
    want = run(hip, sc)
    assert same_bits(got, want[0]) and np.array_equal(inlier, want[1].astype(bool)) and np.array_equal(status, want[4])
    assert inlier.dtype == bool
    with pytest.raises(ValueError, match="max_reproj"):
        tp.triangulate_tracks_robust([p for p in sc.projs], sc.pt_ptr, sc.cam_idx, sc.uv, -1.0)


@pytest.mark.parametrize("device_tracks", [False, True])
def test_retriangulate_structure_on_a_small_incremental_run(hip, sfm, device_tracks):
    from test_gpu_tri_tracks import _Loop
    sc = sfm.scenes.make_scene(5, 4 * _Loop.PER_VIEW, 1.0, seed=53, pixel_noise=0.3)
    loop = _Loop(sfm, sc, device_tracks)
    try:
        loop.register(0)
        for c in range(1, 5):
            loop.register(c)
            loop.bp._BaProcessor__execute_bundle_adjustment()
        bp, tp = loop.bp, loop.tp
        prob = bp._hip_scene.prob
        pt_ptr, cam_idx, uv = prob.structure()
        poses = loop.poses()
        views_before = [(v.rot.copy(), v.loc.copy()) for v in loop.vp.view_list]
        x0 = tp.tri_pts.copy()
        up = bp.ba_upload_bytes
        report = bp.retriangulate_structure(max_reproj_px=4.0, min_angle_deg=1.5)
        assert bp.ba_last_action == "reuse" and up <= bp.ba_upload_bytes <= up + 8 * 5      # at most the five scales go up
        scale = np.array([np.sqrt(abs(v.k[0, 0] * v.k[1, 1])) for v in loop.vp.view_list])
        X, inlier, n_in, best, status, summary = hip.tri_tracks_ransac(
            pt_ptr, cam_idx, uv, tr.camera_projections(sfm, poses), 16.0, np.cos(np.radians(1.5)), 128, 0.5, 3, scale, x0)
        assert rel(tp.tri_pts[0:3], X[0:3]) < 1e-9 and same_bits(tp.tri_pts[3], x0[3])
        assert np.array_equal(report.inlier, inlier) and np.array_equal(report.best_hyp, best)
        assert np.array_equal(report.status, status) and np.array_equal(report.summary, summary)
        assert summary[0] + summary[1] + summary[2] == x0.shape[1] and summary[0] > 0.9 * x0.shape[1]
        for v, (r, l) in zip(loop.vp.view_list, views_before):
            assert same_bits(v.rot, r) and same_bits(v.loc, l)
        # the next bundle adjustment finds everything in place
        bp._BaProcessor__execute_bundle_adjustment()
        assert bp.ba_last_action == "reuse"
        with pytest.raises(ValueError, match="max_hyp"):
            bp.retriangulate_structure(max_hyp=-1)
    finally:
        loop.close()
