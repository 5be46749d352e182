"""GPU tests of the robust resection of cameras: sfm_resect_ransac, its _dev form, sfm_ba_resect and the drop-in methods,
against the float64 NumPy reference of tests/_resect_reference.py.

Decisions (best_hyp, masks, counts, status, summary) are compared EXACTLY: tests/test_resect_host.py asserts that every
camera of every scene used here is settled in the reference, so nothing is left out.  Cameras are compared per camera at
max(1e-9, 100 d_c) in absolute terms, d_c being the reference's own spread of the final camera over the three orders in which
a triple can be handed to the solver: the bound comes from the reference alone."""
from types import SimpleNamespace

import numpy as np
import pytest

import _motion_reference as mr
import _resect_reference as rf

pytestmark = pytest.mark.gpu

IDENTITY = np.array([0.0, 0, 0, 1, 0, 0, 0])
_WORST = {"d_c": 0.0, "device": 0.0}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def free(hip, sc, cm, max_hyp=128, iters=3, cams_init=None, lam=0.5):
    return hip.resect_ransac(cm.view_ptr, cm.uv, cm.X, rf.MAX_ERR2, max_hyp, lam, iters, cam_scale=sc.cam_scale, cams_init=cams_init)


def start_cameras(sc, seed=7, shift=0.1, deg=3.0):
    """The true cameras displaced by `shift` units and a rotation of `deg` degrees about a random axis."""
    rng = np.random.default_rng(seed)
    cams = rf.cams_of(sc)
    cams[:, 0:3] += shift * rng.standard_normal((sc.n_views, 3)) / np.sqrt(3.0)
    axis = rng.standard_normal((sc.n_views, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    half = np.radians(deg) / 2.0
    dq = np.concatenate((np.full((sc.n_views, 1), np.cos(half)), np.sin(half) * axis), axis=1)
    w, x, y, z = cams[:, 3], cams[:, 4], cams[:, 5], cams[:, 6]
    a, b, c, d = dq.T
    cams[:, 3:7] = np.stack((w * a - x * b - y * c - z * d, w * b + x * a + y * d - z * c,
                             w * c - x * d + y * a + z * b, w * d + x * c - y * b + z * a), axis=1)
    return cams


def check_against(ref, cams, inlier, n_in, best, status, summary, cams_init, where=""):
    """Exact decisions, cameras at the per-camera bound, unsolved cameras bit for bit."""
    assert ref.settled.all()
    assert np.array_equal(best, ref.best_hyp), where
    assert np.array_equal(status, ref.status), where
    assert np.array_equal(n_in, ref.n_inliers), where
    assert np.array_equal(inlier, ref.inlier), where
    assert np.array_equal(summary, ref.summary), where
    solved = ref.best_hyp >= 0
    for c in np.flatnonzero(solved):
        diff = float(np.max(np.abs(cams[c] - ref.cams[c])))
        _WORST["d_c"] = max(_WORST["d_c"], ref.d_c[c]); _WORST["device"] = max(_WORST["device"], diff)
        print(where, "camera", c, "d_c %.3e device %.3e" % (ref.d_c[c], diff))
        assert diff <= max(1e-9, 100.0 * ref.d_c[c]), (where, c, diff, ref.d_c[c])
    want = np.tile(IDENTITY, (cams.shape[0], 1)) if cams_init is None else cams_init
    assert same_bits(cams[~solved], want[~solved]), where


def resident(hip, sc, cams0, pts=None):
    prob = hip.BaProblem(sc.n_views, sc.pt_ptr, sc.cam_idx, sc.uv)
    prob.set_state(cams0, sc.pts_true if pts is None else pts)
    return prob


# ---- parity with the reference: prototype scenes, the paths scene, no model, collinear ------------------------------
@pytest.mark.parametrize("name,max_hyp", rf.CASES)
def test_parity_with_the_reference(hip, name, max_hyp):
    sc, cm, ref = rf.scene_and_reference(name, max_hyp)
    cams0 = start_cameras(sc)
    got = free(hip, sc, cm, max_hyp, cams_init=cams0)
    check_against(ref, *got, cams0, where="%s/%d" % (name, max_hyp))
    if name == "proto0":                                     # without cams_init an unsolved camera is the identity; none here
        assert same_bits(free(hip, sc, cm, max_hyp)[0], got[0])
    print("worst d_c %.3e, worst device difference %.3e so far" % (_WORST["d_c"], _WORST["device"]))


def test_cameras_without_a_model_come_back_bit_for_bit(hip):
    sc, cm, ref = rf.scene_and_reference("special")
    cams0 = start_cameras(sc, seed=9)
    cams, inlier, n_in, best, status, summary = free(hip, sc, cm, cams_init=cams0)
    for c in (1, 2):                                         # every key displaced; every point on one line
        assert status[c] & hip.RESECT_NO_MODEL and best[c] == -1 and n_in[c] == 0
        assert same_bits(cams[c], cams0[c]) and not inlier[cm.view_ptr[c]:cm.view_ptr[c + 1]].any()
    assert summary[1] == 2 and summary[0] == 2
    cams = free(hip, sc, cm)[0]
    assert same_bits(cams[1], IDENTITY) and same_bits(cams[2], IDENTITY)
    few = rf.scene("paths")[1].counts < 4
    sc, cm, ref = rf.scene_and_reference("paths", 128)
    cams0 = start_cameras(sc, seed=10)
    cams, inlier, n_in, best, status, summary = free(hip, sc, cm, cams_init=cams0)
    assert np.all(status[few] == hip.RESECT_TOO_FEW) and same_bits(cams[few], cams0[few]) and summary[2] == few.sum()


# ---- the two forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_hyp", [("proto0", 128), ("special", 128), ("paths", 32), ("paths", 1000)])
def test_resident_form_against_the_reference_and_the_free_form(hip, name, max_hyp):
    sc, cm, ref = rf.scene_and_reference(name, max_hyp)
    cams0 = start_cameras(sc)
    with resident(hip, sc, cams0) as prob:
        before = prob.upload_bytes
        out = prob.resect(rf.MAX_ERR2, max_hyp, 0.5, 3, cam_scale=sc.cam_scale)
        assert prob.upload_bytes == before + 8 * sc.n_views                       # the scales, nothing else
        assert prob.get_stats().shape[0] == 0                                     # the cost history restarts
        cams, pts = prob.get_state()
        assert same_bits(pts, sc.pts_true)
    inlier = out.inlier[cm.order]                                                 # scene order -> camera-major
    check_against(ref, cams, inlier, out.n_inliers, out.best_hyp, out.status, out.summary, cams0, where="resident %s" % name)
    got = free(hip, sc, cm, max_hyp, cams_init=cams0)
    for a, b in zip((inlier, out.n_inliers, out.best_hyp, out.status, out.summary), got[1:]):
        assert np.array_equal(a, b)
    for c in range(sc.n_views):
        assert float(np.max(np.abs(cams[c] - got[0][c]))) <= max(1e-9, 100.0 * ref.d_c[c])


def subset(cm, views):
    views = np.asarray(views, dtype=np.int64)
    ent = np.concatenate([np.arange(cm.view_ptr[c], cm.view_ptr[c + 1]) for c in views] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    ptr = np.zeros(views.shape[0] + 1, dtype=np.int32)
    np.cumsum(cm.counts[views], out=ptr[1:])
    return SimpleNamespace(view_ptr=ptr, uv=np.ascontiguousarray(cm.uv[:, ent]), X=np.ascontiguousarray(cm.X[:, ent]),
                           counts=cm.counts[views], ent=ent)


@pytest.mark.parametrize("max_hyp", [32, 1000])
def test_a_camera_does_not_depend_on_the_rest_of_the_batch(hip, max_hyp):
    sc, cm = rf.scene("paths")
    cams0 = start_cameras(sc)
    whole = free(hip, sc, cm, max_hyp, cams_init=cams0)

    def check(views):
        sub = subset(cm, views)
        part = SimpleNamespace(cam_scale=sc.cam_scale[views])
        got = free(hip, part, sub, max_hyp, cams_init=cams0[views])
        assert same_bits(got[0], whole[0][views]) and same_bits(got[1], whole[1][sub.ent]), views
        for k in (2, 3, 4):
            assert np.array_equal(got[k], whole[k][views]), views

    check(np.random.default_rng(3).permutation(sc.n_views))
    check(np.flatnonzero(cm.counts <= 1024))                                      # without the long cameras
    for n in (4, 65, 257, 1025, 5000):                                            # alone
        check(np.flatnonzero(cm.counts == n))


# ---- the resident scene ----------------------------------------------------------------------------------------------
def test_held_cameras_are_untouched_and_still_judged(hip):
    sc, cm, ref = rf.scene_and_reference("proto0")
    cams0 = rf.cams_of(sc)                                                        # held at the true cameras: their inliers are the clean keys
    cams0[[0, 2, 4]] = start_cameras(sc)[[0, 2, 4]]
    mask = np.array([1, 0, 1, 0, 1, 0], dtype=np.uint8)
    want = rf.solve_views(cm.view_ptr, cm.uv, cm.X, sc.cam_scale, cams0, held=mask == 0)
    with resident(hip, sc, cams0) as prob:
        out = prob.resect(rf.MAX_ERR2, 128, 0.5, 3, mask=mask, cam_scale=sc.cam_scale)
        cams, _pts = prob.get_state()
    held = mask == 0
    assert same_bits(cams[held], cams0[held]) and np.all(out.status[held] == hip.RESECT_HELD) and np.all(out.best_hyp[held] == -1)
    assert np.array_equal(out.inlier[cm.order], want.inlier) and np.array_equal(out.n_inliers, want.n_inliers)
    assert np.array_equal(out.status, want.status) and np.array_equal(out.summary, want.summary)
    assert np.array_equal(out.best_hyp[~held], ref.best_hyp[~held])
    for c in np.flatnonzero(~held):
        assert float(np.max(np.abs(cams[c] - ref.cams[c]))) <= max(1e-9, 100.0 * ref.d_c[c])
    held_obs = held[sc.cam_idx]
    assert np.array_equal(out.inlier[held_obs] == 0, sc.displaced[held_obs])


@pytest.mark.parametrize("name", ["proto0_30", "special", "paths"])
def test_resect_then_screen_shows_the_same_flags(hip, name):
    sc, cm = rf.scene(name)
    with resident(hip, sc, start_cameras(sc)) as prob:
        out = prob.resect(rf.MAX_ERR2, 128, 0.5, 3, cam_scale=sc.cam_scale)
        report = prob.screen(rf.MAX_ERR2, 1.0, 0, sc.cam_scale)
    solved = (out.status & (hip.RESECT_TOO_FEW | hip.RESECT_NO_MODEL | hip.RESECT_HELD)) == 0
    of_solved = solved[sc.cam_idx]
    bad = (report.obs_flags & (hip.OBS_HIGH_ERROR | hip.OBS_BEHIND | hip.OBS_NONFINITE)) != 0
    assert solved.any() and np.array_equal(bad[of_solved], out.inlier[of_solved] == 0)
    assert not out.inlier[~of_solved].any()


def test_resect_then_cull_removes_what_was_flagged(hip):
    sc, cm, ref = rf.scene_and_reference("proto0")
    with resident(hip, sc, start_cameras(sc)) as prob:
        out = prob.resect(rf.MAX_ERR2, 128, 0.5, 3, cam_scale=sc.cam_scale)
        assert np.all(out.best_hyp >= 0) and out.summary[5] > 0                   # every camera solved: the cull sees only their flags
        report = prob.cull(rf.MAX_ERR2, 1.0, 0, sc.cam_scale)
        pt_ptr, cam_idx, uv = prob.structure()
    keep = out.inlier != 0
    assert np.array_equal(report.obs_flags == 0, keep) and (~keep).sum() == out.summary[5]
    assert np.array_equal(cam_idx, sc.cam_idx[keep]) and same_bits(uv, np.ascontiguousarray(sc.uv[:, keep]))
    assert np.array_equal(np.diff(pt_ptr), np.bincount(sc.pt_idx[keep], minlength=sc.n_pts))


@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("graph", [0, 1])
def test_resect_leaves_no_stale_state_behind(hip, graph, pending):
    """iterate, resect, iterate under SFM_OPT_DETERMINISTIC ends in the bits of a fresh problem started from the state
    resect left; with iters = 0 and every camera held that is the state of iterate, iterate.  ``pending``: the first
    phase is spelled linearize_reduce / solve_update, so its last back substitution is still owed when resect is called."""
    sc, cm = rf.scene("proto0")
    cams0 = start_cameras(sc, shift=0.02, deg=0.5)
    pts0 = sc.pts_true + 0.02 * np.random.default_rng(21).standard_normal(sc.pts_true.shape)

    def fresh():
        p = hip.BaProblem(sc.n_views, sc.pt_ptr, sc.cam_idx, sc.uv)
        p.set_option(hip.OPT_DETERMINISTIC, 1)
        p.set_option(hip.OPT_GRAPH, graph)
        return p

    def first_phase(prob):
        prob.set_state(cams0, pts0)
        if pending:
            for _ in range(2):
                prob.linearize_reduce(5.0)
                prob.solve_update(5.0)
        else:
            prob.iterate(5.0, 2)

    with fresh() as prob, fresh() as other:
        first_phase(prob)
        out = prob.resect(rf.MAX_ERR2, 128, 0.5, 3, cam_scale=sc.cam_scale)
        assert out.summary[0] == sc.n_views
        cams_mid, pts_mid = prob.get_state()
        prob.iterate(5.0, 2)
        assert prob.get_stats().shape[0] == 2
        other.set_state(cams_mid, pts_mid)
        other.iterate(5.0, 2)
        assert all(same_bits(a, b) for a, b in zip(prob.get_state(), other.get_state()))
        assert same_bits(prob.get_stats(), other.get_stats())
    with fresh() as prob, fresh() as other:
        first_phase(prob)
        held = prob.resect(rf.MAX_ERR2, 128, 0.5, 0, mask=np.zeros(sc.n_views, dtype=np.uint8), cam_scale=sc.cam_scale)
        assert np.all(held.status == hip.RESECT_HELD) and held.summary[0:4].tolist() == [0, 0, 0, 0]
        prob.iterate(5.0, 2)
        first_phase(other)
        if pending:
            other.get_state()                                # the owed back substitution in its own launch, as resect completes it
        other.iterate(5.0, 2)
        assert all(same_bits(a, b) for a, b in zip(prob.get_state(), other.get_state()))


def test_refused_with_a_communicator_and_on_bad_arguments(hip):
    sc, cm = rf.scene("special")
    cams0 = start_cameras(sc)
    lib = hip.load()
    with resident(hip, sc, cams0) as prob:
        comm = hip.Comm(1, 0, hip.comm_unique_id())
        try:
            prob.set_comm(comm)
            with pytest.raises(ValueError, match="communicator"):
                prob.resect(rf.MAX_ERR2)
            prob.set_comm(None)
        finally:
            comm.close()
        for args, word in (((float("nan"), 128, 0.5, 3), "max_err2"), ((-1.0, 128, 0.5, 3), "max_err2"), ((16.0, -1, 0.5, 3), "max_hyp"),
                           ((16.0, 65537, 0.5, 3), "max_hyp"), ((16.0, 128, -1.0, 3), "lambda"), ((16.0, 128, float("nan"), 3), "lambda"),
                           ((16.0, 128, 0.5, -1), "iters")):
            st = lib.sfm_ba_resect(prob._h, args[0], args[1], args[2], args[3], 0, None, None, None, None, None, None, None)
            assert st == hip.E_SHAPE and word in hip.last_error(), args
        assert same_bits(prob.get_state()[0], cams0)
        assert prob.resect(rf.MAX_ERR2, want_outputs=False) is None

    def call(view_ptr, max_err2=16.0):
        cams = np.full((sc.n_views, 7), -7.25)
        st = lib.sfm_resect_ransac(sc.n_views, hip.iptr(np.asarray(view_ptr, dtype=np.int32)), cm.uv.shape[1], hip.dptr(cm.uv),
                                   hip.dptr(cm.X), None, max_err2, 128, 0.5, 3, 0, None, hip.dptr(cams), None, None, None, None, None)
        assert np.all(cams == -7.25)
        return st, hip.last_error()

    ptr = cm.view_ptr.copy()
    for bad in (ptr + 1, np.concatenate((ptr[:-1], [ptr[-1] - 1])), np.array([0, ptr[2], ptr[1], ptr[3], ptr[4]])):
        st, msg = call(bad)
        assert st == hip.E_SHAPE and "view_ptr" in msg
    assert call(ptr, float("nan"))[0] == hip.E_SHAPE
    # a view of more than 2^20 observations: T would not fit 63 bits
    big = (1 << 20) + 1
    cams = np.full((2, 7), -7.25)
    st = lib.sfm_resect_ransac(2, hip.iptr(np.array([0, 5, 5 + big], dtype=np.int32)), 5 + big, hip.dptr(np.zeros((2, 5 + big))),
                               hip.dptr(np.zeros((3, 5 + big))), None, 16.0, 128, 0.5, 3, 0, None, hip.dptr(cams), None, None, None, None, None)
    assert st == hip.E_SHAPE and "camera 1" in hip.last_error() and np.all(cams == -7.25)
    # no view at all; a scene without observations
    cams, inlier, n_in, best, status, summary = hip.resect_ransac([0], np.zeros((2, 0)), np.zeros((3, 0)), 16.0)
    assert cams.shape == (0, 7) and not summary.any()
    cams, inlier, n_in, best, status, summary = hip.resect_ransac([0, 0, 0], np.zeros((2, 0)), np.zeros((3, 0)), 16.0)
    assert same_bits(cams, np.tile(IDENTITY, (2, 1))) and np.all(status == hip.RESECT_TOO_FEW) and summary.tolist() == [0, 0, 2, 0, 0, 0]
    with hip.BaProblem(2, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((2, 0))) as prob:
        out = prob.resect(16.0, mask=[1, 0])
        assert out.status.tolist() == [hip.RESECT_TOO_FEW, hip.RESECT_HELD] and out.summary.tolist() == [0, 0, 1, 0, 0, 0]


# ---- the device form and the optional outputs --------------------------------------------------------------------------
def test_dev_form_in_place_on_a_callers_stream(hip):
    import torch
    sc, cm = rf.scene("paths")
    cams0 = start_cameras(sc)
    want = free(hip, sc, cm, 128, cams_init=cams0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    m = cm.uv.shape[1]
    with torch.cuda.stream(stream):
        d_uv = torch.from_numpy(cm.uv).to(dev); d_x = torch.from_numpy(cm.X).to(dev)
        d_scale = torch.from_numpy(sc.cam_scale).to(dev); d_cams = torch.from_numpy(cams0).to(dev)
        d_in = torch.zeros(m, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(sc.n_views, dtype=torch.int32, device=dev); d_best = torch.zeros_like(d_n); d_st = torch.zeros_like(d_n)
        d_sum = torch.zeros(6, dtype=torch.int64, device=dev)
        stream.synchronize()
        hip.resect_ransac_dev(cm.view_ptr, m, d_uv.data_ptr(), d_x.data_ptr(), rf.MAX_ERR2, 128, 0.5, 3, hip.QUIRKS_REFERENCE,
                              d_scale.data_ptr(), d_cams.data_ptr(), d_cams.data_ptr(), d_in.data_ptr(), d_n.data_ptr(),
                              d_best.data_ptr(), d_st.data_ptr(), d_sum.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    got = (d_cams.cpu().numpy(), d_in.cpu().numpy(), d_n.cpu().numpy(), d_best.cpu().numpy(), d_st.cpu().numpy(), d_sum.cpu().numpy())
    for a, b in zip(got, want):
        assert same_bits(a, b)
    # without the optional arrays
    d_out = torch.zeros_like(d_cams)
    hip.resect_ransac_dev(cm.view_ptr, m, d_uv.data_ptr(), d_x.data_ptr(), rf.MAX_ERR2, 128, 0.5, 3, d_cam_scale=d_scale.data_ptr(),
                          d_cams_out=d_out.data_ptr())
    torch.cuda.synchronize()
    assert same_bits(d_out.cpu().numpy(), free(hip, sc, cm, 128)[0])


def test_any_subset_of_the_outputs_gives_the_same_bytes(hip):
    """Through the raw C calls: what a call computes does not depend on which optional outputs it was asked for."""
    sc, cm = rf.scene("special")
    lib = hip.load()
    v, m = sc.n_views, cm.uv.shape[1]
    cams0 = start_cameras(sc)
    names = ("inlier", "n_inliers", "best_hyp", "status", "summary")

    def run(wanted):
        o = hip._ransac_outputs(v, m)
        cams = np.full((v, 7), -7.25)
        ptrs = [p if k in wanted else None for k, p in zip(names, hip._ransac_pointers(o))]
        hip.check(lib.sfm_resect_ransac(v, hip.iptr(cm.view_ptr), m, hip.dptr(cm.uv), hip.dptr(cm.X), hip.dptr(sc.cam_scale), rf.MAX_ERR2,
                                        128, 0.5, 3, hip.QUIRKS_REFERENCE, hip.dptr(cams0), hip.dptr(cams), *ptrs))
        return cams, o

    def run_resident(wanted):
        o = hip._ransac_outputs(v, m)
        with resident(hip, sc, cams0) as prob:
            ptrs = [p if k in wanted else None for k, p in zip(names, hip._ransac_pointers(o))]
            hip.check(lib.sfm_ba_resect(prob._h, rf.MAX_ERR2, 128, 0.5, 3, hip.QUIRKS_REFERENCE, None, hip.dptr(sc.cam_scale), *ptrs))
            return prob.get_state()[0], o

    for call in (run, run_resident):
        cams_all, o_all = call(names)
        assert o_all.summary[0] == 2 and o_all.inlier.any()
        for wanted in [()] + [(k,) for k in names]:
            cams, o = call(wanted)
            assert same_bits(cams, cams_all), wanted
            for k in names:
                got = getattr(o, k)
                assert same_bits(got, getattr(o_all, k)) if k in wanted else not got.any(), (wanted, k)


# ---- drop-in methods -------------------------------------------------------------------------------------------------
def test_estimate_cam_pose_robust_equals_native(hip, sfm):
    sc, cm, ref = rf.scene_and_reference("proto0")
    K = np.array([[rf.rr.FOCAL, 0.0, 0.0], [0.0, rf.rr.FOCAL, 0.0], [0.0, 0.0, 1.0]])
    cp = sfm.processors.HipCamposeProcessor.__new__(sfm.processors.HipCamposeProcessor)
    cp.damping_factor, cp.iteration = 0.5, 3
    for c in (0, 3):
        lo, hi = cm.view_ptr[c], cm.view_ptr[c + 1]
        pix = np.vstack((rf.rr.FOCAL * cm.uv[:, lo:hi], np.ones((1, hi - lo))))
        pts_h = np.vstack((cm.X[:, lo:hi], np.ones((1, hi - lo))))
        idx, rot, loc = cp.estimate_cam_pose_robust(pix, pts_h, K, rf.MAX_PX, 128)
        uv = sfm.geometry.normalise_pixels(pix, K)
        cams, inlier, _n, best, status, _s = hip.resect_ransac([0, hi - lo], uv, cm.X[:, lo:hi], rf.MAX_ERR2, 128, 0.5, 3,
                                                               cam_scale=np.array([rf.rr.FOCAL]))
        assert isinstance(idx, list) and idx == np.flatnonzero(inlier).tolist() and loc.shape == (3, 1)
        assert same_bits(loc.ravel(), cams[0, 0:3]) and same_bits(rot, sfm.geometry.quaternion_to_rotation_unchecked(cams[0, 3:7]))
        assert cp.resect_last["hypothesis"] == best[0] == ref.best_hyp[c] and np.array_equal(inlier, ref.inlier[lo:hi])
    with pytest.raises(ValueError, match="max_reproj_px"):
        cp.estimate_cam_pose_robust(pix, pts_h, K, -1.0)


@pytest.mark.parametrize("device_tracks", [False, True])
def test_resect_motion_on_a_small_incremental_run(hip, sfm, device_tracks):
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
        x0 = tp.tri_pts.copy()
        report = bp.resect_motion(max_reproj_px=4.0, views=[1, 2, 4])
        assert bp.ba_last_action == "reuse"
        scale = np.array([np.sqrt(abs(v.k[0, 0] * v.k[1, 1])) for v in loop.vp.view_list])
        order = np.argsort(cam_idx, kind="stable")
        pt_idx = np.repeat(np.arange(pt_ptr.shape[0] - 1), np.diff(pt_ptr))
        view_ptr = np.concatenate(([0], np.cumsum(np.bincount(cam_idx, minlength=5))))
        held = np.array([True, False, False, True, False])
        cams, inlier, n_in, best, status, summary = hip.resect_ransac(
            view_ptr, np.ascontiguousarray(uv[:, order]), np.ascontiguousarray(x0[0:3, pt_idx[order]] / x0[3, pt_idx[order]]),
            16.0, 128, bp.damping_factor, 3, bp.ba_quirk_flags, scale, poses)
        now = loop.poses()
        assert np.max(np.abs(now[~held] - cams[~held])) < 1e-9 and np.max(np.abs(now[held] - poses[held])) < 1e-12
        assert np.array_equal(report.best_hyp[~held], best[~held]) and np.all(report.status[held] == hip.RESECT_HELD)
        assert np.array_equal(report.inlier[order][~held[cam_idx[order]]], inlier[~held[cam_idx[order]]])
        assert report.summary[0] == 3 and same_bits(tp.tri_pts, x0)
        bp._BaProcessor__execute_bundle_adjustment()
        assert bp.ba_last_action == "reuse"
        with pytest.raises(ValueError, match="max_hyp"):
            bp.resect_motion(max_hyp=-1)
        with pytest.raises(ValueError, match="view index"):
            bp.resect_motion(views=[5])
    finally:
        loop.close()


# ---- what it achieves --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["proto0", "proto0_30"])
def test_contaminated_cameras_end_nearer_the_clean_pose_than_least_squares(hip, name, capsys):
    """From the true points and cameras displaced by 3 degrees / 0.1 units: resect against refine_cameras for the same
    iterations, each measured by its distance from the pose refined on the clean observations only (the NumPy reference of
    refine_cameras, from the true camera).  The assertion is the ordering, on every contaminated camera."""
    sc, cm = rf.scene(name)
    cams0 = start_cameras(sc)
    clean = ~sc.displaced
    want = mr.refine_cameras(rf.cams_of(sc), sc.pts_true, sc.cam_idx[clean], sc.pt_idx[clean], sc.uv[:, clean], 0.5, 10)[0]
    with resident(hip, sc, cams0) as prob:
        out = prob.resect(rf.MAX_ERR2, 128, 0.5, 3, cam_scale=sc.cam_scale)
        robust = prob.get_state()[0]
    with resident(hip, sc, cams0) as prob:
        prob.refine_cameras(0.5, 3)
        plain = prob.get_state()[0]
    d_robust = np.max(np.abs(robust - want), axis=1)
    d_plain = np.max(np.abs(plain - want), axis=1)
    with capsys.disabled():
        print("\n%s: distance from the clean-only pose, robust %s, least squares %s"
              % (name, np.array2string(d_robust, precision=2), np.array2string(d_plain, precision=2)))
    contaminated = np.bincount(sc.cam_idx[sc.displaced], minlength=sc.n_views) > 0
    assert contaminated.all() and np.all(out.best_hyp >= 0)
    assert np.all(d_robust[contaminated] < d_plain[contaminated])
