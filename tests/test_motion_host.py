"""Host-side checks of the motion-only refinement (sfm_ba_refine_cameras): the NumPy reference of
tests/_motion_reference.py against the oracle's nonlinear PnP, what the reference achieves on the scenes the device tests
use, and the parts of the C ABI that need no device."""
import os
import re

import numpy as np

import _motion_reference as mr
import _robust_reference as rr
import _screen_reference as sr

from conftest import REPO


def _scene(sfm):
    sc = sfm.scenes.make_scene(6, 300, 0.7, seed=21)
    return sc, sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)


def test_reference_agrees_with_the_oracles_pnp(sfm, oracle):
    """One camera, its own observations, K = I on normalised keys, no row-overlap quirk: the motion-only step IS the
    reference's nonlinear PnP step.  Bound 1e-9 relative (the two differ in summation order and in solve against inverse;
    1e-13 to 3e-12 on this scene)."""
    sc, uvn = _scene(sfm)
    assert sc.cam_idx.shape[0] == 1249
    cams0 = sc.cams_init.copy()
    cams0[:, 3:7] /= np.linalg.norm(cams0[:, 3:7], axis=1)[:, None]
    assert np.all(cams0[:, 3] > 0)                               # canonical: q(R(q)) is q, the start PnP derives from R0
    for cam in range(sc.n_cams):
        sel = sc.cam_idx == cam
        n = int(sel.sum())
        pts = sc.pts_init[:, sc.pt_idx[sel]]
        got, _cost, status = mr.refine_cameras(cams0[cam:cam + 1], pts, np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32),
                                               uvn[:, sel], 1e-3, 5, quirks=oracle.Q2_LOC_JAC_SIGN)
        key = np.vstack((uvn[:, sel], np.ones((1, n))))
        rot, loc = oracle.nonlinear_pnp(key, np.vstack((pts, np.ones((1, n)))), np.eye(3), oracle.quat_to_rot(cams0[cam, 3:7]),
                                        cams0[cam, 0:3].reshape(3, 1), 1e-3, 5, quirks=oracle.Q2_LOC_JAC_SIGN)
        assert status[0] == 0
        assert np.max(np.abs(oracle.quat_to_rot(got[0, 3:7]) - rot)) / np.max(np.abs(rot)) < 1e-9
        assert np.max(np.abs(got[0, 0:3] - loc.ravel())) / np.max(np.abs(loc)) < 1e-9


def _rmse_px(oracle, sc, cams, pts, uvn, sel=None):
    scale = float(np.sqrt(abs(sc.intrinsic[0, 0] * sc.intrinsic[1, 1])))
    r = oracle.obs_terms_vec(cams, pts, sc.cam_idx, sc.pt_idx, uvn)[0]
    e = np.sum(r * r, axis=1)
    return scale * float(np.sqrt(np.mean(e if sel is None else e[sel]))), scale


def test_reference_does_its_job(sfm, oracle):
    sc, uvn = _scene(sfm)
    before, scale = _rmse_px(oracle, sc, sc.cams_init, sc.pts_true, uvn)
    cams, cost, status = mr.refine_cameras(sc.cams_init, sc.pts_true, sc.cam_idx, sc.pt_idx, uvn, 0.1, 8)
    after = _rmse_px(oracle, sc, cams, sc.pts_true, uvn)[0]
    assert abs(before - 9.88) < 0.01 and abs(after - 0.735) < 0.001 and not status.any()
    assert np.all(cost[1] < cost[0])
    assert np.allclose(cost[0], mr.per_camera_cost(sc.cams_init, sc.pts_true, sc.cam_idx, sc.pt_idx, uvn), rtol=1e-12)
    o = sr.outlier_scene(sfm)
    uvo = sfm.geometry.normalise_pixels(o.uv_pix, sc.intrinsic)
    want = {rr.LOSS_NONE: (5.39, None), rr.LOSS_HUBER: (0.752, 0.162), rr.LOSS_CAUCHY: (0.708, 0.095)}
    for kind, delta in ((rr.LOSS_NONE, 1.0), (rr.LOSS_HUBER, 5.0 / scale), (rr.LOSS_CAUCHY, 10.0 / scale)):
        cams, _cost, _status = mr.refine_cameras(sc.cams_init, sc.pts_true, sc.cam_idx, sc.pt_idx, uvo, 0.1, 20, kind, delta)
        clean = _rmse_px(oracle, sc, cams, sc.pts_true, uvo, ~o.displaced)[0]
        assert abs(clean - want[kind][0]) < 0.01, (kind, clean)
        if kind != rr.LOSS_NONE:
            r = oracle.obs_terms_vec(cams, sc.pts_true, sc.cam_idx, sc.pt_idx, uvo)[0]
            w = rr.loss_terms(kind, delta, r)[1]
            assert abs(w[o.displaced].max() - want[kind][1]) < 0.001 and w[o.displaced].max() <= 0.2


def test_reference_statuses(sfm, oracle):
    sc, uvn = _scene(sfm)
    mask = np.array([1, 0, 1, 1, 0, 1])
    cams, cost, status = mr.refine_cameras(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 0.1, 2, mask=mask)
    assert np.array_equal(status, np.where(mask == 0, mr.CAM_HELD, 0))
    assert np.array_equal(cams[mask == 0], sc.cams_init[mask == 0]) and np.array_equal(cost[0, mask == 0], cost[1, mask == 0])
    pts = sc.pts_init.copy()
    only0 = np.setdiff1d(sc.pt_idx[sc.cam_idx == 0], sc.pt_idx[sc.cam_idx != 0])
    if only0.size:
        pts[0, only0[0]] = np.nan
        cams, cost, status = mr.refine_cameras(sc.cams_init, pts, sc.cam_idx, sc.pt_idx, uvn, 0.1, 2)
        assert status[0] == mr.CAM_NONFINITE and not status[1:].any()
        assert np.array_equal(cams[0], sc.cams_init[0]) and np.isnan(cost[:, 0]).all()


def test_abi(sfm):
    native = sfm.native
    text = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    for name, value in (("SFM_CAM_EMPTY", 1), ("SFM_CAM_NONFINITE", 2), ("SFM_CAM_BEHIND", 4), ("SFM_CAM_HELD", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert (native.CAM_EMPTY, native.CAM_NONFINITE, native.CAM_BEHIND, native.CAM_HELD) == (1, 2, 4, 8)
    assert (mr.CAM_EMPTY, mr.CAM_NONFINITE, mr.CAM_BEHIND, mr.CAM_HELD) == (1, 2, 4, 8)
    for name in ("sfm_ba_refine_cameras", "sfm_ba_refine_cameras_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text) and name in native.EXPORTS
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = native.load()
    assert hasattr(lib, "sfm_ba_refine_cameras") and hasattr(lib, "sfm_ba_refine_cameras_plan")
    assert hasattr(native.BaProblem, "refine_cameras") and hasattr(sfm.processors.HipBaMixin, "refine_motion")


def test_plan(sfm):
    native = sfm.native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert native.load().sfm_ba_refine_cameras_plan(-1, None, None, None) == native.E_SHAPE
    assert native.refine_cameras_plan(0) == (0, native.refine_cameras_plan(1)[1], 0)
    prev = native.refine_cameras_plan(0)
    sizes = list(range(1, 4200)) + [10 ** 5, 10 ** 6 + 1, 2 ** 31 - 1]
    classes = set()
    for n in sizes:
        n_slices, slice_obs, size_class = native.refine_cameras_plan(n)
        assert slice_obs == prev[1] and slice_obs > 0
        assert n_slices * slice_obs >= n > (n_slices - 1) * slice_obs
        assert n_slices >= prev[0] and size_class >= prev[2] and size_class >= 1          # monotone in n_obs
        classes.add(size_class)
        prev = (n_slices, slice_obs, size_class)
    assert len(classes) >= 2
