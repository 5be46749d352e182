"""HipBaProcessor.process from pixels: the three upenn frames through the product's state machine, with the device
tracker and with the host tracker, against the test helper that has stood in for it so far
(_sift_chain.process_three_on_device, untouched).  Integers must be identical; poses and points before BA are held to
bit identity if the helper's own two runs are bit-identical, otherwise to 10x the spread between them; after BA the
helper's own condition holds (the resident BA is not bit-reproducible without SFM_OPT_DETERMINISTIC)."""
import os
import random
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sift_chain as C  # noqa: E402

pytestmark = pytest.mark.gpu


def frames():
    return [C.fixture(n)["image"] for n in (1, 2, 3)]


def recording_classes(P, log):
    """Subclasses of the product's processors that write down what passes through them."""

    class Ba(P.HipBaProcessor):
        def _BaProcessor__execute_bundle_adjustment(self):
            views = self.view_processor.view_list
            log["rots_before_ba"] = [np.array(v.rot, copy=True) for v in views]
            log["locs_before_ba"] = [np.array(v.loc, copy=True) for v in views]
            log["pts_before_ba"] = np.array(self.tri_processor.tri_pts, copy=True)
            log["rmse_before_ba"] = C.reprojection_rmse(views, self.key_tracker.track_list, self.tri_processor.tri_pts)
            P.HipBaProcessor.execute_bundle_adjustment(self)
            log["rmse_after_ba"] = C.reprojection_rmse(views, self.key_tracker.track_list, self.tri_processor.tri_pts)

    class Epi(P.HipEpipolarProcessor):
        def determine_fundamental_mat(self, matched_pairs, ransac_config=None):
            inl = P.HipEpipolarProcessor.determine_fundamental_mat(self, matched_pairs, ransac_config)
            log["fund_inliers"] = len(inl)
            log["pairs01"] = [np.array(p, copy=True) for p in matched_pairs]
            return inl

    class Cam(P.HipCamposeProcessor):
        def estimate_cam_pose_pnp(self, key_2d_pts, tri_3d_pts, intrinsic_mat, ransac_config=None, damping_factor=None,
                                  iteration=None):
            out = P.HipCamposeProcessor.estimate_cam_pose_pnp(self, key_2d_pts, tri_3d_pts, intrinsic_mat, ransac_config,
                                                              damping_factor, iteration)
            log["pnp_points"], log["pnp_inlier_list"] = key_2d_pts.shape[1], list(out[0])
            log["pnp_rot"], log["pnp_loc"] = out[1], out[2]
            return out

    return Ba, Epi, Cam


def run_helper(sfm, imgs, k):
    """The baseline helper as it is, with a BA processor that also writes down the state it starts from and a cam pose
    processor that writes down the PnP inlier list (the helper itself keeps only its length)."""
    log = {}
    Ba, _Epi, Cam = recording_classes(sfm.processors, log)
    shim = types.SimpleNamespace(**{n: getattr(sfm.processors, n) for n in dir(sfm.processors) if not n.startswith("__")})
    shim.HipBaProcessor = Ba
    shim.HipCamposeProcessor = Cam

    class Tracker(sfm.processors.HipKeyTracker):          # the helper keeps its tracker to itself: remember it
        def __init__(self, *args):
            sfm.processors.HipKeyTracker.__init__(self, *args)
            log["tracker"] = self
    shim.HipKeyTracker = Tracker
    random.seed(99)
    out = C.process_three_on_device(types.SimpleNamespace(processors=shim), imgs, k)
    out.update({key: log[key] for key in ("rots_before_ba", "locs_before_ba", "pts_before_ba", "pnp_inlier_list")})
    assert len(out["pnp_inlier_list"]) == out["pnp_inliers"] and log["pnp_points"] == out["pnp_points"]
    out["tables"] = [t.table for t in log["tracker"].track_list]
    assert out["rmse_before_ba"] == log["rmse_before_ba"]
    return out


def run_process(sfm, imgs, k, device_tracker, capsys):
    P = sfm.processors
    log = {}
    Ba, Epi, Cam = recording_classes(P, log)
    random.seed(99)
    # the helper's configurations, built in its order (each RansacConfig seeds Python's RNG with -1)
    cfg_kt = P.RansacConfig(1e-2, 0.99, 0.75, 8, 200)
    cfg_ep = P.RansacConfig(1e-2, 0.99, 0.75, 8, 300)
    cfg_cp = P.RansacConfig(8.0, 0.99, 0.75, 8, 300)
    vp = P.HipViewProcessor('sift')
    kt = (P.HipDeviceKeyTracker if device_tracker else P.HipKeyTracker)('sift', False, True, False, cfg_kt)
    bp = Ba(vp, kt, Epi(cfg_ep), P.HipTriangulationProcessor(), Cam(cfg_cp, 5, 300))
    bp.ba_verbose = False
    capsys.readouterr()
    try:
        for img in imgs:
            assert bp.process(img, k) is None
        log["prints"] = capsys.readouterr().out.splitlines()
        log["curr_data_idx"] = bp.curr_data_idx
        log["tables"] = [np.array(t.table, copy=True) for t in kt.track_list]
        log["views"] = vp.view_list
        log["n_points"] = bp.tri_processor.tri_pts.shape[1]
        log["tracker"] = type(kt).__name__
    finally:
        bp.ba_release()
        kt.kt_release()
    return log


def max_diff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))) if np.size(a) else 0.0


def test_process_three_frames_equals_the_helper(sfm, hip, capsys):
    imgs, k = frames(), C.halved_k()
    base = run_helper(sfm, imgs, k)
    base2 = run_helper(sfm, imgs, k)
    # spread of the baseline between its own two runs, per quantity
    pre = ("rots_before_ba", "locs_before_ba", "pts_before_ba", "pnp_rot", "pnp_loc")
    assert base["pts_before_ba"].shape == base2["pts_before_ba"].shape
    spread = {key: max_diff(np.array(base[key]), np.array(base2[key])) for key in pre}
    post_spread = {"ba_rot": max_diff(base["ba_rot"], base2["ba_rot"]), "ba_loc": max_diff(base["ba_loc"], base2["ba_loc"])}
    with capsys.disabled():
        print("\nbaseline spread between two runs, before BA: %s; after BA: %s" % (spread, post_spread))

    runs = [run_process(sfm, imgs, k, True, capsys), run_process(sfm, imgs, k, False, capsys)]
    for got in runs:
        who = got["tracker"]
        assert got["prints"] == ["In one image state", "In epipolar state", "In cam pose state"], who
        assert got["curr_data_idx"] == 3
        for v, view in enumerate(got["views"]):
            assert view.is_valid is True and view.ref_idx == 0 and view.idx == v, (who, v)
        # integers: identical
        base_tables = base["tables"]
        assert len(got["tables"]) == 3
        for v in range(3):
            assert got["tables"][v].dtype == base_tables[v].dtype
            np.testing.assert_array_equal(got["tables"][v], base_tables[v], err_msg="%s table %d" % (who, v))
        assert got["fund_inliers"] == base["fund_inliers"], who
        assert got["pnp_points"] == base["pnp_points"] and got["pnp_inlier_list"] == base["pnp_inlier_list"], who
        assert got["n_points"] == base["n_points"], who
        for a, b in zip(got["pairs01"], base["pairs01"]):
            np.testing.assert_array_equal(a, b)
        # poses and points before BA
        for key in pre:
            d = max_diff(np.array(got[key]), np.array(base[key]))
            with capsys.disabled():
                print("%s %s: |process - helper| = %.3e (baseline spread %.3e)" % (who, key, d, spread[key]))
            if spread[key] == 0.0:
                assert d == 0.0, (who, key, d)
            else:
                assert d <= 10.0 * spread[key], (who, key, d, spread[key])
        # after BA: the helper's own condition
        assert np.isfinite(got["rmse_after_ba"]) and got["rmse_after_ba"] <= 1.01 * got["rmse_before_ba"], who
        with capsys.disabled():
            print("%s rmse %.4f -> %.4f px (helper %.4f -> %.4f)" % (who, got["rmse_before_ba"], got["rmse_after_ba"],
                                                                     base["rmse_before_ba"], base["rmse_after_ba"]))
    assert base["pnp_inlier_list"] == base2["pnp_inlier_list"]
    for v in range(3):
        np.testing.assert_array_equal(runs[0]["tables"][v], runs[1]["tables"][v])


def test_process_stops_when_full_and_keeps_its_state(sfm, hip, capsys):
    P = sfm.processors
    imgs, k = frames()[:1], C.halved_k()
    vp = P.HipViewProcessor('sift')
    kt = P.HipDeviceKeyTracker('sift', False, True, False, None)
    bp = P.HipBaProcessor(vp, kt, None, None, None, filter_size=1)
    try:
        bp.process(imgs[0], k)
        assert bp.curr_data_idx == 1 and vp.view_list[0].is_valid is True
        assert vp.view_list[0].key_xy.shape == (len(vp.view_list[0].key_pts), 2)
        up = kt.kt_upload_bytes
        capsys.readouterr()
        assert bp.process(imgs[0], k) is None
        assert capsys.readouterr().out == "Bundle Adjustment processor is full\n"
        assert bp.curr_data_idx == 1 and len(vp.view_list) == 1 and len(kt.track_list) == 1 and kt.kt_upload_bytes == up
    finally:
        kt.kt_release()
