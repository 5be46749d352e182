"""Host-side tests of the screening and culling of the resident scene (sfm_ba_screen / sfm_ba_cull): the NumPy reference
the GPU tests compare against is pinned to the track reference and to a hand-written case, the C ABI declares and exports
the entry points, the Python layers reject malformed calls before any device call, and the culled-pair filter of the
drop-in's rebuild path does what a by-hand filter does."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _screen_reference as sr
import _tracks_reference as tr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sfm_ba_screen", "sfm_ba_cull")


def test_reference_err2_summed_per_point_is_the_track_cost(sfm):
    rs = tr.ragged_scene(sfm)
    ref = sr.screen_reference(rs.pt_ptr, rs.cam_idx, rs.uv, rs.scene.cams_true, rs.x_init[0:3])
    want = tr.track_cost(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init)
    got = np.array([ref.err2[rs.pt_ptr[p]:rs.pt_ptr[p + 1]].sum() for p in range(rs.n_pts)])
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(want)
    single = np.repeat(rs.lengths == 1, rs.lengths)       # a single observation is below min_obs = 2: dropped with its point
    assert np.all(ref.depth > 0) and np.array_equal(ref.obs_flags, np.where(single, sr.OBS_POINT, 0))
    assert np.array_equal(ref.pt_flags == sr.PT_EMPTY, rs.lengths == 0)
    assert np.array_equal(ref.pt_flags == sr.PT_TOO_FEW, rs.lengths == 1)
    assert np.all(ref.min_cos[rs.lengths < 2] == 1.0) and np.all(ref.min_cos[rs.lengths >= 2] < 1.0)
    # the angles worked out on the CPU for this construction
    ang = np.degrees(np.arccos(ref.min_cos[rs.lengths >= 2]))
    assert 2.0 < ang.min() < 3.0 and 20.0 < ang.max() < 21.0


def test_cull_reference_on_a_hand_written_case(sfm):
    """Four points seen from cameras on the x axis looking along +z (identity rotations): point 0 loses one observation
    to the error test, point 1 one to the depth test and then falls below min_obs, point 2 is far away (low angle),
    point 3 is empty."""
    cams = np.zeros((3, 7)); cams[:, 3] = 1.0
    cams[:, 0] = [0.0, 1.0, 2.0]
    pts = np.array([[0.5, 0.0, 1.0, 0.0],
                    [0.0, 0.0, 0.0, 0.0],
                    [4.0, 4.0, 1000.0, 1.0]])
    pt_ptr = np.array([0, 3, 5, 7, 7], dtype=np.int32)
    cam_idx = np.array([0, 1, 2, 0, 1, 0, 2], dtype=np.int32)
    uv = np.empty((2, 7))
    for o, (p, c) in enumerate(zip([0, 0, 0, 1, 1, 2, 2], cam_idx)):
        d = pts[:, p] - cams[c, 0:3]
        uv[:, o] = d[0:2] / d[2]
    uv[0, 2] += 0.5                                     # observation 2 is a gross outlier
    moved = pts.copy()
    ref = sr.screen_reference(pt_ptr, cam_idx, uv, cams, moved, max_err2=0.01, cos_min_angle=np.cos(np.radians(1.0)), min_obs=2)
    assert ref.obs_flags.tolist() == [0, 0, sr.OBS_HIGH_ERROR, 0, 0, sr.OBS_POINT, sr.OBS_POINT]
    assert ref.pt_flags.tolist() == [0, 0, sr.PT_LOW_ANGLE, sr.PT_EMPTY]
    # now camera 1 looks the other way for point 1: put the point behind it
    cams_b = cams.copy()
    cams_b[1, 2] = 8.0                                  # camera 1 moved beyond points 0 and 1 along z
    ref = sr.screen_reference(pt_ptr, cam_idx, uv, cams_b, moved, max_err2=np.inf, cos_min_angle=1.0, min_obs=2)
    assert ref.obs_flags.tolist() == [0, sr.OBS_BEHIND, 0, sr.OBS_POINT, sr.OBS_BEHIND, 0, 0]
    assert ref.pt_flags.tolist() == [0, sr.PT_TOO_FEW, 0, sr.PT_EMPTY]
    assert ref.summary.tolist() == [7, 4, 0, 2, 0, 1, 1, 0]
    assert ref.keep.tolist() == [2, 0, 2, 0]
    new_ptr, new_cam, new_uv = sr.cull_reference(pt_ptr, cam_idx, uv, cams_b, moved, np.inf, 1.0, 2)
    assert new_ptr.tolist() == [0, 2, 2, 4, 4]
    assert new_cam.tolist() == [0, 2, 0, 2]
    assert new_uv.tobytes() == np.ascontiguousarray(uv[:, [0, 2, 5, 6]]).tobytes()
    # min_obs = 0 keeps a point with nothing left; its survivors stay
    ref = sr.screen_reference(pt_ptr, cam_idx, uv, cams_b, moved, np.inf, 1.0, 0)
    assert ref.obs_flags.tolist() == [0, sr.OBS_BEHIND, 0, 0, sr.OBS_BEHIND, 0, 0] and ref.keep.tolist() == [2, 1, 2, 0]


def test_threshold_in_gap_sits_between_two_values():
    v = np.random.default_rng(3).random(500) ** 2
    for q in (0.0, 0.5, 0.9, 1.0):
        t = sr.threshold_in_gap(v, q)
        below = np.count_nonzero(v < t)
        assert 0 < below < 500 and abs(below - q * 499) <= 40
        assert np.min(np.abs(v - t)) >= 0.5e-4 * t
    with pytest.raises(AssertionError):
        sr.threshold_in_gap(np.ones(50), 0.5)


def test_header_declares_and_library_exports_the_entry_points(sfm):
    header = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in sfm.native.EXPORTS
        assert not name.startswith("sfm_track_")
    n = sfm.native
    for name, value, mine in (("SFM_OBS_HIGH_ERROR", 1, n.OBS_HIGH_ERROR), ("SFM_OBS_BEHIND", 2, n.OBS_BEHIND),
                              ("SFM_OBS_NONFINITE", 4, n.OBS_NONFINITE), ("SFM_OBS_POINT", 8, n.OBS_POINT),
                              ("SFM_PT_TOO_FEW", 1, n.PT_TOO_FEW), ("SFM_PT_LOW_ANGLE", 2, n.PT_LOW_ANGLE),
                              ("SFM_PT_EMPTY", 4, n.PT_EMPTY)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
        assert mine == value
    assert (sr.OBS_HIGH_ERROR, sr.OBS_BEHIND, sr.OBS_NONFINITE, sr.OBS_POINT) == (1, 2, 4, 8)
    assert (sr.PT_TOO_FEW, sr.PT_LOW_ANGLE, sr.PT_EMPTY) == (1, 2, 4)
    assert len(n.SIGNATURES["sfm_ba_screen"]) == len(n.SIGNATURES["sfm_ba_cull"]) == 12
    assert len(n.SCREEN_SUMMARY) == 8
    lib = ctypes.CDLL(sfm.native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.sfm_version() >= 102


def test_screen_rejects_malformed_calls_without_a_device(sfm, monkeypatch):
    n = sfm.native

    def no_device(*a, **k):
        raise AssertionError("the library must not be reached")
    monkeypatch.setattr(n, "load", no_device)
    prob = n.BaProblem.__new__(n.BaProblem)             # a handle-less object: the checks come before any use of it
    prob.n_cams, prob._h, prob._lib = 3, None, None
    for method in (prob.screen, prob.cull):
        with pytest.raises(ValueError, match="max_err2"):
            method(max_err2=float("nan"))
        with pytest.raises(ValueError, match="max_err2"):
            method(max_err2=-1.0)
        with pytest.raises(ValueError, match="min_obs"):
            method(min_obs=-1)
        with pytest.raises(ValueError, match="cam_scale"):
            method(cam_scale=np.ones(4))
        with pytest.raises(ValueError, match="cos_min_angle"):
            method(cos_min_angle=-1.5)
        with pytest.raises(ValueError, match="cos_min_angle"):
            method(cos_min_angle=float("nan"))
        with pytest.raises(ValueError, match="group"):
            method(group=3)
    assert n.check_screen(3, np.inf, 1.0, 0, [1.0, 2.0, 3.0])[3].dtype == np.float64


def test_dropin_methods_exist_and_process_does_not_call_them(sfm):
    P = sfm.processors
    sig = inspect.signature(P.HipBaMixin.screen_structure)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("max_reproj_px", None), ("min_angle_deg", None), ("min_obs", 2)]
    sig = inspect.signature(P.HipBaMixin.filter_structure)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("max_reproj_px", 4.0), ("min_angle_deg", 1.5), ("min_obs", 2)]
    sig = inspect.signature(sfm.native.BaProblem.screen)
    assert list(sig.parameters)[:6] == ["self", "max_err2", "cos_min_angle", "min_obs", "cam_scale", "want_outputs"]
    assert sig.parameters["max_err2"].default == np.inf and sig.parameters["cos_min_angle"].default == 1.0
    assert sig.parameters["min_obs"].default == 2 and sig.parameters["want_outputs"].default is True
    assert list(inspect.signature(sfm.native.BaProblem.cull).parameters) == list(sig.parameters)
    for fn in (P.HipBaProcessor.process, P.HipBaProcessor._process_two_view, P.HipBaProcessor._process_register,
               P.HipBaMixin.execute_bundle_adjustment, P.HipBaMixin.refine_structure):
        src = inspect.getsource(fn)
        assert "screen_structure" not in src and "filter_structure" not in src
    assert "7e-6" in P.HipBaMixin.screen_structure.__doc__


def test_filter_structure_needs_the_resident_host_track_scene(sfm):
    P = sfm.processors
    bp = P.HipBaProcessor(None, None, None, None, None)
    bp.ba_resident = False
    with pytest.raises(TypeError, match="ba_resident"):
        bp.filter_structure()
    with pytest.raises(TypeError, match="ba_resident"):
        bp.screen_structure()
    bp = P.HipBaProcessor(None, None, None, None, None)
    bp.ba_device_tracks = True
    with pytest.raises(TypeError, match="ba_device_tracks"):
        bp.filter_structure()
    # malformed thresholds are refused before the views are read
    bp = P.HipBaProcessor(None, None, None, None, None)
    with pytest.raises(ValueError, match="max_reproj_px"):
        bp.filter_structure(max_reproj_px=-1.0)
    with pytest.raises(ValueError, match="min_obs"):
        bp.screen_structure(min_obs=-2)


def test_remove_pairs_equals_a_filter_by_hand(sfm):
    obs = sfm.observations
    rng = np.random.default_rng(8)
    n_pts = 30
    rows = []
    for _c in range(5):
        row = np.full(50, -1, dtype=np.int64)
        seen = rng.choice(n_pts, size=18, replace=False)
        row[rng.choice(np.arange(1, 50), size=18, replace=False)] = seen
        rows.append(row)
    full = obs.build_observations(rows, n_pts)
    pt_ptr, cam_idx, pt_idx, key_idx = full
    m = cam_idx.shape[0]
    assert m == 90
    gone = rng.choice(m, size=25, replace=False)
    gone_pt, gone_cam = pt_idx[gone], cam_idx[gone]
    # plus pairs the list does not hold: ignored
    extra_pt = np.array([0, n_pts + 5], dtype=np.int64)
    extra_cam = np.array([7, 1], dtype=np.int64)
    got = obs.remove_pairs(full, np.concatenate((gone_pt, extra_pt)), np.concatenate((gone_cam, extra_cam)))
    triples = [(int(p), int(c), int(k)) for p, c, k in zip(pt_idx, cam_idx, key_idx)
               if (int(p), int(c)) not in set(zip(gone_pt.tolist(), gone_cam.tolist()))]
    assert got[1].tolist() == [t[1] for t in triples]
    assert got[2].tolist() == [t[0] for t in triples]
    assert got[3].tolist() == [t[2] for t in triples]
    want_ptr = np.zeros(n_pts + 1, dtype=np.int64)
    for p, _c, _k in triples:
        want_ptr[p + 1:] += 1
    assert got[0].tolist() == want_ptr.tolist() and got[0].dtype == np.int32
    assert got[1].shape[0] == m - 25
    # nothing to remove: the list comes back as it is
    same = obs.remove_pairs(full, np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))
    assert all(a is b for a, b in zip(same, full))
    # a point that loses its whole track keeps its (empty) row
    p0 = int(pt_idx[0])
    sel = pt_idx == p0
    got = obs.remove_pairs(full, pt_idx[sel], cam_idx[sel])
    assert got[0][p0 + 1] == got[0][p0] and got[0][-1] == m - sel.sum()
