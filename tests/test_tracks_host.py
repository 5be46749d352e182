"""Host-side tests of triangulation over ragged tracks (sfm_tri_tracks / sfm_ba_refine_points): the NumPy reference the
GPU tests compare against is pinned to the oracle, the C ABI declares and exports the entry points, and the Python
layer rejects malformed calls before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import _tracks_reference as tr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sfm_tri_tracks", "sfm_tri_tracks_dev", "sfm_ba_refine_points")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def test_reference_helper_equals_the_oracle_on_an_all_visible_scene(sfm, oracle):
    sc = sfm.scenes.make_scene(4, 40, 1.0, seed=3)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    projs = tr.camera_projections(sfm, sc.cams_true)
    x_init = np.vstack((sc.pts_init, np.ones((1, sc.n_pts))))
    got, cost = tr.refine_tracks_reference(sc.pt_ptr, sc.cam_idx, uvn, projs, x_init, 0.5, 12)
    pairs = [uvn[:, sc.cam_idx == c] for c in range(sc.n_cams)]
    want = oracle.nonlinear_triangulate_vec(x_init, list(projs), pairs, 0.5, 12)
    assert rel(got, want) < 1e-12
    assert np.array_equal(got[3], x_init[3])
    # the cost rows are the oracle's own residual, before and after
    for row, x in ((0, x_init), (1, want)):
        want_cost = np.zeros(sc.n_pts)
        for v in range(sc.n_cams):
            s = projs[v] @ x
            want_cost += (s[0] / s[2] - pairs[v][0]) ** 2 + (s[1] / s[2] - pairs[v][1]) ** 2
        assert rel(cost[row], want_cost) < 1e-12
    # DLT helper against the vectorised SVD of the rectangular case
    lin, solved = tr.dlt_tracks_reference(sc.pt_ptr, sc.cam_idx, uvn, projs)
    a = np.empty((sc.n_pts, 2 * sc.n_cams, 4))
    for v in range(sc.n_cams):
        a[:, 2 * v] = pairs[v][0][:, None] * projs[v, 2] - projs[v, 0]
        a[:, 2 * v + 1] = pairs[v][1][:, None] * projs[v, 2] - projs[v, 1]
    vh = np.linalg.svd(a)[2]
    assert solved.all() and rel(lin, (vh[:, -1, :] / vh[:, -1, 3:4]).T) < 1e-12


@pytest.mark.parametrize("lam,iters,before,after", [(0.5, 100, 0.135, 0.0042), (5.0, 3, 0.134, 0.055)])
def test_reference_lowers_the_cost_of_every_solvable_point(sfm, lam, iters, before, after):
    rs = tr.ragged_scene(sfm)
    assert sorted(set(rs.lengths.tolist())) == list(tr.TRACK_LENGTHS) and rs.n_pts == 66
    assert all(np.all(np.diff(rs.cam_idx[rs.pt_ptr[p]:rs.pt_ptr[p + 1]]) > 0) for p in range(rs.n_pts))
    x, cost = tr.ragged_reference(sfm, lam, iters)
    many = rs.lengths >= 2
    assert np.all(cost[1, many] < cost[0, many])
    assert np.all(cost[:, rs.lengths == 0] == 0) and np.array_equal(x[:, rs.lengths == 0], rs.x_init[:, rs.lengths == 0])
    # the totals worked out on the CPU for this construction (summed squared residual, normalised units), loosely
    assert 0.5 * before < cost[0].sum() < 2 * before
    assert 0.5 * after < cost[1].sum() < 2 * after


def test_header_declares_and_library_exports_the_entry_points(sfm):
    header = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in sfm.native.EXPORTS
    for name, value in (("SFM_TRACKS_LINEAR", 1), ("SFM_TRACKS_NONLINEAR", 2), ("SFM_TRACK_TOO_FEW", 1),
                        ("SFM_TRACK_NONFINITE", 2), ("SFM_TRACK_BEHIND", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    n = sfm.native
    assert (n.TRACKS_LINEAR, n.TRACKS_NONLINEAR, n.TRACK_TOO_FEW, n.TRACK_NONFINITE, n.TRACK_BEHIND) == (1, 2, 1, 2, 4)
    lib = ctypes.CDLL(sfm.native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.sfm_version() >= 101


def test_tri_tracks_rejects_malformed_calls_without_a_device(sfm, monkeypatch):
    n = sfm.native

    def no_device(*a, **k):
        raise AssertionError("the library must not be reached")
    monkeypatch.setattr(n, "load", no_device)
    pt_ptr = np.array([0, 2, 5], dtype=np.int32)
    cam_idx = np.array([0, 1, 0, 1, 2], dtype=np.int32)
    uv = np.zeros((2, 5)); projs = np.zeros((3, 3, 4)); x = np.ones((4, 2))
    with pytest.raises(ValueError, match="uv"):
        n.tri_tracks(pt_ptr, cam_idx, np.zeros((2, 4)), projs, x)
    with pytest.raises(ValueError, match="pt_ptr"):
        n.tri_tracks(np.array([0, 2, 4], dtype=np.int32), cam_idx, uv, projs, x)
    with pytest.raises(ValueError, match="group"):
        n.tri_tracks(pt_ptr, cam_idx, uv, projs, x, group=3)
    with pytest.raises(ValueError, match="X_init"):
        n.tri_tracks(pt_ptr, cam_idx, uv, projs, None, mode=n.TRACKS_NONLINEAR)
    with pytest.raises(ValueError, match="X_init"):
        n.tri_tracks(pt_ptr, cam_idx, uv, projs, np.ones((4, 3)))
    with pytest.raises(ValueError, match="mode"):
        n.tri_tracks(pt_ptr, cam_idx, uv, projs, x, mode=4)
    with pytest.raises(ValueError, match="projs"):
        n.tri_tracks(pt_ptr, cam_idx, uv, np.zeros((3, 4, 3)), x)
    with pytest.raises(ValueError, match="integer"):
        n.tri_tracks(pt_ptr.astype(np.float64), cam_idx, uv, projs, x)
    with pytest.raises(ValueError, match="iters"):
        n.tri_tracks(pt_ptr, cam_idx, uv, projs, x, iters=-1)


def test_dropin_methods_exist_and_process_does_not_call_them(sfm):
    import inspect
    P = sfm.processors
    sig = inspect.signature(P.HipTriangulationMixin.triangulate_tracks)
    assert list(sig.parameters) == ["self", "projs", "pt_ptr", "cam_idx", "uv", "init_3d_pts", "damping_factor", "iteration"]
    sig = inspect.signature(P.HipBaMixin.refine_structure)
    assert list(sig.parameters) == ["self", "damping_factor", "iteration", "relinearize"]
    assert sig.parameters["relinearize"].default is False
    for fn in (P.HipBaProcessor.process, P.HipBaProcessor._process_two_view, P.HipBaProcessor._process_register):
        src = inspect.getsource(fn)
        assert "refine_structure" not in src and "triangulate_tracks" not in src
    bp = P.HipBaProcessor(None, None, None, None, None)
    bp.ba_resident = False
    with pytest.raises(TypeError, match="ba_resident"):
        bp.refine_structure()


def test_automatic_group_width_follows_the_written_rule(sfm):
    """the narrowest width whose lanes can cache the longest track (6 observations each), widened
    while the call has fewer than 2 waves per SIMD (2 048 waves on 256 CUs) and the next width is no wider than the longest
    track.  The three measured shapes first; host only."""
    auto = sfm.native.tracks_auto_group
    assert auto(20000, 599866, 43) == 8          # C3
    assert auto(12500, 374507, 50) == 16         # one GPU's share of C4
    assert auto(5000, 17263, 10) == 8            # C5-like
    assert auto(1000000, 3000000, 3) == 1        # the rectangular kernel's shape: a thread per point
    assert auto(1000000, 7000000, 7) == 4
    assert auto(66, 2667, 130) == 64
    assert auto(3, 9, 3) == 1                    # nothing to widen over
    assert auto(100, 0, 0) == 1
    assert auto(10, 5000, 500) == 64
    for args in ((20000, 599866, 43), (5, 20, 4), (100000, 10 ** 6, 10)):
        assert auto(*args) in sfm.native.TRACK_GROUPS[1:]
