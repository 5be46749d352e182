"""The scene's one camera-major observation list (BaScene::cam_ptr / cam_obs, ba_cam_list_ensure) under its two users, the
row-panel Schur product (SFM_SCHUR_ROWS) and the motion-only refinement (sfm_ba_refine_cameras): either may build it, it
follows the scene through a growth and a cull, and an empty camera is empty to both.

Bounds: refine_cameras is bit-equal between handles (its summation order is fixed and the list has one order); the rows
iterations are held to 1e-9 relative (max-norm) against each other and the oracle, the bound of the rows cases of
test_gpu_parity.py -- the product adds through unordered LDS atomics, so its bits are not repeatable."""
from types import SimpleNamespace

import numpy as np
import pytest

import _motion_reference as mr
import _screen_reference as sr

pytestmark = pytest.mark.gpu

TOL = 1e-9                    # test_gpu_parity.TOL
LAM_BA, LAM_MO, ITERS = 5.0, 0.1, 2
V_A, N_A, EMPTY, CAM64 = 12, 300, 5, 8
N_NEW_PTS = 5                 # points the appended camera brings along

_CACHE = {}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _subscene(sfm, full, mask):
    """The observations (point, camera) of the fully visible scene ``full`` that ``mask`` (N, V) selects."""
    n, v = mask.shape
    pt_idx, cam_idx = (a.astype(np.int32) for a in np.nonzero(mask))
    pt_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(mask.sum(axis=1), out=pt_ptr[1:])
    uvn = sfm.geometry.normalise_pixels(full.uv_pix, full.intrinsic)
    uv = np.ascontiguousarray(uvn[:, pt_idx.astype(np.int64) * full.n_cams + cam_idx])
    out = SimpleNamespace(n_cams=v, n_pts=n, pt_ptr=pt_ptr, cam_idx=cam_idx, pt_idx=pt_idx, uv=uv,
                          cams=full.cams_init[:v].copy(), pts=full.pts_init[:, :n].copy())
    for a in (out.pt_ptr, out.cam_idx, out.pt_idx, out.uv, out.cams, out.pts):
        a.setflags(write=False)
    return out


def _universe(sfm):
    """13 cameras x 305 points, fully visible: scene A is cut from cameras 0-11 and points 0-299, the growth of check 2
    brings camera 12 and points 300-304."""
    if "universe" not in _CACHE:
        _CACHE["universe"] = sfm.scenes.make_scene(V_A + 1, N_A + N_NEW_PTS, 1.0, seed=77)
    return _CACHE["universe"]


def _scene_a(sfm):
    """12 cameras x 300 points at about 55 %: camera EMPTY sees nothing, camera CAM64 exactly 64 points, every point is
    seen at least twice; more than 1 024 observations = two chunks of the list's fill, every other camera on both sides."""
    if "A" not in _CACHE:
        rng = np.random.default_rng(4)
        mask = rng.random((N_A, V_A)) < 0.645
        mask[:, [EMPTY, CAM64]] = False
        mask[rng.choice(N_A, 64, replace=False), CAM64] = True
        others = [c for c in range(V_A) if c not in (EMPTY, CAM64)]
        for p in np.flatnonzero(mask.sum(axis=1) < 2):
            mask[p, rng.choice(others, 2, replace=False)] = True
        a = _subscene(sfm, _universe(sfm), mask)
        counts = np.bincount(a.cam_idx, minlength=V_A)
        m = a.cam_idx.shape[0]
        assert 1800 <= m <= 2200 and 0.5 <= m / (V_A * N_A) <= 0.6, m
        assert counts[EMPTY] == 0 and counts[CAM64] == 64 and np.diff(a.pt_ptr).min() >= 2
        for c in others:                                               # observations on both sides of index 1 024
            own = np.flatnonzero(a.cam_idx == c)
            assert own[0] < 1024 <= own[-1]
        _CACHE["A"] = a
    return _CACHE["A"]


def _scene_b(sfm):
    """3 cameras x 10 points, fully visible: 30 observations, one partial wave round of a single chunk."""
    if "B" not in _CACHE:
        full = sfm.scenes.make_scene(3, 10, 1.0, seed=78)
        b = _subscene(sfm, full, np.ones((10, 3), dtype=bool))
        assert b.cam_idx.shape[0] == 30
        _CACHE["B"] = b
    return _CACHE["B"]


def _refine(prob):
    cost, status = prob.refine_cameras(LAM_MO, ITERS, want_cost=True, want_status=True)
    return prob.get_state()[0], cost, status


def _rows(hip, prob):
    prob.set_option(hip.OPT_SCHUR, hip.SCHUR_ROWS)
    prob.iterate(LAM_BA, ITERS)
    assert prob.info(hip.INFO_SCHUR_KERNEL) == hip.SCHUR_ROWS
    return prob.get_state()


def _both_users(hip, prob, cams, pts, rows_first):
    """refine_cameras and two rows iterations, each from (cams, pts), in the given order: (refine outputs, rows state)."""
    prob.set_state(cams, pts)
    if rows_first:
        rows = _rows(hip, prob)
        prob.set_state(cams, pts)
        return _refine(prob), rows
    refined = _refine(prob)
    prob.set_state(cams, pts)
    return refined, _rows(hip, prob)


def _either_builds(hip, name, sc):
    """Check 1 on ``sc``, run once: handle 1 refines first, handle 2 iterates first."""
    if ("either", name) not in _CACHE:
        out = []
        for rows_first in (False, True):
            with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, sc.uv) as prob:
                out.append(_both_users(hip, prob, sc.cams, sc.pts, rows_first))
        _CACHE[("either", name)] = out
    return _CACHE[("either", name)]


def _assert_same_results(oracle, got, want, cams, pts, cam_idx, pt_idx, uv, what):
    """``got`` and ``want`` are (refine outputs, rows state) of two handles from the same state of the same scene."""
    (ref_g, rows_g), (ref_w, rows_w) = got, want
    assert all(same_bits(a, b) for a, b in zip(ref_g, ref_w)), what
    ocams, opts = oracle.ba_sparse(cams, pts, cam_idx, pt_idx, uv, LAM_BA, ITERS)
    figures = [rel(rows_g[0], rows_w[0]), rel(rows_g[1], rows_w[1])] + [rel(r[0], ocams) for r in (rows_g, rows_w)] + \
              [rel(r[1], opts) for r in (rows_g, rows_w)]
    print(what, figures)
    assert max(figures) < TOL, (what, figures)
    want_c, want_cost, want_st = mr.refine_cameras(cams, pts, cam_idx, pt_idx, uv, LAM_MO, ITERS)
    assert rel(ref_g[0], want_c) < TOL and rel(ref_g[1], want_cost) < TOL and np.array_equal(ref_g[2], want_st), what


# ---- 1: either user may build the list ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_either_user_builds_the_list(hip, sfm, oracle, name):
    sc = {"A": _scene_a, "B": _scene_b}[name](sfm)
    first, second = _either_builds(hip, name, sc)
    _assert_same_results(oracle, first, second, sc.cams, sc.pts, sc.cam_idx, sc.pt_idx, sc.uv, name)
    assert not np.array_equal(first[0][0], sc.cams) and not np.array_equal(first[1][0], sc.cams)      # both did something


# ---- 2: the list follows the scene ----------------------------------------------------------------------------------
def _changed_against_fresh(hip, oracle, prob, what):
    """``prob`` holds lists of the scene before its change: against a fresh handle of its structure and state, with the
    two users in the other order."""
    pt_ptr, cam_idx, uv = prob.structure()
    cams, pts = prob.get_state()
    v = prob.info(hip.INFO_N_CAMS)
    got = _both_users(hip, prob, cams, pts, rows_first=False)
    with hip.BaProblem(v, pt_ptr, cam_idx, uv) as fresh:
        want = _both_users(hip, fresh, cams, pts, rows_first=True)
    pt_idx = np.repeat(np.arange(pt_ptr.shape[0] - 1), np.diff(pt_ptr)).astype(np.int32)
    _assert_same_results(oracle, got, want, cams, pts, cam_idx, pt_idx, uv, what)
    return got


def test_the_list_follows_an_append(hip, sfm, oracle):
    a, full = _scene_a(sfm), _universe(sfm)
    rng = np.random.default_rng(6)
    old_pts = np.sort(rng.choice(N_A, 40, replace=False))
    new_pts = np.arange(N_A, N_A + N_NEW_PTS)
    obs_pt = np.concatenate((old_pts, new_pts, new_pts, new_pts)).astype(np.int32)       # the new points: cameras 12, 1 and 2
    obs_cam = np.concatenate((np.full(40 + N_NEW_PTS, V_A), np.full(N_NEW_PTS, 1), np.full(N_NEW_PTS, 2))).astype(np.int32)
    uvn = sfm.geometry.normalise_pixels(full.uv_pix, full.intrinsic)
    uv_new = np.ascontiguousarray(uvn[:, obs_pt.astype(np.int64) * full.n_cams + obs_cam])
    with hip.BaProblem(a.n_cams, a.pt_ptr, a.cam_idx, a.uv) as prob:
        _both_users(hip, prob, a.cams, a.pts, rows_first=True)         # list, entries and plan of the scene before the growth
        prob.set_state(a.cams, a.pts)
        prob.append(full.cams_init[V_A:], full.pts_init[:, N_A:], obs_cam, obs_pt, uv_new)
        assert prob.info(hip.INFO_N_CAMS) == V_A + 1 and prob.info(hip.INFO_N_OBS) == a.cam_idx.shape[0] + obs_cam.shape[0]
        (_cams, _cost, status), _rows_state = _changed_against_fresh(hip, oracle, prob, "append")
    assert status[EMPTY] == hip.CAM_EMPTY and not np.delete(status, EMPTY).any()


def test_the_list_follows_a_cull(hip, sfm, oracle):
    a, full = _scene_a(sfm), _universe(sfm)
    scale = float(np.sqrt(abs(full.intrinsic[0, 0] * full.intrinsic[1, 1])))
    rng = np.random.default_rng(8)
    long_tracks = np.flatnonzero(np.diff(a.pt_ptr) >= 4)
    planted = np.array([a.pt_ptr[p] + 1 for p in rng.choice(long_tracks, 7, replace=False)])
    uv = a.uv.copy()
    uv[:, planted] += 150.0 / scale                                    # gross outliers: 150 px each way
    with hip.BaProblem(a.n_cams, a.pt_ptr, a.cam_idx, uv) as prob:
        _both_users(hip, prob, a.cams, a.pts, rows_first=False)        # lists of the scene before the cull
        prob.set_state(full.cams_true[:V_A], full.pts_true[:, :N_A])
        report = prob.cull((20.0 / scale) ** 2, 1.0, 2)
        dropped = np.flatnonzero(report.obs_flags)
        assert np.array_equal(dropped, np.sort(planted)), dropped
        assert prob.info(hip.INFO_N_OBS) == a.cam_idx.shape[0] - planted.shape[0]
        prob.set_state(a.cams, a.pts)
        _changed_against_fresh(hip, oracle, prob, "cull")


# ---- 3: an empty camera, the list built by the rows product -----------------------------------------------------------
def test_empty_camera_after_rows_built_the_list(hip, sfm):
    a = _scene_a(sfm)
    (cams, cost, status), _rows_state = _either_builds(hip, "A", a)[1]
    assert status[EMPTY] == hip.CAM_EMPTY and not np.delete(status, EMPTY).any()
    assert same_bits(cams[EMPTY], a.cams[EMPTY]) and not cost[:, EMPTY].any()
    others = np.arange(V_A) != EMPTY
    assert np.all(cost[1, others] < cost[0, others])
