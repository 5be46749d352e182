"""Motion-only refinement of the resident scene (sfm_ba_refine_cameras) against the NumPy reference of
tests/_motion_reference.py: parity, the boundaries of the work split, status bits, independence of a camera's bits from
everything but its own data, the hygiene of the resident problem, and what the step achieves.

Bound: 1e-9 relative to the largest entry of the reference on cameras and costs -- the bound of the other parity tests;
the device differs from NumPy in summation order, in Cholesky against LU and in reciprocal / rsqrt refinements of a few
1e-16 each, in front of 7x7 systems whose conditioning the damping bounds."""
import numpy as np
import pytest

import _motion_reference as mr
import _robust_reference as rr
import _screen_reference as sr

pytestmark = pytest.mark.gpu

_CACHE = {}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    scale = np.max(np.abs(b[ok])) if ok.any() else 1.0
    return float(np.max(np.abs(a[ok] - b[ok])) / (scale if scale > 0 else 1.0)) if ok.any() else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _scene(sfm):
    """make_scene(6, 300, 0.7, seed=21) with normalised keys, the outlier keys, the focal scale and the two losses."""
    if "scene" not in _CACHE:
        o = sr.outlier_scene(sfm)
        sc = o.scene
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        uvo = sfm.geometry.normalise_pixels(o.uv_pix, sc.intrinsic)
        scale = float(np.sqrt(abs(sc.intrinsic[0, 0] * sc.intrinsic[1, 1])))
        for a in (uvn, uvo):
            a.setflags(write=False)
        _CACHE["scene"] = (sc, uvn, uvo, o.displaced, scale, {rr.LOSS_HUBER: 5.0 / scale, rr.LOSS_CAUCHY: 10.0 / scale})
    return _CACHE["scene"]


def _reference(key, *args, **kwargs):
    """``mr.refine_cameras`` computed once per ``key`` and left unchanged."""
    if key not in _CACHE:
        out = mr.refine_cameras(*args, **kwargs)
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def _device(hip, n_cams, pt_ptr, cam_idx, uv, cams, pts, lam, iters, quirks=None, loss=None, use_loss=False, mask=None):
    """One refine on a fresh problem: (cams, cost, status, pts)."""
    quirks = hip.QUIRKS_REFERENCE if quirks is None else quirks
    with hip.BaProblem(n_cams, pt_ptr, cam_idx, uv) as prob:
        if loss is not None:
            prob.set_loss(*loss)
        prob.set_state(cams, pts)
        cost, status = prob.refine_cameras(lam, iters, quirks, use_loss, mask, want_cost=True, want_status=True)
        out, pts_out = prob.get_state()
    return out, cost, status, pts_out


# ---- parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,use_loss", [(rr.LOSS_NONE, 0), (rr.LOSS_HUBER, 0), (rr.LOSS_HUBER, 1), (rr.LOSS_CAUCHY, 0), (rr.LOSS_CAUCHY, 1)])
def test_parity(hip, sfm, oracle, kind, use_loss):
    sc, uvn, _uvo, _disp, _scale, deltas = _scene(sfm)
    assert sc.cam_idx.shape[0] == 1249 and np.bincount(sc.cam_idx).min() == 190 and np.bincount(sc.cam_idx).max() == 228
    loss = None if kind == rr.LOSS_NONE else (kind, deltas[kind])
    eff_kind, eff_delta = (kind, deltas[kind]) if use_loss else (rr.LOSS_NONE, 1.0)
    for lam in (1e-3, 0.1):
        for iters in (0, 1, 5):
            for quirks in (oracle.QUIRKS_REFERENCE, 0):
                want_c, want_cost, want_st = _reference(("parity", lam, iters, quirks, eff_kind), sc.cams_init, sc.pts_init, sc.cam_idx,
                                                        sc.pt_idx, uvn, lam, iters, eff_kind, eff_delta, quirks)
                cams, cost, status, pts = _device(hip, sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn, sc.cams_init, sc.pts_init, lam, iters,
                                                  quirks, loss, use_loss)
                where = (kind, use_loss, lam, iters, quirks)
                print(where, rel(cams, want_c), rel(cost, want_cost))
                assert rel(cams, want_c) < 1e-9 and rel(cost, want_cost) < 1e-9, where
                assert np.array_equal(status, want_st) and not status.any(), where
                assert same_bits(pts, sc.pts_init), where
                if iters == 0:
                    assert same_bits(cams, sc.cams_init) and same_bits(cost[0], cost[1]), where
                if loss is not None and not use_loss:                  # a loss that is not asked for changes no bit
                    key = ("plain device", lam, iters, quirks)
                    if key not in _CACHE:
                        _CACHE[key] = _device(hip, sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn, sc.cams_init, sc.pts_init, lam, iters, quirks)[0:3]
                    assert all(same_bits(a, b) for a, b in zip((cams, cost, status), _CACHE[key])), where


@pytest.mark.parametrize("kind", [rr.LOSS_NONE, rr.LOSS_HUBER, rr.LOSS_CAUCHY])
def test_cost_row_0_is_the_adjustments_cost(hip, sfm, kind):
    sc, uvn, _uvo, _disp, _scale, deltas = _scene(sfm)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        if kind != rr.LOSS_NONE:
            prob.set_loss(kind, deltas[kind])
        prob.set_state(sc.cams_init, sc.pts_init)
        prob.iterate(0.5, 2)
        cost, _status = prob.refine_cameras(0.1, 0, use_loss=True, want_cost=True)
        assert prob.get_stats().shape == (0,)                          # the cost history restarts
        prob.iterate(0.5, 1)
        stats = prob.get_stats()
    print(kind, float(np.sum(cost[0])), stats)
    assert stats.shape == (1,) and abs(float(np.sum(cost[0])) - stats[0]) <= 1e-12 * stats[0]


# ---- boundaries of the work split ---------------------------------------------------------------------------------
V_B = 8
N_GROUPS = 4                   # scenes the boundary sizes fill, six cameras each
BIG_GROUPS = [2, 3]            # ... and those whose cameras span the larger size classes


def _boundary_sizes(hip):
    """Observation counts at which the plan changes, each at -1, 0, +1, plus the fixed small ones and two slices + 1; the
    class boundaries are found by asking the plan.  Beyond a boundary b the next class works through b observations at a
    time or more: 2 b + 1 and 3 b + 5 make it go round several times with a ragged end."""
    if "sizes" not in _CACHE:
        slice_obs = hip.refine_cameras_plan(1)[1]
        sizes = {1, 3, 7, 64, 65, slice_obs - 1, slice_obs, slice_obs + 1, 2 * slice_obs + 1}
        bounds = [n for n in range(1, 20001) if hip.refine_cameras_plan(n + 1)[2] != hip.refine_cameras_plan(n)[2]]
        assert bounds                                                  # n is the last size of its class
        for n in bounds:
            sizes |= {n - 1, n, n + 1, 2 * n + 1, 3 * n + 5}
        sizes = sorted(s for s in sizes if s > 0)
        while len(sizes) % (V_B - 2):
            sizes.append(2)
        _CACHE["sizes"] = sizes
    return _CACHE["sizes"]


def _built_scene(n_k, seed):
    """V cameras near the origin looking down +z; camera k sees points 0 .. n_k - 1 of a cloud at depth 4 .. 8.  Returns
    (pt_ptr, cam_idx, pt_idx, uv, cams_true, cams_init, pts)."""
    rng = np.random.default_rng(seed)
    n_k = np.asarray(n_k)
    v, n = n_k.shape[0], int(n_k.max())
    pts = np.vstack((rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(4, 8, n)))
    seen = n_k[None, :] > np.arange(n)[:, None]                        # (point, camera), row-major = sorted by (point, camera)
    pt_idx, cam_idx = (a.astype(np.int32) for a in np.nonzero(seen))
    pt_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(seen.sum(axis=1), out=pt_ptr[1:])

    def cameras(spread_c, spread_q):
        c = np.hstack((rng.uniform(-spread_c, spread_c, (v, 3)), np.ones((v, 1)), rng.uniform(-spread_q, spread_q, (v, 3))))
        c[:, 3:7] /= np.linalg.norm(c[:, 3:7], axis=1)[:, None]
        return c

    cams_true = cameras(0.5, 0.05)
    cams_init = cams_true + np.hstack((rng.uniform(-0.05, 0.05, (v, 3)), np.zeros((v, 1)), rng.uniform(-0.01, 0.01, (v, 3))))
    cams_init[:, 3:7] /= np.linalg.norm(cams_init[:, 3:7], axis=1)[:, None]
    oracle = rr._oracle()
    r = oracle.obs_terms_vec(cams_true, pts, cam_idx, pt_idx, np.zeros((2, cam_idx.shape[0])))[0]
    uv = -r.T + rng.normal(0, 1e-3, (2, cam_idx.shape[0]))            # the projection plus a pixel of noise
    return pt_ptr, cam_idx, pt_idx, np.ascontiguousarray(uv), cams_true, cams_init, pts


# The built scenes are refined with the quirk-free Jacobian: their field of view is wide, and with the reference's sign in
# the v-row of J_C (Q2) the undamped step does not contract on the largest cameras -- the parity tests keep Q2.
def _boundary_scene(hip, group):
    key = ("bscene", group)
    if key not in _CACHE:
        sizes = _boundary_sizes(hip)
        n_k = [0] + sizes[group * (V_B - 2):(group + 1) * (V_B - 2)] + [0]      # cameras 0 and V - 1 are empty
        _CACHE[key] = (n_k, _built_scene(n_k, 100 + group))
    return _CACHE[key]


def test_boundary_sizes_cover_the_plan(hip):
    sizes = _boundary_sizes(hip)
    classes = {hip.refine_cameras_plan(n)[2] for n in sizes}
    assert {1, 3, 7, 64, 65} <= set(sizes) and len(classes) >= 2 and len(sizes) // (V_B - 2) == N_GROUPS, sizes


@pytest.mark.parametrize("group", range(N_GROUPS))
def test_boundaries(hip, group):
    n_k, (pt_ptr, cam_idx, pt_idx, uv, _true, cams0, pts) = _boundary_scene(hip, group)
    assert np.array_equal(np.bincount(cam_idx, minlength=V_B), n_k)
    r0 = rr._oracle().obs_terms_vec(cams0, pts, cam_idx, pt_idx, uv)[0]
    delta = float(np.sqrt(np.median(np.sum(r0 * r0, axis=1))))         # half of the observations beyond the quadratic zone
    for kind in (rr.LOSS_NONE, rr.LOSS_CAUCHY):
        want_c, want_cost, want_st = _reference(("boundary", group, kind), cams0, pts, cam_idx, pt_idx, uv, 0.1, 3, kind, delta, 0)
        cams, cost, status, _pts = _device(hip, V_B, pt_ptr, cam_idx, uv, cams0, pts, 0.1, 3, 0,
                                           loss=None if kind == rr.LOSS_NONE else (kind, delta), use_loss=kind != rr.LOSS_NONE)
        per_cam = [rel(cams[c], want_c[c]) for c in range(V_B)]
        print(group, kind, n_k, per_cam, rel(cost, want_cost))
        assert max(per_cam) < 1e-9 and rel(cams, want_c) < 1e-9 and rel(cost, want_cost) < 1e-9
        assert np.array_equal(status, want_st)
        assert status[0] == status[V_B - 1] == hip.CAM_EMPTY and not status[1:V_B - 1].any()
        assert same_bits(cams[[0, V_B - 1]], cams0[[0, V_B - 1]]) and not cost[:, [0, V_B - 1]].any()
        assert np.all(want_cost[1, 1:V_B - 1] < want_cost[0, 1:V_B - 1])


@pytest.mark.parametrize("group", BIG_GROUPS)
def test_status_bits(hip, group):
    n_k, (pt_ptr, cam_idx, pt_idx, uv, _true, cams0, pts) = _boundary_scene(hip, group)
    big = int(np.argmax(n_k))
    assert sorted(n_k)[-1] > sorted(n_k)[-2]
    # HELD under a mask
    mask = np.ones(V_B, dtype=np.uint8)
    mask[[0, 2, big]] = 0
    want_c, want_cost, want_st = mr.refine_cameras(cams0, pts, cam_idx, pt_idx, uv, 0.1, 2, quirks=0, mask=mask)
    cams, cost, status, _pts = _device(hip, V_B, pt_ptr, cam_idx, uv, cams0, pts, 0.1, 2, 0, mask=mask)
    assert np.array_equal(status, want_st) and status[0] == hip.CAM_EMPTY | hip.CAM_HELD and status[2] == status[big] == hip.CAM_HELD
    assert same_bits(cams[mask == 0], cams0[mask == 0]) and same_bits(cost[0, mask == 0], cost[1, mask == 0])
    assert rel(cams, want_c) < 1e-9 and rel(cost, want_cost) < 1e-9
    # BEHIND: two cameras turned by 170 degrees about y look away from every point they see
    turned = cams0.copy()
    small = int(np.argmin(np.where(np.asarray(n_k) > 0, n_k, 10 ** 9)))
    assert hip.refine_cameras_plan(n_k[small])[2] != hip.refine_cameras_plan(n_k[big])[2]
    for c in (small, big):
        turned[c, 3:7] = [np.cos(np.radians(85.0)), 0.0, np.sin(np.radians(85.0)), 0.0]
    for iters, lam in ((0, 0.1), (1, 10.0)):
        want_c, want_cost, want_st = mr.refine_cameras(turned, pts, cam_idx, pt_idx, uv, lam, iters, quirks=0)
        assert want_st[small] == want_st[big] == mr.CAM_BEHIND and np.count_nonzero(want_st == mr.CAM_BEHIND) == 2
        cams, cost, status, _pts = _device(hip, V_B, pt_ptr, cam_idx, uv, turned, pts, lam, iters, 0)
        assert np.array_equal(status, want_st)
        assert rel(cams, want_c) < 1e-9 and rel(cost, want_cost) < 1e-9
    # NONFINITE: a NaN point that only the largest camera sees, and one only the two largest see
    for count in (1, 2):
        order = np.argsort(n_k)
        hit = sorted(int(c) for c in order[-count:])
        bad = pts.copy()
        bad[1, n_k[order[-count]] - 1] = np.nan
        want_c, want_cost, want_st = mr.refine_cameras(cams0, bad, cam_idx, pt_idx, uv, 0.1, 2, quirks=0)
        assert [int(c) for c in np.flatnonzero(want_st == mr.CAM_NONFINITE)] == hit
        cams, cost, status, _pts = _device(hip, V_B, pt_ptr, cam_idx, uv, cams0, bad, 0.1, 2, 0)
        assert np.array_equal(status, want_st)
        assert same_bits(cams[hit], cams0[hit]) and np.isnan(cost[:, hit]).all()
        assert rel(cams, want_c) < 1e-9 and rel(cost, want_cost) < 1e-9


# ---- independence and repeatability -------------------------------------------------------------------------------
@pytest.mark.parametrize("group", BIG_GROUPS)
def test_a_cameras_bits_depend_on_its_own_data_only(hip, group):
    n_k, (pt_ptr, cam_idx, pt_idx, uv, _true, cams0, pts) = _boundary_scene(hip, group)
    classes = [hip.refine_cameras_plan(n)[2] for n in n_k]
    picks = [int(np.argmax(n_k)), int(np.argmin(np.where(np.asarray(n_k) > 0, n_k, 10 ** 9)))]
    assert classes[picks[0]] != classes[picks[1]]
    full = _device(hip, V_B, pt_ptr, cam_idx, uv, cams0, pts, 0.1, 3, 0)
    again = _device(hip, V_B, pt_ptr, cam_idx, uv, cams0, pts, 0.1, 3, 0)
    assert all(same_bits(a, b) for a, b in zip(full, again))            # two calls from the same state
    for c in picks:
        mask = np.zeros(V_B, dtype=np.uint8)
        mask[c] = 1
        cams, cost, status, _pts = _device(hip, V_B, pt_ptr, cam_idx, uv, cams0, pts, 0.1, 3, 0, mask=mask)
        assert same_bits(cams[c], full[0][c]) and same_bits(cost[:, c], full[1][:, c]) and status[c] == full[2][c]
        others = np.arange(V_B) != c
        assert same_bits(cams[others], cams0[others])
    # the same cameras inside a scene with two more cameras appended
    rng = np.random.default_rng(7)
    extra = cams0[[1, 2]] + 0.01
    extra[:, 3:7] /= np.linalg.norm(extra[:, 3:7], axis=1)[:, None]
    n_new = [5, 700]
    obs_cam = np.concatenate([np.full(n, V_B + i, dtype=np.int32) for i, n in enumerate(n_new)])
    obs_pt = np.concatenate([rng.choice(pts.shape[1], n, replace=False).astype(np.int32) for n in n_new])
    r = rr._oracle().obs_terms_vec(extra, pts, obs_cam - V_B, obs_pt, np.zeros((2, obs_cam.shape[0])))[0]
    with hip.BaProblem(V_B, pt_ptr, cam_idx, uv) as prob:
        prob.set_state(cams0, pts)
        prob.refine_cameras(0.1, 0, 0)                                 # the list of the old scene is built, then dropped
        prob.append(extra, np.zeros((3, 0)), obs_cam, obs_pt, np.ascontiguousarray(-r.T))
        assert prob.info(hip.INFO_N_CAMS) == V_B + 2 and prob.info(hip.INFO_N_OBS) == cam_idx.shape[0] + sum(n_new)
        cost, status = prob.refine_cameras(0.1, 3, 0, want_cost=True, want_status=True)
        cams, _pts = prob.get_state()
    assert same_bits(cams[:V_B], full[0]) and same_bits(cost[:, :V_B], full[1]) and np.array_equal(status[:V_B], full[2])
    assert not status[V_B:].any()


# ---- hygiene ------------------------------------------------------------------------------------------------------
def test_upload_accounting_and_outputs(hip, sfm):
    sc, uvn, _uvo, _disp, _scale, _deltas = _scene(sfm)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(sc.cams_init, sc.pts_init)
        up = prob.upload_bytes
        assert prob.refine_cameras(0.1, 1) == (None, None)
        assert prob.upload_bytes == up
        prob.refine_cameras(0.1, 1, mask=np.ones(sc.n_cams))
        assert prob.upload_bytes == up + sc.n_cams
        with pytest.raises(ValueError, match="mask"):
            prob.refine_cameras(0.1, 1, mask=np.ones(sc.n_cams + 1))
    with hip.BaProblem(2, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((2, 0))) as prob:      # no point at all
        up = prob.upload_bytes
        cost, status = prob.refine_cameras(0.1, 3, mask=[1, 0], want_cost=True, want_status=True)
        assert not cost.any() and list(status) == [hip.CAM_EMPTY, hip.CAM_EMPTY | hip.CAM_HELD] and prob.upload_bytes == up


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("pending", [False, True])
def test_refine_cameras_leaves_no_stale_state_behind(hip, sfm, graph, pending):
    """iterate, refine_cameras, iterate under SFM_OPT_DETERMINISTIC ends in the bits of a fresh problem started from the
    state refine_cameras left.  ``pending``: the first phase is spelled linearize_reduce / solve_update, so the back
    substitution of its last iteration is still owed when refine_cameras is called."""
    sc, uvn, _uvo, _disp, _scale, _deltas = _scene(sfm)

    def fresh():
        p = hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn)
        p.set_option(hip.OPT_DETERMINISTIC, 1)
        p.set_option(hip.OPT_GRAPH, graph)
        return p

    with fresh() as prob, fresh() as other:
        prob.set_state(sc.cams_init, sc.pts_init)
        if pending:
            for _ in range(3):
                prob.linearize_reduce(5.0)
                prob.solve_update(5.0)
        else:
            prob.iterate(5.0, 3)
        cost, status = prob.refine_cameras(0.1, 3, want_cost=True, want_status=True)
        assert not status.any() and np.all(cost[1] <= cost[0])
        cams_mid, pts_mid = prob.get_state()
        prob.iterate(5.0, 3)
        assert prob.get_stats().shape[0] == 3
        cams_end, pts_end = prob.get_state()
        other.set_state(cams_mid, pts_mid)
        other.iterate(5.0, 3)
        cams_want, pts_want = other.get_state()
        assert same_bits(cams_end, cams_want) and same_bits(pts_end, pts_want)
        assert same_bits(prob.get_stats(), other.get_stats())


def test_refine_after_a_cull_uses_the_culled_lists(hip, sfm):
    sc, _uvn, uvo, displaced, scale, deltas = _scene(sfm)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvo) as prob:
        prob.set_state(sc.cams_true, sc.pts_true)
        prob.refine_cameras(0.1, 1)                                    # builds the list of the scene before the cull
        prob.set_cameras(sc.cams_true)
        report = prob.cull((20.0 / scale) ** 2, 1.0, 2)
        assert np.all(report.obs_flags[displaced] != 0) and 0 < np.count_nonzero(report.obs_flags) < 200
        new_ptr, new_cam, new_uv = prob.structure()
        want_ptr, want_cam, want_uv = sr.compact(sc.pt_ptr, sc.cam_idx, uvo, report.obs_flags)
        assert np.array_equal(new_ptr, want_ptr) and np.array_equal(new_cam, want_cam) and same_bits(new_uv, want_uv)
        prob.set_cameras(sc.cams_init)
        cost, status = prob.refine_cameras(0.1, 4, want_cost=True, want_status=True)
        cams, pts = prob.get_state()
    pt_of = np.repeat(np.arange(sc.n_pts), np.diff(new_ptr)).astype(np.int32)
    want_c, want_cost, want_st = mr.refine_cameras(sc.cams_init, sc.pts_true, new_cam, pt_of, new_uv, 0.1, 4)
    assert rel(cams, want_c) < 1e-9 and rel(cost, want_cost) < 1e-9 and np.array_equal(status, want_st)
    assert same_bits(pts, sc.pts_true)
    stale = mr.refine_cameras(sc.cams_init, sc.pts_true, sc.cam_idx, sc.pt_idx, uvo, 0.1, 4)[0]
    assert rel(stale, want_c) > 1e-6                                   # the lists before the cull would have ended elsewhere


def test_error_paths(hip, sfm, oracle):
    sc, uvn, _uvo, _disp, _scale, _deltas = _scene(sfm)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(sc.cams_init, sc.pts_init)
        lib, state, up = prob._lib, prob.get_state(), prob.upload_bytes
        mask = np.ones(sc.n_cams, dtype=np.uint8)
        import ctypes
        mptr = mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        for lam, iters, use_loss in ((0.1, -1, 0), (float("nan"), 1, 0), (-1.0, 1, 0), (0.1, 1, 2), (0.1, 1, -1)):
            assert lib.sfm_ba_refine_cameras(prob._h, lam, iters, hip.QUIRKS_REFERENCE, use_loss, mptr, None, None) == hip.E_SHAPE
            assert prob.upload_bytes == up
        with pytest.raises(ValueError):
            prob.refine_cameras(0.1, -1)
        assert all(same_bits(a, b) for a, b in zip(prob.get_state(), state))
        # an input camera that fails the rotation checks: its status, the camera named, nothing changed.  A zero
        # quaternion expands to R = I, which the checks of the reference pass: the oracle says which case is which.
        outcomes = []
        for q in ([0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]):
            bad = sc.cams_init.copy()
            bad[3, 3:7] = q
            try:
                oracle.rot_to_quat(oracle.quat_to_rot(bad[3, 3:7]))
                valid = True
            except ValueError:
                valid = False
            outcomes.append(valid)
            prob.set_cameras(bad)
            if valid:
                want_c, want_cost, want_st = mr.refine_cameras(bad, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 0.1, 2)
                cost, status = prob.refine_cameras(0.1, 2, want_cost=True, want_status=True)
                assert rel(prob.get_state()[0], want_c) < 1e-9 and rel(cost, want_cost) < 1e-9 and np.array_equal(status, want_st)
            else:
                st = lib.sfm_ba_refine_cameras(prob._h, 0.1, 2, hip.QUIRKS_REFERENCE, 0, None, None, None)
                assert st in (hip.E_BAD_ROTATION, hip.E_QW_ZERO, hip.E_SQRT_DOMAIN) and "camera 3" in hip.last_error()
                with pytest.raises(ValueError, match="camera 3"):
                    prob.refine_cameras(0.1, 2)
                prob.set_cameras(sc.cams_init)                         # ... and the problem is as usable as before
                assert all(same_bits(a, b) for a, b in zip(prob.get_state(), state))
        assert False in outcomes                                       # at least one of the cameras was invalid


# ---- it does something ----------------------------------------------------------------------------------------------
def _rmse_px(oracle, sc, scale, cams, pts, uv, sel=None):
    r = oracle.obs_terms_vec(np.asarray(cams), pts, sc.cam_idx, sc.pt_idx, uv)[0]
    e = np.sum(r * r, axis=1)
    return scale * float(np.sqrt(np.mean(e if sel is None else e[sel])))


def test_it_does_something_on_the_clean_scene(hip, sfm, oracle):
    """Facts about the reference (checked on the CPU): from cams_init at the true points, 8 iterations at lambda = 0.1 take
    the reprojection RMSE from 9.88 px to 0.735 px."""
    sc, uvn, _uvo, _disp, scale, _deltas = _scene(sfm)
    want_c, want_cost, _st = _reference(("clean", 8), sc.cams_init, sc.pts_true, sc.cam_idx, sc.pt_idx, uvn, 0.1, 8)
    assert abs(_rmse_px(oracle, sc, scale, sc.cams_init, sc.pts_true, uvn) - 9.88) < 0.01
    assert _rmse_px(oracle, sc, scale, want_c, sc.pts_true, uvn) < 1.0
    cams, cost, status, _pts = _device(hip, sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn, sc.cams_init, sc.pts_true, 0.1, 8)
    assert rel(cams, want_c) < 1e-9 and rel(cost, want_cost) < 1e-9 and not status.any()
    assert _rmse_px(oracle, sc, scale, cams, sc.pts_true, uvn) < 1.0


@pytest.mark.parametrize("kind", [rr.LOSS_NONE, rr.LOSS_HUBER, rr.LOSS_CAUCHY])
def test_it_does_something_on_the_outlier_scene(hip, sfm, oracle, kind):
    """Facts about the reference: 3 % of the keys displaced by 30 to 120 px, true points, cams_init, lambda = 0.1, 20
    iterations; RMSE over the clean observations 5.39 px without a loss, 0.752 px with Huber at 5 px, 0.708 px with Cauchy
    at 10 px, and every displaced observation ends at weight <= 0.2 (0.162 / 0.095)."""
    sc, _uvn, uvo, displaced, scale, deltas = _scene(sfm)
    delta = deltas.get(kind, 1.0)
    want_c, want_cost, _st = _reference(("outlier", kind), sc.cams_init, sc.pts_true, sc.cam_idx, sc.pt_idx, uvo, 0.1, 20, kind, delta)
    clean = _rmse_px(oracle, sc, scale, want_c, sc.pts_true, uvo, ~displaced)
    if kind == rr.LOSS_NONE:
        assert clean > 5.0
    else:
        r = oracle.obs_terms_vec(want_c, sc.pts_true, sc.cam_idx, sc.pt_idx, uvo)[0]
        assert clean < 1.0 and np.all(rr.loss_terms(kind, delta, r)[1][displaced] <= 0.2)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvo) as prob:
        if kind != rr.LOSS_NONE:
            prob.set_loss(kind, delta)
        prob.set_state(sc.cams_init, sc.pts_true)
        cost, status = prob.refine_cameras(0.1, 20, use_loss=True, want_cost=True, want_status=True)
        cams, _pts = prob.get_state()
        w = prob.loss_terms()[1]
    assert rel(cams, want_c) < 1e-9 and rel(cost, want_cost) < 1e-9 and not status.any()
    if kind != rr.LOSS_NONE:
        assert np.all(w[displaced] <= 0.2)


# ---- two independent kernels for the same step ----------------------------------------------------------------------
def test_against_the_pnp_kernel(hip, sfm, oracle):
    sc, uvn, _uvo, _disp, _scale, _deltas = _scene(sfm)
    cams0 = sc.cams_init.copy()
    cams0[:, 3:7] /= np.linalg.norm(cams0[:, 3:7], axis=1)[:, None]
    cams, _cost, status, _pts = _device(hip, sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn, cams0, sc.pts_init, 1e-3, 5, quirks=hip.Q2_LOC_JAC_SIGN)
    assert not status.any()
    for cam in range(sc.n_cams):
        sel = sc.cam_idx == cam
        n = int(sel.sum())
        key = np.vstack((uvn[:, sel], np.ones((1, n))))
        xh = np.vstack((sc.pts_init[:, sc.pt_idx[sel]], np.ones((1, n))))
        rot, loc = hip.pnp_nonlinear(key, xh, np.eye(3), oracle.quat_to_rot(cams0[cam, 3:7]), cams0[cam, 0:3], 1e-3, 5,
                                     quirks=hip.Q2_LOC_JAC_SIGN)
        got = oracle.quat_to_rot(cams[cam, 3:7])
        assert np.max(np.abs(got - rot)) / np.max(np.abs(rot)) < 1e-9
        assert np.max(np.abs(cams[cam, 0:3] - loc.ravel())) / np.max(np.abs(loc)) < 1e-9


# ---- the drop-in --------------------------------------------------------------------------------------------------
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


def test_drop_in_refine_motion(hip, sfm):
    sc, _uvn, uvo, _displaced, scale, deltas = _scene(sfm)
    o = sr.outlier_scene(sfm)
    vp, kt = _Holder(), _Holder()
    vp.view_list, kt.track_list = [], []
    tp = sfm.processors.HipTriangulationProcessor(0.5, 30)
    tp.tri_pts = np.vstack((sc.pts_true, np.ones((1, sc.n_pts))))
    bp = sfm.processors.HipBaProcessor(vp, kt, None, tp, None, iteration=20, damping_factor=0.1)
    bp.ba_verbose = False
    for c in range(sc.n_cams):
        sel = sc.cam_idx == c
        q = sc.cams_init[c, 3:7] / np.linalg.norm(sc.cams_init[c, 3:7])
        pix = o.uv_pix[:, sel]
        vp.view_list.append(_View(sfm.geometry.quaternion_to_rotation(q), sc.cams_init[c, 0:3].reshape(3, 1).copy(), sc.intrinsic.copy(),
                                  [_KP(-1.0, -1.0)] + [_KP(x, y) for x, y in pix.T]))
        track = _Holder()
        track.table = np.full((sc.n_cams, pix.shape[1] + 1), -1, dtype=int)
        track.table[c, 1:] = sc.pt_idx[sel]
        kt.track_list.append(track)
    cams0 = np.stack([sfm.geometry.pack_camera(v.rot, v.loc) for v in vp.view_list])
    try:
        bp.ba_loss = ("huber", 5.0)
        cost, status = bp.refine_motion(views=[1, 4])
        assert bp._hip_scene.prob.loss() == (hip.LOSS_HUBER, 5.0 / scale)
        mask = np.zeros(sc.n_cams, dtype=np.uint8)
        mask[[1, 4]] = 1
        want_c, want_cost, want_st = mr.refine_cameras(cams0, sc.pts_true, sc.cam_idx, sc.pt_idx, uvo, 0.1, 20, rr.LOSS_HUBER,
                                                       deltas[rr.LOSS_HUBER], mask=mask)
        got = np.stack([sfm.geometry.pack_camera(v.rot, v.loc) for v in vp.view_list])
        assert rel(got, want_c) < 1e-9 and rel(cost, want_cost) < 1e-9 and np.array_equal(status, want_st)
        assert same_bits(tp.tri_pts[0:3], sc.pts_true)
        up = bp.ba_upload_bytes
        cost2, status2 = bp.refine_motion(iters=1)                     # the views are as written back and there is no mask: no upload
        assert bp.ba_last_action == "reuse" and bp.ba_upload_bytes == up
        want_c, want_cost, want_st = mr.refine_cameras(got, sc.pts_true, sc.cam_idx, sc.pt_idx, uvo, 0.1, 1, rr.LOSS_HUBER,
                                                       deltas[rr.LOSS_HUBER])
        got = np.stack([sfm.geometry.pack_camera(v.rot, v.loc) for v in vp.view_list])
        assert rel(got, want_c) < 1e-9 and rel(cost2, want_cost) < 1e-9 and np.array_equal(status2, want_st)
    finally:
        bp.ba_release()
