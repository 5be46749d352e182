"""Covariance of the resident scene (sfm_ba_covariance) against route A of tests/_cov_reference.py.

Norm: per block (a camera's 7x7, a point's 3x3), the largest absolute difference over the largest absolute entry of the
reference block (``cr.block_rel``).  Tolerance: ``cr.tolerance`` of the disagreement between the reference's own two float64
routes on the same scene and setting -- max(1e-9, 100 x that) -- measured here again, not copied: at lambda = 0 with two
cameras held cond(H) is ~1e9 and the routes differ by 1e-11 on camera blocks, so a fixed 1e-9 would leave a margin of 30.
A block that is zero in the reference (a held camera, an unobserved point) has to be zero bit for bit."""
import ctypes

import numpy as np
import pytest

import _cov_reference as cr
import _robust_reference as rr

pytestmark = pytest.mark.gpu

_CACHE = {}
GROUPS = (0, 1, 4, 8, 16, 32, 64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check(out, want, ab, where):
    cam_ab, pt_ab, _s = ab
    e_cam, e_pt = cr.block_rel(out.cam_cov, want[0]), cr.block_rel(out.pt_cov, want[1])
    e_s = abs(out.sigma0_sq - want[2]) / want[2] if want[2] else abs(out.sigma0_sq)
    print(where, "cameras %.2e (A-B %.2e)  points %.2e (A-B %.2e)  sigma0^2 %.1e" % (e_cam, cam_ab, e_pt, pt_ab, e_s))
    assert out.pivot_camera is None, where
    assert e_cam <= cr.tolerance(cam_ab) and e_pt <= cr.tolerance(pt_ab), where
    assert e_s < 1e-11, where                      # a sum of M terms in another order, over an integer


# ---- parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["none", "huber_unused", "huber"])
@pytest.mark.parametrize("name", cr.SCENES)
def test_parity(hip, sfm, oracle, name, loss):
    sc, uvn, cams, pts, scale = cr.scene(sfm, oracle, name)
    delta = 5.0 / scale
    kind = rr.LOSS_HUBER if loss == "huber" else rr.LOSS_NONE
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        if loss != "none":
            prob.set_loss(hip.LOSS_HUBER, delta)
        prob.set_state(cams, pts)
        for quirks in (oracle.QUIRKS_REFERENCE, 0):
            for lam, held in cr.settings(name):
                mask = cr.free_mask(sc.n_cams, held)
                ab, want = cr.ab_disagreement((name, quirks, kind, lam, held), cams, pts, sc.cam_idx, sc.pt_idx, uvn, lam, mask,
                                              kind, delta, quirks)
                out = prob.covariance(lam, quirks, loss == "huber", mask)
                _check(out, want, ab, (name, loss, quirks, lam, held))
                assert not out.cam_cov[list(held)].any() and np.all(out.cam_status[list(held)] == hip.COV_CAM_HELD)
                free = np.setdiff1d(np.arange(sc.n_cams), held)
                assert not out.cam_status[free].any() and not out.pt_status.any()
                assert np.all(out.cam_cov[free][:, np.arange(7), np.arange(7)] > 0) and np.all(out.pt_cov[:, [0, 3, 5]] > 0)
        got_state = prob.get_state()
    assert same_bits(got_state[0], cams) and same_bits(got_state[1], pts)


@pytest.mark.parametrize("loss", ["none", "huber"])
def test_single_observations_undamped(hip, sfm, oracle, loss):
    """lambda = 0 with points of one observation: D_p has rank 2, the point is reported, gets zeros, and its observation
    leaves S altogether -- the limit lambda -> 0 (tests/test_cov_host.py).  Reference: route A on the scene without those
    points; sigma0^2 by the formula on the full scene's cost and counts."""
    sc, uvn, cams, pts, scale = cr.scene(sfm, oracle, "single")
    delta = 5.0 / scale
    kind = rr.LOSS_HUBER if loss == "huber" else rr.LOSS_NONE
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        if loss != "none":
            prob.set_loss(hip.LOSS_HUBER, delta)
        prob.set_state(cams, pts)
        for quirks in (oracle.QUIRKS_REFERENCE, 0):
            ab, cam_cov, pt_cov, s0, single = cr.single_undamped(sfm, oracle, quirks, kind, delta, (0, 1))
            out = prob.covariance(0.0, quirks, loss == "huber", cr.free_mask(sc.n_cams, (0, 1)))
            _check(out, (cam_cov, pt_cov, s0), ab + (0.0,), ("single", loss, quirks, 0.0, (0, 1)))
            assert np.array_equal(out.pt_status, np.where(single, hip.COV_PT_SINGULAR, 0)) and not out.pt_cov[single].any()


def test_empty_camera_block_is_one_over_lambda(hip, sfm, oracle):
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "empty")
    assert np.bincount(sc.cam_idx, minlength=sc.n_cams)[4] == 0
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(cams, pts)
        out = prob.covariance(1e-3, mask=cr.free_mask(sc.n_cams, (0, 1)))
    assert np.max(np.abs(out.cam_cov[4] - np.eye(7) / 1e-3)) <= 1e-12 / 1e-3


# ---- boundaries ---------------------------------------------------------------------------------------------------
TRACK_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 70)      # 65 and 70: one workgroup per point
PER_LENGTH = 5


def _built_scene(seen, seed):
    """Cameras near the origin looking down +z at a cloud at depth 4 .. 8; ``seen`` (points, cameras) bool.  Returns
    (pt_ptr, cam_idx, pt_idx, uv, cams, pts): the cameras are a perturbation of those the keys were projected with."""
    rng = np.random.default_rng(seed)
    n, v = seen.shape
    pts = np.vstack((rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(4, 8, n)))
    pt_idx, cam_idx = (a.astype(np.int32) for a in np.nonzero(seen))
    pt_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(seen.sum(axis=1), out=pt_ptr[1:])
    true = np.hstack((rng.uniform(-0.5, 0.5, (v, 3)), np.ones((v, 1)), rng.uniform(-0.05, 0.05, (v, 3))))
    true[:, 3:7] /= np.linalg.norm(true[:, 3:7], axis=1)[:, None]
    cams = true + np.hstack((rng.uniform(-0.02, 0.02, (v, 3)), np.zeros((v, 1)), rng.uniform(-0.005, 0.005, (v, 3))))
    cams[:, 3:7] /= np.linalg.norm(cams[:, 3:7], axis=1)[:, None]
    r = rr._oracle().obs_terms_vec(true, pts, cam_idx, pt_idx, np.zeros((2, cam_idx.shape[0])))[0]
    uv = np.ascontiguousarray(-r.T + rng.normal(0, 1e-3, (2, cam_idx.shape[0])))
    return pt_ptr, cam_idx, pt_idx, uv, cams, pts


def _track_scene():
    """A hub of 70 cameras: PER_LENGTH points of every length in TRACK_LENGTHS, a point of length L seen by cameras 0 .. L-1."""
    if "tracks" not in _CACHE:
        deg = np.repeat(sorted(TRACK_LENGTHS, reverse=True), PER_LENGTH)
        seen = deg[:, None] > np.arange(max(TRACK_LENGTHS))[None, :]
        _CACHE["tracks"] = (deg, _built_scene(seen, 300))
    return _CACHE["tracks"]


def test_track_length_boundaries_and_group_independence(hip):
    """Every track length at which the point kernel changes its work split, on one scene; lambda = 1e-3 (a point with one
    observation has a singular D without damping), the quirk-free Jacobian as the other built scenes use.  Then the
    same call with every group width: not a bit of any point may change."""
    deg, (pt_ptr, cam_idx, pt_idx, uv, cams, pts) = _track_scene()
    v = cams.shape[0]
    assert hip.covariance_plan(v)[3] == 64 and np.array_equal(np.diff(pt_ptr), deg)
    mask = cr.free_mask(v, (0, 1))
    ab, want = cr.ab_disagreement(("tracks",), cams, pts, cam_idx, pt_idx, uv, 1e-3, mask, rr.LOSS_NONE, 1.0, 0)
    with hip.BaProblem(v, pt_ptr, cam_idx, uv) as prob:
        prob.set_state(cams, pts)
        assert prob.info(hip.INFO_MAX_TRACK) == 70
        outs = [prob.covariance(1e-3, 0, False, mask, group) for group in GROUPS]
        undamped = prob.covariance(0.0, 0, False, mask)
    _check(outs[0], want, ab, "track lengths")
    per_length = {int(l): cr.block_rel(outs[0].pt_cov[deg == l], want[1][deg == l]) for l in TRACK_LENGTHS}
    print(per_length)
    assert not outs[0].pt_status.any()
    for group, out in zip(GROUPS[1:], outs[1:]):
        assert same_bits(out.pt_cov, outs[0].pt_cov) and same_bits(out.cam_cov, outs[0].cam_cov), group
    # without damping the points with one observation are reported, come out as zeros and every other point still has a result
    assert undamped.pivot_camera is None
    assert np.array_equal(undamped.pt_status != 0, deg == 1) and np.all(undamped.pt_status[deg == 1] == hip.COV_PT_SINGULAR)
    assert not undamped.pt_cov[deg == 1].any() and np.all(undamped.pt_cov[deg > 1][:, [0, 3, 5]] > 0)
    assert np.all(np.isfinite(undamped.pt_cov)) and np.all(np.isfinite(undamped.cam_cov))


@pytest.mark.parametrize("v", [2, 3, 4, 5, 9, 10, 18, 19, 37, 260])
def test_camera_count_boundaries(hip, v):
    """7 V on both sides of the inverse's block size (64: 9 | 10 cameras), of two blocks (18 | 19), several blocks (37) and
    beyond what the iterations' data-flow solve takes (237 cameras); V = 2 with both held has no system at all.  40 points
    seen by every camera: at V = 260 their tracks also make a thread of the block path take more than one row."""
    if ("cams", v) not in _CACHE:
        _CACHE[("cams", v)] = _built_scene(np.ones((40, v), dtype=bool), 400 + v)
    pt_ptr, cam_idx, pt_idx, uv, cams, pts = _CACHE[("cams", v)]
    block, blocks, _launches, _g = hip.covariance_plan(v)
    assert blocks == -(-7 * v // block)
    mask = cr.free_mask(v, (0, 1))
    with hip.BaProblem(v, pt_ptr, cam_idx, uv) as prob:
        prob.set_state(cams, pts)
        for lam in (0.0, 1e-3):
            ab, want = cr.ab_disagreement(("cams", v, lam), cams, pts, cam_idx, pt_idx, uv, lam, mask, rr.LOSS_NONE, 1.0, 0)
            out = prob.covariance(lam, 0, False, mask)
            _check(out, want, ab, ("V", v, lam))
            assert not out.cam_cov[0:2].any()
            if v == 2:                                     # every camera held: D^-1, to the parity tolerance
                dinv = rr.reduced_system(cams, pts, cam_idx, pt_idx, uv, lam, rr.LOSS_NONE, 1.0, 0)["D_inv"][:, cr.PACK[0], cr.PACK[1]]
                assert cr.block_rel(out.pt_cov, dinv) <= 1e-9


# ---- exact properties ---------------------------------------------------------------------------------------------
def test_points_of_held_cameras_get_d_inverse(hip, sfm, oracle):
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "12x200_tracks")
    held = (0, 1, 2)
    seen_by = [set(sc.cam_idx[sc.pt_ptr[p]:sc.pt_ptr[p + 1]].tolist()) for p in range(sc.n_pts)]
    only_held = np.array([s <= set(held) for s in seen_by])
    assert 0 < only_held.sum() < sc.n_pts
    dinv = oracle.ba_reduced_system(cams, pts, sc.cam_idx, sc.pt_idx, uvn, 0.0)["D_inv"][:, cr.PACK[0], cr.PACK[1]]
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(cams, pts)
        out = prob.covariance(0.0, mask=cr.free_mask(sc.n_cams, held))
        all_held = prob.covariance(0.0, mask=np.zeros(sc.n_cams))
    assert cr.block_rel(out.pt_cov[only_held], dinv[only_held]) <= 1e-9
    assert np.all((out.pt_cov - dinv)[~only_held][:, [0, 3, 5]] > 0)
    assert not all_held.cam_cov.any() and np.all(all_held.cam_status == hip.COV_CAM_HELD)
    assert cr.block_rel(all_held.pt_cov, dinv) <= 1e-9
    assert same_bits(all_held.pt_cov[only_held], out.pt_cov[only_held])      # exactly D^-1: the sum adds zeros


def test_bits_repeat_and_survive_an_append(hip, sfm, oracle):
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "12x200_tracks")
    mask = cr.free_mask(sc.n_cams, (0, 1))
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(cams, pts)
        up = prob.upload_bytes
        first = prob.covariance(0.0, mask=mask)
        assert prob.upload_bytes - up == sc.n_cams                       # the mask alone
        second = prob.covariance(0.0, mask=mask)
        assert prob.upload_bytes - up == 2 * sc.n_cams
    assert same_bits(first.cam_cov, second.cam_cov) and same_bits(first.pt_cov, second.pt_cov) and first.sigma0_sq == second.sigma0_sq
    # the same scene grown on the device: points 120 .. and their observations appended to the first 120
    n0 = 120
    m0 = int(sc.pt_ptr[n0])
    with hip.BaProblem(sc.n_cams, sc.pt_ptr[:n0 + 1], sc.cam_idx[:m0], np.ascontiguousarray(uvn[:, :m0])) as prob:
        prob.set_state(cams, pts[:, :n0])
        prob.append(np.zeros((0, 7)), pts[:, n0:], sc.cam_idx[m0:], sc.pt_idx[m0:], uvn[:, m0:])
        grown = prob.covariance(0.0, mask=mask)
    assert same_bits(grown.cam_cov, first.cam_cov) and same_bits(grown.pt_cov, first.pt_cov) and grown.sigma0_sq == first.sigma0_sq


@pytest.mark.parametrize("graph", [0, 1])
def test_iterations_do_not_notice_the_call(hip, sfm, oracle, graph):
    """iterate, covariance, iterate ends in the bits of iterate, iterate under SFM_OPT_DETERMINISTIC; the cost history runs on."""
    sc, uvn, _cams, _pts, scale = cr.scene(sfm, oracle, "6x300")
    mask = cr.free_mask(sc.n_cams, (0, 1))
    ends = []
    for with_call in (False, True):
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_option(hip.OPT_DETERMINISTIC, 1)      # (the default iteration sums with atomics: two runs of it differ by themselves)
            prob.set_option(hip.OPT_GRAPH, graph)
            prob.set_loss(hip.LOSS_HUBER, 5.0 / scale)
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(0.5, 3)
            if with_call:
                out = prob.covariance(1e-3, use_loss=True, mask=mask)
                assert out.pivot_camera is None
                out = prob.covariance(0.0, 0, mask=None)           # the failing path leaves as little behind (quirk-free: the gauge is exact)
                assert out.pivot_camera is not None
            prob.iterate(0.5, 3)
            ends.append(prob.get_state() + (prob.get_stats(),))
    assert ends[0][2].shape == (6,)
    assert all(same_bits(a, b) for a, b in zip(ends[0], ends[1]))


# ---- failure paths ------------------------------------------------------------------------------------------------
def test_singular_system_is_a_status(hip, sfm, oracle):
    """Nothing held and no damping: the gauge is free, the factorisation meets a pivot that is not positive, the call says
    so and names a camera; the caller's arrays are untouched."""
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "6x300")
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(cams, pts)
        for held in ((), (0,)):
            mask = cr.free_mask(sc.n_cams, held)
            out = prob.covariance(0.0, 0, mask=mask)       # (quirk-free: with Q2 the v-row of J_C is not a derivative and the scale is not exactly free)
            assert out.pivot_camera is not None and 0 <= out.pivot_camera < sc.n_cams and out.pivot_camera not in held
            assert out.cam_cov is None and out.pt_cov is None and np.isnan(out.sigma0_sq)
            assert np.count_nonzero(out.cam_status & hip.COV_CAM_PIVOT) == 1
        cam_cov, pt_cov = np.full((sc.n_cams, 49), 7.0), np.full((sc.n_pts, 6), 7.0)
        pt_status, s0 = np.full(sc.n_pts, 7, dtype=np.int32), ctypes.c_double(7.0)
        st = prob._lib.sfm_ba_covariance(prob._h, 0.0, 0, 0, None, 0, hip.dptr(cam_cov), hip.dptr(pt_cov), None, hip.iptr(pt_status),
                                         ctypes.byref(s0))
        assert st == hip.E_SINGULAR and "positive definite" in hip.last_error()
        assert np.all(cam_cov == 7.0) and np.all(pt_cov == 7.0) and np.all(pt_status == 7) and s0.value == 7.0
        good = prob.covariance(0.0, 0, mask=cr.free_mask(sc.n_cams, (0, 1)))      # the problem is as usable as before
        assert good.pivot_camera is None and np.all(np.isfinite(good.cam_cov))
    # an empty camera that is not held has a zero block: the first pivot that fails is its own
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "empty")
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(cams, pts)
        assert prob.covariance(0.0, mask=cr.free_mask(sc.n_cams, (0, 1))).pivot_camera == 4


def test_refused_arguments(hip, sfm, oracle):
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "6x300")
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(cams, pts)
        for lam in (float("nan"), -1e-3):
            with pytest.raises(ValueError, match="lambda"):
                prob.covariance(lam)
        with pytest.raises(ValueError, match="group"):
            prob.covariance(1e-3, group=2)
        with pytest.raises(ValueError, match="mask"):
            prob.covariance(1e-3, mask=np.ones(sc.n_cams + 1))
        assert prob._lib.sfm_ba_covariance(prob._h, 1e-3, 3, 2, None, 0, None, None, None, None, None) == hip.E_SHAPE
        assert prob._lib.sfm_ba_covariance(prob._h, 1e-3, 3, 0, None, 2, None, None, None, None, None) == hip.E_SHAPE
        comm = hip.Comm(1, 0, hip.comm_unique_id())
        try:
            prob.set_comm(comm)
            with pytest.raises(ValueError, match="communicator"):
                prob.covariance(1e-3)
            prob.set_comm(None)
        finally:
            comm.close()
        assert prob.covariance(1e-3).pivot_camera is None
    # no points at all: nothing to invert but lambda I
    with hip.BaProblem(3, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((2, 0))) as prob:
        prob.set_state(cams[0:3], np.zeros((3, 0)))
        out = prob.covariance(0.5, mask=cr.free_mask(3, (0,)))
        assert not out.cam_cov[0].any() and np.array_equal(out.cam_cov[1], 2.0 * np.eye(7)) and out.sigma0_sq == 0.0
        assert prob.covariance(0.0, mask=cr.free_mask(3, (0,))).pivot_camera == 1


# ---- the Python layer ---------------------------------------------------------------------------------------------
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


def test_structure_uncertainty(hip, sfm, oracle):
    """HipBaMixin.structure_uncertainty on the host-track harness of the incremental tests: sigma0 sqrt(trace) of the
    centre and point blocks of route A at the adjusted state, the first two views held; the scene is not touched."""
    sc, uvn, _cams, _pts, _scale = cr.scene(sfm, oracle, "6x300")
    vp, kt = _Holder(), _Holder()
    vp.view_list, kt.track_list = [], []
    tp = sfm.processors.HipTriangulationProcessor(0.5, 30)
    tp.tri_pts = np.vstack((sc.pts_init, np.ones((1, sc.n_pts))))
    bp = sfm.processors.HipBaProcessor(vp, kt, None, tp, None, iteration=5, damping_factor=0.5)
    bp.ba_verbose = False
    for c in range(sc.n_cams):
        sel = sc.cam_idx == c
        q = sc.cams_init[c, 3:7] / np.linalg.norm(sc.cams_init[c, 3:7])
        keys = [_KP(-1.0, -1.0)] + [_KP(x, y) for x, y in sc.uv_pix[:, sel].T]
        vp.view_list.append(_View(sfm.geometry.quaternion_to_rotation(q), sc.cams_init[c, 0:3].reshape(3, 1).copy(), sc.intrinsic.copy(), keys))
        track = _Holder()
        track.table = np.full((sc.n_cams, len(keys)), -1, dtype=int)
        track.table[c, 1:] = sc.pt_idx[sel]
        kt.track_list.append(track)
    try:
        bp.execute_bundle_adjustment()
        cams = np.stack([sfm.geometry.pack_camera(v.rot, v.loc) for v in vp.view_list])
        pts = tp.tri_pts[0:3].copy()
        up = bp.ba_upload_bytes
        rep = bp.structure_uncertainty()
        assert bp.ba_last_action == "reuse" and bp.ba_upload_bytes - up == sc.n_cams
        raw = bp.structure_uncertainty(scaled=False)
        with pytest.raises(ValueError, match="singular"):
            bp.structure_uncertainty(hold=())
    finally:
        bp.ba_release()
    assert same_bits(tp.tri_pts[0:3], pts)
    cam_cov, pt_cov, s0 = cr.route_a(cams, pts, sc.cam_idx, sc.pt_idx, uvn, 0.0, cr.free_mask(sc.n_cams, (0, 1)), quirks=bp.ba_quirk_flags)
    want_cam = np.sqrt(s0 * (cam_cov[:, 0, 0] + cam_cov[:, 1, 1] + cam_cov[:, 2, 2]))
    want_pt = np.sqrt(s0 * (pt_cov[:, 0] + pt_cov[:, 3] + pt_cov[:, 5]))
    print(rep.sigma0, float(np.max(np.abs(rep.cam_sigma - want_cam)) / want_cam.max()), float(np.max(np.abs(rep.pt_sigma / want_pt - 1))))
    # the cameras went through rot -> q once more on the way back from the views: 1e-7 leaves that round trip room, and
    # is three orders below anything a wrong block, a missing sigma0 or a wrong gauge would give
    assert abs(rep.sigma0 - np.sqrt(s0)) < 1e-7 * np.sqrt(s0)
    assert not rep.cam_sigma[0:2].any() and np.max(np.abs(rep.cam_sigma - want_cam)) < 1e-7 * want_cam.max()
    assert np.max(np.abs(rep.pt_sigma / want_pt - 1)) < 1e-7
    assert np.max(np.abs(raw.pt_sigma * rep.sigma0 / rep.pt_sigma - 1)) < 1e-12
