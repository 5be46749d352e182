"""GPU tests of the two operations that move a resident scene: ``BaProblem.transform`` (sfm_ba_transform) against
``geometry.apply_similarity``, and ``BaProblem.align`` (sfm_ba_align) against ``similarity_ransac`` on the downloaded points and
the NumPy reference of tests/_similarity_reference.py; then the mixin forms ``HipBaMixin.align_structure`` and
``HipCamposeMixin.register_pair_points``.  The scene is 6 cameras x 120 points of ``scenes.make_scene``; its alignment case is
settled in the reference (tests/test_similarity_host.py)."""
import numpy as np
import pytest

import _similarity_reference as sr
import _twoview_pose_reference as tp
from _twoview_checks import same_bits

pytestmark = pytest.mark.gpu

MAX_PX = 2.0                          # the pixel threshold the relative-pose tests judge a pair at


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def start_state(sfm, sc):
    cams = sc.cams_init.copy()
    cams[:, 3:7] /= np.linalg.norm(cams[:, 3:7], axis=1, keepdims=True)
    cams[cams[:, 3] < 0, 3:7] *= -1.0
    return cams, sc.pts_init.copy()


def resident(hip, sfm, sc):
    prob = hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic))
    prob.set_state(*start_state(sfm, sc))
    return prob


def the_similarity():
    return hip_split(sr.align_sim())


def hip_split(sim):
    sim = np.asarray(sim, dtype=np.float64)
    return float(sim[0]), sim[1:10].reshape(3, 3).copy(), sim[10:13].copy()


# ---- transform ------------------------------------------------------------------------------------------------------------
def test_transform_is_apply_similarity_and_keeps_the_cost(hip, sfm):
    sc = sr.align_case(sfm.scenes)[0]
    s, A, t = the_similarity()
    with resident(hip, sfm, sc) as prob:
        cams0, pts0 = prob.get_state()
        cost0 = prob.cost()
        prob.transform(s, A, t)
        cams1, pts1 = prob.get_state()
        want_cams, want_pts = sfm.geometry.apply_similarity((s, A, t), cams0, pts0)
        print("state against apply_similarity: cams %.3e pts %.3e" % (rel(cams1, want_cams), rel(pts1, want_pts)))
        assert rel(cams1, want_cams) <= 1e-12 and rel(pts1, want_pts) <= 1e-12 and np.all(cams1[:, 3] >= 0)
        cost1 = prob.cost()
        print("cost before %.17g after %.17g" % (cost0, cost1))
        assert cost0 > 0 and abs(cost1 - cost0) <= 1e-9 * cost0
        # the inverse brings the state back
        prob.transform(1.0 / s, A.T, -(A.T @ t) / s)
        cams2, pts2 = prob.get_state()
        print("after the inverse: cams %.3e pts %.3e" % (rel(cams2, cams0), rel(pts2, pts0)))
        assert rel(cams2, cams0) <= 1e-12 and rel(pts2, pts0) <= 1e-12


def test_transform_then_iterate_is_set_state_then_iterate(hip, sfm):
    sc = sr.align_case(sfm.scenes)[0]
    s, A, t = the_similarity()
    with resident(hip, sfm, sc) as prob, resident(hip, sfm, sc) as other:
        prob.transform(s, A, t)
        prob.iterate(0.5, 3)
        assert prob.get_stats().shape[0] == 3                  # a moved scene starts a new cost history
        other.set_state(*sfm.geometry.apply_similarity((s, A, t), *other.get_state()))
        other.iterate(0.5, 3)
        got, want = prob.get_state(), other.get_state()
        print("after three iterations: cams %.3e pts %.3e" % (rel(got[0], want[0]), rel(got[1], want[1])))
        assert rel(got[0], want[0]) <= 1e-9 and rel(got[1], want[1]) <= 1e-9


def test_transform_refuses_a_half_turn_and_bad_arguments(hip, sfm):
    sc = sr.align_case(sfm.scenes)[0]
    g = sfm.geometry
    with resident(hip, sfm, sc) as prob:
        before = prob.get_state()
        c = 3
        half = np.diag([1.0, -1.0, -1.0]) @ g.quaternion_to_rotation_unchecked(before[0][c, 3:7]).T      # A R(q_c) = R_pi
        assert g.is_rotation(half)
        with pytest.raises(ValueError, match="camera %d " % c):
            prob.transform(1.5, half, [1.0, 2.0, 3.0])
        assert all(same_bits(a, b) for a, b in zip(prob.get_state(), before))
        for s in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="s = "):
                prob.transform(s, np.eye(3), np.zeros(3))
        for A in (2.0 * np.eye(3), np.diag([1.0, 1.0, -1.0]) * 1.0001, np.array([[1.0, -0.1, 0], [0, 1.0, 0], [0, 0, 1.0]])):
            with pytest.raises(ValueError):
                prob.transform(1.0, A, np.zeros(3))
        with pytest.raises(ValueError):
            prob.transform(1.0, np.eye(3), [0.0, float("nan"), 0.0])
        assert all(same_bits(a, b) for a, b in zip(prob.get_state(), before))
        comm = hip.Comm(1, 0, hip.comm_unique_id())
        try:
            prob.set_comm(comm)
            with pytest.raises(ValueError, match="communicator"):
                prob.transform(1.0, np.eye(3), np.zeros(3))
            prob.set_comm(None)
        finally:
            comm.close()


# ---- align ----------------------------------------------------------------------------------------------------------------
def test_align_without_apply_is_similarity_ransac_on_the_downloaded_points(hip, sfm):
    sc, idx, targets, bad = sr.align_case(sfm.scenes)
    with resident(hip, sfm, sc) as prob:
        before = prob.get_state()
        src = np.ascontiguousarray(before[1][:, idx])
        for rigid in (False, True):
            sim, inlier, n_in, best, status = prob.align(idx, targets, sr.MAX_ERR2, 128, 2, rigid, apply=False)
            want = hip.similarity_ransac([0, idx.size], src, targets, sr.MAX_ERR2, 128, 2, rigid)
            assert same_bits(sim, want[0][0]) and same_bits(inlier, want[1])
            assert (n_in, best, status) == (want[2][0], want[3][0], want[4][0])
            ref = sr.reference([0, idx.size], src, targets, sr.MAX_ERR2, 128, 2, rigid)
            assert ref.settled.all() and status == ref.status[0] and best == ref.best_hyp[0] and np.array_equal(inlier, ref.inlier)
            assert sr.sim_difference(sim, ref.sim[0], ref.ext[0]) <= max(1e-9, 100.0 * ref.d_S[0])
            assert all(same_bits(a, b) for a, b in zip(prob.get_state(), before))


def test_align_moves_the_scene_onto_its_targets(hip, sfm):
    sc, idx, targets, bad = sr.align_case(sfm.scenes)
    with resident(hip, sfm, sc) as prob:
        cams0, pts0 = prob.get_state()
        cost0 = prob.cost()
        ref = sr.reference([0, idx.size], np.ascontiguousarray(pts0[:, idx]), targets, sr.MAX_ERR2, 128, 2)
        sim, inlier, n_in, best, status = prob.align(idx, targets, sr.MAX_ERR2)
        assert status == 0 and n_in == 80 and np.array_equal(inlier.astype(bool), ~bad)
        assert abs(sim[0] - ref.sim[0][0]) / ref.sim[0][0] <= max(1e-9, 100.0 * ref.d_S[0])
        cams1, pts1 = prob.get_state()
        dist = np.linalg.norm(pts1[:, idx] - targets, axis=0)
        print("largest distance of an inlier from its target %.4f, of a wrong one %.4f" % (dist[~bad].max(), dist[bad].min()))
        assert np.all(dist[inlier.astype(bool)] <= np.sqrt(sr.MAX_ERR2) * (1 + 1e-9)) and np.all(dist[bad] > 0.5)
        want_cams, want_pts = sfm.geometry.apply_similarity(sim, cams0, pts0)
        assert rel(cams1, want_cams) <= 1e-12 and rel(pts1, want_pts) <= 1e-12
        assert abs(prob.cost() - cost0) <= 1e-9 * cost0


def test_align_with_too_few_or_bad_arguments_leaves_the_scene(hip, sfm):
    sc, idx, targets, bad = sr.align_case(sfm.scenes)
    with resident(hip, sfm, sc) as prob:
        before = prob.get_state()
        sim, inlier, n_in, best, status = prob.align(idx[:3], targets[:, :3], sr.MAX_ERR2)
        assert status == hip.SIMILARITY_TOO_FEW and not sim.any() and not inlier.any() and (n_in, best) == (0, -1)
        sim, inlier, n_in, best, status = prob.align(np.zeros(0, dtype=np.int32), np.zeros((3, 0)), sr.MAX_ERR2)
        assert status == hip.SIMILARITY_TOO_FEW and not sim.any() and inlier.size == 0 and (n_in, best) == (0, -1)
        # targets no similarity explains: no model
        far = np.random.default_rng(1).standard_normal((3, idx.size)) * 50.0
        sim, inlier, n_in, best, status = prob.align(idx, far, sr.MAX_ERR2)
        assert status == hip.SIMILARITY_NO_MODEL and not sim.any() and not inlier.any() and (n_in, best) == (0, -1)
        for bad_idx in (sc.n_pts, -1):
            wrong = idx.copy()
            wrong[7] = bad_idx
            with pytest.raises(ValueError, match="point_idx"):
                prob.align(wrong, targets, sr.MAX_ERR2)
        with pytest.raises(ValueError):
            prob.align(idx, targets[:, :5], sr.MAX_ERR2)
        with pytest.raises(ValueError):
            prob.align(idx, targets, -1.0)
        assert all(same_bits(a, b) for a, b in zip(prob.get_state(), before))
        comm = hip.Comm(1, 0, hip.comm_unique_id())
        try:
            prob.set_comm(comm)
            with pytest.raises(ValueError, match="communicator"):
                prob.align(idx, targets, sr.MAX_ERR2)
            prob.set_comm(None)
        finally:
            comm.close()
        assert all(same_bits(a, b) for a, b in zip(prob.get_state(), before))


# ---- the mixins -------------------------------------------------------------------------------------------------------------
def test_align_structure_writes_the_moved_scene_back(hip, sfm):
    from test_gpu_screen import _DropIn
    sc, idx, targets, bad = sr.align_case(sfm.scenes)
    run = _DropIn(sfm, sc, sc.uv_pix, 6)
    bp, tri = run.bp, run.tp
    try:
        cams0, pts0 = run.cams(), tri.tri_pts[0:3].copy()
        sim, inlier, n_in, best, status = bp.align_structure(idx, targets, 0.05, apply=False)
        assert bp.ba_last_action == "create" and status == 0 and n_in == 80
        assert same_bits(tri.tri_pts[0:3], pts0) and same_bits(run.cams(), cams0)
        moved = bp.align_structure(idx, targets, 0.05)
        assert bp.ba_last_action == "reuse" and same_bits(moved[0], sim) and same_bits(moved[1], inlier)
        want_cams, want_pts = sfm.geometry.apply_similarity(sim, cams0, pts0)
        assert rel(tri.tri_pts[0:3], want_pts) <= 1e-12 and rel(run.cams(), want_cams) <= 1e-11
        assert np.all(np.linalg.norm(tri.tri_pts[0:3][:, idx[~bad]] - targets[:, ~bad], axis=0) <= 0.05 * (1 + 1e-9))
        up = bp.ba_upload_bytes
        bp.screen_structure()                                  # the host picture is the device's: nothing goes up again but cam_scale
        assert bp.ba_last_action == "reuse" and bp.ba_upload_bytes - up == 8 * 6
        with pytest.raises(ValueError):
            bp.align_structure(idx, targets, -1.0)
    finally:
        bp.ba_release()


def test_register_pair_points_chains_a_pair_onto_a_scene(hip, sfm):
    P = sfm.processors
    cp = P.HipCamposeProcessor(None, 5, 25)
    sc, ref = tp.scene_and_reference("general_displaced")
    k = 2                                                      # the set of 300 matches
    lo, hi = sc.set_ptr[k], sc.set_ptr[k + 1]
    one = np.ones((1, hi - lo))
    pairs = [np.vstack((sc.left[:, lo:hi], one)), np.vstack((sc.right[:, lo:hi], one))]
    rot, centre, front, counts = cp.estimate_relative_pose_robust(pairs, sc.models[k], "fundamental", tp.K_LEFT, tp.K_RIGHT,
                                                                   np.flatnonzero(sc.mask[lo:hi]), tp.MIN_ANGLE_DEG, tp.MIN_PARALLAX)
    front = [i for i in front if sc.mask[lo + i]]              # the matches in front that are not displaced
    assert counts["status"] == 0 and len(front) > 200
    pair_pts = cp.pose_last["X"][:, front]                     # in the pair's frame: the left camera at the origin, |t| = 1
    # the scene holds the same tracks in its own frame, a tenth of them attached to the wrong point
    s0, A0, t0 = hip_split(sr.align_sim())
    rng = np.random.default_rng(9)
    scene_pts = s0 * (A0 @ pair_pts) + t0[:, None] + 1e-3 * rng.standard_normal(pair_pts.shape)
    wrong = np.zeros(len(front), dtype=bool)
    wrong[rng.permutation(len(front))[:len(front) // 10]] = True
    scene_pts[:, wrong] += rng.uniform(1.0, 4.5, (3, int(wrong.sum())))
    s, A, t, inlier, rot2, centre2 = cp.register_pair_points(scene_pts, pair_pts, rot, centre, max_err=0.02)
    assert abs(s - s0) < 1e-2 * s0 and np.abs(A - A0).max() < 1e-2 and t.shape == (3, 1) and centre2.shape == (3, 1)
    assert inlier == np.flatnonzero(~wrong).tolist() and cp.similarity_last["status"] in (0, hip.SIMILARITY_KEPT_HYPOTHESIS)
    # the returned camera sees the scene's points where the pair's right view saw them
    cam = rot2.T @ (scene_pts[:, inlier] - centre2)
    pix = (tp.K_RIGHT @ (cam / cam[2]))[0:2]
    err = np.linalg.norm(pix - sc.right[:, lo:hi][:, np.asarray(front)[inlier]], axis=0)
    print("reprojection of the chained pair: median %.3f px, worst %.3f px" % (np.median(err), err.max()))
    assert np.all(cam[2] > 0) and err.max() <= MAX_PX
    # ... and the pair's left camera is the similarity itself
    _s, _A, _t, _inl, rot1, centre1 = cp.register_pair_points(scene_pts, pair_pts, max_err=0.02)
    assert same_bits(rot1, A) and same_bits(centre1, t)
    none = cp.register_pair_points(scene_pts[:, :3], pair_pts[:, :3], rot, centre)
    assert none[0] == 0.0 and none[3] == [] and cp.similarity_last["status"] == hip.SIMILARITY_TOO_FEW
