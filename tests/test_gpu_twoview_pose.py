"""Relative pose of a verified pair on the device (sfm_twoview_pose) against the NumPy rule of
tests/_twoview_pose_reference.py.  tests/test_twoview_pose_host.py shows on the CPU that every set of every scene used here is
settled, so the decisions -- status, winner, the four counts, n_front, n_parallax, every byte of obs_front, the summary -- are
compared exactly and no set is left out; R, t and the normal agree within max(1e-9, 100 d_P), d_P the spread of the reference's
own routes, and X_out within the same bound relative to its norm where a match is in front, NaN elsewhere."""
import itertools

import numpy as np
import pytest

import _twoview_pose_reference as tp
from test_twoview_pose_host import _lib_status, bad_arguments

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(hip, sc, outputs=None, mask=True):
    kw = {} if outputs is None else {"outputs": outputs}
    return hip.twoview_pose(sc.set_ptr, sc.left, sc.right, sc.models, sc.kinds, tp.K_LEFT, tp.K_RIGHT, tp.COS2_MIN, tp.MIN_PARALLAX,
                            sc.mask if mask else None, **kw)


worst = {"pose": 0.0, "X": 0.0}


def compare(got, ref, sc, what):
    assert np.array_equal(got["status"], ref.status), (what, np.flatnonzero(got["status"] != ref.status))
    assert np.array_equal(got["best_cand"], ref.best), what
    assert np.array_equal(got["cand_front"], ref.cand_front), (what, np.flatnonzero((got["cand_front"] != ref.cand_front).any(axis=1)))
    assert np.array_equal(got["n_front"], ref.n_front) and np.array_equal(got["n_parallax"], ref.n_parallax), what
    assert np.array_equal(got["obs_front"], ref.obs), (what, np.flatnonzero(got["obs_front"] != ref.obs))
    assert np.array_equal(got["summary"], ref.summary), (what, got["summary"], ref.summary)
    assert np.array_equal(np.isnan(got["X"]).any(axis=0), ref.obs == 0) and np.array_equal(np.isnan(got["X"]).all(axis=0), ref.obs == 0), what
    for s in range(sc.counts.size):
        bound = max(1e-9, 100.0 * ref.d_P[s])
        d = max(np.abs(got["R"][s] - ref.R[s]).max(), np.abs(got["t"][s] - ref.t[s]).max(), np.abs(got["normal"][s] - ref.n[s]).max())
        worst["pose"] = max(worst["pose"], float(d))
        assert d <= bound, (what, s, d, bound)
        if ref.best[s] < 0:
            assert not got["R"][s].any() and not got["t"][s].any() and not got["normal"][s].any()
        lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
        front = ref.obs[lo:hi] > 0
        if front.any():
            gx, rx = got["X"][:, lo:hi][:, front], ref.X[:, lo:hi][:, front]
            dx = np.abs(gx - rx).max(axis=0) / np.linalg.norm(rx, axis=0)
            worst["X"] = max(worst["X"], float(dx.max()))
            assert np.all(dx <= bound), (what, s, float(dx.max()), bound)


# ---- parity on every scene ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tp.CASES)
def test_parity_with_the_reference(hip, name):
    sc, ref = tp.scene_and_reference(name)
    got = run(hip, sc)
    compare(got, ref, sc, name)
    print("%s: %d sets, %d matches, worst device difference so far: pose %.3e, X %.3e (relative)"
          % (name, sc.counts.size, sc.left.shape[1], worst["pose"], worst["X"]))


def test_no_mask_means_every_match(hip):
    sc = tp.scene(tp.NO_MASK_CASE)
    ref = tp.reference(sc.set_ptr, sc.left, sc.right, None, sc.models, sc.kinds)
    got = run(hip, sc, mask=False)
    compare(got, ref, sc, "no mask")
    assert got["summary"][5] > 0                              # the displaced matches vote now and are not in front


# ---- batch independence, determinism -------------------------------------------------------------------------------------
def _same_sets(hip, sc, whole, sets, what):
    sub = tp.subset(sc, sets)
    got = hip.twoview_pose(sub.set_ptr, sub.left, sub.right, sub.models, sub.kinds, tp.K_LEFT, tp.K_RIGHT, tp.COS2_MIN, tp.MIN_PARALLAX, sub.mask)
    for name in ("R", "t", "normal", "cand_front", "n_front", "n_parallax", "best_cand", "status"):
        assert same_bits(got[name], whole[name][sets]), (what, name)
    assert same_bits(got["obs_front"], whole["obs_front"][sub.cols]) and same_bits(got["X"], whole["X"][:, sub.cols]), what
    return got


def test_every_set_size_alone_and_in_the_batch(hip):
    sc, ref = tp.scene_and_reference("sizes")
    whole = run(hip, sc)
    for s in range(sc.counts.size):
        got = _same_sets(hip, sc, whole, [s], "alone %d" % sc.counts[s])
        assert got["summary"][0] + got["summary"][1] + got["summary"][2] == 1
    _same_sets(hip, sc, whole, np.random.default_rng(3).permutation(sc.counts.size).tolist(), "permuted")


def test_a_set_alone_and_inside_the_259(hip):
    sc = tp.scene("many")
    whole = run(hip, sc)
    for s in (0, 5, 64, 65, 127, 128, 255, 256, 257, 258):
        _same_sets(hip, sc, whole, [s], "set %d alone" % s)
    _same_sets(hip, sc, whole, list(range(1, 259, 2)), "every other set")


def test_two_calls_give_the_same_bits(hip):
    for name in ("sizes", "many"):
        sc = tp.scene(name)
        first, second = run(hip, sc), run(hip, sc)
        assert all(same_bits(first[k], second[k]) for k in first), name


# ---- the _dev form ------------------------------------------------------------------------------------------------------
def test_dev_form_on_a_callers_stream(hip):
    import torch
    sc = tp.scene("sizes")
    want = run(hip, sc)
    S, M = sc.counts.size, sc.left.shape[1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_left, d_right = torch.from_numpy(sc.left).cuda(), torch.from_numpy(sc.right).cuda()
        d_mask = torch.from_numpy(sc.mask.astype(np.uint8)).cuda()
        d = {"R": torch.full((S, 3, 3), 7.0, dtype=torch.float64, device="cuda"), "t": torch.full((S, 3), 7.0, dtype=torch.float64, device="cuda"),
             "normal": torch.full((S, 3), 7.0, dtype=torch.float64, device="cuda"),
             "cand_front": torch.full((S, 4), -5, dtype=torch.int32, device="cuda"),
             "obs_front": torch.full((M,), 9, dtype=torch.uint8, device="cuda"), "X": torch.full((3, M), 7.0, dtype=torch.float64, device="cuda"),
             "summary": torch.full((6,), -1, dtype=torch.int64, device="cuda")}
        for name in ("n_front", "n_parallax", "best_cand", "status"):
            d[name] = torch.full((S,), -5, dtype=torch.int32, device="cuda")
        stream.synchronize()
        hip.twoview_pose_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), sc.models, sc.kinds, tp.K_LEFT, tp.K_RIGHT, tp.COS2_MIN,
                             tp.MIN_PARALLAX, d_mask.data_ptr(), d["R"].data_ptr(), d["t"].data_ptr(), d["normal"].data_ptr(),
                             d["cand_front"].data_ptr(), d["n_front"].data_ptr(), d["n_parallax"].data_ptr(), d["best_cand"].data_ptr(),
                             d["status"].data_ptr(), d["obs_front"].data_ptr(), d["X"].data_ptr(), d["summary"].data_ptr(),
                             stream.cuda_stream)
        got = {k: v.cpu().numpy() for k, v in d.items()}
        assert same_bits(d_left.cpu().numpy(), sc.left) and same_bits(d_mask.cpu().numpy(), sc.mask.astype(np.uint8))
        # only the pose asked for: nothing else is needed
        R2, t2 = torch.zeros((S, 3, 3), dtype=torch.float64, device="cuda"), torch.zeros((S, 3), dtype=torch.float64, device="cuda")
        stream.synchronize()
        hip.twoview_pose_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), sc.models, sc.kinds, tp.K_LEFT, tp.K_RIGHT, tp.COS2_MIN,
                             tp.MIN_PARALLAX, d_mask.data_ptr(), R2.data_ptr(), t2.data_ptr(), stream=stream.cuda_stream)
        assert same_bits(R2.cpu().numpy(), got["R"]) and same_bits(t2.cpu().numpy(), got["t"])
    for name in want:
        assert same_bits(got[name], want[name]), name


# ---- every subset of the optional outputs -------------------------------------------------------------------------------
def test_every_subset_of_the_optional_outputs(hip):
    sc = tp.subset(tp.scene("sizes"), [1, 3, 5, 6])           # 1, 63, 65 and 1 023 matches, both kinds
    full = hip.twoview_pose(sc.set_ptr, sc.left, sc.right, sc.models, sc.kinds, tp.K_LEFT, tp.K_RIGHT, tp.COS2_MIN, tp.MIN_PARALLAX, sc.mask)
    names = hip.POSE_OUTPUTS
    for k in range(len(names) + 1):
        for subset in itertools.combinations(names, k):
            got = hip.twoview_pose(sc.set_ptr, sc.left, sc.right, sc.models, sc.kinds, tp.K_LEFT, tp.K_RIGHT, tp.COS2_MIN, tp.MIN_PARALLAX,
                                   sc.mask, outputs=subset)
            assert same_bits(got["R"], full["R"]) and same_bits(got["t"], full["t"]), subset
            for name in names:
                if name in subset:
                    assert same_bits(got[name], full[name]), (subset, name)
                else:
                    assert got[name] is None


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_shape_errors_come_from_the_library(hip):
    for args in bad_arguments():
        assert _lib_status(hip, **args) == hip.E_SHAPE, args
    empty = hip.twoview_pose([0], np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((0, 3, 3)), [], tp.K_LEFT, tp.K_RIGHT, tp.COS2_MIN)
    assert empty["R"].shape == (0, 3, 3) and not empty["summary"].any()


def test_the_options_are_the_callers(hip):
    sc = tp.scene(tp.OPTION_SCENE)
    for cos2, min_par in tp.OPTION_CASES:
        ref = tp.reference(sc.set_ptr, sc.left, sc.right, sc.mask, sc.models, sc.kinds, cos2_min=cos2, min_parallax=min_par)
        got = hip.twoview_pose(sc.set_ptr, sc.left, sc.right, sc.models, sc.kinds, tp.K_LEFT, tp.K_RIGHT, cos2, min_par, sc.mask)
        compare(got, ref, sc, (cos2, min_par))
        assert bool((got["status"] & hip.POSE_NO_PARALLAX).any()) == (min_par == 1000)


# ---- the Python entry points -------------------------------------------------------------------------------------------
def _pairs(sc, s):
    lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
    one = np.ones((1, hi - lo))
    return [np.vstack((sc.left[:, lo:hi], one)), np.vstack((sc.right[:, lo:hi], one))]


def test_estimate_relative_pose_robust(hip, sfm):
    P = sfm.processors
    cp = P.HipCamposeProcessor(None, 5, 25)
    for name, kind in (("general_displaced", "fundamental"), ("plane_displaced", "homography")):
        sc, ref = tp.scene_and_reference(name)
        for s in range(sc.counts.size):
            lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
            rot, centre, front, counts = cp.estimate_relative_pose_robust(_pairs(sc, s), sc.models[s], kind, tp.K_LEFT, tp.K_RIGHT,
                                                                          np.flatnonzero(sc.mask[lo:hi]), tp.MIN_ANGLE_DEG, tp.MIN_PARALLAX)
            want_rot, want_centre = tp.to_reference_convention(ref.R[s], ref.t[s])
            bound = max(1e-9, 100.0 * ref.d_P[s])
            assert np.abs(rot - want_rot).max() <= bound and np.abs(centre - want_centre).max() <= bound and centre.shape == (3, 1)
            assert front == np.flatnonzero(ref.obs[lo:hi]).tolist()
            assert (counts["n_front"], counts["n_parallax"], counts["best_cand"], counts["status"]) == \
                (ref.n_front[s], ref.n_parallax[s], ref.best[s], ref.status[s])
            assert np.array_equal(counts["cand_front"], ref.cand_front[s]) and cp.pose_last["X"].shape == (3, hi - lo)
            assert same_bits(cp.pose_last["R"].T @ -cp.pose_last["t"].reshape(3, 1), centre)
    with pytest.raises(ValueError):
        cp.estimate_relative_pose_robust(_pairs(sc, 0), sc.models[0], "homography", tp.K_LEFT, tp.K_RIGHT, min_angle_deg=-1.0)
    # a set without a pose: the identity at the origin, nothing in front
    rot, centre, front, counts = cp.estimate_relative_pose_robust(_pairs(sc, 0), np.zeros((3, 3)), "homography", tp.K_LEFT, tp.K_RIGHT)
    assert same_bits(rot, np.identity(3)) and not centre.any() and front == [] and counts["status"] == hip.POSE_NO_MODEL | hip.POSE_NO_POSE


def test_initialise_pairs_on_a_general_a_plane_and_a_hopeless_set(hip, sfm):
    P = sfm.processors
    K = tp.K_LEFT
    g = tp.family_part("general", 300, 11, 0.1, Kr=K)
    p = tp.family_part("plane", 300, 12, 0.1, Kr=K)
    rng = np.random.default_rng(5)
    hopeless = (rng.uniform(0, 640, (2, 4)), rng.uniform(0, 480, (2, 4)))
    sets = [[g[0], g[1]], [p[0], p[1]], [hopeless[0], hopeless[1]]]
    ep = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
    out = ep.initialise_pairs(sets, K)
    assert [o["verdict"] for o in out] == ["general", "degenerate", "none"]
    assert [o["kind"] for o in out] == ["fundamental", "homography", "fundamental"]
    for o, fam, part, inl in ((out[0], "general", g, "F_inliers"), (out[1], "plane", p, "H_inliers")):
        R0, t0 = tp.planted(fam)
        assert o["best_cand"] >= 0 and not o["status"] & (hip.POSE_NO_POSE | hip.POSE_NO_PARALLAX | hip.POSE_EMPTY | hip.POSE_NO_MODEL)
        assert set(o["front"]) <= set(o[inl]) and o["n_front"] == len(o["front"]) >= 0.95 * len(o[inl])
        assert not set(o["front"]) & set(np.flatnonzero(part[2]).tolist())            # no displaced match votes
        assert o["n_parallax"] >= 0.9 * o["n_front"]
        # the estimated model carries 0.3 px of noise on 270 matches, some 4e-4 rad each: the pose is the planted one well inside 3 degrees
        assert np.abs(o["R"] - R0).max() < 0.05 and o["t"] @ t0 > 0.95, (fam, np.abs(o["R"] - R0).max(), o["t"] @ t0)
        assert np.allclose(o["rot"], o["R"].T) and np.allclose(o["centre"][:, 0], -o["R"].T @ o["t"])
    assert abs(out[1]["normal"] @ tp.PLANE_N) > 0.95
    none = out[2]
    assert none["best_cand"] == -1 and none["status"] & hip.POSE_EMPTY and none["status"] & hip.POSE_NO_POSE and none["front"] == []
    assert same_bits(none["rot"], np.identity(3)) and not none["R"].any()
    assert ep.pose_last["summary"][0] == 2 and ep.pose_last["summary"][2] == 1
    # one call over the three sets is what the sets give alone
    for s in range(3):
        alone = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128)).initialise_pairs([sets[s]], K)[0]
        assert same_bits(alone["R"], out[s]["R"]) and same_bits(alone["t"], out[s]["t"]) and alone["front"] == out[s]["front"]


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def test_pose_pairs_against_the_host_form(hip, sfm):
    P = sfm.processors
    dv = sfm.scenes.make_descriptor_views(n_views=3, n_pts=200, seed=0)
    views = [View(dv.key_pts(v), dv.sift[v]) for v in range(3)]
    K = np.asarray(sfm.scenes.UPENN_K, dtype=np.float64)
    kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
    cp = P.HipCamposeProcessor(None, 5, 25)
    try:
        for v in range(3):
            kt.add_new_view(views[v], views[:v])
        for ref_idx, que_idx in ((0, 1), (0, 2), (1, 2)):
            pairs, r_idx, q_idx = kt.generate_matched_pairs(ref_idx, que_idx, views)
            n = r_idx.shape[1]
            _r, _q, mask = P.verify_pairs(kt, ref_idx, que_idx, 2.0, 128, 2)
            F = kt.twoview_last["fund_mat"]
            assert kt.twoview_last["hypothesis"] >= 0 and mask.sum() >= 0.5 * n
            for inlier in (mask, None):
                down = kt.kt_download_bytes
                got_r, got_q, rot, centre, front, counts = P.pose_pairs(kt, ref_idx, que_idx, F, "fundamental", K, K, inlier, 1.0, 8)
                assert kt.kt_download_bytes == down           # the store downloaded nothing on its own account
                want = cp.estimate_relative_pose_robust(pairs, F, "fundamental", K, K, None if inlier is None else np.flatnonzero(inlier), 1.0, 8)
                assert np.array_equal(got_r, r_idx) and np.array_equal(got_q, q_idx)
                assert same_bits(rot, want[0]) and same_bits(centre, want[1]) and front == want[2]
                for name in ("n_front", "n_parallax", "best_cand", "status"):
                    assert counts[name] == want[3][name], name
                assert same_bits(counts["cand_front"], want[3]["cand_front"])
                for name in ("R", "t", "normal", "obs_front", "X"):
                    assert same_bits(kt.pose_last[name], cp.pose_last[name]), name
                assert counts["best_cand"] >= 0 and (inlier is None or counts["n_front"] >= 0.9 * mask.sum())
        assert P.pose_pairs(kt, 0, 3, F, "fundamental", K, K) is None
    finally:
        kt.kt_release()


# ---- agreement with the existing chain ----------------------------------------------------------------------------------------
def test_the_in_front_set_is_the_one_the_existing_chain_returns(hip, sfm):
    """On a clean general scene the winner's in-front matches are those disambiguate_cam_pose_four returns for the same four
    candidates (index lists only: the chain triangulates by DLT, the vote by the midpoint of the two rays)."""
    P = sfm.processors
    l, r, displaced, F, kind = tp.family_part("general", 300, 21, 0.0, Kr=tp.K_LEFT)
    K = tp.K_LEFT
    cp, tri = P.HipCamposeProcessor(None, 5, 25), P.HipTriangulationProcessor()
    pairs = [np.vstack((l, np.ones((1, 300)))), np.vstack((r, np.ones((1, 300))))]
    out = hip.twoview_pose([0, 300], l, r, [F], [kind], K, K, tp.COS2_MIN, tp.MIN_PARALLAX, outputs=("obs_front", "best_cand", "cand_front"))
    assert out["best_cand"][0] >= 0
    # the same four candidates, in the convention of the chain
    ref = tp.reference([0, 300], l, r, None, [F], [kind], K, K)
    cands = [tp.to_reference_convention(ref.sets[0].cands.R[k], ref.sets[0].cands.t[k]) for k in range(4)]
    ref_proj = K @ np.hstack((np.eye(3), np.zeros((3, 1))))
    projs = [K @ np.hstack((rot.T, -rot.T @ c)) for rot, c in cands]
    pts = [tri.linear_triangulate([ref_proj, pr], pairs) for pr in projs]
    best, valid = cp.disambiguate_cam_pose_four(ref_proj, projs, pts)
    assert best == out["best_cand"][0] and valid == np.flatnonzero(out["obs_front"]).tolist() and len(valid) == 300
