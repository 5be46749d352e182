"""Refinement of a relative pose on the device (sfm_twoview_refine) against the NumPy rule of
tests/_twoview_refine_reference.py.  tests/test_twoview_refine_host.py shows on the CPU that every set of every parity case
used here is settled, so the decisions -- status, n_used, every byte of obs_inlier and obs_front, the counts, the summary -- are
compared exactly and no set is left out; R, t and F_out agree within max(1e-9, 100 d_P), d_P the spread of the reference's own
routes, cost and info within the same bound relative to their size, X_out as the pose tests bound it, and obs_res is the host
hook at the device's own output pose bit for bit.  On the sets of a camera that only rotated the baseline is not determined:
there R, the costs and |t| = 1 are held to the bound (and every decision, exactly)."""
import math

import numpy as np
import pytest

import _twoview_pose_reference as tp
import _twoview_refine_reference as rr
from test_twoview_refine_host import _lib_status, bad_arguments

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(hip, sc, iters=rr.ITERS, lam=rr.LAMBDA, outputs=None, mask=True):
    kw = {} if outputs is None else {"outputs": outputs}
    return hip.twoview_refine(sc.set_ptr, sc.left, sc.right, sc.R_in, sc.t_in, rr.K_LEFT, rr.K_RIGHT, lam, iters, rr.MAX_ERR2, rr.COS2_MIN,
                              sc.mask if mask else None, **kw)


worst = {"pose": 0.0, "F": 0.0, "cost": 0.0, "info": 0.0, "X": 0.0}


def compare(hip, got, ref, sc, what):
    assert np.array_equal(got["status"], ref.status), (what, np.flatnonzero(got["status"] != ref.status), got["status"], ref.status)
    assert np.array_equal(got["n_used"], ref.n_used), what
    assert np.array_equal(got["obs_inlier"], ref.inlier), (what, np.flatnonzero(got["obs_inlier"] != ref.inlier))
    assert np.array_equal(got["obs_front"], ref.front), (what, np.flatnonzero(got["obs_front"] != ref.front))
    assert np.array_equal(got["n_inliers"], ref.n_inliers) and np.array_equal(got["n_front"], ref.n_front), what
    assert np.array_equal(got["n_parallax"], ref.n_parallax), what
    assert np.array_equal(got["summary"], ref.summary), (what, got["summary"], ref.summary)
    assert np.array_equal(np.isnan(got["obs_res"]), np.isnan(ref.res)), what
    assert np.array_equal(np.isnan(got["X"]).any(axis=0), ref.front == 0) and np.array_equal(np.isnan(got["X"]).all(axis=0), ref.front == 0), what
    for s in range(sc.counts.size):
        lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
        bound = max(1e-9, 100.0 * ref.d_P[s])
        rotated = sc.names[s] == "rotation"
        if ref.status[s] & rr.KEPT_INPUT:
            assert same_bits(got["R"][s], sc.R_in[s]) and same_bits(got["t"][s], sc.t_in[s]), (what, s)
        if ref.status[s] & rr.BAD_POSE:
            assert not got["F"][s].any() and not got["cost"][:, s].any() and not got["info"][s].any()
            continue
        d = np.abs(got["R"][s] - ref.R[s]).max()
        if not rotated:
            d = max(d, np.abs(got["t"][s] - ref.t[s]).max())
            dF = np.abs(got["F"][s] - ref.F[s]).max()
            worst["F"] = max(worst["F"], float(dF))
            assert dF <= bound, (what, s, dF, bound)
        if not ref.status[s] & rr.KEPT_INPUT:
            assert abs(np.linalg.norm(got["t"][s]) - 1.0) <= 4e-16, (what, s)
        worst["pose"] = max(worst["pose"], float(d))
        assert d <= bound, (what, s, d, bound)
        for name, want in (("cost", ref.cost[:, s]), ("info", ref.info[s])):
            size = np.abs(want).max()
            dc = np.abs((got[name][:, s] if name == "cost" else got[name][s]) - want).max() / size if size > 0 else 0.0
            worst[name] = max(worst[name], float(dc))
            assert dc <= bound, (what, s, name, dc, bound)
            if size == 0:
                assert not (got[name][:, s] if name == "cost" else got[name][s]).any()
        # the residuals: the host hook at the device's own output pose, bit for bit
        for i in list(range(lo, min(hi, lo + 70))) + list(range(max(lo, hi - 3), hi)):
            r, _J = hip.twoview_refine_test(got["R"][s], got["t"][s], rr.K_LEFT, rr.K_RIGHT, sc.left[0, i], sc.left[1, i], sc.right[0, i],
                                            sc.right[1, i])
            if np.isnan(got["obs_res"][i]):
                assert not (np.isfinite(sc.left[:, i]).all() and np.isfinite(sc.right[:, i]).all()) or np.isnan(r), (what, s, i)
            else:
                assert same_bits(np.float64(r), got["obs_res"][i]), (what, s, i, r, got["obs_res"][i])
        front = ref.front[lo:hi] > 0
        if front.any() and not rotated:
            gx, rx = got["X"][:, lo:hi][:, front], ref.X[:, lo:hi][:, front]
            dx = np.abs(gx - rx).max(axis=0) / np.linalg.norm(rx, axis=0)
            worst["X"] = max(worst["X"], float(dx.max()))
            assert np.all(dx <= bound), (what, s, float(dx.max()), bound)


# ---- parity on every case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,iters,lam", rr.PARITY_CASES)
def test_parity_with_the_reference(hip, name, iters, lam):
    sc, ref = rr.scene_and_reference(name, iters, lam)
    got = run(hip, sc, iters, lam)
    compare(hip, got, ref, sc, (name, iters, lam))
    print("%s, %d iterations, lambda %g: %d sets, %d matches, worst device difference so far: %s"
          % (name, iters, lam, sc.counts.size, sc.left.shape[1], ", ".join("%s %.3e" % kv for kv in worst.items())))


def test_no_mask_means_every_match(hip):
    sc = rr.scene("general")
    ref = rr.reference(sc.set_ptr, sc.left, sc.right, None, sc.R_in, sc.t_in)
    assert ref.settled.all()
    compare(hip, run(hip, sc, mask=False), ref, sc, "no mask")


# ---- batch independence, determinism -------------------------------------------------------------------------------------
PER_SET = ("R", "t", "F", "info", "n_used", "status", "n_inliers", "n_front", "n_parallax")
PER_MATCH = ("obs_res", "obs_inlier", "obs_front")


def _same_sets(hip, sc, whole, sets, what):
    sub = rr.subset(sc, sets)
    got = run(hip, sub)
    for name in PER_SET:
        assert same_bits(got[name], whole[name][sets]), (what, name)
    assert same_bits(got["cost"], whole["cost"][:, sets]), what
    for name in PER_MATCH:
        assert same_bits(got[name], whole[name][sub.cols]), (what, name)
    assert same_bits(got["X"], whole["X"][:, sub.cols]), what
    return got


def test_every_set_size_alone_and_in_the_batch(hip):
    sc = rr.scene("sizes")
    whole = run(hip, sc)
    for s in range(sc.counts.size):
        got = _same_sets(hip, sc, whole, [s], "alone %d" % sc.counts[s])
        assert got["summary"][0] + got["summary"][1] + got["summary"][2] == 1
    _same_sets(hip, sc, whole, np.random.default_rng(3).permutation(sc.counts.size).tolist(), "permuted")


def test_a_set_alone_and_inside_the_259(hip):
    sc = rr.scene("many")
    whole = run(hip, sc)
    for s in (0, 5, 64, 65, 127, 128, 255, 256, 257, 258):
        _same_sets(hip, sc, whole, [s], "set %d alone" % s)
    _same_sets(hip, sc, whole, list(range(1, 259, 2)), "every other set")


def test_two_calls_give_the_same_bits(hip):
    for name in ("sizes", "many"):
        sc = rr.scene(name)
        first, second = run(hip, sc), run(hip, sc)
        assert all(same_bits(first[k], second[k]) for k in first), name


def test_no_iteration_returns_the_input_bits(hip):
    for name in ("sizes", "special", "rotation"):
        sc = rr.scene(name)
        got = run(hip, sc, iters=0)
        assert same_bits(got["R"], sc.R_in) and same_bits(got["t"], sc.t_in), name
        assert same_bits(got["cost"][0], got["cost"][1]) and np.all(got["status"] & hip.REFINE_KEPT_INPUT), name


CONVERGED_ITERS = 20


def test_a_second_refinement_stays_where_the_first_ended(hip):
    """A pose at its minimum is a fixed point: refined again it moves by less than 1e-9 and the guard lets the iterated pose
    stand (its cost moves by rounding only, which the 2^-30 of the guard covers).  The first call takes 20 steps: Gauss-Newton
    converges linearly where the residuals do not vanish, and after six steps the rule itself -- the NumPy reference -- is
    still 3.3e-7 from its fixed point on forward motion and 1.6e-8 on the scene of sizes; after twenty it moves by less than
    1e-14 on every scene (tests/test_twoview_refine_host.py holds it to 1e-12)."""
    for name in ("general_displaced", "plane", "forward", "sizes"):
        sc = rr.scene(name)
        first = run(hip, sc, iters=CONVERGED_ITERS)
        again = hip.twoview_refine(sc.set_ptr, sc.left, sc.right, first["R"], first["t"], rr.K_LEFT, rr.K_RIGHT, rr.LAMBDA, rr.ITERS, rr.MAX_ERR2,
                                   rr.COS2_MIN, sc.mask)
        done = (first["status"] & (hip.REFINE_TOO_FEW | hip.REFINE_BAD_POSE)) == 0
        assert done.any() and not np.any(first["status"][done]) and not np.any(again["status"][done]), (name, first["status"], again["status"])
        moved = max(np.abs(again["R"] - first["R"]).max(), np.abs(again["t"] - first["t"]).max())
        print("%s: a second refinement moves the pose by %.3e" % (name, moved))
        assert moved < 1e-9, (name, moved)
        assert np.array_equal(again["obs_inlier"], first["obs_inlier"]) and np.array_equal(again["obs_front"], first["obs_front"])


# ---- the _dev form ------------------------------------------------------------------------------------------------------
def test_dev_form_on_a_callers_stream(hip):
    import torch
    sc = rr.scene("sizes")
    want = run(hip, sc)
    S, M = sc.counts.size, sc.left.shape[1]
    stream = torch.cuda.Stream()

    def f64(shape):
        return torch.full(shape, 7.0, dtype=torch.float64, device="cuda")

    with torch.cuda.stream(stream):
        d_left, d_right = torch.from_numpy(sc.left).cuda(), torch.from_numpy(sc.right).cuda()
        d_mask = torch.from_numpy(sc.mask.astype(np.uint8)).cuda()
        d_Rin, d_tin = torch.from_numpy(sc.R_in).cuda(), torch.from_numpy(sc.t_in).cuda()
        d = {"R": f64((S, 3, 3)), "t": f64((S, 3)), "F": f64((S, 3, 3)), "cost": f64((2, S)), "info": f64((S, 15)), "obs_res": f64((M,)),
             "X": f64((3, M)), "obs_inlier": torch.full((M,), 9, dtype=torch.uint8, device="cuda"),
             "obs_front": torch.full((M,), 9, dtype=torch.uint8, device="cuda"), "summary": torch.full((6,), -1, dtype=torch.int64, device="cuda")}
        for name in ("n_used", "status", "n_inliers", "n_front", "n_parallax"):
            d[name] = torch.full((S,), -5, dtype=torch.int32, device="cuda")
        stream.synchronize()
        hip.twoview_refine_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), d_Rin.data_ptr(), d_tin.data_ptr(), rr.K_LEFT, rr.K_RIGHT,
                               rr.LAMBDA, rr.ITERS, rr.MAX_ERR2, rr.COS2_MIN, d_mask.data_ptr(), d["R"].data_ptr(), d["t"].data_ptr(),
                               d["F"].data_ptr(), d["cost"].data_ptr(), d["info"].data_ptr(), d["n_used"].data_ptr(), d["status"].data_ptr(),
                               d["obs_res"].data_ptr(), d["obs_inlier"].data_ptr(), d["obs_front"].data_ptr(), d["X"].data_ptr(),
                               d["n_inliers"].data_ptr(), d["n_front"].data_ptr(), d["n_parallax"].data_ptr(), d["summary"].data_ptr(),
                               stream.cuda_stream)
        got = {k: v.cpu().numpy() for k, v in d.items()}
        assert same_bits(d_left.cpu().numpy(), sc.left) and same_bits(d_Rin.cpu().numpy(), sc.R_in) and same_bits(d_tin.cpu().numpy(), sc.t_in)
        # only the pose asked for: nothing else is needed; and in place, the output over the input
        R2, t2 = d_Rin.clone(), d_tin.clone()
        stream.synchronize()
        hip.twoview_refine_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), d_Rin.data_ptr(), d_tin.data_ptr(), rr.K_LEFT, rr.K_RIGHT,
                               rr.LAMBDA, rr.ITERS, rr.MAX_ERR2, rr.COS2_MIN, d_mask.data_ptr(), R2.data_ptr(), t2.data_ptr(),
                               stream=stream.cuda_stream)
        assert same_bits(R2.cpu().numpy(), got["R"]) and same_bits(t2.cpu().numpy(), got["t"])
    for name in want:
        assert same_bits(got[name], want[name]), name


# ---- the optional outputs ---------------------------------------------------------------------------------------------------
def test_every_optional_output_absent_singly_and_together(hip):
    sc = rr.subset(rr.scene("sizes"), [1, 4, 6, 8, 9])           # 1, 8, 63, 65 and 1 023 matches
    full = run(hip, sc)
    names = hip.REFINE_OUTPUTS
    subsets = [tuple(n for n in names if n != gone) for gone in names] + [(), names] + [(n,) for n in names]
    for subset in subsets:
        got = run(hip, sc, outputs=subset)
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
    empty = hip.twoview_refine([0], np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((0, 3, 3)), np.zeros((0, 3)), rr.K_LEFT, rr.K_RIGHT)
    assert empty["R"].shape == (0, 3, 3) and not empty["summary"].any()


# ---- the Python entry points -------------------------------------------------------------------------------------------
def _pairs(sc, s):
    lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
    one = np.ones((1, hi - lo))
    return [np.vstack((sc.left[:, lo:hi], one)), np.vstack((sc.right[:, lo:hi], one))]


def test_refine_relative_pose(hip, sfm):
    P = sfm.processors
    cp = P.HipCamposeProcessor(None, 5, 25)
    for name in ("general_displaced", "plane_displaced"):
        sc, ref = rr.scene_and_reference(name)
        for s in range(sc.counts.size):
            lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
            rot0, centre0 = tp.to_reference_convention(sc.R_in[s], sc.t_in[s])
            rot, centre, before, after, inl, front, info, status = cp.refine_relative_pose(
                _pairs(sc, s), rot0, centre0, rr.K_LEFT, rr.K_RIGHT, np.flatnonzero(sc.mask[lo:hi]), rr.ITERS, rr.LAMBDA, 2.0, tp.MIN_ANGLE_DEG)
            want_rot, want_centre = tp.to_reference_convention(ref.R[s], ref.t[s])
            bound = max(1e-9, 100.0 * ref.d_P[s])
            assert np.abs(rot - want_rot).max() <= bound and np.abs(centre - want_centre).max() <= bound and centre.shape == (3, 1)
            assert status == ref.status[s] == 0 and inl == np.flatnonzero(ref.inlier[lo:hi]).tolist()
            assert front == np.flatnonzero(ref.front[lo:hi]).tolist()
            assert abs(before - np.sqrt(ref.cost[0, s] / ref.n_used[s])) <= 1e-6 * before and abs(after - np.sqrt(ref.cost[1, s] / ref.n_used[s])) <= 1e-6 * after
            assert after ** 2 < 0.07 * before ** 2 and info.shape == (5, 5) and np.array_equal(info, info.T) and np.all(np.linalg.eigvalsh(info) > 0)
            assert same_bits(cp.refine_last["R"].T @ -cp.refine_last["t"].reshape(3, 1), centre)
    with pytest.raises(ValueError):
        cp.refine_relative_pose(_pairs(sc, 0), rot0, centre0, rr.K_LEFT, rr.K_RIGHT, min_angle_deg=-1.0)
    # a pose without a baseline: nothing to refine, the input comes back
    rot, centre, before, after, inl, front, info, status = cp.refine_relative_pose(_pairs(sc, 0), np.identity(3), np.zeros((3, 1)), rr.K_LEFT, rr.K_RIGHT)
    assert status == hip.REFINE_BAD_POSE | hip.REFINE_KEPT_INPUT and same_bits(rot, np.identity(3)) and not centre.any()
    assert np.isnan(before) and np.isnan(after) and inl == [] and front == [] and not info.any()


def test_initialise_pairs_with_refinement(hip, sfm):
    """A general, a plane, a rotation and a hopeless set in one call: the first two are refined, the rotation set (no parallax)
    and the hopeless one come back as the pose call left them; the call without refinement is unchanged."""
    P = sfm.processors
    K = tp.K_LEFT
    g = tp.family_part("general", 300, 11, 0.1, Kr=K)
    p = tp.family_part("plane", 300, 12, 0.1, Kr=K)
    rot = tp.family_part("rotation", 300, 13, 0.0, noise=0.3, Kr=K)
    rng = np.random.default_rng(5)
    hopeless = (rng.uniform(0, 640, (2, 4)), rng.uniform(0, 480, (2, 4)))
    sets = [[g[0], g[1]], [p[0], p[1]], [rot[0], rot[1]], [hopeless[0], hopeless[1]]]

    def processor():
        return P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))

    plain = processor().initialise_pairs(sets, K)
    ep = processor()
    out = ep.initialise_pairs(sets, K, refine_iters=6)
    assert [o["verdict"] for o in out] == ["general", "degenerate", "degenerate", "none"]
    for a, b in zip(plain, out):
        assert "R_refined" not in a and set(a) < set(b)
        for key in a:
            assert same_bits(np.asarray(a[key]), np.asarray(b[key])) if not isinstance(a[key], (str, list)) else a[key] == b[key], key
    for o, fam, part in ((out[0], "general", g), (out[1], "plane", p)):
        R0, t0 = tp.planted(fam)
        assert o["refine_status"] == 0 and o["refine_used"] == o["n_front"] and o["refine_cost"][1] <= o["refine_cost"][0]
        # the refined pose lies at the minimum of the Sampson cost of 270 matches with 0.3 px of noise: well inside a degree of the planted one
        assert np.abs(o["R_refined"] - R0).max() < 0.01 and rr.baseline_angle_deg(o["t_refined"], t0) < 1.0, fam
        assert abs(np.linalg.norm(o["t_refined"]) - 1.0) < 1e-15 and abs(np.linalg.norm(o["F_refined"]) - 1.0) < 1e-15
        assert np.allclose(o["rot_refined"], o["R_refined"].T) and np.allclose(o["centre_refined"][:, 0], -o["R_refined"].T @ o["t_refined"])
        assert not set(o["refine_inliers"]) & set(np.flatnonzero(part[2]).tolist()) and len(o["refine_inliers"]) >= 0.95 * 270
        rms = np.sqrt(o["refine_cost"][1] / o["refine_used"])
        assert 0.15 < rms < 0.45, (fam, rms)
    for o in (out[2], out[3]):          # no parallax / no pose: an empty mask, the pose of the pose call comes back bit for bit
        assert o["refine_status"] == hip.REFINE_EMPTY | hip.REFINE_TOO_FEW | hip.REFINE_KEPT_INPUT | (0 if o["best_cand"] >= 0 else hip.REFINE_BAD_POSE)
        assert same_bits(o["R_refined"], o["R"]) and same_bits(o["t_refined"], o["t"]) and o["refine_used"] == 0
    assert out[2]["status"] & (hip.POSE_NO_PARALLAX | hip.POSE_NO_POSE) and out[3]["best_cand"] == -1
    unposed = sum(o["best_cand"] < 0 for o in out[2:])
    assert ep.refine_last["summary"].tolist()[:4] == [2, unposed, 2 - unposed, 0]
    for s in range(4):                  # one call over the four sets is what the sets give alone
        alone = processor().initialise_pairs([sets[s]], K, refine_iters=6)[0]
        assert same_bits(alone["R_refined"], out[s]["R_refined"]) and same_bits(alone["t_refined"], out[s]["t_refined"])
        assert alone["refine_inliers"] == out[s]["refine_inliers"]


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def test_refine_pairs_against_the_host_form(hip, sfm):
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
            _r, _q, mask = P.verify_pairs(kt, ref_idx, que_idx, 2.0, 128, 2)
            F = kt.twoview_last["fund_mat"]
            plain = P.pose_pairs(kt, ref_idx, que_idx, F, "fundamental", K, K, mask, 1.0, 8)
            down = kt.kt_download_bytes
            got_r, got_q, rot, centre, front, counts = P.pose_pairs(kt, ref_idx, que_idx, F, "fundamental", K, K, mask, 1.0, 8, refine_iters=6)
            assert kt.kt_download_bytes == down               # the store downloaded nothing on its own account
            assert np.array_equal(got_r, r_idx) and np.array_equal(got_q, q_idx)
            assert same_bits(rot, plain[2]) and same_bits(centre, plain[3]) and front == plain[4] and set(plain[5]) < set(counts)
            assert counts["best_cand"] >= 0 and counts["refine_status"] == 0 and counts["refine_used"] == counts["n_front"]
            want = cp.refine_relative_pose(pairs, rot, centre, K, K, front, 6, 0.0, 2.0, 1.0)
            R_in, t_in = P.pose_from_reference_convention(rot, centre)
            direct = kt._store.refine_pairs(ref_idx, que_idx, R_in, t_in, K, K, 0.0, 6, 4.0, math.cos(math.radians(1.0)) ** 2,
                                            np.isin(np.arange(r_idx.shape[1]), front))
            for name in ("R", "t", "F", "info", "obs_res", "obs_inlier", "obs_front", "X"):
                assert same_bits(direct[name], cp.refine_last[name]), name
            for name in ("n_used", "status", "n_inliers", "n_front", "n_parallax"):
                assert direct[name] == cp.refine_last[name], name
            assert same_bits(direct["cost"], cp.refine_last["cost"]) and same_bits(direct["R"].T.copy(), want[0])
            assert np.array_equal(direct["r_idx"], r_idx[0]) and np.array_equal(direct["q_idx"], q_idx[0])
            # pose_pairs refines the library's own (R, t), not their round trip through (rot, centre): the same minimum
            assert np.abs(counts["R_refined"] - direct["R"]).max() < 1e-9 and np.abs(counts["t_refined"] - direct["t"]).max() < 1e-9
            assert counts["refine_cost"][1] <= counts["refine_cost"][0] and counts["refine_inliers"] == np.flatnonzero(direct["obs_inlier"]).tolist()
    finally:
        kt.kt_release()
