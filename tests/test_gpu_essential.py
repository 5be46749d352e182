"""GPU tests of the robust essential matrix: sfm_essential_ransac, its _dev form and the Python entry points, against the
float64 reference of tests/_essential_reference.py.  Decisions (status, best_hyp, best_root, n_valid, n_inliers, obs_inlier,
summary) are exact on settled sets -- every set of every parity case is settled, tests/test_essential_host.py checks that on
the CPU; E_out and F_out are within max(1e-9, 100 d) of the reference, d the reference's own two-route difference (d_E
entry-wise, d_G in the G measure of the two-view reference)."""
import math

import numpy as np
import pytest

import _essential_reference as er
import _twoview_ransac_reference as tv
from _twoview_checks import same_bits, subset as _subset

pytestmark = pytest.mark.gpu

DECISIONS = ("inlier", "n_inliers", "best_hyp", "best_root", "n_valid", "status")


def run(hip, sc, Km=er.K, max_hyp=128, max_err2=er.MAX_ERR2, outputs=None):
    kw = {} if outputs is None else {"outputs": outputs}
    return hip.essential_ransac(sc.set_ptr, sc.left, sc.right, Km, Km, max_err2, max_hyp, **kw)


def canonical(A):
    """Frobenius norm 1 and the entry of largest magnitude positive (where two entries tie to the last bit, either may be)."""
    return abs(np.linalg.norm(A) - 1.0) < 1e-14 and A.max() >= np.abs(A).max() * (1.0 - 4e-16)


def check_against(ref, got, where=""):
    """Exact decisions, matrices at the per-set bound, sets without a model as zeros."""
    assert ref.settled.all(), where
    for name in DECISIONS:
        assert np.array_equal(got[name], getattr(ref, name)), (where, name)
    assert np.array_equal(got["summary"], ref.summary), where
    solved = ref.best_hyp >= 0
    for s in np.flatnonzero(solved):
        d_E = float(np.max(np.abs(got["E"][s] - ref.E[s])))
        d_G = tv.g_difference(got["F"][s], ref.F[s], ref.c[s])
        print(where, "set", s, "d_E %.3e device %.3e | d_G %.3e device %.3e" % (ref.d_E[s], d_E, ref.d_G[s], d_G))
        assert d_E <= max(1e-9, 100.0 * ref.d_E[s]), (where, s, d_E, ref.d_E[s])
        assert d_G <= max(1e-9, 100.0 * ref.d_G[s]), (where, s, d_G, ref.d_G[s])
        assert canonical(got["E"][s]) and canonical(got["F"][s]), (where, s)
        sv = np.linalg.svd(got["E"][s])[1]
        assert abs(sv[0] - sv[1]) < 1e-9 and sv[2] < 1e-9, (where, s, sv)
    for name in ("E", "F"):
        assert same_bits(got[name][~solved], np.zeros_like(got[name][~solved])), (where, name)
    assert (got["best_root"][~solved] == -1).all() and (got["n_inliers"][~solved] == 0).all()


def same_sets(hip, sc, whole, sets, Km, max_hyp, what):
    """The sets `sets` of the scene in a call of their own give the bits they have in `whole`, the result of the whole scene."""
    sub = _subset(sc, sets)
    got = run(hip, sub, Km, max_hyp)
    for k, s in enumerate(sets):
        for name in ("E", "F", "n_inliers", "best_hyp", "best_root", "n_valid", "status"):
            assert same_bits(got[name][k], whole[name][s]), (what, s, name)
        assert same_bits(got["inlier"][sub.set_ptr[k]:sub.set_ptr[k + 1]], whole["inlier"][sc.set_ptr[s]:sc.set_ptr[s + 1]]), (what, s)
    return got


# ---- parity with the reference on every case --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.CASES, ids=lambda c: "%s-%g-%d" % c)
def test_parity_with_the_reference(hip, case):
    name, max_err2, max_hyp = case
    sc, Km, ref = er.case_reference(case)
    check_against(ref, run(hip, sc, Km, max_hyp, max_err2), where="%s/%g/%d" % case)


def test_every_set_size_alone(hip):
    """0, 5, 6, 7, 15 .. 2 049 matches, each in a call of its own: the reference's decisions and the bits of the one call."""
    case = ("paths", er.MAX_ERR2, 128)
    sc, Km, ref = er.case_reference(case)
    assert sc.counts.tolist() == list(er.PATHS_COUNTS)
    whole = run(hip, sc, Km, 128)
    check_against(ref, whole, where="paths in one call")
    for s in range(sc.counts.size):
        got = same_sets(hip, sc, whole, [s], Km, 128, "alone")
        want = [0, 0, 0, 0, 0, 0]
        want[0 if ref.status[s] == 0 else (2 if ref.status[s] & er.TOO_FEW else 1)] = 1
        if ref.status[s] == 0:
            want[4], want[5] = int(ref.n_inliers[s]), int(sc.counts[s] - ref.n_inliers[s])
        assert got["summary"].tolist() == want, s


def test_ties_go_to_the_lowest_valid_candidate(hip):
    """Under a threshold every match passes, every valid candidate has every match: the winner is the lowest (h, r)."""
    case = ("ties", er.EVERYONE, er.TIES_HYP)
    sc, Km, ref = er.case_reference(case)
    got = run(hip, sc, Km, er.TIES_HYP, er.EVERYONE)
    check_against(ref, got, where="ties")
    assert got["n_inliers"].tolist() == sc.counts.tolist() and got["inlier"].all()
    for s in range(sc.counts.size):                            # no valid candidate comes before the winner
        first = run(hip, _subset(sc, [s]), Km, int(got["best_hyp"][s]) + 1, er.EVERYONE)
        assert first["best_hyp"][0] == got["best_hyp"][s] and first["best_root"][0] == got["best_root"][s] == 0
        if got["best_hyp"][s] > 0:
            before = run(hip, _subset(sc, [s]), Km, int(got["best_hyp"][s]), er.EVERYONE)
            assert before["n_valid"][0] == 0 and before["status"][0] == hip.ESSENTIAL_NO_MODEL


def test_degenerate_sets(hip):
    """Identical points, a noise-free pure rotation, non-finite coordinates: the reference's routes need not agree on these,
    so what is asserted is what the rule says of any answer -- finite canonical outputs or zeros, the mask that of F_out (no
    match within 1e-6 of the threshold decides otherwise), the counts consistent, a non-finite match nobody's inlier."""
    sc = er.scene("degenerate")
    got = run(hip, sc)
    again = run(hip, sc)
    assert all(same_bits(got[k], again[k]) for k in got)
    assert got["status"][0] == hip.ESSENTIAL_NO_MODEL and got["n_valid"][0] == 0       # identical points: no finite solution
    assert got["status"][2] == 0                                                         # 58 clean finite matches remain
    total = [0, 0]
    for s in range(3):
        lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
        E, F, mask = got["E"][s], got["F"][s], got["inlier"][lo:hi].astype(bool)
        assert np.isfinite(E).all() and np.isfinite(F).all()
        if got["status"][s]:
            assert not E.any() and not F.any() and not mask.any() and got["best_hyp"][s] == got["best_root"][s] == -1
            continue
        assert canonical(E) and canonical(F) and got["n_inliers"][s] == mask.sum() >= er.MIN_COUNT
        d2 = tv.sampson(F, *tv.set_of(sc, s))
        assert np.array_equal(mask[tv.inliers(d2, er.MAX_ERR2 * (1 - 1e-6))], np.ones(tv.inliers(d2, er.MAX_ERR2 * (1 - 1e-6)).sum(), dtype=bool))
        assert not mask[~tv.inliers(d2, er.MAX_ERR2 * (1 + 1e-6))].any()
        total[0] += int(mask.sum()); total[1] += int((~mask).sum())
    lo = sc.set_ptr[2]
    assert not got["inlier"][lo + 17] and not got["inlier"][lo + 40]
    assert got["summary"][4:].tolist() == total and got["summary"][:4].sum() == 3 and got["summary"][3] == 0


def test_six_matches_five_matches_and_an_empty_call(hip):
    sc = er.scene("paths")
    l, r = tv.set_of(sc, int(np.flatnonzero(sc.counts == 7)[0]))
    few = hip.essential_ransac([0, 5], l[:, :5], r[:, :5], er.K, er.K, er.MAX_ERR2)
    assert few["status"].tolist() == [hip.ESSENTIAL_TOO_FEW] and few["summary"].tolist() == [0, 0, 1, 0, 0, 0]
    assert not few["E"].any() and not few["F"].any() and not few["inlier"].any()
    assert few["best_hyp"].tolist() == [-1] and few["best_root"].tolist() == [-1] and few["n_valid"].tolist() == [0]
    none = hip.essential_ransac([0], np.zeros((2, 0)), np.zeros((2, 0)), er.K, er.K, er.MAX_ERR2)
    assert none["E"].shape == (0, 3, 3) and not none["summary"].any()


# ---- a set's bits depend on its own matches, the intrinsics and the options only ---------------------------------------------
@pytest.mark.parametrize("max_hyp", [5, 65])
def test_batch_independence_bit_for_bit(hip, max_hyp):
    sc = er.scene("paths")
    whole = run(hip, sc, er.K, max_hyp)
    again = run(hip, sc, er.K, max_hyp)
    assert all(same_bits(whole[k], again[k]) for k in whole)           # two calls
    n_sets = sc.counts.size
    same_sets(hip, sc, whole, np.random.default_rng(3).permutation(n_sets).tolist(), er.K, max_hyp, "permuted")
    same_sets(hip, sc, whole, [s for s in range(n_sets) if sc.counts[s] <= er.LONG], er.K, max_hyp, "without the long sets")


def test_dev_form_on_a_callers_stream(hip):
    import torch
    sc = er.scene("paths")
    want = run(hip, sc, er.K, 65)
    S, M = sc.counts.size, sc.left.shape[1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_left, d_right = torch.from_numpy(sc.left).cuda(), torch.from_numpy(sc.right).cuda()
        d_E, d_F = (torch.full((S, 9), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        d_in = torch.full((M,), 9, dtype=torch.uint8, device="cuda")
        d_n, d_best, d_root, d_valid, d_st = (torch.full((S,), -5, dtype=torch.int32, device="cuda") for _ in range(5))
        d_sum = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        stream.synchronize()
        hip.essential_ransac_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), er.K, er.K, er.MAX_ERR2, 65, d_E.data_ptr(),
                                 d_F.data_ptr(), d_in.data_ptr(), d_n.data_ptr(), d_best.data_ptr(), d_root.data_ptr(),
                                 d_valid.data_ptr(), d_st.data_ptr(), d_sum.data_ptr(), stream.cuda_stream)
        tensors = dict(E=d_E, F=d_F, inlier=d_in, n_inliers=d_n, best_hyp=d_best, best_root=d_root, n_valid=d_valid, status=d_st,
                       summary=d_sum)
        got = {k: t.cpu().numpy() for k, t in tensors.items()}
        assert same_bits(d_left.cpu().numpy(), sc.left) and same_bits(d_right.cpu().numpy(), sc.right)
        # only the matrix asked for: every other buffer stays as it is
        d_E2 = torch.zeros((S, 9), dtype=torch.float64, device="cuda")
        stream.synchronize()
        hip.essential_ransac_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), er.K, er.K, er.MAX_ERR2, 65, d_E2.data_ptr(),
                                 stream=stream.cuda_stream)
        assert same_bits(d_E2.cpu().numpy(), got["E"])
        assert all(same_bits(t.cpu().numpy(), got[k]) for k, t in tensors.items())
    for k in got:
        assert same_bits(got[k].reshape(want[k].shape), want[k]), k


def test_every_optional_output_absent(hip):
    sc = _subset(er.scene("paths"), [1, 4, 9, 11])            # 5, 15, 65 and 256 matches
    full = run(hip, sc, er.K, 65)
    names = hip.ESSENTIAL_OUTPUTS
    subsets = [()] + [(n,) for n in names] + [tuple(m for m in names if m != n) for n in names]
    for chosen in subsets:
        got = run(hip, sc, er.K, 65, outputs=chosen)
        assert same_bits(got["E"], full["E"]), chosen
        for name in names:
            if name in chosen:
                assert same_bits(got[name], full[name]), (chosen, name)
            else:
                assert got[name] is None


def test_the_c_entry_points_refuse_what_the_header_says(hip):
    """SFM_E_SHAPE from the library itself, past the Python checks, and the output untouched."""
    lib = hip.load()
    left = np.zeros((2, 6))
    E = np.full(9, 7.0)
    good = np.array([0, 6], dtype=np.int32)
    Kg = np.ascontiguousarray(er.K).reshape(9)

    def call(ptr=good, n_sets=1, M=6, max_err2=4.0, max_hyp=128, Kl=Kg, Kr=Kg):
        ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        return lib.sfm_essential_ransac(n_sets, hip.iptr(ptr), M, hip.dptr(left), hip.dptr(left), hip.dptr(Kl), hip.dptr(Kr), max_err2,
                                        max_hyp, hip.dptr(E), None, None, None, None, None, None, None, None)

    lower, scaled, nan = Kg.copy(), Kg.copy(), Kg.copy()
    lower[3], scaled[8], nan[0] = 1e-3, 2.0, np.nan
    for kw in (dict(max_err2=float("nan")), dict(max_err2=-1.0), dict(max_hyp=-1), dict(max_hyp=65537), dict(ptr=[1, 6]),
               dict(ptr=[0, 3, 2, 6], n_sets=3), dict(ptr=[0, 5]), dict(n_sets=-1), dict(M=-1), dict(Kl=lower), dict(Kr=scaled),
               dict(Kl=nan)):
        assert call(**kw) == hip.E_SHAPE, kw
    assert np.all(E == 7.0)


# ---- the Python entry points ---------------------------------------------------------------------------------------------------
def _pairs(sc, s):
    lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
    one = np.ones((1, hi - lo))
    return [np.vstack((sc.left[:, lo:hi], one)), np.vstack((sc.right[:, lo:hi], one))]


def _epipolar(P):
    return P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))


def test_determine_essential_mat_robust(hip, sfm):
    case = ("half_displaced", er.MAX_ERR2, 128)
    sc, Km, ref = er.case_reference(case)
    ep = _epipolar(sfm.processors)
    idx = ep.determine_essential_mat_robust(_pairs(sc, 2), Km, Km)
    lo, hi = sc.set_ptr[2], sc.set_ptr[3]
    assert idx == np.flatnonzero(ref.inlier[lo:hi]).tolist()
    last = ep.essential_last
    assert (last["hypothesis"], last["root"], last["n_valid"], last["status"]) == (ref.best_hyp[2], ref.best_root[2], ref.n_valid[2], 0)
    alone = run(hip, _subset(sc, [2]), Km)
    assert same_bits(ep.esse_mat, alone["E"][0]) and ep.fund_mat[2][2] == 1.0 and same_bits(ep.fund_mat, alone["F"][0] / alone["F"][0][2][2])
    assert np.max(np.abs(ep.esse_mat - ref.E[2])) <= max(1e-9, 100.0 * ref.d_E[2])
    before_e, before_f = ep.esse_mat.copy(), ep.fund_mat.copy()
    few = [m[:, :5] for m in _pairs(sc, 0)]
    assert ep.determine_essential_mat_robust(few, Km, Km) == [] and same_bits(ep.esse_mat, before_e) and same_bits(ep.fund_mat, before_f)
    assert ep.essential_last["status"] == hip.ESSENTIAL_TOO_FEW and ep.essential_last["hypothesis"] == -1
    with pytest.raises(ValueError):
        ep.determine_essential_mat_robust(_pairs(sc, 0), Km, Km, max_sampson_px=-1.0)


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def test_essential_pairs_against_the_host_form(hip, sfm):
    """The pairs of a device tracker: the bits of determine_essential_mat_robust on the downloaded pairs, no coordinate down."""
    P = sfm.processors
    dv = sfm.scenes.make_descriptor_views(n_views=3, n_pts=200, seed=0)
    views = [View(dv.key_pts(v), dv.sift[v]) for v in range(3)]
    K = np.asarray(sfm.scenes.UPENN_K, dtype=np.float64)
    kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
    try:
        for v in range(3):
            kt.add_new_view(views[v], views[:v])
        for ref_idx, que_idx in ((0, 1), (0, 2), (1, 2)):
            pairs, r_idx, q_idx = kt.generate_matched_pairs(ref_idx, que_idx, views)
            ep = _epipolar(P)
            want = ep.determine_essential_mat_robust(pairs, K, K, 2.0, 65)
            down = kt.kt_download_bytes
            got_r, got_q, mask = P.essential_pairs(kt, ref_idx, que_idx, K, K, 2.0, 65)
            assert kt.kt_download_bytes == down               # the store downloaded nothing on its own account
            assert np.array_equal(got_r, r_idx) and np.array_equal(got_q, q_idx)
            assert np.flatnonzero(mask).tolist() == want and len(want) >= er.MIN_COUNT
            for name in ("esse_mat", "fund_mat"):
                assert same_bits(kt.essential_last[name], ep.essential_last[name]), name
            for name in ("hypothesis", "root", "n_valid", "status", "inliers"):
                assert kt.essential_last[name] == ep.essential_last[name], name
        assert P.essential_pairs(kt, 0, 3, K, K) is None
    finally:
        kt.kt_release()


def test_estimate_relative_pose_minimal(hip, sfm):
    """Half of the matches displaced: the outputs are the composition of the three reference modules."""
    import _twoview_pose_reference as tp
    import _twoview_refine_reference as rr
    P = sfm.processors
    case = ("half_displaced", er.MAX_ERR2, 128)
    sc, Km, ref = er.case_reference(case)
    s = 2
    lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
    l, r = tv.set_of(sc, s)
    cp = P.HipCamposeProcessor(None, 5, 25)
    rot, centre, before, after, inl, front, info, status = cp.estimate_relative_pose_minimal(_pairs(sc, s), Km, Km)
    assert cp.essential_last["inliers"] == np.flatnonzero(ref.inlier[lo:hi]).tolist() and cp.essential_last["root"] == ref.best_root[s]
    # the same composition through the three native calls, bit for bit
    cos2 = math.cos(math.radians(2.0)) ** 2
    ess = run(hip, _subset(sc, [s]), Km)
    posed = hip.twoview_pose([0, hi - lo], l, r, ess["F"], [hip.POSE_FROM_F], Km, Km, cos2, 1, ess["inlier"])
    fine = hip.twoview_refine([0, hi - lo], l, r, posed["R"], posed["t"], Km, Km, 0.0, 6, 4.0, cos2, (posed["obs_front"] > 0).astype(np.uint8))
    assert same_bits(rot, fine["R"][0].T.copy()) and same_bits(centre, (-fine["R"][0].T @ fine["t"][0]).reshape(3, 1))
    assert status == fine["status"][0] == 0 and inl == np.flatnonzero(fine["obs_inlier"]).tolist() and front == np.flatnonzero(fine["obs_front"]).tolist()
    # ... and the reference modules on the reference's own essential result
    pose_ref = tp.reference([0, hi - lo], l, r, ref.inlier[lo:hi], [ref.F[s]], [tp.FROM_F], Km, Km, cos2, 1)
    assert pose_ref.settled.all() and posed["best_cand"][0] == pose_ref.best[0] >= 0 and np.array_equal(posed["obs_front"], pose_ref.obs)
    fine_ref = rr.reference([0, hi - lo], l, r, pose_ref.obs > 0, pose_ref.R, pose_ref.t, Km, Km, 0.0, 6, 4.0, cos2)
    assert fine_ref.settled.all()
    want_rot, want_centre = tp.to_reference_convention(fine_ref.R[0], fine_ref.t[0])
    bound = max(1e-9, 100.0 * max(fine_ref.d_P[0], pose_ref.d_P[0], ref.d_E[s]))
    print("pose: device %.3e %.3e bound %.3e" % (np.abs(rot - want_rot).max(), np.abs(centre - want_centre).max(), bound))
    assert np.abs(rot - want_rot).max() <= bound and np.abs(centre - want_centre).max() <= bound
    assert inl == np.flatnonzero(fine_ref.inlier).tolist() and front == np.flatnonzero(fine_ref.front).tolist()
    # the planted motion of two_views: rot_y(0.15), t = (-1, 0.1, 0.2); 150 clean matches with 0.5 px of noise
    t0 = np.array([-1.0, 0.1, 0.2]) / np.linalg.norm([-1.0, 0.1, 0.2])
    assert np.abs(rot.T - tv._rot_y(0.15)).max() < 0.01 and rr.baseline_angle_deg(-rot.T @ centre[:, 0], t0) < 2.0
    # a key displaced by 30 to 120 px in a random direction lands within 2 px of its epipolar line with probability about
    # 4 asin(2 / 75) / (2 pi) = 1.7 %: such matches cannot be told from clean ones; 5 % of the displaced is the bound
    displaced = set(np.flatnonzero(sc.displaced[lo:hi]).tolist())
    assert len(set(inl) & displaced) <= 0.05 * len(displaced) and after <= before
    with pytest.raises(ValueError):
        cp.estimate_relative_pose_minimal(_pairs(sc, s), Km, Km, min_angle_deg=91.0)


def test_initialise_pairs_minimal(hip, sfm):
    """minimal=False is today's dictionary on the cases of tests/test_gpu_twoview_refine.py; minimal=True changes the general
    set only, to the model of one essential_ransac call."""
    import _twoview_pose_reference as tp
    import _twoview_refine_reference as rr
    P = sfm.processors
    K = tp.K_LEFT
    g = tp.family_part("general", 300, 11, 0.1, Kr=K)
    p = tp.family_part("plane", 300, 12, 0.1, Kr=K)
    rot = tp.family_part("rotation", 300, 13, 0.0, noise=0.3, Kr=K)
    rng = np.random.default_rng(5)
    hopeless = (rng.uniform(0, 640, (2, 4)), rng.uniform(0, 480, (2, 4)))
    sets = [[g[0], g[1]], [p[0], p[1]], [rot[0], rot[1]], [hopeless[0], hopeless[1]]]

    def same(a, b):
        return a == b if isinstance(a, (str, list)) else same_bits(np.asarray(a), np.asarray(b))

    for iters in (0, 6):
        plain = _epipolar(P).initialise_pairs(sets, K, refine_iters=iters)
        off = _epipolar(P).initialise_pairs(sets, K, refine_iters=iters, minimal=False)
        assert [set(a) == set(b) and all(same(a[k], b[k]) for k in a) for a, b in zip(plain, off)] == [True] * 4
        ep = _epipolar(P)
        on = ep.initialise_pairs(sets, K, refine_iters=iters, minimal=True)
        assert [o["verdict"] for o in on] == ["general", "degenerate", "degenerate", "none"]
        for a, b in zip(plain[1:], on[1:]):                     # not general: nothing changes
            assert set(a) == set(b) and all(same(a[k], b[k]) for k in a)
        o = on[0]
        ess = hip.essential_ransac([0, 300], g[0], g[1], K, K, 4.0, 128)
        assert o["kind"] == "essential" and same_bits(o["E"], ess["E"][0]) and o["E_inliers"] == np.flatnonzero(ess["inlier"]).tolist()
        assert (o["E_status"], o["E_hypothesis"], o["E_root"]) == (0, ess["best_hyp"][0], ess["best_root"][0])
        assert all(same(o[k], plain[0][k]) for k in ("F", "H", "F_inliers", "H_inliers", "F_status", "H_status", "verdict"))
        R0, t0 = tp.planted("general")
        assert o["best_cand"] >= 0 and np.abs(o["R"] - R0).max() < 0.05 and rr.baseline_angle_deg(o["t"], t0) < 5.0
        assert not set(o["E_inliers"]) & set(np.flatnonzero(g[2]).tolist()) and len(o["E_inliers"]) >= 0.9 * 270
        assert ep.essential_last["status"][0] == 0 and len(ep.essential_last["status"]) == 4
        if iters:
            assert o["refine_status"] == 0 and np.abs(o["R_refined"] - R0).max() < 0.01 and rr.baseline_angle_deg(o["t_refined"], t0) < 1.0
