"""GPU tests of the robust homography: sfm_homography_ransac, its _dev form and the Python entry points, against the float64
NumPy reference of tests/_homography_reference.py.

Decisions (status, best_hyp, n_inliers, the mask, the summary) are compared EXACTLY: tests/test_homography_host.py asserts that
every set of every scene used here is settled in the reference at every setting used, so nothing is left out.  The matrix is
compared per set in the measure D^-1 H D / |D^-1 H D| at max(1e-9, 100 d_H), d_H being the reference's own spread of the final
matrix over its two null-vector routes and three thresholds: the bound comes from the reference alone."""
import itertools

import numpy as np
import pytest

import _homography_reference as hg
import _twoview_ransac_reference as tv
from _twoview_checks import same_bits, subset as _subset

pytestmark = pytest.mark.gpu

_WORST = {"d_H": 0.0, "device": 0.0}


def run(hip, sc, max_hyp=128, iters=hg.ITERS, max_err2=hg.MAX_ERR2):
    return hip.homography_ransac(sc.set_ptr, sc.left, sc.right, max_err2, max_hyp, iters)


def check_against(ref, H, inlier, n_in, best, status, summary, where=""):
    """Exact decisions, matrices at the per-set bound, sets without a model as nine zeros."""
    assert ref.settled.all()
    assert np.array_equal(status, ref.status), where
    assert np.array_equal(best, ref.best_hyp), where
    assert np.array_equal(n_in, ref.n_inliers), where
    assert np.array_equal(inlier, ref.inlier), where
    assert np.array_equal(summary, ref.summary), where
    solved = ref.best_hyp >= 0
    for s in np.flatnonzero(solved):
        diff = hg.h_difference(H[s], ref.H[s], ref.c[s])
        if ref.d_H[s] < 1e-3:                                  # (the collinear set: a family of matrices explains it)
            _WORST["d_H"] = max(_WORST["d_H"], ref.d_H[s]); _WORST["device"] = max(_WORST["device"], diff)
        print(where, "set", s, "d_H %.3e device %.3e" % (ref.d_H[s], diff))
        assert diff <= max(1e-9, 100.0 * ref.d_H[s]), (where, s, diff, ref.d_H[s])
        assert abs(np.linalg.norm(H[s]) - 1.0) < 1e-14 and H[s].flat[np.argmax(np.abs(H[s]))] > 0
    assert not H[~solved].any() and same_bits(H[~solved], np.zeros_like(H[~solved])), where
    print("worst d_H %.3e, worst device difference %.3e so far" % (_WORST["d_H"], _WORST["device"]))


def same_sets(hip, sc, whole, sets, max_hyp, what):
    """The sets `sets` of the scene in a call of their own give the bits they have in `whole`, the result of the whole scene."""
    sub = _subset(sc, sets)
    H, inlier, n_in, best, status, _summary = run(hip, sub, max_hyp)
    for k, s in enumerate(sets):
        assert same_bits(H[k], whole[0][s]), (what, s)
        assert same_bits(inlier[sub.set_ptr[k]:sub.set_ptr[k + 1]], whole[1][sc.set_ptr[s]:sc.set_ptr[s + 1]]), (what, s)
        assert (n_in[k], best[k], status[k]) == (whole[2][s], whole[3][s], whole[4][s]), (what, s)


# ---- parity with the reference on every case --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hg.CASES + hg.PATH_CASES, ids=lambda c: "%s-%g-%d-%d" % c)
def test_parity_with_the_reference(hip, case):
    name, max_err2, max_hyp, iters = case
    sc, ref = hg.case_reference(case)
    check_against(ref, *run(hip, sc, max_hyp, iters, max_err2), where="%s/%g/%d/%d" % case)


@pytest.mark.parametrize("name", list(hg.FAMILIES))
def test_parity_on_the_geometry_families(hip, name):
    sc = hg.scene(name)
    for case in hg.GEOMETRY_CASES:
        if case[0] == name:
            _name, max_err2, max_hyp, iters = case
            check_against(hg.case_reference(case)[1], *run(hip, sc, max_hyp, iters, max_err2), where="%s/%g/%d/%d" % case)


def test_degenerate_sets_bit_for_bit(hip):
    sc, ref = hg.scene_and_reference("degenerate")
    H, inlier, n_in, best, status, summary = run(hip, sc)
    assert status.tolist() == [0, hip.HOMOGRAPHY_NO_MODEL, hip.HOMOGRAPHY_NO_MODEL] and best.tolist() == [0, -1, -1]
    assert same_bits(H[1:], np.zeros((2, 3, 3))) and n_in.tolist() == [sc.counts[0], 0, 0]
    assert inlier[:sc.set_ptr[1]].all() and not inlier[sc.set_ptr[1]:].any()
    assert summary.tolist() == [1, 2, 0, 0, sc.counts[0], 0]
    again = run(hip, sc)
    assert all(same_bits(a, b) for a, b in zip(again, (H, inlier, n_in, best, status, summary)))


def test_four_matches_and_an_empty_call(hip):
    sc = hg.scene("proto0")
    few = hip.homography_ransac([0, 4], sc.left[:, :4], sc.right[:, :4], hg.MAX_ERR2)
    assert few[4].tolist() == [hip.HOMOGRAPHY_TOO_FEW] and few[5].tolist() == [0, 0, 1, 0, 0, 0] and not few[0].any()
    assert few[3].tolist() == [-1] and few[2].tolist() == [0] and not few[1].any()
    none = hip.homography_ransac([0], np.zeros((2, 0)), np.zeros((2, 0)), hg.MAX_ERR2)
    assert none[0].shape == (0, 3, 3) and not none[5].any()


def test_the_c_entry_points_refuse_what_the_header_says(hip):
    """SFM_E_SHAPE from the library itself, past the Python checks, and the output untouched."""
    lib = hip.load()
    left = np.zeros((2, 5))
    H = np.full(9, 7.0)
    good = np.array([0, 5], dtype=np.int32)

    def call(ptr=good, n_sets=1, M=5, max_err2=4.0, max_hyp=128, iters=2):
        ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        return lib.sfm_homography_ransac(n_sets, hip.iptr(ptr), M, hip.dptr(left), hip.dptr(left), max_err2, max_hyp, iters,
                                         hip.dptr(H), None, None, None, None, None)

    for kw in (dict(max_err2=float("nan")), dict(max_err2=-1.0), dict(max_hyp=-1), dict(max_hyp=65537), dict(iters=-1),
               dict(ptr=[1, 5]), dict(ptr=[0, 3, 2, 5], n_sets=3), dict(ptr=[0, 4]), dict(n_sets=-1), dict(M=-1)):
        assert call(**kw) == hip.E_SHAPE, kw
    assert np.all(H == 7.0)


def test_no_refit_rounds(hip):
    sc, ref = hg.scene_and_reference("paths", 128, 0)
    got = run(hip, sc, 128, 0)
    check_against(ref, *got, where="paths/128 iters 0")
    assert not (got[4] & hip.HOMOGRAPHY_KEPT_HYPOTHESIS).any()
    counts = [got[2]]
    for iters in (1, 2, 5):
        more = run(hip, sc, 128, iters)
        assert np.array_equal(more[3], got[3])                 # the winner does not depend on the refit
        counts.append(more[2])
    assert all(np.all(b >= a) for a, b in zip(counts, counts[1:]))     # a round stands only with at least the standing count


# ---- a set's bits depend on its own matches and the options only --------------------------------------------------------
@pytest.mark.parametrize("max_hyp", [65, 128])
def test_batch_independence_bit_for_bit(hip, max_hyp):
    sc = hg.scene("paths")
    whole = run(hip, sc, max_hyp)
    n_sets = sc.counts.size
    alone = [int(np.flatnonzero(sc.counts == n)[0]) for n in hg.ALONE]
    assert sc.counts[alone].tolist() == list(hg.ALONE)
    for s in alone:                                            # 5, 63, 65, 257, 1 025 and 5 000 matches, alone
        same_sets(hip, sc, whole, [s], max_hyp, "alone")
    same_sets(hip, sc, whole, np.random.default_rng(3).permutation(n_sets).tolist(), max_hyp, "permuted")
    same_sets(hip, sc, whole, [s for s in range(n_sets) if sc.counts[s] <= hg.LONG], max_hyp, "without the long sets")


# ---- the _dev form ------------------------------------------------------------------------------------------------------
def test_dev_form_on_a_callers_stream(hip):
    import torch
    sc = hg.scene("paths")
    want = run(hip, sc, 65)
    S, M = sc.counts.size, sc.left.shape[1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_left, d_right = torch.from_numpy(sc.left).cuda(), torch.from_numpy(sc.right).cuda()
        d_H = torch.full((S, 9), 7.0, dtype=torch.float64, device="cuda")
        d_in = torch.full((M,), 9, dtype=torch.uint8, device="cuda")
        d_n, d_best, d_st = (torch.full((S,), -5, dtype=torch.int32, device="cuda") for _ in range(3))
        d_sum = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        stream.synchronize()
        hip.homography_ransac_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), hg.MAX_ERR2, 65, hg.ITERS, d_H.data_ptr(),
                                  d_in.data_ptr(), d_n.data_ptr(), d_best.data_ptr(), d_st.data_ptr(), d_sum.data_ptr(),
                                  stream.cuda_stream)
        got = [t.cpu().numpy() for t in (d_H, d_in, d_n, d_best, d_st, d_sum)]
        assert same_bits(d_left.cpu().numpy(), sc.left) and same_bits(d_right.cpu().numpy(), sc.right)
        # only the matrix asked for: every other buffer stays as it is
        d_H2 = torch.zeros((S, 9), dtype=torch.float64, device="cuda")
        stream.synchronize()
        hip.homography_ransac_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), hg.MAX_ERR2, 65, hg.ITERS, d_H2.data_ptr(),
                                  stream=stream.cuda_stream)
        assert same_bits(d_H2.cpu().numpy(), got[0])
        assert all(same_bits(t.cpu().numpy(), g) for t, g in zip((d_in, d_n, d_best, d_st, d_sum), got[1:]))
    got[0] = got[0].reshape(S, 3, 3)
    for a, b in zip(got, want):
        assert same_bits(a, b)


# ---- every subset of the optional outputs -------------------------------------------------------------------------------
def test_every_subset_of_the_optional_outputs(hip):
    sc = _subset(hg.scene("paths"), [1, 4, 9, 11])            # 4, 15, 65 and 256 matches
    full = hip.homography_ransac(sc.set_ptr, sc.left, sc.right, hg.MAX_ERR2, 65)
    names = hip.HOMOGRAPHY_OUTPUTS
    for k in range(len(names) + 1):
        for subset in itertools.combinations(names, k):
            got = hip.homography_ransac(sc.set_ptr, sc.left, sc.right, hg.MAX_ERR2, 65, outputs=subset)
            assert same_bits(got[0], full[0]), subset
            for i, name in enumerate(names):
                if name in subset:
                    assert same_bits(got[1 + i], full[1 + i]), (subset, name)
                else:
                    assert got[1 + i] is None


# ---- the mixin ----------------------------------------------------------------------------------------------------------
def _pairs(sc, s, count=None):
    lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
    hi = hi if count is None else lo + count
    one = np.ones((1, hi - lo))
    return [np.vstack((sc.left[:, lo:hi], one)), np.vstack((sc.right[:, lo:hi], one))]


def test_determine_homography_robust(hip, sfm):
    P = sfm.processors
    sc, ref = hg.scene_and_reference("proto1")
    ep = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
    assert same_bits(ep.homography, np.identity(3))
    idx = ep.determine_homography_robust(_pairs(sc, 1))
    lo, hi = sc.set_ptr[1], sc.set_ptr[2]
    assert idx == np.flatnonzero(ref.inlier[lo:hi]).tolist()
    assert ep.homography_last["hypothesis"] == ref.best_hyp[1] and ep.homography_last["status"] == ref.status[1]
    H = run(hip, _subset(sc, [1]))[0][0]
    assert ep.homography[2][2] == 1.0 and same_bits(ep.homography, H / H[2][2])
    assert hg.h_difference(ep.homography, ref.H[1], ref.c[1]) <= max(1e-9, 100.0 * ref.d_H[1])
    before = ep.homography.copy()
    assert ep.determine_homography_robust(_pairs(sc, 0, 4)) == [] and same_bits(ep.homography, before)
    assert ep.homography_last["status"] == hip.HOMOGRAPHY_TOO_FEW and ep.homography_last["hypothesis"] == -1


def test_classify_matches_against_the_reference_verdicts(hip, sfm):
    P = sfm.processors
    scenes = [hg.scene(name) for name in ("plane", "rotation", "general")]
    sets = [_pairs(sc, 2) for sc in scenes] + [_pairs(scenes[0], 2, 4)]      # 300 matches each, and a set of four
    want = []
    for name in ("plane", "rotation", "general"):
        sc, href = hg.scene_and_reference(name)
        l, r = hg.set_of(sc, 2)
        fref = tv.reference([0, l.shape[1]], l, r, hg.MAX_ERR2, 128, hg.ITERS)
        want.append((hg.verdict(href.n_inliers[2], href.best_hyp[2] >= 0, fref.n_inliers[0], fref.best_hyp[0] >= 0),
                     np.flatnonzero(href.inlier[sc.set_ptr[2]:sc.set_ptr[3]]).tolist()))
    assert [w[0] for w in want] == ["degenerate", "degenerate", "general"]
    ep = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
    out = ep.classify_matches(sets)
    assert [o["verdict"] for o in out] == ["degenerate", "degenerate", "general", "none"]
    for o, (_v, h_idx) in zip(out, want):
        assert o["H_inliers"] == h_idx and o["H_status"] in (0, hip.HOMOGRAPHY_KEPT_HYPOTHESIS)
    assert out[3]["H_status"] == hip.HOMOGRAPHY_TOO_FEW and out[3]["F_status"] == hip.TWOVIEW_TOO_FEW
    assert not out[3]["H"].any() and not out[3]["F"].any() and out[3]["H_inliers"] == [] == out[3]["F_inliers"]
    assert len(ep.homography_last["hypothesis"]) == 4 and len(ep.twoview_last["status"]) == 4
    verified = ep.verify_matches(sets)                          # the fundamental half is verify_matches' bit for bit
    for o, (F, idx, status) in zip(out, verified):
        assert same_bits(o["F"], F) and o["F_inliers"] == idx and o["F_status"] == status
