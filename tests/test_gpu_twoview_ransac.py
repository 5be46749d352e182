"""GPU tests of the robust two-view geometry: sfm_twoview_ransac, its _dev form and the Python entry points, against the
float64 NumPy reference of tests/_twoview_ransac_reference.py.

Decisions (status, best_hyp, n_inliers, the mask, the summary) are compared EXACTLY: tests/test_twoview_ransac_host.py asserts
that every set of every scene used here is settled in the reference at every max_hyp used, so nothing is left out.  The
matrix is compared per set in the G measure at max(1e-9, 100 d_G), d_G being the reference's own spread of the final matrix
over its two null-vector routes and three thresholds: the bound comes from the reference alone."""
import itertools
import random

import numpy as np
import pytest

import _twoview_ransac_reference as tv
from _twoview_checks import check_against, run, same_bits, same_sets as _same_sets, subset as _subset

pytestmark = pytest.mark.gpu

_WORST = {"d_G": 0.0, "device": 0.0}


# ---- parity with the reference: prototype scenes, the paths scene at every max_hyp, the degenerate sets ------------------
@pytest.mark.parametrize("name,max_hyp", tv.CASES)
def test_parity_with_the_reference(hip, name, max_hyp):
    sc, ref = tv.scene_and_reference(name, max_hyp)
    got = run(hip, sc, max_hyp)
    check_against(ref, *got, where="%s/%d" % (name, max_hyp), worst=_WORST)
    print("worst d_G %.3e, worst device difference %.3e so far" % (_WORST["d_G"], _WORST["device"]))


def test_degenerate_sets_bit_for_bit(hip):
    sc, ref = tv.scene_and_reference("degenerate")
    F, inlier, n_in, best, status, summary = run(hip, sc)
    assert status.tolist() == [0, hip.TWOVIEW_NO_MODEL, hip.TWOVIEW_NO_MODEL] and best.tolist()[1:] == [-1, -1]
    assert same_bits(F[1:], np.zeros((2, 3, 3))) and n_in.tolist() == [sc.counts[0], 0, 0]
    assert inlier[:sc.set_ptr[1]].all() and not inlier[sc.set_ptr[1]:].any()
    assert summary.tolist() == [1, 2, 0, 0, sc.counts[0], 0]
    again = run(hip, sc)
    assert all(same_bits(a, b) for a, b in zip(again, (F, inlier, n_in, best, status, summary)))
    # a set of eight matches, and an empty call
    few = hip.twoview_ransac([0, 8], sc.left[:, :8], sc.right[:, :8], tv.MAX_ERR2)
    assert few[4].tolist() == [hip.TWOVIEW_TOO_FEW] and few[5].tolist() == [0, 0, 1, 0, 0, 0] and not few[0].any()
    none = hip.twoview_ransac([0], np.zeros((2, 0)), np.zeros((2, 0)), tv.MAX_ERR2)
    assert none[0].shape == (0, 3, 3) and not none[5].any()


def test_no_refit_rounds(hip):
    sc, ref = tv.scene_and_reference("paths", 128, 0)
    got = run(hip, sc, 128, 0)
    check_against(ref, *got, where="paths/128 iters 0", worst=_WORST)
    assert not (got[4] & hip.TWOVIEW_KEPT_HYPOTHESIS).any()
    full = run(hip, sc, 128)
    assert np.array_equal(full[3], got[3])                    # the winner does not depend on the refit
    assert np.all(full[2] >= got[2])                          # a round stands only with at least the standing count


# ---- a set's bits depend on its own matches and the options only --------------------------------------------------------
@pytest.mark.parametrize("max_hyp", [65, 128])
def test_batch_independence_bit_for_bit(hip, max_hyp):
    sc = tv.scene("paths")
    whole = run(hip, sc, max_hyp)
    n_sets = sc.counts.size
    for s in (2, 7, 9, 12, 15, 17):                           # 9, 63, 65, 257, 1 025 and 5 000 matches, alone
        _same_sets(hip, sc, whole, [s], max_hyp, "alone")
    _same_sets(hip, sc, whole, np.random.default_rng(3).permutation(n_sets).tolist(), max_hyp, "permuted")
    _same_sets(hip, sc, whole, [s for s in range(n_sets) if sc.counts[s] <= tv.LONG], max_hyp, "without the long sets")


# ---- the _dev form ------------------------------------------------------------------------------------------------------
def test_dev_form_on_a_callers_stream_in_place(hip):
    import torch
    sc = tv.scene("paths")
    want = run(hip, sc, 65)
    S, M = sc.counts.size, sc.left.shape[1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_left, d_right = torch.from_numpy(sc.left).cuda(), torch.from_numpy(sc.right).cuda()
        d_F = torch.full((S, 9), 7.0, dtype=torch.float64, device="cuda")
        d_in = torch.full((M,), 9, dtype=torch.uint8, device="cuda")
        d_n, d_best, d_st = (torch.full((S,), -5, dtype=torch.int32, device="cuda") for _ in range(3))
        d_sum = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        stream.synchronize()
        hip.twoview_ransac_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), tv.MAX_ERR2, 65, tv.ITERS, d_F.data_ptr(),
                               d_in.data_ptr(), d_n.data_ptr(), d_best.data_ptr(), d_st.data_ptr(), d_sum.data_ptr(),
                               stream.cuda_stream)
        got = [t.cpu().numpy() for t in (d_F, d_in, d_n, d_best, d_st, d_sum)]
        assert same_bits(d_left.cpu().numpy(), sc.left) and same_bits(d_right.cpu().numpy(), sc.right)
        # only the matrix asked for: every other buffer stays as it is
        d_F2 = torch.zeros((S, 9), dtype=torch.float64, device="cuda")
        stream.synchronize()
        hip.twoview_ransac_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), tv.MAX_ERR2, 65, tv.ITERS, d_F2.data_ptr(),
                               stream=stream.cuda_stream)
        assert same_bits(d_F2.cpu().numpy(), got[0])
    got[0] = got[0].reshape(S, 3, 3)
    for a, b in zip(got, want):
        assert same_bits(a, b)


# ---- every subset of the optional outputs -------------------------------------------------------------------------------
def test_every_subset_of_the_optional_outputs(hip):
    sc = _subset(tv.scene("paths"), [1, 4, 9, 11])            # 8, 15, 65 and 256 matches
    full = hip.twoview_ransac(sc.set_ptr, sc.left, sc.right, tv.MAX_ERR2, 65)
    names = hip.TWOVIEW_OUTPUTS
    for k in range(len(names) + 1):
        for subset in itertools.combinations(names, k):
            got = hip.twoview_ransac(sc.set_ptr, sc.left, sc.right, tv.MAX_ERR2, 65, outputs=subset)
            assert same_bits(got[0], full[0]), subset
            for i, name in enumerate(names):
                if name in subset:
                    assert same_bits(got[1 + i], full[1 + i]), (subset, name)
                else:
                    assert got[1 + i] is None


# ---- the Python entry points -------------------------------------------------------------------------------------------
def _pairs(sc, s):
    lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
    one = np.ones((1, hi - lo))
    return [np.vstack((sc.left[:, lo:hi], one)), np.vstack((sc.right[:, lo:hi], one))]


def test_epipolar_processor_entry_points(hip, sfm):
    P = sfm.processors
    sc, ref = tv.scene_and_reference("proto1")
    ep = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
    out = ep.verify_matches([_pairs(sc, 0), _pairs(sc, 1)])
    assert ep.twoview_last["hypothesis"] == ref.best_hyp.tolist() and np.array_equal(ep.twoview_last["summary"], ref.summary)
    for s, (F, idx, status) in enumerate(out):
        lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
        assert idx == np.flatnonzero(ref.inlier[lo:hi]).tolist() and status == ref.status[s]
        assert tv.g_difference(F, ref.F[s], ref.c[s]) <= max(1e-9, 100.0 * ref.d_G[s])
    idx = ep.determine_fundamental_mat_robust(_pairs(sc, 1))
    assert idx == out[1][1] and ep.twoview_last["hypothesis"] == ref.best_hyp[1] and ep.twoview_last["status"] == ref.status[1]
    assert ep.fund_mat[2][2] == 1.0 and same_bits(ep.fund_mat, out[1][0] / out[1][0][2][2])
    ep.extract_essential_mat(tv.K, tv.K)                      # the matrix is in the form the next step expects
    assert np.isfinite(ep.esse_mat).all()
    with pytest.raises(ValueError, match="Insufficient matched pairs : 7"):
        ep.determine_fundamental_mat_robust([np.ones((3, 7)), np.ones((3, 7))])
    before = ep.fund_mat.copy()
    pairs = _pairs(sc, 0)
    assert ep.determine_fundamental_mat_robust([pairs[0][:, :8], pairs[1][:, :8]]) == [] and same_bits(ep.fund_mat, before)
    assert ep.twoview_last["status"] == hip.TWOVIEW_TOO_FEW


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def test_verify_pairs_against_the_host_form(hip, sfm):
    dv = sfm.scenes.make_descriptor_views(n_views=3, n_pts=200, seed=0)
    views = [View(dv.key_pts(v), dv.sift[v]) for v in range(3)]
    kt = sfm.processors.HipDeviceKeyTracker("sift", False, True, False, None)
    try:
        for v in range(3):
            kt.add_new_view(views[v], views[:v])
        for ref_idx, que_idx in ((0, 1), (0, 2), (1, 2)):
            pairs, r_idx, q_idx = kt.generate_matched_pairs(ref_idx, que_idx, views)
            n = r_idx.shape[1]
            assert n >= 9
            down = kt.kt_download_bytes
            got_r, got_q, mask = sfm.processors.verify_pairs(kt, ref_idx, que_idx, 2.0, 128, 2)
            assert kt.kt_download_bytes == down               # the store downloaded nothing on its own account
            F, inlier, _n, best, status, _summary = hip.twoview_ransac([0, n], pairs[0][0:2], pairs[1][0:2], 4.0, 128, 2)
            assert np.array_equal(got_r, r_idx) and np.array_equal(got_q, q_idx)
            assert mask.dtype == bool and np.array_equal(mask, inlier.astype(bool))
            assert same_bits(kt.twoview_last["fund_mat"], F[0])
            assert kt.twoview_last["hypothesis"] == best[0] >= 0 and kt.twoview_last["status"] == status[0]
            assert mask.sum() >= 0.5 * n                      # the scene's true pairs are consistent
        assert sfm.processors.verify_pairs(kt, 0, 3) is None
    finally:
        kt.kt_release()


# ---- ordering: the robust matrix is closer to the clean matches than the reference routine's --------------------------
def _rms_sampson(F, l, r):
    return float(np.sqrt(np.mean(tv.sampson(np.asarray(F, dtype=np.float64), l, r))))


@pytest.mark.parametrize("name", ["proto1", "proto2"])
def test_closer_to_the_clean_matches_than_the_reference_routine(hip, sfm, name):
    P = sfm.processors
    sc = tv.scene(name)
    for s in range(sc.counts.size):
        lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
        clean = ~sc.displaced[lo:hi]
        l, r = sc.left[:, lo:hi], sc.right[:, lo:hi]
        ep = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
        random.seed(1234)
        ep.determine_fundamental_mat(_pairs(sc, s))
        plain = _rms_sampson(ep.fund_mat, l[:, clean], r[:, clean])
        ep.determine_fundamental_mat_robust(_pairs(sc, s))
        robust = _rms_sampson(ep.fund_mat, l[:, clean], r[:, clean])
        print("%s set %d (%d matches): RMS Sampson distance over the clean matches, robust %.4f px, determine_fundamental_mat %.4f px"
              % (name, s, hi - lo, robust, plain))
        assert robust < plain
