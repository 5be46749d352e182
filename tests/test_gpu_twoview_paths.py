"""GPU tests of the robust two-view geometry on what the scenes of tests/test_gpu_twoview_ransac.py never reach: eight
families of two-view geometry at three thresholds and 0, 1, 2 and 5 refit rounds (tv.GEOMETRY_CASES), where the reference
shows SFM_TWOVIEW_KEPT_HYPOTHESIS and every number of standing rounds from 0 to 5; ties at the largest count that the pick
must break by the lower h; 259 sets in one call; +inf and a NaN in the second score block.

The rule is the one of the existing tests: tests/test_twoview_ransac_host.py asserts that every set of every case here is
settled in the reference and that the cases reach what they are there for, so decisions compare EXACTLY with no set left
out, and the matrix per set in the G measure at max(1e-9, 100 d_G), d_G from the reference of that very case."""
import itertools

import numpy as np
import pytest

import _twoview_ransac_reference as tv
from _twoview_checks import check_against, run, same_bits, same_sets

pytestmark = pytest.mark.gpu


def _run_case(hip, case, iters=None):
    name, max_err2, max_hyp, case_iters = case
    return run(hip, tv.scene(name), max_hyp, case_iters if iters is None else iters, max_err2)


def _parity(hip, case, worst, unrefined):
    """One case against its reference.  Where the reference kept the hypothesis the device says so, and its matrix is the
    one of the call without refit rounds, bit for bit.  unrefined: that call's matrices per (scene, max_err2, max_hyp)."""
    name, max_err2, max_hyp, iters = case
    sc, ref = tv.case_reference(case)
    got = _run_case(hip, case)
    check_against(ref, *got, where="%s/%g/%d/%d" % case, worst=worst)
    F, status, summary = got[0], got[4], got[5]
    kept = np.flatnonzero(ref.status & tv.KEPT_HYPOTHESIS)
    assert np.array_equal(np.flatnonzero(status & hip.TWOVIEW_KEPT_HYPOTHESIS), kept), case
    assert summary[3] == kept.size
    if kept.size:
        key = (name, max_err2, max_hyp)
        if key not in unrefined:
            unrefined[key] = _run_case(hip, case, iters=0)
        F0, status0 = unrefined[key][0], unrefined[key][4]
        for s in kept:
            assert status0[s] == 0 and status[s] == hip.TWOVIEW_KEPT_HYPOTHESIS, (case, s)
            assert F[s].any() and same_bits(F[s], F0[s]), (case, s)
    return got


# ---- parity with the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tv.FAMILIES))
def test_parity_over_the_geometry_cases(hip, name):
    worst, unrefined, n_kept, stood = {"d_G": 0.0, "device": 0.0}, {}, 0, set()
    cases = [case for case in tv.GEOMETRY_CASES if case[0] == name]
    assert len(cases) == 13
    for case in cases:
        _parity(hip, case, worst, unrefined)
        ref = tv.case_reference(case)[1]
        n_kept += int(ref.summary[3])
        stood |= set(ref.stood[ref.best_hyp >= 0].tolist())
    print("family %s: %d cases, %d sets with the kept hypothesis, standing rounds %s, worst d_G %.3e, worst device difference %.3e"
          % (name, len(cases), n_kept, sorted(stood), worst["d_G"], worst["device"]))


@pytest.mark.parametrize("case", tv.PATH_CASES, ids=[case[0] for case in tv.PATH_CASES])
def test_parity_on_ties_many_sets_and_non_finite_coordinates(hip, case):
    worst = {"d_G": 0.0, "device": 0.0}
    sc, ref = tv.case_reference(case)
    F, inlier, n_in, best, status, summary = _parity(hip, case, worst, {})
    print("scene %s: %d sets, summary %s, worst d_G %.3e, worst device difference %.3e"
          % (case[0], sc.counts.size, summary.tolist(), worst["d_G"], worst["device"]))
    if case[0] == "nonfinite":
        assert status.tolist() == [hip.TWOVIEW_NO_MODEL] * 2 and best.tolist() == [-1, -1] and n_in.tolist() == [0, 0]
        assert same_bits(F, np.zeros((2, 3, 3))) and not inlier.any() and summary.tolist() == [0, 2, 0, 0, 0, 0]


# ---- a set's bits depend on its own matches and the options only --------------------------------------------------------
def test_batch_independence_across_the_families(hip):
    parts = [tv.set_of(tv.scene(name), 1) for name in tv.FAMILIES]                # the 130 matches of every family
    sc = tv._batch([(l, r, np.zeros(l.shape[1], dtype=bool)) for l, r in parts])
    max_err2, iters = 16.0, 5
    whole = run(hip, sc, 128, iters, max_err2)
    n_sets = sc.counts.size
    for s in range(n_sets):
        same_sets(hip, sc, whole, [s], 128, "alone", iters, max_err2)
    same_sets(hip, sc, whole, np.random.default_rng(5).permutation(n_sets).tolist(), 128, "permuted", iters, max_err2)
    # each set is its family's own: the call of the family's scene gives the same bits too
    for s, name in enumerate(tv.FAMILIES):
        own = run(hip, tv.scene(name), 128, iters, max_err2)
        assert same_bits(own[0][1], whole[0][s]) and (own[2][1], own[3][1], own[4][1]) == (whole[2][s], whole[3][s], whole[4][s])


def test_batch_independence_of_many_sets(hip):
    case = tv.PATH_CASES[1]
    sc, ref = tv.case_reference(case)
    whole = _run_case(hip, case)
    n_sets = sc.counts.size
    kept = np.flatnonzero(ref.status & tv.KEPT_HYPOTHESIS).tolist()
    # the first and the last set, a set of every size from the middle, a set that kept its hypothesis, the one before the last
    taken = [0, n_sets - 1] + list(range(126, 132)) + kept[:1] + [n_sets - 2]
    assert set(sc.counts[taken].tolist()) == set(tv.MANY_SIZES)
    for s in taken:
        same_sets(hip, sc, whole, [s], case[2], "alone", case[3], case[1])
    same_sets(hip, sc, whole, taken, case[2], "taken out together", case[3], case[1])
    same_sets(hip, sc, whole, list(range(n_sets - 1, -1, -1)), case[2], "reversed", case[3], case[1])


# ---- the _dev form and the optional outputs where a hypothesis is kept ---------------------------------------------------
def _kept_case(iters=None, max_err2=None, other_than=()):
    """The first geometry case in which the reference keeps a hypothesis (and, if there is one, also finds no model)."""
    found = None
    for case in tv.GEOMETRY_CASES:
        if case[0] in other_than or (iters is not None and case[3] != iters) or (max_err2 is not None and case[1] != max_err2):
            continue
        ref = tv.case_reference(case)[1]
        if ref.summary[3] > 0 and ref.summary[1] > 0:
            return case
        if ref.summary[3] > 0 and found is None:
            found = case
    assert found is not None
    return found


def test_every_subset_of_the_optional_outputs_on_a_kept_hypothesis(hip):
    case = _kept_case()
    name, max_err2, max_hyp, iters = case
    sc, ref = tv.case_reference(case)
    assert ref.summary[3] > 0 and ref.summary[1] > 0
    full = _run_case(hip, case)
    check_against(ref, *full, where="%s/%g/%d/%d" % case)
    assert full[5][3] == ref.summary[3] and np.array_equal(full[4] & hip.TWOVIEW_KEPT_HYPOTHESIS, ref.status & tv.KEPT_HYPOTHESIS)
    names = hip.TWOVIEW_OUTPUTS
    for k in range(len(names) + 1):
        for outputs in itertools.combinations(names, k):
            got = hip.twoview_ransac(sc.set_ptr, sc.left, sc.right, max_err2, max_hyp, iters, outputs=outputs)
            assert same_bits(got[0], full[0]), outputs
            for i, out in enumerate(names):
                if out in outputs:
                    assert same_bits(got[1 + i], full[1 + i]), (outputs, out)
                else:
                    assert got[1 + i] is None


def test_dev_form_on_a_kept_hypothesis(hip):
    import torch
    case = _kept_case()
    name, max_err2, max_hyp, iters = case
    sc, ref = tv.case_reference(case)
    want = _run_case(hip, case)
    S, M = sc.counts.size, sc.left.shape[1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_left, d_right = torch.from_numpy(sc.left).cuda(), torch.from_numpy(sc.right).cuda()
        d_F = torch.full((S, 9), 7.0, dtype=torch.float64, device="cuda")
        d_in = torch.full((M,), 9, dtype=torch.uint8, device="cuda")
        d_n, d_best, d_st = (torch.full((S,), -5, dtype=torch.int32, device="cuda") for _ in range(3))
        d_sum = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        stream.synchronize()
        hip.twoview_ransac_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), max_err2, max_hyp, iters, d_F.data_ptr(),
                               d_in.data_ptr(), d_n.data_ptr(), d_best.data_ptr(), d_st.data_ptr(), d_sum.data_ptr(),
                               stream.cuda_stream)
        got = [t.cpu().numpy() for t in (d_F, d_in, d_n, d_best, d_st, d_sum)]
        # the status and the summary alone, then the matrix alone: every other buffer stays as it is
        d_st2 = torch.full((S,), -5, dtype=torch.int32, device="cuda")
        d_sum2 = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        d_F2 = torch.zeros((S, 9), dtype=torch.float64, device="cuda")
        d_F3 = torch.zeros((S, 9), dtype=torch.float64, device="cuda")
        stream.synchronize()
        hip.twoview_ransac_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), max_err2, max_hyp, iters, d_F2.data_ptr(),
                               d_status=d_st2.data_ptr(), d_summary=d_sum2.data_ptr(), stream=stream.cuda_stream)
        hip.twoview_ransac_dev(sc.set_ptr, M, d_left.data_ptr(), d_right.data_ptr(), max_err2, max_hyp, iters, d_F3.data_ptr(),
                               stream=stream.cuda_stream)
        assert same_bits(d_st2.cpu().numpy(), got[4]) and same_bits(d_sum2.cpu().numpy(), got[5])
        assert same_bits(d_F2.cpu().numpy(), got[0]) and same_bits(d_F3.cpu().numpy(), got[0])
    got[0] = got[0].reshape(S, 3, 3)
    for a, b in zip(got, want):
        assert same_bits(a, b)
    assert np.array_equal(got[4], ref.status) and got[5][3] == ref.summary[3] > 0


# ---- the Python entry points ---------------------------------------------------------------------------------------------
def _pairs(sc, s):
    l, r = tv.set_of(sc, s)
    one = np.ones((1, l.shape[1]))
    return [np.vstack((l, one)), np.vstack((r, one))]


def test_entry_points_on_a_kept_hypothesis_and_on_two_motions(hip, sfm):
    P = sfm.processors
    max_err2, iters = 4.0, 2                                    # max_sampson_px = 2
    kept_case = _kept_case(iters, max_err2, other_than=("two_motions",))
    sc_k, ref_k = tv.case_reference(kept_case)
    s_k = int(np.flatnonzero(ref_k.status & tv.KEPT_HYPOTHESIS)[0])
    sc_m, ref_m = tv.case_reference(("two_motions", max_err2, 128, iters))
    s_m = 1
    chosen = [(sc_k, ref_k, s_k), (sc_m, ref_m, s_m)]
    ep = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
    out = ep.verify_matches([_pairs(sc, s) for sc, _ref, s in chosen], 2.0, 128, iters)
    assert ep.twoview_last["hypothesis"] == [int(ref.best_hyp[s]) for _sc, ref, s in chosen]
    assert ep.twoview_last["status"] == [int(ref.status[s]) for _sc, ref, s in chosen]
    assert ep.twoview_last["status"][0] & hip.TWOVIEW_KEPT_HYPOTHESIS
    n_kept = sum(int(ref.status[s] & tv.KEPT_HYPOTHESIS != 0) for _sc, ref, s in chosen)
    assert ep.twoview_last["summary"][0] == 2 and ep.twoview_last["summary"][3] == n_kept
    for (sc, ref, s), (F, idx, status) in zip(chosen, out):
        lo, hi = sc.set_ptr[s], sc.set_ptr[s + 1]
        assert status == ref.status[s] and idx == np.flatnonzero(ref.inlier[lo:hi]).tolist()
        assert tv.g_difference(F, ref.F[s], ref.c[s]) <= max(1e-9, 100.0 * ref.d_G[s])
        alone = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
        assert alone.determine_fundamental_mat_robust(_pairs(sc, s), 2.0, 128, iters) == idx
        assert alone.twoview_last["status"] == ref.status[s] and alone.twoview_last["hypothesis"] == ref.best_hyp[s]
        assert alone.twoview_last["summary"][3] == int(ref.status[s] & tv.KEPT_HYPOTHESIS != 0)
        assert alone.fund_mat[2][2] == 1.0 and same_bits(alone.fund_mat, F / F[2][2])
