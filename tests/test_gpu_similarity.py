"""GPU tests of the robust similarity: sfm_similarity_ransac, its _dev form and the Python entry point, against the float64
NumPy reference of tests/_similarity_reference.py.

Decisions (status, best_hyp, n_inliers, the mask, the summary) are compared EXACTLY: tests/test_similarity_host.py asserts that
every set of every case used here is settled in the reference, so nothing is left out.  The model is compared per set in the
measure max(|ds| / s, max |dA|, |dt| / extent) at max(1e-9, 100 d_S), d_S being the reference's own spread of the final model
over its two routes and three thresholds: the bound comes from the reference alone -- also where the targets lie a million
units from the origin."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import _similarity_reference as sr
from _twoview_checks import same_bits

pytestmark = pytest.mark.gpu

_WORST = {"d_S": 0.0, "device": 0.0}


def run(hip, sc, max_hyp=128, iters=sr.ITERS, max_err2=sr.MAX_ERR2, rigid=False):
    return hip.similarity_ransac(sc.set_ptr, sc.src, sc.dst, max_err2, max_hyp, iters, rigid)


def is_rotation(A):
    """verify_rotation of csrc/sfm_math.h: the one-sided test of the reference."""
    return np.linalg.det(A) - 1 < 1e-8 and not np.any(np.linalg.inv(A) - A.T > 1e-8)


def check_against(ref, sim, inlier, n_in, best, status, summary, where=""):
    """Exact decisions, models at the per-set bound, sets without a model as thirteen zeros."""
    assert ref.settled.all()
    assert np.array_equal(status, ref.status), where
    assert np.array_equal(best, ref.best_hyp), where
    assert np.array_equal(n_in, ref.n_inliers), where
    assert np.array_equal(inlier, ref.inlier), where
    assert np.array_equal(summary, ref.summary), where
    solved = ref.best_hyp >= 0
    for k in np.flatnonzero(solved):
        diff = sr.sim_difference(sim[k], ref.sim[k], ref.ext[k])
        _WORST["d_S"] = max(_WORST["d_S"], ref.d_S[k]); _WORST["device"] = max(_WORST["device"], diff)
        print(where, "set", k, "d_S %.3e device %.3e" % (ref.d_S[k], diff))
        assert diff <= max(1e-9, 100.0 * ref.d_S[k]), (where, k, diff, ref.d_S[k])
        assert sim[k, 0] > 0 and is_rotation(sim[k, 1:10].reshape(3, 3)), (where, k)
    assert same_bits(sim[~solved], np.zeros_like(sim[~solved])), where
    print("worst d_S %.3e, worst device difference %.3e so far" % (_WORST["d_S"], _WORST["device"]))


def subset(sc, sets):
    parts = [sr.set_of(sc, k) for k in sets]
    counts = [p[0].shape[1] for p in parts]
    return SimpleNamespace(set_ptr=np.concatenate(([0], np.cumsum(counts))).astype(np.int32),
                           src=np.ascontiguousarray(np.hstack([p[0] for p in parts])), dst=np.ascontiguousarray(np.hstack([p[1] for p in parts])))


def same_sets(hip, sc, whole, sets, max_hyp, what):
    """The sets `sets` of the scene in a call of their own give the bits they have in `whole`, the result of the whole scene."""
    sub = subset(sc, sets)
    sim, inlier, n_in, best, status, _summary = run(hip, sub, max_hyp)
    for k, s in enumerate(sets):
        assert same_bits(sim[k], whole[0][s]), (what, s)
        assert same_bits(inlier[sub.set_ptr[k]:sub.set_ptr[k + 1]], whole[1][sc.set_ptr[s]:sc.set_ptr[s + 1]]), (what, s)
        assert (n_in[k], best[k], status[k]) == (whole[2][s], whole[3][s], whole[4][s]), (what, s)


# ---- parity with the reference on every case: set sizes 4 .. 2 049, max_hyp 1 .. 1 000, iters 0 and 3, rigid, 259 sets,
# ---- empty sets and sets below four between others, ties, targets a million units away --------------------------------------
@pytest.mark.parametrize("case", sr.CASES, ids=sr.case_id)
def test_parity_with_the_reference(hip, case):
    name, max_err2, max_hyp, iters, rigid = case
    sc, ref = sr.case_reference(case)
    got = run(hip, sc, max_hyp, iters, max_err2, rigid)
    check_against(ref, *got, where=sr.case_id(case))
    if rigid:
        assert np.all(got[0][:, 0] == 1.0)
    if iters == 0:
        assert not (got[4] & hip.SIMILARITY_KEPT_HYPOTHESIS).any()
    if name == "kept":                                         # no round stood: the model is the winning hypothesis itself
        assert got[4].tolist() == [hip.SIMILARITY_KEPT_HYPOTHESIS] * 2
        assert all(same_bits(a, b) for a, b in zip(run(hip, sc, max_hyp, 0, max_err2)[:4], got[:4]))


def test_degenerate_sets_bit_for_bit(hip):
    sc, ref = sr.scene_and_reference("degenerate")
    sim, inlier, n_in, best, status, summary = run(hip, sc)
    # all src on one line, all src identical: no model, thirteen zeros; a NaN row in dst: never an inlier
    assert status.tolist() == [hip.SIMILARITY_NO_MODEL, hip.SIMILARITY_NO_MODEL, 0] and best[:2].tolist() == [-1, -1]
    assert same_bits(sim[:2], np.zeros((2, 13))) and n_in.tolist() == [0, 0, 59]
    lo = int(sc.set_ptr[2])
    assert not inlier[:lo].any() and inlier[lo + 17] == 0 and inlier[lo:].sum() == 59
    assert summary.tolist() == [1, 2, 0, 0, 59, 1]
    again = run(hip, sc)
    assert all(same_bits(a, b) for a, b in zip(again, (sim, inlier, n_in, best, status, summary)))


def test_a_tie_goes_to_the_lower_hypothesis(hip):
    sc, ref = sr.scene_and_reference("ties", 1000, sr.ITERS, sr.EVERYONE)
    got = run(hip, sc, 1000, 0, sr.EVERYONE)
    assert np.array_equal(got[3], ref.best_hyp) and np.array_equal(got[2], sc.counts)
    for k in range(2):                  # the winner is the first hypothesis that counts the whole set: none below it is valid
        a, b = sr.set_of(sc, k)
        hyp = sr._hypotheses(a, b, 1000, 0, False)
        counts = sr._counts(hyp, sr.err2(hyp[1], hyp[2], hyp[3], a, b), sr.EVERYONE)
        assert got[3][k] == int(np.flatnonzero(counts == a.shape[1])[0])


def test_too_few_and_an_empty_call(hip):
    sc = sr.scene("proto")
    few = hip.similarity_ransac([0, 3], sc.src[:, :3], sc.dst[:, :3], sr.MAX_ERR2)
    assert few[4].tolist() == [hip.SIMILARITY_TOO_FEW] and few[5].tolist() == [0, 0, 1, 0, 0, 0] and same_bits(few[0], np.zeros((1, 13)))
    assert few[3].tolist() == [-1] and few[2].tolist() == [0] and not few[1].any()
    none = hip.similarity_ransac([0], np.zeros((3, 0)), np.zeros((3, 0)), sr.MAX_ERR2)
    assert none[0].shape == (0, 13) and not none[5].any()
    empty = hip.similarity_ransac([0, 0, 0], np.zeros((3, 0)), np.zeros((3, 0)), sr.MAX_ERR2)
    assert empty[4].tolist() == [hip.SIMILARITY_TOO_FEW] * 2 and empty[5].tolist() == [0, 0, 2, 0, 0, 0]


def test_the_refit_never_loses_inliers(hip):
    sc = sr.scene("paths")
    got = run(hip, sc, 128, 0)
    counts = [got[2]]
    for iters in (1, 2, 5):
        more = run(hip, sc, 128, iters)
        assert np.array_equal(more[3], got[3])                 # the winner does not depend on the refit
        counts.append(more[2])
    assert all(np.all(b >= a) for a, b in zip(counts, counts[1:]))     # a round stands only with at least the standing count


# ---- a set's bits depend on its own correspondences and the options only ------------------------------------------------
@pytest.mark.parametrize("max_hyp", [65, 128])
def test_batch_independence_and_run_to_run_equality(hip, max_hyp):
    sc = sr.scene("paths")
    whole = run(hip, sc, max_hyp)
    assert all(same_bits(a, b) for a, b in zip(run(hip, sc, max_hyp), whole))
    n_sets = sc.counts.size
    for s in sr.ALONE:                                         # 4, 63, 65, 1 025 and 2 049 correspondences, alone
        same_sets(hip, sc, whole, [s], max_hyp, "alone")
    same_sets(hip, sc, whole, np.random.default_rng(3).permutation(n_sets).tolist(), max_hyp, "permuted")
    same_sets(hip, sc, whole, [s for s in range(n_sets) if sc.counts[s] <= 100], max_hyp, "without the long sets")


# ---- the _dev form ------------------------------------------------------------------------------------------------------
def test_dev_form_on_a_callers_stream(hip):
    import torch
    sc = sr.scene("paths")
    want = run(hip, sc, 65)
    S, M = sc.counts.size, sc.src.shape[1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_src, d_dst = torch.from_numpy(sc.src).cuda(), torch.from_numpy(sc.dst).cuda()
        d_sim = torch.full((S, 13), 7.0, dtype=torch.float64, device="cuda")
        d_in = torch.full((M,), 9, dtype=torch.uint8, device="cuda")
        d_n, d_best, d_st = (torch.full((S,), -5, dtype=torch.int32, device="cuda") for _ in range(3))
        d_sum = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        stream.synchronize()
        hip.similarity_ransac_dev(sc.set_ptr, M, d_src.data_ptr(), d_dst.data_ptr(), sr.MAX_ERR2, 65, sr.ITERS, False, d_sim.data_ptr(),
                                  d_in.data_ptr(), d_n.data_ptr(), d_best.data_ptr(), d_st.data_ptr(), d_sum.data_ptr(),
                                  stream.cuda_stream)
        got = [t.cpu().numpy() for t in (d_sim, d_in, d_n, d_best, d_st, d_sum)]
        assert same_bits(d_src.cpu().numpy(), sc.src) and same_bits(d_dst.cpu().numpy(), sc.dst)
        # only the model asked for: every other buffer stays as it is
        d_sim2 = torch.zeros((S, 13), dtype=torch.float64, device="cuda")
        stream.synchronize()
        hip.similarity_ransac_dev(sc.set_ptr, M, d_src.data_ptr(), d_dst.data_ptr(), sr.MAX_ERR2, 65, sr.ITERS, False, d_sim2.data_ptr(),
                                  stream=stream.cuda_stream)
        assert same_bits(d_sim2.cpu().numpy(), got[0])
        assert all(same_bits(t.cpu().numpy(), g) for t, g in zip((d_in, d_n, d_best, d_st, d_sum), got[1:]))
    for a, b in zip(got, want):
        assert same_bits(a, b)


# ---- every subset of the optional outputs -------------------------------------------------------------------------------
def test_every_subset_of_the_optional_outputs(hip):
    sc = subset(sr.scene("paths"), [1, 3, 6, 4])              # 4, 3, 65 and 63 correspondences
    full = hip.similarity_ransac(sc.set_ptr, sc.src, sc.dst, sr.MAX_ERR2, 65)
    names = hip.SIMILARITY_OUTPUTS
    for k in range(len(names) + 1):
        for chosen in itertools.combinations(names, k):
            got = hip.similarity_ransac(sc.set_ptr, sc.src, sc.dst, sr.MAX_ERR2, 65, outputs=chosen)
            assert same_bits(got[0], full[0]), chosen
            for i, name in enumerate(names):
                if name in chosen:
                    assert same_bits(got[1 + i], full[1 + i]), (chosen, name)
                else:
                    assert got[1 + i] is None
