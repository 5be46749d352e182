"""Host-side checks of the robust homography (no GPU): the stratified sampler against the NumPy sampler and Python integers,
the argument checks, and the NumPy reference of tests/_homography_reference.py on the scenes the GPU tests use -- EVERY set of
every scene at every setting tests/test_gpu_homography.py uses is settled, so the GPU tests compare decisions exactly and leave
nothing out; the scenes reach what they are there for; and the verdict of processors.classify_matches, taken from the
reference's counts alone, names the plane and the pure rotation "degenerate" and the general scene "general"."""
import numpy as np
import pytest

import _homography_reference as hg
import _twoview_ransac_reference as tv


@pytest.mark.parametrize("max_hyp", [1, 128, 65536])
def test_the_sample_of_every_hypothesis(sfm, max_hyp):
    native = sfm.native
    for n in (5, 6, 7, 8, 9, 17, 64, 363, 1 << 20):
        want = hg.sample_indices(n, max_hyp)
        lo, hi = np.arange(4) * n // 4, np.arange(1, 5) * n // 4
        assert np.all(want >= lo) and np.all(want < hi) and np.all(np.diff(want, axis=1) > 0)       # one per stratum, ascending
        for h in range(max_hyp):
            H, idx = native.homography_sample(n, max_hyp, h)
            assert H == max_hyp and idx == tuple(want[h].tolist()), (n, max_hyp, h)
        assert native.homography_sample(n, max_hyp, -1) == (max_hyp, (-1,) * 4) == native.homography_sample(n, max_hyp, max_hyp)
    assert native.homography_sample(100, 0, 127)[0] == 128
    assert native.homography_sample(100, 0, 127) == native.homography_sample(100, 128, 127)


def test_the_numpy_sampler_is_the_rule_in_python_integers():
    for n, h in ((5, 0), (17, 5), (363, 127), (5000, 999), (1 << 20, 65535)):
        want = [k * n // 4 + hg.mix(4 * h + k) % ((k + 1) * n // 4 - k * n // 4) for k in range(4)]
        assert hg.sample_indices(n, h + 1)[h].tolist() == want
    assert hg.mix(0) == 0xE220A8397B1DCDAF                    # splitmix64's first output from state 0


def test_out_of_range_arguments(sfm):
    native = sfm.native
    for n, max_hyp in ((4, 128), (0, 128), (-1, 128), (100, -1), (100, 65537)):
        assert native.homography_sample(n, max_hyp, 0) == (0, (-1,) * 4), (n, max_hyp)
        assert hg.hypothesis_count(n, max_hyp) == 0
    left = np.zeros((2, 5))
    for kw in (dict(max_err2=float("nan")), dict(max_err2=-1.0), dict(max_hyp=-1), dict(max_hyp=65537), dict(max_hyp=1.5),
               dict(iters=-1), dict(iters=0.5)):
        args = dict(max_err2=4.0)
        args.update(kw)
        with pytest.raises(ValueError):
            native.homography_ransac([0, 5], left, left, **args)
        with pytest.raises(ValueError):
            native.homography_ransac_dev([0, 5], 5, 0, 0, **args)
    for ptr in ([1, 5], [0, 3, 2, 5], [0, 4], []):
        with pytest.raises(ValueError, match="set_ptr"):
            native.homography_ransac(ptr, left, left, 4.0)
    with pytest.raises(ValueError, match="left"):
        native.homography_ransac([0, 5], left, np.zeros((2, 4)), 4.0)
    with pytest.raises(ValueError, match="left"):
        native.homography_ransac([0, 5], np.zeros((3, 5)), np.zeros((3, 5)), 4.0)
    with pytest.raises(ValueError, match="outputs"):
        native.homography_ransac([0, 5], left, left, 4.0, outputs=("mask",))
    assert (native.HOMOGRAPHY_TOO_FEW, native.HOMOGRAPHY_NO_MODEL, native.HOMOGRAPHY_KEPT_HYPOTHESIS) == \
        (hg.TOO_FEW, hg.NO_MODEL, hg.KEPT_HYPOTHESIS)
    assert (native.HOMOGRAPHY_MAX_HYP, native.HOMOGRAPHY_DEFAULT_HYP, native.HOMOGRAPHY_MIN_MATCHES) == (hg.HYP_MAX, hg.HYP_DEFAULT, hg.MIN_MATCHES)
    assert native.HOMOGRAPHY_SUMMARY[0] == "sets_solved" and len(native.HOMOGRAPHY_SUMMARY) == 6
    assert native.HOMOGRAPHY_OUTPUTS == ("inlier", "n_inliers", "best_hyp", "status", "summary")
    for name in ("sfm_homography_ransac", "sfm_homography_ransac_dev", "sfm_homography_sample"):
        assert name in native.EXPORTS


@pytest.mark.parametrize("name", ["proto1", "proto2"])
def test_the_reference_rejects_the_displaced_matches(name, capsys):
    sc, ref = hg.scene_and_reference(name)
    assert np.all(ref.best_hyp >= 0) and ref.summary[0] == len(hg.PROTO_COUNTS)
    clean_out = int(((ref.inlier == 0) & ~sc.displaced).sum())
    bad_in = int(((ref.inlier == 1) & sc.displaced).sum())
    with capsys.disabled():
        print("\n%s: %d matches, %d displaced, %d clean rejected, %d displaced accepted"
              % (name, sc.displaced.size, int(sc.displaced.sum()), clean_out, bad_in))
    assert sc.displaced.sum() > 0 and bad_in == 0             # (a clean match 2 px off in either image is rejected too:
    assert clean_out <= 0.1 * (~sc.displaced).sum()           #  0.5 px of noise on both keys puts a few per cent there)


@pytest.mark.parametrize("case", hg.CASES + hg.PATH_CASES + hg.EXTRA_CASES, ids=lambda c: "%s-%g-%d-%d" % c)
def test_every_set_of_every_scene_is_settled(case, capsys):
    sc, ref = hg.case_reference(case)
    solved = ref.best_hyp >= 0
    with capsys.disabled():
        print("\n%s: %d sets, %d unsettled, worst d_H %.3e, summary %s"
              % (case, sc.counts.size, int((~ref.settled).sum()), ref.d_H[solved & (ref.d_H < 1e-3)].max(initial=0.0), ref.summary.tolist()))
    assert ref.settled.all(), np.flatnonzero(~ref.settled)
    assert ref.summary[0] + ref.summary[1] + ref.summary[2] == sc.counts.size and ref.summary[4] == ref.inlier.sum()


@pytest.mark.parametrize("name", list(hg.FAMILIES))
def test_every_set_of_every_geometry_case_is_settled(name, capsys):
    sc = hg.scene(name)
    assert sc.counts.tolist() == list(hg.FAMILY_COUNTS)
    cases = [case for case in hg.GEOMETRY_CASES if case[0] == name]
    assert len(cases) == len(hg.FAMILY_ERR2) * len(hg.FAMILY_ITERS)
    worst, statuses, stood = 0.0, np.zeros(8, dtype=int), np.zeros(6, dtype=int)
    for case in cases:
        ref = hg.case_reference(case)[1]
        assert ref.settled.all(), (case, np.flatnonzero(~ref.settled))
        assert ref.summary[0] + ref.summary[1] + ref.summary[2] == sc.counts.size and ref.summary[4] == ref.inlier.sum()
        worst = max(worst, ref.d_H.max())
        statuses += np.bincount(ref.status, minlength=8)
        stood += np.bincount(ref.stood[ref.best_hyp >= 0], minlength=6)
    with capsys.disabled():
        print("\n%s: %d cases of %d sets, 0 unsettled, worst d_H %.3e, statuses 0 / NO_MODEL / KEPT: %d / %d / %d, stood 0..5: %s"
              % (name, len(cases), sc.counts.size, worst, statuses[0], statuses[hg.NO_MODEL], statuses[hg.KEPT_HYPOTHESIS], stood.tolist()))
    assert statuses[0] + statuses[hg.KEPT_HYPOTHESIS] > 0      # no family rests on sets without a model


def test_the_geometry_cases_reach_the_kept_hypothesis_and_every_number_of_rounds():
    kept_iters, stood, no_model = set(), set(), False
    for case in hg.GEOMETRY_CASES:
        iters = case[3]
        ref = hg.case_reference(case)[1]
        kept = (ref.status & hg.KEPT_HYPOTHESIS) != 0
        assert not (kept & (ref.best_hyp < 0)).any() and np.array_equal(kept, (ref.best_hyp >= 0) & (ref.stood == 0) & (iters > 0))
        assert ref.summary[3] == kept.sum() and np.all(ref.stood <= iters)
        if kept.any():
            kept_iters.add(iters)
        stood |= set(ref.stood[ref.best_hyp >= 0].tolist())
        no_model |= bool(ref.summary[1] > 0)
    assert kept_iters                      # KEPT_HYPOTHESIS occurs
    assert stood == {0, 1, 2, 3, 4, 5}
    assert no_model                        # ... and so does a set of 40 matches without a model


def test_the_paths_scene_has_every_count():
    sc = hg.scene("paths")
    assert sc.counts.tolist() == list(hg.PATHS_COUNTS) and sc.counts.max() == 5000
    for max_hyp in hg.PATHS_HYP:
        ref = hg.scene_and_reference("paths", max_hyp)[1]
        assert np.array_equal((ref.status & hg.TOO_FEW) != 0, sc.counts < 5)
        if max_hyp >= 63:                                      # (one hypothesis is a displaced sample in some sets)
            assert np.all(ref.best_hyp[sc.counts >= 16] >= 0)      # (sets of 5, 6 or 15 matches allow few samples)
    assert [int(np.flatnonzero(sc.counts == n)[0]) for n in hg.ALONE] == [2, 7, 9, 12, 15, 17]


def test_the_degenerate_scene_is_what_it_says():
    sc, ref = hg.scene_and_reference("degenerate")
    assert ref.status.tolist() == [0, hg.NO_MODEL, hg.NO_MODEL] and ref.best_hyp.tolist() == [0, -1, -1]
    lo, hi = sc.set_ptr[0], sc.set_ptr[1]
    l, r = sc.left[:, lo:hi], sc.right[:, lo:hi]
    for p in (l, r):                                           # every match on one line, in both images
        assert np.linalg.matrix_rank(np.vstack((p, np.ones((1, p.shape[1])))).T) == 2
    assert ref.inlier[lo:hi].all() and ref.stood[0] == hg.ITERS
    assert not ref.H[1:].any() and not ref.inlier[hi:].any()
    assert np.isnan(sc.right).sum() == 1 and np.isfinite(sc.left).all()
    assert np.ptp(sc.left[:, sc.set_ptr[1]:sc.set_ptr[2]], axis=1).max() == 0.0


def test_the_ties_scene_has_ties_a_pick_can_get_wrong(capsys):
    every, two_px = hg.PATH_CASES[0], hg.PATH_CASES[1]
    assert every[0] == two_px[0] == "ties" and every[1] == hg.EVERYONE and two_px[1] == hg.MAX_ERR2
    sc, ref = hg.case_reference(every)
    assert sc.counts.size == 2 and ref.settled.all() and not ref.status.any()
    for s in range(2):              # every finite match is an inlier of every valid hypothesis: the lowest valid h wins
        counts = hg.hypothesis_counts(*hg.set_of(sc, s), every[1], every[2])
        valid = np.flatnonzero(counts >= 0)
        assert valid.size >= 3 and np.all(counts[valid] == sc.counts[s]) and ref.best_hyp[s] == valid[0]
        assert ref.n_inliers[s] == sc.counts[s]
    sc, ref = hg.case_reference(two_px)
    assert ref.settled.all() and not ref.status.any()
    for s in range(2):
        counts = hg.hypothesis_counts(*hg.set_of(sc, s), two_px[1], two_px[2])
        tied = np.flatnonzero(counts == counts.max())
        with capsys.disabled():
            print("\nties set %d: %d matches, %d hypotheses at the largest count %d, the first of them %s"
                  % (s, sc.counts[s], tied.size, counts.max(), tied[:8].tolist()))
        assert tied.size >= 3 and tied[0] != 0 and ref.best_hyp[s] == tied[0] and (tied >= 64).any()
        # a pick that prefers the lower lane over the lower h takes another one
        assert (tied[1:] % 64 < tied[0] % 64).any()
        other = hg.hypothesis_counts(*hg.set_of(sc, s), two_px[1], two_px[2], 1)
        assert np.array_equal(np.flatnonzero(other == other.max()), tied)


def test_the_many_sets_scene_is_what_it_says():
    case = hg.PATH_CASES[2]
    sc, ref = hg.case_reference(case)
    n_sets = sc.counts.size
    assert case[0] == "many_sets" and n_sets == 259 and set(sc.counts.tolist()) == set(hg.MANY_SIZES)
    small = sc.counts < hg.MIN_MATCHES
    assert small[0] and small[-1] and (small[1:-1][:-1] & small[1:-1][1:]).any()
    assert ref.settled.all()
    assert ref.summary[0] + ref.summary[1] + ref.summary[2] == n_sets and np.all(ref.summary[:3] > 0)
    assert ref.summary[2] == small.sum()


# ---- the verdict, from the reference's counts alone ------------------------------------------------------------------------
@pytest.mark.parametrize("name,want", [("plane", "degenerate"), ("rotation", "degenerate"), ("general", "general")])
def test_the_verdict_of_the_families(name, want, capsys):
    sc, href = hg.scene_and_reference(name)
    fref = tv.reference(sc.set_ptr, sc.left, sc.right, hg.MAX_ERR2, 128, hg.ITERS)
    for s in range(sc.counts.size):
        ratio = href.n_inliers[s] / max(int(fref.n_inliers[s]), 1)
        with capsys.disabled():
            print("\n%s set %d (%d matches): homography %d, fundamental %d inliers, ratio %.2f"
                  % (name, s, sc.counts[s], href.n_inliers[s], fref.n_inliers[s], ratio))
        assert fref.best_hyp[s] >= 0                           # the eight-point solve returns some matrix in every family
        assert hg.verdict(href.n_inliers[s], href.best_hyp[s] >= 0, fref.n_inliers[s], fref.best_hyp[s] >= 0) == want
        assert ratio >= 0.85 if want == "degenerate" else ratio < 0.25
    assert hg.verdict(0, False, 0, False) == "none" and hg.verdict(7, True, 0, False) == "degenerate"
    assert hg.verdict(0, False, 30, True) == "general" and hg.verdict(79, True, 100, True) == "general"
    assert hg.verdict(80, True, 100, True) == "degenerate"
