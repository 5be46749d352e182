"""Host-side checks of the robust two-view geometry (no GPU): the stratified sampler against the NumPy sampler and Python
integers, the argument checks, and the NumPy reference of tests/_twoview_ransac_reference.py on the scenes the GPU tests
use -- it rejects no clean match on the prototype scenes, and EVERY set of every scene any test uses is settled at every
max_hyp used, so the GPU tests compare decisions exactly and leave nothing out.  For the geometry families and the further
scenes of tests/test_gpu_twoview_paths.py it also asserts that the reference reaches what those scenes are there for."""
import numpy as np
import pytest

import _twoview_ransac_reference as tv


@pytest.mark.parametrize("max_hyp", [1, 128, 65536])
def test_the_sample_of_every_hypothesis(sfm, max_hyp):
    native = sfm.native
    for n in (9, 10, 15, 16, 17, 64, 363, 1 << 20):
        want = tv.sample_indices(n, max_hyp)
        lo, hi = np.arange(8) * n // 8, np.arange(1, 9) * n // 8
        assert np.all(want >= lo) and np.all(want < hi) and np.all(np.diff(want, axis=1) > 0)       # one per stratum, ascending
        for h in range(max_hyp):
            H, idx = native.twoview_sample(n, max_hyp, h)
            assert H == max_hyp and idx == tuple(want[h].tolist()), (n, max_hyp, h)
        assert native.twoview_sample(n, max_hyp, -1) == (max_hyp, (-1,) * 8) == native.twoview_sample(n, max_hyp, max_hyp)
    assert native.twoview_sample(100, 0, 127)[0] == 128 and native.twoview_sample(100, 0, 127) == native.twoview_sample(100, 128, 127)


def test_the_numpy_sampler_is_the_rule_in_python_integers():
    for n, h in ((9, 0), (17, 5), (363, 127), (5000, 999), (1 << 20, 65535)):
        want = [k * n // 8 + tv.mix(8 * h + k) % ((k + 1) * n // 8 - k * n // 8) for k in range(8)]
        assert tv.sample_indices(n, h + 1)[h].tolist() == want
    assert tv.mix(0) == 0xE220A8397B1DCDAF                    # splitmix64's first output from state 0


def test_out_of_range_arguments(sfm):
    native = sfm.native
    for n, max_hyp in ((8, 128), (0, 128), (-1, 128), (100, -1), (100, 65537)):
        assert native.twoview_sample(n, max_hyp, 0) == (0, (-1,) * 8), (n, max_hyp)
        assert tv.hypothesis_count(n, max_hyp) == 0
    for kw in (dict(max_err2=float("nan")), dict(max_err2=-1.0), dict(max_hyp=-1), dict(max_hyp=65537), dict(max_hyp=1.5),
               dict(iters=-1), dict(iters=0.5)):
        args = dict(max_err2=4.0)
        args.update(kw)
        with pytest.raises(ValueError):
            native.check_twoview(**args)
    assert native.check_twoview(4, 0, 2) == (4.0, 0, 2) and native.check_twoview(0.0, 65536, 0) == (0.0, 65536, 0)
    left = np.zeros((2, 5))
    for ptr in ([1, 5], [0, 3, 2, 5], [0, 4], []):
        with pytest.raises(ValueError, match="set_ptr"):
            native.check_twoview_sets(ptr, left, left)
    with pytest.raises(ValueError, match="left"):
        native.check_twoview_sets([0, 5], left, np.zeros((2, 4)))
    with pytest.raises(ValueError, match="left"):
        native.check_twoview_sets([0, 5], np.zeros((3, 5)), np.zeros((3, 5)))
    with pytest.raises(ValueError, match="outputs"):
        native.twoview_ransac([0, 5], left, left, 4.0, outputs=("mask",))
    assert (native.TWOVIEW_TOO_FEW, native.TWOVIEW_NO_MODEL, native.TWOVIEW_KEPT_HYPOTHESIS) == \
        (tv.TOO_FEW, tv.NO_MODEL, tv.KEPT_HYPOTHESIS)
    assert (native.TWOVIEW_MAX_HYP, native.TWOVIEW_DEFAULT_HYP, native.TWOVIEW_MIN_MATCHES) == (tv.HYP_MAX, tv.HYP_DEFAULT, tv.MIN_MATCHES)
    assert native.TWOVIEW_SUMMARY[0] == "sets_solved" and len(native.TWOVIEW_SUMMARY) == 6


@pytest.mark.parametrize("name", ["proto1", "proto2"])
def test_the_reference_rejects_no_clean_match(name, capsys):
    sc, ref = tv.scene_and_reference(name)
    assert np.all(ref.best_hyp >= 0) and ref.summary[0] == len(tv.PROTO_COUNTS)
    clean_out = int(((ref.inlier == 0) & ~sc.displaced).sum())
    bad_in = int(((ref.inlier == 1) & sc.displaced).sum())
    with capsys.disabled():
        print("\n%s: %d matches, %d displaced, %d clean rejected, %d displaced accepted"
              % (name, sc.displaced.size, int(sc.displaced.sum()), clean_out, bad_in))
    assert clean_out == 0                # (a displaced match that is accepted moved along its epipolar line)


@pytest.mark.parametrize("name,max_hyp", tv.CASES)
def test_every_set_of_every_scene_is_settled(name, max_hyp, capsys):
    sc, ref = tv.scene_and_reference(name, max_hyp)
    solved = ref.best_hyp >= 0
    with capsys.disabled():
        print("\n%s, max_hyp %d: %d sets, %d unsettled, worst d_G %.3e, summary %s"
              % (name, max_hyp, sc.counts.size, int((~ref.settled).sum()),
                 ref.d_G[solved & (ref.d_G < 1e-3)].max(initial=0.0), ref.summary.tolist()))
    assert ref.settled.all(), np.flatnonzero(~ref.settled)
    assert ref.summary[0] + ref.summary[1] + ref.summary[2] == sc.counts.size and ref.summary[4] == ref.inlier.sum()


def test_the_settled_flag_holds_with_no_refit_rounds():
    sc, ref = tv.scene_and_reference("paths", 128, 0)
    assert ref.settled.all() and not ref.stood.any() and not (ref.status & tv.KEPT_HYPOTHESIS).any()


def test_the_degenerate_scene_is_what_it_says():
    sc, ref = tv.scene_and_reference("degenerate")
    assert ref.status.tolist() == [0, tv.NO_MODEL, tv.NO_MODEL] and ref.best_hyp.tolist()[1:] == [-1, -1]
    lo, hi = sc.set_ptr[0], sc.set_ptr[1]
    assert ref.inlier[lo:hi].all() and ref.stood[0] == tv.ITERS         # every matrix [e]x H explains the whole plane
    assert not ref.F[1:].any() and not ref.inlier[hi:].any()
    assert np.isnan(sc.right).sum() == 1


def test_the_paths_scene_has_every_count():
    sc = tv.scene("paths")
    assert sc.counts.tolist() == list(tv.PATHS_COUNTS)
    ref = tv.scene_and_reference("paths", 128)[1]
    assert np.array_equal((ref.status & tv.TOO_FEW) != 0, sc.counts < 9)
    assert np.all(ref.best_hyp[sc.counts >= 10] >= 0)            # (the nine matches of set 2 allow few samples: no model)


# ---- the geometry families and the further scenes of tests/test_gpu_twoview_paths.py -------------------------------------
# These conditions hold of the reference alone (the seeds were chosen for them): they keep the GPU tests, which walk the same
# lists and leave no set out, from passing without having reached what they are there for.
def _family_cases(name):
    return [case for case in tv.GEOMETRY_CASES if case[0] == name]


@pytest.mark.parametrize("name", list(tv.FAMILIES))
def test_every_set_of_every_geometry_case_is_settled(name, capsys):
    sc = tv.scene(name)
    assert sc.counts.tolist() == list(tv.FAMILY_COUNTS)
    cases = _family_cases(name)
    assert len(cases) == len(tv.FAMILY_ERR2) * len(tv.FAMILY_ITERS) + 1
    assert sorted({c[1] for c in cases}) == sorted([tv.family_err2(name, e) for e in tv.FAMILY_ERR2] + [tv.EVERYONE])
    worst, statuses, stood = 0.0, np.zeros(8, dtype=int), np.zeros(6, dtype=int)
    for case in cases:
        ref = tv.case_reference(case)[1]
        assert ref.settled.all(), (case, np.flatnonzero(~ref.settled))
        assert ref.summary[0] + ref.summary[1] + ref.summary[2] == sc.counts.size and ref.summary[4] == ref.inlier.sum()
        worst = max(worst, ref.d_G.max())
        statuses += np.bincount(ref.status, minlength=8)
        stood += np.bincount(ref.stood[ref.best_hyp >= 0], minlength=6)
    with capsys.disabled():
        print("\n%s: %d cases of %d sets, 0 unsettled, worst d_G %.3e, statuses 0 / NO_MODEL / KEPT: %d / %d / %d, stood 0..5: %s"
              % (name, len(cases), sc.counts.size, worst, statuses[0], statuses[tv.NO_MODEL], statuses[tv.KEPT_HYPOTHESIS], stood.tolist()))


def test_the_geometry_cases_reach_the_kept_hypothesis_and_every_number_of_rounds():
    families, kept_iters, stood, rejected_later, kept_beside_no_model = set(), set(), set(), False, False
    for case in tv.GEOMETRY_CASES:
        name, _max_err2, _max_hyp, iters = case
        ref = tv.case_reference(case)[1]
        kept = (ref.status & tv.KEPT_HYPOTHESIS) != 0
        assert not (kept & (ref.best_hyp < 0)).any() and np.array_equal(kept, (ref.best_hyp >= 0) & (ref.stood == 0) & (iters > 0))
        assert ref.summary[3] == kept.sum() and np.all(ref.stood <= iters)
        if kept.any():
            families.add(name)
            kept_iters.add(iters)
        stood |= set(ref.stood[ref.best_hyp >= 0].tolist())
        rejected_later |= bool(((ref.stood > 0) & (ref.stood < iters)).any())
        kept_beside_no_model |= bool(ref.summary[3] > 0 and ref.summary[1] > 0)
    assert len(families) >= 5, families
    assert {1, 2, 5} <= kept_iters
    assert stood == {0, 1, 2, 3, 4, 5}
    assert rejected_later                 # a round is rejected after an earlier one stood
    assert kept_beside_no_model           # one call with summary[3] > 0 and summary[1] > 0
    # what the scenes that came with the feature never reach
    for name, max_hyp in tv.CASES:
        ref = tv.scene_and_reference(name, max_hyp)[1]
        assert not (ref.status & tv.KEPT_HYPOTHESIS).any() and ref.stood.max() <= 2


def test_under_the_threshold_of_everyone_the_first_valid_hypothesis_wins():
    for case in tv.GEOMETRY_CASES:
        name, max_err2, max_hyp, _iters = case
        if max_err2 != tv.EVERYONE:
            continue
        sc, ref = tv.case_reference(case)
        assert (ref.best_hyp >= 0).any()
        for s in range(sc.counts.size):
            counts = tv.hypothesis_counts(*tv.set_of(sc, s), max_err2, max_hyp)
            valid = np.flatnonzero(counts >= 0)
            if ref.best_hyp[s] >= 0:
                assert ref.n_inliers[s] == sc.counts[s] and ref.best_hyp[s] == valid[0] and np.all(counts[valid] == sc.counts[s])
            else:
                assert valid.size == 0


def test_the_ties_scene_has_ties_a_pick_can_get_wrong(capsys):
    case = tv.PATH_CASES[0]
    sc, ref = tv.case_reference(case)
    assert case[0] == "ties" and sc.counts.size == 2 and ref.settled.all() and not ref.status.any()
    for s in range(2):
        counts = tv.hypothesis_counts(*tv.set_of(sc, s), case[1], case[2])
        tied = np.flatnonzero(counts == counts.max())
        with capsys.disabled():
            print("\nties set %d: %d matches, %d hypotheses at the largest count %d, the first of them %s"
                  % (s, sc.counts[s], tied.size, counts.max(), tied[:8].tolist()))
        assert tied.size >= 3 and tied[0] != 0 and ref.best_hyp[s] == tied[0]
        assert (tied >= 64).any()
        # a pick that prefers the lower lane over the lower h takes another one: a later tied h sits in a lane below the first's
        # (so there are h1 < h2 among the tied with h2 % 64 < h1 % 64)
        assert (tied[1:] % 64 < tied[0] % 64).any()
        for route in (0, 1):                                    # and the ties are no accident of one null-vector route
            other = tv.hypothesis_counts(*tv.set_of(sc, s), case[1], case[2], route)
            assert np.array_equal(np.flatnonzero(other == other.max()), tied)


def test_the_many_sets_scene_is_what_it_says():
    case = tv.PATH_CASES[1]
    sc, ref = tv.case_reference(case)
    n_sets = sc.counts.size
    assert case[0] == "many_sets" and n_sets >= 257 and set(sc.counts.tolist()) == set(tv.MANY_SIZES)
    small = sc.counts < tv.MIN_MATCHES
    assert small[0] and small[-1] and (small[1:-1][:-1] & small[1:-1][1:]).any()
    assert ref.settled.all()
    assert ref.summary[0] + ref.summary[1] + ref.summary[2] == n_sets and np.all(ref.summary[:3] > 0)
    assert ref.summary[2] == small.sum() and ref.summary[3] > 0


def test_the_nonfinite_scene_is_what_it_says():
    case = tv.PATH_CASES[2]
    sc, ref = tv.case_reference(case)
    assert case[0] == "nonfinite" and sc.counts.tolist() == [60, 1100]
    both = np.hstack((sc.left, sc.right))
    assert np.flatnonzero(~np.isfinite(sc.left[0])).tolist() == [31] and sc.left[0, 31] == np.inf and np.isfinite(sc.left[1]).all()
    assert np.flatnonzero(~np.isfinite(sc.right[0])).tolist() == [60 + 1050] and np.isnan(sc.right[0, 60 + 1050])
    assert np.isfinite(sc.right[1]).all() and (~np.isfinite(both)).sum() == 2
    assert ref.settled.all() and ref.status.tolist() == [tv.NO_MODEL, tv.NO_MODEL] and ref.best_hyp.tolist() == [-1, -1]
    assert not ref.F.any() and not ref.inlier.any() and ref.summary.tolist() == [0, 2, 0, 0, 0, 0]
