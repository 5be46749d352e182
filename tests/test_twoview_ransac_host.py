"""Host-side checks of the robust two-view geometry (no GPU): the stratified sampler against the NumPy sampler and Python
integers, the argument checks, and the NumPy reference of tests/_twoview_ransac_reference.py on the scenes the GPU tests
use -- it rejects no clean match on the prototype scenes, and EVERY set of every scene any test uses is settled at every
max_hyp used, so the GPU tests compare decisions exactly and leave nothing out."""
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
