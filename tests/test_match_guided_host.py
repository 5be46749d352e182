"""Host-side checks of guided matching (no GPU): matching.filter_guided against a loop, the adjugate the library forms
against numpy.linalg.inv, the argument checks, and the conditions tests/test_gpu_match_guided.py rests on -- EVERY row of every
case it runs is settled in the NumPy reference of tests/_match_guided_reference.py (so the GPU tests compare every row
exactly), the cases reach what they are there for, and the twin scene shows the point of the feature on the reference alone:
the ratio test loses every twinned match, the gate brings back every one it admits and nothing it rejects."""
import numpy as np
import pytest

import _match_guided_reference as mg


def test_filter_guided_against_a_loop(sfm):
    rng = np.random.default_rng(5)
    n = 4000
    best = rng.integers(-1, 50, n).astype(np.int32)
    d0 = rng.integers(0, 40, n).astype(np.float32)
    d1 = (d0 + rng.integers(0, 30, n)).astype(np.float32)
    d1[rng.random(n) < 0.2] = np.inf                            # no second neighbour
    d1[rng.random(n) < 0.1] = 0.0                               # a zero second distance keeps nothing and raises nothing
    exact = rng.random(n) < 0.1                                 # d0 == 0.7 d1 in float64 is not "<"
    d1[exact], d0[exact] = 10.0, 7.0
    d0[best < 0] = np.inf
    mutual = rng.random(n) < 0.7
    for ratio in (0.7, 0.5, 1.0):
        q, t = sfm.matching.filter_guided(best, d0, d1, mutual, ratio)
        wq, wt = mg.filter_loop(best, d0, d1, mutual, ratio)
        assert q.tolist() == wq.tolist() and t.tolist() == wt.tolist()
    q, _t = sfm.matching.filter_guided(best, d0, d1, mutual)
    assert not np.any(d1[q] == 0.0) and np.all(best[q] >= 0) and np.all(mutual[q])
    assert np.any(np.isinf(d1[q])) and q.shape[0] > 100
    assert not np.any(exact[q] & (d0[q] == 7.0))
    q, t = sfm.matching.filter_guided(np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, bool))
    assert q.shape == (0,) and t.shape == (0,)


def test_the_adjugate_is_the_inverse_up_to_scale(sfm):
    native = sfm.native
    rng = np.random.default_rng(11)
    mats = [mg.true_homography(), np.eye(3), np.diag([2.0, 3.0, 5.0])] + [rng.normal(size=(3, 3)) for _ in range(20)]
    for H in mats:
        G = native.homography_adjugate(H)
        inv = np.linalg.inv(H) * np.linalg.det(H)
        assert np.allclose(G, inv, rtol=1e-12, atol=1e-12 * np.abs(inv).max())
        assert np.allclose(G, mg.adjugate(H), rtol=1e-13, atol=1e-15)
        assert np.allclose(H @ G, np.linalg.det(H) * np.eye(3), atol=1e-12 * max(1.0, np.abs(H).max() ** 3))
    assert np.array_equal(native.homography_adjugate(np.eye(3)), np.eye(3))            # not scaled
    assert np.array_equal(native.homography_adjugate(2.0 * np.eye(3)), 4.0 * np.eye(3))
    singular = np.outer([1.0, 2.0, 3.0], [1.0, 1.0, 1.0])
    assert np.abs(native.homography_adjugate(singular) @ singular).max() < 1e-12     # finite, rank <= 1


def test_argument_checks(sfm):
    native = sfm.native
    F = mg.true_fundamental()
    assert (native.GUIDE_NONE, native.GUIDE_FUNDAMENTAL, native.GUIDE_HOMOGRAPHY) == (mg.NONE, mg.FUNDAMENTAL, mg.HOMOGRAPHY)
    assert native.GUIDED_OUTPUTS == mg.OUTPUTS
    for name in ("sfm_match_guided", "sfm_match_guided_dev", "sfm_match_guided_track", "sfm_match_guided_set_pairs", "sfm_homography_adjugate"):
        assert name in native.EXPORTS
    kind, model, e2 = native.check_guided(3, ["none", "fundamental", native.GUIDE_HOMOGRAPHY], [None, F, np.eye(3)], 4)
    assert kind.tolist() == [0, 1, 2] and model.shape == (3, 9) and e2 == 4.0
    assert np.array_equal(model[0], np.zeros(9)) and np.array_equal(model[1], F.reshape(9))
    for bad in (float("nan"), -1.0, -0.0 - 1e-300):
        with pytest.raises(ValueError, match="max_err2"):
            native.check_guided(1, [1], [F], bad)
    assert native.check_guided(1, [1], [F], 0.0)[2] == 0.0 and native.check_guided(1, [1], [F], float("inf"))[2] == float("inf")
    for k in (3, -1, "epipolar"):
        with pytest.raises(ValueError, match="gate"):
            native.check_guided(1, [k], [F], 4.0)
    for m in (np.full((3, 3), np.nan), np.where(np.eye(3) > 0, np.inf, F), np.zeros((2, 3)), None):
        with pytest.raises((ValueError, TypeError)):
            native.check_guided(1, [1], [m], 4.0)
    native.check_guided(1, [0], [np.full((3, 3), np.nan)], 4.0)        # the model of an ungated reference is not read
    with pytest.raises(ValueError, match="references"):
        native.check_guided(2, [1], [F], 4.0)
    for model in (None, ("affine", F), ("fundamental", np.zeros((2, 2))), 5):
        if model is None:
            continue
        with pytest.raises(ValueError, match="model"):
            sfm.processors._guided_model(model)
    assert sfm.processors._guided_model(("homography", np.eye(3)))[0] == "homography"


def _all_cases():
    out = []
    for kind in (mg.FUNDAMENTAL, mg.HOMOGRAPHY):
        out += [(nq, nt, dim, kind, "l2", False) for nq, nt, dim in mg.PARITY_CASES]
        out += [(mg.MID[0], mg.MID[1], 32, kind, "hamming", False), (mg.MID[0], mg.MID[1], 32, kind, "l2", True)]
    return out


def test_every_row_of_every_parity_case_is_settled(capsys):
    total = rows = 0
    some, none, one = 0, 0, 0
    frac = {mg.FUNDAMENTAL: [0, 0], mg.HOMOGRAPHY: [0, 0]}
    for nq, nt, dim, kind, metric, fl in _all_cases():
        sc, ref = mg.case(nq, nt, dim, kind, metric=metric, float_rows=fl)
        assert ref["settled"].all(), (nq, nt, dim, kind, metric, fl, np.flatnonzero(~ref["settled"]))
        total += nq * nt
        rows += nq
        frac[kind][0] += int(ref["n_admitted"].sum())
        frac[kind][1] += nq * nt
        none += int((ref["n_admitted"] == 0).sum())
        one += int((ref["n_admitted"] == 1).sum())
        some += int((ref["n_admitted"] >= 2).sum())
        assert np.all((ref["best_idx"] >= 0) == (ref["n_admitted"] >= 1)) and np.all((ref["second_idx"] >= 0) == (ref["n_admitted"] >= 2))
        if nt >= 1023 and nq >= 127 and metric == "l2" and not fl:
            # what the case is there for: the true partner is admitted and is the best for most queries
            hit = ref["best_idx"][sc.true_que] == sc.true_ref
            assert hit.mean() > 0.9, (nq, nt, dim, kind, hit.mean())
    with capsys.disabled():
        print("\nguided parity cases: %d pairs, %d rows; rows with 0 / 1 / >= 2 admitted keys: %d / %d / %d; admitted share F %.4f, H %.5f"
              % (total, rows, none, one, some, frac[mg.FUNDAMENTAL][0] / frac[mg.FUNDAMENTAL][1],
                 frac[mg.HOMOGRAPHY][0] / frac[mg.HOMOGRAPHY][1]))
    assert none > 100 and one > 100 and some > 100
    assert 0.005 < frac[mg.FUNDAMENTAL][0] / frac[mg.FUNDAMENTAL][1] < 0.1
    assert frac[mg.HOMOGRAPHY][0] / frac[mg.HOMOGRAPHY][1] < 0.02


@pytest.mark.parametrize("float_mixed", [False, True])
def test_the_batch_scene_is_settled(float_mixed):
    sc = mg.batch_scene(float_mixed)
    assert [k for _xy, _d, k, _m in sc.refs] == [mg.NONE, mg.FUNDAMENTAL, mg.HOMOGRAPHY, mg.FUNDAMENTAL]
    for (xy, desc, kind, _model), out in zip(sc.refs, sc.out):
        assert out["settled"].all()
        if kind == mg.NONE:
            assert np.all(out["n_admitted"] == desc.shape[0])
        else:
            assert 0 < out["n_admitted"].sum() < 0.2 * out["n_admitted"].size * desc.shape[0]
    if float_mixed:
        assert not np.array_equal(sc.refs[1][1], np.round(sc.refs[1][1])) and np.array_equal(sc.que_desc, np.round(sc.que_desc))


def test_a_zero_threshold_admits_nothing_on_noisy_keys():
    for kind in (mg.FUNDAMENTAL, mg.HOMOGRAPHY):
        sc, _ = mg.case(129, 1025, 128, kind)
        ref = mg.reference(sc.norm, sc.que_desc, sc.ref_desc, sc.que_xy, sc.ref_xy, kind, mg.model_of(sc, kind), 0.0)
        assert ref["settled"].all() and np.all(ref["n_admitted"] == 0) and np.all(ref["best_idx"] == -1)
        assert np.all(np.isposinf(ref["best_dist"])) and not ref["mutual"].any()
        xy = sc.que_xy.copy()
        xy[7, 0] = np.nan                                       # a NaN coordinate admits nothing, at any threshold
        ref = mg.reference(sc.norm, sc.que_desc, sc.ref_desc, xy, sc.ref_xy, kind, mg.model_of(sc, kind), 4.0)
        assert ref["settled"].all() and ref["n_admitted"][7] == 0 and ref["best_idx"][7] == -1 and ref["n_admitted"].sum() > 0


@pytest.mark.parametrize("planar", [False, True])
def test_the_twin_scene_shows_the_point(planar, capsys):
    sc = mg.twin_scene(planar)
    kind = mg.HOMOGRAPHY if planar else mg.FUNDAMENTAL
    model = mg.model_of(sc, kind)
    true = {(int(sc.true_ref[k]), int(sc.true_que[k])) for k in range(sc.true_ref.shape[0])}
    twinned = {(int(sc.true_ref[k]), int(sc.true_que[k])) for k in sc.twinned}
    # the twin's row is closer to the true row than the ratio test tolerates, and it sits off the gate
    plain = mg.plain_knn_pairs(sc)
    assert len(twinned) >= 60 and not (plain & twinned)                     # plain KNN with ratio 0.7 loses EVERY twinned match
    assert len(plain & true) >= 0.9 * (len(true) - len(twinned))            # (and keeps the others)
    ref = mg.reference(sc.norm, sc.que_desc, sc.ref_desc, sc.que_xy, sc.ref_xy, kind, model, 4.0)
    assert ref["settled"].all()
    ok = mg.admitted(kind, model, sc.ref_xy, sc.que_xy, 4.0)
    for k, twin in zip(sc.twinned, sc.twin_key):
        assert not ok[sc.true_que[k], twin]                                  # >= 20 px from what the gate admits
    r_idx, q_idx = mg.pairs_of(ref)
    got = set(zip(r_idx.tolist(), q_idx.tolist()))
    admitted_twinned = {(t, q) for t, q in twinned if ok[q, t]}
    assert admitted_twinned <= got                                           # guided keeps every twinned match the gate admits
    assert all(ok[q, t] for t, q in got)                                     # and returns no pair the gate rejects
    assert len(admitted_twinned) >= 0.85 * len(twinned)
    assert np.all(np.diff(r_idx) > 0) and len(set(q_idx.tolist())) == q_idx.shape[0]      # one to one, sorted by reference key
    with capsys.disabled():
        print("\ntwin scene (%s): %d true matches, %d twinned, plain knn keeps %d true and 0 twinned; guided keeps %d pairs, "
              "%d true, %d of %d admitted twinned" % ("plane" if planar else "general", len(true), len(twinned), len(plain & true),
                                                      len(got), len(got & true), len(got & twinned), len(admitted_twinned)))
    assert len(got - true) <= 0.05 * len(got)


def test_the_ties_scene():
    """Two train keys with the same row at the same distance: the lower index wins; gated out, the other is promoted."""
    t = mg.ties_scene()
    both = mg.reference(t.norm, t.que_desc, t.ref_desc, t.que_xy, t.ref_xy, mg.HOMOGRAPHY, np.eye(3), 4.0)
    assert both["settled"].all() and both["best_idx"].tolist() == t.want_both_best and both["second_idx"].tolist() == t.want_both_second
    assert np.all(both["best_dist"][:2].view(np.uint32) == both["second_dist"][:2].view(np.uint32))
    moved = mg.reference(t.norm, t.que_desc, t.ref_desc, t.que_xy, t.ref_xy_lower_out, mg.HOMOGRAPHY, np.eye(3), 4.0)
    assert moved["settled"].all() and moved["best_idx"].tolist() == t.want_moved_best and moved["n_admitted"].tolist() == t.want_moved_count
