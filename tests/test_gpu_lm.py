"""The cost of the resident scene and the Levenberg-Marquardt control of the matrix-free bundle adjustment (sfm_ba_cost,
sfm_ba_minimize_pcg, ``BaProblem.cost`` / ``minimize_pcg``, ``HipBaMixin.ba_solver = "lm"``) against the NumPy reference of
tests/_lm_reference.py.

What is exact: the accept / reject sequence and the stop reason -- tests/test_lm_host.py measures that no gain ratio of the
reference comes closer than 4.6e-3 to the threshold and that every stopping quantity is a factor 2 clear of its threshold,
nine orders above the device's distance from NumPy.  What is bounded: every logged scalar at 1e-9 relative (rho at 1e-9 times
the cancellation F / |F - F_trial| of its numerator), the final state at ``pr.tolerance`` of the disagreement of the two
NumPy routes on the same setting, in the norm ``pr.rel``."""
import numpy as np
import pytest

import _lm_reference as lr
import _pcg_reference as pr
import _robust_reference as rr
import _screen_reference as sr

pytestmark = pytest.mark.gpu

GROUPS = (0, 1, 4, 8, 16, 32, 64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _problem(hip, c, loss="none"):
    prob = hip.BaProblem(c.n_cams, c.pt_ptr, c.cam_idx, c.uv)
    if loss != "none":
        prob.set_loss(loss, c.delta)
    return prob


def _close(got, want, tol=1e-9):
    return abs(got - want) <= tol * abs(want)


# ---- 1: sfm_ba_cost -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", lr.LOSSES)
@pytest.mark.parametrize("name", lr.SCENES)
def test_cost_against_numpy(hip, sfm, oracle, name, loss):
    """1e-12 relative against the NumPy cost, for both quirk settings and every group width (hub70 has tracks of every
    length 1 .. 70); 1e-13 against the cost iterate_pcg reports for the same state."""
    c = pr.case(sfm, name)
    want = lr.state_cost(c, c.cams, c.pts, loss)
    worst = 0.0
    with _problem(hip, c, loss) as prob:
        prob.set_state(c.cams, c.pts)
        for quirks in (oracle.QUIRKS_REFERENCE, 0):
            for group in GROUPS:
                got = prob.cost(quirks, group)
                worst = max(worst, abs(got - want) / want)
                assert abs(got - want) <= 1e-12 * want, (name, loss, quirks, group, got, want)
        for group in (0, 8):
            got = prob.cost(group=group)
            lin = prob.iterate_pcg(5.0, 1, group=group).cost[0]
            prob.set_state(c.cams, c.pts)
            print(name, loss, group, "cost against pcg_linearize %.1e" % (abs(got - lin) / lin))
            assert abs(got - lin) <= 1e-13 * lin, (name, loss, group, got, lin)
        with pytest.raises(ValueError):
            prob.cost(group=2)
    print(name, loss, "worst against NumPy %.1e" % worst)


def test_cost_changes_nothing(hip, sfm):
    c = pr.case(sfm, "6x300")
    with _problem(hip, c, "huber") as prob, _problem(hip, c, "huber") as other:
        for p in (prob, other):
            p.set_option(hip.OPT_DETERMINISTIC, 1)
            p.set_state(c.cams, c.pts)
            p.iterate(5.0, 2)
        first = prob.cost()
        assert prob.cost() == first and prob.cost(group=8) == prob.cost(group=8)
        assert all(same_bits(x, y) for x, y in zip(prob.get_state(), other.get_state()))
        prob.iterate(5.0, 2)
        other.iterate(5.0, 2)
        assert all(same_bits(x, y) for x, y in zip(prob.get_state(), other.get_state()))
        assert same_bits(prob.get_stats(), other.get_stats())
        for p in (prob, other):
            p.set_state(c.cams, c.pts)
            p.iterate_pcg(5.0, 1)
        prob.cost(group=16)
        a, b = prob.iterate_pcg(5.0, 1), other.iterate_pcg(5.0, 1)
        assert all(same_bits(x, y) for x, y in zip(prob.get_state(), other.get_state())) and same_bits(a.cost, b.cost)
    # nothing left to fit: the cost is 0 and no trial runs
    sc = sfm.scenes.make_scene(3, 10, 1.0, seed=4)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)) as prob:
        prob.set_state(sc.cams_init, sc.pts_init)
        prob.cull(0.0, 1.0, 0)
        assert prob.info(hip.INFO_N_OBS) == 0 and prob.cost() == 0.0
        out = prob.minimize_pcg()
        assert (out.trials, out.cost, out.stop) == (0, 0.0, hip.LM_STOP_MAX_TRIALS)


# ---- 2: parity with the reference ---------------------------------------------------------------------------------------
def _check_run(hip, prob, c, out, ref, bound, mask, where, group=0, truncated=False):
    log = out.log
    assert out.trials == ref["trials"] <= lr.TRIALS and out.stop == ref["stop"], where
    assert log["accepted"].tolist() == lr.sequence(ref) and out.accepted == ref["accepted"], where
    worst = worst_rho = 0.0
    for got, want in zip(log, ref["log"]):
        for field in ("lam", "cost", "cost_trial", "predicted", "step_norm", "grad_inf"):
            worst = max(worst, abs(got[field] - want[field]) / abs(want[field]))
            assert _close(got[field], want[field]), (where, field, got[field], want[field])
        amp = max(1.0, want["cost"] / abs(want["cost"] - want["cost_trial"]))
        worst_rho = max(worst_rho, abs(got["rho"] - want["rho"]) / (1e-9 * amp))
        assert abs(got["rho"] - want["rho"]) <= 1e-9 * amp, (where, got["rho"], want["rho"], amp)
        if truncated:
            assert got["cg_status"] == want["cg_status"] and got["cg_iters"] == want["cg_iters"], where
            assert _close(got["cg_rel"], want["cg_rel"], 1e-6), where
        else:
            assert got["cg_status"] == hip.PCG_CONVERGED and got["cg_rel"] <= lr.CG_TOL, where
    assert _close(out.lam, ref["lam"]) and _close(out.cost, ref["cost"]), where
    cams, pts = prob.get_state()
    e_c, e_p = pr.rel(cams, ref["cams"]), pr.rel(pts, ref["pts"])
    print(where, "trials %d rejected %d scalars %.1e rho %.2f of its bound cameras %.1e points %.1e bound %.1e" % (
        out.trials, out.trials - out.accepted, worst, worst_rho, e_c, e_p, bound))
    assert e_c <= bound and e_p <= bound, where
    # invariants
    costs = [log["cost"][0]] + log["cost_trial"][log["accepted"] == 1].tolist()
    assert all(b < a for a, b in zip(costs, costs[1:])) and out.cost == costs[-1], where
    assert prob.cost(group=group) == out.cost, where
    if mask is not None:
        held = np.flatnonzero(mask == 0)
        assert same_bits(cams[held], c.cams[held]), where
    return cams, pts


@pytest.mark.parametrize("loss", lr.LOSSES)
@pytest.mark.parametrize("name", lr.SCENES)
def test_parity(hip, sfm, oracle, name, loss):
    c = pr.case(sfm, name)
    q = oracle.QUIRKS_REFERENCE
    with _problem(hip, c, loss) as prob:
        for l0 in lr.LAMBDA0S:
            for which in lr.MASKS:
                ref, _p, dis = lr.both(sfm, name, q, loss, which, lambda0=l0)
                mask = pr.free_mask(c.n_cams, which)
                prob.set_state(c.cams, c.pts)
                out = prob.minimize_pcg(mask, lambda0=l0, ftol=0.0, cg_tol=lr.CG_TOL, max_trials=lr.TRIALS, quirks=q)
                _check_run(hip, prob, c, out, ref, pr.tolerance(dis), mask, (name, loss, l0, which))


@pytest.mark.parametrize("name", ("6x300", "12x200_tracks"))
def test_parity_with_truncated_cg(hip, sfm, oracle, name):
    """cg_max_iters = 3: every solve ends at the limit with a residual that is not small, so the x.r_cg term of the
    predicted decrease carries weight; against the reference's own PCG truncated in the same way."""
    c = pr.case(sfm, name)
    q = oracle.QUIRKS_REFERENCE
    with _problem(hip, c) as prob:
        for l0 in lr.LAMBDA0S:
            ref = lr.run(sfm, name, "pcg", q, "none", "held01", lambda0=l0, cg_max_iters=3, max_trials=8)
            assert any(r["cg_status"] == pr.PCG_MAX_ITERS and r["cg_rel"] > 1e-6 for r in ref["log"])
            assert min(abs(r["rho"] - lr.MIN_GAIN) for r in ref["log"]) >= 1e-6
            mask = pr.free_mask(c.n_cams, "held01")
            prob.set_state(c.cams, c.pts)
            out = prob.minimize_pcg(mask, lambda0=l0, ftol=0.0, cg_tol=lr.CG_TOL, cg_max_iters=3, max_trials=8, quirks=q)
            _check_run(hip, prob, c, out, ref, 1e-9, mask, (name, "truncated", l0), truncated=True)


# ---- 3: one trial -------------------------------------------------------------------------------------------------------
def test_one_accepted_trial_is_one_outer_iteration(hip, sfm, oracle):
    c = pr.case(sfm, "6x300")
    mask = pr.free_mask(c.n_cams, "held01")
    with _problem(hip, c) as prob:
        prob.set_state(c.cams, c.pts)
        fixed = prob.iterate_pcg(5.0, 1, mask=mask, tol=1e-10, group=8)
        want = prob.get_state()
        prob.set_state(c.cams, c.pts)
        out = prob.minimize_pcg(mask, lambda0=5.0, cg_tol=1e-10, group=8, max_trials=1)
        got = prob.get_state()
        assert out.trials == 1 and out.accepted == 1 and out.stop == hip.LM_STOP_MAX_TRIALS and out.log["accepted"][0] == 1
        assert all(same_bits(x, y) for x, y in zip(got, want))
        assert out.log["cg_iters"][0] == fixed.cg_iters[0] and out.log["cg_rel"][0] == fixed.cg_rel[0]
        assert abs(out.log["cost"][0] - fixed.cost[0]) <= 1e-13 * fixed.cost[0]
        assert out.cost == out.log["cost_trial"][0] == prob.cost(group=8)


def test_one_rejected_trial_restores_the_state(hip, sfm, oracle):
    name, loss, which = "12x200_tracks", "huber", "held01"
    c = pr.case(sfm, name)
    ref = lr.run(sfm, name, "direct", oracle.QUIRKS_REFERENCE, loss, which, lambda0=1e-4)
    k = lr.sequence(ref).index(0)
    cams0, pts0 = ref["states"][k]
    lam = ref["log"][k]["lam"]
    mask = pr.free_mask(c.n_cams, which)
    with _problem(hip, c, loss) as prob, _problem(hip, c, loss) as other:
        for p in (prob, other):
            p.set_state(cams0, pts0)
        before = prob.get_state()
        cost0 = prob.cost()
        out = prob.minimize_pcg(mask, lambda0=lam, ftol=0.0, cg_tol=lr.CG_TOL, max_trials=1)
        assert out.trials == 1 and out.accepted == 0 and out.log["accepted"][0] == 0 and out.stop == hip.LM_STOP_MAX_TRIALS
        want = ref["log"][k]
        amp = max(1.0, want["cost"] / abs(want["cost"] - want["cost_trial"]))
        assert out.log["rho"][0] <= hip.LM_MIN_GAIN and abs(out.log["rho"][0] - want["rho"]) <= 1e-9 * amp
        assert out.lam == 2.0 * lam and out.cost == cost0 == prob.cost()
        assert all(same_bits(x, y) for x, y in zip(prob.get_state(), before))
        # the prepared cameras went back with the state: the next call gives the bits it gives without the rejected trial
        a, b = prob.iterate_pcg(0.5, 2, mask=mask), other.iterate_pcg(0.5, 2, mask=mask)
        assert all(same_bits(x, y) for x, y in zip(prob.get_state(), other.get_state())) and same_bits(a.cost, b.cost)


# ---- 4: invariants ------------------------------------------------------------------------------------------------------
def test_all_cameras_held_and_no_trials(hip, sfm, oracle):
    c = pr.case(sfm, "6x300")
    ref, _p, dis = lr.both(sfm, "6x300", oracle.QUIRKS_REFERENCE, "none", "all_held", lambda0=5.0, max_trials=4)
    mask = pr.free_mask(c.n_cams, "all_held")
    with _problem(hip, c) as prob:
        prob.set_state(c.cams, c.pts)
        out = prob.minimize_pcg(mask, lambda0=5.0, ftol=0.0, cg_tol=lr.CG_TOL, max_trials=4)
        assert out.trials == ref["trials"] == 4 and out.log["accepted"].tolist() == lr.sequence(ref) and out.accepted >= 1
        cams, pts = prob.get_state()
        assert same_bits(cams, c.cams) and not np.array_equal(pts, c.pts)
        assert pr.rel(pts, ref["pts"]) <= pr.tolerance(dis)
        for got, want in zip(out.log, ref["log"]):
            assert got["cg_iters"] == 0 and _close(got["grad_inf"], want["grad_inf"]) and _close(got["predicted"], want["predicted"])
        # max_trials = 0: the cost, and nothing else
        prob.set_state(c.cams, c.pts)
        up = prob.upload_bytes
        out = prob.minimize_pcg(mask, max_trials=0)
        assert (out.trials, out.accepted, out.stop, out.lam) == (0, 0, hip.LM_STOP_MAX_TRIALS, 5.0) and out.log.shape == (0,)
        assert out.cost == prob.cost() and prob.upload_bytes == up
        assert all(same_bits(x, y) for x, y in zip(prob.get_state(), (c.cams, c.pts)))


def test_group_independence_of_the_decisions(hip, sfm, oracle):
    name, loss, which = "hub70", "huber", "held01"
    c = pr.case(sfm, name)
    ref, _p, dis = lr.both(sfm, name, oracle.QUIRKS_REFERENCE, loss, which, lambda0=1e-4)
    mask = pr.free_mask(c.n_cams, which)
    with _problem(hip, c, loss) as prob:
        for group in (1, 8, 64):
            prob.set_state(c.cams, c.pts)
            out = prob.minimize_pcg(mask, lambda0=1e-4, ftol=0.0, cg_tol=lr.CG_TOL, max_trials=lr.TRIALS, group=group)
            _check_run(hip, prob, c, out, ref, pr.tolerance(dis), mask, (name, "group", group), group)
        again = prob.get_state()
        prob.set_state(c.cams, c.pts)
        prob.minimize_pcg(mask, lambda0=1e-4, ftol=0.0, cg_tol=lr.CG_TOL, max_trials=lr.TRIALS, group=64)
        assert all(same_bits(x, y) for x, y in zip(prob.get_state(), again))      # the same call, the same bits


# ---- 5: the stop reasons ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reason", sorted(lr.STOPS))
def test_stop_reasons(hip, sfm, oracle, reason):
    name, loss, which, options = lr.STOPS[reason]
    c = pr.case(sfm, name)
    ref, _p, dis = lr.both(sfm, name, oracle.QUIRKS_REFERENCE, loss, which, **options)
    mask = pr.free_mask(c.n_cams, which)
    opts = dict(ftol=0.0, cg_tol=lr.CG_TOL)
    opts.update(options)
    with _problem(hip, c, loss) as prob:
        prob.set_state(c.cams, c.pts)
        out = prob.minimize_pcg(mask, **opts)
        print(hip.LM_STOP_NAMES[reason], out.trials, out.log["accepted"].tolist(), out.lam)
        assert out.stop == reason == ref["stop"] and out.trials == ref["trials"] and out.log["accepted"].tolist() == lr.sequence(ref)
        assert _close(out.lam, ref["lam"]) and _close(out.cost, ref["cost"])
        assert _close(out.log["grad_inf"][-1], ref["log"][-1]["grad_inf"])
        cams, pts = prob.get_state()
        assert pr.rel(cams, ref["cams"]) <= pr.tolerance(dis) and pr.rel(pts, ref["pts"]) <= pr.tolerance(dis)
        assert prob.cost() == out.cost


def test_an_empty_free_camera(hip, sfm):
    """The empty camera's block is lambda I: it factors at every damping the options allow, its rhs is zero and its location
    does not move.  (Neither SFM_LM_STOP_SINGULAR nor SFM_LM_STOP_BREAKDOWN can be reached on these scenes with lambda > 0:
    `pr.diagonal_block_pivots` gives 0.039 for the weakest block of this scene at lambda = 1e-13.)"""
    c = pr.case(sfm, "empty")
    with _problem(hip, c) as prob:
        prob.set_state(c.cams, c.pts)
        out = prob.minimize_pcg(None, lambda0=5.0, max_trials=3)
        cams, _pts = prob.get_state()
        assert out.trials == 3 and out.bad_camera == -1 and out.stop == hip.LM_STOP_MAX_TRIALS
        assert np.array_equal(cams[pr.EMPTY_CAMERA, 0:3], c.cams[pr.EMPTY_CAMERA, 0:3])


# ---- 6: refusals --------------------------------------------------------------------------------------------------------
def test_refusals(hip, sfm):
    c = pr.case(sfm, "6x300")
    nan, inf = float("nan"), float("inf")
    with _problem(hip, c) as prob:
        prob.set_state(c.cams, c.pts)
        lib, h = prob._lib, prob._h
        bad = [dict(lambda0=0.0), dict(lambda0=nan), dict(lambda_min=0.0), dict(lambda_min=10.0), dict(lambda_max=1.0), dict(lambda_max=inf),
               dict(ftol=-1.0), dict(xtol=nan), dict(gtol=-1.0), dict(cg_tol=0.0), dict(cg_tol=1.0), dict(cg_max_iters=-1),
               dict(max_trials=-1), dict(group=3)]
        for kw in bad:
            opt, _m = hip.check_lm(c.n_cams)
            for k, v in kw.items():
                setattr(opt, k, v)
            assert lib.sfm_ba_minimize_pcg(h, opt, None, None, None, None, None, None, None, None) == hip.E_SHAPE, kw
        assert lib.sfm_ba_minimize_pcg(h, None, None, None, None, None, None, None, None, None) == hip.E_SHAPE
        assert lib.sfm_ba_cost(h, 3, 0, None) == hip.E_SHAPE and lib.sfm_ba_cost(h, 3, 5, None) == hip.E_SHAPE
        with pytest.raises(ValueError):
            prob.minimize_pcg(np.ones(c.n_cams + 1))
        comm = hip.Comm(1, 0, hip.comm_unique_id())
        try:
            prob.set_comm(comm)
            with pytest.raises(ValueError, match="communicator"):
                prob.minimize_pcg()
            with pytest.raises(ValueError, match="communicator"):
                prob.cost()
            prob.set_comm(None)
        finally:
            comm.close()
        assert all(same_bits(x, y) for x, y in zip(prob.get_state(), (c.cams, c.pts)))
        assert prob.minimize_pcg(max_trials=2).trials == 2      # the handle is usable


# ---- 7: the drop-in -----------------------------------------------------------------------------------------------------
class _KP:
    def __init__(self, x, y):
        self.pt = (float(x), float(y))


class _View:
    def __init__(self, rot, loc, k, key_pts):
        self.rot, self.loc, self.k, self.key_pts = rot, loc, k, key_pts

    def update_cam_pose(self, rot, loc):
        self.rot, self.loc = rot, loc


class _Holder:
    pass


def _drop_in(sfm, sc, uv_pix):
    vp, kt = _Holder(), _Holder()
    vp.view_list, kt.track_list = [], []
    tp = sfm.processors.HipTriangulationProcessor(0.5, 30)
    tp.tri_pts = np.vstack((sc.pts_init, np.ones((1, sc.n_pts))))
    bp = sfm.processors.HipBaProcessor(vp, kt, None, tp, None, iteration=20, damping_factor=0.5)
    bp.ba_verbose = False
    for cam in range(sc.n_cams):
        sel = sc.cam_idx == cam
        q = sc.cams_init[cam, 3:7] / np.linalg.norm(sc.cams_init[cam, 3:7])
        keys = [_KP(-1.0, -1.0)] + [_KP(x, y) for x, y in uv_pix[:, sel].T]
        vp.view_list.append(_View(sfm.geometry.quaternion_to_rotation(q), sc.cams_init[cam, 0:3].reshape(3, 1).copy(), sc.intrinsic.copy(), keys))
        track = _Holder()
        track.table = np.full((sc.n_cams, len(keys)), -1, dtype=int)
        track.table[cam, 1:] = sc.pt_idx[sel]
        kt.track_list.append(track)
    return bp, vp, tp


def test_drop_in(hip, sfm):
    """The outlier scene (37 displaced observations) under Huber 5 px: 20 trials from damping_factor = 0.5 leave the clean
    observations no worse than 20 fixed Huber iterations at 0.5 do in NumPy (measured in NumPy: 0.85 px against 1.33 px)."""
    o = sr.outlier_scene(sfm)
    sc = o.scene
    uvn = sfm.geometry.normalise_pixels(o.uv_pix, sc.intrinsic)
    scale = float(np.sqrt(abs(sc.intrinsic[0, 0] * sc.intrinsic[1, 1])))

    def clean_rmse_px(cams, pts):
        r = rr._oracle().obs_terms_vec(np.asarray(cams), np.asarray(pts), sc.cam_idx, sc.pt_idx, uvn)[0]
        return float(scale * np.sqrt(np.mean(np.sum(r * r, axis=1)[~o.displaced])))

    bp, vp, tp = _drop_in(sfm, sc, o.uv_pix)
    cams0 = np.stack([sfm.geometry.pack_camera(v.rot, v.loc) for v in vp.view_list])
    want_c, want_p, _costs = rr.ba_robust(cams0, tp.tri_pts[0:3].copy(), sc.cam_idx, sc.pt_idx, uvn, 0.5, 20, rr.LOSS_HUBER, 5.0 / scale)
    bp.ba_solver, bp.ba_loss = "lm", ("huber", 5.0)
    try:
        bp.execute_bundle_adjustment()
        last = bp.ba_lm_last
        assert last is not None and bp.ba_pcg_last is None and 1 <= last.accepted <= last.trials <= 20
        assert last.log.shape == (last.trials,) and last.stop in (hip.LM_STOP_MAX_TRIALS, hip.LM_STOP_FTOL)
        assert bp._hip_scene.prob.loss() == (hip.LOSS_HUBER, 5.0 / scale)
        cams = np.stack([sfm.geometry.pack_camera(v.rot, v.loc) for v in vp.view_list])
        got, fixed = clean_rmse_px(cams, tp.tri_pts[0:3]), clean_rmse_px(want_c, want_p)
        print("clean RMSE: lm %.3f px in %d trials (%d accepted), 20 fixed iterations %.3f px" % (got, last.trials, last.accepted, fixed))
        assert got <= fixed
    finally:
        bp.ba_release()
    bp, vp, tp = _drop_in(sfm, sc, o.uv_pix)
    bp.ba_solver, bp.ba_resident = "lm", False
    vp.view_list = None
    with pytest.raises(TypeError, match="ba_resident"):
        bp.execute_bundle_adjustment()
