"""NumPy reference of the Levenberg-Marquardt control of the matrix-free bundle adjustment (sfm_ba_minimize_pcg).

The loop is the one include/sfm_hip.h states, built on tests/_pcg_reference.py: every trial takes the reduced system of
``pr.system`` at the current damping, solves it by ``pr.solve_direct`` or ``pr.solve_pcg`` (``route``), applies the step with
``pr.apply_step`` and judges it by the cost of the trial state.  ``predicted`` is the dense definition
|r|^2 - |r - J h|^2 summed over the observations (each term formed as (J h).(2 r - J h), which is the same number without
the cancellation); ``predicted_closed`` is the closed form the device evaluates.  The rows of the log carry the fields of
``sfm_lm_trial`` under the names of ``native.LmTrial``.

The settings the host test measures and the device test is held to are defined here once; ``run`` computes a setting once
per route and leaves it unchanged."""
import numpy as np

import _pcg_reference as pr
import _robust_reference as rr

MIN_GAIN = 1e-3
STOP_MAX_TRIALS, STOP_FTOL, STOP_XTOL, STOP_GTOL, STOP_LAMBDA_MAX, STOP_BREAKDOWN, STOP_SINGULAR = 0, 1, 2, 3, 4, 5, 6

SCENES = ("6x300", "12x200_tracks", "hub70", "empty", "260")
LAMBDA0S = (5.0, 1e-4)
LOSSES = pr.LOSSES
MASKS = ("held01", "last3")
TRIALS = 12
CG_TOL = 1e-13
FIELDS = ("lam", "cost", "cost_trial", "predicted", "rho", "step_norm", "grad_inf", "cg_rel", "cg_iters", "cg_status", "accepted")

# One setting per stop reason: (scene, loss, mask, options).  The thresholds were chosen from the reference's own logs so
# that the deciding quantity is a factor 2 or more past the threshold at the stopping trial and a factor 2 or more short of
# it at every earlier one (tests/test_lm_host.py asserts both).
STOPS = {
    STOP_FTOL: ("6x300", "none", "held01", dict(lambda0=5.0, ftol=0.06, max_trials=10)),             # trial 1: 0.028 after 0.71
    STOP_XTOL: ("6x300", "cauchy", "last3", dict(lambda0=1e-4, xtol=2e-3, max_trials=10)),           # trial 6: 3.7e-4 after >= 9.6e-3
    STOP_GTOL: ("6x300", "none", "held01", dict(lambda0=5.0, gtol=1.0, max_trials=10)),              # trial 1: 0.41 after 11
    STOP_LAMBDA_MAX: ("hub70", "huber", "held01", dict(lambda0=1e-4, lambda_max=1.3e-4, max_trials=10)),      # trial 2 is the first rejection: 2.66e-4
    STOP_MAX_TRIALS: ("6x300", "none", "held01", dict(lambda0=5.0, max_trials=3)),
}


def state_cost(c, cams, pts, loss):
    return rr.state_cost(cams, pts, c.cam_idx, c.pt_idx, c.uv, pr.loss_kind(loss), c.delta)


def minimize(c, route, quirks, loss="none", which="none", lambda0=5.0, lambda_min=1e-8, lambda_max=1e8, ftol=0.0, xtol=0.0,
             gtol=0.0, cg_tol=CG_TOL, cg_max_iters=None, max_trials=TRIALS, cams=None, pts=None):
    """dict(cams, pts, log, trials, accepted, stop, lam, cost, states): ``log`` a list of dicts with FIELDS and
    ``predicted_closed``; ``states[i]`` the (cams, pts) trial i started from."""
    assert route in ("direct", "pcg")
    mask = pr.free_mask(c.n_cams, which)
    cams = np.array(c.cams if cams is None else cams, dtype=np.float64).reshape(-1, 7)
    pts = np.array(c.pts if pts is None else pts, dtype=np.float64)
    _free, rows = pr._free_rows(c.n_cams, mask)
    lam, nu = float(lambda0), 2.0
    cost = state_cost(c, cams, pts, loss)
    log, states, accepted, stop = [], [], 0, STOP_MAX_TRIALS
    for _trial in range(max_trials):
        t = pr.system(c, cams, pts, lam, quirks, loss)
        grad = max(float(np.max(np.abs(t["rhs"][rows]))) if rows.size else 0.0, float(np.max(np.abs(t["ex"]))))
        states.append((cams.copy(), pts.copy()))
        row = dict.fromkeys(FIELDS, 0.0)
        row.update(lam=lam, cost=cost, cost_trial=cost, grad_inf=grad, cg_iters=0, cg_status=pr.PCG_CONVERGED, accepted=0,
                   predicted_closed=0.0)
        if gtol > 0 and grad <= gtol:
            log.append(row)
            stop = STOP_GTOL
            break
        if route == "direct":
            dp, count, status, cg_rel = pr.solve_direct(t, c.n_cams, mask), 0, pr.PCG_CONVERGED, 0.0
        else:
            dp, count, status, hist = pr.solve_pcg(t, c.n_cams, mask, cg_tol, cg_max_iters)
            cg_rel = float(np.sqrt(hist[-1] / hist[0])) if hist[0] > 0 else 0.0
            if status == pr.PCG_BREAKDOWN:
                states.pop()
                stop = STOP_BREAKDOWN
                break
        cams_t, pts_t = pr.apply_step(t, cams, pts, c.cam_idx, c.pt_idx, dp, mask)
        x = dp.reshape(-1, 7)
        btd = np.zeros_like(t["ex"])
        np.add.at(btd, c.pt_idx, np.einsum('mij,mi->mj', t["W"], x[c.cam_idx]))
        dx = np.einsum('pij,pj->pi', t["D_inv"], t["ex"] - btd)
        jh = np.einsum('mki,mi->mk', t["Jp"], x[c.cam_idx]) + np.einsum('mki,mi->mk', t["Jx"], dx[c.pt_idx])
        predicted = float(np.sum(jh * (2.0 * t["r"] - jh)))
        h2 = float(dp @ dp + np.sum(dx * dx))
        r_cg = t["rhs"][rows] - t["S"][np.ix_(rows, rows)] @ dp[rows] if rows.size else np.zeros(0)
        closed = float(np.einsum('pi,pij,pj->', t["ex"], t["D_inv"], t["ex"]) + dp[rows] @ t["rhs"][rows] + dp[rows] @ r_cg + lam * h2)
        cost_t = state_cost(c, cams_t, pts_t, loss)
        rho = (cost - cost_t) / predicted if predicted != 0 else float("nan")
        ok = bool(predicted > 0 and np.isfinite(cost_t) and rho > MIN_GAIN)
        row.update(cost_trial=cost_t, predicted=predicted, predicted_closed=closed, rho=rho, step_norm=float(np.sqrt(h2)),
                   cg_rel=cg_rel, cg_iters=count, cg_status=status, accepted=int(ok))
        log.append(row)
        if ok:
            f = 2.0 * rho - 1.0
            lam, nu = max(lambda_min, lam * max(1.0 / 3.0, 1.0 - f * f * f)), 2.0
            accepted += 1
            state_norm = float(np.sqrt(np.sum(cams * cams) + np.sum(pts * pts)))
            if ftol > 0 and cost - cost_t <= ftol * cost:
                stop = STOP_FTOL
            elif xtol > 0 and row["step_norm"] <= xtol * (state_norm + xtol):
                stop = STOP_XTOL
            row["state_norm"] = state_norm
            cams, pts, cost = cams_t, pts_t, cost_t
            if stop != STOP_MAX_TRIALS:
                break
        else:
            lam, nu = lam * nu, 2.0 * nu
            if lam > lambda_max:
                stop = STOP_LAMBDA_MAX
                break
    return dict(cams=cams, pts=pts, log=log, trials=len(log), accepted=accepted, stop=stop, lam=lam, cost=cost, states=states)


_RUNS = {}


def run(sfm, name, route, quirks, loss, which, **options):
    """``minimize`` from the case's start state, once per setting and route, left unchanged."""
    key = (name, route, quirks, loss, which, tuple(sorted(options.items())))
    if key not in _RUNS:
        out = minimize(pr.case(sfm, name), route, quirks, loss, which, **options)
        out["cams"].setflags(write=False)
        out["pts"].setflags(write=False)
        _RUNS[key] = out
    return _RUNS[key]


def table_settings():
    """(scene, lambda0, loss, mask) of the host table and the device parity test."""
    return [(n, l0, loss, which) for n in SCENES for l0 in LAMBDA0S for loss in LOSSES for which in MASKS]


def both(sfm, name, quirks, loss, which, **options):
    """The two routes of one setting and the disagreement of their final states (``pr.rel``)."""
    d, p = run(sfm, name, "direct", quirks, loss, which, **options), run(sfm, name, "pcg", quirks, loss, which, **options)
    return d, p, max(pr.rel(p["cams"], d["cams"]), pr.rel(p["pts"], d["pts"]))


def sequence(out):
    return [r["accepted"] for r in out["log"]]
