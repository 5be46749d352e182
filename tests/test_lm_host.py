"""Host-side checks of the Levenberg-Marquardt control of the matrix-free bundle adjustment (sfm_ba_cost,
sfm_ba_minimize_pcg): the interface that needs no device, and what the NumPy reference of tests/_lm_reference.py does on
the settings the device test holds the library to -- with the margins that make the accept / reject sequence and the stop
reasons quantities a device can be held to exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

import _lm_reference as lr
import _pcg_reference as pr

from conftest import REPO


# ---- the interface ------------------------------------------------------------------------------------------------------
def test_abi(sfm):
    native = sfm.native
    text = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    for name, value in (("SFM_LM_STOP_MAX_TRIALS", 0), ("SFM_LM_STOP_FTOL", 1), ("SFM_LM_STOP_XTOL", 2), ("SFM_LM_STOP_GTOL", 3),
                        ("SFM_LM_STOP_LAMBDA_MAX", 4), ("SFM_LM_STOP_BREAKDOWN", 5), ("SFM_LM_STOP_SINGULAR", 6)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert re.search(r"#define\s+SFM_LM_MIN_GAIN\s+1e-3\b", text) and native.LM_MIN_GAIN == 1e-3 == lr.MIN_GAIN
    assert (native.LM_STOP_MAX_TRIALS, native.LM_STOP_FTOL, native.LM_STOP_XTOL, native.LM_STOP_GTOL, native.LM_STOP_LAMBDA_MAX,
            native.LM_STOP_BREAKDOWN, native.LM_STOP_SINGULAR) == (0, 1, 2, 3, 4, 5, 6)
    assert (lr.STOP_MAX_TRIALS, lr.STOP_FTOL, lr.STOP_XTOL, lr.STOP_GTOL, lr.STOP_LAMBDA_MAX, lr.STOP_BREAKDOWN,
            lr.STOP_SINGULAR) == (0, 1, 2, 3, 4, 5, 6)
    assert re.search(r"typedef struct sfm_lm_options\s*\{", text) and re.search(r"typedef struct sfm_lm_trial\s*\{", text)
    for name in ("sfm_ba_cost", "sfm_ba_minimize_pcg", "sfm_lm_options_default", "sfm_lm_trial_size"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text) and name in native.EXPORTS
    # the fields of the two structures, in the header's order
    for struct, cls in (("sfm_lm_options", native.LmOptions), ("sfm_lm_trial", native.LmTrial)):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                kind, names = decl.split(None, 1)
                fields += [(n.strip(), kind) for n in names.split(",")]
        want = [("lam" if n == "lambda" else n, ctypes.c_double if k == "double" else ctypes.c_int) for n, k in fields]
        assert [(n, t) for n, t in cls._fields_] == want, struct
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = native.load()
    opt = native.LmOptions()
    assert lib.sfm_lm_options_default(ctypes.byref(opt)) == ctypes.sizeof(native.LmOptions)
    assert lib.sfm_lm_trial_size() == ctypes.sizeof(native.LmTrial) == native.LM_TRIAL_DTYPE.itemsize
    assert lib.sfm_lm_options_default(None) == 0
    got = {name: getattr(opt, name) for name, _t in native.LmOptions._fields_}
    assert got == dict(lambda0=5.0, lambda_min=1e-8, lambda_max=1e8, ftol=1e-8, xtol=0.0, gtol=0.0, cg_tol=1e-10, cg_max_iters=0,
                       max_trials=50, quirks=native.QUIRKS_REFERENCE, group=0) == native.LM_DEFAULTS
    assert hasattr(native.BaProblem, "cost") and hasattr(native.BaProblem, "minimize_pcg")
    mixin = sfm.processors.HipBaMixin
    assert (mixin.ba_solver, mixin.ba_hold_views, mixin.ba_pcg_tol, mixin.ba_pcg_max_iters) == ("dense", None, 1e-10, 0)
    assert (mixin.ba_lm_ftol, mixin.ba_lm_xtol, mixin.ba_lm_gtol, mixin.ba_lm_last) == (1e-8, 0.0, 0.0, None)


def test_check_lm_rejects_bad_arguments(sfm):
    check = sfm.native.check_lm
    opt, mask = check(6)
    assert mask is None and {n: getattr(opt, n) for n, _t in sfm.native.LmOptions._fields_} == sfm.native.LM_DEFAULTS
    opt, mask = check(6, [1, 0, 1, 1, 2, 1], lambda0=1e-4, max_trials=0, group=8, xtol=1e-6)
    assert (opt.lambda0, opt.max_trials, opt.group, opt.xtol) == (1e-4, 0, 8, 1e-6) and mask.tolist() == [1, 0, 1, 1, 1, 1]
    nan, inf = float("nan"), float("inf")
    bad = [dict(lambda0=0.0), dict(lambda0=-1.0), dict(lambda0=nan), dict(lambda0=inf, lambda_max=inf), dict(lambda_min=0.0),
           dict(lambda_min=10.0), dict(lambda_max=1.0), dict(lambda_max=inf), dict(lambda_min=nan), dict(ftol=-1e-9), dict(ftol=nan),
           dict(xtol=-1.0), dict(xtol=nan), dict(gtol=-1.0), dict(gtol=nan), dict(cg_tol=0.0), dict(cg_tol=1.0), dict(cg_tol=nan),
           dict(cg_max_iters=-1), dict(cg_max_iters=2.5), dict(max_trials=-1), dict(max_trials=1.5), dict(max_trials=True), dict(max_trials=float("inf")),
           dict(cg_max_iters=float("inf")), dict(max_trials=float("nan")),
           dict(group=2), dict(group=128), dict(group=-1), dict(mask=[1, 1, 1]), dict(mask=np.ones(7)), dict(trials=3)]
    for kw in bad:
        with pytest.raises(ValueError):
            check(6, **kw)


def test_mixin_checks_lm_before_anything_is_read(sfm):
    class Host(sfm.processors.HipBaMixin):
        damping_factor, iteration = 5.0, 7

    h = Host()
    h.ba_solver = "lm"
    assert h.ba_pcg_native() == (None,)
    assert h.ba_pcg_native(4)[0] is None
    h.ba_hold_views = (1, 3)
    assert h.ba_pcg_native(4)[0].tolist() == [1, 0, 1, 0]
    o = h.ba_lm_options()
    assert (o["lambda0"], o["max_trials"], o["ftol"], o["cg_tol"]) == (5.0, 7, 1e-8, 1e-10)
    h.ba_lm_ftol = -1.0
    with pytest.raises(ValueError):
        h.ba_pcg_native()
    h.ba_lm_ftol, h.ba_resident = 1e-8, False
    with pytest.raises(TypeError, match="ba_resident"):
        h.ba_pcg_native()
    h.ba_resident, h.ba_solver = True, "newton"
    with pytest.raises(ValueError):
        h.ba_pcg_native()


# ---- the reference's behaviour ------------------------------------------------------------------------------------------
def _print_log(out):
    for i, r in enumerate(out["log"]):
        print("   %2d %s lambda %.3e F %.6e F_trial %.6e predicted %.3e rho %+.4f |h| %.2e grad %.2e cg %d" % (
            i, "+" if r["accepted"] else "-", r["lam"], r["cost"], r["cost_trial"], r["predicted"], r["rho"], r["step_norm"],
            r["grad_inf"], r["cg_iters"]))


@pytest.mark.parametrize("name", lr.SCENES)
def test_reference_table(sfm, oracle, name):
    """Per setting of the table: the two NumPy routes take the same accept / reject sequence; no gain ratio comes closer
    than 1e-6 to SFM_LM_MIN_GAIN (measured: 4.6e-3 at the closest, `6x300`, Cauchy, `last3`, lambda0 = 1e-4); the accepted
    costs strictly decrease; the closed form of the predicted decrease equals the dense definition to 1e-10 (measured:
    9.2e-15).  Printed: trials, rejections, final cost and the disagreement of the two routes in the final state, which the
    device test's bound is made of (measured: at most 1.1e-11, `empty`, Cauchy, `last3`, lambda0 = 1e-4)."""
    q = oracle.QUIRKS_REFERENCE
    print("\n%-14s %7s %-7s %-7s %6s %4s %12s %9s %9s %9s" % ("scene", "lambda0", "loss", "mask", "trials", "rej", "final cost",
                                                          "disagree", "margin", "pred err"))
    for scene, l0, loss, which in lr.table_settings():
        if scene != name:
            continue
        d, p, dis = lr.both(sfm, scene, q, loss, which, lambda0=l0)
        rows = d["log"] + p["log"]
        margin = min(abs(r["rho"] - lr.MIN_GAIN) for r in rows)
        pred = max(abs(r["predicted_closed"] - r["predicted"]) / abs(r["predicted"]) for r in rows)
        print("%-14s %7g %-7s %-7s %6d %4d %12.5e %9.2e %9.2e %9.2e" % (scene, l0, loss, which, d["trials"], d["trials"] - d["accepted"],
                                                                     d["cost"], dis, margin, pred))
        where = (scene, l0, loss, which)
        assert lr.sequence(d) == lr.sequence(p) and d["stop"] == p["stop"] == lr.STOP_MAX_TRIALS and d["trials"] == lr.TRIALS, where
        assert margin >= 1e-6, where
        assert pred <= 1e-10, where
        for out in (d, p):
            costs = [out["log"][0]["cost"]] + [r["cost_trial"] for r in out["log"] if r["accepted"]]
            assert all(b < a for a, b in zip(costs, costs[1:])), where
            assert out["cost"] == costs[-1], where


def test_rejections_are_exercised(sfm, oracle):
    """At least three settings reject at least one trial (measured: 50 of the 60, up to 8 of 12 trials)."""
    q = oracle.QUIRKS_REFERENCE
    counts = {}
    for scene, l0, loss, which in lr.table_settings():
        if scene in ("hub70", "12x200_tracks") and loss == "huber" and l0 == 1e-4:
            d = lr.run(sfm, scene, "direct", q, loss, which, lambda0=l0)
            counts[(scene, which)] = d["trials"] - d["accepted"]
    print(counts)
    assert sum(1 for v in counts.values() if v >= 1) >= 3 and max(counts.values()) >= 6


@pytest.mark.parametrize("name", lr.SCENES)
def test_predicted_decrease_with_truncated_cg(sfm, oracle, name):
    """cg_max_iters = 3 on every setting of the table: the CG residual is not small, and the closed form's x.r_cg term
    carries it.  (With three free cameras and good damping three iterations can converge; the scene as a whole must
    have trials that end at the limit with a residual above 1e-6.)"""
    worst, truncated = 0.0, 0
    for scene, l0, loss, which in lr.table_settings():
        if scene != name:
            continue
        out = lr.run(sfm, scene, "pcg", oracle.QUIRKS_REFERENCE, loss, which, lambda0=l0, cg_max_iters=3)
        assert out["trials"] == lr.TRIALS
        truncated += sum(1 for r in out["log"] if r["cg_status"] == pr.PCG_MAX_ITERS and r["cg_rel"] > 1e-6)
        for r in out["log"]:
            worst = max(worst, abs(r["predicted_closed"] - r["predicted"]) / abs(r["predicted"]))
            assert abs(r["predicted_closed"] - r["predicted"]) <= 1e-10 * abs(r["predicted"]), (scene, l0, loss, which, r)
    print(name, "worst closed form against the dense definition, truncated CG: %.1e over %d truncated trials" % (worst, truncated))
    assert truncated >= lr.TRIALS


def deciding_quantities(out, reason, options):
    """Per trial of a reference log, the ratio quantity / threshold of the rule ``reason`` (None where the rule is not
    evaluated): <= 1 stops.  LAMBDA_MAX is turned round (threshold / quantity), so that <= 1 stops there too."""
    ratios = []
    lam_next = [r["lam"] for r in out["log"][1:]] + [out["lam"]]
    for r, nxt in zip(out["log"], lam_next):
        if reason == lr.STOP_FTOL:
            ratios.append((r["cost"] - r["cost_trial"]) / (options["ftol"] * r["cost"]) if r["accepted"] else None)
        elif reason == lr.STOP_XTOL:
            ratios.append(r["step_norm"] / (options["xtol"] * (r["state_norm"] + options["xtol"])) if r["accepted"] else None)
        elif reason == lr.STOP_GTOL:
            ratios.append(r["grad_inf"] / options["gtol"])
        elif reason == lr.STOP_LAMBDA_MAX:
            ratios.append(None if r["accepted"] else options["lambda_max"] / nxt)
    return ratios


@pytest.mark.parametrize("reason", sorted(lr.STOPS))
def test_one_setting_per_stop_reason(sfm, oracle, reason):
    scene, loss, which, options = lr.STOPS[reason]
    d, p, _dis = lr.both(sfm, scene, oracle.QUIRKS_REFERENCE, loss, which, **options)
    print()
    _print_log(d)
    assert d["stop"] == p["stop"] == reason and lr.sequence(d) == lr.sequence(p)
    if reason == lr.STOP_MAX_TRIALS:
        assert d["trials"] == options["max_trials"]
        return
    assert 1 < d["trials"] < options["max_trials"]            # the rule decided, after at least one trial that went on
    for out in (d, p):
        ratios = [x for x in deciding_quantities(out, reason, options) if x is not None]
        print("quantity / threshold per trial:", ["%.3g" % x for x in ratios])
        assert ratios[-1] <= 0.5 and all(x >= 2.0 for x in ratios[:-1]), ratios


@pytest.mark.parametrize("name", ("12x200_tracks", "hub70", "tracks40"))
def test_value(sfm, oracle, name):
    """15 trials from lambda0 = 5 end below half the cost that 15 iterations at the fixed lambda = 5 reach (cameras 0 and 1
    held, no loss, quirks 0)."""
    c = pr.case(sfm, name)
    cams, pts = c.cams, c.pts
    for _ in range(15):
        cams, pts, _cost = pr.step_direct(c, cams, pts, 5.0, 0, "none", pr.free_mask(c.n_cams, "held01"))
    fixed = lr.state_cost(c, cams, pts, "none")
    out = lr.run(sfm, name, "direct", 0, "none", "held01", lambda0=5.0, max_trials=15)
    print(name, "start %.3e fixed %.3e adaptive %.3e (%.1fx), %d rejected" % (out["log"][0]["cost"], fixed, out["cost"], fixed / out["cost"],
                                                                         out["trials"] - out["accepted"]))
    assert out["cost"] < 0.5 * fixed
