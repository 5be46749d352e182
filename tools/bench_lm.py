#!/usr/bin/env python3
"""Timing of the Levenberg-Marquardt control (sfm_ba_minimize_pcg) against the fixed-damping outer iteration it is built on
(sfm_ba_iterate_pcg, unchanged code: the yardstick), on the scenes of tools/bench_pcg.py: C3, C4share, tracks1000.

Per scene:

  * wall milliseconds per trial of ``minimize_pcg`` against wall milliseconds per outer iteration of ``iterate_pcg``, the two
    alternating region by region in one process, each region `iters` trials / iterations from the same start state at
    lambda = 5 with cg_tol = 1e-10.  lambda_min = lambda0 pins the damping while the gain ratio stays above one half (the
    dampings the trials used are recorded); the MEDIAN over the regions and the spread (max - min) / median;
  * the wall time of one ``cost`` call (a blocking call: the ba_cost kernel, the reduction, one 8-byte read and the
    synchronisation -- an upper bound of the kernel's device time), median of `cost_calls`;
  * the bytes the three state copies of a trial move (cameras 56 B, prepared cameras 152 B, points 24 B, read and written);
  * the trials and milliseconds ``minimize_pcg`` (lambda0 = 5, default bounds) takes to reach the cost that 15 iterations of
    ``iterate_pcg`` at lambda = 5 reach, and the milliseconds of those 15 iterations.

    python tools/bench_lm.py [--shapes C3,C4share,tracks1000] [--regions 7] [--iters 3] [--out profiles/lm/bench_lm.json]

Prints one JSON line (and rewrites --out after every scene)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pcg import make_shape, region      # noqa: E402  (the same scenes, the same timed region)

LAM, TOL = 5.0, 1e-10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C4share,tracks1000")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3, help="trials / outer iterations per region")
    ap.add_argument("--cost-calls", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"regions": args.regions, "iters": args.iters, "lambda": LAM, "cg_tol": TOL, "shapes": {}}

    def dump():
        line = json.dumps(out)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    for name in args.shapes.split(","):
        sc = make_shape(sfm, name)
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        m, n, v = sc.n_obs, sc.n_pts, sc.n_cams
        entry = {"n_cams": v, "n_pts": n, "n_obs": m, "state_copy_bytes": 2 * (56 * v + 152 * v + 24 * n),
                 "cost_read_bytes": 20 * m + 24 * n + 152 * v}
        with native.BaProblem(v, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            last = {}

            def reset():
                prob.set_state(sc.cams_init, sc.pts_init)

            def fixed():
                last["fixed"] = prob.iterate_pcg(LAM, args.iters, tol=TOL)

            def lm():
                last["lm"] = prob.minimize_pcg(lambda0=LAM, lambda_min=LAM, ftol=0.0, cg_tol=TOL, max_trials=args.iters)

            region(lm, reset, native.synchronize)                 # warm-up: code objects, camera-major list, pool blocks
            region(fixed, reset, native.synchronize)
            t_lm, t_fixed = [], []
            for _ in range(args.regions):                         # alternating
                t_lm.append(region(lm, reset, native.synchronize))
                t_fixed.append(region(fixed, reset, native.synchronize))
            t_lm, t_fixed = np.array(t_lm) / args.iters, np.array(t_fixed) / args.iters
            log = last["lm"].log
            reset()
            prob.cost()
            t_cost = []
            for _ in range(args.cost_calls):
                t0 = time.perf_counter()
                prob.cost()
                t_cost.append(time.perf_counter() - t0)
            entry.update(lm_ms_per_trial=float(np.median(t_lm) * 1e3), lm_spread=float((t_lm.max() - t_lm.min()) / np.median(t_lm)),
                         fixed_ms_per_iteration=float(np.median(t_fixed) * 1e3),
                         fixed_spread=float((t_fixed.max() - t_fixed.min()) / np.median(t_fixed)),
                         lm_over_fixed=float(np.median(t_lm) / np.median(t_fixed)),
                         overhead_ms_per_trial=float((np.median(t_lm) - np.median(t_fixed)) * 1e3),
                         cost_call_ms=float(np.median(t_cost) * 1e3), cost_call_min_ms=float(np.min(t_cost) * 1e3),
                         lm_lambdas=[float(x) for x in log["lam"]], lm_accepted=[int(x) for x in log["accepted"]],
                         lm_cg_iters=[int(x) for x in log["cg_iters"]], fixed_cg_iters=[int(x) for x in last["fixed"].cg_iters])
            # the cost 15 fixed iterations reach, and what the controlled minimisation needs to get there
            t15 = region(lambda: prob.iterate_pcg(LAM, 15, tol=TOL), reset, native.synchronize)
            target = prob.cost()
            reset()
            start = prob.cost()
            full = prob.minimize_pcg(lambda0=LAM, ftol=0.0, cg_tol=TOL, max_trials=50)
            reached = [i + 1 for i, r in enumerate(full.log) if r["accepted"] and r["cost_trial"] <= target]
            entry.update(start_cost=start, fixed15_cost=target, fixed15_ms=float(t15 * 1e3), lm50_cost=full.cost,
                         lm50_rejected=int(full.trials - full.accepted), lm50_stop=native.LM_STOP_NAMES[full.stop],
                         trials_to_fixed15_cost=reached[0] if reached else None)
            if reached:
                k = reached[0]
                t_k = [region(lambda: prob.minimize_pcg(lambda0=LAM, ftol=0.0, cg_tol=TOL, max_trials=k), reset, native.synchronize)
                       for _ in range(3)]
                entry["ms_to_fixed15_cost"] = float(np.median(t_k) * 1e3)
        out["shapes"][name] = entry
        print("%s: lm %.3f ms / trial, fixed %.3f ms / iteration, cost call %.3f ms, %s trials to the cost of 15 iterations" % (
            name, entry["lm_ms_per_trial"], entry["fixed_ms_per_iteration"], entry["cost_call_ms"], entry["trials_to_fixed15_cost"]),
            file=sys.stderr, flush=True)
        dump()
    print(dump())


if __name__ == "__main__":
    main()
