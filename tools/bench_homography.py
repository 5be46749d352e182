#!/usr/bin/env python3
"""Timing of the robust homography (sfm_homography_ransac -> homography_norm_kernel, homography_hyp_kernel,
homography_score_kernel, homography_pick_kernel, homography_refit_kernel, homography_judge_kernel) on

    1x2000   one pair of views, 2 000 matches
    9x8000   a new view of 8 000 matches against nine resident views, in one call

each at max_hyp 32 and 128 with two refit rounds, and next to each sfm_twoview_ransac on the same arrays in the same run:
what processors.classify_matches pays for its second model.  Matches: focal 800, points on the plane
z = 6.5 + 0.1 x + 0.05 y, 0.5 px noise on both keys, a tenth of the right keys displaced by 30 - 120 px; threshold 2 px.
Both are the host-array forms: a call uploads its coordinates, runs its kernels, downloads its outputs and synchronises.

A timed region is `inner` back-to-back calls (at least 0.1 s); the figure is the MEDIAN over the regions of region time /
inner, the spread is (max - min) / median over the same regions.  The two calls are timed alternately, twice each, and both
rounds are kept: the difference between the rounds of one call is the run-to-run spread a difference between the two calls
has to exceed.  `tests_per_call` = hypotheses x matches is an upper bound of the transfer tests of the scoring kernel (an
invalid hypothesis is skipped); FLOP_PER_TEST counts a FMA as two.

    python tools/bench_homography.py [--cases 1x2000,9x8000] [--max-hyp 32,128] [--regions 7] [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2 and one
case, and read the homography_* and twoview_* rows.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tri_ransac import time_call  # noqa: E402  (the same regions)

MAX_PX, ITERS, REGION_S = 2.0, 2, 0.1
FLOP_PER_TEST = 42      # per half: three rows of two FMAs (12), eu and ev (4), lhs (3), w^2 and rhs (2)


def plane_matches(n, frac, seed, noise=0.5):
    rng = np.random.default_rng(seed)
    k = np.array([[800.0, 0, 320], [0, 800.0, 240], [0, 0, 1]])
    x = rng.uniform(-2, 2, (2, n))
    x = np.vstack((x, 6.5 + 0.1 * x[0] + 0.05 * x[1]))
    a = 0.15
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    left = k @ x
    left = left[:2] / left[2]
    right = k @ (rot @ x + np.array([[-1.0], [0.1], [0.2]]))
    right = right[:2] / right[2]
    left = left + rng.normal(0, noise, left.shape)
    right = right + rng.normal(0, noise, right.shape)
    bad = rng.random(n) < frac
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(30, 120, n)
    return left, right + bad * np.vstack((np.cos(ang), np.sin(ang))) * mag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x2000,9x8000")
    ap.add_argument("--max-hyp", default="32,128")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_homography.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"max_px": MAX_PX, "iters": ITERS, "regions": args.regions, "region_s": REGION_S, "flop_per_test": FLOP_PER_TEST, "cases": {}}
    for case in args.cases.split(","):
        n_sets, n = (int(v) for v in case.split("x"))
        parts = [plane_matches(n, 0.1, 100 + s) for s in range(n_sets)]
        set_ptr = np.arange(n_sets + 1, dtype=np.int32) * n
        left = np.ascontiguousarray(np.hstack([p[0] for p in parts]))
        right = np.ascontiguousarray(np.hstack([p[1] for p in parts]))
        entry = {"n_sets": n_sets, "matches_per_set": n, "runs": []}
        for max_hyp in [int(h) for h in args.max_hyp.split(",")]:
            def homography():
                return native.homography_ransac(set_ptr, left, right, MAX_PX ** 2, max_hyp, ITERS)

            def twoview():
                return native.twoview_ransac(set_ptr, left, right, MAX_PX ** 2, max_hyp, ITERS)

            run = {"max_hyp": max_hyp, "tests_per_call": int(n_sets * max_hyp * n),
                   "homography_summary": dict(zip(native.HOMOGRAPHY_SUMMARY, homography()[5].tolist())),
                   "twoview_summary": dict(zip(native.TWOVIEW_SUMMARY, twoview()[5].tolist())),
                   "homography_ransac": [], "twoview_ransac": []}
            for _round in range(2):                            # alternately, so that a drift of the machine shows in both
                run["homography_ransac"].append(time_call(homography, lambda: None, args.regions, REGION_S))
                run["twoview_ransac"].append(time_call(twoview, lambda: None, args.regions, REGION_S))
            entry["runs"].append(run)
        out["cases"][case] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
