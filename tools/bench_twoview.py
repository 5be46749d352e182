#!/usr/bin/env python3
"""Timing of the robust two-view geometry (sfm_twoview_ransac -> twoview_norm_kernel, twoview_hyp_kernel,
twoview_score_kernel, twoview_pick_kernel, twoview_refit_kernel, twoview_judge_kernel) on

    1x2000   one set of 2 000 matches
    1x8000   one set of 8 000 matches
    9x8000   nine sets of 8 000 matches          (a new view against nine resident ones)

each at max_hyp 128 and 1 024 with two refit rounds, and next to each the existing sfm_fundamental_ransac at the same
number of hypotheses, called once per set with samples drawn beforehand.  Matches: focal 800, points 4 - 9 units deep,
0.5 px noise on both keys, a tenth of the right keys displaced by 30 - 120 px; threshold 2 px (4 px^2).  Both are the
host-array forms: a call uploads its coordinates, runs its kernels, downloads its outputs and synchronises.

A timed region is `inner` back-to-back calls; the figure is the MEDIAN over the regions of region time / inner, the spread
is (max - min) / median over the same regions.  `tests_per_call` = hypotheses x matches is an upper bound of the Sampson
tests of the scoring kernel (an invalid hypothesis is skipped); FLOP_PER_TEST counts a FMA as two and the division as one.

    python tools/bench_twoview.py [--cases 1x2000,1x8000,9x8000] [--max-hyp 128,1024] [--regions 7] [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2 and one
case, and read the twoview_* rows.
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

MAX_PX, ITERS, PARENT_THRESHOLD = 2.0, 2, 1e-2
FLOP_PER_TEST = 33      # six two-term FMAs chains (24), den (7), e^2 and the division (2)


def matches(n, frac, seed, noise=0.5):
    rng = np.random.default_rng(seed)
    k = np.array([[800.0, 0, 320], [0, 800.0, 240], [0, 0, 1]])
    x = np.vstack((rng.uniform(-2, 2, (2, n)), rng.uniform(4, 9, (1, n))))
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
    ap.add_argument("--cases", default="1x2000,1x8000,9x8000")
    ap.add_argument("--max-hyp", default="128,1024")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_twoview.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"max_px": MAX_PX, "iters": ITERS, "regions": args.regions, "parent_threshold": PARENT_THRESHOLD,
           "flop_per_test": FLOP_PER_TEST, "cases": {}}
    for case in args.cases.split(","):
        n_sets, n = (int(v) for v in case.split("x"))
        parts = [matches(n, 0.1, 100 + s) for s in range(n_sets)]
        set_ptr = np.arange(n_sets + 1, dtype=np.int32) * n
        left = np.ascontiguousarray(np.hstack([p[0] for p in parts]))
        right = np.ascontiguousarray(np.hstack([p[1] for p in parts]))
        entry = {"n_sets": n_sets, "matches_per_set": n, "runs": []}
        for max_hyp in [int(h) for h in args.max_hyp.split(",")]:
            report = native.twoview_ransac(set_ptr, left, right, MAX_PX ** 2, max_hyp, ITERS)
            run = time_call(lambda: native.twoview_ransac(set_ptr, left, right, MAX_PX ** 2, max_hyp, ITERS), lambda: None,
                            args.regions)
            run["max_hyp"] = max_hyp
            run["summary"] = dict(zip(native.TWOVIEW_SUMMARY, report[5].tolist()))
            run["tests_per_call"] = int(n_sets * max_hyp * n)
            rng = np.random.default_rng(7)
            samples = [np.stack([rng.choice(n, 8, replace=False) for _ in range(max_hyp)]).astype(np.int32) for _ in range(n_sets)]

            def parent():
                for s in range(n_sets):
                    native.fundamental_ransac(parts[s][0], parts[s][1], samples[s], PARENT_THRESHOLD)

            run["fundamental_ransac"] = time_call(parent, lambda: None, args.regions)
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
