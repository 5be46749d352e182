#!/usr/bin/env python3
"""Timing of the robust essential matrix (sfm_essential_ransac -> essential_hyp_kernel, essential_score_kernel,
essential_pick_kernel, essential_judge_kernel) on

    1x2000   one pair of views, 2 000 matches
    9x8000   a new view of 8 000 matches against nine resident views, in one call

at 128 and 1 024 hypotheses, next to sfm_twoview_ransac with iters = 0 (eight-point hypotheses, no refit) on the same sets.
The matches are those of tools/bench_twoview_pose.py (focal 800, 0.5 px noise on both keys, a tenth of the right keys displaced
by 30 - 120 px).  Both calls are the host-array forms: a call uploads its coordinates, runs its kernels, downloads its outputs
and synchronises.

A timed region is `inner` back-to-back calls (at least 0.1 s); the figure is the MEDIAN over the regions of region time /
inner, the spread is (max - min) / median over the same regions.  The calls are timed alternately, twice each, and both rounds
are kept: the difference between the rounds of one call is the run-to-run spread a difference between two calls has to exceed.

    python tools/bench_essential.py [--cases 1x2000,9x8000] [--hyps 128,1024] [--regions 7] [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2, one case and
one hypothesis count, and read the essential_* rows.
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
from bench_twoview_pose import K, REGION_S, matches  # noqa: E402  (the same sets)

MAX_PX = 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x2000,9x8000")
    ap.add_argument("--hyps", default="128,1024")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_essential.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"max_px": MAX_PX, "regions": args.regions, "region_s": REGION_S, "cases": {}}
    for case in args.cases.split(","):
        n_sets, n = (int(v) for v in case.split("x"))
        set_ptr = np.arange(n_sets + 1, dtype=np.int32) * n
        parts = [matches(n, False, 100 + s) for s in range(n_sets)]
        left = np.ascontiguousarray(np.hstack([p[0] for p in parts]))
        right = np.ascontiguousarray(np.hstack([p[1] for p in parts]))
        clean = np.concatenate([p[2] for p in parts])
        for max_hyp in (int(v) for v in args.hyps.split(",")):

            def essential():
                return native.essential_ransac(set_ptr, left, right, K, K, MAX_PX ** 2, max_hyp)

            def eight_point():
                return native.twoview_ransac(set_ptr, left, right, MAX_PX ** 2, max_hyp, 0)

            calls = {"essential_ransac": essential, "twoview_ransac_iters0": eight_point}
            res, f8 = essential(), eight_point()
            entry = {"n_sets": n_sets, "matches_per_set": n, "max_hyp": max_hyp,
                     "summary": dict(zip(native.ESSENTIAL_SUMMARY, res["summary"].tolist())),
                     "n_valid": res["n_valid"].tolist(), "clean_matches": int(clean.sum()),
                     "clean_kept": int((res["inlier"].astype(bool) & clean).sum()),
                     "clean_kept_eight_point": int((f8[1].astype(bool) & clean).sum())}
            runs = {name: [] for name in calls}
            for _round in range(2):                            # alternately, so that a drift of the machine shows in all
                for name, call in calls.items():
                    runs[name].append(time_call(call, lambda: None, args.regions, REGION_S))
            entry["runs"] = runs
            out["cases"]["%s@%d" % (case, max_hyp)] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
