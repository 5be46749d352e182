#!/usr/bin/env python3
"""Timing of the robust resection of the resident scene (sfm_ba_resect -> resect_hyp_kernel, resect_score_kernel,
resect_pick_kernel, resect_refit_kernel, resect_judge_kernel): max_hyp 32 and 128, next to the motion-only refinement
(sfm_ba_refine_cameras, 3 iterations), the robust re-triangulation (sfm_ba_retriangulate) and the screening (sfm_ba_screen)
of the same scene, at

    C3       50 cameras x 20 000 points, 60 % visibility            (bench.py's flagship scene)
    C4share  200 cameras x 12 500 points, 15 % visibility           (one GPU's share of C4 on eight)
    C5like   10 views x 5 000 points, consecutive-view tracks       (the shape an incremental run leaves)

A timed region is `inner` back-to-back calls, each ending in the call's own stream synchronise (nothing comes down: no
output is requested); the figure is the MEDIAN over the regions of region time / inner, the spread is
(max - min) / median over the same regions.  The scene is warmed with one region per configuration first.  Thresholds:
4 px through cam_scale = sqrt(|fx fy|), lambda 0.5, 3 refit iterations.  The scene is adjusted first (--ba-iters
iterations at lambda 5) and every configuration starts from the adjusted cameras and points; `summary_max_hyp_128` says
what the call then decides, `score_flop_upper` bounds the scoring kernel's arithmetic: 34 floating-point operations per
(pose, observation) -- 18 of the projection, 7 of the refined reciprocal, 4 of the residual, 5 of err2, a FMA counted as
two -- over four poses per hypothesis (about half of them are valid and scored).

    python tools/bench_resect.py [--shapes C3,C4share,C5like] [--max-hyp 32,128] [--regions 7] [--out FILE]

Prints one JSON line.  The scoring kernel's time alone: run it once more under `rocprofv3 --kernel-trace --stats` with
--regions 2 and read resect_score_kernel's rows.
"""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tri_ransac import time_call  # noqa: E402  (the same regions)
from bench_tri_tracks import make_shape  # noqa: E402  (the same three scenes)

MAX_PX, MIN_ANGLE_DEG, LAM, ITERS = 4.0, 1.5, 0.5, 3
FLOP_PER_TEST = 34


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C4share,C5like")
    ap.add_argument("--max-hyp", default="32,128")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--ba-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resect.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    max_err2, cos_min = MAX_PX ** 2, math.cos(math.radians(MIN_ANGLE_DEG))
    out = {"max_px": MAX_PX, "lambda": LAM, "iters": ITERS, "regions": args.regions, "ba_iters": args.ba_iters, "shapes": {}}
    for name in args.shapes.split(","):
        sc = make_shape(sfm, name)
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        scale = np.full(sc.n_cams, math.sqrt(abs(float(sc.intrinsic[0, 0]) * float(sc.intrinsic[1, 1]))))
        per_cam = np.bincount(sc.cam_idx, minlength=sc.n_cams)
        entry = {"n_cams": sc.n_cams, "n_pts": sc.n_pts, "n_obs": sc.n_obs, "most_obs": int(per_cam.max()),
                 "mean_obs": float(per_cam.mean()), "resect": []}
        with native.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(5.0, args.ba_iters)
            cams_adjusted, pts_adjusted = prob.get_state()

            def reset():
                prob.set_state(cams_adjusted, pts_adjusted)

            report = prob.resect(max_err2, 128, LAM, ITERS, cam_scale=scale)
            entry["summary_max_hyp_128"] = dict(zip(native.RESECT_SUMMARY, report.summary.tolist()))
            for max_hyp in [int(h) for h in args.max_hyp.split(",")]:
                run = time_call(lambda: prob.resect(max_err2, max_hyp, LAM, ITERS, cam_scale=scale, want_outputs=False),
                                reset, args.regions)
                run["max_hyp"] = max_hyp
                # an upper bound of the scored poses: four per hypothesis (the valid ones are about half of them)
                run["score_flop_upper"] = int(FLOP_PER_TEST * 4 * sum(min(max_hyp, n * (n - 1) * (n - 2) // 6) * n for n in per_cam.tolist()))
                entry["resect"].append(run)
            entry["refine_cameras_3"] = time_call(lambda: prob.refine_cameras(LAM, 3), reset, args.regions)
            entry["retriangulate_128"] = time_call(lambda: prob.retriangulate(max_err2, cos_min, 128, LAM, ITERS, scale, want_outputs=False),
                                                   reset, args.regions)
            entry["screen"] = time_call(lambda: prob.screen(max_err2, cos_min, 2, scale, want_outputs=False), reset, args.regions)
        out["shapes"][name] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
