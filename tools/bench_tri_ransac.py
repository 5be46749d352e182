#!/usr/bin/env python3
"""Timing of the robust re-triangulation of the resident scene (sfm_ba_retriangulate -> tri_ransac_score_kernel,
tri_ransac_refit_kernel): every group width and the automatic choice, max_hyp 32 and 128, next to the structure-only
refinement (sfm_ba_refine_points, 3 iterations) and the screening (sfm_ba_screen) of the same scene, at

    C3       50 cameras x 20 000 points, 60 % visibility            (bench.py's flagship scene)
    C4share  200 cameras x 12 500 points, 15 % visibility           (one GPU's share of C4 on eight)
    C5like   10 views x 5 000 points, consecutive-view tracks       (the shape an incremental run leaves)

A timed region is `inner` back-to-back calls, each ending in the call's own stream synchronise (nothing comes down: no
output is requested); the figure is the MEDIAN over the regions of region time / inner, the spread is
(max - min) / median over the same regions.  The scene is warmed with one region per configuration first.  Thresholds:
4 px through cam_scale = sqrt(|fx fy|), rays at least 1.5 degrees apart, lambda 0.5, 3 refit iterations.  The scene is
adjusted first (--ba-iters iterations at lambda 5), so that the cameras are the ones a re-triangulation would meet, and
every configuration starts from the adjusted points; `summary_max_hyp_128` says what the call then decides.

    python tools/bench_tri_ransac.py [--shapes C3,C4share,C5like] [--max-hyp 32,128] [--groups 0,1,4,8,16,32,64]
                                     [--regions 7] [--out FILE]

Prints one JSON line.  The scoring kernel's time alone: run it once more under `rocprofv3 --kernel-trace --stats` with
--regions 2 and read tri_ransac_score_kernel's rows.
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tri_tracks import make_shape  # noqa: E402  (the same three scenes)

MAX_PX, MIN_ANGLE_DEG, LAM, ITERS = 4.0, 1.5, 0.5, 3


def time_call(call, reset, regions, target_s=0.02):
    reset()
    call()                                            # loads the code object of this instantiation
    t0 = time.perf_counter()
    call()
    one = max(time.perf_counter() - t0, 1e-6)
    inner = int(min(2000, max(5, target_s / one)))
    for _ in range(inner):                            # warm-up region
        call()
    per_call = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        per_call.append((time.perf_counter() - t0) / inner)
    per_call = np.array(per_call)
    med = float(np.median(per_call))
    return {"ms_per_call": med * 1e3, "spread": float((per_call.max() - per_call.min()) / med), "calls_per_region": inner}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C4share,C5like")
    ap.add_argument("--max-hyp", default="32,128")
    ap.add_argument("--groups", default="0,1,4,8,16,32,64")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--ba-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tri_ransac.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    max_err2, cos_min = MAX_PX ** 2, math.cos(math.radians(MIN_ANGLE_DEG))
    out = {"max_px": MAX_PX, "min_angle_deg": MIN_ANGLE_DEG, "lambda": LAM, "iters": ITERS, "regions": args.regions, "ba_iters": args.ba_iters,
           "shapes": {}}
    for name in args.shapes.split(","):
        sc = make_shape(sfm, name)
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        scale = np.full(sc.n_cams, math.sqrt(abs(float(sc.intrinsic[0, 0]) * float(sc.intrinsic[1, 1]))))
        lens = np.diff(sc.pt_ptr)
        entry = {"n_cams": sc.n_cams, "n_pts": sc.n_pts, "n_obs": sc.n_obs, "longest_track": int(lens.max()),
                 "mean_track": float(lens.mean()), "group_auto": native.tracks_auto_group(sc.n_pts, sc.n_obs, int(lens.max())),
                 "retriangulate": []}
        with native.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(5.0, args.ba_iters)
            pts_adjusted = prob.get_state()[1]

            def reset():
                prob.set_points(0, pts_adjusted)

            summary = prob.retriangulate(max_err2, cos_min, 128, LAM, ITERS, scale).summary
            entry["summary_max_hyp_128"] = dict(zip(native.RANSAC_SUMMARY, summary.tolist()))
            for max_hyp in [int(h) for h in args.max_hyp.split(",")]:
                for group in [int(g) for g in args.groups.split(",")]:
                    run = time_call(lambda: prob.retriangulate(max_err2, cos_min, max_hyp, LAM, ITERS, scale, group, want_outputs=False),
                                    reset, args.regions)
                    run.update({"max_hyp": max_hyp, "group": group})
                    entry["retriangulate"].append(run)
            entry["refine_points_3"] = time_call(lambda: prob.refine_points(LAM, 3, native.TRACKS_NONLINEAR, 0, want_outputs=False),
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
