#!/usr/bin/env python3
"""Timing of the structure-only refinement over ragged tracks (sfm_ba_refine_points -> tri_tracks_nonlinear_kernel) on
resident scenes: every group width and the automatic choice, 3 and 100 iterations, at

    C3       50 cameras x 20 000 points, 60 % visibility            (bench.py's flagship scene)
    C4share  200 cameras x 12 500 points, 15 % visibility           (one GPU's share of C4 on eight)
    C5like   10 views x 5 000 points, consecutive-view tracks       (the shape an incremental run leaves)

A timed region is `inner` back-to-back calls, each ending in the call's own stream synchronise (nothing comes down:
cost and status are not requested); the figure is the MEDIAN over the regions of region time / inner, the spread is
(max - min) / median over the same regions.  The scene is warmed with one region per configuration first.

Flop count (FMA = 2, v_rcp_f64 = 1), per iteration: 97 per observation (projection 21, reciprocal with its refinement 7,
iz^2 1, the 2 x 3 Jacobian 24, residual 4, the nine sums 36, cost 4) + 54 per point (adjugate 18, determinant 5,
reciprocal 7, delta 18, damping 3, update 3; counted once per point although every lane of a group computes it).
Share of peak = that count / time / 78.6 TFLOP/s (FP64 vector peak of the MI355X).

    python tools/bench_tri_tracks.py [--shapes C3,C4share,C5like] [--iters 3,100] [--groups 0,1,4,8,16,32,64]
                                     [--regions 7] [--out FILE]

Prints one JSON line.  Kernel time against wall time: run it once more under `rocprofv3 --kernel-trace --stats` with
--regions 2 and read tri_tracks_nonlinear_kernel's row.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FP64_VECTOR_PEAK = 78.6e12
FLOPS_PER_OBS, FLOPS_PER_POINT = 97, 54


def make_shape(sfm, name):
    sc = sfm.scenes
    if name == "C3":
        return sc.make_scene(50, 20000, 0.6, seed=0)
    if name == "C4share":
        return sc.make_scene(200, 12500, 0.15, seed=0)
    if name == "C5like":
        return sc.make_scene(10, 5000, seed=0, structure=sc.Structure(mean_track=4.0, heavy=0.05))
    raise SystemExit("unknown shape %s" % name)


def time_config(native, prob, pts_init, lam, iters, group, regions, target_s=0.02):
    def call():
        prob.refine_points(lam, iters, native.TRACKS_NONLINEAR, group, want_outputs=False)

    prob.set_points(0, pts_init)
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
    return med, float((per_call.max() - per_call.min()) / med), inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C4share,C5like")
    ap.add_argument("--iters", default="3,100")
    ap.add_argument("--groups", default="0,1,4,8,16,32,64")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tri_tracks.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"flops_per_observation_iteration": FLOPS_PER_OBS, "flops_per_point_iteration": FLOPS_PER_POINT,
           "fp64_vector_peak": FP64_VECTOR_PEAK, "regions": args.regions, "shapes": {}}
    for name in args.shapes.split(","):
        sc = make_shape(sfm, name)
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        lens = np.diff(sc.pt_ptr)
        entry = {"n_cams": sc.n_cams, "n_pts": sc.n_pts, "n_obs": sc.n_obs, "longest_track": int(lens.max()),
                 "mean_track": float(lens.mean()), "runs": []}
        with native.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_state(sc.cams_init, sc.pts_init)
            for iters in [int(i) for i in args.iters.split(",")]:
                flops = iters * (FLOPS_PER_OBS * sc.n_obs + FLOPS_PER_POINT * sc.n_pts)
                for group in [int(g) for g in args.groups.split(",")]:
                    med, spread, inner = time_config(native, prob, sc.pts_init, args.lam, iters, group, args.regions)
                    entry["runs"].append({"iters": iters, "group": group,
                                          "group_used": group or native.tracks_auto_group(sc.n_pts, sc.n_obs, int(lens.max())), "ms_per_call": med * 1e3, "spread": spread,
                                          "calls_per_region": inner, "obs_iterations_per_s": sc.n_obs * iters / med,
                                          "frac_fp64_vector_peak": flops / med / FP64_VECTOR_PEAK})
        out["shapes"][name] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
