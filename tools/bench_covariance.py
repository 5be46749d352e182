#!/usr/bin/env python3
"""Timing of the covariance of a resident scene (sfm_ba_covariance) at

    C3       50 cameras x 20 000 points, 60 % visibility            (bench.py's flagship scene)
    C4share  200 cameras x 12 500 points, 15 % visibility           (one GPU's share of C4 on eight)
    C5like   10 views x 5 000 points, consecutive-view tracks       (the shape an incremental run leaves)

with the first two cameras held and lambda = 0, after a few iterations of the adjustment.  Two kinds of figures:

  * wall time per call, as a caller sees it (allocation from the pool, the mask upload, the status read-back in the middle
    of the inverse, the download of the blocks, the final synchronise): the MEDIAN over the regions of region time / inner,
    the spread (max - min) / median over the same regions, one warm-up region; for the whole call, for the cameras alone
    (want_points=False) and with every camera held (the per-point terms and D^-1 alone);
  * device time of the call's four phases -- per-point terms, S, the inverse, the point kernels -- from the hipEvents the
    call records under SFM_OPT_TIMING (sfm_ba_covariance_times), median over the same number of calls made separately
    (the events cost stream bubbles, so the wall figures are taken without them).

Next to them, the yardstick: one full bundle-adjustment iteration of the same scene, timed the same way
(`iters` iterations per call, the state reset before every region).

    python tools/bench_covariance.py [--shapes C3,C4share,C5like] [--regions 7] [--group 0] [--out FILE]

Prints one JSON line.
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


def make_shape(sfm, name):
    sc = sfm.scenes
    if name == "C3":
        return sc.make_scene(50, 20000, 0.6, seed=0)
    if name == "C4share":
        return sc.make_scene(200, 12500, 0.15, seed=0)
    if name == "C5like":
        return sc.make_scene(10, 5000, seed=0, structure=sc.Structure(mean_track=4.0, heavy=0.05))
    raise SystemExit("unknown shape %s" % name)


def time_regions(call, reset, regions, target_s=0.05):
    reset()
    call()                                            # loads the code objects, builds the camera-major list
    reset()
    t0 = time.perf_counter()
    call()
    one = max(time.perf_counter() - t0, 1e-6)
    inner = int(min(500, max(3, target_s / one)))
    per_call = []
    for region in range(regions + 1):                 # region 0 warms up
        reset()
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        if region:
            per_call.append((time.perf_counter() - t0) / inner)
    per_call = np.array(per_call)
    med = float(np.median(per_call))
    return med, float((per_call.max() - per_call.min()) / med), inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C4share,C5like")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--group", type=int, default=0)
    ap.add_argument("--iters", type=int, default=5, help="iterations per call of the yardstick")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_covariance.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"regions": args.regions, "group": args.group, "shapes": {}}
    for name in args.shapes.split(","):
        sc = make_shape(sfm, name)
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        tracks = np.diff(sc.pt_ptr)
        block, blocks, launches, _g = native.covariance_plan(sc.n_cams)
        entry = {"n_cams": sc.n_cams, "n_pts": sc.n_pts, "n_obs": sc.n_obs, "track_mean": float(tracks.mean()), "track_max": int(tracks.max()),
                 "pairs": int(np.sum(tracks * (tracks + 1) // 2)), "inverse_blocks": blocks, "inverse_launches": launches,
                 "sigma_bytes": 8 * (blocks * block) ** 2}
        mask = np.ones(sc.n_cams, dtype=np.uint8)
        mask[0:2] = 0
        with native.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(0.5, 5)
            cams, pts = prob.get_state()

            def iterate():
                prob.iterate(0.5, args.iters)
                native.synchronize()

            med, spread, inner = time_regions(iterate, lambda: prob.set_state(cams, pts), args.regions)
            entry["ba_iteration_ms"] = med * 1e3 / args.iters
            entry["ba_iteration_spread"] = spread
            prob.set_state(cams, pts)
            first = prob.covariance(0.0, mask=mask, group=args.group)
            if first.pivot_camera is not None:
                raise SystemExit("%s: singular at camera %d" % (name, first.pivot_camera))
            entry["sigma0_px"] = float(np.sqrt(first.sigma0_sq) * np.sqrt(abs(sc.intrinsic[0, 0] * sc.intrinsic[1, 1])))
            entry["pt_sigma_median"] = float(np.median(np.sqrt(first.sigma0_sq * (first.pt_cov[:, 0] + first.pt_cov[:, 3] + first.pt_cov[:, 5]))))
            for key, kwargs in (("all", dict(mask=mask)), ("cameras_only", dict(mask=mask, want_points=False)),
                                ("all_held", dict(mask=np.zeros(sc.n_cams, dtype=np.uint8)))):
                med, spread, inner = time_regions(lambda: prob.covariance(0.0, group=args.group, **kwargs), lambda: None, args.regions)
                entry["wall_%s_ms" % key] = med * 1e3
                entry["wall_%s_spread" % key] = spread
                entry["wall_%s_calls_per_region" % key] = inner
            prob.set_option(native.OPT_TIMING, 1)
            phases = []
            for _ in range(args.regions):
                prob.covariance(0.0, mask=mask, group=args.group)
                phases.append(prob.covariance_times())
            prob.set_option(native.OPT_TIMING, 0)
            phases = np.array(phases)
            for k, key in enumerate(("terms", "build_s", "inverse", "points")):
                entry["device_%s_ms" % key] = float(np.median(phases[:, k]))
                entry["device_%s_spread" % key] = float((phases[:, k].max() - phases[:, k].min()) / max(np.median(phases[:, k]), 1e-9))
            entry["call_over_ba_iteration"] = entry["wall_all_ms"] / entry["ba_iteration_ms"]
            entry["points_kernel_over_ba_iteration"] = entry["device_points_ms"] / entry["ba_iteration_ms"]
        out["shapes"][name] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
