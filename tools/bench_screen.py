#!/usr/bin/env python3
"""Timing of the screening and culling of a resident bundle-adjustment scene (sfm_ba_screen / sfm_ba_cull ->
ba_screen_kernel, ba_cull_scan_kernel, ba_cull_scatter_kernel) at

    C3       50 cameras x 20 000 points, 60 % visibility            (bench.py's flagship scene)
    C4share  200 cameras x 12 500 points, 15 % visibility           (one GPU's share of C4 on eight)
    C5like   10 views x 5 000 points, consecutive-view tracks       (the shape an incremental run leaves)

after one bundle-adjustment iteration, against what the library offered for the same result before these entry points:

    host round trip   BaProblem.structure() + get_state(), the NumPy screening of tests/_screen_reference.py,
                      a new BaProblem of the compacted lists + set_state           (each part timed on its own)
    refine_points     BaProblem.refine_points(iters=0, want_outputs=False): one pass over the same data

`screen` is timed with every group width and the automatic one, with the per-observation outputs downloaded and with the
summary alone; `cull` is timed on a new problem per repetition (it changes the scene), the thresholds at the 0.9 quantile
of err2 and 2 degrees.  A timed region is `inner` back-to-back calls, each ending in the call's own stream synchronise;
the figure is the MEDIAN over the regions of region time / inner, the spread (max - min) / median.

Counts per call (kept here, from the shapes): bytes the screen kernel must move = 37 per observation (cam_idx 4, u and v
16, err2 and depth 16, flags 1) + 44 per point (px, py, pz 24, pt_ptr 4, min_cos 8, pt_flags 4, keep 4); flops (FMA = 2,
v_rcp_f64 / v_rsq_f64 = 1) = 53 per observation (projection 18, reciprocal 7, residual 4, err2 5, ray 19) + 6 per ordered
pair of observations of a point.  Shares: bytes / time / 8.0 TB/s and flops / time / 78.6 TFLOP/s;
they are whole-call figures unless the run is repeated under `rocprofv3 --kernel-trace --stats` for the kernel's row.

    python tools/bench_screen.py [--shapes C3,C4share,C5like] [--groups 0,1,4,8,16,32,64] [--regions 7] [--out FILE]

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
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK = 8.0e12
FP64_VECTOR_PEAK = 78.6e12
BYTES_PER_OBS, BYTES_PER_POINT = 37, 44
FLOPS_PER_OBS, FLOPS_PER_PAIR = 53, 6


def make_shape(sfm, name):
    sc = sfm.scenes
    if name == "C3":
        return sc.make_scene(50, 20000, 0.6, seed=0)
    if name == "C4share":
        return sc.make_scene(200, 12500, 0.15, seed=0)
    if name == "C5like":
        return sc.make_scene(10, 5000, seed=0, structure=sc.Structure(mean_track=4.0, heavy=0.05))
    raise SystemExit("unknown shape %s" % name)


def time_call(call, regions, target_s=0.02):
    call()                                            # loads the code object
    t0 = time.perf_counter()
    call()
    one = max(time.perf_counter() - t0, 1e-6)
    inner = int(min(2000, max(3, target_s / one)))
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


def time_once(call, repeats):
    """Median of `repeats` single calls (for calls that cannot be repeated on the same object, or are slow)."""
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts)
    return {"ms_per_call": float(np.median(ts)) * 1e3, "spread": float((ts.max() - ts.min()) / np.median(ts)), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C4share,C5like")
    ap.add_argument("--groups", default="0,1,4,8,16,32,64")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_screen.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    sr = importlib.import_module("_screen_reference")
    native = sfm.native
    native.init(0)
    out = {"bytes_per_observation": BYTES_PER_OBS, "bytes_per_point": BYTES_PER_POINT, "flops_per_observation": FLOPS_PER_OBS,
           "flops_per_ordered_pair": FLOPS_PER_PAIR, "hbm_peak": HBM_PEAK, "fp64_vector_peak": FP64_VECTOR_PEAK,
           "regions": args.regions, "shapes": {}}
    for name in args.shapes.split(","):
        sc = make_shape(sfm, name)
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        lens = np.diff(sc.pt_ptr).astype(np.int64)
        n_bytes = BYTES_PER_OBS * sc.n_obs + BYTES_PER_POINT * sc.n_pts
        n_flops = FLOPS_PER_OBS * sc.n_obs + FLOPS_PER_PAIR * int(np.sum(lens * (lens - 1)))
        entry = {"n_cams": sc.n_cams, "n_pts": sc.n_pts, "n_obs": sc.n_obs, "longest_track": int(lens.max()),
                 "mean_track": float(lens.mean()), "bytes": n_bytes, "flops": n_flops,
                 "group_auto": native.tracks_auto_group(sc.n_pts, sc.n_obs, int(lens.max())), "screen": [], "cull": None}

        def fresh():
            prob = native.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn)
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(5.0, 1)
            return prob

        with fresh() as prob:
            cams, pts = prob.get_state()
            base = prob.screen()
            max_err2 = float(np.quantile(base.err2, 0.9))
            cos_min = float(np.cos(np.radians(2.0)))
            for group in [int(g) for g in args.groups.split(",")]:
                for want in (False, True):
                    r = time_call(lambda: prob.screen(max_err2, cos_min, 2, want_outputs=want, group=group), args.regions)
                    r.update({"group": group, "outputs": want, "frac_hbm_peak": n_bytes / (r["ms_per_call"] * 1e-3) / HBM_PEAK,
                              "frac_fp64_vector_peak": n_flops / (r["ms_per_call"] * 1e-3) / FP64_VECTOR_PEAK})
                    entry["screen"].append(r)
            entry["refine_points_iters0"] = time_call(
                lambda: prob.refine_points(0.5, 0, native.TRACKS_NONLINEAR, 0, want_outputs=False), args.regions)
            entry["ba_iteration"] = time_call(lambda: (prob.iterate(5.0, 1), native.synchronize()), args.regions)
            prob.set_state(cams, pts)
            # the host round trip, part by part
            entry["host_download"] = time_once(lambda: (prob.structure(), prob.get_state()), 5)
            pt_ptr, cam_idx, uv = prob.structure()
            ref_box = {}

            def numpy_screen():
                ref_box["ref"] = sr.screen_reference(pt_ptr, cam_idx, uv, cams, pts, max_err2, cos_min, 2)
                ref_box["lists"] = sr.compact(pt_ptr, cam_idx, uv, ref_box["ref"].obs_flags)
            entry["host_numpy_screen"] = time_once(numpy_screen, 1)
            new_ptr, new_cam, new_uv = ref_box["lists"]

            def rebuild():
                with native.BaProblem(sc.n_cams, new_ptr, new_cam, new_uv) as again:
                    again.set_state(cams, pts)
            entry["host_rebuild"] = time_once(rebuild, 5)
            entry["host_round_trip_ms"] = sum(entry[k]["ms_per_call"] for k in ("host_download", "host_numpy_screen", "host_rebuild"))
            got = prob.screen(max_err2, cos_min, 2)
            entry["flags_equal_reference"] = bool(np.array_equal(got.obs_flags, ref_box["ref"].obs_flags))
            entry["obs_kept"] = int(got.summary[1])

        # cull changes the scene: one new problem per repetition, only the cull call inside the clock
        ts = []
        for want in (False, True):
            ts = []
            for _ in range(6):
                with fresh() as prob:
                    prob.get_state()
                    t0 = time.perf_counter()
                    prob.cull(max_err2, cos_min, 2, want_outputs=want)
                    ts.append(time.perf_counter() - t0)
            ts = np.array(ts[1:])                     # the first loads the code objects
            r = {"ms_per_call": float(np.median(ts)) * 1e3, "spread": float((ts.max() - ts.min()) / np.median(ts)), "repeats": 5,
                 "outputs": want}
            entry["cull_outputs" if want else "cull"] = r
        out["shapes"][name] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
