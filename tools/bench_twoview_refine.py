#!/usr/bin/env python3
"""Timing of the refinement of a relative pose (sfm_twoview_refine -> refine_iterate_kernel, refine_judge_kernel) on

    1x2000   one pair of views, 2 000 matches
    9x8000   a new view of 8 000 matches against nine resident views, in one call

at six iterations, next to sfm_twoview_pose on the same sets for scale.  The matches are those of tools/bench_twoview_pose.py
(focal 800, 0.5 px noise on both keys, a tenth of the right keys displaced by 30 - 120 px and masked out); the start pose is
the planted one turned by a degree and a half.  Both calls are the host-array forms: a call uploads its coordinates, runs its
kernels, downloads its outputs and synchronises; `refine_pose_only` asks for R and t alone, so that less comes down.

A timed region is `inner` back-to-back calls (at least 0.1 s); the figure is the MEDIAN over the regions of region time /
inner, the spread is (max - min) / median over the same regions.  The calls are timed alternately, twice each, and both rounds
are kept: the difference between the rounds of one call is the run-to-run spread a difference between two calls has to exceed.

    python tools/bench_twoview_refine.py [--cases 1x2000,9x8000] [--regions 7] [--iters 6] [--lib FILE] [--out FILE]

Prints one JSON line.  --lib loads another build of the library (one made with -DSFM_REFINE_THREADS=..., for a comparison of
workgroup sizes).  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2 and one case,
and read the refine_* rows.
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
from bench_twoview_pose import K, MIN_ANGLE_DEG, MIN_PARALLAX, REGION_S, matches  # noqa: E402  (the same sets)

MAX_PX = 2.0


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    k = w / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.identity(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x2000,9x8000")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_twoview_refine.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    if args.lib:
        native.LIB_PATH = os.path.abspath(args.lib)
    native.init(0)
    cos2 = float(np.cos(np.radians(MIN_ANGLE_DEG)) ** 2)
    a = 0.15
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([-1.0, 0.1, 0.2]) / np.linalg.norm([-1.0, 0.1, 0.2])
    turn = rodrigues((0.01, -0.02, 0.015))
    out = {"iters": args.iters, "max_px": MAX_PX, "regions": args.regions, "region_s": REGION_S, "lib": args.lib, "cases": {}}
    for case in args.cases.split(","):
        n_sets, n = (int(v) for v in case.split("x"))
        set_ptr = np.arange(n_sets + 1, dtype=np.int32) * n
        parts = [matches(n, False, 100 + s) for s in range(n_sets)]
        left = np.ascontiguousarray(np.hstack([p[0] for p in parts]))
        right = np.ascontiguousarray(np.hstack([p[1] for p in parts]))
        mask = np.concatenate([p[2] for p in parts])
        models = [p[3] for p in parts]
        R_in, t_in = np.stack([turn @ rot] * n_sets), np.stack([turn.T @ t] * n_sets)

        def refine(outputs=native.REFINE_OUTPUTS):
            return native.twoview_refine(set_ptr, left, right, R_in, t_in, K, K, 0.0, args.iters, MAX_PX ** 2, cos2, mask, outputs=outputs)

        def pose():
            return native.twoview_pose(set_ptr, left, right, models, ["fundamental"] * n_sets, K, K, cos2, MIN_PARALLAX, mask)

        calls = {"twoview_refine": refine, "refine_pose_only": lambda: refine(()), "twoview_pose": pose}
        res = refine()
        used = res["n_used"].astype(np.float64)
        entry = {"n_sets": n_sets, "matches_per_set": n, "summary": dict(zip(native.REFINE_SUMMARY, res["summary"].tolist())),
                 "status": res["status"].tolist(), "rms_before": np.sqrt(res["cost"][0] / used).tolist(),
                 "rms_after": np.sqrt(res["cost"][1] / used).tolist(),
                 "baseline_error_deg": [float(np.degrees(np.arccos(min(abs(tt @ t), 1.0)))) for tt in res["t"]],
                 "baseline_error_start_deg": float(np.degrees(np.arccos(min(abs(t_in[0] @ t), 1.0))))}
        pose()
        runs = {name: [] for name in calls}
        for _round in range(2):                                # alternately, so that a drift of the machine shows in all
            for name, call in calls.items():
                runs[name].append(time_call(call, lambda: None, args.regions, REGION_S))
        entry["runs"] = runs
        out["cases"][case] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
