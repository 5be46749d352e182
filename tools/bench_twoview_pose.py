#!/usr/bin/env python3
"""Timing of the relative pose of verified pairs (sfm_twoview_pose -> pose_vote_kernel, pose_cand_kernel, pose_score_kernel,
pose_judge_kernel) on

    1x2000   one pair of views, 2 000 matches
    9x8000   a new view of 8 000 matches against nine resident views, in one call

for both kinds of model (F: general motion; H: points on a plane), next to the existing route on the same sets: per pair
essential_from_fundamental, pose_candidates, four tri_linear calls and cheirality (host round trips between all of them; it
has no homography form, so the H sets are timed against the F route of the same size).  Matches: focal 800, 0.5 px noise on
both keys, a tenth of the right keys displaced by 30 - 120 px and masked out; the models are the planted ones.  Both routes
are the host-array forms: a call uploads its coordinates, runs its kernels, downloads its outputs and synchronises.

A timed region is `inner` back-to-back calls (at least 0.1 s); the figure is the MEDIAN over the regions of region time /
inner, the spread is (max - min) / median over the same regions.  The calls are timed alternately, twice each, and both rounds
are kept: the difference between the rounds of one call is the run-to-run spread a difference between two calls has to exceed.

    python tools/bench_twoview_pose.py [--cases 1x2000,9x8000] [--regions 7] [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2 and one
case, and read the pose_* rows.
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

MIN_ANGLE_DEG, MIN_PARALLAX, REGION_S = 2.0, 8, 0.1
K = np.array([[800.0, 0, 320], [0, 800.0, 240], [0, 0, 1]])
PLANE_D = 6.5               # the plane z = 6.5 + 0.1 x + 0.05 y, i.e. (-0.1, -0.05, 1) . X = 6.5


def matches(n, planar, seed, frac=0.1, noise=0.5):
    """(left, right, mask, F, H) of one pair: rotation 0.15 rad about y, translation (-1, 0.1, 0.2) / norm."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, (2, n))
    x = np.vstack((x, 6.5 + 0.1 * x[0] + 0.05 * x[1] if planar else rng.uniform(4, 9, n)))
    a = 0.15
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([-1.0, 0.1, 0.2])
    left = K @ x
    left = left[:2] / left[2]
    right = K @ (rot @ x + t[:, None])
    right = right[:2] / right[2]
    left = left + rng.normal(0, noise, left.shape)
    right = right + rng.normal(0, noise, right.shape)
    bad = rng.random(n) < frac
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(30, 120, n)
    right = right + bad * np.vstack((np.cos(ang), np.sin(ang))) * mag
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ rot @ Ki
    nrm = np.array([-0.1, -0.05, 1.0])
    H = K @ (rot + np.outer(t, nrm) / PLANE_D) @ Ki
    return left, right, ~bad, F / np.linalg.norm(F), H / np.linalg.norm(H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x2000,9x8000")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_twoview_pose.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    cos2 = float(np.cos(np.radians(MIN_ANGLE_DEG)) ** 2)
    ref_proj = K @ np.hstack((np.eye(3), np.zeros((3, 1))))
    out = {"min_angle_deg": MIN_ANGLE_DEG, "min_parallax": MIN_PARALLAX, "regions": args.regions, "region_s": REGION_S, "cases": {}}
    for case in args.cases.split(","):
        n_sets, n = (int(v) for v in case.split("x"))
        set_ptr = np.arange(n_sets + 1, dtype=np.int32) * n
        entry = {"n_sets": n_sets, "matches_per_set": n, "tests_per_call": int(4 * n_sets * n)}
        calls = {}
        chain_sets = None
        for kind, planar in (("fundamental", False), ("homography", True)):
            parts = [matches(n, planar, 100 + s) for s in range(n_sets)]
            left = np.ascontiguousarray(np.hstack([p[0] for p in parts]))
            right = np.ascontiguousarray(np.hstack([p[1] for p in parts]))
            mask = np.concatenate([p[2] for p in parts])
            models = [p[3] if kind == "fundamental" else p[4] for p in parts]

            def pose(left=left, right=right, mask=mask, models=models, kind=kind):
                return native.twoview_pose(set_ptr, left, right, models, [kind] * n_sets, K, K, cos2, MIN_PARALLAX, mask)

            calls["twoview_pose_" + kind] = pose
            res = pose()
            entry["summary_" + kind] = dict(zip(native.POSE_SUMMARY, res["summary"].tolist()))
            entry["status_" + kind] = res["status"].tolist()
            if kind == "fundamental":
                chain_sets = [(p[0][:, p[2]], p[1][:, p[2]], p[3]) for p in parts]

        def chain():
            best = []
            for l, r, F in chain_sets:                         # one pair at a time, the inliers only
                esse = native.essential_from_fundamental(F / F[2, 2], K, K)
                r1, r2, c1, c2 = native.pose_candidates(esse)
                projs = [K @ np.hstack((rr.T, -rr.T @ cc)) for rr, cc in ((r1, c1), (r1, c2), (r2, c1), (r2, c2))]
                uv = np.stack((l, r))
                pts = [native.tri_linear(np.stack((ref_proj, p)), uv) for p in projs]
                best.append(native.cheirality(ref_proj, np.array(projs), np.array(pts))[2])
            return best

        calls["existing_chain_fundamental"] = chain
        chain()
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
