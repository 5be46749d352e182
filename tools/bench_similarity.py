#!/usr/bin/env python3
"""Timing of the robust similarity (sfm_similarity_ransac -> similarity_hyp_kernel, similarity_score_kernel,
similarity_pick_kernel, similarity_refit_kernel, similarity_judge_kernel) on

    1x2000   one set of 2 000 correspondences
    9x8000   nine sets of 8 000, in one call

each at max_hyp 128 and 1 024 with two refit rounds, and next to each sfm_homography_ransac on sets of the same size in the
same run (the same frame with a lighter model: 12 doubles and one half against 18 and two).  Correspondences: points in a
8 x 6 x 4 box, s in 0.3 .. 3, noise 0.01, a tenth displaced by 1 .. 4.5 units; threshold 0.05.  Both are the host-array
forms: a call uploads its coordinates, runs its kernels, downloads its outputs and synchronises.

Then `BaProblem.align` on the 20 000 points of configuration C3 (all of them as correspondences, a fifth of the targets
wrong), next to the host route it replaces: `get_state`, a NumPy Umeyama fit over the TRUE inliers (the host route is
given the answer a robust host fit would first have to find), `apply_similarity`, `set_state`.

A timed region is `inner` back-to-back calls (at least 0.1 s); the figure is the MEDIAN over the regions of region time /
inner, the spread is (max - min) / median over the same regions.  The two calls of a pair are timed alternately, twice
each, and both rounds are kept.  `tests_per_call` = hypotheses x correspondences bounds the tests of the scoring kernel;
FLOP_PER_TEST counts a FMA as two.

    python tools/bench_similarity.py [--cases 1x2000,9x8000] [--max-hyp 128,1024] [--regions 7] [--no-align] [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2, one
case and --no-align, and read the similarity_* and homography_* rows.
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

from bench_homography import plane_matches  # noqa: E402
from bench_tri_ransac import time_call  # noqa: E402  (the same regions)

MAX_ERR, ITERS, REGION_S = 0.05, 2, 0.1
FLOP_PER_TEST = 29      # three rows of three FMAs (18), three differences (3), lhs (5), the two comparisons (2), the count (1)


def rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def two_frames(a, frac, seed, noise=0.01):
    """dst (3, n) and the wrong ones (n,) for the points a (3, n): a random similarity, noise, a share displaced."""
    rng = np.random.default_rng(seed)
    n = a.shape[1]
    b = rng.uniform(0.3, 3.0) * (rotation(rng) @ a) + rng.uniform(-5, 5, (3, 1)) + noise * rng.standard_normal((3, n))
    bad = rng.random(n) < frac
    d = rng.standard_normal((3, n))
    return b + bad * d / np.linalg.norm(d, axis=0) * rng.uniform(1.0, 4.5, n), bad


def umeyama(a, b):
    mu_a, mu_b = a.mean(axis=1, keepdims=True), b.mean(axis=1, keepdims=True)
    da, db = a - mu_a, b - mu_b
    U, D, Vt = np.linalg.svd(db @ da.T / a.shape[1])
    S = np.array([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    A = (U * S) @ Vt
    s = float((D * S).sum() / ((da * da).sum() / a.shape[1]))
    return s, A, (mu_b - s * A @ mu_a).ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x2000,9x8000")
    ap.add_argument("--max-hyp", default="128,1024")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--no-align", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_similarity.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"max_err": MAX_ERR, "iters": ITERS, "regions": args.regions, "region_s": REGION_S, "flop_per_test": FLOP_PER_TEST, "cases": {}}
    for case in [c for c in args.cases.split(",") if c]:
        n_sets, n = (int(v) for v in case.split("x"))
        set_ptr = np.arange(n_sets + 1, dtype=np.int32) * n
        rng = np.random.default_rng(7)
        src = np.ascontiguousarray((rng.random((3, n_sets * n)) - 0.5) * np.array([[8.0], [6.0], [4.0]]))
        dst = np.ascontiguousarray(np.hstack([two_frames(src[:, k * n:(k + 1) * n], 0.1, 100 + k)[0] for k in range(n_sets)]))
        parts = [plane_matches(n, 0.1, 100 + k) for k in range(n_sets)]
        left = np.ascontiguousarray(np.hstack([p[0] for p in parts]))
        right = np.ascontiguousarray(np.hstack([p[1] for p in parts]))
        entry = {"n_sets": n_sets, "per_set": n, "runs": []}
        for max_hyp in [int(h) for h in args.max_hyp.split(",")]:
            def similarity():
                return native.similarity_ransac(set_ptr, src, dst, MAX_ERR ** 2, max_hyp, ITERS)

            def homography():
                return native.homography_ransac(set_ptr, left, right, 4.0, max_hyp, ITERS)

            run = {"max_hyp": max_hyp, "tests_per_call": int(n_sets * max_hyp * n),
                   "similarity_summary": dict(zip(native.SIMILARITY_SUMMARY, similarity()[5].tolist())),
                   "homography_summary": dict(zip(native.HOMOGRAPHY_SUMMARY, homography()[5].tolist())),
                   "similarity_ransac": [], "homography_ransac": []}
            for _round in range(2):                            # alternately, so that a drift of the machine shows in both
                run["similarity_ransac"].append(time_call(similarity, lambda: None, args.regions, REGION_S))
                run["homography_ransac"].append(time_call(homography, lambda: None, args.regions, REGION_S))
            entry["runs"].append(run)
        out["cases"][case] = entry

    if not args.no_align:
        sc = sfm.scenes.make_config("C3")
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        cams0 = sc.cams_init.copy()
        cams0[:, 3:7] /= np.linalg.norm(cams0[:, 3:7], axis=1, keepdims=True)
        idx = np.arange(sc.n_pts, dtype=np.int32)
        targets, bad = two_frames(sc.pts_init, 0.2, 5)
        targets = np.ascontiguousarray(targets)
        with native.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            def reset():
                prob.set_state(cams0, sc.pts_init)

            def align():
                reset()
                return prob.align(idx, targets, MAX_ERR ** 2, 128, ITERS)

            def host_route():
                reset()
                cams, pts = prob.get_state()
                s, A, t = umeyama(pts[:, ~bad], targets[:, ~bad])
                prob.set_state(*sfm.geometry.apply_similarity((s, A, t), cams, pts))

            def only_reset():
                reset()

            sim, inlier, n_in, _best, status = align()
            entry = {"n_pts": sc.n_pts, "n_cams": sc.n_cams, "wrong": int(bad.sum()), "n_inliers": n_in, "status": status,
                     "wrong_kept": int((inlier.astype(bool) & bad).sum()), "align": [], "host_route": [], "set_state_alone": []}
            for _round in range(2):
                entry["align"].append(time_call(align, lambda: None, args.regions, REGION_S))
                entry["host_route"].append(time_call(host_route, lambda: None, args.regions, REGION_S))
                entry["set_state_alone"].append(time_call(only_reset, lambda: None, args.regions, REGION_S))
            out["align_C3"] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
