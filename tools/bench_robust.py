#!/usr/bin/env python3
"""Cost of the robust losses (sfm_ba_set_loss) per bundle-adjustment iteration: `BaProblem.iterate` with no loss, Huber at
5 px and Cauchy at 10 px, eager and with SFM_OPT_GRAPH, at

    C3       50 cameras x 20 000 points, 60 % visibility            (bench.py's flagship scene)
    C4share  200 cameras x 12 500 points, 15 % visibility           (one GPU's share of C4 on eight)
    C5like   10 views x 5 000 points, consecutive-view tracks       (the shape an incremental run leaves)

with 3 % of the observations displaced by 30 to 120 px, so that both zones of the Huber loss are taken.  A timed region is
one `iterate(lambda, K)` call followed by a device synchronise, K chosen so that the region lasts about `--window` seconds
(default 0.4); the state is uploaded again before every region (outside the clock), so every region does the same work;
one warm-up region (which also captures the graphs) is discarded.  The figure is the MEDIAN over the regions of
region time / K, the spread (max - min) / median; `ratio` is a loss's median over the plain median of the same setting.

Extra flops per observation and evaluation of the loss, counted here from the device function (FMA = 2, a hardware
reciprocal / square-root estimate = 1; a float64 division is taken as 17 and a float64 square root as 13, the compiler's
usual Newton expansions, log1p as 60 -- estimates, not counter readings):
    common   |r|^2 3, s 1, scaling r / Jp / Jx 22                                   = 26
    Huber    + two square roots 26, two divisions 34, rho 3      (s > 1 only)       = 89
    Cauchy   + 1 + s 1, square root 13, two divisions 34, log1p 60, rho 1           = 135
The loss is evaluated twice per observation and iteration (back substitution and linearisation, fused or not) when the
track fits its lane group and three times when it does not (the linearisation's third pass recomputes the terms).

    python tools/bench_robust.py [--shapes C3,C4share,C5like] [--regions 7] [--window 0.4] [--out FILE]

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

FLOPS_COMMON, FLOPS_HUBER, FLOPS_CAUCHY = 26, 89, 135
LAMBDA = 5.0


def make_shape(sfm, name):
    sc = sfm.scenes
    if name == "C3":
        return sc.make_scene(50, 20000, 0.6, seed=0)
    if name == "C4share":
        return sc.make_scene(200, 12500, 0.15, seed=0)
    if name == "C5like":
        return sc.make_scene(10, 5000, seed=0, structure=sc.Structure(mean_track=4.0, heavy=0.05))
    raise SystemExit("unknown shape %s" % name)


def displaced_pixels(scene):
    rng = np.random.default_rng(5)
    m = scene.cam_idx.shape[0]
    hit = rng.choice(m, size=int(0.03 * m), replace=False)
    radius, angle = rng.uniform(30.0, 120.0, hit.shape[0]), rng.uniform(0.0, 2.0 * np.pi, hit.shape[0])
    uv = scene.uv_pix.copy()
    uv[:, hit] += radius * np.vstack((np.cos(angle), np.sin(angle)))
    return uv


def time_iterations(native, prob, scene, regions, window):
    def region(k):
        prob.set_state(scene.cams_init, scene.pts_init)
        native.synchronize()
        t0 = time.perf_counter()
        prob.iterate(LAMBDA, k)
        native.synchronize()
        return time.perf_counter() - t0

    region(4)                                         # loads the code objects
    k = int(min(4000, max(8, window / (region(8) / 8))))
    region(k)                                         # warm-up (captures the graphs when they are on)
    per_iter = np.array([region(k) / k for _ in range(regions)])
    med = float(np.median(per_iter))
    return {"ms_per_iteration": med * 1e3, "spread": float((per_iter.max() - per_iter.min()) / med), "iterations_per_region": k,
            "region_s": med * k, "graph_replays": prob.info(native.INFO_GRAPH_REPLAYS)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C4share,C5like")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_robust.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"flops_common": FLOPS_COMMON, "flops_huber": FLOPS_HUBER, "flops_cauchy": FLOPS_CAUCHY, "lambda": LAMBDA,
           "regions": args.regions, "window_s": args.window, "shapes": {}}
    for name in args.shapes.split(","):
        sc = make_shape(sfm, name)
        uvn = sfm.geometry.normalise_pixels(displaced_pixels(sc), sc.intrinsic)
        scale = float(np.sqrt(abs(sc.intrinsic[0, 0] * sc.intrinsic[1, 1])))
        lens = np.diff(sc.pt_ptr).astype(np.int64)
        group = 4
        while group < 64 and group < sc.n_obs / max(sc.n_pts, 1):
            group <<= 1
        evals = int(np.sum(np.where(lens <= group, 2, 3) * lens))          # loss evaluations per iteration
        entry = {"n_cams": sc.n_cams, "n_pts": sc.n_pts, "n_obs": sc.n_obs, "lane_group": group,
                 "loss_evaluations_per_iteration": evals,
                 "extra_flops_per_observation": {"huber": FLOPS_HUBER * evals / sc.n_obs, "cauchy": FLOPS_CAUCHY * evals / sc.n_obs},
                 "runs": []}
        for graph in (0, 1):
            plain_ms = None
            for loss, px in (("none", None), ("huber", 5.0), ("cauchy", 10.0)):
                with native.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
                    prob.set_option(native.OPT_GRAPH, graph)
                    if px is not None:
                        prob.set_loss(loss, px / scale)
                    r = time_iterations(native, prob, sc, args.regions, args.window)
                    s = prob.loss_terms()[0]
                if loss == "none":
                    plain_ms = r["ms_per_iteration"]
                r.update({"loss": loss, "delta_px": px, "graph": graph, "ratio": r["ms_per_iteration"] / plain_ms,
                          "share_beyond_delta": float(np.mean(s > 1.0)) if px is not None else None})
                entry["runs"].append(r)
        out["shapes"][name] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
