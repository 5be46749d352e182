#!/usr/bin/env python3
"""Timing of the matrix-free bundle adjustment (sfm_ba_iterate_pcg) against the dense-system iteration (sfm_ba_iterate) at

    C3          50 cameras x 20 000 points, 60 % visibility           (bench.py's flagship scene)
    C4share     200 cameras x 12 500 points, 15 % visibility          (one GPU's share of C4 on eight)
    C4          200 cameras x 100 000 points, 15 % visibility         (all of C4 on one GPU)
    tracks1000  1 000 cameras x 50 000 points, Structure(mean_track=8) (track-structured, beyond the single-launch solve)

for lambda in {5.0, 0.5} and cg_tol in {1e-6, 1e-10}.  Per scene and setting:

  * wall milliseconds per outer iteration of ``iterate_pcg`` and of ``iterate`` on the same scene in the same process, the two
    alternating region by region, each region `iters` iterations from the same start state with a synchronise at its end;
    the MEDIAN over the regions and the spread (max - min) / median; one warm-up region each;
  * CG iterations per outer iteration and the statuses;
  * the four parts from sfm_ba_pcg_times (device time by hipEvents, taken in calls of their own: the events cost stream
    bubbles), per outer iteration;
  * per CG iteration, the bytes the two matvec passes move by construction and the bandwidth the measured CG-loop time implies.
    By construction: pass one reads J_o (160 B), cam_idx (4 B) and writes v_o (16 B) per observation, reads D_p^-1 and pt_ptr
    (52 B) per point -- p, and its own re-reads of v_o and Jx, stay in cache; pass two reads cam_obs (4 B), Jp_o (112 B) and
    v_o (16 B) per observation and writes 56 B per 64 observations.  The CG-loop time also holds the one-workgroup vector
    update and the host's flag reads, so the implied bandwidth is a LOWER bound on what the two passes reach.

    python tools/bench_pcg.py [--shapes C3,C4share,C4,tracks1000] [--regions 7] [--iters 3] [--out profiles/pcg/bench_pcg.json]

Prints one JSON line (and rewrites --out after every scene, so a run cut short keeps what it measured).
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

HBM_ACHIEVABLE_TBS = 6.3
L2_BYTES, MALL_BYTES = 8 * 4 * 2 ** 20, 256 * 2 ** 20      # 4 MB of L2 per XCD, 256 MB of Infinity Cache


def make_shape(sfm, name):
    sc = sfm.scenes
    if name == "C3":
        return sc.make_scene(50, 20000, 0.6, seed=0)
    if name == "C4share":
        return sc.make_scene(200, 12500, 0.15, seed=0)
    if name == "C4":
        return sc.make_scene(200, 100000, 0.15, seed=0)
    if name == "tracks1000":
        return sc.make_scene(1000, 50000, seed=0, structure=sc.Structure(mean_track=8))
    raise SystemExit("unknown shape %s" % name)


def region(call, reset, sync):
    reset()
    sync()
    t0 = time.perf_counter()
    call()
    sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C4share,C4,tracks1000")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3, help="outer iterations per region")
    ap.add_argument("--group", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pcg.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"regions": args.regions, "iters": args.iters, "group": args.group, "hbm_achievable_TBs": HBM_ACHIEVABLE_TBS, "shapes": {}}

    def dump():
        line = json.dumps(out)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    for name in args.shapes.split(","):
        t0 = time.perf_counter()
        sc = make_shape(sfm, name)
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        tracks = np.diff(sc.pt_ptr)
        m, n, v = sc.n_obs, sc.n_pts, sc.n_cams
        pass1 = 180 * m + 52 * n
        pass2 = 132 * m + 56 * (m // 64 + v)
        working = 160 * m + 16 * m + 48 * n + 8 * m
        entry = {"n_cams": v, "n_pts": n, "n_obs": m, "track_mean": float(tracks.mean()), "track_max": int(tracks.max()),
                 "scene_build_s": time.perf_counter() - t0, "dense_S_bytes": 8 * (7 * v) ** 2, "pcg_bytes_per_obs": 176 + 35 * 8 / 64,
                 "pass1_bytes": pass1, "pass2_bytes": pass2, "working_set_bytes": working,
                 "fits": "L2" if working <= L2_BYTES else ("Infinity Cache" if working <= MALL_BYTES else "HBM"), "settings": {}}
        with native.BaProblem(v, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            def reset():
                prob.set_state(sc.cams_init, sc.pts_init)

            for lam in (5.0, 0.5):
                def dense():
                    prob.iterate(lam, args.iters)

                for tol in (1e-6, 1e-10):
                    last = {}

                    def pcg():
                        last["out"] = prob.iterate_pcg(lam, args.iters, tol=tol, group=args.group)

                    region(pcg, reset, native.synchronize)            # warm-up: code objects, camera-major list, pool blocks
                    region(dense, reset, native.synchronize)
                    t_pcg, t_dense = [], []
                    for _ in range(args.regions):                     # alternating
                        t_pcg.append(region(pcg, reset, native.synchronize))
                        t_dense.append(region(dense, reset, native.synchronize))
                    t_pcg, t_dense = np.array(t_pcg) / args.iters, np.array(t_dense) / args.iters
                    region(pcg, reset, native.synchronize)            # (the loop ended on the dense route)
                    res = last["out"]
                    cams_p, pts_p = prob.get_state()
                    region(dense, reset, native.synchronize)
                    cams_d, pts_d = prob.get_state()
                    prob.set_option(native.OPT_TIMING, 1)
                    parts = []
                    for _ in range(args.regions):
                        reset()
                        prob.iterate_pcg(lam, args.iters, tol=tol, group=args.group)
                        parts.append(prob.pcg_times() / args.iters)
                    prob.set_option(native.OPT_TIMING, 0)
                    parts = np.median(np.array(parts), axis=0)
                    cg = float(np.mean(res.cg_iters))
                    per_cg_ms = parts[2] / max(cg, 1.0)
                    s = {"pcg_ms_per_iteration": float(np.median(t_pcg) * 1e3),
                         "pcg_spread": float((t_pcg.max() - t_pcg.min()) / np.median(t_pcg)),
                         "dense_ms_per_iteration": float(np.median(t_dense) * 1e3),
                         "dense_spread": float((t_dense.max() - t_dense.min()) / np.median(t_dense)),
                         "pcg_over_dense": float(np.median(t_pcg) / np.median(t_dense)),
                         "cg_iters": [int(k) for k in res.cg_iters], "cg_status": [int(k) for k in res.cg_status],
                         "cg_rel": [float(k) for k in res.cg_rel],
                         "device_linearise_ms": float(parts[0]), "device_blocks_ms": float(parts[1]), "device_cg_loop_ms": float(parts[2]),
                         "device_backsub_ms": float(parts[3]), "host_whole_call_ms": float(parts[4]),
                         "cg_iteration_ms": float(per_cg_ms),
                         "implied_TBs_lower_bound": float((pass1 + pass2) / (per_cg_ms * 1e-3) / 1e12) if per_cg_ms > 0 else 0.0,
                         "state_rel_diff_to_dense": float(max(np.max(np.abs(cams_p - cams_d)) / np.max(np.abs(cams_d)),
                                                              np.max(np.abs(pts_p - pts_d)) / np.max(np.abs(pts_d))))}
                    entry["settings"]["lambda=%g,tol=%g" % (lam, tol)] = s
                    print("%s lambda=%g tol=%g: pcg %.3f ms, dense %.3f ms, cg %s" % (name, lam, tol, s["pcg_ms_per_iteration"],
                                                                                    s["dense_ms_per_iteration"], s["cg_iters"]), file=sys.stderr, flush=True)
        out["shapes"][name] = entry
        dump()
    print(dump())


if __name__ == "__main__":
    main()
