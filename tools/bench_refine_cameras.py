#!/usr/bin/env python3
"""Timing of the motion-only refinement of a resident scene (sfm_ba_refine_cameras) at

    C3       50 cameras x 20 000 points, 60 % visibility            (bench.py's flagship scene)
    C4share  200 cameras x 12 500 points, 15 % visibility           (one GPU's share of C4 on eight)
    C5like   10 views x 5 000 points, consecutive-view tracks       (the shape an incremental run leaves)

for 3 and 30 iterations, and next to each the existing pose refinement, `sfm_pnp_nonlinear_batch_dev`, on the SAME
observations gathered into its layout on the device (K = I on the normalised keys, quirks = Q2 only): the yardstick.  The two
do the same arithmetic per observation; refine_cameras reads the resident scene through its camera-major list, runs one pass
more (the evaluation at the output camera) and ends in its own synchronise, the PnP call gets contiguous copies and is
synchronised by the tool.

A timed region is `inner` back-to-back calls from the same start state, each ending in a stream synchronise (nothing comes
down: cost and status are not requested); the figure is the MEDIAN over the regions of region time / inner, the spread
(max - min) / median over the same regions.  One warm-up region per configuration.  The cameras are reset before every
region (sfm_ba_set_cameras: 2.8 KB at C3) outside the timed calls, so every region does the same work.

    python tools/bench_refine_cameras.py [--shapes C3,C4share,C5like] [--iters 3,30] [--regions 7] [--out FILE]

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


def time_regions(call, reset, regions, target_s=0.02):
    reset()
    call()                                            # loads the code objects, builds the camera-major list
    reset()
    t0 = time.perf_counter()
    call()
    one = max(time.perf_counter() - t0, 1e-6)
    inner = int(min(2000, max(5, target_s / one)))
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
    ap.add_argument("--iters", default="3,30")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine_cameras.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    dev = torch.device("cuda:0")
    out = {"regions": args.regions, "lambda": args.lam, "shapes": {}}
    for name in args.shapes.split(","):
        sc = make_shape(sfm, name)
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        counts = np.bincount(sc.cam_idx, minlength=sc.n_cams)
        classes = np.bincount([native.refine_cameras_plan(int(n))[2] for n in counts], minlength=5)
        entry = {"n_cams": sc.n_cams, "n_pts": sc.n_pts, "n_obs": sc.n_obs, "obs_per_camera_min": int(counts.min()),
                 "obs_per_camera_max": int(counts.max()), "cameras_per_size_class": classes.tolist(), "runs": []}
        cams0 = sc.cams_init.copy()
        cams0[:, 3:7] /= np.linalg.norm(cams0[:, 3:7], axis=1)[:, None]
        # the PnP layout of the same observations: camera-major, ascending point inside a camera
        order = np.argsort(sc.cam_idx, kind="stable")
        offsets = np.zeros(sc.n_cams + 1, dtype=np.int32)
        np.cumsum(counts, out=offsets[1:])
        uv3 = np.vstack((uvn[:, order], np.ones((1, sc.n_obs))))
        x4 = np.vstack((sc.pts_init[:, sc.pt_idx[order]], np.ones((1, sc.n_obs))))
        rots = np.stack([sfm.geometry.quaternion_to_rotation(q) for q in cams0[:, 3:7]])
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
             dict(off=offsets, uv=uv3, x=x4, k=np.tile(np.eye(3).ravel(), (sc.n_cams, 1)), r0=rots.reshape(-1, 9),
                  c0=cams0[:, 0:3]).items()}
        r_out = torch.empty((sc.n_cams, 9), dtype=torch.float64, device=dev)
        c_out = torch.empty((sc.n_cams, 3), dtype=torch.float64, device=dev)
        st_out = torch.empty(sc.n_cams, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with native.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_state(cams0, sc.pts_init)
            for iters in [int(i) for i in args.iters.split(",")]:
                def refine():
                    prob.refine_cameras(args.lam, iters, native.Q2_LOC_JAC_SIGN)

                def pnp():
                    native.pnp_nonlinear_batch_dev(sc.n_cams, t["off"].data_ptr(), sc.n_obs, t["uv"].data_ptr(), t["x"].data_ptr(),
                                                   t["k"].data_ptr(), t["r0"].data_ptr(), t["c0"].data_ptr(), args.lam, iters,
                                                   native.Q2_LOC_JAC_SIGN, r_out.data_ptr(), c_out.data_ptr(), st_out.data_ptr(),
                                                   0, int(counts.max()))
                    native.synchronize()

                med, spread, inner = time_regions(refine, lambda: prob.set_cameras(cams0), args.regions)
                # the same call with the cameras of size class 3 on class 4's launches (SFM_OPT_DEBUG bit 32768): what the
                # single streaming workgroup per camera is worth against two launches per pass
                prob.set_option(native.OPT_DEBUG, 32768)
                med4, spread4, _inner4 = time_regions(refine, lambda: prob.set_cameras(cams0), args.regions)
                prob.set_option(native.OPT_DEBUG, 0)
                pmed, pspread, pinner = time_regions(pnp, lambda: None, args.regions)
                # the two kernels agree on what they computed (1e-9: tests/test_gpu_refine_cameras.py asserts it)
                prob.set_cameras(cams0)
                refine()
                got = prob.get_state()[0]
                pnp()
                dev_c = float(np.max(np.abs(got[:, 0:3] - c_out.cpu().numpy())) / np.max(np.abs(got[:, 0:3])))
                entry["runs"].append({"iters": iters, "refine_cameras_ms_per_call": med * 1e3, "refine_cameras_ms_per_iteration": med * 1e3 / iters,
                                      "refine_cameras_spread": spread, "calls_per_region": inner,
                                      "class3_on_class4_launches_ms_per_call": med4 * 1e3, "class3_on_class4_launches_spread": spread4,
                                      "pnp_batch_dev_ms_per_call": pmed * 1e3, "pnp_batch_dev_ms_per_iteration": pmed * 1e3 / iters,
                                      "pnp_batch_dev_spread": pspread, "pnp_calls_per_region": pinner,
                                      "pnp_status_ok": bool((st_out == 0).all().item()), "centre_deviation_rel": dev_c})
        out["shapes"][name] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
