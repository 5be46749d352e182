#!/usr/bin/env python3
"""Timing of the rotation averaging (sfm_rotation_average -> the key-major list kernels, rotavg_tree_kernel,
rotavg_score_kernel, rotavg_adopt_kernel, rotavg_step_kernel, rotavg_accept_kernel, rotavg_judge_kernel) on random connected
view graphs of

    100x800   1000x8000   1000x30000      (views x edges)

each at max_hyp 128 and 1 024 and at iters 0 and 2 (two Gauss-Newton steps per round).  Edges: the true relative rotation
times 0.5 degrees of noise, 3 % of them replaced by random rotations; 5 degrees admitted.  The call is the host-array form: it
uploads the graph, builds the adjacency, runs its kernels, downloads its outputs and synchronises.

The yardstick is the NumPy reference of tests/_rotavg_reference.py on the same host (there is no parent to compare with).  It
is run ONCE per shape and iters at `--ref-hyp` hypotheses (default 8).  Its hypotheses cost the same each and its refit does
not depend on their number, so `reference_ms_scaled` = (time at iters 0) x max_hyp / ref_hyp + (time at iters - time at
iters 0): an estimate, marked as scaled; `reference_ms_at_ref_hyp` is what was measured.

A timed region is `inner` back-to-back calls (at least 0.1 s); the figure is the MEDIAN over the regions of region time /
inner, the spread is (max - min) / median over the same regions; two rounds, both kept.

    python tools/bench_rotavg.py [--cases 100x800,1000x8000,1000x30000] [--max-hyp 128,1024] [--iters 0,2] [--regions 7]
                                 [--ref-hyp 8] [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2 --ref-hyp 0
and one case, and read the rotavg_* rows.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

from bench_tri_ransac import time_call  # noqa: E402  (the same regions)
import _rotavg_reference as rr  # noqa: E402

MAX_ANGLE_DEG, NOISE_DEG, WRONG, STEPS, REGION_S = 5.0, 0.5, 0.03, 2, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="100x800,1000x8000,1000x30000")
    ap.add_argument("--max-hyp", default="128,1024")
    ap.add_argument("--iters", default="0,2")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--ref-hyp", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rotavg.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"max_angle_deg": MAX_ANGLE_DEG, "noise_deg": NOISE_DEG, "wrong_share": WRONG, "steps": STEPS, "regions": args.regions,
           "region_s": REGION_S, "ref_hyp": args.ref_hyp, "cases": {}}
    for case in [c for c in args.cases.split(",") if c]:
        V, E = (int(v) for v in case.split("x"))
        g = rr.make_case(case, V, rr.topo_random(V, np.random.default_rng(V + E), E), 7, noise_deg=NOISE_DEG, wrong_share=WRONG,
                         max_angle_deg=MAX_ANGLE_DEG)
        entry = {"views": V, "edges": E, "runs": []}

        def reference(iters):
            t0 = time.perf_counter()
            rr.run(g.V, g.edges, g.rel, 0, g.cos_max, args.ref_hyp, iters, STEPS, route="cg")
            return time.perf_counter() - t0

        ref_0 = reference(0) if args.ref_hyp > 0 else None
        for iters in [int(v) for v in args.iters.split(",")]:
            ref_s = None if ref_0 is None else (ref_0 if iters == 0 else reference(iters))
            for max_hyp in [int(h) for h in args.max_hyp.split(",")]:
                def call():
                    return native.rotation_average(g.V, g.edges, g.rel, 0, g.cos_max, max_hyp, iters, STEPS, cg_tol=1e-10, cg_max=200)

                got = call()
                run = {"max_hyp": max_hyp, "iters": iters, "tests_per_call": int(max_hyp) * E, "status": got[6], "best_hyp": got[5],
                       "summary": dict(zip(native.ROTAVG_SUMMARY, got[7].tolist())), "rotation_average": []}
                if ref_s is not None:
                    run["reference_ms_at_ref_hyp"] = ref_s * 1e3
                    run["reference_ms_scaled"] = (ref_0 * max_hyp / args.ref_hyp + max(ref_s - ref_0, 0.0)) * 1e3
                for _round in range(2):
                    run["rotation_average"].append(time_call(call, lambda: None, args.regions, REGION_S))
                entry["runs"].append(run)
        out["cases"][case] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
