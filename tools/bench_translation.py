#!/usr/bin/env python3
"""Timing of the translation averaging (sfm_translation_average -> the key-major list kernels, transavg_direct_kernel,
transavg_conn_kernel, transavg_solve_kernel, transavg_output_kernel) on random connected view graphs of

    100x800   1000x8000   1000x30000      (views x edges)

each at rounds 0 and 8, with the polish.  Edges: the true direction turned by up to 0.5 degrees, 3 % of them replaced by a
direction 30 .. 150 degrees away; 5 degrees admitted, mu = 0.01, CG to 1e-13.  The call is the host-array form: it uploads the
graph, builds the adjacency, runs its kernels, downloads its outputs and synchronises.

The yardstick is the NumPy reference of tests/_transavg_reference.py (its CG route) on the same host, run ONCE per shape and
rounds (`--no-ref` leaves it out).  The CG iterations of every solve come from the call's own log.

A timed region is `inner` back-to-back calls (at least 0.1 s); the figure is the MEDIAN over the regions of region time /
inner, the spread is (max - min) / median over the same regions; two rounds of regions, both kept.

    python tools/bench_translation.py [--cases 100x800,1000x8000,1000x30000] [--rounds 0,8] [--regions 7] [--no-ref] [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2 --no-ref and
one case, and read the transavg_* rows.
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
import _transavg_reference as tr  # noqa: E402

MAX_ANGLE_DEG, NOISE_DEG, WRONG, MU, CG_TOL, CG_MAX, REGION_S = 5.0, 0.5, 0.03, 0.01, 1e-13, 500, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="100x800,1000x8000,1000x30000")
    ap.add_argument("--rounds", default="0,8")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_translation.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"max_angle_deg": MAX_ANGLE_DEG, "noise_deg": NOISE_DEG, "wrong_share": WRONG, "mu": MU, "cg_tol": CG_TOL, "cg_max": CG_MAX,
           "regions": args.regions, "region_s": REGION_S, "cases": {}}
    for case in [c for c in args.cases.split(",") if c]:
        V, E = (int(v) for v in case.split("x"))
        g = tr.make_case(case, V, rr.topo_random(V, np.random.default_rng(V + E), E), 7, noise_deg=NOISE_DEG, wrong_share=WRONG,
                         max_angle_deg=MAX_ANGLE_DEG, mu=MU)
        entry = {"views": V, "edges": E, "runs": []}
        for rounds in [int(v) for v in args.rounds.split(",")]:
            def call():
                return native.translation_average(g.V, g.edges, g.R, g.t, None, 0, g.cos_max, MU, rounds, 1, CG_TOL, CG_MAX)

            got = call()
            run = {"rounds": rounds, "polish": 1, "status": got[6], "n_inliers": got[5], "summary": dict(zip(native.TRANSAVG_SUMMARY, got[7].tolist())),
                   "cg_iterations": got[8][:, 1].astype(int).tolist(), "flags_exact": bool(np.array_equal(got[1] == 0, g.replaced)),
                   "translation_average": []}
            if not args.no_ref:
                t0 = time.perf_counter()
                ref = tr.run(g.V, g.edges, g.R, g.t, None, 0, g.cos_max, MU, rounds, 1, route="cg", cg_tol=CG_TOL, cg_max=CG_MAX)
                run["reference_ms"] = (time.perf_counter() - t0) * 1e3
                run["reference_cg_iterations"] = ref.log[:, 1].astype(int).tolist()
                run["decisions_equal"] = bool(np.array_equal(ref.edge_inlier, got[1]) and ref.status == got[6])
            for _round in range(2):
                run["translation_average"].append(time_call(call, lambda: None, args.regions, REGION_S))
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
