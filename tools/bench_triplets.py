#!/usr/bin/env python3
"""Timing of the view-triplet filter (sfm_view_triplets -> the key-major list kernels twice, triplets_other_end_kernel,
triplets_own_end_kernel, triplets_adjacency_kernel, triplets_enumerate_kernel, triplets_summary_kernel and the prefix sum) on

    band100x8   band1000x8   band1000x30   complete200      (views on a band joined to the next k; the complete graph)

Edges: the true relative rotation times 0.5 degrees of noise, 10 % of them replaced by random rotations; 5 degrees admitted for
the loop.  The call is the host-array form: it uploads the graph, sorts the adjacency, runs its kernels, downloads its outputs
and synchronises.

Two yardsticks, both in the same job: (a) the NumPy reference of tests/_triplets_reference.py on the same host, run ONCE per
shape; (b) sfm_rotation_average at 128 trees and 2 rounds on the same graph -- the call the filter protects.  The filter is
worth its place if it costs a fraction of that averaging: `ratio_to_averaging` reports it and nothing asserts it.

A timed region is `inner` back-to-back calls (at least 0.1 s); the figure is the MEDIAN over the regions of region time /
inner, the spread is (max - min) / median over the same regions; two rounds, both kept.

    python tools/bench_triplets.py [--cases band100x8,band1000x8,band1000x30,complete200] [--groups 0] [--regions 7]
                                   [--no-reference] [--no-averaging] [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2
--no-reference --no-averaging and one case, and read the triplets_* and ba_cam_list_* rows.
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
import _triplets_reference as tr  # noqa: E402

MAX_DEG, NOISE_DEG, WRONG, REGION_S = 5.0, 0.5, 0.1, 0.1


def graph(case):
    if case.startswith("band"):
        V, k = (int(v) for v in case[4:].split("x"))
        pairs = tr.topo_band(V, k, np.random.default_rng(V + k))
    elif case.startswith("complete"):
        V = int(case[8:])
        pairs = rr.topo_complete(V, None)
    else:
        raise SystemExit("unknown case %r" % case)
    return tr.make_case(case, V, pairs, 7, noise_deg=NOISE_DEG, wrong_share=WRONG, max_loop_deg=MAX_DEG, max_angle_deg=MAX_DEG)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="band100x8,band1000x8,band1000x30,complete200")
    ap.add_argument("--groups", default="0")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--no-averaging", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_triplets.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"max_loop_deg": MAX_DEG, "noise_deg": NOISE_DEG, "wrong_share": WRONG, "regions": args.regions, "region_s": REGION_S, "cases": {}}
    for case in [c for c in args.cases.split(",") if c]:
        g = graph(case)
        E = int(g.edges.shape[0])
        entry = {"views": g.V, "edges": E, "runs": []}
        if not args.no_reference:
            t0 = time.perf_counter()
            ref = tr.run(g.V, g.edges, g.rel, None, g.cos_loop)
            entry["reference_ms"] = (time.perf_counter() - t0) * 1e3
        if not args.no_averaging:
            def averaging():
                return native.rotation_average(g.V, g.edges, g.rel, 0, g.cos_max, 128, 2, 2, cg_tol=1e-10, cg_max=200)

            averaging()
            entry["rotation_average"] = [time_call(averaging, lambda: None, args.regions, REGION_S) for _round in range(2)]
        for group in [int(v) for v in args.groups.split(",")]:
            def call():
                return native.view_triplets(g.V, g.edges, g.rel, None, g.cos_loop, 1, 0, 0, group)

            got = call()
            summary = dict(zip(native.TRIPLET_SUMMARY, got[4].tolist()))
            run = {"group": group, "summary": summary, "tests_per_call": 3 * summary["triplets"], "view_triplets": []}
            if not args.no_reference:
                run["equals_reference"] = bool(np.array_equal(got[0], ref.edge_keep) and np.array_equal(got[1], ref.n_tri)
                                               and np.array_equal(got[2], ref.n_ok) and np.array_equal(got[4], ref.summary))
            for _round in range(2):
                run["view_triplets"].append(time_call(call, lambda: None, args.regions, REGION_S))
            if not args.no_averaging:
                run["ratio_to_averaging"] = [a["ms_per_call"] / b["ms_per_call"] for a, b in zip(run["view_triplets"], entry["rotation_average"])]
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
