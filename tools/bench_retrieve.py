#!/usr/bin/env python3
"""Timing of the view-pair selection: sfm_vocab_train, sfm_view_describe and sfm_view_pairs separately (host-array forms: each
uploads what it takes, runs its kernels, downloads its outputs and synchronises), on band scenes of

    100x2000   100x8000   1000x2000   1000x8000       (views x keys per view, 128 dimensions)      at K = 64 and 256 words

A view sees a window of a pool of landmarks that slides with its index (neighbours share two thirds of their keys); a key is
its landmark's uint8 descriptor plus noise.  4 rounds of training, k = 8 neighbours, sequential = 1.

Two yardsticks, both in the same job: (a) the NumPy reference of tests/_retrieve_reference.py on the same host, run ONCE per
shape and step (left out above --reference-max-keys keys in all); (b) the descriptor searches the selection saves:
sfm_match_dev of one view of the shape against another, timed the same way, times V (V - 1) / 2 (every pair, what
add_new_view does) against times the number of listed pairs plus the selection itself.  The ratios are reported, nothing is
asserted.

A timed region is `inner` back-to-back calls (at least 0.1 s, at least 5 calls); the figure is the MEDIAN over the regions of
region time / inner, the spread is (max - min) / median over the same regions; two rounds, both kept.

    python tools/bench_retrieve.py [--cases 100x2000,...] [--words 64,256] [--regions 7] [--reference-max-keys N] [--once]
                                   [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --once (one call of each
step, no reference, no matcher) and one case, and read the retr_* and ba_cam_list_* rows.
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
import _retrieve_reference as rr  # noqa: E402

D, ITERS, NBRS, SEQUENTIAL, REGION_S = 128, 4, 8, 1, 0.1


def scene(V, keys, seed=1):
    """V uint8 (keys, D) arrays: view a holds the landmarks a * keys / 3 .. a * keys / 3 + keys - 1 of a pool, shuffled, each
    with +-12 of noise per dimension."""
    rng = np.random.default_rng(seed)
    step = max(keys // 3, 1)
    pool = rng.integers(0, 256, (step * (V - 1) + keys, D), dtype=np.uint8)
    pool[rng.random(pool.shape) < 0.3] = 0
    views = []
    for a in range(V):
        idx = rng.permutation(keys) + a * step
        noisy = pool[idx].astype(np.int16) + rng.integers(-12, 13, (keys, D), dtype=np.int16)
        views.append(np.clip(noisy, 0, 255).astype(np.uint8))
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="100x2000,100x8000,1000x2000,1000x8000")
    ap.add_argument("--words", default="64,256")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reference-max-keys", type=int, default=2100000)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieve.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"dim": D, "iters": ITERS, "k": NBRS, "sequential": SEQUENTIAL, "regions": args.regions, "region_s": REGION_S, "cases": {}}
    for case in [c for c in args.cases.split(",") if c]:
        V, keys = (int(v) for v in case.split("x"))
        views = scene(V, keys)
        sets = [native.DescriptorSet(native.MATCH_L2, v) for v in views]
        entry = {"views": V, "keys_per_view": keys, "runs": []}
        if not args.once:                                      # one descriptor search of this shape, device arrays, synchronised
            bufs = [torch.empty((1, keys), dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.int32, torch.float32, torch.uint8)]

            def search():
                native.match_dev(sets[1], [sets[0]], native.MATCH_KNN2, *(b.data_ptr() for b in bufs))
                native.synchronize()

            entry["match_dev"] = [time_call(search, lambda: None, args.regions, REGION_S) for _round in range(2)]
        with_reference = not args.once and V * keys <= args.reference_max_keys
        for K in [int(v) for v in args.words.split(",")]:
            run = {"K": K}
            words, log = native.vocab_train(sets, K, ITERS, 1)
            with native.DescriptorSet(native.MATCH_L2, words) as voc:
                d = native.view_describe(voc, sets, outputs=("desc", "norm2"))
                p = native.view_pairs(d["desc"], d["norm2"], NBRS, sequential=SEQUENTIAL)
                near = {(a, a + 1) for a in range(V - 1)} | {(a, a + 2) for a in range(V - 2)}
                listed = set(map(tuple, p["pairs"].tolist()))
                run.update(n_pairs=p["n_pairs"], all_pairs=V * (V - 1) // 2, near_listed=len(near & listed), near=len(near),
                           inertia=log[:, 0].tolist(), max_abs_q=int(np.abs(d["desc"]).max()))
                if with_reference:
                    t0 = time.perf_counter()
                    ref_words, ref_log = rr.train(np.concatenate(views), K, ITERS, 1)
                    t1 = time.perf_counter()
                    ref_d = rr.describe(ref_words, views)
                    t2 = time.perf_counter()
                    ref_p = rr.pairs(ref_d["desc"], ref_d["norm2"], NBRS, sequential=SEQUENTIAL)
                    t3 = time.perf_counter()
                    run["reference_ms"] = {"train": (t1 - t0) * 1e3, "describe": (t2 - t1) * 1e3, "pairs": (t3 - t2) * 1e3}
                    run["equals_reference"] = bool(
                        np.array_equal(words, ref_words) and np.array_equal(log, ref_log) and np.array_equal(d["desc"], ref_d["desc"])
                        and np.array_equal(d["norm2"], ref_d["norm2"]) and np.array_equal(p["nbr"], ref_p["nbr"])
                        and np.array_equal(rr.bits(p["nbr_score"]), rr.bits(ref_p["nbr_score"])) and np.array_equal(p["pairs"], ref_p["pairs"])
                        and np.array_equal(p["how"], ref_p["how"]) and np.array_equal(rr.bits(p["pair_score"]), rr.bits(ref_p["pair_score"])))
                if not args.once:
                    steps = {"train": lambda: native.vocab_train(sets, K, ITERS, 1),
                             "describe": lambda: native.view_describe(voc, sets, outputs=("desc", "norm2")),
                             "pairs": lambda: native.view_pairs(d["desc"], d["norm2"], NBRS, sequential=SEQUENTIAL)}
                    for name, call in steps.items():
                        run[name] = [time_call(call, lambda: None, args.regions, REGION_S) for _round in range(2)]
                    select_ms = sum(run[name][1]["ms_per_call"] for name in steps)
                    search_ms = entry["match_dev"][1]["ms_per_call"]
                    run["select_ms"] = select_ms
                    run["match_all_pairs_ms"] = search_ms * run["all_pairs"]
                    run["match_listed_pairs_ms"] = search_ms * run["n_pairs"]
                    run["ratio_all_to_select_plus_listed"] = run["match_all_pairs_ms"] / (select_ms + run["match_listed_pairs_ms"])
                    if with_reference:
                        run["ratio_reference_to_device"] = {name: run["reference_ms"][name] / run[name][1]["ms_per_call"] for name in steps}
            entry["runs"].append(run)
        for s in sets:
            s.close()
        out["cases"][case] = entry
        sys.stderr.write("%s done\n" % case)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
