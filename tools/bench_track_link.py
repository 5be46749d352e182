#!/usr/bin/env python3
"""Timing of the track linking (sfm_link_tracks -> link_verify / init / union / flatten / fill / order / gather kernels and the
two prefix sums of csrc/sfm_track_link.hip) on ring scenes of

    100x2000x800   1000x8000x8000   1000x8000x30000      (views x keys per view x pairs)

Views stand on a ring; a scene point is seen by L consecutive views, L uniform in 2 .. 14 (tracks of mean length 8); the pairs
are (i, i + d) for d = 1, 2, ... until the count is reached (pairs beyond the longest track share nothing and are listed all
the same); a shared point is matched with 85 %, and 3 % of the matches name a random key of the second view.

The ARRAY form is the host-array call (it uploads the matches, runs its kernels, downloads every output and synchronises) and
the device-pointer call on resident arrays (kernels and the two small reads only).  `--scan 1,2` times the device form under
each prefix-sum route, which is how the crossover of kLkScanCrossover is found.  The STORE form (TrackStore.link) runs on the
cases of --store-cases: a store holds a dense table per view, views x keys ints, so only the small shape by default.

The yardstick is the vectorised propagation route of tests/_track_link_reference.py on the same host, run ONCE per shape
(`--no-ref` leaves it out).  A timed region is `inner` back-to-back calls (at least 0.1 s); the figure is the MEDIAN over the
regions of region time / inner, the spread is (max - min) / median over the same regions.

    python tools/bench_track_link.py [--cases ...] [--store-cases 100x2000x800] [--scan 0] [--regions 7] [--no-ref] [--out FILE]

Prints one JSON line.  The kernels' times alone: run it under `rocprofv3 --kernel-trace --stats` with --regions 2 --no-ref
--store-cases "" and one case, and read the link_* and *scan* rows.
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
import _track_link_reference as ref  # noqa: E402

L_MIN, L_MAX, KEEP, WRONG, REGION_S = 2, 14, 0.85, 0.03, 0.1


def ring_case(V, keys, P, seed):
    rng = np.random.default_rng(seed)
    N = V * keys * 2 // (L_MIN + L_MAX)
    length = rng.integers(L_MIN, L_MAX + 1, N)
    first = rng.integers(0, V, N)
    start = np.concatenate(([0], np.cumsum(length)))
    point = np.repeat(np.arange(N), length)
    off = np.arange(start[-1]) - start[point]
    view = (first[point] + off) % V
    # the key of an observation: its place among the observations of its view, in a random order
    order = np.lexsort((rng.random(view.size), view))
    n_keys = np.bincount(view, minlength=V)
    key_ptr = np.concatenate(([0], np.cumsum(n_keys)))
    key = np.empty(view.size, dtype=np.int64)
    key[order] = np.arange(view.size) - key_ptr[view[order]]
    parts = []
    for d in range(1, (P + V - 1) // V + 1):
        idx = np.flatnonzero(off + d < length[point])
        idx = idx[(view[idx] + (d - 1) * V < P) & (rng.random(idx.size) < KEEP)]
        parts.append((view[idx] + (d - 1) * V, key[idx], key[idx + d], view[idx + d]))
    pair = np.concatenate([p[0] for p in parts])
    a, b, second = (np.concatenate([p[k] for p in parts]) for k in (1, 2, 3))
    wrong = rng.random(pair.size) < WRONG
    b[wrong] = (rng.random(int(wrong.sum())) * n_keys[second[wrong]]).astype(np.int64)
    by_pair = np.argsort(pair, kind="stable")
    pair_ptr = np.concatenate(([0], np.cumsum(np.bincount(pair, minlength=P)))).astype(np.int64)
    p = np.arange(P)
    pair_views = np.stack((p % V, (p % V + p // V + 1) % V), axis=1).astype(np.int32)
    return {"key_ptr": key_ptr.astype(np.int32), "pair_views": pair_views, "pair_ptr": pair_ptr, "a": a[by_pair].astype(np.int32),
            "b": b[by_pair].astype(np.int32), "mask": None, "min_len": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="100x2000x800,1000x8000x8000,1000x8000x30000")
    ap.add_argument("--store-cases", default="100x2000x800")
    ap.add_argument("--scan", default="0")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_link.py needs an MI355X (no GPU visible); nothing is measured without one")
    sfm = importlib.import_module("structure-from-motion_amd")
    native = sfm.native
    native.init(0)
    out = {"track_length": [L_MIN, L_MAX], "match_share": KEEP, "wrong_share": WRONG, "regions": args.regions, "region_s": REGION_S, "cases": {}}
    store_cases = [c for c in args.store_cases.split(",") if c]
    for name in [c for c in args.cases.split(",") if c]:
        V, keys, P = (int(v) for v in name.split("x"))
        c = ring_case(V, keys, P, V + P)
        K, M = int(c["key_ptr"][-1]), int(c["pair_ptr"][-1])

        def host_form():
            return native.track_link(c["key_ptr"], c["pair_views"], c["pair_ptr"], c["a"], c["b"])

        got = host_form()
        entry = {"views": V, "keys": K, "pairs": P, "matches": M, "summary": dict(zip(native.LINK_SUMMARY, got["summary"].tolist())),
                 "plan": native.track_link_plan(V, K, M)}
        if not args.no_ref:
            t0 = time.perf_counter()
            want = ref.link(c, "propagation")
            entry["reference_ms"] = (time.perf_counter() - t0) * 1e3
            entry["equal_to_reference"] = bool(ref.same(got, want))
        entry["host_form"] = time_call(host_form, lambda: None, args.regions, REGION_S)
        d_a, d_b = torch.from_numpy(c["a"]).cuda(), torch.from_numpy(c["b"]).cuda()
        d_out = [torch.empty(n, dtype=torch.int32, device="cuda") for n in (K, K // 2 + 2, K, K)]
        d_sum = torch.empty(8, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        entry["device_form"] = {}
        for scan in [int(v) for v in args.scan.split(",")]:
            def dev_form():
                return native.track_link_dev(c["key_ptr"], c["pair_views"], c["pair_ptr"], d_a.data_ptr(), d_b.data_ptr(), scan=scan,
                                             d_key_track=d_out[0].data_ptr(), d_pt_ptr=d_out[1].data_ptr(), d_cam_idx=d_out[2].data_ptr(),
                                             d_key_idx=d_out[3].data_ptr(), d_summary=d_sum.data_ptr())

            assert dev_form() == (int(got["summary"][2]), int(got["summary"][5]))
            entry["device_form"]["scan_%d" % scan] = time_call(dev_form, lambda: None, args.regions, REGION_S)
        del d_a, d_b, d_out
        if name in store_cases:
            rng = np.random.default_rng(1)
            with native.TrackStore() as store:
                for v in range(V):
                    n = int(c["key_ptr"][v + 1] - c["key_ptr"][v])
                    store.add_view(rng.uniform(0, 1000, (n, 2)))
                    store.set_normalised(v, rng.standard_normal((2, n)))
                kept = 0
                for p, (r, q) in enumerate(c["pair_views"]):
                    a, b = c["a"][c["pair_ptr"][p]:c["pair_ptr"][p + 1]], c["b"][c["pair_ptr"][p]:c["pair_ptr"][p + 1]]
                    _, ia = np.unique(a, return_index=True)
                    _, ib = np.unique(b[ia], return_index=True)
                    store.set_pairs(int(r), int(q), a[ia][ib], b[ia][ib])
                    kept += int(np.count_nonzero(b[ia][ib] > 0))
                pairs = [(int(r), int(q)) for r, q in c["pair_views"]]
                summary = store.link(pairs)
                entry["store_form"] = {"matches": kept, "table_entries_read": int(sum(store.n_keys(r) for r, _ in pairs)),
                                       "summary": dict(zip(native.LINK_SUMMARY, summary.tolist())),
                                       "link": time_call(lambda: store.link(pairs), lambda: None, args.regions, REGION_S)}
                assert summary[0] == kept
        out["cases"][name] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
