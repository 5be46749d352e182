#!/usr/bin/env python3
"""Key-track bookkeeping around the matching kernels: HipDeviceKeyTracker (tracks on the device, csrc/sfm_track.hip)
against HipKeyTracker (the host path of matching.py), in one process on the same inputs.

Run on an MI355X:  timeout -k 10 900 python tools/bench_track.py [--reps 20] [--sizes 2000,5000,8000] [--refs 1,9] [--process]

Per (N keys, R resident views), for the LAST view of a make_descriptor_views workload:
  * wall time of ``add_new_view`` followed by ``generate_matched_pairs(0, new, views)`` -- both calls block, so a host
    clock around them is the time a caller waits -- for both trackers, alternating, each on a fresh tracker that
    already holds the R views (set-up not timed): median, min and max over the timed calls after the warm-up ones;
  * device time (hip events on a torch side stream around the enqueued work) of sfm_match_dev alone and of
    sfm_track_extend_dev alone on its outputs.
``--process`` adds the wall time of ``HipBaProcessor.process`` per upenn frame (tests/golden/g13_upenn_*.npz) with either
tracker.  Kernel-level times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.  Prints one
JSON line per configuration; starts nothing else on the GPU."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class View:
    def __init__(self, key_pts, key_descriptors, key_xy):
        self.key_pts, self.key_descriptors, self.key_xy = key_pts, key_descriptors, key_xy


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4)}


def workload(sfm, n_keys, n_views, seed):
    n_dup = max(6, n_keys // 100)
    n_pts = n_keys                                          # 0.8 n seen points + distractors + 2 n_dup copies: about n_keys keys
    dv = sfm.scenes.make_descriptor_views(n_views=n_views, n_pts=n_pts, seed=seed, visibility=0.8,
                                          n_distract=max(0, n_keys - int(0.8 * n_pts) - 2 * n_dup), n_dup=n_dup, orb_flips=1)
    return [View(dv.key_pts(v), dv.sift[v], dv.pix[v].astype(np.float32).astype(np.float64)) for v in range(n_views)]


def timed_last_view(cls, views, is_knn):
    kt = cls("sift", False, is_knn, False, None)
    try:
        for v in range(len(views) - 1):
            kt.add_new_view(views[v], views[:v])
        new = len(views) - 1
        t0 = time.perf_counter()
        kt.add_new_view(views[new], views[:new])
        t1 = time.perf_counter()
        pairs = kt.generate_matched_pairs(0, new, views)
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, pairs[1].shape[1]
    finally:
        kt.kt_release()


def device_stage_times(nat, torch, views, reps, warmup):
    """hip-event time of the matching launch and of the track extend on its outputs (microseconds, medians).  The work
    and the events go on a stream of torch's own making: torch's default stream has the handle 0, which the library
    takes for "my own stream", and events on the default stream would then time nothing."""
    side = torch.cuda.Stream()
    stream = side.cuda_stream
    assert stream != 0
    sets = [nat.DescriptorSet(nat.MATCH_L2, v.key_descriptors) for v in views]
    store = nat.TrackStore()
    try:
        for v in views:
            store.add_view(v.key_xy)
        r, n = len(views) - 1, len(views[-1].key_pts)
        outs = [torch.empty((r, n), dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.int32, torch.float32, torch.uint8)]
        ptrs = [o.data_ptr() for o in outs]
        match_us, extend_us = [], []
        for i in range(warmup + reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record(side)
            nat.match_dev(sets[-1], sets[:-1], nat.MATCH_KNN2, *ptrs, stream=stream)
            e[1].record(side)
            store.extend_dev(r, r, nat.MATCH_KNN2, *ptrs, stream=stream)
            e[2].record(side)
            torch.cuda.synchronize()
            if i >= warmup:
                match_us.append(e[0].elapsed_time(e[1]) * 1e3)
                extend_us.append(e[1].elapsed_time(e[2]) * 1e3)
        return stats(match_us), stats(extend_us)
    finally:
        store.close()
        for s in sets:
            s.close()


def process_times(sfm, reps):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _sift_chain as C
    P = sfm.processors
    imgs, k = [C.fixture(n)["image"] for n in (1, 2, 3)], C.halved_k()
    out = {}
    for name, cls in (("host", P.HipKeyTracker), ("device", P.HipDeviceKeyTracker)):
        per_frame = [[], [], []]
        for rep in range(reps + 1):
            cfg = P.RansacConfig(1e-2, 0.99, 0.75, 8, 200)
            vp, kt = P.HipViewProcessor('sift'), cls('sift', False, True, False, cfg)
            bp = P.HipBaProcessor(vp, kt, P.HipEpipolarProcessor(P.RansacConfig(1e-2, 0.99, 0.75, 8, 300)), P.HipTriangulationProcessor(),
                                  P.HipCamposeProcessor(P.RansacConfig(8.0, 0.99, 0.75, 8, 300), 5, 300))
            bp.ba_verbose = False
            try:
                for f, img in enumerate(imgs):
                    t0 = time.perf_counter()
                    bp.process(img, k)
                    if rep:                                     # the first pass warms up
                        per_frame[f].append((time.perf_counter() - t0) * 1e3)
            finally:
                bp.ba_release()
                kt.kt_release()
        out[name] = [stats(f) for f in per_frame]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="2000,5000,8000")
    ap.add_argument("--refs", default="1,9")
    ap.add_argument("--nn1", action="store_true", help="plain 1-NN matching (dense duplicates) instead of knn + ratio test")
    ap.add_argument("--process", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_track.py needs an MI355X")
    sfm = importlib.import_module("structure-from-motion_amd")
    nat, P = sfm.native, sfm.processors
    nat.init(0)
    for n in [int(x) for x in a.sizes.split(",")]:
        for r in [int(x) for x in a.refs.split(",")]:
            views = workload(sfm, n, r + 1, seed=n + r)
            times = {"host": ([], []), "device": ([], [])}
            n_pairs = {}
            for i in range(a.warmup + a.reps):                      # alternate the two trackers
                for name, cls in (("host", P.HipKeyTracker), ("device", P.HipDeviceKeyTracker)):
                    add_ms, pairs_ms, n_pairs[name] = timed_last_view(cls, views, not a.nn1)
                    if i >= a.warmup:
                        times[name][0].append(add_ms)
                        times[name][1].append(pairs_ms)
            assert n_pairs["host"] == n_pairs["device"]
            match_us, extend_us = device_stage_times(nat, torch, views, a.reps, a.warmup)
            row = {"keys": len(views[-1].key_pts), "resident_views": r, "mode": "nn1" if a.nn1 else "knn2", "pairs_0_new": n_pairs["host"],
                   "reps": a.reps}
            for name in ("host", "device"):
                total = [x + y for x, y in zip(*times[name])]
                row[name + "_ms"] = {"add_new_view": stats(times[name][0]), "generate_matched_pairs": stats(times[name][1]),
                                     "both": stats(total)}
            row["speedup_both_median"] = round(row["host_ms"]["both"]["median"] / row["device_ms"]["both"]["median"], 3)
            row["event_us"] = {"sfm_match_dev": match_us, "sfm_track_extend_dev": extend_us}
            print(json.dumps(row), flush=True)
    if a.process:
        print(json.dumps({"process_ms_per_upenn_frame": process_times(sfm, max(3, a.reps // 4))}), flush=True)


if __name__ == "__main__":
    main()
