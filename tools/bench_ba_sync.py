#!/usr/bin/env python3
"""The structure step of the per-view bundle adjustment: HipBaMixin.ba_device_tracks on (the observation list is built
and compared on the device, csrc/sfm_track.hip + csrc/sfm_ba_host.hip) against off (the track tables come down, are
diffed and gathered on the host and the new observations go up through sfm_ba_append), in one process on the same inputs.

Run on an MI355X:  timeout -k 10 1100 python tools/bench_ba_sync.py [--reps 20] [--warmup 3] [--sizes 2000,5000,8000]
                                                                     [--views 3,10] [--iterations 3,1]

Per (N keys, V views, BA iterations), for the LAST view of a seeded make_descriptor_views workload through
HipDeviceKeyTracker: every pass builds a fresh tracker and processor, registers the views 0 .. V-2 (usage lists that make
each view observe the points known so far, one key per point, never key 0, so that both paths append), runs their bundle
adjustment, registers view V-1 -- none of it timed -- and then times ``execute_bundle_adjustment``: the call blocks, so a
host clock around it is what a caller waits.  The two settings alternate pass by pass; median, min and max over the
timed passes after the warm-up ones.  ``iterations = 1`` leaves less solver time around the structure step.  Also per
setting: what the call did and the bytes it moved (BA uploads, tracker uploads and downloads).  Prints one JSON line
per configuration; starts nothing else on the GPU."""
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
    def __init__(self, rot, loc, k, key_pts, key_descriptors, key_xy):
        self.rot, self.loc, self.k = rot, loc, k
        self.key_pts, self.key_descriptors, self.key_xy = key_pts, key_descriptors, key_xy

    def update_cam_pose(self, rot, loc):
        self.rot, self.loc = rot, loc


class Holder:
    pass


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4)}


def workload(sfm, n_keys, n_views, seed):
    """The descriptor views of tools/bench_track.py plus the plan of the incremental loop: per view c >= 1 the scene points
    that become known with it (seen by view c and an earlier view) and, per view v <= c, the (keys, point ids) to write."""
    n_dup = max(6, n_keys // 100)
    dv = sfm.scenes.make_descriptor_views(n_views=n_views, n_pts=n_keys, seed=seed, visibility=0.8,
                                          n_distract=max(0, n_keys - int(0.8 * n_keys) - 2 * n_dup), n_dup=n_dup, orb_flips=1)
    first_key = []                                       # per view: scene point -> its first key > 0, or -1
    for v in range(n_views):
        fk = np.full(n_keys, -1, dtype=np.int64)
        p = dv.point[v]
        keys = np.flatnonzero(p >= 0)
        keys = keys[keys > 0][::-1]
        fk[p[keys]] = keys                               # reversed: the smallest key is written last
        first_key.append(fk)
    tri_of = np.full(n_keys, -1, dtype=np.int64)         # scene point -> index in tri_pts
    order, plan = [], [None]
    for c in range(1, n_views):
        earlier = np.zeros(n_keys, dtype=bool)
        for v in range(c):
            earlier |= first_key[v] >= 0
        new = np.flatnonzero((first_key[c] >= 0) & earlier & (tri_of < 0))
        tri_of[new] = len(order) + np.arange(new.shape[0])
        order.extend(new.tolist())
        writes = []
        for v in range(c + 1):
            pts = new if v < c else np.flatnonzero((first_key[c] >= 0) & (tri_of >= 0))
            pts = pts[first_key[v][pts] >= 0]
            writes.append((first_key[v][pts], tri_of[pts]))
        plan.append((new.shape[0], writes))
    rng = np.random.default_rng(seed + 1)
    tri = dv.pts[:, np.array(order, dtype=np.int64)] + rng.normal(0, 0.01, (3, len(order)))
    return dv, plan, np.vstack((tri, np.ones((1, tri.shape[1]))))


def one_pass(P, dv, plan, tri, n_views, iterations, device_tracks):
    vp, tp = Holder(), Holder()
    vp.view_list, tp.tri_pts = [], np.zeros((4, 0))
    kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
    bp = P.HipBaProcessor(vp, kt, None, tp, None, iteration=iterations, damping_factor=5)
    bp.ba_verbose = False
    bp.ba_device_tracks = device_tracks
    try:
        n_known = 0
        for c in range(n_views):
            xy = dv.pix[c].astype(np.float32).astype(np.float64)
            view = View(dv.rots[c].copy(), dv.locs[c].reshape(3, 1).copy(), dv.intrinsic.copy(), dv.key_pts(c), dv.sift[c], xy)
            kt.add_new_view(view, vp.view_list)
            vp.view_list.append(view)
            if c == 0:
                continue
            n_new, writes = plan[c]
            for v, (keys, ids) in enumerate(writes):
                kt.track_list[v].update_usage(keys[np.newaxis, :], ids[np.newaxis, :])
            n_known += n_new
            tp.tri_pts = tri[:, :n_known].copy()
            before = (bp.ba_upload_bytes, kt.kt_upload_bytes, kt.kt_download_bytes)
            t0 = time.perf_counter()
            bp.execute_bundle_adjustment()
            ms = (time.perf_counter() - t0) * 1e3
        after = (bp.ba_upload_bytes, kt.kt_upload_bytes, kt.kt_download_bytes)
        scene = bp._hip_scene
        return ms, {"action": bp.ba_last_action, "n_pts": n_known, "n_obs": scene.prob.n_obs,
                    "ba_upload_bytes": after[0] - before[0], "kt_upload_bytes": after[1] - before[1],
                    "kt_download_bytes": after[2] - before[2]}
    finally:
        bp.ba_release()
        kt.kt_release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="2000,5000,8000")
    ap.add_argument("--views", default="3,10")
    ap.add_argument("--iterations", default="3,1")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ba_sync.py needs an MI355X")
    sfm = importlib.import_module("structure-from-motion_amd")
    sfm.native.init(0)
    P = sfm.processors
    for iterations in [int(x) for x in a.iterations.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            for n_views in [int(x) for x in a.views.split(",")]:
                dv, plan, tri = workload(sfm, n, n_views, seed=n + n_views)
                times, facts = {"on": [], "off": []}, {}
                for i in range(a.warmup + a.reps):                  # alternate the two settings
                    for name in ("on", "off"):
                        ms, facts[name] = one_pass(P, dv, plan, tri, n_views, iterations, name == "on")
                        if i >= a.warmup:
                            times[name].append(ms)
                assert facts["on"]["n_obs"] == facts["off"]["n_obs"]
                row = {"keys": int(dv.pix[-1].shape[0]), "views": n_views, "iterations": iterations, "reps": a.reps,
                       "on_ms": stats(times["on"]), "off_ms": stats(times["off"]), "on": facts["on"], "off": facts["off"]}
                row["off_over_on_median"] = round(row["off_ms"]["median"] / row["on_ms"]["median"], 3)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
