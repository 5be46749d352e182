#!/usr/bin/env python3
"""Guided matching against the plain call on the same sets: one query view of N SIFT-like keys against R resident views
(exact L2, best two and the mutual flag), the key coordinates on the device.

Run on an MI355X:  python tools/bench_match_guided.py [--cases 2000x1,8000x9] [--reps 20] [--rounds 5] [--out FILE]
Per case four calls are timed alternately, `rounds` times over (hip events around `reps` warmed calls on one stream):
  plain    sfm_match_dev in SFM_MATCH_MUTUAL
  none     sfm_match_guided_dev with SFM_GUIDE_NONE on every reference (it launches the ungated kernels)
  F        ... with the true fundamental matrix at 2 px (general scene)
  H        ... with the true homography at 2 px (planar scene)
The scenes are those of tests/_match_guided_reference.py (two views, 640 x 480, 0.5 px of key noise); every reference view
is the scene's reference view with its keys shuffled again.  Prints one JSON line per case: the median and the range of the
milliseconds per call of every kind, the ratios of the medians to the plain call, the admitted share of the F and H gates.
With --trace KIND only that kind is run (`--reps` calls of it), for a ``rocprofv3 --kernel-trace --stats`` run of this script."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2000x1,8000x9")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", default="", help="run only this kind (plain, none, F or H)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import _match_guided_reference as mg
    sfm = importlib.import_module("structure-from-motion_amd")
    nat = sfm.native
    nat.init(0)
    stream = torch.cuda.Stream()
    lines = []
    for case in a.cases.split(","):
        n, r = (int(x) for x in case.split("x"))
        rng = np.random.default_rng(n + r)
        work = {}
        for name, planar in (("F", False), ("H", True)):
            sc = mg.make_scene(n, n, 128, planar=planar, seed=1)
            perms = [rng.permutation(n) for _ in range(r)]
            work[name] = dict(sc=sc, q=nat.DescriptorSet(nat.MATCH_L2, sc.que_desc.astype(np.uint8)),
                              refs=[nat.DescriptorSet(nat.MATCH_L2, sc.ref_desc[p].astype(np.uint8)) for p in perms],
                              xy=[np.ascontiguousarray(sc.ref_xy[p].T) for p in perms])
        with torch.cuda.stream(stream):
            dt = (torch.int32, torch.float32, torch.int32, torch.float32, torch.uint8, torch.int32)
            outs = [torch.empty((r, n), dtype=t, device="cuda") for t in dt]
            ptrs = [o.data_ptr() for o in outs]
            for w in work.values():
                w["d_q"] = torch.from_numpy(np.ascontiguousarray(w["sc"].que_xy.T)).cuda()
                w["d_r"] = [torch.from_numpy(x).cuda() for x in w["xy"]]
                w["qxy"] = (w["d_q"][0].data_ptr(), w["d_q"][1].data_ptr())
                w["rxy"] = [(t[0].data_ptr(), t[1].data_ptr()) for t in w["d_r"]]
            f, h = work["F"], work["H"]
            calls = {
                "plain": lambda: nat.match_dev(f["q"], f["refs"], nat.MATCH_MUTUAL, *ptrs[:5], stream=stream.cuda_stream),
                "none": lambda: nat.match_guided_dev(f["q"], f["qxy"], f["refs"], f["rxy"], [nat.GUIDE_NONE] * r, [None] * r, 4.0,
                                                     *ptrs, stream=stream.cuda_stream),
                "F": lambda: nat.match_guided_dev(f["q"], f["qxy"], f["refs"], f["rxy"], [nat.GUIDE_FUNDAMENTAL] * r, [f["sc"].F] * r, 4.0,
                                                  *ptrs, stream=stream.cuda_stream),
                "H": lambda: nat.match_guided_dev(h["q"], h["qxy"], h["refs"], h["rxy"], [nat.GUIDE_HOMOGRAPHY] * r, [h["sc"].H] * r, 4.0,
                                                  *ptrs, stream=stream.cuda_stream),
            }
            if a.trace:
                for _ in range(a.reps):
                    calls[a.trace]()
                stream.synchronize()
                continue
            share = {}
            for name in ("F", "H"):
                calls[name]()
                stream.synchronize()
                share[name] = float(outs[5].sum().item()) / (float(n) * n * r)
            ms = {name: [] for name in calls}
            for name in calls:
                for _ in range(3):
                    calls[name]()
            stream.synchronize()
            for _ in range(a.rounds):
                for name in calls:                               # the kinds alternate inside a round
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.reps):
                        calls[name]()
                    e1.record(stream)
                    stream.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / a.reps)
        med = {name: float(np.median(v)) for name, v in ms.items()}
        rec = dict(N=n, R=r, reps=a.reps, rounds=a.rounds,
                   ms={name: dict(median=round(med[name], 4), min=round(min(v), 4), max=round(max(v), 4)) for name, v in ms.items()},
                   ratio_to_plain={name: round(med[name] / med["plain"], 3) for name in ms},
                   admitted_share={k: round(v, 6) for k, v in share.items()})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        for w in work.values():
            w["q"].close()
            for s in w["refs"]:
                s.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
