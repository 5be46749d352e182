#!/usr/bin/env python3
"""Descriptor matching throughput: one new view of N SIFT keys against R resident views (exact L2, knnMatch k = 2).

Run on an MI355X:  python tools/bench_match.py [--reps 20] [--cpu]
Per (N, R): device time of the matching call (hip events around warmed, synchronised sfm_match_dev calls on torch's
stream), GFLOP/s of its dot-product part (2 Q T D) and the share of the dense BF16 MFMA peak (16 x 157.3 TF), and,
with --cpu, the NumPy stand-in (tests/_bfmatcher_numpy.py) on the host for the same work.  Kernel-level times come
from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.  Prints one JSON line per configuration."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
PEAK_BF16 = 16 * 157.3e12


def sift_like(rng, n):
    d = rng.gamma(0.6, 1.0, (n, 128))
    return np.clip(np.rint(d / np.linalg.norm(d, axis=1, keepdims=True) * 512.0), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu", action="store_true", help="also time the NumPy stand-in (slow)")
    ap.add_argument("--sizes", default="2000,5000,8000")
    ap.add_argument("--refs", default="1,9")
    a = ap.parse_args()
    import torch
    sfm = importlib.import_module("structure-from-motion_amd")
    nat = sfm.native
    nat.init(0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    for n in [int(x) for x in a.sizes.split(",")]:
        for r in [int(x) for x in a.refs.split(",")]:
            q = nat.DescriptorSet(nat.MATCH_L2, sift_like(rng, n))
            refs = [nat.DescriptorSet(nat.MATCH_L2, sift_like(rng, n)) for _ in range(r)]
            outs = [torch.empty((r, n), dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.int32, torch.float32, torch.uint8)]
            ptrs = [o.data_ptr() for o in outs]
            for _ in range(3):
                nat.match_dev(q, refs, nat.MATCH_KNN2, *ptrs, stream=stream)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                nat.match_dev(q, refs, nat.MATCH_KNN2, *ptrs, stream=stream)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.reps
            flop = 2.0 * n * n * r * 128
            t0 = time.perf_counter()
            nat.match(q, refs, nat.MATCH_KNN2)
            host_us = (time.perf_counter() - t0) * 1e6
            rec = dict(N=n, R=r, device_us=round(us, 1), gflops=round(flop / us * 1e-3, 1),
                       share_bf16_peak=round(flop / (us * 1e-6) / PEAK_BF16, 4), blocking_call_us=round(host_us, 1))
            if a.cpu:
                import _bfmatcher_numpy as bfm
                t0 = time.perf_counter()
                for ref in range(r):
                    bfm.neighbours(bfm.NORM_L2, sift_like(np.random.default_rng(1), n), sift_like(np.random.default_rng(2), n), k=2)
                rec["numpy_standin_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            print(json.dumps(rec), flush=True)
            q.close()
            for s in refs:
                s.close()


if __name__ == "__main__":
    main()
