"""Wall time per blocking sift_detect call at 640 x 480 and 1280 x 960 (frames of tests/golden, the larger one upsampled by
pixel repetition), and the NumPy stand-in on the host for comparison.  Prints one JSON line.

    python tools/bench_sift.py [--reps 20] [--no-cpu]

Kernel breakdown: run under ``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_sift.py --no-cpu``."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sift needs an MI355X")
    native = importlib.import_module("structure-from-motion_amd").native
    native.init(0)
    img = np.load(os.path.join(REPO, "tests", "golden", "g13_upenn_1.npz"))["image"]
    out = {}
    for name, im in (("640x480", img), ("1280x960", np.kron(img, np.ones((2, 2), np.uint8)))):
        for _ in range(3):
            kp = native.sift_detect(im)
        # sift_detect blocks until its results are on the host (it synchronises its stream twice on the way), so the
        # host clock around it is the wall time of a call: kernels, copies and the host sort.  Kernel time alone comes
        # from the rocprofv3 trace.
        t0 = time.perf_counter()
        for _ in range(a.reps):
            native.sift_detect(im)
        out[name] = {"ms_per_call_wall": (time.perf_counter() - t0) * 1e3 / a.reps, "keypoints": int(len(kp["x"]))}
        if not a.no_cpu:
            import _sift_numpy as S
            t0 = time.perf_counter()
            S.detect(im)
            out[name]["ms_numpy_stand_in"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"sift": out}))


if __name__ == "__main__":
    main()
