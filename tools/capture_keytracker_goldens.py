#!/usr/bin/env python3
"""Capture KeyTracker goldens from the REAL reference (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/capture_keytracker_goldens.py [REFERENCE_DIR]

Imports the reference's ``key_tracker`` (read-only; never copied) with a ``cv2`` placeholder whose ``BFMatcher`` is
the NumPy stand-in of the matching contract (tests/_bfmatcher_numpy.py), drives the real ``KeyTracker.add_new_view``
over the seeded views of ``scenes.make_descriptor_views`` in five configurations and writes
``tests/golden/g12_keytracker_<case>.npz`` (inputs, every track table, a digest of ``random.getstate()`` after the
run) plus ``tests/golden/g12_keytracker_api.json`` (KeyTracker / KeyTrack method parameters and the call of
``__extend_list`` in ``add_new_view``).  ``g11_reference_api.json`` is not touched.
"""
import hashlib
import importlib
import inspect
import json
import os
import random
import sys
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")

warnings.filterwarnings("ignore", category=DeprecationWarning)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import _bfmatcher_numpy as bfm                               # noqa: E402

cv2 = types.ModuleType("cv2")
cv2.NORM_L2, cv2.NORM_HAMMING, cv2.BFMatcher = bfm.NORM_L2, bfm.NORM_HAMMING, bfm.BFMatcher
sys.modules["cv2"] = cv2
import utils as ref_utils                                    # noqa: E402
import key_tracker as ref_kt                                 # noqa: E402

sfm = importlib.import_module("structure-from-motion_amd")

# name -> (key_type, is_cross_check, is_knn_match, is_fund_inlier, scene seed)
CASES = {
    "sift_knn": ("sift", False, True, False, 11),
    "sift_knn_fund": ("sift", False, True, True, 12),
    "sift_cross": ("sift", True, True, False, 13),
    "sift_match": ("sift", False, False, False, 14),
    "orb_knn": ("orb", False, True, False, 15),
}
N_VIEWS = 5
RANSAC = dict(inlier_threshold=1e-2, subset_confidence=0.99, sample_confidence=0.75, sample_num=8, iteration=300)


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def rng_digest():
    return hashlib.sha256(repr(random.getstate()).encode()).hexdigest()


def capture(name, key_type, cross, knn, fund, seed):
    dv = sfm.scenes.make_descriptor_views(n_views=N_VIEWS, seed=seed)
    desc = dv.sift if key_type == "sift" else dv.orb
    views = [View(dv.key_pts(v), desc[v]) for v in range(N_VIEWS)]
    cfg = ref_utils.RansacConfig(**RANSAC)                   # seeds Python's RNG with -1 (utils.py)
    kt = ref_kt.KeyTracker(key_type, cross, knn, fund, cfg)
    for v in range(N_VIEWS):
        kt.add_new_view(views[v], views[:v], knn, fund, cfg)
    out = dict(key_type=np.array(key_type), flags=np.array([cross, knn, fund], dtype=bool), n_views=np.array(N_VIEWS),
               ransac=np.array([RANSAC[k] for k in ("inlier_threshold", "subset_confidence", "sample_confidence",
                                                     "sample_num", "iteration")], dtype=np.float64),
               rng_digest=np.array(rng_digest()))
    for v in range(N_VIEWS):
        out["pix_%d" % v] = dv.pix[v]
        out["desc_%d" % v] = desc[v]
        out["table_%d" % v] = np.asarray(kt.track_list[v].table, dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "g12_keytracker_%s.npz" % name), **out)
    n_pairs = sum(int((kt.track_list[v].table >= 0).sum()) for v in range(N_VIEWS))
    print("g12_keytracker_%s: %d table entries" % (name, n_pairs))


def api():
    rec = {}
    for cls in (ref_kt.KeyTracker, ref_kt.KeyTrack):
        rec[cls.__name__] = {n: list(inspect.signature(f).parameters) for n, f in vars(cls).items()
                             if inspect.isfunction(f)}
    src = inspect.getsource(ref_kt.KeyTracker.add_new_view)
    rec["add_new_view_calls"] = [ln.strip() for ln in src.splitlines() if "__extend_list(" in ln]
    rec["mangled"] = [n for n in dir(ref_kt.KeyTracker) if n.startswith("_KeyTracker__")]
    with open(os.path.join(OUT, "g12_keytracker_api.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    for case, args in CASES.items():
        capture(case, *args)
    api()
