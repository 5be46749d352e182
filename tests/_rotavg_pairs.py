"""A small view graph whose edges are pairs of tests/_twoview_pose_reference.py: every edge is one set of matches of a family
with its planted relative rotation, so the true absolute rotations follow by chaining the planted ones.

The pair poses of that module's scenes are held to ``max |R - R0| < 0.05`` per entry (tests/test_gpu_twoview_pose.py).  For a
rotation error of angle a, ``|R - R0|_F = 2 sqrt(2) sin(a / 2)`` and ``|.|_F <= 3 max |.|``: a pair inside that bound is within
``PAIR_DEG = 2 asin(0.15 / (2 sqrt 2))`` = 6.08 degrees of its planted rotation.  Angles add along a chain and a geodesic ball
of that size is convex, so a view at depth d of the graph is within ``d PAIR_DEG`` of its true rotation whichever of its
parallel pairs the averaging follows or blends; two parallel pairs may disagree by ``2 PAIR_DEG``, which is the residual
angle the averaging has to admit."""
import math
from types import SimpleNamespace

import numpy as np

import _twoview_pose_reference as tp

PAIR_ENTRY = 0.05
PAIR_DEG = math.degrees(2.0 * math.asin(3.0 * PAIR_ENTRY / (2.0 * math.sqrt(2.0))))
# (ref, que, family, seed): parallel pairs between 0 and 1 and between 1 and 2, then one pair on to view 3
SPEC = ((0, 1, "general", 11), (0, 1, "general", 13), (1, 2, "plane", 12), (1, 2, "plane", 14), (2, 3, "general", 11))


def angle_deg(A, B):
    c = 0.5 * (np.trace(np.asarray(A).T @ np.asarray(B)) - 1.0)
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


def pose_graph(n=300, displaced_share=0.1):
    K = tp.K_LEFT
    sets, planted = [], []
    for ref, que, fam, seed in SPEC:
        l, r, _displaced, _model, _kind = tp.family_part(fam, n, seed, displaced_share, Kr=K)
        sets.append([l, r])
        planted.append(tp.planted(fam)[0])
    truth = [np.identity(3)]
    truth.append(planted[0] @ truth[0])
    truth.append(planted[2] @ truth[1])
    truth.append(planted[4] @ truth[2])
    return SimpleNamespace(K=K, sets=sets, pairs=[(s[0], s[1]) for s in SPEC], planted=planted, n_views=4, truth=truth,
                           depth=(0, 1, 2, 3), max_angle_deg=2.0 * PAIR_DEG, pair_deg=PAIR_DEG)
