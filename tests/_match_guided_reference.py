"""Guided matching in NumPy float64 (test code only): the rule of include/sfm_hip.h, block 'guided matching', on top of
the distances of tests/_bfmatcher_numpy.py.

The library evaluates the gate with fused multiply-adds in a fixed order; NumPy has none, so a pair whose error sits within
rounding of the threshold may be decided differently.  Every gate is therefore evaluated at ``max_err2``,
``max_err2 (1 - 1e-6)`` and ``max_err2 (1 + 1e-6)``; a (reference, query) row is SETTLED iff the three runs agree on the best,
the second, the mutual flag and the count.  The relative rounding error of either test is some 1e-15 for the coordinates used
here (hundreds of pixels, models of unit order), nine orders below the bracket.  The GPU tests compare settled rows only; the
host tests assert that every row of every case IS settled (a seed is changed, never the condition).

The scenes: two pinhole views (640 x 480, focal length 500) of a general or a planar scene, the reference view LEFT and the
query view RIGHT, 0.5 px of noise on every key, descriptors of integer rows like scenes.make_descriptor_views (a base row of
norm 512 per 3-D point, +-2 of noise per key), keys without a partner at random places with random rows, both views
shuffled.  The true F and H come from the cameras."""
import functools

import numpy as np

import _bfmatcher_numpy as bf

NONE, FUNDAMENTAL, HOMOGRAPHY = 0, 1, 2
BRACKET = 1e-6
RATIO = 0.7
OUTPUTS = ("best_idx", "best_dist", "second_idx", "second_dist", "mutual", "n_admitted")
K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])
WIDTH, HEIGHT = 640.0, 480.0

NQ = (1, 127, 128, 129, 257)                      # around the 128-row tile
NT = (1, 15, 16, 17, 1023, 1024, 1025, 2049)      # around the 16-column tile and the 1 024-column chunk
DIM_CASES = [(nq, nt, dim) for dim in (32, 200) for nq in (127, 129) for nt in (17, 1025)]


def adjugate(H):
    """adj H by cofactors (the header's formula without the fused rounding)."""
    h = np.asarray(H, dtype=np.float64).reshape(9)
    return np.array([h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                     h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                     h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]).reshape(3, 3)


def sampson2(F, ref_xy, que_xy):
    """(Q, T) squared Sampson distances, the reference key left and the query key right."""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    lx, ly = ref_xy[:, 0][None, :], ref_xy[:, 1][None, :]
    rx, ry = que_xy[:, 0][:, None], que_xy[:, 1][:, None]
    a = [F[i, 0] * lx + F[i, 1] * ly + F[i, 2] for i in range(3)]
    b = [F[0, i] * rx + F[1, i] * ry + F[2, i] for i in range(2)]
    e = rx * a[0] + ry * a[1] + a[2]
    with np.errstate(all="ignore"):
        return (e * e) / (a[0] * a[0] + a[1] * a[1] + b[0] * b[0] + b[1] * b[1])


def _half(A, px, py, qx, qy, max_err2):
    u = A[0, 0] * px + A[0, 1] * py + A[0, 2]
    v = A[1, 0] * px + A[1, 1] * py + A[1, 2]
    w = A[2, 0] * px + A[2, 1] * py + A[2, 2]
    eu, ev = u - qx * w, v - qy * w
    with np.errstate(all="ignore"):
        lhs = eu * eu + ev * ev
        return np.isfinite(lhs) & (w * w > 0.0) & (lhs <= max_err2 * (w * w))


def admitted(kind, model, ref_xy, que_xy, max_err2):
    """(Q, T) bool: the pairs the gate admits."""
    ref_xy, que_xy = np.asarray(ref_xy, dtype=np.float64), np.asarray(que_xy, dtype=np.float64)
    if kind == NONE:
        return np.ones((que_xy.shape[0], ref_xy.shape[0]), dtype=bool)
    if kind == FUNDAMENTAL:
        d2 = sampson2(model, ref_xy, que_xy)
        with np.errstate(all="ignore"):
            return np.isfinite(d2) & (d2 <= max_err2)
    H = np.asarray(model, dtype=np.float64).reshape(3, 3)
    lx, ly = ref_xy[:, 0][None, :], ref_xy[:, 1][None, :]
    rx, ry = que_xy[:, 0][:, None], que_xy[:, 1][:, None]
    return _half(H, lx, ly, rx, ry, max_err2) & _half(adjugate(H), rx, ry, lx, ly, max_err2)


_MAX = np.iinfo(np.uint64).max


def select(dist, ok):
    """The six outputs of one reference from the (Q, T) float32 distances and the admission mask."""
    nq, nt = dist.shape
    bits = dist.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)
    keys = np.where(ok, bits | np.arange(nt, dtype=np.uint64)[None, :], _MAX)
    out = {"best_idx": np.full(nq, -1, dtype=np.int32), "second_idx": np.full(nq, -1, dtype=np.int32),
           "best_dist": np.full(nq, np.inf, dtype=np.float32), "second_dist": np.full(nq, np.inf, dtype=np.float32)}
    rows = np.arange(nq)
    for name in ("best", "second"):
        m = keys.argmin(1)
        have = keys[rows, m] != _MAX
        out[name + "_idx"][have] = m[have]
        out[name + "_dist"][have] = dist[rows, m][have]
        keys[rows, m] = _MAX
    ckeys = np.where(ok, bits | np.arange(nq, dtype=np.uint64)[:, None], _MAX)
    cbest = ckeys.argmin(0)
    cbest = np.where(ckeys[cbest, np.arange(nt)] != _MAX, cbest, -1)
    b = out["best_idx"]
    out["mutual"] = (b >= 0) & (cbest[np.maximum(b, 0)] == rows)
    out["n_admitted"] = ok.sum(1).astype(np.int32)
    return out


def guided(norm, query, train, que_xy, ref_xy, kind, model, max_err2, dist=None):
    dist = bf.distances(norm, query, train) if dist is None else dist
    return select(dist, admitted(kind, model, ref_xy, que_xy, max_err2))


def reference(norm, query, train, que_xy, ref_xy, kind, model, max_err2, dist=None):
    """The outputs at ``max_err2`` and ``settled`` (Q,) bool."""
    dist = bf.distances(norm, query, train) if dist is None else dist
    runs = [guided(norm, query, train, que_xy, ref_xy, kind, model, max_err2 * f, dist) for f in (1.0, 1.0 - BRACKET, 1.0 + BRACKET)]
    settled = np.ones(dist.shape[0], dtype=bool)
    for other in runs[1:]:
        for name in OUTPUTS:
            a, b = runs[0][name], other[name]
            settled &= (a.view(np.uint32) == b.view(np.uint32)) if a.dtype == np.float32 else (a == b)
    out = dict(runs[0])
    out["settled"] = settled
    return out


def filter_loop(best_idx, best_dist, second_dist, mutual, ratio=RATIO):
    """matching.filter_guided as a loop over Python floats."""
    q, t = [], []
    for i in range(len(best_idx)):
        if best_idx[i] < 0 or not mutual[i]:
            continue
        d0, d1 = float(best_dist[i]), float(second_dist[i])
        if d1 == float("inf") or d0 < ratio * d1:
            q.append(i)
            t.append(int(best_idx[i]))
    return np.array(q, dtype=np.int64), np.array(t, dtype=np.int64)


def pairs_of(out, ratio=RATIO):
    """(r_idx, q_idx) sorted by reference key: what guided_pairs returns."""
    q, t = filter_loop(out["best_idx"], out["best_dist"], out["second_dist"], out["mutual"], ratio)
    order = np.argsort(t, kind="stable")
    return t[order], q[order]


# ---- scenes -------------------------------------------------------------------------------------------------------------
def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


R1 = _rot(0.02, -0.06, 0.03)
T1 = np.array([0.6, 0.05, 0.1])
PLANE_N, PLANE_D = np.array([-0.2, -0.1, 1.0]), 6.0          # n . X = d: Z = 6 + 0.2 X + 0.1 Y


def true_fundamental():
    tx = np.array([[0, -T1[2], T1[1]], [T1[2], 0, -T1[0]], [-T1[1], T1[0], 0]])
    F = np.linalg.inv(K).T @ tx @ R1 @ np.linalg.inv(K)
    return F / np.linalg.norm(F)


def true_homography():
    H = K @ (R1 + np.outer(T1, PLANE_N) / PLANE_D) @ np.linalg.inv(K)
    return H / np.linalg.norm(H)


def _rows(rng, n, dim):
    base = rng.gamma(0.6, 1.0, (n, dim))
    return np.clip(np.rint(base / np.maximum(np.linalg.norm(base, axis=1, keepdims=True), 1e-9) * 512.0), 0, 255)


class Scene:
    pass


def make_scene(nq, nt, dim=128, planar=False, seed=0, metric="l2", float_rows=False, noise_px=0.5, shuffle=True, n_shared=None):
    """A query view of nq keys and a reference view of nt keys sharing n_shared (default: min(nq, nt)) 3-D points."""
    rng = np.random.default_rng([seed, nq, nt, dim, int(planar)])
    n = min(nq, nt) if n_shared is None else n_shared
    X = np.vstack((rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(4.5, 8.0, n)))
    if planar:
        X[2] = PLANE_D + 0.2 * X[0] + 0.1 * X[1]
    p0 = K @ X
    p1 = K @ (R1 @ X + T1[:, None])
    sc = Scene()
    xy = []
    for p, total in ((p0, nt), (p1, nq)):
        shared = (p[0:2] / p[2]).T + rng.normal(0.0, noise_px, (n, 2))
        extra = np.column_stack((rng.uniform(0, WIDTH, total - n), rng.uniform(0, HEIGHT, total - n)))
        xy.append(np.vstack((shared, extra)))
    if metric == "hamming":
        base = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        rows = []
        for total in (nt, nq):
            flip = np.zeros((n, dim), dtype=np.uint8)
            flip[np.arange(n), rng.integers(0, dim, n)] = 1 << rng.integers(0, 8, n).astype(np.uint8)
            rows.append(np.vstack((base ^ flip, rng.integers(0, 256, (total - n, dim), dtype=np.uint8))))
    else:
        base = _rows(rng, n, dim)
        rows = [np.vstack((np.clip(base + rng.integers(-2, 3, (n, dim)), 0, 255), _rows(rng, total - n, dim))).astype(np.float32)
                for total in (nt, nq)]
        if float_rows:
            # half-integers: not integer-valued, so the general-float path; every (a - b)^2 is a multiple of 1/4 and a row
            # sum stays below 2^24 / 4 for dim <= 64, so the fp32 sum is exact in any order and the distance has one value
            assert dim <= 64
            rows = [(r + 0.5 * (rng.random(r.shape) < 0.5)).astype(np.float32) for r in rows]
    sc.float_rows = bool(float_rows)
    perm_t = rng.permutation(nt) if shuffle else np.arange(nt)
    perm_q = rng.permutation(nq) if shuffle else np.arange(nq)
    sc.ref_xy, sc.ref_desc = np.ascontiguousarray(xy[0][perm_t]), np.ascontiguousarray(rows[0][perm_t])
    sc.que_xy, sc.que_desc = np.ascontiguousarray(xy[1][perm_q]), np.ascontiguousarray(rows[1][perm_q])
    sc.true_ref, sc.true_que = np.argsort(perm_t)[:n], np.argsort(perm_q)[:n]      # key of shared point k in either view
    sc.norm = bf.NORM_HAMMING if metric == "hamming" else bf.NORM_L2
    sc.F, sc.H = true_fundamental(), true_homography()
    sc.planar = planar
    return sc


def model_of(sc, kind):
    return None if kind == NONE else (sc.F if kind == FUNDAMENTAL else sc.H)


def scene_distances(sc, ref_desc=None):
    """(Q, T) float32 distances of the contract; half-integer rows are doubled to integers (float32(sqrt(4 s)) / 2 is
    float32(sqrt(s)): a power of two commutes with the rounding)."""
    ref_desc = sc.ref_desc if ref_desc is None else ref_desc
    if getattr(sc, "float_rows", False):
        return bf.distances(sc.norm, 2.0 * sc.que_desc.astype(np.float64), 2.0 * ref_desc.astype(np.float64)) * np.float32(0.5)
    return bf.distances(sc.norm, sc.que_desc, ref_desc)


@functools.lru_cache(maxsize=None)
def case(nq, nt, dim=128, kind=FUNDAMENTAL, seed=0, metric="l2", float_rows=False, max_err2=4.0):
    """(scene, reference outputs) of one parity case, computed once per process; the homography gate gets the planar scene."""
    sc = make_scene(nq, nt, dim, planar=kind == HOMOGRAPHY, seed=seed, metric=metric, float_rows=float_rows)
    ref = reference(sc.norm, sc.que_desc, sc.ref_desc, sc.que_xy, sc.ref_xy, kind, model_of(sc, kind), max_err2, scene_distances(sc))
    return sc, ref


PARITY_CASES = [(nq, nt, 128) for nq in NQ for nt in NT] + DIM_CASES
MID = (129, 1025)                                            # Hamming width 32 and the general-float path (dim 32)


@functools.lru_cache(maxsize=None)
def batch_scene(float_mixed=False, seed=3):
    """One query view against four reference views for the batch-independence test: gates none, fundamental, homography,
    fundamental, over 40, 1 030, 300 and 17 keys.  Every reference view is the reference view of its own make_scene with the
    query view replaced by the common one (the geometry is the same: one pair of cameras).  With ``float_mixed`` the rows
    have dim 32 and the second reference set is half-integer (the call takes the general-float path as a whole)."""
    dim = 32 if float_mixed else 128
    sizes, kinds = (40, 1030, 300, 17), (NONE, FUNDAMENTAL, HOMOGRAPHY, FUNDAMENTAL)
    que = make_scene(200, 1030, dim, planar=False, seed=seed)
    sc = Scene()
    sc.que_xy, sc.que_desc, sc.norm, sc.kinds = que.que_xy, que.que_desc, que.norm, kinds
    sc.float_rows = False
    sc.refs = []
    for r, (nt, kind) in enumerate(zip(sizes, kinds)):
        one = que if nt == 1030 else make_scene(200, nt, dim, planar=kind == HOMOGRAPHY, seed=seed + 1 + r)
        desc = one.ref_desc
        if float_mixed and r == 1:
            desc = (desc + 0.5 * (np.arange(desc.size).reshape(desc.shape) % 3 == 0)).astype(np.float32)
        sc.refs.append((one.ref_xy, desc, kind, model_of(one, kind)))
    sc.float_rows = float_mixed
    sc.out = [reference(sc.norm, sc.que_desc, desc, sc.que_xy, xy, kind, model, 4.0, scene_distances(sc, desc))
              for xy, desc, kind, model in sc.refs]
    return sc


def ties_scene():
    """Canonical ties under the identity homography at 2 px (every decision is exact: the errors are 0.25, 1 and 100 px^2):
    query 0 has the train keys 0 and 1 with one and the same row within reach, query 1 the train keys 2 and 3; eight more
    train keys are out of reach.  ``ref_xy_lower_out`` moves the keys 0 and 2 out of the gate."""
    rng = np.random.default_rng(42)
    t = Scene()
    t.norm, t.float_rows = bf.NORM_L2, False
    rows = _rows(rng, 12, 128)
    t.que_desc = np.clip(rows[[0, 2]] + rng.integers(-2, 3, (2, 128)), 0, 255).astype(np.float32)
    t.ref_desc = np.vstack((rows[[0, 0, 2, 2]], rows[4:12])).astype(np.float32)
    t.que_xy = np.array([[100.0, 100.0], [300.0, 300.0]])
    far = np.column_stack((np.full(8, 500.0), 50.0 + 10.0 * np.arange(8)))
    t.ref_xy = np.vstack(([[100.5, 100.0], [101.0, 100.0], [300.0, 301.0], [301.0, 300.0]], far))
    t.ref_xy_lower_out = t.ref_xy.copy()
    t.ref_xy_lower_out[0] = [110.0, 100.0]
    t.ref_xy_lower_out[2] = [300.0, 310.0]
    t.want_both_best, t.want_both_second = [0, 2], [1, 3]
    t.want_moved_best, t.want_moved_count = [1, 3], [1, 1]
    return t


# ---- the scene that shows the point: twins ----------------------------------------------------------------------------
TWIN_MIN_PX = 20.0


@functools.lru_cache(maxsize=None)
def twin_scene(planar=False, seed=0, n_pts=240, n_extra=60, share=3):
    """make_scene (unshuffled, so key k of either view is point k for k < n_pts) in which every `share`-th true match has
    a TWIN in the reference view: a key whose row differs from the true reference row by +-1 per element, at least 20 px from
    where the gate admits (the query key's epipolar line; H^-1 of the query key for the plane).  Key 0 of the query view is a
    key without a partner (generate_matched_pairs never pairs it: quirk Q3)."""
    rng = np.random.default_rng([seed, 77, int(planar)])
    sc = make_scene(n_pts + n_extra, n_pts + n_extra, 128, planar=planar, seed=seed, shuffle=False, n_shared=n_pts)
    # swap query key 0 (a shared point) with the last query key (an extra): point 0 is then the last query key
    for arr in (sc.que_xy, sc.que_desc):
        arr[[0, -1]] = arr[[-1, 0]]
    sc.true_ref = np.arange(n_pts)
    sc.true_que = np.concatenate(([n_pts + n_extra - 1], np.arange(1, n_pts)))
    sc.twinned = np.arange(1, n_pts, share)                    # shared points with a twin
    twin_xy, twin_desc = [], []
    for k in sc.twinned:
        q = sc.que_xy[sc.true_que[k]]
        while True:
            cand = np.array([rng.uniform(0, WIDTH), rng.uniform(0, HEIGHT)])
            if planar:
                back = adjugate(sc.H) @ np.array([q[0], q[1], 1.0])
                far = np.hypot(*(cand - back[0:2] / back[2])) >= TWIN_MIN_PX
            else:
                line = sc.F.T @ np.array([q[0], q[1], 1.0])
                far = abs(line @ np.array([cand[0], cand[1], 1.0])) / np.hypot(line[0], line[1]) >= TWIN_MIN_PX
            if far:
                break
        twin_xy.append(cand)
        twin_desc.append(np.clip(sc.ref_desc[sc.true_ref[k]] + rng.integers(-1, 2, 128), 0, 255))
    sc.twin_key = np.arange(sc.ref_xy.shape[0], sc.ref_xy.shape[0] + len(sc.twinned))
    sc.ref_xy = np.ascontiguousarray(np.vstack((sc.ref_xy, np.array(twin_xy))))
    sc.ref_desc = np.ascontiguousarray(np.vstack((sc.ref_desc, np.array(twin_desc)))).astype(np.float32)
    return sc


def plain_knn_pairs(sc, ratio=RATIO):
    """(train, query) pairs that knnMatch k = 2 and the ratio test keep."""
    idx, dist, _ = bf.neighbours(sc.norm, sc.que_desc, sc.ref_desc, k=2)
    keep = dist[:, 0].astype(np.float64) < ratio * dist[:, 1].astype(np.float64)
    return {(int(idx[i, 0]), int(i)) for i in np.flatnonzero(keep)}
