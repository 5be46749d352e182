"""Float64 NumPy references for triangulation over ragged tracks (sfm_tri_tracks), and the shared ragged test scene.

The nonlinear reference is the oracle's ``nonlinear_triangulate`` called point by point with that point's own
projections and keys; the linear one is ``np.linalg.svd`` of the point's (2k x 4) DLT matrix, rows per observation
u then v (as tests/test_gpu_linear_and_incremental.py builds it for the rectangular kernel)."""
import importlib
from types import SimpleNamespace

import numpy as np

# every length is G - 1, G, G + 1 or 2 G + 1 for some group width G in {1, 4, 8, 16, 32, 64}: where the dealing of
# observations to lanes, the register cache (2 and 4 observations per lane) and the re-reading fallback change over
TRACK_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130)
GROUPS = (1, 4, 8, 16, 32, 64)


def _oracle():
    return importlib.import_module("sfm_oracle")


def track_cost(pt_ptr, cam_idx, uv, projs, x):
    """sum |f - b|^2 over each point's track at x (4, n): (n,)."""
    oracle = _oracle()
    n = pt_ptr.shape[0] - 1
    cost = np.zeros(n)
    for p in range(n):
        obs = range(pt_ptr[p], pt_ptr[p + 1])
        if len(obs):
            err = oracle.reproj_error(x[:, p], [projs[cam_idx[o]] for o in obs], [(uv[0, o], uv[1, o]) for o in obs])
            cost[p] = float(err @ err)
    return cost


def refine_tracks_reference(pt_ptr, cam_idx, uv, projs, x_init, lam, iters):
    """(X (4, n), cost (2, n)): ``oracle.nonlinear_triangulate`` per point over the point's own views; empty tracks keep
    their input."""
    oracle = _oracle()
    pt_ptr = np.asarray(pt_ptr); cam_idx = np.asarray(cam_idx)
    uv = np.asarray(uv, dtype=np.float64); projs = np.asarray(projs, dtype=np.float64)
    out = np.array(x_init, dtype=np.float64, copy=True)
    for p in range(pt_ptr.shape[0] - 1):
        obs = range(pt_ptr[p], pt_ptr[p + 1])
        if len(obs):
            out[:, p:p + 1] = oracle.nonlinear_triangulate(out[:, p:p + 1], [projs[cam_idx[o]] for o in obs],
                                                           [uv[:, o:o + 1] for o in obs], lam, iters)
    cost = np.vstack((track_cost(pt_ptr, cam_idx, uv, projs, np.asarray(x_init, dtype=np.float64)),
                      track_cost(pt_ptr, cam_idx, uv, projs, out)))
    return out, cost


def dlt_tracks_reference(pt_ptr, cam_idx, uv, projs, x_init=None):
    """(X (4, n), solved (n,) bool): the null vector of every track's DLT matrix by SVD, divided by its W; tracks with
    fewer than two observations keep x_init (or (0, 0, 0, 1))."""
    n = pt_ptr.shape[0] - 1
    out = np.zeros((4, n)); out[3] = 1.0
    if x_init is not None:
        out[:] = x_init
    solved = np.zeros(n, dtype=bool)
    for p in range(n):
        obs = np.arange(pt_ptr[p], pt_ptr[p + 1])
        if obs.size < 2:
            continue
        a = np.empty((2 * obs.size, 4))
        pr = projs[cam_idx[obs]]
        a[0::2] = uv[0, obs][:, None] * pr[:, 2] - pr[:, 0]
        a[1::2] = uv[1, obs][:, None] * pr[:, 2] - pr[:, 1]
        vh = np.linalg.svd(a)[2]
        out[:, p] = vh[-1] / vh[-1, 3]
        solved[p] = True
    return out, solved


def camera_projections(sfm, cams):
    """(V, 3, 4): [R^T | -R^T C] of packed cameras [C, q]."""
    projs = []
    for c in np.asarray(cams, dtype=np.float64).reshape(-1, 7):
        rot = sfm.geometry.quaternion_to_rotation_unchecked(c[3:7])
        projs.append(np.hstack((rot.T, rot.T @ -c[0:3].reshape(3, 1))))
    return np.stack(projs)


_SCENES = {}
_REFINED = {}


def ragged_scene(sfm, seed=0):
    """The shared test scene: 130 cameras, 66 points, three points of every length of TRACK_LENGTHS (each track a sorted
    random subset of the cameras), keys normalised with inv(K), projections [R^T | -R^T C] of the true cameras, initial
    points = truth + N(0, 0.05)."""
    if seed in _SCENES:
        return _SCENES[seed]
    sc = sfm.scenes.make_scene(130, 66, 1.0, seed=7)
    rng = np.random.default_rng(seed)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    lengths = np.repeat(np.array(TRACK_LENGTHS), 3)
    assert lengths.shape[0] == sc.n_pts
    pt_ptr = np.zeros(sc.n_pts + 1, dtype=np.int32)
    np.cumsum(lengths, out=pt_ptr[1:])
    cam_idx = np.empty(pt_ptr[-1], dtype=np.int32)
    uv = np.empty((2, pt_ptr[-1]))
    for p in range(sc.n_pts):
        cams = np.sort(rng.choice(sc.n_cams, size=lengths[p], replace=False))
        cam_idx[pt_ptr[p]:pt_ptr[p + 1]] = cams
        uv[:, pt_ptr[p]:pt_ptr[p + 1]] = uvn[:, p * sc.n_cams + cams]        # all-visible scene: observation (p, c) at p V + c
    x_init = np.vstack((sc.pts_true + rng.normal(0.0, 0.05, sc.pts_true.shape), np.ones((1, sc.n_pts))))
    out = SimpleNamespace(scene=sc, pt_ptr=pt_ptr, cam_idx=cam_idx, uv=uv, projs=camera_projections(sfm, sc.cams_true),
                          x_init=x_init, lengths=lengths, n_pts=sc.n_pts, seed=seed)
    for arr in (pt_ptr, cam_idx, uv, out.projs, x_init, lengths):
        arr.setflags(write=False)
    _SCENES[seed] = out
    return out


def ragged_reference(sfm, lam, iters, seed=0):
    """refine_tracks_reference on ragged_scene(seed), computed once per (lam, iters) and left unchanged."""
    key = (seed, float(lam), int(iters))
    if key not in _REFINED:
        rs = ragged_scene(sfm, seed)
        x, cost = refine_tracks_reference(rs.pt_ptr, rs.cam_idx, rs.uv, rs.projs, rs.x_init, lam, iters)
        x.setflags(write=False); cost.setflags(write=False)
        _REFINED[key] = (x, cost)
    return _REFINED[key]
