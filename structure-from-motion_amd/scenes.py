"""Seeded synthetic bundle-adjustment scenes.

The reference has no scene generator (its demo needs OpenCV SIFT on the upenn BMPs,
ba_processor.py:443-546); BASELINE.json's configs 2-4 are "synthetic V cams x N points at
p% visibility".  This module is the single definition of that workload: it is used by
bench.py, by the GPU parity tests and by tools/capture_goldens.py (which additionally
stores the generated arrays inside the golden fixtures so the tests never depend on the
generator staying bit-stable).

Conventions follow the reference: ``rot`` = R, ``loc`` = C (camera centre), world->camera
``p = R^T (X - C)`` (view_processor.py:53-57); the intrinsics are the demo's upenn K
(ba_processor.py:457-459); the camera block is ``[Cx,Cy,Cz,qw,qx,qy,qz]``
(ba_processor.py:285-288).
"""
from dataclasses import dataclass

import numpy as np
from scipy.spatial.transform import Rotation

from .geometry import rotation_to_quaternion

UPENN_K = np.array([[568.996140852, 0.0, 643.21055941],
                    [0.0, 568.988362396, 477.982801038],
                    [0.0, 0.0, 1.0]])

# BASELINE.json configs (name -> cams, points, visibility)
CONFIGS = {
    "C2": dict(n_cams=5, n_pts=2000, visibility=1.0),
    "C3": dict(n_cams=50, n_pts=20000, visibility=0.6),
    "C4": dict(n_cams=200, n_pts=100000, visibility=0.15),
}


@dataclass
class Scene:
    """Observation-list form of a BA problem (what crosses the C-ABI)."""
    intrinsic: np.ndarray      # (3,3)
    cams_true: np.ndarray      # (V,7)
    cams_init: np.ndarray      # (V,7)  [C, q]
    pts_true: np.ndarray       # (3,N)
    pts_init: np.ndarray       # (3,N)
    pt_ptr: np.ndarray         # (N+1,) int32 CSR over observations sorted by (point, cam)
    cam_idx: np.ndarray        # (M,) int32
    pt_idx: np.ndarray         # (M,) int32
    uv_pix: np.ndarray         # (2,M) pixel observations

    @property
    def n_cams(self):
        return self.cams_init.shape[0]

    @property
    def n_pts(self):
        return self.pts_init.shape[1]

    @property
    def n_obs(self):
        return self.cam_idx.shape[0]


def _project(rot, loc, pts, intrinsic):
    cam = rot.T @ (pts - loc.reshape(3, 1))
    pix = intrinsic @ cam
    return pix[0:2] / pix[2:3], cam[2]


def visibility_mask(rng, n_cams, n_pts, visibility):
    """Bernoulli(p) per (cam, point); every point is forced into at least two cameras."""
    vis = rng.random((n_cams, n_pts)) < visibility
    need = np.flatnonzero(vis.sum(axis=0) < 2)
    for p in need:
        extra = rng.choice(n_cams, size=2, replace=False)
        vis[extra, p] = True
    return vis


@dataclass(frozen=True)
class Structure:
    """Track-structured visibility, the shape the reference's incremental loop produces (ba_processor.py:137-267):
    a point enters with its second registered view and is then seen by a run of consecutive views.

    Every point gets a birth view and a track length ``1 + Geometric(1 / (mean_track - 1))`` (at least 2, mean
    ``mean_track``) and is seen by the consecutive views ``[birth, birth + length)`` of its camera group, clipped at the
    group's last view.  On top of that:

    ``heavy``     fraction of points seen by every view of their group from their birth on (long tracks);
    ``single``    fraction of points with exactly one observation;
    ``empty``     camera indices with no observation at all (they are left out of every run);
    ``clusters``  the cameras split into this many disjoint groups of consecutive indices, each point seen within one
                  group only: the reduced camera system is block-diagonal;
    ``hub``       camera indices that see every point (left out of the runs, added to every point afterwards).

    Points are numbered in birth order, as the reference's incremental loop numbers them."""
    mean_track: float = 4.0
    heavy: float = 0.0
    single: float = 0.0
    empty: tuple = ()
    clusters: int = 1
    hub: tuple = ()

    def groups(self, n_cams):
        """The cameras each group's runs go over, in order: ``clusters`` consecutive index ranges without the empty
        and hub cameras."""
        skip = set(self.empty) | set(self.hub)
        return [[int(c) for c in part if c not in skip] for part in np.array_split(np.arange(n_cams), self.clusters)]


def structured_mask(rng, n_cams, n_pts, st):
    """Visibility of a ``Structure`` (see there): (n_cams, n_pts) bool, columns in birth order."""
    if st.mean_track < 2:
        raise ValueError("mean_track must be >= 2")
    if not 0 <= st.heavy + st.single <= 1:
        raise ValueError("heavy + single must lie in [0, 1]")
    if st.hub and st.single > 0:
        raise ValueError("hub cameras see every point: no point can have a single observation")
    if set(st.hub) & set(st.empty):
        raise ValueError("a camera cannot be both a hub and empty")
    groups = st.groups(n_cams)
    if any(len(g) < 2 for g in groups):
        raise ValueError("every camera group needs at least two cameras that are neither empty nor hubs")
    group = rng.integers(0, len(groups), n_pts)
    kind = rng.random(n_pts)                       # [0, single): one view; [single, single + heavy): to the group's end
    single = kind < st.single
    heavy = ~single & (kind < st.single + st.heavy)
    length = 1 + (rng.geometric(1.0 / (st.mean_track - 1.0), n_pts) if st.mean_track > 2 else np.ones(n_pts, dtype=np.int64))
    u = rng.random(n_pts)
    vis = np.zeros((n_cams, n_pts), dtype=bool)
    birth_cam = np.empty(n_pts, dtype=np.int64)
    for p in range(n_pts):
        g = groups[group[p]]
        n = len(g)
        if single[p]:
            b = int(u[p] * n)
            e = b + 1
        else:
            b = int(u[p] * (n - 1))                # at least two views left from the birth on
            e = n if heavy[p] else min(n, b + int(length[p]))
        vis[g[b:e], p] = True
        birth_cam[p] = g[b]
    vis[list(st.hub), :] = True
    return vis[:, np.argsort(birth_cam, kind="stable")]


def make_scene(n_cams, n_pts, visibility=1.0, seed=0, pixel_noise=0.5,
               rot_noise=0.01, loc_noise=0.05, pt_noise=0.05, structure=None):
    """A seeded scene.  ``structure=None``: Bernoulli(``visibility``) per (camera, point) (``visibility_mask``; the
    stream bench.py and the goldens are built from).  ``structure=Structure(...)``: track-structured visibility
    (``visibility`` is then unused); the geometry is drawn the same way."""
    rng = np.random.default_rng(seed)
    intrinsic = UPENN_K.copy()

    pts_true = np.vstack((rng.uniform(-4, 4, n_pts),
                          rng.uniform(-3, 3, n_pts),
                          rng.uniform(8, 16, n_pts)))

    rots, locs = [np.eye(3)], [np.zeros(3)]
    for _ in range(1, n_cams):
        ang = rng.uniform(-0.15, 0.15, 3)
        rots.append(Rotation.from_euler('zyx', ang).as_matrix())
        locs.append(rng.uniform(-1.5, 1.5, 3) * np.array([1.0, 0.3, 0.5]))

    if structure is None:
        vis = visibility_mask(rng, n_cams, n_pts, visibility)
    else:
        vis = structured_mask(rng, n_cams, n_pts, structure)

    # observation list sorted by (point, cam): the reference's BA loop order (ba_processor.py:304-306)
    pt_idx, cam_idx = np.nonzero(vis.T)
    pt_idx = pt_idx.astype(np.int32)
    cam_idx = cam_idx.astype(np.int32)
    m = pt_idx.shape[0]
    uv = np.empty((2, m))
    for c in range(n_cams):
        sel = np.flatnonzero(cam_idx == c)
        pix, _depth = _project(rots[c], locs[c], pts_true[:, pt_idx[sel]], intrinsic)
        uv[:, sel] = pix
    uv += rng.normal(0.0, pixel_noise, uv.shape)

    pt_ptr = np.zeros(n_pts + 1, dtype=np.int32)
    np.cumsum(np.bincount(pt_idx, minlength=n_pts), out=pt_ptr[1:])

    cams_true = np.empty((n_cams, 7))
    cams_init = np.empty((n_cams, 7))
    for c in range(n_cams):
        cams_true[c, 0:3] = locs[c]
        cams_true[c, 3:7] = rotation_to_quaternion(rots[c]).reshape(4)
        if c == 0:
            r0, c0 = rots[c], locs[c]
        else:
            r0 = rots[c] @ Rotation.from_rotvec(rng.normal(0.0, rot_noise, 3)).as_matrix()
            c0 = locs[c] + rng.normal(0.0, loc_noise, 3)
        cams_init[c, 0:3] = c0
        cams_init[c, 3:7] = rotation_to_quaternion(r0).reshape(4)
    pts_init = pts_true + rng.normal(0.0, pt_noise, pts_true.shape)

    return Scene(intrinsic, cams_true, cams_init, pts_true, pts_init,
                 pt_ptr, cam_idx, pt_idx, uv)


def make_config(name, seed=0, n_pts=None):
    cfg = dict(CONFIGS[name])
    if n_pts is not None:
        cfg["n_pts"] = n_pts
    return make_scene(seed=seed, **cfg)


def reprojection_rmse(cams, pts, scene):
    """Pixel RMSE ``sqrt(mean ||K pi(R^T (X - C)) - uv||^2)`` over all observations
    (the metric definition of BASELINE.md section 4)."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    pts = np.asarray(pts, dtype=np.float64)
    c = cams[scene.cam_idx]
    w, x, y, z = c[:, 3], c[:, 4], c[:, 5], c[:, 6]
    d = pts[:, scene.pt_idx].T - c[:, 0:3]
    # rows of R^T applied to d
    r00 = 1 - 2 * z * z - 2 * y * y; r01 = -2 * z * w + 2 * y * x; r02 = 2 * y * w + 2 * z * x
    r10 = 2 * x * y + 2 * w * z; r11 = 1 - 2 * z * z - 2 * x * x; r12 = 2 * z * y - 2 * x * w
    r20 = 2 * x * z - 2 * w * y; r21 = 2 * y * z + 2 * w * x; r22 = 1 - 2 * y * y - 2 * x * x
    px = r00 * d[:, 0] + r10 * d[:, 1] + r20 * d[:, 2]
    py = r01 * d[:, 0] + r11 * d[:, 1] + r21 * d[:, 2]
    pz = r02 * d[:, 0] + r12 * d[:, 1] + r22 * d[:, 2]
    k = scene.intrinsic
    u = k[0, 0] * px / pz + k[0, 1] * py / pz + k[0, 2]
    v = k[1, 1] * py / pz + k[1, 2]
    err = (u - scene.uv_pix[0]) ** 2 + (v - scene.uv_pix[1]) ** 2
    return float(np.sqrt(err.mean()))


# ---- descriptor views for KeyTracker.__extend_list (key_tracker.py:213-317) ----------------------------------------
class KeyPoint:
    """The part of ``cv2.KeyPoint`` the pipeline reads: ``pt`` = (x, y) pixels."""
    __slots__ = ("pt",)

    def __init__(self, x, y):
        self.pt = (float(x), float(y))


@dataclass
class DescriptorViews:
    """Per view: keys (pixels), SIFT-like uint8 descriptors (n, 128), ORB-like uint8 descriptors (n, 32), and the
    3D point each key observes (-1 for a distractor)."""
    intrinsic: np.ndarray
    pts: np.ndarray    # (3, n_pts) the scene's points
    rots: list
    locs: list
    pix: list          # (n_v, 2) float64
    sift: list         # (n_v, 128) uint8
    orb: list          # (n_v, 32) uint8
    point: list        # (n_v,) int64

    def key_pts(self, v):
        return [KeyPoint(x, y) for x, y in self.pix[v]]


def make_descriptor_views(n_views=5, n_pts=200, seed=0, visibility=0.8, n_distract=40, noise=2, orb_flips=10, n_dup=6):
    """Seeded matching workload: a projected scene whose 3D points carry an integer SIFT-like base descriptor (norm
    about 512, clipped to [0, 255]) observed with small integer noise per key, distractor keys with random
    descriptors, and an ORB-like 256-bit variant (random base bits, ``orb_flips`` flipped per observation).  Each
    view also repeats ``n_dup`` of its rows verbatim at the end (exact ties between train rows: the lower index must
    win) and ``n_dup`` rows with extra noise (several queries on one train row: the duplicate removal, quirk Q14)."""
    rng = np.random.default_rng(seed)
    intrinsic = UPENN_K.copy()
    pts = np.vstack((rng.uniform(-4, 4, n_pts), rng.uniform(-3, 3, n_pts), rng.uniform(8, 16, n_pts)))
    base = rng.gamma(0.6, 1.0, (n_pts, 128))
    base = np.clip(np.rint(base / np.linalg.norm(base, axis=1, keepdims=True) * 512.0), 0, 255)
    orb_base = rng.integers(0, 2, (n_pts, 256), dtype=np.uint8)
    rots, locs, pix, sift, orb, point = [], [], [], [], [], []
    for v in range(n_views):
        ang = rng.uniform(-0.1, 0.1, 3) if v else np.zeros(3)
        rot = Rotation.from_euler('zyx', ang).as_matrix()
        loc = np.array([0.4 * v, 0.05 * rng.normal(), 0.1 * rng.normal()]) if v else np.zeros(3)
        seen = np.flatnonzero(rng.random(n_pts) < visibility)
        uv, _ = _project(rot, loc, pts[:, seen], intrinsic)
        d_s = np.clip(base[seen] + rng.integers(-noise, noise + 1, (seen.shape[0], 128)), 0, 255)
        bits = orb_base[seen].copy()
        for i in range(seen.shape[0]):
            bits[i, rng.choice(256, orb_flips, replace=False)] ^= 1
        dis_s = rng.gamma(0.6, 1.0, (n_distract, 128))
        dis_s = np.clip(np.rint(dis_s / np.linalg.norm(dis_s, axis=1, keepdims=True) * 512.0), 0, 255)
        dis_b = rng.integers(0, 2, (n_distract, 256), dtype=np.uint8)
        dis_uv = np.vstack((rng.uniform(0, 1280, n_distract), rng.uniform(0, 960, n_distract)))
        p = np.concatenate((seen, np.full(n_distract, -1)))
        u = np.hstack((uv, dis_uv)).T
        ds = np.vstack((d_s, dis_s))
        db = np.vstack((bits, dis_b))
        perm = rng.permutation(p.shape[0])
        p, u, ds, db = p[perm], u[perm], ds[perm], db[perm]
        same = rng.choice(p.shape[0], n_dup, replace=False)            # verbatim copies: exact ties
        near = rng.choice(p.shape[0], n_dup, replace=False)            # noisy copies: duplicate train indices
        ds_near = np.clip(ds[near] + rng.integers(-noise, noise + 1, (n_dup, 128)), 0, 255)
        db_near = db[near].copy()
        db_near[np.arange(n_dup), rng.integers(0, 256, n_dup)] ^= 1
        p = np.concatenate((p, p[same], p[near]))
        u = np.vstack((u, u[same], u[near] + rng.normal(0, 0.5, (n_dup, 2))))
        ds = np.vstack((ds, ds[same], ds_near))
        db = np.vstack((db, db[same], db_near))
        rots.append(rot); locs.append(loc)
        pix.append(u.astype(np.float64))
        sift.append(ds.astype(np.uint8))
        orb.append(np.packbits(db, axis=1))
        point.append(p.astype(np.int64))
    return DescriptorViews(intrinsic, pts, rots, locs, pix, sift, orb, point)
