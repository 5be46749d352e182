"""Float64 NumPy reference of the motion-only refinement of the resident scene (sfm_ba_refine_cameras).

One pass takes r, Jp of all observations from ``oracle.obs_terms_vec``, weights them with ``_robust_reference.loss_terms``,
accumulates U_c = sum Jp^T Jp and g_c = sum Jp^T r with ``np.add.at`` and applies ``np.linalg.solve(U_c + lam I, g_c)`` to
every camera that moves; q is normalised afterwards.  The points are held.  Per-camera costs are taken at entry and at exit."""
import numpy as np

import _robust_reference as rr

CAM_EMPTY, CAM_NONFINITE, CAM_BEHIND, CAM_HELD = 1, 2, 4, 8


def per_camera_cost(cams, pts, cam_idx, pt_idx, uv, kind=rr.LOSS_NONE, delta=1.0):
    """(V,): every camera's share of the minimised cost at the given state."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    with np.errstate(all="ignore"):
        r = rr._oracle().obs_terms_vec(cams, np.asarray(pts, dtype=np.float64), cam_idx, pt_idx, uv)[0]
        rho = rr.loss_terms(kind, delta, r)[2]
    out = np.zeros(cams.shape[0])
    np.add.at(out, cam_idx, rho * (1.0 if kind == rr.LOSS_NONE else delta * delta))
    return out


def refine_cameras(cams, pts, cam_idx, pt_idx, uv, lam, iters, kind=rr.LOSS_NONE, delta=1.0, quirks=None, mask=None):
    """(cams (V, 7), cost (2, V), status (V,)) in the words of include/sfm_hip.h: a held or empty camera is evaluated once,
    a camera that meets a non-finite sum, a failing solve or an invalid updated rotation comes back as it went in with
    CAM_NONFINITE and its entry cost in both rows."""
    oracle = rr._oracle()
    quirks = oracle.QUIRKS_REFERENCE if quirks is None else quirks
    cams = np.array(cams, dtype=np.float64, copy=True).reshape(-1, 7)
    cams_in = cams.copy()
    pts = np.asarray(pts, dtype=np.float64)
    cam_idx = np.asarray(cam_idx); pt_idx = np.asarray(pt_idx)
    nv = cams.shape[0]
    counts = np.bincount(cam_idx, minlength=nv)
    held = np.zeros(nv, dtype=bool) if mask is None else (np.asarray(mask).ravel() == 0)
    my_iters = np.where(held | (counts == 0), 0, iters)
    status = np.zeros(nv, dtype=np.int32)
    status[counts == 0] |= CAM_EMPTY
    status[held] |= CAM_HELD
    dead = np.zeros(nv, dtype=bool)
    cost = np.zeros((2, nv))
    scale = 1.0 if kind == rr.LOSS_NONE else delta * delta
    for it in range(iters + 1):
        act = (counts > 0) & ~dead & (my_iters >= it)
        if not act.any():
            break
        with np.errstate(all="ignore"):
            r, jp, _jx = oracle.obs_terms_vec(cams, pts, cam_idx, pt_idx, uv, quirks)
            _s, w, rho = rr.loss_terms(kind, delta, r)
            if kind != rr.LOSS_NONE:
                sw = np.sqrt(w)
                r, jp = r * sw[:, None], jp * sw[:, None, None]
            share = np.zeros(nv)
            np.add.at(share, cam_idx, rho * scale)
            u = np.zeros((nv, 7, 7))
            np.add.at(u, cam_idx, np.einsum("mki,mkj->mij", jp, jp))
            g = np.zeros((nv, 7))
            np.add.at(g, cam_idx, np.einsum("mki,mk->mi", jp, r))
            rots = np.stack([oracle.quat_to_rot_unchecked(cams[c, 3:7]) for c in range(nv)])
            depth = np.einsum("mj,mj->m", rots[cam_idx][:, :, 2], pts[:, pt_idx].T - cams[cam_idx, 0:3])
        for c in np.flatnonzero(act):
            if it == 0:
                cost[0, c] = share[c]
            ok = bool(np.isfinite(u[c]).all() and np.isfinite(g[c]).all() and np.isfinite(share[c]))
            new = None
            if ok and it < my_iters[c]:
                try:
                    new = cams[c] + np.linalg.solve(u[c] + lam * np.eye(7), g[c])
                    new[3:7] /= np.sqrt(np.sum(np.square(new[3:7])))
                    ok = bool(np.isfinite(new).all())
                    if ok:
                        oracle.rot_to_quat(oracle.quat_to_rot(new[3:7]))
                except (np.linalg.LinAlgError, ValueError):
                    ok = False
            if not ok:
                dead[c] = True
                status[c] |= CAM_NONFINITE
                cams[c] = cams_in[c]
                cost[1, c] = cost[0, c]
            elif it == my_iters[c]:
                cost[1, c] = share[c]
                if np.any(depth[cam_idx == c] <= 0):
                    status[c] |= CAM_BEHIND
            else:
                cams[c] = new
    return cams, cost, status
