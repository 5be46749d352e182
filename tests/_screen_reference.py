"""Float64 NumPy reference of the screening and culling of a bundle-adjustment scene (sfm_ba_screen / sfm_ba_cull).

Projections are ``_tracks_reference.camera_projections`` of the packed cameras, [R(q)^T | -R(q)^T C]; everything else is
written out per point, in the words of include/sfm_hip.h."""
import importlib
from types import SimpleNamespace

import numpy as np

import _tracks_reference as tr

OBS_HIGH_ERROR, OBS_BEHIND, OBS_NONFINITE, OBS_POINT = 1, 2, 4, 8
PT_TOO_FEW, PT_LOW_ANGLE, PT_EMPTY = 1, 2, 4


def _sfm():
    return importlib.import_module("structure-from-motion_amd")


def screen_reference(pt_ptr, cam_idx, uv, cams, pts, max_err2=np.inf, cos_min_angle=1.0, min_obs=2, cam_scale=None):
    """The fields of ``BaProblem.screen`` (err2, depth, obs_flags, min_cos, pt_flags, summary) plus ``keep`` (N,), the
    observations every point keeps.  cams (V, 7) packed [C, q], pts (3, N)."""
    pt_ptr = np.asarray(pt_ptr); cam_idx = np.asarray(cam_idx)
    uv = np.asarray(uv, dtype=np.float64); cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    pts = np.asarray(pts, dtype=np.float64)
    n, m = pt_ptr.shape[0] - 1, cam_idx.shape[0]
    projs = tr.camera_projections(_sfm(), cams)
    scale = np.ones(cams.shape[0]) if cam_scale is None else np.asarray(cam_scale, dtype=np.float64)
    pt_of = np.repeat(np.arange(n), np.diff(pt_ptr))
    xh = np.vstack((pts, np.ones((1, n))))
    with np.errstate(all="ignore"):
        s = np.einsum("oij,jo->oi", projs[cam_idx], xh[:, pt_of]) if m else np.zeros((0, 3))
        depth = s[:, 2].copy()
        err2 = scale[cam_idx] ** 2 * ((s[:, 0] / s[:, 2] - uv[0]) ** 2 + (s[:, 1] / s[:, 2] - uv[1]) ** 2)
        flags = np.zeros(m, dtype=np.uint8)
        finite = np.isfinite(err2)
        flags[~finite] |= OBS_NONFINITE
        flags[finite & (err2 > max_err2)] |= OBS_HIGH_ERROR
        flags[depth <= 0] |= OBS_BEHIND
        min_cos = np.ones(n)
        pt_flags = np.zeros(n, dtype=np.int32)
        keep = np.zeros(n, dtype=np.int64)
        summary = np.zeros(8, dtype=np.int64)
        for p in range(n):
            obs = np.arange(pt_ptr[p], pt_ptr[p + 1])
            if obs.size == 0:
                pt_flags[p] = PT_EMPTY
                continue
            live = obs[flags[obs] == 0]
            if live.size >= 2:
                rays = cams[cam_idx[live], 0:3] - pts[:, p]
                rays = rays / np.linalg.norm(rays, axis=1, keepdims=True)
                cos = rays @ rays.T
                min_cos[p] = cos[np.triu_indices(live.size, 1)].min()
            if live.size < min_obs:
                pt_flags[p] |= PT_TOO_FEW
            if live.size >= 2 and cos_min_angle < 1 and min_cos[p] > cos_min_angle:
                pt_flags[p] |= PT_LOW_ANGLE
            if pt_flags[p] & (PT_TOO_FEW | PT_LOW_ANGLE):
                flags[live] = OBS_POINT
                summary[5] += live.size
            else:
                keep[p] = live.size
    summary[0] = m
    summary[1] = keep.sum()
    summary[2] = np.count_nonzero(flags & OBS_HIGH_ERROR)
    summary[3] = np.count_nonzero(flags & OBS_BEHIND)
    summary[4] = np.count_nonzero(flags & OBS_NONFINITE)
    summary[6] = np.count_nonzero(pt_flags & PT_TOO_FEW)
    summary[7] = np.count_nonzero(pt_flags & PT_LOW_ANGLE)
    return SimpleNamespace(err2=err2, depth=depth, obs_flags=flags, min_cos=min_cos, pt_flags=pt_flags, summary=summary,
                           keep=keep)


def compact(pt_ptr, cam_idx, uv, obs_flags):
    """(pt_ptr, cam_idx, uv) of the observations whose flags are clear, in their old order."""
    pt_ptr = np.asarray(pt_ptr); cam_idx = np.asarray(cam_idx); uv = np.asarray(uv, dtype=np.float64)
    n = pt_ptr.shape[0] - 1
    stay = np.asarray(obs_flags) == 0
    pt_of = np.repeat(np.arange(n), np.diff(pt_ptr))
    new_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(pt_of[stay], minlength=n), out=new_ptr[1:])
    return new_ptr, cam_idx[stay].astype(np.int32), np.ascontiguousarray(uv[:, stay])


def cull_reference(pt_ptr, cam_idx, uv, cams, pts, max_err2=np.inf, cos_min_angle=1.0, min_obs=2, cam_scale=None):
    """The compacted (pt_ptr, cam_idx, uv) ``BaProblem.cull`` leaves on the device."""
    ref = screen_reference(pt_ptr, cam_idx, uv, cams, pts, max_err2, cos_min_angle, min_obs, cam_scale)
    return compact(pt_ptr, cam_idx, uv, ref.obs_flags)


def threshold_in_gap(values, quantile):
    """A threshold no value is close to: the midpoint of the widest gap among the 40 sorted values around the quantile.
    The gap is at least 1e-4 relative, so a flag can differ between two float64 evaluations only through a real error."""
    v = np.sort(np.asarray(values, dtype=np.float64)[np.isfinite(values)])
    k = int(round(quantile * (v.shape[0] - 1)))
    lo = max(0, min(k - 20, v.shape[0] - 40))
    win = v[lo:lo + 40]
    assert win.shape[0] >= 2
    g = int(np.argmax(np.diff(win)))
    mid = 0.5 * (win[g] + win[g + 1])
    assert (win[g + 1] - win[g]) >= 1e-4 * abs(mid), (win[g], win[g + 1])
    return float(mid)


_OUTLIER = {}


def outlier_scene(sfm):
    """The drop-in's end-to-end scene: make_scene(6, 300, 0.7, seed=21) with 3 % of its observations, chosen by
    default_rng(5), displaced by 30 to 120 px in a random direction.  Returns the scene with the displaced pixels and
    ``displaced`` (M,) bool; built once and left unchanged."""
    if "scene" not in _OUTLIER:
        sc = sfm.scenes.make_scene(6, 300, 0.7, seed=21)
        rng = np.random.default_rng(5)
        m = sc.cam_idx.shape[0]
        hit = rng.choice(m, size=int(0.03 * m), replace=False)
        radius = rng.uniform(30.0, 120.0, hit.shape[0])
        angle = rng.uniform(0.0, 2.0 * np.pi, hit.shape[0])
        uv_pix = sc.uv_pix.copy()
        uv_pix[:, hit] += radius * np.vstack((np.cos(angle), np.sin(angle)))
        displaced = np.zeros(m, dtype=bool)
        displaced[hit] = True
        for arr in (uv_pix, displaced):
            arr.setflags(write=False)
        _OUTLIER["scene"] = SimpleNamespace(scene=sc, uv_pix=uv_pix, displaced=displaced)
    return _OUTLIER["scene"]
