"""Three upenn frames from pixels: the first three steps of BaProcessor.process (ba_processor.py:43-270), shared by the
CPU run that fixes the bounds (test_sift_host.py) and the device run held to them (test_gpu_sift.py).

``recorded`` gives the reference's recorded poses of views 0-2 relative to view 0; ``epipolar_fraction`` measures
keypoint quality against them without any part of the two-view chain."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture(n):
    return np.load(os.path.join(GOLDEN, "g13_upenn_%d.npz" % n))


def halved_k():
    k = fixture(1)["K"].copy()
    k[:2] *= 0.5                                          # the fixtures are halved frames
    return k


def recorded(view):
    """Recorded rotation and centre of ``view`` in view 0's frame."""
    g = fixture(1)
    r0, c0 = g["rotations"][0], g["centres"][0].reshape(3, 1)
    return r0.T @ g["rotations"][view], r0.T @ (g["centres"][view].reshape(3, 1) - c0)


def rot_angle_deg(ra, rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(ra.T @ rb) - 1) / 2, -1, 1))))


def dir_angle_deg(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    return float(np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1))))


def epipolar_fraction(left, right, k, view, tol_px=2.0):
    """Share of the pairs (3, n) pixel arrays of views 0 and ``view`` whose right point lies within tol_px of the
    epipolar line of the recorded relative pose."""
    rot, loc = recorded(view)
    t = -rot.T @ loc                                       # x_v = R^T (X - C)
    tx = np.array([[0, -t[2, 0], t[1, 0]], [t[2, 0], 0, -t[0, 0]], [-t[1, 0], t[0, 0], 0]])
    kinv = np.linalg.inv(k)
    fund = kinv.T @ tx @ rot.T @ kinv
    lines = fund @ left
    d = np.abs(np.sum(lines * right, axis=0)) / np.hypot(lines[0], lines[1])
    return float(np.mean(d <= tol_px)), float(np.median(d))


def reprojection_rmse(views, track_list, tri_pts):
    """RMSE (px) over every (view, key) whose own table row names a triangulated point."""
    err = []
    for v, view in enumerate(views):
        row = track_list[v].table[v]
        keys = np.flatnonzero(row >= 0)
        if len(keys) == 0:
            continue
        x = tri_pts[:, row[keys]]
        p = view.cam_proj @ x
        uv = np.array([view.key_pts[k].pt for k in keys]).T
        err.append(np.sum((p[0:2] / p[2] - uv) ** 2, axis=0))
    return float(np.sqrt(np.mean(np.concatenate(err))))


def dlt_triangulate(p1, p2, left, right):
    out = np.zeros((4, left.shape[1]))
    for i in range(left.shape[1]):
        a = np.vstack((left[0, i] * p1[2] - p1[0], left[1, i] * p1[2] - p1[1],
                       right[0, i] * p2[2] - p2[0], right[1, i] * p2[2] - p2[1]))
        x = np.linalg.svd(a)[2][-1]
        out[:, i] = x / x[3]
    return out


def dlt_pnp_ransac(uv, xh, k, rng, iters=300, thr=8.0):
    """Six-point DLT PnP in a RANSAC loop (pixel threshold): (inlier indices, R, C)."""
    kinv = np.linalg.inv(k)
    xn = kinv @ uv
    best = (np.zeros(0, dtype=int), None, None)
    for _ in range(iters):
        s = rng.choice(uv.shape[1], 6, replace=False)
        a = []
        for i in s:
            X = xh[:, i]
            a.append(np.concatenate((X, np.zeros(4), -xn[0, i] * X)))
            a.append(np.concatenate((np.zeros(4), X, -xn[1, i] * X)))
        p = np.linalg.svd(np.array(a))[2][-1].reshape(3, 4)
        u, sv, vt = np.linalg.svd(p[:, 0:3])
        rt = u @ vt
        scale = sv[0]
        if np.linalg.det(rt) < 0:
            rt, scale = -rt, -scale
        t = p[:, 3:4] / scale
        proj = k @ np.hstack((rt, t))
        q = proj @ xh
        ok = (q[2] > 0) & (np.hypot(q[0] / q[2] - uv[0], q[1] / q[2] - uv[1]) < thr)
        if ok.sum() > len(best[0]):
            best = (np.flatnonzero(ok), rt.T, -rt.T @ t)
    return best


def process_three_on_device(sfm, imgs, k):
    """ba_processor.py:43-270 for views 0, 1, 2 through the drop-ins (HipViewProcessor, HipKeyTracker,
    HipEpipolarProcessor, HipCamposeProcessor, HipTriangulationProcessor, HipBaProcessor), with the reference's RANSAC
    configurations (ba_processor.py:463-488) except the epipolar threshold (1e-2)."""
    proc = sfm.processors
    cfg_kt = proc.RansacConfig(1e-2, 0.99, 0.75, 8, 200)
    cfg_ep = proc.RansacConfig(1e-2, 0.99, 0.75, 8, 300)
    cfg_cp = proc.RansacConfig(8.0, 0.99, 0.75, 8, 300)
    vp = proc.HipViewProcessor('sift')
    kt = proc.HipKeyTracker('sift', False, True, False, cfg_kt)
    epi = proc.HipEpipolarProcessor(cfg_ep)
    tp = proc.HipTriangulationProcessor()
    cp = proc.HipCamposeProcessor(cfg_cp, 5, 300)
    bp = proc.HipBaProcessor(vp, kt, epi, tp, cp)
    bp.ba_verbose = False
    out = {}
    for idx, img in enumerate(imgs):
        view = vp.generate_view(img, idx, k)
        kt.add_new_view(view, vp.view_list)
        vp.add_view(view)
        views = vp.view_list
        if idx == 0:
            views[0].is_valid = True
        elif idx == 1:
            pairs, r_idx, q_idx = kt.generate_matched_pairs(0, 1, views)
            out["pairs01"] = pairs
            out["fund_inliers"] = len(epi.determine_fundamental_mat(pairs))
            epi.extract_essential_mat(views[0].k, views[1].k)
            r1, r2, c1, c2 = cp.extract_cam_pose_from_essential_mat(epi.esse_mat)
            rs, cs = [r1, r1, r2, r2], [c1, c2, c1, c2]
            projs4 = [k @ np.hstack((r.T, -r.T @ c)) for r, c in zip(rs, cs)]
            ref_proj = views[0].cam_proj
            tris = [tp.linear_triangulate([ref_proj, p], pairs) for p in projs4]
            best, valid = cp.disambiguate_cam_pose_four(ref_proj, projs4, tris)
            views[1].update_cam_pose(rs[best], cs[best])
            valid = np.array(valid)[np.newaxis, :]
            vpairs = [np.take_along_axis(pairs[0], valid, axis=1), np.take_along_axis(pairs[1], valid, axis=1)]
            pts = tp.nonlinear_triangulate(np.take_along_axis(tris[best], valid, axis=1), [ref_proj, projs4[best]], vpairs)
            tri_idx = np.arange(pts.shape[1], dtype=int)[np.newaxis, :]
            kt.track_list[0].update_usage(np.take(r_idx, valid), tri_idx)
            kt.track_list[1].update_usage(np.take(q_idx, valid), tri_idx)
            views[1].is_valid = True
            views[1].ref_idx = 0
            tp.add_tri_pt(pts)
        else:
            cur = views[idx]
            b = kt.find_best_view(idx)
            cur.ref_idx = b
            pairs, b_key, c_key = kt.generate_matched_pairs(b, idx, views)
            b_tri_idx, b_tri_val = kt.track_list[b].extract_constructed_points()
            used, b_i, t_i = np.intersect1d(b_key, b_tri_idx, return_indices=True)
            tri_pts = np.take_along_axis(tp.tri_pts, np.take_along_axis(b_tri_val, t_i[np.newaxis, :], axis=1), axis=1)
            c_pts = np.take_along_axis(pairs[1], b_i[np.newaxis, :], axis=1)
            inl, c_rot, c_loc = cp.estimate_cam_pose_pnp(c_pts, tri_pts, cur.k)
            out["pnp_points"], out["pnp_inliers"] = c_pts.shape[1], len(inl)
            cur.update_cam_pose(c_rot, c_loc)
            cur.is_valid = True
            out["pnp_rot"], out["pnp_loc"] = c_rot, c_loc
            unused = kt.track_list[b].extract_unconstructed_points()
            un_val, b_i2, _ = np.intersect1d(b_key, unused, return_indices=True)
            un_val = un_val[np.newaxis, :]
            b_pts = np.take_along_axis(pairs[0], b_i2[np.newaxis, :], axis=1)
            c_pts2 = np.take_along_axis(pairs[1], b_i2[np.newaxis, :], axis=1)
            new = tp.triangulate([views[b].cam_proj, cur.cam_proj], [b_pts, c_pts2])
            tri_idx = np.arange(tp.tri_pts.shape[1], tp.tri_pts.shape[1] + new.shape[1], dtype=int)[np.newaxis, :]
            kt.track_list[b].update_usage(un_val, tri_idx)
            kt.track_list[idx].update_usage(np.take(kt.track_list[b].table[idx, :], un_val), tri_idx)
            tp.add_tri_pt(new)
            out["rmse_before_ba"] = reprojection_rmse(views, kt.track_list, tp.tri_pts)
            bp._BaProcessor__execute_bundle_adjustment()
            out["rmse_after_ba"] = reprojection_rmse(views, kt.track_list, tp.tri_pts)
            out["n_points"] = tp.tri_pts.shape[1]
            out["ba_rot"], out["ba_loc"] = cur.rot, cur.loc
    bp.ba_release()
    kt.kt_release()
    out["views"] = vp.view_list
    return out
