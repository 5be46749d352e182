"""Drop-in mirrors of the reference's ``*_processor`` classes for the nonlinear-refinement hot path.

Same method names, argument meaning, defaults, return shapes, in-place semantics, prints and
exceptions as the reference; the arithmetic runs in libsfm_hip.so on an MI355X.

Two ways to use them:

* as **mixins in front of the reference classes** — the reference keeps its front end, linear
  solvers and state machine, the hot path is overridden::

      class TriangulationProcessor(HipTriangulationMixin, triangulation_processor.TriangulationProcessor): pass
      class CamposeProcessor(HipCamposeMixin, campose_processor.CamposeProcessor): pass
      class BaProcessor(HipBaMixin, ba_processor.BaProcessor): pass

* as the **standalone classes** below (``HipTriangulationProcessor`` ...), which carry the
  constructor state of the reference classes and are what the tests drive.

Reference interfaces mirrored (file:line in the reference repo):
  TriangulationProcessor.nonlinear_triangulate / construct_jacobian_matrix / triangulate
      triangulation_processor.py:160-234 / 237-271 / 31-88
  CamposeProcessor.nonlinear_estimate_cam_pose_pnp / construct_jacobian_matrix / estimate_cam_pose_pnp
      campose_processor.py:308-459 / 462-482 / 192-246
  BaProcessor.__execute_bundle_adjustment          ba_processor.py:274-439
  KeyTracker.__extend_list                         key_tracker.py:213-317
  View / ViewProcessor.__extract_keys              view_processor.py:14-106 / 110-202
"""
import logging
import math
import pickle

import numpy as np

from . import matching, native
from .geometry import (normalise_pixels, pack_cameras, quaternion_to_rotation_unchecked, quaternions_to_rotations)
from .observations import KeyCache, ObservationTracker, build_observations, gather_normalised_keys, remove_pairs
from .q13 import det_branch_fires, reference_winner
from .sampling import sample_indices


# ------------------------------------------------------------------------------------------------
class HipTriangulationMixin:
    """Hot-path methods of TriangulationProcessor (triangulation_processor.py:7-309)."""

    def nonlinear_triangulate(self, init_3d_pts, projs, matched_pairs,
                              damping_factor=None, iteration=None):
        # falsy -> instance default, exactly like the reference (tri:200-203, quirk Q4)
        if not damping_factor:
            damping_factor = self.damping_factor
        if not iteration:
            iteration = self.iteration
        num_pts = matched_pairs[0].shape[1]
        num_views = len(projs)
        init = np.ascontiguousarray(np.asarray(init_3d_pts), dtype=np.float64)
        if num_pts == 0:
            return np.copy(init)
        uv = np.empty((num_views, 2, num_pts), dtype=np.float64)
        for v in range(num_views):
            uv[v] = np.asarray(matched_pairs[v])[0:2, :]
        projs_arr = np.stack([np.asarray(p, dtype=np.float64).reshape(3, 4) for p in projs])
        # the reference iterates over matched_pairs[0].shape[1] columns of a copy of init_3d_pts
        out = np.copy(init)
        out[:, :num_pts] = native.tri_nonlinear(projs_arr, uv, init[:, :num_pts], damping_factor, iteration)
        return out

    def construct_jacobian_matrix(self, tri_3d_pt, projs, num_views):
        projs_arr = np.stack([np.asarray(p, dtype=np.float64).reshape(3, 4) for p in projs[:num_views]])
        jx = native.jac_pt(projs_arr[None], np.asarray(tri_3d_pt, dtype=np.float64).reshape(1, 4))
        return jx[0]

    def triangulate(self, projs, matched_pairs, damping_factor=None, iteration=None):
        if not damping_factor:
            damping_factor = self.damping_factor
        if not iteration:
            iteration = self.iteration
        num_projs = len(projs)
        num_views = len(matched_pairs)
        if num_projs != num_views:
            logging.warning('%s : the numbers of views and of projections are different, %d and %d',
                            self.__class__.__name__, num_views, num_projs)
            raise ValueError("different numbers of views and projections : {} - {}".format(num_views, num_projs))
        if num_projs < 2:
            logging.warning('%s : insufficient projections, %d', self.__class__.__name__, num_projs)
            raise ValueError("insufficient projections : {}".format(num_projs))
        # linear (tri:85) + nonlinear (tri:86) in one device call: the DLT points never visit the host
        uv, projs_arr = self._pack_views(projs, matched_pairs)
        return native.triangulate(projs_arr, uv, damping_factor, iteration)

    def triangulate_tracks(self, projs, pt_ptr, cam_idx, uv, init_3d_pts=None, damping_factor=None, iteration=None):
        """Every point from its OWN views (no reference counterpart: the reference triangulates rectangular batches only).
        Point i owns observations ``pt_ptr[i]:pt_ptr[i+1]`` of ``cam_idx`` (index into ``projs``) / ``uv`` (2, M), in the
        coordinates of ``projs``.  Linear then nonlinear when ``init_3d_pts`` is None, else nonlinear from it; returns the
        (4, n) points.  Per-point cost and status are ``native.tri_tracks``'s."""
        if not damping_factor:
            damping_factor = self.damping_factor
        if not iteration:
            iteration = self.iteration
        projs_arr = np.stack([np.asarray(p, dtype=np.float64).reshape(3, 4) for p in projs])
        mode = native.TRACKS_NONLINEAR if init_3d_pts is not None else native.TRACKS_LINEAR | native.TRACKS_NONLINEAR
        out, _cost, _status = native.tri_tracks(pt_ptr, cam_idx, uv, projs_arr, init_3d_pts, mode, damping_factor, iteration)
        return out

    def triangulate_tracks_robust(self, projs, pt_ptr, cam_idx, uv, max_reproj, min_angle_deg=1.5, max_hyp=128, cam_scale=None,
                                  init_3d_pts=None, damping_factor=None, iteration=3):
        """``triangulate_tracks`` for tracks that may hold wrong observations (``native.tri_tracks_ransac``; no reference
        counterpart): every pair of a track's observations (at most ``max_hyp``, evenly spaced) proposes a point, the
        proposal with the most observations within ``max_reproj`` wins, and the point is refitted over those.
        ``max_reproj`` is in the units of ``uv`` times ``cam_scale`` (V,); ``min_angle_deg`` is the smallest angle between
        the two generating rays (None: no gate).  ``init_3d_pts`` (4, n) is what an unsolved point keeps.  Returns
        ``(points (4, n), inlier (M,) bool, status (n,) of native.RANSAC_* bits)``."""
        if not damping_factor:
            damping_factor = self.damping_factor
        if not float(max_reproj) >= 0.0:
            raise ValueError("max_reproj must be >= 0, got {!r}".format(max_reproj))
        if min_angle_deg is not None and not 0.0 <= float(min_angle_deg) <= 180.0:
            raise ValueError("min_angle_deg must be in [0, 180] or None, got {!r}".format(min_angle_deg))
        cos_min_angle = 1.0 if min_angle_deg is None else math.cos(math.radians(float(min_angle_deg)))
        projs_arr = np.stack([np.asarray(p, dtype=np.float64).reshape(3, 4) for p in projs])
        out, inlier, _n, _best, status, _summary = native.tri_tracks_ransac(
            pt_ptr, cam_idx, uv, projs_arr, float(max_reproj) ** 2, cos_min_angle, max_hyp, damping_factor, iteration, cam_scale,
            init_3d_pts)
        return out, inlier.astype(bool), status

    @staticmethod
    def _pack_views(projs, matched_pairs):
        num_views = len(matched_pairs)
        num_pts = matched_pairs[0].shape[1]
        uv = np.empty((num_views, 2, num_pts), dtype=np.float64)
        for v in range(num_views):
            uv[v] = np.asarray(matched_pairs[v])[0:2, :]
        projs_arr = np.stack([np.asarray(p, dtype=np.float64).reshape(3, 4) for p in projs])
        return uv, projs_arr

    def linear_triangulate(self, projs, matched_pairs):
        """DLT triangulation (triangulation_processor.py:91-157) on the device: per point the null
        vector of the (2V x 4) system, divided by W.  Same sanity checks / prints / ``None`` returns."""
        if len(matched_pairs) != len(projs) != 2:       # sic: chained comparison of the reference (Q12)
            print('{}:{} - num of projs {} and matched pairs {} need to be 2'.format(
                self.__class__.__name__, 'linear_triangulate', len(projs), len(matched_pairs)))
            return None
        if matched_pairs[0].shape[1] != matched_pairs[1].shape[1]:
            print('{}:{} - matched pairs number does not match {} vs {}'.format(
                self.__class__.__name__, 'linear_triangulate',
                matched_pairs[0].shape[1], matched_pairs[1].shape[1]))
            return None
        uv, projs_arr = self._pack_views(projs, matched_pairs)
        return native.tri_linear(projs_arr, uv)


class HipTriangulationProcessor(HipTriangulationMixin):
    """Standalone TriangulationProcessor: constructor state of triangulation_processor.py:12-28."""

    def __init__(self, damping_factor=0.5, iteration=100):
        self.damping_factor = damping_factor
        self.iteration = iteration
        self.tri_pts = None

    def add_tri_pt(self, tri_pt):
        if not np.any(self.tri_pts):
            self.tri_pts = tri_pt
        else:
            self.tri_pts = np.hstack((self.tri_pts, tri_pt))


# ------------------------------------------------------------------------------------------------
class HipCamposeMixin:
    """Hot-path methods of CamposeProcessor (campose_processor.py:11-808)."""

    quirk_flags = native.QUIRKS_REFERENCE        # bug-compatible by default
    reproduce_q13 = True                         # the RANSAC winner the reference's LAPACK would have left standing (q13.py);
                                                 # False: the sane RANSAC (every hypothesis with its sign-invariant centre)
    ransac_last = None                           # diagnostics of the last RANSAC call

    def nonlinear_estimate_cam_pose_pnp(self, key_2d_pts, tri_3d_pts, intrinsic_mat,
                                        init_rot, init_loc, damping_factor=None, iteration=None):
        if not damping_factor:
            damping_factor = self.damping_factor
        if not iteration:
            iteration = self.iteration
        if key_2d_pts.shape[1] != tri_3d_pts.shape[1]:
            logging.warning('%s : different numbers of key points and of triangulated points',
                            self.__class__.__name__)
            raise ValueError("key pts num - triangulated pts num : {} - {}"
                             .format(key_2d_pts.shape[1], tri_3d_pts.shape[1]))
        rot, loc = native.pnp_nonlinear(key_2d_pts, tri_3d_pts, intrinsic_mat, init_rot, init_loc,
                                        damping_factor, iteration, self.quirk_flags)
        return rot, loc

    def construct_jacobian_matrix(self, rot, loc, pt_3d):
        jp, st = native.jac_cam(np.asarray(rot, dtype=np.float64).reshape(1, 3, 3),
                                np.asarray(loc, dtype=np.float64).reshape(1, 3),
                                np.asarray(pt_3d, dtype=np.float64).reshape(1, 4), self.quirk_flags)
        native.check(int(st[0]))
        return jp[0]

    def linear_estimate_cam_pose_pnp(self, key_2d_pts, tri_3d_pts, intrinsic_mat, ransac_config=None):
        """RANSAC 6-point DLT PnP (campose_processor.py:249-305, 485-633).  The six-point samples are drawn
        here with ``random.sample`` exactly as the reference does (same consumption of Python's global RNG
        stream, campose:531; ``sampling.sample_indices`` draws them in bulk); every hypothesis is solved and scored on the device."""
        inliers, rot, loc = self._linear_pnp(key_2d_pts, tri_3d_pts, intrinsic_mat, ransac_config)
        return inliers.tolist(), rot, loc

    def _check_pnp_input(self, key_2d_pts, tri_3d_pts):
        if key_2d_pts.shape[1] != tri_3d_pts.shape[1]:
            logging.warning('%s : different numbers of key points and of triangulated points',
                            self.__class__.__name__)
            raise ValueError("key pts num - triangulated pts num : {} - {}"
                             .format(key_2d_pts.shape[1], tri_3d_pts.shape[1]))
        num_pts = key_2d_pts.shape[1]
        if num_pts < 6:
            logging.warning('%s : required equal or more than six points %d', self.__class__.__name__, num_pts)
            raise ValueError("required equal or more than six points {}".format(num_pts))
        return num_pts

    def _q13_winner(self, key_2d_pts, tri_3d_pts, intrinsic_mat, samples, rots, locs, counts, counts_neg):
        """Quirk Q13 (q13.py): the device has solved and scored every hypothesis, under its centre C and under -C; which of
        the two the reference would have scored is its LAPACK's decision, asked of NumPy for the hypotheses that can still
        win.  Returns (rot, loc) of the reference's winner, or None when no hypothesis has an inlier."""
        kinv = np.linalg.inv(intrinsic_mat)

        def fires(h):
            idx = samples[h].tolist()
            return det_branch_fires(kinv @ key_2d_pts[:, idx], tri_3d_pts[:, idx])        # campose:532-535

        best, fired = reference_winner(counts, counts_neg, fires)
        self.ransac_last = {"hypothesis": best, "q13_fired": fired,
                            "sane_winner": int(np.argmax(counts)) if counts.max() > 0 else -1}
        if best < 0:
            return None
        return rots[best].copy(), (-locs[best] if fired else locs[best]).reshape(3, 1).copy()

    def _linear_pnp(self, key_2d_pts, tri_3d_pts, intrinsic_mat, ransac_config):
        """``linear_estimate_cam_pose_pnp`` with the inlier indices as an int array (the list the reference returns costs
        0.1 ms to build and 0.25 ms to turn back into an index at 5 000 inliers: ``estimate_cam_pose_pnp`` builds it once)."""
        if not ransac_config:
            ransac_config = self.ransac_config
        num_pts = self._check_pnp_input(key_2d_pts, tri_3d_pts)
        samples = sample_indices(num_pts, 6, ransac_config.iteration, as_array=True)       # = [random.sample(range(num_pts), 6) ...], campose:531
        if not self.reproduce_q13:
            rot, loc, inlier_indices, _best = native.pnp_linear_ransac(
                key_2d_pts, tri_3d_pts, intrinsic_mat, samples, ransac_config.inlier_threshold, as_array=True)
            return inlier_indices, rot, loc
        rots, locs, counts, counts_neg = native.pnp_ransac_evaluate(
            key_2d_pts, tri_3d_pts, intrinsic_mat, samples, ransac_config.inlier_threshold)
        won = self._q13_winner(key_2d_pts, tri_3d_pts, intrinsic_mat, samples, rots, locs, counts, counts_neg)
        if won is None:                                # no hypothesis has an inlier: the initial pose (campose:519-522)
            return np.empty(0, dtype=np.intp), np.identity(3), np.zeros((3, 1))
        rot, loc = won
        inlier_indices = native.pnp_inlier_mask(key_2d_pts, tri_3d_pts, intrinsic_mat, rot, loc, ransac_config.inlier_threshold,
                                                as_array=True)
        return inlier_indices, rot, loc

    def estimate_cam_pose_pnp(self, key_2d_pts, tri_3d_pts, intrinsic_mat,
                              ransac_config=None, damping_factor=None, iteration=None):
        if not ransac_config:
            ransac_config = self.ransac_config
        if not damping_factor:
            damping_factor = self.damping_factor
        if not iteration:
            iteration = self.iteration
        if self.reproduce_q13:
            # RANSAC evaluation and refinement around the host's choice of the winner, the view resident on the device in
            # between (sfm_pnp_ransac_begin / _finish): one upload of the keys and points, no host-side gather of the inliers
            num_pts = self._check_pnp_input(key_2d_pts, tri_3d_pts)
            samples = sample_indices(num_pts, 6, ransac_config.iteration, as_array=True)   # campose:531
            session, rots, locs, counts, counts_neg = native.pnp_ransac_begin(
                key_2d_pts, tri_3d_pts, intrinsic_mat, samples, ransac_config.inlier_threshold)
            try:
                won = self._q13_winner(key_2d_pts, tri_3d_pts, intrinsic_mat, samples, rots, locs, counts, counts_neg)
            except BaseException:
                native.pnp_session_destroy(session)
                raise
            if won is not None:
                sel, ref_rot, ref_loc = native.pnp_ransac_finish(session, won[0], won[1], ransac_config.inlier_threshold,
                                                                 damping_factor, iteration, self.quirk_flags)
                return sel.tolist(), ref_rot, ref_loc      # a list is the reference's return type (campose:246)
            native.pnp_session_destroy(session)
            sel, ini_rot, ini_loc = np.empty(0, dtype=np.intp), np.identity(3), np.zeros((3, 1))      # campose:519-522
        else:
            sel, ini_rot, ini_loc = self._linear_pnp(key_2d_pts, tri_3d_pts, intrinsic_mat, ransac_config)
        ref_rot, ref_loc = self.nonlinear_estimate_cam_pose_pnp(
            key_2d_pts[:, sel], tri_3d_pts[:, sel], intrinsic_mat,
            ini_rot, ini_loc, damping_factor, iteration)
        return sel.tolist(), ref_rot, ref_loc          # a list is the reference's return type (campose:246)

    def estimate_cam_pose_robust(self, key_2d_pts, tri_3d_pts, intrinsic_mat, max_reproj_px=4.0, max_hyp=128, iteration=None,
                                 damping_factor=None):
        """``estimate_cam_pose_pnp`` by calibrated three-point hypotheses (``native.resect_ransac``; no reference counterpart):
        every triple of the view's correspondences (at most ``max_hyp``, evenly spaced, no random number) proposes up to four
        poses, the pose with the most correspondences within ``max_reproj_px`` wins and is refitted over those.  The keys are
        normalised with ``inv(K)``; the pixel threshold scales the normalised residual by ``sqrt(|k[0, 0] k[1, 1]|)`` as
        ``screen_structure`` does.  Falsy ``iteration`` / ``damping_factor`` fall back to the processor's.  Returns what
        ``estimate_cam_pose_pnp`` returns -- inlier indices (a list), rot, loc (3, 1) -- with the identity at the origin and
        no inliers for a view without a model; ``resect_last`` keeps best_hyp, status and the summary."""
        if not damping_factor:
            damping_factor = self.damping_factor
        if not iteration:
            iteration = self.iteration
        if not float(max_reproj_px) >= 0.0:
            raise ValueError("max_reproj_px must be >= 0, got {!r}".format(max_reproj_px))
        key_2d_pts, tri_3d_pts = np.asarray(key_2d_pts, dtype=np.float64), np.asarray(tri_3d_pts, dtype=np.float64)
        if key_2d_pts.shape[1] != tri_3d_pts.shape[1]:
            raise ValueError("key pts num - triangulated pts num : {} - {}".format(key_2d_pts.shape[1], tri_3d_pts.shape[1]))
        num_pts = key_2d_pts.shape[1]
        intrinsic = np.asarray(intrinsic_mat, dtype=np.float64)
        uv = normalise_pixels(key_2d_pts, intrinsic)
        pts = np.ascontiguousarray(tri_3d_pts[0:3, :] / tri_3d_pts[3:4, :]) if tri_3d_pts.shape[0] == 4 else tri_3d_pts
        scale = math.sqrt(abs(float(intrinsic[0, 0]) * float(intrinsic[1, 1])))
        cams, inlier, _n, best, status, summary = native.resect_ransac(
            [0, num_pts], uv, pts, float(max_reproj_px) ** 2, max_hyp, damping_factor, iteration, self.quirk_flags,
            np.array([scale]))
        self.resect_last = {"hypothesis": int(best[0]), "status": int(status[0]), "summary": summary}
        rot = quaternion_to_rotation_unchecked(cams[0, 3:7])
        return np.flatnonzero(inlier).tolist(), rot, cams[0, 0:3].reshape(3, 1).copy()

    # ---- two-view initialisation (campose_processor.py:29-189) --------------------------------------------
    def extract_cam_pose_from_essential_mat(self, esse_mat):
        """(r1, r2, c1, c2) of campose_processor.py:29-100.  The set {r1, r2} x {c1, c2} is the reference's;
        which rotation is called r1 and which sign c1 carries follows LAPACK's singular-vector signs there and
        the device's Jacobi sweep here (the caller tries all four combinations, ba_processor.py:81-97)."""
        return native.pose_candidates(esse_mat)

    def evalulate_cam_pose_cheirality(self, proj_1, proj_2, tri_3d_pts):
        """Indices of the points in front of both cameras (campose_processor.py:133-189)."""
        mask, _counts, _best = native.cheirality(proj_1, np.asarray(proj_2)[np.newaxis], np.asarray(tri_3d_pts)[np.newaxis])
        return np.flatnonzero(mask[0]).tolist()

    def disambiguate_cam_pose_four(self, ref_proj, projs_four, tri_3d_pts_four):
        """(best_idx, most_valid_indices) of campose_processor.py:102-131: one device call for the four candidates."""
        mask, counts, best = native.cheirality(ref_proj, np.array(projs_four), np.array(tri_3d_pts_four))
        if counts[best] == 0:
            return 0, []
        return best, np.flatnonzero(mask[best]).tolist()

    def estimate_relative_pose_robust(self, matched_pairs, model, kind, K_left, K_right, inliers=None, min_angle_deg=2.0,
                                      min_parallax=8):
        """The pose of the right (query) view relative to the left (reference) view from a verified two-view model (one
        ``native.twoview_pose``; no reference counterpart): ``model`` is the fundamental matrix (``kind="fundamental"``)
        or the homography (``kind="homography"``) of ``matched_pairs`` ([ref_pts, que_pts], (2 or 3, n) pixel coordinates),
        ``inliers`` the indices of the matches that vote (None: all).  The four candidate poses are scored by the number of
        voting matches in front of both cameras, and the winner's matches that subtend at least ``min_angle_deg`` degrees
        are counted as its parallax.

        Returns ``rot, centre (3, 1), front_idx (a list), counts``: ``rot`` and ``centre`` in the convention of
        ``extract_cam_pose_from_essential_mat`` / ``ba_processor.py:81-97`` (projection ``K [rot^T | -rot^T centre]``).  The
        library's pose is (R, t) with ``X_right = R X_left + t`` and ``|t| = 1``; the conversion is ``rot = R^T`` and
        ``centre = -R^T t``.  Without a winner ``rot`` is the identity, ``centre`` zeros and the list empty.  ``counts`` is a
        dict: ``n_front``, ``n_parallax``, ``cand_front`` (4,), ``best_cand``, ``status`` (``native.POSE_*`` bits).
        ``pose_last`` keeps these, ``R``, ``t``, the plane normal, ``obs_front`` and the triangulated points ``X`` (3, n).
        ``min_angle_deg`` and ``min_parallax`` are the caller's options; the defaults (2 degrees, 8 matches) are common
        choices for an initial pair, not constants measured by this project."""
        if not 0.0 <= float(min_angle_deg) <= 90.0:
            raise ValueError("min_angle_deg must be in [0, 90], got {!r}".format(min_angle_deg))
        left = np.asarray(matched_pairs[0], dtype=np.float64)[0:2, :]
        right = np.asarray(matched_pairs[1], dtype=np.float64)[0:2, :]
        if left.shape != right.shape:
            raise ValueError("matched pairs of different sizes : {} - {}".format(left.shape[1], right.shape[1]))
        num = left.shape[1]
        mask = None
        if inliers is not None:
            mask = np.zeros(num, dtype=np.uint8)
            mask[np.asarray(inliers, dtype=np.int64)] = 1
        out = native.twoview_pose([0, num], left, right, [model], [kind], K_left, K_right, math.cos(math.radians(float(min_angle_deg))) ** 2,
                                  min_parallax, mask)
        return _pose_result(self, out, 0, 0, num)

    def refine_relative_pose(self, matched_pairs, rot, centre, K_left, K_right, inliers=None, iters=6, damping=0.0, max_px=2.0,
                             min_angle_deg=2.0):
        """A relative pose refined on the matches themselves (one ``native.twoview_refine``; no reference counterpart): damped
        Gauss-Newton on the Sampson distance in pixels over the five parameters of a calibrated pair, ``iters`` steps with
        the damping ``damping``, over the matches ``inliers`` indexes (None: all).  ``rot`` and ``centre`` are in the convention
        of ``estimate_relative_pose_robust`` in and out (``rot = R^T``, ``centre = -R^T t``); the baseline comes back with
        unit length.  The matches are then judged against the refined pose at ``max_px`` pixels and ``min_angle_deg``.

        Returns ``rot, centre (3, 1), rms_before, rms_after, inlier_idx, front_idx, info, status``: the RMS Sampson distance of
        the matches that counted before and after (NaN without a pass), the indices of all matches within ``max_px`` and of those
        in front of both cameras, ``info`` the (5, 5) matrix sum J^T J at the refined pose in its chart (three rotation and
        two baseline-direction parameters; the caller derives conditioning or a covariance from it) and ``status``
        (``native.REFINE_*`` bits).  With ``native.REFINE_KEPT_INPUT`` the pose that went in comes back.  ``refine_last`` keeps
        the whole result of the call."""
        if not 0.0 <= float(min_angle_deg) <= 90.0:
            raise ValueError("min_angle_deg must be in [0, 90], got {!r}".format(min_angle_deg))
        if not float(max_px) >= 0.0:
            raise ValueError("max_px must be >= 0, got {!r}".format(max_px))
        left = np.asarray(matched_pairs[0], dtype=np.float64)[0:2, :]
        right = np.asarray(matched_pairs[1], dtype=np.float64)[0:2, :]
        if left.shape != right.shape:
            raise ValueError("matched pairs of different sizes : {} - {}".format(left.shape[1], right.shape[1]))
        num = left.shape[1]
        mask = None
        if inliers is not None:
            mask = np.zeros(num, dtype=np.uint8)
            mask[np.asarray(inliers, dtype=np.int64)] = 1
        R, t = pose_from_reference_convention(rot, centre)
        out = native.twoview_refine([0, num], left, right, [R], [t], K_left, K_right, damping, iters, float(max_px) ** 2,
                                    math.cos(math.radians(float(min_angle_deg))) ** 2, mask)
        return _refine_result(self, out)

    similarity_last = None                       # what the last register_pair_points call returned from the device

    def register_pair_points(self, scene_pts, pair_pts, pair_rot=None, pair_centre=None, max_err=0.05, max_hyp=128, iteration=2,
                             rigid=False):
        """Chain a verified pair onto a scene (one ``native.similarity_ransac``; no reference counterpart): ``pair_pts``
        (3 or 4, n) are the points ``estimate_relative_pose_robust`` triangulated for the pair, in the pair's frame (the
        left camera at the origin, a baseline of length one), ``scene_pts`` (3 or 4, n) the scene's points of the same
        tracks.  The similarity ``scene ~ s A pair + t`` is estimated with correspondences farther than ``max_err`` (scene
        units) from their target counted as wrong.

        Returns ``s, A (3, 3), t (3, 1), inlier_idx (a list), rot, centre (3, 1)``: the last two are the pair's second
        camera (``pair_rot``, ``pair_centre`` in the reference's convention, projection ``K [rot^T | -rot^T centre]``; None:
        the identity at the origin, i.e. the pair's first camera) moved into the scene's frame, ``rot = A pair_rot`` and
        ``centre = s A pair_centre + t``.  Without a model ``s`` is 0, ``A`` and ``rot`` are the identity, ``t`` and ``centre``
        zeros and the list empty.  ``similarity_last`` keeps ``sim``, ``inlier``, ``n_inliers``, ``best_hyp``, ``status``."""
        scene_pts = np.asarray(scene_pts, dtype=np.float64)
        pair_pts = np.asarray(pair_pts, dtype=np.float64)
        if scene_pts.ndim != 2 or pair_pts.ndim != 2 or scene_pts.shape[0] not in (3, 4) or pair_pts.shape[0] not in (3, 4) \
                or scene_pts.shape[1] != pair_pts.shape[1]:
            raise ValueError("scene_pts and pair_pts must be (3 or 4, n), got {} and {}".format(scene_pts.shape, pair_pts.shape))
        if not float(max_err) >= 0.0:
            raise ValueError("max_err must be >= 0, got {!r}".format(max_err))
        n = pair_pts.shape[1]
        src, dst = np.ascontiguousarray(pair_pts[0:3]), np.ascontiguousarray(scene_pts[0:3])
        sim, inlier, n_inliers, best_hyp, status, _summary = native.similarity_ransac([0, n], src, dst, float(max_err) ** 2, max_hyp,
                                                                                       iteration, rigid)
        self.similarity_last = dict(sim=sim[0], inlier=inlier, n_inliers=int(n_inliers[0]), best_hyp=int(best_hyp[0]),
                                    status=int(status[0]))
        if status[0] & (native.SIMILARITY_TOO_FEW | native.SIMILARITY_NO_MODEL):
            return 0.0, np.eye(3), np.zeros((3, 1)), [], np.eye(3), np.zeros((3, 1))
        s, A, t = native.split_similarity(sim[0])
        rot = np.eye(3) if pair_rot is None else np.asarray(pair_rot, dtype=np.float64).reshape(3, 3)
        centre = np.zeros(3) if pair_centre is None else np.asarray(pair_centre, dtype=np.float64).reshape(3)
        return s, A, t.reshape(3, 1), np.flatnonzero(inlier).tolist(), A @ rot, (s * (A @ centre) + t).reshape(3, 1)

    @staticmethod
    def _rotation_edges(pair_results, who):
        """``edges (E, 2) int32, rel (E, 9), used``: the posed entries of ``pair_results`` as the edges of a view graph;
        ``used[e]`` is the entry of edge ``e``."""
        edges, rel, used = [], [], []
        for k, entry in enumerate(pair_results):
            if isinstance(entry, dict):
                if entry.get("best_cand", 0) < 0 or entry.get("status", 0) & native.POSE_NO_POSE:
                    continue
                ref, que, R = entry["ref"], entry["que"], entry["R"]
            else:
                ref, que, R = entry
            if R is None or not np.any(R):
                continue
            edges.append((int(ref), int(que)))
            rel.append(np.asarray(R, dtype=np.float64).reshape(9))
            used.append(k)
        if not edges:
            raise ValueError("{}: no pair with a pose".format(who))
        return np.array(edges, dtype=np.int32), np.array(rel), used

    def filter_view_graph(self, pair_results, n_views, max_loop_deg=5.0, min_ok=1, min_pct=0, keep_untested=False):
        """The triplet filter over the relative poses of verified pairs (one ``native.view_triplets``; no reference
        counterpart): around every triangle of the view graph the three relative rotations must compose to the identity
        within ``max_loop_deg``.  ``pair_results`` holds the entries ``average_rotations`` takes, and a pair without a pose is
        skipped exactly as there.  A pair is kept iff at least ``min_ok`` and ``min_pct`` per cent of its triangles are
        consistent; a pair in no triangle gets ``keep_untested``.

        Returns ``keep, verdict``: ``keep`` one bool per entry of ``pair_results`` (False without a pose) and ``verdict`` a
        dict with ``pairs`` (the index into ``pair_results`` of every edge), ``edge_keep``, ``n_tri``, ``n_ok``, ``kept_idx``
        (all per edge) and ``summary`` (a dict over ``native.TRIPLET_SUMMARY``).  ``triplets_last`` keeps it."""
        edges, rel, used = self._rotation_edges(pair_results, "filter_view_graph")
        verdict = self._filter_edges(edges, rel, used, n_views, max_loop_deg, min_ok, min_pct, keep_untested)
        keep = np.zeros(len(pair_results), dtype=bool)
        keep[np.asarray(used, dtype=np.int64)[verdict["kept_idx"]]] = True
        return keep, verdict

    def _filter_edges(self, edges, rel, used, n_views, max_loop_deg=5.0, min_ok=1, min_pct=0, keep_untested=False):
        """The verdict dict of ``filter_view_graph`` for the edges ``_rotation_edges`` made."""
        if not 0.0 <= float(max_loop_deg) < 90.0:
            raise ValueError("max_loop_deg must be in [0, 90), got {!r}".format(max_loop_deg))
        edge_keep, n_tri, n_ok, kept_idx, summary = native.view_triplets(
            n_views, edges, rel, max_loop_deg=float(max_loop_deg), min_ok=min_ok, min_pct=min_pct, keep_untested=int(bool(keep_untested)))
        verdict = dict(pairs=used, edge_keep=edge_keep.astype(bool), n_tri=n_tri, n_ok=n_ok, kept_idx=kept_idx,
                       summary=dict(zip(native.TRIPLET_SUMMARY, (int(v) for v in summary))))
        self.triplets_last = verdict
        return verdict

    def average_rotations(self, pair_results, n_views, root=0, max_angle_deg=5.0, max_hyp=128, iteration=2, triplets=None):
        """Absolute rotations of ``n_views`` views from the relative poses of their verified pairs (one
        ``native.rotation_average``; no reference counterpart).  ``pair_results`` holds one entry per pair: a triple
        ``(ref, que, R)`` with ``X_que = R X_ref + t``, or a dict ``initialise_pairs`` returned to which the caller added the
        view indices as ``"ref"`` and ``"que"``.  A pair without a pose (``R`` None or all zeros; a dict with
        ``best_cand < 0`` or ``native.POSE_NO_POSE``) is skipped.  An edge counts as consistent while its residual angle is at
        most ``max_angle_deg``; ``max_hyp`` spanning trees are scored and ``iteration`` refit rounds of two Gauss-Newton
        steps follow.  ``triplets`` is None or a dict of the options of ``filter_view_graph`` (``max_loop_deg``, ``min_ok``,
        ``min_pct``, ``keep_untested``): the filter runs first and the averaging sees the kept edges only.

        Returns ``rots, verdict``: ``rots`` is a list of ``n_views`` (3, 3) matrices in the reference's convention
        (``rot = R_v^T``, projection ``K [rot^T | -rot^T centre]``; the identity for ``root``, None for a view without a
        rotation) and ``verdict`` a dict with ``pairs`` (the index into ``pair_results`` of every edge), ``edge_inlier``,
        ``edge_cos``, ``view_status``, ``n_inliers``, ``best_hyp``, ``status`` and ``summary``.  With ``triplets`` the edges are
        still all posed pairs: an edge the filter dropped has ``edge_inlier`` False and ``edge_cos`` NaN, and
        ``verdict["triplets"]`` is the filter's verdict over the same edges.  ``rotation_last`` keeps it."""
        if not 0.0 <= float(max_angle_deg) < 90.0:
            raise ValueError("max_angle_deg must be in [0, 90), got {!r}".format(max_angle_deg))
        edges, rel, used = self._rotation_edges(pair_results, "average_rotations")
        filtered = None
        if triplets is not None:
            unknown = set(triplets) - {"max_loop_deg", "min_ok", "min_pct", "keep_untested"}
            if unknown:
                raise ValueError("average_rotations: unknown triplets options {!r}".format(sorted(unknown)))
            filtered = self._filter_edges(edges, rel, used, n_views, **triplets)
            kept = filtered["kept_idx"]
            if kept.size == 0:
                raise ValueError("average_rotations: the triplet filter kept no pair")
            all_edges, edges, rel = edges, edges[kept], rel[kept]
        R, edge_inlier, edge_cos, view_status, n_inliers, best_hyp, status, summary = native.rotation_average(
            n_views, edges, rel, root=root, max_angle_deg=float(max_angle_deg), max_hyp=max_hyp, iters=iteration, steps=2)
        has = (view_status & native.ROTAVG_UNREACHED) == 0 if not status & native.ROTAVG_NO_MODEL else np.zeros(int(n_views), dtype=bool)
        rots = [R[v].T.copy() if has[v] else None for v in range(int(n_views))]
        edge_inlier = edge_inlier.astype(bool)
        if filtered is not None:
            full_inlier, full_cos = np.zeros(all_edges.shape[0], dtype=bool), np.full(all_edges.shape[0], np.nan)
            full_inlier[kept], full_cos[kept] = edge_inlier, edge_cos
            edge_inlier, edge_cos = full_inlier, full_cos
        verdict = dict(pairs=used, edge_inlier=edge_inlier, edge_cos=edge_cos, view_status=view_status, n_inliers=n_inliers,
                       best_hyp=best_hyp, status=status, summary=summary)
        if filtered is not None:
            verdict["triplets"] = filtered
        self.rotation_last = verdict
        return rots, verdict

    def average_translations(self, pair_results, rots_or_R, n_views, root=0, max_angle_deg=5.0, rounds=8, edge_mask=None):
        """Positions of ``n_views`` views from the unit translations of their posed pairs and known rotations (one
        ``native.translation_average``; no reference counterpart).  ``pair_results`` holds the entries ``average_rotations``
        takes, with the translation: a quadruple ``(ref, que, R, t)`` or a dict of ``initialise_pairs`` with ``"ref"`` and
        ``"que"`` added; a pair without a pose (or without ``t``) is skipped exactly as there, so that the edges of the two calls
        are the same.  ``rots_or_R`` is the list ``average_rotations`` returned (``rot = R_v^T``, None without a rotation) or an
        array (V, 3, 3) of the library's ``R_v``.  ``edge_mask`` has one entry per EDGE (``edge_inlier`` of the rotation
        verdict): a zero leaves the edge out.  An edge counts as consistent while the angle between its direction and the
        baseline of the solution is at most ``max_angle_deg``; ``rounds`` reweighted solves follow the first, then a polish.

        Returns ``centres, verdict``: ``centres`` a list of ``n_views`` (3, 1) columns in the reference's convention (the
        camera centre in world coordinates; zeros for ``root``, None for a view without a position) and ``verdict`` a dict
        with ``pairs``, ``edge_inlier``, ``edge_cos``, ``edge_len``, ``view_status``, ``n_inliers``, ``status``, ``summary``
        and ``log``.  ``translation_last`` keeps it."""
        if not 0.0 <= float(max_angle_deg) < 90.0:
            raise ValueError("max_angle_deg must be in [0, 90), got {!r}".format(max_angle_deg))
        n_views = int(n_views)
        if isinstance(rots_or_R, np.ndarray):
            R = np.asarray(rots_or_R, dtype=np.float64).reshape(n_views, 3, 3)
        else:
            if len(rots_or_R) != n_views:
                raise ValueError("average_translations: {} rotations for {} views".format(len(rots_or_R), n_views))
            R = np.zeros((n_views, 3, 3))
            for v, rot in enumerate(rots_or_R):
                if rot is not None:
                    R[v] = np.asarray(rot, dtype=np.float64).reshape(3, 3).T
        edges, ts, used = [], [], []
        for k, entry in enumerate(pair_results):
            if isinstance(entry, dict):
                if entry.get("best_cand", 0) < 0 or entry.get("status", 0) & native.POSE_NO_POSE:
                    continue
                ref, que, Rel, t = entry["ref"], entry["que"], entry["R"], entry["t"]
            else:
                ref, que, Rel, t = entry
            if Rel is None or not np.any(Rel) or t is None:
                continue
            edges.append((int(ref), int(que)))
            ts.append(np.asarray(t, dtype=np.float64).reshape(3))
            used.append(k)
        if not edges:
            raise ValueError("average_translations: no pair with a pose")
        C, edge_inlier, edge_cos, edge_len, view_status, n_inliers, status, summary, log = native.translation_average(
            n_views, np.array(edges, dtype=np.int32), R, np.array(ts), edge_mask=edge_mask, root=root, max_angle_deg=float(max_angle_deg),
            rounds=rounds, polish=1)
        has = (view_status & native.TRANSAVG_UNREACHED) == 0 if not status & native.TRANSAVG_NO_MODEL else np.zeros(n_views, dtype=bool)
        centres = [C[v].reshape(3, 1).copy() if has[v] else None for v in range(n_views)]
        verdict = dict(pairs=used, edge_inlier=edge_inlier.astype(bool), edge_cos=edge_cos, edge_len=edge_len, view_status=view_status,
                       n_inliers=n_inliers, status=status, summary=summary, log=log)
        self.translation_last = verdict
        return centres, verdict

    def estimate_relative_pose_minimal(self, matched_pairs, K_left, K_right, max_px=2.0, max_hyp=128, refine_iters=6, min_angle_deg=2.0):
        """The relative pose of a calibrated pair straight from its matches (no reference counterpart): ONE
        ``native.essential_ransac`` (five-point hypotheses at ``max_px`` pixels of Sampson distance), then ONE
        ``native.twoview_pose`` with the winner's pixel matrix as a fundamental matrix and its inliers voting, then ONE
        ``native.twoview_refine`` of ``refine_iters`` Gauss-Newton steps over the matches in front, judged at ``max_px`` and
        ``min_angle_deg``.  ``matched_pairs`` is [ref_pts, que_pts], (2 or 3, n) pixel coordinates.

        Returns what ``refine_relative_pose`` returns, in the reference's convention: ``rot, centre (3, 1), rms_before,
        rms_after, inlier_idx, front_idx, info, status``.  Without a model or without a pose the refinement sees an empty
        mask and answers with ``native.REFINE_*`` bits; what the pose call left comes back.  ``essential_last`` keeps the
        result of the first call, ``pose_last`` and ``refine_last`` those of the other two."""
        if not 0.0 <= float(min_angle_deg) <= 90.0:
            raise ValueError("min_angle_deg must be in [0, 90], got {!r}".format(min_angle_deg))
        if not float(max_px) >= 0.0:
            raise ValueError("max_px must be >= 0, got {!r}".format(max_px))
        left = np.asarray(matched_pairs[0], dtype=np.float64)[0:2, :]
        right = np.asarray(matched_pairs[1], dtype=np.float64)[0:2, :]
        if left.shape != right.shape:
            raise ValueError("matched pairs of different sizes : {} - {}".format(left.shape[1], right.shape[1]))
        num = left.shape[1]
        cos2 = math.cos(math.radians(float(min_angle_deg))) ** 2
        ess = native.essential_ransac([0, num], left, right, K_left, K_right, float(max_px) ** 2, max_hyp)
        self.essential_last = _essential_entry(ess, 0, 0, num)
        posed = native.twoview_pose([0, num], left, right, ess["F"], [native.POSE_FROM_F], K_left, K_right, cos2, 1, ess["inlier"])
        _pose_result(self, posed, 0, 0, num)
        front = (posed["obs_front"] > 0).astype(np.uint8)
        if posed["best_cand"][0] < 0:
            front[:] = 0
        out = native.twoview_refine([0, num], left, right, posed["R"], posed["t"], K_left, K_right, 0.0, refine_iters, float(max_px) ** 2,
                                    cos2, front)
        return _refine_result(self, out)


class HipEpipolarMixin:
    """Eight-point RANSAC and essential-matrix extraction of ``EpipolarProcessor`` (epipolar_processor.py:22-95)
    on the device.  Expects ``self.ransac``; sets ``self.fund_mat`` / ``self.esse_mat`` as the reference does."""

    def determine_fundamental_mat(self, matched_pairs, ransac_config=None):
        cfg = self.ransac if ransac_config is None else ransac_config
        left, right = np.asarray(matched_pairs[0]), np.asarray(matched_pairs[1])
        rows = left.shape[1]
        if rows < 8:
            logging.error('%s : number of matched pairs needs equal or more than eight')
            raise ValueError("Insufficient matched pairs : {}".format(rows))
        # same consumption of Python's global RNG stream as epipolar:225 (no draw when rows == 8)
        samples = None if rows == 8 else sample_indices(rows, 8, cfg.iteration, as_array=True)
        fund, inliers, _best = native.fundamental_ransac(left, right, samples, cfg.inlier_threshold)
        self.fund_mat = fund
        return inliers

    def extract_essential_mat(self, left_intrinsic_mat, right_intrinsic_mat):
        self.esse_mat = native.essential_from_fundamental(self.fund_mat, left_intrinsic_mat, right_intrinsic_mat)

    @staticmethod
    def _twoview_sets(list_of_matched_pairs):
        """set_ptr, left (2, M), right (2, M) of a list of [ref_pts, que_pts] pairs ((2 or 3, n) pixel coordinates each)."""
        lefts = [np.asarray(mp[0], dtype=np.float64)[0:2, :] for mp in list_of_matched_pairs]
        rights = [np.asarray(mp[1], dtype=np.float64)[0:2, :] for mp in list_of_matched_pairs]
        for l, r in zip(lefts, rights):
            if l.shape != r.shape:
                raise ValueError("matched pairs of different sizes : {} - {}".format(l.shape[1], r.shape[1]))
        set_ptr = np.concatenate(([0], np.cumsum([l.shape[1] for l in lefts]))).astype(np.int32)
        left = np.ascontiguousarray(np.hstack(lefts)) if lefts else np.zeros((2, 0))
        right = np.ascontiguousarray(np.hstack(rights)) if rights else np.zeros((2, 0))
        return set_ptr, left, right

    def verify_matches(self, list_of_matched_pairs, max_sampson_px=2.0, max_hyp=128, iteration=2):
        """Geometric verification of several sets of matches in ONE device call (``native.twoview_ransac``; no reference
        counterpart): per set the fundamental matrix of its consistent subset under a Sampson distance of
        ``max_sampson_px`` pixels.  Returns one ``(F (3, 3) of Frobenius norm 1, inlier indices (a list), status)`` per set;
        a set without a model (fewer than nine matches, or no hypothesis with nine inliers) has a zero matrix and no
        inliers.  ``twoview_last`` keeps the hypotheses, statuses and the summary of the call."""
        if not float(max_sampson_px) >= 0.0:
            raise ValueError("max_sampson_px must be >= 0, got {!r}".format(max_sampson_px))
        set_ptr, left, right = self._twoview_sets(list_of_matched_pairs)
        F, inlier, _n, best, status, summary = native.twoview_ransac(set_ptr, left, right, float(max_sampson_px) ** 2, max_hyp,
                                                                     iteration)
        self.twoview_last = {"hypothesis": best.tolist(), "status": status.tolist(), "summary": summary}
        return [(F[s], np.flatnonzero(inlier[set_ptr[s]:set_ptr[s + 1]]).tolist(), int(status[s]))
                for s in range(set_ptr.shape[0] - 1)]

    def determine_fundamental_mat_robust(self, matched_pairs, max_sampson_px=2.0, max_hyp=128, iteration=2):
        """``determine_fundamental_mat`` by the robust two-view geometry (``native.twoview_ransac``; no reference
        counterpart): stratified eight-point hypotheses without a random number, scored by the Sampson distance in pixels,
        the winner refitted over its inliers.  Sets ``self.fund_mat`` to the matrix divided by ``F[2][2]``, as
        ``extract_essential_mat`` expects, and returns the inlier indices (a list); without a model ``fund_mat`` is left
        as it was and the list is empty.  ``twoview_last`` keeps hypothesis, status and the summary."""
        rows = np.asarray(matched_pairs[0]).shape[1]
        if rows < 8:
            logging.error('%s : number of matched pairs needs equal or more than eight')
            raise ValueError("Insufficient matched pairs : {}".format(rows))
        (F, inliers, status), = self.verify_matches([matched_pairs], max_sampson_px, max_hyp, iteration)
        last = self.twoview_last
        self.twoview_last = {"hypothesis": last["hypothesis"][0], "status": status, "summary": last["summary"]}
        if status & (native.TWOVIEW_TOO_FEW | native.TWOVIEW_NO_MODEL):
            return []
        self.fund_mat = F / F[2][2]
        return inliers

    def determine_homography_robust(self, matched_pairs, max_transfer_px=2.0, max_hyp=128, iteration=2):
        """The homography of one set of matches by the robust estimator (``native.homography_ransac``; no reference
        counterpart): stratified four-point hypotheses without a random number, scored by the transfer error in both
        images (``max_transfer_px`` pixels), the winner refitted over its inliers.  Sets ``self.homography`` (left to right)
        to the matrix divided by ``H[2][2]`` and returns the inlier indices (a list); without a model ``homography`` is
        left as it was and the list is empty.  ``homography_last`` keeps hypothesis, status and the summary."""
        if not float(max_transfer_px) >= 0.0:
            raise ValueError("max_transfer_px must be >= 0, got {!r}".format(max_transfer_px))
        set_ptr, left, right = self._twoview_sets([matched_pairs])
        H, inlier, _n, best, status, summary = native.homography_ransac(set_ptr, left, right, float(max_transfer_px) ** 2,
                                                                        max_hyp, iteration)
        self.homography_last = {"hypothesis": int(best[0]), "status": int(status[0]), "summary": summary}
        if status[0] & (native.HOMOGRAPHY_TOO_FEW | native.HOMOGRAPHY_NO_MODEL):
            return []
        self.homography = H[0] / H[0][2][2]
        return np.flatnonzero(inlier).tolist()

    def determine_essential_mat_robust(self, matched_pairs, K_left, K_right, max_sampson_px=2.0, max_hyp=128):
        """The essential matrix of one set of matches of a calibrated pair (``native.essential_ransac``; no reference
        counterpart): stratified five-point hypotheses without a random number, up to ten solutions each, scored by the
        Sampson distance in pixels; no refit.  Sets ``self.esse_mat`` to the canonical matrix (Frobenius norm 1) and
        ``self.fund_mat`` to its pixel matrix divided by ``F[2][2]``, and returns the inlier indices (a list); without a model
        both are left as they were and the list is empty.  ``essential_last`` keeps E, F (norm 1), hypothesis, root, the
        number of valid candidates, status and the summary."""
        if not float(max_sampson_px) >= 0.0:
            raise ValueError("max_sampson_px must be >= 0, got {!r}".format(max_sampson_px))
        set_ptr, left, right = self._twoview_sets([matched_pairs])
        out = native.essential_ransac(set_ptr, left, right, K_left, K_right, float(max_sampson_px) ** 2, max_hyp)
        self.essential_last = _essential_entry(out, 0, 0, left.shape[1])
        self.essential_last["summary"] = out["summary"]
        if out["status"][0]:
            return []
        self.esse_mat = out["E"][0]
        self.fund_mat = out["F"][0] / out["F"][0][2][2]
        return self.essential_last["inliers"]

    def classify_matches(self, list_of_matched_pairs, max_px=2.0, max_hyp=128, iteration=2, planar_ratio=0.8):
        """Both two-view models of several sets of matches and a verdict per set (no reference counterpart): ONE
        ``native.twoview_ransac`` call and ONE ``native.homography_ransac`` call over the same arrays, both at ``max_px``
        pixels (Sampson distance and transfer error).  Returns one dict per set: ``F`` and ``H`` (3, 3) of Frobenius norm 1
        (zeros without the model), ``F_inliers`` and ``H_inliers`` (lists of indices), ``F_status``, ``H_status`` and
        ``verdict``:
          ``"none"``        neither model stands;
          ``"degenerate"``  the homography stands and either the fundamental matrix does not, or
                            ``n_H >= planar_ratio * n_F`` of their inlier counts: the matches are explained by a plane or a
                            pure rotation, and the fundamental matrix is not to be trusted;
          ``"general"``     otherwise.
        ``planar_ratio`` is the caller's option; its default 0.8 is the value COLMAP uses for the same test
        (``max_H_inlier_ratio``), not a constant measured by this project.  ``twoview_last`` and ``homography_last`` keep
        the hypotheses, statuses and summaries of the two calls."""
        if not float(max_px) >= 0.0:
            raise ValueError("max_px must be >= 0, got {!r}".format(max_px))
        set_ptr, left, right = self._twoview_sets(list_of_matched_pairs)
        F, f_in, f_n, f_best, f_status, f_summary = native.twoview_ransac(set_ptr, left, right, float(max_px) ** 2, max_hyp, iteration)
        H, h_in, h_n, h_best, h_status, h_summary = native.homography_ransac(set_ptr, left, right, float(max_px) ** 2, max_hyp, iteration)
        self.twoview_last = {"hypothesis": f_best.tolist(), "status": f_status.tolist(), "summary": f_summary}
        self.homography_last = {"hypothesis": h_best.tolist(), "status": h_status.tolist(), "summary": h_summary}
        out = []
        for s in range(set_ptr.shape[0] - 1):
            lo, hi = set_ptr[s], set_ptr[s + 1]
            has_f, has_h = bool(f_best[s] >= 0), bool(h_best[s] >= 0)
            if not (has_f or has_h):
                verdict = "none"
            elif has_h and (not has_f or h_n[s] >= planar_ratio * f_n[s]):
                verdict = "degenerate"
            else:
                verdict = "general"
            out.append({"F": F[s], "H": H[s], "F_inliers": np.flatnonzero(f_in[lo:hi]).tolist(),
                        "H_inliers": np.flatnonzero(h_in[lo:hi]).tolist(), "F_status": int(f_status[s]),
                        "H_status": int(h_status[s]), "verdict": verdict})
        return out

    def initialise_pairs(self, list_of_matched_pairs, K, K_right=None, max_px=2.0, max_hyp=128, iteration=2, planar_ratio=0.8,
                         min_angle_deg=2.0, min_parallax=8, refine_iters=0, minimal=False):
        """Verdict and relative pose of several sets of matches (no reference counterpart): ``classify_matches`` and then ONE
        ``native.twoview_pose`` over all sets, every set posed from the model its verdict trusts with that model's inliers
        voting: F for ``"general"``, H for ``"degenerate"``; a ``"none"`` set is passed with an empty mask and comes back
        without a pose.  ``K`` is the intrinsic matrix of every left view and, unless ``K_right`` is given, of every right
        view.  Returns one dict per set: ``verdict``, ``kind``, ``R``, ``t`` (X_right = R X_left + t), ``rot``, ``centre`` (the
        reference's convention, see ``estimate_relative_pose_robust``), ``normal``, ``front`` (indices), ``n_front``,
        ``n_parallax``, ``cand_front``, ``best_cand``, ``status``, and the entries of ``classify_matches``.  A pair to start
        from has a pose, no ``native.POSE_NO_PARALLAX`` and the largest ``n_parallax``.  ``pose_last`` keeps the summary.

        With ``refine_iters > 0`` ONE ``native.twoview_refine`` follows over all sets, each pose refined on its matches in front
        (``obs_front > 0``) by that many Gauss-Newton steps and judged at ``max_px``; a set with ``native.POSE_NO_POSE`` or
        ``native.POSE_NO_PARALLAX`` is passed with an empty mask and comes back as it went in (after a pure rotation the
        baseline is not determined and the iteration would wander).  Every dict then also has ``R_refined``, ``t_refined``,
        ``rot_refined``, ``centre_refined``, ``F_refined`` (Frobenius norm 1, for guided matching), ``refine_inliers`` and
        ``refine_front`` (indices), ``refine_cost`` (before, after), ``refine_used`` and ``refine_status``
        (``native.REFINE_*`` bits); ``refine_last`` keeps the summary.

        With ``minimal=True`` the sets whose verdict is ``"general"`` take their model from ONE ``native.essential_ransac``
        over all sets at the same ``max_px`` and ``max_hyp`` (five-point hypotheses with the intrinsics) in place of the
        eight-point F: where that call has a model, its pixel matrix poses the set and its inliers vote, and the dict gains
        ``E``, ``E_inliers``, ``E_status``, ``E_hypothesis`` and ``E_root`` (``kind`` is then ``"essential"``); a general set
        without an essential model keeps its F.  The verdicts themselves do not change; ``essential_last`` keeps the summary."""
        if not 0.0 <= float(min_angle_deg) <= 90.0:
            raise ValueError("min_angle_deg must be in [0, 90], got {!r}".format(min_angle_deg))
        refine_iters = native._count("refine_iters", refine_iters)
        verdicts = self.classify_matches(list_of_matched_pairs, max_px, max_hyp, iteration, planar_ratio)
        set_ptr, left, right = self._twoview_sets(list_of_matched_pairs)
        ess = None
        if minimal:
            ess = native.essential_ransac(set_ptr, left, right, K, K if K_right is None else K_right, float(max_px) ** 2, max_hyp)
            self.essential_last = {"summary": ess["summary"], "status": ess["status"].tolist()}
        mask = np.zeros(left.shape[1], dtype=np.uint8)
        models, kinds, from_e = [], [], []
        for s, v in enumerate(verdicts):
            use_h = v["verdict"] == "degenerate"
            use_e = ess is not None and v["verdict"] == "general" and ess["status"][s] == 0
            from_e.append(use_e)
            kinds.append(native.POSE_FROM_H if use_h else native.POSE_FROM_F)
            models.append(ess["F"][s] if use_e else (v["H"] if use_h else v["F"]))
            if use_e:
                mask[set_ptr[s]:set_ptr[s + 1]] = ess["inlier"][set_ptr[s]:set_ptr[s + 1]]
            elif v["verdict"] != "none":
                mask[set_ptr[s] + np.asarray(v["H_inliers"] if use_h else v["F_inliers"], dtype=np.int64)] = 1
        out = native.twoview_pose(set_ptr, left, right, models, kinds, K, K if K_right is None else K_right,
                                  math.cos(math.radians(float(min_angle_deg))) ** 2, min_parallax, mask,
                                  outputs=("normal", "cand_front", "n_front", "n_parallax", "best_cand", "status", "obs_front", "summary"))
        self.pose_last = {"summary": out["summary"], "status": out["status"].tolist()}
        result = []
        for s, v in enumerate(verdicts):
            R, t = out["R"][s], out["t"][s]
            won = out["best_cand"][s] >= 0
            entry = dict(v)
            entry.update({"kind": "homography" if kinds[s] == native.POSE_FROM_H else "fundamental", "R": R, "t": t,
                          "rot": R.T.copy() if won else np.identity(3), "centre": (-R.T @ t).reshape(3, 1),
                          "normal": out["normal"][s], "front": np.flatnonzero(out["obs_front"][set_ptr[s]:set_ptr[s + 1]]).tolist(),
                          "n_front": int(out["n_front"][s]), "n_parallax": int(out["n_parallax"][s]),
                          "cand_front": out["cand_front"][s], "best_cand": int(out["best_cand"][s]), "status": int(out["status"][s])})
            if from_e[s]:
                e = _essential_entry(ess, s, set_ptr[s], set_ptr[s + 1])
                entry.update({"kind": "essential", "E": e["esse_mat"], "E_inliers": e["inliers"], "E_status": e["status"],
                              "E_hypothesis": e["hypothesis"], "E_root": e["root"]})
            result.append(entry)
        if refine_iters > 0:
            skip = native.POSE_NO_POSE | native.POSE_NO_PARALLAX
            front = (out["obs_front"] > 0).astype(np.uint8)
            for s in range(len(verdicts)):
                if out["status"][s] & skip:
                    front[set_ptr[s]:set_ptr[s + 1]] = 0
            ref = native.twoview_refine(set_ptr, left, right, out["R"], out["t"], K, K if K_right is None else K_right, 0.0, refine_iters,
                                        float(max_px) ** 2, math.cos(math.radians(float(min_angle_deg))) ** 2, front,
                                        outputs=("F", "cost", "n_used", "status", "obs_inlier", "obs_front", "summary"))
            self.refine_last = {"summary": ref["summary"], "status": ref["status"].tolist()}
            for s, entry in enumerate(result):
                entry.update(_refined_entry(ref, s, set_ptr[s], set_ptr[s + 1], entry["best_cand"] >= 0))
        return result


    def guided_matches(self, query, query_xy, ref, ref_xy, model, max_px=2.0, ratio=matching.RATIO, metric=native.MATCH_L2):
        """``guided_pairs`` over host arrays, for callers without a track store (no reference counterpart): ``query`` and
        ``ref`` are (n, dim) descriptor arrays (or ``native.DescriptorSet`` objects, which are left open), ``query_xy`` and
        ``ref_xy`` their (n, 2) key coordinates, ``model`` ``("fundamental", F)`` or ``("homography", H)`` with the reference
        view left and the query view right.  One ``native.match_guided`` at ``max_px`` pixels, then
        ``matching.filter_guided``.  Returns ``r_idx (1, n), q_idx (1, n)`` sorted by reference key; ``guided_last`` keeps
        the number of admitted reference keys per query."""
        if not float(max_px) >= 0.0:
            raise ValueError("max_px must be >= 0, got {!r}".format(max_px))
        kind, mat = _guided_model(model)
        own = []
        sets = []
        for d in (query, ref):
            if isinstance(d, native.DescriptorSet):
                sets.append(d)
            else:
                sets.append(native.DescriptorSet(metric, d))
                own.append(sets[-1])
        try:
            out = native.match_guided(sets[0], query_xy, [sets[1]], [ref_xy], [kind], [mat], float(max_px) ** 2,
                                      outputs=("best_idx", "best_dist", "second_dist", "mutual", "n_admitted"))
        finally:
            for s in own:
                s.close()
        self.guided_last = {"n_admitted": out["n_admitted"][0]}
        q, t = matching.filter_guided(out["best_idx"][0], out["best_dist"][0], out["second_dist"][0], out["mutual"][0], ratio)
        order = np.argsort(t, kind="stable")
        return t[order].reshape(1, -1).astype(int), q[order].reshape(1, -1).astype(int)


class HipEpipolarProcessor(HipEpipolarMixin):
    """Standalone EpipolarProcessor (constructor of epipolar_processor.py:13-20)."""

    def __init__(self, ransac_config):
        self.fund_mat = np.identity(3)
        self.esse_mat = np.identity(3)
        self.homography = np.identity(3)
        self.ransac = ransac_config


class RansacConfig:
    """Mirror of utils.RansacConfig (utils.py:129-174): iteration count raised to the confidence bound and
    Python's global RNG seeded with -1 on construction."""

    def __init__(self, inlier_threshold, subset_confidence, sample_confidence, sample_num, iteration,
                 is_use_seed=True):
        self.inlier_threshold = inlier_threshold
        self.subset_confidence = subset_confidence
        self.sample_confidence = sample_confidence
        self.sample_num = int(sample_num)
        self.iteration = int(iteration)
        self.random_seed = -1
        calc_iteration = math.log(1.0 - subset_confidence) / math.log(1.0 - math.pow(sample_confidence, sample_num))
        if calc_iteration > iteration:
            print('RANSAC : iteration increases from {} to {}'.format(iteration, calc_iteration))
            self.iteration = int(calc_iteration)
        if is_use_seed:
            import random
            random.seed(self.random_seed)


class HipCamposeProcessor(HipCamposeMixin):
    """Standalone CamposeProcessor (constructor of campose_processor.py:12-26)."""

    def __init__(self, ransac_config, damping_factor, iteration):
        self.ransac_config = ransac_config
        self.damping_factor = damping_factor
        self.iteration = iteration


# ------------------------------------------------------------------------------------------------
class _ResidentScene:
    """What the drop-in keeps between two BA calls of one processor: the device-resident problem and a host picture of
    what it holds (the track-table rows as of the last call, the key coordinates of every view, intrinsics, the poses and
    points of the last write-back), enough to decide what is NEW in the next call."""

    def __init__(self):
        self.prob = None
        self.tracker = ObservationTracker()      # self rows + per-view visibility as of the last call
        self.keys = KeyCache()                   # (n_keys, 2) pixel coordinates per view, converted once
        self.ks = []              # copies of view.k
        self.n_views = 0
        self.n_pts = 0
        self.pts_written = None   # (3, N) the points of the last write-back
        self.rots_written = None  # (V, 3, 3) / (V, 3): the poses of the last write-back (what view.rot / .loc hold if untouched)
        self.locs_written = None
        self.n_views_before = 0
        self.from_device = False  # the structure came from the tracker's device tables (ba_device_tracks): the host picture above is not kept
        self.retired_bytes = 0    # upload bytes of problems this scene has replaced
        self.cams_synced = False  # the device cameras are the views' poses as the last update left them (no iteration since)
        # (point, camera) pairs filter_structure has removed: the tracker keeps the uncut picture, a rebuild leaves them out
        self.culled_pt = np.empty(0, dtype=np.int64)
        self.culled_cam = np.empty(0, dtype=np.int64)
        self.loss_prob = None     # the problem ba_loss was last applied to, and what was applied (None: never, it runs plain)
        self.loss_applied = None

    def close(self):
        if self.prob is not None:
            self.retired_bytes += self.prob.upload_bytes
            self.prob.close()
            self.prob = None

    @property
    def upload_bytes(self):
        return self.retired_bytes + (self.prob.upload_bytes if self.prob is not None else 0)


class HipBaMixin:
    """``BaProcessor.__execute_bundle_adjustment`` (ba_processor.py:274-439) on the device.

    Reads ``self.view_processor.view_list`` (``.rot/.loc/.k/.key_pts[i].pt``),
    ``self.key_tracker.track_list[i].table``, ``self.tri_processor.tri_pts``, ``self.iteration``,
    ``self.damping_factor``; writes the refined poses back through ``view.update_cam_pose`` and the
    refined points into ``tri_pts[0:3, :]`` in place; prints the reference's DEBUG lines.

    The reference runs this after EVERY registered view, over all views and all points
    (ba_processor.py:267).  The scene therefore stays resident on the device between calls
    (``ba_resident``): each call diffs the observation list against what the device holds and uploads
    only what is new -- the new view's pose, the new points, the new observations (``sfm_ba_append``) --
    plus whatever pose or old point the caller changed since the last write-back.  (The reference re-derives every
    quaternion from ``view.rot`` at the start of a call, ba:285-288; for views whose ``rot`` / ``loc`` still hold what the
    last call wrote, that round trip q -> R(q) -> q(R) runs on the device, ``sfm_ba_rederive_quaternions``.)  If anything was REMOVED (an observation,
    a point, a view), an existing key -> point entry of a track table changed, or a view's key LIST or intrinsic matrix was
    replaced, the problem is rebuilt from scratch.  The pixel coordinates of a key are read ONCE, when its view's key list is
    first seen (``observations.KeyCache``): ``view.key_pts`` is treated as immutable -- the reference's front end never edits a
    ``cv2.KeyPoint`` after detection (view_processor.py) -- and a caller that does edit ``key_pts[i].pt`` in place has to call
    ``ba_release()`` (or hand the view a new list) for the edit to reach the device.  The track tables of a
    ``HipDeviceKeyTracker`` follow the same rule the other way round: ``track_list[i].table`` is a host picture of the device
    table, and a write into it is not propagated to the device (``HipDeviceKeyTrack``).
    ``ba_upload_bytes`` reports the PCIe bytes spent so far; ``ba_release()`` frees the device copy.

    ``ba_device_tracks = True`` (off by default; needs ``ba_resident`` and a ``HipDeviceKeyTracker`` as ``self.key_tracker``,
    anything else raises ``TypeError``) builds the observation list where the tracks already are: no ``track_list[v].table``
    is read, nothing is diffed or gathered on the host.  Each call makes sure the tracker's store holds every view's
    normalised key coordinates (computed on the host from the coordinates the tracker uploaded, once per view and again when
    ``view.k`` changes), has the device build the list (``TrackStore.build_observations``) and compare it with the resident
    structure (``BaProblem.sync_tracks``).  Then the DEVICE tables are the truth: a host-side replacement of
    ``track_list[v].table`` (its setter) is not seen.  The observation list is the same as the host path's in every case,
    but ``ba_last_action`` may be ``"append"`` or ``"reuse"`` where the host path conservatively says ``"create"``:
    ``ObservationTracker.diff`` rebuilds on a second key for an observed point and on key index 0 even when the list does
    not change, the device compares the lists themselves."""

    ba_quirk_flags = native.QUIRKS_REFERENCE
    ba_verbose = True          # the reference prints unconditionally (ba:418-439)
    ba_resident = True         # keep the problem on the device between calls (False: one sfm_ba_solve per call)
    ba_last_action = None      # "create" | "append" | "reuse" | "solve": what the last call did (diagnostics / tests)
    ba_device_tracks = False   # build the observation list from a HipDeviceKeyTracker's device tables (class docstring)
    ba_loss = None             # None | ("huber", px) | ("cauchy", px): robust loss of the resident adjustment (ba_loss_native)
    ba_solver = "dense"        # "dense": sfm_ba_iterate, S formed and factored | "pcg": sfm_ba_iterate_pcg, matrix-free (ba_pcg_native)
                               # | "lm": sfm_ba_minimize_pcg, the matrix-free route under Levenberg-Marquardt control
    ba_hold_views = None       # view indices held by the "pcg" / "lm" solvers (their rot / loc are left alone), None: every view moves
    ba_pcg_tol = 1e-10         # relative tolerance of the preconditioned residual
    ba_pcg_max_iters = 0       # CG iteration limit, 0: min(7 free views, 1000)
    ba_pcg_last = None         # the result object of the last iterate_pcg call (iters_done, cost, cg_iters, cg_rel, cg_status)
    ba_lm_ftol = 1e-8          # "lm": stop when an accepted step lowers the cost by no more than this share of it (0: off)
    ba_lm_xtol = 0.0           # "lm": stop when an accepted step is no longer than this share of the state's norm (0: off)
    ba_lm_gtol = 0.0           # "lm": stop when the gradient's largest entry is no larger than this (0: off)
    ba_lm_last = None          # the result object of the last minimize_pcg call (trials, accepted, stop, lam, cost, log)

    def ba_loss_native(self):
        """``ba_loss`` as the native ``(kind, delta)`` or None, without touching the device.  The pixel scale becomes
        delta = px / sqrt(|k[0, 0] k[1, 1]|) in the normalised coordinates the adjustment works in; a problem has ONE delta,
        so views whose focal scales differ by more than 1e-12 relative raise ``ValueError``, as does a malformed setting.
        ``BaProblem.set_loss`` has the semantics; it needs ``ba_resident`` (the one-shot ``sfm_ba_solve`` is plain least
        squares).  Applied whenever the resident problem is created or replaced and when the attribute changes; the
        default None never calls ``set_loss``.  Nothing in ``process()`` sets it."""
        if self.ba_loss is None:
            return None
        try:
            name, px = self.ba_loss
        except (TypeError, ValueError):
            raise ValueError("ba_loss must be None or (\"huber\" | \"cauchy\", pixels), got {!r}".format(self.ba_loss))
        if not isinstance(name, str) or name.lower() not in ("huber", "cauchy"):
            raise ValueError("ba_loss must name \"huber\" or \"cauchy\", got {!r}".format(name))
        if not self.ba_resident:
            raise TypeError("ba_loss needs ba_resident")
        kind, px = native.check_loss(name, px)
        scales = np.array([math.sqrt(abs(float(v.k[0, 0]) * float(v.k[1, 1]))) for v in self.view_processor.view_list])
        if scales.size == 0 or not np.all(np.isfinite(scales)) or not np.all(scales > 0.0):
            raise ValueError("ba_loss needs views with finite, non-zero focal scales")
        if np.max(np.abs(scales - scales[0])) > 1e-12 * scales[0]:
            raise ValueError("ba_loss needs one focal scale for all views (one delta per problem), got {} .. {}".format(
                scales.min(), scales.max()))
        return native.check_loss(kind, px / scales[0])

    def ba_pcg_native(self, view_num=None):
        """``ba_solver`` and ``ba_hold_views`` checked without touching the device or the views: None for the dense solver,
        else a one-element tuple with the mask (uint8 (view_num,), 1 = free; None when nothing is held or ``view_num`` is
        None).  ``ba_hold_views`` with the dense solver (``sfm_ba_iterate`` cannot hold a camera) and ``"pcg"`` without
        ``ba_resident`` raise ``TypeError``; a bad tolerance, limit or view index raises ``ValueError``.  ``"lm"`` follows the
        rules of ``"pcg"``, with ``damping_factor`` as the first damping and ``iteration`` as the number of trials
        (``ba_lm_options``)."""
        if self.ba_solver not in ("dense", "pcg", "lm"):
            raise ValueError("ba_solver must be \"dense\", \"pcg\" or \"lm\", got {!r}".format(self.ba_solver))
        if self.ba_solver == "dense":
            if self.ba_hold_views is not None:
                raise TypeError("ba_hold_views needs ba_solver = \"pcg\" or \"lm\" (the dense solver cannot hold a view)")
            return None
        if not self.ba_resident:
            raise TypeError("ba_solver = \"{}\" needs ba_resident".format(self.ba_solver))
        if self.ba_solver == "lm":
            native.check_lm(0, None, **self.ba_lm_options())
        else:
            native.check_pcg(0, self.damping_factor, self.iteration, None, self.ba_pcg_tol, self.ba_pcg_max_iters)
        if self.ba_hold_views is None or view_num is None:
            return (None,)
        idx = np.asarray(list(self.ba_hold_views), dtype=np.int64).ravel()
        if idx.size and (idx.min() < 0 or idx.max() >= view_num):
            raise ValueError("ba_hold_views: view index outside the {} views".format(view_num))
        mask = np.ones(view_num, dtype=np.uint8)
        mask[idx] = 0
        return (mask,)

    def ba_lm_options(self):
        """The options ``ba_solver = "lm"`` hands to ``BaProblem.minimize_pcg``: ``damping_factor`` as ``lambda0`` (the
        default bounds, widened where they would not hold it), ``iteration`` as ``max_trials``, the ``ba_lm_*`` tolerances
        and the ``ba_pcg_*`` settings of the inner solve."""
        lam0, dflt = float(self.damping_factor), native.LM_DEFAULTS
        return dict(lambda0=lam0, lambda_min=min(dflt["lambda_min"], lam0) if lam0 > 0 else dflt["lambda_min"],
                    lambda_max=max(dflt["lambda_max"], lam0), ftol=self.ba_lm_ftol, xtol=self.ba_lm_xtol, gtol=self.ba_lm_gtol,
                    cg_tol=self.ba_pcg_tol, cg_max_iters=self.ba_pcg_max_iters, max_trials=self.iteration,
                    quirks=self.ba_quirk_flags)

    def _ba_apply_loss(self, scene, loss):
        """Make the resident problem's loss what ``ba_loss`` asks for (``loss`` = ``ba_loss_native()``): one ``set_loss`` when
        the problem is new or the setting changed, none while a problem has only ever run plain."""
        applied = scene.loss_applied if scene.loss_prob is scene.prob else None
        if loss != applied:
            if loss is None:
                scene.prob.set_loss(native.LOSS_NONE)
            else:
                scene.prob.set_loss(*loss)
        scene.loss_prob, scene.loss_applied = scene.prob, loss

    def ba_release(self):
        scene = self.__dict__.pop("_hip_scene", None)
        if scene is not None:
            scene.close()

    @property
    def ba_upload_bytes(self):
        scene = self.__dict__.get("_hip_scene")
        return scene.upload_bytes if scene is not None else 0

    # ---- resident problem ---------------------------------------------------------------------------
    def _ba_sync_structure(self, views, tri_num, n_same, new_cams, init_tri_pts):
        """Bring the resident problem to the current observation list; returns it.  ``new_cams`` are the packed cameras of
        the views from ``n_same`` on (the first ``n_same`` are unchanged since the last write-back).

        The track tables are diffed incrementally (``observations.ObservationTracker``: only the entries that changed
        since the last call are looked at, ba:309's semantics preserved); pure growth becomes one ``sfm_ba_append``,
        anything else a rebuild."""
        scene = self.__dict__.get("_hip_scene")
        if scene is None:
            scene = self.__dict__["_hip_scene"] = _ResidentScene()
        view_num = len(views)
        n_old = scene.n_views_before = scene.n_views
        if self.ba_device_tracks:
            return self._ba_sync_device_tracks(scene, views, tri_num, n_same, new_cams, init_tri_pts)
        rows = [self.key_tracker.track_list[v].table[v, :] for v in range(view_num)]
        same_intrinsics = scene.prob is not None and not scene.from_device and view_num >= n_old and all(
            np.array_equal(views[v].k, scene.ks[v]) for v in range(n_old))
        grown = scene.tracker.diff(rows, tri_num) if same_intrinsics else None
        if grown is not None:
            cam_new, pt_new, key_new = grown
            if cam_new.shape[0] == 0 and view_num == n_old and tri_num == scene.n_pts:
                self.ba_last_action = "reuse"
                return scene
            try:
                uv_new = scene.keys.gather_normalised(views, cam_new, key_new)                  # ba:339-342, new keys only
                cams_app = new_cams[n_old - n_same:] if n_same <= n_old else pack_cameras(
                    np.stack([np.asarray(v.rot, dtype=np.float64) for v in views[n_old:]]),
                    np.stack([np.asarray(v.loc, dtype=np.float64).reshape(3) for v in views[n_old:]]))
                scene.prob.append(cams_app, init_tri_pts[:, scene.n_pts:tri_num], cam_new, pt_new, uv_new)
            except Exception:
                self.ba_release()          # the tracker has moved on, the device has not: start over on the next call
                raise
            self.ba_last_action = "append"
        else:
            scene.close()
            pt_ptr, cam_idx, _pt_idx, key_idx = remove_pairs(scene.tracker.reset(rows, tri_num),                # ba:309
                                                             scene.culled_pt, scene.culled_cam)
            uv_norm = scene.keys.gather_normalised(views, cam_idx, key_idx)
            scene.prob = native.BaProblem(view_num, pt_ptr, cam_idx, uv_norm)
            scene.pts_written = None
            scene.rots_written = scene.locs_written = None
            self.ba_last_action = "create"
        scene.from_device = False
        scene.ks = [np.array(v.k, dtype=np.float64, copy=True) for v in views]
        scene.n_views = view_num
        scene.n_pts = tri_num
        return scene

    def _ba_check_device_tracks(self):
        if not isinstance(self.key_tracker, HipDeviceKeyTracker):
            raise TypeError("ba_device_tracks needs a HipDeviceKeyTracker as key_tracker, not {}".format(
                type(self.key_tracker).__name__))
        if not self.ba_resident:
            raise TypeError("ba_device_tracks needs ba_resident")

    def _ba_sync_device_tracks(self, scene, views, tri_num, n_same, new_cams, init_tri_pts):
        """``_ba_sync_structure`` with ``ba_device_tracks``: the tracker's store builds the list, the device compares it with
        the resident structure (class docstring)."""
        kt = self.key_tracker
        store = kt._store
        view_num, n_old = len(views), scene.n_views
        if store is None or store.n_views < view_num:
            raise native.SfmHipError("ba_device_tracks: the device store holds %s views, the scene %d"
                                     % ("no" if store is None else store.n_views, view_num))
        norm = kt.__dict__.get("_norm_ks")                    # (store, per view: the k its normalised table was made with)
        if norm is None or norm[0] is not store:
            norm = kt.__dict__["_norm_ks"] = (store, [])
        ks = norm[1]
        for v in range(view_num):                             # ba:339-342 for all keys of a view, once per (view, k)
            k = np.asarray(views[v].k, dtype=np.float64)
            if v >= len(ks):
                ks.extend([None] * (v + 1 - len(ks)))
            if ks[v] is None or not np.array_equal(ks[v], k):
                store.set_normalised(v, normalise_pixels(kt._xy[v].T, k))
                ks[v] = k.copy()
        store.build_observations(view_num, tri_num)           # ba:309
        action = native.SYNC_REPLACED
        if scene.prob is not None and view_num >= n_old and tri_num >= scene.n_pts:
            try:
                cams_app = new_cams[n_old - n_same:] if n_same <= n_old else pack_cameras(
                    np.stack([np.asarray(v.rot, dtype=np.float64) for v in views[n_old:]]),
                    np.stack([np.asarray(v.loc, dtype=np.float64).reshape(3) for v in views[n_old:]]))
                action, _n_new = scene.prob.sync_tracks(store, cams_app, init_tri_pts[:, scene.n_pts:tri_num])
            except Exception:
                self.ba_release()
                raise
        if action == native.SYNC_REUSE:
            self.ba_last_action = "reuse"
        elif action == native.SYNC_GROWN:
            self.ba_last_action = "append"
        else:
            scene.close()
            scene.prob = native.BaProblem.from_tracks(store)
            scene.pts_written = None
            scene.rots_written = scene.locs_written = None
            self.ba_last_action = "create"
        scene.from_device = True
        if scene.tracker.rows:
            scene.tracker = ObservationTracker()              # the host picture is not kept on this path
        scene.n_views = view_num
        scene.n_pts = tri_num
        return scene

    def _ba_update_resident(self, views, init_rots, init_locs, init_tri_pts):
        """Bring the resident scene up to the caller's views, track tables and points (structure, cameras, points), uploading
        only what is new or changed; returns it.  On a failure the resident copy is dropped."""
        view_num, tri_num = len(views), init_tri_pts.shape[1]
        scene = self.__dict__.get("_hip_scene")
        # cameras the caller did not touch since the last write-back: their quaternion q(R(q)) (ba:285-288 after
        # ba:412) is re-derived on the device; only changed or new views are packed on the host and uploaded
        n_same = 0
        if scene is not None and scene.prob is not None and scene.rots_written is not None:
            n_old = min(scene.rots_written.shape[0], view_num)
            if np.array_equal(init_rots[:n_old], scene.rots_written[:n_old]) and np.array_equal(init_locs[:n_old], scene.locs_written[:n_old]):
                n_same = n_old
        new_cams = pack_cameras(init_rots[n_same:], init_locs[n_same:]) if n_same < view_num else np.zeros((0, 7))
        loss = self.ba_loss_native()          # (raises before anything reaches the device)
        scene = self._ba_sync_structure(views, tri_num, n_same, new_cams, init_tri_pts)
        prob = scene.prob
        try:
            self._ba_apply_loss(scene, loss)
            if self.ba_last_action == "create":
                prob.set_cameras(pack_cameras(init_rots, init_locs) if n_same else new_cams)
                prob.set_points(0, init_tri_pts)
            else:
                if n_same == view_num or (self.ba_last_action == "append" and n_same == scene.n_views_before):
                    if not scene.cams_synced:                     # (refine_structure has left them re-derived already)
                        prob.rederive_quaternions(0, n_same)      # appended cameras went up with sfm_ba_append
                else:
                    cams_all = pack_cameras(init_rots, init_locs) if n_same else new_cams
                    prob.set_cameras(cams_all)
                # points the caller did not touch since the last write-back are already on the device (bit for
                # bit what get_state returned); appended points went up with sfm_ba_append
                done = 0 if scene.pts_written is None else min(scene.pts_written.shape[1], tri_num)
                if scene.pts_written is None:
                    prob.set_points(0, init_tri_pts)          # no record of what the device holds: upload everything
                elif done and not np.array_equal(init_tri_pts[:, :done], scene.pts_written[:, :done]):
                    prob.set_points(0, init_tri_pts[:, :done])
        except Exception:
            self.ba_release()
            raise
        scene.cams_synced = True
        return scene

    def refine_structure(self, damping_factor=None, iteration=None, relinearize=False):
        """Structure-only refinement of the resident scene: every point from all its observations with the cameras held
        (``BaProblem.refine_points``), after the scene has been brought up to date exactly as ``execute_bundle_adjustment``
        does.  ``relinearize`` runs the DLT over each track first.  Writes ``tri_processor.tri_pts[0:3]`` in place, leaves
        the views alone and returns ``(cost (2, N), status (N,))``.  It is triangulation: falsy ``damping_factor`` /
        ``iteration`` fall back to ``tri_processor``'s.  Needs ``ba_resident``; nothing in ``process()`` calls it."""
        if not self.ba_resident:
            raise TypeError("refine_structure needs ba_resident")
        if self.ba_device_tracks:
            self._ba_check_device_tracks()
        if not damping_factor:
            damping_factor = self.tri_processor.damping_factor
        if not iteration:
            iteration = self.tri_processor.iteration
        views = self.view_processor.view_list
        tri_pts = self.tri_processor.tri_pts
        init_rots = np.stack([np.asarray(v.rot, dtype=np.float64) for v in views])
        init_locs = np.stack([np.asarray(v.loc, dtype=np.float64).reshape(3) for v in views])
        init_tri_pts = np.ascontiguousarray(tri_pts[0:3, :], dtype=np.float64)
        scene = self._ba_update_resident(views, init_rots, init_locs, init_tri_pts)
        mode = native.TRACKS_NONLINEAR | (native.TRACKS_LINEAR if relinearize else 0)
        try:
            cost, status = scene.prob.refine_points(damping_factor, iteration, mode)
            _cams, pts = scene.prob.get_state()
        except Exception:
            self.ba_release()
            raise
        scene.pts_written = pts
        scene.rots_written, scene.locs_written = init_rots, init_locs      # the poses the device cameras were brought up to
        tri_pts[0:3, :] = pts
        return cost, status

    def retriangulate_structure(self, max_reproj_px=4.0, min_angle_deg=1.5, max_hyp=128, iteration=3, damping_factor=None):
        """Robust re-triangulation of the resident scene (``BaProblem.retriangulate``), after it has been brought up to date
        exactly as ``refine_structure`` does: every point from the consistent subset of its own track -- the pair of
        observations whose point has the most observations within ``max_reproj_px`` (rays at least ``min_angle_deg`` apart;
        at most ``max_hyp`` pairs per track), refitted over those.  Thresholds convert as ``screen_structure``'s.  Writes
        ``tri_processor.tri_pts[0:3]`` in place, leaves the views and the track tables alone and returns the native report
        (``inlier``, ``n_inliers``, ``best_hyp``, ``status``, ``summary``; observations in the order of
        ``prob.structure()``).  A point without a model keeps its coordinates.  Falsy ``damping_factor`` falls back to
        ``tri_processor``'s.  Needs ``ba_resident``; nothing in ``process()`` calls it."""
        if self.ba_device_tracks:
            self._ba_check_device_tracks()
        if not damping_factor:
            damping_factor = self.tri_processor.damping_factor
        if max_reproj_px is None:
            raise ValueError("retriangulate_structure needs max_reproj_px")
        native.check_ransac(0, 0.0, 1.0, max_hyp, damping_factor, iteration)      # before anything reaches the device
        scene, max_err2, cos_min_angle, cam_scale = self._ba_screen_scene("retriangulate_structure", max_reproj_px, min_angle_deg, 0)
        try:
            report = scene.prob.retriangulate(max_err2, cos_min_angle, max_hyp, damping_factor, iteration, cam_scale)
            _cams, pts = scene.prob.get_state()
        except Exception:
            self.ba_release()
            raise
        scene.pts_written = pts
        self.tri_processor.tri_pts[0:3, :] = pts
        return report

    def refine_motion(self, iters=None, views=None, use_loss=True, damping_factor=None):
        """Motion-only refinement of the resident scene: every camera from all its resident observations with the points
        held (``BaProblem.refine_cameras``), after the scene has been brought up to date exactly as
        ``execute_bundle_adjustment`` does.  ``views``: the indices of the views to refine (None: all; the others are held
        through the mask).  ``use_loss``: reweight by ``ba_loss`` when one is set.  Falsy ``iters`` / ``damping_factor``
        fall back to ``self.iteration`` / ``self.damping_factor``.  Writes the poses back through ``view.update_cam_pose``
        as ``execute_bundle_adjustment`` does, leaves ``tri_pts`` alone and returns ``(cost (2, V), status (V,))``.
        Needs ``ba_resident``; nothing in ``process()`` calls it."""
        if not self.ba_resident:
            raise TypeError("refine_motion needs ba_resident")
        if self.ba_device_tracks:
            self._ba_check_device_tracks()
        if not damping_factor:
            damping_factor = self.damping_factor
        if not iters:
            iters = self.iteration
        view_list = self.view_processor.view_list
        view_num = len(view_list)
        mask = None
        if views is not None:
            idx = np.asarray(list(views), dtype=np.int64).ravel()
            if idx.size and (idx.min() < 0 or idx.max() >= view_num):
                raise ValueError("refine_motion: view index outside the {} views".format(view_num))
            mask = np.zeros(view_num, dtype=np.uint8)
            mask[idx] = 1
        init_rots = np.stack([np.asarray(v.rot, dtype=np.float64) for v in view_list])
        init_locs = np.stack([np.asarray(v.loc, dtype=np.float64).reshape(3) for v in view_list])
        init_tri_pts = np.ascontiguousarray(self.tri_processor.tri_pts[0:3, :], dtype=np.float64)
        scene = self._ba_update_resident(view_list, init_rots, init_locs, init_tri_pts)
        try:
            scene.cams_synced = False
            cost, status = scene.prob.refine_cameras(damping_factor, iters, self.ba_quirk_flags, bool(use_loss), mask,
                                                     want_cost=True, want_status=True)
            cams, pts, rots = scene.prob.get_state_rot()
        except Exception:
            self.ba_release()
            raise
        scene.pts_written = pts                        # (the points did not move: bit for bit what the device was given)
        scene.rots_written, scene.locs_written = rots, cams[:, 0:3].copy()
        for view_idx in range(view_num):
            view_list[view_idx].update_cam_pose(rots[view_idx].copy(), cams[view_idx, 0:3].reshape(3, 1).copy())
        return cost, status

    def resect_motion(self, max_reproj_px=4.0, max_hyp=128, iteration=3, damping_factor=None, views=None):
        """Robust resection of the resident cameras (``BaProblem.resect``), after the scene has been brought up to date
        exactly as ``refine_motion`` does: every camera from the consistent subset of its own resident observations -- the
        triple whose pose has the most observations within ``max_reproj_px`` (at most ``max_hyp`` triples per camera),
        refitted over those, the points held.  ``views``: the indices of the views to resect (None: all; the others are held
        and only judged).  The threshold converts as ``screen_structure``'s.  Writes the poses back through
        ``view.update_cam_pose`` as ``refine_motion`` does, leaves ``tri_pts`` and the track tables alone and returns the
        native report (``inlier`` in the order of ``prob.structure()``, ``n_inliers``, ``best_hyp``, ``status``, ``summary``).
        A camera without a model keeps its pose.  Falsy ``damping_factor`` falls back to ``self.damping_factor``.  Needs
        ``ba_resident``; nothing in ``process()`` calls it."""
        if not self.ba_resident:
            raise TypeError("resect_motion needs ba_resident")
        if self.ba_device_tracks:
            self._ba_check_device_tracks()
        if not damping_factor:
            damping_factor = self.damping_factor
        if max_reproj_px is None:
            raise ValueError("resect_motion needs max_reproj_px")
        native.check_resect(0, 0.0, max_hyp, damping_factor, iteration)      # before anything reaches the device
        view_list = self.view_processor.view_list
        mask = None
        if views is not None:
            idx = np.asarray(list(views), dtype=np.int64).ravel()
            if idx.size and (idx.min() < 0 or idx.max() >= len(view_list)):
                raise ValueError("resect_motion: view index outside the {} views".format(len(view_list)))
            mask = np.zeros(len(view_list), dtype=np.uint8)
            mask[idx] = 1
        scene, max_err2, _cos, cam_scale = self._ba_screen_scene("resect_motion", max_reproj_px, None, 0)
        try:
            scene.cams_synced = False
            report = scene.prob.resect(max_err2, max_hyp, damping_factor, iteration, self.ba_quirk_flags, mask, cam_scale)
            cams, pts, rots = scene.prob.get_state_rot()
        except Exception:
            self.ba_release()
            raise
        scene.pts_written = pts                        # (the points did not move: bit for bit what the device was given)
        scene.rots_written, scene.locs_written = rots, cams[:, 0:3].copy()
        for view_idx, view in enumerate(view_list):
            view.update_cam_pose(rots[view_idx].copy(), cams[view_idx, 0:3].reshape(3, 1).copy())
        return report

    def _ba_screen_scene(self, who, max_reproj_px, min_angle_deg, min_obs):
        """The resident scene brought up to date as ``refine_structure`` does, and the native arguments of a screening:
        (scene, max_err2, cos_min_angle, cam_scale)."""
        if not self.ba_resident:
            raise TypeError("{} needs ba_resident".format(who))
        if max_reproj_px is not None and not float(max_reproj_px) >= 0.0:
            raise ValueError("max_reproj_px must be >= 0 or None, got {!r}".format(max_reproj_px))
        if min_angle_deg is not None and not 0.0 <= float(min_angle_deg) <= 180.0:
            raise ValueError("min_angle_deg must be in [0, 180] or None, got {!r}".format(min_angle_deg))
        max_err2 = float("inf") if max_reproj_px is None else float(max_reproj_px) ** 2
        cos_min_angle = 1.0 if min_angle_deg is None else math.cos(math.radians(float(min_angle_deg)))
        native.check_screen(0, max_err2, cos_min_angle, min_obs, None)      # before anything reaches the device
        views = self.view_processor.view_list
        init_rots = np.stack([np.asarray(v.rot, dtype=np.float64) for v in views])
        init_locs = np.stack([np.asarray(v.loc, dtype=np.float64).reshape(3) for v in views])
        init_tri_pts = np.ascontiguousarray(self.tri_processor.tri_pts[0:3, :], dtype=np.float64)
        scene = self._ba_update_resident(views, init_rots, init_locs, init_tri_pts)
        # what the device holds now, so that the next call uploads nothing again (as refine_structure records it)
        scene.pts_written = init_tri_pts.copy()
        scene.rots_written, scene.locs_written = init_rots, init_locs
        cam_scale = np.array([math.sqrt(abs(float(v.k[0, 0]) * float(v.k[1, 1]))) for v in views])
        return scene, max_err2, cos_min_angle, cam_scale

    @staticmethod
    def _ba_screen_report(report):
        report.err_px = np.sqrt(report.err2)
        report.min_angle_deg = np.degrees(np.arccos(np.clip(report.min_cos, -1.0, 1.0)))
        return report

    def screen_structure(self, max_reproj_px=None, min_angle_deg=None, min_obs=2):
        """Judge the resident scene without changing it (``BaProblem.screen``), after it has been brought up to date exactly
        as ``refine_structure`` does: reprojection error and depth per observation, surviving observations and widest
        triangulation angle per point.  Returns the native report (``err2``, ``depth``, ``obs_flags``, ``min_cos``,
        ``pt_flags``, ``summary``; observations in the order of ``prob.structure()``) with ``err_px = sqrt(err2)`` and
        ``min_angle_deg`` added.  ``None`` switches a test off.

        The pixel threshold scales the normalised residual of view v by ``sqrt(|k[0, 0] k[1, 1]|)``: exact for square pixels
        without skew; for the UPENN intrinsics the test scenes use, the two focal lengths differ from it by 7e-6 relative.
        Neither the device state nor ``tri_pts``, the views or the track tables change.  Needs ``ba_resident``; nothing in
        ``process()`` calls it."""
        if self.ba_device_tracks:
            self._ba_check_device_tracks()
        scene, max_err2, cos_min_angle, cam_scale = self._ba_screen_scene("screen_structure", max_reproj_px, min_angle_deg, min_obs)
        try:
            return self._ba_screen_report(scene.prob.screen(max_err2, cos_min_angle, min_obs, cam_scale))
        except Exception:
            self.ba_release()
            raise

    def align_structure(self, point_idx, targets, max_err, max_hyp=128, iteration=2, rigid=False, apply=True):
        """Align the resident scene to ``targets`` (3, n) of its points ``point_idx`` (n,) -- surveyed control points, the
        points another reconstruction has for the same tracks -- by a robust similarity (``BaProblem.align``), after the scene
        has been brought up to date exactly as ``refine_structure`` does.  ``max_err`` is in the units of ``targets``.  With
        ``apply`` and a model the scene moves on the device, and ``tri_processor.tri_pts[0:3]`` and every view's pose are
        written back as ``resect_motion`` writes them; without, nothing changes.  Returns the native tuple ``(sim (13,),
        inlier (n,), n_inliers, best_hyp, status)``.  The cost of the scene is that of before; its covariances and the
        meaning of a damping factor are not (include/sfm_hip.h).  Needs ``ba_resident``; nothing in ``process()`` calls it."""
        if not self.ba_resident:
            raise TypeError("align_structure needs ba_resident")
        if self.ba_device_tracks:
            self._ba_check_device_tracks()
        if not float(max_err) >= 0.0:
            raise ValueError("max_err must be >= 0, got {!r}".format(max_err))
        native.check_similarity(float(max_err) ** 2, max_hyp, iteration, rigid)      # before anything reaches the device
        views = self.view_processor.view_list
        tri_pts = self.tri_processor.tri_pts
        init_rots = np.stack([np.asarray(v.rot, dtype=np.float64) for v in views])
        init_locs = np.stack([np.asarray(v.loc, dtype=np.float64).reshape(3) for v in views])
        init_tri_pts = np.ascontiguousarray(tri_pts[0:3, :], dtype=np.float64)
        scene = self._ba_update_resident(views, init_rots, init_locs, init_tri_pts)
        scene.pts_written = init_tri_pts.copy()
        scene.rots_written, scene.locs_written = init_rots, init_locs
        try:
            result = scene.prob.align(point_idx, targets, float(max_err) ** 2, max_hyp, iteration, rigid, apply)
            moved = bool(apply) and not result[4] & (native.SIMILARITY_TOO_FEW | native.SIMILARITY_NO_MODEL)
            if moved:
                scene.cams_synced = False
                cams, pts, rots = scene.prob.get_state_rot()
        except Exception:
            self.ba_release()
            raise
        if moved:
            scene.pts_written = pts
            scene.rots_written, scene.locs_written = rots, cams[:, 0:3].copy()
            tri_pts[0:3, :] = pts
            for view_idx, view in enumerate(views):
                view.update_cam_pose(rots[view_idx].copy(), cams[view_idx, 0:3].reshape(3, 1).copy())
        return result

    def filter_structure(self, max_reproj_px=4.0, min_angle_deg=1.5, min_obs=2):
        """``screen_structure``, then remove what failed from the resident scene on the device (``BaProblem.cull``): the
        observations whose reprojection error exceeds ``max_reproj_px`` or that lie behind their camera, and the points
        left with fewer than ``min_obs`` observations or with no pair of rays ``min_angle_deg`` apart.  Returns the report,
        which describes the scene before the cull (``obs_flags == 0`` marks what remains).

        ``tri_pts``, the views and the track tables stay as they are -- the reference's object model has no removed
        observation; a point that lost its track keeps its index and simply stops moving.  The removed (point, camera)
        pairs are remembered with the resident scene: later growth appends to the culled scene, a later rebuild leaves
        the pairs out, ``ba_release()`` forgets them.  Not available with ``ba_device_tracks`` (the device-built list
        would differ from the culled scene and replace it).  Needs ``ba_resident``; nothing in ``process()`` calls it."""
        if self.ba_device_tracks:
            raise TypeError("filter_structure does not support ba_device_tracks")
        scene, max_err2, cos_min_angle, cam_scale = self._ba_screen_scene("filter_structure", max_reproj_px, min_angle_deg, min_obs)
        try:
            pt_ptr, cam_idx, _uv = scene.prob.structure(want_uv=False)
            report = scene.prob.cull(max_err2, cos_min_angle, min_obs, cam_scale)
        except Exception:
            self.ba_release()
            raise
        gone = np.flatnonzero(report.obs_flags)
        if gone.size:
            pt_of = np.repeat(np.arange(pt_ptr.shape[0] - 1, dtype=np.int64), np.diff(pt_ptr))
            scene.culled_pt = np.concatenate((scene.culled_pt, pt_of[gone]))
            scene.culled_cam = np.concatenate((scene.culled_cam, cam_idx[gone].astype(np.int64)))
        return self._ba_screen_report(report)

    def structure_uncertainty(self, hold=(0, 1), scaled=True, use_loss=True, damping_factor=0.0):
        """How well the resident scene is determined (``BaProblem.covariance``), after it has been brought up to date exactly
        as ``screen_structure`` does.  ``hold``: the views whose poses fix the gauge -- by default the first two registered
        views, the pair whose relative pose the two-view initialisation fixes; with fewer than two held and no damping the
        system is singular and a ``ValueError`` names the view at which that showed.  Returns a namespace with
        ``cam_sigma`` (V,): standard deviation of a view's centre, sqrt(trace of the centre's 3x3), 0 for a held view;
        ``pt_sigma`` (N,): sqrt(trace Sigma_pp), 0 for a point without observations; both in world units, multiplied by
        ``sigma0`` when ``scaled`` (normalised image units otherwise cancel only for a unit-variance residual);
        ``sigma0`` (normalised image units), and the native report as ``cov``.  ``use_loss``: weight by ``ba_loss`` when one
        is set.  Nothing on the device, in ``tri_pts`` or in the views changes.  Needs ``ba_resident``."""
        if self.ba_device_tracks:
            self._ba_check_device_tracks()
        from types import SimpleNamespace
        views = self.view_processor.view_list
        idx = np.asarray(list(hold), dtype=np.int64).ravel()
        if idx.size and (idx.min() < 0 or idx.max() >= len(views)):
            raise ValueError("structure_uncertainty: held view outside the {} views".format(len(views)))
        scene, _e, _c, _s = self._ba_screen_scene("structure_uncertainty", None, None, 0)
        mask = np.ones(len(views), dtype=np.uint8)
        mask[idx] = 0
        try:
            cov = scene.prob.covariance(float(damping_factor), self.ba_quirk_flags, bool(use_loss), mask)
        except Exception:
            self.ba_release()
            raise
        if cov.pivot_camera is not None:
            raise ValueError("structure_uncertainty: the system is singular at view {} (hold at least two views)".format(cov.pivot_camera))
        sigma0 = math.sqrt(max(cov.sigma0_sq, 0.0))
        scale = sigma0 if scaled else 1.0
        cam_var = np.maximum(cov.cam_cov[:, 0, 0] + cov.cam_cov[:, 1, 1] + cov.cam_cov[:, 2, 2], 0.0)
        pt_var = np.maximum(cov.pt_cov[:, 0] + cov.pt_cov[:, 3] + cov.pt_cov[:, 5], 0.0)
        return SimpleNamespace(cam_sigma=scale * np.sqrt(cam_var), pt_sigma=scale * np.sqrt(pt_var), sigma0=sigma0, cov=cov)

    def execute_bundle_adjustment(self):
        if self.ba_device_tracks:
            self._ba_check_device_tracks()
        self.ba_loss_native()                         # a bad ba_loss (or one without ba_resident) stops here, before anything is read
        self.ba_pcg_native()                          # ... as does ba_hold_views with the dense solver, or "pcg" without ba_resident
        views = self.view_processor.view_list
        pcg = self.ba_pcg_native(len(views))
        held = np.zeros(len(views), dtype=bool) if pcg is None or pcg[0] is None else pcg[0] == 0
        tri_pts = self.tri_processor.tri_pts
        view_num = len(views)
        tri_num = tri_pts.shape[1]
        init_rots = np.stack([np.asarray(v.rot, dtype=np.float64) for v in views])                    # ba:287
        init_locs = np.stack([np.asarray(v.loc, dtype=np.float64).reshape(3) for v in views])         # ba:288
        init_tri_pts = np.ascontiguousarray(tri_pts[0:3, :], dtype=np.float64)                          # ba:292-294

        if self.ba_resident:
            scene = self._ba_update_resident(views, init_rots, init_locs, init_tri_pts)
            prob = scene.prob
            try:
                scene.cams_synced = False
                if pcg is None:
                    prob.iterate(self.damping_factor, self.iteration, self.ba_quirk_flags)
                elif self.ba_solver == "lm":
                    self.ba_lm_last = prob.minimize_pcg(pcg[0], **self.ba_lm_options())
                else:
                    self.ba_pcg_last = prob.iterate_pcg(self.damping_factor, self.iteration, self.ba_quirk_flags, pcg[0],
                                                        self.ba_pcg_tol, self.ba_pcg_max_iters)
                cams, pts, rots = prob.get_state_rot()                                             # ba:412 (validated on the device)
            except Exception:
                # the device state has advanced (or is invalid: a bad rotation) while tri_pts / the views keep the old
                # values; the reference re-reads them on every call (ba:292-294), so the next call must start from the
                # host state again: drop the resident copy rather than continue from diverged device points
                self.ba_release()
                raise
            scene.pts_written = pts
            scene.rots_written, scene.locs_written = rots, cams[:, 0:3].copy()
            if held.any():
                # a held view keeps its rot / loc; the device holds the quaternion packed from them, not q(R(q)) of a
                # written pose, so the next call packs and uploads the cameras again instead of re-deriving them
                scene.rots_written = rots.copy()
                scene.rots_written[held] = np.nan
        else:
            init_cam_poses = pack_cameras(init_rots, init_locs)
            rows = [self.key_tracker.track_list[v].table[v, :] for v in range(view_num)]
            pt_ptr, cam_idx, _pt_idx, key_idx = build_observations(rows, tri_num)                  # ba:309
            uv_norm = gather_normalised_keys(views, cam_idx, key_idx)                              # ba:339-342
            cams, pts = native.ba_solve(view_num, pt_ptr, cam_idx, uv_norm, init_cam_poses, init_tri_pts,
                                        self.damping_factor, self.iteration, self.ba_quirk_flags)
            rots = quaternions_to_rotations(cams[:, 3:7])                                          # ba:412 (validated)
            self.ba_last_action = "solve"

        for view_idx in range(view_num):                                                       # ba:409-413
            if not held[view_idx]:
                views[view_idx].update_cam_pose(rots[view_idx].copy(), cams[view_idx, 0:3].reshape(3, 1).copy())
        tri_pts[0:3, :] = pts                                                                  # ba:415-416

        if self.ba_verbose:                                                                    # ba:418-439
            from scipy.spatial.transform import Rotation
            # (the reference converts its packed quaternions back: R(q(R)) == R to rounding; all views in two calls --
            # one Rotation object per view costs ~0.1 ms each, more than the device spends on a small scene)
            init_angles = Rotation.from_matrix(init_rots).as_euler('zyx', degrees=True).reshape(view_num, 3)
            refi_angles = Rotation.from_matrix(np.stack([quaternion_to_rotation_unchecked(cams[v, 3:7]) for v in range(view_num)])
                                               ).as_euler('zyx', degrees=True).reshape(view_num, 3)
            for view_idx in range(view_num):
                diff_loc = math.sqrt(np.sum(np.square(init_locs[view_idx] - cams[view_idx, 0:3])))
                print('DEBUG: {}-th view loc distance changes {} unit'.format(view_idx, diff_loc))
                print('DEBUG: {}-th view angles changes {} degree'.format(view_idx, np.abs(init_angles[view_idx] - refi_angles[view_idx])))
            moved = np.sqrt(np.sum(np.square(init_tri_pts - pts), axis=0))
            for tri_idx in np.flatnonzero(moved >= 5):
                print('DEBUG: {}-th pt loc changes more than 5 unit, {} unit'.format(tri_idx, moved[tri_idx]))

    # the reference calls the name-mangled private method (ba_processor.py:267)
    _BaProcessor__execute_bundle_adjustment = execute_bundle_adjustment


class HipBaProcessor(HipBaMixin):
    """Standalone BaProcessor (ba_processor.py:22-270): the constructor state, the bundle adjustment of ``HipBaMixin`` and
    the incremental state machine ``process(img, k)`` from pixels to poses, on the drop-ins of this module
    (``HipViewProcessor``, ``HipKeyTracker`` or ``HipDeviceKeyTracker``, ``HipEpipolarProcessor``,
    ``HipTriangulationProcessor``, ``HipCamposeProcessor``); no OpenCV is involved.  With the reference's own classes use
    ``class BaProcessor(HipBaMixin, ba_processor.BaProcessor)`` instead, which keeps the reference's ``process``."""

    def __init__(self, view_processor, key_tracker, epi_processor, tri_processor, campose_processor,
                 filter_size=10, iteration=3, damping_factor=5):
        self.curr_data_idx = 0
        self.filter_size = filter_size
        self.iteration = iteration
        self.damping_factor = damping_factor
        self.view_processor = view_processor
        self.key_tracker = key_tracker
        self.epi_processor = epi_processor
        self.tri_processor = tri_processor
        self.campose_processor = campose_processor

    def process(self, img, k):
        """One frame of ba_processor.py:43-270: detect, match into the key tracks, then by the number of views so far
        -- the first view only becomes valid; the second gets its pose from the essential matrix and seeds the point
        cloud; every later one is registered by PnP against view 0's points, adds the points it shares with view 0 and
        ends in a bundle adjustment over everything.  Prints, ``curr_data_idx``, ``ref_idx`` / ``is_valid`` and the two
        ``sys.exit`` conditions are the reference's; its BA_DEBUG block (cv2.solvePnPRansac) is not ported."""
        if self.curr_data_idx >= self.filter_size:
            print('Bundle Adjustment processor is full')
            return
        idx = self.curr_data_idx
        view = self.view_processor.generate_view(img, idx, k)                             # ba:49
        self.key_tracker.add_new_view(view, self.view_processor.view_list)                # ba:52
        self.view_processor.add_view(view)                                                # ba:55
        views = self.view_processor.view_list
        if idx == 0:
            print('In one image state')
            views[0].is_valid = True
        elif idx == 1:
            print('In epipolar state')
            self._process_two_view(views, k)
        else:
            print('In cam pose state')
            self._process_register(views, idx)
        self.curr_data_idx += 1                                                           # ba:270

    def _process_two_view(self, views, k):
        """ba:66-132: views 0 and 1 from their matches alone."""
        kt, tp, cp, ep = self.key_tracker, self.tri_processor, self.campose_processor, self.epi_processor
        pairs, r_idx, q_idx = kt.generate_matched_pairs(0, 1, views)
        ep.determine_fundamental_mat(pairs)
        ep.extract_essential_mat(views[0].k, views[1].k)
        r1, r2, c1, c2 = cp.extract_cam_pose_from_essential_mat(ep.esse_mat)
        rots, locs = [r1, r1, r2, r2], [c1, c2, c1, c2]                                   # ba:83-89: the four (R, C) combinations
        projs = [k @ np.hstack((r.T, -r.T @ c)) for r, c in zip(rots, locs)]
        ref_proj = views[0].cam_proj
        candidates = [tp.linear_triangulate([ref_proj, p], pairs) for p in projs]         # ba:93-96
        best, valid = cp.disambiguate_cam_pose_four(ref_proj, projs, candidates)
        views[1].update_cam_pose(rots[best], locs[best])
        valid = np.array(valid)[np.newaxis, :]                                            # ba:109-110
        in_front = [np.take_along_axis(pairs[0], valid, axis=1), np.take_along_axis(pairs[1], valid, axis=1)]
        pts = tp.nonlinear_triangulate(np.take_along_axis(candidates[best], valid, axis=1), [ref_proj, projs[best]], in_front)
        tri_idx = np.arange(0, pts.shape[1], dtype=int)[np.newaxis, :]
        kt.track_list[0].update_usage(np.take(r_idx, valid), tri_idx)                     # ba:120-125
        kt.track_list[1].update_usage(np.take(q_idx, valid), tri_idx)
        views[1].is_valid = True
        views[1].ref_idx = 0
        tp.add_tri_pt(pts)

    def _process_register(self, views, idx):
        """ba:140-267: pose of view ``idx`` by PnP on the points its reference view already has, new points from the
        matches that have none yet, bundle adjustment."""
        import sys
        kt, tp, cp = self.key_tracker, self.tri_processor, self.campose_processor
        cur = views[idx]
        ref = kt.find_best_view(idx)
        ref_view = views[ref]
        cur.ref_idx = ref
        pairs, ref_key, _cur_key = kt.generate_matched_pairs(ref, idx, views)
        ref_track = kt.track_list[ref]
        built_key, built_pt = ref_track.extract_constructed_points()
        if built_key.shape[1] != tp.tri_pts.shape[1]:                                     # ba:172-174
            sys.exit('ERROR: even best_view_idx assumption does not work !!!')
        used, in_pairs, in_built = np.intersect1d(ref_key, built_key, return_indices=True)
        used = used[np.newaxis, :]
        in_pairs, in_built = in_pairs[np.newaxis, :], in_built[np.newaxis, :]
        known = np.take_along_axis(tp.tri_pts, np.take_along_axis(built_pt, in_built, axis=1), axis=1)
        seen = np.take_along_axis(pairs[1], in_pairs, axis=1)
        _inliers, rot, loc = cp.estimate_cam_pose_pnp(seen, known, cur.k)                # ba:191-192
        cur.update_cam_pose(rot, loc)
        cur.is_valid = True

        free = ref_track.extract_unconstructed_points()
        projs = [ref_view.cam_proj, cur.cam_proj]
        fresh, in_pairs, _ = np.intersect1d(ref_key, free, return_indices=True)           # ba:229-230
        fresh = fresh[np.newaxis, :]
        both, _, _ = np.intersect1d(fresh, used, return_indices=True)
        if np.any(both) != False:                                                         # noqa: E712  (sic, ba:235-237)
            sys.exit('ERROR: the intersect of unused and used inters sets is NOT empty')
        in_pairs = in_pairs[np.newaxis, :]
        new_pts = tp.triangulate(projs, [np.take_along_axis(pairs[0], in_pairs, axis=1),
                                         np.take_along_axis(pairs[1], in_pairs, axis=1)])
        first = tp.tri_pts.shape[1]
        tri_idx = np.arange(first, first + new_pts.shape[1], dtype=int)[np.newaxis, :]
        ref_track.update_usage(fresh, tri_idx)                                            # ba:252-253
        kt.track_list[idx].update_usage(np.take(ref_track.table[idx, :], fresh), tri_idx)    # ba:256-258
        tp.add_tri_pt(new_pts)
        self._BaProcessor__execute_bundle_adjustment()                                    # ba:267


# ------------------------------------------------------------------------------------------------
INVALID_MATCH_VAL = NOT_USED_TRI_VAL = -1          # key_tracker.py:8


class HipKeyTrackerMixin:
    """``KeyTracker.__extend_list`` (key_tracker.py:213-317) with the brute-force matching on the device.

    Reads ``self.key_type`` / ``is_cross_check`` / ``track_list`` and ``view.key_pts`` / ``view.key_descriptors``;
    writes the ``KeyTrack.table`` rows the reference writes.  Every view's descriptors stay resident on the device
    (one ``native.DescriptorSet`` per view index) and are uploaded again only when the view's ``key_descriptors``
    object is another one, so a new view uploads only itself.  The new view is matched against all earlier views in
    one launch; the ratio / crossCheck filter, the duplicate removal (quirk Q14), the optional fundamental-matrix
    inliers (``HipEpipolarProcessor``, per reference view in the reference's order: Python's global RNG stream is
    consumed identically; quirk Q15) and the table writes run on the host (``matching.py``).
    ``kt_upload_bytes`` reports the descriptor bytes uploaded so far; ``kt_release()`` frees the device copies."""

    def kt_release(self):
        sets = self.__dict__.pop("_hip_desc", None)
        for _obj, ds in (sets or {}).values():
            ds.close()

    @property
    def kt_upload_bytes(self):
        return self.__dict__.get("_hip_desc_bytes", 0)

    def _kt_metric(self):
        return native.MATCH_L2 if self.key_type in ['sift', 'surf'] else native.MATCH_HAMMING    # key_tracker.py:82-85

    def _kt_set(self, idx, descriptors):
        sets = self.__dict__.setdefault("_hip_desc", {})
        have = sets.get(idx)
        if have is not None and have[0] is descriptors:
            return have[1]
        if have is not None:
            have[1].close()
        ds = native.DescriptorSet(self._kt_metric(), descriptors)
        sets[idx] = (descriptors, ds)
        self.__dict__["_hip_desc_bytes"] = self.__dict__.get("_hip_desc_bytes", 0) + ds.upload_bytes
        return ds

    def _extend_list(self, new_view, views, is_knn_match=False, is_fund_inlier=False, ransac_config=None):
        key_num = len(new_view.key_pts)
        new_track_idx = len(self.track_list)
        refs = []
        for ref_idx, ref_view in enumerate(views):
            d = ref_view.key_descriptors
            if d is None or len(d) == 0:      # undefined without cv2 (deviation of Q16)
                raise ValueError("reference view {} has no descriptors".format(ref_idx))
            refs.append(self._kt_set(ref_idx, d))
        query = self._kt_set(new_track_idx, new_view.key_descriptors)
        mode = matching.match_mode(is_knn_match, self.is_cross_check)
        if refs and query.n:
            nn = native.match(query, refs, mode)
        else:
            empty_i = np.full((len(refs), 0), -1, dtype=np.int32)
            empty_f = np.zeros((len(refs), 0), dtype=np.float32)
            nn = (empty_i, empty_f, empty_i, empty_f, np.zeros((len(refs), 0), dtype=bool))

        for track in self.track_list:                                           # key_tracker.py:236-237
            track.expand_table()
        new_track = type(self.track_list[0])(len(self.track_list) + 1, key_num, new_track_idx)   # key_tracker.py:240

        keys = KeyCache() if is_fund_inlier else None
        all_views = list(views) + [new_view]
        for ref_idx in range(len(refs)):                                        # key_tracker.py:247
            q, t, d = matching.filter_matches(nn[0][ref_idx], nn[1][ref_idx], nn[2][ref_idx], nn[3][ref_idx], nn[4][ref_idx],
                                              is_knn_match, self.is_cross_check)
            n_in = None
            if is_fund_inlier:                                                  # key_tracker.py:294-299
                qk, tk, _dk = matching.dedup_matches(q, t, d)
                ref_pts = np.ones((3, tk.shape[0])); que_pts = np.ones((3, qk.shape[0]))
                ref_pts[0:2] = keys.keys(all_views, ref_idx)[tk].T
                que_pts[0:2] = keys.keys(all_views, len(views))[qk].T
                ep = HipEpipolarProcessor(ransac_config)
                n_in = len(ep.determine_fundamental_mat([ref_pts, que_pts], ransac_config))
            wq, wt = matching.table_writes(q, t, d, n_in)
            self.track_list[ref_idx].table[new_track_idx, wt] = wq              # key_tracker.py:313
            new_track.table[ref_idx, wq] = wt                                   # key_tracker.py:314
        self.track_list.append(new_track)

    # the reference calls the name-mangled private method (key_tracker.py:126)
    def _KeyTracker__extend_list(self, new_view, views, is_knn_match=False, is_fund_inlier=False, ransac_config=None):
        return self._extend_list(new_view, views, is_knn_match, is_fund_inlier, ransac_config)


class HipKeyTrack:
    """Mirror of key_tracker.KeyTrack (key_tracker.py:14-59)."""

    def __init__(self, rows, cols, idx):
        self.table = np.empty((rows, cols), dtype='int')
        self.table.fill(INVALID_MATCH_VAL)
        self.idx = idx
        self.key_num = cols

    def expand_table(self):
        arr = np.full((1, self.key_num), INVALID_MATCH_VAL, dtype='int')
        self.table = np.append(self.table, arr, 0)

    def update_usage(self, used_indices, tri_indices):
        # for (i, j), val in ndenumerate(used_indices): table[idx, val] = tri_indices[0, j]  (used_indices is 2-D)
        used = np.asarray(used_indices)
        self.table[self.idx, used.reshape(-1)] = np.asarray(tri_indices)[0, np.indices(used.shape)[1].reshape(-1)]

    def extract_unconstructed_points(self):
        return np.asarray(np.where(self.table[self.idx, :] == NOT_USED_TRI_VAL))

    def extract_constructed_points(self):
        indices = np.asarray(np.where(self.table[self.idx, :] != NOT_USED_TRI_VAL))
        return indices, np.take(self.table[self.idx, :], indices)


class HipKeyTracker(HipKeyTrackerMixin):
    """Standalone KeyTracker (key_tracker.py:63-344) without cv2: the constructor's fields, ``add_new_view``,
    ``generate_matched_pairs``, ``find_best_view``, ``is_visible`` and ``clear``, so that the BA drop-in runs on it."""

    def __init__(self, key_type, is_cross_check, is_knn_match, is_fund_inlier, ransac_config):
        self.key_type = key_type
        self.is_cross_check = is_cross_check
        self.is_knn_match = is_knn_match
        self.is_fund_inlier = is_fund_inlier
        self.ransac_config = ransac_config
        self.track_list = []

    def add_new_view(self, new_view, views, is_knn_match=None, is_fund_inlier=None, ransac_config=None):
        # falsy -> instance default (key_tracker.py:114-119, quirk Q17)
        if not is_knn_match:
            is_knn_match = self.is_knn_match
        if not is_fund_inlier:
            is_fund_inlier = self.is_fund_inlier
        if not ransac_config:
            ransac_config = self.ransac_config
        if len(self.track_list) == 0:
            self.track_list.append(HipKeyTrack(1, len(new_view.key_pts), 0))
        else:
            self._KeyTracker__extend_list(new_view, views, is_knn_match, is_fund_inlier, ransac_config)

    def generate_matched_pairs(self, ref_idx, que_idx, views):
        """key_tracker.py:132-181 (entries ``row > 0`` only: key 0 of the query view is never paired, quirk Q3)."""
        if ref_idx < 0 or que_idx < 0 or ref_idx >= len(self.track_list) or que_idx >= len(self.track_list):
            print('{}:{} - invalid ref_idx {} or invalid que_idx {}'.format(
                self.__class__.__name__, 'generate_matched_pairs', ref_idx, que_idx))
            return None
        row = self.track_list[ref_idx].table[que_idx:que_idx + 1, :]
        r_idx = np.where(row > 0)[1]
        q_idx = row[0, r_idx]
        num = r_idx.shape[0]
        ref_pts = np.zeros((3, num)); ref_pts[2] = 1.0
        que_pts = np.zeros((3, num)); que_pts[2] = 1.0
        for c, (pts, views_idx, idx) in enumerate(((ref_pts, ref_idx, r_idx), (que_pts, que_idx, q_idx))):
            kp = views[views_idx].key_pts
            for j, k in enumerate(idx.tolist()):
                pts[0, j], pts[1, j] = kp[k].pt[0], kp[k].pt[1]
        return [ref_pts, que_pts], r_idx.reshape(1, num).astype(int), q_idx.reshape(1, num).astype(int)

    def find_best_view(self, input_idx):
        if input_idx < 0 or input_idx >= len(self.track_list):
            print('{}:{} - invalid input_idx {}'.format(self.__class__.__name__, 'find_best_view', input_idx))
            return -1
        return 0

    def is_visible(self, view_idx, tri_pt_idx):
        key_idx = np.where(self.track_list[view_idx].table[view_idx, :] == tri_pt_idx)
        if np.any(key_idx):
            key_idx = key_idx[0][0]
        else:
            key_idx = -1
        return key_idx

    def clear(self):
        self.track_list = []


class HipDeviceKeyTrack:
    """``KeyTrack`` of a ``HipDeviceKeyTracker``: the table lives in the tracker's ``native.TrackStore``.

    ``table`` is an int64 host copy, downloaded again only when the device copy has changed since the last read.  It is a
    picture, not the table: writing into it does NOT reach the device (use ``update_usage``), just as editing
    ``view.key_pts[i].pt`` after the view was added does not (the coordinates were copied when the view came in).
    ``update_usage`` and the two ``extract_*`` methods run on the device copy and return what ``HipKeyTrack`` returns."""

    def __init__(self, tracker, idx, key_num):
        self._tracker = tracker
        self.idx = idx
        self.key_num = key_num
        self._host = None
        self._host_version = -1

    @property
    def table(self):
        version = self._tracker._versions[self.idx]
        if self._host is None or self._host_version != version:
            self._host = self._tracker._store.table(self.idx).astype('int')
            self._host_version = version
        return self._host

    @table.setter
    def table(self, value):               # a host-side replacement (a slice for a smaller problem): the device keeps its own
        self._host = value
        self._host_version = self._tracker._versions[self.idx]

    def update_usage(self, used_indices, tri_indices):
        used = np.asarray(used_indices)
        keys = used.reshape(-1).astype(np.int64)
        tri = np.asarray(tri_indices)[0, np.indices(used.shape)[1].reshape(-1)]
        keys = np.where(keys < 0, keys + self.key_num, keys)                 # NumPy's negative indices
        if keys.shape[0] and (keys.min() < 0 or keys.max() >= self.key_num):
            raise IndexError("index out of bounds for axis 1 with size {}".format(self.key_num))
        self._tracker._store.update_usage(self.idx, keys, tri)
        self._tracker._versions[self.idx] += 1

    def extract_unconstructed_points(self):
        return self._tracker._store.unconstructed(self.idx).astype(np.int64)[np.newaxis, :]

    def extract_constructed_points(self):
        keys, tri = self._tracker._store.constructed(self.idx)
        return keys.astype(np.int64)[np.newaxis, :], tri.astype('int')[np.newaxis, :]


class HipDeviceKeyTracker(HipKeyTrackerMixin):
    """``HipKeyTracker`` with the key tracks resident on the device (``native.TrackStore``, csrc/sfm_track.hip): the same
    constructor and methods, the same tables.  ``add_new_view`` uploads the new view's descriptors and key coordinates,
    matches it against every earlier view and runs the ratio / crossCheck filter, the duplicate removal (quirk Q14)
    and the table writes on the device, with no neighbour array on the host; only the per-view status comes back
    (quirk Q16: the exception the reference raises, at the same query, tables left as the reference leaves them).  With
    ``is_fund_inlier`` the kept lists come back, ``HipEpipolarProcessor`` runs per reference view in the reference's
    order (Python's global RNG stream is consumed identically) and the prefixes are written (quirk Q15).

    Key coordinates come from ``view.key_xy`` ((n, 2), attached by ``HipViewProcessor.generate_view``) or, without it,
    from one pass over ``view.key_pts``; ``generate_matched_pairs`` reads the device copy, so its ``views`` argument is not
    looked at.  ``track_list[i]`` is a ``HipDeviceKeyTrack``.  ``kt_upload_bytes`` counts descriptors, coordinates and
    usage lists; ``kt_download_bytes`` what came back; ``kt_release()`` frees the device copies."""

    def __init__(self, key_type, is_cross_check, is_knn_match, is_fund_inlier, ransac_config):
        self.key_type = key_type
        self.is_cross_check = is_cross_check
        self.is_knn_match = is_knn_match
        self.is_fund_inlier = is_fund_inlier
        self.ransac_config = ransac_config
        self.track_list = []
        self._store = None
        self._versions = []               # per view: bumped whenever the device table changes
        self._xy = []                     # per view: the (n, 2) coordinates that went up (fundamental-inlier pairs)
        self._retired_bytes = [0, 0]

    def kt_release(self):
        HipKeyTrackerMixin.kt_release(self)
        if self._store is not None:
            self._retired_bytes[0] += self._store.upload_bytes
            self._retired_bytes[1] += self._store.download_bytes
            self._store.close()
            self._store = None

    @property
    def kt_upload_bytes(self):
        return (self.__dict__.get("_hip_desc_bytes", 0) + self._retired_bytes[0]
                + (self._store.upload_bytes if self._store is not None else 0))

    @property
    def kt_download_bytes(self):
        return self._retired_bytes[1] + (self._store.download_bytes if self._store is not None else 0)

    @staticmethod
    def _key_xy(view):
        xy = getattr(view, "key_xy", None)
        if xy is None or len(xy) != len(view.key_pts):
            xy = np.array([kp.pt for kp in view.key_pts], dtype=np.float64)
        return np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)

    def add_new_view(self, new_view, views, is_knn_match=None, is_fund_inlier=None, ransac_config=None):
        # falsy -> instance default (key_tracker.py:114-119, quirk Q17)
        if not is_knn_match:
            is_knn_match = self.is_knn_match
        if not is_fund_inlier:
            is_fund_inlier = self.is_fund_inlier
        if not ransac_config:
            ransac_config = self.ransac_config
        if len(self.track_list) == 0:
            if self._store is not None:
                self.kt_release()
            self._store = native.TrackStore()
            self._versions, self._xy = [0], [self._key_xy(new_view)]
            self._store.add_view(self._xy[0])
            self.track_list.append(HipDeviceKeyTrack(self, 0, len(new_view.key_pts)))
        else:
            self._KeyTracker__extend_list(new_view, views, is_knn_match, is_fund_inlier, ransac_config)

    def _register_views(self, views):
        """Bring the views ``views[len(self.track_list):]`` into the store WITHOUT matching them: their coordinates and
        descriptors go up, every table gets their (empty) rows and ``track_list`` their ``HipDeviceKeyTrack``.  What
        ``match_pairs`` fills afterwards; ``add_new_view`` may still follow.  Returns the number of views added."""
        first = len(self.track_list)
        if self._store is not None and self._store.n_views != first:
            raise native.SfmHipError("HipDeviceKeyTracker: the device store holds %d views, track_list %d" % (self._store.n_views, first))
        for idx in range(first, len(views)):
            view = views[idx]
            xy = self._key_xy(view)
            d = view.key_descriptors
            if d is not None and len(d) and len(d) != xy.shape[0]:
                raise ValueError("{} descriptors for {} keys".format(len(d), xy.shape[0]))
            if self._store is None:
                self._store = native.TrackStore()
            self._kt_set(idx, d)
            self._store.add_view(xy)
            self._versions = [v + 1 for v in self._versions] + [0]
            self._xy.append(xy)
            self.track_list.append(HipDeviceKeyTrack(self, idx, xy.shape[0]))
        return len(self.track_list) - first

    def _extend_list(self, new_view, views, is_knn_match=False, is_fund_inlier=False, ransac_config=None):
        key_num = len(new_view.key_pts)
        new_idx = len(self.track_list)
        store = self._store
        if store is None or store.n_views != new_idx:
            raise native.SfmHipError("HipDeviceKeyTracker: the device store holds %s views, track_list %d"
                                     % ("no" if store is None else store.n_views, new_idx))
        if len(views) > new_idx:
            raise ValueError("{} reference views for view {}".format(len(views), new_idx))
        refs = []
        for ref_idx, ref_view in enumerate(views):
            d = ref_view.key_descriptors
            if d is None or len(d) == 0:      # undefined without cv2 (deviation of Q16)
                raise ValueError("reference view {} has no descriptors".format(ref_idx))
            refs.append(self._kt_set(ref_idx, d))
        query = self._kt_set(new_idx, new_view.key_descriptors)
        if refs and query.n != key_num:
            raise ValueError("{} descriptors for {} keys".format(query.n, key_num))
        mode = matching.match_mode(is_knn_match, self.is_cross_check)
        xy = self._key_xy(new_view)

        store.add_view(xy)                                                      # key_tracker.py:236-240
        self._versions = [v + 1 for v in self._versions] + [0]
        self._xy.append(xy)
        try:
            store.match_views(new_idx, query, refs, mode, write=not is_fund_inlier)
            status, bad, n_kept = store.extend_status(len(refs))
            for ref_idx in range(len(refs)):                                    # key_tracker.py:247
                if status[ref_idx] == native.TRACK_NO_SECOND:
                    raise IndexError("tuple index out of range")                # item[1] of a one-element knnMatch result
                if status[ref_idx] == native.TRACK_ZERO_SECOND:
                    raise ZeroDivisionError("float division by zero")           # item[0].distance / item[1].distance
                if status[ref_idx] != native.TRACK_OK:
                    raise ValueError("reference view {}: query {} has a neighbour outside the view".format(ref_idx, bad[ref_idx]))
                if is_fund_inlier:                                              # key_tracker.py:294-314
                    qk, tk = store.kept(ref_idx, int(n_kept[ref_idx]))
                    ref_pts = np.ones((3, tk.shape[0])); que_pts = np.ones((3, qk.shape[0]))
                    ref_pts[0:2] = self._xy[ref_idx][tk].T
                    que_pts[0:2] = xy[qk].T
                    ep = HipEpipolarProcessor(ransac_config)
                    n_in = len(ep.determine_fundamental_mat([ref_pts, que_pts], ransac_config))
                    store.write_kept(ref_idx, n_in)
        except BaseException:
            # the reference has expanded every table and written the pairs before the failing one, and has not
            # appended the new track: the same here
            store.drop_last_view()
            self._versions.pop()
            self._xy.pop()
            raise
        self.track_list.append(HipDeviceKeyTrack(self, new_idx, key_num))

    def generate_matched_pairs(self, ref_idx, que_idx, views):
        """key_tracker.py:132-181 from the device copy (entries ``> 0`` only: quirk Q3).  Nothing goes up; the count and
        the four result arrays come down."""
        if ref_idx < 0 or que_idx < 0 or ref_idx >= len(self.track_list) or que_idx >= len(self.track_list):
            print('{}:{} - invalid ref_idx {} or invalid que_idx {}'.format(
                self.__class__.__name__, 'generate_matched_pairs', ref_idx, que_idx))
            return None
        r_idx, q_idx, ref_pts, que_pts = self._store.pairs(ref_idx, que_idx)
        num = r_idx.shape[0]
        return [ref_pts, que_pts], r_idx.reshape(1, num).astype(int), q_idx.reshape(1, num).astype(int)

    def find_best_view(self, input_idx):
        if input_idx < 0 or input_idx >= len(self.track_list):
            print('{}:{} - invalid input_idx {}'.format(self.__class__.__name__, 'find_best_view', input_idx))
            return -1
        return 0

    def is_visible(self, view_idx, tri_pt_idx):
        key_idx = np.where(self._store.row(view_idx, view_idx) == tri_pt_idx)
        if np.any(key_idx):
            key_idx = key_idx[0][0]
        else:
            key_idx = -1
        return key_idx

    def clear(self):
        self.kt_release()
        self.track_list = []
        self._versions, self._xy = [], []


# ------------------------------------------------------------------------------------------------
def verify_pairs(tracker, ref_idx, que_idx, max_sampson_px=2.0, max_hyp=128, iteration=2):
    """The pairs ``tracker.generate_matched_pairs(ref_idx, que_idx)`` returns (``tracker``: a ``HipDeviceKeyTracker``),
    verified geometrically without leaving the device (``TrackStore.verify_pairs``: the pairs are gathered into device
    buffers and handed to the robust two-view geometry on the same stream; no coordinate comes down).  Returns
    ``r_idx (1, n), q_idx (1, n), inlier (n,) bool``; ``tracker.twoview_last`` keeps the matrix (Frobenius norm 1),
    hypothesis and status.  A function of the module, not a method: the tracker's class keeps the reference's public
    methods and ``kt_release`` only."""
    n_views = len(tracker.track_list)
    if ref_idx < 0 or que_idx < 0 or ref_idx >= n_views or que_idx >= n_views:
        print('{}:{} - invalid ref_idx {} or invalid que_idx {}'.format(
            tracker.__class__.__name__, 'verify_pairs', ref_idx, que_idx))
        return None
    if not float(max_sampson_px) >= 0.0:
        raise ValueError("max_sampson_px must be >= 0, got {!r}".format(max_sampson_px))
    r_idx, q_idx, inlier, fund, best, status = tracker._store.verify_pairs(ref_idx, que_idx, float(max_sampson_px) ** 2, max_hyp,
                                                                           iteration)
    tracker.twoview_last = {"fund_mat": fund, "hypothesis": best, "status": status}
    num = r_idx.shape[0]
    return r_idx.reshape(1, num).astype(int), q_idx.reshape(1, num).astype(int), inlier.astype(bool)


def _essential_entry(out, s, lo, hi):
    """What the callers of ``native.essential_ransac`` keep of set ``s`` (matches lo .. hi - 1) of its result."""
    return {"esse_mat": out["E"][s], "fund_mat": out["F"][s], "inliers": np.flatnonzero(out["inlier"][lo:hi]).tolist(),
            "hypothesis": int(out["best_hyp"][s]), "root": int(out["best_root"][s]), "n_valid": int(out["n_valid"][s]),
            "status": int(out["status"][s])}


def essential_pairs(tracker, ref_idx, que_idx, K_left, K_right, max_sampson_px=2.0, max_hyp=128):
    """``determine_essential_mat_robust`` over the pairs ``tracker.generate_matched_pairs(ref_idx, que_idx)`` returns
    (``tracker``: a ``HipDeviceKeyTracker``; the reference key is LEFT, the query key RIGHT) without a coordinate leaving the
    device: the gather of ``verify_pairs`` (``TrackStore.pairs_dev``) fills device buffers, and ``native.essential_ransac_dev``
    reads them on the same stream as one set.  Only the count of pairs comes down between the two steps, and the indices, the
    mask and the model after them.  Returns ``r_idx (1, n), q_idx (1, n), inlier (n,) bool``; ``tracker.essential_last`` keeps
    what ``determine_essential_mat_robust`` keeps.  A function of the module, like ``verify_pairs``."""
    n_views = len(tracker.track_list)
    if ref_idx < 0 or que_idx < 0 or ref_idx >= n_views or que_idx >= n_views:
        print('{}:{} - invalid ref_idx {} or invalid que_idx {}'.format(
            tracker.__class__.__name__, 'essential_pairs', ref_idx, que_idx))
        return None
    if not float(max_sampson_px) >= 0.0:
        raise ValueError("max_sampson_px must be >= 0, got {!r}".format(max_sampson_px))
    import torch
    store = tracker._store
    cap = max(store.n_keys(ref_idx), 1)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_count = torch.empty(2, dtype=torch.int32, device="cuda")
        d_r, d_q = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))
        d_ref, d_que = (torch.empty(3 * cap, dtype=torch.float64, device="cuda") for _ in range(2))
        store.pairs_dev(ref_idx, que_idx, d_count.data_ptr(), d_r.data_ptr(), d_q.data_ptr(), d_ref.data_ptr(), d_que.data_ptr(),
                        stream.cuda_stream)
        count = d_count.cpu().numpy()
        if count[1]:
            raise ValueError("table[{}][{}] names a key the query view does not have".format(ref_idx, que_idx))
        num = int(count[0])
        d_E, d_F = (torch.empty(9, dtype=torch.float64, device="cuda") for _ in range(2))
        d_in = torch.empty(max(num, 1), dtype=torch.uint8, device="cuda")
        d_int = torch.empty(5, dtype=torch.int32, device="cuda")      # n_inliers, best_hyp, best_root, n_valid, status
        ints = [d_int.data_ptr() + 4 * k for k in range(5)]
        # the packed (3, n) point arrays begin with the x row and the y row: the [2][n] layout of the robust estimators
        native.essential_ransac_dev([0, num], num, d_ref.data_ptr(), d_que.data_ptr(), K_left, K_right, float(max_sampson_px) ** 2,
                                    max_hyp, d_E.data_ptr(), d_F.data_ptr(), d_in.data_ptr(), *ints, stream=stream.cuda_stream)
        r_idx, q_idx = d_r[:num].cpu().numpy(), d_q[:num].cpu().numpy()
        inlier = d_in[:num].cpu().numpy()
        got = d_int.cpu().numpy()
        out = {"E": d_E.cpu().numpy().reshape(1, 3, 3), "F": d_F.cpu().numpy().reshape(1, 3, 3), "inlier": inlier}
    out.update({name: got[k:k + 1] for k, name in enumerate(("n_inliers", "best_hyp", "best_root", "n_valid", "status"))})
    tracker.essential_last = _essential_entry(out, 0, 0, num)
    return r_idx.reshape(1, num).astype(int), q_idx.reshape(1, num).astype(int), inlier.astype(bool)


def _pose_result(owner, out, s, lo, hi):
    """(rot, centre, front indices, counts) of set ``s`` of a ``native.twoview_pose`` result (matches lo .. hi - 1), kept as
    ``owner.pose_last``."""
    R, t = out["R"][s], out["t"][s]
    won = out["best_cand"][s] >= 0
    counts = {"n_front": int(out["n_front"][s]), "n_parallax": int(out["n_parallax"][s]), "cand_front": out["cand_front"][s].copy(),
              "best_cand": int(out["best_cand"][s]), "status": int(out["status"][s])}
    last = dict(counts)
    last.update({"R": R, "t": t, "normal": out["normal"][s], "obs_front": out["obs_front"][lo:hi], "X": out["X"][:, lo:hi]})
    owner.pose_last = last
    rot = R.T.copy() if won else np.identity(3)
    return rot, (-R.T @ t).reshape(3, 1), np.flatnonzero(out["obs_front"][lo:hi]).tolist(), counts


def pose_from_reference_convention(rot, centre):
    """(R, t) with X_right = R X_left + t and |t| = 1 of a pose given as ``rot = R^T`` and ``centre = -R^T t``; a centre at the
    origin gives t = 0, which the refinement answers with ``native.REFINE_BAD_POSE``."""
    R = np.ascontiguousarray(np.asarray(rot, dtype=np.float64).reshape(3, 3).T)
    t = -R @ np.asarray(centre, dtype=np.float64).reshape(3)
    norm = np.linalg.norm(t)
    return R, (t / norm if norm > 0 and np.isfinite(norm) else t)


def _refined_entry(ref, s, lo, hi, posed):
    """The keys a refinement adds to the dict of set ``s`` (matches lo .. hi - 1) of ``initialise_pairs`` / ``pose_pairs``."""
    R, t = ref["R"][s], ref["t"][s]
    return {"R_refined": R, "t_refined": t, "rot_refined": R.T.copy() if posed else np.identity(3),
            "centre_refined": (-R.T @ t).reshape(3, 1), "F_refined": ref["F"][s],
            "refine_inliers": np.flatnonzero(ref["obs_inlier"][lo:hi]).tolist(),
            "refine_front": np.flatnonzero(ref["obs_front"][lo:hi]).tolist(), "refine_cost": ref["cost"][:, s].copy(),
            "refine_used": int(ref["n_used"][s]), "refine_status": int(ref["status"][s])}


def _refine_result(owner, out):
    """(rot, centre, rms before, rms after, inlier indices, front indices, info (5, 5), status) of the one set of a
    ``native.twoview_refine`` result, kept as ``owner.refine_last``."""
    R, t = out["R"][0], out["t"][0]
    used, status = int(out["n_used"][0]), int(out["status"][0])
    passes = used >= native.REFINE_MIN_USED and not status & native.REFINE_BAD_POSE
    rms = np.sqrt(out["cost"][:, 0] / used) if passes else np.full(2, np.nan)
    last = {name: (out[name][0] if name in ("F", "info", "n_used", "status", "n_inliers", "n_front", "n_parallax") else out[name])
            for name in native.REFINE_OUTPUTS if name != "summary"}
    last.update({"R": R, "t": t, "cost": out["cost"][:, 0].copy()})
    owner.refine_last = last
    return (R.T.copy(), (-R.T @ t).reshape(3, 1), float(rms[0]), float(rms[1]), np.flatnonzero(out["obs_inlier"]).tolist(),
            np.flatnonzero(out["obs_front"]).tolist(), native.info_matrix(out["info"][0]), status)


def pose_pairs(tracker, ref_idx, que_idx, model, kind, K_left, K_right, inlier=None, min_angle_deg=2.0, min_parallax=8, refine_iters=0,
               max_px=2.0):
    """``estimate_relative_pose_robust`` over the pairs ``tracker.generate_matched_pairs(ref_idx, que_idx)`` returns
    (``tracker``: a ``HipDeviceKeyTracker``) without leaving the device (``TrackStore.pose_pairs``: the pairs are gathered
    into device buffers and posed on the same stream; nothing goes up but the model, the intrinsics and the optional mask
    ``inlier`` (n,) of ``verify_pairs``, no coordinate comes down).  Returns ``r_idx (1, n), q_idx (1, n), rot, centre,
    front_idx, counts`` as that method does; ``tracker.pose_last`` keeps what its ``pose_last`` keeps.  A function of the
    module, like ``verify_pairs``.

    With ``refine_iters > 0`` ONE ``TrackStore.refine_pairs`` follows on the same pairs, still without a coordinate coming
    down: the pose refined on its matches in front by that many Gauss-Newton steps and judged at ``max_px`` pixels, with an
    empty mask if the pose has ``native.POSE_NO_POSE`` or ``native.POSE_NO_PARALLAX``.  ``counts`` then also has the keys
    ``initialise_pairs`` adds (``R_refined`` ... ``refine_status``); the pose returned stays the unrefined one."""
    refine_iters = native._count("refine_iters", refine_iters)
    n_views = len(tracker.track_list)
    if ref_idx < 0 or que_idx < 0 or ref_idx >= n_views or que_idx >= n_views:
        print('{}:{} - invalid ref_idx {} or invalid que_idx {}'.format(
            tracker.__class__.__name__, 'pose_pairs', ref_idx, que_idx))
        return None
    if not 0.0 <= float(min_angle_deg) <= 90.0:
        raise ValueError("min_angle_deg must be in [0, 90], got {!r}".format(min_angle_deg))
    o = tracker._store.pose_pairs(ref_idx, que_idx, model, kind, K_left, K_right, math.cos(math.radians(float(min_angle_deg))) ** 2,
                                  min_parallax, inlier)
    num = o["r_idx"].shape[0]
    out = {"R": o["R"][None], "t": o["t"][None], "normal": o["normal"][None], "cand_front": o["cand_front"][None],
           "obs_front": o["obs_front"], "X": o["X"]}
    out.update({name: np.array([o[name]]) for name in ("n_front", "n_parallax", "best_cand", "status")})
    rot, centre, front, counts = _pose_result(tracker, out, 0, 0, num)
    if refine_iters > 0:
        if not float(max_px) >= 0.0:
            raise ValueError("max_px must be >= 0, got {!r}".format(max_px))
        skip = o["status"] & (native.POSE_NO_POSE | native.POSE_NO_PARALLAX)
        mask = np.zeros(num, dtype=np.uint8) if skip else (o["obs_front"] > 0).astype(np.uint8)
        f = tracker._store.refine_pairs(ref_idx, que_idx, o["R"], o["t"], K_left, K_right, 0.0, refine_iters, float(max_px) ** 2,
                                        math.cos(math.radians(float(min_angle_deg))) ** 2, mask)
        ref = {"R": f["R"][None], "t": f["t"][None], "F": f["F"][None], "cost": f["cost"].reshape(2, 1), "obs_inlier": f["obs_inlier"],
               "obs_front": f["obs_front"], "n_used": np.array([f["n_used"]]), "status": np.array([f["status"]])}
        counts.update(_refined_entry(ref, 0, 0, num, counts["best_cand"] >= 0))
        tracker.refine_last = f
    return o["r_idx"].reshape(1, num).astype(int), o["q_idx"].reshape(1, num).astype(int), rot, centre, front, counts


def orient_views(tracker, pairs, K, K_right=None, root=0, max_sampson_px=2.0, max_hyp=128, iteration=2, min_angle_deg=2.0,
                 min_parallax=8, max_angle_deg=5.0, tree_hyp=128, rounds=2, triplets=None):
    """Absolute rotations of the views of a ``HipDeviceKeyTracker`` from the listed ``pairs`` ``(ref_idx, que_idx)``: per
    pair ONE ``verify_pairs`` and, where it has a model, ONE ``pose_pairs`` from that model with its inliers voting (no
    coordinate comes down), then ONE ``HipCamposeMixin.average_rotations`` over the poses found.  Returns ``rots, verdict,
    poses``: the first two as ``average_rotations`` returns them (``verdict["pairs"]`` indexes ``pairs``), ``poses`` one dict
    per listed pair (``R``, ``t``, ``status`` of the pose call, ``twoview_status``; ``R`` is None without a pose).
    ``triplets`` (None, or a dict of the options of ``filter_view_graph``) puts the triplet filter in front of the averaging,
    as ``average_rotations`` describes.  A function of the module, like ``verify_pairs``; ``process()`` does not call it."""
    K_right = K if K_right is None else K_right
    n_views = len(tracker.track_list)
    poses, triples = [], []
    for ref_idx, que_idx in pairs:
        entry = {"ref": int(ref_idx), "que": int(que_idx), "R": None, "t": None, "status": native.POSE_NO_POSE, "twoview_status": None}
        got = verify_pairs(tracker, ref_idx, que_idx, max_sampson_px, max_hyp, iteration)
        if got is not None:
            entry["twoview_status"] = int(tracker.twoview_last["status"])
            if tracker.twoview_last["hypothesis"] >= 0:
                posed = pose_pairs(tracker, ref_idx, que_idx, tracker.twoview_last["fund_mat"], "fundamental", K, K_right, got[2],
                                   min_angle_deg, min_parallax)
                counts = posed[5]
                entry["status"] = counts["status"]
                if counts["best_cand"] >= 0 and not counts["status"] & native.POSE_NO_POSE:
                    entry["R"], entry["t"] = tracker.pose_last["R"].copy(), tracker.pose_last["t"].copy()
            entry["r_idx"], entry["q_idx"], entry["inlier"] = got[0].reshape(-1), got[1].reshape(-1), got[2]      # for link_views
        poses.append(entry)
        triples.append((entry["ref"], entry["que"], entry["R"]))
    rots, verdict = HipCamposeMixin().average_rotations(triples, n_views, root, max_angle_deg, tree_hyp, rounds, triplets=triplets)
    return rots, verdict, poses


def locate_views(tracker, pairs, K, K_right=None, root=0, max_sampson_px=2.0, max_hyp=128, iteration=2, min_angle_deg=2.0,
                 min_parallax=8, max_angle_deg=5.0, tree_hyp=128, rounds=2, max_direction_deg=5.0, translation_rounds=8, triplets=None):
    """Absolute rotations AND positions of the views of a ``HipDeviceKeyTracker``: ``orient_views`` over the listed ``pairs``,
    then ONE ``HipCamposeMixin.average_translations`` over the same poses with the rotations found and the rotation verdict
    as the edge mask (a pair whose rotation disagrees with the graph lends no direction).  Returns ``rots, centres, verdicts,
    poses``: ``rots`` and ``poses`` as ``orient_views`` returns them, ``centres`` as ``average_translations`` does (all None
    where the rotations have no model), ``verdicts`` the dict ``{"rotation": ..., "translation": ...}`` (the second None
    without a rotation model).  ``triplets`` goes to ``orient_views``: a pair the triplet filter dropped is no inlier of the
    rotation verdict and lends no direction either.  A function of the module, like ``orient_views``; ``process()`` does not
    call it."""
    rots, rot_verdict, poses = orient_views(tracker, pairs, K, K_right, root, max_sampson_px, max_hyp, iteration, min_angle_deg,
                                            min_parallax, max_angle_deg, tree_hyp, rounds, triplets=triplets)
    n_views = len(tracker.track_list)
    if rot_verdict["status"] & native.ROTAVG_NO_MODEL:
        return rots, [None] * n_views, {"rotation": rot_verdict, "translation": None}, poses
    quads = [(p["ref"], p["que"], p["R"], p["t"]) for p in poses]
    centres, tr_verdict = HipCamposeMixin().average_translations(quads, rots, n_views, root, max_direction_deg, translation_rounds,
                                                                 edge_mask=rot_verdict["edge_inlier"])
    return rots, centres, {"rotation": rot_verdict, "translation": tr_verdict}, poses


def link_key_mask(n_ref_keys, inliers=None, pair_mask=None):
    """The per-key mask ``TrackStore.link`` takes, on the host: for pair ``p`` ``n_ref_keys[p]`` bytes, one per key of its
    reference view, the pairs concatenated in their order.  ``inliers[p]`` is None (every match of the pair is used: all
    ones) or ``(r_idx, mask)``: the reference keys of the pair's matches as ``generate_matched_pairs`` / ``verify_pairs``
    return them and the mask over those matches; the byte of ``r_idx[k]`` is set iff ``mask[k]``.  ``pair_mask[p]`` false
    drops the whole pair (all zeros).  A key without a match has no table entry, so its byte is never looked at."""
    n_ref_keys = [int(n) for n in n_ref_keys]
    P = len(n_ref_keys)
    if inliers is not None and len(inliers) != P:
        raise ValueError("link: {} inlier masks for {} pairs".format(len(inliers), P))
    if pair_mask is not None and len(pair_mask) != P:
        raise ValueError("link: {} pair verdicts for {} pairs".format(len(pair_mask), P))
    parts = []
    for p, n in enumerate(n_ref_keys):
        if pair_mask is not None and not pair_mask[p]:
            parts.append(np.zeros(n, dtype=np.uint8))
            continue
        if inliers is None or inliers[p] is None:
            parts.append(np.ones(n, dtype=np.uint8))
            continue
        r_idx, mask = inliers[p]
        r_idx, mask = np.asarray(r_idx, dtype=np.int64).reshape(-1), np.asarray(mask).reshape(-1) != 0
        if r_idx.shape != mask.shape:
            raise ValueError("link: pair {} has {} matches and {} mask entries".format(p, r_idx.size, mask.size))
        if r_idx.size and (r_idx.min() < 0 or r_idx.max() >= n):
            raise ValueError("link: pair {} names a reference key outside 0 .. {}".format(p, n - 1))
        part = np.zeros(n, dtype=np.uint8)
        part[r_idx[mask]] = 1
        parts.append(part)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def link_views(tracker, pairs, inliers=None, pair_mask=None, min_len=2, want_key_track=True):
    """Multi-view tracks of a ``HipDeviceKeyTracker`` from the matches of the listed ``pairs`` ``(ref_idx, que_idx)``
    (``TrackStore.link``: connected components of the match graph, read from the tables where they lie; a component with two
    keys of one view is dropped).  ``inliers[p]`` is the mask ``verify_pairs`` returned over the pair's matches -- or the
    tuple ``(r_idx, mask)``, which saves fetching the table row to find the matches' reference keys -- or None; ``pair_mask``
    drops whole pairs (the rotation and translation verdicts).  Only the per-key mask goes up.  The tracks become the
    store's observation list (every view named needs ``set_normalised`` coordinates), ready for
    ``BaProblem.from_tracks``.  Returns ``summary, key_track``: a dict over ``native.LINK_SUMMARY`` and the per-key verdicts of
    all keys of the store, views concatenated (None unless ``want_key_track``).  A function of the module, like
    ``verify_pairs``; ``process()`` does not call it."""
    store = tracker._store
    pairs = [(int(r), int(q)) for r, q in pairs]
    n_views = len(tracker.track_list)
    for r, q in pairs:
        if not (0 <= r < n_views and 0 <= q < n_views) or r == q:
            raise ValueError("link: pair ({}, {}) must join two different views in 0 .. {}".format(r, q, n_views - 1))
    key_mask = None
    if inliers is not None or pair_mask is not None:
        filled = None
        if inliers is not None:
            filled = []
            for p, item in enumerate(inliers):
                if item is None or isinstance(item, tuple):
                    filled.append(item)
                else:                                                   # a bare mask: the matches are the row's entries > 0
                    filled.append((np.flatnonzero(store.row(pairs[p][0], pairs[p][1]) > 0), item))
        key_mask = link_key_mask([store.n_keys(r) for r, _ in pairs], filled, pair_mask)
    key_track = None
    if want_key_track:
        import torch
        total = sum(store.n_keys(v) for v in range(n_views))
        d_track = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        summary = store.link(pairs, key_mask, min_len, d_track.data_ptr())
        key_track = d_track[:total].cpu().numpy()
    else:
        summary = store.link(pairs, key_mask, min_len)
    return dict(zip(native.LINK_SUMMARY, (int(v) for v in summary))), key_track


def reconstruct_views(tracker, pairs, K, root=0, min_len=2, lam=5.0, iters=10, solver="iterate", refine_iters=20, retriangulate_px=None,
                      cull_px=None, set_normalised=True, **locate):
    """A global reconstruction of the views of a ``HipDeviceKeyTracker`` from the listed ``pairs``, on the device from the
    matches to the adjusted scene: ``locate_views`` (``locate`` are its options, ``triplets=`` for the triplet filter among
    them; one intrinsic matrix ``K`` for every view),
    ``link_views`` over the pairs both verdicts admit with each pair's verification inliers, a ``BaProblem`` from the tracks
    with the averaged rotations and centres as cameras, ``refine_points`` (DLT, then Gauss-Newton) for the points, with
    ``retriangulate_px`` the robust re-triangulation and with ``cull_px`` a cull at that many pixels, then ``iters``
    iterations of ``solver``: ``"iterate"`` (all cameras move, the gauge is the damping's) or ``"pcg"`` (``minimize_pcg`` with
    ``root`` and the view farthest from it held: the second fixes the scale).  Only the per-key masks go up -- and, with
    ``set_normalised``, once the normalised key coordinates the observation list gathers from; the verdicts and the result
    come down.  Returns a dict: ``rots``, ``centres`` (lists in the reference's convention, None for a view without a pose),
    ``points`` (3, n_tracks), ``key_track``, ``summary`` of the linking, ``verdicts``, ``poses``, ``pair_mask``, ``cameras`` (V, 7),
    ``rots_averaged`` and ``centres_averaged`` (what ``locate_views`` gave, before the adjustment), ``pt_ptr`` and ``cam_idx`` of the
    adjusted scene and ``cost`` (the cost after the points were made, then after every iteration or accepted trial).  A function of the
    module, like ``locate_views``; ``process()`` does not call it."""
    if solver not in ("iterate", "pcg"):
        raise ValueError("solver must be 'iterate' or 'pcg', got {!r}".format(solver))
    pairs = [(int(r), int(q)) for r, q in pairs]
    rots, centres, verdicts, poses = locate_views(tracker, pairs, K, None, root, **locate)
    tv = verdicts["translation"]
    if tv is None or tv["status"] & native.TRANSAVG_NO_MODEL:
        raise ValueError("reconstruct_views: the pairs give no rotations or no positions")
    pair_mask = np.zeros(len(pairs), dtype=bool)
    both = verdicts["rotation"]["edge_inlier"] & tv["edge_inlier"]
    pair_mask[np.asarray(tv["pairs"], dtype=np.int64)[both]] = True
    located = [rots[v] is not None and centres[v] is not None for v in range(len(rots))]
    for p, (r, q) in enumerate(pairs):
        pair_mask[p] &= located[r] and located[q]
    store = tracker._store
    n_views = len(tracker.track_list)
    if set_normalised:
        for v in range(n_views):
            store.set_normalised(v, normalise_pixels(tracker._xy[v].T, K))
    inliers = [(e["r_idx"], e["inlier"]) if "inlier" in e else None for e in poses]
    summary, key_track = link_views(tracker, pairs, inliers, pair_mask, min_len)
    cams = pack_cameras([rots[v] if located[v] else np.identity(3) for v in range(n_views)],
                                 [centres[v] if located[v] else np.zeros(3) for v in range(n_views)])
    px2 = 1.0 / float(K[0][0]) ** 2                                         # a squared pixel in normalised units
    with native.BaProblem.from_tracks(store) as prob:
        prob.set_state(cams, np.zeros((3, prob.n_pts)))
        prob.refine_points(0.0, 0, native.TRACKS_LINEAR, want_outputs=False)
        prob.refine_points(0.5, refine_iters, native.TRACKS_NONLINEAR, want_outputs=False)
        if retriangulate_px is not None:
            prob.retriangulate(float(retriangulate_px) ** 2 * px2, want_outputs=False)
        if cull_px is not None:
            prob.cull(float(cull_px) ** 2 * px2, want_outputs=False)
        cost = [prob.cost()]
        if solver == "iterate":
            for _ in range(int(iters)):
                prob.iterate(lam, 1)
                cost.append(prob.cost())
        else:
            free = np.array(located, dtype=np.uint8)
            far = max((v for v in range(n_views) if located[v]), key=lambda v: float(np.linalg.norm(centres[v] - centres[root])))
            free[[root, far]] = 0
            done = prob.minimize_pcg(free, lambda0=lam, max_trials=int(iters))
            cost.extend(float(c) for c in done.log["cost"][done.log["accepted"] != 0])
        cams_out, points = prob.get_state()
        structure = prob.structure(want_uv=False)
    rot_out = quaternions_to_rotations(cams_out[:, 3:7])
    return {"rots": [rot_out[v] if located[v] else None for v in range(n_views)],
            "centres": [cams_out[v, 0:3].reshape(3, 1).copy() if located[v] else None for v in range(n_views)], "points": points,
            "key_track": key_track, "summary": summary, "verdicts": verdicts, "poses": poses, "pair_mask": pair_mask, "cameras": cams_out,
            "rots_averaged": rots, "centres_averaged": centres,
            "pt_ptr": structure[0], "cam_idx": structure[1], "cost": np.array(cost)}


def _guided_model(model):
    """(gate name, (3, 3) matrix) of a ``model`` argument of the guided-matching entry points."""
    try:
        kind, mat = model
    except (TypeError, ValueError):
        raise ValueError("model must be ('fundamental', F) or ('homography', H), got {!r}".format(model))
    if kind not in ("fundamental", "homography"):
        raise ValueError("model must be ('fundamental', F) or ('homography', H), got kind {!r}".format(kind))
    mat = np.asarray(mat, dtype=np.float64)
    if mat.shape != (3, 3):
        raise ValueError("the {} model must be a (3, 3) matrix, got shape {}".format(kind, mat.shape))
    return kind, mat


def guided_pairs(tracker, ref_idx, que_idx, max_px=2.0, ratio=matching.RATIO, model=None, write=False, max_hyp=128, iteration=2):
    """Guided matching of two views of a ``HipDeviceKeyTracker`` (no reference counterpart): the descriptor search
    repeated with the candidates of every query key restricted to the reference keys a verified two-view model admits
    within ``max_px`` pixels, so that a look-alike off the epipolar line no longer fails the ratio test.

    ``model`` is ``("fundamental", F)`` or ``("homography", H)`` in pixel coordinates, the reference view left and the
    query view right; with ``model=None`` the fundamental matrix comes from ``verify_pairs`` over the pairs the tables
    hold, and ``None`` is returned when no model stands (``tracker.twoview_last`` keeps the status).  One
    ``TrackStore.match_guided`` on the tracker's resident descriptor sets and coordinates (nothing goes up), then
    ``matching.filter_guided``: mutual best neighbours among the admitted pairs that pass the ratio test (``ratio`` 0.7 is
    the reference's constant) or have no admitted rival.  Returns ``r_idx (1, n), q_idx (1, n)`` sorted by reference key.
    ``write=True`` replaces the matches of the two views in the device tables by these pairs (``TrackStore.set_pairs``)
    and bumps their versions; nothing calls this on its own."""
    n_views = len(tracker.track_list)
    if ref_idx < 0 or que_idx < 0 or ref_idx >= n_views or que_idx >= n_views or ref_idx == que_idx:
        print('{}:{} - invalid ref_idx {} or invalid que_idx {}'.format(
            tracker.__class__.__name__, 'guided_pairs', ref_idx, que_idx))
        return None
    if not float(max_px) >= 0.0:
        raise ValueError("max_px must be >= 0, got {!r}".format(max_px))
    if model is None:
        verify_pairs(tracker, ref_idx, que_idx, max_px, max_hyp, iteration)
        if tracker.twoview_last["status"] & (native.TWOVIEW_TOO_FEW | native.TWOVIEW_NO_MODEL):
            return None
        model = ("fundamental", tracker.twoview_last["fund_mat"])
    kind, mat = _guided_model(model)
    sets = tracker.__dict__.get("_hip_desc", {})
    if ref_idx not in sets or que_idx not in sets:
        raise native.SfmHipError("guided_pairs: the descriptors of view {} or {} are not resident".format(ref_idx, que_idx))
    ref_set, que_set = sets[ref_idx][1], sets[que_idx][1]
    import torch
    stream = tracker.__dict__.get("_guided_stream")
    if stream is None:
        stream = tracker.__dict__["_guided_stream"] = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        best = torch.empty((1, que_set.n), dtype=torch.int32, device="cuda")
        d0 = torch.empty((1, que_set.n), dtype=torch.float32, device="cuda")
        d1 = torch.empty((1, que_set.n), dtype=torch.float32, device="cuda")
        mutual = torch.empty((1, que_set.n), dtype=torch.uint8, device="cuda")
        tracker._store.match_guided(que_idx, que_set, [ref_idx], [ref_set], [kind], [mat], float(max_px) ** 2,
                                    d_best_idx=best.data_ptr(), d_best_dist=d0.data_ptr(), d_second_dist=d1.data_ptr(),
                                    d_mutual=mutual.data_ptr(), stream=stream.cuda_stream)
        best, d0, d1, mutual = (t.cpu().numpy()[0] for t in (best, d0, d1, mutual))
    q, t = matching.filter_guided(best, d0, d1, mutual, ratio)
    order = np.argsort(t, kind="stable")
    r_idx, q_idx = t[order], q[order]
    if write:
        tracker._store.set_pairs(ref_idx, que_idx, r_idx, q_idx)
        tracker._versions[ref_idx] += 1
        tracker._versions[que_idx] += 1
    return r_idx.reshape(1, -1).astype(int), q_idx.reshape(1, -1).astype(int)


def _resident_sets(tracker, who, n_views=None):
    sets = tracker.__dict__.get("_hip_desc", {})
    n = len(sets) if n_views is None else n_views
    missing = [v for v in range(n) if v not in sets]
    if n == 0 or missing:
        raise native.SfmHipError("{}: the descriptors of view {} are not resident".format(who, missing[0] if missing else 0))
    return [sets[v][1] for v in range(n)]


def register_views(tracker, views):
    """Bring ``views`` into a ``HipDeviceKeyTracker`` without matching them (``_register_views``: coordinates and descriptors go
    up, the tables get their empty rows), so that ``select_pairs`` and ``match_pairs`` can follow.  A function of the module:
    the tracker's class keeps the reference's public methods and ``kt_release`` only.  Returns the number of views added."""
    if not isinstance(tracker, HipDeviceKeyTracker):
        raise TypeError("register_views runs on a HipDeviceKeyTracker, got {}".format(type(tracker).__name__))
    return tracker._register_views(views)


def select_pairs(tracker, K=64, iters=4, seed=1, k=8, min_score=-np.inf, mutual=False, sequential=0, vocab=None):
    """Which pairs of views to match (no reference counterpart; include/sfm_hip.h, block "view pairs"), from the resident
    descriptor sets of a ``HipKeyTracker`` or ``HipDeviceKeyTracker`` (views 0 .. n - 1, e.g. after ``register_views``): a
    vocabulary of ``K`` words trained on them by ``iters`` rounds (``native.vocab_train``; or ``vocab``, uint8 (K, D) words
    from elsewhere), one VLAD descriptor per view (``native.view_describe``), every view's ``k`` best partners by score and
    the list of pairs (``native.view_pairs``): a < b is listed iff one lists the other (``mutual``: both do) or
    ``b - a <= sequential``.  Returns ``(pairs, verdict)``: the list of ``(ref_idx, que_idx)``, ref < que, sorted, that
    ``match_pairs``, ``orient_views`` and ``reconstruct_views`` take, and a dict of ``nbr``, ``nbr_score``, ``how``,
    ``pair_score``, ``word_count``, ``norm2``, ``words`` and ``log`` (None with a given vocabulary).  Nothing calls this on
    its own."""
    sets = _resident_sets(tracker, "select_pairs")
    log = None
    if vocab is None:
        words, log = native.vocab_train(sets, K, iters, seed)
    else:
        words = np.ascontiguousarray(vocab, dtype=np.uint8)
        if words.ndim != 2 or words.shape[1] != sets[0].dim:
            raise ValueError("vocab must be uint8 (K, {}), got shape {}".format(sets[0].dim, words.shape))
    with native.DescriptorSet(native.MATCH_L2, words) as voc:
        d = native.view_describe(voc, sets, outputs=("desc", "norm2", "word_count"))
    p = native.view_pairs(d["desc"], d["norm2"], k, min_score, mutual, sequential)
    verdict = dict(nbr=p["nbr"], nbr_score=p["nbr_score"], how=p["how"], pair_score=p["pair_score"], word_count=d["word_count"],
                   norm2=d["norm2"], words=words, log=log)
    return [(int(a), int(b)) for a, b in p["pairs"]], verdict


def match_pairs(tracker, views, pairs, is_knn_match=None):
    """Match only the listed ``pairs`` of ``views`` into the tables of a ``HipDeviceKeyTracker`` (no reference counterpart).

    The views not yet in the store are registered without matching (``_register_views``).  Then, for every query view, ONE
    ``TrackStore.match_guided`` with no gate over its listed earlier views -- the neighbours ``sfm_match`` gives, bit for bit
    -- followed by what the host tracker does with them (``matching.filter_matches``, the duplicate removal of quirk Q14,
    ``matching.table_writes``) and ``TrackStore.set_pairs``: the rows of a listed pair are those ``add_new_view`` writes
    for it, the rows of every other pair stay -1.  ``pairs`` holds ``(ref_idx, que_idx)`` in either order; a pair listed
    twice is matched once.  The fundamental-inlier option (quirk Q15) is not supported.  Returns the number of pairs
    matched."""
    if not isinstance(tracker, HipDeviceKeyTracker):
        raise TypeError("match_pairs runs on a HipDeviceKeyTracker, got {}".format(type(tracker).__name__))
    if tracker.is_fund_inlier:
        raise ValueError("match_pairs does not support is_fund_inlier (quirk Q15): match with add_new_view instead")
    if not is_knn_match:                                                        # falsy -> instance default, as add_new_view
        is_knn_match = tracker.is_knn_match
    n_views = len(views)
    by_query = {}
    for a, b in pairs:
        a, b = int(a), int(b)
        if a == b or min(a, b) < 0 or max(a, b) >= n_views:
            raise ValueError("pair ({}, {}) must name two different views in 0 .. {}".format(a, b, n_views - 1))
        by_query.setdefault(max(a, b), set()).add(min(a, b))
    tracker._register_views(views)
    sets = _resident_sets(tracker, "match_pairs", n_views)
    cross = bool(tracker.is_cross_check)
    import torch
    stream = tracker.__dict__.get("_guided_stream")
    if stream is None:
        stream = tracker.__dict__["_guided_stream"] = torch.cuda.Stream()
    done = 0
    for que in sorted(by_query):
        refs = sorted(by_query[que])
        query = sets[que]
        for r in refs:
            if sets[r].n == 0:      # undefined without cv2 (deviation of Q16)
                raise ValueError("reference view {} has no descriptors".format(r))
        if query.n == 0:
            continue
        shape = (len(refs), query.n)
        with torch.cuda.stream(stream):
            bi = torch.empty(shape, dtype=torch.int32, device="cuda")
            si = torch.empty(shape, dtype=torch.int32, device="cuda")
            bd = torch.empty(shape, dtype=torch.float32, device="cuda")
            sd = torch.empty(shape, dtype=torch.float32, device="cuda")
            mu = torch.zeros(shape, dtype=torch.uint8, device="cuda")
            tracker._store.match_guided(que, query, refs, [sets[r] for r in refs], ["none"] * len(refs), np.zeros((len(refs), 9)), 0.0,
                                        d_best_idx=bi.data_ptr(), d_best_dist=bd.data_ptr(), d_second_idx=si.data_ptr(),
                                        d_second_dist=sd.data_ptr(), d_mutual=mu.data_ptr() if cross else 0, stream=stream.cuda_stream)
            bi, bd, si, sd, mu = (t.cpu().numpy() for t in (bi, bd, si, sd, mu))
        for i, ref in enumerate(refs):
            q, t, d = matching.filter_matches(bi[i], bd[i], si[i], sd[i], mu[i].astype(bool), is_knn_match, cross)
            wq, wt = matching.table_writes(q, t, d)
            tracker._store.set_pairs(ref, que, wt, wq)
            tracker._versions[ref] += 1
            done += 1
        tracker._versions[que] += 1
    return done


class HipKeyPoint:
    """The ``cv2.KeyPoint`` fields the reference reads and writes (view_processor.py:100-101, 178-180)."""
    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x=0.0, y=0.0, size=0.0, angle=-1.0, response=0.0, octave=0, class_id=-1):
        self.pt = (float(x), float(y))
        self.size = float(size)
        self.angle = float(angle)
        self.response = float(response)
        self.octave = int(octave)
        self.class_id = int(class_id)

    def __repr__(self):
        return "HipKeyPoint(pt=%r, size=%r, angle=%r, response=%r, octave=%d)" % (
            self.pt, self.size, self.angle, self.response, self.octave)


def keypoints_from_arrays(kp):
    """HipKeyPoint list of a ``native.sift_detect`` result (float32 fields widened to Python floats, as cv2 does)."""
    return [HipKeyPoint(x, y, s, a, r, o) for x, y, s, a, r, o in
            zip(kp["x"].tolist(), kp["y"].tolist(), kp["size"].tolist(), kp["angle"].tolist(), kp["response"].tolist(),
                kp["octave"].tolist())]


class HipViewProcessorMixin:
    """``ViewProcessor.__extract_keys`` (view_processor.py:199-202) with SIFT detection on the device: returns
    (list of HipKeyPoint, float32 (n, 128) descriptors), what ``detectAndCompute(img, None)`` returns for
    ``SIFT_create()`` by the contract of INTEGRATION.md 'SIFT detection'.  An image without keypoints gives
    ``([], None)``, as cv2 does.  ``_hip_extract_keys`` returns the same two and the coordinates as an (n, 2) float64
    array: the float32 values widened exactly, what ``key_pts[i].pt`` holds."""

    def _hip_extract_keys(self, img):
        if getattr(self, "key_type", "sift") != "sift":
            raise ValueError("HipViewProcessorMixin: only key_type 'sift' runs on the device, got %r" % (self.key_type,))
        kp = native.sift_detect(img)
        if len(kp["x"]) == 0:
            return [], None, np.zeros((0, 2))
        return keypoints_from_arrays(kp), kp["descriptors"], np.stack((kp["x"], kp["y"]), axis=1).astype(np.float64)

    def _ViewProcessor__extract_keys(self, img):
        return self._hip_extract_keys(img)[:2]


class HipView:
    """Standalone View (view_processor.py:14-106): the same constructor fields, ``update_cam_pose``,
    ``update_intrinsic_mat`` and ``write_keys``."""

    def __init__(self, img, idx, k, key_pts, key_descriptors):
        self.img = img
        self.idx = idx
        self.ref_idx = idx
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors
        self.rot = np.identity(3, dtype=float)
        self.loc = np.zeros((3, 1), dtype=float)
        self.k = k
        self.cam_pose = np.hstack((self.rot, self.loc))
        self.cam_proj = self.k @ np.hstack((self.rot.T, self.rot.T @ -self.loc))
        self.is_valid = False

    def update_cam_pose(self, rot, loc):
        self.rot = rot
        self.loc = loc
        self.cam_pose = np.hstack((self.rot, self.loc))
        self.cam_proj = self.k @ np.hstack((self.rot.T, self.rot.T @ -self.loc))

    def update_intrinsic_mat(self, k):
        self.k = k
        self.cam_proj = self.k @ np.hstack((self.rot.T, self.rot.T @ -self.loc))

    def write_keys(self, key_file_path):
        if key_file_path[-4:] != '.pkl':
            logging.error('%s : incorrect key file path : %s', self.__class__.__name__, key_file_path)
            return
        temp_array = []
        for idx, point in enumerate(self.key_pts):
            temp_array.append((point.pt, point.size, point.angle, point.response, point.octave, point.class_id,
                               self.key_descriptors[idx]))
        with open(key_file_path, 'wb') as keys_file:
            pickle.dump(temp_array, keys_file)


class HipViewProcessor(HipViewProcessorMixin):
    """Standalone ViewProcessor (view_processor.py:110-202) without cv2: ``generate_view``, ``add_view`` and keys read
    back from ``.pkl``.  ``key_type='orb'`` raises ``ValueError``: the reference's ``cv.ORB_create(nkeys=1500)`` names
    no ORB_create argument (INTEGRATION.md 'SIFT detection'); any other key type also raises, where the reference
    logs and calls ``sys.exit(0)``."""

    def __init__(self, key_type='sift'):
        if key_type != 'sift':
            raise ValueError("HipViewProcessor: only key_type 'sift' is supported, got %r" % (key_type,))
        self.key_type = key_type
        self.view_list = []

    def add_view(self, view):
        self.view_list.append(view)

    def generate_view(self, img, index, k, key_path=None):
        if not key_path:
            key_pts, key_descriptors, key_xy = self._hip_extract_keys(img)
        else:
            key_pts, key_descriptors = self._ViewProcessor__read_keys(key_path, img)
            key_xy = np.array([p.pt for p in key_pts], dtype=np.float64).reshape(-1, 2)
        view = HipView(img, index, k, key_pts, key_descriptors)
        view.key_xy = key_xy              # (n, 2) float64 of key_pts[i].pt, read by HipDeviceKeyTracker
        return view

    def _ViewProcessor__read_keys(self, key_path, img):
        try:
            if key_path[-4:] != '.pkl':
                logging.error('%s : incorrect key file path : %s', self.__class__.__name__, key_path)
                return None
            with open(key_path, 'rb') as f:
                keys = pickle.load(f)
            key_pts = [HipKeyPoint(p[0][0], p[0][1], p[1], p[2], p[3], p[4], p[5]) for p in keys]
            key_descriptors = np.array([p[6] for p in keys])
            return key_pts, key_descriptors
        except FileNotFoundError:
            logging.error('%s : pkl file %s not found ', key_path, self.__class__.__name__)
            return self._ViewProcessor__extract_keys(img)
