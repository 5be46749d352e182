/* sfm_hip.h — C-ABI of libsfm_hip.so: the MI355X (gfx950) back end for the nonlinear-refinement
 * hot path of willSapgreen/structure-from-motion.
 *
 * The reference is pure Python and has no FFI layer; its boundary for this path is the public
 * method surface of three classes.  Every entry point below names the reference interface it
 * replaces (file:line relative to the reference repo).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions (identical to the reference): float64 everywhere; rot = R (3x3 row-major),
 * loc = C (camera centre); world->camera p = R^T (X - C); quaternion [qw,qx,qy,qz]; a camera
 * parameter block is 7 doubles [Cx,Cy,Cz,qw,qx,qy,qz] (ba_processor.py:285-288); 3D points are
 * homogeneous columns; 2D points are pixel columns [u,v,1].
 *
 * Unless a function says "device", all pointers are HOST memory borrowed for the duration of the
 * call; outputs are caller-allocated.  Calls are blocking (they synchronise the library stream)
 * except sfm_ba_iterate / sfm_ba_linearize_reduce / sfm_ba_solve_update, which only enqueue.
 * No exception crosses the boundary: every function returns SFM_OK (0) or a negative status;
 * sfm_last_error() returns a message for the calling thread's last failure.
 */
#ifndef SFM_HIP_H
#define SFM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------------------------- */
#define SFM_OK               0
#define SFM_E_SHAPE         -1   /* bad sizes -> ValueError (campose_processor.py:353-357, triangulation_processor.py:65-74) */
#define SFM_E_BAD_ROTATION  -2   /* verify_rotation_mat failed -> ValueError (utils.py:43-45, 93-95) */
#define SFM_E_QW_ZERO       -3   /* |qw| < 1e-6 -> ValueError (utils.py:49-51) */
#define SFM_E_SQRT_DOMAIN   -4   /* 1 + tr R < 0 -> math.sqrt ValueError (utils.py:47) */
#define SFM_E_HIP           -5   /* HIP runtime error */
#define SFM_E_NO_DEVICE     -6   /* no gfx950 device visible */
#define SFM_E_HANDLE        -7   /* null / destroyed problem handle */
#define SFM_E_RCCL          -9   /* the RCCL library could not be loaded, or one of its calls failed (sfm_comm_*, sfm_ba_set_comm) */
#define SFM_E_RANK          -8   /* rank-2 projection of a fundamental / essential matrix is not rank 2 -> ValueError (epipolar_processor.py:187-190, 90-93) */

/* ---- quirk bits; the reference's behaviour = SFM_QUIRKS_REFERENCE ------ */
#define SFM_Q1_PNP_ROW_OVERLAP  1  /* campose_processor.py:404-405: rows stored at [pt:pt+2] */
#define SFM_Q2_LOC_JAC_SIGN     2  /* campose_processor.py:802-804: sign of the v-row of d/dC */
#define SFM_QUIRKS_REFERENCE    3
/* Q13 (not a selectable bit: it is not a property of the arithmetic but of the host's LAPACK): the six-point DLT of the
 * linear PnP (campose_processor.py:565-633) negates loc together with rot when det(rot) < 0 (campose:629-631).  rot and
 * the null vector it comes from flip sign together, loc = rot @ -cam_mat[:, 3] / s does not -- so whether that branch
 * is taken, and with it whether the returned centre is C or -C, depends on the arbitrary sign LAPACK gives the
 * last right-singular vector.  Measured on the reference's own PnP fixture (tests/golden/g5_pnp.npz, 300 seeded
 * hypotheses) and on the captured per-view chains (tests/golden/g10_incremental_*.npz): the branch fires for about half
 * of the hypotheses, each of which then usually scores next to nothing -- so the reference's winner is the first
 * best hypothesis AMONG THOSE ITS LAPACK DID NOT RUIN, typically not the first best hypothesis.
 * The device returns the sign-invariant centre C for every hypothesis (sfm_pnp_linear_ransac: the sane RANSAC).
 * Reproducing the reference needs the host's LAPACK, so it is split (round 4): sfm_pnp_ransac_evaluate returns every
 * hypothesis' pose and its inlier counts under (R, C) AND under (R, -C); the Python drop-in asks NumPy -- the very
 * library the reference would have asked -- for the branch decision of the few hypotheses that can win
 * (structure-from-motion_amd/q13.py), picks the reference's winner and fetches its inlier mask with
 * sfm_pnp_inlier_mask.  tests/test_gpu_linear_and_incremental.py asserts the per-hypothesis facts on the reference's
 * fixture, tests/test_gpu_chain_golden.py the winners, inlier lists and RNG stream of whole per-view chains. */
#define SFM_Q13_PNP_LOC_SIGN_UNDEFINED 0

/* ---- Schur-product algorithm selection (sfm_ba_set_option SFM_OPT_SCHUR) ---------------------- */
#define SFM_SCHUR_AUTO    0  /* the cheapest of the three below by cost models fitted on MI355X */
#define SFM_SCHUR_PAIRS   1  /* sparse product over 18 x 18-camera LDS tiles: only camera pairs that share a point (small scenes) */
#define SFM_SCHUR_MFMA    2  /* dense v_mfma_f64_16x16x4 SYRK over the materialised, zero-filled Z (LDS-DMA staged; high visibility) */
#define SFM_SCHUR_ROWS    3  /* sparse product over LDS row panels: one observation owns its camera's block row of its point's
                              * contribution (many cameras at low visibility: BASELINE config 4) */

#define SFM_OPT_SCHUR        1
#define SFM_OPT_DEBUG        3  /* profiling ablations of the Schur kernel (1 no MFMA, 4 no staging DMA: results are wrong when set; 8 = record clock stamps; 16 = keep ba_backsub and ba_linearize as separate launches, 64 = block column steps even for P <= 56 (no single-launch small-system solve), 256 = single-launch solve up to P = 64 instead of 56, 512 = block-row back substitution instead of dp = L^-T y with the inverse carried through the column steps, 128 = never pick the row-panel sparse product, 1024 = the column steps of the reduced solve as separate launches (ba_chol_step) where the single data-flow launch would run (9 to 237 cameras), 2048 = dp = X y and the camera update as their own launch (ba_inv_apply) behind the data-flow launch, 4096 = its tasks dealt by workgroup index instead of taken by ticket (A/B only: needs every workgroup of the launch resident): results unchanged; the environment variable SFM_FLOW_SOLVE=0 selects the column-step launches (bit 1024) for every handle of the process; 8192 = test of the data-flow launch's bounded waits: one hand-over is never announced, every wait gives up after 20 000 polls and the solve reports SFM_E_HIP; 16384 = the split-K reduce of the dense product always as its own launch (sfm_ba_iterate on one GPU otherwise leaves it to the first tasks of the data-flow launch: same sums in a fixed order); 32768 = sfm_ba_refine_cameras works on cameras of size class 3 with the launches of class 4 (A/B only: same slice order) */
#define SFM_OPT_DETERMINISTIC 4 /* 1: fixed summation order everywhere -- one wave per ba_linearize workgroup (ordered LDS accumulation), the
                                 * atomic-free dense Schur product, a single-writer split-K / camera-accumulator reduce.  Two runs from the
                                 * same state then agree bit for bit (the default path agrees to ~1e-13).  Needs the dense product to fit
                                 * and V <= 234; slower (C3: see DESIGN.md). */
#define SFM_OPT_GRAPH         5 /* 1: sfm_ba_iterate captures the steady-state iteration body (fused linearise, Schur product, reduce,
                                 * reduced solve) as a hipGraph -- one per camera-slot parity -- and replays it for every iteration
                                 * after the first; same kernels, same arguments, same results.  Off by default: on this stack the
                                 * kernels of an iteration already run back to back from eager launches. */
#define SFM_OPT_TIMING_STRIDE 6 /* bracket a timed kernel class only every value-th time it runs (default 1): an event pair costs two
                                 * ~6 us stream bubbles on this stack, so a measurement that must not disturb what it measures samples */
#define SFM_OPT_TIMING       2  /* bitmask (1 << SFM_K_x): bracket those kernel classes with hipEvents */

/* ---- robust loss of the resident bundle adjustment (sfm_ba_set_loss) -------------------------- */
#define SFM_LOSS_NONE    0  /* plain sum of squares, as the reference (ba_processor.py:376) */
#define SFM_LOSS_HUBER   1  /* rho(s) = s for s <= 1, else 2 sqrt(s) - 1;  w(s) = 1 for s <= 1, else 1 / sqrt(s) */
#define SFM_LOSS_CAUCHY  2  /* rho(s) = log1p(s);  w(s) = 1 / (1 + s) */

/* ---- items of sfm_ba_info -------------------------------------------------------------------------- */
#define SFM_INFO_SCHUR_KERNEL  1  /* SFM_SCHUR_PAIRS / SFM_SCHUR_MFMA / SFM_SCHUR_ROWS: the product kernel the next iteration launches
                                   * (asking builds the row-panel product's work split if that is the candidate, so the answer is
                                   * the kernel that will run, not the one that was hoped for).  NOT a pure query: when it has
                                   * to build that split it completes a deferred back substitution (as sfm_ba_flush does) and
                                   * enqueues kernels on the problem's stream -- do not ask between sfm_ba_linearize_reduce and
                                   * sfm_ba_solve_update of one iteration, nor inside a stream capture */
#define SFM_INFO_UPLOAD_BYTES  2  /* host -> device bytes moved on behalf of this handle since sfm_ba_create */
#define SFM_INFO_N_CAMS        3
#define SFM_INFO_N_PTS         4
#define SFM_INFO_N_OBS         5
#define SFM_INFO_MAX_TRACK     6  /* longest track (observations of one point) */
#define SFM_INFO_GRAPH_REPLAYS 7  /* iterations sfm_ba_iterate carried out as hipGraph replays (SFM_OPT_GRAPH) */
#define SFM_INFO_REDUCE_IN_SOLVE 8 /* 1 if the last iteration sfm_ba_iterate enqueued left the split-K reduce of the dense product to the
                                   * data-flow solve's launch (no ba_schur_reduce launch: one GPU, 37 to 237 cameras, not deterministic), else 0 */
#define SFM_INFO_PCG_HELD_POINTS 9 /* points whose D_p was not positive definite or not finite in the last outer iteration of
                                   * sfm_ba_iterate_pcg: they were held for that iteration (arises only at lambda = 0) */
#define SFM_INFO_SOLVE_PATH    10 /* how the next reduced camera solve runs: SFM_SOLVE_SMALL (one workgroup, up to 8 cameras), SFM_SOLVE_FLOW
                                   * (the persistent data-flow launch: 9 to 237 cameras on a device of at least 2 compute units) or
                                   * SFM_SOLVE_STEPS (one launch per block column) */
#define SFM_SOLVE_SMALL 0
#define SFM_SOLVE_FLOW  1
#define SFM_SOLVE_STEPS 2

/* ---- kernel ids for sfm_ba_kernel_time ------------------------------------------------------- */
#define SFM_K_PREP       0
#define SFM_K_LINEARIZE  1
#define SFM_K_SCHUR      2
#define SFM_K_SOLVE      3
#define SFM_K_BACKSUB    4
#define SFM_K_REDUCE     5  /* ba_schur_reduce: split-K slabs + camera accumulators -> [S | rhs] */
#define SFM_K_COUNT      6

/* ---- library / device ------------------------------------------------------------------------ */
int sfm_version(void);
/* Select the HIP device this process drives (one process per GPU) and create the library stream. */
int sfm_init(int device);
int sfm_shutdown(void);
/* Default stream of the library (hipStream_t as void*): the host-pointer entry points run on it and a new BA
 * problem starts on it.  NULL = the library's own stream (created by sfm_init, alive until sfm_shutdown).
 * A resident BA problem keeps the stream it was given (sfm_ba_set_stream), whatever this is set to later. */
int sfm_set_stream(void* hip_stream);
int sfm_synchronize(void);
/* A hook for tests, in the sense of sfm_rotation_plan's cap_bytes: every launch shape and plan that depends on the device's
 * compute-unit count is made for min(n, the device's count) from now on, so that the plans of a partitioned MI355X (CPX: 32
 * compute units per logical device, QPX 64, DPX 128) can be run on a whole one.  n = 0 removes the limit; n < 0 is
 * SFM_E_SHAPE.  The effective count never exceeds the device's own: more would oversubscribe launches whose workgroups
 * wait for each other.  Works before sfm_init (the host-only plan functions then see min(n, 256)) and survives
 * sfm_shutdown.  A resident BA problem sized its workspaces from the plans of its creation: while any sfm_ba_problem
 * exists the call returns SFM_E_SHAPE and changes nothing.  The workgroups still run on every compute unit of the device:
 * the limit shapes the plans, it does not mask hardware. */
int sfm_set_cu_limit(int n);
/* *device = the device's compute units (256 before sfm_init), *effective = what the plans see.  Either may be NULL. */
int sfm_cu_count(int* device, int* effective);
/* Diagnostic: 1 when the process runs with SFM_POOL_REDZONE=1 -- every device buffer of the library then sits between
 * two 4 KB zones of 0xA5 that are checked (after a device-wide synchronise) whenever the buffer goes back to the pool;
 * a kernel that wrote outside its buffer aborts the process with a message.  For test runs only. */
int sfm_pool_redzone_active(void);
/* Diagnostic: pool mode bits (1 = SFM_POOL_REDZONE, 2 = SFM_POOL_GUARD: every device buffer is its own virtual-memory
 * mapping that ends where the buffer ends, followed by a reserved, unmapped granule -- an out-of-bounds READ past the end
 * faults at the access; one test pass on the GPU box runs under it).  *tail_slack = mapped bytes behind a probe buffer of
 * probe_bytes (guard mode: < 16; -1 before sfm_init), *guard_allocs = buffers handed out in guard mode so far. */
int sfm_pool_mode(int64_t probe_bytes, int64_t* tail_slack, int64_t* guard_allocs);
const char* sfm_last_error(void);

/* ---- unit-level helpers (parity hooks; batched) ------------------------------------------------ */
/* utils.convert_quaternion_to_rotation (utils.py:64-97).  status[i] = SFM_OK / SFM_E_BAD_ROTATION. */
int sfm_quat_to_rot(int n, const double* q /*[n][4]*/, double* R /*[n][9]*/, int* status /*[n]*/);
/* utils.convert_rotation_to_quaternion (utils.py:28-60). */
int sfm_rot_to_quat(int n, const double* R /*[n][9]*/, double* q /*[n][4]*/, int* status /*[n]*/);
/* CamposeProcessor.construct_jacobian_matrix(rot, loc, pt_3d) -> (2,7) (campose_processor.py:462-482). */
int sfm_jac_cam(int n, const double* R /*[n][9]*/, const double* C /*[n][3]*/, const double* X /*[n][4]*/,
                int quirks, double* Jp /*[n][2][7]*/, int* status /*[n]*/);
/* TriangulationProcessor.construct_jacobian_matrix(tri_3d_pt, projs, num_views) -> (2*num_views,3)
 * (triangulation_processor.py:237-271). */
int sfm_jac_pt(int n, int n_views, const double* projs /*[n][n_views][3][4]*/, const double* X /*[n][4]*/,
               double* Jx /*[n][2*n_views][3]*/);

/* ---- TriangulationProcessor.nonlinear_triangulate (triangulation_processor.py:160-234) --------- */
/* One thread per point, all iterations in registers.  Row W of X is carried through unchanged. */
int sfm_tri_nonlinear(int m, int n_views, const double* projs /*[n_views][3][4]*/,
                      const double* uv /*[n_views][2][m]*/, const double* X_in /*[4][m]*/,
                      double lambda, int iters, double* X_out /*[4][m]*/);

/* ---- TriangulationProcessor.linear_triangulate (triangulation_processor.py:91-157) ------------------ */
/* DLT: per point the null vector of the (2 n_views x 4) matrix of rows u P[2,:] - P[0,:], v P[2,:] - P[1,:],
 * divided by its W (streaming Givens QR + one-sided Jacobi SVD per thread). */
int sfm_tri_linear(int m, int n_views, const double* projs /*[n_views][3][4]*/, const double* uv /*[n_views][2][m]*/,
                   double* X_out /*[4][m]*/);
/* TriangulationProcessor.triangulate (triangulation_processor.py:31-88): linear then nonlinear, the
 * initial points never leave the device. */
int sfm_triangulate(int m, int n_views, const double* projs /*[n_views][3][4]*/, const double* uv /*[n_views][2][m]*/,
                    double lambda, int iters, double* X_out /*[4][m]*/);

/* ---- CamposeProcessor.nonlinear_estimate_cam_pose_pnp (campose_processor.py:308-459) ----------- */
int sfm_pnp_nonlinear(int n, const double* uv_pix /*[3][n]*/, const double* X /*[4][n]*/,
                      const double K[9], const double R0[9], const double C0[3],
                      double lambda, int iters, int quirks, double R_out[9], double C_out[3]);
/* Independent views in one launch (one workgroup per view); view v owns columns
 * [offsets[v], offsets[v+1]) of uv_pix / X.  status[v] per view. */
int sfm_pnp_nonlinear_batch(int n_views, const int* offsets /*[n_views+1]*/, int total,
                            const double* uv_pix /*[3][total]*/, const double* X /*[4][total]*/,
                            const double* K /*[n_views][9]*/, const double* R0 /*[n_views][9]*/,
                            const double* C0 /*[n_views][3]*/, double lambda, int iters, int quirks,
                            double* R_out /*[n_views][9]*/, double* C_out /*[n_views][3]*/,
                            int* status /*[n_views]*/);

/* ---- DEVICE-pointer, stream-ordered forms of the calls above ---------------------------------------------- */
/* Same kernels, same layouts, but every pointer is DEVICE memory, the work is only ENQUEUED on `hip_stream`
 * (hipStream_t as void*; NULL = the library stream) and the call returns without synchronising: the per-view loop of
 * the reference (PnP at ba_processor.py:191, triangulate at :246, BA at :267) can chain them on one stream around a
 * resident BA problem.  d_status of the PnP form is read by the caller after its own synchronisation
 * (SFM_OK / SFM_E_BAD_ROTATION / SFM_E_QW_ZERO / SFM_E_SQRT_DOMAIN per view).  d_X_out may equal d_X_in. */
int sfm_tri_nonlinear_dev(int m, int n_views, const double* d_projs /*[n_views][3][4]*/, const double* d_uv /*[n_views][2][m]*/,
                          const double* d_X_in /*[4][m]*/, double lambda, int iters, double* d_X_out /*[4][m]*/, void* hip_stream);
int sfm_tri_linear_dev(int m, int n_views, const double* d_projs, const double* d_uv, double* d_X_out /*[4][m]*/, void* hip_stream);
int sfm_triangulate_dev(int m, int n_views, const double* d_projs, const double* d_uv, double lambda, int iters,
                        double* d_X_out /*[4][m]*/, void* hip_stream);
int sfm_pnp_nonlinear_batch_dev(int n_views, const int* d_offsets /*[n_views+1]*/, int total, const double* d_uv_pix /*[3][total]*/,
                                const double* d_X /*[4][total]*/, const double* d_K /*[n_views][9]*/, const double* d_R0 /*[n_views][9]*/,
                                const double* d_C0 /*[n_views][3]*/, double lambda, int iters, int quirks,
                                double* d_R_out /*[n_views][9]*/, double* d_C_out /*[n_views][3]*/, int* d_status /*[n_views]*/,
                                int max_view_points /* size of the largest view (the offsets are on the device); 0 = unknown.
                                                       Views of up to 1024 points and larger ones run on different kernels, each
                                                       launched over the whole batch; a truthful value <= 1024 saves the second
                                                       launch.  A view's result depends on its own size only, never on the batch.
                                                       A view LARGER than a non-zero value is not refined: d_R_out, d_C_out are its
                                                       d_R0, d_C0 and its d_status is SFM_E_SHAPE; the call still returns SFM_OK, and
                                                       every view within the value gets what a truthful call gives it. */,
                                void* hip_stream);
/* X_out[4][n] = (px, py, pz, 1)[index[i]]: the 2D-3D association of ba_processor.py:184-188 (np.take of tri_pts) for points
 * that already live on the device (sfm_ba_points_ptr), so that the per-view PnP uploads keys and indices only. */
int sfm_gather_points_dev(int n, const int* d_index /*[n]*/, const double* d_px, const double* d_py, const double* d_pz,
                          double* d_X_out /*[4][n]*/, void* hip_stream);

/* ---- CamposeProcessor.linear_estimate_cam_pose_pnp (campose_processor.py:249-305, 485-633) ----------- */
/* RANSAC over 6-point DLT hypotheses.  The caller draws the n_hyp six-point samples (the reference uses
 * Python's global `random.sample`, campose:531, so the host keeps the RNG stream); the device solves every
 * hypothesis (12x12 null vector + 3x3 polar factor), scores all points against `threshold` in pixels and
 * returns the FIRST hypothesis with the largest inlier count, its inlier mask and count.  If no hypothesis
 * has an inlier the reference's initial identity pose is returned with *best_hypothesis = -1. */
int sfm_pnp_linear_ransac(int n, const double* uv_pix /*[3][n]*/, const double* X /*[4][n]*/, const double K[9],
                          int n_hyp, const int* samples /*[n_hyp][6]*/, double threshold,
                          double R_out[9], double C_out[3], int* inlier_mask /*[n]*/, int* n_inliers,
                          int* best_hypothesis);

/* The same hypotheses, for a caller that reproduces quirk Q13 (above): pose (R, C) of every six-point sample, its inlier
 * count under (R, C) and under (R, -C) -- what the reference scores when its det(rot) < 0 branch fired (campose:629-631). */
int sfm_pnp_ransac_evaluate(int n, const double* uv_pix /*[3][n]*/, const double* X /*[4][n]*/, const double K[9],
                            int n_hyp, const int* samples /*[n_hyp][6]*/, double threshold,
                            double* R_out /*[n_hyp][9]*/, double* C_out /*[n_hyp][3]*/, int* counts /*[n_hyp]*/,
                            int* counts_neg /*[n_hyp]*/);
/* Inlier mask and count of ONE pose: pixel reprojection error of every point against `threshold` (campose:544-554). */
int sfm_pnp_inlier_mask(int n, const double* uv_pix /*[3][n]*/, const double* X /*[4][n]*/, const double K[9],
                        const double R[9], const double C[3], double threshold, int* inlier_mask /*[n]*/, int* n_inliers);

/* CamposeProcessor.estimate_cam_pose_pnp (campose_processor.py:192-246) as two calls around the host's choice of the winner,
 * with the view's keys and points RESIDENT on the device in between: sfm_pnp_ransac_begin = sfm_pnp_ransac_evaluate + a
 * session; sfm_pnp_ransac_finish(session, R, C of the chosen hypothesis, ...) = the inlier mask of that pose, the inlier
 * columns compacted on the device in ascending order (campose:236-237) and `iters` nonlinear iterations on them
 * (campose:239) -- the result of sfm_pnp_inlier_mask followed by sfm_pnp_nonlinear on the gathered columns, bit for bit,
 * with one upload instead of three.  finish releases the session (also when it fails); sfm_pnp_session_destroy releases
 * one that is never finished. */
typedef struct sfm_pnp_session sfm_pnp_session;
int sfm_pnp_ransac_begin(int n, const double* uv_pix /*[3][n]*/, const double* X /*[4][n]*/, const double K[9],
                         int n_hyp, const int* samples /*[n_hyp][6]*/, double threshold,
                         double* R_out /*[n_hyp][9]*/, double* C_out /*[n_hyp][3]*/, int* counts /*[n_hyp]*/,
                         int* counts_neg /*[n_hyp]*/, sfm_pnp_session** out);
int sfm_pnp_ransac_finish(sfm_pnp_session* session, const double R[9], const double C[3], double threshold,
                          double lambda, int iters, int quirks, int* inlier_mask /*[n]*/, int* n_inliers,
                          double R_out[9], double C_out[3]);
int sfm_pnp_session_destroy(sfm_pnp_session* session);

/* Parity hook: every hypothesis of the RANSAC above -- pose and inlier count of each six-point sample
 * (campose_processor.py:524-560 loop body, 565-633). */
int sfm_pnp_six_point_hypotheses(int n, const double* uv_pix /*[3][n]*/, const double* X /*[4][n]*/, const double K[9],
                                 int n_hyp, const int* samples /*[n_hyp][6]*/, double threshold,
                                 double* R_out /*[n_hyp][9]*/, double* C_out /*[n_hyp][3]*/, int* counts /*[n_hyp]*/);

/* ---- Two-view initialisation ------------------------------------------------- */
/* EpipolarProcessor.determine_fundamental_mat (epipolar_processor.py:22-57 = __normalize 97-137,
 * __estimate_ransac 196-247 over __estimate_eight_pts 140-193, __denormalize 251-267).  left/right are rows 0-1
 * of the matched KeyPt arrays.  The caller draws the n_hyp eight-index samples (Python's `random.sample`,
 * epipolar:225); the device normalises the points, solves every hypothesis (8x9 null vector, rank-2 projection,
 * / f[2][2]), scores |x_r^T F x_l| < threshold on the normalised pairs and returns the FIRST hypothesis with
 * the largest inlier count, de-normalised and divided by F[2][2].  n == 8: the single estimate from all eight
 * pairs, every pair an inlier (epipolar:219-221; samples/n_hyp ignored).  n < 8: SFM_E_SHAPE.  A hypothesis whose
 * rank-2 projection has rank != 2: SFM_E_RANK (the reference raises ValueError, epipolar:187-190).  No hypothesis
 * with an inlier: *best_hypothesis = -1, mask all zero, F = NaN (the reference divides its zero matrix by
 * F[2][2] = 0, epipolar:216, 266). */
int sfm_fundamental_ransac(int n, const double* left /*[2][n]*/, const double* right /*[2][n]*/, int n_hyp,
                           const int* samples /*[n_hyp][8]*/, double threshold, double F_out[9],
                           int* inlier_mask /*[n]*/, int* n_inliers, int* best_hypothesis);
/* Parity hook: EpipolarProcessor.__estimate_eight_pts (epipolar_processor.py:140-193) for n_hyp samples of the
 * given (already normalised) pairs [n][4] = (x_l, y_l, x_r, y_r).  status[h] = SFM_OK / SFM_E_RANK. */
int sfm_fundamental_eight_point(int n, const double* pairs /*[n][4]*/, int n_hyp, const int* samples /*[n_hyp][8]*/,
                                double* F_out /*[n_hyp][9]*/, int* status /*[n_hyp]*/);
/* EpipolarProcessor.extract_essential_mat (epipolar_processor.py:60-95): E = U diag(1,1,0) V^T of
 * K_right^T F K_left, divided by E[2][2]. */
int sfm_essential_from_fundamental(const double F[9], const double K_left[9], const double K_right[9], double E_out[9]);
/* CamposeProcessor.extract_cam_pose_from_essential_mat (campose_processor.py:29-100): the two rotations
 * (R_out[0], R_out[1], camera->world convention of the reference's return value) and the centre c1 (c2 = -c1).
 * The reference's ORDER of (r1, r2) and SIGN of c1 follow LAPACK's singular-vector signs; the set of four
 * candidates {r1, r2} x {c1, -c1} is what is defined, and what callers (ba_processor.py:81-97) consume. */
int sfm_pose_candidates(const double E[9], double R_out[18], double C1_out[3]);
/* CamposeProcessor.evalulate_cam_pose_cheirality / disambiguate_cam_pose_four (campose_processor.py:102-189)
 * for k candidate (projection, point set) pairs against the reference projection P1: mask[c][i] = both depths
 * (third rows of P1 X, P2_c X) positive, counts[c] = their number, *best = FIRST candidate with the strictly
 * largest count starting from 0 (so 0 if no candidate has a valid point). */
int sfm_cheirality(int k, int n, const double P1[12], const double* P2 /*[k][12]*/, const double* X /*[k][4][n]*/,
                   int* mask /*[k][n]*/, int* counts /*[k]*/, int* best);

/* ---- BaProcessor.__execute_bundle_adjustment (ba_processor.py:274-439) ------------------------- */
/* Observations are sorted by (point, camera) — the reference's loop order (ba_processor.py:304-306)
 * — and given as a CSR over points: observation o in [pt_ptr[p], pt_ptr[p+1]) belongs to point p and
 * camera cam_idx[o]; uv_norm[0][o], uv_norm[1][o] = inv(K)[u,v,1]^T / z (ba_processor.py:339-342). */
int sfm_ba_solve(int V, int N, int64_t M, const int* pt_ptr /*[N+1]*/, const int* cam_idx /*[M]*/,
                 const double* uv_norm /*[2][M]*/, double* cams /*[V][7] in/out*/,
                 double* pts /*[3][N] in/out*/, double lambda, int iters, int quirks);

/* Device-resident problem: upload once, iterate many times (what bench.py times). */
typedef struct sfm_ba_problem sfm_ba_problem;
int sfm_ba_create(int V, int N, int64_t M, const int* pt_ptr, const int* cam_idx,
                  const double* uv_norm, sfm_ba_problem** out);
int sfm_ba_destroy(sfm_ba_problem* p);
int sfm_ba_set_option(sfm_ba_problem* p, int option, int value);
/* Run every copy and kernel of THIS problem on an existing HIP stream (e.g. a torch stream, so that an RCCL
 * all-reduce issued under it orders with the kernels).  Each problem has its own stream: several problems in
 * one process do not interfere.  NULL = the library's own stream.  Synchronises the previous stream. */
int sfm_ba_set_stream(sfm_ba_problem* p, void* hip_stream);
/* Facts about a resident problem (SFM_INFO_*). */
int sfm_ba_info(sfm_ba_problem* p, int what, int64_t* value);
int sfm_ba_set_state(sfm_ba_problem* p, const double* cams /*[V][7]*/, const double* pts /*[3][N]*/);
/* Replace only the cameras / only the points [first, first + count) of the resident state: the per-view BA call
 * of the reference (ba_processor.py:267) re-reads poses and points that did not change since the previous
 * call's write-back; the drop-in uploads what did. */
int sfm_ba_set_cameras(sfm_ba_problem* p, const double* cams /*[V][7]*/);
int sfm_ba_set_points(sfm_ba_problem* p, int first, int count, const double* pts /*[3][count]*/);
/* Enqueue `iters` damped Gauss-Newton iterations (ba_processor.py:297-406) on the library stream. */
int sfm_ba_iterate(sfm_ba_problem* p, double lambda, int iters, int quirks);
/* Per-iteration statistics without a state download (the `stats` of SURVEY.md section 8(b)): cost[i] = sum over this
 * problem's observations of |b - f|^2 in normalised image coordinates (the quantity ba_processor.py:376 minimises)
 * at the linearisation point of iteration i, for the iterations run since the state was last uploaded (set_state /
 * set_cameras / set_points / append start a new history; at most 256 iterations are kept).  sqrt(cost / M) is the RMS
 * residual; in a sharded run every rank reports its own observations.  Synchronises. */
int sfm_ba_get_stats(sfm_ba_problem* p, double* cost /*[max_iters]*/, int max_iters, int* n_iters);
/* Robust loss inside the linearisation.  With e_o = |b - f|^2 of observation o (normalised image coordinates) and
 * s_o = e_o / delta^2, the iterations minimise delta^2 sum_o rho(s_o) instead of sum_o e_o: every iteration is the same
 * damped Gauss-Newton step on the reweighted problem (IRLS: r, Jp, Jx of an observation are scaled by sqrt(w(s_o)) at the
 * linearisation point; no second-order correction), in sfm_ba_iterate, in the split sfm_ba_linearize_reduce /
 * sfm_ba_solve_update and with a communicator alike.  lambda, the quirks, the Schur products, the reduced solve and the
 * camera update only ever see weighted blocks.  While a loss is set sfm_ba_get_stats reports delta^2 sum rho(s).
 *   delta is in normalised units (pixels / focal scale), finite and > 0; it is ignored for SFM_LOSS_NONE.  A bad kind or
 *   delta returns SFM_E_SHAPE and leaves the problem as it was.
 *   The call completes a deferred back substitution with the OLD loss, drops captured graphs and restarts the cost
 *   history (as sfm_ba_set_points does); it uploads nothing.  The loss belongs to the handle: it survives sfm_ba_append,
 *   sfm_ba_cull and sfm_ba_sync_tracks like the options.  With SFM_LOSS_NONE (the default) the iterations launch the very
 *   kernels they launched before this call existed.
 * Plain least squares regardless of this setting: sfm_ba_solve, sfm_ba_refine_points, sfm_ba_screen / sfm_ba_cull's
 * errors, and the PnP and triangulation solvers.  sfm_ba_refine_cameras uses it when its use_loss argument says so. */
int sfm_ba_set_loss(sfm_ba_problem* p, int kind, double delta);
int sfm_ba_get_loss(sfm_ba_problem* p, int* kind, double* delta);
/* Parity hook: s_o, w(s_o), rho(s_o) of every observation at the current state, in the resident (point, camera) order, from
 * the device function the iteration kernels weight with.  With SFM_LOSS_NONE: s = e, w = 1, rho = e.  Completes a deferred
 * back substitution and expands the cameras if needed; changes nothing else.  Synchronises. */
int sfm_ba_loss_terms(sfm_ba_problem* p, double* s /*host [M] or NULL*/, double* w /*host [M] or NULL*/,
                      double* rho /*host [M] or NULL*/);
/* Synchronise, copy the state back, and report the first device-side failure (bad rotation ...). */
int sfm_ba_get_state(sfm_ba_problem* p, double* cams, double* pts);
/* sfm_ba_get_state plus R(q) of every camera (what ba_processor.py:412 computes from the refined quaternions with
 * convert_quaternion_to_rotation, validated: a failing camera is reported exactly as by sfm_ba_get_state). */
int sfm_ba_get_state_rot(sfm_ba_problem* p, double* cams /*[V][7]*/, double* pts /*[3][N]*/, double* rots /*[V][9]*/);
/* q <- convert_rotation_to_quaternion(R(q)) for the resident cameras [first, first + count): the round trip through the
 * rotation matrix that the reference performs between two BA calls (view.rot = R(q) at ba_processor.py:412-413, q = q(view.rot)
 * at ba:285-288) done on the device, for cameras the caller did not change since the last write-back: the per-view BA call then
 * uploads nothing for them.  Enqueues only. */
int sfm_ba_rederive_quaternions(sfm_ba_problem* p, int first, int count);
/* Grow a resident problem in place — the incremental pipeline registers a view, triangulates new points and
 * re-runs global BA (ba_processor.py:137-267).  n_new_cams cameras (indices V..)
 * and n_new_pts points (indices N..) are appended with their initial state; n_new_obs observations of ANY
 * (camera, point) pair not yet present are merged into the (point, camera)-sorted list.  The existing keys,
 * cameras and points never leave the device and ONLY the new cameras, points and observations are uploaded
 * (SFM_INFO_UPLOAD_BYTES grows by 56 n_new_cams + 24 n_new_pts + 24 n_new_obs): the merge itself runs on the
 * device (count / scan / bucket / merge kernels), every workspace is re-planned for the new size.  The handle,
 * its options, stream and current state survive; an externally bound reduced buffer survives when no camera
 * was added, otherwise the library's own buffer takes over and the caller binds a new one (its size follows
 * V).  On error the problem is unchanged.  Blocking. */
int sfm_ba_append(sfm_ba_problem* p, int n_new_cams, const double* cams /*[n_new_cams][7]*/, int n_new_pts,
                  const double* pts /*[3][n_new_pts]*/, int64_t n_new_obs, const int* obs_cam /*[n_new_obs]*/,
                  const int* obs_pt /*[n_new_obs]*/, const double* uv_norm /*[2][n_new_obs]*/);
/* Accumulated device time of one kernel class since the last reset (needs SFM_OPT_TIMING = 1);
 * synchronises.  *launches may be NULL. */
int sfm_ba_kernel_time(sfm_ba_problem* p, int kernel_id, double* total_ms, int* launches);
int sfm_ba_reset_timing(sfm_ba_problem* p);
/* Calibration of those brackets: the average hipEvent-to-hipEvent time around a kernel that does nothing, on the
 * problem's stream, between other launches (n samples).  A bracket reads the kernel's duration PLUS this (the events'
 * own stream bubbles); bench.py subtracts it, less the ~1.5 us an empty kernel itself takes.  Synchronises. */
int sfm_ba_event_overhead(sfm_ba_problem* p, int n, double* avg_ms);
/* Diagnostic: shader-clock stamps written by instrumented kernels when SFM_OPT_DEBUG has bit 8 set. */
int sfm_ba_debug_stamps(sfm_ba_problem* p, unsigned long long* out, int n);
/* Diagnostic (host only, needs no device): the task table of the data-flow reduced solve for nbk = ceil(7 V / 32) block columns,
 * in the order its workgroups take it: {type, row, column, sort key} per task, type 0 = a block of L, 1 = the last library-side
 * block of a row + its two hand-over blocks, 2 = the hand-over block (i, i-1), 3 = a block of the rhs row, 4 = a block of an
 * identity row.  Returns the number of tasks (0 outside 2 .. 52 block columns); fills at most `capacity` of them. */
int sfm_ba_flow_tasks(int nbk, int* out, int capacity);
/* Workgroups of that launch on a device of n_cus compute units for a table of n_tasks tasks (host only): the chain, and
 * min(n_tasks, n_cus - 32) task workgroups from 41 compute units on, min(n_tasks, n_cus - 1) below, never fewer than one.
 * 0 for n_cus < 2 or n_tasks < 1: there is no such launch, the solve runs one launch per block column. */
int sfm_ba_flow_grid(int n_cus, int n_tasks);
/* The same for n_cams cameras with the reduce deferred into the launch (sfm_ba_iterate on one GPU, dense product): type 5 = the
 * accumulators of camera `row`, part `column` of 4; type 6 = block (row, column) of S, rows 8 q .. 8 q + 7 with q = key & 3. */
int sfm_ba_flow_tasks_deferred(int n_cams, int* out, int capacity);

/* Multi-GPU split of one iteration (points sharded by rank, cameras replicated):
 *   sfm_ba_linearize_reduce : this rank's partial reduced system [S (P x P, P = 7V padded to
 *                             sfm_ba_reduced_ld) | rhs (P)] -> the reduced buffer (device)
 *   <caller all-reduces (SUM, double) the reduced buffer across ranks, e.g. RCCL via torch.distributed>
 *   sfm_ba_solve_update     : + lambda I, factor, solve, update cameras, back-substitute own points
 * sfm_ba_iterate == these two back to back on one rank. */
int sfm_ba_linearize_reduce(sfm_ba_problem* p, double lambda, int quirks);
int sfm_ba_solve_update(sfm_ba_problem* p, double lambda, int quirks);
/* sfm_ba_solve_update may leave the back substitution of the points (ba_processor.py:405-406) to the next
 * sfm_ba_linearize_reduce, whose launch then does both in one pass over the observations.  Every entry point that
 * reads or replaces the state completes it first; a loop that only times linearize_reduce / solve_update calls ends
 * with sfm_ba_flush so that its last iteration is complete as well.  Enqueues only. */
int sfm_ba_flush(sfm_ba_problem* p);
/* DEVICE pointers of the resident points (SoA, n_pts doubles each) and the stream the problem runs on: the current
 * state after everything enqueued so far (a deferred back substitution is enqueued first).  Valid until the next
 * sfm_ba_append / sfm_ba_destroy. */
int sfm_ba_points_ptr(sfm_ba_problem* p, void** d_px, void** d_py, void** d_pz, int* n_pts);
int sfm_ba_stream(sfm_ba_problem* p, void** hip_stream);

/* ---- triangulation and structure-only refinement over ragged multi-view tracks ------------------------------------
 * A point owns the observations [pt_ptr[i], pt_ptr[i+1]) of a CSR (cam_idx[M], uv[2][M] SoA, in the coordinates of
 * projs[n_views][3][4]) and is solved from exactly those views:
 *   SFM_TRACKS_LINEAR     TriangulationProcessor.linear_triangulate over the track (rows per observation: u, then v);
 *   SFM_TRACKS_NONLINEAR  `iters` steps X[0:3] -= inv(sum Jx^T Jx + lambda I) sum Jx^T (f - b) over the track
 *                         (TriangulationProcessor.nonlinear_triangulate = the point half of a bundle-adjustment
 *                         iteration with the cameras held), from X_init, or from the DLT result when both bits are set.
 * Row W of X is read, used in the projection and carried unchanged.  `group` lanes share a point (1, 4, 8, 16, 32, 64;
 * 0 = chosen from n_pts, M and the longest track): a point's result depends on its own track, its input and the group
 * width only -- not on the other points of the call, the grid or timing.  iters = 0 with SFM_TRACKS_NONLINEAR is a
 * pure evaluation (points come out as they went in).  An empty track is a no-op; a track of one observation is
 * refined (the damping makes it solvable) but not solved linearly.
 * cost[2][n_pts] (optional): sum |f - b|^2 over the track at the input point (row 0) and at the output point (row 1).
 * status[n_pts] (optional): a mask of the SFM_TRACK_* bits below.
 * The CSR is validated on the device (pt_ptr[0] == 0, non-decreasing, pt_ptr[n_pts] == M, cam_idx in range); a failure
 * returns SFM_E_SHAPE, sfm_last_error names the index, nothing is written.  The _dev form takes device pointers,
 * waits once for that verdict and then only enqueues on hip_stream. */
#define SFM_TRACKS_LINEAR    1   /* DLT from the track; needs >= 2 observations */
#define SFM_TRACKS_NONLINEAR 2   /* damped Gauss-Newton from X (or from the DLT result when both bits are set) */
#define SFM_TRACK_TOO_FEW    1   /* the linear pass was requested and the track has fewer than 2 observations: the point keeps its
                                    input for that pass ((0, 0, 0, 1) when there is no X_init) */
#define SFM_TRACK_NONFINITE  2   /* a non-finite value or a zero determinant turned up: the point is written back as it came in */
#define SFM_TRACK_BEHIND     4   /* at the output point s[2] <= 0 for at least one observation (informational) */
int sfm_tri_tracks(int n_pts, int n_views, int64_t M, const int* pt_ptr, const int* cam_idx,
                   const double* uv /*[2][M]*/, const double* projs /*[n_views][3][4]*/,
                   int mode, double lambda, int iters, int group,
                   const double* X_init /*[4][n_pts], may be NULL when mode has LINEAR*/,
                   double* X_out /*[4][n_pts]*/, double* cost /*[2][n_pts] or NULL*/, int* status /*[n_pts] or NULL*/);
int sfm_tri_tracks_dev(int n_pts, int n_views, int64_t M, const int* d_pt_ptr, const int* d_cam_idx,
                       const double* d_uv, const double* d_projs, int mode, double lambda, int iters, int group,
                       const double* d_X_init, double* d_X_out /* may equal d_X_init */, double* d_cost, int* d_status,
                       void* hip_stream);
/* The group width `group` = 0 stands for, from the three quantities it may depend on (host only; the rule is DESIGN.md section 16). */
int sfm_tri_tracks_auto_group(int n_pts, int64_t M, int max_track);
/* The same on the resident scene, in place: observations and points (W = 1) are the problem's, the projections are
 * [R(q)^T | -R(q)^T C] of the prepared cameras the linearisation reads, so cost row 0 summed over the points is the
 * bundle adjustment's cost at the same state.  Completes a deferred back substitution first; cameras and their prepared
 * form are untouched; the points are treated as by sfm_ba_set_points (the cost history restarts).  Runs on the problem's
 * stream and uploads nothing.  cost / status are HOST arrays ([2][N], [N]) or NULL.  An empty problem returns SFM_OK. */
int sfm_ba_refine_points(sfm_ba_problem* p, int mode, double lambda, int iters, int group,
                         double* cost /*host [2][N] or NULL*/, int* status /*host [N] or NULL*/);

/* ---- robust triangulation of ragged tracks: pair hypotheses, inlier refit -------------------------------------------
 * sfm_tri_tracks solves a point by least squares over every observation of its track; one mismatched key then moves the
 * point.  Here the consistent subset of the track is found first.  The CSR, uv and projs are sfm_tri_tracks'.  W = 1:
 * with s = P_c (X, 1), err2 = cam_scale[c]^2 ((s0/s2 - u)^2 + (s1/s2 - v)^2) is sfm_ba_screen's quantity, and an
 * observation is an INLIER of X iff s2 > 0, err2 is finite and err2 <= max_err2.  The rule, per track of n observations:
 *   1. Hypotheses.  The P = n (n - 1) / 2 pairs (i < j) are numbered in lexicographic order.  The track has
 *      H = min(P, max_hyp) hypotheses; hypothesis h is pair k = h when P <= max_hyp, else k = floor(h P / max_hyp) in
 *      64-bit integers.  No random number anywhere.  max_hyp = 0 means 128; its range is 1 .. 65 536.
 *   2. Its point.  The four rows a = u p3 - p1, a = v p3 - p2 of the two observations, solved inhomogeneously:
 *      N = sum a[0:3] a[0:3]^T, g = -sum a[3] a[0:3], X = N^-1 g (3x3 adjugate).  A zero or non-finite determinant or a
 *      non-finite X makes the hypothesis invalid.
 *   3. Angle gate.  With r = (C - X) / |C - X| of the two generating cameras (C: the camera centre -- of the resident
 *      cameras, or -M^-1 p4 of projs = [M | p4]) the hypothesis is invalid if r_i . r_j > cos_min_angle;
 *      cos_min_angle >= 1 switches the gate off.  A non-finite r_i . r_j (X on a centre) is invalid either way.
 *   4. Pair gate.  The hypothesis is invalid unless both generating observations are inliers of X.
 *   5. Score, lexicographic: the inlier count over the whole track (an integer); then the smaller r_i . r_j of the
 *      generating pair (the wider baseline); then the lower h.  None of the three depends on `group`, on the other points
 *      of the call or on timing: one lane forms X and the cosine from the pair alone and counts in an integer.
 *   6. Refit.  Step 2's solve over all inliers of the winner, then `iters` steps X -= inv(sum Jx^T Jx + lambda I)
 *      sum Jx^T (f - b) over those inliers (sfm_tri_tracks' step), the mask fixed.  The refit stands iff every solve
 *      succeeded, it is finite and its own inlier count over the whole track is at least the winner's; otherwise the
 *      hypothesis point and its mask stand and SFM_RANSAC_KEPT_HYPOTHESIS is set.  obs_inlier / n_inliers describe the
 *      point that stands.  A solved point comes out with W = 1.
 *   7. With SFM_RANSAC_TOO_FEW or SFM_RANSAC_NO_MODEL the point comes out bit for bit as it went in (X_init, the
 *      resident point, or (0, 0, 0, 1) without X_init), n_inliers = 0, best_hyp = -1, its obs_inlier entries are 0.
 *   8. summary[6], counted on the device with integer atomics: points solved, points NO_MODEL, points TOO_FEW, points
 *      KEPT_HYPOTHESIS, observations flagged inlier, observations of solved points flagged outlier.
 * `group` lanes share a point (1, 4, 8, 16, 32, 64; 0 = sfm_tri_tracks_auto_group): best_hyp and the winner's count do
 * not depend on it; the refit's sums do, so a point's bits depend on its track, its input, the options and the width.
 * A NaN or negative max_err2, cos_min_angle < -1 or NaN, max_hyp outside 0 .. 65 536, iters < 0, a negative or NaN
 * lambda or a bad group return SFM_E_SHAPE and launch nothing.  The CSR is validated as sfm_tri_tracks validates it (one
 * read-back before anything is written).  cam_scale[n_views], X_init and every output but X_out may be NULL.
 * The _dev form takes device pointers (d_summary: int64[6] on the device) and runs on hip_stream; d_X_out may equal
 * d_X_init; it returns when the work is done (its work buffers go back to the pool). */
#define SFM_RANSAC_TOO_FEW          1   /* the track has fewer than 2 observations */
#define SFM_RANSAC_NO_MODEL         2   /* no valid hypothesis */
#define SFM_RANSAC_KEPT_HYPOTHESIS  4   /* the refit did not stand: the point is the winning hypothesis itself */
#define SFM_RANSAC_SAMPLED          8   /* P > max_hyp: not every pair was a hypothesis (informational) */
int sfm_tri_tracks_ransac(int n_pts, int n_views, int64_t M, const int* pt_ptr, const int* cam_idx,
                          const double* uv /*[2][M]*/, const double* projs /*[n_views][3][4]*/,
                          const double* cam_scale /*[n_views] or NULL*/, double max_err2, double cos_min_angle, int max_hyp,
                          double lambda, int iters, int group, const double* X_init /*[4][n_pts] or NULL*/,
                          double* X_out /*[4][n_pts]*/, unsigned char* obs_inlier /*[M] or NULL*/,
                          int* n_inliers /*[n_pts] or NULL*/, int* best_hyp /*[n_pts] or NULL*/,
                          int* status /*[n_pts] or NULL*/, int64_t* summary /*[6] or NULL*/);
int sfm_tri_tracks_ransac_dev(int n_pts, int n_views, int64_t M, const int* d_pt_ptr, const int* d_cam_idx,
                              const double* d_uv, const double* d_projs, const double* d_cam_scale, double max_err2,
                              double cos_min_angle, int max_hyp, double lambda, int iters, int group,
                              const double* d_X_init, double* d_X_out /* may equal d_X_init */,
                              unsigned char* d_obs_inlier, int* d_n_inliers, int* d_best_hyp, int* d_status,
                              int64_t* d_summary, void* hip_stream);
/* The same on the resident scene, in place, following sfm_ba_refine_points: observations and points (W = 1) are the
 * problem's, projections and centres those of the prepared cameras.  Completes a deferred back substitution first; only
 * points move (the cost history restarts); cameras, their prepared form, graphs and the structure are untouched.  With a
 * communicator it is local to the rank's points, as the cull is.  sfm_ba_retriangulate(t) followed by sfm_ba_cull(t)
 * removes what it flagged.  cam_scale and the outputs are HOST arrays or NULL.  An empty problem returns SFM_OK. */
int sfm_ba_retriangulate(sfm_ba_problem* p, double max_err2, double cos_min_angle, int max_hyp, double lambda, int iters,
                         int group, const double* cam_scale /*host [V] or NULL*/, unsigned char* obs_inlier /*host [M]*/,
                         int* n_inliers /*host [N]*/, int* best_hyp /*host [N]*/, int* status /*host [N]*/,
                         int64_t* summary /*[6]*/);
/* Host only: the hypothesis count H of a track of n observations (0 for n < 2 or a max_hyp out of range) and, for
 * 0 <= h < H, the pair (*i < *j) of hypothesis h. */
int sfm_tri_ransac_pair(int n, int max_hyp, int h, int* i, int* j);

/* ---- motion-only refinement of the resident scene: every camera from its own observations, the points held ----------
 * The other half of sfm_ba_refine_points.  For every camera c with cam_mask[c] != 0 and at least one observation, `iters`
 * times: r_o = b - f and Jp_o (2x7 with respect to [C, q]) of the camera's observations exactly as one linearisation of the
 * bundle adjustment forms them (R(q), t and q^ = q(R(q)) of the prepared camera, the Q2 bit of `quirks` honoured, the Q1
 * bit ignored); with use_loss = 1 and a loss on the handle both are scaled by sqrt(w(s_o)) as the iterations scale them;
 *   U = sum Jp^T Jp,  g = sum Jp^T r,  dp = inv(U + lambda I) g,  cam += dp,  q /= |q|      (ba_processor.py:382-392 without
 * the point blocks), then R(q), its checks and q^ for the next pass.  iters = 0 is a pure evaluation: the cameras come out
 * bit for bit as they went in.
 *   cost[0][c] / cost[1][c]: the camera's share of the minimised cost (sum e_o, or delta^2 sum rho(s_o) with the loss) at
 *   the input / output camera; row 0 summed over the cameras is what sfm_ba_get_stats reports for an iteration linearised at
 *   that state.  A held, empty or NONFINITE camera reports its row 0 in both rows (0 for an empty one).
 *   status[c]: a mask of the SFM_CAM_* bits below.
 * Determinism: a camera's result bits depend on its own observations (in ascending point order), its own state, the points
 * it sees, lambda, iters, quirks and the loss -- not on the other cameras, the mask, the grid or timing.  The 35 sums are
 * formed per slice of consecutive observations and added in slice order; how a camera of n_obs observations is worked on is
 * a function of n_obs alone, reported by the _plan call: size class 0 = empty, 1 / 2 = one workgroup runs all iterations in
 * one launch with the observations in registers, 3 = the same with the observations read again in every pass, 4 = two
 * launches per pass.
 * Completes a deferred back substitution first and prepares the cameras if they are not; an INPUT camera that fails the
 * rotation checks returns its status, names the camera and leaves the state as it was.  Afterwards the cameras are treated
 * as by sfm_ba_set_cameras: the cost history restarts, captured graphs stay, the prepared form is rebuilt before the next
 * linearisation.  Points, observations, options and the loss are untouched.  Only cam_mask is uploaded.  Runs on the
 * problem's stream; blocking.  iters < 0, a NaN or negative lambda, use_loss outside {0, 1} or an attached communicator
 * (the points are sharded: the replicas would diverge) return SFM_E_SHAPE and launch nothing.  An empty problem or one
 * without observations returns SFM_OK.  cost / status are HOST arrays or NULL. */
#define SFM_CAM_EMPTY      1   /* the camera has no observation: untouched (informational) */
#define SFM_CAM_NONFINITE  2   /* a non-finite value turned up, or the updated camera failed the rotation checks of
                                  cam_prepare: the camera is written back as it came in */
#define SFM_CAM_BEHIND     4   /* at the output camera s[2] <= 0 for at least one of its observations (informational) */
#define SFM_CAM_HELD       8   /* cam_mask[c] == 0: untouched */
int sfm_ba_refine_cameras(sfm_ba_problem* p, double lambda, int iters, int quirks, int use_loss,
                          const unsigned char* cam_mask /*host [V] or NULL = every camera*/,
                          double* cost /*host [2][V] or NULL*/, int* status /*host [V] or NULL*/);
/* host only, needs no device: how a camera of n_obs observations is worked on (any output may be NULL) */
int sfm_ba_refine_cameras_plan(int64_t n_obs, int* n_slices, int* slice_obs, int* size_class);

/* ---- robust resection of cameras: three-point hypotheses, inlier refit ---------------------------------------------
 * sfm_ba_refine_cameras fits a camera by least squares over every observation it owns; a share of mismatched keys then
 * moves the pose.  Here the consistent subset of a camera's observations is found first: the camera-side counterpart of
 * the robust triangulation above.  A camera owns n observations: normalised keys u, v in the coordinates of the K-free
 * projection [R(q)^T | -R(q)^T C], each with its point X; scale = cam_scale[c], or 1.  With s = R(q)^T X - R(q)^T C,
 * err2 = scale^2 ((s0/s2 - u)^2 + (s1/s2 - v)^2) is sfm_ba_screen's quantity, and an observation is an INLIER of a pose
 * iff s2 > 0, err2 is finite and err2 <= max_err2.  The rule, per camera:
 *   1. n < 4: SFM_RESECT_TOO_FEW.
 *   2. Hypotheses.  The T = n (n - 1) (n - 2) / 6 triples (i < j < l) are numbered in lexicographic order.  The camera has
 *      H = min(T, max_hyp) hypotheses; hypothesis h is triple k = h when T <= max_hyp, else k = floor(h T / max_hyp) in
 *      64-bit integers.  No random number anywhere.  max_hyp = 0 means 128; its range is 1 .. 65 536.  A camera of more
 *      than 2^20 observations returns SFM_E_SHAPE naming the camera (T must fit 63 bits).
 *   3. Poses of a triple.  Bearings f = (u, v, 1) / |(u, v, 1)|; a2 = |X_j - X_l|^2, b2 = |X_i - X_l|^2,
 *      c2 = |X_i - X_j|^2; ca = f_j . f_l, cb = f_i . f_l, cg = f_i . f_j; depths s_j = x s_i, s_l = y s_i from Grunert's
 *      quartic A4 y^4 + A3 y^3 + A2 y^2 + A1 y + A0 = 0 with p = (a2 - c2) / b2, q = (a2 + c2) / b2,
 *        A4 = (p - 1)^2 - 4 (c2 / b2) ca^2
 *        A3 = 4 (p (1 - p) cb - (1 - q) ca cg + 2 (c2 / b2) ca^2 cb)
 *        A2 = 2 (p^2 - 1 + 2 p^2 cb^2 + 2 ((b2 - c2) / b2) ca^2 - 4 q ca cb cg + 2 ((b2 - a2) / b2) cg^2)
 *        A1 = 4 (-p (1 + p) cb + 2 (a2 / b2) cg^2 cb - (1 - q) ca cg)
 *        A0 = (1 + p)^2 - 4 (a2 / b2) cg^2
 *        x = ((p - 1) y^2 - 2 p cb y + 1 + p) / (2 (cg - y ca)),   s_i = sqrt(b2 / (1 + y^2 - 2 y cb)).
 *      Every real root with x, y, s_i > 0 gives a pose: R^T and t from the two right-handed frames spanned by
 *      (P_j - P_i, (P_j - P_i) x (P_l - P_i)), once of the camera-frame points s f and once of the world points.  A
 *      triple has at most four poses, numbered r = 0 .. 3 by ascending s_i.  Invalid: non-finite or zero a2, b2, c2, a
 *      zero frame normal (collinear points), a zero or non-finite A4, a zero divisor, a non-finite pose, or a rotation
 *      that sfm_rot_to_quat refuses (qw below 1e-6).  How the real roots are found is not part of the rule: a conjugate
 *      pair whose imaginary part is below 1e-7 (1 + |real part|) counts as a double root, and every root is polished by two
 *      Newton steps on the quartic; what one solver gets wrong is caught by step 4.
 *   4. Triple gate.  A pose is invalid unless its three generating observations are inliers of it.
 *   5. Score, lexicographic: the inlier count over all n observations (an integer); then the lower h; then the lower r.
 *      A winner needs a count of at least 4 (a model that explains only its own three points explains nothing), otherwise
 *      SFM_RESECT_NO_MODEL.  The count and the winner depend on nothing but the camera's own data.
 *   6. Refit.  The winner becomes cam7 = [C, q] = [-R t, sfm_rot_to_quat(R)]; then `iters` steps of sfm_ba_refine_cameras'
 *      update over the observations that are inliers of the winner's pose [R^T | t] (the mask fixed, no loss, the Q2 bit
 *      of `quirks` honoured).  The refit stands iff every solve and every expansion of the camera succeeded, it is finite
 *      and its own inlier count over all n is at least the winner's; otherwise the hypothesis camera stands and
 *      SFM_RESECT_KEPT_HYPOTHESIS is set.  obs_inlier / n_inliers describe the camera that stands, EXPANDED as every
 *      operation on a scene expands it and projected as sfm_ba_screen projects: on the resident scene sfm_ba_resect(t)
 *      followed by sfm_ba_screen(t) shows HIGH_ERROR | BEHIND | NONFINITE exactly where obs_inlier == 0, for every solved
 *      camera, by construction.
 *   7. With SFM_RESECT_TOO_FEW or SFM_RESECT_NO_MODEL the camera comes out bit for bit as it went in (cams_init, the
 *      resident camera, or (0, 0, 0, 1, 0, 0, 0) without cams_init), n_inliers = 0, best_hyp = -1, its obs_inlier entries are
 *      0.  A held camera (cam_mask[c] == 0, resident form) is untouched and SFM_RESECT_HELD, but it is still judged at its
 *      current expansion: obs_inlier and n_inliers are filled for it.
 *   8. summary[6], counted on the device with integer atomics: cameras solved, cameras NO_MODEL, cameras TOO_FEW, cameras
 *      KEPT_HYPOTHESIS, observations flagged inlier, observations of solved cameras flagged outlier.
 * Determinism: no floating-point atomic; best_hyp and the counts are integers and do not depend on the grid or on
 * timing; the refit's 36 sums are formed per slice of 64 consecutive observations and added in slice order, so a camera's
 * bits depend on its own observations, their points and the options only.  A camera of any size takes the same path.
 * Free form: view_ptr[n_views + 1] (HOST in both forms: the launches are planned from it) delimits the observations of a
 * view in uv = [2][M] and X = [3][M] (the point of every observation).  A NaN or negative max_err2, max_hyp outside
 * 0 .. 65 536, iters < 0, a negative or NaN lambda, or a view_ptr that does not start at 0, decreases or does not end at M
 * return SFM_E_SHAPE and launch nothing.  cam_scale, cams_init and every output but cams_out may be NULL.  The _dev form
 * takes device pointers (d_summary: int64[6] on the device) and runs on hip_stream; d_cams_out may equal d_cams_init; it
 * returns when the work is done (its work buffers go back to the pool). */
#define SFM_RESECT_TOO_FEW          1   /* the camera has fewer than 4 observations */
#define SFM_RESECT_NO_MODEL         2   /* no valid pose with at least 4 inliers */
#define SFM_RESECT_KEPT_HYPOTHESIS  4   /* the refit did not stand: the camera is the winning hypothesis itself */
#define SFM_RESECT_SAMPLED          8   /* T > max_hyp: not every triple was a hypothesis (informational) */
#define SFM_RESECT_HELD            16   /* cam_mask[c] == 0: untouched, judged only */
int sfm_resect_ransac(int n_views, const int* view_ptr /*host [n_views+1]*/, int64_t M, const double* uv /*[2][M]*/,
                      const double* X /*[3][M]*/, const double* cam_scale /*[n_views] or NULL*/, double max_err2,
                      int max_hyp, double lambda, int iters, int quirks, const double* cams_init /*[n_views][7] or NULL*/,
                      double* cams_out /*[n_views][7]*/, unsigned char* obs_inlier /*[M] or NULL*/,
                      int* n_inliers /*[n_views] or NULL*/, int* best_hyp /*[n_views] or NULL*/,
                      int* status /*[n_views] or NULL*/, int64_t* summary /*[6] or NULL*/);
int sfm_resect_ransac_dev(int n_views, const int* view_ptr /*host [n_views+1]*/, int64_t M, const double* d_uv,
                          const double* d_X, const double* d_cam_scale, double max_err2, int max_hyp, double lambda,
                          int iters, int quirks, const double* d_cams_init, double* d_cams_out /* may equal d_cams_init */,
                          unsigned char* d_obs_inlier, int* d_n_inliers, int* d_best_hyp, int* d_status,
                          int64_t* d_summary, void* hip_stream);
/* The same on the resident scene, in place, following sfm_ba_refine_cameras: a camera's observations are those of the
 * scene's camera-major list (ascending point), its points the resident ones.  Completes a deferred back substitution
 * first; only cameras move and they are treated as by sfm_ba_set_cameras (the cost history restarts, the prepared form is
 * rebuilt); points, observations, options, the loss and captured graphs are untouched.  sfm_ba_resect(t) followed by
 * sfm_ba_cull(t) removes the flagged observations of the solved cameras.  With a communicator attached it is refused
 * (SFM_E_SHAPE).  cam_mask, cam_scale and the outputs are HOST arrays or NULL; obs_inlier is in the scene's observation
 * order.  A problem without observations returns SFM_OK with every free camera TOO_FEW. */
int sfm_ba_resect(sfm_ba_problem* p, double max_err2, int max_hyp, double lambda, int iters, int quirks,
                  const unsigned char* cam_mask /*host [V] or NULL = every camera*/, const double* cam_scale /*host [V] or NULL*/,
                  unsigned char* obs_inlier /*host [M]*/, int* n_inliers /*host [V]*/, int* best_hyp /*host [V]*/,
                  int* status /*host [V]*/, int64_t* summary /*[6]*/);
/* Host only, needs no device: the hypothesis count H of a camera of n observations (0 for n < 3, n > 2^20 or a max_hyp
 * out of range) and, for 0 <= h < H, the triple (*i < *j < *l) of hypothesis h. */
int sfm_resect_triple(int n, int max_hyp, int h, int* i, int* j, int* l);

/* ---- robust two-view geometry: sampled eight-point hypotheses, inlier refit ----------------------------------------
 * sfm_fundamental_ransac scores host-drawn samples by |x_r^T F x_l| on normalised coordinates (a residual without a unit),
 * returns the best eight-point matrix as it is and handles one pair of views.  Here the consistent subset of the matches
 * between two views is found, for a batch of sets in one call: the third robust estimator, next to the point
 * (sfm_tri_tracks_ransac) and the camera (sfm_resect_ransac).  A call holds n_sets sets of matches; left and right are
 * [2][M] pixel coordinates (the x row, then the y row); set s owns the matches set_ptr[s] .. set_ptr[s + 1] - 1, n of them.
 * The rule, per set:
 *   1. n < 9: SFM_TWOVIEW_TOO_FEW.
 *   2. The test.  For a matrix F (row-major 3x3, pixel coordinates): a = F (x_l, y_l, 1)^T, b = F^T (x_r, y_r, 1)^T,
 *      e = (x_r, y_r, 1) . a; the squared Sampson distance d2 = e^2 / (a0^2 + a1^2 + b0^2 + b1^2) is in pixels squared.  A
 *      match is an INLIER of F iff d2 is finite and d2 <= max_err2.  One function (twoview_inlier, csrc/sfm_obs_test.h)
 *      that every stage below calls.
 *   3. Normalisation.  T = [s 0 -s mx; 0 s -s my; 0 0 1] per image over all n matches of the set: (mx, my) the centroid,
 *      s = sqrt(2) / (mean distance from the centroid) (Hartley; the layout of epipolar_processor.py:97-137, whose scale
 *      sqrt(2 n) / (sum of distances) differs from this by sqrt(n)).  If T_l or T_r is not finite (a NaN coordinate,
 *      identical points) the set is SFM_TWOVIEW_NO_MODEL.
 *   4. Hypotheses.  H = max_hyp (0 means 128; range 1 .. 65 536), whatever n.  Hypothesis h uses, for k = 0 .. 7, the match
 *      lo_k + mix(8 h + k) mod (hi_k - lo_k) with lo_k = floor(k n / 8), hi_k = floor((k + 1) n / 8): one match of every
 *      eighth of the set, so the eight indices are distinct and ascending.  mix is the splitmix64 finaliser in unsigned
 *      64-bit arithmetic: z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *      z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31.  No random-number state and no floating point:
 *      sfm_twoview_sample returns the same indices on any machine.
 *   5. Matrix of a sample.  The eight-point solve of sfm_fundamental_eight_point on the normalised matches: the null
 *      vector of the 8x9 design matrix (rows x1 x2, y1 x2, x2, x1 y2, y1 y2, y2, x1, y1, 1 with 1 = left, 2 = right), as
 *      a 3x3 matrix projected to rank 2 (its two largest singular values kept; invalid unless sigma_1 > 3 eps sigma_0),
 *      WITHOUT the division by f[2][2]; then F = T_r^T f T_l, scaled to Frobenius norm 1 with its entry of largest
 *      magnitude positive (the lowest index on a tie).  Invalid if rank-deficient or not finite.  How the null vector is
 *      found is not part of the rule.
 *   6. Sample gate.  A hypothesis is invalid unless its own eight matches are inliers of it.
 *   7. Score, lexicographic: the inlier count over all n matches (an integer); then the lower h.  A winner needs a count
 *      of at least 9, otherwise SFM_TWOVIEW_NO_MODEL.
 *   8. Refit, up to `iters` rounds.  The inlier mask of the standing matrix; the transforms of step 3 over those inliers
 *      only; the 9x9 moment matrix A^T A of the inliers' design rows; its eigenvector of smallest eigenvalue, then rank-2
 *      projection, de-normalisation and scaling as in step 5.  The round stands iff the result is valid and its inlier
 *      count over all n is at least the standing count (it then becomes the standing matrix and count); otherwise the
 *      rounds stop.  SFM_TWOVIEW_KEPT_HYPOTHESIS iff iters > 0 and no round stood.
 *   9. Outputs, all optional but F_out.  F_out[n_sets][9]: the standing matrix, scaled as in step 5; nine zeros with
 *      TOO_FEW or NO_MODEL.  obs_inlier[M], n_inliers, best_hyp (-1 without a model), status and summary[6] (sets solved,
 *      sets NO_MODEL, sets TOO_FEW, sets KEPT_HYPOTHESIS, matches flagged inlier, matches of solved sets flagged outlier)
 *      describe the standing matrix, judged once more by the function of step 2.
 * Determinism: no floating-point atomic; the counts are integers; every floating-point sum over matches (the sums of the
 * normalisation and the 45 moment sums) is formed per slice of 64 consecutive matches of the set and the slices are added
 * in ascending order.  A set's bits depend on its own matches and the options only, never on the batch.
 * set_ptr[n_sets + 1] is a HOST array in both forms (the launches are planned from it).  A NaN or negative max_err2,
 * max_hyp outside 0 .. 65 536, iters < 0, or a set_ptr that does not start at 0, decreases or does not end at M return
 * SFM_E_SHAPE and launch nothing.  The _dev form takes device pointers (d_summary: int64[6] on the device), runs on
 * hip_stream and returns when the work is done (its work buffers go back to the pool). */
#define SFM_TWOVIEW_TOO_FEW          1   /* the set has fewer than 9 matches */
#define SFM_TWOVIEW_NO_MODEL         2   /* no valid hypothesis with at least 9 inliers, or no finite normalisation */
#define SFM_TWOVIEW_KEPT_HYPOTHESIS  4   /* no refit round stood: the matrix is the winning hypothesis itself */
int sfm_twoview_ransac(int n_sets, const int* set_ptr /*host [n_sets+1]*/, int64_t M, const double* left /*[2][M]*/,
                       const double* right /*[2][M]*/, double max_err2, int max_hyp, int iters,
                       double* F_out /*[n_sets][9]*/, unsigned char* obs_inlier /*[M] or NULL*/,
                       int* n_inliers /*[n_sets] or NULL*/, int* best_hyp /*[n_sets] or NULL*/,
                       int* status /*[n_sets] or NULL*/, int64_t* summary /*[6] or NULL*/);
int sfm_twoview_ransac_dev(int n_sets, const int* set_ptr /*host [n_sets+1]*/, int64_t M, const double* d_left,
                           const double* d_right, double max_err2, int max_hyp, int iters, double* d_F_out,
                           unsigned char* d_obs_inlier, int* d_n_inliers, int* d_best_hyp, int* d_status,
                           int64_t* d_summary, void* hip_stream);
/* Host only, needs no device: the hypothesis count H of a set of n matches (0 for n < 9 or a max_hyp out of range) and,
 * for 0 <= h < H, the eight ascending match indices of hypothesis h. */
int sfm_twoview_sample(int n, int max_hyp, int h, int idx[8]);

/* ---- robust homography: sampled four-point hypotheses, inlier refit ------------------------------------------------
 * A fundamental matrix is not determined when the matches lie on one plane or the camera only rotated: the eight-point
 * solve then returns some rank-2 matrix that explains every match.  The model of those cases is the homography, the
 * fourth robust estimator; with both models per pair a caller can tell the cases apart (processors.classify_matches).
 * A call holds n_sets sets of matches; left and right are [2][M] pixel coordinates (the x row, then the y row); set s owns
 * the matches set_ptr[s] .. set_ptr[s + 1] - 1, n of them.  The rule, per set, step for step that of the block above:
 *   1. n < 5: SFM_HOMOGRAPHY_TOO_FEW.
 *   2. The test.  A model is a pair of row-major 3x3 matrices (H, G) in pixel coordinates, H mapping left to right and G
 *      right to left.  half(A, p, q): (u, v, w) = A (p_x, p_y, 1)^T, each row as fma(A0, x, fma(A1, y, A2));
 *      eu = fma(-q_x, w, u), ev = fma(-q_y, w, v); lhs = fma(eu, eu, ev * ev), rhs = max_err2 * (w * w); true iff lhs is
 *      finite, w * w > 0 and lhs <= rhs.  A match is an INLIER iff half(H, l, r) and half(G, r, l): the transfer error in
 *      each image is at most max_err2 pixels squared, without a division.  One function (homography_inlier,
 *      csrc/sfm_obs_test.h) that every stage below calls.
 *   3. Normalisation.  Step 3 of the two-view rule: the Hartley transforms T_l, T_r over all n matches; if one of them is
 *      not finite the set is SFM_HOMOGRAPHY_NO_MODEL.
 *   4. Hypotheses.  H = max_hyp (0 means 128; range 1 .. 65 536), whatever n.  Hypothesis h uses, for k = 0 .. 3, the match
 *      lo_k + mix(4 h + k) mod (hi_k - lo_k) with lo_k = floor(k n / 4), hi_k = floor((k + 1) n / 4): one match of every
 *      quarter of the set, so the four indices are distinct and ascending.  mix is the splitmix64 finaliser of the two-view
 *      rule.  sfm_homography_sample returns the same indices on any machine.
 *   5. Matrix of a sample.  Every normalised match (x1, y1) -> (x2, y2) gives the design rows
 *      (-x1, -y1, -1, 0, 0, 0, x2 x1, x2 y1, x2) and (0, 0, 0, -x1, -y1, -1, y2 x1, y2 y1, y2); the null vector of the 8x9
 *      matrix, read as a 3x3 matrix h, is invalid unless sigma_2 > 3 eps sigma_0 (full rank).  H = T_r^-1 h T_l and
 *      G = T_l^-1 adj(h) T_r, adj the adjugate (nothing is divided by a determinant); each is scaled to Frobenius norm 1
 *      with its entry of largest magnitude positive (the lowest index on a tie).  Invalid if not finite.  How the null
 *      vector and the adjugate are computed is not part of the rule.
 *   6. Sample gate.  A hypothesis is invalid unless its own four matches are inliers of it.
 *   7. Score, lexicographic: the inlier count over all n matches (an integer); then the lower h.  A winner needs a count
 *      of at least 5, otherwise SFM_HOMOGRAPHY_NO_MODEL.
 *   8. Refit, up to `iters` rounds.  The inlier mask of the standing model; the transforms of step 3 over those inliers
 *      only; the 9x9 moment matrix A^T A of the inliers' design rows (two per inlier); its eigenvector of smallest
 *      eigenvalue, then as in step 5.  The round stands iff the result is valid and its inlier count over all n is at least
 *      the standing count; otherwise the rounds stop.  SFM_HOMOGRAPHY_KEPT_HYPOTHESIS iff iters > 0 and no round stood.
 *   9. Outputs, all optional but H_out.  H_out[n_sets][9]: the standing H, scaled as in step 5; nine zeros with TOO_FEW or
 *      NO_MODEL.  obs_inlier[M], n_inliers, best_hyp (-1 without a model), status and summary[6] have the meaning and
 *      order they have for sfm_twoview_ransac and describe the standing model, judged once more by the function of step 2.
 * Determinism, argument errors (SFM_E_SHAPE, nothing launched) and the conventions of the _dev form (set_ptr on the host,
 * d_summary int64[6] on the device, work buffers returned to the pool, the call returns when the work is done) are those
 * of sfm_twoview_ransac. */
#define SFM_HOMOGRAPHY_TOO_FEW          1   /* the set has fewer than 5 matches */
#define SFM_HOMOGRAPHY_NO_MODEL         2   /* no valid hypothesis with at least 5 inliers, or no finite normalisation */
#define SFM_HOMOGRAPHY_KEPT_HYPOTHESIS  4   /* no refit round stood: the model is the winning hypothesis itself */
int sfm_homography_ransac(int n_sets, const int* set_ptr /*host [n_sets+1]*/, int64_t M, const double* left /*[2][M]*/,
                          const double* right /*[2][M]*/, double max_err2, int max_hyp, int iters,
                          double* H_out /*[n_sets][9]*/, unsigned char* obs_inlier /*[M] or NULL*/,
                          int* n_inliers /*[n_sets] or NULL*/, int* best_hyp /*[n_sets] or NULL*/,
                          int* status /*[n_sets] or NULL*/, int64_t* summary /*[6] or NULL*/);
int sfm_homography_ransac_dev(int n_sets, const int* set_ptr /*host [n_sets+1]*/, int64_t M, const double* d_left,
                              const double* d_right, double max_err2, int max_hyp, int iters, double* d_H_out,
                              unsigned char* d_obs_inlier, int* d_n_inliers, int* d_best_hyp, int* d_status,
                              int64_t* d_summary, void* hip_stream);
/* Host only, needs no device: the hypothesis count H of a set of n matches (0 for n < 5 or a max_hyp out of range) and,
 * for 0 <= h < H, the four ascending match indices of hypothesis h. */
int sfm_homography_sample(int n, int max_hyp, int h, int idx[4]);

/* ---- covariance of the resident scene: per-camera and per-point blocks ---------------------------------------------
 * How well the current state is determined.  With H = J^T J + lambda I = [A B; B^T D] of one linearisation at the current
 * state (r, Jp, Jx exactly as the iterations form them, the Q2 bit of `quirks` honoured; with use_loss = 1 and a loss on
 * the handle scaled by sqrt(w(s_o)) as the iterations scale them), A = U + lambda I, D = V + lambda I, Y_o = W_o D_p^-1:
 *   cam_cov[c]  = the 7x7 diagonal block of inv(S_ff), S = A - B D^-1 B^T, row-major, in the [C, q] parametrisation
 *   pt_cov[p]   = D_p^-1 + sum over o, o' in track(p) of Y_o^T Sigma_{c(o) c(o')} Y_o'     as (xx, xy, xz, yy, yz, zz)
 *   *sigma0_sq  = cost / (2 M - 7 V_free - 3 N_observed), cost the linearisation's sum (the robust cost with the loss);
 *                 0 when the denominator is not positive
 * The covariances are NOT scaled by sigma0^2.  The gauge is fixed by holding cameras: cam_mask[c] == 0 holds camera c (the
 * convention of sfm_ba_refine_cameras), which removes its rows and columns from S -- S_ff is the Schur complement of the
 * problem in which those cameras are constants.  A held camera's block is zero and it adds nothing to a point's sum; a
 * point seen only by held cameras gets D_p^-1; a mask that holds every camera is valid.  With nothing held the seven
 * gauge directions of S have the eigenvalue lambda exactly, so the result says nothing about the data.
 *   cam_status[c]: SFM_COV_CAM_HELD; SFM_COV_CAM_PIVOT on the camera at which the factorisation of S_ff met a pivot that
 *   is not positive (not above 1e-9 x the row's diagonal entry of S: rounding noise; a positive definite system whose
 *   pivots fall below that, nothing held with a lambda nine orders below the diagonal of S for instance, is refused too).  Then the call returns SFM_E_SINGULAR,
 *   cam_cov / pt_cov / pt_status / sigma0_sq are untouched and nothing non-finite is produced.  That is what holding fewer than two
 *   cameras with lambda = 0 gives (the scale, or the whole gauge, is free).
 *   pt_status[p]: SFM_COV_PT_EMPTY (no observation: zeros), SFM_COV_PT_SINGULAR (D_p is not positive definite, one
 *   observation with lambda = 0 for instance: zeros, and the point's observations are left out of S altogether, U
 *   included.  For one observation that is the limit lambda -> 0: Jx (Jx^T Jx + lambda I)^-1 Jx^T -> I_2, the observation
 *   says nothing about its camera; for a longer track whose D_p is singular it errs on the large side).  Such a point
 *   still counts in sigma0_sq, whose formula is the one above on the whole scene.
 * `group` lanes share a point in the point kernel (1, 4, 8, 16, 32, 64; 0 = automatic); tracks longer than 64 take one
 * workgroup per point.  Determinism: no floating-point atomic anywhere; two calls return the same bits, and pt_cov[p] does
 * not depend on `group`.  The inverse is a dense FP64 Cholesky in 64 x 64 blocks (sfm_ba_covariance_plan), for every V.
 * Completes a deferred back substitution first and prepares the cameras if they are not; an INPUT camera that fails the
 * rotation checks returns its status and names the camera.  Works in buffers of its own: state, loss, options, cost
 * history, captured graphs and every buffer of the iterations are untouched, so `iterate; covariance; iterate` ends in the
 * bits of `iterate; iterate`.  Only cam_mask is uploaded.  Runs on the problem's stream; blocking.  A NaN or negative
 * lambda, use_loss outside {0, 1}, a bad group or an attached communicator (the points are sharded: Sigma_ff would need
 * the all-reduced S) return SFM_E_SHAPE and launch nothing.  All output arrays are HOST arrays or NULL. */
#define SFM_E_SINGULAR     -10  /* sfm_ba_covariance: the free cameras' system is not positive definite; sfm_ba_iterate_pcg: a diagonal block is not */
#define SFM_COV_CAM_HELD     8  /* cam_mask[c] == 0: the block is zero (= SFM_CAM_HELD) */
#define SFM_COV_CAM_PIVOT   16  /* the first camera with a pivot that is not positive */
#define SFM_COV_PT_EMPTY     4  /* the point has no observation (= SFM_PT_EMPTY) */
#define SFM_COV_PT_SINGULAR  8  /* D_p is not positive definite */
int sfm_ba_covariance(sfm_ba_problem* p, double lambda, int quirks, int use_loss,
                      const unsigned char* cam_mask /*host [V] or NULL = every camera free*/, int group,
                      double* cam_cov /*host [V][49] or NULL*/, double* pt_cov /*host [N][6] or NULL*/,
                      int* cam_status /*host [V] or NULL*/, int* pt_status /*host [N] or NULL*/, double* sigma0_sq /*or NULL*/);
/* host only, needs no device: block size of the dense inverse, its block count and kernel launches for n_cams cameras, and
 * the longest track a lane group takes (any output may be NULL) */
int sfm_ba_covariance_plan(int n_cams, int* block, int* n_blocks, int* n_launches, int* group_max_track);
/* Device time (ms, hipEvents) of the four phases of the last sfm_ba_covariance on this handle -- per-point terms, S, the
 * inverse (with its one status read-back), the point kernels -- if any SFM_OPT_TIMING bit was set during that call; zeros
 * otherwise and for a phase that did not run.  Measurement only: the events cost stream bubbles. */
int sfm_ba_covariance_times(sfm_ba_problem* p, double* ms /*[4]*/);

/* ---- matrix-free bundle adjustment of the resident scene: PCG on the reduced camera system, cameras can be held -----
 * `iters` outer iterations, each one iteration of sfm_ba_iterate with the solve replaced: S dp = rhs is solved by
 * conjugate gradients preconditioned with the diagonal 7x7 blocks of S (block Jacobi), and S is never formed -- q = S p is
 * two passes over the observations (by point, then by camera through the camera-major list).  r, Jp, Jx of every
 * observation are those of the iterations (the handle's loss applies, the Q2 bit of `quirks` is honoured).
 *   cam_mask[c] == 0 holds camera c (the convention of sfm_ba_refine_cameras): it has no unknowns, its seven doubles are
 *   never written; NULL = every camera free.  A mask that holds every camera is valid (the points still move).
 *   CG starts from x = 0 and stops when r^T M^-1 r <= cg_tol^2 r0^T M^-1 r0, or after cg_max_iters iterations
 *   (0: min(7 V_free, 1000)); the step found so far is then applied (SFM_PCG_MAX_ITERS).  p^T S p <= 0 or a non-finite
 *   scalar is SFM_PCG_BREAKDOWN: nothing of that outer iteration is applied and the loop stops.
 *   A point whose D_p is not positive definite or not finite is held for that iteration (SFM_INFO_PCG_HELD_POINTS); a point
 *   with no observation is untouched.  A free camera whose diagonal block does not factor (a pivot not above 1e-9 of its
 *   diagonal entry, as in sfm_ba_covariance; an empty free camera at lambda = 0 is the case) ends the call with
 *   SFM_E_SINGULAR: *bad_camera names it (the lowest such camera), and state and outputs are as they were before the call.
 *   Per outer iteration i < *iters_done: cost[i] the minimised cost at its linearisation, cg_iters[i], cg_rel[i] =
 *   sqrt(r^T M^-1 r / r0^T M^-1 r0) at exit, cg_status[i].  All outputs are HOST arrays or NULL.
 * `group` lanes share a point in the point kernels (1, 4, 8, 16, 32, 64; 0 = automatic, from the mean track length); lanes
 * stride over longer tracks.  Determinism: no floating-point atomic; the bits depend on the scene, the arguments and
 * `group` only.  The updated cameras are normalised and checked as the iterations check them (same error codes).
 * Completes a deferred back substitution first and prepares the cameras if they are not.  Works in buffers of its own:
 * nothing an iteration owns is touched.  Afterwards the state is treated as by sfm_ba_set_state without the upload: the
 * cost history restarts, the prepared cameras are rebuilt before the next linearisation.  Only the mask is uploaded.  Runs
 * on the problem's stream; blocking.  iters < 0, cg_tol outside (0, 1), cg_max_iters < 0, a bad group, a negative or
 * non-finite lambda or an attached communicator return SFM_E_SHAPE and launch nothing; iters = 0 does nothing. */
#define SFM_PCG_CONVERGED  0
#define SFM_PCG_MAX_ITERS  1   /* cg_max_iters reached; the step found so far was applied */
#define SFM_PCG_BREAKDOWN  2   /* p^T S p <= 0 or a non-finite scalar: nothing of this outer iteration was applied, the loop stopped */
int sfm_ba_iterate_pcg(sfm_ba_problem* p, double lambda, int iters, int quirks,
                       const unsigned char* cam_mask /*host [V] or NULL*/, double cg_tol, int cg_max_iters, int group,
                       int* iters_done, double* cost /*host [iters] or NULL*/, int* cg_iters /*host [iters] or NULL*/,
                       double* cg_rel /*host [iters] or NULL*/, int* cg_status /*host [iters] or NULL*/, int* bad_camera /*or NULL*/);
/* Milliseconds of the last sfm_ba_iterate_pcg on this handle, summed over its outer iterations: linearisation, camera
 * blocks, CG loop (with its flag reads), back substitution and camera update -- device time by hipEvents, zeros unless an
 * SFM_OPT_TIMING bit was set during the call -- and [4] the whole call by the host's clock (always). */
int sfm_ba_pcg_times(sfm_ba_problem* p, double* ms /*[5]*/);

/* ---- the cost of the resident scene ----------------------------------------------------------------------------------
 * *cost = delta^2 sum rho(|b - f|^2 / delta^2) with the handle's loss, the plain sum |b - f|^2 without one, at the current
 * state, from the prepared cameras the linearisation reads.  Residuals only: no Jacobian is formed or written.
 * `group` lanes share a point (1, 4, 8, 16, 32, 64; 0 = the width sfm_ba_iterate_pcg picks); lane l adds observations
 * l, l + group, ... of the track in ascending order, the group is a fixed tree, the points are added in a fixed order: no
 * floating-point atomic, the bits depend on the scene, the state and `group` only.  The value agrees with the cost
 * sfm_ba_iterate_pcg reports for the same state to rounding (1e-13 relative), not bit for bit.
 * Completes a deferred back substitution first and prepares the cameras if they are not; changes nothing else on the
 * handle (state, cost history, captured graphs): `iterate; cost; iterate` ends in the bits of `iterate; iterate`.  Uploads
 * nothing.  Runs on the problem's stream; blocking.  A bad group, a null cost or an attached communicator (the points are
 * sharded: the value would be one rank's share) return SFM_E_SHAPE and launch nothing; a scene without observations costs 0.  `quirks` is accepted for symmetry: no bit of it changes a residual. */
int sfm_ba_cost(sfm_ba_problem* p, int quirks, int group, double* cost);

/* ---- Levenberg-Marquardt control of the matrix-free bundle adjustment -------------------------------------------------
 * sfm_ba_iterate_pcg with a damping that adapts, steps that are judged before they stand, and stopping rules: the rule
 * of Madsen, Nielsen and Tingleff ("Methods for non-linear least squares problems", 2004, algorithm 3.16) with this
 * project's lambda I damping.  F is always sfm_ba_cost of a state.
 *   F = cost(state), lambda = lambda0, nu = 2; then at most max_trials trials, each:
 *   1. one outer iteration of sfm_ba_iterate_pcg at lambda, from the linearisation through the CG loop (same kernels, same
 *      order, the mask, the handle's loss, the Q2 bit of quirks, cg_tol, cg_max_iters);
 *   2. grad_inf = max(|rhs|_inf over the free cameras, |ex|_inf over the points) of that linearisation: the gradient with
 *      the points eliminated, zero exactly where the full gradient is; if gtol > 0 and grad_inf <= gtol: SFM_LM_STOP_GTOL,
 *      nothing is solved;
 *   3. cameras, prepared cameras and points are copied aside, and the step is applied as sfm_ba_iterate_pcg applies it
 *      (back substitution, cams += x, q /= |q|, the prepared camera and its checks);
 *   4. F_trial = cost(trial state);
 *      predicted = |r|^2 - |r - J h|^2 of the linearisation (r, J scaled by sqrt(w) with a loss), h = (x on the cameras,
 *      dx_p on the points) the step as applied before the normalisation, evaluated without a pass over the observations as
 *        sum_p ex_p^T D_p^-1 ex_p + x.rhs + x.r_cg + lambda (|x|^2 + sum_p |dx_p|^2),   r_cg = rhs - S x of the CG loop;
 *      step_norm = sqrt(|x|^2 + sum_p |dx_p|^2);  rho = (F - F_trial) / predicted;
 *   5. accepted iff predicted > 0, F_trial is finite and rho > SFM_LM_MIN_GAIN.
 *      accepted: the trial state stands; lambda = max(lambda_min, lambda max(1/3, 1 - (2 rho - 1)^3)), nu = 2;
 *        SFM_LM_STOP_FTOL if ftol > 0 and F - F_trial <= ftol F; else SFM_LM_STOP_XTOL if xtol > 0 and
 *        step_norm <= xtol (|state| + xtol), |state| the 2-norm of all 7 V + 3 N doubles of the state the trial started
 *        from; then F = F_trial.
 *      rejected: cameras, prepared cameras and points are copied back (device to device); lambda *= nu, nu *= 2;
 *        SFM_LM_STOP_LAMBDA_MAX if lambda > lambda_max.  The next trial linearises anew at the restored state.
 *   When the trials run out: SFM_LM_STOP_MAX_TRIALS.  A CG breakdown ends the call with SFM_LM_STOP_BREAKDOWN, a free
 *   camera whose diagonal block does not factor with SFM_LM_STOP_SINGULAR and *bad_camera: nothing of that trial is
 *   applied, and the call returns SFM_OK.  A trial camera that fails the checks of the iterations ends the call with their
 *   error code, after the restore.  In every case the state on return is the last accepted one (the entry state if there
 *   is none), *cost_out its cost, *lambda_out the damping the next trial would have used.
 * The decision and the sums of steps 2 and 4 are made on the device (lm_sums, lm_decide: a lane's own terms in ascending
 * order, a fixed tree per wave, the wave totals in order; no floating-point atomic); the host reads one sfm_lm_trial row
 * and the next lambda per trial and does what it says.  log[i], i < *trials_done, is the row of trial i; a trial that
 * ended in BREAKDOWN or SINGULAR has no row, one that ended in GTOL has a row with lambda, cost = cost_trial = F and
 * grad_inf, the rest zero.  A scene without observations has cost 0 and runs no trial.  Determinism: the bits depend on
 * the scene, the state, the options and `group` only.
 * Works in buffers of its own and the PCG work buffers; nothing sfm_ba_iterate owns is touched.  Afterwards the handle is
 * as after sfm_ba_iterate_pcg (the cost history restarts, the prepared cameras are rebuilt).  Only the mask is uploaded.
 * Runs on the problem's stream; blocking.  Returns SFM_E_SHAPE and launches nothing for: a null opt; lambda_min, lambda0,
 * lambda_max not finite, not positive or not in that order; a negative or NaN ftol, xtol or gtol; cg_tol outside (0, 1);
 * cg_max_iters < 0; max_trials < 0; a bad group; an attached communicator.  max_trials = 0 reports the current cost and
 * does nothing else.  Every output pointer may be NULL. */
#define SFM_LM_MIN_GAIN 1e-3          /* a trial stands only if it realised more than this share of the predicted decrease */
#define SFM_LM_STOP_MAX_TRIALS 0
#define SFM_LM_STOP_FTOL       1
#define SFM_LM_STOP_XTOL       2
#define SFM_LM_STOP_GTOL       3
#define SFM_LM_STOP_LAMBDA_MAX 4
#define SFM_LM_STOP_BREAKDOWN  5
#define SFM_LM_STOP_SINGULAR   6
typedef struct sfm_lm_options {
  double lambda0, lambda_min, lambda_max;   /* 0 < lambda_min <= lambda0 <= lambda_max, all finite */
  double ftol, xtol, gtol;                  /* each >= 0; 0 switches that test off */
  double cg_tol; int cg_max_iters;          /* as sfm_ba_iterate_pcg */
  int max_trials;                           /* >= 0; linearise-solve-evaluate rounds, accepted or not */
  int quirks, group;
} sfm_lm_options;
typedef struct sfm_lm_trial {
  double lambda, cost, cost_trial, predicted, rho, step_norm, grad_inf, cg_rel;
  int cg_iters, cg_status, accepted, reserved;
} sfm_lm_trial;
/* lambda0 5, lambda_min 1e-8, lambda_max 1e8, ftol 1e-8, xtol 0, gtol 0, cg_tol 1e-10, cg_max_iters 0, max_trials 50,
 * quirks SFM_QUIRKS_REFERENCE, group 0; returns sizeof(sfm_lm_options) (0 for a null opt).  Host only. */
int sfm_lm_options_default(sfm_lm_options* opt);
int sfm_lm_trial_size(void);                /* sizeof(sfm_lm_trial); host only */
int sfm_ba_minimize_pcg(sfm_ba_problem* p, const sfm_lm_options* opt, const unsigned char* cam_mask /*host [V] or NULL*/,
                        sfm_lm_trial* log /*host [max_trials] or NULL*/, int* trials_done, int* accepted_steps,
                        int* stop_reason, double* lambda_out, double* cost_out, int* bad_camera);

/* ---- screening and culling of the resident scene's observations ----------------------------------------------------
 * Judges every observation of the resident CSR at the current state and every point by what is left of its track.  For
 * observation o of point p in camera c, with s = [R(q)^T | t]_c (X_p, 1) of the prepared cameras the linearisation reads
 * (the projection of sfm_ba_refine_points, so err2 summed over a track is its cost row 0 when cam_scale is NULL):
 *   depth[o] = s[2],   err2[o] = cam_scale[c]^2 ((s0/s2 - u)^2 + (s1/s2 - v)^2)      (cam_scale NULL: 1)
 * and obs_flags[o] is a mask of SFM_OBS_*.  The observations with none of HIGH_ERROR, BEHIND, NONFINITE are the point's
 * survivors: n_keep of them, and min_cos[p] = the minimum over survivor pairs i < j of r_i . r_j, r_i = (C_i - X) / |C_i - X|
 * (1.0 with fewer than two).  pt_flags[p] is a mask of SFM_PT_*; a point with TOO_FEW or LOW_ANGLE is dropped: its survivors
 * get SFM_OBS_POINT, so obs_flags[o] == 0 marks exactly the observations that remain.
 *   max_err2 = +inf switches the error test off, cos_min_angle >= 1 the angle test; min_obs >= 0.  A NaN or negative
 *   max_err2, cos_min_angle < -1 (or NaN), min_obs < 0 or a bad group return SFM_E_SHAPE and launch nothing.
 * `group` lanes share a point (1, 4, 8, 16, 32, 64; 0 = sfm_tri_tracks_auto_group of the scene): no output depends on it,
 * on the other points or on timing -- err2 and depth come from one lane, min_cos is a minimum, the counts are integers.
 * summary[8] (counted on the device): observations before, observations kept, HIGH_ERROR, BEHIND, NONFINITE, observations
 * dropped with their point, points dropped for TOO_FEW, points dropped for LOW_ANGLE.
 * sfm_ba_screen completes a deferred back substitution first, prepares the cameras if they are not, runs on the
 * problem's stream, uploads only cam_scale and changes nothing in the problem (state, cost history, captured graphs).
 * sfm_ba_cull screens in the same way and then removes what failed: if nothing is dropped the problem is untouched (no
 * allocation, graphs kept, summary[1] == summary[0]); otherwise a scene of (V, N, M') is built on the device (the kept
 * cam_idx / u / v scattered in their old order, cameras and points copied bit for bit, nothing uploaded) and adopted as
 * by sfm_ba_append: options, stream, communicator and a bound reduced buffer survive, the cost history restarts, graphs
 * are dropped.  Point and camera indices are stable: a dropped point keeps its slot with an empty track (and stops
 * moving), a camera may be left without observations, M' = 0 is legal.  The outputs describe the scene BEFORE the cull.
 * With a communicator attached the cull is local to this rank's points: no collective.  All output arrays are HOST
 * arrays or NULL.  Blocking. */
#define SFM_OBS_HIGH_ERROR 1   /* err2 > max_err2 */
#define SFM_OBS_BEHIND     2   /* s[2] <= 0 */
#define SFM_OBS_NONFINITE  4   /* err2 is not finite (HIGH_ERROR is then not set) */
#define SFM_OBS_POINT      8   /* none of the above, but the point was dropped */
#define SFM_PT_TOO_FEW     1   /* the track was not empty and n_keep < min_obs */
#define SFM_PT_LOW_ANGLE   2   /* n_keep >= 2, cos_min_angle < 1 and min_cos > cos_min_angle */
#define SFM_PT_EMPTY       4   /* the track was already empty (informational, not a drop) */
int sfm_ba_screen(sfm_ba_problem* p, double max_err2, double cos_min_angle, int min_obs, int group,
                  const double* cam_scale /*host [V] or NULL*/,
                  double* err2 /*host [M] or NULL*/, double* depth /*host [M] or NULL*/,
                  unsigned char* obs_flags /*host [M] or NULL*/, double* min_cos /*host [N] or NULL*/,
                  int* pt_flags /*host [N] or NULL*/, int64_t* summary /*[8] or NULL*/);
int sfm_ba_cull(sfm_ba_problem* p, double max_err2, double cos_min_angle, int min_obs, int group,
                const double* cam_scale /*host [V] or NULL*/,
                double* err2 /*host [M] or NULL*/, double* depth /*host [M] or NULL*/,
                unsigned char* obs_flags /*host [M] or NULL*/, double* min_cos /*host [N] or NULL*/,
                int* pt_flags /*host [N] or NULL*/, int64_t* summary /*[8] or NULL*/);
/* DEVICE pointer + element count of the contiguous reduced buffer (doubles).  It holds [S | rhs] between sfm_ba_linearize_reduce and
 * sfm_ba_solve_update (what the caller all-reduces); the factorisation overwrites it, and sfm_ba_iterate on one GPU may never form S
 * in it at all (SFM_INFO_REDUCE_IN_SOLVE) -- use sfm_ba_reduced_system to look at S. */
int sfm_ba_reduced_buffer(sfm_ba_problem* p, void** device_ptr, int64_t* n_doubles, int* ld);
/* Bind an externally owned DEVICE buffer (e.g. a torch tensor) as the reduced buffer. */
int sfm_ba_bind_reduced_buffer(sfm_ba_problem* p, void* device_ptr, int64_t n_doubles);

/* ---- the exchange step inside the library ("library owns its RCCL communicators") --------------
 * One process per GPU.  Rank 0 calls sfm_comm_unique_id and hands the 128 bytes to the other ranks by whatever channel the
 * application has (MPI, a file, torch.distributed ...); every rank then calls sfm_comm_create (ncclCommInitRank on the
 * device of sfm_init) and attaches the communicator to its shard's problem.  From then on sfm_ba_iterate IS the sharded
 * loop: per iteration linearise + partial reduce, ncclAllReduce(SUM, double) of the packed [S | rhs] buffer on the
 * problem's stream, replicated atomic-free solve, back substitution of the rank's own points -- K iterations enqueued by
 * ONE call, no host code between them, a plain C program included.  RCCL is loaded with dlopen on first use (librccl.so.1
 * / librccl.so: a process that already carries torch's copy gets that one); the library has no link-time dependency on it.
 * The reference has no distributed code; the algebra is ba_processor.py:376-406 (sums over points). */
typedef struct sfm_comm sfm_comm;
/* SFM_OK when RCCL can be loaded in this process (so that all ranks can agree on the library path BEFORE any of them
 * enters ncclCommInitRank), SFM_E_RCCL otherwise. */
int sfm_comm_available(void);
int sfm_comm_unique_id(char id_out[128]);
int sfm_comm_create(int world_size, int rank, const char id[128], sfm_comm** out);
int sfm_comm_destroy(sfm_comm* comm);
/* Attach (or, with NULL, detach) a communicator: the problem's iterations then all-reduce the reduced buffer that is
 * bound at that moment (the library's own, or a caller's: sfm_ba_bind_reduced_buffer). */
int sfm_ba_set_comm(sfm_ba_problem* p, sfm_comm* comm);

/* Parity hooks: per-observation terms and the reduced system at the given state (one linearisation,
 * ba_processor.py:317-382).  S is (7V x 7V) row-major (both triangles filled), rhs (7V). */
int sfm_ba_residual_jacobian(int V, int N, int64_t M, const int* pt_ptr, const int* cam_idx,
                             const double* uv_norm, const double* cams, const double* pts, int quirks,
                             double* r /*[M][2]*/, double* Jp /*[M][2][7]*/, double* Jx /*[M][2][3]*/);
int sfm_ba_reduced_system(int V, int N, int64_t M, const int* pt_ptr, const int* cam_idx,
                          const double* uv_norm, const double* cams, const double* pts,
                          double lambda, int quirks, int schur_mode,
                          double* S /*[7V][7V]*/, double* rhs /*[7V]*/);
/* sfm_ba_reduced_system of the reweighted problem (sfm_ba_set_loss(kind, delta) before the linearisation). */
int sfm_ba_reduced_system_loss(int V, int N, int64_t M, const int* pt_ptr, const int* cam_idx,
                               const double* uv_norm, const double* cams, const double* pts,
                               double lambda, int quirks, int schur_mode, int loss_kind, double loss_delta,
                               double* S /*[7V][7V]*/, double* rhs /*[7V]*/);

/* ---- descriptor matching: KeyTracker.__extend_list (key_tracker.py:213-317) ------------------------------------
 * cv2.BFMatcher.knnMatch / .match of the new view's descriptors against every earlier view (key_tracker.py:248-263),
 * the matcher built with NORM_L2 for key_type 'sift' / 'surf' and NORM_HAMMING otherwise (key_tracker.py:82-85).
 * A descriptor set is uploaded once and stays resident; sfm_match runs one query set against n_refs reference sets
 * in one launch.  Per (reference r, query i), at [r * n_query + i]: the best and second-best train index and float32
 * distance by the order (distance, train index) -- ties go to the lower index -- and, in SFM_MATCH_MUTUAL, whether i
 * is also the best query of its best train index (crossCheck, same tie rule).  Missing neighbours (a reference view
 * with one descriptor has no second) are index -1, distance +inf.
 * L2 distance = float32(sqrt(s)), correctly rounded; for integer-valued rows in [0, 255] (every uint8 set; float sets
 * checked at creation) s = sum (a - b)^2 is exact (bf16 MFMA, int32), otherwise s is an fp32 sum of unspecified
 * order.  Hamming distance = popcount(a ^ b) over the row's bytes, as a float.  Limits: L2 dim <= 256, Hamming rows
 * <= 256 bytes.  The ratio test, crossCheck filtering, duplicate removal and table writes (key_tracker.py:267-314) run
 * on the host (structure-from-motion_amd/matching.py) or, from the device outputs, in the track store below. */
#define SFM_MATCH_L2       0   /* cv2.NORM_L2 */
#define SFM_MATCH_HAMMING  1   /* cv2.NORM_HAMMING */
#define SFM_MATCH_KNN2     0   /* knnMatch(k=2): best and second best (key_tracker.py:259-260) */
#define SFM_MATCH_NN1      1   /* match() without crossCheck: the best (key_tracker.py:262-263) */
#define SFM_MATCH_MUTUAL   2   /* crossCheck: the best and the mutual flag (key_tracker.py:256-258, 83) */
#define SFM_DESC_U8        0   /* uint8 rows (every SIFT / ORB descriptor OpenCV emits as uint8 or integer float32) */
#define SFM_DESC_F32       1   /* float32 rows (L2 only) */
#define SFM_DESC_INFO_N            1
#define SFM_DESC_INFO_DIM          2
#define SFM_DESC_INFO_EXACT        3   /* 1 when the exact integer L2 path applies to this set */
#define SFM_DESC_INFO_UPLOAD_BYTES 4   /* host -> device bytes of the upload */
typedef struct sfm_desc_set sfm_desc_set;
/* Upload n rows of dim elements (bytes for Hamming) and convert them on the device.  n = 0 is a legal (empty) set. */
int sfm_desc_create(int metric, int n, int dim, int dtype, const void* data, sfm_desc_set** out);
int sfm_desc_destroy(sfm_desc_set* set);
int sfm_desc_info(const sfm_desc_set* set, int what, int64_t* value);
/* Blocking host form: every output is [n_refs][query n], caller-allocated; any output may be NULL.  A metric or dim
 * that differs between the sets, an empty reference set or an unknown mode returns SFM_E_SHAPE. */
int sfm_match(sfm_desc_set* query, int n_refs, sfm_desc_set* const* refs, int mode, int* best_idx, float* best_dist,
              int* second_idx, float* second_dist, uint8_t* mutual);
/* device form: the outputs are DEVICE pointers; enqueues on hip_stream (NULL = the library stream) and returns. */
int sfm_match_dev(sfm_desc_set* query, int n_refs, sfm_desc_set* const* refs, int mode, int* d_best_idx, float* d_best_dist,
                  int* d_second_idx, float* d_second_dist, uint8_t* d_mutual, void* hip_stream);

/* ---- guided matching: the descriptor search gated by a verified two-view model (no reference counterpart) ----------
 * sfm_match with the candidates of every query restricted to the train keys that the model of the pair of views admits.
 * Inputs: the query set with its key coordinates (qx[i], qy[i]); n_refs reference sets with theirs (rx[r][t], ry[r][t]);
 * per reference r a gate kind[r] and a row-major 3x3 model model[9 r .. 9 r + 8] in pixel coordinates; one max_err2 in
 * pixels squared.  As in sfm_twoview_verify_pairs(ref, que), the reference key is LEFT and the query key is RIGHT.
 *   SFM_GUIDE_NONE         every pair is admitted: all outputs of that reference equal sfm_match's bit for bit; its
 *                          model and coordinates are not read (they may be NULL);
 *   SFM_GUIDE_FUNDAMENTAL  (train t, query i) is admitted iff the squared Sampson distance under F = model is finite and
 *                          <= max_err2: twoview_inlier(F, x_t, y_t, x_i, y_i, max_err2), the test sfm_twoview_ransac uses;
 *   SFM_GUIDE_HOMOGRAPHY   the model is H, left to right; G = adj H by cofactors, each as fma(a, b, -(c d)):
 *                            G0 = fma(H4, H8, -(H5 H7))  G1 = fma(H2, H7, -(H1 H8))  G2 = fma(H1, H5, -(H2 H4))
 *                            G3 = fma(H5, H6, -(H3 H8))  G4 = fma(H0, H8, -(H2 H6))  G5 = fma(H2, H3, -(H0 H5))
 *                            G6 = fma(H3, H7, -(H4 H6))  G7 = fma(H1, H6, -(H0 H7))  G8 = fma(H0, H4, -(H1 H3))
 *                          (sfm_homography_adjugate), not scaled, computed once on the host; the pair is admitted iff the
 *                          transfer error in each image is finite and <= max_err2: homography_inlier((H, G), ...), the
 *                          test sfm_homography_ransac uses.  This is the test with (H, adj H): the estimator formed its
 *                          own G from the normalised matrix, so a match at the threshold may differ from its mask.
 * Per (reference r, query i), at [r * n_query + i], among the ADMITTED train keys only: the best and second-best index
 * and float32 distance by sfm_match's order (distance, train index); the mutual flag, where the best query of a train
 * key is taken among the queries admitted with it (admission is a property of the pair, so crossCheck stays
 * symmetric); n_admitted, the int32 number of admitted train keys.  No admitted key: index -1, distance +inf, mutual 0,
 * count 0.  A NaN coordinate admits nothing (the tests require a finite error).
 * Every output is optional and the non-NULL ones select the work: the cross-check runs only when mutual is wanted, the
 * counts are kept only when n_admitted is.  There is no mode argument.  SFM_E_SHAPE, with nothing launched: a NaN or
 * negative max_err2, an unknown kind, a non-finite model entry of a gated reference, a metric or dimension mismatch, an
 * empty reference set, missing coordinates of a gated pair.  Counts are integers and there is no floating-point
 * atomic: the bits of a (reference, query) row depend on that reference and that query only. */
#define SFM_GUIDE_NONE         0
#define SFM_GUIDE_FUNDAMENTAL  1
#define SFM_GUIDE_HOMOGRAPHY   2
/* Blocking host form: coordinates are HOST arrays (qx, qy of query n; rx[r], ry[r] of the reference's n), copied up;
 * outputs [n_refs][query n], caller-allocated. */
int sfm_match_guided(sfm_desc_set* query, const double* qx, const double* qy, int n_refs, sfm_desc_set* const* refs,
                     const double* const* rx, const double* const* ry, const int* kind /*[n_refs]*/,
                     const double* model /*[n_refs][9]*/, double max_err2, int* best_idx, float* best_dist, int* second_idx,
                     float* second_dist, uint8_t* mutual, int* n_admitted);
/* device form: d_qx, d_qy, the entries of the HOST arrays d_rx[n_refs], d_ry[n_refs] and the outputs are DEVICE
 * pointers; kind and model are host arrays.  Enqueues on hip_stream (NULL = the library stream) and returns. */
int sfm_match_guided_dev(sfm_desc_set* query, const double* d_qx, const double* d_qy, int n_refs, sfm_desc_set* const* refs,
                         const double* const* d_rx, const double* const* d_ry, const int* kind, const double* model,
                         double max_err2, int* d_best_idx, float* d_best_dist, int* d_second_idx, float* d_second_dist,
                         uint8_t* d_mutual, int* d_n_admitted, void* hip_stream);
/* G = adj H as above (host; needs no device). */
int sfm_homography_adjugate(const double H[9], double G[9]);

/* ---- relative pose of a verified pair: four candidates, cheirality vote, parallax -------------------------------
 * What follows a verified model of a pair of views (sfm_twoview_ransac: F; sfm_homography_ransac: H): the pose of the
 * right view in the frame of the left one, for many sets of matches in one call.  A pose (R, t) means
 * X_right = R X_left + t with |t| = 1.  The sets have the layout of sfm_twoview_ransac: set_ptr[n_sets + 1] on the host,
 * left and right [2][M] pixel coordinates; obs_mask[M] (optional, NULL = every match) selects the matches that vote;
 * model[n_sets][9] and kind[n_sets] (SFM_POSE_FROM_F or SFM_POSE_FROM_H) give the model of every set; K_left[9] and
 * K_right[9], row-major, once per call, upper triangular with K[2][2] = 1 -- anything else is SFM_E_SHAPE.
 *   1. Rays.  a = K_left^-1 (x_l, y_l, 1)^T and b = K_right^-1 (x_r, y_r, 1)^T by back substitution, third component 1.  A
 *      match is SELECTED iff its mask byte is non-zero and a, b are finite.
 *   2. Candidates from F.  E0 = K_right^T F K_left = U S V^T, s0 >= s1 >= s2; invalid unless E0 is finite and
 *      s1 > 3 eps s0.  With W = [0 -1 0; 1 0 0; 0 0 1]: R_a = det(U W V^T) U W V^T, R_b = det(U W^T V^T) U W^T V^T;
 *      t0 = +-U[:, 2] with its entry of largest magnitude positive (the lowest index on a tie).  The rotations are ordered
 *      by trace, the larger first: R_0, R_1.  Candidate c = 2 i + j is (R_i, t0) for j = 0 and (R_i, -t0) for j = 1.
 *   3. Candidates from H.  Hn = K_right^-1 H K_left; invalid unless Hn is finite and s2 > 3 eps s0 (the rank test of the
 *      robust homography).  Hn is divided by s1.  Sign vote: over the selected matches the counts of b . (Hn a) > 0 and
 *      < 0, integers; Hn is negated iff the negatives outnumber the positives.  With the eigenvalues l0 >= l1 >= l2 of
 *      Hn^T Hn and their eigenvectors v0, v1, v2 (v0 x v1 = v2): invalid unless l0 - l2 > 0;
 *      u+- = (sqrt(1 - l2) v0 +- sqrt(l0 - 1) v2) / sqrt(l0 - l2), the radicands clamped at 0; for each sign
 *      U = [v1, u, v1 x u], W = [Hn v1, Hn u, (Hn v1) x (Hn u)], R = W U^T, n = v1 x u, T = (Hn - R) n (the four-solution
 *      decomposition of Ma, Soatto, Kosecka and Sastry).  A rotation whose T is not finite or zero is invalid with both
 *      its candidates.  The rotations are ordered by trace, the larger first; t0 = T / |T| takes the sign of step 2 and
 *      the candidates 2 i + j are formed as there.  n_out is the normal of the winner, scaled and signed so that
 *      Hn = R + (|T| t_out) n_out^T; zeros for kind F.
 *   4. The test (pose_front, csrc/sfm_obs_test.h; one function for every stage and for sfm_twoview_pose_test).  For a
 *      candidate (R, t) and a selected match: a' = R a; p = a'.a', q = b.b, r = a'.b, d = p q - r r;
 *      m1 = r (b.t) - q (a'.t), m2 = p (b.t) - r (a'.t): the numerators of the two midpoint depths over the common
 *      denominator d.  IN FRONT iff d, m1, m2 are finite and d > 0, m1 > 0, m2 > 0; no division.  HAS PARALLAX iff in
 *      front and not (r > 0 and r r > cos2_min p q).  cos2_min is the squared cosine of the caller's minimum triangulation
 *      angle, in [0, 1]; NaN or a value outside is SFM_E_SHAPE.  In the operation order of the function:
 *        a'_i = fma(R[3i], a0, fma(R[3i+1], a1, R[3i+2]));  p = fma(a'0, a'0, fma(a'1, a'1, a'2 a'2));
 *        q = fma(b0, b0, fma(b1, b1, 1));  r = fma(a'0, b0, fma(a'1, b1, a'2));  d = fma(p, q, -(r r));
 *        bt = fma(b0, t0, fma(b1, t1, t2));  at = fma(a'0, t0, fma(a'1, t1, a'2 t2));
 *        m1 = fma(r, bt, -(q at));  m2 = fma(p, bt, -(r at));  parallax: not (r > 0 and r r > cos2_min (p q)).
 *   5. Score, lexicographic: the number of selected matches in front (an integer), then the lower candidate number.  A
 *      winner needs a count of at least 1, otherwise SFM_POSE_NO_POSE.
 *   6. Status bits as below.  min_parallax >= 0 is an integer option; a negative one is SFM_E_SHAPE.
 *   7. Outputs, all optional but R_out and t_out: R_out[n_sets][9], t_out[n_sets][3] (zeros without a winner), n_out
 *      [n_sets][3], cand_front[n_sets][4] (-1 for an invalid candidate), n_front and n_parallax of the winner, best_cand
 *      (-1 without a winner), status, obs_front[M] (1 in front, 2 with parallax, 0 otherwise), X_out[3][M] (the midpoint
 *      (lambda1 a' + t + lambda2 b) / 2 taken back to the left frame; NaN where the match is not in front), summary[6]:
 *      sets posed | sets with a selected match and no winner (NO_MODEL, or NO_POSE alone) | EMPTY | TIED among the posed |
 *      matches in front | selected matches of posed sets that are not in front.
 *   8. No floating-point atomic, integer counts: a set's bits depend on the set, the intrinsics and the options only.  The
 *      call returns when the work is done and the work buffers are back in the pool; the _dev form takes device pointers
 *      (set_ptr, kind, model, K_left, K_right stay host arrays) and a stream (NULL = the library stream).  Both forms check
 *      their arguments before they look for a device: a bad argument is SFM_E_SHAPE on a machine without one. */
#define SFM_POSE_FROM_F       0
#define SFM_POSE_FROM_H       1
#define SFM_POSE_EMPTY        1   /* no selected match */
#define SFM_POSE_NO_MODEL     2   /* the model is invalid by step 2 or step 3 */
#define SFM_POSE_NO_POSE      4   /* there is no winner: no valid candidate has a selected match in front */
#define SFM_POSE_TIED         8   /* another valid candidate has the winner's count */
#define SFM_POSE_NO_PARALLAX 16   /* the winner's parallax count is below min_parallax */
#define SFM_POSE_CANDIDATES   4
int sfm_twoview_pose(int n_sets, const int* set_ptr /*host [n_sets+1]*/, int64_t M, const double* left /*[2][M]*/,
                     const double* right /*[2][M]*/, const unsigned char* obs_mask /*[M] or NULL*/,
                     const double* model /*[n_sets][9]*/, const int* kind /*[n_sets]*/, const double K_left[9],
                     const double K_right[9], double cos2_min, int min_parallax, double* R_out /*[n_sets][9]*/,
                     double* t_out /*[n_sets][3]*/, double* n_out, int* cand_front, int* n_front, int* n_parallax, int* best_cand,
                     int* status, unsigned char* obs_front, double* X_out /*[3][M]*/, int64_t* summary /*[6]*/);
int sfm_twoview_pose_dev(int n_sets, const int* set_ptr /*host*/, int64_t M, const double* d_left, const double* d_right,
                         const unsigned char* d_obs_mask, const double* model /*host*/, const int* kind /*host*/,
                         const double K_left[9] /*host*/, const double K_right[9] /*host*/, double cos2_min, int min_parallax,
                         double* d_R_out, double* d_t_out, double* d_n_out, int* d_cand_front, int* d_n_front,
                         int* d_n_parallax, int* d_best_cand, int* d_status, unsigned char* d_obs_front, double* d_X_out,
                         int64_t* d_summary, void* hip_stream);
/* The test of step 4 on the host (needs no device): a and b are the first two components of the rays. */
int sfm_twoview_pose_test(const double R[9], const double t[3], const double a[2], const double b[2], double cos2_min,
                          int* front, int* parallax);

/* ---- refinement of a relative pose: damped Gauss-Newton on the Sampson distance, five parameters -----------------
 * What follows sfm_twoview_pose: for many sets of matches in one call, a given pose (R, t), X_right = R X_left + t, is
 * moved on its 5-dimensional manifold to the minimum of the sum of squared Sampson distances IN PIXELS of the selected
 * matches, and the matches are judged against the result.  The sets, obs_mask and the intrinsics are those of
 * sfm_twoview_pose; R_in[n_sets][9] (row-major) and t_in[n_sets][3] are the poses.  Options: lambda >= 0 (damping),
 * iters >= 0, max_err2 >= 0 (the judge's squared Sampson bound), cos2_min in [0, 1]; anything else is SFM_E_SHAPE.
 *   1. Selected.  A match is SELECTED iff its mask byte is non-zero and its four pixel coordinates are finite; n_used is
 *      their number.
 *   2. Pose check.  A set whose R_in or t_in is not finite, or whose t_in is zero (or has no finite squared length), is
 *      BAD_POSE -- a set sfm_twoview_pose left without a winner is.  Otherwise t = t_in / |t_in|; R_in is taken as a
 *      rotation, it is the caller's.
 *   3. Model of a pose (refine_model, csrc/sfm_obs_test.h).  E = [t]x R; F = K_right^-T E K_left^-1 by substitution through
 *      the triangular intrinsics, not scaled.  Chart at (R, t): theta = (w0, w1, w2, d0, d1), R(theta) = exp([w]x) R by
 *      Rodrigues' formula, t(theta) = (t + d0 b1 + d1 b2) / |.| with k the index of the smallest |t_k| (the lowest on a tie),
 *      b1 = (t x e_k) / |t x e_k|, b2 = t x b1.  The derivatives at theta = 0 are dF_j = K_right^-T dE_j K_left^-1 with
 *      dE_j = [t]x [e_j]x R for j < 3, dE_3 = [b1]x R, dE_4 = [b2]x R.
 *   4. Residual of a match (refine_residual, csrc/sfm_obs_test.h; one function for the passes, the judge and
 *      sfm_twoview_refine_test).  With x = (x_l, y_l, 1), y = (x_r, y_r, 1), a = F x, b = F^T y: e = y . a,
 *      s = a0^2 + a1^2 + b0^2 + b1^2, r = e / sqrt(s), and with da = dF_j x, db = dF_j^T y
 *      J_j = (y . dF_j x) / sqrt(s) - (e / s^(3/2)) (a0 da0 + a1 da1 + b0 db0 + b1 db1).  In the operation order of the function:
 *        a_i = fma(F[3i], x_l, fma(F[3i+1], y_l, F[3i+2]));  b_i = fma(F[i], x_r, fma(F[3+i], y_r, F[6+i]));
 *        e = fma(x_r, a0, fma(y_r, a1, a2));  s = fma(a0, a0, a1 a1) + fma(b0, b0, b1 b1);  r = e / sqrt(s);
 *        de = fma(x_r, da0, fma(y_r, da1, da2));  g = fma(a0, da0, fma(a1, da1, fma(b0, db0, b1 db1)));
 *        J_j = fma(-(r / s), g, de (1 / sqrt(s))).
 *   5. One pass.  c = sum r^2, U = sum J^T J (15 sums), g = sum J^T r (5 sums) over the selected matches; an unselected match
 *      adds zeros.  The 21 sums are formed per slice of 64 consecutive matches of the set and the slices are added in
 *      slice order.
 *   6. One step.  (U + lambda diag U) d = -g by a 5x5 Cholesky factorisation; a pivot that is not finite or not > 0 sets
 *      SINGULAR and ends the iterations at the standing pose.  Otherwise the pose becomes (R(d), t(d)).  `iters` steps,
 *      unconditionally -- no step is accepted or rejected -- and at most iters + 1 passes: the last pass gives the cost and
 *      U at the iterated pose.
 *   7. Guard.  The output is the iterated pose iff a step was taken, every entry of the pose and both costs are finite
 *      (NONFINITE otherwise) and c_out <= c_in (1 + 2^-30).  Otherwise the input (R_in, t_in) comes back bit for bit, with
 *      KEPT_INPUT, its cost in both entries of `cost` and U of the first pass in `info`.  iters = 0 is a pure evaluation.
 *   8. Too few.  n_used < 8 is TOO_FEW (EMPTY as well at 0): no pass is made and the input comes back.
 *   9. Judge at the output pose (R_out, t_out as they are written), over every match of the set whether selected or not:
 *      obs_res[M] the signed residual of step 4 (NaN where a coordinate is not finite or the set is BAD_POSE);
 *      obs_inlier[M] = twoview_inlier(F_out, ..., max_err2); obs_front[M] 0 / 1 / 2 by the test of the relative pose
 *      (pose_front) at cos2_min, needing finite rays; X_out[3][M] the midpoint as sfm_twoview_pose gives it, NaN where the
 *      match is not in front; n_inliers, n_front, n_parallax count the SELECTED matches.  A BAD_POSE set has zeros.
 *  10. Outputs, all optional but R_out and t_out: F_out[n_sets][9] the pixel fundamental matrix of the output pose with
 *      the norm and sign of sfm_twoview_ransac's F_out (zeros for BAD_POSE); cost[2][n_sets] the input and the output
 *      cost and info[n_sets][15] the upper triangle of U at the output pose, row by row (zeros where no pass was made);
 *      n_used, status; summary[6]: sets that made a pass | BAD_POSE | other sets with EMPTY or TOO_FEW | KEPT_INPUT among
 *      the first | their inliers | their selected matches that are not inliers.
 *  No floating-point atomic: a set's bits depend on the set, its pose, the intrinsics and the options only.  The _dev
 *  form takes device pointers (set_ptr and the intrinsics stay host arrays) and a stream (NULL = the library stream).
 *  Both forms check their arguments before they look for a device. */
#define SFM_REFINE_EMPTY       1   /* no selected match */
#define SFM_REFINE_TOO_FEW     2   /* fewer than 8 selected matches */
#define SFM_REFINE_BAD_POSE    4   /* the input pose is not finite or its translation is zero */
#define SFM_REFINE_SINGULAR    8   /* a pivot of the damped normal equations was not positive: the iterations ended there */
#define SFM_REFINE_NONFINITE  16   /* the iterated pose or a cost is not finite */
#define SFM_REFINE_KEPT_INPUT 32   /* the output is the input, bit for bit */
int sfm_twoview_refine(int n_sets, const int* set_ptr /*host [n_sets+1]*/, int64_t M, const double* left /*[2][M]*/,
                       const double* right /*[2][M]*/, const unsigned char* obs_mask /*[M] or NULL*/,
                       const double* R_in /*[n_sets][9]*/, const double* t_in /*[n_sets][3]*/, const double K_left[9],
                       const double K_right[9], double lambda, int iters, double max_err2, double cos2_min,
                       double* R_out /*[n_sets][9]*/, double* t_out /*[n_sets][3]*/, double* F_out, double* cost /*[2][n_sets]*/,
                       double* info /*[n_sets][15]*/, int* n_used, int* status, double* obs_res /*[M]*/,
                       unsigned char* obs_inlier, unsigned char* obs_front, double* X_out /*[3][M]*/, int* n_inliers,
                       int* n_front, int* n_parallax, int64_t* summary /*[6]*/);
int sfm_twoview_refine_dev(int n_sets, const int* set_ptr /*host*/, int64_t M, const double* d_left, const double* d_right,
                           const unsigned char* d_obs_mask, const double* d_R_in, const double* d_t_in,
                           const double K_left[9] /*host*/, const double K_right[9] /*host*/, double lambda, int iters,
                           double max_err2, double cos2_min, double* d_R_out, double* d_t_out, double* d_F_out, double* d_cost,
                           double* d_info, int* d_n_used, int* d_status, double* d_obs_res, unsigned char* d_obs_inlier,
                           unsigned char* d_obs_front, double* d_X_out, int* d_n_inliers, int* d_n_front, int* d_n_parallax,
                           int64_t* d_summary, void* hip_stream);
/* Steps 3 and 4 on the host (needs no device): the residual and the Jacobian row of one match at the pose (R, t) as given. */
int sfm_twoview_refine_test(const double R[9], const double t[3], const double K_left[9], const double K_right[9], double xl,
                            double yl, double xr, double yr, double* r, double J[5]);

/* ---- robust essential matrix: sampled five-point hypotheses ----------------------------------------------------------
 * The calibrated estimator of the two-view chain: every hypothesis comes from five matches and the caller's intrinsics
 * and is an essential matrix already.  Sets are laid out as in sfm_twoview_ransac: set_ptr[n_sets + 1] on the host, left
 * and right [2][M] pixels; K_left, K_right as in sfm_twoview_pose (upper triangular, K[2][2] = 1, else SFM_E_SHAPE).  Per
 * set of n matches:
 *   1. n < 6: SFM_ESSENTIAL_TOO_FEW.
 *   2. Rays a = K_left^-1 (x_l, y_l, 1)^T, b = K_right^-1 (x_r, y_r, 1)^T by back substitution.
 *   3. The test of a match against an essential matrix E is twoview_inlier(F, ...): the squared Sampson distance in
 *      pixels against max_err2, with F = K_r^-T E K_l^-1 formed by substitution through the triangular intrinsics and
 *      scaled to Frobenius norm 1 with its entry of largest magnitude positive.  One function forms F in the hypothesis
 *      kernel and on the host; one function tests in the hypothesis kernel, the score and the judge.
 *   4. H = max_hyp hypotheses (0 = 128; 1 .. 65 536).  Hypothesis h uses, for k = 0 .. 4, the match
 *      lo_k + mix(5 h + k) mod (hi_k - lo_k), lo_k = floor(k n / 5), hi_k = floor((k + 1) n / 5), mix the splitmix64 finaliser.
 *   5. The solutions of a sample: with N0 .. N3 a basis of the null space of the 5x9 matrix of rows b (x) a (entry
 *      3 i + j multiplies b_i a_j), the real solutions (x, y, z) of det E = 0 and 2 E E^T E - tr(E E^T) E = 0 for
 *      E = x N0 + y N1 + z N2 + N3.  Each E is scaled to Frobenius norm 1 with its entry of largest magnitude positive
 *      (the lowest index on a tie); the solutions are numbered r = 0, 1, ... by ascending E[0] of that form.  At most ten;
 *      non-finite ones are left out.  How null space and roots are found is not part of the rule.
 *   6. Sample gate: a candidate is invalid unless its own five matches are inliers of it.
 *   7. Score, lexicographic: the inlier count over all n matches, then the lower h, then the lower r.  A winner needs a
 *      count of at least 6, otherwise SFM_ESSENTIAL_NO_MODEL.  There is no refit (compose sfm_twoview_refine).
 *   8. Outputs, all optional but E_out: E_out[n_sets][9] canonical as in step 5; F_out[n_sets][9] as in step 3 (the norm
 *      and sign of sfm_twoview_ransac's F_out); obs_inlier[M], n_inliers, best_hyp, best_root (-1 without a model);
 *      n_valid[n_sets] the candidates that passed the gate; status; summary[6]: sets solved | NO_MODEL | TOO_FEW | 0 |
 *      matches flagged inlier | matches of solved sets flagged outlier.  Zeros for TOO_FEW and NO_MODEL.
 *  No floating-point atomic, integer counts: a set's bits depend on its matches, the intrinsics and the options only.
 *  The _dev form takes device pointers (set_ptr and the intrinsics stay host arrays; d_summary is int64[6] on the device)
 *  and a stream (NULL = the library stream).  Both forms check their arguments (a NaN or negative max_err2, max_hyp out of
 *  range, bad offsets, bad intrinsics: SFM_E_SHAPE) before they look for a device. */
#define SFM_ESSENTIAL_TOO_FEW   1   /* the set has fewer than 6 matches */
#define SFM_ESSENTIAL_NO_MODEL  2   /* no valid candidate with at least 6 inliers */
int sfm_essential_ransac(int n_sets, const int* set_ptr /*host [n_sets+1]*/, int64_t M, const double* left /*[2][M]*/,
                         const double* right /*[2][M]*/, const double K_left[9], const double K_right[9], double max_err2,
                         int max_hyp, double* E_out /*[n_sets][9]*/, double* F_out /*[n_sets][9]*/, unsigned char* obs_inlier,
                         int* n_inliers, int* best_hyp, int* best_root, int* n_valid, int* status, int64_t* summary /*[6]*/);
int sfm_essential_ransac_dev(int n_sets, const int* set_ptr /*host*/, int64_t M, const double* d_left, const double* d_right,
                             const double K_left[9] /*host*/, const double K_right[9] /*host*/, double max_err2, int max_hyp,
                             double* d_E_out, double* d_F_out, unsigned char* d_obs_inlier, int* d_n_inliers, int* d_best_hyp,
                             int* d_best_root, int* d_n_valid, int* d_status, int64_t* d_summary, void* hip_stream);
/* Step 4 on the host: the five indices of hypothesis h of a set of n matches; returns H (0 for n < 6 or a bad max_hyp).
 * idx is written only for 0 <= h < H. */
int sfm_essential_sample(int n, int max_hyp, int h, int idx[5]);
/* Step 5 on the host, by the function the hypothesis kernel runs: a[5][2], b[5][2] the first two components of the rays,
 * E[10][9] the canonical solutions in the order of step 5 (zeros beyond *n). */
int sfm_essential_solve(const double* a /*[5][2]*/, const double* b /*[5][2]*/, double* E /*[10][9]*/, int* n);

/* ---- robust similarity: sampled three-point hypotheses, inlier refit; moving and aligning the resident scene ---------
 * What every call above returns lives in a frame of its own: a verified pair in the pair's frame with a baseline of
 * length one, a resident scene in the gauge of its first two views, surveyed points in metres.  The relation between two
 * such frames is the seven-parameter similarity b ~ s A a + t (s > 0, A a rotation), the sixth robust estimator.
 * A call holds n_sets sets of 3D-3D correspondences; src and dst are [3][M] (the x row, the y row, the z row); set k owns
 * the correspondences set_ptr[k] .. set_ptr[k + 1] - 1, n of them.  The rule, per set:
 *   1. n < 4: SFM_SIMILARITY_TOO_FEW.
 *   2. The test.  A model under test is 12 doubles (Mx, t) with Mx[i][j] = s * A[i][j] (one rounding each).
 *      e_i = b_i - fma(Mx_i0, a_x, fma(Mx_i1, a_y, fma(Mx_i2, a_z, t_i))); lhs = fma(e_0, e_0, fma(e_1, e_1, e_2 * e_2)).
 *      A correspondence is an INLIER iff lhs is finite and lhs <= max_err2, in squared units of the dst frame.  The
 *      back-transfer error times s^2 is the same quantity, so there is no second half.  One function (similarity_inlier,
 *      csrc/sfm_obs_test.h) that every stage below calls.
 *   3. Hypotheses.  H = max_hyp (0 means 128; range 1 .. 65 536), whatever n.  Hypothesis h uses, for k = 0 .. 2, the
 *      correspondence lo_k + mix(3 h + k) mod (hi_k - lo_k) with lo_k = floor(k n / 3), hi_k = floor((k + 1) n / 3): one of
 *      every third of the set, so the three indices are distinct and ascending.  mix is the splitmix64 finaliser of the
 *      two-view rule.  sfm_similarity_sample returns the same indices on any machine.
 *   4. Model of a sample, and of an inlier set (Umeyama 1991).  Over its m correspondences the centroids mu_a, mu_b first;
 *      from the centred coordinates Sigma = (1/m) sum (b - mu_b)(a - mu_a)^T and var_a = (1/m) sum |a - mu_a|^2 (two passes:
 *      targets a million units from the origin lose nothing).  With Sigma = U D V^T, A = U diag(1, 1, det U det V) V^T,
 *      never a reflection; s = (D_0 + D_1 + det U det V D_2) / var_a, or s = 1 with SFM_SIMILARITY_RIGID in flags;
 *      t = mu_b - s A mu_a.  Valid iff everything is finite, var_a > 0, s > 0 and D_1 > 3 eps D_0: a collinear sample leaves
 *      the rotation about its line free.  How the decomposition is computed is not part of the rule.
 *   5. Sample gate.  A hypothesis is invalid unless its own three correspondences are inliers of it (with scale, three
 *      points over-determine the seven parameters).
 *   6. Score, lexicographic: the inlier count over all n (an integer); then the lower h.  A winner needs a count of at
 *      least 4, otherwise SFM_SIMILARITY_NO_MODEL.
 *   7. Refit, up to `iters` rounds.  Step 4 over the inliers of the standing model.  The round stands iff its model is
 *      valid and its inlier count over all n is at least the standing count; otherwise the rounds stop.
 *      SFM_SIMILARITY_KEPT_HYPOTHESIS iff iters > 0 and no round stood.
 *   8. Outputs, all optional but sim_out.  sim_out[n_sets][13]: s, A row-major, t of the standing model; thirteen zeros with
 *      TOO_FEW or NO_MODEL.  obs_inlier[M], n_inliers, best_hyp (-1 without a model), status and summary[6] have the meaning
 *      and order they have for sfm_homography_ransac and describe the standing model, judged once more by the function of
 *      step 2.
 * No floating-point atomic, integer counts, slice-ordered sums: a set's bits depend on its correspondences and the options
 * only.  Argument errors (a NaN or negative max_err2, max_hyp out of range, iters < 0, unknown flag bits, bad offsets, a
 * null array: SFM_E_SHAPE, nothing launched, outputs untouched) are found before a device is looked for.  The _dev form
 * takes device pointers (set_ptr stays a host array, d_summary is int64[6] on the device) and a stream (NULL = the library
 * stream); it returns when the work is done. */
#define SFM_SIMILARITY_TOO_FEW          1   /* the set has fewer than 4 correspondences */
#define SFM_SIMILARITY_NO_MODEL         2   /* no valid hypothesis with at least 4 inliers */
#define SFM_SIMILARITY_KEPT_HYPOTHESIS  4   /* no refit round stood: the model is the winning hypothesis itself */
#define SFM_SIMILARITY_RIGID            1   /* flags: s = 1, a rigid motion */
int sfm_similarity_ransac(int n_sets, const int* set_ptr /*host [n_sets+1]*/, int64_t M, const double* src /*[3][M]*/,
                          const double* dst /*[3][M]*/, double max_err2, int max_hyp, int iters, int flags,
                          double* sim_out /*[n_sets][13]: s, A row-major, t*/, unsigned char* obs_inlier /*[M] or NULL*/,
                          int* n_inliers /*[n_sets] or NULL*/, int* best_hyp /*[n_sets] or NULL*/,
                          int* status /*[n_sets] or NULL*/, int64_t* summary /*[6] or NULL*/);
int sfm_similarity_ransac_dev(int n_sets, const int* set_ptr /*host [n_sets+1]*/, int64_t M, const double* d_src,
                              const double* d_dst, double max_err2, int max_hyp, int iters, int flags, double* d_sim_out,
                              unsigned char* d_obs_inlier, int* d_n_inliers, int* d_best_hyp, int* d_status,
                              int64_t* d_summary, void* hip_stream);
/* Host only, needs no device: the hypothesis count H of a set of n correspondences (0 for n < 4 or a max_hyp out of range)
 * and, for 0 <= h < H, the three ascending indices of hypothesis h. */
int sfm_similarity_sample(int n, int max_hyp, int h, int idx[3]);

/* ---- rotation averaging: spanning-tree hypotheses of a view graph, inlier refit on the Lie algebra -------------------
 * The seventh robust estimator.  A graph has V views and E edges; edge e is (i_e, j_e, Rel_e[9]) with i_e != j_e and says
 * R_j = Rel_e R_i, R_v taking world coordinates to the frame of view v: the R of sfm_twoview_pose with left i and right j.
 * Parallel edges are allowed.  `root` is the view whose rotation is the identity.  All matrices are row-major.  The rule:
 *   1. The test.  For rotations R_i, R_j and edge e, P = Rel_e R_i with
 *        P[a][b] = fma(Rel[a][0], R_i[0][b], fma(Rel[a][1], R_i[1][b], Rel[a][2] * R_i[2][b])),
 *      lhs = trace(R_j^T P), started as P[0][0] * R_j[0][0] and continued lhs = fma(P[a][b], R_j[a][b], lhs) over the other
 *      eight entries in row-major order.  The edge is an INLIER iff lhs is finite and lhs >= fma(2, cos_max, 1); cos_max, in
 *      (0, 1], is the cosine of the largest admitted residual angle.  No division, no acos.  One function
 *      (rotation_edge_inlier, csrc/sfm_obs_test.h) that every stage calls; sfm_rotation_edge_test is its host entry.
 *   2. Hypotheses: spanning trees.  H = max_hyp (0 means 128; range 1 .. 65 536).  Hypothesis h is a breadth-first tree from
 *      the view `root` for h = 0 and mix((h << 32) | 0xFFFFFFFF) mod V otherwise (64-bit words).  The views of level d are
 *      those without a depth that have an edge to a view of depth d - 1; such a view takes as parent edge the one among
 *      those edges with the smallest (key, e), key = e for h = 0 and mix((h << 32) | e) otherwise; mix is the splitmix64
 *      finaliser of the two-view rule.  Rotations follow the tree from the identity at its root: forward along an edge
 *      R_j = Rel_e R_i by the product of step 1, backward R_i = Rel_e^T R_j with
 *        Q[a][b] = fma(Rel[0][a], R_j[0][b], fma(Rel[1][a], R_j[1][b], Rel[2][a] * R_j[2][b])).
 *      Views the tree does not reach hold NaN.  A hypothesis is valid iff its tree has an edge, reaches `root` and every
 *      reached rotation is finite.  sfm_rotation_tree returns the same tree on any machine.
 *   3. Score, lexicographic: the inlier count over all E edges (an integer; an edge with a NaN end is an outlier, a tree edge
 *      an inlier by construction); then the lower h.  No valid hypothesis (root has no edge): SFM_ROTAVG_NO_MODEL.
 *   4. Gauge.  The winner is multiplied on the right by R_root^T once,
 *        G[a][b] = fma(R_v[a][0], R_root[b][0], fma(R_v[a][1], R_root[b][1], R_v[a][2] * R_root[b][2])),
 *      and the root itself takes the exact identity.  The count that stands is the one scored.
 *   5. Refit, up to `iters` rounds of `steps` Gauss-Newton steps each.  S is the inlier set of the standing model; the FREE
 *      views are those connected to `root` through edges of S, except `root`; every other view is held for the round.  Per
 *      step, for every edge of S between connected views, d_e = log(R_j^T Rel_e R_i) as a 3-vector (with v the vee of
 *      (M - M^T) / 2, c = (trace - 1) / 2: d = (atan2(|v|, c) / |v|) v, the series 1 + |v|^2 / 6 + 3 |v|^4 / 40 below |v| = 1e-4;
 *      cos_max > 0 keeps the angle below a quarter turn).  The update w minimises sum_S |d_e + w_i - w_j|^2 with w = 0 on
 *      `root` and on held views: the graph Laplacian of S (integer degrees) times I_3 on the free views, right-hand side
 *      b_v = sum of d_e over the edges of S with j_e = v minus the sum over those with i_e = v.  Then R_v <- R_v exp([w_v]x).
 *      How the system is solved is not part of the rule; the library runs Jacobi-preconditioned conjugate gradients from
 *      w = 0 until |r|^2 <= cg_tol^2 |b|^2 or for cg_max iterations (then SFM_ROTAVG_CG_LIMIT is set and the step is taken
 *      with what it has).  A round stands iff every rotation of a free view is finite and its inlier count over all E is at
 *      least the standing count; otherwise the rounds stop.  SFM_ROTAVG_KEPT_HYPOTHESIS iff iters > 0 and no round stood.
 *   6. Outputs, all optional but R_out.  R_out[V][9]: nine zeros for a view outside root's component, or with no model.
 *      edge_inlier[E] (0 with no model).  edge_cos[E]: (lhs - 1) / 2 of the standing model, NaN where an end has no rotation.
 *      view_status[V]: SFM_ROTAVG_UNREACHED, no path from `root` in the input graph; SFM_ROTAVG_HELD, not connected to `root`
 *      through the final inlier edges (its rotation is the last one it had; with no model every view is held).  n_inliers,
 *      best_hyp (-1 with no model), status.  summary[6]: views with a rotation | unreached | held | inlier edges | outlier
 *      edges between two views with rotations | rounds that stood.
 *   7. Argument errors (SFM_E_SHAPE, found before a device is looked for, nothing launched, outputs untouched): V < 2, E < 1,
 *      E >= 2^31 (and E >= 2^30: the 2 E edge ends are numbered by an int), an index out of range, i == j, root out of range,
 *      cos_max NaN or outside (0, 1], max_hyp out of range, iters < 0, steps < 1, cg_tol not in (0, 1), cg_max < 1, a null
 *      array.  Each Rel_e must pass verify_rotation: SFM_E_BAD_ROTATION, sfm_last_error naming the lowest such edge (the
 *      _dev form finds it with one kernel, before anything else is launched).
 * No floating-point atomic, integer counts, dot products per slice of 64 views in slice order: the bits depend on the graph
 * and the options only.  The hypotheses are scored in batches whose rotations [batch][V][9] stay within 256 MiB; the winner
 * is carried across batches by (count, h).  One graph per call.  The _dev form takes d_rel and every output on the device
 * and a stream (NULL = the library stream); `edges` stays a HOST array, as set_ptr does elsewhere: it is checked, uploaded
 * and turned into the view-major adjacency by the call.  It returns when the work is done. */
#define SFM_ROTAVG_NO_MODEL         1   /* status: no valid spanning tree */
#define SFM_ROTAVG_KEPT_HYPOTHESIS  2   /* status: no refit round stood: the model is the winning tree itself */
#define SFM_ROTAVG_CG_LIMIT         4   /* status: a Gauss-Newton step ended its CG at cg_max */
#define SFM_ROTAVG_UNREACHED        1   /* view_status: no path from root in the input graph */
#define SFM_ROTAVG_HELD             2   /* view_status: not connected to root through the final inlier edges */
int sfm_rotation_average(int V, int64_t E, const int* edges /*[E][2]*/, const double* rel /*[E][9]*/, int root, double cos_max,
                         int max_hyp, int iters, int steps, double cg_tol, int cg_max, double* R_out /*[V][9]*/,
                         unsigned char* edge_inlier /*[E] or NULL*/, double* edge_cos /*[E] or NULL*/,
                         int* view_status /*[V] or NULL*/, int* n_inliers, int* best_hyp, int* status, int64_t* summary /*[6]*/);
int sfm_rotation_average_dev(int V, int64_t E, const int* edges /*host [E][2]*/, const double* d_rel, int root, double cos_max,
                             int max_hyp, int iters, int steps, double cg_tol, int cg_max, double* d_R_out,
                             unsigned char* d_edge_inlier, double* d_edge_cos, int* d_view_status, int* d_n_inliers,
                             int* d_best_hyp, int* d_status, int64_t* d_summary, void* hip_stream);
/* Host only, needs no device: the hypothesis count H (0 for bad arguments) and, for 0 <= h < H, the tree of hypothesis h:
 * parent_edge_out[V] (-1 for the tree's root and for views it does not reach) and depth_out[V] (-1 where not reached). */
int sfm_rotation_tree(int V, int64_t E, const int* edges /*[E][2]*/, int root, int max_hyp, int h, int* parent_edge_out, int* depth_out);
/* Step 1 on the host, by the function the kernels run: 1 for an inlier, *lhs_out (may be NULL) the trace. */
int sfm_rotation_edge_test(const double Ri[9], const double Rj[9], const double Rel[9], double cos_max, double* lhs_out);
/* The batch plan, host only: hypotheses per batch and the number of batches for V views under a cap of cap_bytes on the
 * rotations of a batch.  cap_bytes also becomes the cap of the calls that follow (a hook for tests); 0 restores 256 MiB. */
int sfm_rotation_plan(int V, int max_hyp, int64_t cap_bytes, int* batch, int* n_batches);

/* ---- translation averaging: view positions from the directions of a view graph, rotations known ----------------------
 * The graph is that of the rotation averaging: V views, E edges (i_e, j_e), i_e != j_e, parallel edges allowed.  R[V][9] are
 * the absolute rotations (world to view, row-major: the R_out of sfm_rotation_average; nine zeros: the view has no
 * rotation), t[E][3] the t of sfm_twoview_pose with left i_e and right j_e (X_j = Rel X_i + t; its length is not used),
 * edge_mask[E] optional bytes (0 excludes an edge; NULL: none is excluded).  `root` is the view at the origin.  The rule:
 *   1. Directions.  u[a] = -fma(R_j[0][a], t[0], fma(R_j[1][a], t[1], R_j[2][a] * t[2])), m = fma(u[0], u[0], fma(u[1], u[1],
 *      u[2] * u[2])), d_e[a] = u[a] / sqrt(m): with R_j = Rel_e R_i the world direction from c_i to c_j.  The edge is USED iff
 *      its mask byte is non-zero (or there is no mask), both ends have a rotation (an entry of the nine is non-zero) and
 *      tt = fma(t[0], t[0], fma(t[1], t[1], t[2] * t[2])) is finite and positive.  Every other edge has weight 0 throughout
 *      and verdict 0.
 *   2. The test.  For positions c: v = c_j - c_i, dv = fma(d[0], v[0], fma(d[1], v[1], d[2] * v[2])), n2 = fma(v[0], v[0],
 *      fma(v[1], v[1], v[2] * v[2])).  A used edge is an INLIER iff dv and n2 are finite, dv > 0 and dv * dv >= cc * n2 with
 *      cc = cos_max * cos_max formed once; cos_max, in (0, 1], is the cosine of the largest admitted angle between d_e and
 *      c_j - c_i.  No division, no square root, no acos.  One function (translation_edge_inlier, csrc/sfm_obs_test.h) that
 *      every stage calls; sfm_translation_edge_test is its host entry.
 *   3. A solve takes weights w_e and target lengths l_e; an edge takes part iff w_e > 0 (a NaN does not).  The FREE views are
 *      those joined to `root` through edges that take part, except `root`; every other view is held at the position it has
 *      (zero before the first solve); `root` is at zero throughout.  The solve minimises
 *        sum_e w_e ( |P_e v_e|^2 + mu (d_e . v_e - l_e)^2 ),  P_e = I - d_e d_e^T,  v_e = c_j - c_i
 *      over the free views (mu in (0, 1]; 0 means 0.01): a symmetric positive definite system of 3x3 blocks with the edge
 *      block B_e = w_e (I - (1 - mu) d_e d_e^T), the diagonal block of a view the sum of B_e over its edges, -B_e between
 *      the ends of an edge, and the right-hand side + w_e mu l_e d_e at j_e, - the same at i_e.  The library forms, per
 *      view and over its adjacency in the order of the key-major list (entry x = 2 e + dir, dir = 1 where the view is j_e),
 *        B_e y:  g = (1 - mu) * fma(d[0], y[0], fma(d[1], y[1], d[2] * y[2])),  z[a] = w * fma(-g, d[a], y[a]),  y = u_v - u_o,
 *        the diagonal block D[a][b] += w * fma(-(1 - mu), d[a] * d[b], a == b), the right-hand side b[a] += sg * (((w * mu) * l) * d[a]),
 *      and the inverse of D by its cofactors over the determinant.  How the system is solved is not part of the rule: the
 *      library runs conjugate gradients preconditioned by those inverses, from the standing positions, until
 *      |r|^2 <= cg_tol^2 |b|^2 (looked at before the first iteration too) or for cg_max iterations; then
 *      SFM_TRANSAVG_CG_LIMIT is set and the result is taken as it is.  Every dot product is formed per slice of 64 views
 *      and the slices are added in slice order.
 *   4. Rounds.  Round 0 solves with w_e = 1 on the used edges and l_e = 1.  Then `rounds` times weights and lengths are
 *      reset from the standing positions and the system is solved again: s2 = 2 - 2 * (dv / sqrt(n2)), the squared chord of
 *      the residual angle (s2 = 2 where n2 is zero or not finite); w_e = 1 / (1 + s2 / sigma2), sigma2 = 2 - 2 * cos_max, a
 *      Cauchy weight at the admitted angle; l_e = dv where dv > 0, else 1.  After the last solve every used edge is judged
 *      by step 2; that set and its count stand.
 *   5. Polish.  If `polish`, one more solve with w_e = 1 on the inliers, 0 elsewhere, and l_e = dv of the standing model.  It
 *      stands iff every free position is finite and its inlier count over all used edges is at least the standing count;
 *      otherwise the standing model is kept and SFM_TRANSAVG_KEPT_ROUNDS is set.  The decision is taken on the device.
 *   6. Status SFM_TRANSAVG_NO_MODEL: `root` has no rotation, `root` has no used edge, or a free position is not finite after
 *      round 0; then C_out is all zeros, every verdict is 0, every view is held and the log is all zeros.  Outputs, all
 *      optional but C_out.  C_out[V][3]: zeros for a view without a position (not reached from `root` over used edges).
 *      edge_inlier[E].  edge_cos[E]: dv / sqrt(n2), NaN where n2 is zero or not finite or the edge is not used.  edge_len[E]:
 *      dv of the final model, the baseline in the solution's unit (the caller scales a pair's own reconstruction with it);
 *      NaN where the edge is not used.  view_status[V]: SFM_TRANSAVG_NO_ROTATION | SFM_TRANSAVG_UNREACHED (no path from `root`
 *      over used edges) | SFM_TRANSAVG_HELD (not joined to `root` through the final inliers).  n_inliers, status.
 *      summary[6]: views with a position | without a rotation | unreached | held | inlier edges | used outlier edges.
 *      log[rounds + 2][4] doubles, a row per solve (row rounds + 1 is the polish, zeros without one): its inlier count, its
 *      CG iterations, whether it stood (1 for a round), and its cost sum_e w_e ((n2 - dv * dv) + mu (dv - l_e)^2) under the
 *      weights of that solve, summed per slice of 64 edges in slice order.
 *   7. Argument errors (SFM_E_SHAPE, found before a device is looked for, nothing launched, outputs untouched): V < 2, E < 1,
 *      E >= 2^30, an index out of range, i == j, root out of range, cos_max NaN or outside (0, 1], mu NaN or outside [0, 1],
 *      rounds < 0, polish not 0 or 1, cg_tol not in (0, 1), cg_max < 1, a null required array.  A non-zero R_v that fails
 *      verify_rotation: SFM_E_BAD_ROTATION, sfm_last_error naming the lowest such view (the _dev form finds it with one
 *      kernel, before anything else is launched).
 * No floating-point atomic, integer counts, slice-ordered sums: the bits depend on the graph and the options only.  The host
 * reads nothing between the launches of a call.  One graph per call.  With cos_max = 1 and rounds > 0 sigma2 is zero and the
 * weights are 0 or NaN: no edge takes part in the later rounds and the positions of round 0 stay.  The _dev form takes d_R,
 * d_t, d_edge_mask and every output on the device and a stream (NULL = the library stream); `edges` stays a HOST array.  It
 * returns when the work is done. */
#define SFM_TRANSAVG_NO_MODEL     1   /* status: root has no rotation or no used edge, or round 0 gave no finite positions */
#define SFM_TRANSAVG_KEPT_ROUNDS  2   /* status: the polish did not stand: the model is that of the rounds */
#define SFM_TRANSAVG_CG_LIMIT     4   /* status: a solve ended its CG at cg_max */
#define SFM_TRANSAVG_NO_ROTATION  1   /* view_status: R_v is nine zeros */
#define SFM_TRANSAVG_UNREACHED    2   /* view_status: no path from root over used edges */
#define SFM_TRANSAVG_HELD         4   /* view_status: not joined to root through the final inlier edges */
int sfm_translation_average(int V, int64_t E, const int* edges /*[E][2]*/, const double* R /*[V][9]*/, const double* t /*[E][3]*/,
                            const unsigned char* edge_mask /*[E] or NULL*/, int root, double cos_max, double mu, int rounds,
                            int polish, double cg_tol, int cg_max, double* C_out /*[V][3]*/, unsigned char* edge_inlier /*[E] or NULL*/,
                            double* edge_cos /*[E] or NULL*/, double* edge_len /*[E] or NULL*/, int* view_status /*[V] or NULL*/,
                            int* n_inliers, int* status, int64_t* summary /*[6]*/, double* log /*[rounds + 2][4]*/);
int sfm_translation_average_dev(int V, int64_t E, const int* edges /*host [E][2]*/, const double* d_R, const double* d_t,
                                const unsigned char* d_edge_mask, int root, double cos_max, double mu, int rounds, int polish,
                                double cg_tol, int cg_max, double* d_C_out, unsigned char* d_edge_inlier, double* d_edge_cos,
                                double* d_edge_len, int* d_view_status, int* d_n_inliers, int* d_status, int64_t* d_summary,
                                double* d_log, void* hip_stream);
/* Step 2 on the host, by the function the kernels run: 1 for an inlier; *dv_out and *n2_out (may be NULL) its terms. */
int sfm_translation_edge_test(const double d[3], const double ci[3], const double cj[3], double cos_max, double* dv_out,
                              double* n2_out);

/* ---- track linking: multi-view tracks from verified pairwise matches ---------------------------------------------------
 * V views; key_ptr[V + 1] (host) gives key k of view v the global id g = key_ptr[v] + k, K = key_ptr[V] < 2^31.  P pairs:
 * pair_views[P][2] (host) and pair_ptr[P + 1] (host, int64); the matches of pair p are a[m], b[m] for pair_ptr[p] <= m <
 * pair_ptr[p + 1], a[m] a key of the pair's first view and b[m] a key of its second; M = pair_ptr[P].  mask[M] optional
 * bytes.  min_len >= 2.  The rule:
 *   1. A match is USED iff mask is NULL or its byte is non-zero.  Duplicate matches, a pair listed twice and a pair listed
 *      as (i, j) and as (j, i) are all legal.
 *   2. label[g] is the smallest global id in the connected component of g under the used matches.  The definition does
 *      not depend on the order of matches, pairs, launches or timing: any algorithm that reaches it gives the same bits.
 *   3. Per component: `size` is its number of keys.  It is in CONFLICT iff two of its keys belong to one view; size > V is
 *      a conflict by counting alone.  A component of one key is UNMATCHED.  Otherwise CONFLICT takes precedence over SHORT
 *      (size < min_len), and everything else is KEPT.
 *   4. Kept components are numbered 0 .. n_tracks - 1 by ascending label.  key_track[K]: the track number, or
 *      SFM_LINK_UNMATCHED, SFM_LINK_SHORT, SFM_LINK_CONFLICT.  pt_ptr[n_tracks + 1].  cam_idx[] and key_idx[] hold a
 *      track's members by ascending global id, which is ascending view: the order sfm_tri_tracks and sfm_ba_create take;
 *      key_idx is the key's index inside its view.
 *   5. summary[8] (int64): used matches | components of at least two keys | kept components | conflicting components |
 *      short components | observations (pt_ptr[n_tracks]) | the longest kept track | the largest component.
 *   6. Optional output label_out[K].
 * Every output may be NULL.  The caller's buffers are sized from K: pt_ptr holds K / 2 + 2 entries, cam_idx and key_idx
 * hold K; only pt_ptr[0 .. n_tracks] and the first pt_ptr[n_tracks] entries of cam_idx and key_idx are written.  There is
 * no two-call protocol.
 * Refusals (SFM_E_SHAPE, sfm_last_error names the item, found before a device is looked for, every output untouched):
 * key_ptr not starting at 0 or decreasing; a pair with a view out of range or with both views equal; pair_ptr not
 * starting at 0 or decreasing; min_len < 2; a bad `group` or `scan`; and a key index out of its view's range, in a used
 * match or a masked one alike -- the host form finds the lowest such match on the host, the _dev form by one verify kernel
 * (atomicMin) whose word is read once before anything else is launched.
 * How: a lock-free union-find (the root with the larger id is hooked under the root with the smaller one by
 * compare-and-swap, so a component's root is its minimum), integer counts, prefix sums over the roots in id order, a
 * scatter, then a group of `group` lanes per component (0 = automatic; 1, 4 .. 64) that ranks the members by id and finds
 * a conflict as two neighbouring members of one view, a second prefix sum over the kept flags and a gather.  Only integer
 * atomics whose result does not depend on their order; no workgroup waits for another one.  `scan` picks the prefix-sum
 * route: 0 automatic, 1 one workgroup, 2 device-wide (three launches); the bits do not depend on it or on `group`.
 * sfm_link_tracks takes host arrays and blocks.  sfm_link_tracks_dev takes a, b, mask and every output on the device and a
 * stream (NULL = the library stream); key_ptr, pair_views and pair_ptr stay HOST arrays.  The host reads the verify word,
 * then the two counts *n_tracks and *n_obs (host, may be NULL) at the end, and nothing else; it returns when the work is
 * done. */
#define SFM_LINK_UNMATCHED  -1
#define SFM_LINK_SHORT      -2
#define SFM_LINK_CONFLICT   -3
int sfm_link_tracks(int V, const int* key_ptr /*[V + 1]*/, int P, const int* pair_views /*[P][2]*/, const int64_t* pair_ptr /*[P + 1]*/,
                   const int* a /*[M]*/, const int* b /*[M]*/, const unsigned char* mask /*[M] or NULL*/, int min_len, int group,
                   int scan, int* key_track /*[K]*/, int* pt_ptr /*[K / 2 + 2]*/, int* cam_idx /*[K]*/, int* key_idx /*[K]*/,
                   int64_t* summary /*[8]*/, int* label_out /*[K]*/);
int sfm_link_tracks_dev(int V, const int* key_ptr /*host*/, int P, const int* pair_views /*host*/, const int64_t* pair_ptr /*host*/,
                       const int* d_a, const int* d_b, const unsigned char* d_mask, int min_len, int group, int scan,
                       int* d_key_track, int* d_pt_ptr, int* d_cam_idx, int* d_key_idx, int64_t* d_summary, int* d_label_out,
                       int* n_tracks /*host*/, int64_t* n_obs /*host*/, void* hip_stream);
/* The launch plan, host only: plan[8] = grid of the union (and verify) kernel | lane-group width | grid of the ordering
 * kernel | grid of the pass over components beyond 64 members | prefix-sum route over the K keys (1 one workgroup, 2
 * device-wide) | its tiles | route over the K / 2 components | its tiles.  Grids follow sfm_set_cu_limit. */
int sfm_link_tracks_plan(int V, int64_t K, int64_t M, int group, int scan, int* plan /*[8]*/);

/* ---- view triplets: the cycle-consistency filter of a view graph -------------------------------------------------------
 * The graph is that of the rotation averaging: V views, E edges (i_e, j_e, Rel_e[9]), i_e != j_e, parallel edges allowed,
 * R_j = Rel_e R_i, row-major.  Around every triangle of the graph the three relative rotations must compose to the
 * identity; a wrong edge breaks every triangle it lies in.  edge_mask[E] optional bytes (0 excludes an edge; NULL: none is
 * excluded).  The rule:
 *   1. Oriented edge.  For edge e with ends lo < hi: M_e (frame lo -> frame hi) is Rel_e if i_e = lo, otherwise its
 *      transpose: a copy of entries, exact.
 *   2. Triplet.  Three edges (e_ab, e_bc, e_ac) over three distinct views a < b < c, e_ab joining a and b and so on.  Every
 *      combination of parallel edges is a triplet of its own: two parallel edges on each side give eight.  A masked edge is
 *      in no triplet.
 *   3. The test is rotation_edge_inlier(Ri = M_ab, Rj = M_ac, Rel = M_bc, thr) of csrc/sfm_obs_test.h, unchanged (step 1 of
 *      the rotation averaging): P = M_bc M_ab in that function's fma order, lhs = trace(M_ac^T P) in its order.  The triplet
 *      is CONSISTENT iff lhs is finite and lhs >= fma(2, cos_loop, 1); cos_loop, in (0, 1], is the cosine of the largest
 *      admitted loop angle.  A triplet's bits depend on the triplet alone, whichever edge or lane finds it.
 *      sfm_view_triplet_test is the host entry.
 *   4. Per-edge counts (int64): n_tri[e] the number of triplets that hold e, n_ok[e] the consistent ones among them.
 *   5. Verdict edge_keep[e], all in integers: a masked edge gets 0; an edge with n_tri = 0 is UNTESTED and gets
 *      keep_untested (0 or 1); otherwise 1 iff n_ok >= min_ok (min_ok >= 1; 0 means 1) and 100 * n_ok >= min_pct * n_tri
 *      (min_pct in 0 .. 100; 64-bit products).
 *   6. Outputs, all optional.  edge_keep[E] (bytes), n_tri[E], n_ok[E].  kept_idx[E] (int32) with *n_kept (host): the
 *      ascending edge numbers with edge_keep = 1, by a prefix sum -- what the caller compacts `edges` and `rel` with; only
 *      its first *n_kept entries are written.  summary[8] (int64): triplets | consistent triplets | edges tested | kept |
 *      dropped though tested | untested | masked | the largest n_tri.
 *   7. Argument errors (SFM_E_SHAPE, found before a device is looked for, nothing launched, outputs untouched): V < 3, E < 1,
 *      E >= 2^30 (the 2 E edge ends are numbered by an int), an index out of range, i == j, cos_loop NaN or outside (0, 1],
 *      min_ok < 0, min_pct outside 0 .. 100, keep_untested not 0 or 1, a bad `group`, a null `edges` or `rel`.  Each Rel_e
 *      must pass verify_rotation: SFM_E_BAD_ROTATION, sfm_last_error naming the lowest such edge (the _dev form finds it
 *      with one kernel, before anything else is launched).
 * The definition does not depend on the order of edges, lanes, launches or timing: any enumeration that reaches it gives
 * the same bits.  How: the view-major adjacency sorted by (view, neighbour, edge) -- two stable passes of the key-major list,
 * the other end first -- then a group of `group` lanes per edge (0 = automatic; 1, 4 .. 64) that strides over the shorter
 * adjacency of the edge's ends and looks every neighbour up in the longer one by binary search.  Every edge enumerates all
 * its triplets, so a triplet is tested three times, always in the order of step 3, and there is no atomic on the way to
 * n_tri and n_ok; the summary uses 64-bit integer atomics.  No floating-point sum at all: the bits do not depend on `group`.
 * sfm_view_triplets takes host arrays and blocks.  sfm_view_triplets_dev takes d_rel, d_edge_mask and every output array on
 * the device and a stream (NULL = the library stream); `edges` stays a HOST array, as in the two averaging calls.  The host
 * reads the verify word and *n_kept (host, may be NULL) and nothing else; it returns when the work is done. */
int sfm_view_triplets(int V, int64_t E, const int* edges /*[E][2]*/, const double* rel /*[E][9]*/,
                      const unsigned char* edge_mask /*[E] or NULL*/, double cos_loop, int min_ok, int min_pct, int keep_untested,
                      int group, unsigned char* edge_keep /*[E]*/, int64_t* n_tri /*[E]*/, int64_t* n_ok /*[E]*/,
                      int* kept_idx /*[E]*/, int64_t* summary /*[8]*/, int* n_kept);
int sfm_view_triplets_dev(int V, int64_t E, const int* edges /*host [E][2]*/, const double* d_rel, const unsigned char* d_edge_mask,
                          double cos_loop, int min_ok, int min_pct, int keep_untested, int group, unsigned char* d_edge_keep,
                          int64_t* d_n_tri, int64_t* d_n_ok, int* d_kept_idx, int64_t* d_summary, int* n_kept /*host*/,
                          void* hip_stream);
/* Step 3 on the host, by the function the kernels run: 1 for a consistent triplet, *lhs_out (may be NULL) the trace. */
int sfm_view_triplet_test(const double Mab[9], const double Mbc[9], const double Mac[9], double cos_loop, double* lhs_out);

/* ---- view pairs: which pairs of views to match, from one short descriptor per view -------------------------------------
 * A vocabulary of K words is trained from the resident descriptor sets, every view is summarised by one VLAD descriptor
 * (per word the power-normalised sum of the residuals of its keys), all views are compared through these descriptors and
 * each view keeps its k best partners.  The whole rule is stated in integers, except the score, which is three correctly
 * rounded fp64 operations: every output is a function of the input alone.
 * Sets: every set of a call is an exact L2 set (SFM_DESC_INFO_EXACT = 1) of one dimension D <= 256; anything else is
 * SFM_E_SHAPE with nothing launched.  s(x, c) = sum (x[d] - c[d])^2, an exact integer.  mix = the splitmix64 finaliser of
 * the robust estimators' samplers (block "robust two-view geometry").  Limits: 1 <= K <= 1024, K D <= 131 072, a view has
 * at most 2^22 keys, V <= 65 536, 1 <= k <= 64; the keys of a describe call number fewer than 2^31.
 *   1. Vocabulary, sfm_vocab_train.  The rows of the n_sets sets are numbered by concatenation in set order, N in all.
 *      train_cap = 0 stands for 2^20, its maximum is 2^22.  The training rows are all rows when N <= train_cap, otherwise
 *      rows floor(j N / train_cap), j = 0 .. train_cap - 1; T is their number; T < K is SFM_E_SHAPE.
 *      Start: word w is training row lo_w + mix(seed K + w) mod (hi_w - lo_w), lo_w = floor(w T / K), hi_w =
 *      floor((w + 1) T / K), seed K + w taken mod 2^64.  sfm_vocab_init_rows returns, on any machine, the K rows of the
 *      CONCATENATION these are (the training row mapped through floor(j N / train_cap) where N > train_cap).
 *      A round: a(j) = argmin_w (s(x_j, c_w), w) -- a tie goes to the lower word; n_w the number of rows of word w and
 *      S_w[d] = sum x_j[d] (below 2^31 by the cap); c_w[d] = floor((2 S_w[d] + n_w) / (2 n_w)), the mean rounded half up,
 *      where n_w > 0; a word without a row keeps its bytes.  `iters` rounds are run unconditionally, 0 <= iters <= 64;
 *      iters = 0 returns the start.  words_out[K][D] uint8 (host).
 *      log (host, int64 [iters + 1][3], may be NULL): per round, under the words the round started with: the inertia
 *      sum_j s(x_j, c_a(j)) | the number of words without a row | the number of words whose bytes the round changed; the
 *      last row is the same under the final words, with 0 changed.
 *   2. View descriptors, sfm_view_describe(vocab, n_views, views, ...): vocab is a set of K rows (sfm_desc_create of
 *      words_out, or a vocabulary from elsewhere).  Per view: a(i) as above; r[w][d] = sum over a(i) = w of
 *      (x_i[d] - c_w[d]), int32; q[w][d] = sgn(r) min(isqrt(|r|), 127), int8, isqrt the exact floor square root;
 *      norm2 = sum q^2 (below 2^31).  Outputs, all optional, the non-NULL ones select the work: desc int8 [V][K D],
 *      word-major; norm2 int64 [V]; word_count int32 [V][K]; assign int32 per key, the views concatenated; residual int32
 *      [V][K D].  An empty view gives zeros.
 *   3. Pairs, sfm_view_pairs(V, len, desc int8 [V][len], norm2 int64 [V], k, min_score, mutual, sequential, ...), len <=
 *      131 072, every |desc| <= 127 (so that the dot products stay in int32: 127^2 * 131 072 < 2^31).
 *      dot(a, b) = sum desc_a desc_b, exact.  score(a, b) = (double)dot / sqrt((double)norm2_a * (double)norm2_b): a
 *      product, a square root and a division, each correctly rounded, never contracted.  sfm_view_score is that function
 *      on the host and returns the kernel's bits.
 *      b is a CANDIDATE of a iff b != a, norm2_a > 0, norm2_b > 0 and score >= min_score (NaN min_score: SFM_E_SHAPE).
 *      The NEIGHBOURS of a are its first k candidates by (score descending, b ascending): nbr[V][k] int32 and
 *      nbr_score[V][k] double; missing entries are -1 and -inf.
 *      The pair a < b is LISTED iff (mutual = 0: b is a neighbour of a or a is a neighbour of b; mutual = 1: both) or
 *      b - a <= sequential (sequential >= 0, 0 = none: the consecutive frames of a sequence, whatever their descriptors).
 *      pairs[cap][2] int32, sorted lexicographically, and *n_pairs, the true count: only the first min(*n_pairs, cap)
 *      rows of pairs, how and pair_score are written.  how int32 per pair: 1 (a lists b) | 2 (b lists a) | 4
 *      (sequential).  pair_score double per pair: the score, -inf where a norm is zero.  dot int32 [V][V], optional.
 *      The rule names no order of evaluation: permuting the views permutes the result.
 *   4. Argument errors (SFM_E_SHAPE before a device is looked for, outputs untouched): a NULL or non-exact or Hamming set,
 *      mixed D, K or K D or V or k or iters or train_cap outside the limits, T < K, NaN min_score, mutual not 0 or 1,
 *      sequential < 0, cap < 0, len outside 1 .. 131 072, a NULL desc or norm2, how or pair_score without pairs
 *      where cap > 0.
 * How.  Assignment (training and describing): tiles of 128 rows against all K words by v_mfma_f32_16x16x32_bf16 on the sets'
 * resident bf16 rows and integer norms (exact: block "descriptor matching"), a lane's running best by one unsigned compare
 * of (s << 32 | w).  Accumulation: int32 sums of x per (word, dimension) and the word counts, per workgroup in LDS where
 * (K D + K) 4 bytes fit, by global int32 atomics otherwise -- integer addition is associative, the route does not show;
 * r = S - n c.  Scores: the V x V dot products by v_mfma_i32_16x16x64_i8 in strips of rows (a bounded work buffer, or
 * `dot` itself when it is asked for), a wave per view selects its neighbours with (score key, index) compares; the
 * reverse lists by the key-major list; a count per view, the shared prefix sum, a fill, and one wave per listed pair for
 * pair_score.  No floating-point atomic and no floating-point sum anywhere: the bits do not depend on the device, the
 * compute-unit limit or timing.
 * The host forms take host arrays (the sets are handles) and block; the _dev forms take device arrays and a stream (NULL
 * = the library stream); *n_pairs is a host integer. */
int sfm_vocab_train(int n_sets, sfm_desc_set* const* sets, int K, int iters, uint64_t seed, int64_t train_cap,
                    uint8_t* words_out /*[K][D]*/, int64_t* log /*[iters + 1][3] or NULL*/);
int sfm_vocab_init_rows(int64_t N, int K, uint64_t seed, int64_t train_cap, int64_t* rows_out /*[K]*/);
int sfm_view_describe(sfm_desc_set* vocab, int n_views, sfm_desc_set* const* views, int8_t* desc, int64_t* norm2, int* word_count,
                      int* assign, int* residual);
int sfm_view_describe_dev(sfm_desc_set* vocab, int n_views, sfm_desc_set* const* views, int8_t* d_desc, int64_t* d_norm2,
                          int* d_word_count, int* d_assign, int* d_residual, void* hip_stream);
int sfm_view_pairs(int V, int len, const int8_t* desc, const int64_t* norm2, int k, double min_score, int mutual, int sequential,
                   int64_t cap, int* nbr /*[V][k]*/, double* nbr_score /*[V][k]*/, int* pairs /*[cap][2]*/, int* how /*[cap]*/,
                   double* pair_score /*[cap]*/, int* dot /*[V][V]*/, int64_t* n_pairs);
int sfm_view_pairs_dev(int V, int len, const int8_t* d_desc, const int64_t* d_norm2, int k, double min_score, int mutual,
                       int sequential, int64_t cap, int* d_nbr, double* d_nbr_score, int* d_pairs, int* d_how, double* d_pair_score,
                       int* d_dot, int64_t* n_pairs /*host*/, void* hip_stream);
/* The score of step 3 on the host, by the function the kernels run.  SFM_E_SHAPE for a NULL score_out. */
int sfm_view_score(int dot, int64_t norm2_a, int64_t norm2_b, double* score_out);
/* The resident scene moved by X' = s A X + t, on the device: every point by the formula, every camera block [C, q] to
 * C' = s A C + t and q' = q(A R(q)), the library's canonical quaternion of the product (qw >= 0, not renormalised).
 * Refused before any launch: s not finite or not positive (SFM_E_SHAPE), A failing verify_rotation
 * (SFM_E_BAD_ROTATION), a communicator attached.  The new cameras go to a work buffer first; if q(A R(q)) of any camera
 * fails (a half turn: |qw| < 1e-6) the call fails with that camera's status and the lowest such camera named, and the
 * scene is left bit for bit as it was.  Reprojection residuals are invariant, R'^T (X' - C') = s R^T (X - C): the cost and
 * every inlier decision of the scene are those of before.  Not invariant: the damping lambda I of an iteration (a step of
 * the moved scene is not the moved step unless s = 1 and lambda = 0 up to rounding) and every covariance in world units
 * (sfm_ba_covariance), which scales with s^2 and turns with A.  Afterwards the state is treated as after sfm_ba_set_state. */
int sfm_ba_transform(sfm_ba_problem* p, double s, const double A[9], const double t[3]);
/* The resident scene aligned to targets: the resident points point_idx[0 .. n) are gathered on the device as src, target is
 * uploaded as dst, and sfm_similarity_ransac_dev runs on them as one set on the problem's stream (options as above).  With
 * apply != 0 and a model the scene is then moved by it as sfm_ba_transform moves it, the model read from device memory:
 * nothing comes down between the two.  Then the outputs are downloaded: sim_out[13], inlier[n], n_inliers, best_hyp,
 * status (any of the last four may be NULL).  A point_idx outside 0 .. N - 1: SFM_E_SHAPE.  n = 0, too few correspondences
 * or no model are not errors: `status` says so and the scene is untouched.  A camera at a half turn fails the call as it
 * fails sfm_ba_transform, the scene untouched and the outputs written. */
int sfm_ba_align(sfm_ba_problem* p, int n, const int* point_idx /*host [n]*/, const double* target /*host [3][n]*/,
                 double max_err2, int max_hyp, int iters, int flags, int apply, double* sim_out /*[13]*/,
                 unsigned char* inlier /*[n] or NULL*/, int* n_inliers, int* best_hyp, int* status);

/* ---- SIFT detection: ViewProcessor.__extract_keys (view_processor.py:151-164, 199-202) --------------------------
 * cv.SIFT_create().detectAndCompute(img, None) by the contract of INTEGRATION.md 'SIFT detection' (firstOctave -1,
 * nfeatures 0, no mask): keypoints sorted by (x, y asc; size desc; angle asc; response desc; octave desc) without
 * duplicates, their cv2 fields after the firstOctave fixup, and (n, 128) float32 descriptors with integer values in
 * [0, 255].  img is (height, width) gray or (height, width, 3) BGR uint8 with rows row_stride_bytes apart.  A bad
 * shape, channel count or parameter returns SFM_E_SHAPE; an image whose octave count is <= 0 gives zero keypoints.
 * The call is blocking; it enqueues on params->stream (NULL = the library stream). */
typedef struct sfm_sift_params {
  int n_octave_layers;        /* nOctaveLayers, 3; 1 .. 16 */
  double contrast_threshold;  /* contrastThreshold, 0.04 */
  double edge_threshold;      /* edgeThreshold, 10 */
  double sigma;               /* sigma, 1.6 */
  int keep_pyramid;           /* 1: keep the Gaussian and DoG levels on the device for sfm_sift_result_copy_level */
  void* stream;               /* hipStream_t or NULL */
} sfm_sift_params;
#define SFM_SIFT_INFO_N             1   /* final keypoints */
#define SFM_SIFT_INFO_N_OCTAVES     2
#define SFM_SIFT_INFO_N_PRE         3   /* refined keypoints before orientation */
#define SFM_SIFT_INFO_N_LAYERS      4
#define SFM_SIFT_INFO_KEEPS_PYRAMID 5
#define SFM_SIFT_LEVEL_GAUSS        0   /* levels 0 .. L + 2 of an octave */
#define SFM_SIFT_LEVEL_DOG          1   /* levels 0 .. L + 1 of an octave */
typedef struct sfm_sift_result sfm_sift_result;
/* params NULL = the defaults above. */
int sfm_sift_detect(const uint8_t* img, int height, int width, int channels, int64_t row_stride_bytes,
                    const sfm_sift_params* params, sfm_sift_result** out);
int sfm_sift_result_info(const sfm_sift_result* r, int what, int64_t* value);
/* height and width of every level of pyramid octave `octave` (0 = the x2 base image). */
int sfm_sift_result_level_shape(const sfm_sift_result* r, int octave, int* height, int* width);
/* Caller-allocated [n] outputs (descriptors [n][128]); any may be NULL. */
int sfm_sift_result_copy(const sfm_sift_result* r, float* x, float* y, float* size, float* angle, float* response,
                         int32_t* octave, float* descriptors);
/* Debug: the refined keypoints before orientation ([n_pre], pyramid coordinates, packed octave before the fixup), in
 * the order (x, y asc; size desc; response desc; octave desc). */
int sfm_sift_result_copy_pre(const sfm_sift_result* r, float* x, float* y, float* size, float* response, int32_t* octave);
/* Debug: one Gaussian or DoG level ([height][width] of its octave); needs keep_pyramid. */
int sfm_sift_result_copy_level(const sfm_sift_result* r, int kind, int octave, int level, float* out);
int sfm_sift_result_destroy(sfm_sift_result* r);
/* The float32 blur weights the library uses for a Gaussian of this sigma (ksize = rint(8 sigma + 1) | 1 taps; at
 * most `capacity` are written; weights may be NULL to ask for ksize). */
int sfm_sift_blur_kernel(double sigma, int capacity, float* weights, int* ksize);

/* ---- device-resident key tracks: KeyTrack / KeyTracker (key_tracker.py:14-59, 132-181, 213-317) --------------------
 * One store per KeyTracker.  Per view it holds, on the device: the key count n, the key coordinates as doubles
 * (KeyPoint.pt: float32 values widened exactly) and the view's KeyTrack.table as int32 rows of n entries, -1 = invalid
 * match / not used.  Rows are allocated with spare capacity, so adding a view appends a row to every table without
 * copying it.  A table has its own row count: sfm_track_add_view gives every existing table one more row and the new
 * table (number of views) rows, as key_tracker.py:236-240 does; sfm_track_drop_last_view takes the last view away again
 * and leaves the other tables' rows as they are (the state the reference is in when __extend_list raises).
 * Host forms block and copy; _dev forms take DEVICE pointers and a stream (NULL = the library stream) and enqueue.
 * The store remembers the stream of its last enqueue: a blocking form waits for that stream (not for the device), and
 * an enqueue on a different stream first waits for the one before it. */
#define SFM_TRACK_INFO_N_VIEWS        1
#define SFM_TRACK_INFO_N_KEYS         2   /* of `view` */
#define SFM_TRACK_INFO_N_ROWS         3   /* of `view`'s table */
#define SFM_TRACK_INFO_UPLOAD_BYTES   4   /* host -> device bytes so far (coordinates, usage lists) */
#define SFM_TRACK_INFO_DOWNLOAD_BYTES 5   /* device -> host bytes so far */
#define SFM_TRACK_INFO_OBS_VIEWS      6   /* views of the last sfm_obs_build, -1 if there is no list */
#define SFM_TRACK_INFO_OBS_PTS        7   /* its points */
#define SFM_TRACK_INFO_N_OBS          8   /* its observations */
#define SFM_TRACK_OK          0   /* per-reference status of an extend */
#define SFM_TRACK_NO_SECOND   1   /* knn: a query without a second neighbour (the reference's IndexError, quirk Q16) */
#define SFM_TRACK_ZERO_SECOND 2   /* knn: a second distance of 0 (the reference's ZeroDivisionError, quirk Q16) */
#define SFM_TRACK_BAD_TRAIN   3   /* a kept train index outside the reference view's keys (never from sfm_match_dev) */
typedef struct sfm_track_store sfm_track_store;
int sfm_track_create(sfm_track_store** out);
int sfm_track_destroy(sfm_track_store* s);
/* `view` is ignored for the store-wide items. */
int sfm_track_info(const sfm_track_store* s, int what, int view, int64_t* value);
/* Add a view of n keys at (x[i], y[i]) (host arrays; n = 0 is legal): *view_out = its index. */
int sfm_track_add_view(sfm_track_store* s, int n, const double* x, const double* y, int* view_out);
int sfm_track_drop_last_view(sfm_track_store* s);
/* key_tracker.py:247-291 for view `new_view` against the views 0 .. n_refs-1, from the [n_refs][n_query] arrays
 * sfm_match_dev wrote (n_query = the new view's key count; arrays a mode does not read may be NULL):
 *   filter : knn -- (double)d0 / (double)d1 < 0.7 in correctly rounded fp64; mutual -- the mutual flag; 1-NN -- all;
 *            the survivors compacted in query order;
 *   dedup  : quirk Q14 -- one entry per distinct train index t, ordered by the rank of t's first appearance; the entry
 *            is the last later match i of t with dist[i] < dist_filtered[rank(t)], or t's first appearance.
 * Nothing is raised on the device: a reference view whose knn result has a query without a second neighbour or with a
 * zero second distance gets that status and its first offending query (the first query that hits either), and an empty
 * kept list.  The kept lists stay in the store until the next call. */
int sfm_track_match_dedup_dev(sfm_track_store* s, int new_view, int n_refs, int mode, const int* d_best_idx,
                              const float* d_best_dist, const int* d_second_idx, const float* d_second_dist,
                              const uint8_t* d_mutual, void* hip_stream);
/* The same followed by the writes of key_tracker.py:305-314, table[ref][new_view, t] = q and table[new_view][ref, q] = t
 * over each kept list, in one call with nothing downloaded in between; a reference view writes only if its status and
 * that of every reference view before it is SFM_TRACK_OK (the reference would have raised before reaching it). */
int sfm_track_extend_dev(sfm_track_store* s, int new_view, int n_refs, int mode, const int* d_best_idx,
                         const float* d_best_dist, const int* d_second_idx, const float* d_second_dist,
                         const uint8_t* d_mutual, void* hip_stream);
/* sfm_match_dev of `query` (the new view's descriptors, one row per key) against refs[0 .. n_refs-1] (the descriptors of
 * the views 0 .. n_refs-1) into buffers the store owns, then sfm_track_extend_dev (write != 0) or
 * sfm_track_match_dedup_dev (write == 0) on them: no neighbour array visits the host. */
int sfm_track_match_views(sfm_track_store* s, int new_view, sfm_desc_set* query, int n_refs, sfm_desc_set* const* refs,
                          int mode, int write, void* hip_stream);
/* Blocking: per reference view of the last match_dedup / extend the status, the first offending query (-1 if none)
 * and the length of the kept list.  Any output may be NULL. */
int sfm_track_extend_status(sfm_track_store* s, int n_refs, int* status, int* first_bad, int* n_kept);
/* Blocking: the kept (query, train) list of reference view `ref`; q and t hold n_kept entries. */
int sfm_track_kept_copy(sfm_track_store* s, int ref, int* q, int* t);
/* The writes for reference view `ref` over the first n entries of its kept list (quirk Q15: the number of
 * fundamental-matrix inliers; n < 0 or n > n_kept: the whole list).  Enqueues. */
int sfm_track_write_kept(sfm_track_store* s, int ref, int n, void* hip_stream);
/* KeyTracker.generate_matched_pairs (key_tracker.py:161-181): the entries > 0 of table[ref][que, :] in ascending key
 * order (key 0 of the query view is never paired: quirk Q3).  Outputs, packed for the count n found:
 * r_idx[n], q_idx[n], ref_pts (3, n) and que_pts (3, n) row-major doubles with row 2 = 1.0.  Every buffer must hold
 * the reference view's key count (3 x for the points).  d_count[0] = n; d_count[1] != 0 if an entry named no key of
 * the query view (its coordinates are then NaN; the host form returns SFM_E_SHAPE). */
int sfm_track_pairs_dev(sfm_track_store* s, int ref, int que, int* d_count, int* d_r_idx, int* d_q_idx,
                        double* d_ref_pts, double* d_que_pts, void* hip_stream);
int sfm_track_pairs(sfm_track_store* s, int ref, int que, int* n, int* r_idx, int* q_idx, double* ref_pts,
                    double* que_pts);
/* The pairs of a track store's table[ref][que] (sfm_track_pairs_dev, into buffers of the pool) verified by
 * sfm_twoview_ransac_dev as one set on the library's stream: *n pairs, r_idx[n], q_idx[n], inlier[n] (HOST arrays that hold
 * the reference view's key count, or NULL), F_out[9], best_hyp and status of the set.  Only the count comes down between
 * the two steps; the coordinates stay on the device. */
int sfm_twoview_verify_pairs(sfm_track_store* s, int ref, int que, double max_err2, int max_hyp, int iters, int* n, int* r_idx,
                           int* q_idx, unsigned char* inlier, double F_out[9], int* best_hyp, int* status);
/* processors.pose_pairs (a track store; not part of the KeyTrack interface): the pairs of table[ref][que] gathered on the
 * device (the reference key LEFT, the query key RIGHT) and posed as one set.  Only the model and the intrinsics go up (and the
 * optional mask `inlier` over the pairs in their order, a byte each, of which the first *n are read; the caller knows *n
 * from the verification that produced the mask), only the count of pairs comes down between the two steps.  r_idx,
 * q_idx and obs_front are host arrays of cap entries (cap = the keys of view ref), X_out of 3 cap, filled as [3][*n]. */
int sfm_twoview_pose_pairs(sfm_track_store* s, int ref, int que, const unsigned char* inlier /*host [*n] or NULL*/,
                           const double model[9], int kind, const double K_left[9], const double K_right[9], double cos2_min,
                           int min_parallax, int* n, int* r_idx, int* q_idx, double R_out[9], double t_out[3], double n_out[3],
                           int* cand_front, int* n_front, int* n_parallax, int* best_cand, int* status,
                           unsigned char* obs_front, double* X_out);
/* TrackStore.refine_pairs: the same pairs gathered on the device and their pose (R_in, t_in) refined as one set by
 * sfm_twoview_refine's rule.  Nothing goes up but the pose, the intrinsics and the optional mask `inlier` (of which the
 * first *n bytes are read), only the count of pairs comes down between the two steps.  r_idx, q_idx, obs_res, obs_inlier and
 * obs_front are host arrays of cap entries (cap = the keys of view ref), X_out of 3 cap, filled as [3][*n]; every output
 * but n, R_out and t_out may be NULL. */
int sfm_twoview_refine_pairs(sfm_track_store* s, int ref, int que, const unsigned char* inlier /*host [*n] or NULL*/,
                             const double R_in[9], const double t_in[3], const double K_left[9], const double K_right[9],
                             double lambda, int iters, double max_err2, double cos2_min, int* n, int* r_idx, int* q_idx,
                             double R_out[9], double t_out[3], double F_out[9], double cost[2], double info[15], int* n_used,
                             int* status, double* obs_res, unsigned char* obs_inlier, unsigned char* obs_front, double* X_out,
                             int* n_inliers, int* n_front, int* n_parallax);
/* (The next two work on a track store; like sfm_obs_* and sfm_twoview_verify_pairs they are not part of the KeyTrack /
 * KeyTracker surface the sfm_track_* names cover.)
 * sfm_match_guided_dev with the coordinates the store already holds: `query` is the descriptor set of view que_view,
 * refs[r] that of view ref_views[r] (any views of the store, in any order; each set has its view's key count).  No
 * coordinate is uploaded.  Outputs are DEVICE pointers; follows the store's stream rule (above). */
int sfm_match_guided_track(sfm_track_store* s, int que_view, sfm_desc_set* query, int n_refs, const int* ref_views,
                           sfm_desc_set* const* refs, const int* kind, const double* model, double max_err2, int* d_best_idx,
                           float* d_best_dist, int* d_second_idx, float* d_second_dist, uint8_t* d_mutual, int* d_n_admitted,
                           void* hip_stream);
/* Replace the matches between the views ref and que by n pairs (host arrays): row que of table[ref] and row ref of
 * table[que] are set to -1, then table[ref][que, r_idx[k]] = q_idx[k] and table[que][ref, q_idx[k]] = r_idx[k].  An index
 * out of range or repeated on either side, ref == que, or a table without the row returns SFM_E_SHAPE and writes
 * nothing.  The only way a guided result enters the tables.  Blocking. */
int sfm_match_guided_set_pairs(sfm_track_store* s, int ref, int que, int n, const int* r_idx, const int* q_idx);
/* KeyTrack.update_usage: table[view][view, keys[i]] = tri[i] (host arrays).  A key given twice takes the LAST value,
 * as NumPy's fancy assignment does; a key outside [0, n) returns SFM_E_SHAPE and writes nothing. */
int sfm_track_update_usage(sfm_track_store* s, int view, int n, const int* keys, const int* tri);
/* KeyTrack.extract_constructed_points / extract_unconstructed_points: the keys of the view's own row that are != -1
 * (with their values) / == -1, ascending.  Buffers hold the view's key count; tri may be NULL. */
int sfm_track_constructed(sfm_track_store* s, int view, int* n, int* keys, int* tri);
int sfm_track_unconstructed(sfm_track_store* s, int view, int* n, int* keys);
/* Copy out one table ([rows][n keys]) or one of its rows. */
int sfm_track_copy_table(sfm_track_store* s, int view, int* out);
int sfm_track_copy_row(sfm_track_store* s, int view, int row, int* out);

/* ---- bundle-adjustment observations from the resident tracks (ba_processor.py:304-310, 339-342) --------------------
 * (sfm_obs_*: they work on a track store, but are not part of the KeyTrack / KeyTracker surface the sfm_track_* names cover.)
 * The normalised coordinates inv(K) @ [x, y, 1] / w of ALL n keys of `view` (host arrays u, v; n must be the view's
 * key count).  The product is the host's BLAS product, whose bits a kernel cannot reproduce: the host computes it once
 * per view (again when the view's intrinsic matrix changes) and the device only gathers from it.  16 n bytes, counted in
 * SFM_TRACK_INFO_UPLOAD_BYTES.  Blocking. */
int sfm_obs_set_normalised(sfm_track_store* s, int view, int n, const double* u, const double* v);
/* The observation list of the loop ba_processor.py:304-310 over the views 0 .. n_views-1 and the points 0 .. n_pts-1,
 * from the views' own rows table[v][v, :], in buffers the store owns: pt_ptr[n_pts + 1], cam_idx[M], key_idx[M], u[M],
 * v[M], sorted by (point, view).  KeyTracker.is_visible's semantics (key_tracker.py:198-204, quirk Q3): view v sees
 * point p iff some key k > 0 has table[v][v, k] == p, and the observation is then the SMALLEST such key, 0 included;
 * entries < 0 or >= n_pts are ignored.  Every view with keys needs its normalised table.  *n_obs = M (may be NULL).
 * The min / max-key scratch holds 2 n_views n_pts ints; above 2^28 ints (1 GiB) the call returns SFM_E_SHAPE.
 * Blocking (the count M comes back, 4 bytes that SFM_TRACK_INFO_DOWNLOAD_BYTES leaves out); the list stays valid until
 * the next build. */
int sfm_obs_build(sfm_track_store* s, int n_views, int n_pts, int64_t* n_obs);
/* Blocking: the list of the last build (uv is (2, M) row-major: all u, then all v).  Any output may be NULL; the sizes
 * come from sfm_track_info (SFM_TRACK_INFO_OBS_PTS, SFM_TRACK_INFO_N_OBS).  Counted as download bytes. */
int sfm_obs_copy(sfm_track_store* s, int* pt_ptr, int* cam_idx, int* key_idx, double* uv);

/* The store form of the track linking (block "track linking" above).  pairs[P][2] = (ref, que) (host).  The matches of pair p are the entries q = table[ref][que, r] with
 * q > 0 (quirk Q3), exactly the set sfm_track_pairs returns, read where they lie: a = r, b = q.  key_mask (host or NULL)
 * holds one byte per key of each pair's reference view, concatenated in pair order (match (r, q) is used iff the byte of r
 * is non-zero); it is the only upload.  The result becomes the store's current observation list, in the buffers
 * sfm_obs_build fills: n_views is the store's view count, n_pts = n_tracks, u and v are gathered from the normalised
 * tables (sfm_obs_set_normalised); sfm_track_info(OBS_*), sfm_obs_copy, sfm_ba_create_from_tracks and sfm_ba_sync_tracks
 * then work on it unchanged.  Refused with the store as it was: a view out of range, ref == que, a table without the row, a
 * view named in `pairs` that has keys but no normalised coordinates, min_len < 2.  A table entry that names a key its
 * query view does not have is found by the verify kernel; the store is then left without a current observation list.  No
 * table is written.  d_key_track: [total keys of the store] on the device, or NULL.  Blocking, on the library stream, after
 * the store's pending work (the store's stream rule). */
int sfm_link_tracks_views(sfm_track_store* s, int P, const int* pairs /*host [P][2]*/, const unsigned char* key_mask /*host or NULL*/,
                         int min_len, int* d_key_track, int64_t* summary /*[8]*/);

/* A resident BA problem (see sfm_ba_create) whose structure is the store's current observation list, copied device to
 * device: nothing is uploaded, SFM_INFO_UPLOAD_BYTES starts at 0.  Cameras and points are set as after sfm_ba_create.
 * The problem keeps no reference to the store. */
#define SFM_SYNC_REUSE    0   /* the list is the resident structure: nothing changed, nothing uploaded */
#define SFM_SYNC_GROWN    1   /* every resident track is part of the list's track of the same point: the problem adopted the list */
#define SFM_SYNC_REPLACED 2   /* anything else: the problem is unchanged, the caller builds a new one */
int sfm_ba_create_from_tracks(sfm_track_store* s, sfm_ba_problem** out);
/* Compare the store's current list (V2 views, N2 points) with the resident structure (V, N) on the device and bring the
 * problem up to it.  REUSE: V2 == V, N2 == N and every track, camera index and u, v bit pattern is the same.  GROWN:
 * V2 >= V, N2 >= N, n_new_cams == V2 - V, n_new_pts == N2 - N and every resident track is a subsequence of the new
 * track of its point with bitwise equal u, v; the problem then becomes one of the new sizes that holds the list, the old
 * cameras and points (device to device) and the new ones (cams_new (n_new_cams, 7), pts_new (3, n_new_pts) row-major,
 * the only upload: 56 n_new_cams + 24 n_new_pts bytes), and keeps handle, options, stream, communicator and counters
 * as sfm_ba_append does.  REPLACED: an observation went away, its key or its u, v changed, there are fewer views or
 * points, or the counts do not match.  *n_new_obs = the observations added (0 unless GROWN; may be NULL).  Blocking. */
int sfm_ba_sync_tracks(sfm_ba_problem* p, sfm_track_store* s, int n_new_cams, const double* cams_new, int n_new_pts,
                       const double* pts_new, int* action, int64_t* n_new_obs);
/* Blocking: the resident observation list in the layout sfm_ba_create takes: pt_ptr[N + 1], cam_idx[M], uv_norm (2, M)
 * (sizes from sfm_ba_info).  Any output may be NULL. */
int sfm_ba_get_structure(sfm_ba_problem* p, int* pt_ptr, int* cam_idx, double* uv_norm);

#ifdef __cplusplus
}
#endif
#endif /* SFM_HIP_H */
