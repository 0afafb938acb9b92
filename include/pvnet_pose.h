/*
 * pvnet_pose.h -- C ABI of libpvnet_pose.so: clean-pvnet's pose from 2D-3D keypoint correspondences, start included, for a
 * whole batch on the device (HIP, gfx950).  One wavefront per image, binary64 throughout.
 *
 * What it replaces (per image, on the host, in the reference):
 *   default path   lib/utils/pvnet/pvnet_pose_utils.py:5-38, pnp(kpt_3d, kpt_2d, K): cv2.solvePnP(..., SOLVEPNP_ITERATIVE)
 *                  = a DLT start on non-planar points, then Levenberg-Marquardt on the plain reprojection error; called from
 *                  lib/evaluators/{linemod,custom,tless_test}/pvnet.py (:188, :97, :239) and the visualizers.
 *   cfg.test.un_pnp  lib/csrc/uncertainty_pnp/un_pnp_utils.py:26-38: cv2.solvePnP(..., SOLVEPNP_P3P) on the four
 *                  best-weighted keypoints, then the Ceres refinement (include/pvnet_pnp.h); with four keypoints the P3P pose
 *                  is the result (:34-38).
 *
 * Start methods (their host twins are clean_pvnet_amd/un_pnp_utils.py's initial_pose_p3p / initial_pose_dlt):
 *   PVP_START_P3P  key = wxx + wxy per keypoint (un_pnp_utils.py:26), a non-finite key ranks lowest; the four largest keys,
 *                  ascending, a tie broken by the index (the higher one comes later).  Grunert's P3P on the first three, the
 *                  fourth picks among the solutions by its reprojection error; a solution that puts it behind the camera is
 *                  skipped, a collinear object triple has none.  No solution and pn >= 6: the weighted DLT of
 *                  initial_pose_dlt(P, p, K, order_key=key) (status PVP_STATUS_DLT_FALLBACK); pn < 6: no start.
 *   PVP_START_DLT  initial_pose_dlt(P, p, K): the smallest right singular vector of the 2pn x 12 system of the conditioned
 *                  points, sign by det, rotation orthogonalised by SVD with scale = the mean singular value.  pn < 6 has no
 *                  start (OpenCV's DLT refuses it too).  A planar model (OpenCV's test: the scatter matrix of the centred 3D
 *                  points has eigenvalues l1 >= l2 >= l3 with l3 / l2 < 1e-3) gets PVP_STATUS_PLANAR: the homography start
 *                  OpenCV takes there is not implemented.
 *                  The keyed DLT keeps the keypoints with a positive key; with fewer than six of them it takes the six
 *                  largest keys (a tie goes to the lower index; 0, negative and non-finite keys all count as 0), each
 *                  + 1e-12, row weight max(sqrt(key / max key), 1e-3).  Those six make the system 12 x 12 with rows of
 *                  weight 1e-3, condition number ~1e5: its null vector comes from a one-sided Jacobi SVD of the system
 *                  itself (as accurate as svd(A): the start equals the twin's to ~1e-9), not from the eigenvectors of
 *                  the normal matrix A^T A, which every other DLT start here uses and which would leave it to ~1e-6.
 * Rotation matrix -> angle-axis (both starts end with it; un_pnp_utils.rotation_to_angle_axis is its twin): with v the
 *                  antisymmetric part of R (|v| = 2 sin th) and c = (trace - 1) / 2 the angle is atan2(|v| / 2, c), never
 *                  acos(c), which loses half the digits at 0 and at pi; below 1e-9 rad the result is v / 2; the axis is
 *                  v / |v| while c > -0.5 and otherwise the largest row (the first of equals) of (R + R^T) / 2 - c I =
 *                  (1 - c) a a^T, signed by v.  An error e in R moves the rotation returned by O(e) at every angle; at a
 *                  half turn w and -w are the same rotation and rounding picks between them.
 * Both starts also run inside pvp_pose_batched when the P3P start falls back.  The refinement is the LM of pvnet_pnp.h
 * (the same device code), with the weights given or, without them, identity weights (1, 0, 1).
 */
#ifndef PVNET_POSE_H_
#define PVNET_POSE_H_

#include <stdint.h>

#define PVP_START_P3P 0
#define PVP_START_DLT 1

/* d_status, one code per image.  A failed image (code < 0) gets NaN in every output row; the others are unaffected. */
#define PVP_STATUS_P3P 0           /* P3P start */
#define PVP_STATUS_DLT 1           /* DLT start */
#define PVP_STATUS_DLT_FALLBACK 2  /* DLT start after P3P found no solution */
#define PVP_STATUS_NO_START -1     /* no start: pn < 6 for the DLT, or P3P found no solution and pn < 6 */
#define PVP_STATUS_PLANAR -2       /* planar model: the DLT start does not apply */
#define PVP_STATUS_NONFINITE -3    /* a non-finite keypoint or camera entry, a singular camera matrix, or (pvp_pose_batched
                                      with weights) a non-finite weight */

#ifdef __cplusplus
extern "C" {
#endif

/* The start only, for a batch, on DEVICE pointers, launched on `stream` (hipStream_t as void*); no allocation, no
 * synchronisation.
 *   d_pts2d [B,pn,2]   d_wgt2d [B,pn,3] = (wxx,wxy,wyy), read for the P3P key only; NULL is allowed with PVP_START_DLT
 *   d_pts3d [pn,3] shared when pts3d_batched == 0, else [B,pn,3];   d_K [9] row-major, shared when K_batched == 0, else [B,9]
 *   d_rt    [B,6] angle-axis + translation;   d_status [B] int32.   pn in [4, 4096].
 * Replaces un_pnp_utils.py:26-32 (P3P) and the DLT start of pvnet_pose_utils.py:19-23 (cv2.solvePnP, SOLVEPNP_ITERATIVE).
 * Returns 0 (also for B == 0, nothing launched), -1 (bad arguments, checked before any launch) or a hipError_t. */
int pvp_initial_pose_batched(const double *d_pts2d, const double *d_pts3d, const double *d_wgt2d, const double *d_K,
                             int method, double *d_rt, int *d_status, int B, int pn, int pts3d_batched, int K_batched,
                             void *stream);

/* Start and refinement in one launch.  Arguments as above, plus
 *   d_wgt2d        NULL = unweighted (identity weights), then only PVP_START_DLT is accepted; with weights a non-finite
 *                  weight makes the image PVP_STATUS_NONFINITE
 *   d_result_rt    [B,6] the refined pose (with PVP_START_P3P and pn == 4 the P3P pose, unrefined: un_pnp_utils.py:34-38)
 *   d_Rt           [B,3,4] or NULL: [R | t] of d_result_rt, R = Rodrigues(angle-axis)
 *   d_init_rt      [B,6] or NULL: the start
 *   d_info         [B,4] or NULL: initial cost, final cost, iterations, termination as in pvp_uncertainty_pnp_batched;
 *                  NaN for an image that was not refined
 *   max_iterations <= 0 selects 50, function_tolerance <= 0 selects 1e-6 (pvnet_pnp.h).
 * Replaces pvnet_pose_utils.py:5-38 (without weights) and un_pnp_utils.py:26-57 (with them), per image on the host.
 * Returns 0 (also for B == 0, nothing launched), -1 (bad arguments, checked before any launch) or a hipError_t. */
int pvp_pose_batched(const double *d_pts2d, const double *d_pts3d, const double *d_wgt2d, const double *d_K, int method,
                     double *d_result_rt, double *d_Rt, double *d_init_rt, int *d_status, double *d_info, int B, int pn,
                     int pts3d_batched, int K_batched, int max_iterations, double function_tolerance, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_POSE_H_ */
