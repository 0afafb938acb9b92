/*
 * pvnet_icp.h -- C ABI of libpvnet_icp.so: one stage of the ICP pose refinement for a whole batch of poses on the device
 * (HIP, gfx950), from the depth renders of the poses and the sensor images to the refined poses.
 *
 * What it replaces (per image and per stage, on the host, in the reference): ICPRefiner.refine and icp of
 * lib/utils/icp/icp_utils.py:83-176, reached through Evaluator.icp_refine (lib/evaluators/linemod/pvnet.py:102-116,
 * tless_test/pvnet.py:143-158, custom/pvnet.py:75-86) -- an OpenGL depth render, two numpy point clouds, a radius filter, a
 * draw of up to 3000 points from each cloud and up to 200 rounds of a scikit-learn nearest-neighbour search with a 3x3 SVD fit.
 * The render itself comes from pvs_render_depth_batched (include/pvnet_vsd.h).
 *
 * Everything runs on the caller's stream in a workspace the caller owns; no call allocates, synchronises or reads back.
 * No workgroup waits for another: the rounds are launches on the stream, and a pose that has converged makes every later
 * launch return at once.  The library is compiled with -ffp-contract=off.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * Arithmetic contract.  Everything is binary64 and uses only + - * / sqrt and comparisons, each rounded once, in the stated
 * order.  tests/icp_twin.py is the numpy twin the device equals bit for bit.
 *
 *   sums        two fixed orders over a list v_0 .. v_(m-1), padded with +0.0 to a multiple of 256:
 *               TILE    tiles of 256 consecutive values, each reduced by a binary tree over its 256 slots (slot j += slot
 *                       j + 128, then 64, ... 1), the tile sums added in ascending tile order (as in pvnet_vsd.h);
 *               STRIDE  slot j = ((v_j + v_(j+256)) + v_(j+512)) + ..., then one binary tree over the 256 slots.
 *   clouds      (rgbd_to_point_cloud, :7-13) pixel (u, v) with depth z belongs to a cloud when z != 0; its point is
 *               x = ((u - cx)*z)/fx,  y = ((v - cy)*z)/fy,  z.  Pixels are ranked in row-major order (numpy's nonzero).
 *               synthetic  z = the float32 render widened to binary64.
 *               real       z = float64(raw)*depth_scale for a uint16 sensor image, the value widened for float32 / float64;
 *                          with a mask, only the pixels whose mask value equals 1 (:150 of tless_test/pvnet.py).
 *   synthetic   n_syn = the number of points;  centroid_k = TILE(k-th coordinate over the flat image, +0.0 outside the
 *   statistics  cloud) / float64(n_syn);  with d = p - centroid:  max_dist = sqrt(max over the cloud of (dx*dx + dy*dy) + dz*dz)
 *               (sqrt is monotone, so this is the largest of the distances, :141).
 *   filter      a real point is kept when sqrt((dx*dx + dy*dy) + dz*dz) < max_mean_dist_factor*max_dist, d = p - centroid
 *               (:147-148); n_real counts the kept points, which are ranked in row-major order again.
 *   visibility  not enough visible points  <=>  float64(n_real) < float64(n_syn)/20.0  (:149).
 *   samples     n = min(n_real, n_syn, n_max) (:155-156).  Sample k < n of a cloud of `count` points is the point of rank
 *               idx[k]: injected (the first n columns of d_idx_syn / d_idx_real), or drawn from a 32-bit word as
 *               idx = (word * count) >> 32  (d_words).  An injected index outside [0, count) gives PVI_BAD_INDEX.
 *   a round     (icp, :101-116) with the source samples s_i and the destination samples d_j, i, j < n:
 *               1. nn(i) = the j that minimises (ex*ex + ey*ey) + ez*ez, e = s_i - d_j; the lowest j wins a tie;
 *               2. mean = STRIDE(sqrt of that minimum) / float64(n);
 *               3. (R, t) = fit(s_i -> d_nn(i));
 *               4. s_i := (((R_k0*x + R_k1*y) + R_k2*z) + t_k) for k = 0, 1, 2;
 *               5. stop when |prev - mean| < tolerance (prev = 0 before the first round, = mean afterwards) or after
 *                  max_iterations rounds.
 *               Then (R, t) = fit(original samples -> final s_i) once more (:119).
 *   fit         (best_fit_transform, :35-80) of the pairs a_i -> b_i:  cA_k = STRIDE(a_ik)/float64(n), cB alike.
 *               depth_only and not no_depth:  R = I,  t = cB - cA.
 *               otherwise  S_kl = STRIDE((a_ik - cA_k)*(b_il - cB_l)), the rotation below, and
 *               t_k = cB_k - ((R_k0*cA_0 + R_k1*cA_1) + R_k2*cA_2);  no_depth and not depth_only:  t_2 := 0.
 *   rotation    Horn's closed form: the proper rotation that maximises trace(R*S) is that of the unit quaternion (w, x, y, z)
 *               which is the eigenvector of the largest eigenvalue of the symmetric
 *                 N = [ (Sxx+Syy)+Szz   Syz-Szy          Szx-Sxz          Sxy-Syx        ]
 *                     [       .         (Sxx-Syy)-Szz    Sxy+Syx          Szx+Sxz        ]
 *                     [       .               .          (Syy-Sxx)-Szz    Syz+Szy        ]
 *                     [       .               .                .          (Szz-Sxx)-Syy  ]
 *               -- the same rotation as V*diag(1, 1, det(V*U^T))*U^T of the reference's SVD with its reflection fix (:64-70)
 *               wherever that is unique.  N is diagonalised by cyclic Jacobi sweeps over the pairs (p, q) = (0,1), (0,2),
 *               (0,3), (1,2), (1,3), (2,3), V = I at the start, at most 30 sweeps, ended by the first sweep without a
 *               rotation.  A pair with g = |N_pq| is skipped (and N_pq := 0) when g == 0 or (|N_pp| + g == |N_pp| and
 *               |N_qq| + g == |N_qq|); otherwise
 *                 theta = (N_qq - N_pp)/(2*N_pq);  r = sqrt(theta*theta + 1);  tt = 1/(|theta| + r), negated when theta < 0;
 *                 c = 1/sqrt(tt*tt + 1);  s = tt*c;
 *                 N_pp -= tt*N_pq;  N_qq += tt*N_pq;  N_pq := 0;
 *                 for the two other k:  (N_kp, N_kq) := (c*N_kp - s*N_kq,  s*N_kp + c*N_kq)   (and symmetrically)
 *                 for every k:          (V_kp, V_kq) := (c*V_kp - s*V_kq,  s*V_kp + c*V_kq).
 *               The eigenvector is the column of V of the largest N_jj (the lowest j wins a tie), divided by
 *               sqrt(((w*w + x*x) + y*y) + z*z), and
 *                 R = [ 1-2*(yy+zz)  2*(xy-wz)    2*(xz+wy)   ]
 *                     [ 2*(xy+wz)    1-2*(xx+zz)  2*(yz-wx)   ]      with xx = x*x, xy = x*y, ... wz = w*z.
 *                     [ 2*(xz-wy)    2*(yz+wx)    1-2*(xx+yy) ]
 *   after       (refine, :159-176) with no_depth, the step is dropped (PVI_ROTATION_LIMIT, the pose unchanged) when
 *               (((R_00 + R_11) + R_22) - 1)/2 < cos_limit, cos_limit = cos(20 degrees) computed by the caller.  Otherwise
 *               R' = R*R_est with R'_kl = (R_k0*E_0l + R_k1*E_1l) + R_k2*E_2l (R_est copied when the fit's R = I by mode),
 *               t'_k = ((R_k0*t_0 + R_k1*t_1) + R_k2*t_2) + t_k  with t_est on the right.
 */
#ifndef PVNET_ICP_H_
#define PVNET_ICP_H_

#include <stddef.h>
#include <stdint.h>

/* sensor_kind: the element type of the sensor image */
#define PVI_DEPTH_U16 0
#define PVI_DEPTH_F32 1
#define PVI_DEPTH_F64 2

/* mask_kind: the element type of the mask */
#define PVI_MASK_NONE 0
#define PVI_MASK_U8 1    /* uint8 or bool */
#define PVI_MASK_I64 2

/* status (column PVI_STATUS of d_info) */
#define PVI_REFINED 0
#define PVI_EMPTY_RENDER 1     /* the pose renders nothing: pose unchanged (:140-143) */
#define PVI_NOT_VISIBLE 2      /* not enough visible points: pose unchanged (:149-152) */
#define PVI_ROTATION_LIMIT 3   /* the rotation of the step exceeds the limit: step dropped (:159-163) */
#define PVI_BAD_POSE 4         /* a non-finite entry or t_z <= 0: pose unchanged (linemod/pvnet.py:105) */
#define PVI_SMALL_MASK 5       /* fewer than min_mask_pixels pixels equal to 1: pose unchanged (tless_test/pvnet.py:148) */
#define PVI_BAD_INDEX 6        /* an injected sample index outside its cloud: pose unchanged */

/* columns of d_info */
#define PVI_STATUS 0
#define PVI_N_SYN 1
#define PVI_N_REAL 2
#define PVI_N 3
#define PVI_ROUNDS 4           /* rounds of the loop that ran (the reference's i + 1) */
#define PVI_INFO_COLUMNS 5

/* flags */
#define PVI_DEPTH_ONLY 1
#define PVI_NO_DEPTH 2

#define PVI_MAX_SIDE 16384
#define PVI_MAX_SAMPLES 16384

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of d_workspace that pvi_refine_batched needs.  0 for an empty batch or bad sizes. */
size_t pvi_workspace_bytes(int P, int H, int W, int n_max);

/* One stage of ICPRefiner.refine (icp_utils.py:134-176, with icp :83-126, best_fit_transform :35-80 and
 * rgbd_to_point_cloud :7-13) for P poses, on DEVICE pointers, launched on `stream` (hipStream_t as void*).
 *   d_render   [P,H,W] float32, the depth render of each pose (pvs_render_depth_batched)
 *   d_sensor   [P/per_image,H,W] of `sensor_kind`: pose p looks at image p / per_image;  depth_scale applies to
 *              PVI_DEPTH_U16 only
 *   d_mask     [P/per_mask,H,W] of `mask_kind` (NULL with PVI_MASK_NONE): pose p takes mask p / per_mask
 *   d_pose     [P,3,4] binary64 [R | t] in the units of the render;   d_K [9] row-major, or [P,9] when K_batched
 *   d_idx_syn, d_idx_real  [P,n_max] int32 injected sample indices, or both NULL: then
 *   d_words    [P,2,n_max] int64 whose low 32 bits are the random words (row 0 synthetic, row 1 real)
 *   flags      PVI_DEPTH_ONLY | PVI_NO_DEPTH as the reference's two arguments
 *   d_pose_out [P,3,4] binary64;   d_info [P,PVI_INFO_COLUMNS] int32
 *   d_workspace  pvi_workspace_bytes(P, H, W, n_max) bytes, 16-byte aligned; contents need not survive the call
 * Arithmetic: the contract at the top of this file.
 * Returns 0 (also for P == 0, nothing launched), -1 (bad arguments, checked before any launch) or a hipError_t. */
int pvi_refine_batched(const float *d_render, const void *d_sensor, int sensor_kind, double depth_scale, int per_image,
                       const void *d_mask, int mask_kind, int per_mask, int min_mask_pixels, const double *d_pose,
                       const double *d_K, int K_batched, const int32_t *d_idx_syn, const int32_t *d_idx_real,
                       const long long *d_words, int flags, double max_mean_dist_factor, int n_max, int max_iterations,
                       double tolerance, double cos_limit, double *d_pose_out, int32_t *d_info, void *d_workspace, int P,
                       int H, int W, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_ICP_H_ */
