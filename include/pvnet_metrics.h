/*
 * pvnet_metrics.h -- C ABI of libpvnet_metrics.so: clean-pvnet's pose scores (ADD, ADD-S, 2D projection, 5 cm 5 degrees)
 * and the mask intersection / union for a whole batch on the device (HIP, gfx950).
 *
 * What it replaces (per image, on the host, in numpy, in the reference): the bodies of Evaluator.add_metric,
 * .projection_2d, .cm_degree_5_metric and .mask_iou of lib/evaluators/linemod/pvnet.py:59-100 (the same code in
 * custom/pvnet.py:88-107 and tless_test/pvnet.py:107-125), and under add_metric(syn=True) the per-image round trip of
 * lib/csrc/nn/nn_utils.py:5-20 (host -> device copies, one search kernel shaped for one image, a copy back).
 *
 * Arithmetic contract.  binary64, one rounding per operation, no contraction, in this order:
 *   cloud      x[i] = ((m0*R[i,0] + m1*R[i,1]) + m2*R[i,2]) + t[i], m the float32 model point widened: np.dot(model,
 *              pose[:, :3].T) + pose[:, 3] (linemod/pvnet.py:70-71).
 *   ADD        mean over the points of sqrt((dx*dx + dy*dy) + dz*dz) between the two clouds (:77).
 *   ADD-S      both clouds rounded to float32 (nn_utils.py:11-12); for every point of the ground-truth cloud the nearest
 *              point of the predicted cloud by (dx*dx + dy*dy) + dz*dz in binary32, strict `<`, first minimum wins
 *              (nearest_neighborhood.cu:48-117, as libpvnet_nn.so); the distance that enters the mean is the binary64
 *              distance between predicted point idx and the ground-truth point (:74-75).
 *   projection u[i] = (x0*K[i,0] + x1*K[i,1]) + x2*K[i,2], pixel = (u0/u2, u1/u2) for both poses
 *              (pvnet_pose_utils.py:41-50), mean over the points of sqrt(du*du + dv*dv) (linemod/pvnet.py:60-62).
 *   5 cm 5 deg translation = sqrt((dx*dx + dy*dy) + dz*dz) * 100 of the two t; trace = sum_i ((Rp[i,0]*Rg[i,0] +
 *              Rp[i,1]*Rg[i,1]) + Rp[i,2]*Rg[i,2]) clamped to [-1, 3], angle = acos((trace - 1) / 2) * (180 / pi)
 *              (pvnet_pose_utils.py:53-60).
 *   sums       over the N points: tiles of 256 consecutive points, each reduced by a binary tree over its 256 slots
 *              (slot j += slot j + 128, then 64, ... 1), the tile sums then added in ascending tile order.  The order
 *              depends on N only -- not on B, the grid or the slab count -- and there are no floating-point atomics:
 *              two identical calls return the same bits, image i of a batch the same bits as a batch of image i alone.
 *   non-finite a pose (predicted or ground truth) containing a non-finite value gives NaN in the five columns of that
 *              image and zeros in its d_adds_idx row; the other images are unaffected.
 */
#ifndef PVNET_METRICS_H_
#define PVNET_METRICS_H_

#include <stddef.h>
#include <stdint.h>

/* columns of d_metrics */
#define PVM_ADD 0       /* ADD mean distance (model units) */
#define PVM_ADDS 1      /* ADD-S mean distance; NaN for an image whose d_symmetric byte is 0 */
#define PVM_PROJ2D 2    /* mean 2D projection distance (pixels) */
#define PVM_TRANS_CM 3  /* translation distance * 100 */
#define PVM_ANG_DEG 4   /* angular distance (degrees) */

#ifdef __cplusplus
extern "C" {
#endif

/* The number of slabs the reference cloud of the ADD-S search is split into when `slabs` <= 0 is passed below: 1 when the
 * batch alone gives the chip about twelve blocks per compute unit, more for smaller batches, never so many that a slab
 * holds fewer than 64 points.  The result of a call does not depend on it. */
int pvm_adds_slabs(int B, int N);

/* Bytes of d_workspace that pvm_pose_metrics_batched needs for (B, N, slabs); slabs <= 0 = pvm_adds_slabs(B, N).
 * 0 for B <= 0 or N <= 0. */
size_t pvm_workspace_bytes(int B, int N, int slabs);

/* The five scores of B (prediction, ground truth) pose pairs of one object model, on DEVICE pointers, launched on
 * `stream` (hipStream_t as void*); no allocation, no synchronisation.
 *   d_pose_pred, d_pose_gt [B,3,4] binary64 [R | t];   d_model [N,3] float32
 *   d_K          [9] row-major, shared when K_batched == 0, else [B,9]
 *   d_symmetric  NULL (no image is symmetric: the search is not launched) or [B] bytes: ADD-S for the images whose byte
 *                is set, so a non-symmetric image does not pay for the search
 *   d_metrics    [B,5] binary64, columns PVM_*
 *   d_adds_idx   NULL or [B,N] int32: the neighbour indices of the symmetric images, zeros for the others
 *   d_workspace  pvm_workspace_bytes(B, N, slabs) bytes, 16-byte aligned; contents need not survive the call
 *   slabs        <= 0 selects pvm_adds_slabs(B, N); a value above N is taken as N (a test and tuning hook)
 * Replaces linemod/pvnet.py:59-94 with nn_utils.py:5-20 and pvnet_pose_utils.py:41-60, per image on the host.
 * Returns 0 (also for B == 0, nothing launched), -1 (bad arguments, checked before any launch) or a hipError_t. */
int pvm_pose_metrics_batched(const double *d_pose_pred, const double *d_pose_gt, const float *d_model, const double *d_K,
                             const uint8_t *d_symmetric, double *d_metrics, int32_t *d_adds_idx, void *d_workspace,
                             int B, int N, int K_batched, int slabs, void *stream);

/* (mask_pred & mask_gt).sum() and (mask_pred | mask_gt).sum() per image, exact integers (linemod/pvnet.py:96-100, there
 * on the host after two copies).  Each mask is B images of H*W contiguous elements of 1, 4 or 8 bytes (bool / uint8,
 * int32, int64: the int64 mask decode_keypoint writes against any of them), image b starting `*_stride_b` ELEMENTS after
 * image b-1, so a slice of a larger batch is accepted.  `&` and `|` are bitwise on the values widened to 64 bits, as numpy
 * does for integer arrays.
 *   d_inter, d_union [B] int64, written by the call (set to zero on `stream` first, then integer atomic adds: exact).
 * Returns 0 (also for B == 0), -1 (bad arguments, checked before any launch) or a hipError_t. */
int pvm_mask_iou_batched(const void *d_mask_pred, const void *d_mask_gt, long long pred_stride_b, long long gt_stride_b,
                         int pred_elem_size, int gt_elem_size, long long *d_inter, long long *d_union, int B, int H, int W,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_METRICS_H_ */
