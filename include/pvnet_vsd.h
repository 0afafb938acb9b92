/*
 * pvnet_vsd.h -- C ABI of libpvnet_vsd.so: a batched depth rasteriser and the Visible Surface Discrepancy of every
 * (prediction, ground truth) pair of every image of a batch, on the device (HIP, gfx950).
 *
 * What it replaces (per pose pair, on the host, in the reference): Evaluator.vsd_metric of
 * lib/evaluators/tless_test/pvnet.py:66-105 -- one OpenGL render per predicted and per ground-truth pose
 * (DepthRender.render, lib/utils/renderer/opengl_utils.py:405-492), depth_im_to_dist_im (lib/utils/vsd/misc.py:42-60) on
 * each, estimate_visib_mask_gt / _est (lib/utils/vsd/visibility.py:6-29) and vsd (lib/utils/vsd/vsd_utils.py:5-48): about
 * ten numpy passes over a 720x540 image per pair.
 *
 * Everything runs on the caller's stream in a workspace the caller owns; no call allocates, synchronises or reads back.
 * The library is compiled with -ffp-contract=off: every operation below is rounded once, in the stated order.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * Arithmetic contract of the rasteriser.  OpenGL leaves sub-pixel snapping and the fill rule to the hardware, so it cannot
 * be matched bit for bit; the conventions are the reference's (eye-space Z of the nearest surface, v_eye_depth
 * :103-122; no face culling, :439; background 0; fragments outside [near, far] dropped) and the rest is stated here.
 * tests/vsd_twin.py is the numpy twin the device equals bit for bit.
 *
 *   half pixel  pixel (x, y) is sampled at image coordinates (x + 0.5, y + 0.5) of K: _compute_calib_proj (:147-182) maps
 *               K's image plane onto the viewport [0, W] x [0, H] and OpenGL samples a pixel at its centre.
 *   eye space   binary64, the float32 model point (x, y, z) widened first:
 *               X = ((r00*x + r01*y) + r02*z) + t0, Y and Z with rows 1 and 2 of [R | t] in the same order.
 *               Once per (pose, vertex).
 *   near clip   a vertex is inside when Z >= near.  A triangle with no vertex inside is dropped; with all three inside it
 *               is one piece; otherwise it is clipped against Z = near in eye space.  The new vertex on the edge from an
 *               inside vertex p to an outside vertex q (always in this direction, so that two triangles sharing the edge
 *               get the same vertex) is  t = (near - Zp) / (Zq - Zp),  X = Xp + t*(Xq - Xp),  Y = Yp + t*(Yq - Yp),
 *               Z = near.  With the triangle's vertices rotated (cyclic order kept) to (a, b, c):
 *                 a inside, b and c outside:  one piece   (a, ab, ac)
 *                 a and b inside, c outside:  two pieces  (a, b, bc) and (a, bc, ac)
 *               Coverage comes from the pieces, depth from the plane of the original triangle.
 *   projection  binary64, K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]] (the other entries are not read):
 *               u = (fx*X + s*Y)/Z + cx,  v = (fy*Y)/Z + cy.
 *   snapping    8 sub-pixel bits: U = floor(256*u + 0.5), V = floor(256*v + 0.5), as integers.  A piece with a vertex
 *               whose |U| or |V| exceeds 2^28 (or is not a number) is skipped.
 *   coverage    exact, in 64-bit integers.  The doubled area of a piece is (U1-U0)*(V2-V0) - (V1-V0)*(U2-U0); a piece of
 *               area zero is skipped, one of negative area has vertices 1 and 2 exchanged.  For each edge a -> b of
 *               (0->1, 1->2, 2->0) with dx = Ub-Ua, dy = Vb-Va the edge function of the sample (px, py) =
 *               (256x+128, 256y+128) is  E = dx*(py - Va) - dy*(px - Ua).  The sample is covered when every E > 0, or
 *               E = 0 on an edge that owns its line: dy > 0, or dy = 0 and dx > 0.  Two triangles walk a shared edge in
 *               opposite directions, so exactly one of them owns it.
 *   depth       with the three eye-space vertices v0, v1, v2 of the unclipped triangle in the order of its face row,
 *               a = v1 - v0, b = v2 - v0:  n = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0),
 *               num = (n0*v00 + n1*v01) + n2*v02;  per sample  dy = ((y+0.5) - cy)/fy,
 *               dx = (((x+0.5) - cx) - s*dy)/fx,  den = (n0*dx + n1*dy) + n2,  Z = num/den.  den = 0 skips the sample;
 *               it is kept when near <= Z <= far, Z is rounded to float32, and the pixel takes the minimum over all
 *               triangles.  The minimum of positive floats is the unsigned minimum of their bit patterns (an integer
 *               atomic): the image does not depend on the order of the triangles, on the batch or on scheduling.
 *   bad input   a face row with an index outside [0, N) is skipped (checked on the device, nothing is read on the host).
 *               A pose with a non-finite entry gives an all-zero image.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * Arithmetic contract of VSD, per pixel (x, y) of image i and pair (prediction a, ground truth b), in this order:
 *
 *   test depth  d_test = float64(raw) * depth_scale for a uint16 image (the reference: load_depth(path) * 0.1,
 *               tless_test/pvnet.py:69), the value itself widened to binary64 for a float32 / float64 image.
 *   distance    binary64, for the test image and for each float32 render widened to binary64 (misc.py:42-60):
 *               Xs = ((x - cx)*depth)*(1.0/fx),  Ys = ((y - cy)*depth)*(1.0/fy),
 *               dist = sqrt((Xs*Xs + Ys*Ys) + depth*depth).
 *   visibility  valid = dist_test > 0 and dist_model > 0;  d_diff = float32(dist_model) - float32(dist_test) in binary32;
 *               visib = d_diff <= float32(delta) and valid (visibility.py:6-20).
 *               visib_gt = visib(gt);  visib_est = visib(est) or (visib_gt and dist_est > 0) (:22-29).
 *   cost        on visib_gt and visib_est, binary64: c = |dist_gt - dist_est|.  'step': 1 when c >= tau.
 *               'tlinear': min(c*(1.0/tau), 1.0).
 *   counts      union = #(visib_gt or visib_est), inter = #(visib_gt and visib_est), cost = the sum of the step costs
 *               (counted for either cost type): integers, summed with integer atomics -- exact in any order.
 *   tlinear sum the costs of the H*W pixels in row-major order (0.0 where the pixel is not in the intersection) in tiles
 *               of 256 consecutive pixels, each reduced by a binary tree over its 256 slots (slot j += slot j + 128, then
 *               64, ... 1), the tile sums then added in ascending tile order.  The order depends on H*W only; no atomics
 *               on floats.
 *   error       e = (cost + (union - inter)) / float64(union), and 1.0 when union = 0 (vsd_utils.py:41-48).  With 'step'
 *               everything in front of the division is an integer: e equals the reference bit for bit.
 */
#ifndef PVNET_VSD_H_
#define PVNET_VSD_H_

#include <stddef.h>
#include <stdint.h>

/* cost_type of pvs_vsd_batched */
#define PVS_COST_STEP 0
#define PVS_COST_TLINEAR 1

/* test_kind of pvs_vsd_batched: the element type of the sensor image */
#define PVS_TEST_U16 0   /* uint16: the T-LESS depth PNG as stored */
#define PVS_TEST_F32 1
#define PVS_TEST_F64 2

/* columns of d_counts */
#define PVS_UNION 0
#define PVS_INTER 1
#define PVS_COST 2       /* the pixels of the intersection with c >= tau (the 'step' cost), counted for either cost type */

/* the largest image side either entry point accepts */
#define PVS_MAX_SIDE 16384

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of d_workspace that pvs_render_depth_batched needs: the eye-space and snapped vertices of every pose.  0 for
 * P <= 0 or N <= 0. */
size_t pvs_render_workspace_bytes(int P, int N);

/* Depth images of one triangle mesh at P poses (replaces DepthRender.render, opengl_utils.py:405-492, one OpenGL context
 * and one read-back per pose), on DEVICE pointers, launched on `stream` (hipStream_t as void*).
 *   d_pts    [N,3] float32;   d_faces [F,3] int32;   d_pose [P,3,4] binary64 [R | t]
 *   d_K      [9] row-major, shared when K_batched == 0, else [P,9]
 *   d_depth  [P,H,W] float32, written whole by the call: eye-space Z of the nearest surface, 0 = background
 *   d_workspace  pvs_render_workspace_bytes(P, N) bytes, 16-byte aligned; contents need not survive the call
 *   near, far    0 < near <= far, in the units of the model and of t
 * Arithmetic: the rasteriser contract at the top of this file, the half-pixel offset included.
 * Returns 0 (also for P == 0, nothing launched; F == 0 gives all-zero images), -1 (bad arguments, checked before any
 * launch) or a hipError_t. */
int pvs_render_depth_batched(const float *d_pts, const int32_t *d_faces, const double *d_pose, const double *d_K,
                             float *d_depth, void *d_workspace, int P, int N, int F, int K_batched, int W, int H,
                             double near, double far, void *stream);

/* Bytes of d_workspace that pvs_vsd_batched needs: one binary64 tile sum per (pair, tile of 256 pixels) with
 * PVS_COST_TLINEAR, nothing with PVS_COST_STEP.  0 for an empty batch. */
size_t pvs_vsd_workspace_bytes(int n, int p, int g, int H, int W, int cost_type);

/* The VSD error of the p x g (prediction, ground truth) pairs of each of n images from their depth renders (replaces
 * misc.py:42-60, visibility.py:6-29 and vsd_utils.py:5-48 run per pair on the host, tless_test/pvnet.py:82-101).
 *   d_depth_est  [n,p,H,W] float32 renders of the predicted poses;   d_depth_gt [n,g,H,W] of the ground-truth poses
 *   d_depth_test [n,H,W] of `test_kind`, the sensor image;  depth_scale applies to PVS_TEST_U16 only
 *   d_K          [9] row-major, shared when K_batched == 0, else [n,9]
 *   d_counts     [n,p,g,3] int64, columns PVS_*: written by the call (zeroed on `stream`, then integer atomic adds)
 *   d_e          [n,p,g] binary64, the error
 *   d_workspace  pvs_vsd_workspace_bytes(...) bytes, 16-byte aligned (may be NULL when that is 0)
 * Arithmetic: the VSD contract at the top of this file.
 * Returns 0 (also for an empty batch), -1 (bad arguments, checked before any launch) or a hipError_t. */
int pvs_vsd_batched(const float *d_depth_est, const float *d_depth_gt, const void *d_depth_test, int test_kind,
                    double depth_scale, const double *d_K, int K_batched, double delta, double tau, int cost_type,
                    long long *d_counts, double *d_e, void *d_workspace, int n, int p, int g, int H, int W, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_VSD_H_ */
