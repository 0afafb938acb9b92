"""Detector heat maps -> boxes -> PVNet crops, and the crops' keypoints and masks back onto the image, on the device
(``libpvnet_vote.so``, the last section of include/pvnet_vote.h).

The reference's detector -> crop -> PVNet path decodes the detector's heat maps with ``decode_ct_hm``
(lib/utils/ct/ct_decode.py:52-75, lib/networks/ct/dla.py:20-26), copies the image to the host, runs ``cv2.warpAffine`` once per
box, normalises in numpy and copies each crop back (lib/networks/ct_pvnet/res.py:14-60; the T-LESS test loader adds a box
blanking step, lib/utils/tless/tless_test_utils.py:57-79).  Behind the network its evaluator maps the keypoints back with an
inverse affine on the host and warps the crop's segmentation onto the 720 x 540 canvas with ``cv2.warpAffine(INTER_NEAREST)``
(lib/evaluators/tless_test/pvnet.py:229-245).  The four functions here are those steps for a batch: CUDA tensors in and out, the
current stream, nothing read back, no state.  ``uncrop_keypoints`` feeds ``pose.pose_batched`` / ``pose.solve_pose`` and
``uncrop_mask`` feeds ``icp.icp_refine(mask=...)`` as they are.  Each equals its numpy twin (tests/crop_twin.py) bit for bit;
parity of the two warps with ``cv2.warpAffine`` is unpinned.  There is no CPU fallback.
"""
import ctypes

from . import _native

_lib = _native.bind("crop", "libpvnet_vote.so", last_error="pvv_last_error", prefix="crop", plain_calls=True)

MAX_K = 256                        # PVV_CT_MAX_K
_WORKSPACE_PER_BOX = 96            # PVV_CROP_WORKSPACE_PER_BOX
_MAX_BOXES = 65535                 # per launch


def decode_ct_hm(ct_hm, wh, K=100, clip=True):
    """``decode_ct_hm(ct_hm, wh, K=K)`` without ``ae`` (ct_decode.py:52-75), then ``clip_to_image`` with the heat map's own size
    when ``clip`` (data_utils.py:373-377, as dla.py:24 calls it).
    :param ct_hm:  [B,C,H,W] float32 CUDA tensor, after the sigmoid (finite, >= 0)
    :param wh:     [B,2,H,W] float32
    :return:       ct [B,K,2] float32 (x, y), detection [B,K,6] float32 (x0, y0, x1, y1, value, class), count [B] int32
    A peak is a pixel not smaller than any of its 8 neighbours inside its class plane, a candidate a peak > 0.  The rows are an
    image's ``K`` candidates by descending value, the lower ``c*H*W + y*W + x`` first among equals -- the reference's rows
    whenever the top ``K + 1`` values are distinct.  ``count = min(K, candidates)``; the rows from there on are zeros."""
    import torch
    _native.need_cuda(ct_hm, "ct_hm", "crop")
    _native.need_cuda(wh, "wh", "crop")
    if ct_hm.dtype != torch.float32 or wh.dtype != torch.float32:
        raise TypeError("crop: ct_hm and wh must be float32, got %s and %s" % (ct_hm.dtype, wh.dtype))
    B, C, H, W = ct_hm.shape
    assert tuple(wh.shape) == (B, 2, H, W), (ct_hm.shape, wh.shape)
    K = int(K)
    if not 1 <= K <= MAX_K or K > H * W:
        raise ValueError("crop: K must lie in [1, min(%d, H*W = %d)], got %d" % (MAX_K, H * W, K))
    dev = ct_hm.device
    hm, whc = ct_hm.contiguous(), wh.contiguous()
    ct = torch.empty(B, K, 2, dtype=torch.float32, device=dev)
    det = torch.empty(B, K, 6, dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    if B:
        ws, _ = _lib.workspace("pvv_ct_workspace_bytes", dev, B, C, H, W, K)
        _lib.call("pvv_ct_decode", dev, hm.data_ptr(), whc.data_ptr(), B, C, H, W, K, int(bool(clip)), ws.data_ptr(),
                  ws.numel(), ct.data_ptr(), det.data_ptr(), count.data_ptr())
    return ct, det, count


def crop_boxes(img, boxes, image_index, out_size, *, scale_ratio, box_ratio=None, mean, std):
    """``_crop`` / ``pvnet_transform`` (ct_pvnet/res.py:14-32, tless_test_utils.py:57-79) for ``N`` boxes.
    :param img:          [B,H,W,3] uint8 CUDA tensor, channels as stored
    :param boxes:        [N,4] float32 or float64 (x0, y0, x1, y1) in ``img`` pixels
    :param image_index:  [N] int32 / int64, the image each box is cut from
    :param out_size:     (ow, oh)
    :param scale_ratio:  ``tless_config.scale_ratio``
    :param box_ratio:    ``tless_config.box_ratio`` for the test loader's blanking (tless_test_utils.py:65-69), None for none
    :param mean, std:    3 floats each
    :return: dict: ``inp`` [N,3,oh,ow] float32, ``center`` [N,2] float32, ``scale`` [N] float32, ``trans`` [N,2,3] float64
             (image -> crop) and ``valid`` [N] bool.  A box with a non-finite entry, a scale <= 0 or an ``image_index`` outside
             the batch is not valid: its centre, scale and ``trans`` are zeros and its crop is normalised zeros."""
    import torch
    for t, what in ((img, "img"), (boxes, "boxes"), (image_index, "image_index")):
        _native.need_cuda(t, what, "crop")
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
        raise TypeError("crop: img must be [B,H,W,3] uint8, got %s %s" % (tuple(img.shape), img.dtype))
    if boxes.dtype not in (torch.float32, torch.float64):
        raise TypeError("crop: boxes must be float32 or float64, got %s" % boxes.dtype)
    if image_index.dtype not in (torch.int32, torch.int64):
        raise TypeError("crop: image_index must be int32 or int64, got %s" % image_index.dtype)
    ow, oh = (int(v) for v in out_size)
    N = boxes.shape[0]
    assert tuple(boxes.shape) == (N, 4) and tuple(image_index.shape) == (N,), (boxes.shape, image_index.shape)
    mean_c, std_c = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    dev = img.device
    B, H, W = (int(v) for v in img.shape[:3])
    im = img.contiguous()
    bx = boxes.to(torch.float64).contiguous()                                    # (a float32 is a binary64: nothing is rounded)
    ix = image_index.clamp(-1, B).to(torch.int32).contiguous()
    out = {"inp": torch.empty(N, 3, oh, ow, dtype=torch.float32, device=dev), "center": torch.empty(N, 2, dtype=torch.float32, device=dev),
           "scale": torch.empty(N, dtype=torch.float32, device=dev), "trans": torch.empty(N, 2, 3, dtype=torch.float64, device=dev),
           "valid": torch.empty(N, dtype=torch.bool, device=dev)}
    for lo in range(0, N, _MAX_BOXES):
        n = min(N - lo, _MAX_BOXES)
        ws = _native.workspace(n * _WORKSPACE_PER_BOX, dev)
        _lib.call("pvv_crop_boxes", dev, im.data_ptr(), B, H, W, bx[lo:].data_ptr(), ix[lo:].data_ptr(), n, ow, oh,
                  float(scale_ratio), int(box_ratio is not None), float(box_ratio or 0.0), mean_c, std_c, ws.data_ptr(), ws.numel(),
                  out["inp"][lo:].data_ptr(), out["center"][lo:].data_ptr(), out["scale"][lo:].data_ptr(),
                  out["trans"][lo:].data_ptr(), out["valid"][lo:].data_ptr())
    return out


def uncrop_keypoints(kpt_2d, trans):
    """Crop pixels -> image pixels (tless_test/pvnet.py:233-234): ``trans`` [N,2,3] float64 of ``crop_boxes`` inverted and applied
    in binary64.  ``kpt_2d`` [N,K,2] float32 or float64; returns [N,K,2] float64.  ``var`` needs no transform for PnP: the map is
    an isotropic scale without rotation, so the minimiser is unchanged (the reference does not transform it either)."""
    import torch
    _native.need_cuda(kpt_2d, "kpt_2d", "crop")
    _native.need_cuda(trans, "trans", "crop")
    if kpt_2d.dtype not in (torch.float32, torch.float64):
        raise TypeError("crop: kpt_2d must be float32 or float64, got %s" % kpt_2d.dtype)
    N, K = kpt_2d.shape[0], kpt_2d.shape[1]
    assert tuple(kpt_2d.shape) == (N, K, 2) and tuple(trans.shape) == (N, 2, 3) and trans.dtype == torch.float64, (kpt_2d.shape, trans.shape)
    kp, tr = kpt_2d.contiguous(), trans.contiguous()
    out = torch.empty(N, K, 2, dtype=torch.float64, device=kp.device)
    if N and K:
        _lib.call("pvv_uncrop_keypoints", kp.device, kp.data_ptr(), int(kp.dtype == torch.float64), tr.data_ptr(), N, K, out.data_ptr())
    return out


def uncrop_mask(mask, trans, canvas_size):
    """The crops' masks on the canvas (tless_test/pvnet.py:243-245): nearest neighbour with ``trans`` [N,2,3] (canvas -> crop, as
    ``crop_boxes`` returns it) as the destination -> source map, 0 outside the crop.
    :param mask:         [N,h,w] uint8, bool or int64 with values in [0, 255] (``decode_keypoint``'s ``mask``)
    :param canvas_size:  (Wc, Hc)
    :return:             [N,Hc,Wc] uint8"""
    import torch
    _native.need_cuda(mask, "mask", "crop")
    _native.need_cuda(trans, "trans", "crop")
    if mask.dtype not in (torch.uint8, torch.bool, torch.int64):
        raise TypeError("crop: mask has dtype %s, supported are uint8, bool and int64" % mask.dtype)
    m = _native.u8(mask)
    Wc, Hc = (int(v) for v in canvas_size)
    N, h, w = m.shape
    assert tuple(trans.shape) == (N, 2, 3) and trans.dtype == torch.float64, (trans.shape, trans.dtype)
    tr = trans.contiguous()
    out = torch.empty(N, Hc, Wc, dtype=torch.uint8, device=m.device)
    for lo in range(0, N, _MAX_BOXES):
        n = min(N - lo, _MAX_BOXES)
        _lib.call("pvv_uncrop_mask", m.device, m[lo:].data_ptr(), m.element_size(), h, w, tr[lo:].data_ptr(), n, Hc, Wc, out[lo:].data_ptr())
    return out
