"""GPU: float16 / bfloat16 seg and vertex fields go into the voting path as they are (PVV_FLAG_VERTEX_* / PVV_FLAG_SEG_*).
The kernels widen each element as they read it -- exact -- so every output must be bit-identical to the same call on the
`.float()` copy of the field, with the same seed, and stay float32; no float32 copy may appear anywhere."""
import ctypes

import numpy as np
import pytest
import torch

from tests import capi

pytestmark = pytest.mark.gpu

HALF = [torch.float16, torch.bfloat16]
COUNT = ["AUTO", "EXACT", "FULL", "STAGED"]


def same(a, b):
    """bit-identical (NaN payloads included) and the same dtype / shape"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int16), b.contiguous().view(
            torch.int32 if b.element_size() == 4 else torch.int16)
    return torch.equal(a, b)


def layouts(v, dt):
    """the f32 NHWC field -> {name: the same numbers in dtype dt}: NHWC, the planar view of resnet18.py:66-68, and NHWC starting
    at an odd element offset (no aligned pair load: the scalar path)"""
    B, H, W, K, _ = v.shape
    nhwc = v.to(dt)
    planar = v.reshape(B, H, W, 2 * K).permute(0, 3, 1, 2).contiguous().to(dt).permute(0, 2, 3, 1).view(B, H, W, K, 2)
    raw = torch.empty(v.numel() + 1, dtype=dt, device=v.device)
    raw[1:].copy_(v.reshape(-1))
    odd = raw[1:].view(B, H, W, K, 2)
    assert odd.data_ptr() % 4 == 2
    return {"nhwc": nhwc, "planar": planar, "odd": odd}


_DATA = {}


def batch(synth, gpu, name):
    if name not in _DATA:
        cfg = synth.CONFIGS[name]
        _DATA[name] = synth.make_batch(**cfg, device=gpu)
    return _DATA[name]


@pytest.mark.parametrize("dt", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_layer_v3_every_count_kernel_and_layout(synth, pkg, gpu, cfg, dt):
    from clean_pvnet_amd import ransac_voting as ext
    d = batch(synth, gpu, cfg)
    mask, v = d["mask"], d["vertex"]
    B = v.shape[0]
    for lname, vh in layouts(v, dt).items():
        vf = vh.float()
        for ck in COUNT:
            kc = getattr(ext, "COUNT_" + ck)
            got, want = [], []
            for field, res in ((vh, got), (vf, want)):
                st = torch.full((B,), -1, dtype=torch.int32, device=gpu)
                out, win, tn, _ws = ext.ransac_voting_v3(mask, field, 512, 0.99, 5, 30000, None, None, 1234, ext.SINGULAR_REFERENCE,
                                                         0, kc, st)
                res += [out, win, tn, st]
            assert got[0].dtype == torch.float32
            assert all(same(a, b) for a, b in zip(got, want)), (cfg, lname, ck, dt)


@pytest.mark.parametrize("dt", HALF, ids=["f16", "bf16"])
def test_python_layers_v3_and_v1(synth, pkg, gpu, dt):
    from clean_pvnet_amd.ransac_voting_gpu import ransac_voting_layer, ransac_voting_layer_v3
    for cfg in ("cfg2", "cfg3"):
        d = batch(synth, gpu, cfg)
        for lname, vh in layouts(d["vertex"], dt).items():
            for layer in (ransac_voting_layer_v3, ransac_voting_layer):
                got = layer(d["mask"], vh, 512, 0.99, seed=99)
                want = layer(d["mask"], vh.float(), 512, 0.99, seed=99)
                assert got.dtype == torch.float32 and same(got, want), (cfg, lname, layer.__name__)


@pytest.mark.parametrize("dt", HALF, ids=["f16", "bf16"])
def test_estimate_with_hypotheses(synth, pkg, gpu, dt):
    from clean_pvnet_amd.ransac_voting_gpu import estimate_voting_distribution_with_mean, ransac_voting_layer_v3
    for cfg, B in (("cfg2", 1), ("cfg3", 8)):
        d = batch(synth, gpu, cfg)
        mask, v = d["mask"][:B], d["vertex"][:B]
        for lname, vh in layouts(v, dt).items():
            mean = ransac_voting_layer_v3(mask, vh.float(), 512, 0.99, seed=5)
            got = estimate_voting_distribution_with_mean(mask, vh, mean, output_hyp=True, return_weights=True, seed=6)
            want = estimate_voting_distribution_with_mean(mask, vh.float(), mean, output_hyp=True, return_weights=True, seed=6)
            assert all(g.dtype == torch.float32 for g in got[1:])
            assert all(same(g, w) for g, w in zip(got, want)), (cfg, lname)


def network_output(synth, gpu, B, H, W, K, dt, seed, C=2, seg_stride=1):
    """the real caller's layout: seg and vertex as channel slices of ONE [B, C*seg_stride + 2K, H, W] tensor of dtype dt, with
    torch.argmax's corner cases (NaN, ties) at tile starts / ends (the pattern of test_gpu_decode_layout.py)"""
    d = synth.make_batch(B=B, H=H, W=W, K=K, fg=0.06, sigma=0.05, seed=seed, planar=True, device=gpu)
    g = torch.Generator(device=gpu).manual_seed(seed)
    x = torch.empty(B, C * seg_stride + 2 * K, H, W, device=gpu)
    seg = x[:, 0:C * seg_stride:seg_stride]
    seg.copy_(torch.randn(B, C, H, W, generator=g, device=gpu) * 0.1)
    seg[:, 0] += 1.0
    seg[:, 1][d["mask"] != 0] += 4.0
    pts = [0, 1, 2047, 2048, 4095, H * W - 1, H * W - 2, H * W // 2 + 3]
    for i, p in enumerate(pts):
        if not 0 <= p < H * W:
            continue
        y, xx = divmod(p, W)
        b = i % B
        if i % 4 == 0:
            seg[b, 0, y, xx] = float("nan")
        elif i % 4 == 1:
            seg[b, 1, y, xx] = float("nan")
        elif i % 4 == 2:
            seg[b, :, y, xx] = float("nan")
        else:
            seg[b, :, y, xx] = 0.75
    x[:, C * seg_stride:].copy_(d["vertex"].permute(0, 3, 4, 1, 2).reshape(B, 2 * K, H, W))
    x = x.to(dt)
    return x[:, 0:C * seg_stride:seg_stride], x[:, C * seg_stride:]


@pytest.mark.parametrize("dt", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("B", [64, 1])
def test_decode_keypoint_on_the_network_layout(synth, pkg, gpu, B, dt):
    from clean_pvnet_amd.decode import decode_keypoint
    seg, ver = network_output(synth, gpu, B, 480, 640, 9, dt, seed=70 + B)
    for un_pnp in (False, True):
        got = decode_keypoint({"seg": seg, "vertex": ver}, un_pnp=un_pnp, weights=un_pnp, seed=31)
        want = decode_keypoint({"seg": seg.float(), "vertex": ver.float()}, un_pnp=un_pnp, weights=un_pnp, seed=31)
        assert same(got["mask"], torch.argmax(seg, 1)) and same(got["mask"], want["mask"])
        keys = ["kpt_2d"] + (["var", "var_weights"] if un_pnp else [])
        for k in keys:
            assert got[k].dtype == torch.float32 and same(got[k], want[k]), (B, un_pnp, k)


GENERIC = [
    # B, H, W, C, channels_last, what: none of these is two aligned contiguous planes -> k_tile_scan with the argmax inside
    (3, 96, 128, 3, False, "three classes"),
    (3, 96, 128, 2, True, "strided seg: channels last"),
    (2, 97, 131, 2, False, "H*W not a multiple of 4 (or 8)"),
]


@pytest.mark.parametrize("dt", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("B,H,W,C,channels_last,what", GENERIC, ids=[c[-1] for c in GENERIC])
def test_generic_scan_path(synth, pkg, gpu, B, H, W, C, channels_last, what, dt):
    from clean_pvnet_amd import ransac_voting as ext
    seg, ver = network_output(synth, gpu, B, H, W, 3, dt, seed=H + C, C=C)
    if channels_last:
        seg = seg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert seg.stride(3) == C
    vertex = ver.permute(0, 2, 3, 1).view(B, H, W, 3, 2)
    for max_num in (30000, 150):
        got = ext.decode_keypoint_v3(seg, vertex, 64, 0.99, 5, max_num, None, None, 11, ext.SINGULAR_REFERENCE)
        want = ext.decode_keypoint_v3(seg.float(), vertex.float(), 64, 0.99, 5, max_num, None, None, 11, ext.SINGULAR_REFERENCE)
        assert same(got[1], torch.argmax(seg, 1)), what
        assert all(same(g, w) for g, w in zip(got, want)), (what, max_num)


def test_mixed_dtypes(synth, pkg, gpu):
    from clean_pvnet_amd.decode import decode_keypoint
    seg, ver = network_output(synth, gpu, 4, 480, 640, 9, torch.float32, seed=5)
    for s, v in ((seg.to(torch.bfloat16), ver), (seg, ver.to(torch.float16)), (seg.to(torch.float16), ver.to(torch.bfloat16))):
        for un_pnp in (False, True):
            got = decode_keypoint({"seg": s, "vertex": v}, un_pnp=un_pnp, weights=un_pnp, seed=8)
            want = decode_keypoint({"seg": s.float(), "vertex": v.float()}, un_pnp=un_pnp, weights=un_pnp, seed=8)
            for k in ("mask", "kpt_2d") + (("var", "var_weights") if un_pnp else ()):
                assert same(got[k], want[k]), (s.dtype, v.dtype, un_pnp, k)


def test_adversarial_values(synth, pkg, gpu):
    """fp16 subnormals, NaN and +-inf in the vertex field at foreground pixels; NaN / tie logits at tile boundaries (above)"""
    from clean_pvnet_amd import ransac_voting as ext
    B, H, W, K = 2, 480, 640, 4
    seg, ver = network_output(synth, gpu, B, H, W, K, torch.float16, seed=3)
    fg = torch.nonzero(torch.argmax(seg, 1)[0].flatten()).flatten()
    ver = ver.clone()
    sub = torch.tensor([2.0 ** -24, -(2.0 ** -20), 3 * 2.0 ** -17, -(2.0 ** -15)], dtype=torch.float16, device=gpu)
    special = torch.tensor([float("nan"), float("inf"), -float("inf")], dtype=torch.float16, device=gpu)
    flat = ver[0].reshape(2 * K, H * W)
    for i, p in enumerate(fg[:400].tolist()):
        flat[i % (2 * K), p] = sub[i % 4]
    for i, p in enumerate(fg[400:409].tolist()):
        flat[i % (2 * K), p] = special[i % 3]
    assert bool(((ver[0].abs() < 2.0 ** -14) & (ver[0] != 0)).any()) and bool(torch.isnan(ver[0]).any()) and bool(torch.isinf(ver[0]).any())
    vertex = ver.permute(0, 2, 3, 1).view(B, H, W, K, 2)
    for count_kernel in (ext.COUNT_AUTO, ext.COUNT_EXACT):
        got = ext.decode_keypoint_v3(seg, vertex, 128, 0.99, 5, 30000, None, None, 2, ext.SINGULAR_REFERENCE, 0, count_kernel)
        want = ext.decode_keypoint_v3(seg.float(), vertex.float(), 128, 0.99, 5, 30000, None, None, 2, ext.SINGULAR_REFERENCE, 0,
                                      count_kernel)
        assert same(got[1], torch.argmax(seg, 1))
        assert all(same(g, w) for g, w in zip(got, want))
        mask = got[1]
        for dt in HALF:
            vh = vertex.to(dt) if dt != torch.float16 else vertex
            a = ext.ransac_voting_v3(mask, vh, 128, 0.99, 5, 30000, None, None, 2, ext.SINGULAR_REFERENCE, 0, count_kernel)
            b = ext.ransac_voting_v3(mask, vh.float(), 128, 0.99, 5, 30000, None, None, 2, ext.SINGULAR_REFERENCE, 0, count_kernel)
            assert all(same(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("dt", HALF, ids=["f16", "bf16"])
def test_against_the_cpu_oracle(synth, pkg, gpu, oracle, dt):
    from clean_pvnet_amd.ransac_voting_gpu import ransac_voting_layer_v3
    from clean_pvnet_amd import ransac_voting as ext
    cfg = {**synth.CONFIGS["cfg1"], "B": 2}
    d = synth.make_batch(**cfg)
    mask, vh = d["mask"], d["vertex"].to(dt)
    tn = [int(x) for x in (mask != 0).sum((1, 2))]
    idxs = synth.make_idxs(tn, cfg["hn"], cfg["K"])
    m, v, i = mask.to(gpu), vh.to(gpu), idxs.to(gpu)
    out = ransac_voting_layer_v3(m, v, cfg["hn"], inlier_thresh=0.99, idxs=i)
    _o, win, tnn, _ws = ext.ransac_voting_v3(m, v, cfg["hn"], 0.99, 5, 30000, i, None, 0, ext.SINGULAR_REFERENCE)
    det = []
    want = oracle.ransac_voting_layer_v3(mask.numpy(), vh.float().numpy(), cfg["hn"], 0.99, idxs=idxs.numpy(), details=det)
    assert tnn.cpu().tolist() == tn
    assert np.array_equal(win.cpu().numpy(), np.stack([r["win_counts"] for r in det]))
    assert float(np.abs(out.cpu().numpy() - want).max()) <= 1e-4


@pytest.mark.parametrize("dt,vbit,sbit", [(torch.float16, 2, 8), (torch.bfloat16, 4, 16)], ids=["f16", "bf16"])
def test_c_abi_with_raw_2byte_pointers(synth, pkg, gpu, dt, vbit, sbit):
    L = capi.load()
    B, H, W, K, hn = 4, 480, 640, 9, 512
    seg, ver = network_output(synth, gpu, B, H, W, K, dt, seed=21)
    vh = ver.permute(0, 2, 3, 1).view(B, H, W, K, 2)
    mask = torch.argmax(seg, 1)
    res = {}
    for name, v, s, flags in (("half", vh, seg, (vbit, sbit)), ("f32", vh.float(), seg.float(), (0, 0))):
        draws = torch.empty(B, K, hn, 2, dtype=torch.int32, device=gpu)
        out, win, tn = capi.v3(mask, v, hn, 0.99, seed=9, flags=1 | flags[0], draws_out=draws)
        # pvv_decode_keypoint_v3: the seg bit applies to d_seg
        p = capi.problem(mask, v, hn, 0.99, seed=9, flags=1 | flags[0] | flags[1])
        p.seg_classes = 2
        p.seg_stride[:] = s.stride()
        n = L.pvv_workspace_bytes(ctypes.byref(p))
        assert n > 0, L.pvv_last_error()
        ws = torch.empty(n, dtype=torch.uint8, device=gpu)
        mo = torch.empty(B, H, W, dtype=torch.int64, device=gpu)
        o2 = torch.empty(B, K, 2, device=gpu)
        w2 = torch.empty(B, K, dtype=torch.int32, device=gpu)
        t2 = torch.empty(B, dtype=torch.int32, device=gpu)
        capi.check(L.pvv_decode_keypoint_v3(ctypes.byref(p), capi.ptr(s), capi.ptr(v), None, None, capi.ptr(ws), n, capi.ptr(mo),
                                            capi.ptr(o2), capi.ptr(w2), capi.ptr(t2), capi.stream()))
        res[name] = [out, win, tn, draws, mo, o2, w2, t2]
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(res["half"], res["f32"]))
    assert same(res["half"][4], mask)


def test_no_fp32_copy_of_either_field(synth, pkg, gpu):
    """peak memory of a cfg3 B = 64 bf16 decode_keypoint call grows by no more than the workspace + outputs + 1 MB (an fp32 copy
    of seg alone would be 157 MB, of the vertex field 1.4 GB); the workspace is the same size for every dtype"""
    from clean_pvnet_amd import ransac_voting as ext
    from clean_pvnet_amd.decode import decode_keypoint
    L = capi.load()
    B, H, W, K = 64, 480, 640, 9
    seg, ver = network_output(synth, gpu, B, H, W, K, torch.bfloat16, seed=64)
    vertex = ver.permute(0, 2, 3, 1).view(B, H, W, K, 2)
    mask = torch.empty(B, H, W, dtype=torch.int64, device=gpu)
    outputs = B * H * W * 8 + B * K * (2 + 4 + 3 + 1) * 4 + B * 4
    for un_pnp in (False, True):
        if un_pnp:
            p = capi.problem(mask, vertex, 512, 0.99, max_num=30000, flags=1)
            wsb = L.pvv_workspace_bytes_un_pnp(ctypes.byref(p), 4096)
        else:
            wsb = ext.workspace_bytes(B, H, W, K, 128, max_num=100, mask_elem_size=8, device_rng=True)
        assert wsb > 0
        decode_keypoint({"seg": seg, "vertex": ver}, un_pnp=un_pnp, weights=un_pnp, seed=1)     # warm: allocator state
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = decode_keypoint({"seg": seg, "vertex": ver}, un_pnp=un_pnp, weights=un_pnp, seed=1)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - base
        assert grew <= wsb + outputs + (1 << 20), (un_pnp, grew, wsb, outputs)
        del out
    m = torch.argmax(seg, 1)
    sizes = {dt: ext.ransac_voting_v3(m, vertex.to(dt), 512, 0.99, 5, 30000, None, None, 3, ext.SINGULAR_REFERENCE)[3].numel()
             for dt in (torch.float32, torch.float16, torch.bfloat16)}
    assert len(set(sizes.values())) == 1, sizes


def test_dtype_rules(synth, pkg, gpu):
    from clean_pvnet_amd import ransac_voting as ext
    from clean_pvnet_amd.decode import decode_keypoint
    from clean_pvnet_amd.ransac_voting_gpu import estimate_voting_distribution_with_mean, ransac_voting_layer, ransac_voting_layer_v3
    d = synth.make_batch(**synth.CONFIGS["cfg1"], device=gpu)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        ransac_voting_layer_v3(d["mask"], d["vertex"].double(), 64, 0.99)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        ext.decode_keypoint_v3(torch.zeros(1, 2, 128, 128, dtype=torch.float64, device=gpu), d["vertex"], 64, 0.99, 5, 100, None,
                               None, 1, ext.SINGULAR_REFERENCE)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        for B in (1, 0):
            mask, v = d["mask"][:B], d["vertex"][:B].to(dt)
            mean = ransac_voting_layer_v3(mask, v, 64, 0.99)
            assert mean.dtype == torch.float32 and ransac_voting_layer(mask, v, 64, 0.99).dtype == torch.float32
            est = estimate_voting_distribution_with_mean(mask, v, mean, output_hyp=True, return_weights=True)
            assert all(t.dtype == torch.float32 for t in est), (dt, B, [t.dtype for t in est])
            out = decode_keypoint({"seg": torch.zeros(B, 2, 128, 128, dtype=dt, device=gpu),
                                   "vertex": torch.zeros(B, 8, 128, 128, dtype=dt, device=gpu)}, un_pnp=True, weights=True)
            assert out["mask"].dtype == torch.int64
            assert all(out[k].dtype == torch.float32 for k in ("kpt_2d", "var", "var_weights")), (dt, B)
