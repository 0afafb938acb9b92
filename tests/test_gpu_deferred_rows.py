"""Rows the first count launch gathers itself (compaction.hpp: HypArgs.defer_mask; count_bf16.hpp: gather blocks).

A v3 call counted in stages leaves the ``dirs`` rows of a staged, unsubsampled image that lie outside the first launch's chunks to gather
blocks of that launch's grid (behind its first resident generation of count blocks).  Nothing a caller sees may change, and once the
call has completed the workspace holds what the full pass leaves: keypoints, winner counts and tn equal those of COUNT_FULL and COUNT_EXACT bit for bit (tests/test_gpu_staged.py's
rule), ``coords`` and ``dirs`` below tn equal the full pass's byte for byte -- for both vertex layouts, the half-precision fields and
two mask types --, and graph replay, the decode paths and ``rerun_count_kernel`` see no difference.

One batch, 96 x 128, K = 3, hn = 128, max_num = 6000 (cap = 6683 rows: 13 chunks), side by side: a normal image (5530 rows: 11 chunks),
8 chunks + 1 row (its last chunk is a rest chunk of one row), a multiple of 512, an image below 8 chunks (counted completely by the
first launch: never deferred), an empty one, one below min_num, and one with 9000 foreground pixels (subsampled: staged, never
deferred).  With injected index pairs the subsampling is k_tile_subsample's, with the device RNG it is fused into k_compact_hyp.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, K, HN, MAX_NUM, SEED = 96, 128, 3, 128, 6000, 17
ROWS = (5530, 8 * 512 + 1, 10 * 512, 3000, 0, 3, 9000)
DEFERRED = (1, 1, 1, 0, 0, 0, 0)


def _field(B, h, w, k, seed):
    """[B,h,w,k,2] unit directions towards k keypoints per image, 0.02 rad of noise; defined on every pixel."""
    g = torch.Generator().manual_seed(seed)
    kpt = torch.rand(B, k, 2, generator=g) * torch.tensor([w, h], dtype=torch.float32)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    d = kpt[:, None, None] - torch.stack([xs, ys], -1)[None, :, :, None]
    ang = torch.atan2(d[..., 1], d[..., 0]) + 0.02 * torch.randn(B, h, w, k, generator=g)
    return torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous()


def _masks(rows, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(len(rows), h * w, dtype=torch.int64)
    for i, n in enumerate(rows):
        m[i, torch.randperm(h * w, generator=g)[:n]] = 1
    return m.view(len(rows), h, w)


@functools.lru_cache(maxsize=None)
def _batch():
    mask, vertex = _masks(ROWS, H, W, SEED), _field(len(ROWS), H, W, K, SEED + 1)
    g = torch.Generator().manual_seed(SEED + 2)
    idxs = torch.randint(0, 2900, (len(ROWS), HN, K, 2), generator=g, dtype=torch.int32)      # (rows beyond tn are clamped)
    return mask, vertex, idxs


def _v3(ext, mask, vertex, ck, idxs=None, hn=HN, max_num=MAX_NUM):
    return ext.ransac_voting_v3(mask, vertex, hn, 0.99, 5, max_num, idxs, None, SEED, ext.SINGULAR_ZERO, count_kernel=ck)


def _rows(ext, ws, shape, ck, device_rng, tn, max_num=MAX_NUM):
    """(coords rows, dirs rows, deferred flags) of a completed call's workspace, the rows below tn as int32 bit patterns per image."""
    B, h, w, k, hn = shape
    L = ext.workspace_layout(B, h, w, k, hn, max_num, 8, ck, device_rng)
    assert L["total"] == ws.numel()
    cap = L["cap"]
    coords = ws[L["coords"]:L["coords"] + B * cap * 8].view(torch.int32).view(B, cap, 2).cpu()
    dirs = ws[L["dirs"]:L["dirs"] + B * k * cap * 8].view(torch.int32).view(B, k, cap, 2).cpu()
    flags = ws[L["deferred"]:L["deferred"] + 4 * B].view(torch.int32).cpu().tolist() if L["deferred"] else None
    return [coords[b, :tn[b]] for b in range(B)], [dirs[b, :, :tn[b]] for b in range(B)], flags


def _same_results(a, b, what):
    for x, y, nm in zip(a[:3], b[:3], ("keypoints", "winner counts", "tn")):
        assert torch.equal(x, y), (what, nm)


def _same_rows(ext, staged, full, shape, device_rng, what, max_num=MAX_NUM):
    tn = full[2].cpu().tolist()
    cs, ds, flags = _rows(ext, staged[3], shape, ext.COUNT_STAGED, device_rng, tn, max_num)
    cf, df, none = _rows(ext, full[3], shape, ext.COUNT_FULL, device_rng, tn, max_num)
    assert none is None
    for b in range(shape[0]):
        assert torch.equal(cs[b], cf[b]), (what, "coords", b)
        assert torch.equal(ds[b], df[b]), (what, "dirs", b, int((ds[b] != df[b]).any(-1).sum()))
    return flags


def _planar(vertex):
    """The view resnet18.py:66-68 hands over: [B,2K,h,w] storage, permuted to [B,h,w,K,2]."""
    B, h, w, k, _ = vertex.shape
    x = vertex.permute(0, 3, 4, 1, 2).reshape(B, 2 * k, h, w).contiguous()
    return x.permute(0, 2, 3, 1).view(B, h, w, k, 2)


@pytest.mark.parametrize("inject", [True, False], ids=["injected_idxs", "device_rng"])
@pytest.mark.parametrize("layout,dtype,mask_dtype", [
    ("contiguous", "float32", "int64"), ("planar", "float32", "int64"), ("contiguous", "float16", "bool"),
    ("planar", "bfloat16", "int64"), ("planar", "float16", "int64"), ("contiguous", "bfloat16", "bool")])
def test_staged_call_with_deferred_rows_equals_the_full_and_exact_passes(pkg, gpu, layout, dtype, mask_dtype, inject):
    from clean_pvnet_amd import ransac_voting as ext
    mask, vertex, idxs = _batch()
    m = mask.to(getattr(torch, mask_dtype)).to(gpu)
    v = vertex.to(getattr(torch, dtype)).to(gpu)
    if layout == "planar":
        v = _planar(v)
        assert not v.is_contiguous()
    i = idxs.to(gpu) if inject else None
    full, exact = _v3(ext, m, v, ext.COUNT_FULL, i), _v3(ext, m, v, ext.COUNT_EXACT, i)
    _same_results(full, exact, "full vs exact")
    tn = full[2].cpu().tolist()
    # (3 pixels < min_num: skipped, tn = 0; the subsampled image keeps about max_num rows, still eight chunks and below cap)
    assert tn[:6] == list(ROWS[:5]) + [0] and 8 * 512 < tn[6] < 6683 and abs(tn[6] - MAX_NUM) < 6 * MAX_NUM ** 0.5
    shape = (len(ROWS), H, W, K, HN)
    for rep in range(2):
        staged = _v3(ext, m, v, ext.COUNT_STAGED, i)
        _same_results(staged, full, "staged vs full, call %d" % rep)
        flags = _same_rows(ext, staged, full, shape, not inject, (layout, dtype, mask_dtype, inject, rep))
        assert flags == list(DEFERRED)


def test_more_than_64_images(pkg, gpu):
    """70 images of 64 x 96, K = 2 (the gather blocks' table is built 64 images per round): 4608 rows = 9 chunks, every seventh image
    below 8 chunks, one empty."""
    from clean_pvnet_amd import ransac_voting as ext
    B, h, w, k = 70, 64, 96, 2
    rows = [3000 if b % 7 == 0 else 4608 - 5 * b for b in range(B)]
    rows[33] = 0
    m, v = _masks(rows, h, w, SEED + 5).to(gpu), _field(B, h, w, k, SEED + 6).to(gpu)
    full = _v3(ext, m, v, ext.COUNT_FULL, max_num=30000)
    _same_results(full, _v3(ext, m, v, ext.COUNT_EXACT, max_num=30000), "full vs exact")
    assert full[2].cpu().tolist() == rows
    staged = _v3(ext, m, v, ext.COUNT_STAGED, max_num=30000)
    _same_results(staged, full, "staged vs full")
    flags = _same_rows(ext, staged, full, (B, h, w, k, HN), True, "70 images", max_num=30000)
    assert flags == [1 if n > 7 * 512 else 0 for n in rows]


def test_eighth_schedule_rows(synth, pkg, gpu):
    """The eighth first stage (mask 0x02: the gather blocks fetch seven chunks of eight).  A forced COUNT_STAGED call picks it from
    K * B * H * W * 0.02 / 512 chunks per block slot of the second launch >= 5.8 (host_count.hpp: stage_schedule), whatever the masks
    hold: 480 x 640, K = 9 needs B >= 70 at 256 CUs; 72 images of config 3 (6144 rows = 12 chunks each), hn = 128."""
    from clean_pvnet_amd import ransac_voting as ext
    B, K = 72, 9
    d = synth.make_batch(**{**synth.CONFIGS["cfg3"], "B": B}, seed=SEED + 9, device=gpu)
    m, v = d["mask"], d["vertex"]
    full = _v3(ext, m, v, ext.COUNT_FULL, max_num=30000)
    tn = full[2].cpu().tolist()
    assert sum(n > 7 * 512 for n in tn) > B // 2
    staged = _v3(ext, m, v, ext.COUNT_STAGED, max_num=30000)
    _same_results(staged, full, "staged vs full")
    flags = _same_rows(ext, staged, full, (B, 480, 640, K, HN), True, "eighth schedule", max_num=30000)
    assert flags == [1 if n > 7 * 512 else 0 for n in tn]


def test_graph_replay_decode_paths_and_rerun(pkg, gpu):
    from clean_pvnet_amd import ransac_voting as ext
    mask, vertex, _idxs = _batch()
    B = len(ROWS)
    m, v = mask.to(gpu), vertex.to(gpu)
    full = _v3(ext, m, v, ext.COUNT_FULL)
    torch.cuda.synchronize()
    # capture and replay
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _v3(ext, m, v, ext.COUNT_STAGED)
        with torch.cuda.graph(g, stream=s):
            got = _v3(ext, m, v, ext.COUNT_STAGED)
    for _ in range(2):
        got[0].zero_()
        got[3].fill_(0xFF)                                             # (every workspace word the replay reads, it writes first)
        g.replay()
    torch.cuda.synchronize()
    _same_results(got, full, "graph replay")
    assert _same_rows(ext, got, full, (B, H, W, K, HN), True, "graph replay") == list(DEFERRED)
    # rerun_count_kernel on the workspace a deferred call returned (a workspace with the staged tail is re-run in stages: the shim
    # checks its size): nothing is gathered again, every row is there, and the pass finds the winners' counts again
    staged = _v3(ext, m, v, ext.COUNT_STAGED)
    L = ext.workspace_layout(B, H, W, K, HN, MAX_NUM, 8, ext.COUNT_STAGED, True)
    counts = lambda ws: ws[L["counts"]:L["counts"] + 4 * B * K * HN].view(torch.int32).view(B, K, HN)   # noqa: E731
    live = full[2] > 0
    for _ in range(2):
        staged[3][L["deferred"]:L["deferred"] + 4 * B].fill_(0xFF)     # (the flags are the producing call's: a re-run reads none)
        ext.rerun_count_kernel(m, v, HN, 0.99, 5, MAX_NUM, staged[3], True, ext.COUNT_STAGED)
        assert torch.equal(counts(staged[3]).amax(-1)[live], full[1][live])
    # decode_keypoint on the network's tensor, without and with un_pnp (COUNT_STAGED_ESTIMATE stages v3's columns too)
    x = torch.empty(B, 2 + 2 * K, H, W, device=gpu)
    x[:, 0] = 3.0 * (m == 0)
    x[:, 1] = 3.0 * (m != 0)
    x[:, 2:] = v.permute(0, 3, 4, 1, 2).reshape(B, 2 * K, H, W)
    seg, vtx = x[:, :2], x[:, 2:].permute(0, 2, 3, 1).view(B, H, W, K, 2)
    dec = lambda ck: ext.decode_keypoint_v3(seg, vtx, HN, 0.99, 5, MAX_NUM, None, None, SEED, ext.SINGULAR_ZERO, 0, ck)   # noqa: E731
    a, b = dec(ext.COUNT_STAGED), dec(ext.COUNT_FULL)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert torch.equal(a[0], full[0]) and torch.equal(a[2], full[1]) and torch.equal(a[3], full[2])
    un = lambda ck: ext.decode_keypoint_un_pnp(seg, vtx, HN, 300, 0.99, 5, MAX_NUM, None, None, None, SEED, ext.SINGULAR_ZERO, 0, ck)   # noqa: E731
    a, b = un(ext.COUNT_STAGED_ESTIMATE), un(ext.COUNT_FULL)
    for p, q, nm in zip(a, b, ("keypoints", "mask", "covariances", "weights", "winner counts", "tn")):
        assert torch.equal(p, q) or bool(((p == q) | (p.isnan() & q.isnan())).all()), nm
    assert torch.equal(a[0], full[0]) and torch.equal(a[4], full[1])
