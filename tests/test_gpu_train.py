"""PVNet's vote targets and training loss on the MI355X (clean_pvnet_amd.train) against the numpy twin (tests/train_twin.py,
itself pinned to the reference's own results in tests/test_train.py): the target, the vote loss and the vote gradient as bytes
in both target forms; the seg loss and the seg gradient within a neighbouring float32 (binary64 exp and log of two libraries
would have to differ by about 2^29 units to move a float32 rounding further); the reference's formula in torch ops on the
same device within the twin's derived bounds; strided views, the four mask dtypes, bad labels, NaN predictions, empty masks,
reruns and the absence of synchronisation.  ``torch.autograd.gradcheck`` is not used: the kernels are float32 by contract.

The shapes are the smallest that reach every path (train_twin.GPU_CASES): 37x53 (H*W odd: the scalar form, one full and one
partial tile), 40x64 (the 16-byte form, 2.5 tiles, float32 keypoints), 480x640 at B = 1 (300 tiles: an image slot sums two),
B = 3 with one empty mask; K in {1, 9}, C in {2, 3}."""
import numpy as np
import pytest

from tests import train_twin as twin

pytestmark = pytest.mark.gpu
CASES = list(twin.GPU_CASES)
MASK_DTYPES = ("uint8", "bool", "int32", "int64")


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _run(gpu, d, form, mask=None, views=False, go=None, vp=None, sp=None):
    """Forward and backward of ``pvnet_loss`` on the case ``d``; everything as numpy."""
    import torch
    from clean_pvnet_amd.train import pvnet_loss
    K, C = d["K"], d["C"]
    vp = d["vertex_pred"] if vp is None else vp
    sp = d["seg_pred"] if sp is None else sp
    if views:                                                      # resnet18.py:93-94: seg and vertex are slices of one tensor
        whole = _t(gpu, np.concatenate([sp, vp], 1)).requires_grad_(True)
        seg_pred, vertex_pred = whole[:, :C], whole[:, C:]
        assert not vertex_pred.is_contiguous() or whole.shape[0] == 1
    else:
        vertex_pred, seg_pred = _t(gpu, vp).requires_grad_(True), _t(gpu, sp).requires_grad_(True)
    m = _t(gpu, d["mask"]) if mask is None else mask
    target = {"kpt_2d": _t(gpu, d["kpt_2d"])} if form == "kpt_2d" else {"vertex": _t(gpu, d["target"])}
    vote, seg = pvnet_loss(vertex_pred, seg_pred, m, **target)
    assert vote.dim() == 0 and seg.dim() == 0 and vote.dtype == torch.float32 and seg.dtype == torch.float32
    if go is None:
        (vote + seg).backward()
    else:
        torch.autograd.backward([vote, seg], [_t(gpu, np.float32(go[0])), _t(gpu, np.float32(go[1]))])
    if views:
        gv, gs = whole.grad[:, C:], whole.grad[:, :C]
    else:
        gv, gs = vertex_pred.grad, seg_pred.grad
    return {"vote_loss": vote.detach().cpu().numpy(), "seg_loss": seg.detach().cpu().numpy(), "vote_grad": gv.cpu().numpy(),
            "seg_grad": gs.cpu().numpy()}


_runs = {}


def _result(gpu, name, form):
    """The plain run of a case in one target form, computed once and shared; read-only."""
    if (name, form) not in _runs:
        _runs[name, form] = _run(gpu, twin.reference(name), form)
    return _runs[name, form]


def _same(a, b, zero_sign=True):
    """The four results as bytes; ``zero_sign=False`` takes -0 for +0."""
    canon = (lambda v: v) if zero_sign else (lambda v: v + np.float32(0))
    return all(canon(a[k]).tobytes() == canon(b[k]).tobytes() for k in ("vote_loss", "seg_loss", "vote_grad", "seg_grad"))


# ------------------------------------------------------------------------------------------------------------ 1. the twin
@pytest.mark.parametrize("name", CASES)
def test_compute_vertex_equals_the_twin_as_bytes(pkg, gpu, name):
    from clean_pvnet_amd.train import compute_vertex
    d = twin.reference(name)
    got = compute_vertex(_t(gpu, d["mask"]), _t(gpu, d["kpt_2d"])).cpu().numpy()
    assert got.shape == d["target"].shape and got.dtype == np.float32
    diff = got.view(np.uint32) != d["target"].view(np.uint32)
    print("%s: %d of %d target elements differ" % (name, diff.sum(), diff.size))
    assert not diff.any()
    one = compute_vertex(_t(gpu, d["mask"][0]), _t(gpu, d["kpt_2d"][0])).cpu().numpy()     # [H,W] and [K,2], as the loader calls it
    assert one.tobytes() == d["target"][0].tobytes()


@pytest.mark.parametrize("form", ["kpt_2d", "vertex"])
@pytest.mark.parametrize("name", CASES)
def test_losses_and_gradients_equal_the_twin(pkg, gpu, name, form):
    d, got = twin.reference(name), _result(gpu, name, form)
    print("%s/%s: vote loss %r twin %r; seg loss %r twin %r" % (name, form, got["vote_loss"], d["vote_loss"], got["seg_loss"], d["seg_loss"]))
    assert np.isfinite(got["vote_loss"]) and got["vote_loss"].tobytes() == d["vote_loss"].tobytes()
    diff = got["vote_grad"].view(np.uint32) != d["vote_grad"].view(np.uint32)
    print("  vote gradient: %d of %d elements differ" % (diff.sum(), diff.size))
    assert not diff.any()
    ul, ug = twin.ulp_apart(got["seg_loss"], d["seg_loss"]), twin.ulp_apart(got["seg_grad"], d["seg_grad"])
    print("  seg loss %d float32 apart; seg gradient at most %d apart, %d of %d elements differ" % (ul, ug.max(), (ug > 0).sum(), ug.size))
    assert ul <= 1 and ug.max() <= 1


def test_an_upstream_gradient_is_read_from_the_device(pkg, gpu):
    d = twin.reference("vec_40x64")
    go = (-0.37, 2.5)
    got = _run(gpu, d, "kpt_2d", go=go)
    assert got["vote_grad"].tobytes() == twin.vote_grad(d["vertex_pred"], d["target"], d["mask"], go[0]).tobytes()
    assert twin.ulp_apart(got["seg_grad"], twin.seg_grad(d["seg_pred"], d["mask"], go[1])[0]).max() <= 1


def test_an_unused_loss_counts_as_a_zero_gradient(pkg, gpu):
    from clean_pvnet_amd.train import pvnet_loss
    d = twin.reference("scalar_37x53")
    vp, sp = _t(gpu, d["vertex_pred"]).requires_grad_(True), _t(gpu, d["seg_pred"]).requires_grad_(True)
    vote, _ = pvnet_loss(vp, sp, _t(gpu, d["mask"]), kpt_2d=_t(gpu, d["kpt_2d"]))
    vote.backward()
    assert vp.grad.cpu().numpy().tobytes() == d["vote_grad"].tobytes() and not sp.grad.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------------------ 2. torch on the device
@pytest.mark.parametrize("name", CASES)
def test_against_the_references_formula_in_torch_ops(pkg, gpu, name):
    import torch
    d, got = twin.reference(name), _result(gpu, name, "kpt_2d")
    vp, sp = _t(gpu, d["vertex_pred"]).requires_grad_(True), _t(gpu, d["seg_pred"]).requires_grad_(True)
    mask, target = _t(gpu, d["mask"]), _t(gpu, d["target"])
    weight = mask[:, None].float()                                                  # lib/train/trainers/pvnet.py:25-32
    vote = torch.nn.functional.smooth_l1_loss(vp * weight, target * weight, reduction='sum') / weight.sum() / target.size(1)
    seg = torch.nn.CrossEntropyLoss()(sp, mask.long())
    (vote + seg).backward()
    B, C, H, W = d["seg_pred"].shape
    vote, seg = float(vote.detach()), float(seg.detach())
    zmax, zrange = float(np.abs(d["seg_pred"]).max()), float(d["seg_pred"].max() - d["seg_pred"].min())
    bv, bs = twin.vote_bound_f32(vote, d["vertex_pred"].size), twin.seg_bound_f32(seg, B * H * W, C, zmax)
    print("%s: vote %r torch %r (bound %.3g); seg %r torch %r (bound %.3g)" % (name, got["vote_loss"], vote, bv, got["seg_loss"], seg, bs))
    assert abs(float(got["vote_loss"]) - vote) <= bv and abs(float(got["seg_loss"]) - seg) <= bs
    gv, gs = vp.grad.cpu().numpy(), sp.grad.cpu().numpy()
    ev = np.abs(got["vote_grad"].astype(np.float64) - gv) - twin.vote_grad_bound_f32(gv)
    es, bg = np.abs(got["seg_grad"].astype(np.float64) - gs).max(), twin.seg_grad_bound_f32(C, zrange, 1.0, B * H * W)
    print("  vote gradient: max excess over the bound %.3g; seg gradient: max |diff| %.3g (bound %.3g)" % (ev.max(), es, bg))
    assert (ev <= 0).all() and es <= bg


# ------------------------------------------------------------------------------------------------------------ 3. views and mask dtypes
@pytest.mark.parametrize("form", ["kpt_2d", "vertex"])
@pytest.mark.parametrize("name", ["scalar_37x53", "vec_40x64"])
def test_channel_slices_of_one_tensor_equal_the_contiguous_run(pkg, gpu, name, form):
    got = _run(gpu, twin.reference(name), form, views=True)
    # the gradient of a slice reaches the whole tensor through torch's own backward of the slice, which adds it to zeros: a -0
    # arrives as +0, everything else as it was written
    assert _same(got, _result(gpu, name, form), zero_sign=False)
    assert got["vote_loss"].tobytes() == _result(gpu, name, form)["vote_loss"].tobytes()


@pytest.mark.parametrize("name", ["scalar_37x53", "empty_of_three"])
def test_the_four_mask_dtypes_give_equal_results(pkg, gpu, name):
    import torch
    from clean_pvnet_amd.train import compute_vertex
    d, want = twin.reference(name), _result(gpu, name, "kpt_2d")
    for dt in MASK_DTYPES:
        src = (d["mask"] == 1) if dt == "bool" else d["mask"]                       # bool has no label 2: its own comparison below
        m = _t(gpu, src).to(getattr(torch, dt))
        got = _run(gpu, d, "kpt_2d", mask=m)
        if dt == "bool" and (d["mask"] > 1).any():
            want_bool = _run(gpu, d, "kpt_2d", mask=_t(gpu, src.astype(np.uint8)))
            assert _same(got, want_bool), dt
        else:
            assert _same(got, want), dt
        assert compute_vertex(m, _t(gpu, d["kpt_2d"])).cpu().numpy().tobytes() == d["target"].tobytes(), dt


# ------------------------------------------------------------------------------------------------------------ 4. the edges
@pytest.mark.parametrize("name,dt,label", [("scalar_37x53", "uint8", 2), ("vec_40x64", "int64", -1), ("vec_40x64", "int32", 1 << 20)])
def test_a_label_out_of_range_gives_nan_and_no_fault(pkg, gpu, name, dt, label):
    import torch
    d = twin.reference(name)
    m = _t(gpu, d["mask"]).to(getattr(torch, dt))
    m[-1, -1, -1] = label
    assert twin.bad_labels(m.cpu().numpy(), d["C"]) == 1
    for form in ("kpt_2d", "vertex"):
        got = _run(gpu, d, form, mask=m)
        assert np.isnan(got["vote_loss"]) and np.isnan(got["seg_loss"])
        assert np.isnan(got["vote_grad"]).all() and np.isnan(got["seg_grad"]).all()
    torch.cuda.synchronize()                                                        # and the device is still there
    assert _same(_run(gpu, d, "kpt_2d"), _result(gpu, name, "kpt_2d"))


def test_a_nan_prediction_on_the_background_reaches_the_vote_loss_only(pkg, gpu):
    d = twin.reference("scalar_37x53")
    assert d["mask"][0, 0, 0] == 0
    vp = d["vertex_pred"].copy()
    vp[0, 3, 0, 0] = np.nan
    got = _run(gpu, d, "kpt_2d", vp=vp)
    assert np.isnan(got["vote_loss"]) and got["seg_loss"].tobytes() == _result(gpu, "scalar_37x53", "kpt_2d")["seg_loss"].tobytes()
    assert np.isnan(got["vote_grad"][0, 3, 0, 0]) and np.isnan(got["vote_grad"]).sum() == 1


def test_an_empty_batch_mask_gives_a_nan_vote_loss(pkg, gpu):
    d = dict(twin.reference("vec_40x64"))
    d["mask"] = np.zeros_like(d["mask"])
    for form in ("kpt_2d", "vertex"):
        got = _run(gpu, d, form)
        want_seg, _ = twin.seg_loss(d["seg_pred"], d["mask"])
        assert np.isnan(got["vote_loss"]) and np.isfinite(got["seg_loss"]) and twin.ulp_apart(got["seg_loss"], want_seg) <= 1
        assert np.isfinite(got["seg_grad"]).all()


def test_one_empty_image_beside_others_is_not_special(pkg, gpu):
    d, got = twin.reference("empty_of_three"), _result(gpu, "empty_of_three", "kpt_2d")
    assert not d["mask"][1].any() and d["mask"][0].any() and d["mask"][2].any()
    assert not got["vote_grad"][1].any() and got["vote_grad"][0].any() and np.isfinite(got["vote_loss"])


# ------------------------------------------------------------------------------------------------------------ 5. no host sync
def test_nothing_synchronises_and_reruns_give_the_same_bits(pkg, gpu):
    import torch
    from clean_pvnet_amd.train import compute_vertex, pvnet_loss
    cases = []
    for name in ("scalar_37x53", "vec_40x64"):
        d = twin.reference(name)
        cases.append((d, {k: _t(gpu, d[k]) for k in ("vertex_pred", "seg_pred", "mask", "kpt_2d", "target")}))
    go = torch.ones((), device=gpu)
    torch.cuda.synchronize()
    runs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            out = []
            for d, t in cases:
                for target in ({"kpt_2d": t["kpt_2d"]}, {"vertex": t["target"]}):
                    vp, sp = t["vertex_pred"].clone().requires_grad_(True), t["seg_pred"].clone().requires_grad_(True)
                    vote, seg = pvnet_loss(vp, sp, t["mask"], **target)
                    torch.autograd.backward([vote, seg], [go, go])
                    out += [vote.detach(), seg.detach(), vp.grad, sp.grad]
                out.append(compute_vertex(t["mask"], t["kpt_2d"]))
            runs.append(out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(*runs):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert runs[0][0].cpu().numpy().tobytes() == cases[0][0]["vote_loss"].tobytes()


def test_network_wrapper_trains_a_step_on_the_device(pkg, gpu):
    import torch
    from torch import nn
    from clean_pvnet_amd.train import NetworkWrapper
    d = twin.reference("vec_40x64")

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.bias = nn.Parameter(torch.zeros(d["C"] + 2 * d["K"], 1, 1))

        def forward(self, inp):
            x = inp + self.bias
            return {"seg": x[:, :d["C"]], "vertex": x[:, d["C"]:]}

    w = NetworkWrapper(Net()).to(gpu)
    batch = {"inp": _t(gpu, np.concatenate([d["seg_pred"], d["vertex_pred"]], 1)), "mask": _t(gpu, d["mask"]),
             "kpt_2d": _t(gpu, d["kpt_2d"]), "meta": {}}
    output, loss, stats, image_stats = w(batch)
    loss.backward()
    got = _result(gpu, "vec_40x64", "kpt_2d")
    assert stats["vote_loss"].detach().cpu().numpy().tobytes() == got["vote_loss"].tobytes() and image_stats == {}
    assert stats["seg_loss"].detach().cpu().numpy().tobytes() == got["seg_loss"].tobytes() and float(stats["loss"].detach()) == float(loss.detach())
    g = np.concatenate([got["seg_grad"], got["vote_grad"]], 1).astype(np.float64)
    n = g.shape[0] * g.shape[2] * g.shape[3]                                        # torch's own float32 sum of our gradient, any order
    assert (np.abs(w.net.bias.grad.cpu().numpy().ravel() - g.sum((0, 2, 3))) <= (n + 1) * twin.U * np.abs(g).sum((0, 2, 3))).all()
    batch["vertex"] = _t(gpu, d["target"])                                          # a loader that still ships the field
    assert w(batch)[2]["vote_loss"].detach().cpu().numpy().tobytes() == got["vote_loss"].tobytes()


def test_a_refused_call_reads_as_its_binding_says(pkg, gpu):
    """``_native.bind(...).call``: the library refuses NULL pointers in host code, before any launch; bound with the error string
    the failure names the module and says what the library recorded, bound without it reads plainly."""
    from clean_pvnet_amd import _native
    args = (None, 0, None, 0, 1, 1, 4, 4, None)                                     # B = K = 1, H = W = 4, NULL tensors
    with pytest.raises(RuntimeError) as ei:
        _native.bind("probe", "libpvnet_vote.so", last_error="pvv_last_error").call("pvv_vertex_target", gpu, *args)
    assert str(ei.value) == "clean_pvnet_amd.probe: pvv_vertex_target failed (-1): train: NULL device pointer"
    with pytest.raises(RuntimeError) as ei:
        _native.bind("probe", "libpvnet_vote.so").call("pvv_vertex_target", gpu, *args)
    assert str(ei.value) == "pvv_vertex_target failed (-1)"
