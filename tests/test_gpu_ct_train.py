"""The detector's heat-map targets and training loss on the MI355X (clean_pvnet_amd.ct_train) against the numpy twin
(tests/ct_train_twin.py, itself pinned to the reference's own results in tests/test_ct_train.py): the rows of the targets and every
centre of the heat map as bytes, every other heat-map element within one float32 (the exp of another library, rounded once);
both losses and the logit gradient within one float32 ulp, the wh gradient as bytes; both target forms of the wrapper, the
``num_pos == 0`` branch, logits clamped on both sides, upstream gradients, an unused loss, channel slices of one tensor read in
place, reruns, an index out of range, and the reference's fixtures.

The shapes are the smallest that reach every path (ct_train_twin.GPU_CASES): 2x3x37x53 (C*H*W odd: the scalar form, five full
tiles and a partial one), 1x4x8x12 (the 16-byte form, less than a tile, N = 1), 3x30x34x45 (N = 130, integer boxes, an image
with num = 0), 1x30x96x128 (360 tiles: the image slots wrap)."""
import numpy as np
import pytest

from tests import ct_train_twin as twin

pytestmark = pytest.mark.gpu
CASES = list(twin.GPU_CASES)
TARGET_CASES = ["c3_37x53", "c30_34x45_int", "vec_4x8x12"]


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _targets(gpu, d, dtype=None):
    """``ct_targets`` on the boxes of the case ``d``; everything as numpy."""
    import torch
    from clean_pvnet_amd.ct_train import ct_targets
    boxes, cls, num = _t(gpu, d["boxes"]), _t(gpu, d["cls"]), _t(gpu, d["num"])
    if dtype is not None:
        boxes, cls, num = boxes.to(getattr(torch, dtype)), cls.to(torch.int32), num.to(torch.int32)
    out = ct_targets(boxes, cls, num, d["C"], d["H"], d["W"])
    dtypes = (torch.float32, torch.float32, torch.int64, torch.int64, torch.float32, torch.int64)
    assert all(t.dtype == dt and t.is_contiguous() for t, dt in zip(out, dtypes))
    return dict(zip(("ct_hm", "wh", "ct_cls", "ct_ind", "ct_01", "ct_num"), (t.cpu().numpy() for t in out)))


def _run(gpu, d, views=False, go=None, only=None, ind=None, ind_dtype=None):
    """Forward and backward of ``ct_loss`` on the case ``d``; everything as numpy."""
    import torch
    from clean_pvnet_amd.ct_train import ct_loss
    C = d["C"]
    if views:                                                      # the heads as channel slices of one [B,32,H,W] tensor
        B, _, H, W = d["ct_hm_pred"].shape
        rest = np.full((B, 32 - C - 2, H, W), 7, np.float32)
        whole = _t(gpu, np.concatenate([d["ct_hm_pred"], d["wh_pred"], rest], 1)).requires_grad_(True)
        hp, wp = whole[:, :C], whole[:, C:C + 2]
        assert whole.shape[1] == 32 and (not hp.is_contiguous() or B == 1)
    else:
        hp, wp = _t(gpu, d["ct_hm_pred"]).requires_grad_(True), _t(gpu, d["wh_pred"]).requires_grad_(True)
    ct_ind = _t(gpu, d["ct_ind"] if ind is None else ind)
    if ind_dtype is not None:
        ct_ind = ct_ind.to(getattr(torch, ind_dtype))
    ct, wh = ct_loss(hp, wp, _t(gpu, d["ct_hm"]), _t(gpu, d["wh"]), ct_ind, _t(gpu, d["ct_01"]))
    assert ct.dim() == 0 and wh.dim() == 0 and ct.dtype == torch.float32 and wh.dtype == torch.float32
    if only == "ct":
        ct.backward()
    elif go is None:
        (ct + wh).backward()
    else:
        torch.autograd.backward([ct, wh], [_t(gpu, np.float32(go[0])), _t(gpu, np.float32(go[1]))])
    gh, gw = (whole.grad[:, :C], whole.grad[:, C:C + 2]) if views else (hp.grad, wp.grad)
    out = {"ct_loss": ct.detach().cpu().numpy(), "wh_loss": wh.detach().cpu().numpy(), "hm_grad": gh.cpu().numpy(), "wh_grad": gw.cpu().numpy()}
    if views:
        out["rest_grad"] = whole.grad[:, C + 2:].cpu().numpy()
    return out


_runs = {}


def _result(gpu, name):
    """The plain run of a case, computed once and shared; read-only."""
    if name not in _runs:
        _runs[name] = _run(gpu, twin.reference(name))
    return _runs[name]


def _same(a, b, zero_sign=True):
    canon = (lambda v: v) if zero_sign else (lambda v: v + np.float32(0))
    return all(canon(a[k]).tobytes() == canon(b[k]).tobytes() for k in ("ct_loss", "wh_loss", "hm_grad", "wh_grad"))


def _ulp(x):
    x = np.abs(np.float32(x))
    return float(np.nextafter(x, np.float32(np.inf)) - x)


# ------------------------------------------------------------------------------------------------------------ 1. the targets
@pytest.mark.parametrize("name", TARGET_CASES)
def test_targets_equal_the_twin(pkg, gpu, name):
    d = twin.reference(name)
    got = _targets(gpu, d)
    for k in ("wh", "ct_cls", "ct_ind", "ct_01", "ct_num"):
        assert got[k].dtype == d[k].dtype and got[k].tobytes() == d[k].tobytes(), k
    centres = d["ct_hm"] == 1
    assert got["ct_hm"].shape == d["ct_hm"].shape and np.array_equal(got["ct_hm"] == 1, centres)
    apart = twin.ulp_apart(got["ct_hm"], d["ct_hm"])
    print("%s: %d of %d heat-map elements differ from the twin, at most %d float32 apart; %d centres, %d elements > 0"
          % (name, (apart > 0).sum(), apart.size, apart.max(), centres.sum(), (d["ct_hm"] > 0).sum()))
    assert apart.max() <= 1 and np.array_equal(got["ct_hm"] == 0, d["ct_hm"] == 0) and not np.signbit(got["ct_hm"]).any()
    if d["B"] == 3:
        assert d["num"][2] == 0 and got["ct_num"][2] == 0 and not got["ct_hm"][2].any() and not got["ct_01"][2].any()


@pytest.mark.parametrize("name,dtype", [("c3_37x53", "float32"), ("c30_34x45_int", "int32")])
def test_int32_classes_counts_and_boxes_give_the_same_targets(pkg, gpu, name, dtype):
    d = twin.reference(name)
    a, b = _targets(gpu, d), _targets(gpu, d, dtype)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_float_boxes_with_fractions_round_as_the_twin_does(pkg, gpu):
    rng = np.random.default_rng(5)                                 # centres on .5 and beside it, sizes on integers and beside them
    N, C, H, W = 130, 3, 37, 53
    x0, y0 = rng.integers(0, W - 8, N) + rng.choice([0, 0.5, 0.25], N), rng.integers(0, H - 8, N) + rng.choice([0, 0.5, 0.75], N)
    boxes = np.stack([x0, y0, x0 + rng.integers(1, 20, N) + rng.choice([0, 1e-3, -1e-3], N), y0 + rng.integers(1, 16, N)], 1)[None].astype(np.float32)
    d = {"boxes": boxes, "cls": rng.integers(0, C, (1, N)), "num": np.array([N]), "C": C, "H": H, "W": W}
    want, got = twin.ct_targets(boxes, d["cls"], d["num"], C, H, W), _targets(gpu, d)
    for k in ("wh", "ct_cls", "ct_ind", "ct_01", "ct_num"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(got["ct_hm"] == 1, want["ct_hm"] == 1) and twin.ulp_apart(got["ct_hm"], want["ct_hm"]).max() <= 1


# ------------------------------------------------------------------------------------------------------------ 2. the loss
@pytest.mark.parametrize("name", CASES)
def test_losses_and_gradients_equal_the_twin(pkg, gpu, name):
    d, got = twin.reference(name), _result(gpu, name)
    uc, uw = twin.ulp_apart(got["ct_loss"], d["ct_loss"]), twin.ulp_apart(got["wh_loss"], d["wh_loss"])
    print("%s: ct_loss %r twin %r (%d float32 apart); wh_loss %r twin %r (%d apart)" % (name, got["ct_loss"], d["ct_loss"], uc, got["wh_loss"], d["wh_loss"], uw))
    assert np.isfinite(got["ct_loss"]) and np.isfinite(got["wh_loss"]) and uc <= 1 and uw <= 1
    ug = twin.ulp_apart(got["hm_grad"], d["hm_grad"])
    print("  logit gradient at most %d float32 apart, %d of %d elements differ" % (ug.max(), (ug > 0).sum(), ug.size))
    assert ug.max() <= 1 and np.array_equal(got["hm_grad"] == 0, d["hm_grad"] == 0)
    diff = got["wh_grad"].view(np.uint32) != d["wh_grad"].view(np.uint32)
    print("  wh gradient: %d of %d elements differ, %d are not zero" % (diff.sum(), diff.size, (d["wh_grad"] != 0).sum()))
    assert not diff.any()
    if name == "no_pos":
        assert not (d["ct_hm"] == 1).any() and got["ct_loss"] > 0 and got["hm_grad"].any()
    if name.startswith("clamp"):
        assert not got["hm_grad"][np.abs(d["ct_hm_pred"]) >= 12].any()


@pytest.mark.parametrize("name", list(twin.GOLDEN_CASES))
def test_against_the_references_fixtures(pkg, gpu, name):
    """The rule of tests/test_ct_train.py with the device's own distance from the twin added: a neighbouring float32 (the exp and
    log of another library).  The gradients are those of the wrapper's loss, ct_loss + 0.1 * wh_loss."""
    g, d = twin.load_golden(name), twin.reference(name)
    got = _run(gpu, d, go=(1.0, 0.1))
    e_ct, e_wh = abs(float(got["ct_loss"]) - float(g["ct_loss"])), abs(float(got["wh_loss"]) - float(g["wh_loss"]))
    b_ct, b_wh = 2 * _ulp(g["ct_loss"]) + float(g["ct_loss_f32_dist"]), 2 * _ulp(g["wh_loss"]) + float(g["wh_loss_f32_dist"])
    print("%s: ct_loss |diff| to the float32 run %.3g (bound %.3g); wh_loss %.3g (bound %.3g)" % (name, e_ct, b_ct, e_wh, b_wh))
    assert e_ct <= b_ct and e_wh <= b_wh
    apart = twin.ulp_apart(got["hm_grad"], g["hm_grad64"].astype(np.float32))
    print("  logit gradient at most %d float32 from the float64 run" % apart.max())
    assert apart.max() <= 2                                        # one to the twin, the twin one to the run
    assert got["wh_grad"].tobytes() == g["wh_grad"].tobytes()
    w = int(g["width"])
    t = _targets(gpu, d)
    for k in ("wh", "ct_cls", "ct_ind", "ct_01"):
        assert np.ascontiguousarray(t[k][:, :w]).tobytes() == g[k].tobytes(), k
    assert t["ct_num"].tobytes() == g["ct_num"].tobytes() and np.array_equal(t["ct_hm"] == 1, g["ct_hm"] == 1)
    assert twin.ulp_apart(t["ct_hm"], g["ct_hm"]).max() <= 1


def test_upstream_gradients_are_read_from_the_device(pkg, gpu):
    d = twin.reference("c3_37x53")
    got = _run(gpu, d, go=(1.0, 0.1))
    a = (d["wh_pred"], d["wh"], d["ct_ind"], d["ct_01"])
    assert got["wh_grad"].tobytes() == twin.wh_grad(*a, go=0.1).tobytes()
    assert got["hm_grad"].tobytes() == _result(gpu, "c3_37x53")["hm_grad"].tobytes()
    got = _run(gpu, d, go=(-0.37, 2.5))
    assert got["wh_grad"].tobytes() == twin.wh_grad(*a, go=2.5).tobytes()
    assert twin.ulp_apart(got["hm_grad"], twin.focal_grad(d["ct_hm_pred"], d["ct_hm"], -0.37)[0]).max() <= 1


def test_an_unused_loss_counts_as_a_zero_gradient(pkg, gpu):
    d = twin.reference("c3_37x53")
    got = _run(gpu, d, only="ct")
    assert got["hm_grad"].tobytes() == _result(gpu, "c3_37x53")["hm_grad"].tobytes() and not got["wh_grad"].any()


@pytest.mark.parametrize("name", ["c3_37x53", "c30_34x45_int", "vec_4x8x12"])
def test_channel_slices_of_one_tensor_are_read_in_place(pkg, gpu, name):
    got = _run(gpu, twin.reference(name), views=True)
    # the gradient of a slice reaches the whole tensor through torch's own backward of the slice, which adds it to zeros: a -0
    # arrives as +0, everything else as it was written
    assert _same(got, _result(gpu, name), zero_sign=False) and not got["rest_grad"].any()
    assert got["ct_loss"].tobytes() == _result(gpu, name)["ct_loss"].tobytes()


def test_int32_indices_give_the_same_results(pkg, gpu):
    assert _same(_run(gpu, twin.reference("c3_37x53"), ind_dtype="int32"), _result(gpu, "c3_37x53"))


def test_the_same_call_twice_gives_the_same_bytes(pkg, gpu):
    import torch
    from clean_pvnet_amd.ct_train import ct_loss, ct_targets
    cases = []
    for name in ("c3_37x53", "slots_30x96x128"):
        d = twin.reference(name)
        cases.append((d, {k: _t(gpu, d[k]) for k in ("ct_hm_pred", "wh_pred", "ct_hm", "wh", "ct_ind", "ct_01", "boxes", "cls", "num")}))
    go = torch.ones((), device=gpu)
    torch.cuda.synchronize()
    runs = []
    torch.cuda.set_sync_debug_mode("error")                        # nothing is read back
    try:
        for _ in range(2):
            out = []
            for d, t in cases:
                hp, wp = t["ct_hm_pred"].clone().requires_grad_(True), t["wh_pred"].clone().requires_grad_(True)
                ct, wh = ct_loss(hp, wp, t["ct_hm"], t["wh"], t["ct_ind"], t["ct_01"])
                torch.autograd.backward([ct, wh], [go, go])
                out += [ct.detach(), wh.detach(), hp.grad, wp.grad]
                out += list(ct_targets(t["boxes"], t["cls"], t["num"], d["C"], d["H"], d["W"]))
            runs.append(out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(*runs):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert runs[0][0].cpu().numpy().tobytes() == _result(gpu, "c3_37x53")["ct_loss"].tobytes()


# ------------------------------------------------------------------------------------------------------------ 3. robustness
@pytest.mark.parametrize("bad", [37 * 53, -1, 1 << 40])
def test_an_index_out_of_range_gives_nan_and_no_fault(pkg, gpu, bad):
    import torch
    d = twin.reference("c3_37x53")
    ind = d["ct_ind"].copy()
    assert d["ct_01"][1, 2] == 1 and d["ct_01"][0, -1] == 0
    ind[1, 2] = bad
    assert twin.bad_indices(ind, d["ct_01"], 37 * 53) == 1
    got = _run(gpu, d, ind=ind)
    assert np.isnan(got["wh_loss"]) and np.isnan(got["wh_grad"]).all()
    assert got["ct_loss"].tobytes() == _result(gpu, "c3_37x53")["ct_loss"].tobytes()
    assert got["hm_grad"].tobytes() == _result(gpu, "c3_37x53")["hm_grad"].tobytes()
    ind = d["ct_ind"].copy()
    ind[0, -1] = bad                                               # at a position of weight 0 it adds nothing
    assert _same(_run(gpu, d, ind=ind), _result(gpu, "c3_37x53"))
    torch.cuda.synchronize()                                       # and the device is still there
    assert _same(_run(gpu, d), _result(gpu, "c3_37x53"))


# ------------------------------------------------------------------------------------------------------------ 4. the wrapper
@pytest.mark.parametrize("name", ["c3_37x53", "c30_34x45_int"])
def test_network_wrapper_trains_a_step_in_both_target_forms(pkg, gpu, name):
    import torch
    from torch import nn
    from clean_pvnet_amd.ct_train import NetworkWrapper
    d = twin.reference(name)
    C = d["C"]

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.bias = nn.Parameter(torch.zeros(C + 2, 1, 1))

        def forward(self, inp):
            x = inp + self.bias
            return {"ct_hm": x[:, :C], "wh": x[:, C:]}

    want = _run(gpu, d, go=(1.0, 0.1))
    inp = _t(gpu, np.concatenate([d["ct_hm_pred"], d["wh_pred"]], 1))
    shipped = {"inp": inp, "ct_hm": _t(gpu, d["ct_hm"]), "wh": _t(gpu, d["wh"]), "ct_ind": _t(gpu, d["ct_ind"]), "ct_01": _t(gpu, d["ct_01"])}
    boxes = {"inp": inp, "boxes": _t(gpu, d["boxes"]), "cls": _t(gpu, d["cls"]), "num": _t(gpu, d["num"])}
    for form, batch in (("shipped", shipped), ("boxes", boxes)):
        if form == "boxes":                                        # the device's own heat map: a neighbouring float32 off the centres
            want = _run(gpu, dict(d, ct_hm=_targets(gpu, d)["ct_hm"]), go=(1.0, 0.1))
        w = NetworkWrapper(Net()).to(gpu)
        output, loss, stats, image_stats = w(batch)
        loss.backward()
        assert list(stats) == ["ct_loss", "wh_loss", "loss"] and image_stats == {} and set(output) == {"ct_hm", "wh"}
        ct, wh = stats["ct_loss"].detach().cpu().numpy(), stats["wh_loss"].detach().cpu().numpy()
        assert ct.tobytes() == want["ct_loss"].tobytes() and wh.tobytes() == want["wh_loss"].tobytes(), form
        assert float(loss.detach()) == float(np.float32(ct) + np.float32(0.1) * np.float32(wh))
        g = np.concatenate([want["hm_grad"], want["wh_grad"]], 1).astype(np.float64)
        n = g.shape[0] * g.shape[2] * g.shape[3]
        got = w.net.bias.grad.cpu().numpy().ravel()                # torch's own float32 sum of our gradient, any order
        assert (np.abs(got - g.sum((0, 2, 3))) <= (n + 1) * twin.U * np.abs(g).sum((0, 2, 3))).all(), form
