"""Every device entry point on poisoned, guarded memory (tests/guarded.py).

Each call below runs three times, once per fill of ``guarded.FILLS``, with every device input a ``guarded_copy`` (0xFF bands: an
over-read that reaches a result changes it) and every tensor the call allocates -- outputs, workspaces, temporaries -- carved from an
arena of its own.  ``guarded_runs`` asserts for each run

  (a) no band of any arena changed: nothing was stored outside an output, a workspace or a temporary;
  (b) -- in the test -- the results equal the twin / oracle / golden values by the rule of the module's own GPU test, and, here, the
      three runs are the same bytes: no output element is left unwritten, nothing depends on what a workspace held before;
  (c) every device tensor of the returned structure lies in an arena and the module's workspace was requested (so a test cannot pass
      because an allocation slipped past the mode);
  (d) the body of every input arena is unchanged: no call writes its inputs.

The scenarios are the smallest ones of the modules' own GPU tests, taken from their twins (tests/*_twin.py) or from those tests; the
voting batches are new (``synth.make_batch``) and listed at ``VOTE_CASES``.

Out of reach of this method, and out of scope: the host-pointer launchers (``findNearestPointIdxLauncher`` of libpvnet_nn, the host
entry of libpvnet_pnp) allocate with ``hipMalloc`` inside the library; ``dist`` / ``rccl``, graph capture and side streams.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import capi, guarded
from tests import tolerances as tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------------------ the driver
def _map(f, x):
    if isinstance(x, dict):
        return {k: _map(f, v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_map(f, v) for v in x)
    if isinstance(x, np.ndarray):
        return f(torch.tensor(x))
    return f(x) if isinstance(x, torch.Tensor) else x


def _tensors(x):
    if isinstance(x, dict):
        x = list(x.values())
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _tensors(v)]
    return [x] if isinstance(x, torch.Tensor) else []


def _host(x):
    return _map(lambda t: t.detach().cpu().numpy(), x)


def _same_bytes(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same_bytes(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_bytes(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    return a == b


def _first_difference(a, b, path=""):
    if isinstance(a, dict):
        for k in a:
            d = _first_difference(a[k], b[k], "%s[%r]" % (path, k))
            if d:
                return d
    elif isinstance(a, (list, tuple)):
        for i, (x, y) in enumerate(zip(a, b)):
            d = _first_difference(x, y, "%s[%d]" % (path, i))
            if d:
                return d
    elif isinstance(a, np.ndarray) and not _same_bytes(a, b):
        w = np.argwhere(np.ascontiguousarray(a).view(np.uint8).reshape(-1) != np.ascontiguousarray(b).view(np.uint8).reshape(-1))
        return "%s %s %s: %d bytes differ, first at byte %d" % (path, a.dtype, a.shape, len(w), int(w[0]))
    return None


def guarded_runs(gpu, what, inputs, call, *, workspace, derived=(), before=None):
    """``call(g, m)`` -- ``g`` the guarded copies of ``inputs``, ``m`` the mode -- once per fill; returns the result of the first run
    as numpy after asserting (a), (c), (d) for each run and that the three results are the same bytes.
    ``workspace``: True -- ``_native.workspace`` must have been asked for more than 0 bytes; False -- for none at all; "ext" -- the call
    goes through the pybind shim, whose workspace is an ``at::empty`` of bytes (the call appends it to ``m.workspaces``).
    ``derived``: keys of the returned dict that torch ops compute from the kernels' outputs; they need not lie in an arena."""
    runs = []
    for fill in guarded.FILLS:
        if before is not None:
            before()
        m = guarded.Guarded(gpu, fill=fill)
        with m:
            g = _map(m.guarded_copy, inputs)
            n_inputs = len(m.arenas)
            result = call(g, m)
            violations = m.check()
            written = m.inputs_changed()
        assert violations == [], "%s, fill 0x%02X: %s" % (what, fill, violations)                                # (a)
        assert written == [], "%s, fill 0x%02X: inputs written: %s" % (what, fill, [(a.index, a.shape) for a in written])   # (d)
        owned = {k: v for k, v in result.items() if k not in derived} if isinstance(result, dict) else result
        outs = [t for t in _tensors(owned) if t.device.type == gpu.type]
        assert outs and all(m.owns(t) for t in outs), "%s: outputs outside the arenas: %s" % (
            what, [(tuple(t.shape), t.dtype) for t in outs if not m.owns(t)])                                     # (c)
        assert not any(t.untyped_storage().data_ptr() == a.buf.untyped_storage().data_ptr() for t in outs for a in m.arenas[:n_inputs]), \
            "%s: an output aliases an input" % what
        asked = [n for n, _ in m.workspaces]
        if workspace is False:
            assert asked == [], (what, asked)
        else:
            assert asked and max(asked) > 0 and all(m.owns(t) and t.numel() == max(n, 16) for n, t in m.workspaces), (what, asked)
        print("%s, fill 0x%02X: %d arenas checked (%d inputs), workspace bytes %s" % (what, fill, len(m.arenas), n_inputs, asked))
        runs.append(_host(result))
    for fill, r in zip(guarded.FILLS[1:], runs[1:]):
        assert _same_bytes(r, runs[0]), "%s: fill 0x%02X gives other bytes than fill 0x%02X: %s" % (
            what, fill, guarded.FILLS[0], _first_difference(runs[0], r))
    return runs[0]


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_the_helper_sees_planted_faults_in_device_memory(gpu):
    """What tests/test_guarded.py plants on CPU tensors, on the device: a byte stored one past an output (inside its arena, with the
    fill's own value), an element left unwritten, a written input."""
    got = []
    for fill in guarded.FILLS:
        with guarded.Guarded(gpu, fill=fill) as m:
            x = m.guarded_copy(torch.arange(7, dtype=torch.float32))
            out = torch.empty(7, dtype=torch.float32, device=gpu)
            out[:6] = x[:6] * 2                                                          # forgets the last element
            assert m.check() == [] and m.inputs_changed() == [] and m.owns(out) and m.owns(x) and not m.owns(x * 2)
            a = m.arenas[-1]
            assert a.shape == (7,) and out.data_ptr() == a.buf.data_ptr() + guarded.G and out.data_ptr() % guarded.G == 0
            torch.as_strided(a.buf, (1,), (1,), guarded.G + a.n).fill_(fill)
            (v,) = m.check()
            assert v.arena is a and v.offset == 28
            x[0] = 5.0
            assert m.inputs_changed() == [m.arenas[0]]
            got.append(out.cpu().numpy().tobytes())
    assert len(set(got)) == 3 and len({g[:24] for g in got}) == 1


# ------------------------------------------------------------------------------------------------------------ ransac_voting
# New small batches.  45 x 70: neither side a multiple of 8.  "bk129": B * K = 129 >= 128, the banded select + refit
# (k_select_refit<BAND>).  "stage": the smallest shape whose problem may stage, so that the workspace holds the leader words and
# ``stage_hint`` reports: host_stage.hpp:41-42 asks hn >= 128, cap >= kStageMinChunks * 4 * kBfPixPerWave = 8 * 4 * 128 = 4096 rows
# (so H * W >= 4096: 59 x 70 = 4130, again no multiple of 8) and B * K * hn * min(H * W, cap) >= kStageMinWork * kStageProxyFg = 4e8:
# with K = 9, hn = 512 that is B = 22 (4.19e8; B = 21 gives 4.00e8 - 1.6e5).  Its even images are all foreground (tn = 4130 > 3584:
# eight chunks), which is what COUNT_STAGED then really counts in stages.
VOTE_CASES = {
    "small": dict(B=2, H=45, W=70, K=3, hn=64, fg=0.10, sigma=0.02, seed=5),
    "bk129": dict(B=43, H=45, W=70, K=3, hn=64, fg=0.10, sigma=0.02, seed=6),
    "stage": dict(B=22, H=59, W=70, K=9, hn=512, fg=0.30, sigma=0.02, seed=7),
}


@functools.lru_cache(maxsize=None)
def _vote_case(name):
    """(batch, idxs, tn) on the host, and the oracle's (means, win_counts, tn) for the injected idxs: computed once."""
    from clean_pvnet_amd import synth
    from oracle import vote_oracle
    c = VOTE_CASES[name]
    d = synth.make_batch(**{k: v for k, v in c.items() if k != "hn"})
    if name == "stage":
        d["mask"][::2] = 1
    tn = [int(x) for x in (d["mask"] != 0).sum((1, 2))]
    idxs = synth.make_idxs(tn, c["hn"], c["K"], seed=c["seed"])
    return d, idxs, tn


@functools.lru_cache(maxsize=None)
def _vote_want(name, half=None):
    from oracle import vote_oracle
    d, idxs, tn = _vote_case(name)
    vertex = d["vertex"] if half is None else d["vertex"].to(getattr(torch, half)).float()
    det = []
    want = vote_oracle.ransac_voting_layer_v3(d["mask"].numpy(), vertex.numpy(), VOTE_CASES[name]["hn"], 0.99, idxs=idxs.numpy(), details=det)
    win = np.stack([r["win_counts"] if not r["skipped"] else np.zeros(vertex.shape[3], np.int32) for r in det])
    return want, win, np.array([r["tn"] for r in det], np.int32)


def _shutdown():
    from clean_pvnet_amd import ransac_voting as ext
    torch.cuda.synchronize()
    ext.shutdown()


def _check_v3(got, name, half=None):
    """test_gpu_parity._check_v3's rule: tn and the winners' inlier counts bit-exact, the means within tests/tolerances.py."""
    want, win, tn = _vote_want(name, half)
    np.testing.assert_array_equal(got["tn"], tn)
    np.testing.assert_array_equal(got["win"], win)
    tol.assert_means_close(got["out"], want)


def _v3_ext(name, count_kernel=None, half=None, device_rng=False):
    """One guarded ``ext.ransac_voting_v3`` call of the case as a ``call(g, m)``: the workspace it returns must be the size the library
    reports for that layout (injected idxs reserve draw storage, the device RNG does not)."""
    from clean_pvnet_amd import ransac_voting as ext
    c = VOTE_CASES[name]
    ck = ext.COUNT_AUTO if count_kernel is None else count_kernel

    def call(g, m):
        out, win, tn, ws = ext.ransac_voting_v3(g["mask"], g["vertex"], c["hn"], 0.99, 5, 30000, None if device_rng else g["idxs"], None, 11,
                                                ext.SINGULAR_REFERENCE, count_kernel=ck)
        assert ws.numel() == ext.workspace_bytes(c["B"], c["H"], c["W"], c["K"], c["hn"], 30000, 8, ck, device_rng)
        m.workspaces.append((ws.numel(), ws))
        return {"out": out, "win": win, "tn": tn}
    return call


def _vote_inputs(name, half=None):
    d, idxs, _tn = _vote_case(name)
    v = d["vertex"] if half is None else d["vertex"].to(getattr(torch, half))
    return {"mask": d["mask"], "vertex": v, "idxs": idxs}


@pytest.mark.parametrize("name", ["small", "bk129"])
def test_voting_v3_with_injected_index_pairs(oracle, pkg, gpu, name):
    got = guarded_runs(gpu, "v3 %s" % name, _vote_inputs(name), _v3_ext(name), workspace="ext", before=_shutdown)
    _check_v3(got, name)
    _shutdown()


def test_voting_v3_with_the_device_rng_takes_the_lean_workspace(oracle, pkg, gpu):
    """Nothing injected: PVV_FLAG_DEVICE_RNG, no draw storage in the workspace.  The keypoints equal the unguarded call's under the same
    seed as bytes, and recover the keypoints the field was built from (test_gpu_parity's rule for the free-running forms)."""
    from clean_pvnet_amd import ransac_voting as ext
    d, _idxs, tn = _vote_case("small")
    c = VOTE_CASES["small"]
    lean, full = (ext.workspace_bytes(c["B"], c["H"], c["W"], c["K"], c["hn"], 30000, 8, ext.COUNT_AUTO, rng) for rng in (True, False))
    assert lean < full
    got = guarded_runs(gpu, "v3 small, device RNG", _vote_inputs("small"), _v3_ext("small", device_rng=True), workspace="ext", before=_shutdown)
    _shutdown()
    out, win, tnn, _ws = ext.ransac_voting_v3(d["mask"].to(gpu), d["vertex"].to(gpu), c["hn"], 0.99, 5, 30000, None, None, 11, ext.SINGULAR_REFERENCE)
    assert _bits_equal(got["out"], out.cpu().numpy()) and _bits_equal(got["win"], win.cpu().numpy())
    assert got["tn"].tolist() == tn and np.abs(got["out"] - d["kpt_2d"].numpy()).max() < 6.0
    _shutdown()


@pytest.mark.parametrize("half", ["float16", "bfloat16"])
def test_voting_v3_on_a_half_precision_field(oracle, pkg, gpu, half):
    """The kernels widen as they read: the result is the oracle's on the widened field."""
    got = guarded_runs(gpu, "v3 small %s" % half, _vote_inputs("small", half), _v3_ext("small", half=half), workspace="ext", before=_shutdown)
    _check_v3(got, "small", half)
    _shutdown()


@pytest.mark.parametrize("kernel", ["COUNT_AUTO", "COUNT_STAGED"])
def test_voting_v3_at_the_smallest_shape_that_may_stage(oracle, pkg, gpu, kernel):
    """22 x 59 x 70, K = 9, hn = 512 (host_stage.hpp:41-42, worked out at VOTE_CASES): the workspace holds the leader words and
    the call leaves its stage hint; under COUNT_STAGED the all-foreground images are counted in stages."""
    from clean_pvnet_amd import ransac_voting as ext
    c = VOTE_CASES["stage"]
    d, _idxs, tn = _vote_case("stage")
    assert max(tn) == c["H"] * c["W"] > 7 * 4 * 128 and min(tn) < 7 * 4 * 128
    args = (c["B"], c["H"], c["W"], c["K"], c["hn"], 30000, 8)
    assert ext.workspace_bytes(*args, ext.COUNT_AUTO, False) > ext.workspace_bytes(*args, ext.COUNT_FULL, False)     # the leader words
    fewer = (c["B"] - 1,) + args[1:]                                                     # one image less: below the bound, nothing reserved
    assert ext.workspace_bytes(*fewer, ext.COUNT_AUTO, False) == ext.workspace_bytes(*fewer, ext.COUNT_FULL, False)
    call = _v3_ext("stage", count_kernel=getattr(ext, kernel))

    def with_hint(g, m):
        res = call(g, m)
        torch.cuda.synchronize()
        # AUTO leaves its hint for a problem that may stage (host_front.hpp: stage_hint_claim); a forced kernel does not consult it
        assert ext.stage_hint(g["mask"], g["vertex"], c["hn"])[0] == (kernel == "COUNT_AUTO")
        return res
    got = guarded_runs(gpu, "v3 stage %s" % kernel, _vote_inputs("stage"), with_hint, workspace="ext", before=_shutdown)
    _check_v3(got, "stage")
    _shutdown()
    assert not ext.stage_hint(d["mask"].to(gpu), d["vertex"].to(gpu), c["hn"])[0]


def test_voting_layers_and_the_c_abi(oracle, pkg, gpu):
    """``ransac_voting_layer_v3`` / ``ransac_voting_layer`` through the drop-in path and ``pvv_ransac_voting_v3`` through ctypes
    (tests/capi.py allocates out, win, tn and a workspace of exactly ``pvv_workspace_bytes`` with torch.empty: all carved)."""
    from lib.csrc.ransac_voting.ransac_voting_gpu import ransac_voting_layer, ransac_voting_layer_v3
    want, win, tn = _vote_want("small")

    def layers(g, m):
        a = ransac_voting_layer_v3(g["mask"], g["vertex"], 64, inlier_thresh=0.99, idxs=g["idxs"])
        b = ransac_voting_layer(g["mask"], g["vertex"], 64, inlier_thresh=0.99, idxs=g["idxs"])
        ws = [x for x in m.arenas if x.kind == "factory" and x.dtype == torch.uint8 and len(x.shape) == 1]
        assert len(ws) == 2
        m.workspaces.extend((x.n, x.body) for x in ws)
        return {"v3": a, "v1": b}
    got = guarded_runs(gpu, "voting layers", _vote_inputs("small"), layers, workspace="ext", before=_shutdown)
    tol.assert_means_close(got["v3"], want)
    tol.assert_means_close(got["v1"], want)                                              # no singular keypoint: v1 is v3

    def cabi(g, m):
        out, w, t = capi.v3(g["mask"], g["vertex"], 64, 0.99, idxs=g["idxs"])
        ws = [x for x in m.arenas if x.kind == "factory" and x.dtype == torch.uint8 and len(x.shape) == 1]
        assert len(ws) == 1
        m.workspaces.append((ws[0].n, ws[0].body))
        return {"out": out, "win": w, "tn": t}
    _check_v3(guarded_runs(gpu, "pvv_ransac_voting_v3", _vote_inputs("small"), cabi, workspace="ext", before=_shutdown), "small")
    _shutdown()


def _ext_workspaces(m, n):
    ws = [x for x in m.arenas if x.kind == "factory" and x.dtype == torch.uint8 and len(x.shape) == 1]
    assert len(ws) == n, [(x.op, x.shape) for x in ws]
    m.workspaces.extend((x.n, x.body) for x in ws)


def test_estimate_voting_distribution_with_mean(oracle, pkg, gpu):
    """test_gpu_parity.test_estimate_parity's rule: covariances within tests/tolerances.py, hypotheses and ratios bit-exact."""
    from lib.csrc.ransac_voting.ransac_voting_gpu import estimate_voting_distribution_with_mean
    from clean_pvnet_amd import synth
    d, _i, tn = _vote_case("small")
    K = VOTE_CASES["small"]["K"]
    assert tn == [int(x) for x in (d["mask"] == 1).sum((1, 2))]
    idxs = synth.make_idxs(tn, 256, K, seed=77)
    mean = d["kpt_2d"] + 0.25
    det = []
    _m, want = oracle.estimate_voting_distribution_with_mean(d["mask"].numpy(), d["vertex"].numpy(), mean.numpy(), 64, 256, idxs=idxs.numpy(), details=det)

    def call(g, m):
        ret, cov, hyp, ratio = estimate_voting_distribution_with_mean(g["mask"], g["vertex"], g["mean"], 64, 256, idxs=g["idxs"], output_hyp=True)
        assert ret is g["mean"]
        lean = estimate_voting_distribution_with_mean(g["mask"], g["vertex"], g["mean"], 64, 256, return_weights=True, seed=3)   # device RNG, no counts
        _ext_workspaces(m, 2)
        return {"cov": cov, "hyp": hyp, "ratio": ratio, "cov_rng": lean[1], "weights_rng": lean[2]}
    got = guarded_runs(gpu, "estimate", {"mask": d["mask"], "vertex": d["vertex"], "mean": mean, "idxs": idxs}, call, workspace="ext",
                       derived=("hyp", "ratio"), before=_shutdown)                       # (torch.cat / a division of the counts: ransac_voting_gpu.py:183-188)
    tol.assert_cov_close(got["cov"], want)
    for b in range(2):
        np.testing.assert_array_equal(got["hyp"][b].view(np.uint32), det[b]["hypo_pts"].transpose(1, 0, 2).view(np.uint32))
        np.testing.assert_array_equal(got["ratio"][b], (det[b]["counts"].astype(np.float32) / np.float32(det[b]["tn"])).T)
    assert np.isfinite(got["cov_rng"]).all() and (got["cov_rng"][:, :, 0, 0] > 0).all() and np.isfinite(got["weights_rng"]).all()
    _shutdown()


def test_decode_keypoint_v3_and_un_pnp(oracle, pkg, gpu):
    """The scenario of test_gpu_parity.test_decode_keypoint_un_pnp_one_pass_equals_the_two_calls at 45 x 70: ``decode_keypoint_v3``
    and the fused ``decode_keypoint_un_pnp`` on injected draws against the oracle by that test's rule, and the dict mirror
    ``decode.decode_keypoint`` in both branches (device RNG) against the unguarded call under the same seed."""
    from clean_pvnet_amd import ransac_voting as ext, synth
    from clean_pvnet_amd.decode import decode_keypoint
    B, H, W, K, hn, hn_est = 3, 45, 70, 5, 64, 160
    d = synth.make_batch(B=B, H=H, W=W, K=K, fg=0.10, sigma=0.05, seed=91, planar=True)
    x = torch.empty(B, 2 + 2 * K, H, W)
    x[:, :2] = torch.randn(B, 2, H, W, generator=torch.Generator().manual_seed(2)) * 0.1
    x[:, 0] += 1.0
    x[:, 1][d["mask"] != 0] += 4.0
    x[2, 1] = -9.0                                                                       # an image without foreground
    x[:, 2:] = d["vertex"].permute(0, 3, 4, 1, 2).reshape(B, 2 * K, H, W)
    mask_ref = torch.argmax(x[:, :2], 1)
    vertex_ref = x[:, 2:].permute(0, 2, 3, 1).reshape(B, H, W, K, 2)
    tn = [int(v) for v in (mask_ref != 0).sum((1, 2))]
    assert tn[2] == 0 and min(tn[:2]) > 100
    idxs, idxs_est = synth.make_idxs(tn, hn, K, seed=91), synth.make_idxs(tn, hn_est, K, seed=92)
    want = oracle.ransac_voting_layer_v3(mask_ref.numpy(), vertex_ref.numpy(), hn, 0.99, idxs=idxs.numpy())
    _m, want_cov = oracle.estimate_voting_distribution_with_mean(mask_ref.numpy(), vertex_ref.numpy(), want, hn_est, hn_est, idxs=idxs_est.numpy())

    def call(g, m):
        seg, ver = g["x"][:, :2], g["x"][:, 2:]                                          # channel slices of one tensor, read in place
        vertex = ver.permute(0, 2, 3, 1).view(B, H, W, K, 2)
        kpt2, mask2, win2, tn2 = ext.decode_keypoint_v3(seg, vertex, hn, 0.99, 5, 30000, g["idxs"], None, 0, ext.SINGULAR_REFERENCE)
        kpt, mask, cov, w, win, tnn = ext.decode_keypoint_un_pnp(seg, vertex, hn, hn_est, 0.99, 5, 30000, g["idxs"], g["idxs_est"], None, 0,
                                                                 ext.SINGULAR_REFERENCE)
        _ext_workspaces(m, 2)
        plain = decode_keypoint({"seg": seg, "vertex": ver}, un_pnp=False, seed=4)
        fused = decode_keypoint({"seg": seg, "vertex": ver}, un_pnp=True, weights=True, seed=4)
        keys = ("mask", "kpt_2d", "var", "var_weights")
        return {"v3": (kpt2, mask2, win2, tn2), "un_pnp": (kpt, mask, cov, w, win, tnn), "plain": {k: plain[k] for k in keys[:2]},
                "fused": {k: fused[k] for k in keys}}
    got = guarded_runs(gpu, "decode_keypoint", {"x": x, "idxs": idxs, "idxs_est": idxs_est}, call, workspace="ext", before=_shutdown)
    kpt, mask, cov, w, win, tnn = got["un_pnp"]
    for a, b in zip(got["v3"], (kpt, mask, win, tnn)):
        assert _bits_equal(a, b)
    np.testing.assert_array_equal(mask, mask_ref.numpy())
    assert tnn.tolist() == tn
    tol.assert_means_close(kpt, want)
    np.testing.assert_allclose(cov, want_cov, rtol=1e-3, atol=1e-3)                      # (the mean differs by <= 1e-4 px from the oracle's)
    _shutdown()
    xd = x.to(gpu)
    for key, kw in (("plain", dict(un_pnp=False)), ("fused", dict(un_pnp=True, weights=True))):
        o = decode_keypoint({"seg": xd[:, :2], "vertex": xd[:, 2:]}, seed=4, **kw)
        for k in got[key]:
            assert _bits_equal(got[key][k], o[k].cpu().numpy()), (key, k)
    _shutdown()


def test_legacy_kernels_and_count_inliers(oracle, pkg, gpu):
    """The reference's four kernels and ``count_inliers`` on the compacted first image of the small batch (test_gpu_parity's
    rule: every output bit-exact).  The two voting kernels write into a caller's zeroed buffer: it is made inside the mode."""
    from clean_pvnet_amd import ransac_voting as ext
    d, _i, _tn = _vote_case("small")
    _fg, coords, direct = oracle.compact_v3(d["mask"][0].numpy(), d["vertex"][0].numpy())
    tn, vn, _ = direct.shape
    hn = 37
    idxs = np.random.RandomState(1).randint(0, tn, size=(hn, vn, 2)).astype(np.int32)
    idxs[0, :, 1] = idxs[0, :, 0]                                                        # degenerate -> (0, 0)
    want = {"hyp": oracle.generate_hypothesis(direct, coords, idxs), "hyp_vp": oracle.generate_hypothesis_vanishing_point(direct, coords, idxs)}
    want["inl"] = oracle.voting_for_hypothesis(direct, coords, want["hyp"], np.zeros((hn, vn, tn), np.uint8), 0.99)
    want["inl_vp"] = oracle.voting_for_hypothesis_vanishing_point(direct, coords, want["hyp_vp"], np.zeros((hn, vn, tn), np.uint8), 0.99)
    want["counts"] = oracle.count_inliers(direct, coords, want["hyp"], 0.99)
    assert tn % 64 and want["inl"].sum() > 0 and want["inl_vp"].sum() > 0

    def call(g, m):
        hyp = ext.generate_hypothesis(g["direct"], g["coords"], g["idxs"])
        hyp_vp = ext.generate_hypothesis_vanishing_point(g["direct"], g["coords"], g["idxs"])
        inl, inl_vp = torch.zeros(hn, vn, tn, dtype=torch.uint8, device=gpu), torch.zeros(hn, vn, tn, dtype=torch.uint8, device=gpu)
        ext.voting_for_hypothesis(g["direct"], g["coords"], hyp, inl, 0.99)
        ext.voting_for_hypothesis_vanishing_point(g["direct"], g["coords"], hyp_vp, inl_vp, 0.99)
        counts = ext.count_inliers(g["direct"], g["coords"], hyp, 0.99)
        return {"hyp": hyp, "hyp_vp": hyp_vp, "inl": inl, "inl_vp": inl_vp, "counts": counts}
    got = guarded_runs(gpu, "legacy kernels", {"direct": direct, "coords": coords, "idxs": idxs}, call, workspace=False)
    for k in want:
        assert _bits_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------------------ crop
def test_decode_ct_hm(pkg, gpu):
    """test_gpu_crop's smallest heat maps (the tie case, 1 x 2 x 8 x 8, and the short case, B = 3) and the 3 x 4 x 34 x 45, K = 20
    maps of test_gpu_det_eval.test_decoded_heat_maps_run_through: (ct, det, count) equal the twin bit for bit."""
    from clean_pvnet_amd.crop import decode_ct_hm
    from tests import crop_twin as twin
    rng = np.random.default_rng(11)
    B, C, H, W = 3, 4, 34, 45
    hm = rng.uniform(0, 0.3, (B, C, H, W)).astype(np.float32)
    for b in range(B):
        for _ in range(12 if b else 0):
            hm[b, rng.integers(C), rng.integers(H), rng.integers(W)] = rng.uniform(0.4, 1.0)
    hm[0] = 0
    wh = rng.uniform(2, 14, (B, 2, H, W)).astype(np.float32)
    for what, (h, w, K) in (("tie", twin.tie_case()), ("short", twin.short_case()), ("34x45 K=20", (hm, wh, 20))):
        got = guarded_runs(gpu, "decode_ct_hm %s" % what, {"hm": h, "wh": w}, lambda g, m: decode_ct_hm(g["hm"], g["wh"], K=K), workspace=True)
        want = twin.decode_ct_hm(h, w, K=K)
        assert all(_bits_equal(a, b) for a, b in zip(got, want)), what


def test_crops_and_the_ways_back(pkg, gpu):
    """test_gpu_crop: the 32 x 32 crops of six boxes (one invalid) and the odd 70 x 37 output, ``uncrop_keypoints`` (K = 9, N = 5)
    and ``uncrop_mask`` onto the 71 x 53 canvas (the byte-wise store), each equal to the twin bit for bit."""
    from clean_pvnet_amd.crop import crop_boxes, uncrop_keypoints, uncrop_mask
    from tests import crop_twin as twin
    from tests.test_gpu_crop import KW, _crop_inputs
    img, boxes, index = _crop_inputs()
    for out_size, ratio in (((32, 32), None), ((70, 37), 0.9)):
        want = twin.crop_boxes(img, boxes, index, out_size, box_ratio=ratio, **KW)
        want.pop("u8")
        got = guarded_runs(gpu, "crop_boxes %s" % (out_size,), {"img": img, "boxes": boxes, "index": index},
                           lambda g, m: crop_boxes(g["img"], g["boxes"], g["index"], out_size, box_ratio=ratio, **KW), workspace=True)
        assert set(got) == set(want) and all(_bits_equal(got[k], want[k]) for k in want), out_size
    rng = np.random.default_rng(7)
    kpt = rng.random((5, 9, 2)) * 256 - 20
    trans = np.stack([twin.box_transform(b, (256, 256), twin.SCALE_RATIO)[2] for b in twin.BOXES])
    trans[3] = 0
    got = guarded_runs(gpu, "uncrop_keypoints", {"kpt": kpt, "trans": trans}, lambda g, m: uncrop_keypoints(g["kpt"], g["trans"]), workspace=False)
    assert _bits_equal(got, twin.uncrop_keypoints(kpt, trans))
    canvas = (71, 53)
    rng = np.random.default_rng(9)
    mask = (rng.random((3, 40, 48)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (3, 40, 48)).astype(np.uint8)
    trans = np.stack([twin.box_transform(np.asarray(b) * canvas[0] / 72.0, (48, 40), twin.SCALE_RATIO)[2] for b in twin.BOXES[[0, 1, 4]]])
    got = guarded_runs(gpu, "uncrop_mask", {"mask": mask, "trans": trans}, lambda g, m: uncrop_mask(g["mask"], g["trans"], canvas), workspace=False)
    assert _bits_equal(got, twin.uncrop_mask(mask, trans, canvas))


# ------------------------------------------------------------------------------------------------------------ dcn, dcn_train
DCN_CASES = ("odd_k_small_m", "uncached_odd_group", "two_groups_m33")      # P no multiple of 128; KK > 9; M no multiple of 32


@pytest.mark.parametrize("name", DCN_CASES)
def test_dcn_forward_columns_and_backward(pkg, gpu, name):
    """test_gpu_dcn / test_gpu_dcn_train: the output, the columns and the five gradients equal the twins bit for bit (-0 as +0;
    grad_weight and grad_bias not even a zero's sign)."""
    from clean_pvnet_amd import dcn, dcn_train
    from tests import dcn_train_twin, dcn_twin
    d = dcn_train_twin.reference(name)
    geo = (d["stride"], d["padding"], d["dilation"], d["dg"])
    inputs = {k: d[k] for k in ("input", "offset", "mask", "weight", "bias", "gout")}

    def forward(g, m):
        return {"out": dcn.dcn_v2_conv(g["input"], g["offset"], g["mask"], g["weight"], g["bias"], *geo),
                "col": dcn.columns(g["input"], g["offset"], g["mask"], d["kernel"], *geo)}
    got = guarded_runs(gpu, "dcn %s" % name, inputs, forward, workspace=False)
    assert dcn_twin.same_bits(got["out"], d["out"]) and dcn_twin.same_bits(got["col"], d["col"])

    def backward(g, m):
        grads = dcn_train.dcn_v2_backward(g["input"], g["offset"], g["mask"], g["weight"], g["bias"], g["gout"], *geo)
        leaves = [g[k].requires_grad_(True) for k in ("input", "offset", "mask", "weight", "bias")]
        out = dcn_train.dcn_v2_conv(*leaves, *geo)
        through = torch.autograd.grad(out, leaves, g["gout"])
        return {"grads": list(grads), "out": out.detach(), "through": list(through)}
    got = guarded_runs(gpu, "dcn_train %s" % name, inputs, backward, workspace=True)
    for a, b, w in zip(got["grads"], got["through"], d["grads"]):
        assert dcn_twin.same_bits(a, w) and _bits_equal(a, b)
    assert _bits_equal(got["grads"][3], d["grads"][3]) and _bits_equal(got["grads"][4], d["grads"][4])
    assert dcn_twin.same_bits(got["out"], d["out"])


# ------------------------------------------------------------------------------------------------------------ train, ct_train
@pytest.mark.parametrize("form", ["kpt_2d", "vertex"])
def test_pvnet_targets_and_losses(pkg, gpu, form):
    """test_gpu_train's smallest case, 2 x 37 x 53 (H * W odd: the scalar form, a partial tile): the target, the vote loss and
    the vote gradient as bytes, the seg loss and gradient within a neighbouring float32."""
    from clean_pvnet_amd.train import compute_vertex, pvnet_loss
    from tests import train_twin as twin
    d = twin.reference("scalar_37x53")

    def call(g, m):
        vp, sp = g["vertex_pred"].requires_grad_(True), g["seg_pred"].requires_grad_(True)
        target = compute_vertex(g["mask"], g["kpt_2d"])
        vote, seg = pvnet_loss(vp, sp, g["mask"], **({"kpt_2d": g["kpt_2d"]} if form == "kpt_2d" else {"vertex": g["target"]}))
        gv, gs = torch.autograd.grad([vote, seg], [vp, sp], [torch.ones_like(vote), torch.ones_like(seg)])
        return {"target": target, "vote_loss": vote.detach(), "seg_loss": seg.detach(), "vote_grad": gv, "seg_grad": gs}
    got = guarded_runs(gpu, "pvnet_loss %s" % form, {k: d[k] for k in ("vertex_pred", "seg_pred", "mask", "kpt_2d", "target")}, call, workspace=True)
    for k in ("target", "vote_loss", "vote_grad"):
        assert _bits_equal(got[k], d[k]), k
    assert twin.ulp_apart(got["seg_loss"], d["seg_loss"]) <= 1 and twin.ulp_apart(got["seg_grad"], d["seg_grad"]).max() <= 1


def test_ct_targets_and_losses(pkg, gpu):
    """test_gpu_ct_train's smallest case, 1 x 4 x 8 x 12 (the 16-byte form, less than a tile, N = 1), and the targets of
    3 x 30 x 34 x 45 (N = 130, an image with num = 0), by that module's rules."""
    from clean_pvnet_amd.ct_train import ct_loss, ct_targets
    from tests import ct_train_twin as twin
    keys = ("ct_hm", "wh", "ct_cls", "ct_ind", "ct_01", "ct_num")
    for name in ("vec_4x8x12", "c30_34x45_int"):
        d = twin.reference(name)
        got = guarded_runs(gpu, "ct_targets %s" % name, {k: d[k] for k in ("boxes", "cls", "num")},
                           lambda g, m: dict(zip(keys, ct_targets(g["boxes"], g["cls"], g["num"], d["C"], d["H"], d["W"]))), workspace=False)
        for k in keys[1:]:
            assert _bits_equal(got[k], d[k]), (name, k)
        assert np.array_equal(got["ct_hm"] == 1, d["ct_hm"] == 1) and np.array_equal(got["ct_hm"] == 0, d["ct_hm"] == 0)
        assert twin.ulp_apart(got["ct_hm"], d["ct_hm"]).max() <= 1 and not np.signbit(got["ct_hm"]).any()
    d = twin.reference("vec_4x8x12")

    def call(g, m):
        hp, wp = g["ct_hm_pred"].requires_grad_(True), g["wh_pred"].requires_grad_(True)
        ct, wh = ct_loss(hp, wp, g["ct_hm"], g["wh"], g["ct_ind"], g["ct_01"])
        gh, gw = torch.autograd.grad([ct, wh], [hp, wp], [torch.ones_like(ct), torch.ones_like(wh)])
        return {"ct_loss": ct.detach(), "wh_loss": wh.detach(), "hm_grad": gh, "wh_grad": gw}
    got = guarded_runs(gpu, "ct_loss", {k: d[k] for k in ("ct_hm_pred", "wh_pred", "ct_hm", "wh", "ct_ind", "ct_01")}, call, workspace=True)
    assert twin.ulp_apart(got["ct_loss"], d["ct_loss"]) <= 1 and twin.ulp_apart(got["wh_loss"], d["wh_loss"]) <= 1
    assert twin.ulp_apart(got["hm_grad"], d["hm_grad"]).max() <= 1 and np.array_equal(got["hm_grad"] == 0, d["hm_grad"] == 0)
    assert _bits_equal(got["wh_grad"], d["wh_grad"])


# ------------------------------------------------------------------------------------------------------------ augment, ct_augment
def test_pvnet_augment_and_transform(pkg, gpu):
    """test_gpu_augment: the mixed batch (B = 5, 48 x 70 -> 40 x 66: crop, pad, an empty and a single-pixel mask) and the
    transform of four 40 x 66 images with a blur and all four jitter steps, as bytes."""
    from clean_pvnet_amd.augment import pvnet_augment, pvnet_transform
    from tests import augment_twin as twin
    img, mask, kpt, d = twin.mixed_batch((40, 66))
    want = twin.pvnet_augment(img, mask, kpt, (40, 66), d, **twin.MIXED_KW)
    got = guarded_runs(gpu, "pvnet_augment", {"img": img, "mask": mask, "kpt": kpt},
                       lambda g, m: pvnet_augment(g["img"], g["mask"], g["kpt"], (40, 66), d, **twin.MIXED_KW), workspace=True)
    assert all(_bits_equal(got[k], want[k]) for k in ("img", "mask", "kpt_2d", "path", "window"))
    img = np.stack([twin.image(50 + i, 40, 66) for i in range(4)])
    d = twin.draws_for(4, 9)
    d[:, 4], d[:, 10] = 0.1, (np.array([0, 7, 14, 21]) + 0.5) / 24
    amp = (0.4, 0.4, 0.4, 0.5)
    got = guarded_runs(gpu, "pvnet_transform", {"img": img}, lambda g, m: pvnet_transform(g["img"], d, jitter=amp, mean=twin.MEAN, std=twin.STD),
                       workspace=True)
    assert _bits_equal(got, twin.pvnet_transform(img, d, jitter=amp))
    got = guarded_runs(gpu, "pvnet_transform, no draws", {"img": img}, lambda g, m: pvnet_transform(g["img"], None, mean=twin.MEAN, std=twin.STD),
                       workspace=False)
    assert _bits_equal(got, twin.pvnet_transform(img, None))


def test_ct_compose_and_augment(pkg, gpu):
    """test_gpu_ct_augment's smallest case: B = 1 on the 30 x 50 canvas, N = 3, input_size (44, 72), and (44, 70), whose width takes
    the one-pixel-per-lane colour kernel; every output as bytes.  ``center``, ``scale`` and the two ``trans_*`` are host tensors
    (ct_augment.py: "as host tensors: they are functions of the draws alone"), so only their values are compared."""
    from clean_pvnet_amd import ct_augment
    from tests import ct_augment_twin as twin
    for B, input_size, boxes in ((1, (44, 72), "linear"), (5, (44, 70), "linear")):
        bg, inst_img, inst_mask, _cls, num, d = twin.batch(B, 50 + B)
        N = inst_img.shape[1]
        want_c = twin.compose(bg, inst_img, inst_mask, num, d)
        want_a = twin.augment(want_c["img"], want_c["label"], d, n_instances=N, input_size=input_size, boxes=boxes)

        def call(g, m):
            c = ct_augment.ct_compose(g["bg"], g["inst_img"], g["inst_mask"], g["num"], d)
            return {"compose": c, "augment": ct_augment.ct_augment(c["img"], c["label"], d, n_instances=N, input_size=input_size, boxes=boxes)}
        got = guarded_runs(gpu, "ct_augment B=%d %s" % (B, input_size), {"bg": bg, "inst_img": inst_img, "inst_mask": inst_mask, "num": num},
                           call, workspace=True)
        assert all(_bits_equal(got["compose"][k], want_c[k]) for k in ("img", "label", "place"))
        for k in ("inp", "orig_img", "boxes", "center", "scale", "trans_input", "trans_output"):
            assert _bits_equal(got["augment"][k], want_a[k]), k


# ------------------------------------------------------------------------------------------------------------ model
def test_model_fps_diameter_and_bounds(pkg, gpu):
    """test_gpu_model's smallest clouds (n = 1, 2, 63, 65 of every kind) in both forms of the sampling, and the tiled kernels'
    partial tile (n = 2 * 1024 + 17): indices, diameter and bounds equal the twin as bytes."""
    from clean_pvnet_amd import model
    from tests import model_twin as twin
    for n in (1, 2, 63, 65, 2 * twin.TILE + 17):
        kinds = twin.KINDS if n < 100 else ("gauss",)
        for kind in kinds:
            p = twin.cloud(kind, n, twin.kind_seed(kind, n))
            sn = max(twin.sample_counts(n)) if n < 100 else 8
            start = n // 2

            def call(g, m):
                out = {"one_block": model.farthest_point_sampling(g["p"], sn, True, path=model.ONE_BLOCK),
                       "tiled": model.farthest_point_sampling(g["p"], sn, False, start, path=model.TILED),
                       "diameter": model.diameter(g["p"][None])}
                out["lo"], out["hi"] = model.bounds(g["p"][None])
                return out
            got = guarded_runs(gpu, "model %s n=%d" % (kind, n), {"p": p}, call, workspace=True)
            assert _bits_equal(got["one_block"], twin.fps(p, sn)) and _bits_equal(got["tiled"], twin.fps(p, sn, start)), (kind, n)
            assert _bits_equal(got["diameter"], np.array([twin.diameter(p)])), (kind, n)
            assert np.array_equal(got["lo"][0], p.min(0)) and np.array_equal(got["hi"][0], p.max(0))


# ------------------------------------------------------------------------------------------------------------ pose, un_pnp_utils
def test_solve_pose_and_the_batched_refinement(pkg, gpu):
    """test_gpu_pose's smallest batches (four problems of 4 and of 9 keypoints): the P3P start against the host twin within that
    test's tolerance, ``solve_pose`` in both branches and ``uncertainty_pnp_batched`` from a given start against the unguarded
    call as bytes (test_batch_layouts_failures_and_determinism: two identical calls give the same bits) and, at 9 keypoints,
    at the minimum scipy finds (``_same_minimum``)."""
    from clean_pvnet_amd.pose import initial_pose_batched, solve_pose
    from clean_pvnet_amd.un_pnp_utils import initial_pose_dlt, uncertainty_pnp_batched
    from oracle import pnp_oracle as po
    from tests.test_gpu_pose import CASES, _same_minimum, _start_tolerance, _twin_start
    from tests.test_pnp import KMAT, problem
    for pn in (4, 9):
        probs = [problem(s, pn=pn, noise=n)[:3] for s, p, n in CASES if p == pn]
        inputs = {"p2": np.stack([q[0] for q in probs]), "P": np.stack([q[1] for q in probs]), "W": np.stack([q[2] for q in probs]),
                  "K": np.asarray(KMAT, np.float64)}
        starts = [_twin_start(P, p2, W) for p2, P, W in probs]
        assert all(s[0] is not None for s in starts)
        inputs["rt0"] = np.stack([s[0] for s in starts])

        def call(g, m):
            rt, st = initial_pose_batched(g["p2"], g["P"], g["K"], g["W"], method="p3p")
            o = solve_pose({"kpt_2d": g["p2"], "var_weights": g["W"]}, g["P"], g["K"], un_pnp=True)
            out = {"start": rt, "start_status": st, "pose_un": o["pose"], "status_un": o["pose_status"]}
            if pn >= 6:
                o = solve_pose({"kpt_2d": g["p2"]}, g["P"], g["K"])
                out.update(pose=o["pose"], status=o["pose_status"])
                out["refined"], out["info"] = uncertainty_pnp_batched(g["p2"], g["W"], g["P"], g["K"], g["rt0"], max_iterations=200,
                                                                      function_tolerance=1e-15, return_info=True)
            return out
        got = guarded_runs(gpu, "pose pn=%d" % pn, inputs, call, workspace=False)
        for i, (p2, P, W) in enumerate(probs):
            assert got["start_status"][i] == starts[i][1]
            np.testing.assert_allclose(got["start"][i], starts[i][0], rtol=0, atol=_start_tolerance(P, p2, W, starts[i][0]))
        dev = {k: torch.tensor(v, device=gpu) for k, v in inputs.items()}
        o = solve_pose({"kpt_2d": dev["p2"], "var_weights": dev["W"]}, dev["P"], dev["K"], un_pnp=True)
        assert _bits_equal(got["pose_un"], o["pose"].cpu().numpy()) and _bits_equal(got["status_un"], o["pose_status"].cpu().numpy())
        assert (got["status_un"] == 0).all() and np.isfinite(got["pose_un"]).all()
        if pn >= 6:
            o = solve_pose({"kpt_2d": dev["p2"]}, dev["P"], dev["K"])
            assert _bits_equal(got["pose"], o["pose"].cpu().numpy()) and (got["status"] == 1).all()
            for i, (p2, P, W) in enumerate(probs):
                xs, _ = po.solve_scipy(starts[i][0], p2, P, W, KMAT)
                if max(float(np.abs(po.rodrigues(got["refined"][i, :3]) - po.rodrigues(xs[:3])).max()), float(np.abs(got["refined"][i, 3:] - xs[3:]).max())) <= 1e-3:
                    _same_minimum(got["refined"][i], xs, p2, P, W, ("scipy", pn, i))
                one = np.tile([1.0, 0.0, 1.0], (pn, 1))
                xs, _ = po.solve_scipy(initial_pose_dlt(P, p2, KMAT), p2, P, one, KMAT)
                np.testing.assert_allclose(got["pose"][i, :, :3], po.rodrigues(xs[:3]), atol=1e-5)
                np.testing.assert_allclose(got["pose"][i, :, 3], xs[3:], atol=1e-5)


# ------------------------------------------------------------------------------------------------------------ metrics
@pytest.mark.parametrize("n", [1, 255])
def test_pose_metrics_and_the_mask_counts(oracle, pkg, gpu, n):
    """test_gpu_metrics.test_adds_search_bit_exact_for_every_slab_count at its smallest clouds, b = 3: the neighbour indices equal
    the oracle's, the values lie within tests/metrics_twin.py's bounds; the mask counts equal the fixture's."""
    from clean_pvnet_amd.metrics import mask_counts, pose_metrics
    from tests import metrics_twin as twin
    from tests.test_gpu_metrics import VALUES, _poses
    b = 3
    model = twin.cloud(n, 100 + n)
    Pp, Pg = _poses(b, 7 * n + b)
    want_idx = np.stack([oracle.find_nearest_point_idx(twin.transform(model, Pp[i]).astype(np.float32), twin.transform(model, Pg[i]).astype(np.float32))
                         for i in range(b)])
    c = load("metrics_masks")
    inputs = {"Pp": Pp, "Pg": Pg, "model": model, "K": twin.LINEMOD_K, "mp": c["mask_pred"].astype(np.int64), "mg": c["mask_gt"]}

    def call(g, m):
        out = {slabs: pose_metrics(g["Pp"], g["Pg"], g["model"], g["K"], symmetric=True, return_idx=True, slabs=slabs) for slabs in (0, 7)}
        out["inter"], out["union"] = mask_counts(g["mp"], g["mg"])
        return out
    got = guarded_runs(gpu, "pose_metrics n=%d" % n, inputs, call, workspace=True)
    for slabs in (0, 7):
        np.testing.assert_array_equal(got[slabs]["adds_idx"], want_idx)
        for i in range(b):
            ref = twin.pose_metrics(Pp[i], Pg[i], model, twin.LINEMOD_K, search=oracle.find_nearest_point_idx)
            twin.assert_close({k: float(got[slabs][k][i]) for k in VALUES}, ref, n, what="n=%d image %d" % (n, i))
    assert _bits_equal(got[0]["adds"], got[7]["adds"])
    np.testing.assert_array_equal(got["inter"], c["inter"])
    np.testing.assert_array_equal(got["union"], c["union"])


# ------------------------------------------------------------------------------------------------------------ vsd
def test_render_depth_on_the_clip_and_size_class_meshes(pkg, gpu):
    """test_gpu_vsd_rules: the clip mesh (29 x 23: P * H * W % 4 = 3, the scalar tail of the resolve pass) and the size-class
    mesh equal the twin as float32 bit patterns."""
    from clean_pvnet_amd.vsd import render_depth
    from tests import vsd_twin as twin
    for what, s in (("clip", twin.clip_mesh()), ("size classes", twin.size_class_mesh())):
        want = twin.render_depth(s["pts"], s["faces"], s["pose"], s["K"], s["size"], s["near"], s["far"])
        inputs = {"pts": s["pts"], "faces": s["faces"], "pose": np.asarray(s["pose"], np.float64)[None], "K": np.asarray(s["K"], np.float64)}
        got = guarded_runs(gpu, "render_depth %s" % what, inputs,
                           lambda g, m: render_depth(g["pts"], g["faces"], g["pose"], g["K"], s["size"], s["near"], s["far"]), workspace=True)
        assert (want > 0).any() and _bits_equal(got[0], want), what


def test_vsd_evaluator(pkg, gpu):
    """``VsdEvaluator.evaluate`` on the clip and size-class meshes: two predictions (the mesh's pose and a shifted one) against the
    ground truth on a sensor image that is the ground-truth render (float32, model units).  ``e`` equals the twin's ``vsd_pair``
    on the twin's renders exactly (test_gpu_vsd's rule for the fixed-order sums); ``hits`` is a comparison of ``e`` made by torch."""
    from clean_pvnet_amd.vsd import VsdEvaluator
    from tests import vsd_twin as twin
    for what, s in (("clip", twin.clip_mesh()), ("size classes", twin.size_class_mesh())):
        pose = np.asarray(s["pose"], np.float64)
        moved = pose.copy()
        moved[:, 3] += [0.03, 0.0, 0.25]                                                 # (the meshes lie 1 to 16 units in front of the camera)
        renders = [twin.render_depth(s["pts"], s["faces"], p, s["K"], s["size"], s["near"], s["far"]) for p in (pose, moved)]
        sensor = renders[0].astype(np.float32)
        delta, tau = 0.5, 1.0
        want = np.array([[[twin.vsd_pair(r, renders[0], sensor.astype(np.float64), s["K"], delta, tau, "step")["e"]] for r in renders]])
        inputs = {"est": np.stack([pose, moved])[None], "gt": pose[None, None], "sensor": sensor[None], "K": np.asarray(s["K"], np.float64),
                  "pts": np.asarray(s["pts"], np.float32), "faces": np.asarray(s["faces"], np.int32)}

        def call(g, m):
            ev = VsdEvaluator(g["pts"], g["faces"], s["size"], error_thresh=0.3, delta=delta, tau=tau, depth_scale=1.0, t_scale=1.0,
                              near=s["near"], far=s["far"], device=gpu)
            hits = ev.evaluate(g["est"], g["gt"], g["sensor"], g["K"])
            return {"e": ev.last["e"], "hits": hits}
        got = guarded_runs(gpu, "VsdEvaluator %s" % what, inputs, call, workspace=True, derived=("hits",))   # (vsd.py:212: e < thresh, any)
        print("%s: e %s twin %s" % (what, got["e"].tolist(), want.tolist()))
        assert _bits_equal(got["e"], want) and got["e"][0, 0, 0] == 0.0 and 0.1 < got["e"][0, 1, 0] < 0.5 and got["hits"].tolist() == [True]


# ------------------------------------------------------------------------------------------------------------ icp
def test_icp_refine_with_injected_samples(pkg, gpu):
    """test_gpu_icp on ``icp_edge``: both stages with the fixture's samples equal the twin as binary64 bit patterns, the info
    columns are equal (``state`` array and the renders are temporaries of the call: carved and checked)."""
    from clean_pvnet_amd.icp import refine
    from tests import icp_twin as twin
    from tests import vsd_twin as vt
    from tests.test_gpu_icp import INFO, STAGE
    c = load("icp_edge")
    r = twin.regenerate("icp_edge", c)
    kw = dict(depth_scale=float(c["depth_scale"]), n_max=int(c["n_max"]), tolerance=float(c["tolerance"]), angle_limit_deg=float(c["angle_limit_deg"]))
    starts = (vt.scaled(c["pose_est"], float(c["t_scale"])), c["twin_stage"][0])
    for s in range(2):
        inputs = {"raw": torch.from_numpy(r["raw"]), "start": np.asarray(starts[s], np.float64), "K": c["K"], "pts": r["pts"], "faces": r["faces"],
                  "mask": r["mask"], "syn": c["idx"][s, 0], "real": c["idx"][s, 1]}

        def call(g, m):
            out, info = refine(g["raw"], g["start"], g["K"], g["pts"], g["faces"], mask=g["mask"], samples=(g["syn"], g["real"]),
                               return_info=True, **STAGE[s], **kw)
            return {"pose": out, "info": torch.stack([info[k] for k in INFO], 1), "columns": info}
        got = guarded_runs(gpu, "icp_edge stage %d" % (s + 1), inputs, call, workspace=True, derived=("info",))   # (a torch.stack of the columns)
        np.testing.assert_array_equal(got["info"], c["info"][s])
        assert _bits_equal(got["pose"], np.asarray(c["twin_stage"][s], np.float64))


# ------------------------------------------------------------------------------------------------------------ render
@pytest.mark.parametrize("bg", [False, True])
def test_render_color_on_the_scene(pkg, gpu, bg):
    """test_gpu_render's 70 x 45 scene (two meshes, three instances, a block of the shading pass that spans both images), with and
    without a background, with ``return_face``: img, label, depth, face and area as bytes."""
    from clean_pvnet_amd import render
    from tests.test_gpu_render import KEYS, _scene
    s = _scene()
    inputs = {k: s[k] for k in ("pts", "colors", "faces", "pose", "K", "obj")}
    if bg:
        inputs["bg"] = s["bg"]

    def call(g, m):
        return render.render_color(g["pts"], g["colors"], g["faces"], g["pose"], g["K"], s["size"], ranges=s["ranges"], obj=g["obj"],
                                   bg=g.get("bg"), bg_color=(7, 130, 255), near=s["near"], far=s["far"], ambient=s["ambient"], return_face=True)
    got = guarded_runs(gpu, "render_color 70x45 bg=%s" % bg, inputs, call, workspace=True)
    want = s["want_bg"] if bg else s["want"]
    assert all(_bits_equal(got[k], want[k]) for k in KEYS)


@pytest.mark.parametrize("images", [2, 1])
def test_render_color_on_the_clip_scene(pkg, gpu, images):
    """29 x 23 = 667 pixels: two images end in a group of two pixels, one image in a group of three."""
    from clean_pvnet_amd import render
    from tests.test_gpu_render import KEYS, _clip_scene, _want
    s = _clip_scene()
    s = {**s, "pose": s["pose"][:images]}
    assert (s["size"][0] * s["size"][1] * images) % 4 == (2 if images == 2 else 3)
    want = _want(s)

    def call(g, m):
        return render.render_color(g["pts"], g["colors"], g["faces"], g["pose"], g["K"], s["size"], near=s["near"], far=s["far"],
                                   ambient=s["ambient"], return_face=True)
    got = guarded_runs(gpu, "render_color 29x23 x %d" % images, {k: s[k] for k in ("pts", "colors", "faces", "pose", "K")}, call, workspace=True)
    assert all(_bits_equal(got[k], want[k]) for k in KEYS)


# ------------------------------------------------------------------------------------------------------------ det_eval
def test_box_iou_and_the_detector_evaluator(pkg, gpu):
    """test_gpu_det_eval on ``det_eval_random``: the IoU matrix of that test's boxes, every stage output of one ``evaluate`` ("every
    row, the unused ones included"), and precision, recall and scores after ``summarize`` equal the twin bit for bit.  The sorted
    keys and the permutation come from ``torch.sort`` (det_eval.py:297); the result block is a ``torch.full`` of the call: carved."""
    from clean_pvnet_amd import det_eval
    from tests import det_eval_twin as twin
    rng = np.random.default_rng(3)
    gt = np.array([[0, 0, 2, 1], [10, 10, 40, 40], [10, 10, 40, 40], [3.25, 7.5, 11.13, 9.87], [50, 50, 0, 10]], np.float64)
    crowd = np.array([0, 0, 1, 0, 0], np.int32)
    dt = np.concatenate([np.array([[0, 0, 1, 1], [2, 0, 5, 5], [100, 100, 5, 5], [12, 12, 20, 20], [10, 10, 40, 40], [0, 0, 0, 0]], np.float64),
                         np.round(rng.uniform(0, 45, (59, 4)), 2)])
    got = guarded_runs(gpu, "box_iou", {"dt": dt, "gt": gt, "crowd": crowd}, lambda g, m: det_eval.box_iou(g["dt"], g["gt"], g["crowd"]), workspace=False)
    assert _bits_equal(got, twin.box_iou(dt, gt, crowd))
    s, want = twin.fixture_with_twin("det_eval_random")
    B = len(s["img_ids"])
    inputs = {"det": s["detection"]}
    if s["num"] is not None:
        inputs["num"] = np.asarray(s["num"])

    def call(g, m):
        ev = det_eval.DetEvaluator(s)
        ev.evaluate(g["det"], [s["img_ids"][b] for b in range(B)], s["center"], s["scale"], s["inp_hw"], num=g.get("num"))
        last = ev.last
        ev.summarize()
        return {"mapped": last["mapped"], "keys": last["keys"], "words": last["words"], "npig": ev.npig.astype(np.int32),
                "keys_sorted": ev.order["keys"], **{k: ev.eval[k] for k in ("precision", "recall", "scores")}}
    got = guarded_runs(gpu, "DetEvaluator", inputs, call, workspace=True, derived=("keys_sorted",))
    for k in ("box", "score", "area", "n", "cat"):
        assert _bits_equal(got["mapped"][k], want["mapped"][0][k]), k
    assert _bits_equal(got["keys"], want["keys"][0]) and _bits_equal(got["words"].view(np.uint32), want["words"][0])
    assert _bits_equal(got["npig"], want["npig"]) and _bits_equal(got["keys_sorted"], want["keys_sorted"])
    for k in ("precision", "recall", "scores"):
        assert _bits_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------------------ nn
def test_nn_find_nearest_on_device_pointers(oracle, pkg, gpu):
    """test_nn.test_hip_nearest_neighbour_device_pointers_batched_exclude_self: b = 3, pn = 777, every point's nearest other point."""
    L = capi.load("nn")
    b, pn, dim = 3, 777, 3
    pts = np.random.RandomState(4).randn(b, pn, dim).astype(np.float32)

    def call(g, m):
        idx = torch.empty(b, pn, dtype=torch.int32, device=gpu)
        rc = L.pvv_nn_find_nearest(g["pts"].data_ptr(), g["pts"].data_ptr(), idx.data_ptr(), b, pn, pn, dim, 1, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return idx
    got = guarded_runs(gpu, "pvv_nn_find_nearest", {"pts": pts}, call, workspace=False)
    for bi in range(b):
        np.testing.assert_array_equal(got[bi], oracle.find_nearest_point_idx(pts[bi], pts[bi], exclude_self=True))
