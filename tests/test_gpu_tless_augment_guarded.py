"""``tless_compose`` -> ``tless_pvnet_augment`` and ``rotate_image`` on poisoned, guarded memory (tests/test_gpu_guarded.py has the
driver and states what it asserts): the smallest scenario of tests/test_gpu_tless_augment.py, three fills, the bands intact, the
three results the same bytes and the twin's."""
import numpy as np
import pytest

from tests import tless_augment_twin as twin
from tests.test_gpu_guarded import _bits_equal, guarded_runs

pytestmark = pytest.mark.gpu


def test_tless_compose_augment_and_rotate(pkg, gpu):
    from clean_pvnet_amd import tless_augment as ta
    bg, img, mask, kpt, oi, om, d = twin.batch(1, 53)
    fused_bg, num = twin.fused_backgrounds(bg)[:, ::-1].copy(), np.array([2], np.int64)
    d[0, twin.TOP] = 0.75                                                   # the occluded branch: every kernel's every path runs
    want_c = twin.compose(bg, img, mask, kpt, oi, om, d, fused_bg=fused_bg, num=num)
    want_a = twin.augment(want_c["img"], want_c["mask"], want_c["kpt_2d"], want_c["bbox"], d, input_size=twin.INPUT_SIZE)
    deg = np.array([[30., 200.]])
    want_r = twin.rotate_image(oi, deg)

    def call(g, m):
        c = ta.tless_compose(g["bg"], g["img"], g["mask"], g["kpt"], g["oi"], g["om"], d, fused_bg=g["fused_bg"], num=g["num"])
        a = ta.tless_pvnet_augment(c["img"], c["mask"], c["kpt_2d"], c["bbox"], d, input_size=twin.INPUT_SIZE)
        return {"compose": c, "augment": a, "rotate": ta.rotate_image(g["oi"], deg)}
    got = guarded_runs(gpu, "tless_augment", {"bg": bg, "img": img, "mask": mask, "kpt": kpt, "oi": oi, "om": om, "fused_bg": fused_bg, "num": num},
                       call, workspace=True)
    for k in twin.COMPOSE_KEYS:
        assert _bits_equal(got["compose"][k], want_c[k]), k
    for k in twin.AUGMENT_KEYS:
        assert _bits_equal(got["augment"][k], want_a[k]), k
    for k in ("out", "size", "rot"):
        assert _bits_equal(got["rotate"][k], want_r[k]), k
