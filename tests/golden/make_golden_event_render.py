#!/usr/bin/env python
"""event_render.npz: inputs and outputs of the REFERENCE's event-count renderer, event_visualisation.plot_event_cnt
(myutils/vis_events/matplotlib_plot_events.py:125-248) with the defaults infer_BMCNet.py:90-97 calls it with, imported from the
reference checkout named by the environment variable BMC_REFERENCE (build container only; only the data is committed).

cv2 is absent there.  The function uses it for one thing, cv2.cvtColor(img, cv2.COLOR_BGR2RGB) on a uint8 [H,W,3] image, which
reverses the last axis and nothing else: the stub module of ref_stubs gets a COLOR_BGR2RGB constant and a cvtColor that does
exactly that.  What is recorded is the array the function RETURNS, not the figure matplotlib draws from it.

Per case k: cnt_k (float32 [2,h,w]; the function is given cnt_k.transpose(1, 2, 0), after np.round for the cases flagged in
round_k) and img_k (the returned uint8 [h,w,3]); name_k says what the case is for.  Every case has at most 64 x 64 pixels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("BMC_REFERENCE")
if not REF:
    sys.exit("set BMC_REFERENCE to the reference checkout")
sys.path.insert(0, REF)
import ref_stubs  # noqa: E402

ref_stubs.install()
cv2 = sys.modules["cv2"]
cv2.COLOR_BGR2RGB = 4


def _cvt(img, code):
    assert code == cv2.COLOR_BGR2RGB and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    return np.ascontiguousarray(img[:, :, ::-1])


cv2.cvtColor = _cvt
import matplotlib.pyplot as plt  # noqa: E402
from myutils.vis_events.matplotlib_plot_events import event_visualisation  # noqa: E402

from event_render_ref import render_np  # noqa: E402


def cases(rng):
    def poisson(h, w, lam=0.6):
        return rng.poisson(lam, (2, h, w)).astype(np.float32)

    for h, w in ((7, 9), (24, 40), (31, 57)):              # 31 x 57: ragged, N - 1 = 1766 is no multiple of 100
        yield "poisson_%dx%d" % (h, w), poisson(h, w), False
    yield "n101_integral_indices", poisson(1, 101, 2.0), False
    yield "n1", np.array([[[3.0]], [[1.0]]], np.float32), False
    yield "n1_zero", np.zeros((2, 1, 1), np.float32), False
    yield "n15", poisson(3, 5, 1.5), False
    yield "gaussian_dense", rng.normal(0.0, 2.0, (2, 33, 47)).astype(np.float32), False
    yield "gaussian_shifted", (rng.normal(0.0, 1.0, (2, 64, 64)) * np.array([3.0, 0.5])[:, None, None]
                               + np.array([-1.0, 2.0])[:, None, None]).astype(np.float32), False
    yield "constant", np.full((2, 6, 11), 3.0, np.float32), False              # min == max: the unnormalised quirk
    yield "constant_half", np.full((2, 6, 11), 0.25, np.float32), False
    yield "constant_unequal", np.stack([np.full((5, 8), 2.0), np.full((5, 8), 0.5)]).astype(np.float32), False
    a = poisson(20, 30, 1.2)
    a[0] = 0
    yield "positive_all_zero", a, False
    a = poisson(20, 30, 1.2)
    a[1] = 0
    yield "negative_all_zero", a, False
    yield "all_zero", np.zeros((2, 9, 13), np.float32), False
    yield "halves_rounded", (rng.integers(0, 9, (2, 17, 23)) * 0.5).astype(np.float32), True
    yield "prediction_like_rounded", np.abs(rng.normal(0.0, 1.3, (2, 48, 64))).astype(np.float32), True
    a = poisson(32, 48, 0.4)
    a[0, 3, 5], a[1, 10, 7], a[0, 31, 47], a[1, 0, 0] = 900.0, 250.0, 60.0, 1e6
    yield "large_counts_clip", a, False
    a = poisson(16, 16, 0.05)                               # so sparse that both percentiles of a channel are 0
    yield "sparse", a, False
    a = poisson(12, 18, 3.0)
    a[0, ::2] = -0.0
    yield "negative_zero", a, False


def main():
    rng = np.random.default_rng(20261018)
    vis = event_visualisation()
    out, k, bad = {}, 0, 0
    for name, cnt, rnd in cases(rng):
        assert cnt.dtype == np.float32 and cnt[0].size <= 64 * 64
        x = np.round(cnt) if rnd else cnt
        img = vis.plot_event_cnt(np.array(x.transpose(1, 2, 0), copy=True), is_save=False)
        plt.close("all")
        assert img.dtype == np.uint8 and img.shape == cnt.shape[1:] + (3,)
        out["name_%d" % k], out["cnt_%d" % k], out["round_%d" % k], out["img_%d" % k] = np.array(name), cnt, np.array(rnd), img
        same = np.array_equal(render_np(cnt, round=rnd), img)
        bad += not same
        print("%-28s %s %s" % (name, cnt.shape[1:], "ok" if same else "RESTATEMENT DIFFERS"))
        k += 1
    out["n"] = np.array(k)
    path = os.path.join(HERE, "event_render.npz")
    np.savez_compressed(path, **out)
    print("%d cases written, %d bytes; the restatement differs on %d" % (k, os.path.getsize(path), bad))
    assert bad == 0


if __name__ == "__main__":
    main()
