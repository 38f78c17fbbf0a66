"""What the voxel encoders would return if a compiler fused one of their multiply-adds: events_to_voxel
(dataloader/encodings.py:272-287) and events_to_voxel_torch (:100-148) restated event by event in float32, with ONE of the two
places where a product feeds a sum rounded once instead of twice (float64 intermediates: a product of two float32 numbers is
exact there).

    site "t":   |t * (bins - 1) - b|   the reference rounds the product t * (bins - 1) (:280, :129) before it subtracts b;
    site "acc": acc + p * w            the reference rounds the weight p * w (:284, :134) before index_put_ adds it.

NEVER an expected value.  tests/test_voxel_bins_cpu.py uses it to prove that the inputs of tests/golden/voxel_bins.npz tell the
two arithmetics apart, so that the GPU comparison against those fixtures cannot pass on a kernel that fuses either site.
fuse=None is the reference's own arithmetic (checked against the fixtures there, so the restatement itself is right)."""
import numpy as np

f32, f64 = np.float32, np.float64


def _grid(xs, ys, tn, ps, bins, H, W, fuse, flip):
    """tn: float32 times already on the bin axis, before the product with (bins - 1) -> [bins,H,W] float32."""
    assert fuse in (None, "t", "acc")
    xs, ys, tn, ps = (np.asarray(a, f32) for a in (xs, ys, tn, ps))
    bad = (xs >= W) | (xs < 0) | (ys >= H) | (ys < 0)
    xi = np.where(bad, 0, xs.astype(np.int64))
    yi = np.where(bad, 0, ys.astype(np.int64))
    if flip:
        yi = H - yi - 1
    out = np.zeros((bins, H, W), f32)
    scaled = (tn * f32(bins - 1)).astype(f32)                               # rounded product (the reference)
    for b in range(bins):
        if fuse == "t":
            d = (tn.astype(f64) * f64(bins - 1) - f64(b)).astype(f32)         # fma(t, bins - 1, -b): one rounding
        else:
            d = (scaled - f32(b)).astype(f32)
        w = np.maximum(f32(0), (f32(1.0) - np.abs(d)).astype(f32))
        img = out[b]
        for e in range(len(xs)):
            if bad[e] and b == 0:                                           # the first bin's call masks out-of-range events
                continue
            if fuse == "acc":
                img[yi[e], xi[e]] = f32(f64(img[yi[e], xi[e]]) + f64(ps[e]) * f64(w[e]))    # fma(p, w, acc)
            else:
                img[yi[e], xi[e]] = img[yi[e], xi[e]] + f32(ps[e] * w[e])
    return out


def voxel(xs, ys, ts, ps, bins, H, W, fuse=None):
    """events_to_voxel: vertical flip, out-of-range events land on [H-1, 0] from the second bin on."""
    return _grid(xs, ys, ts, ps, bins, H, W, fuse, True)


def voxel_torch(xs, ys, ts, ps, bins, H, W, fuse=None):
    """events_to_voxel_torch (temporal_bilinear=True): no flip, t_norm = (ts - ts[0]) / (ts[-1] - ts[0] + 1e-6) * (B - 1)."""
    ts = np.asarray(ts, f32)
    if len(ts) <= 3 or float(ts.sum()) == 0:
        return np.zeros((bins, H, W), f32)
    dt = f32(f32(ts[-1] - ts[0]) + f32(1e-6))
    q = ((ts - ts[0]).astype(f32) / dt).astype(f32)
    return _grid(xs, ys, q, ps, bins, H, W, fuse, False)
