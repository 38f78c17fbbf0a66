"""PSNR and SSIM of two-channel count images in float64, plain numpy: the oracle of bmc_slot_quality (include/bmc_hip_quality.h
states the definitions; they are scikit-image's peak_signal_noise_ratio and structural_similarity with its defaults, per channel,
as the reference's psnr_loss / ssim_loss call them, loss/restore.py:44-93).  Nothing here imports the code under test.

The SSIM map is a DIRECT 49-term sliding window: the five sums of a window position are accumulated term by term, row-major over
the 7 x 7 window, and the map is evaluated from the sums exactly as the header writes it.  test_quality_cpu.py pins it to
scikit-image's own code path (scipy.ndimage.uniform_filter of the images and their products, cov_norm = 49 / 48, cropped by 3
pixels) and records how far the two float64 formulations lie apart."""
import numpy as np

WIN = 7
K1, K2 = 0.01, 0.03

# The spread between this file's mean SSIM of a channel and the uniform_filter formulation's, as test_quality_cpu.py measures it
# (the largest over the shapes of tests/test_gpu_quality.py with that file's contents, and over 7x7, 8x13, 40x72, 48x80 with
# integer counts up to 191): 2.0e-15, at 7x7 with counts up to 191; the Poisson contents of the GPU tests give 1.4e-15.  The test
# fails if it measures more than FLOOR, or less than a quarter of it.
FLOOR = 2.0e-15
# The bar of the GPU tests on a channel's mean SSIM, absolute, against this oracle: 1000 x FLOOR, at least 1e-13, and it must not
# exceed 1e-10.  The margin covers the kernel's different but fixed association of the same float64 sums (row sums first, then the
# seven rows; tile partials in a tree); a kernel that needs more is defective.
SSIM_BAR = max(1000 * FLOOR, 1e-13)
assert SSIM_BAR <= 1e-10
# sse, relative: the kernel and numpy add the same non-negative float64 terms (the squares, each rounded once, identically) in
# different orders.  Any summation order of n non-negative terms is within (n - 1) u of the exact sum, u = 2^-53, so two orders
# lie at most 2 (n - 1) u apart: 2.3e-10 at the n = 2^20 terms the kernel may meet, a bound that needs every rounding to go the
# same way.  The largest test shape has n = 96 * 120 = 11 520 terms per image and channel: 2 (n - 1) u = 2.6e-12 in that worst
# case; both sides add in trees (numpy pairwise; the kernel 16 terms per lane, then a tree over 1 024 lanes and the parts), whose
# bound is the depth, about log2(n) u + 16 u = 30 u = 3.3e-15 each.  1e-12 is 150 times that and below the any-order worst case.
SSE_BAR = 1e-12


def data_range(g, data_range="gt"):
    """g [2,h,w] -> R [2]: max(g[c]) - min(g) over BOTH channels (restore.py:85), or the constant."""
    g = np.asarray(g, np.float64)
    if isinstance(data_range, str):
        assert data_range == "gt"
        return np.array([g[0].max() - g.min(), g[1].max() - g.min()])
    return np.array([float(data_range)] * 2)


def window_sums(x, y):
    """x, y [h,w] float64 -> the five [h-6, w-6] images of 49-term sums s_x, s_y, s_xx, s_yy, s_xy, each accumulated term by
    term, row-major over the window."""
    h, w = x.shape
    terms = (x, y, x * x, y * y, x * y)
    sums = [np.zeros((h - WIN + 1, w - WIN + 1)) for _ in terms]
    for dy in range(WIN):
        for dx in range(WIN):
            for s, t in zip(sums, terms):
                s += t[dy:dy + h - WIN + 1, dx:dx + w - WIN + 1]
    return sums


def ssim_map(a, g, R):
    """One channel: a, g [h,w] (any float type), R its data range -> S [h-6, w-6] float64."""
    x, y = np.asarray(a, np.float64), np.asarray(g, np.float64)
    n = float(WIN * WIN)
    sx, sy, sxx, syy, sxy = window_sums(x, y)
    C1, C2 = (K1 * R) * (K1 * R), (K2 * R) * (K2 * R)
    ux, uy = sx / n, sy / n
    vx, vy, vxy = (sxx - sx * sx / n) / (n - 1), (syy - sy * sy / n) / (n - 1), (sxy - sx * sy / n) / (n - 1)
    with np.errstate(all="ignore"):
        return ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def raw_record(a, g, rng="gt"):
    """a, g [2,h,w] float32 -> [2 channels, 4] float64 = {sse, gt_max, gt_min, ssim_sum}, the record bmc_slot_quality writes
    (ssim_sum = nan for R_c == 0)."""
    a64, g64 = np.asarray(a, np.float64), np.asarray(g, np.float64)
    R = data_range(g64, rng)
    out = np.zeros((2, 4))
    for c in range(2):
        d = a64[c] - g64[c]
        out[c] = ((d * d).sum(), g64[c].max(), g64.min(), ssim_map(a64[c], g64[c], R[c]).sum() if R[c] != 0 else np.nan)
    return out


def finish(raw, rng, size):
    """Records [..., 2, 4] of h x w images -> (psnr [...], ssim [...]): the host's finishing, IEEE results standing."""
    raw = np.asarray(raw, np.float64)
    h, w = size
    R = raw[..., 1] - raw[..., 2] if isinstance(rng, str) else np.full(raw.shape[:-1], float(rng))
    with np.errstate(all="ignore"):
        psnr = 10.0 * np.log10(R * R / (raw[..., 0] / np.float64(h * w)))
        ssim = raw[..., 3] / np.float64((h - WIN + 1) * (w - WIN + 1))
        return (psnr[..., 0] + psnr[..., 1]) / 2.0, (ssim[..., 0] + ssim[..., 1]) / 2.0


def quality(a, g, rng="gt"):
    """a, g [N,2,h,w] -> (psnr [N], ssim [N]) float64: the mean over the two channels of psnr_c and ssim_c."""
    a, g = np.asarray(a), np.asarray(g)
    return finish(np.stack([raw_record(x, y, rng) for x, y in zip(a, g)]), rng, a.shape[-2:])


def ssim_map_uniform_filter(a, g, R):
    """scikit-image's structural_similarity code path for one channel (win_size 7, gaussian_weights False, use_sample_covariance
    True): uniform_filter means of the images and their products, cov_norm = NP / (NP - 1), the map cropped by (win - 1) // 2."""
    from scipy.ndimage import uniform_filter
    x, y = np.asarray(a, np.float64), np.asarray(g, np.float64)
    NP = WIN * WIN
    cov_norm = NP / (NP - 1)
    ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
    uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    with np.errstate(all="ignore"):
        S = (A1 * A2) / (B1 * B2)
    pad = (WIN - 1) // 2
    return S[pad:-pad, pad:-pad]


def make_images(h, w, seed, lam=3.0, noise=0.6):
    """N = 3 image pairs [3,2,h,w] float32 with different content: Poisson counts g and a = g + float noise; image 1 has a == g
    bit for bit; image 2 has channel 1 of g empty (a keeps its noise there)."""
    rng = np.random.default_rng(seed)
    g = rng.poisson(lam, (3, 2, h, w)).astype(np.float32)
    g[2, 1] = 0.0
    a = (g + noise * rng.standard_normal(g.shape)).astype(np.float32)
    a[1] = g[1]
    return a, g


def shapes(TH, TW):
    """The (h, w) of the kernel tests for tiles of TH x TW window positions: one position; one more column / row; exactly one
    full tile; four tiles, three of them one position thick; ragged and multi-tile; and one with 2 * h * w above 1024 * 16,
    where the stats launch runs more than one part."""
    return [(7, 7), (7, 8), (8, 7), (TH + 6, TW + 6), (TH + 7, TW + 7), (2 * TH + 6 + 3, 3 * TW + 6 + 5), (96, 120)]
