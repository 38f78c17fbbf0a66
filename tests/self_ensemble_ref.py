"""The self-ensemble of multi-stream inference restated in numpy (include/bmc_hip.h "multi-stream inference"): the
orientation O_o of a two-channel image and the merge bmc_slot_commit makes of a group's predictions."""
import numpy as np

H_BIT, V_BIT, P_BIT = 1, 2, 4          # the orientation code: horizontal, vertical, polarity


def orient(img, o):
    """O_o(img)[..., c, y, x] = img[..., c ^ p, v ? H-1-y : y, h ? W-1-x : x] for img [..., 2, H, W] -> a contiguous copy."""
    assert img.shape[-3] == 2 and 0 <= o < 8
    out = img
    if o & P_BIT:
        out = out[..., ::-1, :, :]
    if o & V_BIT:
        out = out[..., ::-1, :]
    if o & H_BIT:
        out = out[..., ::-1]
    return np.ascontiguousarray(out)


def merge(preds, codes):
    """preds [K,2,sH,sW] float32, member j in orientation codes[j] -> the merged canonical prediction [2,sH,sW]: a float32 sum
    of the un-oriented members in member order, every addition rounded on its own, then one multiplication by float32(1/K)."""
    K = len(codes)
    assert K in (2, 4, 8) and preds.shape[0] == K and preds.dtype == np.float32
    acc = orient(preds[0], codes[0])
    for j in range(1, K):
        acc = (acc + orient(preds[j], codes[j])).astype(np.float32)
    return (acc * np.float32(1.0 / K)).astype(np.float32)


def esr_mse(merged, gt):
    """The metric kernel's sum for a prediction of the ground truth's size: float32 difference and square, summed in float64."""
    d = (merged.astype(np.float32) - gt.astype(np.float32)).astype(np.float32)
    return float((d * d).astype(np.float32).astype(np.float64).sum() / d.size)
