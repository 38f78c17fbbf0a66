"""Fused BIE block (bilateral information exchange, reference models/submodules.py:38-77) in its "twin" form:
`first` and `second` are the two batch halves of ONE tensor x12, so every weight-shared pair of the reference
(conv1 == conv2, convf1 == convf2) is one launch over the doubled batch.

Forward and backward are written out launch by launch (no autograd inside): every gradient that has several
contributions (x12: residual block + convf + value conv; xs: convf twice + skip; center: Gram + unclustering; v: Gram
+ attention) is accumulated by convolution epilogues (residual / accumulate) instead of separate add kernels, the
ReLU backward of the residual block is a mask epilogue, and the crossed skip connections (out_1 + Res(x_2),
out_2 + Res(x_1)) are batch-rotated operand reads -- no roll / cat copies.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import torch

from . import lib, ops
from .ops import ConvSpec, _dense_spec, _need_gpu, _null_src, _src, _stream, conv_launch, dgrad_launch, pgemm_raw, round_up

_SPEC2 = {}

# Fused centre chain (csrc/chain.hip): convf -> LayerNorm2d -> clustering in one launch per direction.  fp32 MFMA only
# (the bf16-plane modes keep the unfused launches); BMC_FUSE_CHAIN=0 switches it off (A/B measurements, cross-checks).
FUSE_CHAIN = os.environ.get("BMC_FUSE_CHAIN", "1") != "0"
_CHAIN_CACHE = {}



# Attention without the value tensor (fp32 arithmetic modes).  v = W_v x + b_v enters the BIE twice -- the Gram matrix
# att = scale * c^T v and the product out = softmax(att) v -- and both are linear in v, so with G0 = c^T x (the same
# pixel-reduction GEMM, on x instead of v) and s = the column sums of c (its bias slabs):
#     att = scale * (G0 W_v^T + s b_v^T),        out = (P W_v) x + P b_v           (P = softmax(att), per sample)
# i.e. v is never formed: the forward loses the value convolution, the backward loses its data-gradient convolution and its
# weight-gradient GEMM (dW_v = P^T dM + da^T G0 from C x C matrices, dM = g_out^T x taking the place of g_out^T v), three of
# the BIE's thirteen full-size 1x1 launches -- against a handful of C x C x C products per sample.  Same mathematics, another
# order of summation (the parity bars of tests/parity_bars.py hold it); BMC_BIE_VFREE=0 restores the explicit form, which the
# bf16 mode keeps (its operand-rounding oracle rounds v).
# Not for small launches: the three full-size launches it removes cost 12-15 us each at 31x56, the eight small ones it adds
# 5-6 us each plus their weight packs (31x56: 82.3 -> 96.6 ms, 48x64: 111.5 -> 124.9 ms; break-even at 64x96, 154.2 vs 155.0 ms;
# 90x120: 232.4 -> 228.3 ms; 180x240: 743 -> 710 ms) -- from 2^16 pixels per launch.
VFREE = os.environ.get("BMC_BIE_VFREE", "1") != "0"
VFREE_MIN_PIXELS = int(os.environ.get("BMC_BIE_VFREE_MIN_PIXELS", 1 << 16))


def vfree_supported(npx):
    return VFREE and ops.MATH in (0, 3) and npx >= VFREE_MIN_PIXELS


def _gram_on_x(c_src, x_src, B, H, W, Cn, dev):
    """-> (G0 [B,C,C], s [B,C]): G0_b = sum_px c_b[px,:]^T x_b[px,:], s_b = sum_px c_b[px,:] (one pixel-reduction launch per
    sample group + its reduction; c_src / x_src: lib.Src over B launch batches)."""
    slabs, nsplit, G, bsl = pgemm_raw(c_src, [x_src], B, H, W, 1, 1, Cn, Cn, dev, flops=2.0 * B * H * W * Cn * Cn, want_bias=True)
    G0 = torch.empty((B, Cn, Cn), device=dev, dtype=torch.float32)
    sc = torch.empty((B, Cn), device=dev, dtype=torch.float32)
    lib.call(lib._red_w, "bmc_pgemm_reduce_weight", slabs.data_ptr(), nsplit, G, 1, Cn, Cn, None, Cn, G0.data_ptr(), 0,
             bsl.data_ptr(), sc.data_ptr(), _stream())
    return G0, sc


def _times_wt(m, vec, wg, bg, bpg, alpha, out):
    """out[b] = alpha (m[b] W_g^T + vec[b] b_g^T)  (m [B,C,C], vec [B,C]; wg [G,C(j),C(k)], bg [G,C]; g = b // bpg): the Gram
    matrix of the attention from G0 = center^T x, and dP from dM = g_out^T x."""
    B, Cn, _ = m.shape
    ops.small_mm([((m, Cn * Cn, 0, Cn, 1), (wg, 0, Cn * Cn, 1, Cn), None)], B, bpg, Cn, Cn, Cn, c=(out, Cn * Cn, 0, Cn, 1),
                 alpha=alpha, uv=((vec, Cn, 0), (bg, 0, Cn)))
    return out


def _times_w(m, wg, bg, bpg, out, out_strides, vec=None):
    """out[b][i][k] = sum_j m[b][i][j] W_g[j][k] (written with out_strides = (batch, i, k) strides: plain, into a column block
    of a wider matrix, or transposed), vec[b][i] = sum_j m[b][i][j] b_g[j]."""
    B, Cn, _ = m.shape
    ops.small_mm([((m, Cn * Cn, 0, Cn, 1), (wg, 0, Cn * Cn, Cn, 1), (bg, 0, Cn, 1) if vec is not None else None)], B, bpg, Cn, Cn, Cn,
                 c=(out, out_strides[0], 0, out_strides[1], out_strides[2]), vec_out=(vec, Cn, 0) if vec is not None else None)


def _value_param_grads(p, dM, tg, da, G0, sc, w_params, b_params, npx):
    """dW_v[g] = sum over the group's samples of P^T dM + da^T G0, db_v[g] = sum of P^T t + da^T s.  The per-sample products are
    written in the slab layout of the pixel-reduction GEMM (sample = split), so the sum over a group's samples, the routing
    into the parameters' .grad (or back to autograd) and the weight-gradient stream are ops.reduce_wgrad's, as for every other
    weight gradient.  -> (dw [G,C,C], db [G,C]) or (None, None)."""
    groups = len(w_params)
    B, Cn, _ = p.shape
    n, cc, dev = B // groups, Cn * Cn, p.device
    mp = round_up(Cn, 32)
    slab, bslab = groups * mp * mp, groups * 4 * mp
    slabs = torch.empty(n * slab, device=dev, dtype=torch.float32)       # [n][G][1][mp][mp]; the reduction reads rows / columns < C only
    bsl = torch.zeros(n * bslab, device=dev, dtype=torch.float32)        # [n][G][4][mp]: part 0 written, parts 1-3 zero
    params = list(w_params) + list(b_params)
    with ops.wgrad_side(npx, params, (p, dM, tg, da, G0, sc)):
        ops._on_side(slabs, bsl)
        # batch b = g * n + s  ->  slab s, group g
        ops.small_mm([((p, cc, 0, 1, Cn), (dM, cc, 0, Cn, 1), (tg, Cn, 0, 1)), ((da, cc, 0, 1, Cn), (G0, cc, 0, Cn, 1), (sc, Cn, 0, 1))],
                     B, n, Cn, Cn, Cn, c=(slabs, slab, mp * mp - n * slab, mp, 1), vec_out=(bsl, bslab, 4 * mp - n * bslab))
        one = groups == 1
        return ops.reduce_wgrad(slabs, n, groups, 1, Cn, _dense_spec(Cn), dev, bsl, w_params[0] if one else tuple(w_params),
                                b_params[0] if one else tuple(b_params), (Cn, Cn) if one else (groups, Cn, Cn))


def chain_supported(Cn):
    # (bf16x6 is an fp32-equivalent mode: the native fp32 fused chain is a valid member of it)
    return FUSE_CHAIN and ops.MATH in (0, 3) and Cn in (32, 64, 128)


def _chain_streams(wf, wc, Cn):
    """Weight streams of bmc_chain_fwd / bmc_chain_bwd for (convf.weight, clustering.weight), cached per parameter
    version: the forward stream is pack(W_f) | pack(W_c); the backward stream is T(W_c) T(W_c) T1(W_f) T1(W_f) T0(W_f)
    (include/bmc_hip.h)."""
    key = (id(wf), id(wc))
    hit = _CHAIN_CACHE.get(key)
    if hit is not None and hit[0]() is wf and hit[1]() is wc and hit[2] == (wf._version, wc._version):
        return hit[3], hit[4]
    dev = wf.device
    s1, s2 = _dense_spec(Cn), _spec2(Cn)
    st = _stream()

    def pack(w, spec, cin):
        out = torch.empty(spec.kpad * Cn, device=dev, dtype=torch.float32)
        lib.call(lib._pack_w, "bmc_pack_weight", w.data_ptr(), spec.kmap(dev).data_ptr(), 1, Cn, cin, 1, spec.kpad, Cn,
                 out.data_ptr(), st)
        return out

    def pack_t(w, spec, cin, src_index):
        out = torch.empty(Cn * Cn, device=dev, dtype=torch.float32)
        lib.call(lib._pack_wt, "bmc_pack_weight_t", w.data_ptr(), spec.kmap(dev).data_ptr(), 1, Cn, cin, 1,
                 src_index * Cn, Cn, Cn, Cn, out.data_ptr(), st)
        return out

    wfd, wcd = wf.detach().contiguous(), wc.detach().contiguous()
    fwd = torch.cat([pack(wfd, s2, 2 * Cn), pack(wcd, s1, Cn)])
    tc, t0, t1 = pack_t(wcd, s1, Cn, 0), pack_t(wfd, s2, 2 * Cn, 0), pack_t(wfd, s2, 2 * Cn, 1)
    bwd = torch.cat([tc, tc, t1, t1, t0])
    if len(_CHAIN_CACHE) > 64:
        for k in [k for k, v in _CHAIN_CACHE.items() if v[0]() is None or v[1]() is None]:
            del _CHAIN_CACHE[k]
    _CHAIN_CACHE[key] = (weakref.ref(wf), weakref.ref(wc), (wf._version, wc._version), fwd, bwd)
    return fwd, bwd


def chain_fwd(s0, s1, wf, bf, gamma, beta, wc, bc, eps, B, H, W, Cn, dev):
    """-> (yhat [B,H,W,C], rstd [B*H*W], centre [B,H,W,C]); s0 / s1: lib.Src of C channels each."""
    fwd, _ = _chain_streams(wf, wc, Cn)
    yhat = torch.empty((B, H, W, Cn), device=dev, dtype=torch.float32)
    centre = torch.empty((B, H, W, Cn), device=dev, dtype=torch.float32)
    rstd = torch.empty(B * H * W, device=dev, dtype=torch.float32)
    a = lib.ChainFwdArgs()
    a.s0, a.s1 = s0, s1
    a.wstream = fwd.data_ptr()
    a.bias_f, a.bias_c, a.gamma, a.beta = bf.data_ptr(), bc.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    a.eps = eps
    a.yhat, a.rstd, a.centre = yhat.data_ptr(), rstd.data_ptr(), centre.data_ptr()
    a.B, a.C, a.H, a.W = B, Cn, H, W
    e0 = ops._prof_begin()
    lib.call(lib._chain_fwd, "bmc_chain_fwd", C.byref(a), _stream())
    ops._prof_end(e0, "chain_kernel<fwd>", 2.0 * B * H * W * Cn * 3 * Cn, B * H * W * (16.0 * Cn + 4))
    return yhat, rstd, centre


def chain_bwd(dc, yhat, rstd, gamma, wf, wc, add, n, H, W, Cn, dev, ds1=None):
    """-> (dz [2n,H,W,C], ds1 [2n,H,W,C], ds0 [n,H,W,C]); dc: lib.Src over 2n launch batches, add: lib.Src or None;
    ds1: optional preallocated destination."""
    _, bwd = _chain_streams(wf, wc, Cn)
    dz = torch.empty((2 * n, H, W, Cn), device=dev, dtype=torch.float32)
    if ds1 is None:
        ds1 = torch.empty((2 * n, H, W, Cn), device=dev, dtype=torch.float32)
    ds0 = torch.empty((n, H, W, Cn), device=dev, dtype=torch.float32)
    a = lib.ChainBwdArgs()
    a.dcentre = dc
    a.wstream = bwd.data_ptr()
    a.gamma, a.yhat, a.rstd = gamma.data_ptr(), yhat.data_ptr(), rstd.data_ptr()
    a.dz, a.ds1, a.ds0 = dz.data_ptr(), ds1.data_ptr(), ds0.data_ptr()
    a.ds0_add = add if add is not None else _null_src()
    a.n, a.C, a.H, a.W = n, Cn, H, W
    e0 = ops._prof_begin()
    lib.call(lib._chain_bwd, "bmc_chain_bwd", C.byref(a), _stream())
    ops._prof_end(e0, "chain_kernel<bwd>", 2.0 * 2 * n * H * W * Cn * 3 * Cn, 2 * n * H * W * (20.0 * Cn + 4))
    return dz, ds1, ds0


def _spec2(c):
    s = _SPEC2.get(c)
    if s is None:
        s = ConvSpec.dense(c, c)
        _SPEC2[c] = s
    return s


# --------------------------------------------------------------------------
# The launch steps of the block, each written once.  BIETwinFn and BIEFirstFn (below) are compositions of them and differ in
# DATA only: the batch window a step covers (the first nb of the 2n images) and the number of value-weight groups.  No step is
# told which node calls it.
# --------------------------------------------------------------------------
def _X(t, shift=0, mod=None, b0=0, B=None):
    """Operand descriptor over all channels of t [*,H,W,C]: B launch images (default: all of t) from image b0 on, read
    batch-rotated by `shift` modulo `mod`."""
    return _src(t, 0, t.shape[3], shift, mod, b0, t.shape[0] if B is None else B)


def _new(b, like):
    return torch.empty((b,) + like.shape[1:], device=like.device, dtype=torch.float32)


def _value_weights(p_w, ws, p_b=None, bs=None):
    """The G = len(ws) weight groups of the value convolutions -> (w4 [G,C,C,1], its pack-cache owner, bias [G,C]; None
    without bs).  One group: the parameter itself, reshaped.  Several: stacked once per parameter version (ops.stacked, keyed by
    p_w / p_b, the caller's parameter objects -- saved tensors are fresh aliases in every backward); the stack owns its pack."""
    Cn = ws[0].shape[0]
    if len(ws) == 1:
        return ws[0].detach().reshape(1, Cn, Cn, 1), p_w[0], bs[0].detach().reshape(1, Cn) if bs is not None else None
    w4 = ops.stacked(p_w, lambda: torch.stack([w.detach().reshape(Cn, Cn, 1) for w in ws]), "v1x1")
    return w4, w4, ops.stacked(p_b, lambda: torch.stack([b.detach() for b in bs]), "stack") if bs is not None else None


def _centres_fwd(x12, xs, wf, bf, gamma, beta, wc, bc, eps):
    """[c1; c2] = clustering(LN(convf(cat[xs, other half]))) in the one fused launch -> (yhat, rstd, c12)."""
    B2, H, W, Cn = x12.shape
    n = B2 // 2
    return chain_fwd(_X(xs, mod=n, B=B2), _X(x12, shift=n, mod=B2), wf, bf.detach(), gamma.detach(), beta.detach(), wc, bc.detach(),
                     eps, B2, H, W, Cn, x12.device)


def _attention_fwd(c_src, x_src, res_src, w4, owner, bias, scale, nb, like, vfree):
    """o[b] = softmax(scale c_b^T v_b) v_b + residual[b] over nb launch images; v = W_g x + b_g, the value convolution with
    the weights of group g = b // (nb / G) (_value_weights).  vfree: the form that never builds v (top of this file).
    -> (o, P, v, G0, s): v is None in the vfree form, G0 and s in the explicit one."""
    _, H, W, Cn = like.shape
    dev, s1 = like.device, _dense_spec(Cn)
    G = w4.shape[0]
    o = _new(nb, like)
    if vfree:       # att = scale (G0 W_v^T + s b_v^T), out = (P W_v) x + P b_v
        G0, sc = _gram_on_x(c_src, x_src, nb, H, W, Cn, dev)
        wg, v = w4.view(G, Cn, Cn), None
        att = _times_wt(G0, sc, wg, bias, nb // G, scale, torch.empty_like(G0))
        p = torch.empty_like(att)
        lib.call(lib._sm_fwd, "bmc_softmax_fwd", att.data_ptr(), nb * Cn, Cn, p.data_ptr(), _stream())
        pw, pb = torch.empty_like(p), torch.empty_like(sc)                                 # P W_v [b, i, k],  P b_v [b, i]
        _times_w(p, wg, bias, nb // G, pw, (Cn * Cn, Cn, 1), vec=pb)
        conv_launch([x_src], pw.view(nb, Cn, Cn, 1), s1, None, pb, o, nb, residual=res_src, bpg=1)
    else:
        G0 = sc = None
        v = _new(nb, like)
        conv_launch([x_src], w4, s1, owner, bias, v, nb, bpg=nb // G)
        # channel attention per sample
        slabs, nsplit, Gs = pgemm_raw(c_src, [_X(v)], nb, H, W, 1, 1, Cn, Cn, dev, flops=2.0 * nb * H * W * Cn * Cn)
        att = torch.empty((nb, Cn, Cn), device=dev, dtype=torch.float32)
        lib.call(lib._red_p, "bmc_pgemm_reduce_plain", slabs.data_ptr(), nsplit, Gs, Cn, Cn, scale, att.data_ptr(), _stream())
        p = torch.empty_like(att)
        lib.call(lib._sm_fwd, "bmc_softmax_fwd", att.data_ptr(), nb * Cn, Cn, p.data_ptr(), _stream())
        conv_launch([_X(v)], p.view(nb, Cn, Cn, 1), s1, None, None, o, nb, residual=res_src, bpg=1)
    return o, p, v, G0, sc


def _uncluster_fwd(c12, wu, bu, xs):
    """shared stream: xs_new = unclustering(cat[c1, c2]) + xs."""
    n, _, _, Cn = xs.shape
    xs_new = _new(n, xs)
    conv_launch([_X(c12, b0=0, B=n), _X(c12, b0=n, B=n)], wu.detach().reshape(1, Cn, 2 * Cn, 1), _spec2(Cn), wu, bu.detach(), xs_new, n,
                residual=_X(xs))
    return xs_new


def _attention_bwd(g_o, g_x, x12, c12, v, p, G0, sc, w4, bias, scale, w_params, b_params, p_wu, p_bu, wu, window):
    """Backward of _attention_fwd over its nb = len(p) images (the first nb of x12 / c12) and of _uncluster_fwd, up to the
    centres: dP, the softmax, dc12 [2n] = the attention's Gram term on the first nb images + the unclustering's data gradient on
    all of them, and the parameter gradients of the unclustering and of the value convolutions (v is None: the vfree form).
    -> (dc12, dv, w_dx, dwv, dbv, dwu, dbu); what is left for _attention_dx is dv (explicit form) or the matrices w_dx (vfree)."""
    nb, Cn, _ = p.shape
    B2, H, W, _ = x12.shape
    n = B2 // 2
    dev, s2 = x12.device, _spec2(Cn)
    G = w4.shape[0]
    g_src = _X(g_o)
    # ---- out = P v (+ residual): dP
    if v is None:       # dM = g_o^T x, t = column sums of g_o;  dP = dM W_v^T + t b_v^T
        wg = w4.view(G, Cn, Cn)
        dM, tg = _gram_on_x(g_src, _X(x12, B=nb), nb, H, W, Cn, dev)
        dp = _times_wt(dM, tg, wg, bias, nb // G, 1.0, torch.empty_like(dM))
    else:
        slabs, nsplit, Gs = pgemm_raw(g_src, [_X(v)], nb, H, W, 1, 1, Cn, Cn, dev, flops=2.0 * nb * H * W * Cn * Cn)
        dp = torch.empty_like(p)
        lib.call(lib._red_p, "bmc_pgemm_reduce_plain", slabs.data_ptr(), nsplit, Gs, Cn, Cn, 1.0, dp.data_ptr(), _stream())
    # ---- softmax, Gram (att = scale * center v^T)
    da = torch.empty_like(p)
    lib.call(lib._sm_bwd, "bmc_softmax_bwd", p.data_ptr(), dp.data_ptr(), nb * Cn, Cn, scale, da.data_ptr(), _stream())
    dwv = dbv = dv = w_dx = None
    if v is None:
        # value-convolution parameters: dW_v = P^T dM + da^T G0, db_v = P^T t + da^T s (summed over the group's samples)
        dwv, dbv = _value_param_grads(p, dM, tg, da, G0, sc, w_params, b_params, nb * H * W)
    # Each of dv and d center has two contributions that are 1x1 products with per-sample / per-half matrices: ONE
    # two-source launch each (K = 2C, the matrices side by side) instead of a launch + accumulating launches --
    #   dv[b]      = P_b^T g_o[b] + da_b^T center[b]                                             (b < nb)
    #   dcenter[b] = (b < nb: da_b v[b]) + W_u[:, half(b)]^T g_x[b mod n]     (unclustering reads cat[c1, c2]; images from nb on
    #                                                                          have no attention term: a zero matrix)
    dc12 = _new(B2, x12)
    # [B2, C (c_i), C (co)], cached per version of the unclustering weight and batch size (it is the same in all 8 windows)
    w_ut = ops.stacked((p_wu,), lambda: wu.detach().view(Cn, 2, Cn).permute(1, 2, 0).repeat_interleave(n, 0).contiguous(), "wut%d" % n)
    gx2 = _X(g_x, mod=n, B=B2)
    if v is None:
        # without v:  dx12 (+)= (P W_v)^T g_o + (da W_v)^T center  (_attention_dx, once dx12 exists);
        #             dcenter = (da W_v) x + da b_v + W_u[:, half]^T g_x
        # the per-sample matrices are written straight into the two-source weight layouts [b][cout][cin of source 0 | 1]
        alloc = torch.zeros if nb < B2 else torch.empty         # (rows of the images from nb on are never written: they stay zero)
        w_dx = torch.empty((nb, Cn, 2 * Cn, 1), device=dev, dtype=torch.float32)
        w_dc = alloc((B2, Cn, 2 * Cn, 1), device=dev, dtype=torch.float32)
        w_dc.view(B2, Cn, 2 * Cn)[:, :, Cn:] = w_ut
        ds = alloc((B2, Cn), device=dev, dtype=torch.float32)
        cc2 = 2 * Cn * Cn
        _times_w(da, wg, bias, nb // G, w_dc, (cc2, 2 * Cn, 1), vec=ds)                        # [da W_v | .],  da b_v
        _times_w(da, wg, bias, nb // G, w_dx[:, :, Cn:], (cc2, 1, 2 * Cn))                     # [. | (da W_v)^T]
        _times_w(p, wg, bias, nb // G, w_dx, (cc2, 1, 2 * Cn))                                 # [(P W_v)^T | .]
        conv_launch([_X(x12), gx2], w_dc, s2, None, ds, dc12, B2, bpg=1)
    else:
        dv = _new(nb, x12)
        w_dv = torch.cat([p.transpose(1, 2), da.transpose(1, 2)], 2).view(nb, Cn, 2 * Cn, 1)
        conv_launch([g_src, _X(c12, B=nb)], w_dv, s2, None, None, dv, nb, bpg=1)
        da2 = da if nb == B2 else torch.cat([da, da.new_zeros((B2 - nb, Cn, Cn))], 0)
        w_dc = torch.cat([da2, w_ut], 2).view(B2, Cn, 2 * Cn, 1)
        conv_launch([_X(v, mod=nb, B=B2), gx2], w_dc, s2, None, None, dc12, B2, bpg=1)
    # ---- unclustering(cat[c1, c2]) + xs: weight gradient
    dwu, dbu = ops.wgrad(_X(g_x), [_X(c12, b0=0, B=n), _X(c12, b0=n, B=n)], s2, n, H, W, 1, Cn, dev, p_wu, p_bu, keep=(g_x, c12),
                         window=window, merge_pgemm=True)
    if v is not None:   # ---- value convs: one weight group per parameter
        one = G == 1
        dwv, dbv = ops.wgrad(_X(dv), [_X(x12, B=nb)], _dense_spec(Cn), nb, H, W, 1, Cn, dev, w_params[0] if one else w_params,
                             b_params[0] if one else b_params, G=G, w_shape=None if one else (G, Cn, Cn, 1, 1), keep=(dv, x12),
                             window=window, merge_pgemm=True)
    return dc12, dv, w_dx, dwv, dbv, dwu, dbu


def _chain_bwd_tail(dc12, yhat, rstd, gamma, beta, wf, wc, g_x, xs, x12, params, window, ds1=None):
    """clustering, LayerNorm, convf: ONE data-gradient launch (csrc/chain.hip) and the parameter gradients that follow from it.
    dx12 = conv_f^T (second half of its inputs; written into ds1 where given), dxs = skip + conv_f^T (first half) summed over
    both halves.  params: the caller's (convf w, b, norm w, b, clustering w, b).
    -> (dx12, dxs, dwf, dbf, dgamma, dbeta, dwc, dbc)"""
    p_wf, p_bf, p_gamma, p_beta, p_wc, p_bc = params
    B2, H, W, Cn = x12.shape
    n = B2 // 2
    dev = x12.device
    dz12, dx12, dxs = chain_bwd(_X(dc12), yhat, rstd, gamma.detach(), wf, wc, _X(g_x), n, H, W, Cn, dev, ds1=ds1)
    # G = dc^T yhat and the clustering bias gradient (temporaries: dW_c, dgamma, dbeta follow from them)
    Gm, dbc_t = ops.wgrad(_X(dc12), [_X(yhat)], _dense_spec(Cn), B2, H, W, 1, Cn, dev, None, None, w_shape=(Cn, Cn), merge_pgemm=True)
    sg = ops.sink_group([p_wc, p_bc, p_gamma, p_beta])
    if sg is not None:
        (o_w, o_b, o_g, o_bt), acc = sg
        dwc = dbc = dgamma = dbeta = None
    else:
        o_w, o_b, acc = Gm, None, 0
        o_g = dgamma = torch.empty(Cn, device=dev, dtype=torch.float32)
        o_bt = dbeta = torch.empty(Cn, device=dev, dtype=torch.float32)
        dwc, dbc = Gm.view(wc.shape), dbc_t
    lib.call(lib._chain_affine, "bmc_chain_affine_grads", Gm.data_ptr(), dbc_t.data_ptr(), wc.detach().data_ptr(),
             gamma.detach().data_ptr(), beta.detach().data_ptr(), Cn, o_w.data_ptr(),
             o_b.data_ptr() if o_b is not None else None, o_g.data_ptr(), o_bt.data_ptr(), acc, _stream())
    dwf, dbf = ops.wgrad(_X(dz12), [_X(xs, mod=n, B=B2), _X(x12, shift=n, mod=B2)], _spec2(Cn), B2, H, W, 1, Cn, dev, p_wf, p_bf,
                         keep=(dz12, xs, x12), window=window, merge_pgemm=True)
    return dx12, dxs, dwf, dbf, dgamma, dbeta, dwc, dbc


def _attention_dx(g_o, c12, dv, w_dx, w4, owner, dx12, accumulate):
    """dx12[:nb] (=|+=) what the attention hands back to the value convolutions' input: through the matrices w_dx of the vfree
    form, or dv through the value convolutions."""
    Cn = dx12.shape[3]
    if w_dx is not None:
        nb = w_dx.shape[0]
        conv_launch([_X(g_o), _X(c12, B=nb)], w_dx, _spec2(Cn), None, None, dx12, nb, bpg=1, accumulate=accumulate)
    else:
        nb = dv.shape[0]
        dgrad_launch(_X(dv), w4, _dense_spec(Cn), 0, owner, dx12, nb, bpg=nb // w4.shape[0], accumulate=accumulate)


class BIETwinFn(torch.autograd.Function):
    """inputs: x12 [2n,H,W,C] = [first; second], xs [n,H,W,C], then the 16 parameter tensors
    (res.conv1 w,b; res.conv2 w,b; convf w,b; norm w,b; clustering w,b; unclustering w,b; v1 w,b; v2 w,b).
    outputs: o12 = [softmax(att1) v1 + Res(second); softmax(att2) v2 + Res(first)], xs_new.
    Every step covers all 2n images; v1 / v2 are two weight groups of one launch; the crossed residual is a batch-rotated
    read.  Keeps the unfused centre chain (FUSE_CHAIN off, the bf16 mode) and writes dx12 into the input's gradient slot."""

    @staticmethod
    def forward(ctx, x12, xs, rw1, rb1, rw2, rb2, wf, bf, gamma, beta, wc, bc, wu, bu, wv1, bv1, wv2, bv2, scale, eps):
        _need_gpu(x12)
        x12, xs = x12.contiguous(), xs.contiguous()
        B2, H, W, Cn = x12.shape
        n = B2 // 2
        dev = x12.device
        s1, s2 = _dense_spec(Cn), _spec2(Cn)
        # residual block on both halves (shared weights)
        t12, r12 = _new(B2, x12), _new(B2, x12)
        ops.res_block_fwd(_X(x12), rw1, rb1, rw2, rb2, s1, t12, r12)
        # centres: clustering(LN(convf(cat[xs, other half])))
        fused = chain_supported(Cn)
        if fused:       # one launch; saved for backward: yhat (normalised, before the affine) and rstd
            z12, stats, c12 = _centres_fwd(x12, xs, wf, bf, gamma, beta, wc, bc, eps)
            y12 = z12
        else:
            z12, y12, c12 = _new(B2, x12), _new(B2, x12), _new(B2, x12)
            conv_launch([_X(xs, mod=n, B=B2), _X(x12, shift=n, mod=B2)], wf.detach().reshape(1, Cn, 2 * Cn, 1), s2, wf, bf.detach(), z12, B2)
            stats = torch.empty(B2 * H * W * 2, device=dev, dtype=torch.float32)
            lib.call(lib._ln_fwd, "bmc_layernorm_fwd", z12.data_ptr(), gamma.data_ptr(), beta.data_ptr(), B2 * H * W, Cn, eps,
                     y12.data_ptr(), stats.data_ptr(), _stream())
            conv_launch([_X(y12)], wc.detach().reshape(1, Cn, Cn, 1), s1, wc, bc.detach(), c12, B2)
        # values: v1 on the first half, v2 on the second (two weight groups); attention per sample, residual = the OTHER half's block
        w4, owner, bias = _value_weights((wv1, wv2), (wv1, wv2), (bv1, bv2), (bv1, bv2))
        vfree = vfree_supported(B2 * H * W)
        o12, p, v12, G0, sc = _attention_fwd(_X(c12), _X(x12), _X(r12, shift=n, mod=B2), w4, owner, bias, scale, B2, x12, vfree)
        xs_new = _uncluster_fwd(c12, wu, bu, xs)
        ctx.save_for_backward(x12, xs, t12, z12, stats, y12, c12, G0 if vfree else v12, p, rw1, rw2, wf, gamma, wc, wu, wv1, wv2, beta,
                              *((sc, bv1, bv2) if vfree else ()))
        ctx.vfree = vfree
        ctx.owners = (rw1, rw2, wf, wc, wu)
        ctx.window = ops.current_window()
        ctx.params = (rw1, rb1, rw2, rb2, wf, bf, gamma, beta, wc, bc, wu, bu)     # the caller's objects (gradient sinks)
        ctx.vparams = (wv1, wv2, bv1, bv2)
        ctx.scale = scale
        ctx.fused = fused
        ctx.gslot = getattr(x12, "_bmc_gslot", None)     # (set before .contiguous(): see the top of this function)
        return o12, xs_new

    @staticmethod
    def backward(ctx, do12, dxs_new):
        saved = ctx.saved_tensors           # (once: a second access breaks torch.utils.checkpoint's unpack bookkeeping)
        x12, xs, t12, z12, stats, y12, c12, v12, p, rw1, rw2, wf, gamma, wc, wu, wv1, wv2, beta = saved[:18]
        G0 = sc = bvs = None
        if ctx.vfree:
            G0, v12, sc, bvs = v12, None, saved[18], saved[19:]
        o_rw1, o_rw2, o_wf, o_wc, o_wu = ctx.owners
        p_rw1, p_rb1, p_rw2, p_rb2, p_wf, p_bf, p_gamma, p_beta, p_wc, p_bc, p_wu, p_bu = ctx.params
        p_wv, p_bv = ctx.vparams[:2], ctx.vparams[2:]
        B2, H, W, Cn = x12.shape
        n = B2 // 2
        dev = x12.device
        s1, s2 = _dense_spec(Cn), _spec2(Cn)
        g_o = do12.contiguous() if do12 is not None else torch.zeros_like(x12)
        g_x = dxs_new.contiguous() if dxs_new is not None else torch.zeros_like(xs)
        w4, owner, bias = _value_weights(p_wv, (wv1, wv2), p_bv, bvs)
        dc12, dv12, w_dx, dwv, dbv, dwu, dbu = _attention_bwd(g_o, g_x, x12, c12, v12, p, G0, sc, w4, bias, ctx.scale, p_wv, p_bv,
                                                              p_wu, p_bu, wu, ctx.window)
        if ctx.fused:               # y12 holds yhat, stats rstd
            dx12, dxs, dwf, dbf, dgamma, dbeta, dwc, dbc = _chain_bwd_tail(
                dc12, y12, stats, gamma, beta, wf, wc, g_x, xs, x12, (p_wf, p_bf, p_gamma, p_beta, p_wc, p_bc), ctx.window,
                ds1=ops.grad_slot(ctx.gslot, x12))
            _attention_dx(g_o, c12, dv12, w_dx, w4, owner, dx12, True)                                         # dx12 += attention
        else:
            w_f, w_c = wf.detach().reshape(1, Cn, 2 * Cn, 1), wc.detach().reshape(1, Cn, Cn, 1)
            dx12 = ops.grad_slot(ctx.gslot, x12)
            _attention_dx(g_o, c12, dv12, w_dx, w4, owner, dx12, False)                                        # dx12  =
            # ---- clustering, LayerNorm, convf
            dwc, dbc = ops.wgrad(_X(dc12), [_X(y12)], s1, B2, H, W, 1, Cn, dev, p_wc, p_bc, keep=(dc12, y12), window=ctx.window, merge_pgemm=True)
            dy12 = _new(B2, x12)
            dgrad_launch(_X(dc12), w_c, s1, 0, o_wc, dy12, B2)
            dz12 = _new(B2, x12)
            ws = torch.empty(2 * 1024 * Cn, device=dev, dtype=torch.float32)
            sg = ops.sink_group([p_gamma, p_beta])
            if sg is not None:
                (o_g, o_bt), ln_acc = sg
                dgamma = dbeta = None
            else:
                o_g = dgamma = torch.empty(Cn, device=dev, dtype=torch.float32)
                o_bt = dbeta = torch.empty(Cn, device=dev, dtype=torch.float32)
                ln_acc = 0
            lib.call(lib._ln_bwd, "bmc_layernorm_bwd", dy12.data_ptr(), z12.data_ptr(), stats.data_ptr(), gamma.data_ptr(),
                     B2 * H * W, Cn, dz12.data_ptr(), ws.data_ptr(), o_g.data_ptr(), o_bt.data_ptr(), ln_acc, _stream())
            dwf, dbf = ops.wgrad(_X(dz12), [_X(xs, mod=n, B=B2), _X(x12, shift=n, mod=B2)], s2, B2, H, W, 1, Cn, dev, p_wf, p_bf,
                                 keep=(dz12, xs, x12), window=ctx.window, merge_pgemm=True)
            dxs = _new(n, x12)
            dgrad_launch(_X(dz12, b0=0, B=n), w_f, s2, 0, o_wf, dxs, n, residual=_X(g_x))                      # dxs  = skip + half 0
            dgrad_launch(_X(dz12, b0=n, B=n), w_f, s2, 0, o_wf, dxs, n, accumulate=True)                       # dxs += half 1
            dgrad_launch(_X(dz12, shift=n, mod=B2), w_f, s2, 1, o_wf, dx12, B2, accumulate=True)               # dx12 += (rotated)
        # ---- residual block, upstream gradient = batch-rotated g_o: dx12 += conv1^T + skip
        _, dw1, db1, dw2, db2 = ops.res_block_bwd(_X(g_o, shift=n, mod=B2), g_o, _X(x12), x12, t12, rw1, rw2, (o_rw1, o_rw2),
                                                  (p_rw1, p_rb1, p_rw2, p_rb2), s1, ctx.window, dx=dx12)
        gv = (None,) * 4 if dwv is None else (dwv[0].reshape(wv1.shape), dbv[0], dwv[1].reshape(wv2.shape), dbv[1])
        return (dx12, dxs, dw1, db1, dw2, db2, dwf, dbf, dgamma, dbeta, dwc, dbc, dwu, dbu, *gv, None, None)


class BIEFirstFn(torch.autograd.Function):
    """BIETwinFn without everything that only feeds its SECOND output (the last ParallelBlk of the backbone never reads it,
    models/BMCNet.py:75-82): x12 [2n,H,W,C] = [first; second], xs [n,H,W,C] ->
        o1 = softmax(att1) v1(first) + Res(second)   [n],   xs_new = unclustering(cat[c1, c2]) + xs   [n].
    The same steps over narrower windows: the residual block on the second half only, values / Gram / softmax / attention on
    the first half only (one weight group); both centres are still needed (unclustering) and come from the one fused chain
    launch.  Needs the fused chain; no gradient slot."""

    @staticmethod
    def forward(ctx, x12, xs, rw1, rb1, rw2, rb2, wf, bf, gamma, beta, wc, bc, wu, bu, wv1, bv1, scale, eps):
        _need_gpu(x12)
        x12, xs = x12.contiguous(), xs.contiguous()
        B2, H, W, Cn = x12.shape
        n = B2 // 2
        t2, r2 = _new(n, x12), _new(n, x12)
        ops.res_block_fwd(_X(x12, b0=n, B=n), rw1, rb1, rw2, rb2, _dense_spec(Cn), t2, r2)
        yhat, rstd, c12 = _centres_fwd(x12, xs, wf, bf, gamma, beta, wc, bc, eps)
        w4, owner, bias = _value_weights((wv1,), (wv1,), (bv1,), (bv1,))
        vfree = vfree_supported(B2 * H * W)
        o1, p, v1, G0, sc = _attention_fwd(_X(c12, B=n), _X(x12, B=n), _X(r2), w4, owner, bias, scale, n, x12, vfree)
        xs_new = _uncluster_fwd(c12, wu, bu, xs)
        ctx.save_for_backward(x12, xs, t2, yhat, rstd, c12, G0 if vfree else v1, p, rw1, rw2, wf, gamma, wc, wu, wv1, beta,
                              *((sc, bv1) if vfree else ()))
        ctx.vfree = vfree
        ctx.owners = (rw1, rw2, wf, wc, wu, wv1)
        ctx.window = ops.current_window()
        ctx.params = (rw1, rb1, rw2, rb2, wf, bf, gamma, beta, wc, bc, wu, bu, wv1, bv1)     # the caller's objects (gradient sinks)
        ctx.scale = scale
        return o1, xs_new

    @staticmethod
    def backward(ctx, do1, dxs_new):
        saved = ctx.saved_tensors
        x12, xs, t2, yhat, rstd, c12, v1, p, rw1, rw2, wf, gamma, wc, wu, wv1, beta = saved[:16]
        G0 = sc = bvs = None
        if ctx.vfree:
            G0, v1, sc, bvs = v1, None, saved[16], saved[17:]
        o_rw1, o_rw2, o_wf, o_wc, o_wu, o_wv1 = ctx.owners
        p_rw1, p_rb1, p_rw2, p_rb2, p_wf, p_bf, p_gamma, p_beta, p_wc, p_bc, p_wu, p_bu, p_wv1, p_bv1 = ctx.params
        n, Cn = x12.shape[0] // 2, x12.shape[3]
        g_o = do1.contiguous() if do1 is not None else torch.zeros_like(t2)
        g_x = dxs_new.contiguous() if dxs_new is not None else torch.zeros_like(xs)
        w4, owner, bias = _value_weights((o_wv1,), (wv1,), (p_bv1,), bvs)
        dc12, dv1, w_dx, dwv1, dbv1, dwu, dbu = _attention_bwd(g_o, g_x, x12, c12, v1, p, G0, sc, w4, bias, ctx.scale, (p_wv1,), (p_bv1,),
                                                               p_wu, p_bu, wu, ctx.window)
        if dwv1 is not None:
            dwv1 = dwv1.view(wv1.shape)                 # ([C,C] from the vfree form's products)
        dx12, dxs, dwf, dbf, dgamma, dbeta, dwc, dbc = _chain_bwd_tail(
            dc12, yhat, rstd, gamma, beta, wf, wc, g_x, xs, x12, (p_wf, p_bf, p_gamma, p_beta, p_wc, p_bc), ctx.window)
        _attention_dx(g_o, c12, dv1, w_dx, w4, owner, dx12, True)                                              # dx12[first] += attention
        # ---- residual block (second half), upstream gradient = g_o: dx12[second] += conv1^T + skip
        _, dw1, db1, dw2, db2 = ops.res_block_bwd(_X(g_o), g_o, _X(x12, b0=n, B=n), x12, t2, rw1, rw2, (o_rw1, o_rw2),
                                                  (p_rw1, p_rb1, p_rw2, p_rb2), _dense_spec(Cn), ctx.window, dx=dx12, out_b0=n)
        return (dx12, dxs, dw1, db1, dw2, db2, dwf, dbf, dgamma, dbeta, dwc, dbc, dwu, dbu, dwv1, dbv1, None, None)


def bie_first(m, x12, xs):
    """m: models.submodules.BIE; -> (o1, xs_new) (BIEFirstFn)."""
    r = m.conv1
    return BIEFirstFn.apply(x12, xs, r.conv1.weight, r.conv1.bias, r.conv2.weight, r.conv2.bias, m.convf1.weight,
                            m.convf1.bias, m.norm_s.weight, m.norm_s.bias, m.clustering.weight, m.clustering.bias,
                            m.unclustering.weight, m.unclustering.bias, m.v1.weight, m.v1.bias, m.scale, m.norm_s.eps)


def bie_twin(m, x12, xs):
    """m: models.submodules.BIE module (parameter container)."""
    r = m.conv1
    return BIETwinFn.apply(x12, xs, r.conv1.weight, r.conv1.bias, r.conv2.weight, r.conv2.bias, m.convf1.weight,
                           m.convf1.bias, m.norm_s.weight, m.norm_s.bias, m.clustering.weight, m.clustering.bias,
                           m.unclustering.weight, m.unclustering.bias, m.v1.weight, m.v1.bias, m.v2.weight, m.v2.bias,
                           m.scale, m.norm_s.eps)


class Stack2Fn(torch.autograd.Function):
    """Declares that tensors a and b (which already ARE the two batch halves of `buf`) form one tensor -- no copy;
    backward hands each producer its half of the gradient as a view."""

    @staticmethod
    def forward(ctx, a, b, slot):
        buf, n = slot.t, a.shape[0]
        assert a.data_ptr() == buf.data_ptr() and b.data_ptr() == buf[n:].data_ptr() and buf.shape[0] == 2 * n
        ctx.n = n
        return buf

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.n], g[ctx.n:], None


class Unstack2Fn(torch.autograd.Function):
    """t [2n,...] -> (t[:n], t[n:]) as views; backward concatenates the two gradients with ONE copy (the generic
    slice backward would zero-fill and add two full-size tensors)."""

    @staticmethod
    def forward(ctx, t, n=None):
        # (n: split point, default the middle -- models/BMCNet.py's [xs_p_st; xs_n_st | xs] is a 2B / B split)
        n = t.shape[0] // 2 if n is None else n
        ctx.n = n
        ctx.shape = t.shape
        return t[:n], t[n:]

    @staticmethod
    def unstack(t):
        """apply() + the gradient-pair tags on the two views (ops.GradPair): consumers that know the protocol write their
        input gradients into the halves of one buffer, and backward below hands it on without a copy."""
        a, b = Unstack2Fn.apply(t)
        if t.requires_grad and a.grad_fn is not None:
            pair = ops.GradPair(t.shape[0] // 2, t.shape)
            a._bmc_gslot, b._bmc_gslot = (pair, 0), (pair, 1)
            a.grad_fn.pair = pair        # backward drops the pair's reference to the buffer (graph nodes outlive their backward)
        return a, b

    @staticmethod
    def backward(ctx, g1, g2):
        if g1 is not None and g2 is not None and g1.is_contiguous() and g2.is_contiguous() \
                and g1.untyped_storage().data_ptr() == g2.untyped_storage().data_ptr() \
                and g2.storage_offset() == g1.storage_offset() + g1.numel():
            # the two gradients already lie back to back in one buffer (ops.StackViewsFn.backward hands out such views)
            out = torch.empty(0, device=g1.device, dtype=g1.dtype)
            out.set_(g1.untyped_storage(), g1.storage_offset(), tuple(ctx.shape), torch.empty(ctx.shape, device="meta").stride())
            pair = getattr(ctx, "pair", None)
            if pair is not None:
                pair.buf = None          # `out` owns the storage from here on
            return out, None
        pair = getattr(ctx, "pair", None)
        if pair is not None:
            pair.buf = None
        z = lambda k: torch.zeros((k,) + tuple(ctx.shape[1:]), device=(g1 if g1 is not None else g2).device)
        return torch.cat([g1 if g1 is not None else z(ctx.n), g2 if g2 is not None else z(ctx.shape[0] - ctx.n)], 0), None
