"""The launch lists of the two fused BIE autograd nodes (bmc_hip/bie.py: BIETwinFn, BIEFirstFn), pinned: the ordered entry-point
names that one forward and one backward pass through bmc_hip.lib.call, with weight packs cached (one warm-up pass), at
C = 32, n = 2, 13x21 in fp32 with the fused centre chain, for both forms of the attention (bie.VFREE forced on / off).

The lists below were recorded from the two nodes as they were written out twice (before they became compositions of one set of
launch steps); the order of the launches and of the ops.wgrad calls feeds the weight-gradient merge queue and the side stream,
so a step that moves shows here.  The memo of pointer tables (ops._TABLES) is keyed by device addresses, which depend on
what the allocator did before: the recorded pass starts with an empty memo, so every bmc_ptr_table launch of the pass is in
its list whatever ran earlier in the process.  Both nodes take xs_new from the same chain launch and the same unclustering launch: on the
same inputs it is bit-identical between them.
"""
import pytest
import torch

from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401

pytestmark = pytest.mark.gpu

# (node, VFREE) -> (forward, backward).  The tail of every backward list is the end-of-pass flush of the weight-gradient merge
# queue: per queued weight its pointer tables (one per operand), the pixel-reduction GEMM and its reduction.
LISTS = {
    ("twin", True): (
        ["bmc_conv", "bmc_conv", "bmc_chain_fwd", "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_small_mm",
         "bmc_softmax_fwd", "bmc_small_mm", "bmc_pack_weight", "bmc_conv", "bmc_conv"],
        ["bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_small_mm", "bmc_softmax_bwd", "bmc_small_mm",
         "bmc_pgemm_reduce_weight_groups", "bmc_small_mm", "bmc_small_mm", "bmc_small_mm", "bmc_pack_weight",
         "bmc_conv", "bmc_chain_bwd", "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_chain_affine_grads",
         "bmc_pack_weight", "bmc_conv", "bmc_conv", "bmc_conv", "bmc_ptr_table", "bmc_ptr_table", "bmc_ptr_table",
         "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_ptr_table", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm",
         "bmc_pgemm_reduce_weight", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight",
         "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight"]),
    ("twin", False): (
        ["bmc_conv", "bmc_conv", "bmc_chain_fwd", "bmc_conv", "bmc_pgemm", "bmc_pgemm_reduce_plain",
         "bmc_softmax_fwd", "bmc_pack_weight", "bmc_conv", "bmc_conv"],
        ["bmc_pgemm", "bmc_pgemm_reduce_plain", "bmc_softmax_bwd", "bmc_pack_weight", "bmc_conv", "bmc_pack_weight",
         "bmc_conv", "bmc_pgemm", "bmc_pgemm_reduce_weight_groups", "bmc_chain_bwd", "bmc_pgemm",
         "bmc_pgemm_reduce_weight", "bmc_chain_affine_grads", "bmc_conv", "bmc_conv", "bmc_conv", "bmc_ptr_table",
         "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_ptr_table", "bmc_ptr_table",
         "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm",
         "bmc_pgemm_reduce_weight", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight"]),
    ("first", True): (
        ["bmc_conv", "bmc_conv", "bmc_chain_fwd", "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_small_mm",
         "bmc_softmax_fwd", "bmc_small_mm", "bmc_pack_weight", "bmc_conv", "bmc_conv"],
        ["bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_small_mm", "bmc_softmax_bwd", "bmc_small_mm",
         "bmc_pgemm_reduce_weight", "bmc_small_mm", "bmc_small_mm", "bmc_small_mm", "bmc_pack_weight", "bmc_conv",
         "bmc_chain_bwd", "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_chain_affine_grads", "bmc_pack_weight",
         "bmc_conv", "bmc_conv", "bmc_conv", "bmc_ptr_table", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm",
         "bmc_pgemm_reduce_weight", "bmc_ptr_table", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm",
         "bmc_pgemm_reduce_weight", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight",
         "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight"]),
    ("first", False): (
        ["bmc_conv", "bmc_conv", "bmc_chain_fwd", "bmc_conv", "bmc_pgemm", "bmc_pgemm_reduce_plain",
         "bmc_softmax_fwd", "bmc_pack_weight", "bmc_conv", "bmc_conv"],
        ["bmc_pgemm", "bmc_pgemm_reduce_plain", "bmc_softmax_bwd", "bmc_pack_weight", "bmc_conv", "bmc_pack_weight",
         "bmc_conv", "bmc_chain_bwd", "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_chain_affine_grads", "bmc_conv",
         "bmc_conv", "bmc_conv", "bmc_ptr_table", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm",
         "bmc_pgemm_reduce_weight", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight",
         "bmc_ptr_table", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_ptr_table",
         "bmc_ptr_table", "bmc_pgemm", "bmc_pgemm_reduce_weight", "bmc_ptr_table", "bmc_ptr_table", "bmc_pgemm",
         "bmc_pgemm_reduce_weight"]),
}


def _run(node, vfree, monkeypatch):
    """-> (forward names, backward names, xs_new) of the second of two passes of `node` over fixed seeded inputs."""
    dev = _gpu()
    from bmc_hip import bie, lib, ops
    from models.submodules import BIE
    ops.set_math("fp32")
    monkeypatch.setattr(bie, "VFREE", vfree)
    monkeypatch.setattr(bie, "VFREE_MIN_PIXELS", 0)
    monkeypatch.setattr(bie, "FUSE_CHAIN", True)
    monkeypatch.setattr(ops, "ACCUM_PARAM_GRADS", True)
    torch.manual_seed(4)
    Cn, n, H, W = 32, 2, 13, 21
    m = BIE(Cn).to(dev)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(4.0).add_(0.05 * torch.randn_like(p))
    x12, xs = torch.randn(2 * n, H, W, Cn, device=dev), torch.randn(n, H, W, Cn, device=dev)
    go, gx = torch.randn(2 * n, H, W, Cn, device=dev), torch.randn(n, H, W, Cn, device=dev)
    names, call = [], lib.call

    def spy(fn, what, *args):
        names.append(what)
        return call(fn, what, *args)
    monkeypatch.setattr(lib, "call", spy)
    fn = bie.bie_twin if node == "twin" else bie.bie_first
    for rec in (False, True):      # (the first pass fills the weight-pack caches)
        for p in m.parameters():
            p.grad = None
        if rec:     # every pointer table of the recorded pass is built in it (bmc_ptr_table): the memo is keyed by addresses
            monkeypatch.setattr(ops, "_TABLES", {})
        a, b = x12.clone().requires_grad_(), xs.clone().requires_grad_()
        torch.cuda.synchronize()
        del names[:]
        o, xs_new = fn(m, a, b)
        fwd = list(names)
        del names[:]
        torch.autograd.backward([o, xs_new], [go[:o.shape[0]], gx])
        torch.cuda.synchronize()
        bwd = list(names)
    assert a.grad is not None and b.grad is not None
    return fwd, bwd, xs_new.detach()


@pytest.mark.parametrize("vfree", [True, False], ids=["vfree", "explicit"])
@pytest.mark.parametrize("node", ["twin", "first"])
def test_bie_node_launch_list(node, vfree, monkeypatch):
    fwd, bwd, _ = _run(node, vfree, monkeypatch)
    want_fwd, want_bwd = LISTS[node, vfree]
    assert fwd == want_fwd
    assert bwd == want_bwd


@pytest.mark.parametrize("vfree", [True, False], ids=["vfree", "explicit"])
def test_first_output_node_shares_xs_new_with_twin_bit_for_bit(vfree, monkeypatch):
    _, _, xs_twin = _run("twin", vfree, monkeypatch)
    _, _, xs_first = _run("first", vfree, monkeypatch)
    assert torch.equal(xs_first, xs_twin)
