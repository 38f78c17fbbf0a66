#!/usr/bin/env python3
"""Launch sequence and result bits of one small training pass, one JSON line per case: the ordered (kind, flops) list of the
conv / pixel-reduction / weight-gradient launches (ops.PROFILE), the loss's bit pattern and the SHA-256 of every parameter's
.grad.  The pass is deterministic, so two commits that route every launch alike print byte-identical output: the check for
a refactor of the dispatch layer.  Uses only the models, ops.set_math and ops.PROFILE.

    python tools/step_trace.py [case index ...]        (default: all cases)
"""
import hashlib
import json
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bmcnet-esr_amd"))

from bmc_hip import ops  # noqa: E402
from models.BMCNet import BMCNet  # noqa: E402
from models.BMCNet_plain import BMCNet_plain  # noqa: E402

SCALE, N_C, N_B = 4, 128, 2
# (model, H, W, batch, math mode, move every bias off zero: the forward F(4x4) launches need dense biases)
CASES = [(m, 31, 56, 4, "fp32", False) for m in ("BMCNet", "BMCNet_plain")]             # merged and paired routes
CASES += [(m, 90, 120, 2, "fp32", False) for m in ("BMCNet", "BMCNet_plain")]
CASES += [(m, 180, 240, 1, "fp32", nz) for nz in (False, True) for m in ("BMCNet", "BMCNet_plain")]      # F(4x4) weight gradients
CASES += [("BMCNet", 31, 56, 4, "bf16", False), ("BMCNet", 31, 56, 4, "bf16x6", False)]


def run(name, H, W, B, math, nonzero_bias):
    dev = torch.device("cuda:0")
    ops.set_math(math)
    torch.manual_seed(1234)
    plain = name == "BMCNet_plain"
    model = (BMCNet_plain if plain else BMCNet)(SCALE, N_C, N_B)
    if nonzero_bias:
        g = torch.Generator().manual_seed(99)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n.endswith(".bias"):
                    p.add_((torch.randint(0, 2, p.shape, generator=g) * 2 - 1).to(p.dtype) * 1e-2)
    model.to(dev)
    g = torch.Generator().manual_seed(7)
    frames = torch.poisson(torch.full((B, 3, 2, H, W), 0.3), generator=g).to(dev)
    gts = torch.poisson(torch.full((B, 3, 2, SCALE * H, SCALE * W), 0.3), generator=g).to(dev)
    z = lambda c: torch.zeros(B, c, H, W, device=dev)
    state = (z(N_C), z(2 * SCALE * SCALE)) if plain else (z(N_C), z(N_C), z(N_C), z(2 * SCALE * SCALE))
    ops.PROFILE = []
    loss = 0
    for i in range(2):
        out = model.forward_loss(frames[:, i:i + 2].transpose(1, 2), *state, i == 0, gts[:, i + 1])
        state, loss = tuple(out[:-1]), loss + out[-1]
    loss.backward()
    torch.cuda.synchronize()
    launches, ops.PROFILE = [(r[0], r[1]) for r in ops.PROFILE], None
    counts = {}
    for kind, _ in launches:
        counts[kind] = counts.get(kind, 0) + 1
    grads = {n: hashlib.sha256(p.grad.detach().cpu().contiguous().numpy().tobytes()).hexdigest() if p.grad is not None else None
             for n, p in model.named_parameters()}
    return {"case": [name, H, W, B, math, nonzero_bias], "loss_bits": "%08x" % struct.unpack("<I", struct.pack("<f", float(loss.detach())))[0],
            "counts": dict(sorted(counts.items())), "launches": launches, "grads": grads}


def main():
    picks = [int(a) for a in sys.argv[1:]] or range(len(CASES))
    for i in picks:
        print(json.dumps(run(*CASES[i]), sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
