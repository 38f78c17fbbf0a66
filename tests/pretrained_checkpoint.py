"""The reference's pretrained checkpoint (pretrain/BMCNet_plain_nfs_x4.pth) rebuilt from the data stored under tests/golden/:
plain_pretrained_weights.npz holds its 24 distinct tensors, plain_pretrained_layout.json its 120 keys in file order with the
tensor each one aliases (tests/golden/make_golden_r2.py writes both).  The result is the state_dict torch.load gives for
that file: same keys, same order, aliased keys sharing one storage."""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def reference_checkpoint():
    z = np.load(os.path.join(GOLDEN, "plain_pretrained_weights.npz"), allow_pickle=False)
    tensors = {k[2:]: torch.tensor(z[k]) for k in z.files}
    with open(os.path.join(GOLDEN, "plain_pretrained_layout.json")) as f:
        keys = json.load(f)["keys"]
    return OrderedDict((k, tensors[owner]) for k, owner in keys)


def write_reference_checkpoint(path):
    """The checkpoint as a file, in torch.save's format (what the reference's own file is)."""
    torch.save(reference_checkpoint(), path)
    return path
