"""The package boundary of the drop-in recipe of INTEGRATION.md.  The recipe itself (the reference's own import block with
sys.path = [bmcnet-esr_amd, reference]) needs the reference's source tree: tests/dropin_check.py checks it by hand where
that tree exists (BMC_REFERENCE=<reference tree> python tests/dropin_check.py)."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_package_does_not_shadow_reference_packages():
    """Nothing under bmcnet-esr_amd/ may be named like a reference package other than `models` (the boundary)."""
    pkg = os.path.join(os.path.dirname(HERE), "bmcnet-esr_amd")
    top = {n.split(".")[0] for n in os.listdir(pkg) if not n.startswith("__")}
    assert not top & {"dataloader", "config", "loss", "logger", "myutils", "generate_dataset", "train", "infer_BMCNet"}, top
