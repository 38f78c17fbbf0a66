"""ISA properties of the F(4x4) weight-gradient kernels (csrc/wino4_wgrad.hip), read from the gfx950 assembly: no flat memory
instructions, no scratch, two waves per SIMD, and no full vector-memory wait in front of an MFMA of the stage loop (the LDS-DMA
pieces are requested between MFMAs and waited for once, behind the stage's last MFMA)."""
import os
import re
import subprocess

import pytest

from test_isa_hygiene import CSRC, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    o = os.path.join(tmp_path_factory.mktemp("w4g"), "wino4_wgrad.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", o, os.path.join(CSRC, "wino4_wgrad.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return o


def _main(ks):
    hits = [(n, k) for n, k in ks.items() if "wino4_wgrad_kernel" in n]
    assert len(hits) == 1, list(ks)
    return hits[0][1]


def test_no_flat_no_scratch_two_waves_per_simd(asm):
    ks = _kernels(asm)
    k = _main(ks)
    assert k["flat"] == 0 and k["ScratchSize"] == 0 and k["scratch_in_loop"] == 0, k
    assert k["Occupancy"] == 2, k
    red = [v for n, v in ks.items() if "wino4_wgrad_reduce_kernel" in n]
    assert red and red[0]["flat"] == 0 and red[0]["ScratchSize"] == 0


def test_no_full_vector_memory_wait_in_front_of_an_mfma(asm):
    """Per basic block of the main kernel: an `s_waitcnt vmcnt(0)` may follow the block's MFMAs (the end of a stage), never
    precede one of them.  The 18 MFMAs of every stage form (8 wave roles x 3 loop forms) are all there."""
    body, name = [], None
    for ln in open(asm):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name = m.group(1)
            continue
        if name and "wino4_wgrad_kernel" in name:
            if re.match(r"^; -- End function", ln):
                break
            body.append(ln.split(";")[0] if not re.match(r"^; %bb\.\d+:", ln) else ln)
    blocks, cur = [], []
    for ln in body:
        if re.match(r"^\.LBB\d+_\d+:", ln) or re.match(r"^; %bb\.\d+:", ln):
            blocks.append(cur)
            cur = []
        cur.append(ln)
    blocks.append(cur)
    n_mfma = 0
    for b in blocks:
        seen_vm0 = False
        for ln in b:
            if re.search(r"s_waitcnt.*vmcnt\(0\)", ln):
                seen_vm0 = True
            if "v_mfma" in ln:
                n_mfma += 1
                assert not seen_vm0, "vmcnt(0) in front of an MFMA:\n" + "".join(b)
    assert n_mfma == 8 * 3 * 18, n_mfma
