"""The device assembly of csrc/optim.hip for tests/test_optim_cpu.py and tests/test_optim_clip_cpu.py: compiled once per process
as tests/test_isa_hygiene.py compiles the MFMA kernels, nothing is executed."""
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bmcnet-esr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# Waves per SIMD of every kernel in the commit BEFORE the two step families shared one walk (a gfx950 compile of that commit, not of
# the code under test): template arguments as they stand in the mangled name -> the Occupancy line.  The floor of this file's kernels.
PARENT_OCCUPANCY = {
    "adam_kernelILb1ELb1ELb0EE": 4, "adam_kernelILb1ELb0ELb0EE": 4,          # <AMS, NORM, CAP>
    "adam_kernelILb0ELb1ELb0EE": 5, "adam_kernelILb0ELb0ELb0EE": 5,
    "adam_kernelILb1ELb1ELb1EE": 3, "adam_kernelILb1ELb0ELb1EE": 3,
    "adam_kernelILb0ELb1ELb1EE": 4, "adam_kernelILb0ELb0ELb1EE": 4,
    "clip_step_kernelILb1ELb0EE": 2, "clip_step_kernelILb1ELb1EE": 2,        # <AMS, CAP>
    "clip_step_kernelILb0ELb0EE": 3, "clip_step_kernelILb0ELb1EE": 3,
    "grad_sq_kernelE": 8,
}


@functools.lru_cache(maxsize=None)
def kernels():
    """mangled kernel name -> {"flat", "ld16", "st16": instruction counts; "ScratchSize", "Occupancy": the compiler's figures}"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "optim.s")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                            "--cuda-device-only", "-o", out, os.path.join(CSRC, "optim.hip")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        found, cur = {}, None
        for ln in open(out):
            m = re.match(r"^(_Z\w+):", ln)
            if m:
                cur = found[m.group(1)] = {"flat": 0, "ld16": 0, "st16": 0}
                continue
            if cur is None:
                continue
            code = ln.split(";")[0]
            cur["flat"] += bool(re.search(r"\bflat_(load|store|atomic)", code))
            cur["ld16"] += "global_load_dwordx4" in code
            cur["st16"] += "global_store_dwordx4" in code
            m = re.match(r"^; (ScratchSize|Occupancy): (\d+)", ln)
            if m:
                cur[m.group(1)] = int(m.group(2))
                if m.group(1) == "Occupancy":
                    cur = None
    return found


def check_family(want):
    """What both device-assembly tests assert of the ONE translation unit: 8 adam_kernel, 4 clip_step_kernel, 1 grad_sq_kernel and
    one advance kernel, 14 in all; no flat_ memory instruction and no scratch memory anywhere; no kernel below its parent's occupancy.
    -> the kernels whose name holds `want`."""
    found = kernels()
    count = lambda part: sum(part in n for n in found)
    assert (count("adam_kernel"), count("clip_step_kernel"), count("grad_sq_kernel")) == (8, 4, 1), sorted(found)
    assert count("advance_kernel") == 1 == count("adam_advance_kernel") and len(found) == 14, sorted(found)
    for n, k in found.items():
        assert k["flat"] == 0 and k["ScratchSize"] == 0, (n, k)
    floors = {n: [f for part, f in PARENT_OCCUPANCY.items() if part in n] for n in found if "advance_kernel" not in n}
    assert all(len(f) == 1 for f in floors.values()) and len(floors) == len(PARENT_OCCUPANCY), floors
    for n, (floor,) in floors.items():
        assert found[n]["Occupancy"] >= floor, (n, found[n], floor)
    return {n: k for n, k in found.items() if want in n}
