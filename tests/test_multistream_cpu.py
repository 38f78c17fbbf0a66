"""CPU checks of multi-stream inference (infer.MultiStreamSR): the slot scheduler (pure Python) and the gfx950 code of the
slot kernels (csrc/slots.hip: no flat memory instructions, no scratch), with the ISA helpers of test_isa_hygiene.py."""
import os
import shutil
import subprocess

import pytest

from infer import SlotScheduler


def _run(sched):
    plans = []
    while True:
        p = sched.plan()
        if p is None:
            return plans
        plans.append(p)


def test_slot_order_reuse_and_window_indices():
    s = SlotScheduler(2)
    a, b, c = s.add(3), s.add(1), s.add(2)
    assert (a, b, c) == (0, 1, 2)
    plans = _run(s)
    assert plans == [
        [(a, 0, True), (b, 0, True)],
        [(a, 1, False), (c, 0, True)],      # b finished: slot 1 is reused by the next queued recording, with a reset
        [(a, 2, False), (c, 1, False)],
    ]
    assert not s.pending()


def test_empty_slots_and_late_arrivals():
    s = SlotScheduler(3)
    a = s.add(2)
    assert s.plan() == [(a, 0, True), None, None]
    b = s.add(1)                                # queued mid-run: takes the first free slot
    assert s.plan() == [(a, 1, False), (b, 0, True), None]
    assert s.plan() is None
    c = s.add(1)
    assert s.plan() == [(c, 0, True), None, None]
    assert s.plan() is None


def test_every_window_runs_once_in_order():
    s = SlotScheduler(3)
    lens = [5, 1, 4, 2, 7, 3, 1]
    hs = [s.add(n) for n in lens]
    seen = {h: [] for h in hs}
    slot_of = {}
    for p in _run(s):
        assert len(p) == 3
        for k, e in enumerate(p):
            if e is None:
                continue
            h, i, reset = e
            assert reset == (i == 0)
            assert slot_of.setdefault(h, k) == k       # a recording stays in its slot
            seen[h].append(i)
    assert all(seen[h] == list(range(n)) for h, n in zip(hs, lens))


def test_empty_queue():
    s = SlotScheduler(4)
    assert not s.pending()
    assert s.plan() is None
    assert s.plan() is None


@pytest.mark.parametrize("bad", [0, 257, -1])
def test_slot_count_is_checked(bad):
    with pytest.raises(ValueError):
        SlotScheduler(bad)


def test_recording_without_windows_is_refused():
    with pytest.raises(ValueError):
        SlotScheduler(2).add(0)


# ------------------------------------------------------------------ ISA of csrc/slots.hip
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def slots_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    from test_isa_hygiene import CSRC, ROOT, _kernels
    d = tmp_path_factory.mktemp("isa_slots")
    o = os.path.join(d, "slots.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", o, os.path.join(CSRC, "slots.hip")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    ks = {n: k for n, k in _kernels(o).items() if "NumVgprs" in k}
    shutil.rmtree(d, ignore_errors=True)
    assert len(ks) == 3, sorted(ks)
    return ks


def test_slot_kernels_have_no_flat_memory_instructions(slots_isa):
    assert not [(n, k["flat"]) for n, k in slots_isa.items() if k["flat"]]


def test_slot_kernels_have_no_scratch(slots_isa):
    assert not [(n, k["ScratchSize"]) for n, k in slots_isa.items() if k["ScratchSize"]]
