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


# ------------------------------------------------------------------ the layout of the slot table (bmc_hip/slots.py)
def test_table_layout_offsets_and_refusals():
    """The byte offsets of a table of S = 3 slots, as literals: every section is S entries of its struct behind the one before
    (40, 192, 48 / 56 timed, 24 and 64 bytes an entry); a section that is off takes no room."""
    from bmc_hip import slots
    sections, total = slots.table_layout(3, events=True, emit=True, timed=True, clock=True, hot=True)
    assert sections == [("slot", slots.SLOT_DTYPE, 0), ("events", slots.SLOT_EVENTS_DTYPE, 120),
                        ("emit", slots.SLOT_EMIT_TIMED_DTYPE, 696), ("clock", slots.SLOT_CLOCK_DTYPE, 864),
                        ("hot", slots.SLOT_HOT_DTYPE, 936)] and total == 1128
    sections, total = slots.table_layout(3, events=True, emit=True)
    assert sections[2] == ("emit", slots.SLOT_EMIT_DTYPE, 696) and total == 840 and len(sections) == 3
    sections, total = slots.table_layout(3, events=False, emit=True)
    assert sections == [("slot", slots.SLOT_DTYPE, 0), ("emit", slots.SLOT_EMIT_DTYPE, 120)] and total == 264
    assert slots.table_layout(3) == ([("slot", slots.SLOT_DTYPE, 0)], 120)
    with pytest.raises(ValueError, match="timed=True needs emit=True"):
        slots.table_layout(3, timed=True)
    with pytest.raises(ValueError, match="clock=True needs timed=True"):
        slots.table_layout(3, emit=True, clock=True)
    with pytest.raises(ValueError, match="hot=True needs events=True"):
        slots.table_layout(3, hot=True)


def test_session_limits_are_the_slot_limits():
    """Every MultiStreamSR.MAX_* is an alias of the limit bmc_hip/slots.py mirrors from include/bmc_hip.h, not a second copy."""
    from bmc_hip import slots
    from infer import MultiStreamSR
    aliases = dict(MAX_COUNT_LIMIT="MAX_COUNT_LIMIT", MAX_COUNT_TIMED="MAX_COUNT_TIMED", MAX_WINDOW_CAPACITY="MAX_WINDOW_CAPACITY",
                   MAX_VOXEL_BINS="MAX_VOXEL_BINS", MAX_ITEMS_FILTERED="HOT_MAX_ITEMS", MAX_SEQN_EVENTS="MAX_SEQN",
                   MAX_WIDTH_EVENTS="MAX_ENCODE_WIDTH")
    assert sorted(k for k in vars(MultiStreamSR) if k.startswith("MAX_")) == sorted(aliases)
    for name, limit in aliases.items():
        assert getattr(MultiStreamSR, name) is getattr(slots, limit), name


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
