"""Which kernel conv_run gives a layer (csrc/conv_plan.h conv_plan), without a GPU: tests/golden/conv_plan_table.json holds one row per distinct
combination of selection inputs and switch state that the benchmark (default and --full) and tests/test_{conv,conv_modes,x101,backward}_gpu.py
reach, with the launch the if / else chain of conv_run chose for it BEFORE conv_plan existed (recorded from that commit, not from this code);
the rows of the cases of tests/test_conv_exact_gpu.py came later and were recorded from the rules current then (the table's "what" field).
amp_debug_conv_plan must give exactly that: kernel, epilogue, N tiles, grid, stagger, dominant flag.  A pull request that changes a rule
regenerates the table (tools/conv_plan_table.py) and shows the moved layers as its diff."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# values of amp::ConvKernel without a row (none since the cases of tests/test_conv_exact_gpu.py have rows: F16X3S_256 -- a split input on 256-wide
# tiles with the ring kernel switched off -- was the last one)
UNREACHED = {}


def test_every_recorded_choice_is_reproduced():
    import conv_plan_table as T
    t = T.load()
    assert len(t["rows"]) > 1000
    keys = {(tuple(r[0]), tuple(r[1])) for r in t["rows"]}
    assert len(keys) == len(t["rows"]), "duplicate rows"
    wrong = [(r, now) for r in t["rows"] for now in [T.plan(r[0], r[1])] if now != r[2]]
    assert not wrong, f"{len(wrong)} rows differ, the first: {dict(zip(T.INPUTS, wrong[0][0][0]))} {dict(zip(T.SWITCHES, wrong[0][0][1]))}: " \
                      f"recorded {wrong[0][0][2]}, now {wrong[0][1]}"


def test_every_kernel_has_a_row():
    import conv_plan_table as T
    names = T.kernel_names()
    assert len(names) == len(set(names)) >= 20
    covered = {r[2][0] for r in T.load()["rows"]}
    assert covered - {"ERROR"} <= set(names)
    assert set(UNREACHED) <= set(names)
    assert not (set(UNREACHED) & covered), "a kernel listed as unreached has rows: take it off the list"
    missing = set(names) - covered - set(UNREACHED)
    assert not missing, f"no row reaches {sorted(missing)}"


def test_dominant_flag_belongs_to_the_dominant_kernels():
    import conv_plan_table as T
    for r in T.load()["rows"]:
        assert r[2][5] == (1 if r[2][0] in ("SPLIT_128x256", "PATCH256", "GLDS_128") else 0), r
