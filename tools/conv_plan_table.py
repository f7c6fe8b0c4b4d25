"""tests/golden/conv_plan_table.json: which launch conv_run gives each layer (csrc/conv_plan.h conv_plan), one row per distinct combination of
selection inputs and switch state.

python tools/conv_plan_table.py            rewrite the "chosen" half of every row from its inputs through amp_debug_conv_plan (no GPU)
python tools/conv_plan_table.py --check    exit 1 and list the rows whose recorded choice differs, write nothing

A pull request that changes a selection rule runs the first form and commits the result: the fixture diff shows exactly which layers moved.
tests/test_conv_plan.py holds the library to the table."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.json")

# the order amp_debug_conv_plan reads its two integer arrays in, and the order of a row's "chosen" list
INPUTS = ["mode", "B", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "relu", "res_mode", "out_mode", "groups", "fmt", "in_shift", "force_f32",
          "has_res", "has_mask", "has_scale", "fuse", "rpn_ld"]
SWITCHES = ["f16x3_bn256", "short_k", "tall64", "split_ring", "korder", "patch256", "nloop", "mask_tail_loop", "patch_conv", "stagger", "generic_epi", "ablate"]
CHOSEN = ["kernel", "epi", "ntn", "nblk", "stagger", "dominant", "nloop_nt"]
ERROR = ["ERROR", 0, 0, 0, 0, 0, 0]      # conv_run refuses the combination


class PlanOut(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("kernel", "epi", "ntn", "nblk", "stagger", "dominant", "tiles_x", "tiles_y", "nloop_nt", "rpn_nbp")]


def _lib():
    from ampis_amd import _lib
    L = _lib.lib()
    L.amp_debug_conv_plan.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(PlanOut)]
    L.amp_debug_conv_plan.restype = C.c_int
    L.amp_debug_conv_kernel_name.argtypes = [C.c_int]
    L.amp_debug_conv_kernel_name.restype = C.c_char_p
    return L


def kernel_names():
    """Every value of amp::ConvKernel, in enum order."""
    L, out = _lib(), []
    while L.amp_debug_conv_kernel_name(len(out)) is not None:
        out.append(L.amp_debug_conv_kernel_name(len(out)).decode())
    return out


def plan(inputs, switches):
    """The "chosen" list amp_debug_conv_plan gives for one row's inputs and switch state."""
    assert len(inputs) == len(INPUTS) and len(switches) == len(SWITCHES)
    L, o = _lib(), PlanOut()
    if L.amp_debug_conv_plan((C.c_int * len(inputs))(*inputs), (C.c_int * len(switches))(*switches), C.byref(o)) != 0:
        return list(ERROR)
    return [L.amp_debug_conv_kernel_name(o.kernel).decode(), o.epi, o.ntn, o.nblk, o.stagger, o.dominant, o.nloop_nt]


def load(path=TABLE):
    t = json.load(open(path))
    assert t["inputs"] == INPUTS and t["switches"] == SWITCHES and t["chosen"] == CHOSEN, "column lists of the table and of this tool differ"
    return t


def save(t, path=TABLE):
    with open(path, "w") as f:      # one row per line: a moved layer is one changed line
        f.write("{\n")
        for k in ("what", "inputs", "switches", "chosen"):
            f.write(f" {json.dumps(k)}: {json.dumps(t[k])},\n")
        f.write(' "rows": [\n')
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in t["rows"]))
        f.write("\n ]\n}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    t = load()
    moved = 0
    for r in t["rows"]:
        now = plan(r[0], r[1])
        if now != r[2]:
            moved += 1
            print(dict(zip(INPUTS, r[0])), {k: v for k, v in zip(SWITCHES, r[1])}, ":", r[2], "->", now)
            r[2] = now
    print(f"{moved} of {len(t['rows'])} rows differ")
    if args.check:
        sys.exit(1 if moved else 0)
    save(t)


if __name__ == "__main__":
    main()
