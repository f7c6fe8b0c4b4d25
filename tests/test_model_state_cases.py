"""Keeps the table of tests/model_state_cases.py honest against ampis_amd/csrc/model.hip, without a GPU: every extern "C" entry point whose
body marks the split copies stale (`split_stale = true`), clears `finalized` or writes `img_hw` is named by at least one case, and the table
names no function the file does not define.  A mutator added later fails here until it gets a case.  Nothing else is searched for in the
source."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import model_state_cases as T

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ampis_amd", "csrc", "model.hip")
MUTATES = re.compile(r"m->split_stale\s*=\s*true|m->finalized\s*=\s*false|m->img_hw\s*(=[^=]|\.\s*(assign|clear|resize|push_back|swap|insert|erase)\b)")
HEADER = re.compile(r"^(?!static\b)[A-Za-z_][\w \*]*?\b(amp_\w+)\s*\(", re.M)


def entry_points():
    """{name: body} of the definitions inside model.hip's `extern "C" { ... }` block (and its one-line extern "C" definitions).  A definition
    starts at column 0 and ends with the next `}` at column 0, or, for a one-line definition, where the next one starts."""
    text = open(SRC).read()
    out = {}
    for m in re.finditer(r'^extern "C" \w[\w \*]*?\b(amp_\w+)\s*\(.*$', text, re.M):
        out[m.group(1)] = m.group(0)
    start = text.index('\nextern "C" {\n')
    end = text.index('\n}  // extern "C"')
    for chunk in re.split(r"^}.*$", text[start:end], flags=re.M):
        heads = list(HEADER.finditer(chunk))
        for h, nxt in zip(heads, heads[1:] + [None]):
            out[h.group(1)] = chunk[h.start():nxt.start() if nxt else len(chunk)]
    return out


def test_the_parser_sees_the_entry_points_it_is_about():
    ep = entry_points()
    for name in ("amp_model_create", "amp_model_load_tensor", "amp_model_finalize", "amp_model_infer", "amp_model_forward_losses",
                 "amp_model_forward_backward", "amp_model_sgd_step", "amp_model_sgd_step_ex", "amp_model_set_image_sizes", "amp_model_get_tap",
                 "amp_debug_set_rpn_train_fuse"):
        assert name in ep, name
    assert "train_entry" not in ep and "refresh_split_weights" not in ep          # static / internal functions are no entry points
    assert "sgd_chunks_run" in ep["amp_model_sgd_step"] and "sgd_chunks_run" not in ep["amp_model_sgd_step_ex"]          # one body per name


def test_every_mutating_entry_point_has_a_case():
    mutators = sorted(n for n, body in entry_points().items() if MUTATES.search(body))
    assert {"amp_model_sgd_step", "amp_model_sgd_step_ex", "amp_model_load_tensor", "amp_model_broadcast_params", "amp_model_set_image_sizes"} <= set(mutators)
    named = {f for c in T.CASES for f in c["calls"]}
    missing = [n for n in mutators if n not in named]
    assert not missing, f"entry points that change the model's derived state without a case in tests/model_state_cases.py: {missing}"


def test_the_table_names_only_functions_that_exist():
    ep = entry_points()
    unknown = sorted({f for c in T.CASES for f in c["calls"]} - set(ep))
    assert not unknown, unknown


def test_the_table_is_well_formed():
    names = [c["name"] for c in T.CASES]
    assert len(set(names)) == len(names)
    for c in T.CASES:
        assert callable(c["apply"]) and c["what"] and c["calls"] and set(c["sizes"]) <= set("ab") and "a" in c["sizes"], c["name"]
    at_b = {c["name"] for c in T.CASES if "b" in c["sizes"]}
    assert at_b == {"sgd_plain", "sgd_general", "two_steps_no_infer", "infer_between_steps", "forward_only_after_step"}
