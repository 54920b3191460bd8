"""GPU suite: the decisions of launch_conv (csrc/nc_conv.hip) held to a recorded fixture.

Every convolution path is bit-exact against the oracle, so the op tests cannot see a launch that moved to another kernel instance, tile
or staging form: only the benchmark can, as a time.  With NC_LAUNCH_LOG set the engine writes one "conv_plan ..." line per launch_conv
call -- form, kernel symbol, grid, threads, LDS bytes and, for the template, TM TN NW CB flat narrow slim dist xv co_group n_co_tiles
n_t_tiles n_cb xw xneg -- and this test compares those lines, case by case and in order, with tests/golden/conv_plans.json.

The fixture was recorded with the launch_conv that preceded the plan / launch split (given only the log line, written from its locals),
so a line that differs is a change of behaviour: it is fixed in the engine, never in the fixture.  The fixture keeps, per case, each
distinct line once in the order of first appearance (the observed lines are reduced the same way), and for a switch row only the cases
whose lines differ from the default row's; every case is compared in every row.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import test_ops_gpu as T  # noqa: E402
from conftest import dac_cfg_from_meta, encodec_cfg_from_meta, load_golden, snac_cfg_from_meta  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_plans.json")
PREFIX = "conv_plan "
# the families conv_instance() serves (csrc/nc_conv.hip) and the six paths launch_conv tries in front of the template
TEMPLATE_FORMS = {"plain", "narrow", "slim", "sub", "sub_narrow", "subg", "fused", "fusedw", "in2", "in2_sub", "dist", "dist_sub",
                  "xv", "xv_fused", "xv_sub", "xv_subg"}
SPECIAL_FORMS = {"skinny", "thin_inm", "thin", "stem", "small", "pointwise", "k3_stream"}

# The first four rows of test_children_gpu.FALLBACK_ROWS (the four-row subset of the switch matrix that test began as), then the three
# switches that undo a planning step outright.
ROWS = [
    {},
    {"NC_NO_GN_FUSE": "1", "NC_NO_IN2": "1", "NC_NO_CONV3S": "1"},
    {"NC_LSTM_STEPWISE": "1", "NC_NO_TINY_TILES": "1", "NC_NO_SUBPIXEL": "1"},
    {"NC_NO_FUSE": "1", "NC_ENCODEC_NO_FUSE": "1", "NC_DAC_RVQ_STAGEWISE": "1"},
    {"NC_NO_FLAT_GN": "1", "NC_LSTM_NO_ELU": "1", "NC_NO_DIST_SMALL": "1", "NC_LSTM_UB": "2", "NC_NO_SUBPIXEL_ANY": "1"},
    {"NC_NO_FLAT": "1"},
    {"NC_NO_XV": "1"},
    {"NC_NO_TILE_ALTS": "1"},
]


# Forms the case lists of tests/test_ops_gpu.py do not reach, each at the smallest shape that does: its EXTRA_* lists (kept there, where
# the same shapes are held to the oracle by value).
EXTRA_CONV1D, EXTRA_SUBPIXEL, EXTRA_RES_UNIT = T.EXTRA_CONV1D, T.EXTRA_SUBPIXEL, T.EXTRA_RES_UNIT


def row_key(row):
    return "+".join(f"{k}={v}" for k, v in sorted(row.items())) or "default"


def _unique(lines):
    return list(dict.fromkeys(lines))


# ------------------------------------------------------------------------------------------------------------------- the child
def _op_cases():
    """(key, thunk) per launch sequence: the case builders of tests/test_ops_gpu.py over their own case lists, engine only."""
    def conv(builder, *a):
        def run():
            sp = builder(*a)
            T._engine(sp[0] if isinstance(sp, tuple) else sp)
        return f"{builder.__name__[5:]}{a}", run

    def res_unit(C, Tn, d, B):
        def run():
            sp7, sp1 = T.case_res_unit(C, Tn, d, B, seed=C + d)
            T._engine(sp7)
            T._engine(sp1)
            # the one-launch unit; the whole-channel tile of the wide units is not packed under these two switches (as in test_ops_gpu)
            if C < 192 or not any(os.environ.get(k) == "1" for k in ("NC_NO_WIDE_FUSE", "NC_NO_TILE_ALTS")):
                T.ops.res_unit(sp7["x"], sp7["w"], sp7["b"], sp7["alpha_in"], sp7["alpha_out"], sp1["w"], sp1["b"], dil=d, fused=True)
        return f"res_unit{(C, Tn, d, B)}", run

    out = [conv(T.case_conv1d, *c) for c in T.CONV_CASES]
    out += [conv(T.case_conv_transpose, *c) for c in T.TRANSPOSE_CASES]
    out += [conv(T.case_flattened, *c) for c in T.FLAT_CASES]
    out += [conv(T.case_subpixel, *c) for c in T.SUBPIXEL_CASES]
    out += [conv(T.case_small, *c) for c in T.SMALL_CASES]
    out += [conv(T.case_k16_wide, *c) for c in T.K16_WIDE_CASES]
    out += [conv(T.case_short_row_stride1, 7, *c) for c in T.K7_SHORT_CASES]
    out += [conv(T.case_short_row_stride1, 3, *c) for c in T.K3_SHORT_CASES]
    out += [conv(T.case_pointwise_short, *c) for c in T.POINTWISE_SHORT_CASES]
    out += [res_unit(*c) for c in T.RES_UNIT_CASES]
    out += [conv(T.case_tanh_head)]
    out += [conv(T.case_epilogue, *c, sn, rs) for c in T.EPI_SHAPES for sn in (False, True) for rs in (False, True)]
    out += [conv(T.case_conv1d, *c) for c in EXTRA_CONV1D] + [conv(T.case_subpixel, *c) for c in EXTRA_SUBPIXEL] + [res_unit(*c) for c in EXTRA_RES_UNIT]
    return out


def _model_cases():
    from neuralcodecs_amd import DAC, SNAC, Encodec
    from neuralcodecs_amd.weights import (dac_synthetic_state_dict, encodec_synthetic_state_dict, save_blob, snac_noise,
                                          snac_synthetic_state_dict)
    kinds = {"dac": (DAC, dac_cfg_from_meta, dac_synthetic_state_dict), "snac": (SNAC, snac_cfg_from_meta, snac_synthetic_state_dict),
             "encodec": (Encodec, encodec_cfg_from_meta, encodec_synthetic_state_dict)}
    for name in ("dac_small", "snac_small", "snac_small_attn", "encodec_small24", "encodec_small48"):
        kind = name.split("_")[0]
        cls, cfg_of, weights = kinds[kind]
        g = load_golden(name)
        cfg = cfg_of(g["meta"])
        m = cls(cfg)
        m.load_blob(save_blob(weights(cfg, seed=g["meta"]["weight_seed"])))
        st = {}

        def encode(m=m, g=g, st=st):
            st["enc"] = m.encode(g["pcm"])

        def decode(m=m, g=g, st=st, kind=kind, cfg=cfg):
            enc = st["enc"]
            if kind == "dac":
                m.decode(enc[0])
            elif kind == "snac":
                m.decode(enc, snac_noise(cfg, g["meta"]["B"], g["z"].shape[-1], seed=g["meta"]["noise_seed"]))
            else:
                m.decode(enc, g["pcm"].shape[-1])
            m.dispose()

        yield f"{name} encode", encode
        yield f"{name} decode", decode


def _child(out_path):
    log = os.environ["NC_LAUNCH_LOG"]
    pos = 0

    def new_lines():
        nonlocal pos
        if not os.path.exists(log):      # (the engine opens the log at its first launch)
            return []
        with open(log) as f:
            f.seek(pos)
            new = f.read()
            pos = f.tell()
        return [ln[len(PREFIX):] for ln in new.splitlines() if ln.startswith(PREFIX)]

    seen = {}
    for cases in (_op_cases(), _model_cases()):
        for key, run in cases:
            new_lines()                  # (whatever loading a model launched is not part of a case)
            run()
            assert key not in seen, key
            seen[key] = _unique(new_lines())
    with open(out_path, "w") as f:
        json.dump(seen, f)


def run_row(row, tmp_path, n):
    """One fresh child for a switch row (the switches are read once per process); returns {case: [distinct log lines in order]}."""
    out = str(tmp_path / f"plans_{n}.json")
    e = dict(os.environ, NC_CONV_PLAN_CHILD=out, NC_LAUNCH_LOG=str(tmp_path / f"launch_{n}.log"), **row)
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (row, r.stdout[-3000:], r.stderr[-1500:])
    with open(out) as f:
        return json.load(f)


def test_conv_plans_match_the_recorded_fixture(tmp_path):
    """One child after the other, each under its own timeout; the first child that does not exit 0 ends the test."""
    if os.environ.get("NC_CONV_PLAN_CHILD"):
        _child(os.environ["NC_CONV_PLAN_CHILD"])
        return                                              # (a child does not start children)
    with open(FIXTURE) as f:
        want = json.load(f)["rows"]
    assert set(want) == {row_key(r) for r in ROWS}
    n_lines, forms = 0, set()
    for n, row in enumerate(ROWS):
        got = run_row(row, tmp_path, n)
        exp = {case: want[row_key(row)].get(case, lines) for case, lines in want["default"].items()}
        assert list(got) == list(exp), (row, "the cases differ", sorted(set(got) ^ set(exp)))
        for case in exp:
            assert got[case] == exp[case], (f"{row_key(row)}: {case}: launch_conv decided otherwise than the recorded parent", got[case], exp[case])
            n_lines += len(got[case])
            forms |= {ln.split()[0] for ln in got[case]}
    assert forms <= TEMPLATE_FORMS | SPECIAL_FORMS, sorted(forms - TEMPLATE_FORMS - SPECIAL_FORMS)
    print("\nCONVPLANS " + json.dumps(dict(rows=len(ROWS), lines=n_lines, forms=sorted(forms),
                                          unreached=sorted((TEMPLATE_FORMS | SPECIAL_FORMS) - forms))))
