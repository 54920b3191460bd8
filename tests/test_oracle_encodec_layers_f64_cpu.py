"""CPU suite: every activation between the layers of the C oracle's Encodec (RefEncodec.trace) against the binary64 layers of tests/ref64.py,
at exactly the cases tests/test_encodec_layers_gpu.py holds the engine to the oracle bit for bit.

The oracle shares its fma chains, its GroupNorm sums and its definitions (reflect index, GroupNorm count, eps, gate order) with the
engine, so "engine == oracle" cannot see a definition both state the same wrong way; torch.nn.functional in binary64 can.  A layer is
judged on the oracle's own binary32 taps that feed it (encodec_layers.judge_tap), its statistics on the conv output they were taken on.
The ratios oracle error / ATen's binary32 error per layer kind are measured here over all cases;
`python tests/test_oracle_encodec_layers_f64_cpu.py --write-bounds` records the largest per kind in tests/golden/op_error_bounds.json,
and M of the judge follows from the recorded figure.  Each test prints one OPREPORT line (run with -s).
"""
import json
import sys

import numpy as np
import pytest

import encodec_layers as EL
import ref64
from oracle import c_oracle

_refs, _traces = {}, {}


def oracle(name):
    if name not in _refs:
        cfg, _, blob = EL.model(name)
        _refs[name] = c_oracle.RefEncodec(cfg, blob)
    return _refs[name]


def trace(case):
    """(input, the oracle's taps) of a case, computed once and shared."""
    if case not in _traces:
        x = EL.case_input(case)
        _traces[case] = (x, oracle(case[0]).trace(x, decoder=case[1] == "dec"))
    return _traces[case]


_judged = {}


def judge_case(case, M):
    """Every tap of a case -> {kind: largest error / ATen error}, largest error / allowed, largest statistics error in ulp32."""
    if (case, M is None) in _judged:
        return _judged[(case, M is None)]
    name, stack, B, L = case
    cfg, sd, _ = EL.model(name)
    x, taps = trace(case)
    table = EL.layers(cfg, stack)
    assert len(taps) == len(table) == 3 + 4 * len(cfg.ratios)
    ratios, worst, worst_stats = {}, 0.0, 0.0
    for i, (layer, (v, stats, raw)) in enumerate(zip(table, taps)):
        what = f"{EL.case_id(case)} tap {i} {layer['name']}"
        kind, ratio, rel = EL.judge_tap(cfg, sd, layer, EL.tap_inputs(taps, layer, x), v, what, M)
        if ratio is not None:
            ratios[kind] = max(ratios.get(kind, 0.0), ratio)
        worst = max(worst, rel)
        assert (stats is not None) == ("_gn" in kind), what
        if stats is not None:
            worst_stats = max(worst_stats, EL.judge_stats(stats, raw, what))
    _judged[(case, M is None)] = (ratios, worst, worst_stats)
    if M is not None:
        _judged[(case, True)] = _judged[(case, False)]          # the ratios of a judged case are the measured ones
    return ratios, worst, worst_stats


@pytest.mark.parametrize("case", EL.CASES, ids=EL.case_id)
def test_oracle_taps_hold_to_the_binary64_layers(case):
    ratios, worst, worst_stats = judge_case(case, EL.multipliers())
    print("\nOPREPORT " + json.dumps(dict(kernel="oracle_encodec_layers", case=EL.case_id(case), worst_err_over_allowed=worst,
                                          err_over_aten_err=ratios, stats_ulp32=worst_stats), sort_keys=True))


@pytest.mark.parametrize("case", EL.TOO_SHORT, ids=EL.case_id)
def test_a_residual_block_on_one_sample_is_refused(case):
    with pytest.raises(RuntimeError):
        oracle(case[0]).trace(EL.case_input(case), decoder=case[1] == "dec")


def measure():
    out = {k: 0.0 for k in EL.KINDS}
    for case in EL.CASES:
        for k, r in judge_case(case, None)[0].items():
            out[k] = max(out[k], r)
    return out


def test_recorded_ratios_cover_the_measured_ones_and_fix_the_multipliers():
    """M[kind] = the next integer above 1.25 x the recorded ratio; what this machine measures must stay inside it.
    Finding: only the convolutions behind a GroupNorm with more than 128 terms need more than the precedent of 4, and they need it in
    step with the length of the reduction (largest ratio per length: about 2 up to 128 terms, 3 to 5 at 192 .. 512, 6 at 768 .. 1792,
    9.3 at 3584): the canonical convolution is ONE fma chain per output in ascending order, whose rounding error grows with the chain,
    where ATen's blocked GEMM adds short partial sums.  It is the cost of the order-exact arithmetic the engine and the oracle share,
    not a definition error; every other kind stays at or below 4.  The four mutations of a definition (reflect index, GroupNorm count,
    eps, gate order) are caught at these tolerances."""
    with open(EL.BOUNDS_PATH) as f:
        rec = json.load(f)["encodec_layers"]["oracle_error_over_aten_error"]
    got, M = measure(), EL.multipliers()
    print("\nOPREPORT " + json.dumps(dict(kernel="oracle_encodec_layers", measured=got, recorded=rec, M=M), sort_keys=True))
    assert set(rec) == set(EL.KINDS)
    for k in EL.KINDS:
        assert M[k] == int(np.floor(1.25 * rec[k])) + 1, (k, rec[k], M[k])
        assert got[k] <= 1.25 * rec[k], f"{k}: oracle error / ATen error {got[k]:.3f} here, {rec[k]} recorded"


@pytest.mark.parametrize("name", ["A", "C", "D1", "E"])
def test_last_taps_are_the_frames_of_encode_and_decode(name):
    """Pins the tap numbering to the model: the last encoder tap is the `emb` of encode_frame (on the RMS-normalised clip), the last decoder
    tap times the scale is decode_frame's output, bit for bit."""
    cfg, sd, _ = EL.model(name)
    ref = oracle(name)
    L = {"A": 258, "C": 400, "D1": 132, "E": 257}[name]
    x = EL.case_input((name, "enc", 2, L))
    codes, scale, emb = ref.encode_frame(x, want_emb=True)
    xn = x if scale is None else (x / scale.reshape(-1, 1, 1)).astype(np.float32)
    taps = ref.trace(xn)
    assert np.array_equal(taps[-1][0], emb), "the last encoder tap is not encode_frame's latent"
    z = np.zeros((2, cfg.dimension, codes.shape[-1]), np.float32)
    for q in range(codes.shape[1]):
        z = z + sd[f"quantizer.layers.{q}.codebook.embed"][codes[:, q]].transpose(0, 2, 1)
    out = ref.trace(z, decoder=True)[-1][0]
    if scale is not None:
        out = (out * scale.reshape(-1, 1, 1)).astype(np.float32)
    assert np.array_equal(out, ref.decode_frame(codes, scale)), "the last decoder tap is not decode_frame's output"


def test_pad_plan_small_inputs_keep_their_zero_extension():
    """ref64.sconv_pad_plan against the lengths the oracle's stack produces for rows shorter than the pads (D9)."""
    assert ref64.sconv_pad_plan(3, 7, 1, False) == (3, 3, 1) and ref64.sconv_pad_plan(4, 7, 1, False) == (3, 3, 0)
    assert ref64.sconv_pad_plan(5, 7, 1, True) == (6, 0, 2)
    assert ref64.sconv_pad_plan(2, 8, 4, False) == (2, 4, 3)              # extra right padding 2, then the zero extension to 5 samples
    taps = oracle("A").trace(EL.case_input(("A", "enc", 1, 3)))
    assert taps[0][0].shape[-1] == 4 and taps[-1][0].shape[-1] == 4


def _write_bounds():
    with open(EL.BOUNDS_PATH) as f:
        tab = json.load(f)
    tab["encodec_layers"] = {
        "what": "largest (|C oracle tap - binary64 layer| / |ATen binary32 layer - binary64 layer|) per layer kind over encodec_layers.CASES, "
                "each layer on the oracle's own binary32 input taps; per tap the largest element error, the rms error for taps of fewer than "
                "encodec_layers.MIN_ELEMS elements; le128 / le512 / gt512: Cin x K terms of the convolution.  M of the judge = "
                "floor(1.25 x ratio) + 1",
        "generator": "python tests/test_oracle_encodec_layers_f64_cpu.py --write-bounds",
        "oracle_error_over_aten_error": {k: round(float(v) + 5e-4, 3) for k, v in measure().items()}}
    with open(EL.BOUNDS_PATH, "w") as f:
        json.dump(tab, f, indent=1)
        f.write("\n")
    print(json.dumps(tab["encodec_layers"], indent=1))


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-bounds"]:
        _write_bounds()
    else:
        sys.exit("usage: python tests/test_oracle_encodec_layers_f64_cpu.py --write-bounds")
