"""Shared by the Encodec layer tests (plain module, not a conftest): the reduced-depth configurations and cases, the table that says which
layer produces each tap of ops.encodec_trace / RefEncodec.trace from which taps, and the judgement of one tap against the binary64 layer
of tests/ref64.py.

A layer is judged on its own inputs: the oracle's binary32 taps that feed it (bit-equal to the engine's, which the GPU test asserts), so
error does not accumulate through the stack.  Tolerances: the first convolution of a weight-norm stack (no GroupNorm, no ELU on either
side) is held to ref64.conv1d_bound on the reflect-padded input; every other layer to M[kind] x the error of ATen's own binary32 answer
for the same layer on the same inputs.  M[kind] is the next integer above 1.25 x the largest oracle error / ATen error the CPU test
measures over CASES (tests/golden/op_error_bounds.json, "encodec_layers"); the engine is bit-equal to the oracle.

Two things keep M a statement about the arithmetic and not about the sample.  A convolution's kind carries the length of its reduction
(Cin x K terms: up to 128, up to 512, longer): the canonical convolution is one fma chain per output, whose error grows with the chain
where ATen's blocked sums do not, so a single multiplier would hold the 14-term stem to the figure the 3584-term layers need.  And "error"
is the largest element error only for taps of at least MIN_ELEMS elements; below that the largest of a few dozen errors is a draw, not a
scale (a 64-element tap once measured 4.8 where the same layer on 12 672 elements gives 1.95), so those taps are measured and judged by
their rms error against ATen's rms error.
"""
import dataclasses
import json
import os

import numpy as np
import torch

import ref64
from neuralcodecs_amd.config import EncodecConfig
from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob
from oracle import c_oracle

BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_error_bounds.json")
KINDS = ("conv_gn_le128", "conv_gn_le512", "conv_gn_gt512", "conv_le128", "conv_le512", "conv_transpose_gn", "conv_transpose", "lstm")
MIN_ELEMS = 1024            # taps with fewer elements: rms error instead of the largest element error
WEIGHT_SEED = 7


def _gn48(ratios, n_filters, **kw):
    """48 kHz-style: non-causal, time_group_norm, two channels, no segmentation; the sampling rate is ~150 x hop so that the frame rate gives
    the quantizer at least one codebook at the top bandwidth (bandwidth 24 -> n_q >= 1)."""
    hop = int(np.prod(ratios))
    return EncodecConfig(sampling_rate=150 * hop, channels=2, norm="time_group_norm", causal=False, normalize=True, segment_seconds=None,
                         target_bandwidths=(3.0, 6.0, 12.0, 24.0), bandwidth=24.0, n_filters=n_filters, ratios=tuple(ratios), **kw)


CONFIGS = {
    "A": _gn48((2,), 32),
    "B": _gn48((4, 2), 32),
    "C": _gn48((5, 4, 2), 32),
    "D": _gn48((2, 2), 128),
    "D1": _gn48((2, 2), 128, lstm_layers=1),
    "A1": dataclasses.replace(_gn48((2,), 32), channels=1),                      # mono (the RMS scale test)
    "E": EncodecConfig(sampling_rate=150 * 8, channels=1, norm="weight_norm", causal=True, normalize=False, n_filters=16, ratios=(4, 2),
                       target_bandwidths=(1.5, 3.0, 6.0, 12.0, 24.0), bandwidth=24.0),
}

# (config, stack, B, L): encoder rows of L samples, decoder rows of L frames.  Each is the smallest shape that reaches its form.
CASES = [
    # A: stem, res_a TMS 1, down2 | C = 64 persistent LSTM | up2 S = 2, thin head
    ("A", "enc", 1, 256), ("A", "enc", 3, 258), ("A", "enc", 1, 514),        # one res_a tile, a tile and two columns, three tiles
    ("A", "enc", 1, 257),                                                    # odd: the streaming kernels fall back
    ("A", "enc", 1, 3),                                                      # shorter than the k = 7 pad: zero extension, never trimmed (D9)
    ("A", "enc", 1, 2), ("A", "enc", 3, 62), ("A", "enc", 1, 64), ("A", "enc", 3, 66),      # 1, 31, 32, 33 frames at the LSTM
    ("A", "dec", 1, 128), ("A", "dec", 3, 129), ("A", "dec", 1, 257),        # 256 / 258 / 514 rows at the last stage; 129 and 257 frames: up2 falls back
    ("A", "dec", 1, 1), ("A", "dec", 3, 31), ("A", "dec", 1, 32), ("A", "dec", 3, 33),
    # B: res_a TMS 2, down4 | C = 128 step-wise | up2 S = 4
    ("B", "enc", 1, 256), ("B", "enc", 3, 516), ("B", "enc", 1, 514), ("B", "enc", 3, 258), ("B", "enc", 1, 1),   # 516 -> 258: T % 4 != 0; 514 -> 257: odd
    ("B", "enc", 1, 248),                                                    # 31 frames (256, 258 and 1 give 32, 33 and 1)
    ("B", "dec", 1, 32), ("B", "dec", 3, 33), ("B", "dec", 1, 31), ("B", "dec", 1, 1),
    # C: down5, the C = 128 block on conv3s / conv1x1 | C = 256 step-wise | stride-5 sub-pixel up-conv with pitched, shifted rows
    ("C", "enc", 1, 400), ("C", "enc", 3, 440), ("C", "enc", 1, 256), ("C", "enc", 3, 258),          # 256 -> 32: T % 5 != 0
    ("C", "enc", 1, 514), ("C", "enc", 1, 40), ("C", "enc", 3, 1240), ("C", "enc", 1, 1280), ("C", "enc", 3, 1320),   # 1, 31, 32, 33 frames
    ("C", "dec", 1, 10), ("C", "dec", 3, 11), ("C", "dec", 1, 4),
    ("C", "dec", 1, 1), ("C", "dec", 3, 31), ("C", "dec", 1, 32), ("C", "dec", 3, 33),
    # D: no streaming width matches (windowed fallbacks) | C = 512 persistent: one tile UBW 2, two tiles UBW 4; one layer
    ("D", "enc", 3, 16), ("D", "enc", 1, 4), ("D", "enc", 3, 124), ("D", "enc", 1, 128), ("D", "enc", 3, 132), ("D", "enc", 17, 160),
    ("D", "dec", 3, 32), ("D", "dec", 1, 33), ("D", "dec", 17, 40), ("D", "dec", 1, 1), ("D", "dec", 3, 31),
    ("D1", "enc", 3, 128), ("D1", "dec", 3, 32),
    # E: causal pads, weight norm, mono, no GroupNorm: derived bound on the first convolutions
    ("E", "enc", 1, 256), ("E", "enc", 3, 258), ("E", "enc", 1, 257), ("E", "enc", 1, 5),
    ("E", "dec", 1, 32), ("E", "dec", 3, 33),
]
# a residual block sees one sample: the stacks must raise
TOO_SHORT = [("C", "enc", 1, 1)]


def case_id(case):
    """cfgA_enc_B1_L256: tokens `pytest -k` (case-insensitive substrings) cannot find in another id or in a file name."""
    return "cfg{}_{}_B{}_L{}".format(*case)


_models = {}


def model(name):
    """(config, state dict, blob) of configuration `name` with the seeded synthetic weights, built once."""
    if name not in _models:
        cfg = CONFIGS[name]
        sd = encodec_synthetic_state_dict(cfg, seed=WEIGHT_SEED)
        _models[name] = (cfg, sd, save_blob(sd))
    return _models[name]


def case_input(case):
    name, stack, B, L = case
    cfg = CONFIGS[name]
    rng = np.random.default_rng(1000 * B + L + (17 if stack == "dec" else 0))
    if stack == "enc":
        return (rng.standard_normal((B, cfg.channels, L)) * 0.5).astype(np.float32)
    return (rng.standard_normal((B, cfg.dimension, L)) * 0.8).astype(np.float32)        # a sum of code vectors has about this spread


# ---------------------------------------------------------------------------------------------------------------- the layer table
def layers(cfg, stack):
    """One entry per tap, in tap order: name, op (conv | conv_transpose | lstm), key of its parameters, stride, inputs (tap indices, -1 = the
    stack's input; two inputs are summed inside the layer as the model does), elu_in (an ELU between the inputs and the convolution)."""
    out = []

    def add(name, op, key, inputs, stride=1, elu_in=False):
        out.append(dict(name=name, op=op, key=key, stride=stride, inputs=list(inputs), elu_in=elu_in))
        return len(out) - 1

    def block(p, key, x):
        s = add(f"{p}.shortcut", "conv", f"{key}.shortcut", [x])
        h = add(f"{p}.block.1 (k = 3)", "conv", f"{key}.block.1", [x], elu_in=True)
        y = add(f"{p}.block.3 (k = 1)", "conv", f"{key}.block.3", [h], elu_in=True)
        return s, y

    if stack == "enc":
        cur, n = add("encoder.0 (first conv)", "conv", "encoder.layers.0", [-1]), 1
        for r in reversed(cfg.ratios):
            s, y = block(f"encoder.{n}", f"encoder.layers.{n}", cur)
            cur = add(f"encoder.{n + 2} (down x{r})", "conv", f"encoder.layers.{n + 2}", [s, y], stride=r, elu_in=True)
            n += 3
        cur = add(f"encoder.{n} (LSTM)", "lstm", f"encoder.layers.{n}", [cur])
        add(f"encoder.{n + 2} (last conv)", "conv", f"encoder.layers.{n + 2}", [cur])         # (the LSTM tap carries the ELU)
    else:
        cur = add("decoder.0 (first conv)", "conv", "decoder.layers.0", [-1])
        ins, n, elu = [add("decoder.1 (LSTM)", "lstm", "decoder.layers.1", [cur])], 2, False
        for r in cfg.ratios:
            u = add(f"decoder.{n + 1} (up x{r})", "conv_transpose", f"decoder.layers.{n + 1}", ins, stride=r, elu_in=elu)
            ins, elu = list(block(f"decoder.{n + 2}", f"decoder.layers.{n + 2}", u)), True
            n += 3
        add(f"decoder.{n + 1} (last conv)", "conv", f"decoder.layers.{n + 1}", ins, elu_in=elu)
    return out


def kind_of(cfg, layer, sd=None):
    """op, GroupNorm or not and, for a convolution, the class of its reduction length Cin x K."""
    if layer["op"] == "lstm":
        return "lstm"
    kind = layer["op"] + ("_gn" if cfg.norm == "time_group_norm" else "")
    if layer["op"] == "conv":
        key = layer["key"] + (".conv.weight" if cfg.norm == "time_group_norm" else ".conv.weight_v")
        n = int(np.prod(sd[key].shape[1:]))
        kind += "_le128" if n <= 128 else "_le512" if n <= 512 else "_gt512"
    return kind


def derived(cfg, layer):
    """The layers with a derived bound: no GroupNorm behind the convolution, no pending GroupNorm and no ELU in front of it."""
    return cfg.norm != "time_group_norm" and layer["op"] == "conv" and layer["inputs"] == [-1]


def conv_params(cfg, sd, layer):
    """(dense binary32 weight, bias, GroupNorm affine or None) of a convolution layer; a weight-norm pair is folded by the oracle's fold (the
    fold is judged on its own in tests/test_oracle_cpu.py), so that the layer is judged on the weight the kernels see."""
    key = layer["key"]
    if key + ".conv.weight" in sd:
        w = sd[key + ".conv.weight"]
    else:
        v = np.ascontiguousarray(sd[key + ".conv.weight_v"], np.float32)
        g = np.ascontiguousarray(sd[key + ".conv.weight_g"], np.float32).reshape(-1)
        w = np.empty_like(v)
        c_oracle.lib().ref_fold_wn_snac(v, g, v.shape[0], int(np.prod(v.shape[1:])), w)
    gn = (sd[key + ".norm.weight"], sd[key + ".norm.bias"]) if cfg.norm == "time_group_norm" else None
    return w, sd.get(key + ".conv.bias"), gn


def lstm_params(cfg, sd, layer):
    return [tuple(sd[f"{layer['key']}.lstm.{nm}_l{i}"] for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for i in range(cfg.lstm_layers)]


def layer_fn(cfg, sd, layer):
    """f(*inputs, dtype=...) -> the layer's output in that precision (ref64 alone)."""
    if layer["op"] == "lstm":
        params = lstm_params(cfg, sd, layer)
        return lambda x, dtype=torch.float64: ref64.slstm_elu(x, params, dtype=dtype)
    w, b, gn = conv_params(cfg, sd, layer)
    f = ref64.seanet_conv if layer["op"] == "conv" else ref64.seanet_conv_transpose

    def run(x, x2=None, dtype=torch.float64):
        return f(x, w, b, stride=layer["stride"], causal=cfg.causal, gn=gn, elu_in=layer["elu_in"], x2=x2, dtype=dtype)
    return run


_tables = None


def multipliers():
    """M per kind: the next integer above 1.25 x the recorded ratio (the quarter: room for another libm in ATen)."""
    global _tables
    if _tables is None:
        with open(BOUNDS_PATH) as f:
            _tables = json.load(f)["encodec_layers"]["oracle_error_over_aten_error"]
    return {k: int(np.floor(1.25 * v)) + 1 for k, v in _tables.items()}


class _few_threads:
    """The layers here are tiny: ATen's default thread pool beside the oracle's OpenMP team only contends (7x slower on 8 cores)."""
    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(min(4, self.n))

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


def judge_tap(cfg, sd, layer, inputs, got, what, M):
    """|got - binary64 layer(inputs)| against the layer's tolerance.  Returns (kind, error / ATen's error or None for a derived bound, error /
    allowed).  M = None measures only (the CPU test's recorder): nothing is asserted but the shape and the derived bounds."""
    f = layer_fn(cfg, sd, layer)
    kind = kind_of(cfg, layer, sd)
    if derived(cfg, layer):
        w, b, _ = conv_params(cfg, sd, layer)
        xp = ref64.sconv_padded(torch.from_numpy(inputs[0]).double(), w.shape[2], layer["stride"], cfg.causal).numpy()
        want = f(*inputs)
        bound = ref64.conv1d_bound(xp, w, b, stride=layer["stride"])
        assert got.shape == want.shape, f"{what}: shape {got.shape}, binary64 layer {want.shape}"
        r = float((np.abs(got.astype(np.float64) - want) / np.maximum(bound, 1e-300)).max())
        assert r <= 1.0, f"{what}: |binary32 - binary64| is {r:.3g} x the derived bound at its worst element"
        return kind, None, r
    with _few_threads():
        want, aten = ref64.aten_errors(f, *inputs)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, binary64 layer {want.shape}"
    mine = np.abs(got.astype(np.float64) - want)
    if want.size >= MIN_ELEMS:
        err, aten_err, norm = float(mine.max()), float(aten.max()), "largest"
    else:
        err, aten_err, norm = float(np.sqrt((mine ** 2).mean())), float(np.sqrt((aten ** 2).mean())), "rms"
    ratio = err / aten_err if aten_err > 0 else (0.0 if err == 0 else float("inf"))
    if M is None:
        return kind, ratio, ratio
    assert err <= M[kind] * aten_err, (f"{what} [{kind}]: {norm} error {err:.3g} against binary64, ATen's own {aten_err:.3g} "
                                       f"(x{ratio:.3g}, allowed x{M[kind]})")
    return kind, ratio, ratio / M[kind]


def judge_stats(stats, raw, what):
    """(mean, rstd) of a tap's GroupNorm against the two-pass binary64 mean and variance of the binary32 conv output they were taken on,
    within 2 ulp32.  The sums are binary64, so the rounding to binary32 dominates -- while E[x^2] / var <= 1e6, asserted on the reference."""
    want, ratio = ref64.two_pass_stats(raw)
    assert np.all(ratio <= 1e6), f"{what}: E[x^2] / var = {ratio.max():.3g}: outside the range the 2 ulp bound is stated for"
    err = np.abs(stats.astype(np.float64) - want) / ref64.ulp32(want)
    assert np.all(err <= 2.0), f"{what}: (mean, rstd) off by {err.max(axis=0)} ulp32 from the two-pass binary64 statistics"
    return float(err.max())


def tap_inputs(taps, layer, x):
    return [x if i < 0 else taps[i][0] for i in layer["inputs"]]


def with_layers(cfg, n):
    return dataclasses.replace(cfg, lstm_layers=n)
