"""Shared by the op tests (plain module, not a conftest): one description of a convolution case, the oracle's composition for it, and
the judgement of a binary32 result -- the oracle's on the CPU, the engine's on the GPU -- against the binary64 reference of ref64.py.

A case is a dict: x, w, b, stride, pad, dil, alpha_in, alpha_out, residual, transposed, out_pad, tanh_out (what ops.conv1d takes).
The result is  tanh?( snake_out?( conv(snake_in?(x)) + b + residual ) ).
"""
import json
import os

import numpy as np

import ref64
from oracle import c_oracle

BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_error_bounds.json")
MARGIN = 1.5            # on the measured activation tables: room for another libm's binary64 sin / tanh only (see the CPU test)
DECADES = list(range(-3, 4))      # |alpha x| (Snake) or |x| (tanh) in [10^d, 10^(d+1)); below 1e-3 counts as -3, 1e4 is the top edge


def spec(x, w, b=None, stride=1, pad=0, dil=1, alpha_in=None, alpha_out=None, residual=None, transposed=False, out_pad=0, tanh_out=False):
    return dict(x=x, w=w, b=b, stride=stride, pad=pad, dil=dil, alpha_in=alpha_in, alpha_out=alpha_out, residual=residual,
                transposed=transposed, out_pad=out_pad, tanh_out=tanh_out)


def oracle_input(sp):
    return c_oracle.snake(sp["x"], sp["alpha_in"]) if sp["alpha_in"] is not None else sp["x"]


def oracle_linear(sp):
    xin = oracle_input(sp)
    if sp["transposed"]:
        assert sp["residual"] is None and sp["dil"] == 1
        return c_oracle.conv_transpose1d(xin, sp["w"], sp["b"], sp["stride"], sp["pad"], sp["out_pad"])
    return c_oracle.conv1d(xin, sp["w"], sp["b"], sp["stride"], sp["pad"], sp["dil"], residual=sp["residual"])


def oracle_conv(sp):
    y = oracle_linear(sp)
    if sp["alpha_out"] is not None:
        y = c_oracle.snake(y, sp["alpha_out"])
    if sp["tanh_out"]:
        y = c_oracle.tanh(y)
    return y


def linear64(sp):
    """binary64 value and binary32 error bound of the linear part, on the oracle's own activated input (so that the error of the input
    activation, judged on its own, is not multiplied through the convolution)."""
    xin = oracle_input(sp)
    if sp["transposed"]:
        a = (xin, sp["w"], sp["b"], sp["stride"], sp["pad"], sp["out_pad"])
        return ref64.conv_transpose1d(*a), ref64.conv_transpose1d_bound(*a)
    a = (xin, sp["w"], sp["b"], sp["stride"], sp["pad"], sp["dil"], 1, sp["residual"])
    return ref64.conv1d(*a), ref64.conv1d_bound(*a)


_tables = None


def tables():
    global _tables
    if _tables is None:
        with open(BOUNDS_PATH) as f:
            _tables = json.load(f)
    return _tables


def _decade(a):
    a = np.abs(np.asarray(a, np.float64))
    with np.errstate(divide="ignore"):
        d = np.floor(np.log10(np.where(a > 0, a, 1e-30)))
    return np.clip(d, DECADES[0], DECADES[-1]).astype(np.int64) - DECADES[0]


def snake_tol(x, alpha):
    """Allowed |oracle Snake - binary64 Snake| per element: the measured table (ulp of the result, per decade of |alpha x|) times MARGIN.
    Defined for |alpha x| <= 1e4, the domain the table was measured on."""
    x = np.asarray(x, np.float64); a = np.asarray(alpha, np.float64).reshape(1, -1, 1)
    assert np.abs(a * x).max() <= 1e4
    tab = np.asarray(tables()["snake_ulp"], np.float64)
    return MARGIN * tab[_decade(a * x)] * ref64.ulp32(ref64.snake(x, alpha))


def tanh_tol(x):
    tab = np.asarray(tables()["tanh_ulp"], np.float64)
    return MARGIN * tab[_decade(x)] * ref64.ulp32(ref64.tanh(x))


def judge_conv(got, sp, what=""):
    """`got` (binary32: the oracle's or the engine's answer for case `sp`) against binary64.  Linear cases: |got - f64| <= dot_bound,
    element by element.  With an epilogue activation f the chain rule gives |f32(l32) - f64(l64)| <= |f32 - f64|(l32) + sup|f'| * |l32 - l64|
    with sup|f'| = sup|1 + sin(2 a x)| = 2 for Snake and 1 for tanh; the first term is the measured activation table.  Returns the largest
    error / allowed over the tensor (for the report)."""
    want, bound = linear64(sp)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, binary64 reference {want.shape}"
    allowed = bound
    if sp["alpha_out"] is not None or sp["tanh_out"]:
        # the activation acts on the binary32 linear value: recover it from the oracle (bit-equal to the engine's, which the caller asserts)
        lin32 = oracle_linear(sp)
        err_lin = np.abs(lin32.astype(np.float64) - want)
        assert np.all(err_lin <= bound), f"{what}: linear part off by {float((err_lin / np.maximum(bound, 1e-300)).max()):.3g} x bound"
        if sp["alpha_out"] is not None:
            tol_act = snake_tol(lin32, sp["alpha_out"])
            want = ref64.snake(want, sp["alpha_out"])
            allowed = 2.0 * bound + tol_act
            lin32 = c_oracle.snake(lin32, sp["alpha_out"])
        if sp["tanh_out"]:
            tol_t = tanh_tol(lin32)
            want = ref64.tanh(want)
            allowed = allowed + tol_t          # tanh' <= 1: what came in is not amplified
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(allowed, 1e-300)).max())
    assert np.all(err <= allowed), f"{what}: |binary32 - binary64| is {ratio:.3g} x the allowed error at its worst element"
    return ratio


# ---- the activation tables: measured from the oracle and binary64 alone -----------------------------------------------------------
ALPHAS = (1e-3, 0.05, 1.0, 7.3, 50.0,                 # the span a checkpoint can hold
          0.5, 0.6, 0.8, 1.25, 1.6, 2.0)               # and the range the op tests draw their alphas from ([0.5, 2): `_alpha`)


def activation_inputs(alpha):
    """x with |alpha x| from denormal to 1e4, both signs, zero: log-spaced magnitudes (dense per decade) plus the edges."""
    mags = np.concatenate([np.logspace(-6, 4, 40001) / alpha, [1e4 / alpha * (1 - 1e-7)], np.float32([1e-45, 1e-40, 1.1754944e-38, 0.0])])
    x = np.concatenate([mags, -mags]).astype(np.float32)
    return x[np.abs(np.float64(np.float32(alpha)) * x.astype(np.float64)) <= 1e4]


def measure_snake():
    """Largest |oracle - binary64| / ulp32(binary64 result) per decade of |alpha x| over ALPHAS."""
    out = np.zeros(len(DECADES))
    for alpha in ALPHAS:
        x = activation_inputs(alpha).reshape(1, 1, -1)
        a = np.float32([alpha])
        want = ref64.snake(x, a)
        err = np.abs(c_oracle.snake(x, a).astype(np.float64) - want) / ref64.ulp32(want)
        d = _decade(a.astype(np.float64).reshape(1, 1, 1) * x.astype(np.float64))
        for i in range(len(DECADES)):
            if np.any(d == i):
                out[i] = max(out[i], float(err[d == i].max()))
    return out


def measure_tanh():
    out = np.zeros(len(DECADES))
    x = activation_inputs(1.0)
    want = ref64.tanh(x)
    err = np.abs(c_oracle.tanh(x).astype(np.float64) - want) / ref64.ulp32(want)
    d = _decade(x)
    for i in range(len(DECADES)):
        if np.any(d == i):
            out[i] = max(out[i], float(err[d == i].max()))
    return out
