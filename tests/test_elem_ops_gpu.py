"""GPU suite: the HBM-bound SNAC kernels (csrc/nc_elem.hip, nc_snac_unit.hip) one at a time through their nc_op_* hooks, at the shapes
where their launchers change kernels and where tiles end -- not only at the few shapes the shipped presets reach inside whole models.

Every case has two judges: np.array_equal(engine, oracle piece) for the bits, and |engine - binary64| <= bound for the meaning
(tests/ref64.py).  The bound is derived where one exists (depthwise taps, pooling, the unit's pointwise chain: ref64.dot_bound, plus the
measured Snake table of tests/golden/op_error_bounds.json behind an activation); LayerNorm and attention (rsqrt, softmax) have none, so
theirs is M_ATEN_* times the error of ATen's own binary32 CPU answer against binary64, computed per case from the two references alone.
Each test prints one `OPREPORT {...}` line (cases, kernel forms by the launcher's rule, largest error / allowed): run with -s to see them.
"""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ref64  # noqa: E402
from neuralcodecs_amd import _lib, ops  # noqa: E402
from op_judge import judge_conv, oracle_conv, snake_tol, spec  # noqa: E402
from oracle import c_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# engine error <= M x ATen's own error, per case.  Started at 4 (ATen's exp is within 1 ulp, the canonical one within 2, and the summation
# orders differ); the largest ratios observed are 1.52 (LayerNorm) and 1.96 (attention, W = 16, one head), both below 2: so 2
# (tests/golden/op_error_bounds.json keeps the figures).
M_ATEN_LN = 2
M_ATEN_ATTN = 2


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _alpha(rng, c):
    a = (0.5 + 1.5 * rng.random(c)).astype(np.float32)
    a[::5] = 0.0
    return a


def _report(kernel, **kw):
    print("\nOPREPORT " + json.dumps(dict(kernel=kernel, **kw), sort_keys=True))


# The kernel form a launcher took is OBSERVED in the children of test_every_form_of_the_launchers_is_observed_and_leaves_this_file_true:
# they run with NC_LAUNCH_LOG set from their first launch on (the engine opens the log once per process), the launchers write one
# "elem <kernel name>" line per launch, and every case asserts those lines against the form the rules below expect.
_LOG = os.environ.get("NC_LAUNCH_LOG") if os.environ.get("NC_ELEM_OPS_CHILD") == "1" else None
_log_pos = 0


def _check_forms(expected, what=""):
    """The "elem" lines the engine logged since the last call are exactly `expected` (in a child; a no-op where no log is kept)."""
    global _log_pos
    if _LOG is None:
        return
    with open(_LOG) as f:
        f.seek(_log_pos)
        new = f.read()
        _log_pos = f.tell()
    seen = [ln[5:] for ln in new.splitlines() if ln.startswith("elem ")]
    assert seen == list(expected), f"{what}: the engine launched {seen}, the launcher's rule says {list(expected)}"


def _env_int(name, dflt):
    try:
        return int(os.environ.get(name, dflt))
    except ValueError:
        return dflt


# ---------------------------------------------------------------------------------------------------------------- depthwise
DW_T = [1, 3, 4, 5, 53, 54, 55, 2044, 2047, 2048, 2049, 2052, 4096 + 2, 6144]
DW_C = [1, 3, 64, 96]
DW_B = [1, 3]
DW_SCALAR_T = [1, 5, 64, 2047, 2048, 2052, 4098]
DW_SCALAR_ONLY = [   # (K, pad, dil): what only dwconv_kernel serves
    (1, 0, 1), (3, 1, 1), (5, 2, 1), (5, 6, 3),             # other kernel sizes, "same" padding
    (7, 0, 1), (7, 7, 1), (7, 0, 3), (7, 21, 3), (7, 0, 9), (7, 63, 9), (3, 0, 1), (3, 3, 1),   # pad != 3 * dil: 0 and K * dil
    (7, 6, 2), (3, 2, 2), (7, 0, 2), (7, 14, 2),            # dilation 2
]


def dw_form(K, pad, dil, T):
    """launch_dwconv's rule (the hook's buffers come from hipMalloc: 16-byte aligned)."""
    vec = os.environ.get("NC_DW_NO_VEC") != "1" and K == 7 and pad == 3 * dil and dil in (1, 3, 9) and T % 4 == 0 and T >= 4
    return f"dwconv_vec_kernel<{dil}>" if vec else "dwconv_kernel"


def dw_oracle(xin, w, b, pad, dil):
    """The oracle's depthwise convolution (groups == C) as the hook defines it: the first T outputs over the zero-extended rows."""
    C, K = w.shape
    T = xin.shape[2]
    if 2 * pad == dil * (K - 1):
        return c_oracle.conv1d(xin, w.reshape(C, 1, K), b, 1, pad, dil, groups=C)
    right = max(0, (K - 1) * dil - pad)
    xp = np.ascontiguousarray(np.pad(xin, ((0, 0), (0, 0), (pad, right))))
    return np.ascontiguousarray(c_oracle.conv1d(xp, w.reshape(C, 1, K), b, 1, 0, dil, groups=C)[:, :, :T])


def dw_judge(got, x, w, b, pad, dil, ai, ao, what):
    """A depthwise result (the engine's, or on the CPU the oracle's own) for x, w, b and the Snakes ai / ao (None: no Snake): equal to the
    oracle's composition bit for bit, and within the binary64 bound: K taps + bias on the oracle-activated input, then the Snake table
    (|Snake'| <= 2 carries the linear error through).  Returns the largest error / allowed."""
    xin = c_oracle.snake(x, ai) if ai is not None else x
    lin32 = dw_oracle(xin, w, b, pad, dil)
    want = c_oracle.snake(lin32, ao) if ao is not None else lin32
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{what}: max abs diff {np.abs(got - want).max()}"
    w64 = ref64.dwconv_first_t(xin, w, b, pad, dil)
    bound = ref64.dwconv_first_t_bound(xin, w, b, pad, dil)
    if ao is not None:
        assert np.all(np.abs(lin32.astype(np.float64) - w64) <= bound), what
        allowed = 2.0 * bound + snake_tol(lin32, ao)
        w64 = ref64.snake(w64, ao)
    else:
        allowed = bound
    err = np.abs(got.astype(np.float64) - w64)
    assert np.all(err <= allowed), f"{what}: {float((err / np.maximum(allowed, 1e-300)).max()):.3g} x the allowed error"
    return float((err / np.maximum(allowed, 1e-300)).max())


def _dw_case(rng, B, C, T, K, pad, dil, s_in, s_out, bias):
    """One hook call on seeded inputs, judged by dw_judge (which tests/test_activation_range_gpu.py calls with values of its own)."""
    x = _rand(rng, B, C, T, scale=1.5)
    w = _rand(rng, C, K, scale=1.0 / np.sqrt(K)); b = _rand(rng, C, scale=0.1) if bias else None
    ai = _alpha(rng, C) if s_in else None
    ao = _alpha(rng, C) if s_out else None
    got = ops.dwconv1d(x, w, b, pad, dil, alpha_in=ai, alpha_out=ao)
    what = f"B={B} C={C} T={T} K={K} pad={pad} dil={dil} snake_in={s_in} snake_out={s_out} bias={bias} [{dw_form(K, pad, dil, T)}]"
    _check_forms([dw_form(K, pad, dil, T)], what)
    return dw_judge(got, x, w, b, pad, dil, ai, ao, what)


@pytest.mark.parametrize("T", DW_T)
@pytest.mark.parametrize("dil", [1, 3, 9])
def test_dwconv_k7_tile_edges_and_short_clips(dil, T):
    """K = 7 with "same" padding at every Snake-in / Snake-out / bias combination.  T = 2044 .. 2052 puts the vector kernel's last group of
    4 on both sides of the 2048-output tile edge, 4098 and 6144 add whole tiles, T % 4 != 0 and T < 4 take the scalar kernel, and
    T <= 54 is a clip shorter than the dilation-9 halo."""
    rng = np.random.default_rng(1000 * dil + T)
    worst, n = 0.0, 0
    for C, B in itertools.product(DW_C, DW_B):
        for s_in, s_out, bias in itertools.product([False, True], repeat=3):
            worst = max(worst, _dw_case(rng, B, C, T, 7, 3 * dil, dil, s_in, s_out, bias)); n += 1
    _report("dwconv", cases=n, form=dw_form(7, 3 * dil, dil, T), T=T, dil=dil, worst_err_over_allowed=worst)


@pytest.mark.parametrize("K,pad,dil", DW_SCALAR_ONLY)
def test_dwconv_shapes_only_the_scalar_kernel_serves(K, pad, dil):
    rng = np.random.default_rng(100 * K + 10 * pad + dil)
    worst, n = 0.0, 0
    for T, C, B in itertools.product(DW_SCALAR_T, [3, 64], [1, 3]):
        assert dw_form(K, pad, dil, T) == "dwconv_kernel"
        for s_in, s_out, bias in ((False, False, True), (True, True, True), (True, False, False)):
            worst = max(worst, _dw_case(rng, B, C, T, K, pad, dil, s_in, s_out, bias)); n += 1
    _report("dwconv", cases=n, form="dwconv_kernel", K=K, pad=pad, dil=dil, worst_err_over_allowed=worst)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_C = [1, 64, 96, 768, 769, 1024, 1536, 4096]
LN_T = [1, 7, 8, 15, 16, 17, 87, 150]


def ln_form(C):
    """launch_layernorm_ct's rule: 16-wide tiles while [C][16] floats fit 48 KB (C <= 768), else 8-wide; NC_LN_TILE forces a width (0 = the
    per-column kernel); whatever was picked must fit 96 KB of LDS with its statistics, else the per-column kernel runs.  So a forced
    NC_LN_TILE=16 at C = 1024 does run layernorm_tile_kernel<16> (64.1 KB of dynamic LDS, opted in), at C = 1536 (96.1 KB) and 4096 it
    falls to layernorm_ct_kernel; C = 4096 takes the per-column kernel in every row (128 KB at tile 8)."""
    env = _env_int("NC_LN_TILE", -1)
    tt = env if env >= 0 else (16 if C * 16 * 4 <= 48 * 1024 else 8)
    if tt in (8, 16) and C * tt * 4 + 2 * tt * 4 <= 96 * 1024:
        return f"layernorm_tile_kernel<{tt}>"
    return "layernorm_ct_kernel"


@pytest.mark.parametrize("C", LN_C)
def test_layer_norm_channel_counts_and_ragged_tiles(C):
    """C = 768 / 769 is the switch from 16- to 8-wide tiles, C = 4096 must take the per-column kernel (none of the listed widths is
    refused); T not a multiple of the tile leaves a ragged last workgroup.  Inputs: standard normal, a large common offset (mean 100,
    spread 1), and constant columns (variance 0: the output is beta)."""
    rng = np.random.default_rng(C)
    worst, aten_worst, n = 0.0, 0.0, 0
    for T, B, kind in itertools.product(LN_T, [1, 3], ["normal", "offset", "constant"]):
        if kind == "normal":
            x = _rand(rng, B, C, T)
        elif kind == "offset":
            x = (100.0 + rng.standard_normal((B, C, T))).astype(np.float32)
        else:
            x = np.ascontiguousarray(np.broadcast_to(_rand(rng, B, 1, T, scale=3.0), (B, C, T)))
        g = _rand(rng, C, scale=0.5) + 1.0; be = _rand(rng, C, scale=0.3)
        what = f"C={C} T={T} B={B} {kind} [{ln_form(C)}]"
        want = c_oracle.layer_norm_ct(x, g, be)
        got = ops.layer_norm(x, g, be)
        _check_forms([ln_form(C)], what)
        assert np.array_equal(got, want), f"{what}: max abs diff {np.abs(got - want).max()}"
        w64, tol, aten_err = ref64.aten_tol(ref64.layer_norm_ct, M_ATEN_LN, x, g, be)
        err = float(np.abs(got.astype(np.float64) - w64).max())
        assert err <= tol, f"{what}: error {err:.3g}, ATen's own {aten_err:.3g}"
        if kind == "constant":
            assert np.array_equal(got, np.broadcast_to(be[None, :, None], got.shape)), what
        if aten_err > 0:
            worst = max(worst, err / aten_err)
        aten_worst = max(aten_worst, aten_err); n += 1
    _report("layer_norm", cases=n, form=ln_form(C), C=C, worst_err_over_aten_err=worst, aten_err=aten_worst)


# ---------------------------------------------------------------------------------------------------------------- attention
def attn_form(W, T):
    return "local_attn_mfma_kernel" if W == 32 and T % 4 == 0 and os.environ.get("NC_ATTN_NO_MFMA") != "1" else "local_attn_kernel"


def _attn_case(qkv, W, what):
    fr = c_oracle.rotary_inv_freq()
    want = c_oracle.local_attn(qkv, W, fr)
    got = ops.local_attn(qkv, W, fr)
    _check_forms([attn_form(W, qkv.shape[2])], what)
    assert np.array_equal(got, want), f"{what}: max abs diff {np.abs(got - want).max()}"
    w64, tol, aten_err = ref64.aten_tol(ref64.local_attn, M_ATEN_ATTN, qkv, W, fr)
    err = float(np.abs(got.astype(np.float64) - w64).max())
    assert err <= tol, f"{what}: error {err:.3g}, ATen's own {aten_err:.3g}"
    return err / aten_err if aten_err > 0 else 0.0


@pytest.mark.parametrize("W", [4, 8, 16, 32])
def test_local_attn_windows_heads_and_lengths(W):
    """Only W = 32 at 1024 / 1536 channels runs inside the models: here every window the kernels serve, 1 / 2 / 16 heads, 1 / 2 / 5 windows."""
    rng = np.random.default_rng(W)
    worst, n = 0.0, 0
    for C, nw, B in itertools.product([64, 128, 1024], [1, 2, 5], [1, 2]):
        T = nw * W
        qkv = _rand(rng, B, 3 * C, T)
        worst = max(worst, _attn_case(qkv, W, f"W={W} C={C} T={T} B={B} [{attn_form(W, T)}]")); n += 1
    _report("local_attn", cases=n, form=attn_form(W, W), W=W, worst_err_over_aten_err=worst)


@pytest.mark.parametrize("W", [4, 8, 16, 32])
def test_local_attn_saturated_and_flat_softmax(W):
    rng = np.random.default_rng(50 + W)
    B, C, T = 2, 128, 2 * W
    qkv = _rand(rng, B, 3 * C, T)
    qkv[:, :2 * C] *= 6.0                                   # q and k: scores of standard deviation 36
    s = ref64.attn_scores(qkv, W)
    assert s.max() >= 30.0 and s.min() <= -30.0             # softmax saturates: exp(s - max) underflows for most keys
    r_sat = _attn_case(qkv, W, f"W={W} saturated")
    qkv = _rand(rng, B, 3 * C, T)
    qkv[:, :C] = 0.0                                        # q == 0: every score is equal, the output is the mean of v over the window
    assert np.all(ref64.attn_scores(qkv, W) == 0.0)
    r_flat = _attn_case(qkv, W, f"W={W} flat")
    _report("local_attn", cases=2, form=attn_form(W, T), W=W, worst_err_over_aten_err=max(r_sat, r_flat), inputs="saturated+flat")


def test_local_attn_refuses_what_it_does_not_serve():
    qkv = np.zeros((1, 192, 64), np.float32)
    for W in (33, 64, 5):                                   # above the 32-step window; 64 % 5 != 0
        with pytest.raises(_lib.NcError, match="status 6"):
            ops.local_attn(qkv, W, c_oracle.rotary_inv_freq())
    with pytest.raises(_lib.NcError, match="status 6"):
        ops.local_attn(np.zeros((1, 96, 32), np.float32), 32, c_oracle.rotary_inv_freq())    # 32 channels: not whole heads of 64
    _check_forms([], "refused calls launch nothing")


# ---------------------------------------------------------------------------------------------------------------- average pool
@pytest.mark.parametrize("s", [2, 4, 8])
def test_avg_pool_strides_and_ragged_lengths(s):
    rng = np.random.default_rng(s)
    worst, n = 0.0, 0
    for rows, T in itertools.product([1, 257], [s, 8 * s, 8 * s + 1, 9 * s - 1, 1000, 1003]):
        x = _rand(rng, rows, T)
        want = c_oracle.avg_pool(x, s)
        got = ops.avg_pool(x, s)
        assert got.shape == (rows, T // s)
        assert np.array_equal(got, want), f"s={s} rows={rows} T={T}"
        err = np.abs(got.astype(np.float64) - ref64.avg_pool(x, s))
        bound = ref64.avg_pool_bound(x, s)
        assert np.all(err <= bound), f"s={s} rows={rows} T={T}"
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max())); n += 1
    _report("avg_pool", cases=n, form="avg_pool_kernel", s=s, worst_err_over_allowed=worst)


# ---------------------------------------------------------------------------------------------------------------- SNAC unit
def _unit_inputs(rng, B, C, T, with_b1, with_next, x=None, a1=None):
    """Seeded inputs of one unit; x, a1: values to use in place of the drawn ones (tests/test_activation_range_gpu.py, which chooses a2
    and the next unit's alpha from the oracle's results afterwards; the draws are made all the same)."""
    xd = _rand(rng, B, C, T, scale=1.5)
    a1d, a2d = _alpha(rng, C), _alpha(rng, C)
    w7 = _rand(rng, C, 7, scale=1.0 / np.sqrt(7)); b7 = _rand(rng, C, scale=0.1)
    w1 = _rand(rng, C, C, scale=1.0 / np.sqrt(C)); b1 = _rand(rng, C, scale=0.1) if with_b1 else None
    and_ = _alpha(rng, C) if with_next else None
    pick = lambda given, drawn: drawn if given is None else given
    return pick(x, xd), w7, b7, pick(a1, a1d), a2d, w1, b1, and_


def _unit_oracle(x, w7, b7, a1, a2, w1, b1, an, dil):
    C = x.shape[1]
    h = c_oracle.snake(c_oracle.conv1d(c_oracle.snake(x, a1), w7.reshape(C, 1, 7), b7, 1, 3 * dil, dil, groups=C), a2)
    sp1 = spec(h, w1.reshape(C, C, 1), b1, residual=x, alpha_out=an)      # the pointwise half, on the oracle's depthwise result
    return oracle_conv(sp1), sp1


@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("C", [64, 96])
def test_snac_unit_fused_equals_unfused_equals_oracle(C, dil):
    """The one-launch unit runs only from 65 536 columns inside a model; the hook runs it wherever usable() allows: T = 256 (one tile), 260 and
    2052 (a last tile of 4 columns), 5000 (19.5 tiles), one clip and three, with and without the next unit's Snake and the pointwise bias.
    The depthwise half is judged in the tests above; here the binary64 bound is on the unit's output (pointwise chain + bias + skip, Snake)."""
    rng = np.random.default_rng(10 * C + dil)
    worst, n = 0.0, 0
    for T, B, with_b1, with_next in itertools.product([256, 260, 2048, 2052, 5000], [1, 3], [False, True], [False, True]):
        x, w7, b7, a1, a2, w1, b1, an = _unit_inputs(rng, B, C, T, with_b1, with_next)
        want, sp1 = _unit_oracle(x, w7, b7, a1, a2, w1, b1, an, dil)
        what = f"C={C} dil={dil} T={T} B={B} b1={with_b1} next={with_next}"
        y_f = ops.snac_unit(x, w7, b7, a1, a2, w1, b1, an, dil=dil, fused=True)
        _check_forms([f"snac_unit_kernel<{C // 32},{dil},{int(with_next)}>"], what)
        y_u = ops.snac_unit(x, w7, b7, a1, a2, w1, b1, an, dil=dil, fused=False)
        _check_forms([dw_form(7, 3 * dil, dil, T)], what + ", two launches")      # (+ the pointwise convolution, logged as conv_mfma)
        assert np.array_equal(y_u, want), f"{what}, two launches: max abs diff {np.abs(y_u - want).max()}"
        assert np.array_equal(y_f, want), f"{what}, one launch: max abs diff {np.abs(y_f - want).max()}"
        worst = max(worst, judge_conv(y_f, sp1, what)); n += 1
    _report("snac_unit", cases=n, form=f"snac_unit_kernel<{C // 32},{dil},*> + two-launch path", worst_err_over_allowed=worst)


@pytest.mark.parametrize("C,T", [(48, 512), (64, 255), (64, 258)])
def test_snac_unit_refuses_instead_of_falling_back(C, T):
    """No one-launch kernel for 48 channels, for T < 256 or for T % 4 != 0: fused = 1 says so (NC_EUNSUPPORTED), fused = 0 computes the unit."""
    rng = np.random.default_rng(C + T)
    x, w7, b7, a1, a2, w1, b1, an = _unit_inputs(rng, 2, C, T, True, True)
    with pytest.raises(_lib.NcError, match="status 6"):
        ops.snac_unit(x, w7, b7, a1, a2, w1, b1, an, dil=3, fused=True)
    want, sp1 = _unit_oracle(x, w7, b7, a1, a2, w1, b1, an, 3)
    _check_forms([], "a refused call launches nothing")
    y_u = ops.snac_unit(x, w7, b7, a1, a2, w1, b1, an, dil=3, fused=False)
    _check_forms([dw_form(7, 9, 3, T)])
    assert np.array_equal(y_u, want)
    judge_conv(y_u, sp1, f"C={C} T={T}")


# ---------------------------------------------------------------------------------------------------------------- the other forms
DW_FORMS = {"dwconv_kernel", "dwconv_vec_kernel<1>", "dwconv_vec_kernel<3>", "dwconv_vec_kernel<9>"}
LN_FORMS = {"layernorm_tile_kernel<16>", "layernorm_tile_kernel<8>", "layernorm_ct_kernel"}
ATTN_FORMS = {"local_attn_kernel", "local_attn_mfma_kernel"}
VARIANT_ROWS = [   # (switches, the tests they bear on, family, the forms of that family the row must reach -- and no other)
    ({}, None, "dwconv", DW_FORMS),
    ({}, None, "layer_norm", LN_FORMS),
    ({}, None, "local_attn", ATTN_FORMS),
    ({"NC_DW_NO_VEC": "1"}, "dwconv or snac_unit", "dwconv", {"dwconv_kernel"}),
    ({"NC_LN_TILE": "0"}, "layer_norm", "layer_norm", {"layernorm_ct_kernel"}),
    ({"NC_LN_TILE": "8"}, "layer_norm", "layer_norm", {"layernorm_tile_kernel<8>", "layernorm_ct_kernel"}),        # C = 4096: 128 KB
    ({"NC_LN_TILE": "16"}, "layer_norm", "layer_norm", {"layernorm_tile_kernel<16>", "layernorm_ct_kernel"}),      # C >= 1536: above 96 KB
    ({"NC_ATTN_NO_MFMA": "1"}, "local_attn", "local_attn", {"local_attn_kernel"}),
]


def test_every_form_of_the_launchers_is_observed_and_leaves_this_file_true(tmp_path):
    """The switches are read once per process, so each row is a fresh child: the default row runs this whole file, a switch row the tests of
    the kernel family it changes (they compare with the oracle: passing in every row is equality across the kernel forms).  Every child
    keeps the engine's launch log and asserts, case by case, that the kernel the launcher took is the one its rule names, so a switch
    without effect or a rule that drifted fails there; here the forms a row reached are held to the set it must reach.  One child after
    the other, each under its own timeout; the first child that does not exit 0 ends the test."""
    if os.environ.get("NC_ELEM_OPS_CHILD") == "1":
        return                                              # (a child does not start children)
    cache = {}
    for n, (row, keys, family, must) in enumerate(VARIANT_ROWS):
        tag = json.dumps([row, keys])
        if tag not in cache:
            e = dict(os.environ, NC_ELEM_OPS_CHILD="1", NC_LAUNCH_LOG=str(tmp_path / f"launch_{n}.log"), **row)
            cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)]
            r = subprocess.run(cmd + (["-k", keys] if keys else []), env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
            assert r.returncode == 0, (row, r.stdout[-3000:], r.stderr[-1500:])
            cache[tag] = [json.loads(ln[9:]) for ln in r.stdout.splitlines() if ln.startswith("OPREPORT ")]
        forms = {rep["form"] for rep in cache[tag] if rep["kernel"] == family}
        assert forms == must, (row, family, sorted(forms))
        _report("variants", row=row, family=family, forms=sorted(forms))
