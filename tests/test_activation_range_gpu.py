"""GPU suite: the places where the engine writes a Snake or a tanh that an op hook can reach, at the arguments a checkpoint can hold
(SITES_NOT_REACHED below records the ones no hook reaches: among them the Snake on the output of DAC's one-launch residual unit).

The other op tests draw Gaussian inputs and alphas in [0.5, 2): there |alpha x| stays below ~12 and the tanh head below ~3.  Here the
shapes of tests/test_ops_gpu.py and tests/test_elem_ops_gpu.py are kept and only the VALUES change: alphas log-uniform in [1e-3, 50]
(every fifth 0), |alpha x| from denormal to 0.9e4 in every decade of op_judge.DECADES, pre-tanh values in all three branches of
nc_tanhf.  One case per kernel form that applies an activation (decided by reading the kernels: see FORMS_WITHOUT_ACTIVATION), each
with three judges: engine == oracle bit for bit, the engine within the existing binary64 bounds (op_judge.judge_conv: the committed
activation tables and MARGIN, unchanged), and the kernel form that launched (observed in a child that keeps the engine's launch log).

The case builders are module-level and open no GPU: tests/test_oracle_ops_f64_cpu.py holds the ORACLE to binary64 at exactly these cases
and re-asserts the builders' own conditions (domain and coverage, on the oracle's values alone).
"""
import functools
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import op_judge  # noqa: E402
import test_elem_ops_gpu as E  # noqa: E402   (imports open no GPU: the engine library is loaded on first use)
import test_ops_gpu as G  # noqa: E402
from neuralcodecs_amd import ops  # noqa: E402
from op_judge import DECADES, judge_conv, oracle_conv, oracle_linear, spec  # noqa: E402
from oracle import c_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_LO, A_HI = 1e-3, 50.0                           # the span of op_judge.ALPHAS: what a checkpoint can hold
U_TOP = 0.9e4                                     # largest |alpha x| drawn: snake_tol's domain ends at 1e4
TINY = float(np.finfo(np.float32).tiny)           # smallest normal
SPECIALS = np.float32([0.0, 1e-45, -1e-45, 1e-40, -1e-40])
MIN_SHARE, MIN_BRANCH = 0.01, 0.05                # coverage the builders assert: per decade of |alpha x|, per branch of tanh


# ---------------------------------------------------------------------------------------------------------------- values
def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def wide_alpha(rng, c, lo=A_LO):
    """Per channel log-uniform in [lo, 50], every fifth channel 0 (identity lanes), channels 1 and 2 pinned to the two ends."""
    a = _log_uniform(rng, lo, A_HI, c).astype(np.float32)
    a[::5] = 0.0
    if c >= 3:
        a[1], a[2] = lo, A_HI
    return a


def wide_x(rng, B, C, T, alpha, halo):
    """x with |alpha_c x| in a chosen decade: the column axis is cut into blocks longer than `halo` (64 columns, fewer where the clip is
    short: seven blocks per clip as long as the halo allows), block j of clip b gets decade DECADES[(b * step + j) % 7], so the
    magnitudes inside a receptive field are homogeneous (a small argument next to large ones vanishes below half an ulp of the sum, and
    bit equality stops seeing it), a clip of seven or more blocks holds every decade, shorter clips go on where the one before stopped,
    and the first and last blocks of neighbouring clips differ.  x = sign * u / alpha_c (sign * u where alpha_c == 0), u log-uniform in
    its decade, capped to [smallest normal, 0.9e4]; a few elements per clip are 0 and binary32 denormals."""
    nd = len(DECADES)
    blk = min(64, max(halo + 1, -(-T // nd)))
    nblk = -(-T // blk)
    step = nblk + 1 if (nblk + 1) % nd else nblk + 2
    dec = np.array([[DECADES[(b * step + j) % nd] for j in range(nblk)] for b in range(B)], np.float64)
    d_col = np.repeat(dec, blk, axis=1)[:, None, :T]
    u = np.clip(10.0 ** (d_col + rng.random((B, C, T))), TINY, U_TOP)
    sign = rng.choice([-1.0, 1.0], (B, C, T))
    a = np.asarray(alpha, np.float64)[None, :, None]
    x = np.ascontiguousarray((sign * u / np.where(a == 0.0, 1.0, a)).astype(np.float32))
    for b in range(B):
        idx = rng.choice(C * T, 2 * len(SPECIALS), replace=False)
        x[b].reshape(-1)[idx] = np.tile(SPECIALS, 2)
    return x


def wide_alpha_out(rng, lin):
    """alpha_out for the oracle's linear result `lin` [B,C,T]: log-uniform in [1e-3, 50], every fifth 0, channels 1 and 2 at the two ends
    (as wide_alpha), then capped per channel at 0.9e4 / max|lin_c| so that |alpha y| stays inside snake_tol's domain."""
    a = wide_alpha(rng, lin.shape[1]).astype(np.float64)
    peak = np.abs(lin.astype(np.float64)).max(axis=(0, 2))
    return np.minimum(a, U_TOP / np.maximum(peak, 1e-30)).astype(np.float32)


def _shares(ax):
    d = op_judge._decade(ax)
    return np.bincount(d.ravel(), minlength=len(DECADES)) / d.size


def snake_coverage(v, alpha, what, every_decade):
    """The builders' condition on a Snake argument, on the oracle's values alone: |alpha v| <= 1e4 everywhere (snake_tol's domain), and of
    the elements of the alpha != 0 channels at least 1 % in every decade (an input activation) or in the top decade [1e3, 1e4) and in the
    bottom one (an output activation, whose values the convolution decides)."""
    nz = np.asarray(alpha) != 0.0
    ax = np.abs(np.asarray(alpha, np.float64)[None, nz, None] * np.asarray(v, np.float64)[:, nz, :])
    assert ax.max() <= 1e4, f"{what}: |alpha x| reaches {ax.max():.6g}"
    sh = _shares(ax)
    need = sh if every_decade else sh[[0, -1]]
    assert need.min() >= MIN_SHARE, f"{what}: share of the elements per decade of |alpha x| {np.round(sh, 4).tolist()}"
    return sh


def tanh_coverage(v, what):
    """At least 5 % of the pre-tanh values in each branch of nc_tanhf: polynomial (< 0.55), exponential, saturated (> 9); all within the
    measured domain of the tanh table."""
    a = np.abs(np.asarray(v, np.float64))
    assert a.max() <= 1e4, what
    sh = np.array([(a < 0.55).mean(), ((a >= 0.55) & (a <= 9.0)).mean(), (a > 9.0).mean()])
    assert sh.min() >= MIN_BRANCH, f"{what}: share of the outputs per tanh branch {np.round(sh, 4).tolist()}"
    return sh


def assert_conditions(sp, what=""):
    """Domain and coverage of a built case (sp["wide"]: which of its activations are wide), before any engine call."""
    wide = sp["wide"]
    if "in" in wide:
        snake_coverage(sp["x"], sp["alpha_in"], what + " alpha_in", True)
    if "out" in wide:
        snake_coverage(oracle_linear(sp), sp["alpha_out"], what + " alpha_out", False)
    if "tanh" in wide:
        lin = oracle_linear(sp)
        tanh_coverage(c_oracle.snake(lin, sp["alpha_out"]) if sp["alpha_out"] is not None else lin, what + " tanh")


def _halo(sp):
    K = sp["w"].shape[2]
    return -(-K // sp["stride"]) - 1 if sp["transposed"] else sp["dil"] * (K - 1)


def widen(sp, seed, w_in=False, w_out=False, w_tanh=False, a_lo=A_LO):
    """A case of the other op tests with the same shapes, weights and bias and other values.
    w_in: wide alpha_in, wide x, and the weights of input channel c times alpha_c -- x_c is u / alpha_c, so every channel then adds
          terms of the same size to a sum, and an error in any one of them shows in the bits.
    w_out: wide alpha_out, chosen post hoc from the oracle's linear result; without w_in the input stays Gaussian and w, b (and the
          residual) are scaled so that the largest |y| is 200.  With w_in the linear result peaks near the largest |u| (~1e4), so the cap
          0.9e4 / max|y_c| pulls nearly every alpha_out down to order 1 or below, the pinned 50 included: LARGE output alphas (a small
          reciprocal) are exercised by the w_out-only cases alone.
    w_tanh: w and b scaled post hoc so that the pre-tanh values span the three branches (Gaussian input: standard deviation 6; wide input:
          the largest at 0.9e4, the decades of the input do the rest)."""
    rng = np.random.default_rng(seed)
    sp = dict(sp, wide=[k for k, on in (("in", w_in), ("out", w_out), ("tanh", w_tanh)) if on])
    scale = lambda s: sp.update(w=(sp["w"] * np.float32(s)), b=None if sp["b"] is None else sp["b"] * np.float32(s),
                                residual=None if sp["residual"] is None else sp["residual"] * np.float32(s))
    if w_in:
        B, C, T = sp["x"].shape
        a = wide_alpha(rng, C, a_lo)
        g = np.where(a == 0.0, np.float32(1.0), a)
        sp.update(alpha_in=a, x=wide_x(rng, B, C, T, a, _halo(sp)), w=sp["w"] * (g[:, None, None] if sp["transposed"] else g[None, :, None]))
    if w_out:
        sp["alpha_out"] = None
        if not w_in:
            scale(200.0 / np.abs(oracle_linear(sp)).max())
        sp["alpha_out"] = wide_alpha_out(rng, oracle_linear(sp))
    if w_tanh:
        lin = oracle_linear(sp).astype(np.float64)
        scale(min(1.0, U_TOP / np.abs(lin).max()) if w_in else 6.0 / lin.std())
    return sp


def negated(sp):
    """The same case with every alpha negated (Snake1d places no sign constraint on alpha)."""
    neg = lambda a: None if a is None else -a
    return dict(sp, alpha_in=neg(sp["alpha_in"]), alpha_out=neg(sp["alpha_out"]), wide=[])


# ---------------------------------------------------------------------------------------------------------------- convolution cases
# Forms of test_conv_plan_gpu.TEMPLATE_FORMS | SPECIAL_FORMS without a case here, by reading their kernels:
#   skinny, thin_inm, k3_stream   apply no Snake and no tanh (launch_conv declines them when alpha_in / alpha_out is set; thin_inm's only
#                                 activation is the ELU of the Encodec input mode)
#   in2, in2_sub                  instances of the template, so they carry its epilogue code -- but they launch only for a second operand
#                                 (ConvIO::x2), which no hook passes and which the Encodec models never combine with a Snake: an open point
# Two forms no existing case list reaches:
#   slim                          k = 3 template instances for Cout <= 64 over >= 1024 columns: SLIM_SHAPE below, the smallest that does
#   sub                           the power-of-two sub-pixel form launches as dist_sub (grids up to 768 workgroups) or sub_narrow (short
#                                 rows) at every small shape; a second child with NC_NO_DIST_SMALL=1 (VARIANT_ROWS) runs the dist_sub and
#                                 dist cases as `sub` and `plain`
# The pointwise kernel has no separate long-row ("streaming") instance any more: launch_conv1x1 has one tile map for every length, so
# G.STREAMING_CASES add no form to the pointwise cases below.
FORMS_WITHOUT_ACTIVATION = {"skinny", "thin_inm", "k3_stream"}
FORMS_NOT_REACHED = {"in2", "in2_sub"}
# Activation code inside forms that ARE reached, which no hook can drive (open points, as the one in test_encodec_layers_gpu.py):
SITES_NOT_REACHED = {
    # The fused residual-unit instances (fused, fusedw, xv_fused) apply a second Snake, that of the unit's consumer, to the unit's output y:
    # ConvArgs::alpha_out2 (nc_conv_kernel.hip.h: loaded into Ep[4 BM .. 6 BM), applied through store_rows / emit_rows_quad at the end of
    # the fused tail).  The DAC model sets it on every one-launch unit (nc_dac.hip: io.alpha_out2 = alpha_next); nc_op_res_unit has no such
    # argument, so test_res_unit_activation_range drives the tail's a2 Snake on the accumulators but never the Snake on y, at any alpha.
    # ops.res_unit needs an `alpha_next` argument (as ops.snac_unit has) before a test can cover it.
    "alpha_out2": ("fused", "fusedw", "xv_fused"),
}
SLIM_SHAPE = (32, 32, 3, 1, 1, 1, 1024, 1)         # (Cin, Cout, K, stride, pad, dil, T, B) as in G.CONV_CASES
WITHOUT_DIST = {"dist_sub": "sub", "dist": "plain"}   # the form of a case under NC_NO_DIST_SMALL=1


def form_of(name):
    form = CONV_CASES[name][0]
    return WITHOUT_DIST.get(form, form) if os.environ.get("NC_NO_DIST_SMALL") == "1" else form


def _k16_wide_two_clips():
    cin, cout, T, _ = G.K16_WIDE_CASES[0]
    return G.case_k16_wide(cin, cout, T, 2)


def _k7_short_one_clip():
    cin, cout, T, _, snake_out = G.K7_SHORT_CASES[2]
    return G.case_short_row_stride1(7, cin, cout, T, 1, snake_out)


def _with_tanh(sp):
    return dict(sp, tanh_out=True)


CONV_CASES = {
    # name: (form, base case of the other op tests, what is widened)
    # -- the template: stagers (alpha_in) and both epilogues (alpha_out; full tiles run store_rows, partial tiles the quad emitter)
    "plain":            ("plain", lambda: G.case_conv1d(*G.CONV_CASES[1]), dict(w_in=True, w_out=True)),       # 777 columns x 2 clips
    "plain_one_clip":   ("plain", lambda: G.case_conv1d(*G.CONV_CASES[2]), dict(w_in=True, w_out=True)),       # 640 = 2.5 tiles, TM = 3
    "plain_out_res":    ("plain", lambda: G.case_epilogue(*G.EPI_SHAPES[1], True, True), dict(w_out=True)),    # 600 = 2 full tiles + 88
    "narrow_out":       ("narrow", lambda: G.case_epilogue(*G.EPI_SHAPES[3], True, False), dict(w_out=True)),
    "narrow_in":        ("narrow", lambda: G.case_flattened(*G.FLAT_CASES[0])[0], dict(w_in=True)),
    "flattened":        ("plain", G.case_flattened_epilogues, dict(w_in=True, w_out=True)),
    "dist_sub":         ("dist_sub", lambda: G.case_conv_transpose(*G.TRANSPOSE_CASES[0]), dict(w_in=True)),   # scalar Snake per staged item
    "sub_narrow":       ("sub_narrow", lambda: G.case_conv_transpose(*G.TRANSPOSE_CASES[2]), dict(w_in=True)),
    "subg":             ("subg", lambda: G.case_subpixel(*G.SUBPIXEL_CASES[0]), dict(w_in=True, w_out=True)),
    "dist":             ("dist", lambda: G.case_conv1d(*G.EXTRA_CONV1D[1]), dict(w_in=True, w_out=True)),
    "slim":             ("slim", lambda: G.case_conv1d(*SLIM_SHAPE), dict(w_in=True, w_out=True)),
    "xv_one_tile":      ("xv", lambda: G.case_xv_epilogue(256, True, True, False), dict(w_in=True, w_out=True)),
    "xv":               ("xv", lambda: G.case_xv_epilogue(592, True, True, True), dict(w_in=True, w_out=True)),
    "xv_sub":           ("xv_sub", lambda: G.case_subpixel(5472, 48, 2, 1, 592, 1, True), dict(w_out=True)),   # (the two-tap XV forms take
    "xv_subg":          ("xv_subg", lambda: G.case_subpixel(5472, 32, 3, 2, 592, 1, True), dict(w_out=True)),  #  no alpha_in: xv_two_tap_layer)
    # -- the pointwise kernel: full row tiles (line 280) with and without the residual, edge columns, a row-partial tile (line 327)
    "pointwise":        ("pointwise", lambda: G.case_epilogue(*G.EPI_SHAPES[4], True, False), dict(w_out=True)),
    "pointwise_res":    ("pointwise", lambda: G.case_epilogue(*G.EPI_SHAPES[5], True, True), dict(w_out=True)),
    "pointwise_rows":   ("pointwise", lambda: G.case_epilogue(*G.EPI_SHAPES[6], True, True), dict(w_out=True)),
    # -- the short-row kernel (per-element reciprocal), the stem
    "small_k16":        ("small", _k16_wide_two_clips, dict(w_out=True)),
    "small_k7":         ("small", _k7_short_one_clip, dict(w_out=True)),
    "stem":             ("stem", lambda: G.case_conv1d(*G.CONV_CASES[0]), dict(w_out=True)),
    # -- tanh: the thin head, and the template's head epilogue behind a wide Snake on the input
    "thin_tanh":        ("thin", lambda: _with_tanh(G.case_conv1d(*G.CONV_CASES[13])), dict(w_tanh=True)),
    "template_tanh":    ("plain", G.case_tanh_head, dict(w_in=True, w_tanh=True)),
}


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """The built case (cached: the tests and the CPU mirror share it, and nobody writes to it); its conditions hold or this raises."""
    _, base, kw = CONV_CASES[name]
    sp = widen(base(), seed=zlib.crc32(name.encode()), **kw)
    assert_conditions(sp, name)
    return sp


# ---------------------------------------------------------------------------------------------------------------- residual units
# fused: 700 columns = 2 tiles of 256 + 188; xv_fused: one full tile, and 592 = 2 + a partial one; fusedw (128-column tiles): 300 = 2 + 44.
# G.RES_UNIT_CASES' (192, 131, 9, 1) runs with 7 clips: 131 columns hold two blocks longer than the dilation-9 halo and a rest, so one clip
# cannot give every decade of |alpha x| a block of its own; over seven clips the decades go round, as in the T = 55 depthwise cases.
RES_UNIT_CASES = {"fused": (64, 700, 1, 2), "xv_fused_one_tile": (64, 256, 1, 1), "xv_fused": (64, 592, 1, 1), "fusedw": (192, 300, 1, 2),
                  "fusedw_d9": (192, 131, 9, 7)}
RES_UNIT_FORMS = {"fused": "fused", "xv_fused_one_tile": "xv_fused", "xv_fused": "xv_fused", "fusedw": "fusedw", "fusedw_d9": "fusedw"}
# (NC_NO_WIDE_FUSE / NC_NO_TILE_ALTS: the whole-channel tile of the wide units is not packed; their one-launch call is then left out)
WIDE_FUSE_OFF = any(os.environ.get(k) == "1" for k in ("NC_NO_WIDE_FUSE", "NC_NO_TILE_ALTS"))


@functools.lru_cache(maxsize=None)
def res_unit_case(name):
    """(sp7, sp1) as G.case_res_unit gives them: a1 wide, a2 post hoc from the oracle's k = 7 linear result."""
    C, T, d, B = RES_UNIT_CASES[name]
    sp7, sp1 = G.case_res_unit(C, T, d, B, seed=C + d)
    sp7 = widen(sp7, seed=zlib.crc32(name.encode()), w_in=True, w_out=True)
    assert_conditions(sp7, name)
    sp1 = dict(spec(oracle_conv(sp7), sp1["w"], sp1["b"], residual=sp7["x"]), wide=[])
    return sp7, sp1


# ---------------------------------------------------------------------------------------------------------------- depthwise, SNAC unit
# dwconv_kernel: T = 55 (not a multiple of 4); dwconv_vec_kernel<dil>: 2048 (whole tiles) and 2052 (a last group of 4).  T = 55 takes 7
# clips: at dilation 9 a clip is one block, and the decades go round over the clips.
DW_CASES = [(dil, T, 7 if T == 55 else 1) for dil in (1, 3, 9) for T in (55, 2048, 2052)]
DW_C = 64


@functools.lru_cache(maxsize=None)
def dw_case(dil, T, B):
    """(x, w, b, alpha_in, alpha_out): wide alpha_in and x, w of channel c times alpha_c, alpha_out post hoc from the oracle's taps."""
    rng = np.random.default_rng(7000 + 10 * T + dil)
    ai = wide_alpha(rng, DW_C)
    x = wide_x(rng, B, DW_C, T, ai, 6 * dil)
    w = E._rand(rng, DW_C, 7, scale=1.0 / np.sqrt(7)) * np.where(ai == 0.0, np.float32(1.0), ai)[:, None]
    b = E._rand(rng, DW_C, scale=0.1)
    lin = E.dw_oracle(c_oracle.snake(x, ai), w, b, 3 * dil, dil)
    ao = wide_alpha_out(rng, lin)
    snake_coverage(x, ai, f"dw {dil} {T} alpha_in", True)
    snake_coverage(lin, ao, f"dw {dil} {T} alpha_out", False)
    return x, w, b, ai, ao


# every instance snac_unit_kernel<C / 32, dil, next> at one full tile (256) and with a last tile of 4 columns (260)
UNIT_CASES = [(C, dil, T, nxt) for C in (64, 96) for dil in (1, 3, 9) for T in (256, 260) for nxt in (False, True)]


@functools.lru_cache(maxsize=None)
def unit_case(C, dil, T, with_next):
    """E._unit_inputs with x and a1 wide, w7 of channel c times a1_c, a2 post hoc from the oracle's depthwise taps and the next unit's
    alpha post hoc from the oracle's pointwise result.  Three clips: 256 / 260 columns are 4 / 5 blocks of 64 (d = 9: 55), the decades
    go round over the clips."""
    rng = np.random.default_rng(9000 + 100 * C + 10 * dil + 2 * (T - 256) + int(with_next))
    B = 3
    a1 = wide_alpha(rng, C)
    x = wide_x(rng, B, C, T, a1, 6 * dil)
    _, w7, b7, _, _, w1, b1, _ = E._unit_inputs(rng, B, C, T, True, with_next, x=x, a1=a1)
    w7 = w7 * np.where(a1 == 0.0, np.float32(1.0), a1)[:, None]
    lin7 = E.dw_oracle(c_oracle.snake(x, a1), w7, b7, 3 * dil, dil)
    a2 = wide_alpha_out(rng, lin7)
    snake_coverage(x, a1, f"unit {C} {dil} {T} a1", True)
    snake_coverage(lin7, a2, f"unit {C} {dil} {T} a2", False)
    an = None
    if with_next:
        _, sp1 = E._unit_oracle(x, w7, b7, a1, a2, w1, b1, None, dil)
        lin1 = oracle_linear(sp1)
        an = wide_alpha_out(rng, lin1)
        snake_coverage(lin1, an, f"unit {C} {dil} {T} next", False)
    return x, w7, b7, a1, a2, w1, b1, an


# ---------------------------------------------------------------------------------------------------------------- the launch log
# The form a launch took is OBSERVED in the child of test_every_activation_form_is_reached_as_the_form_it_names: it runs with NC_LAUNCH_LOG
# set from its first launch on (the engine opens the log once per process) and every case asserts the lines of its own launches.
_LOG = os.environ.get("NC_LAUNCH_LOG") if os.environ.get("NC_ACT_RANGE_CHILD") == "1" else None
_log_pos = 0


def _launched():
    """(conv_plan forms, elem kernels) the engine logged since the last call; (None, None) where no log is kept."""
    global _log_pos
    if _LOG is None:
        return None, None
    if not os.path.exists(_LOG):         # (the engine opens the log at its first launch)
        return [], []
    with open(_LOG) as f:
        f.seek(_log_pos)
        new = f.read().splitlines()
        _log_pos = f.tell()
    return [ln.split()[1] for ln in new if ln.startswith("conv_plan ")], [ln[5:] for ln in new if ln.startswith("elem ")]


def _report(kernel, **kw):
    print("\nOPREPORT " + json.dumps(dict(kernel=kernel, **kw), sort_keys=True))


def _bits(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} elements differ from the oracle, max abs diff {np.nanmax(np.abs(got - want))}"


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_activation_range(name):
    form = form_of(name)
    sp = conv_case(name)
    _launched()
    got = G._engine(sp)
    seen, _ = _launched()
    _bits(got, oracle_conv(sp), name)
    worst = judge_conv(got, sp, f"engine, {name}")
    assert seen is None or seen == [form], f"{name} is meant for the {form} form, launch_conv took {seen}"
    _report("conv", case=name, form=form, observed=seen is not None, worst_err_over_allowed=worst)


@pytest.mark.parametrize("name", list(RES_UNIT_CASES))
def test_res_unit_activation_range(name):
    """The unit in one launch (the fused tail's Snake on the accumulators) and in two (template k = 7 with both Snakes, then 1x1 + skip)."""
    one_launch = not (RES_UNIT_CASES[name][0] >= 192 and WIDE_FUSE_OFF)
    form = RES_UNIT_FORMS[name]
    sp7, sp1 = res_unit_case(name)
    d = sp7["dil"]
    _launched()
    h = G._engine(sp7)
    y_u = ops.res_unit(sp7["x"], sp7["w"], sp7["b"], sp7["alpha_in"], sp7["alpha_out"], sp1["w"], sp1["b"], dil=d, fused=False)
    _launched()
    _bits(h, sp1["x"], f"{name}, k = 7")
    want = oracle_conv(sp1)
    _bits(y_u, want, f"{name}, two launches")
    worst = max(judge_conv(h, sp7, f"engine, {name}, k = 7"), judge_conv(y_u, sp1, f"engine, {name}, two launches"))
    if not one_launch:
        return
    y_f = ops.res_unit(sp7["x"], sp7["w"], sp7["b"], sp7["alpha_in"], sp7["alpha_out"], sp1["w"], sp1["b"], dil=d, fused=True)
    seen, _ = _launched()
    _bits(y_f, want, f"{name}, one launch")
    assert seen is None or seen == [form], f"{name} is meant for the {form} form, launch_conv took {seen}"
    _report("res_unit", case=name, form=form, observed=seen is not None, worst_err_over_allowed=worst)


@pytest.mark.parametrize("dil,T,B", DW_CASES)
def test_dwconv_activation_range(dil, T, B):
    x, w, b, ai, ao = dw_case(dil, T, B)
    form = E.dw_form(7, 3 * dil, dil, T)
    _launched()
    got = ops.dwconv1d(x, w, b, 3 * dil, dil, alpha_in=ai, alpha_out=ao)
    _, seen = _launched()
    what = f"dwconv dil={dil} T={T} B={B} [{form}]"
    worst = E.dw_judge(got, x, w, b, 3 * dil, dil, ai, ao, what)
    assert seen is None or seen == [form], f"{what}: the engine launched {seen}"
    _report("dwconv", case=[dil, T, B], form=form, observed=seen is not None, worst_err_over_allowed=worst)


@pytest.mark.parametrize("C,dil,T,with_next", UNIT_CASES)
def test_snac_unit_activation_range(C, dil, T, with_next):
    x, w7, b7, a1, a2, w1, b1, an = unit_case(C, dil, T, with_next)
    form = f"snac_unit_kernel<{C // 32},{dil},{int(with_next)}>"
    want, sp1 = E._unit_oracle(x, w7, b7, a1, a2, w1, b1, an, dil)
    _launched()
    y_f = ops.snac_unit(x, w7, b7, a1, a2, w1, b1, an, dil=dil, fused=True)
    _, seen = _launched()
    y_u = ops.snac_unit(x, w7, b7, a1, a2, w1, b1, an, dil=dil, fused=False)
    what = f"snac unit C={C} dil={dil} T={T} next={with_next}"
    _bits(y_u, want, what + ", two launches")
    _bits(y_f, want, what + ", one launch")
    worst = judge_conv(y_f, sp1, what)
    assert seen is None or seen == [form], f"{what}: the engine launched {seen}"
    _report("snac_unit", case=[C, dil, T, with_next], form=form, observed=seen is not None, worst_err_over_allowed=worst)


NEGATED = ["plain", "pointwise"]      # a template stager (and its epilogue), the pointwise epilogue; dwconv_vec_kernel<3> below


def test_negative_alpha_equals_the_oracle():
    """Snake1d places no sign constraint on alpha: alpha_in and alpha_out negated, engine == oracle bit for bit.  There is no binary64
    judgement here on purpose: with alpha < 0, x + sin^2(alpha x) / alpha subtracts, the result cancels, and a tolerance in ulps of
    the result (what the activation table is in) means nothing.  (Alphas below the smallest normal, whose reciprocal overflows, are out
    of scope.)"""
    forms = []
    for name in NEGATED:
        sp = negated(conv_case(name))
        _launched()
        got = G._engine(sp)
        seen, _ = _launched()
        _bits(got, oracle_conv(sp), f"{name}, alphas negated")
        assert seen is None or seen == [form_of(name)], (name, seen)
        forms.append(form_of(name))
    dil, T, B = 3, 2052, 1
    x, w, b, ai, ao = dw_case(dil, T, B)
    want = c_oracle.snake(E.dw_oracle(c_oracle.snake(x, -ai), w, b, 3 * dil, dil), -ao)
    _launched()
    got = ops.dwconv1d(x, w, b, 3 * dil, dil, alpha_in=-ai, alpha_out=-ao)
    _, seen = _launched()
    _bits(got, want, "dwconv_vec, alphas negated")
    assert seen is None or seen == [E.dw_form(7, 3 * dil, dil, T)], seen
    _report("negative_alpha", forms=forms + [E.dw_form(7, 3 * dil, dil, T)], observed=seen is not None)


# what the child must report: every form of launch_conv and every elementwise kernel that applies a Snake or a tanh
def expected_forms():
    conv = {v[0] for v in CONV_CASES.values()} | {f for f in RES_UNIT_FORMS.values() if not (f == "fusedw" and WIDE_FUSE_OFF)}
    elem = {E.dw_form(7, 3 * d, d, T) for d, T, _ in DW_CASES} | {f"snac_unit_kernel<{C // 32},{d},{int(n)}>" for C, d, _, n in UNIT_CASES}
    return conv, elem


VARIANT_ROWS = [({}, None), ({"NC_NO_DIST_SMALL": "1"}, "dist")]      # (switches, the cases they bear on)


def test_every_activation_form_is_reached_as_the_form_it_names(tmp_path):
    """Fresh children that keep the launch log run the cases above again; there each asserts the form it launched as, so a planner change
    cannot silently turn them into tests of another instance.  The default row runs this whole file; the row without the distributed
    staging runs the dist_sub and dist cases as `sub` and `plain` (the switches are read once per process).  One child after the other,
    each under its own timeout; the first child that does not exit 0 ends the test.  Here: the forms the children observed are every
    form of launch_conv that carries activation code, but for the ones recorded above as out of the hooks' reach."""
    if os.environ.get("NC_ACT_RANGE_CHILD") == "1":
        return                                              # (a child does not start children)
    import test_conv_plan_gpu as P
    conv, elem = expected_forms()
    conv |= set(WITHOUT_DIST.values())
    assert conv | set(RES_UNIT_FORMS.values()) | FORMS_WITHOUT_ACTIVATION | FORMS_NOT_REACHED == P.TEMPLATE_FORMS | P.SPECIAL_FORMS
    reps = []
    for n, (row, keys) in enumerate(VARIANT_ROWS):
        e = dict(os.environ, NC_ACT_RANGE_CHILD="1", NC_LAUNCH_LOG=str(tmp_path / f"launch_{n}.log"), **row)
        cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)]
        r = subprocess.run(cmd + (["-k", keys] if keys else []), env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (row, r.stdout[-3000:], r.stderr[-1500:])
        reps += [json.loads(ln[9:]) for ln in r.stdout.splitlines() if ln.startswith("OPREPORT ")]
    assert reps and all(rep["observed"] for rep in reps)
    got_conv = {rep["form"] for rep in reps if rep["kernel"] in ("conv", "res_unit")}
    got_elem = {rep["form"] for rep in reps if rep["kernel"] in ("dwconv", "snac_unit")}
    assert got_conv == conv and got_elem == elem, (sorted(got_conv ^ conv), sorted(got_elem ^ elem))
    worst = max(rep["worst_err_over_allowed"] for rep in reps if "worst_err_over_allowed" in rep)
    _report("activation_range", forms=sorted(got_conv) + sorted(got_elem), cases=len(reps), not_reached=sorted(FORMS_NOT_REACHED),
            worst_err_over_allowed=worst)
