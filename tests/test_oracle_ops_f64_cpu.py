"""CPU suite: the ORACLE's primitives against binary64 at every shape the GPU op tests use.

The GPU tests assert engine == oracle bit for bit; the oracle was written next to the kernels with the same fma chains, so that alone
proves agreement, not correctness.  Here c_oracle.conv1d / conv_transpose1d / snake / tanh / vq_argmin and the SNAC pieces are held to
tests/ref64.py at the case lists of tests/test_ops_gpu.py and tests/test_elem_ops_gpu.py themselves (imported, so a case added there is
judged here too): shapes equal, and |oracle - binary64| within the derived bound element by element.

Regenerate the activation tables with:  python tests/test_oracle_ops_f64_cpu.py --write-bounds
"""
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import op_judge  # noqa: E402
import ref64  # noqa: E402
import test_activation_range_gpu as A  # noqa: E402
import test_elem_ops_gpu as E  # noqa: E402   (imports open no GPU: the engine library is loaded on first use)
import test_ops_gpu as G  # noqa: E402
from op_judge import judge_conv, oracle_conv  # noqa: E402
from oracle import c_oracle  # noqa: E402


def _judge_oracle(sp):
    return judge_conv(oracle_conv(sp), sp, "oracle")


# ---- every convolution case of tests/test_ops_gpu.py ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CONV_CASES)
def test_oracle_conv1d_cases(case):
    _judge_oracle(G.case_conv1d(*case))


@pytest.mark.parametrize("case", G.TRANSPOSE_CASES)
def test_oracle_conv_transpose_cases(case):
    _judge_oracle(G.case_conv_transpose(*case))


@pytest.mark.parametrize("case", G.FLAT_CASES)
def test_oracle_flattened_cases(case):
    _judge_oracle(G.case_flattened(*case)[0])


@pytest.mark.parametrize("case", G.RANDOM_CASES)
def test_oracle_random_shape_cases(case):
    _judge_oracle(G.case_random(*case))


@pytest.mark.parametrize("case", G.STREAMING_CASES)
def test_oracle_streaming_cases_on_one_clip(case):
    """8 x 192 x 66 000: the binary64 reference runs on the last clip (clips are independent; the GPU test does the same)."""
    sp = G.case_streaming(*case)
    _judge_oracle(G.one_clip(sp, sp["x"].shape[0] - 1))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("with_snake", [False, True])
@pytest.mark.parametrize("case", G.EPI_SHAPES)
def test_oracle_epilogue_matrix_cases(case, with_snake, with_res):
    _judge_oracle(G.case_epilogue(*case, with_snake, with_res))


@pytest.mark.parametrize("case", G.TRANSPOSE_SHORT_CASES)
def test_oracle_transpose_short_row_cases(case):
    _judge_oracle(G.case_transpose_short(*case))


@pytest.mark.parametrize("case", G.SUBPIXEL_CASES)
def test_oracle_subpixel_any_stride_cases(case):
    """Strides 3, 5, 6, 7 with output_padding = 1 and with pad = 0: what test_conv_length_formulas_and_values never passes."""
    _judge_oracle(G.case_subpixel(*case))


@pytest.mark.parametrize("case", G.SMALL_CASES)
def test_oracle_short_row_strided_cases(case):
    _judge_oracle(G.case_small(*case))


@pytest.mark.parametrize("case", G.K16_WIDE_CASES)
def test_oracle_k16_wide_cases(case):
    _judge_oracle(G.case_k16_wide(*case))


@pytest.mark.parametrize("k,case", [(7, c) for c in G.K7_SHORT_CASES] + [(3, c) for c in G.K3_SHORT_CASES])
def test_oracle_short_row_stride1_cases(k, case):
    _judge_oracle(G.case_short_row_stride1(k, *case))


@pytest.mark.parametrize("case", G.POINTWISE_SHORT_CASES)
def test_oracle_pointwise_short_row_cases(case):
    _judge_oracle(G.case_pointwise_short(*case))


@pytest.mark.parametrize("case", G.RES_UNIT_CASES + [(96, 700, 3, 2)])
def test_oracle_residual_unit_cases(case):
    C, T, d, B = case
    sp7, sp1 = G.case_res_unit(C, T, d, B, seed=5 if case == (96, 700, 3, 2) else C + d)
    _judge_oracle(sp7)
    _judge_oracle(sp1)


def test_oracle_tanh_head_and_flattened_epilogue_cases():
    _judge_oracle(G.case_tanh_head())
    _judge_oracle(G.case_flattened_epilogues())


# ---- depthwise: c_oracle.conv1d(..., groups=C) at the shapes of tests/test_elem_ops_gpu.py -------------------------------------------
def _dw_oracle_case(rng, B, C, T, K, pad, dil):
    x = G._rand(rng, B, C, T, scale=1.5)
    w = G._rand(rng, C, K, scale=1.0 / np.sqrt(K)); b = G._rand(rng, C, scale=0.1)
    got = E.dw_oracle(x, w, b, pad, dil)
    err = np.abs(got.astype(np.float64) - ref64.dwconv_first_t(x, w, b, pad, dil))
    bound = ref64.dwconv_first_t_bound(x, w, b, pad, dil)
    assert got.shape == (B, C, T)
    assert np.all(err <= bound), f"B={B} C={C} T={T} K={K} pad={pad} dil={dil}: {float((err / np.maximum(bound, 1e-300)).max()):.3g} x bound"
    if 2 * pad == dil * (K - 1):      # "same" padding: the hook's definition is the whole convolution, as torch states it
        assert np.all(np.abs(got - ref64.conv1d(x, w.reshape(C, 1, K), b, 1, pad, dil, groups=C)) <= bound)


@pytest.mark.parametrize("dil", [1, 3, 9])
def test_oracle_depthwise_k7(dil):
    rng = np.random.default_rng(dil)
    for T, C, B in itertools.product(E.DW_T, E.DW_C, E.DW_B):
        _dw_oracle_case(rng, B, C, T, 7, 3 * dil, dil)


@pytest.mark.parametrize("K,pad,dil", E.DW_SCALAR_ONLY)
def test_oracle_depthwise_other_shapes(K, pad, dil):
    rng = np.random.default_rng(K + pad + dil)
    for T, C, B in itertools.product(E.DW_SCALAR_T, [3, 64], [1, 3]):
        _dw_oracle_case(rng, B, C, T, K, pad, dil)


# ---- Snake, tanh: the measured tables ------------------------------------------------------------------------------------------------
def test_snake_and_tanh_error_tables():
    """|alpha x| up to 1e4, alpha in {1e-3, 0.05, 1, 7.3, 50}, both signs, zero, denormal x.  The allowed error was measured against binary64
    on the CPU (per decade of |alpha x|, in ulp of the result) and is committed in tests/golden/op_error_bounds.json; the oracle is
    deterministic, so the assertion is that table times 1.5 -- the margin is for another libm's binary64 sin / tanh only (below 1 ulp of
    binary64: it cannot move a binary32 ulp count by more than rounding)."""
    tab = op_judge.tables()
    assert tab["decades"] == op_judge.DECADES
    snake, tanh = op_judge.measure_snake(), op_judge.measure_tanh()
    print("snake ulp per decade", snake.tolist())
    print("tanh  ulp per decade", tanh.tolist())
    assert np.all(snake <= op_judge.MARGIN * np.asarray(tab["snake_ulp"])), snake
    assert np.all(tanh <= op_judge.MARGIN * np.asarray(tab["tanh_ulp"])), tanh
    # alpha == 0 is the identity, exactly; zero and denormals pass through (sin^2 of a denormal underflows to 0)
    x = np.float32([[[-3.0, 0.0, 1e-45, 1e-40, 7.5]]])
    assert np.array_equal(c_oracle.snake(x, np.float32([0.0])), x)
    assert np.array_equal(c_oracle.snake(x[:, :, 1:4], np.float32([1.0])), x[:, :, 1:4])


# ---- the activation range: every case of tests/test_activation_range_gpu.py ------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.CONV_CASES))
def test_oracle_activation_range_conv_cases(name):
    """Wide alphas (1e-3 .. 50), |alpha x| in every decade up to 0.9e4, tanh in all three branches: the oracle within judge_conv, and the
    builder's own domain and coverage conditions (asserted when the case is built, and again here)."""
    sp = A.conv_case(name)
    A.assert_conditions(sp, name)
    print(name, "oracle error / allowed", _judge_oracle(sp))


@pytest.mark.parametrize("name", list(A.RES_UNIT_CASES))
def test_oracle_activation_range_residual_unit_cases(name):
    sp7, sp1 = A.res_unit_case(name)
    A.assert_conditions(sp7, name)
    print(name, "oracle error / allowed", _judge_oracle(sp7), _judge_oracle(sp1))


@pytest.mark.parametrize("dil,T,B", A.DW_CASES)
def test_oracle_activation_range_depthwise_cases(dil, T, B):
    x, w, b, ai, ao = A.dw_case(dil, T, B)
    A.snake_coverage(x, ai, "alpha_in", True)
    lin = E.dw_oracle(c_oracle.snake(x, ai), w, b, 3 * dil, dil)
    A.snake_coverage(lin, ao, "alpha_out", False)
    print("oracle error / allowed", E.dw_judge(c_oracle.snake(lin, ao), x, w, b, 3 * dil, dil, ai, ao, f"oracle, dil={dil} T={T} B={B}"))


@pytest.mark.parametrize("C,dil,T,with_next", A.UNIT_CASES)
def test_oracle_activation_range_snac_unit_cases(C, dil, T, with_next):
    x, w7, b7, a1, a2, w1, b1, an = A.unit_case(C, dil, T, with_next)
    A.snake_coverage(x, a1, "a1", True)
    lin7 = E.dw_oracle(c_oracle.snake(x, a1), w7, b7, 3 * dil, dil)
    A.snake_coverage(lin7, a2, "a2", False)
    E.dw_judge(c_oracle.snake(lin7, a2), x, w7, b7, 3 * dil, dil, a1, a2, "oracle, depthwise half")
    want, sp1 = E._unit_oracle(x, w7, b7, a1, a2, w1, b1, an, dil)
    if with_next:
        A.snake_coverage(op_judge.oracle_linear(sp1), an, "next", False)
    print("oracle error / allowed", judge_conv(want, sp1, "oracle"))


# ---- quantizers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.VQ_CASES)
def test_oracle_vq_argmin_is_the_binary64_argmin(case):
    z, cb = G.case_vq(*case)
    share, flips = G.judge_vq(c_oracle.vq_argmin(z, cb)[0], z, cb, "dac", "oracle")
    print(f"near-tie share {share:.4%}, frames that differ {flips}")


@pytest.mark.parametrize("case", G.EUCLID_CASES)
def test_oracle_euclid_rvq_stages_are_the_binary64_argmin(case):
    ze, books = G.case_euclid(*case)
    r = ze.copy()
    for q in range(books.shape[0]):
        idx = c_oracle.vq_argmin(r, books[q])[0]
        share, flips = G.judge_vq(idx, r, books[q], "euclid", f"oracle, stage {q}")
        print(f"stage {q}: near-tie share {share:.4%}, frames that differ {flips}")
        r = r - books[q][idx].transpose(0, 2, 1)


def test_oracle_rvq_stage_loop_is_refdac_encode_bit_for_bit():
    """rvq_judge.oracle_stages -- the stage loop the quantizer op tests compare the engine with, composed from c_oracle.conv1d and
    c_oracle.vq_argmin -- fed the oracle's own encoder output and the folded dac_small weights, gives RefDAC.encode's codes, latents and
    zq bit for bit."""
    import rvq_judge
    from conftest import dac_cfg_from_meta, load_golden
    from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob
    g = load_golden("dac_small")
    cfg = dac_cfg_from_meta(g["meta"])
    sd = dac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"])
    zq, codes, lat, ze = c_oracle.RefDAC(cfg, save_blob(sd)).encode(g["pcm"])
    fold = lambda p: c_oracle.fold_wn_dac(sd[p + ".weight_v"], sd[p + ".weight_g"])[:, :, 0]
    names = [f"quantizer.quantizers.{i}" for i in range(cfg.n_codebooks)]
    stages, c2, l2, z2 = rvq_judge.oracle_stages(
        ze, np.stack([fold(p + ".in_proj") for p in names]), np.stack([sd[p + ".in_proj.bias"] for p in names]),
        np.stack([sd[p + ".codebook.weight"] for p in names]), np.stack([fold(p + ".out_proj") for p in names]),
        np.stack([sd[p + ".out_proj.bias"] for p in names]))
    assert len(stages) == cfg.n_codebooks and codes.size > 0
    assert np.array_equal(c2, codes) and c2.dtype == codes.dtype
    assert np.array_equal(l2, lat) and np.array_equal(z2, zq)
    assert np.array_equal(stages[0]["r_in"], ze)


# ---- the SNAC pieces the oracle exports ------------------------------------------------------------------------------------------------
def test_oracle_layer_norm_attention_and_pooling_pieces():
    rng = np.random.default_rng(3)
    for C, T in ((64, 17), (769, 8), (1024, 87)):
        x = G._rand(rng, 2, C, T); g = G._rand(rng, C, scale=0.5) + 1.0; be = G._rand(rng, C, scale=0.3)
        w64, tol, _ = ref64.aten_tol(ref64.layer_norm_ct, E.M_ATEN_LN, x, g, be)
        assert np.abs(c_oracle.layer_norm_ct(x, g, be) - w64).max() <= tol
    fr = c_oracle.rotary_inv_freq()
    for W, C, T in ((4, 64, 8), (16, 128, 32), (32, 128, 64)):
        qkv = G._rand(rng, 2, 3 * C, T)
        w64, tol, _ = ref64.aten_tol(ref64.local_attn, E.M_ATEN_ATTN, qkv, W, fr)
        assert np.abs(c_oracle.local_attn(qkv, W, fr) - w64).max() <= tol
    for s, T in ((2, 9), (4, 1003), (8, 64)):
        x = G._rand(rng, 5, T)
        assert np.all(np.abs(c_oracle.avg_pool(x, s) - ref64.avg_pool(x, s)) <= ref64.avg_pool_bound(x, s))


def _write_bounds():
    tab = {"meta": {"generator": "python tests/test_oracle_ops_f64_cpu.py --write-bounds",
                    "what": "largest |C oracle - binary64| in ulp of the binary32 result, per decade of |alpha x| (snake) / |x| (tanh); "
                            "decade d covers [10^d, 10^(d+1)), the first also everything below, the last up to 1e4 inclusive",
                    "alphas": list(op_judge.ALPHAS),
                    "engine_error_over_aten_error_on_mi355x": {"layer_norm": None, "local_attn": None}},
           "decades": op_judge.DECADES,
           "snake_ulp": [round(float(v), 3) for v in op_judge.measure_snake()],
           "tanh_ulp": [round(float(v), 3) for v in op_judge.measure_tanh()]}
    if os.path.exists(op_judge.BOUNDS_PATH):
        with open(op_judge.BOUNDS_PATH) as f:
            old = json.load(f)
        tab["meta"]["engine_error_over_aten_error_on_mi355x"] = old["meta"]["engine_error_over_aten_error_on_mi355x"]
        if "encodec_layers" in old:                       # (recorded by tests/test_oracle_encodec_layers_f64_cpu.py --write-bounds)
            tab["encodec_layers"] = old["encodec_layers"]
    with open(op_judge.BOUNDS_PATH, "w") as f:
        json.dump(tab, f, indent=1)
        f.write("\n")
    print(json.dumps(tab, indent=1))


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-bounds"]:
        _write_bounds()
    else:
        sys.exit("usage: python tests/test_oracle_ops_f64_cpu.py --write-bounds")
