"""GPU suite: the quantizer kernels one at a time through their nc_op_* hooks.

nc_op_dac_rvq runs DacRvq::quantize, the routine DAC's encode calls, in both of its forms: form 1 is dac_rvq_fused_kernel (all stages in
one launch), form 0 the launches per stage (skinny in-projection, vq_argmin_kernel, the 1x1 convolution with the zq += q ; residual -= q
epilogue).  Judges as in the other op tests: the C oracle's stage loop (tests/rvq_judge.py, held to RefDAC.encode on the CPU) for bits and
binary64 (tests/ref64.py) for meaning, through bounds that are derived, never measured.  The cases cover every latent width and codebook
size the one-launch kernel admits, frame counts around its 16-frame workgroup, and clip boundaries inside a workgroup.
nc_op_rvq_update and nc_op_vq_gather are SNAC's update and gather kernels; both are exact operations, compared bit for bit.

Each test prints one `OPREPORT {...}` line (run with -s).  NC_RVQ_REPORT=<path> writes the table of all of them to <path>: that is how
tests/golden/rvq_op_report.json was recorded.  No test reads it.
"""
import itertools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rvq_judge as J  # noqa: E402
from neuralcodecs_amd import _lib, ops  # noqa: E402

D = J.D
_TABLE = []


def _report(kernel, **kw):
    _TABLE.append(dict(kernel=kernel, **kw))
    print("\nOPREPORT " + json.dumps(_TABLE[-1], sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_table():
    yield
    path = os.environ.get("NC_RVQ_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(what="largest error / allowed per case of tests/test_rvq_ops_gpu.py on an MI355X; bit-for-bit comparisons "
                                "report the number of compared values.  A record: no test reads it.", rows=_TABLE), f, indent=1, sort_keys=True)
            f.write("\n")


def _run(x, form, **over):
    a = dict(x, **over)
    return ops.dac_rvq(a["r"], a["w_in"], a["b_in"], a["cb"], a["w_out"], a["b_out"], form=form)


def _same(got, want, what, nan=False):
    for name, g, w in zip(("codes", "zq", "latents"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        ok = np.array_equal(g, w, equal_nan=True) if nan and name != "codes" else np.array_equal(g, w)
        assert ok, f"{what}: {name} differ in {int((g != w).sum())} of {g.size} values"


# ------------------------------------------------------------------------------------------- a. one launch == per stage == oracle
@pytest.mark.parametrize("case", J.CASES + [J.SHIPPED], ids=J.case_id)
def test_one_launch_form_equals_stagewise_form_and_oracle(case):
    x, (_, codes, lat, zq) = J.case(*case)
    want = (codes, zq, lat)
    fused, stagewise = _run(x, 1), _run(x, 0)
    _same(fused, want, "one launch vs oracle")
    _same(stagewise, want, "per stage vs oracle")
    _report("dac_rvq", group="a", case=J.case_id(case), compared=int(codes.size + lat.size + zq.size), mismatches=0)


# ---------------------------------------------------------------------------------------- b. binary64, stage by stage
@pytest.mark.parametrize("case", J.CASES + [J.SHIPPED], ids=J.case_id)
def test_each_stage_against_binary64_on_the_oracles_stage_input(case):
    """Stage i alone (n_q = 1) on the ORACLE's input of that stage, so that one stage's rounding is not multiplied through the next:
    latents are z_e, codes the choice, and zq = 0 + q is q exactly.  z_e and q within the bound of their chains (ref64.conv1d_bound),
    the choice by rvq_judge.judge_choice."""
    x, (stages, _, _, _) = J.case(*case)
    worst = dict(z_e=0.0, choice=0.0, q=0.0)
    differ = 0
    for i, sg in enumerate(stages):
        one = {k: x[k][i:i + 1] for k in ("w_in", "b_in", "cb", "w_out", "b_out")}
        for form in (1, 0):
            what = f"{J.case_id(case)} stage {i} form {form}"
            idx, q, z_e = _run(one, form, r=sg["r_in"])
            idx = idx[:, 0]
            worst["z_e"] = max(worst["z_e"], J.judge_projection(z_e, sg["r_in"], x["w_in"][i], x["b_in"][i], what + " z_e"))
            # the choice is judged on the z_e the kernel chose from; the straight-through value the out-projection saw is the oracle's,
            # which group a holds the engine to
            assert np.array_equal(z_e, sg["z_e"]) and np.array_equal(idx, sg["idx"]), what
            worst["q"] = max(worst["q"], J.judge_projection(q, sg["st"], x["w_out"][i], x["b_out"][i], what + " q"))
        w, d = J.judge_choice(idx, z_e, x["cb"][i], f"{J.case_id(case)} stage {i}")
        worst["choice"] = max(worst["choice"], w)
        differ += d
    _report("dac_rvq", group="b", case=J.case_id(case), worst_err_over_allowed=worst, frames_off_the_binary64_argmin=differ,
            frames=int(len(stages) * stages[0]["idx"].size))


# ------------------------------------------------------------------------------------------------------------------------ c. ties
@pytest.mark.parametrize("L,N", [(256, 64), (256, 1024), (1024, 64), (1024, 1024)])
def test_ties_go_to_the_first_index(L, N):
    """Every codebook row twice (row n + N/2 == row n): every distance occurs twice, bit for bit, and the lower index wins -- within a
    lane's scan (N = 1024: both rows in one lane) and across the lanes' reduction (N = 64: rows 32 lanes apart)."""
    x = J.inputs(L, N, 3, 3, 11, seed=[7, L, N])
    x["cb"] = np.concatenate([x["cb"][:, :N // 2], x["cb"][:, :N // 2]], axis=1)
    _, codes, lat, zq = J.oracle_stages(**x)
    assert codes.max() < N // 2 and len(np.unique(codes)) > 1
    for form in (1, 0):
        got = _run(x, form)
        assert got[0].max() < N // 2, f"form {form}: a tie went to the second copy"
        _same(got, (codes, zq, lat), f"form {form}")
    _report("dac_rvq", group="c", case=f"L{L}-N{N}", compared=int(2 * codes.size), mismatches=0)


# ------------------------------------------------------------------------------------------------------------------ d. non-finite
@pytest.mark.parametrize("L,N", [(256, 64), (1024, 1024)])
def test_non_finite_residuals_stay_in_their_frames(L, N):
    B, T, n_q = 2, 40, 3
    x = J.inputs(L, N, n_q, B, T, seed=[13, L, N])
    clean = {form: _run(x, form) for form in (1, 0)}
    _same(clean[1], clean[0], "clean run, one launch vs per stage")
    # (clip, channel, frame): frames 15 and 16 of a clip (the last and the first frame of two workgroups), channel rows next to each other
    # in LDS, the last frame of the batch
    hits = [(0, 3, 15, np.nan), (0, L - 1, 16, np.inf), (1, 0, 15, -np.inf), (1, 1, 16, np.nan), (0, 200, 5, np.inf), (1, L // 2, T - 1, -np.inf)]
    bad = x["r"].copy()
    for b, c, t, v in hits:
        bad[b, c, t] = v
    got = {form: _run(x, form, r=bad) for form in (1, 0)}
    _same(got[1], got[0], "one launch vs per stage", nan=True)
    touched = np.zeros((B, T), bool)
    for b, _, t, _ in hits:
        touched[b, t] = True
    for form in (1, 0):
        codes, zq, lat = got[form]
        for i in range(n_q):
            want, _ = ops.vq_argmin(lat[:, i * D:(i + 1) * D, :], x["cb"][i])
            assert np.array_equal(codes[:, i, :], want), f"form {form} stage {i}: the codes do not follow the argmin op on that stage's latents"
        assert not np.isfinite(zq.transpose(0, 2, 1)[touched]).all(), "the planted values never reached zq"
        for g, c in zip(got[form], clean[form]):
            assert np.array_equal(g.transpose(0, 2, 1)[~touched], c.transpose(0, 2, 1)[~touched]), f"form {form}: a frame that was not hit changed"
    _report("dac_rvq", group="d", case=f"L{L}-N{N}", hit_frames=int(touched.sum()), clean_frames_compared=int((~touched).sum()), mismatches=0)


# ------------------------------------------------------------------------------------------- e. what the one-launch form declines
DECLINED = [dict(L=128), dict(L=384), dict(L=1280), dict(N=96), dict(N=2048), dict(dim=4), dict(n_q=0)]


@pytest.mark.parametrize("change", DECLINED, ids=lambda c: "%s%d" % next(iter(c.items())))
def test_one_launch_form_declines_without_touching_the_outputs(change):
    shape = dict(L=256, N=64, n_q=2, B=2, T=17, dim=D)
    shape.update(change)
    x = J.inputs(**shape)
    B, T, n_q, dim = shape["B"], shape["T"], shape["n_q"], shape["dim"]
    out = (np.full((B, max(n_q, 1), T), -7, np.int64), np.full((B, shape["L"], T), 7.0, np.float32), np.full((B, max(n_q, 1) * dim, T), 7.0, np.float32))
    st = ops.dac_rvq(x["r"], x["w_in"], x["b_in"], x["cb"], x["w_out"], x["b_out"], form=1, out=out)
    assert st == (_lib.NC_EINVAL if n_q == 0 else _lib.NC_EUNSUPPORTED), (st, _lib.lib().nc_last_error())
    assert np.all(out[0] == -7) and np.all(out[1] == 7.0) and np.all(out[2] == 7.0)
    if n_q == 0:
        assert ops.dac_rvq(x["r"], x["w_in"], x["b_in"], x["cb"], x["w_out"], x["b_out"], form=0, out=out) == _lib.NC_EINVAL
        assert np.all(out[0] == -7) and np.all(out[1] == 7.0) and np.all(out[2] == 7.0)
    _report("dac_rvq", group="e", case=str(change), status=int(st))


@pytest.mark.parametrize("L,N", [(384, 64), (256, 96), (384, 96)])
@pytest.mark.parametrize("B,T", [(3, 11), (2, 140)])
def test_stagewise_form_at_shapes_the_one_launch_form_declines(L, N, B, T):
    """Latent widths and codebook sizes no model test reaches; (2,140) is above the 256 frames at which vq_argmin changes its kernel."""
    x = J.inputs(L, N, 3, B, T)
    stages, codes, lat, zq = J.oracle_stages(**x)
    _same(_run(x, 0), (codes, zq, lat), "per stage vs oracle")
    worst = dict(z_e=0.0, choice=0.0, q=0.0)
    for i, sg in enumerate(stages):
        what = f"L{L} N{N} stage {i}"
        worst["z_e"] = max(worst["z_e"], J.judge_projection(sg["z_e"], sg["r_in"], x["w_in"][i], x["b_in"][i], what + " z_e"))
        worst["choice"] = max(worst["choice"], J.judge_choice(sg["idx"], sg["z_e"], x["cb"][i], what)[0])
        worst["q"] = max(worst["q"], J.judge_projection(sg["q"], sg["st"], x["w_out"][i], x["b_out"][i], what + " q"))
    _report("dac_rvq", group="e", case=f"L{L}-N{N}-q3-B{B}xT{T}", form=0, worst_err_over_allowed=worst)


# ------------------------------------------------------------------------------------------------------------------ f. rvq_update
UPDATE_ROWS = (1, 3, 130)


def _update_lengths(s):
    return sorted({T for T in (s, 8, 248, 256, 264, 1000 * s) if T % s == 0})


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_rvq_update_is_exact(s):
    """zq' = (first ? 0 : zq) + repeat(q, s) and r' = r - repeat(q, s): one binary32 operation each, so numpy's are the same bits.  With
    first = 1 the prior zq is NaN: it must be overwritten, not added to."""
    rng = np.random.default_rng(s)
    n = 0
    for rows, T, first, with_r in itertools.product(UPDATE_ROWS, _update_lengths(s), (0, 1), (False, True)):
        q = rng.standard_normal((rows, T // s)).astype(np.float32)
        zq = np.full((rows, T), np.nan, np.float32) if first else rng.standard_normal((rows, T)).astype(np.float32)
        r = rng.standard_normal((rows, T)).astype(np.float32) if with_r else None
        rep = np.repeat(q, s, axis=1)
        got_zq, got_r = ops.rvq_update(q, zq, r, s=s, first=bool(first))
        what = f"rows {rows} T {T} s {s} first {first} residual {with_r}"
        assert np.array_equal(got_zq, rep if first else zq + rep), what
        assert (got_r is None) if r is None else np.array_equal(got_r, r - rep), what
        n += got_zq.size * (2 if with_r else 1)
    _report("rvq_update", group="f", s=s, rows=list(UPDATE_ROWS), T=_update_lengths(s), compared=n, mismatches=0)


def test_rvq_update_refuses_a_row_that_is_no_multiple_of_the_stride():
    z = np.zeros((2, 9), np.float32)
    st = _lib.lib().nc_op_rvq_update(0, z.ctypes.data, z.ctypes.data, None, 2, 9, 2, 0)
    assert st == _lib.NC_EINVAL


# ------------------------------------------------------------------------------------------------------------------- g. vq_gather
@pytest.mark.parametrize("N", [64, 4096])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 85), (2, 257)])
def test_vq_gather_in_snacs_code_layout(N, B, T):
    """The codes of a level sit inside a clip's row of all levels: an offset into a flat buffer and a batch stride above T.  Codes outside
    [0, N) are clamped to the nearest row -- the engine's behaviour where the reference's Embedding would throw."""
    rng = np.random.default_rng([N, B, T])
    cb = rng.standard_normal((N, D)).astype(np.float32)
    offset, bstride, guard = 5 + T // 2, T + T // 2 + 3, 64
    flat = np.full(offset + B * bstride + 9, 2 ** 62, np.int64)          # what a read outside the rows would meet: clamps to N - 1
    codes = rng.integers(0, N, (B, T))
    odd = [(-1, 0), (N, N - 1), (2 ** 40, N - 1), (-2 ** 40, 0)]
    if T >= 85:
        for k, (c, _) in enumerate(odd):
            codes[k % B, 7 + 16 * k] = c
    else:
        codes[0, 0] = N
    for b in range(B):
        flat[offset + b * bstride:offset + b * bstride + T] = codes[b]
    rows = np.clip(codes, 0, N - 1)
    if T >= 85:
        for k, (_, row) in enumerate(odd):
            assert rows[k % B, 7 + 16 * k] == row
    buf = ops.vq_gather(cb, flat, offset, bstride, B, T, guard=guard, fill=-123.0)
    out = buf[guard:-guard].reshape(B, D, T)
    assert np.array_equal(out, cb[rows].transpose(0, 2, 1))
    assert np.all(buf[:guard] == -123.0) and np.all(buf[-guard:] == -123.0), "the kernel wrote outside its output"
    _report("vq_gather", group="g", N=N, B=B, T=T, compared=int(out.size), mismatches=0)
