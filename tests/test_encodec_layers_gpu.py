"""GPU suite: Encodec layer by layer.  ops.encodec_trace returns every activation the SEANet driver holds between launches (a "tap"), by
the launches the model itself makes; reduced-depth configurations (tests/encodec_layers.py) put every streaming kernel and both persistent
LSTM widths a few layers from the input.  Every tap has two judges: np.array_equal with the C oracle's tap (RefEncodec.trace) for the
bits, and |tap - binary64 layer(inputs)| <= tolerance for the meaning (encodec_layers.judge_tap: a derived bound on the weight-norm
first convolutions, M x ATen's own binary32 error elsewhere), the layer's inputs being the oracle's taps, so a failure names its layer.
(mean, rstd) of a pending GroupNorm are held to the oracle's bit for bit and to two-pass binary64 statistics within 2 ulp32.
The form a layer took is OBSERVED: in the children of test_every_form_is_observed the engine keeps its launch log, and every case
asserts the "enc_form" / "lstm" lines of its last tap against the rules of try_stream_down / try_stream_up / resblock_first_pass /
persistent_ok restated below.  Each test prints one `OPREPORT {...}` line (run with -s).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import encodec_layers as EL  # noqa: E402
import ref64  # noqa: E402
from neuralcodecs_amd import Encodec, ops  # noqa: E402
from oracle import c_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHILD = os.environ.get("NC_ENCODEC_LAYERS_CHILD") == "1"
_LOG = os.environ.get("NC_LAUNCH_LOG") if _CHILD else None
_log_pos = 0


def _report(kernel, **kw):
    print("\nOPREPORT " + json.dumps(dict(kernel=kernel, **kw), sort_keys=True))


def _flag(name):
    return os.environ.get(name, "") not in ("", "0")


def _new_lines():
    """The lines the engine logged since the last call (None where no log is kept: outside a child)."""
    global _log_pos
    if _LOG is None:
        return None
    with open(_LOG) as f:
        f.seek(_log_pos)
        new = f.read()
        _log_pos = f.tell()
    return new.splitlines()


_engines, _oracles = {}, {}


def engine(name):
    if name not in _engines:
        cfg, _, blob = EL.model(name)
        m = Encodec(cfg)
        m.load_blob(blob)
        _engines[name] = m
    return _engines[name]


def oracle(name):
    if name not in _oracles:
        cfg, _, blob = EL.model(name)
        _oracles[name] = c_oracle.RefEncodec(cfg, blob)
    return _oracles[name]


# ---------------------------------------------------------------------------------------------------------------- the launchers' rules
def _lstm_chunks(T, n_layers, may_pipe):
    """lstm_chunk_starts (nc_lstm.hip): the number of chunks of the layer-pipelined persistent form."""
    want = max(1, int(os.environ.get("NC_LSTM_CHUNKS", "6") or 6))
    even = _flag("NC_LSTM_EVEN_CHUNKS")
    starts = [0]
    if n_layers >= 2 and want > 1 and T >= 32 and may_pipe:
        last = 0 if even else max(8, (T // 8) & ~1)
        nbig = want if even else want - 1
        big = max((((T - last) + nbig - 1) // nbig + 1) & ~1, 8)
        t0 = big
        while t0 < ((T - last) & ~1):
            starts.append(t0); t0 += big
        tail0 = (T - last) & ~1
        if last > 0 and tail0 > starts[-1]:
            starts.append(tail0)
    return len(starts)


def _lstm_line(C, N, T, n_layers):
    """persistent_ok / plan_persistent: the persistent kernel for C = 64 and C = 512 on a whole MI355X, else one launch per step."""
    if _flag("NC_LSTM_STEPWISE") or C % 64 or C // 4 not in (128, 16):
        return f"lstm step C={C} layers={n_layers} T={T}"
    tiles = (N + 15) // 16
    ub = int(os.environ.get("NC_LSTM_UB", "0") or 0)
    ubw = 2 if C == 512 and (ub == 2 or (ub != 4 and tiles == 1)) else 4
    chunks = _lstm_chunks(T, n_layers, 4 * C * T * N < 2 ** 31)
    return (f"lstm seq C={C} UBW={ubw} htile={0 if _flag('NC_LSTM_NO_HTILE') else 1} piped={int(chunks > 1)} chunks={chunks} tiles={tiles} "
            f"layers={n_layers} T={T}")


def _dense(C, L):
    return dict(C=C, L=L, rs=L, ptr=0)                      # ptr: byte offset of sample 0 of a row from a 16-byte boundary


def _al8(*acts):
    return all(a["ptr"] % 8 == 0 and a["rs"] % 2 == 0 and (a["C"] * a["rs"]) % 2 == 0 for a in acts)


def expected_forms(cfg, stack, N, L):
    """The "enc_form" / "lstm" lines of one run of a stack, in launch order, by the rules of the driver (nc_encodec.hip) and of the LSTM
    (nc_lstm.hip) for a model of 32 x 2^i filters per stage (the widths the streaming kernels are instantiated for)."""
    no_fuse = _flag("NC_ENCODEC_NO_FUSE")
    gn = cfg.norm == "time_group_norm"
    finish = not _flag("NC_NO_GN_FINISH")
    stream_ok = not no_fuse and not cfg.causal and (not gn or finish)
    out = []

    def res_a(x):
        if stream_ok and not _flag("NC_NO_RES_A") and x["C"] in (32, 64) and x["L"] >= 4 and x["L"] % 2 == 0:
            out.append(f"enc_form res_a<{x['C'] // 32}> {'aligned' if _al8(x) else 'unaligned'}")

    plan = lambda n, k, s: _plan_len(n, k, s, cfg.causal)
    if stack == "enc":
        C, T = cfg.n_filters, plan(L, 7, 1)
        for r in reversed(cfg.ratios):
            x = _dense(C, T)
            res_a(x)
            ok = stream_ok and C % 2 == 0 and C <= 128 and T > max(_pads(T, 2 * r, r, cfg.causal))
            if ok and r == 2 and not _flag("NC_NO_DOWN2") and 2 * C == 64 and T >= 4 and T % 2 == 0:
                out.append(f"enc_form down<2> {'aligned' if _al8(x) else 'unaligned'}")
            elif ok and r == 4 and not _flag("NC_NO_DOWN4") and 2 * C == 128 and C % 8 == 0 and T >= 8 and T % 4 == 0:
                out.append("enc_form down<4> aligned")
            elif ok and r == 5 and not _flag("NC_NO_DOWN5") and 2 * C == 256 and C % 4 == 0 and T >= 10 and T % 5 == 0:
                out.append("enc_form down<5> aligned")
            C, T = 2 * C, plan(T, 2 * r, r)
        out.append(_lstm_line(C, N, T, cfg.lstm_layers))
    else:
        C, T = cfg.n_filters << len(cfg.ratios), plan(L, 7, 1)
        out.append(_lstm_line(C, N, T, cfg.lstm_layers))
        dual = False
        for r in cfg.ratios:
            Lfull = (T - 1) * r + 2 * r
            left = r - r // 2 if not cfg.causal else 0
            s_in = _dense(C, T)
            ok = dual and stream_ok and C % 2 == 0 and C <= 128 and T >= 4 and T % 2 == 0
            if ok and ((r == 2 and not _flag("NC_NO_UP2") and C // 2 == 32) or (r == 4 and not _flag("NC_NO_UP4") and C // 2 == 64)):
                out.append(f"enc_form up<{r}> {'aligned' if _al8(s_in) else 'unaligned'}")
                u = dict(C=C // 2, L=Lfull - r, rs=Lfull, ptr=4 * left % 16)
            elif _flag("NC_NO_UP_PITCH"):
                u = dict(C=C // 2, L=Lfull - r, rs=Lfull, ptr=4 * left % 16)
            else:
                u = dict(C=C // 2, L=Lfull - r, rs=(Lfull + 3) & ~3, ptr=0)          # rows at a pitch of whole 16 bytes, shifted to a boundary
            res_a(u)
            C, T, dual = C // 2, Lfull - r, True
    return out


def _pads(L, k, stride, causal):
    left, right, _ = ref64.sconv_pad_plan(L, k, stride, causal)
    return left, right


def _plan_len(L, k, stride, causal):
    left, right, z = ref64.sconv_pad_plan(L, k, stride, causal)
    return (L + z + left + right - k) // stride + 1


# ---------------------------------------------------------------------------------------------------------------- the taps
@pytest.mark.parametrize("case", EL.CASES, ids=EL.case_id)
def test_engine_taps_equal_the_oracle_and_hold_to_binary64(case):
    name, stack, B, L = case
    cfg, sd, _ = EL.model(name)
    m, dec = engine(name), stack == "dec"
    x = EL.case_input(case)
    taps = oracle(name).trace(x, decoder=dec)
    table = EL.layers(cfg, stack)
    assert ops.encodec_trace_taps(m) == len(table) == len(taps)
    M = EL.multipliers()
    worst, worst_stats, ratios, forms = 0.0, 0.0, {}, None
    for i, (layer, (want, wstats, raw)) in enumerate(zip(table, taps)):
        what = f"{EL.case_id(case)} tap {i} {layer['name']}"
        if i == len(table) - 1:
            _new_lines()                                    # the last tap runs the whole stack: its lines are the case's forms
        got, stats = ops.encodec_trace(m, x, i, decoder=dec)
        if i == len(table) - 1:
            forms = _new_lines()
        assert got.shape == want.shape, f"{what}: shape {got.shape}, oracle {want.shape}"
        assert np.array_equal(got, want), f"{what}: engine != oracle, max abs diff {np.abs(got - want).max():.3g}"
        assert (stats is None) == (wstats is None), f"{what}: pending GroupNorm statistics {'missing' if stats is None else 'unexpected'}"
        if stats is not None:
            assert np.array_equal(stats, wstats), f"{what}: (mean, rstd) engine {stats.tolist()} != oracle {wstats.tolist()}"
            worst_stats = max(worst_stats, EL.judge_stats(stats, raw, what))
        kind, ratio, rel = EL.judge_tap(cfg, sd, layer, EL.tap_inputs(taps, layer, x), got, what, M)
        if ratio is not None:
            ratios[kind] = max(ratios.get(kind, 0.0), ratio)
        worst = max(worst, rel)
    seen = None
    if forms is not None:
        want_forms = expected_forms(cfg, stack, B, L)
        got_forms = [ln for ln in forms if ln.startswith(("enc_form ", "lstm "))]
        assert got_forms == want_forms, f"{EL.case_id(case)}: the engine launched {got_forms}, the launchers' rules say {want_forms}"
        seen = sorted({ln.split(" T=")[0].replace("enc_form ", "") for ln in got_forms} | {ln.split()[1] for ln in forms if ln.startswith("conv_plan ")}
                      | {"gn " + ln[7:] for ln in forms if ln.startswith("enc_gn ")})
    _report("encodec_layers", case=EL.case_id(case), taps=len(table), worst_err_over_allowed=worst, err_over_aten_err=ratios,
            stats_ulp32=worst_stats, forms=seen)


@pytest.mark.parametrize("case", EL.TOO_SHORT, ids=EL.case_id)
def test_a_residual_block_on_one_sample_raises_the_existing_error(case):
    name, stack, B, L = case
    cfg, sd, _ = EL.model(name)
    m, x = engine(name), EL.case_input(case)
    with pytest.raises(ValueError, match="too short"):
        ops.encodec_trace(m, x, ops.encodec_trace_taps(m) - 1, decoder=stack == "dec")
    with pytest.raises(RuntimeError):
        oracle(name).trace(x, decoder=stack == "dec")
    got, _ = ops.encodec_trace(m, x, 0, decoder=stack == "dec")          # the taps in front of that block exist (zero-extended row, D9)
    EL.judge_tap(cfg, sd, EL.layers(cfg, stack)[0], [x], got, f"{EL.case_id(case)} tap 0", EL.multipliers())
    _report("encodec_layers", case=EL.case_id(case), raises="segment too short")


# ---------------------------------------------------------------------------------------------------------------- RMS scale
@pytest.mark.parametrize("L", [255, 256, 257, 4095, 4096, 4097, 9000], ids=lambda L: f"L{L}")
def test_rms_scale_chunk_and_workgroup_edges(L):
    """encode returns the per-clip scale: sqrt(mean(mono^2)) + 1e-8 in binary64 within 2 ulp32, and the oracle's bit for bit.  255 .. 257: the
    256-sample chunk edge; 4095 .. 4097: the 16-chunk workgroup edge; 9000: three workgroups with a ragged last chunk."""
    worst = 0.0
    for name, B in (("A", 1), ("A", 3), ("A1", 1), ("A1", 3)):
        cfg = EL.CONFIGS[name]
        rng = np.random.default_rng(10 * L + B + cfg.channels)
        x = (rng.standard_normal((B, cfg.channels, L)) * (0.1 + rng.random((B, 1, 1)))).astype(np.float32)
        frames = engine(name).encode(x)
        assert len(frames) == 1
        got = np.asarray(frames[0].scale, np.float32).reshape(B)
        _, rs = oracle(name).encode_frame(x)
        what = f"L={L} B={B} channels={cfg.channels}"
        assert np.array_equal(got, rs.reshape(B)), f"{what}: scale engine {got.tolist()} != oracle {rs.reshape(B).tolist()}"
        want = ref64.rms_scale(x)
        err = np.abs(got.astype(np.float64) - want) / ref64.ulp32(want)
        assert np.all(err <= 2.0), f"{what}: scale off by {err.max():.3g} ulp32 from binary64"
        worst = max(worst, float(err.max()))
    _report("rms_scale", L=L, cases=4, form="two_pass" if _flag("NC_RMS_TWO_PASS") else "one_launch", worst_ulp32=worst)


# ---------------------------------------------------------------------------------------------------------------- the other forms
_GN3 = "cfgA_ or cfgB_ or cfgC_"          # (-k matches case-insensitive substrings: the ids are built so that these tokens occur nowhere else)
_STREAM = ["res_a<1> aligned", "res_a<2> aligned", "down<2> aligned", "down<4> aligned", "down<5> aligned", "up<2> aligned", "up<4> aligned"]
# OPEN POINT, the unaligned instances: only res_a's is reachable -- behind the streaming up<2> (rows start one sample into an even pitch)
# and under NC_NO_UP_PITCH.  Both operands of down<2> and up<S> are always the dense s and y of a residual block at an even row length,
# so stream_aligned() is always true there: launch_down2(aligned = false) and launch_up2(aligned = false) are kernel instances that no
# path of the driver selects and that this file therefore cannot run.  They are either dead code to remove or owe an op-level hook of
# their own; neither is done here.
# "gn ...": where the GroupNorm statistics of a conv launch came from (its epilogue, finished in the launch | its epilogue, then
# gn_final_kernel | gn_block_kernel, then gn_final_kernel) -- the observable of the two NC_NO_GN_* rows.
ROWS = [   # (switches, -k expression of the cases the row bears on (None: the whole file), what some form of the row must contain, what none may)
    ({}, None, _STREAM + ["res_a<1> unaligned", "thin", "small", "lstm step C=128", "lstm step C=256", "gn epilogue_finished",
                          "lstm seq C=64 UBW=4 htile=1 piped=0", "lstm seq C=64 UBW=4 htile=1 piped=1", "lstm seq C=512 UBW=2 htile=1 piped=1",
                          "lstm seq C=512 UBW=2 htile=1 piped=0", "lstm seq C=512 UBW=4 htile=1 piped=1", "tiles=2", "layers=1", "one_launch"],
     ["gn epilogue_sums+final"]),
    ({"NC_NO_RES_A": "1"}, _GN3, ["down<2> aligned", "down<4> aligned", "down<5> aligned", "up<2> aligned", "up<4> aligned"], ["res_a<"]),
    ({"NC_NO_DOWN2": "1", "NC_NO_DOWN4": "1", "NC_NO_DOWN5": "1"}, f"_enc_ and ({_GN3})", ["res_a<1> aligned", "res_a<2> aligned"], ["down<"]),
    ({"NC_NO_UP2": "1", "NC_NO_UP4": "1"}, "_dec_ and (cfgB_ or cfgC_)", ["res_a<1> aligned", "res_a<2> aligned"], ["up<", "unaligned"]),
    # (the stem kernel takes no folded pad: the mono first convolution reaches it behind the padded copy of this row)
    ({"NC_ENCODEC_NO_FUSE": "1"}, "cfgA_ or cfgC_ or cfgE_", ["lstm seq C=64", "lstm step C=256", "stem"], ["res_a<", "down<", "up<"]),
    # (rows this short go to the small-shape kernel; with it held to one workgroup the C = 128 block runs on conv3s / conv1x1)
    ({"NC_SMALL_MAX_GRID": "1", "NC_SMALL_WIDE_BELOW": "0"}, "cfgC_", ["k3_stream", "pointwise"] + _STREAM, []),
    ({"NC_NO_UP_PITCH": "1"}, f"_dec_ and ({_GN3})", ["res_a<1> unaligned", "res_a<2> aligned", "up<2> aligned", "up<4> aligned"], ["res_a<1> aligned"]),
    ({"NC_NO_GN_FUSE": "1"}, "cfgA_ or cfgD_", ["gn block_pass+final", "res_a<1> aligned", "down<2> aligned"], ["gn epilogue"]),
    ({"NC_NO_GN_FINISH": "1"}, "cfgA_ or cfgC_", ["gn epilogue_sums+final", "lstm seq C=64", "lstm step C=256"],
     ["gn epilogue_finished", "res_a<", "down<", "up<"]),
    ({"NC_LSTM_STEPWISE": "1"}, "cfgA_ or cfgD_ or cfgD1_", ["lstm step C=64 layers=2", "lstm step C=512 layers=2", "lstm step C=512 layers=1"], ["lstm seq"]),
    ({"NC_LSTM_UB": "4"}, "cfgD_", ["lstm seq C=512 UBW=4 htile=1 piped=1", "tiles=1", "tiles=2"], ["UBW=2"]),
    ({"NC_LSTM_NO_HTILE": "1"}, "cfgA_ or cfgD_", ["lstm seq C=64 UBW=4 htile=0", "lstm seq C=512 UBW=2 htile=0", "lstm seq C=512 UBW=4 htile=0"], ["htile=1"]),
    ({"NC_LSTM_CHUNKS": "1"}, "cfgD_", ["lstm seq C=512 UBW=2 htile=1 piped=0", "lstm seq C=512 UBW=4 htile=1 piped=0"], ["piped=1"]),
    ({"NC_RMS_TWO_PASS": "1"}, "rms_scale", ["two_pass"], ["one_launch"]),
]


def test_every_form_is_observed_and_every_switch_row_leaves_the_taps_equal(tmp_path):
    """The switches are read once per process, so each row is a fresh child with the engine's launch log on: the default row runs this whole
    file, a switch row the configurations it bears on.  In every child every case compares every tap with the oracle -- passing in every row
    is equality across the kernel forms -- and asserts the launcher lines of its stack against the rules above, so a switch without
    effect or a rule that drifted fails there; here the forms a row reached are held to what it must and must not reach.  One child after
    the other, each under its own timeout; the first child that does not exit 0 ends the test."""
    if _CHILD:
        return                                              # (a child does not start children)
    for n, (row, keys, must, must_not) in enumerate(ROWS):
        e = dict(os.environ, NC_ENCODEC_LAYERS_CHILD="1", NC_LAUNCH_LOG=str(tmp_path / f"launch_{n}.log"), **row)
        cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)]
        r = subprocess.run(cmd + (["-k", keys] if keys else []), env=e, capture_output=True, text=True, timeout=420, cwd=ROOT)
        assert r.returncode == 0, (row, r.stdout[-3000:], r.stderr[-1500:])
        reps = [json.loads(ln[9:]) for ln in r.stdout.splitlines() if ln.startswith("OPREPORT ")]
        forms = set()
        for rep in reps:
            forms |= set(rep.get("forms") or []) | ({rep["form"]} if "form" in rep else set())
        missing = [w for w in must if not any(w in f for f in forms)]
        assert not missing, (row, "not reached", missing, sorted(forms))
        hit = sorted(f for f in forms for bad in must_not if bad in f)
        assert not hit, (row, "reached", hit)
        _report("variants", row=row, forms=sorted(forms))
