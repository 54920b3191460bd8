"""CPU suite of the loudness feature: the serial host twins (nc_audio_kweight_host, nc_loudness_host, nc_loudness_normalize_host,
nc_audio_apply_gain_db_host), the coefficient source and the block-table builder, judged by tests/loudness_ref.py -- a binary64 lfilter
loop and the BS.1770 gating with real log10.  The twin-vs-binary64 gaps of the recursion are measured, not derived (the feedback path
admits no useful bound): tests/golden/loudness_bounds.json, written by regenerate(), and the twin is held to MARGIN times what is recorded.
No device is used; tests/test_loudness_gpu.py holds the kernels to these twins bit for bit."""
import ctypes as C

import numpy as np
import pytest

import loudness_ref as R
import quality_ref as Q
from neuralcodecs_amd import LoudnessConfig, _lib
from neuralcodecs_amd import loudness as L

MARGIN = 1.5          # as tests/op_judge.py
RATE = R.RATE


def twin_kweight(x, rate, filt):
    return L.kweight([x], rate, filt, host=True)[0]


def twin_loudness(x, rate, filt, target=-24.0):
    return L.loudness([x], rate, LoudnessConfig(filt, target), host=True)["lufs"][0]


def twin_normalize(x, rate, filt, target):
    return L.normalize_loudness([x], rate, LoudnessConfig(filt, target), host=True)[0][0]


def regenerate():
    return R.write_bounds(twin_kweight, twin_loudness, twin_normalize)


@pytest.fixture(scope="module")
def measured():
    """the twin against the judge on every fixture, computed once"""
    return R.measure(twin_kweight, twin_loudness, twin_normalize)


def _ulps(got, want, eps):
    want = np.asarray(want, np.float64)
    scale = np.where(want == 0, np.finfo(np.float64).tiny, 2.0 ** np.floor(np.log2(np.abs(np.where(want == 0, 1.0, want)))) * eps)
    return np.abs(np.asarray(got, np.float64) - want) / scale


# ------------------------------------------------------------------------------------------------------------------ coefficients, tables
@pytest.mark.parametrize("filt", R.FILTERS)
@pytest.mark.parametrize("rate", [8000, 44100, 48000])
def test_coefficients_and_tables_are_the_binary64_evaluation(rate, filt):
    b, a = L.kweight_coeffs(rate, filt)
    wb, wa = R.coeffs64(rate, filt)
    assert _ulps(b, wb, 2.0 ** -52).max() <= 1 and _ulps(a, wa, 2.0 ** -52).max() <= 1
    got, want = L.kweight_tables(rate, filt), R.tables64(rate, filt)
    for k, eps in (("Hm", 2.0 ** -23), ("Cm", 2.0 ** -23), ("Gs", 2.0 ** -52), ("M", 2.0 ** -52)):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype
        assert _ulps(got[k], want[k], eps).max() <= 1, k
        assert (got[k] == want[k]).mean() >= 0.99, k
    assert (np.triu(got["Hm"], 1) == 0).all() and got["Hm"][0, 0] == np.float32(b[0, 0] * b[1, 0])


def test_reference_coefficients_are_the_widened_literals():
    b, a = L.kweight_coeffs(123456, "reference")
    assert np.array_equal(b, np.float32(R.REF_B).astype(np.float64)) and np.array_equal(a, np.float32(R.REF_A).astype(np.float64))


def test_designed_filter_at_48k_against_the_reference_constants():
    """|designed(48 kHz) - reference| <= 1e-5 on every coefficient: a property of the design.  Observed gap: 9e-16 against the decimal
    constants of LoudnessMeter.cs:41-52 (6e-8 against their binary32 roundings).  The design is the bilinear transform of the analog
    prototypes behind the BS.1770 constants (shelf 1681.97 Hz, +3.9998 dB, Q 0.70718; high pass 38.135 Hz, Q 0.50033, numerator
    (1, -2, 1)).  A round-number RBJ design (+4 dB / 1500 Hz / Q 1/sqrt(2); 38 Hz / Q 0.5) does not have the property: it misses by 1.08e-4
    (shelf b), 4.0e-5 (shelf a), 2.9e-5 (high-pass a) and 9.9e-3 (high-pass b, which RBJ normalises to 0.99504 (1, -2, 1))."""
    b, a = L.kweight_coeffs(48000, "designed")
    gap_b = np.abs(b - np.array(R.REF_B)).max(axis=1)
    gap_a = np.abs(a - np.array(R.REF_A)).max(axis=1)
    print("designed vs reference at 48 kHz: shelf b %.3g a %.3g, high pass b %.3g a %.3g" % (gap_b[0], gap_a[0], gap_b[1], gap_a[1]))
    assert max(gap_b.max(), gap_a.max()) <= 1e-5
    b8, a8 = L.kweight_coeffs(8000, "designed")                                  # and it does follow the rate
    assert np.abs(b8 - b).max() > 0.1 and np.abs(a8 - a).max() > 0.1


# ------------------------------------------------------------------------------------------------------------------ filter
def test_judge_dc_decays_and_a_512_tap_truncation_would_not():
    b, a = R.coeffs64(RATE, "reference")
    step = np.full(12000, 0.2)
    y = R.kweight64(step, RATE, "reference")
    assert abs(y[-1]) < 1e-3 * 0.2 and np.abs(y[-2000:]).max() < 1e-3 * 0.2
    imp = np.zeros(512)
    imp[0] = 1.0
    h1, h2 = R.lfilter(b[0], a[0], imp), R.lfilter(b[1], a[1], imp)
    assert abs(h2.sum()) > 0.05                                                # pole radius 0.995: cut at 512 taps the high pass still passes 12 % of DC
    fir = np.convolve(np.convolve(step, h1)[:step.size], h2)[:step.size]       # what two 512-tap convolutions leave of the offset
    assert abs(fir[-1]) > 1e-3 * 0.2


@pytest.mark.parametrize("filt", R.FILTERS)
def test_twin_filter_against_binary64_lfilter(measured, filt):
    rec = R.bounds()["kweight_rel"]
    for name in R.fixtures():
        key = f"{name}/{filt}"
        print(key, "max|y - y64| / max|y64| =", measured["kweight_rel"][key], "recorded", rec[key])
        assert measured["kweight_rel"][key] <= MARGIN * rec[key], key
        assert rec[key] < 1e-4, key                                            # a wrong coefficient or block edge shows as 1e-2 and more, not as rounding


def test_twin_dc_fixture_output_has_no_offset_left():
    y = twin_kweight(R.fixtures()["dc"], RATE, "reference").astype(np.float64)
    assert abs(y[-2000:].mean()) < 1e-3 * 0.2


def test_twin_blocks_at_every_row_length_equal_the_long_row_prefix_free_run():
    """rows of 1, 63, 64, 65, 127, 129 samples against the judge: block edges and the zero tail of the last block"""
    for n in (1, 63, 64, 65, 127, 129, 1000):
        x = np.float32(0.5) * Q.signal(n, RATE, n)
        y, y64 = twin_kweight(x, RATE, "designed"), R.kweight64(x, RATE, "designed")
        assert y.shape == (n,) and np.abs(y - y64).max() <= 1e-5 * max(np.abs(y64).max(), 1e-3)


# ------------------------------------------------------------------------------------------------------------------ loudness
def test_no_fixture_block_lies_within_a_hundredth_of_a_db_of_a_gate():
    skipped = 0
    for name, x in R.fixtures().items():
        for filt in R.FILTERS:
            g = R.loudness64(x, RATE, filt)
            print(name, filt, "lufs %.4f" % g["lufs"], "blocks", g["n_blocks"], g["n_pass_abs"], g["n_pass_rel"], "closest to a gate %.3f dB" % g["margin_db"])
            assert g["n_blocks"] > 0 and g["margin_db"] > 0.01, (name, filt)
    assert skipped <= 0


def test_twin_lufs_and_counts_against_the_judge(measured):
    rec = R.bounds()
    print("largest |delta LUFS|", measured["lufs_abs"], "recorded", rec["lufs_abs"])
    assert measured["lufs_abs"] <= MARGIN * rec["lufs_abs"] and rec["lufs_abs"] < 1e-4
    fx = R.fixtures()
    for filt in R.FILTERS:
        counts = {}
        for name, x in fx.items():
            want = R.loudness64(x, RATE, filt)
            got = L.loudness([x], RATE, LoudnessConfig(filt), host=True)
            counts[name] = (int(got["n_blocks"][0]), int(got["n_pass_abs"][0]), int(got["n_pass_rel"][0]))
            assert counts[name] == (want["n_blocks"], want["n_pass_abs"], want["n_pass_rel"]), (name, filt)
            assert abs(float(got["gain"][0]) - R.gain64(-24.0, want["lufs"])) <= 1e-5 * R.gain64(-24.0, want["lufs"])
        assert counts["zeros"][1] < counts["zeros"][0] and counts["tones"][1] == counts["tones"][0]         # the stretch of zeros fails the absolute gate
        assert counts["quiet"][2] < counts["quiet"][1] == counts["quiet"][0]                                   # the quiet stretch only the relative one


def test_multichannel_weights_against_the_judge():
    rate = RATE
    chans = np.stack([np.float32(0.3 / (1 + c)) * Q.signal(9000, rate, 60 + c) for c in range(5)])
    for Cn in (2, 5):
        want = R.loudness64(chans[:Cn], rate, "reference")
        got = L.loudness([chans[:Cn]], rate, host=True)
        assert want["margin_db"] > 0.01
        assert abs(float(got["lufs"][0]) - want["lufs"]) <= MARGIN * R.bounds()["lufs_abs"]
        assert int(got["n_pass_rel"][0]) == want["n_pass_rel"]
    mono = L.loudness([chans[3]], rate, host=True)["lufs"][0]
    four = np.zeros((5, 9000), np.float32)
    four[3] = chans[3]
    assert abs(float(L.loudness([four], rate, host=True)["lufs"][0]) - (float(mono) + 10 * np.log10(float(np.float32(1.41))))) < 1e-4


def test_block_structure_and_the_remainder_path():
    rate = 11025
    N, S = R.geometry(rate)
    assert (N, S) == (4410, 1102) and N - 4 * S == 2
    for n, blocks in ((N - 1, 0), (N, 1), (N + S - 1, 1), (N + S, 2), (N + 4 * S + 7, 5)):
        x = np.float32(0.4) * Q.signal(n, rate, 7)
        got = L.loudness([x], rate, host=True)
        want = R.loudness64(x, rate, "reference")
        assert int(got["n_blocks"][0]) == blocks == want["n_blocks"]
        if blocks == 0:
            assert got["lufs"][0] == -70 and got["n_pass_abs"][0] == 0
        else:
            assert abs(float(got["lufs"][0]) - want["lufs"]) <= MARGIN * R.bounds()["lufs_abs"]
    # the two remainder samples count: a spike inside them moves the level of the one-block clip
    x = np.float32(0.01) * Q.signal(N, rate, 8)
    y = x.copy()
    y[N - 1] = 0.9
    assert L.loudness([y], rate, host=True)["lufs"][0] > L.loudness([x], rate, host=True)["lufs"][0] + 1.0
    want = R.loudness64(y, rate, "reference")["lufs"]                       # below -32 one ulp32 is 2^-18, twice the recorded floor
    assert abs(float(L.loudness([y], rate, host=True)["lufs"][0]) - want) <= MARGIN * max(R.bounds()["lufs_abs"], 2.0 ** -18)


def test_silent_and_non_finite_clips():
    zero = np.zeros(9000, np.float32)
    ok = np.float32(0.3) * Q.signal(9000, RATE, 11)
    bad = ok.copy()
    bad[100], bad[101] = np.nan, np.inf
    got = L.loudness([ok, bad, zero, ok], RATE, host=True)
    assert got["lufs"][2] == -70 and np.isfinite(got["gain"][2]) and got["n_pass_abs"][2] == 0 and got["n_blocks"][2] > 0
    assert np.isnan(got["lufs"][1]) and np.isnan(got["gain"][1]) and got["n_bad"][1] == 2 and got["n_bad"][[0, 2, 3]].sum() == 0
    alone = L.loudness([ok], RATE, host=True)
    for k in ("lufs", "gain", "n_blocks", "n_pass_abs", "n_pass_rel"):
        assert got[k][0] == alone[k][0] == got[k][3]


def test_normalize_reaches_the_target_and_gains_undo_each_other(measured):
    rec = R.bounds()
    print("largest |level after normalize + 16|", measured["normalize_abs"], "recorded", rec["normalize_abs"])
    assert measured["normalize_abs"] <= MARGIN * rec["normalize_abs"] and rec["normalize_abs"] < 1e-4
    x = R.fixtures()["tones"]
    lev, rows = L.normalize_loudness([x], RATE, LoudnessConfig("reference", -16.0), host=True)
    assert np.array_equal(lev[0], x * rows["gain"][0])                       # fl(x gain), nothing else
    # one gain step is x 10^(g / 20) within 4 ulp32: nc_expf <= 2 ulp, the rounded argument fl(g GAIN_FACTOR) with the rounded constant
    # <= |arg| 2^-23 <= 1.4 2^-23 for |g| <= 12 dB, the product 0.5 ulp; two steps at most twice that
    for g in (0.5, 3.0, 6.0, 12.0):
        up = L.apply_gain_db([x], [g], host=True)[0]
        want = x.astype(np.float64) * 10.0 ** (g / 20.0)
        assert np.abs(up - want).max() <= 4 * 2.0 ** -23 * np.abs(want).max()
        back = L.apply_gain_db([up], [-g], host=True)[0]
        assert np.abs(back - x.astype(np.float64)).max() <= 8 * 2.0 ** -23 * np.abs(x).max()
    restored = L.restore_ragged(lev, rows, host=True)[0]
    assert np.abs(restored - x.astype(np.float64)).max() <= 8 * 2.0 ** -23 * np.abs(x).max()


def test_packed_layout_in_place_and_each_clip_alone():
    """planar stereo clips at odd offsets with NaN gaps: levelled in place, the gaps untouched, every clip as when measured alone"""
    lens, offs, o = [5000, 3300, 7001], [], 1
    for n in lens:
        for _ in range(2):
            offs.append(o)
            o += n + 3
    buf = np.full(o, np.nan, np.float32)
    for i, at in enumerate(offs):
        buf[at:at + lens[i // 2]] = np.float32(0.2 + 0.1 * i) * Q.signal(lens[i // 2], RATE, 90 + i)
    cfg = LoudnessConfig("designed", -20.0)
    rows = L.loudness_packed(buf, RATE, lens, offs, 2, cfg, host=True)
    work = buf.copy()
    out, oo, nrows = L.normalize_loudness_packed(work, RATE, lens, offs, 2, cfg, in_place=True, host=True)
    assert np.shares_memory(out, work) and oo == offs and np.array_equal(np.isnan(work), np.isnan(buf))
    for b, n in enumerate(lens):
        clip = np.stack([buf[offs[2 * b + c]:offs[2 * b + c] + n] for c in range(2)])
        alone = L.loudness([clip], RATE, cfg, host=True)
        assert alone["lufs"][0] == rows["lufs"][b] == nrows["lufs"][b] and alone["gain"][0] == rows["gain"][b]
        for c in range(2):
            at = offs[2 * b + c]
            assert np.array_equal(work[at:at + n], buf[at:at + n] * rows["gain"][b])


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_host_twins():
    lib, E, i64 = _lib.lib(), _lib.NC_EINVAL, _lib.i64_array
    x = np.zeros(4000, np.float32)
    out = np.zeros(4000, np.float32)
    words = np.zeros((2, L.ROW_WORDS), np.int32)
    good = LoudnessConfig().c_struct()
    px, po, pw = x.ctypes.data, out.ctypes.data, words.ctypes.data

    def loud(pcm=px, B=1, Cn=1, off=(0,), n=(3000,), rate=8000, cfg=good, o=pw):
        return lib.nc_loudness_host(pcm, B, Cn, i64(off) if off is not None else None, i64(n) if n is not None else None, rate,
                                    C.byref(cfg) if cfg is not None else None, o)

    def norm(pcm=px, B=1, Cn=1, off=(0,), n=(3000,), rate=8000, cfg=good, o=po, oo=(0,), rows=pw):
        return lib.nc_loudness_normalize_host(pcm, B, Cn, i64(off), i64(n), rate, C.byref(cfg) if cfg is not None else None, o,
                                              i64(oo) if oo is not None else None, rows)

    def kw(pcm=px, Rn=1, off=(0,), n=(100,), rate=8000, filt=0, o=po, oo=(0,)):
        return lib.nc_audio_kweight_host(pcm, Rn, i64(off), i64(n), rate, filt, o, i64(oo))

    def gain(pcm=px, B=1, Cn=1, off=(0,), n=(100,), db=(1.0,), o=po, oo=(0,)):
        d = np.array(db, np.float32) if db is not None else None
        return lib.nc_audio_apply_gain_db_host(pcm, B, Cn, i64(off), i64(n), d.ctypes.data if d is not None else None, o, i64(oo))

    def cfg(filt=0, target=-24.0):
        c = LoudnessConfig().c_struct()
        c.filter, c.target_db = filt, target
        return c

    assert loud() == _lib.NC_OK and norm() == _lib.NC_OK and kw() == _lib.NC_OK and gain() == _lib.NC_OK
    assert loud(pcm=None) == E and loud(o=None) == E and loud(cfg=None) == E and loud(off=None) == E and loud(n=None) == E
    assert norm(pcm=None) == E and norm(o=None) == E and norm(rows=None) == E and norm(cfg=None) == E and norm(oo=None) == E
    assert kw(pcm=None) == E and kw(o=None) == E and gain(pcm=None) == E and gain(o=None) == E and gain(db=None) == E
    for B, Cn in ((0, 1), (-1, 1), (1, 0), (1, 6), (6554, 5)):
        assert lib.nc_loudness_host(px, B, Cn, i64([0] * max(B * Cn, 1)), i64([10] * max(B, 1)), 8000, C.byref(good), pw) == E, (B, Cn)
    assert kw(Rn=0) == E and kw(Rn=32768, off=[0] * 32768, n=[1] * 32768, oo=[0] * 32768) == E
    assert loud(off=(-1,)) == E and loud(n=(-1,)) == E and norm(oo=(-1,)) == E and kw(off=(-1,)) == E and kw(n=(-1,)) == E and kw(oo=(-1,)) == E
    assert gain(off=(-1,)) == E and gain(n=(-1,)) == E and gain(oo=(-1,)) == E
    assert loud(rate=9) == E and norm(rate=0) == E and kw(rate=9) == E and loud(rate=10) == _lib.NC_OK
    assert loud(cfg=cfg(filt=2)) == E and loud(cfg=cfg(filt=-1)) == E and norm(cfg=cfg(filt=9)) == E and kw(filt=2) == E
    for t in (float("nan"), float("inf"), -float("inf")):
        assert loud(cfg=cfg(target=t)) == E and norm(cfg=cfg(target=t)) == E and gain(db=(t,)) == E
    b = np.zeros(6)
    assert lib.nc_audio_kweight_coeffs(48000, 0, None, b.ctypes.data) == E and lib.nc_audio_kweight_coeffs(48000, 3, b.ctypes.data, b.ctypes.data) == E
    assert lib.nc_audio_kweight_coeffs(9, 1, b.ctypes.data, b.ctypes.data) == E
    assert lib.nc_audio_kweight_tables(48000, 0, None, None, None, None) == E
    assert b"" != lib.nc_last_error()


def test_struct_layouts():
    assert C.sizeof(_lib.NcLoudnessRow) == 24 and C.sizeof(_lib.NcLoudnessCfg) == 8 and L.ROW_WORDS == 6
    assert [f for f, _ in _lib.NcLoudnessRow._fields_] == ["lufs", "gain", "n_blocks", "n_pass_abs", "n_pass_rel", "n_bad"]
