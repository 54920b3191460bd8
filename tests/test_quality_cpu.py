"""CPU suite of the round-trip quality feature: the serial host twins (nc_audio_stft_host, nc_audio_mel_spectrogram_host,
nc_quality_metrics_host), the table builders and nc_log10f, judged by tests/quality_ref.py -- binary64 formulas with derived bounds and
binary32 transcriptions of the reference.  No device is used; tests/test_quality_gpu.py holds the kernels to these twins bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import quality_ref as R
import ref64
from neuralcodecs_amd import QualityConfig, _lib, mel_filterbank, quality
from neuralcodecs_amd.quality import dft_basis, mel_spectrogram, quality_metrics, stft, stft_frames

MARGIN = 1.5          # as tests/op_judge.py: room for another libm's binary64 log10, nothing else
SR = 44100


def lib_log10(xs):
    xs = np.ascontiguousarray(xs, np.float32)
    y = np.empty_like(xs)
    assert _lib.lib().nc_op_log10f(xs.ctypes.data, xs.size, y.ctypes.data) == _lib.NC_OK
    return y


def twin_metrics(x, y, cfg=None, sr=SR):
    r = quality_metrics([y], [x], sample_rate=sr, scales=cfg or QualityConfig.reference_default(), host=True)
    return {k: (v[0] if v.ndim == 1 else v[0]) for k, v in r.items()}


def regenerate():
    return R.write_bounds(lib_log10, lambda x, y: twin_metrics(x, y))


def ulps32(a, b):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / ref64.ulp32(b)


@pytest.mark.parametrize("W,H,n", [(32, 8, 17), (64, 16, 1000), (64, 64, 257), (512, 128, 3001), (2048, 512, 2500)])
def test_twin_stft_against_binary64_convolution_and_torch_stft(W, H, n):
    """Every re / im of the twin lies within ref64.conv1d_bound of the binary64 convolution with the binary64 basis (gamma(W + 1) sum
    |a b|: W chain roundings and the one rounding of the basis entry), and within the same bound of torch.stft in float64 on the padded
    signal.  torch.stft knows sin(pi) = 0 where the binary64 evaluation of the basis gives 1.2e-16: against it the bound gets the binary64
    slack of the basis itself and of the FFT, 32 x 2^-53 sum |x| over the frame (an entry is within (2 pi + 3) 2^-53 of the exact one: the
    rounded angle, cos / sin, the window; a binary64 FFT of length W <= 2048 stays within a few log2 W x 2^-53 sum |x|).
    The frame count is 1 + n // H."""
    x = R.signal(n, SR, seed=W + H)
    (got,) = stft(x, W, H, host=True)
    assert got.shape == (W // 2 + 1, 1 + n // H) and stft_frames(n, W, H) == 1 + n // H
    re, im, bre, bim = R.stft64(x, W, H)
    assert (np.abs(got.real - re) <= bre).all() and (np.abs(got.imag - im) <= bim).all()
    t = R.ref_stft(x, W, H, torch.float64).numpy()
    assert t.shape == got.shape
    xp = np.abs(R.reflect_pad(x, W).astype(np.float64))
    slack = 32 * 2.0 ** -53 * np.array([xp[f * H:f * H + W].sum() for f in range(t.shape[1])])[None, :]
    assert (np.abs(got.real - t.real) <= bre + slack).all() and (np.abs(got.imag - t.imag) <= bim + slack).all()


@pytest.mark.parametrize("W", [32, 256, 2048])
@pytest.mark.parametrize("window", ["hann", "ones"])
def test_basis_table_is_the_rounded_binary64_evaluation(W, window):
    """fl32 of the test's own binary64 evaluation; at most 1 ulp32 apart where two libms' binary64 cos / sin differ in the last place, and
    equal in at least 99 % of the entries."""
    Cb, Sb = dft_basis(W, window)
    C64, S64 = R.basis64(W, window)
    for got, want in ((Cb, C64), (Sb, S64)):
        w32 = want.astype(np.float32)
        assert (np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= ref64.ulp32(want)).all()
        assert (got == w32).mean() >= 0.99


def test_log10_against_binary64_per_decade():
    """nc_log10f on a log-spaced grid over [1e-38, 1e38], 4000 points per decade: the largest error in ulp32 of the result, per decade,
    stays within MARGIN times the recorded table (tests/golden/quality_bounds.json)."""
    table = R.bounds()["log10_ulp32_per_decade"]
    got = R.log10_errors(lib_log10)
    assert set(got) == set(table)
    for d, e in got.items():
        assert e <= MARGIN * table[d], (d, e, table[d])
    assert max(table.values()) < 2.0   # what the SI-SDR bound below relies on


@pytest.mark.parametrize("sr,M,W,fmin,fmax", [(44100, 5, 32, 0.0, None), (44100, 80, 512, 0.0, None), (44100, 150, 2048, 0.0, None),
                                              (44100, 320, 2048, 0.0, None), (16000, 40, 256, 50.0, 7000.0)])
def test_filterbank_against_binary64(sr, M, W, fmin, fmax):
    """Within 1 ulp32 + 1e-12 enorm of the independent binary64 evaluation (a breakpoint comparison flipped by the last place of hz moves
    an entry by slope x that last place); supports exact."""
    fb, lo, hi = mel_filterbank(sr, M, W, fmin, fmax)
    fb64, lo64, hi64, enorm = R.mel_filterbank64(sr, M, W, fmin, fmax)
    assert (np.abs(fb.astype(np.float64) - fb64) <= ref64.ulp32(fb64) + 1e-12 * enorm[:, None]).all()
    assert np.array_equal(lo, lo64) and np.array_equal(hi, hi64)
    outside = np.ones_like(fb, bool)
    for m in range(M):
        outside[m, lo[m]:hi[m]] = False
    assert (fb[outside] == 0).all()


def test_filterbank_against_the_reference_transcription():
    """W = 2048, 150 bands: supports at most one bin per edge from the binary32 transcription's, and |diff| / peak within 4 x the recorded
    gap between that transcription and the binary64 evaluation (the reference evaluates log10 / pow in binary32 at up to 22 kHz)."""
    fb, lo, hi = mel_filterbank(SR, 150, 2048)
    ref = R.ref_mel_filterbank(SR, 150, 2048, 0.0)
    for m in range(150):
        nz = np.nonzero(ref[m])[0]
        assert nz.size and abs(int(nz[0]) - int(lo[m])) <= 1 and abs(int(nz[-1]) + 1 - int(hi[m])) <= 1
    gap = R.bounds()["filterbank_ref_gap_over_peak"]
    assert (np.abs(fb - ref) / fb.max(axis=1, keepdims=True)).max() <= 4 * gap


def test_lowest_bands_of_80_over_512_are_empty_and_give_zero():
    fb, lo, hi = mel_filterbank(SR, 80, 512)
    assert (hi - lo == 0).any()
    x = R.signal(2000, SR, 3)
    (mel,) = mel_spectrogram(x, SR, 512, 128, 80, host=True)
    assert (mel[hi - lo == 0] == 0).all() and (mel[hi - lo > 0] > 0).any()


@pytest.mark.parametrize("row", [0, 1, 2])
def test_twin_metrics_against_binary64(row):
    """l1: the twin adds fl32|x - y| in binary64 and rounds once: 4 ulp32 covers the rounding and any summation order.
    si_sdr_db = fl(10 fl(nc_log10f(fl(ratio)))): the binary64 sums carry ~1e-13; fl(ratio) moves log10 by <= u / ln 10 = 2.6e-8, that is
    <= 0.44 ulp32 of a result >= 0.5 (the fixture's rows have 10 to 35 dB); nc_log10f <= 1.34 x MARGIN = 2.0 ulp32 (recorded table); the
    product rounds once more, 0.5: 2.95 < 4 ulp32.
    mel_mag: |twin - binary64| <= the mean of the element bounds (STFT chain gamma(W + 1), three roundings of the magnitude, the mel chain
    gamma(width + 1)) of both signals, plus the rounding of the difference and of the result.
    mel_log: the same bounds through |d log10 c^2| <= 2 dc / (c ln 10), c >= clamp_eps, plus per element nc_log10f's recorded error x
    MARGIN in ulp32 <= 2^-23 |L| of both logs, the rounding of c c (2 u / ln 10), of the difference, and of the result."""
    x, y = R.metric_fixture()[row]
    cfg = QualityConfig.reference_default()
    got = twin_metrics(x, y, cfg)
    want = R.metrics64(x, y, SR, cfg.windows, cfg.n_mels)
    assert 10.0 <= want["si_sdr_db"] <= 35.0
    assert ulps32(got["l1"], want["l1"]) <= 4
    assert ulps32(got["si_sdr_db"], want["si_sdr_db"]) <= 4
    e_log = MARGIN * max(R.bounds()["log10_ulp32_per_decade"].values()) * 2.0 ** -23
    U = ref64.U
    dist_bound = 0.0
    for i in range(2):
        b_mag = want["mel_bound_mag"][i] + 2 * U * want["mel_mag"][i]
        b_log = want["mel_bound_log"][i] + e_log * want["mel_log_abs"][i] + 2 * 2 * U / math.log(10.0) + 2 * U * want["mel_log"][i]
        assert abs(float(got["mel_mag"][i]) - want["mel_mag"][i]) <= b_mag, (i, got["mel_mag"][i], want["mel_mag"][i], b_mag)
        assert abs(float(got["mel_log"][i]) - want["mel_log"][i]) <= b_log, (i, got["mel_log"][i], want["mel_log"][i], b_log)
        dist_bound += b_mag + b_log
    assert abs(float(got["mel_distance"]) - want["mel_distance"]) <= dist_bound + U * want["mel_distance"]


def test_twin_metrics_against_the_reference_transcription():
    """The twin against L1Loss / SISDRLoss / MelSpectrogramLoss in binary32 torch: within 4 x the recorded relative difference."""
    rec = R.bounds()["twin_vs_reference_relative"]
    for x, y in R.metric_fixture():
        got, ref = twin_metrics(x, y), R.ref_metrics(x, y, SR, [2048, 512], [150, 80])
        for k, r in rec.items():
            assert abs(float(got[k]) - ref[k]) <= 4 * r * abs(ref[k]), (k, got[k], ref[k], r)


def test_identical_zero_and_non_finite_rows():
    cfg = QualityConfig([512, 64], [20, 5])
    a, b, c = R.signal(3000, SR, 1), R.signal(2000, SR, 2), R.signal(2500, SR, 4)
    z = np.zeros(1500, np.float32)
    ref = [a, z, b, c]
    est = [a.copy(), z.copy(), R.degraded(b, 5), R.degraded(c, 6)]
    base = quality_metrics(ref, est, sample_rate=SR, scales=cfg, host=True)
    # identical: l1 and every mel term are 0; errorPower = 0 leaves 10 log10(target / EPS + EPS)
    assert base["l1"][0] == 0 and (base["mel_log"][0] == 0).all() and (base["mel_mag"][0] == 0).all() and base["mel_distance"][0] == 0
    ac = a.astype(np.float64) - math.fsum(a.astype(np.float64)) / a.size
    want = 10.0 * math.log10(math.fsum(ac * ac) / R.EPS32 + R.EPS32)
    assert ulps32(base["si_sdr_db"][0], want) <= 4
    # all zero: finite (scale = EPS / EPS, ratio = EPS)
    assert all(np.isfinite(base[k][1]).all() for k in ("l1", "si_sdr_db", "mel_distance", "mel_log", "mel_mag"))
    assert ulps32(base["si_sdr_db"][1], 10.0 * math.log10(R.EPS32)) <= 4 and (base["n_bad"] == 0).all()
    # a NaN and two infinities in row 2: that row is NaN with the count, the others keep their bits
    bad = [e.copy() for e in est]
    bad[2][100] = np.nan
    rbad = [r.copy() for r in ref]
    rbad[2][7] = np.inf
    rbad[2][1999] = -np.inf
    got = quality_metrics(rbad, bad, sample_rate=SR, scales=cfg, host=True)
    assert got["n_bad"].tolist() == [0, 0, 3, 0]
    for k in ("l1", "si_sdr_db", "mel_distance", "mel_log", "mel_mag"):
        assert np.isnan(got[k][2]).all()
        for r in (0, 1, 3):
            assert np.array_equal(got[k][r], base[k][r])


def test_each_row_alone_equals_the_row_in_the_batch_on_the_host():
    cfg = QualityConfig([256], [40])
    ref = [R.signal(n, SR, n) for n in (1000, 1777)]
    est = [R.degraded(r, 1) for r in ref]
    both = quality_metrics(ref, est, sample_rate=SR, scales=cfg, host=True)
    for b in range(2):
        one = quality_metrics(ref[b:b + 1], est[b:b + 1], sample_rate=SR, scales=cfg, host=True)
        assert all(np.array_equal(one[k][0], both[k][b]) for k in both)


def _cfg(**kw):
    c = QualityConfig([64], [5]).c_struct()
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(c, k)[0] = v[0]
        else:
            setattr(c, k, v)
    return c


def test_every_refusal_of_the_host_twins():
    L = _lib.lib()
    x = np.zeros(200, np.float32)
    out = np.zeros(4096, np.float32)
    rows = np.zeros((1, quality.ROW_WORDS), np.int32)
    i64 = _lib.i64_array
    px, po, pr = x.ctypes.data, out.ctypes.data, rows.ctypes.data

    def stft_status(pcm=px, B=1, off=i64([0]), n=i64([200]), W=64, H=16, window=0, o=po, oo=i64([0])):
        return L.nc_audio_stft_host(pcm, B, off, n, W, H, window, o, oo)

    def mel_status(n=i64([200]), W=64, H=16, M=5, fmin=0.0, fmax=0.0, sr=SR, B=1):
        return L.nc_audio_mel_spectrogram_host(px, B, i64([0]), n, sr, W, H, M, fmin, fmax, po, i64([0]))

    def met_status(cfg, ref=px, est=px, n=i64([200]), B=1, o=pr, sr=SR):
        return L.nc_quality_metrics_host(ref, i64([0]), est, i64([0]), n, B, sr, C.byref(cfg) if cfg is not None else None, o)

    assert stft_status() == _lib.NC_OK and mel_status() == _lib.NC_OK and met_status(_cfg()) == _lib.NC_OK
    E = _lib.NC_EINVAL
    assert stft_status(n=i64([32])) == E and stft_status(n=i64([33])) == _lib.NC_OK          # n <= W/2
    assert mel_status(n=i64([32])) == E and met_status(_cfg(), n=i64([32])) == E
    for W in (16, 48, 4096, 0):                                                                # unadmitted W
        assert stft_status(W=W, H=8) == E and mel_status(W=W, H=8) == E and met_status(_cfg(W=(W,))) == E
    for M in (0, 513, -1):                                                                     # unadmitted n_mels
        assert mel_status(M=M) == E and met_status(_cfg(n_mels=(M,))) == E
    assert mel_status(fmin=100.0, fmax=100.0) == E and mel_status(fmin=200.0, fmax=100.0) == E  # fmax <= fmin
    assert met_status(_cfg(fmin=(100.0,), fmax=(50.0,))) == E
    assert stft_status(B=0) == E and mel_status(B=0) == E and met_status(_cfg(), B=0) == E     # B < 1
    assert stft_status(pcm=None) == E and stft_status(o=None) == E and stft_status(off=None) == E and stft_status(n=None) == E
    assert stft_status(oo=None) == E
    assert met_status(None) == E and met_status(_cfg(), ref=None) == E and met_status(_cfg(), est=None) == E and met_status(_cfg(), o=None) == E
    assert met_status(_cfg(), n=None) == E
    assert stft_status(H=0) == E and stft_status(H=65) == E and stft_status(window=2) == E
    assert met_status(_cfg(n_scales=0)) == E and met_status(_cfg(n_scales=9)) == E and met_status(_cfg(clamp_eps=0.0)) == E
    assert met_status(_cfg(), sr=0) == E
    assert L.nc_audio_mel_filterbank(SR, 5, 64, 0.0, 0.0, None, None, None) == E
    assert stft_frames(32, 64, 16) == -1 and stft_frames(33, 64, 16) == 3


def test_struct_layouts_agree_with_a_compiled_c_consumer(tmp_path):
    """nc_quality_cfg / nc_quality_row: sizeof and offsetof from a C99 program against the ctypes mirrors"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"nc_quality_cfg": _lib.NcQualityCfg, "nc_quality_row": _lib.NcQualityRow}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nc_mi355x.h"', 'int main(void) {']
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "consumer.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "consumer"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        p = ln.split()
        got[(p[0], p[1])] = int(p[2])
    for cname, ct in structs.items():
        assert got[(cname, "size")] == C.sizeof(ct)
        for fname, _ in ct._fields_:
            assert got[(cname, fname)] == getattr(ct, fname).offset, f"{cname}.{fname}"
