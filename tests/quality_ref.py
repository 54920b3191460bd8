"""Judges of the round-trip quality tests (tests/test_quality_cpu.py, tests/test_quality_gpu.py).  Nothing here is code under test and
nothing is shared with the library:

  * the "meaning": torch-CPU transcriptions of the reference members the library replaces -- DSP.STFT, DSP.MelFilterbank with HertzToMel /
    MelToHertz, DSP.MelSpectrogram (AudioTools/AudioTensorDSP.cs:595-894, Utils/AudioExtensions.cs:31-44), L1Loss, SISDRLoss.forward
    (Modules/DAC/SISDRLoss.cs:100-164) and MelSpectrogramLoss.forward (MelSpectrogramLoss.cs:116-137), in the reference's binary32;
  * an independent binary64 evaluation of every formula include/nc_mi355x.h states ("round-trip quality");
  * write_bounds(): the measured tables of tests/golden/quality_bounds.json.
"""
import json
import math
import os

import numpy as np
import torch

import ref64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quality_bounds.json")
EPS32 = float(np.float32(1e-8))


# ------------------------------------------------------------------------------------------------------------------ binary64 formulas
def basis64(W, window="hann"):
    """C, S [W/2+1, W] in binary64: w(n) cos / -w(n) sin of 2 pi ((k n) mod W) / W"""
    n = np.arange(W)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / W) if window == "hann" else np.ones(W)
    k = np.arange(W // 2 + 1)[:, None]
    ang = 2.0 * np.pi * ((k * n[None, :]) % W) / W
    return w[None, :] * np.cos(ang), -w[None, :] * np.sin(ang)


def reflect_pad(x, W):
    return np.pad(np.asarray(x), (W // 2, W // 2), mode="reflect")


def stft64(x, W, H, window="hann"):
    """(re, im) [W/2+1, F] in binary64 and the derived element bound of a binary32 chain: the binary64 basis as a [2(W/2+1), 1, W]
    conv1d weight with stride H on the reflect-padded signal (ref64.conv1d / ref64.conv1d_bound)."""
    C, S = basis64(W, window)
    w = np.concatenate([C, S])[:, None, :]
    xp = reflect_pad(np.asarray(x, np.float32), W)[None, None, :]
    y = ref64.conv1d(xp, w, stride=H)[0]
    bound = ref64.conv1d_bound(xp, w, stride=H)[0]
    K = W // 2 + 1
    return y[:K], y[K:], bound[:K], bound[K:]


def mel_filterbank64(sample_rate, n_mels, n_fft, fmin=0.0, fmax=None):
    """fb [n_mels, n_fft/2+1] binary64, lo, hi, enorm: HTK mel, half-open triangles, 2 / (hz[i+2] - hz[i])"""
    fmax = sample_rate / 2.0 if fmax is None else float(np.float32(fmax))
    fmin = float(np.float32(fmin))
    K = n_fft // 2 + 1
    freq = np.array([(j * sample_rate) / (2 * (K - 1)) for j in range(K)], np.float64)
    m0, m1 = 2595.0 * math.log10(1.0 + fmin / 700.0), 2595.0 * math.log10(1.0 + fmax / 700.0)
    hz = np.array([700.0 * (math.pow(10.0, (m0 + (m1 - m0) * i / (n_mels + 1)) / 2595.0) - 1.0) for i in range(n_mels + 2)])
    fb = np.zeros((n_mels, K))
    lo, hi = np.zeros(n_mels, np.int32), np.zeros(n_mels, np.int32)
    enorm = 2.0 / (hz[2:] - hz[:-2])
    for i in range(n_mels):
        l, c, r = hz[i], hz[i + 1], hz[i + 2]
        up = (freq >= l) & (freq < c)
        dn = (freq >= c) & (freq < r)
        fb[i, up] = (freq[up] - l) / (c - l)
        fb[i, dn] = (r - freq[dn]) / (r - c)
        fb[i] *= enorm[i]
        inside = np.nonzero(up | dn)[0]
        if inside.size:
            lo[i], hi[i] = inside[0], inside[-1] + 1
    return fb, lo, hi, enorm


def metrics64(x, y, sample_rate, windows, n_mels, hops=None, clamp_eps=1e-5, log_weight=1.0, mag_weight=1.0, fmin=None, fmax=None):
    """One row in binary64 (math.fsum for every sum): l1, si_sdr_db, mel_mag[i], mel_log[i], mel_distance, and per scale the bound of the
    binary32 mel values (chain of W + 1 roundings through a chain over the band's bins) that the tests propagate."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.size
    l1 = math.fsum(np.abs(np.float32(x) - np.float32(y)).astype(np.float64)) / n     # fl(x - y) is part of the definition
    xc, yc = x - math.fsum(x) / n, y - math.fsum(y) / n
    syy, sxy = math.fsum(yc * yc), math.fsum(xc * yc)
    scale = (sxy + EPS32) / (syy + EPS32)
    target, error = scale * scale * syy, math.fsum((xc - scale * yc) ** 2)
    ratio = min(target / (error + EPS32) + EPS32, float(np.finfo(np.float32).max))
    out = {"l1": l1, "si_sdr_db": 10.0 * math.log10(ratio), "ratio": ratio, "mel_mag": [], "mel_log": [], "mel_bound_mag": [], "mel_bound_log": []}
    dist = 0.0
    ce = float(np.float32(clamp_eps))
    for i, (W, M) in enumerate(zip(windows, n_mels)):
        H = hops[i] if hops else W // 4
        fb, lo, hi, _ = mel_filterbank64(sample_rate, M, W, 0.0 if fmin is None else fmin[i], None if fmax is None else fmax[i])
        mels, bounds = [], []
        for sig in (x, y):
            re, im, bre, bim = stft64(sig.astype(np.float32), W, H)
            mag = np.sqrt(re * re + im * im)
            # |fl chain - exact| of a magnitude: the two chain bounds through the root (1-Lipschitz in (re, im)) plus 3 roundings
            bmag = np.sqrt(bre * bre + bim * bim) + 3 * ref64.U * mag
            width = int((hi - lo).max())
            mels.append(fb @ mag)
            bounds.append(fb @ bmag + ref64.gamma(width + 1) * (fb @ mag))
        X, Y = mels
        bX, bY = bounds
        cnt = X.size
        mag_mean = math.fsum(np.abs(X - Y).ravel()) / cnt
        LX, LY = np.log10(np.maximum(X, ce) ** 2), np.log10(np.maximum(Y, ce) ** 2)
        log_mean = math.fsum(np.abs(LX - LY).ravel()) / cnt
        out["mel_mag"].append(mag_mean)
        out["mel_log"].append(log_mean)
        out["mel_bound_mag"].append(math.fsum((bX + bY + ref64.U * np.abs(X - Y)).ravel()) / cnt)
        # d log10(c^2) = 2 dc / (c ln 10) <= 2 dc / (max(c - dc, clamp) ln 10); nc_log10f's own error and the roundings of c c and of the
        # difference come on top (added by the test from the measured log10 table)
        dl = lambda v, b: 2.0 * b / (np.maximum(np.maximum(v, ce) - b, ce) * math.log(10.0))
        out["mel_bound_log"].append(math.fsum((dl(X, bX) + dl(Y, bY)).ravel()) / cnt)
        out.setdefault("mel_log_abs", []).append(math.fsum((np.abs(LX) + np.abs(LY)).ravel()) / cnt)
        dist += log_weight * log_mean + mag_weight * mag_mean
    out["mel_distance"] = dist
    return out


# ------------------------------------------------------------------------------------------------------------------ transcriptions
def ref_hertz_to_mel(hz):
    return 2595.0 * torch.log10(1.0 + hz / 700.0)                         # AudioExtensions.cs:33


def ref_mel_to_hertz(mel):
    return 700.0 * (torch.pow(10.0, mel / 2595.0) - 1.0)                  # AudioExtensions.cs:43


def ref_mel_filterbank(sample_rate, n_mels, n_fft, fmin, fmax=None):
    """AudioTensorDSP.cs:844-894 in binary32, statement by statement"""
    fmax = sample_rate / 2.0 if fmax is None else fmax
    fft_freqs = torch.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1, dtype=torch.float32)
    mels = ref_hertz_to_mel(torch.tensor([fmin, fmax], dtype=torch.float32))
    mel_points = torch.linspace(mels[0].item(), mels[1].item(), n_mels + 2, dtype=torch.float32)
    hz = ref_mel_to_hertz(mel_points)
    fb = torch.zeros(n_mels, n_fft // 2 + 1, dtype=torch.float32)
    f = fft_freqs
    for i in range(n_mels):
        l, c, r = hz[i], hz[i + 1], hz[i + 2]
        row = torch.zeros_like(f)
        up = (f >= l) & (f < c)
        dn = (f >= c) & (f < r)
        row[up] = (f[up] - l) / (c - l)
        row[dn] = (r - f[dn]) / (r - c)
        fb[i] = row
    enorm = 2.0 / (hz[2:] - hz[:-2])
    return (fb * enorm.unsqueeze(1)).numpy()


def ref_stft(x, W, H, dtype=torch.float32):
    """AudioTensorDSP.cs:716-809 on one row: reflect padding of W/2, torch.stft(center=False, hann) -> complex [W/2+1, F]"""
    a = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape(1, 1, -1)
    p = torch.nn.functional.pad(a, (W // 2, W // 2), mode="reflect").reshape(1, -1)
    return torch.stft(p, n_fft=W, hop_length=H, window=torch.hann_window(W, dtype=dtype), center=False, return_complex=True)[0]


def ref_mel_spectrogram(x, sample_rate, n_mels, W, H, fmin=0.0, fmax=None):
    """AudioTensorDSP.cs:595-669 with n_fft = W (the one deviation: the reference's max(W, 2048) table cannot be multiplied for W < 2048)"""
    mag = ref_stft(x, W, H).abs()
    fb = torch.from_numpy(ref_mel_filterbank(sample_rate, n_mels, W, fmin, fmax))
    return mag.transpose(0, 1).matmul(fb.t()).transpose(0, 1)


def ref_metrics(x, y, sample_rate, windows, n_mels, clamp_eps=1e-5, log_weight=1.0, mag_weight=1.0):
    """L1Loss, -SISDRLoss.forward (scaling, zeroMean, reduction none) and MelSpectrogramLoss.forward on one row, binary32 torch"""
    xt, yt = torch.from_numpy(np.ascontiguousarray(x)).float(), torch.from_numpy(np.ascontiguousarray(y)).float()
    out = {"l1": torch.nn.functional.l1_loss(xt, yt).item()}
    refs, ests = yt.reshape(1, -1, 1).clone(), xt.reshape(1, -1, 1).clone()
    refs -= refs.mean(dim=1, keepdim=True)
    ests -= ests.mean(dim=1, keepdim=True)
    ref_pow = (refs * refs).sum(-2) + 1e-8
    cross = (ests * refs).sum(-2) + 1e-8
    scale = (cross / ref_pow).unsqueeze(1)
    target = scale * refs
    err = ests - target
    tp, ep = (target * target).sum(1), (err * err).sum(1)
    out["si_sdr_db"] = (10 * torch.log10(tp / (ep + 1e-8) + 1e-8)).item()
    out["mel_mag"], out["mel_log"], dist = [], [], 0.0
    for W, M in zip(windows, n_mels):
        X, Y = ref_mel_spectrogram(x, sample_rate, M, W, W // 4), ref_mel_spectrogram(y, sample_rate, M, W, W // 4)
        lg = torch.nn.functional.l1_loss(X.clamp(clamp_eps).pow(2.0).log10(), Y.clamp(clamp_eps).pow(2.0).log10()).item()
        mg = torch.nn.functional.l1_loss(X, Y).item()
        out["mel_log"].append(lg)
        out["mel_mag"].append(mg)
        dist += log_weight * lg + mag_weight * mg
    out["mel_distance"] = dist
    return out


# ------------------------------------------------------------------------------------------------------------------ fixtures and tables
def signal(n, sample_rate, seed, noise=0.05):
    """a few partials and a little noise, binary32, |x| < 1"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sample_rate
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.4, 0.25, 0.1), rng.uniform(80, 0.4 * sample_rate, 3), rng.uniform(0, 6, 3)))
    return (x + noise * rng.standard_normal(n)).astype(np.float32)


def degraded(x, seed, snr_db=20.0):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(x.size)
    e *= np.sqrt(np.mean(x.astype(np.float64) ** 2) / np.mean(e ** 2)) * 10 ** (-snr_db / 20)
    return (0.9 * x + e).astype(np.float32)


def log10_grid(per_decade=4000):
    """log-spaced binary32 inputs over [1e-38, 1e38] with their decades"""
    xs, decs = [], []
    for d in range(-38, 38):
        g = np.float32(10.0 ** (d + np.arange(per_decade) / per_decade))
        g = g[(g >= np.float32(1.1754944e-38))]
        xs.append(g)
        decs.append(np.full(g.size, d))
    return np.concatenate(xs), np.concatenate(decs)


def log10_errors(f32_log10):
    """largest error of f32_log10 (a function on binary32 arrays) in ulp32 of the result, per decade of the argument"""
    xs, decs = log10_grid()
    got = np.asarray(f32_log10(xs), np.float64)
    want = np.log10(xs.astype(np.float64))
    err = np.abs(got - want) / ref64.ulp32(want)
    return {str(d): float(err[decs == d].max()) for d in range(-38, 38)}


def filterbank_ref_gap(sample_rate=44100, n_mels=150, n_fft=2048):
    """largest |binary32 transcription - binary64 evaluation| / filter peak: neither is code under test"""
    fb64, _, _, _ = mel_filterbank64(sample_rate, n_mels, n_fft)
    fb32 = ref_mel_filterbank(sample_rate, n_mels, n_fft, 0.0).astype(np.float64)
    peak = fb64.max(axis=1, keepdims=True)
    return float((np.abs(fb32 - fb64) / peak).max())


def metric_fixture(sample_rate=44100):
    rows = []
    for b, n in enumerate((3000, 4111, 6000)):
        y = signal(n, sample_rate, 100 + b)
        rows.append((degraded(y, 200 + b, (12.0, 20.0, 30.0)[b]), y))
    return rows


def write_bounds(f32_log10, twin_metrics):
    """tests/golden/quality_bounds.json: `f32_log10` evaluates the library's nc_log10f on an array, `twin_metrics(x, y)` the host twin with
    QualityConfig.reference_default().  Run by hand when the canonical arithmetic changes:
        python -c "import sys; sys.path[:0] = ['tests', '.']; import test_quality_cpu as t; t.regenerate()" """
    twin_gap = {k: 2.0 ** -23 for k in ("l1", "si_sdr_db", "mel_distance")}   # two binary32 results: never held closer than one ulp32
    for x, y in metric_fixture():
        got, ref = twin_metrics(x, y), ref_metrics(x, y, 44100, [2048, 512], [150, 80])
        for k in twin_gap:
            twin_gap[k] = max(twin_gap[k], abs(float(got[k]) - ref[k]) / abs(ref[k]))
    doc = {"log10_ulp32_per_decade": log10_errors(f32_log10), "filterbank_ref_gap_over_peak": filterbank_ref_gap(),
           "twin_vs_reference_relative": twin_gap}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc


def bounds():
    with open(GOLDEN) as f:
        return json.load(f)
