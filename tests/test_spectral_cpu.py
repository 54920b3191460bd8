"""CPU suite of the inverse STFT, the spectral masks and the MFCC: the serial host twins of the library (the bit judge of the kernels,
tests/test_spectral_gpu.py) held to independent binary64 -- tests/spectral_ref.py and torch.istft on complex128 -- within bounds DERIVED
from the binary32 chains (spectral_ref.istft_bound states the derivation), the refusals, the length rule, the masks against a torch
transcription of the reference's linspace compare, and the reference's DCTMatrix transcribed as written."""
import json
import os

import numpy as np
import pytest

import spectral_ref as R
from neuralcodecs_amd import _lib
from neuralcodecs_amd import spectral as S
from neuralcodecs_amd.quality import stft_packed

BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectral_bounds.json")


def _twin(X32, W, H, window, length=0):
    out, _, olens = S.istft_packed(X32.reshape(-1), W, H, window, [X32.shape[1]], None, [length], host=True)
    return out[:olens[0]].astype(np.float64)


def _c128(X32):
    return X32[..., 0].astype(np.float64) + 1j * X32[..., 1].astype(np.float64)


@pytest.mark.parametrize("case", [(32, "hann", 8), (64, "hann", 5), (64, "hann", 32), (128, "ones", 128), (256, "hann", 64), (32, "ones", 1)],
                         ids=lambda c: f"W{c[0]}-{c[1]}-H{c[2]}")
def test_twin_against_the_restatement_and_torch_istft(case):
    import torch
    W, window, H = case
    F = 21
    X32 = R.spectrum(W, F, W + H)
    for length in (0, H * (F - 1) - 3, H * (F - 1) + W // 2 - 1):
        want = R.istft64(_c128(X32), W, H, window, length)
        got = _twin(X32, W, H, window, length)
        assert got.shape == want.shape
        th = torch.istft(torch.from_numpy(_c128(X32)), W, H, window=torch.from_numpy(R.window64(W, window)), center=True,
                         length=length or None).numpy()
        assert np.abs(th - want).max() <= 1e-13 * max(1.0, np.abs(want).max())          # the restatement is torch's recipe
        bound = R.istft_bound(X32, W, H, window, length, want)
        err = np.abs(got - want)
        print(f"W={W} H={H} {window} L={length}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()
        assert np.max(err / bound) > 5e-4                                                # a bound thousands of times too wide would say nothing


def test_idft_basis_is_the_header_table():
    for W, window in ((32, "hann"), (64, "ones"), (2048, "hann")):
        T, ref = S.idft_basis(W, window), R.idft_basis64(W, window)
        assert T.shape == (W, W + 2) and (T[:, 1] == 0).all() and (T[:, W + 1] == 0).all()
        assert not np.signbit(T[:, 1]).any() and not np.signbit(T[:, W + 1]).any()
        # two libm builds may differ in the last binary64 place, which moves a binary32 rounding only next to a tie: 1 ulp, not bit for bit.
        # Entries whose exact value is 0 (cos or sin of a multiple of pi / 2) come out as ~1e-17 / W instead: far below any ulp that counts
        assert (np.abs(T.astype(np.float64) - ref) <= np.maximum(R.ulp32(ref), 1e-16)).all()


@pytest.mark.parametrize("case", [(64, "hann", 16), (64, "hann", 32), (64, "ones", 64)], ids=lambda c: f"W{c[0]}-{c[1]}-H{c[2]}")
def test_round_trip_within_the_two_derived_bounds(case):
    W, window, H = case
    n = 20 * W
    x = R.signal(n, 3 + H)
    spec, so, shapes = stft_packed(x, W, H, window, host=True)
    F = shapes[0][1]
    X32 = spec.reshape(W // 2 + 1, F, 2)
    got = _twin(X32, W, H, window, n)
    e_X = R.stft_error_bound(x, W, H, window)
    bound = R.istft_bound(X32, W, H, window, n, x.astype(np.float64), e_X)
    err = np.abs(got - x.astype(np.float64))
    print(f"W={W} H={H} {window}: max round-trip err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all() and bound.max() < 1e-4


def test_nola_refusal_writes_nothing():
    W = 64
    X32 = R.spectrum(W, 9, 1)
    canvas = np.full(1000, np.nan, np.float32)
    with pytest.raises(ValueError, match="NOLA"):
        S.istft_packed(X32.reshape(-1), W, W, "hann", [9], None, None, None, out=canvas, host=True)
    assert np.isnan(canvas).all()
    out, _, ol = S.istft_packed(X32.reshape(-1), W, W, "ones", [9], None, None, None, out=canvas, host=True)     # the same hop with w = 1 passes
    assert ol == [W * 8] and np.isfinite(out[:W * 8]).all()


def test_length_rule_and_other_refusals():
    W, H, F = 32, 8, 10
    X32 = R.spectrum(W, F, 2)
    assert S.istft_len(F, W, H) == H * (F - 1) == 72
    span = W + H * (F - 1) - W // 2
    full = _twin(X32, W, H, "hann", span + 5)
    assert full.size == span + 5 and (full[span:] == 0).all() and (full[:span] != 0).all()
    assert np.array_equal(_twin(X32, W, H, "hann", 0), full[:72]) and np.array_equal(_twin(X32, W, H, "hann", 40), full[:40])
    L, z = _lib.lib(), _lib.i64_array([0])
    out = np.zeros(200, np.float32)
    p, o = X32.ctypes.data, out.ctypes.data

    def call(B=1, off=z, frames=_lib.i64_array([F]), W_=W, H_=H, win=0, oo=z, length=z, sp=p, op=o):
        return L.nc_audio_istft_host(sp, B, off, frames, W_, H_, win, op, oo, length)

    assert call() == _lib.NC_OK and call(length=None) == _lib.NC_OK
    for bad in (dict(sp=None), dict(op=None), dict(off=None), dict(B=0), dict(B=32768), dict(off=_lib.i64_array([-1])), dict(oo=_lib.i64_array([-1])),
                dict(length=_lib.i64_array([-1])), dict(frames=_lib.i64_array([0])), dict(win=2), dict(W_=48), dict(H_=0), dict(H_=W + 1)):
        assert call(**bad) == _lib.NC_EINVAL, bad
    assert L.nc_audio_istft_len(0, W, H) == -1


def _reference_mask_1d(end, steps, lo, hi):
    """DSP.MaskFrequencies / MaskTimesteps as written: a float32 torch.linspace and fmin <= bins < fmax (AudioTensorDSP.cs:330-337, 379-386)"""
    import torch
    bins = torch.linspace(0, end, steps)
    m = (torch.tensor(lo, dtype=torch.float32) <= bins) & (bins < torch.tensor(hi, dtype=torch.float32))
    return m.numpy()


def test_mask_index_helpers_against_the_reference_transcription():
    rng = np.random.default_rng(9)
    for sr, nbins in ((44100, 1025), (16000, 33), (22051, 17), (8000, 2)):
        step = (sr // 2) / (nbins - 1)
        for _ in range(20):
            lo, hi = sorted((np.float32(rng.integers(0, nbins) + rng.uniform(0.05, 0.95)) * np.float32(step) for _ in range(2)))
            if not lo < hi:
                continue
            for b in (lo, hi):   # the bounds stay a thousandth of a bin spacing away from every bin
                assert abs(float(b) / step - round(float(b) / step)) >= 1e-3
            m = _reference_mask_1d(sr // 2, nbins, float(lo), float(hi))
            k_lo, k_hi = S.mask_freq_bins(sr, nbins, float(lo), float(hi))
            want = np.zeros(nbins, bool)
            want[k_lo:k_hi] = True
            assert np.array_equal(m, want)
    for dur, frames in ((1.0, 63), (2.5, 1000), (0.37, 2)):
        step = dur / (frames - 1)
        for _ in range(20):
            lo, hi = sorted((np.float32((rng.integers(0, frames) + rng.uniform(0.05, 0.95)) * step) for _ in range(2)))
            if not lo < hi:
                continue
            for b in (lo, hi):
                assert abs(float(b) / step - round(float(b) / step)) >= 1e-3
            m = _reference_mask_1d(np.float32(dur).item(), frames, float(lo), float(hi))
            t_lo, t_hi = S.mask_time_frames(dur, frames, float(lo), float(hi))
            want = np.zeros(frames, bool)
            want[t_lo:t_hi] = True
            assert np.array_equal(m, want)
    with pytest.raises(ValueError):
        S.mask_freq_bins(16000, 33, 500.0, 500.0)
    with pytest.raises(ValueError):
        S.mask_time_frames(1.0, 63, 0.5, 0.25)


def test_masks_fill_the_rectangle_and_keep_every_other_bit():
    W, K, fr = 32, 17, [12, 7]
    for val in (0.0, -2.5):
        buf, so = R.ragged_spectra(W, fr, 17)
        before = buf.copy()
        out = S.mask_frequencies(buf, 16000, 1000.0, 3000.0, K, fr, val, so, host=True)
        assert out is buf or np.shares_memory(out, buf)
        k_lo, k_hi = S.mask_freq_bins(16000, K, 1000.0, 3000.0)
        assert (k_lo, k_hi) == (2, 6)
        re, im = np.float32(val * np.cos(val)), np.float32(val * np.sin(val))
        touched = np.zeros(buf.size, bool)
        for b, F in enumerate(fr):
            v = buf[2 * so[b]:2 * (so[b] + K * F)].reshape(K, F, 2)
            assert (v[k_lo:k_hi, :, 0] == re).all() and (v[k_lo:k_hi, :, 1] == im).all()
            m = np.zeros((K, F, 2), bool)
            m[k_lo:k_hi] = True
            touched[2 * so[b]:2 * (so[b] + K * F)] = m.reshape(-1)
        assert np.array_equal(buf.view(np.uint32)[~touched], before.view(np.uint32)[~touched])   # unmasked bins and the gaps: bit-identical
        S.mask_timesteps(buf, 1.0, 0.25, 0.5, K, fr, val, so, host=True)
        t_lo, t_hi = S.mask_time_frames(1.0, 12, 0.25, 0.5)
        assert (buf[2 * so[0]:2 * (so[0] + K * 12)].reshape(K, 12, 2)[:, t_lo:t_hi, 0] == re).all() and t_hi > t_lo


def _logf(xs):
    xs = np.ascontiguousarray(xs, np.float32)
    y = np.empty_like(xs)
    assert _lib.lib().nc_op_logf(xs.ctypes.data, xs.size, y.ctypes.data) == _lib.NC_OK
    return y


def test_logf_stays_within_its_recorded_bound():
    """per decade of x over the positive normal binary32 range, as tests/test_quality_cpu.py measures nc_log10f"""
    rec = json.load(open(BOUNDS))["nc_logf"]
    rng = np.random.default_rng(0)
    worst = 0.0
    for d in range(-37, 38):
        xs = (10.0 ** rng.uniform(d, d + 1, 20000)).astype(np.float32)
        xs = xs[(xs >= np.float32(1.17549435e-38)) & np.isfinite(xs)]
        ref = np.log(xs.astype(np.float64))
        worst = max(worst, float(np.max(np.abs(_logf(xs).astype(np.float64) - ref) / R.ulp32(ref))))
    near = np.float32(1.0) + np.arange(-4000, 4001, dtype=np.float32) * np.float32(2.0 ** -23)
    near = near[near != 1.0]
    ref = np.log(near.astype(np.float64))
    worst = max(worst, float(np.max(np.abs(_logf(near).astype(np.float64) - ref) / R.ulp32(ref))))
    print(f"nc_logf: worst {worst:.3f} ulp (recorded bound {rec['max_ulp']})")
    assert worst <= rec["max_ulp"]
    assert _logf(np.float32([1.0]))[0] == 0.0


def test_dct_matrix_is_orthonormal_and_the_reference_as_written_returns_one_row():
    import torch
    for n_mfcc, n_mels in ((1, 1), (13, 40), (40, 80), (80, 80)):
        d = S.dct_matrix(n_mfcc, n_mels)
        assert np.abs(d.astype(np.float64) @ d.astype(np.float64).T - np.eye(n_mfcc)).max() <= 1e-6
        assert (np.abs(d.astype(np.float64) - R.dct64(n_mfcc, n_mels)) <= R.ulp32(R.dct64(n_mfcc, n_mels))).all()
    with pytest.raises(ValueError):
        S.dct_matrix(41, 40)
    # DSP.DCTMatrix as written (AudioTensorDSP.cs:901-912): ... return dctMatrix.select(0, 0).mul_(1 / sqrt(2))
    n_mfcc, n_mels = 13, 40
    mel_i, mfcc_i = torch.arange(n_mels), torch.arange(n_mfcc).unsqueeze(-1)
    m = torch.cos(mfcc_i * ((2 * mel_i) + 1) * np.pi / (2 * n_mels))
    m *= torch.sqrt(torch.tensor(2.0 / n_mels))
    as_written = m.select(0, 0).mul_(1.0 / torch.sqrt(torch.tensor(2.0)))
    assert tuple(as_written.shape) == (n_mels,)                      # ONE row, not [n_mfcc, n_mels]
    mel_t = torch.rand(7, n_mels)                                    # MFCC's `transposed`: [frames, n_mels]
    assert tuple(mel_t.matmul(as_written).shape) == (7,)             # so DSP.MFCC yields one number per frame, never n_mfcc coefficients
    assert np.allclose(as_written.numpy(), S.dct_matrix(n_mfcc, n_mels)[0], atol=1e-7)   # and that row is row 0 of the intended matrix


@pytest.mark.parametrize("n_mels", [1, 13, 40])
def test_mfcc_twin_against_float64(n_mels):
    """The derived bound per coefficient: L^ = nc_logf(fl(mel + off)) differs from ln(mel + off) by at most B ulp(L) (the recorded nc_logf
    bound) plus the rounding of the sum, u (mel + off) / (mel + off) = u, so |dL| <= B ulp(L) + u (1 + u); the chain of M fmaf on table
    entries rounded once then gives |mfcc^ - mfcc*| <= gamma_(M+1) sum_m |dct||L^| + sum_m |dct| |dL|.  mel itself is the library's
    (binary32) mel spectrogram: the definition starts from it."""
    from neuralcodecs_amd.quality import mel_spectrogram
    rec = json.load(open(BOUNDS))["nc_logf"]["max_ulp"]
    W, H, sr, off = 64, 16, 16000, np.float32(1e-6)
    x = R.signal(3000, 5)
    mel = mel_spectrogram(x, sr, W, H, n_mels, host=True)[0]
    v = (mel + off).astype(np.float32).astype(np.float64)
    Lx = np.log(v)
    for n_mfcc in sorted({1, n_mels}):
        got = S.mfcc([x], sr, W, H, n_mfcc, n_mels, log_offset=float(off), host=True)[0].astype(np.float64)
        d = R.dct64(n_mfcc, n_mels)
        want = d @ Lx
        dL = rec * R.ulp32(Lx) + R.U * (1 + R.U)
        bound = R.gamma(n_mels + 1) * (np.abs(d) @ (np.abs(Lx) + dL)) + np.abs(d) @ dL
        err = np.abs(got - want)
        print(f"n_mels={n_mels} n_mfcc={n_mfcc}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
        assert got.shape == (n_mfcc, 1 + 3000 // H) and (err <= bound).all()
