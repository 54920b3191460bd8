"""Inverse STFT, spectral masks and MFCC (include/nc_mi355x.h "inverse STFT, spectral masks, MFCC"): the reference's
DSP.InverseSTFT, DSP.MaskFrequencies, DSP.MaskTimesteps and DSP.MFCC (AudioTools/AudioTensorDSP.cs:124-151, 307-394, 408-441) on the packed
buffers of stft_packed.  numpy in, numpy out; torch device tensors in, tensors out and nothing leaves the device.  host=True runs the
serial host twin of the library instead of the kernels (no device needed): the two agree bit for bit.  A spectrogram buffer is float32
(re, im) pairs, row b complex64 [W/2+1, frames_b] at COMPLEX element offsets[b], exactly as stft_packed returns it."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .loudness import _buffer, _dev_args, _finish, _is_torch, _out_like, _ptr, _torch
from .quality import WINDOWS, stft_packed


def istft_len(frames: int, W: int, H: int) -> int:
    """nc_audio_istft_len: H (frames - 1), what torch.istft returns with center = True and no length"""
    n = int(_lib.lib().nc_audio_istft_len(int(frames), int(W), int(H)))
    if n < 0:
        raise ValueError(f"istft_len({frames}, {W}, {H}): at least one frame, W >= 2 and H >= 1")
    return n


def idft_basis(W: int, window: str = "hann") -> np.ndarray:
    """nc_audio_idft_basis: the windowed synthesis basis T, float32 [W, W + 2]"""
    T = np.empty((W, W + 2), np.float32)
    _lib.check(_lib.lib().nc_audio_idft_basis(int(W), WINDOWS[window], T.ctypes.data))
    return T


def dct_matrix(n_mfcc: int, n_mels: int) -> np.ndarray:
    """nc_audio_dct_matrix: the orthonormal DCT-II, float32 [n_mfcc, n_mels]"""
    if n_mfcc < 1 or n_mels < 1:
        raise ValueError("n_mfcc and n_mels must be positive")
    d = np.empty((n_mfcc, n_mels), np.float32)
    _lib.check(_lib.lib().nc_audio_dct_matrix(int(n_mfcc), int(n_mels), d.ctypes.data))
    return d


def istft_workspace(set_bytes: int = 0, device_index: int = 0) -> int:
    """nc_audio_istft_workspace: the cap in bytes on the frame scratch of one group of rows; set_bytes > 0 sets it, -1 restores the default"""
    cap = C.c_int64()
    _lib.check(_lib.lib().nc_audio_istft_workspace(int(device_index), int(set_bytes), C.byref(cap)))
    return int(cap.value)


def mask_freq_bins(sample_rate: int, nbins: int, fmin_hz: float, fmax_hz: float):
    """nc_audio_mask_freq_bins: the bins [k_lo, k_hi) that DSP.MaskFrequencies masks"""
    lo, hi = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().nc_audio_mask_freq_bins(int(sample_rate), int(nbins), float(fmin_hz), float(fmax_hz), C.byref(lo), C.byref(hi)))
    return int(lo.value), int(hi.value)


def mask_time_frames(duration: float, frames: int, tmin_s: float, tmax_s: float):
    """nc_audio_mask_time_frames: the frames [t_lo, t_hi) that DSP.MaskTimesteps masks"""
    lo, hi = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().nc_audio_mask_time_frames(float(duration), int(frames), float(tmin_s), float(tmax_s), C.byref(lo), C.byref(hi)))
    return int(lo.value), int(hi.value)


def _spec_rows(spec, frames, offsets, nbins: int, what: str):
    fr = [int(v) for v in frames]
    offs = [int(v) for v in offsets] if offsets is not None else np.concatenate([[0], np.cumsum([nbins * f for f in fr])[:-1]]).astype(np.int64).tolist()
    if len(offs) != len(fr) or not fr:
        raise ValueError(f"{what}: one offset per row, at least one row")
    if any(o < 0 for o in offs) or any(f < 1 for f in fr):
        raise ValueError(f"{what}: negative offset or a row without frames")
    if 2 * max(o + nbins * f for o, f in zip(offs, fr)) > int(spec.shape[0]):
        raise ValueError(f"{what}: a row reaches past the end of the buffer")
    return fr, offs


def istft_packed(spec, W: int, H: Optional[int] = None, window: str = "hann", frames=None, offsets=None, lengths=None, out_offsets=None, out=None,
                 host: bool = False):
    """nc_audio_istft_dev / _host on a packed spectrogram buffer -> (out buffer, out_offsets, out lengths).  lengths: samples per row, 0 or
    None for H (frames - 1).  Defaults: the rows end to end in `spec`, the results end to end in a fresh buffer; `out`: write into this
    buffer."""
    W = int(W)
    H = int(H) if H else W // 4
    b, was_torch = _buffer(spec, host)
    fr, offs = _spec_rows(b, frames, offsets, W // 2 + 1, "istft")
    want = [int(v) for v in lengths] if lengths is not None else [0] * len(fr)
    if len(want) != len(fr) or any(n < 0 for n in want):
        raise ValueError("istft: one length per row, none negative")
    olens = [n if n else istft_len(f, W, H) for n, f in zip(want, fr)]
    oo = [int(v) for v in out_offsets] if out_offsets is not None else np.concatenate([[0], np.cumsum(olens)[:-1]]).astype(np.int64).tolist()
    if len(oo) != len(fr):
        raise ValueError("istft: one output offset per row")
    need = max([o + n for o, n in zip(oo, olens)] + [1])
    if out is None:
        out = _out_like(b, need)
    else:
        if _is_torch(out) != _is_torch(b):
            raise ValueError("istft: `out` must live where the call runs")
        if out.ndim != 1 or int(out.shape[0]) < need or (_is_torch(out) and (out.dtype != _torch().float32 or not out.is_contiguous())) or \
                (not _is_torch(out) and (out.dtype != np.float32 or not out.flags.c_contiguous)):
            raise ValueError("istft: `out` must be a contiguous 1-D float32 buffer that holds every output row")
    L = _lib.lib()
    args = (_ptr(b), len(fr), _lib.i64_array(offs), _lib.i64_array(fr), W, H, WINDOWS[window], _ptr(out), _lib.i64_array(oo), _lib.i64_array(want))
    if host:
        _lib.check(L.nc_audio_istft_host(*args))
        return out, oo, olens
    dev, stream = _dev_args(b)
    _lib.check(L.nc_audio_istft_dev(dev, *args, stream))
    return _finish(b, was_torch, out)[0], oo, olens


def istft(specs, W: int, H: Optional[int] = None, window: str = "hann", lengths=None, host: bool = False):
    """DSP.InverseSTFT (center = true): a list of complex [W/2+1, frames_b] arrays / tensors (what stft returns) -> a list of float32 rows"""
    if len(specs) == 0:
        raise ValueError("the list of spectrograms must not be empty")
    if any(s.ndim != 2 or int(s.shape[0]) != W // 2 + 1 for s in specs):
        raise ValueError(f"every spectrogram must be [{W // 2 + 1}, frames]")
    fr = [int(s.shape[1]) for s in specs]
    if _is_torch(specs[0]):
        torch = _torch()
        flat = torch.cat([torch.view_as_real(s.to(torch.complex64).contiguous()).reshape(-1) for s in specs])
    else:
        flat = np.concatenate([np.ascontiguousarray(np.asarray(s, np.complex64)).view(np.float32).reshape(-1) for s in specs])
    out, oo, olens = istft_packed(flat, W, H, window, fr, None, lengths, None, None, host)
    return [out[o:o + n] for o, n in zip(oo, olens)]


def spec_fill_packed(spec, nbins: int, frames, k_lo, k_hi, t_lo, t_hi, val: float = 0.0, offsets=None, host: bool = False):
    """nc_audio_spec_fill_dev / _host IN PLACE on a packed spectrogram buffer: row b's rectangle [k_lo, k_hi) x [t_lo, t_hi) becomes
    val exp(i val).  A device tensor or (host=True) a contiguous float32 numpy buffer is written where it lies and returned; any other
    input is converted first and the converted buffer returned."""
    b, was_torch = _buffer(spec, host)
    fr, offs = _spec_rows(b, frames, offsets, int(nbins), "spec_fill")
    B = len(fr)
    kl, kh = (C.c_int32 * B)(*[int(v) for v in k_lo]), (C.c_int32 * B)(*[int(v) for v in k_hi])
    args = (_ptr(b), B, _lib.i64_array(offs), _lib.i64_array(fr), int(nbins), kl, kh, _lib.i64_array(t_lo), _lib.i64_array(t_hi), float(val))
    L = _lib.lib()
    if host:
        _lib.check(L.nc_audio_spec_fill_host(*args))
        return b
    dev, stream = _dev_args(b)
    _lib.check(L.nc_audio_spec_fill_dev(dev, *args, stream))
    return _finish(b, was_torch, b)[0]


def _mask(spec, frames, offsets, nbins, rects, val, host):
    """rects: per row (k_lo, k_hi, t_lo, t_hi)"""
    k_lo, k_hi, t_lo, t_hi = zip(*rects)
    return spec_fill_packed(spec, nbins, frames, k_lo, k_hi, t_lo, t_hi, val, offsets, host)


def mask_frequencies(spec, sample_rate: int, fmin_hz, fmax_hz, nbins: int, frames, val: float = 0.0, offsets=None, host: bool = False):
    """DSP.MaskFrequencies on a packed buffer, in place: per row the bins with fmin_hz[b] <= bin_hz < fmax_hz[b] (scalars: every row)"""
    fr = [int(v) for v in frames]
    lo = [float(fmin_hz)] * len(fr) if np.ndim(fmin_hz) == 0 else [float(v) for v in fmin_hz]
    hi = [float(fmax_hz)] * len(fr) if np.ndim(fmax_hz) == 0 else [float(v) for v in fmax_hz]
    rects = [mask_freq_bins(sample_rate, nbins, a, b) + (0, f) for a, b, f in zip(lo, hi, fr)]
    return _mask(spec, fr, offsets, int(nbins), rects, val, host)


def mask_timesteps(spec, duration, tmin_s, tmax_s, nbins: int, frames, val: float = 0.0, offsets=None, host: bool = False):
    """DSP.MaskTimesteps on a packed buffer, in place: per row the frames with tmin_s[b] <= bin_t < tmax_s[b]; duration per row or one"""
    fr = [int(v) for v in frames]
    du = [float(duration)] * len(fr) if np.ndim(duration) == 0 else [float(v) for v in duration]
    lo = [float(tmin_s)] * len(fr) if np.ndim(tmin_s) == 0 else [float(v) for v in tmin_s]
    hi = [float(tmax_s)] * len(fr) if np.ndim(tmax_s) == 0 else [float(v) for v in tmax_s]
    rects = [(0, int(nbins)) + mask_time_frames(d, f, a, b) for d, a, b, f in zip(du, lo, hi, fr)]
    return _mask(spec, fr, offsets, int(nbins), rects, val, host)


def mfcc_packed(x, sample_rate: int, W: int = 2048, H: Optional[int] = None, n_mfcc: int = 40, n_mels: int = 80, fmin: float = 0.0,
                fmax: Optional[float] = None, log_offset: float = 1e-6, lengths=None, offsets=None, out_offsets=None, host: bool = False):
    """nc_audio_mfcc_dev / _host on a packed PCM buffer: (float32 buffer, out_offsets, shapes); row b is [n_mfcc, frames_b]"""
    W = int(W)
    H = int(H) if H else W // 4
    b, was_torch = _buffer(x, host)
    lens = [int(v) for v in lengths] if lengths is not None else [int(b.shape[0])]
    offs = [int(v) for v in offsets] if offsets is not None else np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64).tolist()
    if len(offs) != len(lens) or any(o < 0 for o in offs) or max(o + n for o, n in zip(offs, lens)) > int(b.shape[0]):
        raise ValueError("mfcc: one offset per row, every row within the buffer")
    if min(lens) <= W // 2:
        raise ValueError(f"every row needs more than {W // 2} samples (reflect padding)")
    frames = [1 + n // H for n in lens]
    sizes = [int(n_mfcc) * f for f in frames]
    oo = [int(v) for v in out_offsets] if out_offsets is not None else np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64).tolist()
    out = _out_like(b, max(o + s for o, s in zip(oo, sizes)))
    L = _lib.lib()
    args = (_ptr(b), len(lens), _lib.i64_array(offs), _lib.i64_array(lens), int(sample_rate), W, H, int(n_mels), float(fmin), float(fmax or 0.0),
            int(n_mfcc), float(log_offset), _ptr(out), _lib.i64_array(oo))
    shapes = [(int(n_mfcc), f) for f in frames]
    if host:
        _lib.check(L.nc_audio_mfcc_host(*args))
        return out, oo, shapes
    dev, stream = _dev_args(b)
    _lib.check(L.nc_audio_mfcc_dev(dev, *args, stream))
    return _finish(b, was_torch, out)[0], oo, shapes


def mfcc(rows, sample_rate: int, W: int = 2048, H: Optional[int] = None, n_mfcc: int = 40, n_mels: int = 80, fmin: float = 0.0,
         fmax: Optional[float] = None, log_offset: float = 1e-6, host: bool = False):
    """DSP.MFCC (hann window): a list of 1-D rows -> a list of float32 [n_mfcc, frames_b]"""
    if len(rows) == 0 or any(r.ndim != 1 for r in rows):
        raise ValueError("a non-empty list of 1-D rows")
    lens = [int(r.shape[0]) for r in rows]
    if _is_torch(rows[0]):
        flat = _torch().cat([r.to(_torch().float32) for r in rows])
    else:
        flat = np.concatenate([np.asarray(r, np.float32) for r in rows])
    out, oo, shapes = mfcc_packed(flat, sample_rate, W, H, n_mfcc, n_mels, fmin, fmax, log_offset, lens, None, None, host)
    return [out[o:o + c * f].reshape(c, f) for o, (c, f) in zip(oo, shapes)]


def spectral_mask(x, sample_rate: int, W: int, H: Optional[int] = None, bands: Sequence = (), spans: Sequence = (), lengths=None, offsets=None,
                  window: str = "hann", val: float = 0.0, host: bool = False):
    """stft -> fill -> istft on packed buffers: every row of the packed PCM buffer `x` with the frequency bands [(fmin_hz, fmax_hz), ...] and
    the time spans [(tmin_s, tmax_s), ...] set to val exp(i val), back at its own length -> (out buffer, out_offsets, lengths).  A row's
    duration is its length / sample_rate.  The spectrogram never leaves the device."""
    W = int(W)
    H = int(H) if H else W // 4
    b, was_torch = _buffer(x, host)
    lens = [int(v) for v in lengths] if lengths is not None else [int(b.shape[0])]
    offs = [int(v) for v in offsets] if offsets is not None else np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64).tolist()
    spec, so, shapes = stft_packed(b, W, H, window, lens, offs, None, host)
    nbins, fr = W // 2 + 1, [f for _, f in shapes]
    for lo, hi in bands:
        spec = mask_frequencies(spec, sample_rate, lo, hi, nbins, fr, val, so, host)
    for lo, hi in spans:
        spec = mask_timesteps(spec, [n / float(sample_rate) for n in lens], lo, hi, nbins, fr, val, so, host)
    out, oo, olens = istft_packed(spec, W, H, window, fr, so, lens, offs, None, host)
    return _finish(b, was_torch, out)[0], oo, olens
