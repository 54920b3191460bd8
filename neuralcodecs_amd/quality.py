"""Round-trip quality (include/nc_mi355x.h "round-trip quality"): STFT, mel spectrogram and the per-row metrics L1, SI-SDR
and multi-scale mel distance -- the reference's DSP.STFT / DSP.MelSpectrogram (AudioTools/AudioTensorDSP.cs:595-894) and L1Loss, SISDRLoss,
MelSpectrogramLoss (Modules/DAC/) as evaluation metrics.  numpy in, numpy out; torch device tensors in, tensors out and nothing leaves the
device.  host=True runs the serial host twin of the library instead of the kernels (no device needed): the two agree bit for bit."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib

WINDOWS = {"hann": _lib.NC_WINDOW_HANN, "ones": _lib.NC_WINDOW_ONES}
ROW_WORDS = C.sizeof(_lib.NcQualityRow) // 4


@dataclass
class QualityConfig:
    """nc_quality_cfg: the scales of the mel distance.  hops None: W / 4 each; fmax None: sample_rate / 2."""
    windows: Sequence[int]
    n_mels: Sequence[int]
    hops: Optional[Sequence[int]] = None
    fmin: Optional[Sequence[float]] = None
    fmax: Optional[Sequence[Optional[float]]] = None
    clamp_eps: float = 1e-5
    log_weight: float = 1.0
    mag_weight: float = 1.0

    @classmethod
    def dac_eval(cls):
        """the DAC paper's evaluation set: windows 32 ... 2048, 5 ... 320 mel bands"""
        return cls([32, 64, 128, 256, 512, 1024, 2048], [5, 10, 20, 40, 80, 160, 320])

    @classmethod
    def reference_default(cls):
        """the constructor defaults of MelSpectrogramLoss (MelSpectrogramLoss.cs:44-45)"""
        return cls([2048, 512], [150, 80])

    def c_struct(self) -> "_lib.NcQualityCfg":
        S = len(self.windows)
        if not 1 <= S <= 8 or len(self.n_mels) != S:
            raise ValueError("1 to 8 scales, one n_mels per window")
        c = _lib.NcQualityCfg()
        c.n_scales = S
        for i in range(S):
            c.W[i], c.n_mels[i] = int(self.windows[i]), int(self.n_mels[i])
            c.H[i] = int(self.hops[i]) if self.hops is not None else 0
            c.fmin[i] = float(self.fmin[i]) if self.fmin is not None else 0.0
            c.fmax[i] = float(self.fmax[i]) if self.fmax is not None and self.fmax[i] is not None else 0.0
        c.clamp_eps, c.log_weight, c.mag_weight = float(self.clamp_eps), float(self.log_weight), float(self.mag_weight)
        return c


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _torch():
    import torch
    return torch


def stft_frames(n: int, W: int, H: int) -> int:
    """nc_audio_stft_frames: 1 + n // H, or -1 where n <= W / 2"""
    return int(_lib.lib().nc_audio_stft_frames(int(n), int(W), int(H)))


def dft_basis(W: int, window: str = "hann"):
    """nc_audio_dft_basis: the windowed DFT basis (C, S), float32 [W/2+1, W] each"""
    Cb, Sb = np.empty((W // 2 + 1, W), np.float32), np.empty((W // 2 + 1, W), np.float32)
    _lib.check(_lib.lib().nc_audio_dft_basis(int(W), WINDOWS[window], Cb.ctypes.data, Sb.ctypes.data))
    return Cb, Sb


def mel_filterbank(sample_rate: int, n_mels: int, n_fft: int, fmin: float = 0.0, fmax: Optional[float] = None):
    """nc_audio_mel_filterbank: (fb float32 [n_mels, n_fft/2+1], lo, hi int32 [n_mels]); band m is non-zero inside bins [lo[m], hi[m])"""
    if n_mels < 1 or n_fft < 2:
        raise ValueError("n_mels and n_fft must be positive")
    fb = np.empty((n_mels, n_fft // 2 + 1), np.float32)
    lo, hi = np.empty(n_mels, np.int32), np.empty(n_mels, np.int32)
    _lib.check(_lib.lib().nc_audio_mel_filterbank(int(sample_rate), int(n_mels), int(n_fft), float(fmin), float(fmax or 0.0), fb.ctypes.data,
                                                  lo.ctypes.data, hi.ctypes.data))
    return fb, lo, hi


def _rows_of(x, lengths, offsets):
    """x: a list of 1-D rows, a [B, T] array, one 1-D row, or a packed 1-D buffer with lengths (and element offsets) -> (buffer, offsets, lengths,
    is_torch).  Rows that are device tensors are addressed where they lie, relative to the lowest address: nothing is copied."""
    if isinstance(x, (list, tuple)):
        if len(x) == 0:
            raise ValueError("the list of rows must not be empty")
        if any(r.ndim != 1 for r in x):
            raise ValueError("every row must be 1-D")
        lens = [int(r.shape[0]) for r in x]
        if _is_torch(x[0]):
            torch = _torch()
            rows = [r if (r.dtype == torch.float32 and r.is_contiguous() and r.is_cuda) else r.to(torch.float32).contiguous().cuda() for r in x]
            base = min(rows, key=lambda r: r.data_ptr())
            return (base, rows), [(r.data_ptr() - base.data_ptr()) // 4 for r in rows], lens, True
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
        return np.ascontiguousarray(np.concatenate([np.asarray(r, np.float32) for r in x])), offs, lens, False
    if x.ndim == 2 and lengths is None:
        B, T = int(x.shape[0]), int(x.shape[1])
        lengths, offsets = [T] * B, [b * T for b in range(B)]
    if x.ndim == 1 and lengths is None:
        lengths = [int(x.shape[0])]
    if lengths is None:
        raise ValueError("a packed buffer needs lengths")
    lens = [int(v) for v in lengths]
    offs = [int(v) for v in offsets] if offsets is not None else np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    if _is_torch(x):
        torch = _torch()
        flat = x.reshape(-1).to(torch.float32).contiguous()
        flat = flat if flat.is_cuda else flat.cuda()
        need = max(o + n for o, n in zip(offs, lens))
        if need > flat.numel():
            raise ValueError("a row reaches past the end of the buffer")
        return (flat, [flat]), offs, lens, True
    flat = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
    if max(o + n for o, n in zip(offs, lens)) > flat.size:
        raise ValueError("a row reaches past the end of the buffer")
    return flat, offs, lens, False


def _spectra(kind, x, lengths, offsets, out_offsets, host, W, H, tail):
    """kind 'stft' or 'mel': the packed output buffer and its per-row offsets, sizes and shapes"""
    buf, offs, lens, was_torch = _rows_of(x, lengths, offsets)
    H = int(H) if H else W // 4
    B = len(lens)
    frames = [stft_frames(n, W, H) for n in lens]
    if min(frames) < 0:
        raise ValueError(f"every row needs more than {W // 2} samples (reflect padding)")
    rows_out = (W // 2 + 1) if kind == "stft" else tail[1]
    sizes = [rows_out * f for f in frames]
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    out_offsets = [int(v) for v in out_offsets]
    total = max(o + s for o, s in zip(out_offsets, sizes))
    L = _lib.lib()
    off_a, n_a, oo_a = _lib.i64_array(offs), _lib.i64_array(lens), _lib.i64_array(out_offsets)
    width = 2 if kind == "stft" else 1
    if host:
        flat = buf if not was_torch else np.ascontiguousarray(buf[0].detach().cpu().numpy())
        if was_torch and len(buf[1]) > 1:
            raise ValueError("host=True takes numpy rows")
        out = np.zeros(total * width, np.float32)
        if kind == "stft":
            _lib.check(L.nc_audio_stft_host(flat.ctypes.data, B, off_a, n_a, W, H, tail[0], out.ctypes.data, oo_a))
        else:
            _lib.check(L.nc_audio_mel_spectrogram_host(flat.ctypes.data, B, off_a, n_a, tail[0], W, H, tail[1], tail[2], tail[3], out.ctypes.data, oo_a))
    else:
        torch = _torch()
        base = buf[0] if was_torch else torch.from_numpy(buf).cuda()
        out = torch.zeros(total * width, dtype=torch.float32, device=base.device)
        stream = torch.cuda.current_stream(base.device).cuda_stream
        dev = base.device.index or 0
        if kind == "stft":
            _lib.check(L.nc_audio_stft_dev(dev, base.data_ptr(), B, off_a, n_a, W, H, tail[0], out.data_ptr(), oo_a, stream))
        else:
            _lib.check(L.nc_audio_mel_spectrogram_dev(dev, base.data_ptr(), B, off_a, n_a, tail[0], W, H, tail[1], tail[2], tail[3], out.data_ptr(), oo_a,
                                                      stream))
        if not was_torch:
            torch.cuda.synchronize(base.device)
            out = out.cpu().numpy()
    return out, out_offsets, [(rows_out, f) for f in frames], was_torch and not host


def stft_packed(x, W: int, H: Optional[int] = None, window: str = "hann", lengths=None, offsets=None, out_offsets=None, host: bool = False):
    """nc_audio_stft_dev / _host on a packed buffer: (float32 buffer of (re, im) pairs, out_offsets in complex elements, shapes).  Row b
    is [W/2+1, frames_b] complex at out_offsets[b]."""
    out, oo, shapes, _ = _spectra("stft", x, lengths, offsets, out_offsets, host, int(W), H, (WINDOWS[window],))
    return out, oo, shapes


def stft(x, W: int, H: Optional[int] = None, window: str = "hann", lengths=None, host: bool = False):
    """DSP.STFT (center = true, reflect padding): a list of complex64 [W/2+1, frames_b], one per row"""
    out, oo, shapes, torch_out = _spectra("stft", x, lengths, None, None, host, int(W), H, (WINDOWS[window],))
    res = []
    for o, (k, f) in zip(oo, shapes):
        v = out[2 * o:2 * (o + k * f)].reshape(k, f, 2)
        res.append(_torch().view_as_complex(v) if torch_out else v[..., 0] + 1j * v[..., 1])
    return res


def mel_spectrogram_packed(x, sample_rate: int, W: int, H: Optional[int] = None, n_mels: int = 80, fmin: float = 0.0, fmax: Optional[float] = None,
                           lengths=None, offsets=None, out_offsets=None, host: bool = False):
    """nc_audio_mel_spectrogram_dev / _host on a packed buffer: (float32 buffer, out_offsets, shapes); row b is [n_mels, frames_b]"""
    out, oo, shapes, _ = _spectra("mel", x, lengths, offsets, out_offsets, host, int(W), H, (int(sample_rate), int(n_mels), float(fmin), float(fmax or 0.0)))
    return out, oo, shapes


def mel_spectrogram(x, sample_rate: int, W: int = 2048, H: Optional[int] = None, n_mels: int = 80, fmin: float = 0.0, fmax: Optional[float] = None,
                    lengths=None, host: bool = False):
    """DSP.MelSpectrogram (hann window, n_fft = W): a list of float32 [n_mels, frames_b], one per row"""
    out, oo, shapes = mel_spectrogram_packed(x, sample_rate, W, H, n_mels, fmin, fmax, lengths, None, None, host)
    return [out[o:o + m * f].reshape(m, f) for o, (m, f) in zip(oo, shapes)]


def _unpack_rows(words, S: int, torch_out: bool):
    """[B, ROW_WORDS] 32-bit words of nc_quality_row -> dict of per-row arrays"""
    if torch_out:
        torch = _torch()
        f = words.view(torch.float32)
        return {"l1": f[:, 0], "si_sdr_db": f[:, 1], "mel_distance": f[:, 2], "mel_log": f[:, 3:3 + S], "mel_mag": f[:, 11:11 + S],
                "n_bad": words[:, 19]}
    f = words.view(np.float32)
    return {"l1": f[:, 0].copy(), "si_sdr_db": f[:, 1].copy(), "mel_distance": f[:, 2].copy(), "mel_log": f[:, 3:3 + S].copy(),
            "mel_mag": f[:, 11:11 + S].copy(), "n_bad": words[:, 19].copy()}


def quality_metrics(ref, est, lengths=None, sample_rate: int = 44100, scales: Optional[QualityConfig] = None, ref_offsets=None, est_offsets=None,
                    host: bool = False):
    """nc_quality_metrics_dev / _host: per row (one channel of one clip) l1, si_sdr_db, mel_distance, mel_log / mel_mag [B, n_scales] and
    n_bad.  ref / est: lists of 1-D rows, [B, T] arrays, or packed buffers with lengths and element offsets (the packed input of a ragged
    encode and the packed output of the ragged decode compare in place).  est rows may be longer than `lengths`: the first n count."""
    cfg = scales or QualityConfig.dac_eval()
    c = cfg.c_struct()
    S = int(c.n_scales)
    rbuf, roffs, rlens, r_torch = _rows_of(ref, lengths, ref_offsets)
    ebuf, eoffs, elens, e_torch = _rows_of(est, lengths, est_offsets)
    if len(rlens) != len(elens):
        raise ValueError("ref and est must hold the same number of rows")
    if r_torch != e_torch:
        raise ValueError("ref and est must both be numpy or both be torch")
    lens = [min(a, b) for a, b in zip(rlens, elens)] if lengths is None else [int(v) for v in lengths]
    B = len(lens)
    L = _lib.lib()
    ro, eo, na = _lib.i64_array(roffs), _lib.i64_array(eoffs), _lib.i64_array(lens)
    if host:
        if r_torch:
            raise ValueError("host=True takes numpy rows")
        words = np.zeros((B, ROW_WORDS), np.int32)
        _lib.check(L.nc_quality_metrics_host(rbuf.ctypes.data, ro, ebuf.ctypes.data, eo, na, B, int(sample_rate), C.byref(c), words.ctypes.data))
        return _unpack_rows(words, S, False)
    torch = _torch()
    rb = rbuf[0] if r_torch else torch.from_numpy(rbuf).cuda()
    eb = ebuf[0] if e_torch else torch.from_numpy(ebuf).cuda()
    words = torch.zeros((B, ROW_WORDS), dtype=torch.int32, device=rb.device)
    stream = torch.cuda.current_stream(rb.device).cuda_stream
    _lib.check(L.nc_quality_metrics_dev(rb.device.index or 0, rb.data_ptr(), ro, eb.data_ptr(), eo, na, B, int(sample_rate), C.byref(c),
                                        words.data_ptr(), stream))
    if r_torch:
        return _unpack_rows(words, S, True)
    torch.cuda.synchronize(rb.device)
    return _unpack_rows(words.cpu().numpy(), S, False)


def round_trip_rows(clips, decoded):
    """the rows of a round trip: every channel of every clip next to the same channel of its decode, cut to the clip's length"""
    ref, est = [], []
    for c, d in zip(clips, decoded):
        n = min(int(c.shape[-1]), int(d.shape[-1]))
        c2, d2 = c.reshape(-1, c.shape[-1]), d.reshape(-1, d.shape[-1])
        for ch in range(int(c2.shape[0])):
            ref.append(c2[ch, :n])
            est.append(d2[ch, :n])
    return ref, est


def on_device(clips):
    """(device float32 tensors, whether the caller's were torch)"""
    torch = _torch()
    was_torch = _is_torch(clips[0])
    out = [(c if _is_torch(c) else torch.from_numpy(np.ascontiguousarray(np.asarray(c, np.float32)))).to(torch.float32).contiguous().cuda() for c in clips]
    return out, was_torch


def hand_back(res: dict, was_torch: bool) -> dict:
    if was_torch:
        return res
    dev = res["l1"].device
    _torch().cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in res.items()}
