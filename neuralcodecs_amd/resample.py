"""Band-limited resampling (include/nc_mi355x.h "band-limited resampling"): the windowed-sinc polyphase resampler of the
upstream DAC pipeline (julius resample_frac) in place of the reference's AudioSignal.ResampleFrac (AudioTools/AudioSignal.cs:962-1032),
which the header explains is not mirrored.  numpy in, numpy out; torch device tensors in, tensors out and nothing leaves the device.
host=True runs the serial host twin of the library instead of the kernels (no device needed): the two agree bit for bit.  The _packed form
takes one buffer with per-row lengths and ELEMENT offsets, as the loudness calls do; a row is one channel of one clip."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from .loudness import _buffer, _dev_args, _finish, _is_torch, _out_like, _ptr, _torch


@dataclass
class ResampleConfig:
    """nc_resample_cfg: zero crossings of the sinc on either side and the cutoff as a fraction of the lower Nyquist.  0 stands for the
    default; rolloff = 0.945 is passed as 0, so that it is the library's binary64 default and not 0.945 narrowed to binary32."""
    zeros: int = 24
    rolloff: float = 0.945

    def c_struct(self) -> "_lib.NcResampleCfg":
        c = _lib.NcResampleCfg()
        c.zeros, c.rolloff = int(self.zeros), 0.0 if self.rolloff == 0.945 else float(self.rolloff)
        return c


def _cfg(cfg: Optional[ResampleConfig]):
    return C.byref(cfg.c_struct()) if cfg is not None else None


def resample_sinc_len(n_in: int, src: int, dst: int) -> int:
    """nc_audio_resample_sinc_len: ceil(n_in U / D)"""
    n = int(_lib.lib().nc_audio_resample_sinc_len(int(n_in), int(src), int(dst)))
    if n < 0:
        raise ValueError(f"resample_sinc_len({n_in}, {src}, {dst}): rates must be >= 1 and the length in [0, 2^30]")
    return n


def resample_sinc_geom(src: int, dst: int, cfg: Optional[ResampleConfig] = None) -> dict:
    """nc_audio_resample_sinc_geom: U, D, W, K, K4 of the ratio under cfg"""
    v = [C.c_int32() for _ in range(5)]
    _lib.check(_lib.lib().nc_audio_resample_sinc_geom(int(src), int(dst), _cfg(cfg), *[C.byref(x) for x in v]))
    return dict(zip(("U", "D", "W", "K", "K4"), (int(x.value) for x in v)))


def resample_sinc_table(src: int, dst: int, cfg: Optional[ResampleConfig] = None) -> np.ndarray:
    """nc_audio_resample_sinc_table: h float32 [U, K4]"""
    g = resample_sinc_geom(src, dst, cfg)
    h = np.empty((g["U"], g["K4"]), np.float32)
    _lib.check(_lib.lib().nc_audio_resample_sinc_table(int(src), int(dst), _cfg(cfg), h.ctypes.data))
    return h


def resample_sinc_packed(buf, src: int, dst: int, lengths, offsets=None, out_offsets=None, out=None, cfg: Optional[ResampleConfig] = None,
                         host: bool = False):
    """nc_audio_resample_sinc_dev / _host on a packed buffer -> (out buffer, out_offsets, out lengths).  Defaults: the rows end to end in
    `buf`, the results end to end in a fresh buffer; `out`: write into this buffer (it must not overlap `buf`)."""
    b, was_torch = _buffer(buf, host)
    lens = [int(v) for v in lengths]
    offs = [int(v) for v in offsets] if offsets is not None else np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64).tolist()
    if len(offs) != len(lens):
        raise ValueError("resample_sinc: one offset per row")
    if any(o < 0 for o in offs) or any(n < 0 for n in lens):
        raise ValueError("resample_sinc: negative offset or length")
    if offs and max(o + n for o, n in zip(offs, lens)) > int(b.shape[0]):
        raise ValueError("resample_sinc: a row reaches past the end of the buffer")
    olens = [resample_sinc_len(n, src, dst) for n in lens]
    oo = [int(v) for v in out_offsets] if out_offsets is not None else np.concatenate([[0], np.cumsum(olens)[:-1]]).astype(np.int64).tolist()
    if len(oo) != len(lens):
        raise ValueError("resample_sinc: one output offset per row")
    need = max([o + n for o, n in zip(oo, olens)] + [1])
    if out is None:
        out = _out_like(b, need)
    else:
        if _is_torch(out) != _is_torch(b):
            raise ValueError("resample_sinc: `out` must live where the call runs")
        if out.ndim != 1 or int(out.shape[0]) < need or (_is_torch(out) and (out.dtype != _torch().float32 or not out.is_contiguous())) or \
                (not _is_torch(out) and (out.dtype != np.float32 or not out.flags.c_contiguous)):
            raise ValueError("resample_sinc: `out` must be a contiguous 1-D float32 buffer that holds every output row")
    if sum(lens) == 0:                                   # nothing to read or write (an empty tensor has no address to pass)
        return _finish(b, was_torch, out)[0], oo, olens
    L = _lib.lib()
    args = (_ptr(b), len(lens), _lib.i64_array(offs), _lib.i64_array(lens), int(src), int(dst), _cfg(cfg), _ptr(out), _lib.i64_array(oo))
    if host:
        _lib.check(L.nc_audio_resample_sinc_host(*args))
        return out, oo, olens
    dev, stream = _dev_args(b)
    _lib.check(L.nc_audio_resample_sinc_dev(dev, *args, stream))
    return _finish(b, was_torch, out)[0], oo, olens


def resample_sinc(clips, src: int, dst: int, cfg: Optional[ResampleConfig] = None, host: bool = False):
    """a list of clips ([n] or [C, n] arrays / tensors, any lengths) at `src` Hz -> the list at `dst` Hz, views of one packed buffer"""
    if len(clips) == 0:
        raise ValueError("the list of clips must not be empty")
    shapes = [tuple(int(v) for v in c.shape) for c in clips]
    if any(len(s) not in (1, 2) for s in shapes):
        raise ValueError("every clip must be [n] or [C, n]")
    if _is_torch(clips[0]):
        torch = _torch()
        flat = torch.cat([c.reshape(-1).to(torch.float32) for c in clips])
    else:
        flat = np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in clips])
    lens = [s[-1] for s in shapes for _ in range(1 if len(s) == 1 else s[0])]
    out, oo, olens = resample_sinc_packed(flat, src, dst, lens, cfg=cfg, host=host)
    res, r = [], 0
    for s in shapes:
        rows = 1 if len(s) == 1 else s[0]
        at, m = oo[r] if rows else 0, resample_sinc_len(s[-1], src, dst)
        res.append(out[at:at + rows * m].reshape((m,) if len(s) == 1 else (rows, m)))
        r += rows
    return res


def resample_ragged(clips, sample_rate: int, model_rate: int, host: bool = False):
    """1-D clips of any lengths at `sample_rate` -> the clips at the model's rate, views of one packed buffer and ready for
    normalize_ragged / encode_ragged"""
    if any(c.ndim != 1 for c in clips):
        raise ValueError("every clip must be 1-D")
    return resample_sinc(clips, sample_rate, model_rate, None, host)
