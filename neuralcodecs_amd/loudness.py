"""Loudness (include/nc_mi355x.h "loudness"): ITU-R BS.1770 K-weighting, gated integrated loudness, normalisation to a
target level and the gain that restores a stored level -- the reference's LoudnessMeter.IntegratedLoudness / NormalizeAudio
(AudioTools/LoudnessMeter.cs:127-207) and AudioSignal.Loudness / Normalize (AudioTools/AudioSignal.cs:847-940).  numpy in, numpy out; torch
device tensors in, tensors out and nothing leaves the device.  host=True runs the serial host twin of the library instead of the kernels
(no device needed): the two agree bit for bit.  The _packed forms take one buffer with per-clip lengths and per-channel ELEMENT offsets
(clip b, channel c at offsets[b * channels + c]), so the packed buffers of the ragged encode / decode calls are levelled in place."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib

FILTERS = {"reference": _lib.NC_KWEIGHT_REFERENCE, "designed": _lib.NC_KWEIGHT_DESIGNED}
ROW_WORDS = C.sizeof(_lib.NcLoudnessRow) // 4
GAIN_FACTOR = np.float32(0.11512925464970229)
BLOCK = 64


@dataclass
class LoudnessConfig:
    """nc_loudness_cfg: the coefficient source ("reference": the literals of LoudnessMeter.cs at any rate; "designed": per rate) and the
    level that `gain` leads to."""
    filter: str = "reference"
    target_db: float = -24.0

    def c_struct(self) -> "_lib.NcLoudnessCfg":
        c = _lib.NcLoudnessCfg()
        c.filter, c.target_db = FILTERS[self.filter], float(self.target_db)
        return c


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _torch():
    import torch
    return torch


def kweight_coeffs(sample_rate: int, filter: str = "reference"):
    """nc_audio_kweight_coeffs: (b, a) float64 [2, 3] each; stage 0 the high shelf, stage 1 the high pass"""
    b, a = np.empty((2, 3), np.float64), np.empty((2, 3), np.float64)
    _lib.check(_lib.lib().nc_audio_kweight_coeffs(int(sample_rate), FILTERS[filter], b.ctypes.data, a.ctypes.data))
    return b, a


def kweight_tables(sample_rate: int, filter: str = "reference"):
    """nc_audio_kweight_tables: the block tables Hm float32 [64, 64], Cm float32 [4, 64], Gs float64 [64, 4], M float64 [4, 4]"""
    Hm, Cm = np.empty((BLOCK, BLOCK), np.float32), np.empty((4, BLOCK), np.float32)
    Gs, M = np.empty((BLOCK, 4), np.float64), np.empty((4, 4), np.float64)
    _lib.check(_lib.lib().nc_audio_kweight_tables(int(sample_rate), FILTERS[filter], Hm.ctypes.data, Cm.ctypes.data, Gs.ctypes.data, M.ctypes.data))
    return {"Hm": Hm, "Cm": Cm, "Gs": Gs, "M": M}


def _buffer(x, host: bool):
    """a flat float32 buffer: numpy for the twin, a device tensor otherwise -> (buffer, was_torch)"""
    was_torch = _is_torch(x)
    if host:
        if was_torch:
            raise ValueError("host=True takes numpy buffers")
        return np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)), False
    torch = _torch()
    t = x if was_torch else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
    t = t.reshape(-1)
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        t = t.to(torch.float32).contiguous().cuda()
    return t, was_torch


def _same_memory(buf, x) -> bool:
    if _is_torch(buf):
        return _is_torch(x) and buf.data_ptr() == x.data_ptr()
    return isinstance(x, np.ndarray) and np.shares_memory(buf, x)


def _tables(lengths, offsets, channels: int, numel: int, what: str):
    lens = [int(v) for v in lengths]
    C_ = int(channels)
    if offsets is None:
        offs, at = [], 0
        for n in lens:
            offs += [at + c * n for c in range(C_)]
            at += C_ * n
    else:
        offs = [int(v) for v in offsets]
    if len(offs) != len(lens) * C_:
        raise ValueError(f"{what}: one offset per channel of every clip")
    if any(o < 0 for o in offs) or any(n < 0 for n in lens):
        raise ValueError(f"{what}: negative offset or length")
    if offs and max(o + lens[i // C_] for i, o in enumerate(offs)) > numel:
        raise ValueError(f"{what}: a row reaches past the end of the buffer")
    return lens, offs


def _ptr(buf):
    return buf.data_ptr() if _is_torch(buf) else buf.ctypes.data


def _out_like(buf, numel: int, fill=0.0):
    if _is_torch(buf):
        return _torch().full((numel,), fill, dtype=_torch().float32, device=buf.device)
    return np.full(numel, fill, np.float32)


def _dev_args(buf):
    torch = _torch()
    return buf.device.index or 0, torch.cuda.current_stream(buf.device).cuda_stream


def _unpack_rows(words, torch_out: bool, target_db=None):
    f = words.view(_torch().float32) if torch_out else words.view(np.float32)
    cp = (lambda v: v) if torch_out else (lambda v: v.copy())
    out = {"lufs": cp(f[:, 0]), "gain": cp(f[:, 1]), "n_blocks": cp(words[:, 2]), "n_pass_abs": cp(words[:, 3]), "n_pass_rel": cp(words[:, 4]),
           "n_bad": cp(words[:, 5])}
    if target_db is not None:
        out["target_db"] = float(target_db)
    return out


def _finish(buf, was_torch: bool, *values):
    """device results of a numpy call go back to numpy"""
    if _is_torch(buf) and not was_torch:
        _torch().cuda.synchronize(buf.device)
        return [v.cpu().numpy() if _is_torch(v) else v for v in values]
    return list(values)


def kweight_packed(x, sample_rate: int, filter: str = "reference", lengths=None, offsets=None, out_offsets=None, out=None, host: bool = False):
    """nc_audio_kweight_dev / _host: the K-weighted rows of a packed buffer -> (out buffer, out_offsets).  `out`: write into this buffer."""
    buf, was_torch = _buffer(x, host)
    lens, offs = _tables(lengths if lengths is not None else [buf.shape[0]], offsets, 1, int(buf.shape[0]), "kweight")
    oo = [int(v) for v in out_offsets] if out_offsets is not None else offs
    if out is None:
        out = _out_like(buf, max([o + n for o, n in zip(oo, lens)] + [1]))
    L = _lib.lib()
    args = (_ptr(buf), len(lens), _lib.i64_array(offs), _lib.i64_array(lens), int(sample_rate), FILTERS[filter], _ptr(out), _lib.i64_array(oo))
    if host:
        _lib.check(L.nc_audio_kweight_host(*args))
        return out, oo
    dev, stream = _dev_args(buf)
    _lib.check(L.nc_audio_kweight_dev(dev, *args, stream))
    return _finish(buf, was_torch, out)[0], oo


def kweight(x, sample_rate: int, filter: str = "reference", host: bool = False):
    """the K-weighted rows of a list of 1-D rows (or a [B, T] array): a list of rows"""
    rows = list(x) if isinstance(x, (list, tuple)) else [r for r in (x if x.ndim == 2 else x.reshape(1, -1))]
    lens = [int(r.shape[-1]) for r in rows]
    flat = _torch().cat([r.reshape(-1) for r in rows]) if _is_torch(rows[0]) else np.concatenate([np.asarray(r, np.float32).reshape(-1) for r in rows])
    out, oo = kweight_packed(flat, sample_rate, filter, lens, host=host)
    return [out[o:o + n] for o, n in zip(oo, lens)]


def loudness_packed(x, sample_rate: int, lengths, offsets=None, channels: int = 1, config: Optional[LoudnessConfig] = None, host: bool = False):
    """nc_loudness_dev / _host on a packed buffer: per clip lufs, gain (towards config.target_db), n_blocks, n_pass_abs, n_pass_rel, n_bad"""
    cfg = config or LoudnessConfig()
    c = cfg.c_struct()
    buf, was_torch = _buffer(x, host)
    lens, offs = _tables(lengths, offsets, channels, int(buf.shape[0]), "loudness")
    B = len(lens)
    L = _lib.lib()
    if host:
        words = np.zeros((B, ROW_WORDS), np.int32)
        _lib.check(L.nc_loudness_host(_ptr(buf), B, int(channels), _lib.i64_array(offs), _lib.i64_array(lens), int(sample_rate), C.byref(c), words.ctypes.data))
        return _unpack_rows(words, False, cfg.target_db)
    torch = _torch()
    words = torch.zeros((B, ROW_WORDS), dtype=torch.int32, device=buf.device)
    dev, stream = _dev_args(buf)
    _lib.check(L.nc_loudness_dev(dev, _ptr(buf), B, int(channels), _lib.i64_array(offs), _lib.i64_array(lens), int(sample_rate), C.byref(c),
                                 words.data_ptr(), stream))
    words, = _finish(buf, was_torch, words)
    return _unpack_rows(words, was_torch, cfg.target_db)


def normalize_loudness_packed(x, sample_rate: int, lengths, offsets=None, channels: int = 1, config: Optional[LoudnessConfig] = None, out_offsets=None,
                              out=None, in_place: bool = False, host: bool = False):
    """nc_loudness_normalize_dev / _host on a packed buffer: (levelled buffer, out_offsets, rows).  in_place: write over x (a device tensor or,
    with host=True, a float32 numpy buffer); `out`: write into this buffer at out_offsets."""
    cfg = config or LoudnessConfig()
    c = cfg.c_struct()
    buf, was_torch = _buffer(x, host)
    if in_place and not _same_memory(buf, x):
        raise ValueError("in_place needs a contiguous float32 buffer where the call runs")
    lens, offs = _tables(lengths, offsets, channels, int(buf.shape[0]), "normalize_loudness")
    oo = [int(v) for v in out_offsets] if out_offsets is not None else offs
    if in_place:
        out = buf
    elif out is None:
        out = _out_like(buf, max([o + lens[i // int(channels)] for i, o in enumerate(oo)] + [1]))
    B = len(lens)
    L = _lib.lib()
    tabs = (B, int(channels), _lib.i64_array(offs), _lib.i64_array(lens), int(sample_rate), C.byref(c))
    if host:
        words = np.zeros((B, ROW_WORDS), np.int32)
        _lib.check(L.nc_loudness_normalize_host(_ptr(buf), *tabs, _ptr(out), _lib.i64_array(oo), words.ctypes.data))
        return out, oo, _unpack_rows(words, False, cfg.target_db)
    torch = _torch()
    words = torch.zeros((B, ROW_WORDS), dtype=torch.int32, device=buf.device)
    dev, stream = _dev_args(buf)
    _lib.check(L.nc_loudness_normalize_dev(dev, _ptr(buf), *tabs, _ptr(out), _lib.i64_array(oo), words.data_ptr(), stream))
    out, words = _finish(buf, was_torch, out, words)
    return out, oo, _unpack_rows(words, was_torch, cfg.target_db)


def apply_gain_db_packed(x, db, lengths, offsets=None, channels: int = 1, out_offsets=None, out=None, in_place: bool = False, host: bool = False):
    """nc_audio_apply_gain_db_dev / _host on a packed buffer: clip b times exp(db[b] ln(10) / 20) -> (buffer, out_offsets)"""
    buf, was_torch = _buffer(x, host)
    if in_place and not _same_memory(buf, x):
        raise ValueError("in_place needs a contiguous float32 buffer where the call runs")
    lens, offs = _tables(lengths, offsets, channels, int(buf.shape[0]), "apply_gain_db")
    oo = [int(v) for v in out_offsets] if out_offsets is not None else offs
    if in_place:
        out = buf
    elif out is None:
        out = _out_like(buf, max([o + lens[i // int(channels)] for i, o in enumerate(oo)] + [1]))
    dbv = np.ascontiguousarray(np.asarray(db.detach().cpu().numpy() if _is_torch(db) else db, np.float32).reshape(-1))
    if dbv.size != len(lens):
        raise ValueError("one db value per clip")
    L = _lib.lib()
    args = (_ptr(buf), len(lens), int(channels), _lib.i64_array(offs), _lib.i64_array(lens), dbv.ctypes.data, _ptr(out), _lib.i64_array(oo))
    if host:
        _lib.check(L.nc_audio_apply_gain_db_host(*args))
        return out, oo
    dev, stream = _dev_args(buf)
    _lib.check(L.nc_audio_apply_gain_db_dev(dev, *args, stream))
    return _finish(buf, was_torch, out)[0], oo


def pack_clips(clips):
    """clips: 1-D [n_b] or [C, n_b] arrays / tensors with one C -> (packed buffer, lengths, channels, shapes); channel c of clip b lies
    at the default offsets of the _packed forms"""
    if len(clips) == 0:
        raise ValueError("the list of clips must not be empty")
    shapes = [tuple(int(v) for v in c.shape) for c in clips]
    chans = {1 if len(s) == 1 else s[0] for s in shapes}
    if any(len(s) not in (1, 2) for s in shapes) or len(chans) != 1:
        raise ValueError("every clip must be [n] or [C, n] with one channel count")
    if _is_torch(clips[0]):
        torch = _torch()
        flat = torch.cat([c.reshape(-1).to(torch.float32) for c in clips])
    else:
        flat = np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in clips])
    return flat, [s[-1] for s in shapes], chans.pop(), shapes


def _unpack_clips(buf, shapes):
    out, at = [], 0
    for s in shapes:
        size = int(np.prod(s))
        out.append(buf[at:at + size].reshape(s))
        at += size
    return out


def loudness(clips, sample_rate: int, config: Optional[LoudnessConfig] = None, host: bool = False):
    """AudioSignal.Loudness per clip (clips of any lengths, [n] or [C, n]): a dict of per-clip arrays, see loudness_packed"""
    flat, lens, chans, _ = pack_clips(clips)
    return loudness_packed(flat, sample_rate, lens, None, chans, config, host)


def normalize_loudness(clips, sample_rate: int, config: Optional[LoudnessConfig] = None, host: bool = False):
    """AudioSignal.Normalize per clip: (the levelled clips, as views of one packed buffer, and the rows with the measured levels)"""
    flat, lens, chans, shapes = pack_clips(clips)
    out, _, rows = normalize_loudness_packed(flat, sample_rate, lens, None, chans, config, host=host)
    return _unpack_clips(out, shapes), rows


def apply_gain_db(clips, db, host: bool = False):
    """clip b times exp(db[b] ln(10) / 20): the levelled clips as views of one packed buffer"""
    flat, lens, chans, shapes = pack_clips(clips)
    out, _ = apply_gain_db_packed(flat, db, lens, None, chans, host=host)
    return _unpack_clips(out, shapes)


def restore_db(rows):
    """the per-clip gain in dB that undoes the normalisation `rows` came from: measured lufs - target"""
    lufs = rows["lufs"]
    lufs = lufs.detach().cpu().numpy() if _is_torch(lufs) else np.asarray(lufs)
    return (lufs.astype(np.float32) - np.float32(rows["target_db"])).astype(np.float32)


def normalize_ragged(clips, sample_rate: int, target_db: float = -24.0, filter: str = "reference", host: bool = False):
    """level 1-D clips of any lengths to target_db: (the levelled clips, views of one packed buffer and ready for encode_ragged, rows)"""
    return normalize_loudness(clips, sample_rate, LoudnessConfig(filter, target_db), host)


def restore_ragged(decoded, rows, host: bool = False):
    """undo normalize_ragged on the decoded clips: clip b times the gain of restore_db(rows)[b]"""
    return apply_gain_db(decoded, restore_db(rows), host)
