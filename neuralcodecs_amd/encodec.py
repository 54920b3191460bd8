"""Host-side mirror of the reference's ``Encodec`` model class over the C ABI.

Same members, argument meaning and error behaviour as NeuralCodecs.Torch/Models/Encodec.cs
(``Encodec : Module<Tensor,Tensor>, INeuralCodec``):

    Encodec(config)                         Encodec.cs:46-90   (ArgumentException on a bandwidth outside TargetBandwidths)
    load_weights(path)                      Encodec.cs:375-405 (INeuralCodec.LoadWeights)
    encode(x [B,C,T]) -> List[EncodedFrame] Encodec.cs:259-285 (one frame per 1 s segment at 48 kHz; a single frame at 24 kHz)
    encode_array(float[])                   Encodec.cs:243-252 (reshape(1, channels, -1))
    decode(frames) -> [B,C,T_dec]           Encodec.cs:213-235 (per-frame decode, x scale, triangular overlap-add)
    forward(x)                              Encodec.cs:287-291 (decode(encode(x)) trimmed to the input length)
    set_target_bandwidth(kbps)              Encodec.cs:409-419
    properties frame_rate, bits_per_codebook, num_codebooks, segment_length, segment_stride   Encodec.cs:145-201

numpy arrays use the host API; torch device tensors use the zero-copy `*_dev` API on torch's current stream.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .config import EncodecConfig
from .session import FLUSH
from .weights import save_blob


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


@dataclass
class EncodedFrame:
    """Modules/Encodec/EncodedFrame.cs: codes [B, n_q, T'] int64 and the optional per-clip scale [B, 1]."""
    codes: object
    scale: Optional[object] = None


def _c_config(config: EncodecConfig) -> "_lib.NcEncodecConfig":
    """nc_encodec_config of an EncodecConfig (the derived fields as Encodec.cs:70-84 computes them)."""
    hop = config.hop_length
    frame_rate = int(math.ceil(config.sampling_rate / float(hop)))
    seg = None if config.segment_seconds is None else int(config.segment_seconds * config.sampling_rate)
    stride = None if seg is None else max(1, int((1 - config.overlap) * seg))
    c = _lib.NcEncodecConfig()
    c.sample_rate, c.channels, c.dimension, c.n_filters = config.sampling_rate, config.channels, config.dimension, config.n_filters
    c.n_ratios = len(config.ratios)
    for i, r in enumerate(config.ratios):
        c.ratios[i] = r
    c.lstm_layers, c.compress, c.kernel_size = config.lstm_layers, config.compress, config.kernel_size
    c.last_kernel_size, c.residual_kernel_size = config.last_kernel_size, config.residual_kernel_size
    c.time_group_norm = int(config.norm == "time_group_norm")
    c.causal, c.normalize = int(config.causal), int(config.normalize)
    c.segment_length, c.segment_stride = seg or 0, stride or 0
    c.codebook_size, c.frame_rate, c.bandwidth = config.codebook_size, frame_rate, config.bandwidth
    c.n_codebooks = int(1000 * max(config.target_bandwidths) / (math.ceil(config.sampling_rate / hop) * 10))
    return c


def _ragged_rows(call, lengths, decode: bool):
    """(plan dict, list of row dicts in launch order) of one of the two planner entry points; call(n, lens, plan, rows, cap)"""
    lens = _lib.i64_array(lengths)
    p = _lib.NcEncodecRaggedPlan()
    _lib.check(call(len(lens), lens, C.byref(p), None, 0))
    rows = (_lib.NcEncodecRaggedRow * max(1, int(p.n_rows)))()
    _lib.check(call(len(lens), lens, C.byref(p), rows, int(p.n_rows)))
    plan = {k: int(getattr(p, k)) for k, _ in _lib.NcEncodecRaggedPlan._fields_}
    return plan, [{k: int(getattr(rows[i], k)) for k, _ in _lib.NcEncodecRaggedRow._fields_} for i in range(int(p.n_rows))]


def encodec_ragged_rows(config: EncodecConfig, lengths, decode: bool = False, max_rows: int = 0):
    """nc_encodec_ragged_rows: how a ragged call on clips of these lengths (samples) pools their segments into batches -- from a
    config alone, no device needed."""
    c = _c_config(config)
    return _ragged_rows(lambda n, lens, p, rows, cap: _lib.lib().nc_encodec_ragged_rows(C.byref(c), 1 if decode else 0, n, lens, int(max_rows), p, rows, cap),
                        lengths, decode)


class Encodec(_lib.ProfileMixin):
    def __init__(self, config: Optional[EncodecConfig] = None, device_index: int = 0):
        if config is None:
            raise ValueError("config must not be null")
        if config.bandwidth is None or config.bandwidth not in tuple(config.target_bandwidths):
            raise ValueError(f"Invalid bandwidth {config.bandwidth}. Select one of {list(config.target_bandwidths)}")   # Encodec.cs:49-54
        self.config = config
        self.device_index = device_index
        hop = config.hop_length
        self.frame_rate = int(math.ceil(config.sampling_rate / float(hop)))                                # Encodec.cs:83
        self.bits_per_codebook = int(math.log2(config.codebook_size))
        self.num_codebooks = int(1000 * max(config.target_bandwidths) / (math.ceil(config.sampling_rate / hop) * 10))   # Encodec.cs:70-71
        self.segment_length = None if config.segment_seconds is None else int(config.segment_seconds * config.sampling_rate)
        self.segment_stride = None if self.segment_length is None else max(1, int((1 - config.overlap) * self.segment_length))
        c = _c_config(config)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().nc_encodec_create(C.byref(c), device_index, C.byref(self._h)))

    @property
    def Config(self) -> EncodecConfig:
        return self.config

    @property
    def current_bandwidth(self) -> float:
        return self.config.bandwidth

    # ---- INeuralCodec ----------------------------------------------------------------------
    def load_weights(self, path: str) -> None:
        _lib.check(_lib.lib().nc_codec_load_weights(self._h, str(path).encode()))

    def load_state_dict(self, state_dict) -> None:
        self.load_blob(save_blob(state_dict))

    def load_blob(self, blob: bytes) -> None:
        _lib.check(_lib.lib().nc_codec_load_weights_mem(self._h, blob, len(blob)))

    def dispose(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            try:
                _lib.lib().nc_codec_destroy(self._h)
            finally:
                self._h = C.c_void_p()

    close = dispose

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.dispose()

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    def set_target_bandwidth(self, bandwidth: float) -> None:
        if bandwidth not in tuple(self.config.target_bandwidths):
            raise ValueError(f"This model doesn't support the bandwidth {bandwidth} kbps. "
                             f"Select one of {list(self.config.target_bandwidths)} kbps")              # Encodec.cs:411-416
        _lib.check(_lib.lib().nc_encodec_set_bandwidth(self._h, float(bandwidth)))
        self.config.bandwidth = bandwidth

    def query(self, T: int):
        nf, nq, dl = C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(_lib.lib().nc_encodec_query(self._h, T, C.byref(nf), C.byref(nq), None, 0, C.byref(dl)))   # count first
        lens = (C.c_int64 * max(1, nf.value))()
        _lib.check(_lib.lib().nc_encodec_query(self._h, T, C.byref(nf), C.byref(nq), lens, nf.value, C.byref(dl)))
        return nf.value, nq.value, [lens[i] for i in range(nf.value)], dl.value

    def lstm_stats(self):
        """(stepwise, timeouts): whether the handle has dropped to the step-wise LSTM kernels and how many persistent-launch timeouts it has
        seen (nc_encodec_lstm_stats)."""
        sw, tmo = C.c_int32(0), C.c_int64(0)
        _lib.check(_lib.lib().nc_encodec_lstm_stats(self._h, C.byref(sw), C.byref(tmo)))
        return bool(sw.value), int(tmo.value)

    def _bind_torch_stream(self):
        import torch
        _lib.check(_lib.lib().nc_codec_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device_index).cuda_stream)))   # (the handle's OWN device: one process may drive several)

    # ---- Encode ----------------------------------------------------------------------------
    def _validate(self, x):
        if x is None:
            raise ValueError("audio_data must not be null")
        if x.ndim != 3:
            raise ValueError(f"Expected 3D input tensor [B,C,T], got shape {list(x.shape)}")            # Encodec.cs:493-497
        if x.shape[1] != self.config.channels:
            raise ValueError(f"Expected {self.config.channels} channels, got {x.shape[1]}")             # Encodec.cs:499-503

    def encode(self, x, return_emb: bool = False) -> List[EncodedFrame]:
        self._validate(x)
        B, _, T = x.shape
        nf, nq, lens, _ = self.query(T)
        tot = sum(lens)
        D = self.config.dimension
        if _is_torch(x):
            import torch
            xx = x.contiguous().to(torch.float32)
            codes = torch.empty((B * nq * tot,), dtype=torch.int64, device=xx.device)
            scales = torch.empty((nf, B), dtype=torch.float32, device=xx.device)
            emb = torch.empty((B * D * tot,), dtype=torch.float32, device=xx.device) if return_emb else None
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_encodec_encode_dev(self._h, xx.data_ptr(), B, T, codes.data_ptr(), scales.data_ptr(),
                                                        emb.data_ptr() if emb is not None else None))
        else:
            xx = np.ascontiguousarray(x, dtype=np.float32)
            codes = np.empty((B * nq * tot,), np.int64)
            scales = np.empty((nf, B), np.float32)
            emb = np.empty((B * D * tot,), np.float32) if return_emb else None
            _lib.check(_lib.lib().nc_encodec_encode(self._h, xx.ctypes.data, B, T, codes.ctypes.data, scales.ctypes.data,
                                                    emb.ctypes.data if emb is not None else None))
        frames, embs, o, oe = [], [], 0, 0
        for f, Tf in enumerate(lens):
            c = codes[o:o + B * nq * Tf].reshape(B, nq, Tf)
            o += B * nq * Tf
            frames.append(EncodedFrame(c, scales[f].reshape(B, 1) if self.config.normalize else None))
            if return_emb:
                embs.append(emb[oe:oe + B * D * Tf].reshape(B, D, Tf))
                oe += B * D * Tf
        return (frames, embs) if return_emb else frames

    def encode_array(self, audio_data) -> List[EncodedFrame]:
        if audio_data is None:
            raise ValueError("audio_data must not be null")
        return self.encode(np.asarray(audio_data, dtype=np.float32).reshape(1, self.config.channels, -1))

    # ---- Decode ----------------------------------------------------------------------------
    def decode(self, frames: Sequence[EncodedFrame], length: Optional[int] = None):
        """`length` = sample count of the clip the frames were encoded from (fixes the segment layout for segmented models;
        defaults to the layout implied by the number of frames: all full segments but the last, whose length is inferred)."""
        if frames is None or len(frames) == 0:
            raise ValueError("No frames provided to decode")                                            # Encodec.cs:215-218
        if self.segment_length is None and len(frames) != 1:
            raise ValueError("Expected single frame when no segmentation is used")                      # Encodec.cs:222-225
        for f in frames:
            if f.codes is None:
                raise ValueError("Invalid frame codes in Encodec Decode")
        B, nq, _ = frames[0].codes.shape
        T = length if length is not None else self._infer_length(frames)
        nf, _, lens, Ld = self.query(T)
        if nf != len(frames) or [int(f.codes.shape[-1]) for f in frames] != lens:
            raise ValueError(f"frames do not match the segment layout of a {T}-sample clip: expected {lens}")
        if _is_torch(frames[0].codes):
            import torch
            codes = self._end_to_end([f.codes for f in frames], torch.int64)      # encode()'s own views: the ABI's flat buffers as they are
            if codes is None:
                codes = torch.cat([f.codes.reshape(-1).to(torch.int64) for f in frames]).contiguous()
            scales = None
            if self.config.normalize:
                scales = self._end_to_end([f.scale for f in frames], torch.float32)
                if scales is None:
                    scales = torch.cat([f.scale.reshape(-1).to(torch.float32) for f in frames]).contiguous()
            out = torch.empty((B, self.config.channels, Ld), dtype=torch.float32, device=codes.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_encodec_decode_dev(self._h, codes.data_ptr(), scales.data_ptr() if scales is not None else None,
                                                        B, T, nq, out.data_ptr()))
            return out
        codes = np.ascontiguousarray(np.concatenate([np.asarray(f.codes, np.int64).reshape(-1) for f in frames]))
        scales = None
        if self.config.normalize:
            scales = np.ascontiguousarray(np.concatenate([np.asarray(f.scale, np.float32).reshape(-1) for f in frames]))
        out = np.empty((B, self.config.channels, Ld), np.float32)
        _lib.check(_lib.lib().nc_encodec_decode(self._h, codes.ctypes.data, scales.ctypes.data if scales is not None else None, B, T, nq,
                                                out.ctypes.data))
        return out

    @staticmethod
    def _end_to_end(parts, dtype):
        """The flat tensor the parts are consecutive contiguous views of (what encode() hands out), or None.  No copy, no kernel."""
        try:
            p0 = parts[0]
            base, off = p0.untyped_storage().data_ptr(), p0.storage_offset()
            for p in parts:
                if p.dtype != dtype or not p.is_contiguous() or p.untyped_storage().data_ptr() != base or p.storage_offset() != off:
                    return None
                off += p.numel()
            return p0.as_strided((off - p0.storage_offset(),), (1,), p0.storage_offset())
        except Exception:
            return None

    def _infer_length(self, frames) -> int:
        """Clip length implied by the frames alone, as the reference's Decode(List<EncodedFrame>) sees them (Encodec.cs:213-235):
        the smallest T whose segment layout has exactly these frame counts (nc_encodec_clip_length)."""
        T = C.c_int64()
        lens = (C.c_int64 * len(frames))(*[int(f.codes.shape[-1]) for f in frames])
        _lib.check(_lib.lib().nc_encodec_clip_length(self._h, len(frames), lens, C.byref(T)))
        return T.value

    def forward(self, x):
        frames = self.encode(x)
        return self.decode(frames, x.shape[-1])[..., : x.shape[-1]]                                    # Encodec.cs:290

    # ---- ragged batches (clips of unequal lengths in one call) ------------------------------------
    def set_ragged_rows(self, max_rows: int = 0) -> None:
        """nc_encodec_set_ragged_rows: rows (segments) per launch batch of the ragged calls (0 = default, at most 4096)."""
        _lib.check(_lib.lib().nc_encodec_set_ragged_rows(self._h, int(max_rows)))

    def ragged_rows(self, lengths, decode: bool = False):
        """nc_encodec_ragged_rows_of: (plan, rows) of a ragged call on clips of these lengths under the handle's setting and bandwidth."""
        return _ragged_rows(lambda n, lens, p, rows, cap: _lib.lib().nc_encodec_ragged_rows_of(self._h, 1 if decode else 0, n, lens, p, rows, cap),
                            lengths, decode)

    def ragged_query(self, lengths):
        """nc_encodec_ragged_query: per clip (segments, code frames summed over them, decoded samples)."""
        lens = _lib.i64_array(lengths)
        n = max(1, len(lens))
        nf, fr, dl = (C.c_int32 * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
        _lib.check(_lib.lib().nc_encodec_ragged_query(self._h, len(lens), lens, nf, fr, dl))
        return [int(nf[i]) for i in range(len(lens))], [int(fr[i]) for i in range(len(lens))], [int(dl[i]) for i in range(len(lens))]

    def encode_ragged(self, clips, return_emb: bool = False):
        """nc_encodec_encode_ragged[_dev]: a list of [C, T_b] arrays / device tensors -> per clip the List[EncodedFrame] (leading batch
        of 1) that encode(clip[None]) returns, bit for bit; the segments of all clips run pooled in uniform batches."""
        if clips is None or len(clips) == 0:
            raise ValueError("the list of clips must not be empty")
        for c in clips:
            if c is None or c.ndim != 2 or c.shape[0] != self.config.channels:
                raise ValueError(f"every clip must be [{self.config.channels}, T]")
        B, D = len(clips), self.config.dimension
        lens = [int(c.shape[1]) for c in clips]
        larr = _lib.i64_array(lens)
        nfs, frs, _ = self.ragged_query(lens)
        nq = self.query(1)[1]
        n_codes, n_sc, n_emb = nq * sum(frs), sum(nfs), D * sum(frs)
        if _is_torch(clips[0]):
            import torch
            flat = torch.cat([c.reshape(-1).to(torch.float32) for c in clips]).contiguous()
            codes = torch.empty((max(1, n_codes),), dtype=torch.int64, device=flat.device)
            scales = torch.empty((max(1, n_sc),), dtype=torch.float32, device=flat.device)
            emb = torch.empty((max(1, n_emb),), dtype=torch.float32, device=flat.device) if return_emb else None
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_encodec_encode_ragged_dev(self._h, flat.data_ptr(), B, larr, codes.data_ptr(), scales.data_ptr(),
                                                               emb.data_ptr() if emb is not None else None))
        else:
            flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float32).reshape(-1) for c in clips]))
            codes = np.empty((max(1, n_codes),), np.int64)
            scales = np.empty((max(1, n_sc),), np.float32)
            emb = np.empty((max(1, n_emb),), np.float32) if return_emb else None
            _lib.check(_lib.lib().nc_encodec_encode_ragged(self._h, flat.ctypes.data, B, larr, codes.ctypes.data, scales.ctypes.data,
                                                           emb.ctypes.data if emb is not None else None))
        out, embs, o, osc, oe = [], [], 0, 0, 0
        for T in lens:
            frames, es = [], []
            for f, Tf in enumerate(self.query(T)[2]):
                frames.append(EncodedFrame(codes[o:o + nq * Tf].reshape(1, nq, Tf), scales[osc + f:osc + f + 1].reshape(1, 1) if self.config.normalize else None))
                o += nq * Tf
                if return_emb:
                    es.append(emb[oe:oe + D * Tf].reshape(1, D, Tf))
                    oe += D * Tf
            osc += len(frames)
            out.append(frames)
            embs.append(es)
        return (out, embs) if return_emb else out

    def decode_ragged(self, frame_lists, lengths=None):
        """nc_encodec_decode_ragged[_dev]: per clip a List[EncodedFrame] with a leading batch of 1 -> a list of [C, Ld_b], each the
        decode() of that clip alone, bit for bit.  lengths: the clips' sample counts (default: inferred from the frames as decode() does)."""
        if frame_lists is None or len(frame_lists) == 0:
            raise ValueError("the list of clips must not be empty")
        for fl in frame_lists:
            if fl is None or len(fl) == 0:
                raise ValueError("No frames provided to decode")
            if self.segment_length is None and len(fl) != 1:
                raise ValueError("Expected single frame when no segmentation is used")
            for f in fl:
                if f.codes is None or f.codes.ndim != 3 or f.codes.shape[0] != 1:
                    raise ValueError("Invalid frame codes in Encodec Decode: every frame must be [1, n_q, T']")
        B, nq = len(frame_lists), int(frame_lists[0][0].codes.shape[1])
        if any(int(f.codes.shape[1]) != nq for fl in frame_lists for f in fl):
            raise ValueError("every frame must carry the same number of codebooks")
        lens = [int(t) for t in lengths] if lengths is not None else [self._infer_length(fl) for fl in frame_lists]
        if len(lens) != B:
            raise ValueError("one length per clip")
        for b, (fl, T) in enumerate(zip(frame_lists, lens)):
            nf, _, want, _ = self.query(T)
            if nf != len(fl) or [int(f.codes.shape[-1]) for f in fl] != want:
                raise ValueError(f"clip {b}: frames do not match the segment layout of a {T}-sample clip: expected {want}")
        larr = _lib.i64_array(lens)
        _, _, dls = self.ragged_query(lens)
        Cn = self.config.channels
        if _is_torch(frame_lists[0][0].codes):
            import torch
            codes = torch.cat([f.codes.reshape(-1).to(torch.int64) for fl in frame_lists for f in fl]).contiguous()
            scales = None
            if self.config.normalize:
                scales = torch.cat([f.scale.reshape(-1).to(torch.float32) for fl in frame_lists for f in fl]).contiguous()
            out = torch.empty((max(1, Cn * sum(dls)),), dtype=torch.float32, device=codes.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_encodec_decode_ragged_dev(self._h, codes.data_ptr(), scales.data_ptr() if scales is not None else None,
                                                               B, larr, nq, out.data_ptr()))
        else:
            codes = np.ascontiguousarray(np.concatenate([np.asarray(f.codes, np.int64).reshape(-1) for fl in frame_lists for f in fl]))
            scales = None
            if self.config.normalize:
                scales = np.ascontiguousarray(np.concatenate([np.asarray(f.scale, np.float32).reshape(-1) for fl in frame_lists for f in fl]))
            out = np.empty((max(1, Cn * sum(dls)),), np.float32)
            _lib.check(_lib.lib().nc_encodec_decode_ragged(self._h, codes.ctypes.data, scales.ctypes.data if scales is not None else None,
                                                           B, larr, nq, out.ctypes.data))
        return [p.reshape(Cn, -1) for p in _lib.split_packed(out, [Cn * d for d in dls])]

    def round_trip_quality(self, pcm_list, scales=None):
        """Encode -> decode -> nc_quality_metrics_dev on a list of clips of any lengths, everything on the device: per row (one channel of
        one clip) l1, si_sdr_db, mel_distance, mel_log / mel_mag and n_bad of the decode against the clip (neuralcodecs_amd/quality.py;
        scales: a QualityConfig, default the DAC paper's evaluation set).  numpy clips in, numpy out; device tensors in, tensors out."""
        from . import quality
        clips, was_torch = quality.on_device(pcm_list)
        dec = self.decode_ragged(self.encode_ragged(clips), lengths=[int(c.shape[-1]) for c in clips])
        ref, est = quality.round_trip_rows(clips, dec)
        return quality.hand_back(quality.quality_metrics(ref, est, sample_rate=self.config.sampling_rate, scales=scales), was_torch)

    def normalize_ragged(self, clips, target_db: float = -24.0, filter: str = "reference", host: bool = False):
        """nc_loudness_normalize_dev on 1-D clips of any lengths at the model's sample rate (neuralcodecs_amd/loudness.py): the levelled
        clips, views of one packed buffer and ready for encode_ragged, and the per-clip rows (lufs, gain, ...) to store."""
        from . import loudness
        return loudness.normalize_ragged(clips, self.config.sampling_rate, target_db, filter, host)

    def resample_ragged(self, clips, sample_rate: int, host: bool = False):
        """nc_audio_resample_sinc_dev on 1-D clips of any lengths at `sample_rate` (neuralcodecs_amd/resample.py): the clips at the model's
        sample rate, views of one packed buffer and ready for normalize_ragged / encode_ragged."""
        from . import resample
        return resample.resample_ragged(clips, sample_rate, self.config.sampling_rate, host)

    def restore_ragged(self, decoded, rows, host: bool = False):
        """nc_audio_apply_gain_db_dev: the decoded clips back at the levels normalize_ragged measured (rows: what it returned)."""
        from . import loudness
        return loudness.restore_ragged(decoded, rows, host)

    # ---- stream pool (PCM or frames that arrive over time; segmented models) ----------------------
    def encode_pool(self, n_slots: int) -> "EncodecStreamPool":
        """nc_encodec_stream_pool_create(decode = 0): n_slots live streams encoded segment by segment as their samples arrive."""
        return EncodecStreamPool(self, False, n_slots, None)

    def decode_pool(self, n_slots: int, n_q: Optional[int] = None) -> "EncodecStreamPool":
        """nc_encodec_stream_pool_create(decode = 1): n_slots live streams decoded frame by frame (n_q: codebooks in the pushed codes;
        None = the handle's bandwidth)."""
        return EncodecStreamPool(self, True, n_slots, n_q)

    def encode_session(self) -> "EncodecStreamSession":
        return EncodecStreamSession(self.encode_pool(1))

    def decode_session(self, n_q: Optional[int] = None) -> "EncodecStreamSession":
        return EncodecStreamSession(self.decode_pool(1, n_q))

    # ---- causal streams (PCM or code frames that arrive over time; causal models without segmentation) ----
    def causal_encode_pool(self, n_slots: int) -> "EncodecCausalPool":
        """nc_encodec_causal_pool_create(decode = 0): n_slots live streams encoded hop by hop, the LSTM's state carried."""
        return EncodecCausalPool(self, False, n_slots, None)

    def causal_decode_pool(self, n_slots: int, n_q: Optional[int] = None) -> "EncodecCausalPool":
        """nc_encodec_causal_pool_create(decode = 1): n_slots live streams decoded frame by frame (n_q: codebooks in the pushed codes;
        None = the handle's bandwidth)."""
        return EncodecCausalPool(self, True, n_slots, n_q)

    def causal_encode_session(self) -> "EncodecCausalSession":
        return EncodecCausalSession(self.causal_encode_pool(1))

    def causal_decode_session(self, n_q: Optional[int] = None) -> "EncodecCausalSession":
        return EncodecCausalSession(self.causal_decode_pool(1, n_q))


def encodec_stream_plan(config: EncodecConfig, pushed, emitted, n_in, flush=None, frame_lens=None, decode: bool = False, max_rows: int = 0):
    """nc_encodec_stream_plan: one step of a stream pool from a config alone, no device needed.  Stream i has received pushed[i] samples
    (decode: frames) and emitted emitted[i] segments (decode: samples per channel); it now brings n_in[i] more and flushes where flush[i].
    -> (plan dict, rows in launch order -- `clip` is the stream's index --, per stream {n_frames, code_frames, n_samples})."""
    c = _c_config(config)
    n = len(n_in)
    pu, em, ni = _lib.i64_array(pushed), _lib.i64_array(emitted), _lib.i64_array(n_in)
    fl = (C.c_int32 * max(1, n))(*[int(bool(f)) for f in flush]) if flush is not None else None
    fr = _lib.i64_array(frame_lens) if frame_lens is not None else None
    nf, cf, ns = (C.c_int32 * max(1, n))(), (C.c_int64 * max(1, n))(), (C.c_int64 * max(1, n))()
    p = _lib.NcEncodecRaggedPlan()
    call = lambda rows, cap: _lib.lib().nc_encodec_stream_plan(C.byref(c), 1 if decode else 0, n, pu, em, ni, fl, fr, int(max_rows), C.byref(p), rows, cap, nf, cf, ns)  # noqa: E731
    _lib.check(call(None, 0))
    rows = (_lib.NcEncodecRaggedRow * max(1, int(p.n_rows)))()
    _lib.check(call(rows, int(p.n_rows)))
    plan = {k: int(getattr(p, k)) for k, _ in _lib.NcEncodecRaggedPlan._fields_}
    return (plan, [{k: int(getattr(rows[i], k)) for k, _ in _lib.NcEncodecRaggedRow._fields_} for i in range(int(p.n_rows))],
            [{"n_frames": int(nf[i]), "code_frames": int(cf[i]), "n_samples": int(ns[i])} for i in range(n)])


class _EncodecPool:
    """What the two Encodec pools share: the lifetime of the C pool behind nc_encodec_<_PREFIX>_pool_*, the calls on one slot, the split
    of an entry's value, the ctypes arrays of a step and its torch-or-numpy side."""
    _PREFIX = ""

    def __init__(self, model: Encodec, decode: bool, n_slots: int, n_q: Optional[int]):
        self.model, self.decode, self.n_slots = model, bool(decode), int(n_slots)
        self._p = C.c_void_p()
        self._torch = False
        _lib.check(self._sym("create")(model._h, 1 if decode else 0, int(n_slots), int(n_q or 0), C.byref(self._p)))
        self.n_q = int(n_q) if n_q else model.query(1)[1]

    def _sym(self, name):
        return getattr(_lib.lib(), f"nc_encodec_{self._PREFIX}_pool_{name}")

    def close(self) -> None:
        if getattr(self, "_p", None) is not None and self._p.value:
            try:
                self._sym("destroy")(self._p)
            finally:
                self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset_slot(self, slot: int) -> None:
        _lib.check(self._sym("reset_slot")(self._p, int(slot)))

    def pending(self, slot: int) -> int:
        n = C.c_int64()
        _lib.check(self._sym("pending")(self._p, int(slot), C.byref(n)))
        return n.value

    @staticmethod
    def _split(v):
        """an entry's value -> (data or None, flush)"""
        if v is FLUSH:
            return None, True
        if isinstance(v, tuple) and len(v) == 2 and v[1] is FLUSH:
            return v[0], True
        if v is None:
            raise ValueError("the pushed data must not be null (FLUSH ends a stream)")
        return v, False

    @staticmethod
    def _c(slots, n_in, flush):
        n = len(slots)
        return (C.c_int32 * n)(*slots), _lib.i64_array(n_in), (C.c_int32 * n)(*[int(f) for f in flush])

    def _io(self):
        """-> (empty(k, dtype), ptr(x), cat(parts, dtype), float32, int64, the step symbol) on torch device tensors (torch's current
        stream) or on numpy arrays, whichever the last entries were"""
        if self._torch:
            import torch
            dev = torch.device("cuda", self.model.device_index)
            empty = lambda k, dt: torch.empty((max(1, k),), dtype=dt, device=dev)  # noqa: E731
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            cat = lambda parts, dt: torch.cat([p.reshape(-1).to(dt) for p in parts]).contiguous() if parts else empty(0, dt)  # noqa: E731
            self.model._bind_torch_stream()
            return empty, ptr, cat, torch.float32, torch.int64, self._sym("step_dev")
        empty = lambda k, dt: np.empty((max(1, k),), dt)  # noqa: E731
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=dt).reshape(-1) for p in parts])) if parts else empty(0, dt)  # noqa: E731
        return empty, ptr, cat, np.float32, np.int64, self._sym("step")


class _EncodecPoolSession:
    def __init__(self, pool):
        self.pool = pool

    def push(self, x, **kw):
        out = self.pool.step({0: x}, **kw)
        return (out[0][0], out[1][0]) if isinstance(out, tuple) else out[0]

    def flush(self, x=None, **kw):
        out = self.pool.step({0: FLUSH if x is None else (x, FLUSH)}, **kw)
        return (out[0][0], out[1][0]) if isinstance(out, tuple) else out[0]

    def pending(self) -> int:
        return self.pool.pending(0)

    def reset(self) -> None:
        self.pool.reset_slot(0)

    def close(self) -> None:
        self.pool.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class EncodecStreamPool(_EncodecPool):
    """n_slots independent live streams on one segmented Encodec model, one direction, stepped together (nc_encodec_stream_pool_*).

        out = pool.step({slot: x | FLUSH | (x, FLUSH), ...})

    encode pool: x is PCM [channels, n] (any n >= 0); out[slot] is the list of EncodedFrame (leading batch of 1) of the segments the push
    completed -- often empty.  decode pool: x is a list of EncodedFrame [1, n_q, F]; out[slot] is PCM [channels, n_out].  FLUSH ends the
    slot's stream (after the last x of a tuple) and emits the rest; reset_slot() makes the slot new.  Everything a slot emitted, end to
    end, equals encode() / decode() on the whole stream, bit for bit.  numpy in, numpy out (host API); torch device tensors in, device
    tensors out on torch's current stream."""

    _PREFIX = "stream"

    def _entries(self, entries: dict):
        if not entries:
            raise ValueError("a step needs at least one entry")
        slots, data, flush = [], [], []
        for s, v in entries.items():
            d, f = self._split(v)
            slots.append(int(s)); data.append(d); flush.append(f)
        Cn = self.model.config.channels
        if self.decode:
            data = [[] if d is None else list(d) for d in data]
            for fl in data:
                for f in fl:
                    if f.codes is None or f.codes.ndim != 3 or f.codes.shape[0] != 1 or f.codes.shape[1] != self.n_q:
                        raise ValueError(f"Invalid frame codes: every frame must be [1, {self.n_q}, T']")
            n_in = [len(d) for d in data]
            lens = [int(f.codes.shape[-1]) for fl in data for f in fl]
            some = [f.codes for fl in data for f in fl]
        else:
            for d in data:
                if d is not None and (d.ndim != 2 or d.shape[0] != Cn):
                    raise ValueError(f"every push must be [{Cn}, n]")
            n_in = [0 if d is None else int(d.shape[1]) for d in data]
            lens = None
            some = [d for d in data if d is not None]
        if some:
            self._torch = _is_torch(some[0])
        return slots, data, flush, n_in, lens

    def query(self, entries: dict) -> dict:
        """{slot: (n_frames, code_frames, n_samples)} of the step these entries would be (nc_encodec_stream_pool_query)."""
        slots, _, flush, n_in, lens = self._entries(entries)
        return dict(zip(slots, zip(*self._query(slots, flush, n_in, lens))))

    def _query(self, slots, flush, n_in, lens):
        n = len(slots)
        nf, cf, ns = (C.c_int32 * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
        _lib.check(self._sym("query")(self._p, n, *self._c(slots, n_in, flush), _lib.i64_array(lens) if lens is not None else None, nf, cf, ns))
        return [int(x) for x in nf], [int(x) for x in cf], [int(x) for x in ns]

    def plan(self, entries: dict):
        """(plan, rows in launch order) of the step these entries would be under the pool's current state (nc_encodec_stream_pool_plan):
        as encodec_stream_plan reports them, `clip` being the entry's index."""
        slots, _, flush, n_in, lens = self._entries(entries)
        return self._plan(slots, flush, n_in, lens)

    def _plan(self, slots, flush, n_in, lens):
        n = len(slots)
        c_slots, c_n_in, c_flush = self._c(slots, n_in, flush)
        c_lens = _lib.i64_array(lens) if lens is not None else None
        return _ragged_rows(lambda _n, _l, p, rows, cap: self._sym("plan")(self._p, n, c_slots, c_n_in, c_flush, c_lens, p, rows, cap),
                            [], self.decode)

    def step(self, entries: dict, return_emb: bool = False) -> dict:
        slots, data, flush, n_in, lens = self._entries(entries)
        n = len(slots)
        nf, cf, ns = self._query(slots, flush, n_in, lens)                 # every refusal that needs no device, and the sizes
        m = self.model
        Cn, D, nq = m.config.channels, m.config.dimension, (self.n_q if self.decode else m.query(1)[1])
        c_slots, c_n_in, c_flush = self._c(slots, n_in, flush)
        c_lens = _lib.i64_array(lens) if lens is not None else None
        seg_frames = None
        if not self.decode:                                                 # code frames of every segment an entry emits, in segment order
            seg_frames = [[] for _ in slots]
            for r in sorted(self._plan(slots, flush, n_in, lens)[1], key=lambda r: (r["clip"], r["segment"])):
                seg_frames[r["clip"]].append(r["frames"])
        empty, ptr, cat, f32, i64, fn = self._io()
        if self.decode:
            codes = cat([f.codes for fl in data for f in fl], i64)
            scales = cat([f.scale for fl in data for f in fl], f32) if m.config.normalize else None
            out = empty(Cn * sum(ns), f32)
            _lib.check(fn(self._p, n, c_slots, c_n_in, c_flush, c_lens, ptr(codes), ptr(scales), ptr(out), None, None, Cn * sum(ns), None, None))
            return {s: p.reshape(Cn, -1) for s, p in zip(slots, _lib.split_packed(out, [Cn * k for k in ns]))}
        pcm = cat([d for d in data if d is not None], f32)
        codes, scales = empty(nq * sum(cf), i64), empty(sum(nf), f32)
        emb = empty(D * sum(cf), f32) if return_emb else None
        _lib.check(fn(self._p, n, c_slots, c_n_in, c_flush, None, ptr(pcm), None, ptr(codes), ptr(scales), ptr(emb), nq * sum(cf), None, None))
        res, embs, o, osc = {}, {}, 0, 0
        for s, fr in zip(slots, seg_frames):
            frames, es = [], []
            for Tf in fr:
                frames.append(EncodedFrame(codes[nq * o:nq * (o + Tf)].reshape(1, nq, Tf), scales[osc:osc + 1].reshape(1, 1) if m.config.normalize else None))
                if return_emb:
                    es.append(emb[D * o:D * (o + Tf)].reshape(1, D, Tf))
                o += Tf
                osc += 1
            res[s], embs[s] = frames, es
        return (res, embs) if return_emb else res


class EncodecStreamSession(_EncodecPoolSession):
    """One live stream: a stream pool with one slot.  push(x) -> what became final; flush([x]) ends the stream; reset() starts anew."""


def _causal_rows(call):
    """rows of one of the two causal planner entry points; call(rows, cap, n_rows, n_batches) -> status"""
    nr, nb = C.c_int64(), C.c_int64()
    _lib.check(call(None, 0, C.byref(nr), C.byref(nb)))
    rows = (_lib.NcEncodecCausalRow * max(1, int(nr.value)))()
    _lib.check(call(rows, int(nr.value), C.byref(nr), C.byref(nb)))
    return int(nb.value), [{k: int(getattr(rows[i], k)) for k, _ in _lib.NcEncodecCausalRow._fields_} for i in range(int(nr.value))]


def encodec_causal_plan(config: EncodecConfig, received=(0,), emitted=(0,), n_in=(0,), flush=None, decode: bool = False, max_rows: int = 0):
    """nc_encodec_causal_plan: one step of a causal pool from a config alone, no device needed.  Stream i has received received[i] samples
    (decode: code frames) and emitted emitted[i] frames (decode: decoded that many); it now brings n_in[i] more and flushes where flush[i].
    -> (info dict: hop, halo_e, halo_d, min_frames_e, min_frames_d, carry_e, carry_d, taint_e, taint_d; n_batches; rows in launch order --
    `entry` is the stream's index --; per stream the frames (decode: samples per channel) it emits)."""
    c = _c_config(config)
    n = len(n_in)
    re_, em, ni = _lib.i64_array(received), _lib.i64_array(emitted), _lib.i64_array(n_in)
    fl = (C.c_int32 * max(1, n))(*[int(bool(f)) for f in flush]) if flush is not None else None
    info = _lib.NcEncodecCausalInfo()
    n_out = (C.c_int64 * max(1, n))()
    call = lambda rows, cap, nr, nb: _lib.lib().nc_encodec_causal_plan(C.byref(c), 1 if decode else 0, n, re_, em, ni, fl, int(max_rows), C.byref(info), rows, cap, nr, nb, n_out)  # noqa: E731
    n_batches, rows = _causal_rows(call)
    return {k: int(getattr(info, k)) for k, _ in _lib.NcEncodecCausalInfo._fields_}, n_batches, rows, [int(n_out[i]) for i in range(n)]


class EncodecCausalPool(_EncodecPool):
    """n_slots independent live streams on one causal Encodec model without segmentation (the 24 kHz preset), one direction, stepped
    together (nc_encodec_causal_pool_*; Encodec.Encode / Encodec.Decode with SLSTM.forward's state carried).

        out = pool.step({slot: x | FLUSH | (x, FLUSH), ...})

    encode pool: x is PCM [channels, n] (any n >= 0); out[slot] is codes [1, n_q, F] int64 of the frames that became final -- F is often 0.
    decode pool: x is codes [1, n_q, n] (or [n_q, n]); out[slot] is PCM [channels, n_out].  FLUSH ends the slot's stream (after the x of a
    tuple) and emits the rest; reset_slot() makes the slot new.  Everything a slot emitted, end to end, equals encode() / decode() on the
    whole stream, bit for bit.  numpy in, numpy out (host API); torch device tensors in, device tensors out on torch's current stream."""

    _PREFIX = "causal"

    def _entries(self, entries: dict):
        if not entries:
            raise ValueError("a step needs at least one entry")
        slots, data, flush = [], [], []
        rows = self.n_q if self.decode else self.model.config.channels
        for s, v in entries.items():
            d, f = self._split(v)
            if d is not None:
                if self.decode and d.ndim == 3 and d.shape[0] == 1:
                    d = d[0]
                if d.ndim != 2 or d.shape[0] != rows:
                    raise ValueError(f"every push must be [{rows}, n]")
            slots.append(int(s)); data.append(d); flush.append(f)
        some = [d for d in data if d is not None]
        if some:
            self._torch = _is_torch(some[0])
        return slots, data, flush, [0 if d is None else int(d.shape[1]) for d in data]

    def query(self, entries: dict) -> dict:
        """{slot: code frames (decode pool: samples per channel) the entry would emit} (nc_encodec_causal_pool_query)"""
        slots, _, flush, n_in = self._entries(entries)
        return dict(zip(slots, self._query(slots, flush, n_in)))

    def _query(self, slots, flush, n_in):
        n = len(slots)
        c_slots, c_n_in, c_flush = self._c(slots, n_in, flush)
        n_out = (C.c_int64 * n)()
        _lib.check(self._sym("query")(self._p, n, c_slots, c_n_in, c_flush, n_out))
        return [int(x) for x in n_out]

    def plan(self, entries: dict):
        """(n_batches, rows in launch order) of the step these entries would be under the pool's current state
        (nc_encodec_causal_pool_plan): as encodec_causal_plan reports them, `entry` being the entry's index."""
        slots, _, flush, n_in = self._entries(entries)
        n = len(slots)
        c_slots, c_n_in, c_flush = self._c(slots, n_in, flush)
        return _causal_rows(lambda rows, cap, nr, nb: self._sym("plan")(self._p, n, c_slots, c_n_in, c_flush, rows, cap, nr, nb))

    def step(self, entries: dict, return_emb: bool = False):
        slots, data, flush, n_in = self._entries(entries)
        n = len(slots)
        n_out = self._query(slots, flush, n_in)                            # every refusal that needs no device, and the sizes
        m = self.model
        Cn, D = m.config.channels, m.config.dimension
        nq = self.n_q if self.decode else m.query(1)[1]
        c_slots, c_n_in, c_flush = self._c(slots, n_in, flush)
        empty, ptr, cat, f32, i64, fn = self._io()
        some = [d for d in data if d is not None]
        if self.decode:
            codes = cat(some, i64)
            out = empty(Cn * sum(n_out), f32)
            _lib.check(fn(self._p, n, c_slots, c_n_in, c_flush, ptr(codes), ptr(out), None, Cn * sum(n_out), None))
            return {s: p.reshape(Cn, -1) for s, p in zip(slots, _lib.split_packed(out, [Cn * k for k in n_out]))}
        pcm = cat(some, f32)
        codes = empty(nq * sum(n_out), i64)
        emb = empty(D * sum(n_out), f32) if return_emb else None
        _lib.check(fn(self._p, n, c_slots, c_n_in, c_flush, ptr(pcm), ptr(codes), ptr(emb), nq * sum(n_out), None))
        res = {s: p.reshape(1, nq, -1) for s, p in zip(slots, _lib.split_packed(codes, [nq * k for k in n_out]))}
        if not return_emb:
            return res
        return res, {s: p.reshape(1, D, -1) for s, p in zip(slots, _lib.split_packed(emb, [D * k for k in n_out]))}


class EncodecCausalSession(_EncodecPoolSession):
    """One live causal stream: a causal pool with one slot.  push(x) -> what became final; flush([x]) ends the stream; reset() starts anew."""
