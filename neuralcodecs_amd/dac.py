"""Host-side mirror of the reference's ``DAC`` model class over the C ABI.

Same members, argument meaning and error behaviour as NeuralCodecs.Torch/Models/DAC.cs
(``DAC : Module<Tensor, Dictionary<string,Tensor>>, INeuralCodec``):

    DAC(config)                      DAC.cs:51-93
    load_weights(path)               DAC.cs:345-389   (INeuralCodec.LoadWeights)
    encode(audio, n_quantizers, sample_rate) -> (z, codes, latents, commitment_loss, codebook_loss)   DAC.cs:163-181
    encode_array(float[]) -> float[] (the zQ latents, D12)                                            DAC.cs:205-224
    decode(z) / decode_array(float[])                                                                 DAC.cs:231-253
    from_codes(codes)                                                                                 DAC.cs:101-106
    from_latents(latents) -> (z_q, projected, codes)                  Modules/DAC/ResidualVectorQuantizer.cs:243-300
    forward(audio) -> dict                                                                            DAC.cs:288-303
    dispose()                                                                                         DAC.cs:329-338

Inputs may be numpy arrays (host API: synchronous, returns numpy) or torch CUDA tensors
(device API: zero-copy, enqueued on torch's current stream, returns torch tensors).  All compute
happens in libnc_mi355x.so; nothing here touches the oracle or torch operators.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .config import DACConfig
from .weights import save_blob


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _c_config(config: DACConfig) -> "_lib.NcDacConfig":
    c = _lib.NcDacConfig()
    c.sample_rate, c.encoder_dim, c.decoder_dim = config.sample_rate, config.encoder_dim, config.decoder_dim
    c.n_encoder_rates, c.n_decoder_rates = len(config.encoder_rates), len(config.decoder_rates)
    for i, r in enumerate(config.encoder_rates):
        c.encoder_rates[i] = r
    for i, r in enumerate(config.decoder_rates):
        c.decoder_rates[i] = r
    c.latent_dim = config.latent_dim or 0
    c.n_codebooks, c.codebook_size, c.codebook_dim = config.n_codebooks, config.codebook_size, config.codebook_dim
    return c


def dac_halo(config: DACConfig) -> dict:
    """nc_dac_halo: the frames a chunk of a long clip recomputes on each side, derived from the config alone (no device needed)."""
    h = _lib.NcHalo()
    _lib.check(_lib.lib().nc_dac_halo(C.byref(_c_config(config)), C.byref(h)))
    return {k: int(getattr(h, k)) for k, _ in _lib.NcHalo._fields_}


def dac_ragged_windows(config: DACConfig, frames, decode: bool = False, kept_frames: int = 0, max_windows: int = 0):
    """nc_dac_ragged_windows: the window layout of a ragged call on clips of these frame counts (no device needed)."""
    return _lib.ragged_windows(_lib.lib().nc_dac_ragged_windows, _c_config(config), frames, decode, kept_frames, max_windows)


class DAC(_lib.ProfileMixin):
    def __init__(self, config: Optional[DACConfig] = None, device_index: int = 0):
        if config is None:
            raise ValueError("config must not be null")  # ArgumentNullException.ThrowIfNull(config)
        self.config = config
        self.device_index = device_index
        c = _c_config(config)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().nc_dac_create(C.byref(c), device_index, C.byref(self._h)))
        self.latent_dim = config.resolved_latent_dim
        self.hop_length = config.hop_length

    # ---- INeuralCodec ----------------------------------------------------------------------
    @property
    def Config(self) -> DACConfig:
        return self.config

    def load_weights(self, path: str) -> None:
        _lib.check(_lib.lib().nc_codec_load_weights(self._h, str(path).encode()))

    def load_state_dict(self, state_dict) -> None:
        """TorchSharp-keyed tensors (weight_v/weight_g/bias/alpha/codebook.weight) -> engine."""
        blob = save_blob(state_dict)
        self.load_blob(blob)

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

    # ---- helpers ---------------------------------------------------------------------------
    def frames(self, T: int) -> int:
        return -(-T // self.hop_length)

    def decoded_length(self, frames: int) -> int:
        L = frames
        for s in self.config.decoder_rates:
            L = (L - 1) * s - 2 * ((s + 1) // 2) + 2 * s
        return L

    def _nq(self, n_quantizers) -> int:
        n = self.config.n_codebooks
        return n if (n_quantizers is None or n_quantizers <= 0 or n_quantizers > n) else int(n_quantizers)

    def _bind_torch_stream(self):
        import torch
        _lib.check(_lib.lib().nc_codec_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device_index).cuda_stream)))   # (the handle's OWN device: one process may drive several)

    def synchronize(self) -> None:
        _lib.check(_lib.lib().nc_codec_synchronize(self._h))

    # ---- Encode ----------------------------------------------------------------------------
    def encode(self, audio_data, n_quantizers: Optional[int] = None, sample_rate: Optional[int] = None):
        if audio_data is None:
            raise ValueError("audio_data must not be null")
        if audio_data.ndim != 3 or audio_data.shape[1] != 1:
            raise ValueError("audio must be [B,1,T]")
        B, _, T = audio_data.shape
        nq, Tz, D = self._nq(n_quantizers), self.frames(T), self.config.codebook_dim
        sr = 0 if sample_rate is None else int(sample_rate)
        if _is_torch(audio_data):
            import torch
            x = audio_data.contiguous().to(torch.float32)
            codes = torch.empty((B, nq, Tz), dtype=torch.int64, device=x.device)
            z = torch.empty((B, self.latent_dim, Tz), dtype=torch.float32, device=x.device)
            lat = torch.empty((B, nq * D, Tz), dtype=torch.float32, device=x.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_dac_encode_dev(self._h, x.data_ptr(), B, T, sr, nq, codes.data_ptr(), z.data_ptr(),
                                                    lat.data_ptr()))
            # commitment / codebook loss: 0 in eval mode (ResidualVectorQuantizer.cs:143-156).  Fresh, distinct tensors on every call, as
            # in the reference: a caller may accumulate into them in place (two scalar fills; a cached pair would be shared state)
            return z, codes, lat, torch.zeros((), device=x.device), torch.zeros((), device=x.device)
        x = np.ascontiguousarray(audio_data, dtype=np.float32)
        codes = np.empty((B, nq, Tz), np.int64)
        z = np.empty((B, self.latent_dim, Tz), np.float32)
        lat = np.empty((B, nq * D, Tz), np.float32)
        _lib.check(_lib.lib().nc_dac_encode(self._h, x.ctypes.data, B, T, sr, nq, codes.ctypes.data, z.ctypes.data, lat.ctypes.data))
        return z, codes, lat, np.float32(0.0), np.float32(0.0)

    def encode_audio(self, audio_data):
        """DAC.EncodeAudio (DAC.cs:188-199): zQ only."""
        return self.encode(audio_data)[0]

    def encode_array(self, audio_data) -> np.ndarray:
        """DAC.Encode(float[]) (DAC.cs:205-224): B=1 host wrapper returning the flattened zQ latents (D12)."""
        if audio_data is None:
            raise ValueError("audio_data must not be null")
        x = np.asarray(audio_data, dtype=np.float32).reshape(1, 1, -1)
        return self.encode(x)[0].reshape(-1)

    # ---- Decode ----------------------------------------------------------------------------
    def decode(self, q_audio):
        if q_audio is None:
            raise ValueError("q_audio must not be null")
        if q_audio.ndim != 3 or q_audio.shape[1] != self.latent_dim:
            raise ValueError(f"latents must be [B,{self.latent_dim},T']")
        B, _, Tz = q_audio.shape
        L = self.decoded_length(Tz)
        if _is_torch(q_audio):
            import torch
            z = q_audio.contiguous().to(torch.float32)
            out = torch.empty((B, 1, L), dtype=torch.float32, device=z.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_dac_decode_dev(self._h, z.data_ptr(), B, Tz, out.data_ptr()))
            return out
        z = np.ascontiguousarray(q_audio, dtype=np.float32)
        out = np.empty((B, 1, L), np.float32)
        _lib.check(_lib.lib().nc_dac_decode(self._h, z.ctypes.data, B, Tz, out.ctypes.data))
        return out

    def decode_array(self, q_audio) -> np.ndarray:
        """DAC.Decode(float[]) (DAC.cs:241-253): reshape(1, latent, -1) then decode."""
        if q_audio is None:
            raise ValueError("q_audio must not be null")
        z = np.asarray(q_audio, dtype=np.float32).reshape(1, self.latent_dim, -1)
        return self.decode(z).reshape(-1)

    def from_codes(self, codes):
        if codes is None:
            raise ValueError("codes must not be null")
        if codes.ndim != 3:
            raise ValueError("codes must be [B,n_q,T']")
        B, nq, Tz = codes.shape
        if _is_torch(codes):
            import torch
            c = codes.contiguous().to(torch.int64)
            z = torch.empty((B, self.latent_dim, Tz), dtype=torch.float32, device=c.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_dac_from_codes_dev(self._h, c.data_ptr(), B, nq, Tz, z.data_ptr()))
            return z
        c = np.ascontiguousarray(codes, dtype=np.int64)
        z = np.empty((B, self.latent_dim, Tz), np.float32)
        _lib.check(_lib.lib().nc_dac_from_codes(self._h, c.ctypes.data, B, nq, Tz, z.ctypes.data))
        return z

    def from_latents(self, latents):
        """ResidualVectorQuantizer.FromLatents (Modules/DAC/ResidualVectorQuantizer.cs:243-300): latents [B, C, T'] (the `latents` of
        encode(), or any continuous vectors in that space) -> (z_q [B, latent, T'], projected [B, n_q*D, T'], codes [B, n_q, T']) with
        n_q = min(n_codebooks, C // D).  Clips of unequal lengths: concatenate them along T' into one B = 1 call."""
        if latents is None:
            raise ValueError("latents must not be null")
        if latents.ndim != 3:
            raise ValueError("latents must be [B,C,T']")
        B, Cl, Tz = (int(v) for v in latents.shape)
        D = self.config.codebook_dim
        nq = max(1, min(self.config.n_codebooks, Cl // D))          # (Cl < D: the engine refuses before it writes anything)
        if _is_torch(latents):
            import torch
            x = latents.contiguous().to(torch.float32)
            z = torch.empty((B, self.latent_dim, Tz), dtype=torch.float32, device=x.device)
            proj = torch.empty((B, nq * D, Tz), dtype=torch.float32, device=x.device)
            codes = torch.empty((B, nq, Tz), dtype=torch.int64, device=x.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_dac_from_latents_dev(self._h, x.data_ptr(), B, Cl, Tz, z.data_ptr(), proj.data_ptr(), codes.data_ptr()))
            return z, proj, codes
        x = np.ascontiguousarray(latents, dtype=np.float32)
        z = np.empty((B, self.latent_dim, Tz), np.float32)
        proj = np.empty((B, nq * D, Tz), np.float32)
        codes = np.empty((B, nq, Tz), np.int64)
        _lib.check(_lib.lib().nc_dac_from_latents(self._h, x.ctypes.data, B, Cl, Tz, z.ctypes.data, proj.ctypes.data, codes.ctypes.data))
        return z, proj, codes

    # ---- ragged batches (clips of unequal lengths in one call) ------------------------------------
    @staticmethod
    def _pack(clips, dtype: str):
        """list of arrays / tensors -> (one packed 1-D buffer, is_torch)"""
        if clips is None or len(clips) == 0:
            raise ValueError("the list of clips must not be empty")
        if _is_torch(clips[0]):
            import torch
            return torch.cat([c.reshape(-1).to(getattr(torch, dtype)) for c in clips]).contiguous(), True
        return np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=dtype).reshape(-1) for c in clips])), False

    def encode_ragged(self, clips, n_quantizers: Optional[int] = None):
        """nc_dac_encode_ragged[_dev]: 1-D clips of any lengths -> list of codes [n_q, F_b]; clip b's codes are those of encode() on
        that clip alone, bit for bit."""
        flat, dev = self._pack(clips, "float32")
        B, nq = len(clips), self._nq(n_quantizers)
        lens = [int(c.shape[-1]) if c.ndim else 0 for c in clips]
        if any(c.ndim != 1 for c in clips):
            raise ValueError("every clip must be 1-D")
        sizes = [nq * self.frames(t) for t in lens]
        if dev:
            import torch
            codes = torch.empty(max(1, sum(sizes)), dtype=torch.int64, device=flat.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_dac_encode_ragged_dev(self._h, flat.data_ptr(), B, _lib.i64_array(lens), 0, nq, codes.data_ptr()))
        else:
            codes = np.empty(max(1, sum(sizes)), np.int64)
            _lib.check(_lib.lib().nc_dac_encode_ragged(self._h, flat.ctypes.data, B, _lib.i64_array(lens), 0, nq, codes.ctypes.data))
        return [c.reshape(nq, -1) for c in _lib.split_packed(codes, sizes)]

    def decode_codes_ragged(self, codes):
        """nc_dac_decode_codes_ragged[_dev]: list of codes [n_q, F_b] -> list of 1-D pcm (FromCodes then Decode), each the
        decode(from_codes()) of that clip alone, bit for bit."""
        if codes is None or len(codes) == 0:
            raise ValueError("the list of codes must not be empty")
        if any(c.ndim != 2 or c.shape[0] != codes[0].shape[0] for c in codes):
            raise ValueError("every clip's codes must be [n_q, F] with one n_q")
        flat, dev = self._pack(codes, "int64")
        B, nq = len(codes), int(codes[0].shape[0])
        frames = [int(c.shape[1]) for c in codes]
        sizes = [self.decoded_length(f) for f in frames]
        if dev:
            import torch
            pcm = torch.empty(max(1, sum(sizes)), dtype=torch.float32, device=flat.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_dac_decode_codes_ragged_dev(self._h, flat.data_ptr(), B, _lib.i64_array(frames), nq, pcm.data_ptr()))
        else:
            pcm = np.empty(max(1, sum(sizes)), np.float32)
            _lib.check(_lib.lib().nc_dac_decode_codes_ragged(self._h, flat.ctypes.data, B, _lib.i64_array(frames), nq, pcm.ctypes.data))
        return _lib.split_packed(pcm, sizes)

    def round_trip_quality(self, pcm_list, n_quantizers: Optional[int] = None, scales=None):
        """Encode -> decode -> nc_quality_metrics_dev on a list of clips of any lengths, everything on the device: per row (one channel of
        one clip) l1, si_sdr_db, mel_distance, mel_log / mel_mag and n_bad of the decode against the clip (neuralcodecs_amd/quality.py;
        scales: a QualityConfig, default the DAC paper's evaluation set).  numpy clips in, numpy out; device tensors in, tensors out."""
        from . import quality
        clips, was_torch = quality.on_device(pcm_list)
        dec = self.decode_codes_ragged(self.encode_ragged(clips, n_quantizers))
        ref, est = quality.round_trip_rows(clips, dec)
        return quality.hand_back(quality.quality_metrics(ref, est, sample_rate=self.config.sample_rate, scales=scales), was_torch)

    def normalize_ragged(self, clips, target_db: float = -24.0, filter: str = "reference", host: bool = False):
        """nc_loudness_normalize_dev on 1-D clips of any lengths at the model's sample rate (neuralcodecs_amd/loudness.py): the levelled
        clips, views of one packed buffer and ready for encode_ragged, and the per-clip rows (lufs, gain, ...) to store."""
        from . import loudness
        return loudness.normalize_ragged(clips, self.config.sample_rate, target_db, filter, host)

    def resample_ragged(self, clips, sample_rate: int, host: bool = False):
        """nc_audio_resample_sinc_dev on 1-D clips of any lengths at `sample_rate` (neuralcodecs_amd/resample.py): the clips at the model's
        sample rate, views of one packed buffer and ready for normalize_ragged / encode_ragged."""
        from . import resample
        return resample.resample_ragged(clips, sample_rate, self.config.sample_rate, host)

    def restore_ragged(self, decoded, rows, host: bool = False):
        """nc_audio_apply_gain_db_dev: the decoded clips back at the levels normalize_ragged measured (rows: what it returned)."""
        from . import loudness
        return loudness.restore_ragged(decoded, rows, host)

    # ---- incremental sessions (codes or PCM pushed as they arrive) ---------------------------------
    def decode_session(self, B: int, n_quantizers: Optional[int] = None):
        """nc_session_create(decode): push codes [B, n_q, n] as a model emits them, get the PCM that became final; the pieces
        concatenated are decode(from_codes(all codes)), bit for bit (neuralcodecs_amd/session.py)."""
        from .session import Session
        return Session(self, True, B, self._nq(n_quantizers))

    def encode_session(self, B: int):
        """nc_session_create(encode): push PCM [B, 1, n] of any length as it is recorded, get the codes [B, n_codebooks, n_out] that
        became final; the pieces concatenated are the codes of encode() on the whole clip, bit for bit."""
        from .session import Session
        return Session(self, False, B, 0)

    # ---- session pools (many independent streams stepped in one batch) ------------------------------
    def decode_pool(self, n_slots: int, n_q: Optional[int] = None):
        """nc_session_pool_create(decode): n_slots independent decode streams reading n_q codebooks; one step() advances any subset of
        them, each by its own amount, and every slot returns what a B = 1 decode_session returns for the same pushes, bit for bit
        (neuralcodecs_amd/session.py)."""
        from .session import SessionPool
        return SessionPool(self, True, n_slots, self._nq(n_q))

    def encode_pool(self, n_slots: int):
        """nc_session_pool_create(encode): n_slots independent encode streams (SessionPool)."""
        from .session import SessionPool
        return SessionPool(self, False, n_slots, 0)

    # ---- Dia <-> DAC glue -----------------------------------------------------------
    def decode_code_matrix(self, audio_codes):
        """Dia.Decode (Models/Dia.cs:973-981): codes [T, n_q] (or batched [B, T, n_q]) -> FromCodes -> Decode -> waveform
        [T*hop] (or [B, T*hop]).  One C-ABI call (nc_dac_decode_code_matrix[_dev]): the transpose to the engine's [B, n_q, T] is a
        device kernel, batched clips decode in one launch set."""
        if audio_codes is None:
            raise ValueError("audio_codes must not be null")
        single = audio_codes.ndim == 2
        c = audio_codes[None] if single else audio_codes
        if c.ndim != 3:
            raise ValueError("codes must be [T, n_q] or [B, T, n_q]")
        B, Tz, nq = (int(v) for v in c.shape)
        L = self.decoded_length(Tz)
        if _is_torch(c):
            import torch
            cc = c.contiguous().to(torch.int64)
            audio = torch.empty((B, L), dtype=torch.float32, device=cc.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_dac_decode_code_matrix_dev(self._h, cc.data_ptr(), B, Tz, nq, audio.data_ptr()))
        else:
            cc = np.ascontiguousarray(c, dtype=np.int64)
            audio = np.empty((B, L), np.float32)
            _lib.check(_lib.lib().nc_dac_decode_code_matrix(self._h, cc.ctypes.data, B, Tz, nq, audio.ctypes.data))
        return audio[0] if single else audio

    def encode_to_code_matrix(self, audio, sample_rate: Optional[int] = None):
        """Dia.Encode (Models/Dia.cs:989-1002): audio [C=1, T] (or [B, 1, T]) -> Encode -> codes [T', n_q] (or [B, T', n_q]);
        one C-ABI call (nc_dac_encode_code_matrix[_dev])."""
        if audio is None:
            raise ValueError("audio must not be null")
        single = audio.ndim == 2
        a = audio[None] if single else audio
        if a.ndim != 3 or a.shape[1] != 1:
            raise ValueError("audio must be [1, T] or [B, 1, T]")
        sr = self.config.sample_rate if sample_rate is None else int(sample_rate)
        B, _, T = (int(v) for v in a.shape)
        Tz, nq = self.frames(T), self.config.n_codebooks
        if _is_torch(a):
            import torch
            x = a.contiguous().to(torch.float32)
            codes = torch.empty((B, Tz, nq), dtype=torch.int64, device=x.device)
            self._bind_torch_stream()
            _lib.check(_lib.lib().nc_dac_encode_code_matrix_dev(self._h, x.data_ptr(), B, T, sr, codes.data_ptr()))
        else:
            x = np.ascontiguousarray(a, dtype=np.float32)
            codes = np.empty((B, Tz, nq), np.int64)
            _lib.check(_lib.lib().nc_dac_encode_code_matrix(self._h, x.ctypes.data, B, T, sr, codes.ctypes.data))
        return codes[0] if single else codes

    def decode_dia_output(self, codes_delayed, lengths, delay_pattern, speed=None, valid_range=(0, 1023)):
        """Dia.GenerateOutput (Models/Dia.cs:1010-1093): delayed codes [B, T_gen, C] and the valid length of every item -> list of
        waveforms.  The delay pattern is undone, the last max(delay) steps cut and codes outside valid_range (Dia.cs:53-58) set to 0 in
        one launch that writes the packed ragged layout; all items decode as one ragged batch, each at its own length; speed (one
        factor or one per item, Dia.AdjustSpeed) stretches the waveforms by linear interpolation (neuralcodecs_amd/dia.py)."""
        from .dia import decode_dia_output
        return decode_dia_output(self, codes_delayed, lengths, delay_pattern, speed, valid_range)

    def encode_dia_prompts(self, prompts, batch_size=None, delay_pattern=(0, 8, 9, 10, 11, 12, 13, 14, 15), bos=1026, pad=-1, channels=None):
        """Dia.LoadAudio's mono mix, Dia.Encode and Dia.PrepareAudioPrompt (Models/Dia.cs:827-877, 988-1001, 329-400): a list of 1-D voice
        prompts (None: no prompt) -> (delayed prefill int32 [B, T_max, C], prefill steps), B = max(batch_size, len(prompts)).  All prompts
        encode as one ragged batch, each at its own length, and one launch writes the prefill with its BOS rows and -1 fill; device
        tensors stay on the device.  The prompts are not resampled, as in the reference (neuralcodecs_amd/dia.py)."""
        from .dia import encode_dia_prompts
        return encode_dia_prompts(self, prompts, batch_size, delay_pattern, bos, pad, channels)

    @staticmethod
    def decode_one_frame(model: "DAC", audio_codes):
        """Modules/Dia/AudioUtils.cs:189-199: exactly one [1, n_q, T] frame -> FromCodes -> Decode."""
        if audio_codes.shape[0] != 1:
            raise ValueError(f"Expected one frame, got {audio_codes.shape[0]}")
        return model.decode(model.from_codes(audio_codes))

    # ---- forward ---------------------------------------------------------------------------
    def forward(self, audio_data, sample_rate: Optional[int] = None, n_quantizers: Optional[int] = None):
        z, codes, latents, cl, cbl = self.encode(audio_data, n_quantizers, sample_rate)
        audio = self.decode(z)
        return {"audio": audio, "z": z, "codes": codes, "latents": latents, "vq/commitment_loss": cl, "vq/codebook_loss": cbl}

    def forward_array(self, audio_data) -> np.ndarray:
        """DAC.forward(float[]) (DAC.cs:310-322)."""
        if audio_data is None:
            raise ValueError("audio_data must not be null")
        x = np.asarray(audio_data, dtype=np.float32).reshape(1, 1, -1)
        return self.forward(x)["audio"].reshape(-1)

    # ---- profiling (bench.py) ----------------------------------------------------------------
