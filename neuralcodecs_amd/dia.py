"""Dia's output stage on the device (csrc/nc_dia.hip): the steps the reference runs on either side of DAC in its one production caller.

Mirror of the reference's helpers (same argument meaning):
    dia_apply_delay(codes, delay_pattern, bos, pad)    AudioUtils.BuildDelayIndices / ApplyAudioDelay    Modules/Dia/AudioUtils.cs:19-94
    dia_revert_delay(codes, delay_pattern, valid)      AudioUtils.BuildRevertIndices / RevertAudioDelay  Modules/Dia/AudioUtils.cs:108-176
                                                       + the cut and the mask of Dia.GenerateOutput      Models/Dia.cs:1039-1044
    adjust_speed(rows, speed)                          Dia.AdjustSpeed / TorchUtils.Interp               Models/Dia.cs:947-966
    DAC.decode_dia_output(...)                         Dia.GenerateOutput                                Models/Dia.cs:1010-1093
and of the prompt stage in front of the language model:
    mix_to_mono_ragged(prompts, channels)              Dia.LoadAudio's mono mix                          Models/Dia.cs:851-864
    dia_prefill_pack(codes, delay_pattern, bos, pad)   Dia.PrepareAudioPrompt (+ ApplyAudioDelay)        Models/Dia.cs:329-400
    DAC.encode_dia_prompts(...)                        LoadAudio's mix, Dia.Encode, PrepareAudioPrompt   Models/Dia.cs:827-877, 988-1001, 329-400
and of the sampling stage behind the language model:
    dia_sample_next_token(logits, uniform, ...)        Dia.DecoderStep from the logits on, SampleNextToken  Models/Dia.cs:530-560, 424-501
    dia_sample_host(logits, uniform, ...)              the same bits in serial C++ on the host -- the one call here that needs no device
    DiaGeneration(...).step / .finish                  the loop of Dia.Generate around a caller's model     Models/Dia.cs:664-801

torch device tensors stay on the device (zero-copy, torch's current stream); numpy arrays are copied in and out, as in audio.py.  There
is no CPU implementation here: without the HIP library and a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .audio import _is_torch, _torch

# Dia.cs:53-58: MinValidCodebookIndex = 0, MaxValidCodebookIndex = 1023
VALID_RANGE = (0, 1023)


def _i32_array(values):
    v = [int(x) for x in values]
    return (C.c_int32 * len(v))(*v)


def _f32_array(values):
    v = [float(x) for x in values]
    return (C.c_float * len(v))(*v)


def _speeds(speed, B):
    """None, one factor for all items or one per item -> a host float array (or None)"""
    if speed is None:
        return None
    s = [float(speed)] * B if np.ndim(speed) == 0 else [float(x) for x in speed]
    if len(s) != B:
        raise ValueError("one speed factor per item")
    return _f32_array(s)


def adjust_speed_len(L: int, speed: float) -> int:
    """nc_dia_adjust_speed_len: samples Dia.AdjustSpeed returns for L samples at this speed factor (host arithmetic, no device)."""
    n = int(_lib.lib().nc_dia_adjust_speed_len(int(L), float(speed)))
    if n < 0:
        raise ValueError(f"{L} samples at speed {speed} have no length")
    return n


def _on_device(x, np_dtype, torch_dtype_name):
    """x -> (contiguous device tensor, was_torch)"""
    torch = _torch()
    tdt = getattr(torch, torch_dtype_name)
    if _is_torch(x):
        xt = x.contiguous().to(tdt)
        return (xt if xt.is_cuda else xt.cuda()), True
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np_dtype))).cuda(), False


def _hand_back(out, was_torch):
    if was_torch:
        return out
    _torch().cuda.synchronize(out.device)
    return out.cpu().numpy()


def _codes_btc(codes):
    if codes is None:
        raise ValueError("codes must not be null")
    single = codes.ndim == 2
    c = codes[None] if single else codes
    if c.ndim != 3:
        raise ValueError("codes must be [T, C] or [B, T, C]")
    return c, single


def dia_apply_delay(codes, delay_pattern, bos: int, pad: int = 0):
    """out[b, t, c] = bos where t < delay[c], else codes[b, t - delay[c], c]; codes int64 [B, T, C] (or [T, C])."""
    c, single = _codes_btc(codes)
    B, T, Cn = (int(v) for v in c.shape)
    if len(delay_pattern) != Cn:
        raise ValueError("one delay per channel")
    x, was_torch = _on_device(c, np.int64, "int64")
    torch = _torch()
    out = torch.empty_like(x)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(_lib.lib().nc_dia_apply_delay_dev(x.device.index or 0, x.data_ptr(), B, T, Cn, _i32_array(delay_pattern), int(pad), int(bos),
                                                 out.data_ptr(), stream))
    out = _hand_back(out, was_torch)
    return out[0] if single else out


def dia_revert_delay(codes, delay_pattern, valid_range=VALID_RANGE):
    """codes int64 [B, T, C] (or [T, C]) -> [B, T - max(delay), C]: out[b, t, c] = codes[b, t + delay[c], c], codes outside valid_range
    written as 0 (the matrix Dia.GenerateOutput decodes from)."""
    c, single = _codes_btc(codes)
    B, T, Cn = (int(v) for v in c.shape)
    if len(delay_pattern) != Cn:
        raise ValueError("one delay per channel")
    x, was_torch = _on_device(c, np.int64, "int64")
    torch = _torch()
    out = torch.empty((B, max(0, T - max(int(d) for d in delay_pattern)), Cn), dtype=torch.int64, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(_lib.lib().nc_dia_revert_delay_dev(x.device.index or 0, x.data_ptr(), B, T, Cn, _i32_array(delay_pattern), int(valid_range[0]),
                                                  int(valid_range[1]), out.data_ptr(), stream))
    out = _hand_back(out, was_torch)
    return out[0] if single else out


def dia_revert_pack(codes, lengths, delay_pattern, valid_range=VALID_RANGE):
    """The reverted and masked codes of dia_revert_delay in the packed layout DAC.decode_codes_ragged reads: a list of [C, lengths[b]]."""
    if codes is None or codes.ndim != 3:
        raise ValueError("codes must be [B, T, C]")
    B, T, Cn = (int(v) for v in codes.shape)
    lengths = [int(n) for n in lengths]
    if len(lengths) != B or len(delay_pattern) != Cn:
        raise ValueError("one length per item and one delay per channel")
    x, was_torch = _on_device(codes, np.int64, "int64")
    torch = _torch()
    out = torch.empty(max(1, Cn * sum(max(0, n) for n in lengths)), dtype=torch.int64, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(_lib.lib().nc_dia_revert_pack_dev(x.device.index or 0, x.data_ptr(), B, T, Cn, _i32_array(delay_pattern), _lib.i64_array(lengths),
                                                 int(valid_range[0]), int(valid_range[1]), out.data_ptr(), stream))
    return [p.reshape(Cn, -1) for p in _lib.split_packed(_hand_back(out, was_torch), [Cn * n for n in lengths])]


def adjust_speed(rows, speed):
    """Dia.AdjustSpeed on a list of 1-D waveforms (or one): row b stretched to adjust_speed_len(len, speed[b]) samples by linear
    interpolation; speed is one factor or one per row.  A row whose length does not change comes back as a copy."""
    single = not isinstance(rows, (list, tuple))
    rs = [rows] if single else list(rows)
    if not rs or any(r.ndim != 1 or r.shape[0] == 0 for r in rs):
        raise ValueError("every row must be 1-D and not empty")
    B = len(rs)
    lens = [int(r.shape[0]) for r in rs]
    sp = _speeds(speed, B)
    if sp is None:
        raise ValueError("speed must not be null")
    out_lens = [adjust_speed_len(n, s) for n, s in zip(lens, sp)]
    torch = _torch()
    was_torch = _is_torch(rs[0])
    if was_torch:
        flat = torch.cat([r.to(torch.float32) for r in rs]).contiguous()
        flat = flat if flat.is_cuda else flat.cuda()
    else:
        flat = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(r, np.float32) for r in rs]))).cuda()
    out = torch.empty(sum(out_lens), dtype=torch.float32, device=flat.device)
    stream = torch.cuda.current_stream(flat.device).cuda_stream
    _lib.check(_lib.lib().nc_dia_adjust_speed_dev(flat.device.index or 0, flat.data_ptr(), B, _lib.i64_array(lens), sp, out.data_ptr(), stream))
    pieces = _lib.split_packed(_hand_back(out, was_torch), out_lens)
    return pieces[0] if single else pieces


def output_query(dac, T_gen: int, lengths, delay_pattern, speed=None):
    """nc_dia_output_query: (frames, decoded samples, samples after the speed adjustment) of every item -- host arithmetic."""
    B = len(lengths)
    fr, dl, ol = (C.c_int64 * max(1, B))(), (C.c_int64 * max(1, B))(), (C.c_int64 * max(1, B))()
    _lib.check(_lib.lib().nc_dia_output_query(dac._h, B, int(T_gen), len(delay_pattern), _i32_array(delay_pattern), _lib.i64_array(lengths),
                                              _speeds(speed, B), fr, dl, ol))
    return list(fr)[:B], list(dl)[:B], list(ol)[:B]


def decode_dia_output(dac, codes_delayed, lengths, delay_pattern, speed=None, valid_range=VALID_RANGE):
    """Dia.GenerateOutput: delayed codes int64 [B, T_gen, C] + the valid length of every item -> list of B waveforms.  One revert-and-pack
    launch, the ragged decode of all items, one interpolation launch where a speed factor asks for it (nc_dia_decode_output[_dev])."""
    if codes_delayed is None or codes_delayed.ndim != 3:
        raise ValueError("codes must be [B, T_gen, C]")
    B, T_gen, Cn = (int(v) for v in codes_delayed.shape)
    lengths = [int(n) for n in lengths]
    if len(lengths) != B or len(delay_pattern) != Cn:
        raise ValueError("one length per item and one delay per channel")
    sp = _speeds(speed, B)
    _, _, out_lens = output_query(dac, T_gen, lengths, delay_pattern, speed)
    L = _lib.lib()
    args = (B, T_gen, Cn, _i32_array(delay_pattern), _lib.i64_array(lengths), int(valid_range[0]), int(valid_range[1]), sp)
    if _is_torch(codes_delayed):
        import torch
        c = codes_delayed.contiguous().to(torch.int64)
        pcm = torch.empty(sum(out_lens), dtype=torch.float32, device=c.device)
        dac._bind_torch_stream()
        _lib.check(L.nc_dia_decode_output_dev(dac._h, c.data_ptr(), *args, pcm.data_ptr()))
    else:
        c = np.ascontiguousarray(codes_delayed, dtype=np.int64)
        pcm = np.empty(sum(out_lens), np.float32)
        _lib.check(L.nc_dia_decode_output(dac._h, c.ctypes.data, *args, pcm.ctypes.data))
    return _lib.split_packed(pcm, out_lens)


# ---- prompt stage: voice prompts -> the delayed prefill (nc_dia.hip) -------------------------------------------------------
# DataConfig.DelayPattern / AudioBosValue of the reference's DiaConfig; PrepareAudioPrompt passes padValue -1 (Dia.cs:393-397)
DELAY_PATTERN = (0, 8, 9, 10, 11, 12, 13, 14, 15)
AUDIO_BOS = 1026


def prompt_query(dac, lengths, delay_pattern=DELAY_PATTERN):
    """nc_dia_prompt_query: (frames F_b, prefill steps F_b + 1, T_max = max F_b + max(delay)) for prompts of these lengths in samples
    (0: no prompt) -- host arithmetic."""
    B = len(lengths)
    fr, st, tm = (C.c_int64 * max(1, B))(), (C.c_int32 * max(1, B))(), C.c_int64()
    _lib.check(_lib.lib().nc_dia_prompt_query(dac._h, B, len(delay_pattern), _i32_array(delay_pattern), _lib.i64_array(lengths), fr, st, C.byref(tm)))
    return list(fr)[:B], list(st)[:B], int(tm.value)


def mix_to_mono_ragged(prompts, channels):
    """Dia.LoadAudio's mono mix on a list of interleaved 1-D prompts ([n][ch] flattened; channels: one count per prompt): a binary32
    running sum in channel order, one division; a prompt of one channel comes back as a copy.  One launch per 32 prompts."""
    rs = list(prompts)
    ch = [int(c) for c in channels]
    if not rs or len(ch) != len(rs) or any(r.ndim != 1 for r in rs):
        raise ValueError("a list of 1-D prompts and one channel count per prompt")
    if any(c <= 0 or int(r.shape[0]) % c for r, c in zip(rs, ch)):
        raise ValueError("every prompt holds whole frames of a positive channel count")
    n = [int(r.shape[0]) // c for r, c in zip(rs, ch)]
    torch = _torch()
    was_torch = _is_torch(rs[0])
    if was_torch:
        flat = torch.cat([r.to(torch.float32) for r in rs]).contiguous()
        flat = flat if flat.is_cuda else flat.cuda()
    else:
        flat = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(r, np.float32) for r in rs]))).cuda()
    out = torch.empty(max(1, sum(n)), dtype=torch.float32, device=flat.device)
    stream = torch.cuda.current_stream(flat.device).cuda_stream
    _lib.check(_lib.lib().nc_audio_mix_to_mono_ragged_dev(flat.device.index or 0, flat.data_ptr(), len(rs), _lib.i64_array(n), _i32_array(ch),
                                                          out.data_ptr(), stream))
    return _lib.split_packed(_hand_back(out, was_torch), n)


def dia_prefill_pack(codes, delay_pattern=DELAY_PATTERN, bos: int = AUDIO_BOS, pad: int = -1, T_max=None):
    """Dia.PrepareAudioPrompt on codes that exist: a list of int64 [C, F_b] (None or F_b = 0: no prompt) -> int32 [B, T_max, C] with
    out[b, t, c] = bos where t <= delay[c], codes_b[c][t - delay[c] - 1] up to F_b steps behind it, -1 from there on.  T_max defaults to
    max F_b + max(delay); `pad` is taken as the reference takes it and never written."""
    items = list(codes)
    Cn = len(delay_pattern)
    if not items or any(c is not None and (c.ndim != 2 or int(c.shape[0]) != Cn) for c in items):
        raise ValueError("a list of codes [C, F] with one delay per channel")
    frames = [0 if c is None else int(c.shape[1]) for c in items]
    T = max(frames) + max(int(d) for d in delay_pattern) if T_max is None else int(T_max)
    torch = _torch()
    some = [c for c in items if c is not None and c.shape[1] > 0]
    was_torch = bool(some) and _is_torch(some[0])
    if was_torch:
        flat = torch.cat([c.reshape(-1).to(torch.int64) for c in some]).contiguous()
        flat = flat if flat.is_cuda else flat.cuda()
    else:
        host = np.concatenate([np.asarray(c, np.int64).reshape(-1) for c in some]) if some else np.zeros(1, np.int64)
        flat = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    out = torch.empty((len(items), max(T, 0), Cn), dtype=torch.int32, device=flat.device)
    stream = torch.cuda.current_stream(flat.device).cuda_stream
    _lib.check(_lib.lib().nc_dia_prefill_pack_dev(flat.device.index or 0, flat.data_ptr(), len(items), _lib.i64_array(frames), Cn,
                                                  _i32_array(delay_pattern), int(bos), int(pad), T, out.data_ptr(), stream))
    return _hand_back(out, was_torch)


def encode_dia_prompts(dac, prompts, batch_size=None, delay_pattern=DELAY_PATTERN, bos: int = AUDIO_BOS, pad: int = -1, channels=None):
    """Dia.LoadAudio's mix, Dia.Encode of every prompt and Dia.PrepareAudioPrompt in one call (nc_dia_encode_prompts[_dev]): a list of
    1-D waveforms (None: no prompt; with channels[b] > 1 interleaved [n][ch] flattened) -> (prefill int32 [B, T_max, C], prefill steps),
    B = max(batch_size, len(prompts)).  The prompts are NOT resampled: the reference discards its resampled copy (Dia.cs:870-874)."""
    ps = [] if prompts is None else list(prompts)
    B = max(int(batch_size or 0), len(ps))
    ps += [None] * (B - len(ps))
    if any(p is not None and p.ndim != 1 for p in ps):
        raise ValueError("every prompt must be 1-D (or None)")
    ch = [1] * B if channels is None else [int(c) for c in channels] + [1] * (B - len(channels))
    if len(ch) != B:
        raise ValueError("one channel count per prompt")
    if any(c > 0 and p is not None and int(p.shape[0]) % c for p, c in zip(ps, ch)):
        raise ValueError("every prompt holds whole frames of its channel count")
    lens = [0 if p is None else int(p.shape[0]) // max(c, 1) for p, c in zip(ps, ch)]
    Cn = len(delay_pattern)
    _, _, T_max = prompt_query(dac, lens, delay_pattern)          # (every refusal that is host arithmetic is raised here)
    some = [p for p in ps if p is not None and p.shape[0] > 0]
    steps = (C.c_int32 * max(1, B))()
    L = _lib.lib()
    args = (B, _lib.i64_array(lens), None if channels is None else _i32_array(ch), Cn, _i32_array(delay_pattern), int(bos), int(pad))
    if some and _is_torch(some[0]):
        import torch
        flat = torch.cat([p.to(torch.float32) for p in some]).contiguous()
        out = torch.empty((B, T_max, Cn), dtype=torch.int32, device=flat.device)
        dac._bind_torch_stream()
        _lib.check(L.nc_dia_encode_prompts_dev(dac._h, flat.data_ptr(), *args, out.data_ptr(), steps))
    else:
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32) for p in some])) if some else None
        out = np.empty((B, T_max, Cn), np.int32)
        _lib.check(L.nc_dia_encode_prompts(dac._h, None if flat is None else flat.ctypes.data, *args, out.ctypes.data, steps))
    return out, list(steps)[:B]


# ---- sampling stage: guided logits -> the next row of the delayed code matrix (nc_dia.hip) ------------------------------
# DataConfig.AudioEosValue / AudioPadValue of the reference's DiaConfig; the sampling defaults of Dia.Generate (Dia.cs:615-624)
AUDIO_EOS, AUDIO_PAD = 1024, 1025


def _sample_params(cfg_scale, temperature, top_p, top_k, eos, pad):
    return _lib.NcDiaSampleParams(float(cfg_scale), float(temperature), float(top_p), int(top_k), int(eos), int(pad))


def _logits_shape(logits):
    if logits is None or logits.ndim != 3 or int(logits.shape[0]) % 2 or int(logits.shape[0]) == 0:
        raise ValueError("logits must be [2B, C, V]: row 2b unconditional, row 2b + 1 conditional")
    return int(logits.shape[0]) // 2, int(logits.shape[1]), int(logits.shape[2])


def dia_sample_host(logits, uniform, cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos=AUDIO_EOS, pad=AUDIO_PAD):
    """nc_dia_sample_host: Dia.DecoderStep from the logits on (guidance, masks, SampleNextToken) in serial C++ on the host, no device.
    logits float32 [2B, C, V], uniform float32 [B, C] in [0, 1) -> (tokens int64 [B, C], bad int32 [B]), numpy.  The same bits as
    dia_sample_next_token."""
    B, Cn, V = _logits_shape(logits)
    x = np.ascontiguousarray(np.asarray(logits, dtype=np.float32))
    u = np.ascontiguousarray(np.asarray(uniform, dtype=np.float32))
    if u.shape != (B, Cn):
        raise ValueError("uniform must be [B, C]")
    tokens, bad = np.empty((B, Cn), np.int64), np.empty(B, np.int32)
    p = _sample_params(cfg_scale, temperature, top_p, top_k, eos, pad)
    _lib.check(_lib.lib().nc_dia_sample_host(x.ctypes.data, B, Cn, V, C.byref(p), u.ctypes.data, tokens.ctypes.data, bad.ctypes.data))
    return tokens, bad


def _uniform_on(uniform, B, Cn, device):
    """the draws of a step on the device: the caller's [B, C], or torch.rand"""
    torch = _torch()
    if uniform is None:
        return torch.rand((B, Cn), dtype=torch.float32, device=device)
    u, _ = _on_device(uniform, np.float32, "float32")
    if tuple(u.shape) != (B, Cn):
        raise ValueError("uniform must be [B, C]")
    return u.to(device)


def dia_sample_next_token(logits, uniform=None, cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos=AUDIO_EOS, pad=AUDIO_PAD):
    """nc_dia_sample_dev: Dia.DecoderStep from the logits on in ONE launch.  logits float32 [2B, C, V] -> (tokens int64 [B, C], bad
    int32 [B]); bad[b] != 0: a row of item b has no token (-1).  uniform [B, C] in [0, 1) is the draw of every row (None: torch.rand on the
    device).  The order among equal logits is (value descending, index ascending)."""
    B, Cn, V = _logits_shape(logits)
    x, was_torch = _on_device(logits, np.float32, "float32")
    torch = _torch()
    u = _uniform_on(uniform, B, Cn, x.device)
    tokens = torch.empty((B, Cn), dtype=torch.int64, device=x.device)
    bad = torch.empty(B, dtype=torch.int32, device=x.device)
    p = _sample_params(cfg_scale, temperature, top_p, top_k, eos, pad)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(_lib.lib().nc_dia_sample_dev(x.device.index or 0, x.data_ptr(), B, Cn, V, C.byref(p), u.data_ptr(), tokens.data_ptr(), bad.data_ptr(),
                                            stream))
    if was_torch:
        return tokens, bad
    torch.cuda.synchronize(x.device)
    return tokens.cpu().numpy(), bad.cpu().numpy()


def generate_lengths(finished, prefill_steps, final_step: int, maxd: int):
    """nc_dia_generate_lengths (Dia.cs:775-782, host arithmetic): (lengths, T_gen) from a host copy of the finished steps."""
    B = len(prefill_steps)
    out, tg = (C.c_int64 * max(1, B))(), C.c_int64()
    _lib.check(_lib.lib().nc_dia_generate_lengths(B, _lib.i64_array(finished), _i32_array(prefill_steps), int(final_step), int(maxd), out, C.byref(tg)))
    return list(out)[:B], int(tg.value)


class DiaGeneration:
    """The generation loop of Dia.Generate (Dia.cs:664-801) around a caller's language model, everything but the model on the device:

        gen = DiaGeneration(B, delay_pattern, max_tokens, prefill, prefill_steps)      # the two outputs of DAC.encode_dia_prompts
        while not gen.exhausted and gen.active().any():                                # (poll as rarely as you like)
            logits = lm(gen.tokens())                                                  # float32 [2B, C, V] on the device
            gen.step(logits)                                                           # ONE launch: sample, EOS bookkeeping, write
        codes_delayed, lengths = gen.finish()                                          # what DAC.decode_dia_output takes

    generated is DecoderOutput.GeneratedTokens, int32 [B, audio_length, C] with the prefill copied in; state, active and bad live on the
    device.  numpy in (the prefill), numpy out of finish(); torch device tensors in, tensors out.
    audio_length defaults to max_tokens, the reference's buffer.  A step writes row dec_step + 1, so the last step that fits is the one
    with dec_step + 1 == audio_length - 1: `exhausted` turns true behind it (or at dec_step == max_tokens) and step() raises ValueError.
    With a delay pattern of zeros only, an item that never emits EOS is first cut by the length rule at row max_tokens, which the
    reference's own buffer does not hold either (its loop indexes past it); pass audio_length = max_tokens + 1 to take that step."""

    def __init__(self, B, delay_pattern, max_tokens, prefill, prefill_steps, cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45,
                 eos=AUDIO_EOS, pad=AUDIO_PAD, audio_length=None):
        torch = _torch()
        self.B, self.delay = int(B), [int(d) for d in delay_pattern]
        self.C, self.maxd, self.max_tokens = len(self.delay), max(self.delay), int(max_tokens)
        self.L = self.max_tokens if audio_length is None else int(audio_length)
        self.prefill_steps = [int(s) for s in prefill_steps]
        self.params = _sample_params(cfg_scale, temperature, top_p, top_k, eos, pad)
        self.pad = int(pad)
        self._delay_arr = _i32_array(self.delay)
        pre, self._torch_out = _on_device(prefill, np.int32, "int32")
        if pre.ndim != 3 or int(pre.shape[0]) != self.B or int(pre.shape[2]) != self.C or len(self.prefill_steps) != self.B:
            raise ValueError("prefill must be [B, T, C] with one prefill step per item and one delay per channel")
        if int(pre.shape[1]) > self.L or self.max_tokens > self.L:
            raise ValueError("the prefill and max_tokens must fit audio_length")
        dev = pre.device
        self.device = dev
        self.generated = torch.full((self.B, self.L, self.C), -1, dtype=torch.int32, device=dev)         # DecoderOutput.New / Prefill
        self.generated[:, :pre.shape[1], :] = pre
        self.state = torch.empty((3, self.B), dtype=torch.int64, device=dev)
        self._active = torch.ones(self.B, dtype=torch.int32, device=dev)
        self._bad = torch.zeros(self.B, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().nc_dia_generate_state_init_dev(dev.index or 0, self.B, self.state.data_ptr(), self._stream()))
        self.dec_step = min(self.prefill_steps) - 1                                                     # Dia.cs:664
        self._bos_over = False

    def _stream(self):
        return _torch().cuda.current_stream(self.device).cuda_stream

    @property
    def exhausted(self):
        """no further step fits: max_tokens steps are taken (Dia.cs:681), or row dec_step + 1 lies behind the buffer"""
        return self.dec_step >= self.max_tokens or self.dec_step + 1 >= self.L

    def tokens(self):
        """DecoderOutput.GetTokensAt(decStep): the row the language model reads next, int32 [B, C] (a view of `generated`)"""
        return self.generated[:, self.dec_step, :]

    def step(self, logits, uniform=None):
        """One pass of the loop body behind the language model (Dia.cs:688-756): logits float32 [2B, C, V] -> generated[:, dec_step + 1]."""
        B, Cn, V = _logits_shape(logits)
        if (B, Cn) != (self.B, self.C):
            raise ValueError("logits must be [2B, C, V] of this generation")
        if self.exhausted:
            raise ValueError(f"no step left: dec_step = {self.dec_step}, max_tokens = {self.max_tokens}, audio_length = {self.L}")
        x, _ = _on_device(logits, np.float32, "float32")
        u = _uniform_on(uniform, B, Cn, self.device)
        s = self.dec_step + 1
        if not self._bos_over:                                                                          # Dia.cs:749-753
            self._bos_over = all(self.dec_step - p > self.maxd for p in self.prefill_steps)
        _lib.check(_lib.lib().nc_dia_generate_step_dev(self.device.index or 0, x.data_ptr(), B, Cn, V, C.byref(self.params), u.data_ptr(),
                                                       self._delay_arr, s, self.max_tokens, 0 if self._bos_over else 1,
                                                       self.state.data_ptr(), self.generated.data_ptr(), self.L, self._active.data_ptr(),
                                                       self._bad.data_ptr(), self._stream()))
        self.dec_step += 1

    def active(self):
        """countdown != 0 per item after the last step, bool [B] on the host (this synchronises; the loop ends when none is left)"""
        return self._active.cpu().numpy() != 0

    def bad(self):
        """items that had a row without a token (-1 written) in some step, bool [B] on the host"""
        return self._bad.cpu().numpy() != 0

    def finish(self):
        """Dia.cs:775-801: (codes_delayed int64 [B, T_gen, C], lengths) -- the arguments of DAC.decode_dia_output."""
        torch = _torch()
        finished = self.state[2].cpu().numpy().tolist()
        lengths, T_gen = generate_lengths(finished, self.prefill_steps, self.dec_step + 1, self.maxd)
        out = torch.empty((self.B, max(T_gen, 0), self.C), dtype=torch.int64, device=self.device)
        _lib.check(_lib.lib().nc_dia_generate_collect_dev(self.device.index or 0, self.generated.data_ptr(), self.B, self.L, self.C,
                                                          _i32_array(self.prefill_steps), _lib.i64_array(lengths), self.maxd, self.pad,
                                                          out.data_ptr(), self._stream()))
        return _hand_back(out, self._torch_out), lengths
