"""TEST INFRASTRUCTURE: Dia's prompt stage restated in plain numpy (no torch, no engine).

    prepare_audio_prompt   Models/Dia.cs:329-400 as the reference composes it: full(-1), the BOS row, the copy of every prompt into rows
                           1 .. F, BuildDelayIndices with its clamp, the gather and the two `where`s of ApplyAudioDelay
                           (Modules/Dia/AudioUtils.cs:19-94)
    prefill_closed_form    the same values from one formula per element (what the kernel evaluates)
    mix_mono32             Dia.LoadAudio's mono mix, Models/Dia.cs:851-864, in explicit np.float32 steps

tests/test_dia_prompt_cpu.py holds these to a torch-CPU transcription of the reference; the GPU suite holds the kernels to these.

One place has no reference result.  The prefill has max F + max(delay) rows and the copy writes rows 1 .. F, so with max(delay) == 0 the
longest prompt does not fit and the reference throws (Dia.cs:377; a longest prompt of ONE frame broadcasts into the empty slice and
writes nothing).  prepare_audio_prompt copies the rows that exist there, which is what the closed form gives: the longest prompt loses
its last frame.  With any positive delay the copy is the reference's, row for row."""
import numpy as np

F32 = np.float32


def build_delay_indices(B, T, C, delay):
    """t_idx [B, T, C] = t - delay[c] (int32) and the gather rows [B * T * C, 3] with t clamped to [0, T - 1]"""
    delay_arr = np.asarray(delay, np.int32)
    t_idx_BxT = np.broadcast_to(np.arange(T, dtype=np.int32)[None, :], (B, T))
    t_idx_BxTxC = t_idx_BxT[..., None] - delay_arr.reshape(1, 1, C)
    b_idx = np.broadcast_to(np.arange(B, dtype=np.int32).reshape(B, 1, 1), (B, T, C))
    c_idx = np.broadcast_to(np.arange(C, dtype=np.int32).reshape(1, 1, C), (B, T, C))
    t_clamped = np.clip(t_idx_BxTxC, 0, T - 1)
    indices = np.stack([b_idx.reshape(-1), t_clamped.reshape(-1), c_idx.reshape(-1)], axis=1).astype(np.int64)
    return t_idx_BxTxC, indices


def apply_audio_delay(audio, pad_value, bos_value, precomp):
    t_idx, indices = precomp
    gathered = audio[indices[:, 0], indices[:, 1], indices[:, 2]].reshape(audio.shape)
    mask_bos = t_idx < 0
    mask_pad = t_idx >= audio.shape[1]
    result = np.where(mask_bos, np.asarray(bos_value, audio.dtype), gathered)
    return np.where(mask_pad, np.asarray(pad_value, audio.dtype), result)


def prepare_audio_prompt(prompts_TC, batch, delay, bos, pad=-1):
    """prompts_TC: list of [F, C] code matrices (Dia.Encode's layout) or None -> (int32 [B, T_max, C], steps); `pad` is the padValue
    handed to ApplyAudioDelay (the reference passes -1; any other value shows that it is never written)."""
    C = len(delay)
    max_delay = int(max(delay))
    if not prompts_TC:
        B, maxlength = int(batch), max_delay
    else:
        B = max(int(batch), len(prompts_TC))
        maxlength = max(0 if p is None else int(np.asarray(p).shape[0]) for p in prompts_TC) + max_delay
    prefill = np.full((B, maxlength, C), -1, np.int32)
    prefill[:, 0:1, :] = bos
    steps = []
    for i in range(B):
        prompt = prompts_TC[i] if prompts_TC and i < len(prompts_TC) else None
        if prompt is not None:
            prompt = np.asarray(prompt).astype(np.int64).astype(np.int32)          # `.to(torch.int32)`: the low 32 bits
            n = min(prompt.shape[0], maxlength - 1)                                # == F unless max(delay) == 0 (see the module text)
            prefill[i, 1:n + 1, :] = prompt[:n]
            steps.append(int(prompt.shape[0]) + 1)
        else:
            steps.append(1)
    delayed = apply_audio_delay(prefill, pad, bos, build_delay_indices(B, maxlength, C, delay))
    return delayed.astype(np.int32), steps


def prefill_closed_form(codes_CF, delay, bos, T_max=None):
    """codes_CF: list of [C, F] (the packed ragged layout's items; None or F = 0: no prompt) -> int32 [B, T_max, C]:
    s = t - delay[c]; out = bos for s <= 0, codes[c][s - 1] for 1 <= s <= F, -1 behind it."""
    C = len(delay)
    Fs = [0 if c is None else int(np.asarray(c).shape[1]) for c in codes_CF]
    T = max(Fs) + int(max(delay)) if T_max is None else int(T_max)
    out = np.empty((len(codes_CF), T, C), np.int32)
    for b, (codes, F) in enumerate(zip(codes_CF, Fs)):
        for c in range(C):
            s = np.arange(T, dtype=np.int64) - int(delay[c])
            row = np.full(T, -1, np.int32)
            row[s <= 0] = bos
            inside = (s >= 1) & (s <= F)
            if F:
                row[inside] = np.asarray(codes)[c].astype(np.int64).astype(np.int32)[s[inside] - 1]
            out[b, :, c] = row
    return out


def mix_mono32(x, channels):
    """interleaved [n][channels] flattened -> [n]: `sum += x` in binary32 from 0 in channel order, then `sum / channels`; one channel: the
    input itself (LoadAudio mixes only for channels > 1)"""
    x = np.asarray(x, F32)
    if channels == 1:
        return x.copy()
    frames = x.reshape(-1, channels)
    s = np.zeros(frames.shape[0], F32)
    for c in range(channels):
        s = (s + frames[:, c]).astype(F32)
    return (s / F32(channels)).astype(F32)
