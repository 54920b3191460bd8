"""CPU suite: the numpy restatement of Dia's prompt stage (tests/dia_prompt_ref.py, the truth of the GPU suite) held to a literal torch-CPU
transcription of the reference -- Dia.PrepareAudioPrompt (Models/Dia.cs:329-400) over BuildDelayIndices / ApplyAudioDelay
(Modules/Dia/AudioUtils.cs:19-94) and LoadAudio's mono mix (Dia.cs:851-864) -- and to the closed form the kernel evaluates, with
np.array_equal.  The handle-less exports are held to their refusals and, without a device, to NC_EDEVICE.

With max(delay) == 0 the reference has no result for a batch that holds a prompt: the prefill has max F rows and the copy of the longest
prompt needs F + 1 (Dia.cs:377).  The transcription raises there, as the reference does (a longest prompt of one frame broadcasts into
the empty slice instead, and is compared like every other case); the restatement and the closed form cut the longest prompt's last
frame, and the test holds those two to each other."""
import ctypes as C

import numpy as np
import pytest
import torch

import dia_prompt_ref as R
from neuralcodecs_amd import _lib

PATTERNS = {"dia": [0, 8, 9, 10, 11, 12, 13, 14, 15], "zero": [0] * 9, "one_channel": [3], "descending": [7, 5, 2, 0],
            "repeats": [2, 0, 2, 5, 5, 0, 1]}
BOS, SENTINEL = 1026, -777


# ---- the reference, statement by statement, on torch CPU tensors -------------------------------------------------------------------
def build_delay_indices(B, T, C, delay_pattern):
    delay_arr = torch.tensor(delay_pattern, dtype=torch.int32)
    t_idx_BxT = torch.broadcast_to(torch.arange(T, dtype=torch.int32)[None, :], (B, T))
    t_idx_BxTxC = t_idx_BxT[..., None] - delay_arr.view(1, 1, C)
    b_idx = torch.broadcast_to(torch.arange(B, dtype=torch.int32).view(B, 1, 1), (B, T, C))
    c_idx = torch.broadcast_to(torch.arange(C, dtype=torch.int32).view(1, 1, C), (B, T, C))
    t_clamped = torch.clamp(t_idx_BxTxC, 0, T - 1)
    indices = torch.stack([b_idx.reshape(-1), t_clamped.reshape(-1), c_idx.reshape(-1)], dim=1).to(torch.int64)
    return t_idx_BxTxC, indices


def apply_audio_delay(audio, pad_value, bos_value, precomp):
    t_idx, indices = precomp
    gathered = audio[indices[:, 0], indices[:, 1], indices[:, 2]].view(audio.shape)
    mask_bos = t_idx < 0
    mask_pad = t_idx >= audio.shape[1]
    result = torch.where(mask_bos, torch.tensor(bos_value, dtype=audio.dtype), gathered)
    return torch.where(mask_pad, torch.tensor(pad_value, dtype=audio.dtype), result)


def prepare_audio_prompt(batch_size, audio_prompts, delay_pattern, bos_value, pad_value=-1):
    """Dia.cs:329-400; audio_prompts: list of int64 [F, C] tensors or None"""
    num_channels = len(delay_pattern)
    max_delay = max(delay_pattern)
    if audio_prompts is None or len(audio_prompts) == 0:
        batch, maxlength = batch_size, max_delay
    else:
        batch = max(batch_size, len(audio_prompts))
        maxlength = max(p.shape[0] if p is not None else 0 for p in audio_prompts) + max_delay
    steps = []
    prefill = torch.full((batch, maxlength, num_channels), -1, dtype=torch.int32)
    prefill[:, 0, :] = bos_value
    if audio_prompts is None or len(audio_prompts) == 0:
        steps = [1] * batch
    else:
        for i in range(batch):
            prompt = audio_prompts[i] if i < len(audio_prompts) else None        # ElementAtOrDefault
            if prompt is not None:
                prompt = prompt.to(torch.int32)
                prefill[i, 1:prompt.shape[0] + 1, :] = prompt
                steps.append(int(prompt.shape[0]) + 1)
            else:
                steps.append(1)
    delayed = apply_audio_delay(prefill, pad_value, bos_value, build_delay_indices(batch, maxlength, num_channels, delay_pattern))
    return delayed, steps


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _prompt(F, Cn, seed):
    """[F, C] codes in Dia's range with the values that must survive untouched sprinkled in: -1, the BOS value, the sentinel pad"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 1024, (F, Cn)).astype(np.int64)
    if p.size >= 4:
        p.reshape(-1)[rng.integers(0, p.size, max(1, p.size // 8))] = rng.choice([-1, BOS, 1025], max(1, p.size // 8))
    return p


def _cases(delay):
    """(prompts, batch_size): None entries, F = 1, F below and above max(delay), batch sizes above and below the prompt count"""
    md, Cn = max(delay), len(delay)
    below, above = max(1, md - 1), md + 6
    yield [_prompt(1, Cn, 1)], 1
    yield [_prompt(above, Cn, 2)], 1
    yield [_prompt(below, Cn, 3), None, _prompt(above, Cn, 4)], 3
    yield [None, _prompt(1, Cn, 5), _prompt(above, Cn, 6)], 1                     # batch_size below the prompt count
    yield [_prompt(below, Cn, 7)], 3                                              # and above it: items past the list have no prompt
    yield [_prompt(md + 1, Cn, 8), _prompt(md, Cn, 9) if md else None, None], 3


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_restatement_equals_the_torch_transcription_and_the_closed_form(name):
    delay = PATTERNS[name]
    md = max(delay)
    n = 0
    for prompts, batch in _cases(delay):
        got, steps = R.prepare_audio_prompt(prompts, batch, delay, BOS, SENTINEL)
        B = max(batch, len(prompts))
        F = [0 if p is None else p.shape[0] for p in prompts] + [0] * (B - len(prompts))
        assert got.dtype == np.int32 and got.shape == (B, max(F) + md, len(delay))
        assert steps == [f + 1 for f in F]                                        # F + 1, and 1 where there is no prompt
        closed = R.prefill_closed_form([None if p is None else p.T for p in prompts] + [None] * (B - len(prompts)), delay, BOS)
        assert np.array_equal(got, closed), (name, F, batch)
        assert not np.any(got == SENTINEL)                                        # ApplyAudioDelay's pad is never written
        tp = [None if p is None else torch.from_numpy(p) for p in prompts]
        if md == 0 and max(F) > 1:
            with pytest.raises(RuntimeError):                                     # the longest prompt does not fit its own prefill
                prepare_audio_prompt(batch, tp, delay, BOS, SENTINEL)
            continue                                                              # (max F = 1 there: a [1, C] prompt broadcasts into the empty slice)
        want, want_steps = prepare_audio_prompt(batch, tp, delay, BOS, SENTINEL)
        assert want.dtype == torch.int32 and np.array_equal(got, want.numpy()), (name, F, batch)
        assert steps == want_steps
        n += 1
    assert n == (3 if md == 0 else 6)                                             # without a delay only the batches of F = 1 prompts have a reference result


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("B", [1, 3])
def test_no_prompt_at_all_is_the_bos_row_over_max_delay_steps(name, B):
    delay = PATTERNS[name]
    md = max(delay)
    if md == 0:
        with pytest.raises((RuntimeError, IndexError)):                           # a prefill of no rows cannot hold the BOS row
            prepare_audio_prompt(B, None, delay, BOS)
        return
    for prompts in (None, []):
        want, want_steps = prepare_audio_prompt(B, prompts, delay, BOS, SENTINEL)
        got, steps = R.prepare_audio_prompt(prompts, B, delay, BOS, SENTINEL)
        assert got.shape == (B, md, len(delay)) and np.array_equal(got, want.numpy()) and steps == want_steps == [1] * B
        assert np.array_equal(got, R.prefill_closed_form([None] * B, delay, BOS))
        assert np.all(got[:, 0, :] == BOS) and set(np.unique(got)) <= {BOS, -1}


def test_closed_form_with_a_longer_t_max_and_codes_past_int32():
    delay = PATTERNS["descending"]
    p = _prompt(9, 4, 11)
    p[3, 1], p[4, 2] = 2 ** 31 - 1, 2 ** 32 + 5                                    # the second keeps its low 32 bits, as .to(int32) does
    got, _ = R.prepare_audio_prompt([p], 1, delay, BOS)
    want, _ = prepare_audio_prompt(1, [torch.from_numpy(p)], delay, BOS)
    assert np.array_equal(got, want.numpy()) and (got == 2 ** 31 - 1).sum() == 1 and got[0, 5 + delay[2], 2] == 5
    longer = R.prefill_closed_form([p.T], delay, BOS, T_max=9 + 7 + 20)
    # T_max = F + max(delay) has no room for the last frame of the most delayed channel (rows 0 .. F need F + 1): the reference cuts it,
    # and a longer prefill shows it
    assert np.array_equal(longer[:, :16], got) and longer[0, 16, 0] == p[8, 0]
    longer[0, 16, 0] = -1
    assert np.all(longer[:, 16:] == -1)


def test_mix_mono32_equals_the_loop_of_load_audio():
    rng = np.random.default_rng(3)
    for ch in (1, 2, 3, 6):
        x = (rng.standard_normal(257 * ch) * 3).astype(np.float32)
        want = np.empty(257, np.float32)
        for i in range(257):                                                      # Dia.cs:854-862, statement by statement
            s = np.float32(0)
            for c in range(ch):
                s = np.float32(s + x[i * ch + c])
            want[i] = np.float32(s / np.float32(ch))
        got = R.mix_mono32(x, ch)
        if ch == 1:
            assert got.tobytes() == x.tobytes()                                   # `audioData = buffer`
        else:
            assert got.tobytes() == want.tobytes()
    assert R.mix_mono32(np.array([-0.0], np.float32), 1).tobytes() == np.array([-0.0], np.float32).tobytes()


# ---- the C ABI without a handle -----------------------------------------------------------------------------------------------------------
def _i32(v):
    return (C.c_int32 * len(v))(*v)


def test_prompt_query_and_encode_need_a_dac_handle():
    """nc_dia_prompt_query reads n_codebooks and the hop from the handle, and a handle needs a device: its values and every refusal are
    held to the restatement in the GPU suite (tests/test_dia_prompt_gpu.py).  Without one it is NC_EINVAL, not a crash."""
    L = _lib.lib()
    fr, st, tm = (C.c_int64 * 2)(), (C.c_int32 * 2)(), C.c_int64()
    assert L.nc_dia_prompt_query(None, 2, 9, _i32(PATTERNS["dia"]), _lib.i64_array([5, 0]), fr, st, C.byref(tm)) == _lib.NC_EINVAL
    assert b"null codec handle" in L.nc_last_error()
    out = np.zeros(2 * 20 * 9, np.int32)
    for fn in (L.nc_dia_encode_prompts, L.nc_dia_encode_prompts_dev):
        assert fn(None, None, 2, _lib.i64_array([0, 0]), None, 9, _i32(PATTERNS["dia"]), BOS, -1, out.ctypes.data, st) == _lib.NC_EINVAL
    assert not out.any()


def test_handle_less_exports_refuse_before_the_device_and_never_compute_on_the_host():
    L = _lib.lib()
    delay = PATTERNS["descending"]
    codes = np.arange(4 * 5, dtype=np.int64)
    out = np.full(2 * 12 * 4, 55, np.int32)

    def pack(B=2, frames=(5, 0), Cn=4, d=delay, bos=BOS, pad=-1, T=12, c=codes.ctypes.data, o=out.ctypes.data):
        return L.nc_dia_prefill_pack_dev(0, c, B, _lib.i64_array(frames) if frames is not None else None, Cn, _i32(list(d)) if d is not None else None,
                                         bos, pad, T, o, None)

    E = _lib.NC_EINVAL
    assert pack(B=0) == E and pack(frames=None) == E and pack(d=None) == E and pack(c=None) == E and pack(o=None) == E
    assert pack(Cn=0, d=[]) == E and pack(Cn=33, d=[0] * 33) == E
    assert pack(d=[7, 5, -2, 0]) == E                                             # a negative delay
    assert pack(frames=(5, -1)) == E                                              # a negative frame count
    assert pack(T=11) == E                                                        # below max(frames) + max(delay)
    assert pack(frames=(0, 0), d=[0, 0, 0, 0], T=0) == E                          # nothing can hold the BOS row
    assert pack(bos=2 ** 31) == E and pack(bos=-2 ** 31 - 1) == E and pack(pad=2 ** 31) == E
    assert pack(frames=(2 ** 38, 0), T=2 ** 38 + 7) == E                          # a grid that does not fit
    x = np.arange(12, dtype=np.float32)
    mono = np.full(5, 55, np.float32)

    def mix(B=2, n=(3, 2), ch=(2, 3), i=x.ctypes.data, o=mono.ctypes.data):
        return L.nc_audio_mix_to_mono_ragged_dev(0, i, B, _lib.i64_array(n) if n is not None else None, _i32(list(ch)) if ch is not None else None, o, None)

    assert mix(B=0) == E and mix(n=None) == E and mix(ch=None) == E and mix(i=None) == E and mix(o=None) == E
    assert mix(ch=(2, 0)) == E and mix(ch=(-1, 3)) == E and mix(n=(3, -2)) == E
    if L.nc_device_count() == 0:                                                  # valid calls: no device, no result (host pointers are never read)
        assert pack() == _lib.NC_EDEVICE and b"no CPU fallback" in L.nc_last_error()
        assert mix() == _lib.NC_EDEVICE and b"no CPU fallback" in L.nc_last_error()
    assert np.all(out == 55) and np.all(mono == 55)
