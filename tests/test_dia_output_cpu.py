"""CPU suite: the numpy restatement of Dia's output stage (tests/dia_output_ref.py, the truth of the GPU suite) held to a literal
torch-CPU transcription of the reference -- BuildRevertIndices / RevertAudioDelay, BuildDelayIndices / ApplyAudioDelay
(Modules/Dia/AudioUtils.cs:19-176), AdjustSpeed (Models/Dia.cs:947-966) and Interp (Utils/TorchUtils.cs:58-82) on torch.linspace /
torch.searchsorted -- with np.array_equal, and the host functions of the C ABI held to the restatement.

The linspace positions: ATen's CPU kernel is `start + step * i` / `end - step * (steps - 1 - i)`, and its AVX2 and AVX-512 builds contract
each into ONE fused multiply-add.  With a rounded product and a rounded sum instead, torch.linspace differs at 1 of 21 positions for L 17
at speed 0.8 and at 163 / 2000, 98 / 1250, 62 / 800, 28 / 333 for L 1000 at speeds 0.5, 0.8, 1.25, 3.0; the restatement (and the kernel)
therefore fuse, and test_linspace_restatement_equals_torch_linspace holds them to torch.linspace over those and some hundred other sizes.
Interp is separate tensor operations: a rounded product, then a rounded sum."""
import ctypes as C

import numpy as np
import pytest
import torch

import dia_output_ref as R
from neuralcodecs_amd import _lib

PATTERNS = {"zero": [0] * 9, "dia": [0, 8, 9, 10, 11, 12, 13, 14, 15], "non_monotone": [3, 0, 7, 7, 1, 12, 0, 5, 2]}
SPEEDS = (0.5, 0.8, 0.99999, 1.0, 1.25, 3.0)
LENGTHS = (2, 3, 17, 1000)
PAD, BOS = 1025, 1026


# ---- the reference, statement by statement, on torch CPU tensors -------------------------------------------------------------------
def build_revert_indices(B, T, C, delay_pattern):
    delay_arr = torch.tensor(delay_pattern, dtype=torch.int32)
    t_idx_BT1 = torch.broadcast_to(torch.arange(T).unsqueeze(0), (B, T)).unsqueeze(-1)
    t_idx_BxTxC = torch.minimum(t_idx_BT1 + delay_arr.view(1, 1, C), torch.tensor(T - 1))
    b_idx = torch.broadcast_to(torch.arange(B).view(B, 1, 1), (B, T, C))
    c_idx = torch.broadcast_to(torch.arange(C).view(1, 1, C), (B, T, C))
    indices = torch.stack([b_idx.reshape(-1), t_idx_BxTxC.reshape(-1), c_idx.reshape(-1)], dim=1).to(torch.int64)
    return t_idx_BxTxC, indices


def revert_audio_delay(audio, pad_value, precomp, T):
    t_idx, indices = precomp
    gathered = audio[indices[:, 0], indices[:, 1], indices[:, 2]].view(audio.size())
    return torch.where(t_idx.ge(torch.tensor(T)), torch.tensor(pad_value, dtype=audio.dtype), gathered)


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


def generate_output_codebook(generated, delay_pattern, pad_value, lo=0, hi=1023):
    """Dia.cs:1022-1045: revert, cut the last max(delay) steps, codes outside [lo, hi] -> 0"""
    B, T, C = generated.shape
    unmasked = revert_audio_delay(generated, pad_value, build_revert_indices(B, T, C, delay_pattern), T)
    md = max(delay_pattern)
    codebook = (unmasked[:, :-md, :] if md else unmasked).clone()
    codebook[codebook.lt(lo).logical_or(codebook.gt(hi))] = 0
    return codebook


def interp(x, xp, fp):
    offset = torch.diff(fp) / torch.diff(xp)
    slope = fp[..., :-1] - (offset * xp[..., :-1])
    indices = torch.searchsorted(xp, x, right=False)
    indices = torch.clamp(indices - 1, 0, offset.shape[-1] - 1)
    return (offset.gather(-1, indices) * x) + slope.gather(-1, indices)


def adjust_speed(audio, speed_factor, positions=None):
    speed_factor = np.float32(speed_factor)
    if abs(np.float32(speed_factor - np.float32(1.0))) < np.float32(1e-5):
        return audio
    original_len = audio.size(-1)
    target_len = int(np.float32(original_len) / speed_factor)
    if target_len <= 0 or target_len == original_len:
        return audio
    x_original = torch.arange(original_len)
    x_resampled = torch.linspace(0, original_len - 1, target_len) if positions is None else positions
    return interp(x_resampled, x_original, audio)


# ---- delay patterns -----------------------------------------------------------------------------------------------------------------
def _codes(B, T, C, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 1024, (B, T, C)).astype(np.int64)
    c.reshape(-1)[rng.integers(0, c.size, max(4, c.size // 6))] = rng.choice([-1, 1024, PAD, BOS], max(4, c.size // 6))
    return c


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_revert_and_mask_restatement_equals_the_torch_transcription(name):
    delay = PATTERNS[name]
    md = max(delay)
    for T in list(range(md + 1, md + 6)) + [md + 17, md + 40]:
        for B in (1, 3):
            c = _codes(B, T, len(delay), 100 * T + B)
            want = generate_output_codebook(torch.from_numpy(c), delay, PAD).numpy()
            got = R.mask_invalid(R.revert_delay(c, delay))
            assert got.shape == want.shape == (B, T - md, len(delay))
            assert np.array_equal(got, want), (name, T, B)
            # the pad mask is dead: no reverted value is the pad value unless the input held it there
            raw = revert_audio_delay(torch.from_numpy(c), -777, build_revert_indices(B, T, len(delay), delay), T).numpy()
            assert not np.any(raw == -777)


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_apply_delay_restatement_equals_the_torch_transcription(name):
    delay = PATTERNS[name]
    md = max(delay)
    for T in (1, 2, md, md + 1, md + 2, 40):
        if T <= 0:
            continue
        for B in (1, 2):
            c = _codes(B, T, len(delay), 7 * T + B)
            want = apply_audio_delay(torch.from_numpy(c), -777, BOS, build_delay_indices(B, T, len(delay), delay)).numpy()
            assert np.array_equal(R.apply_delay(c, delay, BOS, -777), want), (name, T, B)
            assert not np.any(want == -777)                                 # ApplyAudioDelay's pad mask never fires
    # delay then revert gives the clip back where it was not pushed out
    c = _codes(2, 50, len(delay), 3)
    back = R.revert_delay(R.apply_delay(c, delay, BOS), delay)
    assert np.array_equal(back, c[:, :50 - md, :])


# ---- speed --------------------------------------------------------------------------------------------------------------------------
def _wave(L, seed):
    return np.random.default_rng(seed).standard_normal(L).astype(np.float32)


@pytest.mark.parametrize("speed", SPEEDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_adjust_speed_len_equals_the_c_sharp_expression_and_the_host_function(L, speed):
    want = adjust_speed(torch.zeros(L), speed).shape[-1]
    assert R.adjust_speed_len(L, speed) == want
    assert _lib.lib().nc_dia_adjust_speed_len(L, speed) == want


@pytest.mark.parametrize("speed", SPEEDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_interp_restatement_equals_the_torch_transcription_on_the_same_positions(L, speed):
    fp = _wave(L, 11 * L)
    T = R.adjust_speed_len(L, speed)
    x = R.linspace32(L, T)
    want = adjust_speed(torch.from_numpy(fp), speed, positions=torch.from_numpy(x)).numpy()
    got = R.adjust_speed(fp, speed)
    assert got.dtype == np.float32 and got.shape == want.shape == (T,)
    assert np.array_equal(got, want), (L, speed, int((got != want).sum()))
    if T != L:
        assert x[0] == 0 and (T == 1 or x[-1] == np.float32(L - 1))
        if T > 1:
            assert np.all(np.diff(x) > 0)


def test_linspace_restatement_equals_torch_linspace():
    rng = np.random.default_rng(5)
    sizes = [(L, R.adjust_speed_len(L, s)) for L in LENGTHS + (100003,) for s in SPEEDS]
    sizes += [(int(rng.integers(2, 200000)), int(rng.integers(1, 200000))) for _ in range(100)]
    sizes += [(2, 1), (2, 2), (2, 3), (3, 2), (1 << 24, 7), (40000, 32769), (40000, 65537)]   # past ATen's grain size: several threads
    for L, T in sizes:
        got, want = R.linspace32(L, T), torch.linspace(0, L - 1, T).numpy()
        assert got.dtype == want.dtype and np.array_equal(got, want), (L, T, int((got != want).sum()))


def test_fma32_rounds_once():
    """the one case a binary64 sum rounds twice: a * b + c half way between two binary32 values but for a bit far below"""
    a, b = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23)          # a * b = 1 - 2^-46 exactly
    c = np.float32(2.0 ** 24 + 2)                                           # ulp 2: c + a * b sits just below the midpoint c + 1
    assert R.fma32(a, b, c) == np.float32(2.0 ** 24 + 2)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(2.0 ** 24 + 4)   # (what rounding twice gives)
    assert R.fma32(np.float32(3), np.float32(5), np.float32(-15)) == 0


@pytest.mark.parametrize("speed", SPEEDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_adjust_speed_restatement_equals_the_torch_transcription(L, speed):
    """The whole of AdjustSpeed, torch.linspace included."""
    fp = _wave(L, 11 * L)
    want = adjust_speed(torch.from_numpy(fp), speed).numpy()
    got = R.adjust_speed(fp, speed)
    T = want.shape[-1]
    if T != L:
        x_t, x_r = torch.linspace(0, L - 1, T).numpy(), R.linspace32(L, T)
        print(f"L {L} speed {speed}: {int((x_t != x_r).sum())} of {T} linspace positions differ, {int((got != want).sum())} samples differ")
    assert got.shape == want.shape
    assert np.array_equal(got, want), (L, speed, int((got != want).sum()), T)


def test_adjust_speed_len_refusals():
    f = _lib.lib().nc_dia_adjust_speed_len
    assert f(0, 1.0) == -1 and f(-5, 0.5) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert f(1000, bad) == -1, bad
    assert f(1000, 1e-9) == -1                                            # a quotient past 2^31
    assert f(7, 8.0) == 7                                                 # (int)(7 / 8) = 0: unchanged
    assert f(100003, 0.99999) == 100004 == R.adjust_speed_len(100003, 0.99999)
    assert f(1000, 0.99999) == 1000


def test_output_query_needs_a_dac_handle():
    """nc_dia_output_query reads n_codebooks and the decoder strides from the handle, and a handle needs a device: its values and every
    refusal are held to the restatement in the GPU suite (tests/test_dia_output_gpu.py).  Without one it is NC_EINVAL, not a crash."""
    L = _lib.lib()
    delay = (C.c_int32 * 9)(*PATTERNS["dia"])
    out = (C.c_int64 * 2)()
    assert L.nc_dia_output_query(None, 2, 40, 9, delay, _lib.i64_array([5, 25]), None, out, out, out) == _lib.NC_EINVAL
    assert b"null codec handle" in L.nc_last_error()
