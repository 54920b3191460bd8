"""CPU suite: the audio pre/post oracle (oracle/audio_ref.py) against hand-worked known answers of the reference's helpers
(Core/Utils/AudioUtils.cs:13-36,45-61,90-101,172-186,204-219,329-354; Models/Dia.cs:918-923)."""
import numpy as np

from oracle import audio_ref as R


def test_pcm16_to_float_known_answers():
    pcm = np.array([0, 1, -1, 16384, -32768, 32767], np.int16)
    out = R.pcm16_to_float(pcm)
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out, np.array([0.0, 2.0 ** -15, -(2.0 ** -15), 0.5, -1.0, 32767.0 / 32768.0], np.float32))
    # planar: L0 R0 L1 R1 -> L0 L1 R0 R1   (NAudioUtils.cs:94-104)
    st = np.array([100, -100, 200, -200], np.int16)
    np.testing.assert_array_equal(R.pcm16_to_float(st, 2, planar=True), np.array([100, 200, -100, -200], np.float32) / 32768.0)


def test_float_to_pcm16_truncates_and_clamps():
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -3.0, 0.99999, 1e-5], np.float32)
    out = R.float_to_pcm16(x)
    # 0.5*32767 = 16383.5 -> 16383 (toward zero); -16383.5 -> -16383
    np.testing.assert_array_equal(out, np.array([0, 16383, -16383, 32767, -32767, 32767, -32767, 32766, 0], np.int16))


def test_mix_to_mono_order_and_division():
    x = np.array([1.0, 2.0, 4.0,  1e8, 1.0, -1e8], np.float32)
    out = R.mix_to_mono(x, 3)
    # frame 1: (1e8 + 1) rounds to 1e8 in float32, then - 1e8 = 0 -> 0/3
    np.testing.assert_array_equal(out, np.array([np.float32(7.0) / np.float32(3.0), 0.0], np.float32))


def test_interleave_round_trip():
    planar = np.arange(10, dtype=np.float32)          # L = 0..4, R = 5..9
    inter = R.interleave(planar, 2)
    np.testing.assert_array_equal(inter, np.array([0, 5, 1, 6, 2, 7, 3, 8, 4, 9], np.float32))
    np.testing.assert_array_equal(R.deinterleave(inter, 2), planar)


def test_resample_linear_known_answers():
    x = np.array([0.0, 1.0, 2.0, 3.0], np.float32)
    up = R.resample_linear(x, 1, 2)                   # positions 0, .5, 1, 1.5, 2, 2.5, 3(last), 3.5(last)
    np.testing.assert_array_equal(up, np.array([0, 0.5, 1, 1.5, 2, 2.5, 3, 3], np.float32))
    down = R.resample_linear(x, 2, 1)                 # positions 0, 2
    np.testing.assert_array_equal(down, np.array([0, 2], np.float32))
    assert R.resample_len(44100, 44100, 24000) == 24000
    assert R.resample_len(1000, 44100, 24000) == int(1000 * (24000 / 44100))
    # a non-dyadic ratio: every output is the binary64 blend rounded once to float32
    y = R.resample_linear(np.array([0.1, 0.7, -0.3], np.float32), 3, 4)
    ratio = 4 / 3
    exp = []
    xin = np.array([0.1, 0.7, -0.3], np.float32)
    for i in range(int(3 * ratio)):
        pos = i / ratio
        idx = int(pos)
        fr = pos - idx
        exp.append(xin[-1] if idx >= 2 else np.float32((1 - fr) * float(xin[idx]) + fr * float(xin[idx + 1])))
    np.testing.assert_array_equal(y, np.array(exp, np.float32))


# ----------------------------------------------------------------------------- what tests/test_audio_gpu.py leans on (tests/audio_judge.py)
import pytest  # noqa: E402

import audio_judge as J  # noqa: E402
from neuralcodecs_amd import _lib  # noqa: E402


def test_float_to_pcm16_nan_is_zero_and_inf_is_full_scale():
    """Math.Min(1f, NaN) is NaN and (short)(NaN * 32767) is 0: a NaN sample is silence, never a full-scale click."""
    x = np.concatenate([J.f32_from_bits(J.QUIET_NANS), np.array([np.inf, -np.inf, -0.0, 3e38, -3e38], np.float32)])
    np.testing.assert_array_equal(R.float_to_pcm16(x), np.array([0, 0, 0, 0, 32767, -32767, 0, 32767, -32767], np.int16))


def test_pcm16_truth_is_the_oracle_on_every_input_used():
    x = J.pcm16_inputs()
    assert x.size == 3 * 65535 + 16 + len(J.QUIET_NANS) and np.isnan(x).sum() == len(J.QUIET_NANS)
    truth = J.pcm16_truth(x)
    np.testing.assert_array_equal(truth, R.float_to_pcm16(x))
    assert set(np.unique(truth)) == set(range(-32767, 32768))                    # every code is reached ...
    k = np.arange(-32767, 32768)
    below, at, above = truth[:65535], truth[65535:2 * 65535], truth[2 * 65535:3 * 65535]
    assert np.array_equal(np.unique(np.concatenate([at - k, below - k, above - k])), [-1, 0, 1])   # ... and both sides of its boundary
    assert (np.abs(at - k) <= 1).all() and (below <= at).all() and (at <= above).all()
    assert (truth[np.isnan(x)] == 0).all() and (truth[np.isinf(x)] == np.sign(x[np.isinf(x)]) * 32767).all()


def test_interleave_and_deinterleave_leave_a_zero_tail():
    """AudioUtils.cs:92-93, 206-207: samplesPerChannel = n / 2 and `new float[n]`, so the odd sample is dropped and its slot is +0.0."""
    five = np.array([1, 2, 3, 4, 5], np.float32)                                  # L = 1 2, R = 3 4, and one sample over
    for got, want in ((R.interleave(five, 2), [1, 3, 2, 4, 0]), (R.deinterleave(five, 2), [1, 3, 2, 4, 0]),
                      (R.interleave(five, 3), [1, 2, 3, 0, 0]), (R.deinterleave(np.arange(1, 9, dtype=np.float32), 3), [1, 4, 2, 5, 3, 6, 0, 0])):
        assert got.dtype == np.float32 and np.array_equal(J.bits_of(got), J.bits_of(np.array(want, np.float32)))
    x = J.f32_from_bits([0x7FC12345, 0x80000000, 0xFFC00001, 0x00000001, 0x3F800000, 0xFF800000])
    assert np.array_equal(J.bits_of(R.deinterleave(R.interleave(x, 3), 3)), J.bits_of(x))     # pure copies: payloads and -0.0 survive


def test_resample_cases_cover_what_they_claim():
    assert len(J.RESAMPLE_CASES) + 2 * len(J.RESAMPLE_EMPTY) == len(J.RATES) * len(J.N_IN) * len(J.ROWS)
    assert set(J.RESAMPLE_EMPTY) == {(2, 1, 1), (4, 3, 1), (48000, 44100, 1), (48000, 8000, 1), (48000, 8000, 2), (48000, 8000, 3),
                                     (100, 1, 1), (100, 1, 2), (100, 1, 3)}
    lens = {(s, d, n): R.resample_len(n, s, d) for s, d, n, _ in J.RESAMPLE_CASES}
    assert 1 in lens.values() and lens[(100, 1, 257)] == 2 and lens[(1, 100, 3001)] == 300100
    for s, d, n, _ in J.RESAMPLE_CASES:                                           # the held branch and the output before it
        if n >= 2 and d >= 2 * s:                                                 # (n - 1) d / s <= n d / s - 2: an output reaches it
            assert J.branch_edge(s, d, n) > 0, (s, d, n)
    assert J.branch_edge(1, 1, 257) == 256 and J.branch_edge(2, 1, 257) is None


@pytest.mark.parametrize("case", J.RESAMPLE_CASES, ids=J.resample_id)
def test_resampler_oracle_stays_inside_the_derived_bound(case):
    src, dst, n_in, B = case
    x, y = J.resample_case(*case)
    worst = max(J.resample_judge(y[b], x[b], src, dst, f"{J.resample_id(case)} row {b}") for b in range(B))
    assert worst <= 1.0
    if n_in == 1:
        assert np.array_equal(y, np.repeat(x, y.shape[1], axis=1))                # every output is x[0]
    e = J.branch_edge(src, dst, n_in)
    if e is not None:
        assert np.array_equal(y[:, e:], np.repeat(x[:, -1:], y.shape[1] - e, axis=1))
    if (src, dst) in ((1, 2), (2, 1), (1, 1), (100, 1)) and n_in > 1:             # positions on integers: the sample itself
        step = src // dst if src >= dst else 1
        o = np.arange(0, y.shape[1], 1 if src >= dst else dst // src)
        i = o * src // dst
        keep = i < n_in
        assert step >= 1 and np.array_equal(y[:, o[keep]], x[:, i[keep]])


def test_sentinels_tell_the_unfused_blend_from_both_fused_ones():
    assert len(J.SENTINELS) >= 4
    for src, dst, o, b0, b1 in J.SENTINELS:
        x0, x1 = J.f32_from_bits([b0, b1])
        (unfused, fused_a, fused_b), index = J.blend_forms(src, dst, o, x0, x1)
        assert unfused != fused_a and unfused != fused_b, (src, dst, o)
        row = np.zeros(index + 4, np.float32)                                     # the oracle is the unfused form
        row[index], row[index + 1] = x0, x1
        assert R.resample_linear(row, src, dst)[o].view(np.uint32) == unfused.view(np.uint32)


def test_resample_len_refuses_what_does_not_fit_an_int():
    L = _lib.lib()
    f = L.nc_audio_resample_len
    assert f(2 ** 31 - 1, 1, 1) == 2 ** 31 - 1 and f(2 ** 31, 1, 1) == -1 and f(2 ** 31 + 1, 1, 1) == -1
    assert f(2 ** 30, 1, 2) == -1 and f(2 ** 30 - 1, 1, 2) == 2 ** 31 - 2 and f(2 ** 32, 2, 1) == -1 and f(2 ** 32 - 2, 2, 1) == 2 ** 31 - 1
    assert f(2 ** 62, 1, 1) == -1 and f(2 ** 40, 48000, 1) == (2 ** 40 * (1 / 48000)).__trunc__()
    assert f(0, 44100, 48000) == 0 and f(-1, 1, 1) == -1
    assert f(100, 0, 1) == -1 and f(100, 1, 0) == -1 and f(100, -1, 1) == -1 and f(100, 1, -5) == -1
    for n, s, d in [(2 ** 31, 1, 1), (2 ** 31 - 1, 1, 1), (2 ** 30, 1, 2), (0, 3, 4), (100, 0, 1), (1000, 44100, 24000), (3001, 1, 100)]:
        assert f(n, s, d) == R.resample_len(n, s, d)
    # refused on the length alone, before any device call: the pointers are never read
    assert L.nc_audio_resample_linear_dev(0, 4096, 1, 2 ** 31, 1, 2, 4096, None) == _lib.NC_EINVAL
    assert b"2^31" in L.nc_last_error()
