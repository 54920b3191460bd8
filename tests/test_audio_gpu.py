"""GPU suite: the audio pre/post kernels (csrc/nc_audio.hip through the C ABI) against the oracle, bit for bit.

The first tests run the Python wrappers on random data.  From `_dev` on, every kernel is called through its `_dev` entry point on slices
of larger device buffers filled with canaries (tests/audio_judge.py: Canvas), at lengths around the 256-thread block, and compared as
bit patterns with a truth written in the test or in tests/audio_judge.py.  The linear resampler has two judges: the oracle for bits and
the exact rational interpolant, within a derived bound, for meaning.

Each of those tests prints one `OPREPORT {...}` line (run with -s).  NC_AUDIO_REPORT=<path> writes the table of all of them, with those of
tests/test_containers_gpu.py when both files run in one process, to <path>: that is how
tests/golden/audio_op_report.json was recorded.  No test reads it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import audio_judge as J  # noqa: E402
from neuralcodecs_amd import _lib, audio  # noqa: E402
from oracle import audio_ref as R  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _write_table():
    yield
    J.write_table()


def test_pcm16_round_trip_and_layouts():
    rng = np.random.default_rng(0)
    pcm = rng.integers(-32768, 32768, size=2 * 50001, dtype=np.int16)
    np.testing.assert_array_equal(audio.pcm16_to_float(pcm), R.pcm16_to_float(pcm))
    np.testing.assert_array_equal(audio.pcm16_to_float(pcm, 2, planar=True), R.pcm16_to_float(pcm, 2, planar=True))
    x = (rng.standard_normal(100003) * 0.7).astype(np.float32)
    x[:4] = [1.0, -1.0, 7.0, -9.0]
    np.testing.assert_array_equal(audio.float_to_pcm16(x), R.float_to_pcm16(x))
    # every int16 except -32768 survives float -> pcm16 of (v/32768 * 32768/32767)... use the exact inverse scale instead
    allv = np.arange(-32767, 32768, dtype=np.int16)
    f = (allv.astype(np.float32) / np.float32(32767.0))
    back = audio.float_to_pcm16(f)
    assert np.abs(back.astype(np.int32) - allv.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_mix_to_mono(channels):
    rng = np.random.default_rng(channels)
    x = rng.standard_normal(channels * 44101).astype(np.float32)
    np.testing.assert_array_equal(audio.convert_to_mono(x, channels), R.mix_to_mono(x, channels))


@pytest.mark.parametrize("channels", [2, 5])
def test_interleave_deinterleave(channels):
    rng = np.random.default_rng(7)
    x = rng.standard_normal(channels * 12345).astype(np.float32)
    inter = audio.deinterleave_to_interleave(x, channels)
    np.testing.assert_array_equal(inter, R.interleave(x, channels))
    np.testing.assert_array_equal(audio.interleave_to_deinterleave(inter, channels), x)


@pytest.mark.parametrize("src,dst", [(44100, 24000), (24000, 44100), (48000, 44100), (16000, 16000), (8000, 44100)])
def test_resample_linear(src, dst):
    rng = np.random.default_rng(src + dst)
    x = rng.standard_normal((3, src // 4 + 17)).astype(np.float32)
    y = audio.resample_linear(x, src, dst)
    assert y.shape == (3, R.resample_len(x.shape[1], src, dst))
    for b in range(3):
        np.testing.assert_array_equal(y[b], R.resample_linear(x[b], src, dst))
    np.testing.assert_array_equal(audio.resample_linear(x[0], src, dst), R.resample_linear(x[0], src, dst))


def test_device_tensors_stay_on_device():
    import torch
    x = torch.randn(2 * 4096, device="cuda")
    m = audio.convert_to_mono(x, 2)
    assert m.is_cuda and m.shape == (4096,)
    np.testing.assert_array_equal(m.cpu().numpy(), R.mix_to_mono(x.cpu().numpy(), 2))
    p = audio.float_to_pcm16(m)
    assert p.is_cuda and p.dtype == torch.int16


def test_argument_errors():
    with pytest.raises(ValueError):
        audio.pcm16_to_float(np.zeros(3, np.int16), channels=2)
    with pytest.raises(ValueError):
        audio.resample_linear(np.zeros(1, np.float32), 44100, 8000)


# ======================================================================================== the `_dev` entry points, one kernel at a time
OK, E = _lib.NC_OK, _lib.NC_EINVAL


def _lengths_of(pool, n, seed):
    """n values of pool in a seeded order, the pool's last values (the non-finite ones) first."""
    order = np.random.default_rng(seed).permutation(pool.size - 8)
    return np.concatenate([pool[-8:], pool[order]])[:n] if n > 1 else pool[-1:]


def test_float_to_pcm16_every_truncation_boundary_and_nonfinite_input():
    """Truth: J.pcm16_truth (the exact binary64 product, one rounding to binary32, truncation).  -0.0 -> 0, +-inf -> +-32767 and every
    NaN -> 0 are inside it (tests/test_audio_cpu.py); a kernel that rounds, or clamps a NaN with fminf / fmaxf, differs."""
    lib, x = _lib.lib(), J.pcm16_inputs()
    compared = 0
    for n in (x.size,) + J.LENGTHS:
        xin = x if n == x.size else _lengths_of(x, n, n)
        src, dst = J.Canvas(np.float32, n, xin), J.Canvas(np.int16, n)
        assert lib.nc_audio_float_to_pcm16_dev(0, src.ptr, n, dst.ptr, None) == OK
        got = dst.read(f"float_to_pcm16 n={n}")
        compared += J.same_bits(got, J.pcm16_truth(xin), f"float_to_pcm16 n={n}")
        assert (got[np.isnan(xin)] == 0).all()
    J.report("float_to_pcm16", lengths=[int(x.size)] + list(J.LENGTHS), compared=compared, mismatches=0)


def test_pcm16_to_float_all_65536_values_and_every_length():
    lib = _lib.lib()
    allv = np.arange(-32768, 32768).astype(np.int16)
    allv = allv[np.random.default_rng(1).permutation(allv.size)]
    compared = 0
    for channels in (1, 2):                                                      # interleaved output: the layout does not depend on channels
        src, dst = J.Canvas(np.int16, allv.size, allv), J.Canvas(np.float32, allv.size)
        assert lib.nc_audio_pcm16_to_float_dev(0, src.ptr, allv.size // channels, channels, 0, dst.ptr, None) == OK
        compared += J.same_bits(dst.read(), (allv.astype(np.float64) * 2.0 ** -15).astype(np.float32), f"all values, {channels} channels")
    for n in J.LENGTHS:
        v = allv[:n]
        src, dst = J.Canvas(np.int16, n, v), J.Canvas(np.float32, n)
        assert lib.nc_audio_pcm16_to_float_dev(0, src.ptr, n, 1, 0, dst.ptr, None) == OK
        compared += J.same_bits(dst.read(), (v.astype(np.float64) * 2.0 ** -15).astype(np.float32), f"n={n}")
    J.report("pcm16_to_float", case="interleaved", compared=compared, mismatches=0)


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_pcm16_to_float_planar_puts_every_frame_and_channel_in_its_place(channels):
    lib, compared = _lib.lib(), 0
    for frames in (1, 257):
        f, c = np.meshgrid(np.arange(frames), np.arange(channels), indexing="ij")
        v = (f * 8 + c - 1000).astype(np.int16)                                   # [frames][channels]: the value names (frame, channel)
        src, dst = J.Canvas(np.int16, v.size, v), J.Canvas(np.float32, v.size)
        assert lib.nc_audio_pcm16_to_float_dev(0, src.ptr, frames, channels, 1, dst.ptr, None) == OK
        got = dst.read().reshape(channels, frames)
        want = np.empty((channels, frames), np.float32)
        for ch in range(channels):
            for fr in range(frames):
                want[ch, fr] = np.float32((fr * 8 + ch - 1000) * 2.0 ** -15)
        compared += J.same_bits(got, want, f"planar {channels} x {frames}")
    J.report("pcm16_to_float", case=f"planar-c{channels}", compared=compared, mismatches=0)


@pytest.mark.parametrize("channels", range(1, 9))
def test_mix_to_mono_sums_in_channel_order(channels):
    lib, compared = _lib.lib(), 0
    for frames in J.LENGTHS:
        x = np.random.default_rng([channels, frames]).standard_normal(frames * channels).astype(np.float32)
        src, dst = J.Canvas(np.float32, x.size, x), J.Canvas(np.float32, frames)
        assert lib.nc_audio_mix_to_mono_dev(0, src.ptr, frames, channels, dst.ptr, None) == OK
        compared += J.same_bits(dst.read(), R.mix_to_mono(x, channels), f"mono {channels} x {frames}")
    J.report("mix_to_mono", case=f"c{channels}", compared=compared, mismatches=0)


def test_mix_to_mono_cancelling_magnitudes_show_the_order_and_nonfinite_stays_in_its_frame():
    lib = _lib.lib()
    big, third = np.float32(1e8), np.float32(1.0) / np.float32(3.0)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    rows = [[big, 1, -big], [1, -big, big], [-big, big, 1],                      # (1e8 + 1) - 1e8 = 0; (1 - 1e8) + 1e8 = 0; (-1e8 + 1e8) + 1 = 1
            [0.5, 0.25, 0.25], [inf, 1, 2], [1, 2, 3], [1, -inf, 2], [4, 5, 6], [1, 2, nan], [7, 8, 9], [inf, 1, -inf], [-0.0, -0.0, -0.0]]
    want = np.array([0, 0, third, third, inf, 2, -inf, 5, nan, 8, nan, 0.0], np.float32)   # the sum starts at +0.0: -0.0 does not survive
    x = np.array(rows, np.float32).reshape(-1)
    src, dst = J.Canvas(np.float32, x.size, x), J.Canvas(np.float32, len(rows))
    assert lib.nc_audio_mix_to_mono_dev(0, src.ptr, len(rows), 3, dst.ptr, None) == OK
    got = dst.read()
    J.same_bits(got, want, "hand-worked rows", created_nan=True)                 # inf - inf makes the NaN of row 10
    with np.errstate(invalid="ignore"):
        J.same_bits(got, R.mix_to_mono(x, 3), "oracle", created_nan=True)
    assert got[8].view(np.uint32) == nan.view(np.uint32)                          # an input NaN goes through the additions as it is
    # the wrapper drops the samples behind the last whole frame (AudioUtils.cs:47)
    for extra in (1, 2):
        tail = np.concatenate([x, np.full(extra, 1e30, np.float32)])
        J.same_bits(audio.convert_to_mono(tail, 3), got, f"convert_to_mono with {extra} samples over", created_nan=True)
    J.report("mix_to_mono", case="order-and-nonfinite", compared=int(3 * got.size), mismatches=0)


def _payload_bits(n, seed):
    """n bit patterns: random, with NaN payloads of both signs, -0.0, a subnormal and the infinities among the first."""
    b = np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC12345, 0x80000000, 0xFFC00001, 0x7F800001, 0x00000001, 0xFF800000, 0x7F800000, 0x00000000], np.uint32)
    k = min(n, special.size)
    b[:k] = special[:k]
    return b


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8])
def test_interleave_and_deinterleave_are_pure_copies_to_the_right_place(channels):
    lib, compared = _lib.lib(), 0
    for frames in J.LENGTHS:
        n = frames * channels
        bits = np.roll(_payload_bits(n, [channels, frames]), frames // 2)          # the special patterns away from index 0
        planar_to_inter = np.empty(n, np.uint32)
        inter_to_planar = np.empty(n, np.uint32)
        for c in range(channels):
            planar_to_inter[c::channels] = bits[c * frames:(c + 1) * frames]       # out[f * C + c] = in[c * F + f]
            inter_to_planar[c * frames:(c + 1) * frames] = bits[c::channels]       # out[c * F + f] = in[f * C + c]
        for fn, want in ((lib.nc_audio_interleave_dev, planar_to_inter), (lib.nc_audio_deinterleave_dev, inter_to_planar)):
            src, dst = J.Canvas(np.float32, n, J.f32_from_bits(bits)), J.Canvas(np.float32, n)
            assert fn(0, src.ptr, frames, channels, dst.ptr, None) == OK
            compared += J.same_bits(dst.read(), J.f32_from_bits(want), f"{channels} x {frames}")
    J.report("interleave+deinterleave", case=f"c{channels}", compared=compared, mismatches=0)


@pytest.mark.parametrize("channels,n", [(2, 5), (2, 515), (3, 770), (3, 772), (5, 1284), (8, 2063)])
def test_wrappers_leave_plus_zero_behind_the_last_whole_frame(channels, n):
    """n % channels samples are over: the reference returns `new float[n]` with them at +0.0.  The device allocator hands back freed
    memory, so a buffer of NaNs is freed first: an output that is not zeroed shows them."""
    import torch
    x = J.f32_from_bits(_payload_bits(n, [channels, n]))
    for fn, ref in ((audio.deinterleave_to_interleave, R.interleave), (audio.interleave_to_deinterleave, R.deinterleave)):
        for kind in ("numpy", "torch"):
            junk = [torch.full((n,), float("nan"), device="cuda") for _ in range(3)]
            del junk
            got = fn(x, channels) if kind == "numpy" else fn(torch.from_numpy(x).cuda(), channels).cpu().numpy()
            J.same_bits(got, ref(x, channels), f"{fn.__name__} {kind}")
            assert n % channels and (J.bits_of(got)[-(n % channels):] == 0).all()
    J.report("interleave+deinterleave", case=f"tail-c{channels}-n{n}", compared=4 * n, mismatches=0)


# -------------------------------------------------------------------------------------------------------------- the linear resampler
def _resample_dev(x, src, dst, stream=None):
    B, n_in = x.shape
    n_out = R.resample_len(n_in, src, dst)
    assert _lib.lib().nc_audio_resample_len(n_in, src, dst) == n_out
    xin, out = J.Canvas(np.float32, x.size, x), J.Canvas(np.float32, B * n_out)
    assert _lib.lib().nc_audio_resample_linear_dev(0, xin.ptr, B, n_in, src, dst, out.ptr, stream) == OK
    return out.read(f"resample {src}->{dst}").reshape(B, n_out)


@pytest.mark.parametrize("case", J.RESAMPLE_CASES, ids=J.resample_id)
def test_resample_linear_bits_of_the_oracle_and_meaning_of_the_exact_interpolant(case):
    src, dst, n_in, B = case
    x, want = J.resample_case(*case)
    got = _resample_dev(x, src, dst)
    J.same_bits(got, want, J.resample_id(case))
    worst = max(J.resample_judge(got[b], x[b], src, dst, f"{J.resample_id(case)} row {b}") for b in range(B))
    if n_in == 1:
        assert np.array_equal(J.bits_of(got), J.bits_of(np.repeat(x, got.shape[1], axis=1)))
    J.report("resample_linear", case=J.resample_id(case), compared=int(got.size), mismatches=0, worst_err_over_allowed=worst)


def test_resample_linear_is_not_contracted():
    """The sentinels of tests/audio_judge.py: inputs at which fma((1 - f), x0, f x1) and fma(f, x1, (1 - f) x0) round to another binary32
    value than the two products and the sum the reference computes.  A build without -ffp-contract=off fails here and nowhere else."""
    for src, dst, o, b0, b1 in J.SENTINELS:
        x0, x1 = J.f32_from_bits([b0, b1])
        (unfused, fused_a, fused_b), index = J.blend_forms(src, dst, o, x0, x1)
        row = np.zeros((1, index + 4), np.float32)
        row[0, index], row[0, index + 1] = x0, x1
        got = _resample_dev(row, src, dst)[0, o]
        assert got.view(np.uint32) == unfused.view(np.uint32), \
            f"{src}->{dst} output {o}: {got!r}; unfused {unfused!r}, contracted {fused_a!r} or {fused_b!r}"
    J.report("resample_linear", case="contraction-sentinels", compared=len(J.SENTINELS), mismatches=0)


def test_resample_linear_nonfinite_samples_stay_where_the_blend_reads_them():
    """fraction 0 on an infinite sample is 0 * inf: the blend creates a NaN there (x86 and the GPU differ in its bits); a NaN sample
    keeps its payload through the held branch; everything two samples away is untouched."""
    x = np.random.default_rng(5).standard_normal((1, 40)).astype(np.float32)
    x[0, 10], x[0, 20], x[0, 30], x[0, 39] = np.inf, -np.inf, J.f32_from_bits([0x7FC12345])[0], J.f32_from_bits([0xFFC00077])[0]
    compared = 0
    for src, dst in ((1, 2), (2, 1), (3, 4), (44100, 48000)):
        with np.errstate(invalid="ignore"):
            want = R.resample_linear(x[0], src, dst)
        got = _resample_dev(x, src, dst)[0]
        clean = np.isfinite(want)
        assert clean.sum() > want.size // 2
        compared += J.same_bits(got[clean], want[clean], f"{src}->{dst} finite outputs")
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
        if (src, dst) == (1, 2):                                                   # positions o / 2 are exact: outputs 78 and 79 are held
            assert (got[78:].view(np.uint32) == 0xFFC00077).all() and got.size == 80
    J.report("resample_linear", case="nonfinite", compared=compared, mismatches=0)


def test_resample_linear_on_a_side_stream():
    import torch
    x, want = J.resample_case(44100, 48000, 3001, 3)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = _resample_dev(x, 44100, 48000, stream=s.cuda_stream)                     # Canvas.read synchronises the device
    J.same_bits(got, want, "side stream")


# --------------------------------------------------------------------------------------------------------------------- the wrappers
def test_wrappers_refuse_a_tensor_of_another_dtype_and_convert_numpy():
    import torch
    f64 = torch.zeros(12, dtype=torch.float64, device="cuda")
    i32 = torch.zeros(12, dtype=torch.int32, device="cuda")
    for call in (lambda t: audio.float_to_pcm16(t), lambda t: audio.convert_to_mono(t, 2), lambda t: audio.deinterleave_to_interleave(t, 2),
                 lambda t: audio.interleave_to_deinterleave(t, 2), lambda t: audio.resample_linear(t, 1, 2)):
        for t in (f64, i32, i32.short(), f64.cpu()):
            with pytest.raises(TypeError, match="float32"):
                call(t)
    for t in (i32, f64, f64.float(), i32.cpu()):
        with pytest.raises(TypeError, match="int16"):
            audio.pcm16_to_float(t)
    # numpy and list input is converted, as documented
    x64 = np.random.default_rng(3).standard_normal(12)
    J.same_bits(audio.float_to_pcm16(x64), R.float_to_pcm16(x64.astype(np.float32)), "float64 numpy")
    J.same_bits(audio.convert_to_mono(x64, 3), R.mix_to_mono(x64.astype(np.float32), 3), "float64 numpy")
    J.same_bits(audio.pcm16_to_float(np.arange(-6, 6)), R.pcm16_to_float(np.arange(-6, 6, dtype=np.int16)), "int64 numpy")
    J.same_bits(audio.pcm16_to_float([3, -4]), R.pcm16_to_float(np.array([3, -4], np.int16)), "list")
    # a transposed view is made contiguous: the kernel sees its logical order
    m = torch.from_numpy(np.arange(24, dtype=np.float32).reshape(4, 6)).cuda()
    J.same_bits(audio.resample_linear(m.T, 1, 2).cpu().numpy(),
                np.stack([R.resample_linear(r, 1, 2) for r in m.T.cpu().numpy()]), "transposed view")
    J.same_bits(audio.float_to_pcm16(m.T / 32).cpu().numpy(), R.float_to_pcm16((m.T / 32).cpu().numpy().reshape(-1)), "transposed view")


# -------------------------------------------------------------------------------------------------------------------- the refusals
def test_refusals_leave_the_outputs_untouched_and_the_device_usable():
    lib = _lib.lib()
    fin, pin = J.Canvas(np.float32, 1024, np.zeros(1024, np.float32)), J.Canvas(np.int16, 1024, np.zeros(1024, np.int16))
    fout, pout = J.Canvas(np.float32, 4096), J.Canvas(np.int16, 1024)
    calls = 0

    def refused(fn, good, **bad):
        """fn(**good) with one argument replaced must return NC_EINVAL."""
        nonlocal calls
        for k, v in bad.items():
            a = dict(good, **{k: v})
            assert fn(*a.values()) == E, (fn.__name__, k, v)
            calls += 1

    refused(lib.nc_audio_pcm16_to_float_dev, dict(dev=0, i=pin.ptr, n=8, c=2, p=0, o=fout.ptr, s=None), i=None, o=None, n=0, c=0, dev=999)
    refused(lib.nc_audio_pcm16_to_float_dev, dict(dev=0, i=pin.ptr, n=8, c=2, p=1, o=fout.ptr, s=None), n=-1, c=-2, dev=-1)
    refused(lib.nc_audio_float_to_pcm16_dev, dict(dev=0, i=fin.ptr, n=8, o=pout.ptr, s=None), i=None, o=None, n=0, dev=999)
    refused(lib.nc_audio_float_to_pcm16_dev, dict(dev=0, i=fin.ptr, n=8, o=pout.ptr, s=None), n=-5)
    for fn in (lib.nc_audio_mix_to_mono_dev, lib.nc_audio_interleave_dev, lib.nc_audio_deinterleave_dev):
        refused(fn, dict(dev=0, i=fin.ptr, n=8, c=2, o=fout.ptr, s=None), i=None, o=None, n=0, c=0, dev=999)
        refused(fn, dict(dev=0, i=fin.ptr, n=8, c=2, o=fout.ptr, s=None), n=-1, c=-1)
    good = dict(dev=0, i=fin.ptr, B=1, n=8, src=1, dst=2, o=fout.ptr, s=None)
    refused(lib.nc_audio_resample_linear_dev, good, i=None, o=None, B=0, n=0, src=0, dst=0, dev=999)
    refused(lib.nc_audio_resample_linear_dev, good, B=-1, n=-1, src=-1, dst=-44100)
    for src, dst, n in J.RESAMPLE_EMPTY:                                          # a clip that would resample to nothing
        assert lib.nc_audio_resample_len(n, src, dst) == 0
        refused(lib.nc_audio_resample_linear_dev, dict(good, src=src, dst=dst), n=n)
    assert fout.untouched() and pout.untouched() and fin.untouched() and pin.untouched()
    with pytest.raises(ValueError):
        audio.resample_linear(np.zeros(3, np.float32), 100, 1)
    x, want = J.resample_case(3, 4, 257, 3)                                        # one valid call follows
    J.same_bits(_resample_dev(x, 3, 4), want, "after the refusals")
    J.same_bits(audio.float_to_pcm16(J.pcm16_inputs()), J.pcm16_truth(J.pcm16_inputs()), "after the refusals")
    J.report("refusals", case="nc_audio", compared=calls, mismatches=0)
