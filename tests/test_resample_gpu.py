"""GPU suite of the band-limited resampler: resample_mfma_kernel, resample_vec_kernel and the copy against the serial host twin of the
library (tests/test_resample_cpu.py holds that to binary64) -- np.array_equal on bit patterns of whole output buffers, no tolerance.  Input
rows sit at odd element offsets with NaN-filled gaps, output rows in a NaN-filled canvas, so a read or a store outside a row shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import resample_ref as R  # noqa: E402
from conftest import dac_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import DAC, ResampleConfig, _lib, resample_sinc, resample_sinc_geom, resample_sinc_len, resample_sinc_packed  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402

# 3 -> 2, 2 -> 3, 2 -> 1, 1 -> 2: small U, the vector kernel.  48000 -> 44100: U = 147 (no multiple of 16), even D, K4 = K.  44100 -> 48000: U a
# multiple of 16, odd D, K = 199 (one zero tap).  16000 -> 44100: U = 441, 28 phase tiles, a 365 KB table.
PAIRS = [(3, 2), (2, 3), (2, 1), (1, 2), (48000, 44100), (44100, 48000), (16000, 44100)]
CAP = 12000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_buffers(got, want):
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _lengths(src, dst, cfg=None):
    """1 and 2; around W, D, the workgroup's 16 frames (16 D) and its stretch (15 D + K4); one row of about a quarter second"""
    g = resample_sinc_geom(src, dst, cfg)
    W, D, K4 = g["W"], g["D"], g["K4"]
    stretch = 15 * D + K4
    long_row = int(0.25 * src) if src >= 1000 else 3001
    lens = [1, 2, W - 1, W, W + 1, D - 1, D, D + 1, 16 * D - 1, 16 * D, 16 * D + 1, stretch - 1, stretch, stretch + 1, long_row]
    return [min(max(n, 0), CAP) for n in lens]


def _packed(lens, seed):
    """(buffer, offsets) with ODD element offsets and gaps of NaN between the rows"""
    offs, o = [], 1
    for n in lens:
        offs.append(o)
        o += n + (2 if (o + n) % 2 else 3)
    buf = np.full(o, np.nan, np.float32)
    for i, (at, n) in enumerate(zip(offs, lens)):
        buf[at:at + n] = R.signal(n, seed + i)
    assert all(v % 2 == 1 for v in offs)
    return buf, offs


def _out_offsets(olens, aligned):
    """rows at multiples of four elements (the 16-byte store) or at odd offsets (the 4-byte stores), a gap behind each"""
    oo, o = [], 4 if aligned else 1
    for n in olens:
        oo.append(o)
        o += n + 3
        o += (-o) % 4 if aligned else (0 if o % 2 else 1)
    return oo, o + 4


def _run_both(buf, lens, offs, src, dst, aligned, cfg=None):
    import torch
    olens = [resample_sinc_len(n, src, dst) for n in lens]
    oo, size = _out_offsets(olens, aligned)
    canvas = np.full(size, np.nan, np.float32)
    want, _, wl = resample_sinc_packed(buf, src, dst, lens, offs, oo, out=canvas.copy(), cfg=cfg, host=True)
    dev_out = torch.from_numpy(canvas.copy()).cuda()
    assert dev_out.data_ptr() % 16 == 0
    got, _, gl = resample_sinc_packed(torch.from_numpy(buf).cuda(), src, dst, lens, offs, oo, out=dev_out, cfg=cfg)
    assert wl == gl == olens
    return got.cpu().numpy(), want, oo, olens


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_resample_equals_the_host_twin(pair, aligned):
    src, dst = pair
    lens = _lengths(src, dst)
    buf, offs = _packed(lens, 100 * src + dst)
    got, want, oo, olens = _run_both(buf, lens, offs, src, dst, aligned)
    assert np.isfinite(np.concatenate([want[o:o + n] for o, n in zip(oo, olens)])).all()
    assert np.isnan(want).sum() == want.size - sum(olens)
    _same_buffers(got, want)


def test_non_default_config_equals_the_host_twin():
    src, dst = 48000, 44100
    cfg = ResampleConfig(8, 1.0)
    g = resample_sinc_geom(src, dst, cfg)
    assert g["K"] < 216 and g["K4"] != g["K"]
    lens = _lengths(src, dst, cfg)
    buf, offs = _packed(lens, 77)
    got, want, _, _ = _run_both(buf, lens, offs, src, dst, True, cfg)
    _same_buffers(got, want)
    _same_buffers(*_run_both(buf, lens, offs, src, dst, False, cfg)[:2])


@pytest.mark.parametrize("pair", [(2, 3), (44100, 48000)], ids=["vector", "matrix"])
def test_non_finite_samples_equal_the_host_twin(pair):
    src, dst = pair
    lens = [4001, 3000]
    buf, offs = _packed(lens, 5)
    buf[offs[0] + 1500], buf[offs[0] + 2600], buf[offs[1] + 7] = np.nan, np.inf, -np.inf
    got, want, oo, olens = _run_both(buf, lens, offs, src, dst, True)
    rows = np.concatenate([want[o:o + n] for o, n in zip(oo, olens)])
    assert np.isnan(rows).any() and np.isfinite(rows).any()
    _same_buffers(got, want)


@pytest.mark.parametrize("pair", [(3, 2), (16000, 44100)], ids=["vector", "matrix"])
def test_rows_are_independent_of_the_batch(pair):
    src, dst = pair
    D = resample_sinc_geom(src, dst)["D"]
    lens = [1, 16 * D + 5, 0, 700, 16 * D, 2901]
    rows = [R.signal(n, 9 + i) for i, n in enumerate(lens)]
    whole = resample_sinc(rows, src, dst)
    again = resample_sinc(rows, src, dst)
    perm = [3, 5, 0, 2, 4, 1]
    shuffled = resample_sinc([rows[i] for i in perm], src, dst)
    for at, i in enumerate(perm):
        alone = resample_sinc([rows[i]], src, dst)[0]
        assert len(alone) == resample_sinc_len(lens[i], src, dst)
        for other in (whole[i], again[i], shuffled[at]):
            _same_buffers(other, alone)


def test_same_rate_copies():
    lens = [1, 255, 256, 257, 3000]
    buf, offs = _packed(lens, 31)
    got, want, oo, olens = _run_both(buf, lens, offs, 44100, 44100, False)
    assert olens == lens
    _same_buffers(got, want)
    for o, at, n in zip(oo, offs, lens):
        _same_buffers(got[o:o + n], buf[at:at + n])


def test_device_tensors_stay_on_the_device_and_on_the_current_stream():
    import torch
    src, dst = 44100, 48000
    rows = [R.signal(n, 60 + n) for n in (5000, 147, 2353)]
    want = resample_sinc(rows, src, dst, host=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = [torch.from_numpy(r).cuda(non_blocking=False) for r in rows]
        got = resample_sinc(dev, src, dst)
        first = resample_sinc([dev[0]], src, dst, ResampleConfig(8, 1.0))[0]      # another table, uploaded while `side` is current
    assert all(g.is_cuda and g.dtype == torch.float32 for g in got)
    side.synchronize()
    for g, w in zip(got, want):
        _same_buffers(g.cpu().numpy(), w)
    _same_buffers(first.cpu().numpy(), resample_sinc([rows[0]], src, dst, ResampleConfig(8, 1.0), host=True)[0])
    again = resample_sinc(dev, src, dst)                                           # the default stream, behind the call on `side`
    torch.cuda.synchronize()
    for g, w in zip(again, want):
        _same_buffers(g.cpu().numpy(), w)


def test_host_buffer_call_equals_the_twin():
    """the plain (synchronous, HOST buffer) export"""
    lib, i64 = _lib.lib(), _lib.i64_array
    src, dst = 48000, 44100
    lens = [2561, 0, 900]
    buf, offs = _packed(lens, 12)
    olens = [resample_sinc_len(n, src, dst) for n in lens]
    oo, size = _out_offsets(olens, False)
    want, _, _ = resample_sinc_packed(buf, src, dst, lens, offs, oo, out=np.full(size, np.nan, np.float32), host=True)
    out = np.full(size, np.nan, np.float32)
    assert lib.nc_audio_resample_sinc(0, buf.ctypes.data, 3, i64(offs), i64(lens), src, dst, None, out.ctypes.data, i64(oo)) == _lib.NC_OK
    _same_buffers(out, want)


def test_refusals_leave_the_device_usable():
    import torch
    lib, i64, E = _lib.lib(), _lib.i64_array, _lib.NC_EINVAL
    x = torch.zeros(4096, dtype=torch.float32, device="cuda")
    out = torch.zeros(8192, dtype=torch.float32, device="cuda")

    def call(pcm=x.data_ptr(), R_=1, off=(0,), n=(1000,), src=48000, dst=44100, o=out.data_ptr(), oo=(0,), dev=0):
        return lib.nc_audio_resample_sinc_dev(dev, pcm, R_, i64(off), i64(n), src, dst, None, o, i64(oo), None)

    assert call(pcm=None) == E and call(o=None) == E and call(R_=0) == E and call(n=(-1,)) == E and call(n=(2 ** 30 + 1,)) == E
    assert call(src=0) == E and call(src=44100, dst=44101) == E and call(off=(-1,)) == E and call(dev=999) == E
    assert call(o=x.data_ptr(), oo=(500,)) == E and call(o=x.data_ptr(), oo=(2000,)) == _lib.NC_OK
    torch.cuda.synchronize()
    row = R.signal(3000, 4)
    _same_buffers(resample_sinc([row], 48000, 44100)[0], resample_sinc([row], 48000, 44100, host=True)[0])   # one valid call follows


def test_dac_resample_ragged_then_encode_ragged_equals_the_twin_path():
    g = load_golden("dac_small")
    cfg = dac_cfg_from_meta(g["meta"])
    with DAC(cfg, device_index=0) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"])))
        lens = [9000, 11800, 7003]
        clips = [np.float32(0.4) * synthetic_pcm(1, 1, T, 48000, seed=500 + i)[0, 0] for i, T in enumerate(lens)]
        at_rate = m.resample_ragged(clips, 48000)
        twin = m.resample_ragged(clips, 48000, host=True)
        assert [len(c) for c in at_rate] == [resample_sinc_len(T, 48000, cfg.sample_rate) for T in lens]
        for a, b in zip(at_rate, twin):
            _same_buffers(a, b)
        codes, codes_twin = m.encode_ragged(at_rate), m.encode_ragged(twin)
        assert len(codes) == 3
        for a, b in zip(codes, codes_twin):
            assert a.shape == b.shape and np.array_equal(a, b)
