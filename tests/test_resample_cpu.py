"""CPU suite of the band-limited resampler: the serial host twin (nc_audio_resample_sinc_host), the geometry and the table builder, judged
by tests/resample_ref.py (a binary64 numpy statement of the header) and by scipy.signal.upfirdn on the interleaved prototype filter, which
shares no indexing with either; the design itself (pass band, stop band) on the binary64 reference; and the record of why the reference's
AudioSignal.ResampleFrac is not mirrored.  No device is used; tests/test_resample_gpu.py holds the kernels to the twin bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import resample_ref as R
from neuralcodecs_amd import ResampleConfig, _lib, resample_sinc, resample_sinc_geom, resample_sinc_len, resample_sinc_packed, resample_sinc_table
from neuralcodecs_amd import resample as RS

CFGS = [None, ResampleConfig(8, 1.0)]


def _kw(cfg):
    return {} if cfg is None else dict(zeros=cfg.zeros, rolloff=cfg.rolloff)


def twin(x, src, dst, cfg=None):
    return resample_sinc([np.asarray(x, np.float32)], src, dst, cfg, host=True)[0]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ geometry, table
@pytest.mark.parametrize("pair", R.PAIRS)
def test_geometry_and_lengths_are_the_reference(pair):
    src, dst = pair
    g = resample_sinc_geom(src, dst)
    q = R.geom(src, dst)
    assert (g["U"], g["D"], g["W"], g["K"]) == R.GEOM[pair] == (q["U"], q["D"], q["W"], q["K"])
    assert g["K4"] == q["K4"] and g["K4"] % 4 == 0 and 0 <= g["K4"] - g["K"] < 4
    for n in (0, 1, 2, 159, 160, 161, 4800, 44100, 2 ** 30):
        assert resample_sinc_len(n, src, dst) == R.n_out(n, src, dst)
    g2, q2 = resample_sinc_geom(src, dst, ResampleConfig(8, 1.0)), R.geom(src, dst, 8, 1.0)
    assert (g2["W"], g2["K"], g2["K4"]) == (q2["W"], q2["K"], q2["K4"])
    assert resample_sinc_geom(src, dst, ResampleConfig(0, 0.0)) == g            # zero fields: the defaults


@pytest.mark.parametrize("cfg", CFGS, ids=["default", "z8r1"])
@pytest.mark.parametrize("pair", R.PAIRS + [(32000, 44100), (3, 2), (2, 3)])
def test_table_is_the_binary64_table_rounded_once(pair, cfg):
    """libm's sin / cos are kept (the header says why): within 1 ulp of binary32 everywhere, equal nearly everywhere"""
    src, dst = pair
    got = resample_sinc_table(src, dst, cfg)
    q, want = R.table32(src, dst, **_kw(cfg))
    assert got.shape == want.shape == (q["U"], q["K4"]) and got.dtype == np.float32
    assert R.ulp_distance(got, want).max() <= 1
    assert (_bits(got) == _bits(want)).mean() >= 0.999
    assert (_bits(got[:, q["K"]:]) == 0).all()                                   # +0, not -0
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= q["K4"] * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ the twin
LENGTHS = [1, 2, 37, 400, 3001]


@pytest.fixture(scope="module")
def twin_runs():
    """(pair, cfg id, n) -> (x, twin result): computed once, shared by the two judges"""
    out = {}
    for pair in R.PAIRS:
        for ci, cfg in enumerate(CFGS):
            for n in LENGTHS:
                x = R.signal(n, 17 * n + ci)
                out[(pair, ci, n)] = (x, twin(x, *pair, cfg))
    return out


@pytest.mark.parametrize("ci", [0, 1], ids=["default", "z8r1"])
@pytest.mark.parametrize("pair", R.PAIRS)
def test_twin_is_within_the_chain_bound_of_binary64(twin_runs, pair, ci):
    for n in LENGTHS:
        x, y = twin_runs[(pair, ci, n)]
        want, mag, q = R.resample64(x, *pair, **_kw(CFGS[ci]))
        assert y.shape == want.shape == (R.n_out(n, *pair),) and y.dtype == np.float32
        err, bound = np.abs(y.astype(np.float64) - want), R.chain_bound(mag, q)
        assert (err <= bound).all(), (n, float((err / np.maximum(bound, 1e-300)).max()))
        assert err.max() > 0 or n <= 2                                          # a binary32 chain, not the judge's own arithmetic


@pytest.mark.parametrize("ci", [0, 1], ids=["default", "z8r1"])
@pytest.mark.parametrize("pair", R.PAIRS)
def test_twin_against_scipy_upfirdn_on_the_interleaved_prototype(twin_runs, pair, ci):
    """y[m U + i] = sum_k h[i][k] xpad[m D + k] is upfirdn(p, xpad, U, D)[o + s] with p[i D + (K - 1 - k) U + (s D - (K - 1) U)] = h[i][k],
    s = ceil((K - 1) U / D): one FIR on the zero-stuffed signal, no frames and no phases"""
    from scipy.signal import upfirdn
    kw = _kw(CFGS[ci])
    q, h = R.table64(*pair, **kw)
    U, D, W, K = q["U"], q["D"], q["W"], q["K"]
    s = -(-(K - 1) * U // D)
    shift = s * D - (K - 1) * U
    p = np.zeros((U - 1) * D + (K - 1) * U + shift + 1)
    i, k = np.meshgrid(np.arange(U), np.arange(K), indexing="ij")
    at = i * D + (K - 1 - k) * U + shift
    assert len(np.unique(at)) == U * K
    p[at] = h
    for n in LENGTHS:
        x, y = twin_runs[(pair, ci, n)]
        no = R.n_out(n, *pair)
        frames = -(-no // U)
        xpad = np.pad(x.astype(np.float64), (W, frames * D + W - n), mode="edge")
        z = upfirdn(p, xpad, U, D)
        want = z[s:s + no]
        mag = upfirdn(np.abs(p), np.abs(xpad), U, D)[s:s + no]
        assert want.shape == y.shape
        err, bound = np.abs(y.astype(np.float64) - want), R.chain_bound(mag, q)
        assert (err <= bound).all(), (n, float((err / np.maximum(bound, 1e-300)).max()))


def test_same_rate_copies_and_empty_rows_write_nothing():
    x = R.signal(100, 3)
    assert np.array_equal(_bits(twin(x, 44100, 44100)), _bits(x))
    canvas = np.full(64, np.nan, np.float32)
    out, oo, olens = resample_sinc_packed(np.concatenate([x[:10], x[:7]]), 2, 3, [10, 0, 7], [0, 10, 10], [1, 20, 30], out=canvas, host=True)
    assert olens == [15, 0, 11] and oo == [1, 20, 30]
    assert np.isnan(out).sum() == 64 - 26 and np.isfinite(out[1:16]).all() and np.isfinite(out[30:41]).all()


def test_nonfinite_samples_stay_local_and_come_out_as_the_quiet_nan():
    src, dst = 48000, 44100
    g = resample_sinc_geom(src, dst)
    x = R.signal(4000, 9)
    x[2000], x[3000] = np.nan, np.inf
    y = twin(x, src, dst)
    bad = ~np.isfinite(y)
    assert bad.any() and (_bits(y[np.isnan(y)]) == 0x7fc00000).all()
    reach = (g["K4"] / g["D"] + 2) * g["U"]
    o = np.flatnonzero(bad)
    assert o.min() >= 2000 * g["U"] / g["D"] - reach and o.max() <= 3000 * g["U"] / g["D"] + reach
    clean = twin(np.where(np.isfinite(x), x, 0).astype(np.float32), src, dst)
    far = np.ones(len(y), bool)
    far[int(o.min()) - 1:int(o.max()) + 2] = False
    assert np.array_equal(_bits(y[far]), _bits(clean[far]))


def test_rows_are_independent_of_the_batch():
    src, dst = 44100, 48000
    lens = [1, 146, 147, 148, 2500, 0, 901]
    rows = [R.signal(n, 50 + i) for i, n in enumerate(lens)]
    whole = resample_sinc(rows, src, dst, host=True)
    again = resample_sinc(rows, src, dst, host=True)
    perm = [4, 0, 6, 2, 5, 1, 3]
    shuffled = resample_sinc([rows[i] for i in perm], src, dst, host=True)
    for at, i in enumerate(perm):
        alone = twin(rows[i], src, dst)
        assert len(alone) == R.n_out(lens[i], src, dst)
        for other in (whole[i], again[i], shuffled[at]):
            assert np.array_equal(_bits(alone), _bits(other)), i
    stereo = resample_sinc([np.stack([rows[4], rows[4][::-1]])], src, dst, host=True)[0]
    assert stereo.shape == (2, len(whole[4])) and np.array_equal(_bits(stereo[0]), _bits(whole[4]))


# ------------------------------------------------------------------------------------------------------------------ the design
DESIGN_PAIRS = [(48000, 44100), (44100, 48000), (24000, 44100), (44100, 16000)]


def _interior(v):
    m = len(v)
    return v[m // 5:m - m // 5]


@pytest.mark.parametrize("pair", DESIGN_PAIRS)
def test_pass_band_is_flat_and_the_stop_band_is_down(pair):
    """on the binary64 reference, so the filter is judged and not the rounding.  Measured: pass band error <= 1.83e-4 (asserted 4e-4: a margin
    of about two for the tone phases not probed); a tone at 1.06 x the new Nyquist comes out at -53.3 dB (48k -> 44.1k) and -55.0 dB (44.1k -> 16k)"""
    src, dst = pair
    n = src // 5
    worst = 0.0
    for f in (100.0, 1000.0, 0.25 * min(src, dst), 0.4 * min(src, dst)):
        y, _, _ = R.resample64(R.tone(f, src, n), src, dst)
        e = float(np.abs(_interior(y - R.tone(f, dst, len(y)))).max())
        print(f"{src} -> {dst}: tone {f:.0f} Hz interior error {e:.3e}")
        worst = max(worst, e)
    assert worst <= 4e-4
    if dst < src:
        y, _, _ = R.resample64(R.tone(0.5 * dst * 1.06, src, n), src, dst)
        db = 20 * np.log10(float(np.abs(_interior(y)).max()) / 0.5)
        print(f"{src} -> {dst}: tone at 1.06 x new Nyquist {db:.1f} dB")
        assert db <= -50.0


def test_the_twin_resamples_a_tone_like_the_reference_design():
    """the product call end to end: a 1 kHz tone through 48k -> 44.1k is the 1 kHz tone at 44.1 kHz"""
    y = twin(R.tone(1000.0, 48000, 9600).astype(np.float32), 48000, 44100)
    assert len(y) == 8820
    assert np.abs(_interior(y - R.tone(1000.0, 44100, 8820))).max() <= 4e-4 + 1e-6


# ------------------------------------------------------------------------------------------------------------------ the deviation
def _reference_resample_frac(x, src, dst):
    """AudioSignal.ResampleFrac (AudioTools/AudioSignal.cs:962-1032) restated in binary64 torch, line for line"""
    import torch
    import torch.nn.functional as F
    g = math.gcd(src, dst)
    U, D = dst // g, src // g
    a = torch.as_tensor(x, dtype=torch.float64).reshape(1, 1, -1)
    t = torch.arange(-64, 65, dtype=torch.float64)
    if U > 1:
        up = torch.zeros((1, 1, a.shape[-1] * U), dtype=torch.float64)
        up[..., ::U] = a
        cut = 1.0 / U
        h = torch.sinc(cut * t) * cut * U * torch.hamming_window(129, dtype=torch.float64)
        h = h / h.sum()
        a = F.conv1d(F.pad(up, (128, 128), mode="reflect"), h.reshape(1, 1, -1))
    if D > 1:
        cut = 1.0 / D
        h = torch.sinc(cut * t) * cut * torch.hamming_window(129, dtype=torch.float64)
        h = h / h.sum()
        a = F.conv1d(F.pad(a, (128, 128), mode="reflect"), h.reshape(1, 1, -1))[..., ::D]
    return a.reshape(-1).numpy()


def test_the_reference_resample_frac_is_not_a_resampler():
    """the three findings of the header's deviation paragraph"""
    x48 = R.tone(1000.0, 48000, 4800, phase=0.0)
    y = _reference_resample_frac(x48, 48000, 44100)
    assert len(y) == 4412 and resample_sinc_len(4800, 48000, 44100) == 4410             # 128 samples per stage, never trimmed
    assert np.abs(y).max() < 0.01                                                       # the 129 taps see at most one non-zero sample
    assert len(_reference_resample_frac(x48, 48000, 24000)) == 2464
    x24 = R.tone(1000.0, 24000, 2400, phase=0.0)
    peak = float(np.abs(_reference_resample_frac(x24, 24000, 48000)[400:-400]).max())
    assert abs(peak - 0.25) <= 0.01                                                     # normalised after zero-stuffing: the gain U is gone
    ours = twin(x24.astype(np.float32), 24000, 48000)
    assert len(ours) == 4800 and abs(float(np.abs(ours[400:-400]).max()) - 0.5) <= 1e-3


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_and_the_calls_stay_usable():
    lib, E, i64 = _lib.lib(), _lib.NC_EINVAL, _lib.i64_array
    x = np.zeros(4096, np.float32)
    out = np.zeros(8192, np.float32)

    def call(pcm=x.ctypes.data, R_=1, off=(0,), n=(1000,), src=48000, dst=44100, cfg=None, o=out.ctypes.data, oo=(0,)):
        c = C.byref(cfg.c_struct()) if cfg is not None else None
        return lib.nc_audio_resample_sinc_host(pcm, R_, i64(off) if off is not None else None, i64(n) if n is not None else None, src, dst, c, o,
                                               i64(oo) if oo is not None else None)

    assert call() == _lib.NC_OK
    assert call(pcm=None) == E and call(o=None) == E and call(off=None) == E and call(n=None) == E and call(oo=None) == E
    assert call(src=0) == E and call(dst=0) == E and call(src=-5) == E
    assert call(R_=0) == E and call(R_=32768, off=[0] * 32768, n=[0] * 32768, oo=[0] * 32768) == E
    assert call(R_=32767, off=[0] * 32767, n=[0] * 32767, oo=[0] * 32767) == _lib.NC_OK
    assert call(n=(-1,)) == E and call(n=(2 ** 30 + 1,)) == E and call(off=(-1,)) == E and call(oo=(-1,)) == E
    assert "2^30" in lib.nc_last_error().decode() or "offset" in lib.nc_last_error().decode()
    for bad in (ResampleConfig(65, 0.945), ResampleConfig(-1, 0.945), ResampleConfig(24, 0.49), ResampleConfig(24, 1.01), ResampleConfig(24, float("nan"))):
        assert call(cfg=bad) == E
    assert call(cfg=ResampleConfig(64, 0.5)) == _lib.NC_OK and call(cfg=ResampleConfig(1, 1.0)) == _lib.NC_OK
    assert call(src=44100, dst=44101) == E and "4 MiB" in lib.nc_last_error().decode()
    assert call(src=32000, dst=44100) == _lib.NC_OK                                     # 641 KB
    # an output row over an input row, in one buffer
    both = np.zeros(4096, np.float32)
    assert call(pcm=both.ctypes.data, o=both.ctypes.data, n=(1000,), oo=(500,)) == E and "overlap" in lib.nc_last_error().decode()
    assert call(pcm=both.ctypes.data, o=both.ctypes.data, n=(1000,), oo=(999,)) == E
    assert call(pcm=both.ctypes.data, o=both.ctypes.data, n=(1000,), oo=(1000,)) == _lib.NC_OK
    assert call(pcm=both.ctypes.data, o=both.ctypes.data, n=(1000,), src=5, dst=5, oo=(0,)) == E   # the copy is held to it as well
    assert call(pcm=both.ctypes.data, o=both.ctypes.data, R_=2, off=(0, 3000), n=(1000, 1000), oo=(1000, 2082)) == E   # row 1's output reaches row 1's input
    assert call(pcm=both.ctypes.data, o=both.ctypes.data, R_=2, off=(0, 3000), n=(1000, 1000), oo=(1000, 2000)) == _lib.NC_OK
    # the handle-less queries
    assert lib.nc_audio_resample_sinc_len(-1, 48000, 44100) == -1 and lib.nc_audio_resample_sinc_len(10, 0, 44100) == -1
    assert lib.nc_audio_resample_sinc_len(2 ** 30 + 1, 48000, 44100) == -1 and lib.nc_audio_resample_sinc_len(10, 5, 5) == 10
    v = [C.c_int32() for _ in range(5)]
    assert lib.nc_audio_resample_sinc_geom(44100, 44101, None, *[C.byref(t) for t in v]) == E
    assert lib.nc_audio_resample_sinc_geom(48000, 44100, None, None, *[C.byref(t) for t in v[1:]]) == E
    assert lib.nc_audio_resample_sinc_table(48000, 44100, None, None) == E
    with pytest.raises(ValueError):
        resample_sinc_geom(48000, 1)
    with pytest.raises(ValueError):
        resample_sinc_len(-3, 48000, 44100)
    with pytest.raises(ValueError):
        RS.resample_sinc_packed(x, 48000, 44100, [5000], host=True)                     # past the end of the buffer
    # one valid call follows
    y = twin(R.signal(500, 1), 3, 2)
    assert len(y) == 334 and np.isfinite(y).all()


def test_model_classes_offer_resample_ragged_on_the_host_twin():
    """DAC / SNAC / Encodec.resample_ragged: a thin call of resample_sinc to the model's rate (host=True needs no handle's device work)"""
    from neuralcodecs_amd import DAC, SNAC, Encodec
    for cls in (DAC, SNAC, Encodec):
        assert callable(getattr(cls, "resample_ragged"))
    clips = [R.signal(n, n) for n in (480, 1000)]
    got = RS.resample_ragged(clips, 48000, 44100, host=True)
    for c, y in zip(clips, got):
        assert np.array_equal(_bits(y), _bits(twin(c, 48000, 44100)))
