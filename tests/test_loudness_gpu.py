"""GPU suite of the loudness feature: kweight_mfma_kernel, the state scan, the energy / gate kernels and the gain kernel against the serial
host twins of the library (tests/test_loudness_cpu.py holds those to binary64) -- np.array_equal everywhere, no tolerance.  Whole output
buffers are compared, NaN-filled gaps between the rows included (as bit patterns), so a store outside a row shows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import quality_ref as R  # noqa: E402
from conftest import dac_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import DAC, LoudnessConfig, _lib  # noqa: E402
from neuralcodecs_amd import loudness as L  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402

KEYS = ("lufs", "gain", "n_blocks", "n_pass_abs", "n_pass_rel", "n_bad")
RATES = [8000, 11025, 16000]
FILTERS = ["reference", "designed"]


def _geom(rate):
    block = np.float32(0.4) * np.float32(rate)
    return int(block), int(block * np.float32(0.25))


def _lengths(rate):
    """1, around the filter block of 64, around one and two gating blocks, and 5 gating blocks not a multiple of 64"""
    N, S = _geom(rate)
    five = N + 4 * S + 7
    assert five % 64 != 0
    return [1, 63, 64, 65, N - 1, N, N + S - 1, N + S, five]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_buffers(got, want):
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _same_rows(got, want):
    for k in KEYS:
        assert np.array_equal(_bits(got[k]) if got[k].dtype == np.float32 else got[k], _bits(want[k]) if want[k].dtype == np.float32 else want[k]), k


def _clips_packed(lens, chans, rate, seed, level=None):
    """(buffer, offsets [B C], lengths) with ODD element offsets and gaps of NaN between the rows"""
    offs, o = [], 1
    for n in lens:
        for _ in range(chans):
            offs.append(o)
            o += n + (2 if (o + n) % 2 else 3)
    buf = np.full(o, np.nan, np.float32)
    for i, at in enumerate(offs):
        n = lens[i // chans]
        amp = (level or (lambda b: 0.5 / (1 + b % 4)))(i // chans)
        buf[at:at + n] = np.float32(amp) * R.signal(n, rate, seed + i)
    assert all(v % 2 == 1 for v in offs)
    return buf, offs


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("rate", RATES)
def test_kweight_equals_the_host_twin(rate, filt):
    lens = _lengths(rate)
    buf, offs = _clips_packed(lens, 1, rate, rate)
    canvas = np.full(buf.size + 5, np.nan, np.float32)
    oo = [o + 4 for o in offs]                                   # odd + 4: still odd, another alignment than the input's
    want, _ = L.kweight_packed(buf, rate, filt, lens, offs, oo, out=canvas.copy(), host=True)
    import torch
    out_dev = torch.from_numpy(canvas.copy()).cuda()
    got, _ = L.kweight_packed(torch.from_numpy(buf).cuda(), rate, filt, lens, offs, oo, out=out_dev)
    assert np.isfinite(np.concatenate([want[o:o + n] for o, n in zip(oo, lens)])).all()
    assert np.isnan(want).sum() == canvas.size - sum(lens)
    _same_buffers(got.cpu().numpy(), want)


def test_kweight_long_row_equals_the_host_twin():
    """one 44.1 kHz second: 690 blocks, eleven workgroups of one row, the last of them partly filled"""
    x = np.float32(0.3) * R.signal(44100, 44100, 5)
    (a,), (b,) = L.kweight([x], 44100), L.kweight([x], 44100, host=True)
    _same_buffers(a, b)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("chans", [1, 2, 5])
@pytest.mark.parametrize("rate", RATES)
def test_loudness_equals_the_host_twin(rate, chans, filt):
    lens = _lengths(rate) if chans == 1 else _lengths(rate)[4:]
    buf, offs = _clips_packed(lens, chans, rate, 3 * rate + chans)
    cfg = LoudnessConfig(filt, -23.0)
    want = L.loudness_packed(buf, rate, lens, offs, chans, cfg, host=True)
    got = L.loudness_packed(buf, rate, lens, offs, chans, cfg)
    N, S = _geom(rate)
    assert want["n_blocks"].tolist() == [(n - N) // S + 1 if n >= N else 0 for n in lens]
    assert (want["lufs"][want["n_blocks"] > 0] > -70).all() and (want["lufs"][want["n_blocks"] == 0] == -70).all()
    _same_rows(got, want)


def test_loudness_one_second_at_44100_and_single_clip():
    x = np.float32(0.2) * R.signal(44100, 44100, 9)
    _same_rows(L.loudness([x], 44100), L.loudness([x], 44100, host=True))                       # B = 1
    st = np.stack([x, np.float32(0.5) * x[::-1]])
    _same_rows(L.loudness([st], 44100), L.loudness([st], 44100, host=True))


def _mixed_batch(rate=8000):
    """B = 7: lengths of every kind, a quiet tail (relative gate), a stretch of zeros (absolute gate), an all-zero clip and one with a NaN"""
    N, S = _geom(rate)
    lens = [N + 6 * S + 3, 63, N, 2 * N + 11, N + 9 * S, N + 2 * S, N + 3 * S + 1]
    clips = [np.float32(0.4 / (1 + i % 3)) * R.signal(n, rate, 40 + i) for i, n in enumerate(lens)]
    clips[0][lens[0] // 2:] *= np.float32(10 ** (-30 / 20))
    clips[4][3 * S:8 * S] = 0.0
    clips[5][:] = 0.0
    clips[6][17] = np.nan
    return clips, rate


def test_gates_silence_and_bad_samples_equal_the_host_twin():
    clips, rate = _mixed_batch()
    want, got = L.loudness(clips, rate, host=True), L.loudness(clips, rate)
    assert want["n_pass_rel"][0] < want["n_pass_abs"][0] == want["n_blocks"][0]
    assert want["n_pass_abs"][4] < want["n_blocks"][4]
    assert want["lufs"][5] == -70 and np.isfinite(want["gain"][5]) and want["n_pass_abs"][5] == 0
    assert np.isnan(want["lufs"][6]) and np.isnan(want["gain"][6]) and want["n_bad"][6] == 1 and want["n_bad"][:6].sum() == 0
    _same_rows(got, want)


def test_batch_independence_permutation_and_repetition():
    clips, rate = _mixed_batch()
    whole = L.loudness(clips, rate)
    again = L.loudness(clips, rate)
    _same_rows(again, whole)
    perm = [3, 6, 0, 5, 1, 4, 2]
    shuffled = L.loudness([clips[i] for i in perm], rate)
    for at, i in enumerate(perm):
        alone = L.loudness([clips[i]], rate)
        for k in KEYS:
            a, b, c = np.atleast_1d(alone[k])[:1], np.atleast_1d(whole[k])[i:i + 1], np.atleast_1d(shuffled[k])[at:at + 1]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(c.view(np.uint32), b.view(np.uint32)), (k, i)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("chans", [1, 2])
def test_normalize_equals_the_host_twin_also_in_place(chans, filt):
    import torch
    rate = 11025
    lens = _lengths(rate)[2:]
    buf, offs = _clips_packed(lens, chans, rate, 71 + chans)
    cfg = LoudnessConfig(filt, -16.0)
    canvas = np.full(buf.size + 8, np.nan, np.float32)
    oo = [o + 3 for o in offs]                                   # even offsets out, odd in: the scalar path
    want, _, wrows = L.normalize_loudness_packed(buf, rate, lens, offs, chans, cfg, out_offsets=oo, out=canvas.copy(), host=True)
    got, _, grows = L.normalize_loudness_packed(torch.from_numpy(buf).cuda(), rate, lens, offs, chans, cfg, out_offsets=oo,
                                                out=torch.from_numpy(canvas.copy()).cuda())
    _same_buffers(got.cpu().numpy(), want)
    _same_rows({k: grows[k].cpu().numpy() for k in KEYS}, wrows)
    hbuf, dbuf = buf.copy(), torch.from_numpy(buf.copy()).cuda()
    _, _, wrows2 = L.normalize_loudness_packed(hbuf, rate, lens, offs, chans, cfg, in_place=True, host=True)
    _, _, grows2 = L.normalize_loudness_packed(dbuf, rate, lens, offs, chans, cfg, in_place=True)
    _same_buffers(dbuf.cpu().numpy(), hbuf)
    _same_rows({k: grows2[k].cpu().numpy() for k in KEYS}, wrows)
    _same_rows(wrows2, wrows)
    assert not np.array_equal(_bits(hbuf), _bits(buf))


def test_normalize_and_gain_on_aligned_rows_take_the_vector_path():
    """rows at multiples of four elements, lengths with every tail 0..3: the 16-byte path and its scalar tail; a NaN clip becomes quiet NaN"""
    rate = 8000
    clips, _ = _mixed_batch(rate)
    clips = [np.ascontiguousarray(c[:len(c) - i % 4]) for i, c in enumerate(clips)]
    lens = [len(c) for c in clips]
    offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 + 4 for n in lens])[:-1]]).tolist()
    buf = np.full(offs[-1] + lens[-1] + 5, np.nan, np.float32)
    for c, o in zip(clips, offs):
        buf[o:o + len(c)] = c
    cfg = LoudnessConfig("reference", -20.0)
    want, _, wrows = L.normalize_loudness_packed(buf.copy(), rate, lens, offs, 1, cfg, in_place=True, host=True)
    import torch
    dbuf = torch.from_numpy(buf.copy()).cuda()
    L.normalize_loudness_packed(dbuf, rate, lens, offs, 1, cfg, in_place=True)
    _same_buffers(dbuf.cpu().numpy(), want)
    assert (_bits(want[offs[6]:offs[6] + lens[6]]) == 0x7fc00000).all()
    db = np.linspace(-9.0, 7.5, len(lens)).astype(np.float32)
    clean = np.where(np.isnan(buf), np.float32(0.25), buf)
    w2, _ = L.apply_gain_db_packed(clean.copy(), db, lens, offs, 1, in_place=True, host=True)
    d2 = torch.from_numpy(clean.copy()).cuda()
    L.apply_gain_db_packed(d2, db, lens, offs, 1, in_place=True)
    _same_buffers(d2.cpu().numpy(), w2)


@pytest.mark.parametrize("chans", [1, 5])
def test_apply_gain_db_equals_the_host_twin(chans):
    rate = 16000
    lens = [1, 2, 3, 4, 5, 63, 1025, 4099]
    buf, offs = _clips_packed(lens, chans, rate, 500 + chans)
    db = np.linspace(-30.0, 12.0, len(lens)).astype(np.float32)
    canvas = np.full(buf.size + 6, np.nan, np.float32)
    oo = [o + 5 for o in offs]
    want, _ = L.apply_gain_db_packed(buf, db, lens, offs, chans, out_offsets=oo, out=canvas.copy(), host=True)
    import torch
    got, _ = L.apply_gain_db_packed(torch.from_numpy(buf).cuda(), db, lens, offs, chans, out_offsets=oo, out=torch.from_numpy(canvas.copy()).cuda())
    _same_buffers(got.cpu().numpy(), want)
    assert np.isnan(want).sum() == canvas.size - chans * sum(lens)


def test_host_buffer_calls_equal_the_twin():
    """the plain (synchronous, HOST buffer) exports"""
    lib = _lib.lib()
    rate, chans = 8000, 2
    lens = [3300, 5000]
    buf, offs = _clips_packed(lens, chans, rate, 900)
    i64 = _lib.i64_array
    cfg = LoudnessConfig("designed", -18.0)
    c = cfg.c_struct()
    want_out, _, want_rows = L.normalize_loudness_packed(buf, rate, lens, offs, chans, cfg, out=np.full(buf.size, np.nan, np.float32), host=True)
    out = np.full(buf.size, np.nan, np.float32)
    words = np.zeros((2, L.ROW_WORDS), np.int32)
    assert lib.nc_loudness_normalize(0, buf.ctypes.data, 2, chans, i64(offs), i64(lens), rate, C.byref(c), out.ctypes.data, i64(offs), words.ctypes.data) == _lib.NC_OK
    _same_buffers(out, want_out)
    _same_rows(L._unpack_rows(words, False), want_rows)
    words2 = np.zeros((2, L.ROW_WORDS), np.int32)
    assert lib.nc_loudness(0, buf.ctypes.data, 2, chans, i64(offs), i64(lens), rate, C.byref(c), words2.ctypes.data) == _lib.NC_OK
    assert np.array_equal(words2, words)
    rows = chans * len(lens)
    row_lens = [lens[i // chans] for i in range(rows)]
    kw = np.full(buf.size, np.nan, np.float32)
    assert lib.nc_audio_kweight(0, buf.ctypes.data, rows, i64(offs), i64(row_lens), rate, 1, kw.ctypes.data, i64(offs)) == _lib.NC_OK
    want_kw, _ = L.kweight_packed(buf, rate, "designed", row_lens, offs, out=np.full(buf.size, np.nan, np.float32), host=True)
    _same_buffers(kw, want_kw)
    db = np.array([-3.0, 4.5], np.float32)
    g = np.full(buf.size, np.nan, np.float32)
    assert lib.nc_audio_apply_gain_db(0, buf.ctypes.data, 2, chans, i64(offs), i64(lens), db.ctypes.data, g.ctypes.data, i64(offs)) == _lib.NC_OK
    want_g, _ = L.apply_gain_db_packed(buf, db, lens, offs, chans, out=np.full(buf.size, np.nan, np.float32), host=True)
    _same_buffers(g, want_g)


def test_calls_on_two_streams_share_the_workspace_in_order():
    """the per-device workspace and pinned row table across streams: two calls on a side stream (the second uploads a table of the
    other filter kind while that stream is current), then, with no host synchronisation, a call on the default stream behind them"""
    import torch
    rate = 44100
    rows = [np.float32(0.3) * R.signal(n, rate, 60 + n) for n in (5000, 147, 2353)]
    cfg = LoudnessConfig("designed", -20.0)
    want = L.kweight(rows, rate, "reference", host=True)
    want_lev, want_rows = L.normalize_loudness(rows, rate, cfg, host=True)
    dev = [torch.from_numpy(r).cuda() for r in rows]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = L.kweight(dev, rate, "reference")
        lev, lrows = L.normalize_loudness(dev, rate, cfg)
    again = L.kweight(dev, rate, "reference")                                      # the default stream, behind the calls on `side`
    torch.cuda.synchronize()
    assert all(g.is_cuda and g.dtype == torch.float32 for g in got + lev + again)
    for g, a, w in zip(got, again, want):
        _same_buffers(g.cpu().numpy(), w)
        _same_buffers(a.cpu().numpy(), w)
    for g, w in zip(lev, want_lev):
        _same_buffers(g.cpu().numpy(), w)
    _same_rows({k: lrows[k].cpu().numpy() for k in KEYS}, want_rows)


def test_refusals_leave_the_device_usable():
    import torch
    lib = _lib.lib()
    x = torch.zeros(4000, dtype=torch.float32, device="cuda")
    out = torch.zeros(4000, dtype=torch.float32, device="cuda")
    rows = torch.zeros((2, L.ROW_WORDS), dtype=torch.int32, device="cuda")
    i64, E = _lib.i64_array, _lib.NC_EINVAL
    good = LoudnessConfig().c_struct()

    def loud(pcm=x.data_ptr(), B=1, Cn=1, off=(0,), n=(3000,), rate=8000, cfg=good, o=rows.data_ptr()):
        return lib.nc_loudness_dev(0, pcm, B, Cn, i64(off), i64(n), rate, C.byref(cfg) if cfg is not None else None, o, None)

    bad_filter, bad_target = LoudnessConfig().c_struct(), LoudnessConfig().c_struct()
    bad_filter.filter, bad_target.target_db = 7, float("inf")
    assert loud(pcm=None) == E and loud(o=None) == E and loud(cfg=None) == E and loud(B=0) == E and loud(Cn=0) == E and loud(Cn=6) == E
    assert loud(off=(-1,)) == E and loud(n=(-1,)) == E and loud(rate=9) == E and loud(cfg=bad_filter) == E and loud(cfg=bad_target) == E
    assert lib.nc_audio_kweight_dev(0, x.data_ptr(), 1, i64([0]), i64([100]), 8000, 5, out.data_ptr(), i64([0]), None) == E
    db = np.array([np.nan], np.float32)
    assert lib.nc_audio_apply_gain_db_dev(0, x.data_ptr(), 1, 1, i64([0]), i64([100]), db.ctypes.data, out.data_ptr(), i64([0]), None) == E
    torch.cuda.synchronize()
    sig = np.float32(0.3) * R.signal(5000, 8000, 3)
    _same_rows(L.loudness([sig], 8000), L.loudness([sig], 8000, host=True))            # one valid call follows


def test_dac_normalize_encode_decode_restore_equals_the_twin_levels():
    g = load_golden("dac_small")
    cfg = dac_cfg_from_meta(g["meta"])
    with DAC(cfg, device_index=0) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"])))
        lens = [7000, 9100, 6503]
        clips = [np.float32(0.3 + 0.2 * i) * synthetic_pcm(1, 1, T, cfg.sample_rate, seed=300 + i)[0, 0] for i, T in enumerate(lens)]
        lev, rows = m.normalize_ragged(clips, -20.0)
        dec = m.decode_codes_ragged(m.encode_ragged(lev))
        back = m.restore_ragged([np.ascontiguousarray(d.reshape(-1)) for d in dec], rows)
        lev_h, rows_h = m.normalize_ragged(clips, -20.0, host=True)
        _same_rows(rows, rows_h)
        for a, b in zip(lev, lev_h):
            _same_buffers(a, b)
        dec_h = m.decode_codes_ragged(m.encode_ragged(lev_h))
        back_h = m.restore_ragged([np.ascontiguousarray(d.reshape(-1)) for d in dec_h], rows_h, host=True)
        assert len(back) == len(clips)
        for a, b in zip(back, back_h):
            _same_buffers(a, b)
