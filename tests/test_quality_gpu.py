"""GPU suite of the round-trip quality feature: stft_mfma_kernel, mel_apply_kernel and the metric kernels against the serial host twins of
the library (tests/test_quality_cpu.py holds those to binary64 and to the reference) -- np.array_equal everywhere, no tolerance.  Whole
output buffers are compared, gaps between the rows included, so a store outside a row shows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import quality_ref as R  # noqa: E402
from conftest import dac_cfg_from_meta, encodec_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import DAC, Encodec, QualityConfig, _lib, mel_filterbank, quality  # noqa: E402
from neuralcodecs_amd.quality import mel_spectrogram_packed, quality_metrics, stft, stft_packed  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, encodec_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402

SR = 44100
KEYS = ("l1", "si_sdr_db", "mel_distance", "mel_log", "mel_mag", "n_bad")
WH = [(32, 8), (64, 16), (64, 64), (512, 128), (2048, 512)]


def _row_sets(W, H):
    """two packed batches of 3 rows: the minimum W/2 + 1, H k - 1, H k, H k + 1 and two long rows; ODD element offsets"""
    k = W // (2 * H) + 3
    return [[W // 2 + 1, H * k - 1, 6000], [H * k, H * k + 1, 5999]]


def _packed(lens, seed):
    """(buffer, odd offsets) with gaps of NaN between the rows: a read outside a row poisons the result"""
    offs, o = [], 1
    for n in lens:
        offs.append(o)
        o += n + (2 if (o + n) % 2 else 3)      # keeps the next offset odd
    buf = np.full(o, np.nan, np.float32)
    for i, (n, at) in enumerate(zip(lens, offs)):
        buf[at:at + n] = R.signal(n, SR, seed + i)
    assert all(v % 2 == 1 for v in offs)
    return buf, offs


def _odd_out_offsets(sizes):
    offs, o = [], 3
    for s in sizes:
        offs.append(o)
        o += s + (2 if (o + s) % 2 else 1)
    return offs


@pytest.mark.parametrize("W,H", WH)
def test_stft_equals_the_host_twin(W, H):
    for s, lens in enumerate(_row_sets(W, H)):
        buf, offs = _packed(lens, 10 * s + W)
        oo = _odd_out_offsets([(W // 2 + 1) * (1 + n // H) for n in lens])
        assert all(v % 2 == 1 for v in oo)
        want, _, shapes = stft_packed(buf, W, H, lengths=lens, offsets=offs, out_offsets=oo, host=True)
        got, _, _ = stft_packed(buf, W, H, lengths=lens, offsets=offs, out_offsets=oo)
        assert shapes == [(W // 2 + 1, 1 + n // H) for n in lens]
        assert np.isfinite(want).all() and np.array_equal(got, want)


@pytest.mark.parametrize("window", ["ones"])
def test_stft_rectangular_window_equals_the_host_twin(window):
    x = R.signal(1000, SR, 77)
    (a,), (b,) = stft(x, 128, 32, window=window), stft(x, 128, 32, window=window, host=True)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("W,M", [(512, 5), (512, 80), (2048, 150), (2048, 320), (32, 5)])
def test_mel_spectrogram_equals_the_host_twin(W, M):
    H = W // 4
    if (W, M) == (512, 80):
        _, lo, hi = mel_filterbank(SR, M, W)
        assert (hi - lo == 0).any()            # the lowest bands have no bin: they must come out 0, not stale
    for s, lens in enumerate(_row_sets(W, H)):
        buf, offs = _packed(lens, 20 * s + W + M)
        oo = _odd_out_offsets([M * (1 + n // H) for n in lens])
        want, _, _ = mel_spectrogram_packed(buf, SR, W, H, M, lengths=lens, offsets=offs, out_offsets=oo, host=True)
        got, _, _ = mel_spectrogram_packed(buf, SR, W, H, M, lengths=lens, offsets=offs, out_offsets=oo)
        assert np.isfinite(want).all() and np.array_equal(got, want)


def _rows(lens, seed, snr=(8.0, 15.0, 25.0, 40.0)):
    ref = [R.signal(n, SR, seed + i) for i, n in enumerate(lens)]
    return ref, [R.degraded(r, seed + 50 + i, snr[i % 4]) for i, r in enumerate(ref)]


def _same(a, b, rows_a=None, rows_b=None):
    for k in KEYS:
        x = a[k] if rows_a is None else a[k][rows_a]
        y = b[k] if rows_b is None else b[k][rows_b]
        assert np.array_equal(x, y, equal_nan=True), (k, x, y)


def test_each_row_alone_any_order_and_twice_give_the_same_bits():
    cfg = QualityConfig([64, 512], [5, 80])
    ref, est = _rows([3000, 4111, 777, 6000], 300)
    both = quality_metrics(ref, est, sample_rate=SR, scales=cfg)
    _same(both, quality_metrics(ref, est, sample_rate=SR, scales=cfg))
    perm = [2, 0, 3, 1]
    shuffled = quality_metrics([ref[i] for i in perm], [est[i] for i in perm], sample_rate=SR, scales=cfg)
    _same(shuffled, both, None, perm)
    for b in range(4):
        one = quality_metrics(ref[b:b + 1], est[b:b + 1], sample_rate=SR, scales=cfg)
        _same(one, both, [0], [b])
    lens = [600, 257]
    buf, offs = _packed(lens, 5)
    a, _, _ = stft_packed(buf, 256, 64, lengths=lens, offsets=offs)
    b0, _, _ = stft_packed(buf, 256, 64, lengths=lens[1:], offsets=offs[1:])
    n1 = 129 * (1 + 257 // 64)
    assert np.array_equal(a[-2 * n1:], b0)


@pytest.mark.parametrize("name", ["dac_eval", "reference_default"])
def test_quality_metrics_equal_the_host_twin_numpy_and_torch(name):
    import torch
    cfg = getattr(QualityConfig, name)()
    ref, est = _rows([3000, 9000, 5001, 7000], 400)
    want = quality_metrics(ref, est, sample_rate=SR, scales=cfg, host=True)
    assert np.isfinite(want["mel_distance"]).all() and (want["si_sdr_db"] > 0).all()
    got = quality_metrics(ref, est, sample_rate=SR, scales=cfg)
    _same(got, want)
    tg = quality_metrics([torch.from_numpy(r).cuda() for r in ref], [torch.from_numpy(e).cuda() for e in est], sample_rate=SR, scales=cfg)
    assert all(v.is_cuda for v in tg.values())
    _same({k: v.cpu().numpy() for k, v in tg.items()}, want)
    # a NaN sample in row 1: a NaN row with the count; the neighbours equal the batch without it
    bad = [e.copy() for e in est]
    bad[1][1234] = np.nan
    gb = quality_metrics(ref, bad, sample_rate=SR, scales=cfg)
    _same(gb, quality_metrics(ref, bad, sample_rate=SR, scales=cfg, host=True))
    assert gb["n_bad"].tolist() == [0, 1, 0, 0] and np.isnan(gb["si_sdr_db"][1]) and np.isnan(gb["mel_log"][1]).all()
    _same(gb, got, [0, 2, 3], [0, 2, 3])


def test_dac_ragged_round_trip_is_compared_in_place():
    """dac_small: encode_ragged -> decode_codes_ragged on 3 clips of unequal lengths, metrics through the two offset tables (ref_off from
    the lengths, est_off from the decoded lengths) on the packed device buffers; they equal the twin on the downloaded waveforms.
    (On this fixture's synthetic weights fewer codebooks do not order si_sdr_db -- checked on the CPU oracle: 3 clips, 4 / 2 / 1
    codebooks, the third clip's si_sdr_db rises -- so no ordering is asserted.)"""
    import torch
    g = load_golden("dac_small")
    cfg = dac_cfg_from_meta(g["meta"])
    m = DAC(cfg)
    m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"])))
    lens = [3000, 4111, 5200]
    clips = [torch.from_numpy(synthetic_pcm(1, 1, t, cfg.sample_rate, seed=60 + i)[0, 0]).cuda() for i, t in enumerate(lens)]
    scales = QualityConfig([512, 64], [40, 5])
    for nq in (cfg.n_codebooks, 2):
        dec = m.decode_codes_ragged(m.encode_ragged(clips, nq))
        dlens = [int(d.shape[0]) for d in dec]
        assert all(d >= n for d, n in zip(dlens, lens))
        packed_ref = torch.cat(clips)
        packed_est = dec[0]._base                    # the packed output of the ragged decode: the clips are views of it
        assert packed_est is not None and packed_est.numel() >= sum(dlens) and dec[0].data_ptr() == packed_est.data_ptr()
        ref_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
        est_off = np.concatenate([[0], np.cumsum(dlens)[:-1]]).tolist()
        got = quality_metrics(packed_ref, packed_est, lengths=lens, sample_rate=cfg.sample_rate, scales=scales, ref_offsets=ref_off, est_offsets=est_off)
        want = quality_metrics([c.cpu().numpy() for c in clips], [d.cpu().numpy()[:n] for d, n in zip(dec, lens)], sample_rate=cfg.sample_rate,
                               scales=scales, host=True)
        _same({k: v.cpu().numpy() for k, v in got.items()}, want)
        if nq == cfg.n_codebooks:
            rt = m.round_trip_quality(clips, scales=scales)
            _same({k: v.cpu().numpy() for k, v in rt.items()}, want)
    m.dispose()


def test_encodec_round_trip_quality_stereo_rows():
    g = load_golden("encodec_small48")
    cfg = encodec_cfg_from_meta(g["meta"])
    m = Encodec(cfg)
    m.load_blob(save_blob(encodec_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"])))
    lens = [4000, 8100, 5000]
    clips = [synthetic_pcm(1, cfg.channels, T, cfg.sampling_rate, seed=900 + i)[0] for i, T in enumerate(lens)]
    scales = QualityConfig([512, 64], [40, 5])
    got = m.round_trip_quality(clips, scales=scales)
    dec = m.decode_ragged(m.encode_ragged(clips), lens)
    ref_rows, est_rows = quality.round_trip_rows(clips, dec)
    assert len(ref_rows) == cfg.channels * len(clips) == got["l1"].shape[0] and cfg.channels == 2
    want = quality_metrics([np.ascontiguousarray(r) for r in ref_rows], [np.ascontiguousarray(e) for e in est_rows], sample_rate=cfg.sampling_rate,
                           scales=scales, host=True)
    _same(got, want)
    m.dispose()


def test_calls_on_two_streams_share_the_workspace_in_order():
    """the per-device workspace and pinned row table across streams: an STFT and a mel spectrogram on a side stream (the second uploads
    a new basis and filterbank while that stream is current), then, with no host synchronisation, the STFT on the default stream"""
    import torch
    W, H = WH[0]
    lens = [5000, 147, 2353]
    buf = np.concatenate([R.signal(n, SR, 60 + n) for n in lens])
    want, _, _ = stft_packed(buf, W, H, lengths=lens, host=True)
    want_mel, _, _ = mel_spectrogram_packed(buf, SR, 128, 32, 20, lengths=lens, host=True)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, _, _ = stft_packed(dev, W, H, lengths=lens)
        mel, _, _ = mel_spectrogram_packed(dev, SR, 128, 32, 20, lengths=lens)
    again, _, _ = stft_packed(dev, W, H, lengths=lens)                              # the default stream, behind the calls on `side`
    torch.cuda.synchronize()
    assert got.is_cuda and mel.is_cuda and again.is_cuda
    assert np.isfinite(want).all() and np.array_equal(got.cpu().numpy(), want) and np.array_equal(again.cpu().numpy(), want)
    assert np.isfinite(want_mel).all() and np.array_equal(mel.cpu().numpy(), want_mel)


def test_refusals_leave_the_device_usable():
    import torch
    L = _lib.lib()
    x = torch.zeros(400, dtype=torch.float32, device="cuda")
    out = torch.zeros(8192, dtype=torch.float32, device="cuda")
    rows = torch.zeros((1, quality.ROW_WORDS), dtype=torch.int32, device="cuda")
    i64 = _lib.i64_array
    px, po, pr = x.data_ptr(), out.data_ptr(), rows.data_ptr()
    E = _lib.NC_EINVAL

    def stft_status(pcm=px, B=1, n=200, W=64, H=16, window=0, o=po):
        return L.nc_audio_stft_dev(0, pcm, B, i64([0]), i64([n]), W, H, window, o, i64([0]), None)

    def mel_status(n=200, W=64, M=5, fmin=0.0, fmax=0.0, B=1):
        return L.nc_audio_mel_spectrogram_dev(0, px, B, i64([0]), i64([n]), SR, W, 16, M, fmin, fmax, po, i64([0]), None)

    def met_status(cfg, ref=px, est=px, n=200, B=1, o=pr):
        return L.nc_quality_metrics_dev(0, ref, i64([0]), est, i64([0]), i64([n]), B, SR, C.byref(cfg) if cfg is not None else None, o, None)

    def cfg(W=64, M=5, fmin=0.0, fmax=0.0):
        return QualityConfig([W], [M], fmin=[fmin], fmax=[fmax]).c_struct()

    assert stft_status(n=32) == E and mel_status(n=32) == E and met_status(cfg(), n=32) == E
    for W in (16, 48, 4096):
        assert stft_status(W=W) == E and mel_status(W=W) == E and met_status(cfg(W=W)) == E
    for M in (0, 513):
        assert mel_status(M=M) == E and met_status(cfg(M=M)) == E
    assert mel_status(fmin=100.0, fmax=100.0) == E and met_status(cfg(fmin=100.0, fmax=50.0)) == E
    assert stft_status(B=0) == E and mel_status(B=0) == E and met_status(cfg(), B=0) == E
    assert stft_status(pcm=None) == E and stft_status(o=None) == E and met_status(None) == E
    assert met_status(cfg(), ref=None) == E and met_status(cfg(), est=None) == E and met_status(cfg(), o=None) == E
    assert stft_status(H=0) == E and stft_status(window=7) == E
    torch.cuda.synchronize()
    sig = R.signal(2000, SR, 8)
    (a,), (b,) = stft(sig, 64, 16), stft(sig, 64, 16, host=True)          # one valid call follows
    assert np.array_equal(a, b)
    ok = quality_metrics([sig], [R.degraded(sig, 1)], sample_rate=SR, scales=QualityConfig([64], [5]))
    _same(ok, quality_metrics([sig], [R.degraded(sig, 1)], sample_rate=SR, scales=QualityConfig([64], [5]), host=True))
    n = i64([2000])
    hrows = np.zeros((1, quality.ROW_WORDS), np.int32)
    c = QualityConfig([64], [5]).c_struct()
    est = R.degraded(sig, 1)
    assert L.nc_quality_metrics(0, sig.ctypes.data, i64([0]), est.ctypes.data, i64([0]), n, 1, SR, C.byref(c), hrows.ctypes.data) == _lib.NC_OK
    assert hrows.view(np.float32)[0, 1] == ok["si_sdr_db"][0]
