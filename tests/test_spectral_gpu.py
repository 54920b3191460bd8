"""GPU suite of the inverse STFT, the spectral masks and the MFCC: istft_mfma_kernel + istft_gather_kernel, spec_fill_kernel and
mfcc_kernel against the serial host twins of the library (tests/test_spectral_cpu.py holds those to binary64) -- np.array_equal on bit
patterns of whole buffers, no tolerance.  Spectrogram rows sit at odd element offsets with NaN-filled gaps, output rows in a NaN-filled
canvas, so a read or a store outside a row shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import spectral_ref as R  # noqa: E402
from neuralcodecs_amd import spectral as S  # noqa: E402
from neuralcodecs_amd.quality import stft_packed  # noqa: E402

FRAMES = [1, 15, 16, 17, 33]   # the 16-frame tile edge
QNAN = 0x7fc00000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_buffers(got, want):
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _length(kind, F, W, H):
    """0 (the default), one short of the default, H frames - 1, and three past the covered span"""
    return [0, max(H * (F - 1) - 1, 0), H * F - 1, W + H * (F - 1) - W // 2 + 3][kind]


def _rows(W, H, shift=0):
    """every frame count with every length rule: 20 ragged rows"""
    fr = [F for F in FRAMES for _ in range(4)]
    want = [_length((i + shift) % 4, F, W, H) for i, F in enumerate(fr)]
    return fr, want


def _run(buf, so, fr, want, W, H, window, host, stream=None):
    import torch
    olens = [n if n else R.default_len(F, H) for n, F in zip(want, fr)]
    canvas, oo = R.out_canvas(olens)
    if host:
        out, _, ol = S.istft_packed(buf, W, H, window, fr, so, want, oo, out=canvas, host=True)
        assert ol == olens
        return out, oo, olens
    dev = torch.from_numpy(canvas).cuda()
    spec = torch.from_numpy(buf).cuda()
    if stream is None:
        out, _, ol = S.istft_packed(spec, W, H, window, fr, so, want, oo, out=dev)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out, _, ol = S.istft_packed(spec, W, H, window, fr, so, want, oo, out=dev)
        stream.synchronize()
    assert ol == olens
    return out.cpu().numpy(), oo, olens


CASES = [(W, "hann", H) for W in (32, 64) for H in (1, 5, W // 4, W // 2)] + [(W, "ones", H) for W in (32, 64) for H in (5, W // 4, W)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"W{c[0]}-{c[1]}-H{c[2]}")
def test_istft_equals_the_host_twin(case):
    W, window, H = case
    fr, want_len = _rows(W, H)
    buf, so = R.ragged_spectra(W, fr, 1000 * W + H)
    want, oo, olens = _run(buf, so, fr, want_len, W, H, window, True)
    got, _, _ = _run(buf, so, fr, want_len, W, H, window, False)
    rows = np.concatenate([want[o:o + n] for o, n in zip(oo, olens)])
    assert np.isfinite(rows).all() and np.isnan(want).sum() == want.size - sum(olens)
    tail = [want[o + W + H * (F - 1) - W // 2:o + n] for o, n, F in zip(oo, olens, fr)]
    assert all((t == 0).all() for t in tail) and sum(t.size for t in tail) >= 3 * 5     # the rows three past the covered span end in zeros
    _same_buffers(got, want)


def test_istft_large_basis_one_row():
    W, H, fr = 2048, 512, [3]
    buf, so = R.ragged_spectra(W, fr, 7)
    want, _, _ = _run(buf, so, fr, [0], W, H, "hann", True)
    got, _, _ = _run(buf, so, fr, [0], W, H, "hann", False)
    _same_buffers(got, want)


def test_rows_alone_permuted_and_repeated_give_the_same_bits():
    W, H = 32, 8
    fr, want_len = _rows(W, H, shift=1)
    buf, so = R.ragged_spectra(W, fr, 31)
    got, oo, olens = _run(buf, so, fr, want_len, W, H, "hann", False)
    again, _, _ = _run(buf, so, fr, want_len, W, H, "hann", False)
    _same_buffers(again, got)
    perm = np.random.default_rng(5).permutation(len(fr))
    pfr, pso, pwl = [fr[i] for i in perm], [so[i] for i in perm], [want_len[i] for i in perm]
    pgot, poo, polens = _run(buf, pso, pfr, pwl, W, H, "hann", False)
    for j, i in enumerate(perm):
        assert np.array_equal(_bits(pgot[poo[j]:poo[j] + polens[j]]), _bits(got[oo[i]:oo[i] + olens[i]]))
    for i in (0, 7, 19):
        one, ooo, ol = _run(buf, [so[i]], [fr[i]], [want_len[i]], W, H, "hann", False)
        assert np.array_equal(_bits(one[ooo[0]:ooo[0] + ol[0]]), _bits(got[oo[i]:oo[i] + olens[i]]))


def test_a_call_on_a_second_stream_after_one_on_the_first():
    import torch
    W, H = 64, 16
    fr, want_len = _rows(W, H)
    buf, so = R.ragged_spectra(W, fr, 77)
    want, _, _ = _run(buf, so, fr, want_len, W, H, "hann", True)
    first, _, _ = _run(buf, so, fr, want_len, W, H, "hann", False)
    second, _, _ = _run(buf, so, fr, want_len, W, H, "hann", False, stream=torch.cuda.Stream())
    _same_buffers(first, want)
    _same_buffers(second, want)


def test_row_groups_under_a_small_cap_change_no_bit():
    W, H = 32, 8
    fr, want_len = _rows(W, H, shift=2)
    buf, so = R.ragged_spectra(W, fr, 91)
    whole, _, _ = _run(buf, so, fr, want_len, W, H, "hann", False)
    default = S.istft_workspace()
    try:
        cap = 4 * W * 40   # the scratch of 40 frames: 33-frame rows alone, the short rows a few at a time
        assert S.istft_workspace(cap) == cap and 4 * W * sum(fr) > 5 * cap
        grouped, _, _ = _run(buf, so, fr, want_len, W, H, "hann", False)
    finally:
        assert S.istft_workspace(-1) == default
    _same_buffers(grouped, whole)


def test_a_nan_and_an_inf_bin_poison_exactly_the_covered_samples_of_their_row():
    W, H, K = 32, 8, 17
    fr, want_len = [17, 33, 16, 17, 15], [0, 0, 0, 0, 0]
    buf, so = R.ragged_spectra(W, fr, 55)
    clean, oo, olens = _run(buf, so, fr, want_len, W, H, "hann", False)
    bad = buf.copy()
    bad[2 * (so[1] + 3 * fr[1] + 9)] = np.nan          # row 1: bin 3 of frame 9, re
    bad[2 * (so[3] + 16 * fr[3] + 12) + 1] = np.inf    # row 3: the IGNORED imaginary part of bin W/2, frame 12: 0 x inf is still a NaN
    want, _, _ = _run(bad, so, fr, want_len, W, H, "hann", True)
    got, _, _ = _run(bad, so, fr, want_len, W, H, "hann", False)
    _same_buffers(got, want)
    for b in range(5):
        row, ref = got[oo[b]:oo[b] + olens[b]], clean[oo[b]:oo[b] + olens[b]]
        if b not in (1, 3):
            assert np.array_equal(_bits(row), _bits(ref))
            continue
        t = 9 if b == 1 else 12
        i = np.arange(olens[b])
        hit = (i + W // 2 >= t * H) & (i + W // 2 < t * H + W)
        assert hit.sum() == W and (_bits(row)[hit] == QNAN).all()
        assert np.array_equal(_bits(row)[~hit], _bits(ref)[~hit])
    assert K == W // 2 + 1


def test_spec_fill_equals_the_twin_and_leaves_the_rest_alone():
    import torch
    W, K = 32, 17
    fr = [16, 17, 33, 1, 15, 17, 33]
    k_lo, k_hi = [0, 0, 0, 0, K - 1, 3, 5], [0, K, 1, K, K, 9, 5]
    t_lo, t_hi = [0, 0, 0, 0, 14, 2, 0], [16, 17, 1, 1, 15, 11, 33]   # empty, full, one bin x one frame at both corners, inner, empty
    for val in (0.0, 1.25):
        buf, so = R.ragged_spectra(W, fr, 200)
        want = S.spec_fill_packed(buf.copy(), K, fr, k_lo, k_hi, t_lo, t_hi, val, so, host=True)
        dev = torch.from_numpy(buf.copy()).cuda()
        got = S.spec_fill_packed(dev, K, fr, k_lo, k_hi, t_lo, t_hi, val, so)
        assert got.data_ptr() == dev.data_ptr()
        _same_buffers(got.cpu().numpy(), want)
        re, im = np.float32(val * np.cos(val)), np.float32(val * np.sin(val))
        touched = np.zeros(buf.size, bool)
        for b, F in enumerate(fr):
            v = want[2 * so[b]:2 * (so[b] + K * F)].reshape(K, F, 2)
            m = np.zeros((K, F, 2), bool)
            m[k_lo[b]:k_hi[b], t_lo[b]:t_hi[b]] = True
            assert (v[..., 0][m[..., 0]] == re).all() and (v[..., 1][m[..., 1]] == im).all()
            touched[2 * so[b]:2 * (so[b] + K * F)] = m.reshape(-1)
        assert touched.sum() == 2 * (K * 17 + 1 + K + 1 + 6 * 9)
        assert np.array_equal(_bits(want)[~touched], _bits(buf)[~touched])


@pytest.mark.parametrize("n_mels", [1, 13, 40])
def test_mfcc_equals_the_host_twin(n_mels):
    import torch
    W, H, sr = 64, 16, 16000
    lens = [33, 1000, 257, 4000, 512]
    offs, o = [], 1
    for n in lens:
        offs.append(o)
        o += n + (2 if (o + n) % 2 else 3)
    buf = np.full(o, np.nan, np.float32)
    for i, (at, n) in enumerate(zip(offs, lens)):
        buf[at:at + n] = R.signal(n, 40 + i)
    for n_mfcc in sorted({1, n_mels}):
        want, oo, shapes = S.mfcc_packed(buf, sr, W, H, n_mfcc, n_mels, lengths=lens, offsets=offs, host=True)
        got, goo, gshapes = S.mfcc_packed(torch.from_numpy(buf).cuda(), sr, W, H, n_mfcc, n_mels, lengths=lens, offsets=offs)
        assert (oo, shapes) == (goo, gshapes) and np.isfinite(want).all()
        _same_buffers(got.cpu().numpy(), want)


def test_spectral_mask_equals_the_three_calls():
    import torch
    W, H, sr = 64, 16, 16000
    lens = [1000, 333, 2048, 97, 640]
    offs, o = [], 1
    for n in lens:
        offs.append(o)
        o += n + (2 if (o + n) % 2 else 3)
    buf = np.full(o, np.nan, np.float32)
    for i, (at, n) in enumerate(zip(offs, lens)):
        buf[at:at + n] = R.signal(n, 60 + i)
    bands, spans = [(300.0, 900.0)], [(0.01, 0.02)]
    dev = torch.from_numpy(buf).cuda()
    got, oo, olens = S.spectral_mask(dev, sr, W, H, bands=bands, spans=spans, lengths=lens, offsets=offs)
    assert oo == offs and olens == lens
    spec, so, shapes = stft_packed(dev, W, H, "hann", lens, offs)
    fr, K = [f for _, f in shapes], W // 2 + 1
    spec = S.mask_frequencies(spec, sr, 300.0, 900.0, K, fr, 0.0, so)
    spec = S.mask_timesteps(spec, [n / sr for n in lens], 0.01, 0.02, K, fr, 0.0, so)
    sep, _, _ = S.istft_packed(spec, W, H, "hann", fr, so, lens, offs)
    _same_buffers(got.cpu().numpy(), sep.cpu().numpy())
    host, _, _ = S.spectral_mask(np.where(np.isnan(buf), 0.0, buf).astype(np.float32), sr, W, H, bands=bands, spans=spans, lengths=lens, offsets=offs, host=True)
    for at, n in zip(offs, lens):
        assert np.array_equal(_bits(got.cpu().numpy()[at:at + n]), _bits(host[at:at + n]))
        assert not np.array_equal(host[at:at + n], buf[at:at + n])
