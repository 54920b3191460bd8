"""GPU suite: ragged batches -- DAC / SNAC Encode and Decode of clips of unequal lengths in one call.

Truth is the existing call on each clip ALONE (B = 1, NC_CHUNK_OFF) from the same handle, and the C oracle on each clip; np.array_equal
everywhere, no tolerance.  Small fixture configs with synthetic weights (as test_chunked_gpu.py); dac_small is the reduced-width DAC with
a decoder stride of 5 (the 5 L - 1 up-convolution), so its decode path covers the odd-stride sample positions.

One batch of 7 clips per direction and kept width C, with W = C + halo_left + halo_right: F = 1 (SNAC: align, the shortest clip it has),
W - align, W, W + align, 3 C + 2 align twice (an equal pair), 6 max_halo + 5 align.  DAC sample lengths are (F - 1) hop + r with r in
{1, 17, hop}: one clip in three ends on a hop multiple.  C in {align, 3 align, max_halo + align}; max_windows in {2, 64}: the windows of
the long clips run split over several launch batches in one setting and as one batch in the other."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import dac_cfg_from_meta, load_golden, snac_cfg_from_meta  # noqa: E402
from neuralcodecs_amd import DAC, SNAC, DACConfig, _lib, dac_halo, snac_halo  # noqa: E402
from neuralcodecs_amd.weights import (dac_synthetic_state_dict, save_blob, snac_noise, snac_synthetic_state_dict,  # noqa: E402
                                      synthetic_pcm)
from oracle import c_oracle  # noqa: E402

FIELDS = ("enc_left", "enc_right", "dec_left", "dec_right")
MAXW = (2, 64)


def _kept_widths(h):
    return [h["align"], 3 * h["align"], max(h[k] for k in FIELDS) + h["align"]]


def _frame_list(h, decode, Ck):
    a, mh = h["align"], max(h[k] for k in FIELDS)
    W = Ck + (h["dec_right"] + h["dec_left"] if decode else h["enc_right"] + h["enc_left"])
    return [a, W - a, W, W + a, 3 * Ck + 2 * a, 3 * Ck + 2 * a, 6 * mh + 5 * a], W


def _launches(m, fn):
    m.profile_enable(True)
    m.profile_reset()
    out = fn()
    n = sum(v["launches"] for v in m.profile_read().values())
    m.profile_enable(False)
    return out, n


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _assert_clips_equal(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        g, w = _np(g), _np(w)
        assert g.shape == w.shape, f"{what}: clip {b} has shape {g.shape}, expected {w.shape}"
        assert np.array_equal(g, w), f"{what}: clip {b} ({w.shape[-1]} columns) differs at {np.argwhere(g != w)[:4].tolist()}"


# ------------------------------------------------------------------------------------------------------------------------ DAC
class _Dac:
    def __init__(self, cfg, weight_seed):
        self.cfg = cfg
        self.blob = save_blob(dac_synthetic_state_dict(cfg, seed=weight_seed))
        self.h = dac_halo(cfg)
        self.m = DAC(cfg)
        self.m.load_blob(self.blob)
        self.m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        self.ref = c_oracle.RefDAC(cfg, self.blob)
        self.cases = {}

    def encode_case(self, which):
        """clips, the codes of every clip alone, the oracle's codes -- computed once per kept width"""
        key = ("enc", which)
        if key not in self.cases:
            cfg, hop = self.cfg, self.cfg.hop_length
            Ck = _kept_widths(self.h)[which]
            frames, W = _frame_list(self.h, False, Ck)
            lens = [(f - 1) * hop + (1, 17, hop)[i % 3] for i, f in enumerate(frames)]
            clips = [synthetic_pcm(1, 1, t, cfg.sample_rate, seed=40 + i)[0, 0] for i, t in enumerate(lens)]
            solo = [self.m.encode(c[None, None])[1][0] for c in clips]
            solo2 = [self.m.encode(c[None, None], n_quantizers=2)[1][0] for c in clips]
            ora = [self.ref.encode(c[None, None])[1][0] for c in clips]
            self.cases[key] = dict(C=Ck, W=W, frames=frames, clips=clips, solo=solo, solo2=solo2, oracle=ora)
        return self.cases[key]

    def decode_case(self, which):
        key = ("dec", which)
        if key not in self.cases:
            cfg = self.cfg
            Ck = _kept_widths(self.h)[which]
            frames, W = _frame_list(self.h, True, Ck)
            rng = np.random.default_rng(50 + which)
            codes = [rng.integers(0, cfg.codebook_size, (cfg.n_codebooks, f)).astype(np.int64) for f in frames]
            solo = [self.m.decode(self.m.from_codes(c[None]))[0, 0] for c in codes]
            ora = [self.ref.decode(self.ref.from_codes(c[None]))[0, 0] for c in codes]
            self.cases[key] = dict(C=Ck, W=W, frames=frames, codes=codes, solo=solo, oracle=ora)
        return self.cases[key]


@pytest.fixture(scope="module")
def dac():
    g = load_golden("dac_small")
    d = _Dac(dac_cfg_from_meta(g["meta"]), g["meta"]["weight_seed"])
    yield d
    d.m.dispose()


def _check_split(m, frames, decode, maxw):
    p = m.ragged_plan(frames, decode)
    W = p["window_frames"]
    assert p["n_windows"] >= 3 and p["n_exact_groups"] == len({f for f in frames if f < W}) >= 2   # F = align and W - align are never cut
    assert (p["n_window_batches"] > 1) == (maxw == 2), p                          # split in one setting, whole in the other
    return p


@pytest.mark.parametrize("maxw", MAXW)
@pytest.mark.parametrize("which", range(3))
def test_dac_encode_ragged_equals_every_clip_alone_and_the_oracle(dac, which, maxw):
    c, m = dac.encode_case(which), dac.m
    m.set_ragged_window(c["C"], maxw)
    p = _check_split(m, c["frames"], False, maxw)
    assert p["kept_frames"] == c["C"] and p["window_frames"] == c["W"]
    codes = m.encode_ragged(c["clips"])
    _assert_clips_equal(codes, c["solo"], f"C {c['C']} max_windows {maxw}: ragged codes against the clip alone")
    _assert_clips_equal(codes, c["oracle"], f"C {c['C']} max_windows {maxw}: ragged codes against the C oracle")


@pytest.mark.parametrize("maxw", MAXW)
@pytest.mark.parametrize("which", range(3))
def test_dac_decode_ragged_equals_every_clip_alone_and_the_oracle(dac, which, maxw):
    c, m = dac.decode_case(which), dac.m
    assert 5 in dac.cfg.decoder_rates and m.decoded_length(c["W"]) == c["W"] * dac.cfg.hop_length - 8   # the 5 L - 1 up-convolution is in play
    m.set_ragged_window(c["C"], maxw)
    _check_split(m, c["frames"], True, maxw)
    pcm = m.decode_codes_ragged(c["codes"])
    _assert_clips_equal(pcm, c["solo"], f"C {c['C']} max_windows {maxw}: ragged pcm against the clip alone")
    _assert_clips_equal(pcm, c["oracle"], f"C {c['C']} max_windows {maxw}: ragged pcm against the C oracle")


def test_dac_ragged_device_entry_points_and_n_quantizers(dac):
    import torch
    m = dac.m
    dev = torch.device("cuda", m.device_index)
    e, d = dac.encode_case(1), dac.decode_case(1)
    m.set_ragged_window(e["C"], 2)
    tc = m.encode_ragged([torch.from_numpy(c).to(dev) for c in e["clips"]])
    tc2 = m.encode_ragged([torch.from_numpy(c).to(dev) for c in e["clips"]], n_quantizers=2)
    h2 = m.encode_ragged(e["clips"], n_quantizers=2)
    m.set_ragged_window(d["C"], 2)
    tp = m.decode_codes_ragged([torch.from_numpy(c).to(dev) for c in d["codes"]])
    hp2 = m.decode_codes_ragged([c[:2] for c in d["codes"]])
    torch.cuda.synchronize()
    m.check_errors()
    assert all(t.is_cuda for t in tc + tp)
    _assert_clips_equal(tc, e["solo"], "device-pointer encode")
    _assert_clips_equal(tc2, e["solo2"], "device-pointer encode, 2 quantizers")
    _assert_clips_equal(h2, e["solo2"], "host-pointer encode, 2 quantizers")
    _assert_clips_equal(tp, d["solo"], "device-pointer decode")
    _assert_clips_equal(hp2, [m.decode(m.from_codes(c[None, :2]))[0, 0] for c in d["codes"]], "host-pointer decode, 2 quantizers")


def test_dac_ragged_is_independent_of_the_clip_order(dac):
    e, d, m = dac.encode_case(2), dac.decode_case(2), dac.m
    perm = [4, 0, 6, 2, 5, 1, 3]
    m.set_ragged_window(e["C"], 2)
    _assert_clips_equal(m.encode_ragged([e["clips"][i] for i in perm]), [e["solo"][i] for i in perm], "permuted encode")
    m.set_ragged_window(d["C"], 2)
    _assert_clips_equal(m.decode_codes_ragged([d["codes"][i] for i in perm]), [d["solo"][i] for i in perm], "permuted decode")


def test_dac_ragged_launches_are_one_uniform_batch_of_windows(dac):
    """No silent per-clip fallback.  6 clips, all >= W frames, max_windows >= n_windows: the call launches what ONE uniform call on
    n_windows rows of W frames launches, plus one gather and one scatter (the design: one table-driven kernel per tensor and batch)."""
    m, cfg, h = dac.m, dac.cfg, dac.h
    Ck = 3 * h["align"]
    m.set_ragged_window(Ck, 64)
    for decode in (False, True):
        W = _frame_list(h, decode, Ck)[1]
        frames = [W, W + 1, W + 2, 2 * W + 1, 6 * max(h[k] for k in FIELDS) + 5, 3 * W]
        nw = m.ragged_plan(frames, decode)
        assert nw["n_exact_groups"] == 0 and nw["n_window_batches"] == nw["n_batches"] == 1
        n = nw["n_windows"]
        if not decode:
            clips = [synthetic_pcm(1, 1, f * cfg.hop_length - 3, cfg.sample_rate, seed=60 + i)[0, 0] for i, f in enumerate(frames)]
            _, got = _launches(m, lambda: m.encode_ragged(clips))
            _, uniform = _launches(m, lambda: m.encode(synthetic_pcm(n, 1, W * cfg.hop_length, cfg.sample_rate, seed=61)))
            solo = sum(_launches(m, lambda c=c: m.encode(c[None, None]))[1] for c in clips)
        else:
            rng = np.random.default_rng(62)
            codes = [rng.integers(0, cfg.codebook_size, (cfg.n_codebooks, f)).astype(np.int64) for f in frames]
            _, got = _launches(m, lambda: m.decode_codes_ragged(codes))
            cu = rng.integers(0, cfg.codebook_size, (n, cfg.n_codebooks, W)).astype(np.int64)
            z, n_fc = _launches(m, lambda: m.from_codes(cu))
            _, n_dec = _launches(m, lambda: m.decode(z))
            uniform = n_fc + n_dec
            solo = sum(_launches(m, lambda c=c: m.decode(m.from_codes(c[None])))[1] for c in codes)
        assert got == uniform + 2, (decode, got, uniform)
        assert got < solo, (decode, got, solo)


def test_dac_ragged_refusals_leave_outputs_untouched(dac):
    m, L = dac.m, _lib.lib()
    m.set_ragged_window(0, 0)
    pcm = np.zeros(4000, np.float32)
    out = np.full(4096, -7, np.int64)
    fout = np.full(4096, -7.0, np.float32)
    codes = np.zeros(4096, np.int64)
    lens = _lib.i64_array

    def enc(fn, p, B, ln, sr, o):
        return fn(m._h, p, B, ln, sr, 0, o)

    for fn in (L.nc_dac_encode_ragged, L.nc_dac_encode_ragged_dev):
        assert enc(fn, pcm.ctypes.data, 2, lens([1000, 0]), 0, out.ctypes.data) == _lib.NC_EINVAL          # a zero-length clip
        assert enc(fn, pcm.ctypes.data, 2, lens([1000, -5]), 0, out.ctypes.data) == _lib.NC_EINVAL
        assert enc(fn, pcm.ctypes.data, 0, lens([1000]), 0, out.ctypes.data) == _lib.NC_EINVAL             # B <= 0
        assert enc(fn, pcm.ctypes.data, 2, lens([1000, 900]), dac.cfg.sample_rate + 1, out.ctypes.data) == _lib.NC_EINVAL   # wrong sample rate
        assert b"sample rate" in L.nc_last_error()
        assert enc(fn, None, 1, lens([1000]), 0, out.ctypes.data) == _lib.NC_EINVAL                        # null pointers
        assert enc(fn, pcm.ctypes.data, 1, None, 0, out.ctypes.data) == _lib.NC_EINVAL
        assert enc(fn, pcm.ctypes.data, 1, lens([1000]), 0, None) == _lib.NC_EINVAL
    for fn in (L.nc_dac_decode_codes_ragged, L.nc_dac_decode_codes_ragged_dev):
        assert fn(m._h, codes.ctypes.data, 2, lens([5, 0]), 2, fout.ctypes.data) == _lib.NC_EINVAL
        assert fn(m._h, codes.ctypes.data, 2, lens([5, 6]), dac.cfg.n_codebooks + 1, fout.ctypes.data) == _lib.NC_EINVAL   # as nc_dac_from_codes
        assert fn(m._h, None, 1, lens([5]), 2, fout.ctypes.data) == _lib.NC_EINVAL
        assert fn(m._h, codes.ctypes.data, 1, lens([5]), 2, None) == _lib.NC_EINVAL
    assert np.all(out == -7) and np.all(fout == -7.0)
    m.synchronize()
    m.check_errors()
    with pytest.raises(ValueError):
        m.set_ragged_window(-1, 0)
    with pytest.raises(ValueError):
        m.ragged_plan([])
    fr, dl = (C.c_int64 * 2)(), (C.c_int64 * 2)()
    _lib.check(L.nc_dac_ragged_query(m._h, 2, lens([1, 1025]), fr, dl))
    assert list(fr) == [m.frames(1), m.frames(1025)] and list(dl) == [m.decoded_length(f) for f in fr]


# ----------------------------------------------------------------------------------------------------------------------- SNAC
class _Snac:
    def __init__(self, name):
        g = load_golden(name)
        self.cfg = cfg = snac_cfg_from_meta(g["meta"])
        self.blob = save_blob(snac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"]))
        self.h = snac_halo(cfg)
        self.m = SNAC(cfg)
        self.m.load_blob(self.blob)
        self.m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        self.ref = c_oracle.RefSNAC(cfg, self.blob)
        self.cases = {}

    def encode_case(self, which):
        key = ("enc", which)
        if key not in self.cases:
            cfg, hop = self.cfg, self.cfg.hop_length
            Ck = _kept_widths(self.h)[which]
            frames, W = _frame_list(self.h, False, Ck)
            lens = [f * hop - (0, 5, hop + 1)[i % 3] for i, f in enumerate(frames)]   # Preprocess pads the last frames
            lens[0] = 3
            assert [self.m.query(t)[1] for t in lens] == frames
            clips = [synthetic_pcm(1, 1, t, cfg.sampling_rate, seed=70 + i)[0, 0] for i, t in enumerate(lens)]
            solo = [[np.ascontiguousarray(lv[0]) for lv in self.m.encode(c[None, None])] for c in clips]
            ora = [[lv[0] for lv in self.ref.encode(c[None, None])[2]] for c in clips]
            self.cases[key] = dict(C=Ck, W=W, frames=frames, clips=clips, solo=solo, oracle=ora)
        return self.cases[key]

    def decode_case(self, which):
        key = ("dec", which)
        if key not in self.cases:
            cfg = self.cfg
            Ck = _kept_widths(self.h)[which]
            frames, W = _frame_list(self.h, True, Ck)
            rng = np.random.default_rng(80 + which)
            codes = [[rng.integers(0, cfg.codebook_size, f // s).astype(np.int64) for s in cfg.vq_strides] for f in frames]
            noise = [snac_noise(cfg, 1, f, seed=90 + i) for i, f in enumerate(frames)]
            solo = [self.m.decode([lv[None] for lv in c], nz)[0, 0] for c, nz in zip(codes, noise)]
            ora = [self.ref.decode([lv[None] for lv in c], nz)[0, 0] for c, nz in zip(codes, noise)]
            self.cases[key] = dict(C=Ck, W=W, frames=frames, codes=codes, noise=noise, solo=solo, oracle=ora)
        return self.cases[key]


@pytest.fixture(scope="module")
def snac():
    d = _Snac("snac_small")
    yield d
    d.m.dispose()


def _assert_levels_equal(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        _assert_clips_equal(g, w, f"{what}, clip {b}")


@pytest.mark.parametrize("maxw", MAXW)
@pytest.mark.parametrize("which", range(3))
def test_snac_encode_ragged_equals_every_clip_alone_and_the_oracle(snac, which, maxw):
    c, m = snac.encode_case(which), snac.m
    m.set_ragged_window(c["C"], maxw)
    p = _check_split(m, c["frames"], False, maxw)
    assert p["kept_frames"] == c["C"] and p["window_frames"] == c["W"]
    codes = m.encode_ragged(c["clips"])
    _assert_levels_equal(codes, c["solo"], f"C {c['C']} max_windows {maxw}: ragged codes against the clip alone")
    _assert_levels_equal(codes, c["oracle"], f"C {c['C']} max_windows {maxw}: ragged codes against the C oracle")


@pytest.mark.parametrize("maxw", MAXW)
@pytest.mark.parametrize("which", range(3))
def test_snac_decode_ragged_with_caller_noise(snac, which, maxw):
    c, m = snac.decode_case(which), snac.m
    m.set_ragged_window(c["C"], maxw)
    _check_split(m, c["frames"], True, maxw)
    pcm = m.decode_ragged(c["codes"], c["noise"])
    _assert_clips_equal(pcm, c["solo"], f"C {c['C']} max_windows {maxw}: ragged pcm against the clip alone")
    _assert_clips_equal(pcm, c["oracle"], f"C {c['C']} max_windows {maxw}: ragged pcm against the C oracle")


def test_snac_decode_ragged_draws_clip_b_from_seed_plus_b(snac):
    c, m = snac.decode_case(1), snac.m
    m.set_ragged_window(c["C"], 2)
    pcm = m.decode_ragged(c["codes"], None, seed=5)
    want = [m.decode([lv[None] for lv in cl], None, seed=5 + b)[0, 0] for b, cl in enumerate(c["codes"])]
    _assert_clips_equal(pcm, want, "noise drawn from seed + b")
    assert not np.array_equal(pcm[3], c["solo"][3])


def test_snac_ragged_device_entry_points_and_clip_order(snac):
    import torch
    m = snac.m
    dev = torch.device("cuda", m.device_index)
    e, d = snac.encode_case(1), snac.decode_case(1)
    perm = [4, 0, 6, 2, 5, 1, 3]
    m.set_ragged_window(e["C"], 2)
    tc = m.encode_ragged([torch.from_numpy(c).to(dev) for c in e["clips"]])
    pc = m.encode_ragged([e["clips"][i] for i in perm])
    m.set_ragged_window(d["C"], 2)
    tp = m.decode_ragged([[torch.from_numpy(lv).to(dev) for lv in c] for c in d["codes"]],
                         [[torch.from_numpy(n).to(dev) for n in nz] for nz in d["noise"]])
    ts = m.decode_ragged([[torch.from_numpy(lv).to(dev) for lv in c] for c in d["codes"]], None, seed=5)
    pp = m.decode_ragged([d["codes"][i] for i in perm], [d["noise"][i] for i in perm])
    torch.cuda.synchronize()
    m.check_errors()
    _assert_levels_equal(tc, e["solo"], "device-pointer encode")
    _assert_levels_equal(pc, [e["solo"][i] for i in perm], "permuted encode")
    _assert_clips_equal(tp, d["solo"], "device-pointer decode")
    _assert_clips_equal(ts, m.decode_ragged(d["codes"], None, seed=5), "device-pointer decode, drawn noise")
    _assert_clips_equal(pp, [d["solo"][i] for i in perm], "permuted decode")


def test_snac_ragged_launches_are_one_uniform_batch_of_windows(snac):
    """As the DAC test; decode gathers two tensors (codes, noise), so it adds three launches to the uniform call's."""
    m, cfg, h = snac.m, snac.cfg, snac.h
    Ck = 3 * h["align"]
    m.set_ragged_window(Ck, 64)
    for decode in (False, True):
        W, a = _frame_list(h, decode, Ck)[1], h["align"]
        frames = [W, W + a, W + 2 * a, 2 * W + a, 6 * max(h[k] for k in FIELDS) + 5 * a, 3 * W]
        nw = m.ragged_plan(frames, decode)
        assert nw["n_exact_groups"] == 0 and nw["n_window_batches"] == nw["n_batches"] == 1
        n = nw["n_windows"]
        rng = np.random.default_rng(63)
        if not decode:
            clips = [synthetic_pcm(1, 1, f * cfg.hop_length - 3, cfg.sampling_rate, seed=64 + i)[0, 0] for i, f in enumerate(frames)]
            _, got = _launches(m, lambda: m.encode_ragged(clips))
            _, uniform = _launches(m, lambda: m.encode(synthetic_pcm(n, 1, W * cfg.hop_length, cfg.sampling_rate, seed=65)))
            solo = sum(_launches(m, lambda c=c: m.encode(c[None, None]))[1] for c in clips)
            extra = 2
        else:
            codes = [[rng.integers(0, cfg.codebook_size, f // s).astype(np.int64) for s in cfg.vq_strides] for f in frames]
            noise = [snac_noise(cfg, 1, f, seed=66 + i) for i, f in enumerate(frames)]
            _, got = _launches(m, lambda: m.decode_ragged(codes, noise))
            cu = [rng.integers(0, cfg.codebook_size, (n, W // s)).astype(np.int64) for s in cfg.vq_strides]
            _, uniform = _launches(m, lambda: m.decode(cu, snac_noise(cfg, n, W, seed=67)))
            solo = sum(_launches(m, lambda c=c, z=z: m.decode([lv[None] for lv in c], z))[1] for c, z in zip(codes, noise))
            extra = 3 if cfg.noise else 2
        assert got == uniform + extra, (decode, got, uniform)
        assert got < solo, (decode, got, solo)


def test_snac_ragged_refusals_leave_outputs_untouched(snac):
    m, L = snac.m, _lib.lib()
    a = snac.h["align"]
    pcm = np.zeros(4000, np.float32)
    out = np.full(4096, -7, np.int64)
    fout = np.full(1 << 16, -7.0, np.float32)
    codes = np.zeros(4096, np.int64)
    lens = _lib.i64_array
    for fn in (L.nc_snac_encode_ragged, L.nc_snac_encode_ragged_dev):
        assert fn(m._h, pcm.ctypes.data, 2, lens([1000, 0]), out.ctypes.data) == _lib.NC_EINVAL
        assert fn(m._h, pcm.ctypes.data, -1, lens([1000]), out.ctypes.data) == _lib.NC_EINVAL
        assert fn(m._h, None, 1, lens([1000]), out.ctypes.data) == _lib.NC_EINVAL
        assert fn(m._h, pcm.ctypes.data, 1, lens([1000]), None) == _lib.NC_EINVAL
    for fn in (L.nc_snac_decode_ragged, L.nc_snac_decode_ragged_dev):
        assert fn(m._h, codes.ctypes.data, 2, lens([a, 0]), None, 0, fout.ctypes.data) == _lib.NC_EINVAL
        assert fn(m._h, codes.ctypes.data, 2, lens([a, a + 1]), None, 0, fout.ctypes.data) == _lib.NC_EINVAL   # as nc_snac_decode on that clip
        assert fn(m._h, None, 1, lens([a]), None, 0, fout.ctypes.data) == _lib.NC_EINVAL
        assert fn(m._h, codes.ctypes.data, 1, lens([a]), None, 0, None) == _lib.NC_EINVAL
    assert np.all(out == -7) and np.all(fout == -7.0)
    m.synchronize()
    m.check_errors()
    with DAC(DACConfig()) as d:                                                    # a handle of the other kind
        assert L.nc_snac_encode_ragged(d._h, pcm.ctypes.data, 1, lens([1000]), out.ctypes.data) == _lib.NC_EINVAL
    assert np.all(out == -7)
