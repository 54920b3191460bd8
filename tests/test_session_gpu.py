"""GPU suite: incremental sessions of DAC and SNAC -- codes or PCM pushed piece by piece; the concatenated output == the one-shot call on
the same handle, bit for bit (np.array_equal only: a mismatch means a kernel instance is not position-independent, which is a finding).

Shapes (the reduced-width fixture configs of tests/test_chunked_gpu.py, B = 2): frames = 2 * max(halos) + 4 * align, so there are
windows at the clip's true left edge, windows with both edges cut and the flush window at the true right edge.  Push patterns: constant
pushes of align frames, irregular pushes, one push larger than hl + hr, everything in one push, a clip shorter than hr."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import dac_cfg_from_meta, load_golden, snac_cfg_from_meta  # noqa: E402
from neuralcodecs_amd import DAC, SNAC, DACConfig, Encodec, EncodecConfig, SNACConfig, _lib, dac_halo, snac_halo  # noqa: E402
from neuralcodecs_amd.weights import (dac_synthetic_state_dict, save_blob, snac_noise, snac_synthetic_state_dict,  # noqa: E402
                                      synthetic_pcm)

B = 2
FIELDS = ("enc_left", "enc_right", "dec_left", "dec_right")
PATTERNS = ("constant", "irregular", "one_large_push", "all_in_one", "shorter_than_hr")


def _pushes(h, decode, frames, which):
    """frame counts of the pushes of pattern `which`; they sum to `frames` except for the clip shorter than hr"""
    a = h["align"]
    hl, hr = (h["dec_right"], h["dec_left"]) if decode else (h["enc_right"], h["enc_left"])
    if which == "constant":
        return [a] * (frames // a)
    if which == "irregular":
        out, left, i = [], frames, 0
        while left > 0:
            out.append(min(left, a * (1, 3, 2, 7, 1, 5)[i % 6]))
            left -= out[-1]
            i += 1
        return out
    if which == "one_large_push":
        return [a, hl + hr + 2 * a, frames - (hl + hr + 3 * a)]
    if which == "all_in_one":
        return [frames]
    return [a] * max(1, (hr - a) // a)


def _launches(m, fn):
    m.profile_enable(True)
    m.profile_reset()
    out = fn()
    n = sum(v["launches"] for v in m.profile_read().values())
    m.profile_enable(False)
    return out, n


def _cat(parts):
    return np.concatenate([np.asarray(p) for p in parts], axis=-1)


# ------------------------------------------------------------------------------------------------------------------------ DAC
@pytest.fixture(scope="module")
def dac_small():
    cfg = dac_cfg_from_meta(load_golden("dac_small")["meta"])
    h = dac_halo(cfg)
    frames = 2 * max(h[k] for k in FIELDS) + 4 * h["align"]
    T = (frames - 1) * cfg.hop_length + 17                                  # not a multiple of the hop
    pcm = synthetic_pcm(B, 1, T, cfg.sample_rate, seed=41)
    m = DAC(cfg)
    m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=load_golden("dac_small")["meta"]["weight_seed"])))
    m.set_chunk_frames(_lib.NC_CHUNK_OFF)
    codes = m.encode(pcm)[1]
    ref = {}

    def audio(n_frames, nq=None):                                           # one-shot references, computed once per shape
        key = (n_frames, nq)
        if key not in ref:
            ref[key] = m.decode(m.from_codes(np.ascontiguousarray(codes[:, :nq, :n_frames])))
        return ref[key]

    def enc(n_samples):
        key = ("enc", n_samples)
        if key not in ref:
            ref[key] = m.encode(np.ascontiguousarray(pcm[:, :, :n_samples]))[1]
        return ref[key]

    yield dict(cfg=cfg, h=h, frames=frames, T=T, pcm=pcm, m=m, codes=codes, audio=audio, enc=enc)
    m.dispose()


def _dac_decode(d, pushes, nq=None, to=None):
    m, codes = d["m"], d["codes"]
    got, pend, o = [], [], 0
    with m.decode_session(B, nq) as s:
        for n in pushes:
            c = np.ascontiguousarray(codes[:, :nq, o:o + n])
            got.append(s.push(to(c) if to else c))
            o += n
            pend.append(s.pending())
        got.append(s.flush())
        assert s.pending() == 0
    return got, pend


@pytest.mark.parametrize("which", PATTERNS)
def test_dac_decode_session_equals_one_shot(dac_small, which):
    d = dac_small
    pushes = _pushes(d["h"], True, d["frames"], which)
    got, pend = _dac_decode(d, pushes)
    want = d["audio"](sum(pushes))
    assert _cat(got).shape == want.shape and np.array_equal(_cat(got), want), which
    assert max(pend) <= d["h"]["dec_left"] + max(pushes)                    # latency: hr frames behind what has arrived
    if which == "shorter_than_hr":
        assert all(g.shape[-1] == 0 for g in got[:-1]), "a clip shorter than hr emitted before the flush"
    if which == "constant":
        assert any(g.shape[-1] > 0 for g in got[:-1]), "nothing was emitted before the flush"


def test_dac_decode_session_two_codebooks(dac_small):
    d = dac_small
    got, _ = _dac_decode(d, _pushes(d["h"], True, d["frames"], "irregular"), nq=2)
    assert np.array_equal(_cat(got), d["audio"](d["frames"], 2))
    assert not np.array_equal(d["audio"](d["frames"], 2), d["audio"](d["frames"]))


def _sample_pushes(pushes, hop, T):
    """the frame pattern in samples, cut to T samples in all"""
    out, left = [], T
    for n in pushes:
        k = min(left, n * hop)
        if k > 0:
            out.append(k)
        left -= k
    if left > 0:
        out.append(left)
    return out


def _encode(m, pcm, sample_pushes, to=None):
    got, o = [], 0
    with m.encode_session(B) as s:
        for n in sample_pushes:
            x = np.ascontiguousarray(pcm[:, :, o:o + n])
            got.append(s.push(to(x) if to else x))
            o += n
        got.append(s.flush())
    return got


@pytest.mark.parametrize("which", PATTERNS + ("sub_hop",))
def test_dac_encode_session_equals_one_shot(dac_small, which):
    d = dac_small
    hop = d["cfg"].hop_length
    if which == "sub_hop":                                                  # pushes of fewer samples than one hop among larger ones
        sp = _sample_pushes([1] * (2 * d["frames"]), hop // 3 + 1, d["T"] // 2) + [d["T"] - d["T"] // 2]
        T = d["T"]
    elif which == "shorter_than_hr":
        fr = sum(_pushes(d["h"], False, d["frames"], which))
        T = fr * hop - 3
        sp = _sample_pushes(_pushes(d["h"], False, d["frames"], which), hop, T)
    else:
        T = d["T"]
        sp = _sample_pushes(_pushes(d["h"], False, d["frames"], which), hop, T)
    assert sum(sp) == T and T % hop != 0
    got = _encode(d["m"], d["pcm"], sp)
    want = d["enc"](T)
    assert _cat(got).shape == want.shape and np.array_equal(_cat(got), want), which
    if which == "shorter_than_hr":
        assert all(g.shape[-1] == 0 for g in got[:-1])


def test_dac_device_pointer_forms_equal_the_host_forms(dac_small):
    import torch
    d = dac_small
    dev = torch.device("cuda", d["m"].device_index)
    to = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    pushes = _pushes(d["h"], True, d["frames"], "irregular")
    host, _ = _dac_decode(d, pushes)
    got, _ = _dac_decode(d, pushes, to=to)
    assert [tuple(g.shape) for g in got] == [tuple(g.shape) for g in host]      # n_out is host arithmetic: known before any synchronisation
    sp = _sample_pushes(_pushes(d["h"], False, d["frames"], "irregular"), d["cfg"].hop_length, d["T"])
    ehost = _encode(d["m"], d["pcm"], sp)
    egot = _encode(d["m"], d["pcm"], sp, to=to)
    assert [tuple(g.shape) for g in egot] == [tuple(g.shape) for g in ehost]
    torch.cuda.synchronize()
    assert all(torch.is_tensor(g) and g.is_cuda for g in got + egot)
    for a, b in zip(got + egot, host + ehost):
        assert np.array_equal(a.cpu().numpy(), b)
    assert np.array_equal(_cat([g.cpu().numpy() for g in got]), d["audio"](d["frames"]))
    assert np.array_equal(_cat([g.cpu().numpy() for g in egot]), d["enc"](d["T"]))


def test_dac_two_sessions_interleaved_on_one_handle(dac_small):
    d = dac_small
    m, codes, pcm = d["m"], d["codes"], d["pcm"]
    pushes = _pushes(d["h"], True, d["frames"], "irregular")
    sp = _sample_pushes(_pushes(d["h"], False, d["frames"], "constant"), d["cfg"].hop_length, d["T"])
    dec, enc, dec1 = m.decode_session(B), m.encode_session(B), m.decode_session(1, 2)
    ga, gb, gc, oa, ob = [], [], [], 0, 0
    for i in range(max(len(pushes), len(sp))):
        if i < len(pushes):
            ga.append(dec.push(np.ascontiguousarray(codes[:, :, oa:oa + pushes[i]])))
            gc.append(dec1.push(np.ascontiguousarray(codes[1:, :2, oa:oa + pushes[i]])))
            oa += pushes[i]
        if i < len(sp):
            gb.append(enc.push(np.ascontiguousarray(pcm[:, :, ob:ob + sp[i]])))
            ob += sp[i]
    gb.append(enc.flush())
    ga.append(dec.flush())
    gc.append(dec1.flush())
    for s in (dec, enc, dec1):
        s.close()
    assert np.array_equal(_cat(ga), d["audio"](d["frames"]))
    assert np.array_equal(_cat(gb), d["enc"](d["T"]))
    assert np.array_equal(_cat(gc), d["audio"](d["frames"], 2)[1:])


def test_dac_reset_reproduces_the_first_run(dac_small):
    d = dac_small
    codes = d["codes"]
    pushes = _pushes(d["h"], True, d["frames"], "irregular")
    with d["m"].decode_session(B) as s:
        runs = []
        for cut in (len(pushes) // 2, len(pushes)):                         # the first run is abandoned half way, without a flush
            got, o = [], 0
            for n in pushes[:cut]:
                got.append(s.push(np.ascontiguousarray(codes[:, :, o:o + n])))
                o += n
            if cut == len(pushes):
                got.append(s.flush())
                with pytest.raises(ValueError):                             # a push after the flush
                    s.push(np.ascontiguousarray(codes[:, :, :1]))
                with pytest.raises(ValueError):
                    s.flush()
            runs.append(got)
            s.reset()
            assert s.pending() == 0
        again, o = [], 0
        for n in pushes:
            again.append(s.push(np.ascontiguousarray(codes[:, :, o:o + n])))
            o += n
        again.append(s.flush())
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert len(again) == len(runs[1]) and all(np.array_equal(a, b) for a, b in zip(again, runs[1]))
    assert np.array_equal(_cat(again), d["audio"](d["frames"]))


# ----------------------------------------------------------------------------------------------------------------------- SNAC
_SNAC = {}


def _snac_small(name):
    if name in _SNAC:
        return _SNAC[name]
    g = load_golden(name)
    cfg = snac_cfg_from_meta(g["meta"])
    h = snac_halo(cfg)
    frames = 2 * max(h[k] for k in FIELDS) + 4 * h["align"]
    T = frames * cfg.hop_length - 5                                     # not a multiple of the hop: Preprocess pads the last frame
    pcm = synthetic_pcm(B, 1, T, cfg.sampling_rate, seed=42)
    noises = snac_noise(cfg, B, frames, seed=43)
    m = SNAC(cfg)
    m.load_blob(save_blob(snac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"])))
    m.set_chunk_frames(_lib.NC_CHUNK_OFF)
    codes = [np.ascontiguousarray(c) for c in m.encode(pcm)]
    ref = {}

    def cut(n_frames, o=0):
        return ([np.ascontiguousarray(c[:, o // s:(o + n_frames) // s]) for c, s in zip(codes, cfg.vq_strides)],
                [np.ascontiguousarray(z[:, :, o * (z.shape[-1] // frames):(o + n_frames) * (z.shape[-1] // frames)]) for z in noises])

    def audio(n_frames):
        if n_frames not in ref:
            c, z = cut(n_frames)
            ref[n_frames] = m.decode(c, z if cfg.noise else None)
        return ref[n_frames]

    def enc(n_samples):
        key = ("enc", n_samples)
        if key not in ref:
            ref[key] = [np.ascontiguousarray(c) for c in m.encode(np.ascontiguousarray(pcm[:, :, :n_samples]))]
        return ref[key]

    _SNAC[name] = dict(cfg=cfg, h=h, frames=frames, T=T, pcm=pcm, m=m, codes=codes, cut=cut, audio=audio, enc=enc)
    return _SNAC[name]


def _snac_decode(d, pushes, to=None):
    got, o = [], 0
    with d["m"].decode_session(B) as s:
        for n in pushes:
            c, z = d["cut"](n, o)
            if to:
                c, z = [to(x) for x in c], [to(x) for x in z]
            got.append(s.push(c, z if d["cfg"].noise else None))
            o += n
        got.append(s.flush())
    return got


@pytest.mark.parametrize("which", PATTERNS)
@pytest.mark.parametrize("name", ["snac_small", "snac_small_attn"])
def test_snac_decode_session_equals_one_shot(name, which):
    d = _snac_small(name)
    pushes = _pushes(d["h"], True, d["frames"], which)
    got = _snac_decode(d, pushes)
    want = d["audio"](sum(pushes))
    assert _cat(got).shape == want.shape and np.array_equal(_cat(got), want), (name, which)
    if which == "shorter_than_hr":
        assert all(g.shape[-1] == 0 for g in got[:-1])


def test_snac_noise_fixture_has_noise_blocks_and_attention():
    cfg = _snac_small("snac_small_attn")["cfg"]
    assert cfg.noise and cfg.attn_window_size, "the explicit-noise cases above need a fixture with NoiseBlocks and LocalMHA"


def _levels_cat(parts, n_levels):
    return [_cat([p[i] for p in parts]) for i in range(n_levels)]


@pytest.mark.parametrize("which", PATTERNS + ("sub_hop",))
@pytest.mark.parametrize("name", ["snac_small", "snac_small_attn"])
def test_snac_encode_session_equals_one_shot(name, which):
    d = _snac_small(name)
    hop = d["cfg"].hop_length
    if which == "sub_hop":
        sp = _sample_pushes([1] * (2 * d["frames"]), hop // 3 + 1, d["T"] // 2) + [d["T"] - d["T"] // 2]
        T = d["T"]
    elif which == "shorter_than_hr":
        T = sum(_pushes(d["h"], False, d["frames"], which)) * hop - 3
        sp = _sample_pushes(_pushes(d["h"], False, d["frames"], which), hop, T)
    else:
        T = d["T"]
        sp = _sample_pushes(_pushes(d["h"], False, d["frames"], which), hop, T)
    assert sum(sp) == T and T % hop != 0
    got = _encode(d["m"], d["pcm"], sp)
    want = d["enc"](T)
    have = _levels_cat(got, len(want))
    for i, (a, b) in enumerate(zip(have, want)):
        assert a.shape == b.shape and np.array_equal(a, b), (name, which, i)


def test_snac_device_pointer_forms_and_seeded_noise():
    import torch
    d = _snac_small("snac_small_attn")
    m = d["m"]
    dev = torch.device("cuda", m.device_index)
    to = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    pushes = _pushes(d["h"], True, d["frames"], "irregular")
    host = _snac_decode(d, pushes)
    got = _snac_decode(d, pushes, to=to)
    assert [tuple(g.shape) for g in got] == [tuple(g.shape) for g in host]
    sp = _sample_pushes(_pushes(d["h"], False, d["frames"], "irregular"), d["cfg"].hop_length, d["T"])
    egot = _encode(m, d["pcm"], sp, to=to)
    torch.cuda.synchronize()
    assert np.array_equal(_cat([g.cpu().numpy() for g in got]), d["audio"](d["frames"]))
    for a, b in zip(_levels_cat([[lv.cpu().numpy() for lv in p] for p in egot], len(d["codes"])), d["enc"](d["T"])):
        assert np.array_equal(a, b)
    # noise == NULL: drawn per push from (seed, frame position) -- reproducible, seed-dependent, and not the one-shot seeded draw
    runs = []
    for seed in (7, 7, 8):
        parts, o = [], 0
        with m.decode_session(B) as s:
            s.set_seed(seed)
            for n in pushes:
                parts.append(s.push(d["cut"](n, o)[0]))
                o += n
            parts.append(s.flush())
        runs.append(_cat(parts))
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[0], runs[2])
    assert runs[0].shape == d["audio"](d["frames"]).shape and np.isfinite(runs[0]).all()


def test_snac_two_sessions_interleaved_on_one_handle():
    d = _snac_small("snac_small_attn")
    m = d["m"]
    pushes = _pushes(d["h"], True, d["frames"], "constant")
    sp = _sample_pushes(_pushes(d["h"], False, d["frames"], "irregular"), d["cfg"].hop_length, d["T"])
    dec, enc = m.decode_session(B), m.encode_session(B)
    ga, gb, oa, ob = [], [], 0, 0
    for i in range(max(len(pushes), len(sp))):
        if i < len(sp):
            gb.append(enc.push(np.ascontiguousarray(d["pcm"][:, :, ob:ob + sp[i]])))
            ob += sp[i]
        if i < len(pushes):
            c, z = d["cut"](pushes[i], oa)
            ga.append(dec.push(c, z))
            oa += pushes[i]
    ga.append(dec.flush())
    gb.append(enc.flush())
    dec.close()
    enc.close()
    assert np.array_equal(_cat(ga), d["audio"](d["frames"]))
    for a, b in zip(_levels_cat(gb, len(d["codes"])), d["enc"](d["T"])):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------ error conventions
def test_error_conventions(dac_small):
    L = _lib.lib()
    with Encodec(EncodecConfig()) as e:
        out = C.c_void_p()
        assert L.nc_session_create(e._h, 1, 1, 0, C.byref(out)) == _lib.NC_EUNSUPPORTED and not out.value
        assert L.nc_session_create(e._h, 0, 1, 0, C.byref(out)) == _lib.NC_EUNSUPPORTED
    d = dac_small
    m = d["m"]
    with pytest.raises(ValueError):
        m.decode_session(0)
    with m.decode_session(B) as s:
        with pytest.raises(ValueError):
            s.flush()                                                       # nothing pushed
    n = C.c_int64(-1)
    with m.decode_session(B) as s:
        codes = np.ascontiguousarray(d["codes"][:, :, :8])
        cap = s.query(8)
        small = np.zeros((B, cap), np.float32)
        assert L.nc_session_push(s._s, codes.ctypes.data, 8, None, small.ctypes.data, cap - 1, C.byref(n)) == _lib.NC_EINVAL
        assert L.nc_session_flush(s._s, small.ctypes.data, s.query(0) - 1, C.byref(n)) == _lib.NC_EINVAL
        assert L.nc_session_push(s._s, None, 8, None, small.ctypes.data, cap, C.byref(n)) == _lib.NC_EINVAL
        assert L.nc_session_push(s._s, codes.ctypes.data, 0, None, small.ctypes.data, cap, C.byref(n)) == _lib.NC_EINVAL
        assert s.pending() == 0 and n.value == -1                           # refused before anything moved
        assert s.push(codes[:, :, :1]).shape[-1] == 0 and s.pending() == 1   # a refused call leaves the session usable
    with DAC(d["cfg"]) as unloaded:                                         # no weights: NC_ESTATE
        with unloaded.decode_session(1) as s:
            with pytest.raises(RuntimeError):
                s.push(np.zeros((1, d["cfg"].n_codebooks, 4), np.int64))
    sn = _snac_small("snac_small")
    a = sn["h"]["align"]
    assert a > 1
    with sn["m"].decode_session(B) as s:
        flat = np.zeros((B, 4 * a), np.int64)
        out = np.zeros((B, s.query(a)), np.float32)
        assert L.nc_session_push(s._s, flat.ctypes.data, a + 1, None, out.ctypes.data, out.shape[1], C.byref(n)) == _lib.NC_EINVAL
        assert L.nc_session_query(s._s, a + 1, C.byref(n)) == _lib.NC_EINVAL
        assert s.pending() == 0


# ------------------------------------------------------------------------------------------------- nothing changes without a session
# Launches of one-shot encode / decode (profiled kernel classes) on the fixtures of tests/test_chunked_gpu.py, as that file records them
PARENT_LAUNCHES = {"dac_small": (39, 30), "snac_small": (44, 44)}


def test_a_handle_without_a_session_launches_what_it_launched_before(dac_small):
    cfg = dac_small["cfg"]
    h = dac_small["h"]
    frames = 6 * max(h[k] for k in FIELDS) + 5 * h["align"]
    pcm = synthetic_pcm(B, 1, (frames - 1) * cfg.hop_length + 17, cfg.sample_rate, seed=21)
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=load_golden("dac_small")["meta"]["weight_seed"])))
        (z, _, _, _, _), n_enc = _launches(m, lambda: m.encode(pcm))
        audio, n_dec = _launches(m, lambda: m.decode(z))
        assert (n_enc, n_dec) == PARENT_LAUNCHES["dac_small"]
        with m.decode_session(B) as s:                                      # ... and a session leaves the one-shot calls as they were
            s.push(np.ascontiguousarray(m.encode(pcm)[1][:, :, :h["dec_left"] + 4]))
            s.flush()
        (z2, _, _, _, _), n_enc2 = _launches(m, lambda: m.encode(pcm))
        audio2, n_dec2 = _launches(m, lambda: m.decode(z2))
        assert (n_enc2, n_dec2) == (n_enc, n_dec) and np.array_equal(audio2, audio)
    g = load_golden("snac_small")
    scfg = snac_cfg_from_meta(g["meta"])
    sh = snac_halo(scfg)
    frames = 6 * max(sh[k] for k in FIELDS) + 5 * sh["align"]
    pcm = synthetic_pcm(B, 1, frames * scfg.hop_length - 5, scfg.sampling_rate, seed=22)
    with SNAC(scfg) as m:
        m.load_blob(save_blob(snac_synthetic_state_dict(scfg, seed=g["meta"]["weight_seed"])))
        codes, n_enc = _launches(m, lambda: m.encode(pcm))
        _, n_dec = _launches(m, lambda: m.decode([np.ascontiguousarray(c) for c in codes], snac_noise(scfg, B, frames, seed=23)))
        assert (n_enc, n_dec) == PARENT_LAUNCHES["snac_small"]


def test_snac_fixtures_are_released():
    for d in _SNAC.values():
        d["m"].dispose()
    _SNAC.clear()


# ---------------------------------------------------------------------------------------------------------- full-size instances
def test_dac44k_decode_session_equals_one_shot():
    """Engine against itself: window-sized and clip-sized layers pick different conv instances here."""
    cfg = DACConfig.dac_44khz()
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=3)))
        pcm = synthetic_pcm(1, 1, 3 * cfg.sample_rate, cfg.sample_rate, seed=31)
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        codes = m.encode(pcm)[1]
        want = m.decode(m.from_codes(codes))
        got = []
        with m.decode_session(1) as s:
            for o in range(0, codes.shape[-1], 32):
                got.append(s.push(np.ascontiguousarray(codes[:, :, o:o + 32])))
            got.append(s.flush())
        assert sum(g.shape[-1] > 0 for g in got) > 4
        assert _cat(got).shape == want.shape and np.array_equal(_cat(got), want)


def test_snac24k_sessions_equal_one_shot():
    cfg = SNACConfig.snac_24khz()
    frames = 2 * 16 + 3 * 4 + 64
    with SNAC(cfg) as m:
        m.load_blob(save_blob(snac_synthetic_state_dict(cfg, seed=4)))
        pcm = synthetic_pcm(1, 1, frames * cfg.hop_length, cfg.sampling_rate, seed=32)
        noises = snac_noise(cfg, 1, frames, seed=33) if cfg.noise else None
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        codes = [np.ascontiguousarray(c) for c in m.encode(pcm)]
        assert int(codes[-1].shape[-1]) * cfg.vq_strides[-1] == frames
        want = m.decode(codes, noises)
        got, enc = [], []
        with m.decode_session(1) as s, m.encode_session(1) as e:
            for o in range(0, frames, 16):
                n = min(16, frames - o)
                c = [np.ascontiguousarray(lv[:, o // st:(o + n) // st]) for lv, st in zip(codes, cfg.vq_strides)]
                z = [np.ascontiguousarray(b[:, :, o * (b.shape[-1] // frames):(o + n) * (b.shape[-1] // frames)]) for b in noises] if noises else None
                got.append(s.push(c, z))
                enc.append(e.push(np.ascontiguousarray(pcm[:, :, o * cfg.hop_length:(o + n) * cfg.hop_length])))
            got.append(s.flush())
            enc.append(e.flush())
        assert np.array_equal(_cat(got), want)
        for a, b in zip(_levels_cat(enc, len(codes)), codes):
            assert a.shape == b.shape and np.array_equal(a, b)
