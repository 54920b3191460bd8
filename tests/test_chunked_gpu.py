"""GPU suite: chunked Encode / Decode / FromCodes of DAC and SNAC (long clips) -- chunked == one-shot, bit for bit.

Shapes (small fixture configs, B = 2): frames = 6 * max_halo + 5 * align, so that there are windows with both halos fully interior,
windows clipped at each clip edge and a final partial chunk; DAC gets a ragged 17-sample tail.  Chunk sizes: align, 3 * align,
max_halo + align, frames - align.  No tolerance anywhere: every kept output is the number the one-shot call produces."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import dac_cfg_from_meta, load_golden, snac_cfg_from_meta  # noqa: E402
from neuralcodecs_amd import DAC, SNAC, DACConfig, Encodec, EncodecConfig, SNACConfig, _lib, dac_halo, snac_halo  # noqa: E402
from neuralcodecs_amd.weights import (dac_synthetic_state_dict, save_blob, snac_noise, snac_synthetic_state_dict,  # noqa: E402
                                      synthetic_pcm)
from oracle import c_oracle  # noqa: E402

B = 2
FIELDS = ("enc_left", "enc_right", "dec_left", "dec_right")
ARENA_BUDGET = 1 << 30   # AUTO on a 2^30-sample clip: 3 buffers x 96 channels x (1024 + 21 frames) x 512 samples x 4 B = 0.6 GB < 1 GiB


def _chunks(h, frames):
    mh = max(h[k] for k in FIELDS)
    return [h["align"], 3 * h["align"], mh + h["align"], frames - h["align"]]


def _launches(m, fn):
    m.profile_enable(True)
    m.profile_reset()
    out = fn()
    n = sum(v["launches"] for v in m.profile_read().values())
    m.profile_enable(False)
    return out, n


# ------------------------------------------------------------------------------------------------------------------------ DAC
@pytest.fixture(scope="module")
def dac_small():
    g = load_golden("dac_small")
    cfg = dac_cfg_from_meta(g["meta"])
    blob = save_blob(dac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"]))
    h = dac_halo(cfg)
    frames = 6 * max(h[k] for k in FIELDS) + 5 * h["align"]
    T = (frames - 1) * cfg.hop_length + 17
    pcm = synthetic_pcm(B, 1, T, cfg.sample_rate, seed=21)
    m = DAC(cfg)
    m.load_blob(blob)
    m.set_chunk_frames(_lib.NC_CHUNK_OFF)
    one = {}
    (one["z"], one["codes"], one["lat"], _, _), one["n_enc"] = _launches(m, lambda: m.encode(pcm))
    one["audio"], one["n_dec"] = _launches(m, lambda: m.decode(one["z"]))
    one["from_codes"] = m.from_codes(one["codes"])
    one["z2"], one["codes2"], one["lat2"], _, _ = m.encode(pcm, n_quantizers=2)
    one["matrix"] = m.encode_to_code_matrix(pcm)
    one["matrix_audio"] = m.decode_code_matrix(one["matrix"])
    one["plan_enc"], one["plan_dec"] = m.chunk_plan(frames, False, B), m.chunk_plan(frames, True, B)
    ref = c_oracle.RefDAC(cfg, blob)
    rz, rcodes, rlat, _ = ref.encode(pcm)
    oracle = {"z": rz, "codes": rcodes, "lat": rlat, "audio": ref.decode(one["z"]), "from_codes": ref.from_codes(one["codes"])}
    yield dict(cfg=cfg, h=h, frames=frames, pcm=pcm, m=m, one=one, oracle=oracle)
    m.dispose()


def test_dac_one_shot_reference_matches_the_oracle(dac_small):
    one, ora = dac_small["one"], dac_small["oracle"]
    assert one["plan_enc"]["n_chunks"] == 1 and one["plan_dec"]["n_chunks"] == 1
    for k in ("z", "codes", "lat", "audio", "from_codes"):
        assert np.array_equal(one[k], ora[k]), k


@pytest.mark.parametrize("which", range(4))
def test_dac_small_chunked_equals_one_shot_and_oracle(dac_small, which):
    d = dac_small
    m, one, ora, frames, pcm = d["m"], d["one"], d["oracle"], d["frames"], d["pcm"]
    chunk = _chunks(d["h"], frames)[which]
    m.set_chunk_frames(chunk)
    try:
        pe, pd = m.chunk_plan(frames, False, B), m.chunk_plan(frames, True, B)
        assert pe["n_chunks"] == pd["n_chunks"] == -(-frames // chunk) > 1                  # no silent one-shot fallback
        assert pe["chunk_frames"] == chunk and pe["halo_left"] == d["h"]["enc_right"] and pe["halo_right"] == d["h"]["enc_left"]
        assert pd["halo_left"] == d["h"]["dec_right"] and pd["halo_right"] == d["h"]["dec_left"]
        (z, codes, lat, _, _), n_enc = _launches(m, lambda: m.encode(pcm))
        audio, n_dec = _launches(m, lambda: m.decode(one["z"]))
        zf = m.from_codes(one["codes"])
        assert n_enc > one["n_enc"] and n_dec > one["n_dec"]
        for name, got, key in (("codes", codes, "codes"), ("z", z, "z"), ("latents", lat, "lat"), ("decode", audio, "audio"),
                               ("from_codes", zf, "from_codes")):
            assert got.shape == one[key].shape
            assert np.array_equal(got, one[key]), f"chunk {chunk}: {name} differs from the one-shot call"
            assert np.array_equal(got, ora[key]), f"chunk {chunk}: {name} differs from the C oracle"
        if which == 0:
            assert pe["arena_bytes"] < one["plan_enc"]["arena_bytes"] and pd["arena_bytes"] < one["plan_dec"]["arena_bytes"]
    finally:
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)


def test_dac_small_chunked_n_quantizers_code_matrix_and_device_api(dac_small):
    import torch
    d = dac_small
    m, one, pcm = d["m"], d["one"], d["pcm"]
    m.set_chunk_frames(3 * d["h"]["align"])
    try:
        z2, codes2, lat2, _, _ = m.encode(pcm, n_quantizers=2)
        assert np.array_equal(codes2, one["codes2"]) and np.array_equal(z2, one["z2"]) and np.array_equal(lat2, one["lat2"])
        mat = m.encode_to_code_matrix(pcm)
        assert np.array_equal(mat, one["matrix"])
        assert np.array_equal(m.decode_code_matrix(one["matrix"]), one["matrix_audio"])
        # device-pointer entry points (torch tensors): the same chunked path without the per-chunk upload / download
        dev = torch.device("cuda", m.device_index)
        tz, tcodes, tlat, _, _ = m.encode(torch.from_numpy(pcm).to(dev))
        taudio = m.decode(torch.from_numpy(one["z"]).to(dev))
        tzf = m.from_codes(torch.from_numpy(one["codes"]).to(dev))
        tmat = m.encode_to_code_matrix(torch.from_numpy(pcm).to(dev))
        tma = m.decode_code_matrix(torch.from_numpy(one["matrix"]).to(dev))
        torch.cuda.synchronize()
        for got, key in ((tz, "z"), (tcodes, "codes"), (tlat, "lat"), (taudio, "audio"), (tzf, "from_codes"), (tmat, "matrix"), (tma, "matrix_audio")):
            assert np.array_equal(got.cpu().numpy(), one[key]), key
    finally:
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)


# ----------------------------------------------------------------------------------------------------------------------- SNAC
_SNAC = {}


def _snac_small(name):
    if name in _SNAC:
        return _SNAC[name]
    g = load_golden(name)
    cfg = snac_cfg_from_meta(g["meta"])
    blob = save_blob(snac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"]))
    h = snac_halo(cfg)
    frames = 6 * max(h[k] for k in FIELDS) + 5 * h["align"]
    T = frames * cfg.hop_length - 5                                   # Preprocess pads the last frame
    pcm = synthetic_pcm(B, 1, T, cfg.sampling_rate, seed=22)
    noises = snac_noise(cfg, B, frames, seed=23)
    m = SNAC(cfg)
    m.load_blob(blob)
    m.set_chunk_frames(_lib.NC_CHUNK_OFF)
    one = {}
    (one["codes"], one["z"], one["zq"]), one["n_enc"] = _launches(m, lambda: m.encode(pcm, return_latents=True))
    one["codes"] = [np.ascontiguousarray(c) for c in one["codes"]]
    one["audio"], one["n_dec"] = _launches(m, lambda: m.decode(one["codes"], noises))
    one["audio_seed"] = m.decode(one["codes"], None, seed=7)
    one["from_codes"] = m.from_codes(one["codes"])
    one["plan_enc"], one["plan_dec"] = m.chunk_plan(frames, False, B), m.chunk_plan(frames, True, B)
    ref = c_oracle.RefSNAC(cfg, blob)
    rz, rzq, rcodes = ref.encode(pcm)
    oracle = {"z": rz, "zq": rzq, "codes": rcodes, "audio": ref.decode(one["codes"], noises), "from_codes": ref.from_codes(one["codes"])}
    _SNAC[name] = dict(cfg=cfg, h=h, frames=frames, pcm=pcm, noises=noises, m=m, one=one, oracle=oracle)
    return _SNAC[name]


@pytest.mark.parametrize("name", ["snac_small", "snac_small_attn"])
def test_snac_one_shot_reference_matches_the_oracle(name):
    d = _snac_small(name)
    one, ora = d["one"], d["oracle"]
    assert one["plan_enc"]["n_chunks"] == 1 and one["plan_dec"]["n_chunks"] == 1
    for a, b in zip(one["codes"], ora["codes"]):
        assert np.array_equal(a, b)
    for k in ("z", "zq", "audio", "from_codes"):
        assert np.array_equal(one[k], ora[k]), k
    assert not np.array_equal(one["audio"], one["audio_seed"])


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("name", ["snac_small", "snac_small_attn"])
def test_snac_small_chunked_equals_one_shot_and_oracle(name, which):
    d = _snac_small(name)
    m, one, ora, frames, pcm, noises = d["m"], d["one"], d["oracle"], d["frames"], d["pcm"], d["noises"]
    chunk = _chunks(d["h"], frames)[which]
    m.set_chunk_frames(chunk)
    try:
        pe, pd = m.chunk_plan(frames, False, B), m.chunk_plan(frames, True, B)
        assert pe["n_chunks"] == pd["n_chunks"] == -(-frames // chunk) > 1
        (codes, z, zq), n_enc = _launches(m, lambda: m.encode(pcm, return_latents=True))
        audio, n_dec = _launches(m, lambda: m.decode(one["codes"], noises))
        audio_seed = m.decode(one["codes"], None, seed=7)
        zf = m.from_codes(one["codes"])
        assert n_enc > one["n_enc"] and n_dec > one["n_dec"]
        for i, (a, b, c) in enumerate(zip(codes, one["codes"], ora["codes"])):
            assert np.array_equal(a, b) and np.array_equal(a, c), f"chunk {chunk}: code level {i} differs"
        for nm, got, key in (("z", z, "z"), ("zq", zq, "zq"), ("decode", audio, "audio"), ("from_codes", zf, "from_codes")):
            assert np.array_equal(got, one[key]), f"chunk {chunk}: {nm} differs from the one-shot call"
            assert np.array_equal(got, ora[key]), f"chunk {chunk}: {nm} differs from the C oracle"
        assert np.array_equal(audio_seed, one["audio_seed"]), f"chunk {chunk}: decode with noise drawn from the seed differs"
        if which == 0:
            assert pe["arena_bytes"] < one["plan_enc"]["arena_bytes"] and pd["arena_bytes"] < one["plan_dec"]["arena_bytes"]
    finally:
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)


def test_snac_small_chunked_device_api():
    import torch
    d = _snac_small("snac_small_attn")
    m, one, pcm, noises = d["m"], d["one"], d["pcm"], d["noises"]
    m.set_chunk_frames(d["h"]["align"])
    try:
        dev = torch.device("cuda", m.device_index)
        codes, z, zq = m.encode(torch.from_numpy(pcm).to(dev), return_latents=True)
        tc = [torch.from_numpy(c).to(dev) for c in one["codes"]]
        audio = m.decode(tc, [torch.from_numpy(n).to(dev) for n in noises])
        audio_seed = m.decode(tc, None, seed=7)
        torch.cuda.synchronize()
        for a, b in zip(codes, one["codes"]):
            assert np.array_equal(a.cpu().numpy(), b)
        assert np.array_equal(z.cpu().numpy(), one["z"]) and np.array_equal(zq.cpu().numpy(), one["zq"])
        assert np.array_equal(audio.cpu().numpy(), one["audio"]) and np.array_equal(audio_seed.cpu().numpy(), one["audio_seed"])
    finally:
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)


# ------------------------------------------------------------------------------------ one staging path for host-pointer calls
# A host-pointer call that is not cut runs the window loop with the clip as its one window, on the same ck_* buffers as the chunked
# calls; a device-pointer call that is not cut is the launch sequence on the caller's arrays.  Same fixtures, np.array_equal only.
# Launches of the fixtures' one-shot encode / decode (profiled kernel classes) as counted on commit 3541718, the last one with the
# hand-written host staging: a clip that is one window launches no more.
PARENT_LAUNCHES = {"dac_small": (39, 30), "snac_small": (44, 44)}


def _modes(h):
    return [_lib.NC_CHUNK_OFF, 3 * h["align"], _lib.NC_CHUNK_AUTO, h["align"], _lib.NC_CHUNK_OFF]


def test_dac_host_encode_without_optional_outputs(dac_small):
    """z = NULL, latents = NULL: the merged path hands the launch sequence null where the hand-written branch handed it staging."""
    d = dac_small
    m, one, pcm = d["m"], d["one"], d["pcm"]
    codes = np.full_like(one["codes"], -1)
    _lib.check(_lib.lib().nc_dac_encode(m._h, pcm.ctypes.data, B, pcm.shape[-1], 0, 0, codes.ctypes.data, None, None))
    assert np.array_equal(codes, one["codes"])


def test_dac_one_handle_alternating_chunk_modes(dac_small):
    """OFF, 3 * align, AUTO, align, OFF on one handle: the shared window buffers only grow and keep no stale bytes."""
    d = dac_small
    m, one, pcm = d["m"], d["one"], d["pcm"]
    try:
        for setting in _modes(d["h"]):
            m.set_chunk_frames(setting)
            z, codes, lat, _, _ = m.encode(pcm)
            for got, key in ((z, "z"), (codes, "codes"), (lat, "lat"), (m.decode(one["z"]), "audio"), (m.from_codes(one["codes"]), "from_codes")):
                assert np.array_equal(got, one[key]), (setting, key)
    finally:
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)


def test_dac_one_shot_launch_counts_host_and_device(dac_small):
    """A one-shot host call launches what it launched before the host calls moved onto the window path (as does the fixture's), and the
    device-pointer one-shot call launches the same (the pitched-copy kernel is outside the profiler: equal counts are what the existing
    switches can show)."""
    import torch
    d = dac_small
    m, one, pcm = d["m"], d["one"], d["pcm"]
    (_, codes, _, _, _), n_enc = _launches(m, lambda: m.encode(pcm))
    audio, n_dec = _launches(m, lambda: m.decode(one["z"]))
    assert (n_enc, n_dec) == (one["n_enc"], one["n_dec"]) == PARENT_LAUNCHES["dac_small"]
    dev = torch.device("cuda", m.device_index)
    tp, tz = torch.from_numpy(pcm).to(dev), torch.from_numpy(one["z"]).to(dev)
    (_, tcodes, _, _, _), n_enc_dev = _launches(m, lambda: m.encode(tp))
    taudio, n_dec_dev = _launches(m, lambda: m.decode(tz))
    assert (n_enc_dev, n_dec_dev) == (n_enc, n_dec)
    assert np.array_equal(tcodes.cpu().numpy(), codes) and np.array_equal(taudio.cpu().numpy(), audio)


def test_snac_host_encode_without_optional_outputs():
    d = _snac_small("snac_small")
    m, one, pcm = d["m"], d["one"], d["pcm"]
    want = np.concatenate(one["codes"], axis=1)
    codes = np.full_like(want, -1)
    _lib.check(_lib.lib().nc_snac_encode(m._h, pcm.ctypes.data, B, pcm.shape[-1], codes.ctypes.data, None, None))
    assert np.array_equal(codes, want)


def test_snac_one_handle_alternating_chunk_modes():
    d = _snac_small("snac_small")
    m, one, pcm, noises = d["m"], d["one"], d["pcm"], d["noises"]
    try:
        for setting in _modes(d["h"]):
            m.set_chunk_frames(setting)
            codes, z, zq = m.encode(pcm, return_latents=True)
            for a, b in zip(codes, one["codes"]):
                assert np.array_equal(a, b), setting
            for got, key in ((z, "z"), (zq, "zq"), (m.decode(one["codes"], noises), "audio"), (m.decode(one["codes"], None, seed=7), "audio_seed")):
                assert np.array_equal(got, one[key]), (setting, key)
    finally:
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)


def test_snac_one_shot_launch_counts_host_and_device():
    import torch
    d = _snac_small("snac_small")
    m, one, pcm, noises = d["m"], d["one"], d["pcm"], d["noises"]
    codes, n_enc = _launches(m, lambda: m.encode(pcm))
    audio, n_dec = _launches(m, lambda: m.decode(one["codes"], noises))
    assert (n_enc, n_dec) == (one["n_enc"], one["n_dec"]) == PARENT_LAUNCHES["snac_small"]
    dev = torch.device("cuda", m.device_index)
    tp = torch.from_numpy(pcm).to(dev)
    tc, tn = [torch.from_numpy(c).to(dev) for c in one["codes"]], [torch.from_numpy(n).to(dev) for n in noises]
    tcodes, n_enc_dev = _launches(m, lambda: m.encode(tp))
    taudio, n_dec_dev = _launches(m, lambda: m.decode(tc, tn))
    assert (n_enc_dev, n_dec_dev) == (n_enc, n_dec)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(tcodes, codes)) and np.array_equal(taudio.cpu().numpy(), audio)


def test_snac_fixtures_are_released():
    for d in _SNAC.values():
        d["m"].dispose()
    _SNAC.clear()


# ---------------------------------------------------------------------------------------------------------- full-size instances
def test_dac44k_chunked_equals_one_shot():
    """Engine against itself: chunk-sized and clip-sized layers pick different conv instances here, so a mismatch means an instance is
    not position-independent -- a finding, not something a tolerance may cover."""
    cfg = DACConfig.dac_44khz()
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=3)))
        pcm = synthetic_pcm(1, 1, 3 * cfg.sample_rate, cfg.sample_rate, seed=31)
        frames = m.frames(pcm.shape[-1])
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        z, codes, lat, _, _ = m.encode(pcm)
        audio = m.decode(z)
        m.set_chunk_frames(64)
        assert m.chunk_plan(frames)["n_chunks"] == -(-frames // 64) > 1
        z2, codes2, lat2, _, _ = m.encode(pcm)
        audio2 = m.decode(z)
        assert np.array_equal(codes2, codes) and np.array_equal(z2, z) and np.array_equal(lat2, lat)
        assert np.array_equal(audio2, audio)


def test_snac44k_chunked_equals_one_shot():
    cfg = SNACConfig.snac_44khz()
    h = snac_halo(cfg)
    frames = 2 * max(h[k] for k in FIELDS) + 3 * h["align"]
    with SNAC(cfg) as m:
        m.load_blob(save_blob(snac_synthetic_state_dict(cfg, seed=4)))
        pcm = synthetic_pcm(1, 1, frames * cfg.hop_length, cfg.sampling_rate, seed=32)
        noises = snac_noise(cfg, 1, frames, seed=33)
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        codes, z, zq = m.encode(pcm, return_latents=True)
        codes = [np.ascontiguousarray(c) for c in codes]
        audio = m.decode(codes, noises)
        m.set_chunk_frames(h["align"])
        assert m.chunk_plan(frames)["n_chunks"] == frames // h["align"] > 1
        codes2, z2, zq2 = m.encode(pcm, return_latents=True)
        audio2 = m.decode(codes, noises)
        for a, b in zip(codes2, codes):
            assert np.array_equal(a, b)
        assert np.array_equal(z2, z) and np.array_equal(zq2, zq) and np.array_equal(audio2, audio)


# ------------------------------------------------------------------------------------------------------------ errors and AUTO
def test_error_conventions():
    with Encodec(EncodecConfig()) as e:
        with pytest.raises(_lib.NcError, match="status 6"):                               # NC_EUNSUPPORTED
            e.set_chunk_frames(64)
        with pytest.raises(_lib.NcError, match="status 6"):
            e.chunk_plan(100)
    with DAC(DACConfig()) as m:
        with pytest.raises(ValueError):
            m.set_chunk_frames(-2)
        with pytest.raises(ValueError):
            m.chunk_plan(0)
        with pytest.raises(ValueError):
            m.chunk_plan(-5, decode=True)
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        m.set_chunk_frames(_lib.NC_CHUNK_AUTO)


def test_auto_keeps_shipped_workloads_one_shot_and_chunks_what_one_shot_refuses():
    """Plans only: nothing is launched."""
    for cfg in (DACConfig.dac_44khz(), DACConfig.dac_24khz(), DACConfig.dac_16khz()):
        with DAC(cfg) as m:
            fr = m.frames(60 * cfg.sample_rate)
            for decode in (False, True):
                for b in (1, 32):
                    assert m.chunk_plan(fr, decode, b)["n_chunks"] == 1, (cfg.sample_rate, decode, b)
    for cfg in (SNACConfig.snac_24khz(), SNACConfig.snac_32khz(), SNACConfig.snac_44khz()):
        with SNAC(cfg) as m:
            fr = -(-60 * cfg.sampling_rate // cfg.hop_length)
            for decode in (False, True):
                assert m.chunk_plan(fr, decode, 32)["n_chunks"] == 1, (cfg.sampling_rate, decode)
    cfg = DACConfig.dac_44khz()
    with DAC(cfg) as m:
        fr = (1 << 30) // cfg.hop_length
        for decode in (False, True):
            p = m.chunk_plan(fr, decode, 1)
            assert p["n_chunks"] > 1 and p["n_chunks"] == -(-fr // p["chunk_frames"])
            assert 0 < p["arena_bytes"] < ARENA_BUDGET
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        assert m.chunk_plan(fr)["n_chunks"] == 1                                          # today's behaviour: the call itself refuses
