"""CPU suite: nc_dac_halo / nc_snac_halo -- the closed-form halos of the long-clip (chunked) calls.

Shape properties on the small fixture configs and every shipped preset; sufficiency against the C oracle on the small configs: a
change of one input sample (one latent frame) must not move the encoder output (the PCM) outside the derived reach.  No upper cap is
asserted: the far edge of the true reach can fall below float32 resolution, so an observed reach is not a bound -- the closed form is
the specification."""
import dataclasses
from math import gcd

import numpy as np
import pytest

from conftest import dac_cfg_from_meta, load_golden, snac_cfg_from_meta
from neuralcodecs_amd import DACConfig, SNACConfig, dac_halo, snac_halo
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob, snac_noise, snac_synthetic_state_dict, synthetic_pcm
from oracle import c_oracle

FIELDS = ("enc_left", "enc_right", "dec_left", "dec_right")
STEP = 0.75   # "a large step" on PCM in [-1, 1] / on latents of order 1


def _small_dac():
    g = load_golden("dac_small")
    return dac_cfg_from_meta(g["meta"]), g["meta"]["weight_seed"]


def _small_snac(name):
    g = load_golden(name)
    return snac_cfg_from_meta(g["meta"]), g["meta"]["weight_seed"]


DAC_CFGS = {"dac_small": lambda: _small_dac()[0], "dac_44khz": DACConfig.dac_44khz, "dac_44khz_16kbps": DACConfig.dac_44khz_16kbps,
            "dac_24khz": DACConfig.dac_24khz, "dac_16khz": DACConfig.dac_16khz}
SNAC_CFGS = {"snac_small": lambda: _small_snac("snac_small")[0], "snac_small_attn": lambda: _small_snac("snac_small_attn")[0],
             "snac_24khz": SNACConfig.snac_24khz, "snac_32khz": SNACConfig.snac_32khz, "snac_44khz": SNACConfig.snac_44khz}


def _check_shape(h, align):
    assert h["align"] == align and align > 0
    for k in FIELDS:
        assert h[k] > 0 and h[k] % align == 0, (k, h)


@pytest.mark.parametrize("name", sorted(DAC_CFGS))
def test_dac_halo_shape_and_monotone(name):
    cfg = DAC_CFGS[name]()
    h = dac_halo(cfg)
    _check_shape(h, 1)
    # one more block (at the latent end of the encoder / the sample end of the decoder) never shrinks a halo
    # (a larger stride also lengthens the frame the halo is counted in, so nothing is claimed for it)
    more = dataclasses.replace(cfg, encoder_rates=tuple(cfg.encoder_rates) + (2,), decoder_rates=tuple(cfg.decoder_rates) + (2,),
                               latent_dim=cfg.resolved_latent_dim)
    ho = dac_halo(more)
    for k in FIELDS:
        assert ho[k] >= h[k], (k, h, ho)


@pytest.mark.parametrize("name", sorted(SNAC_CFGS))
def test_snac_halo_shape_and_monotone(name):
    cfg = SNAC_CFGS[name]()
    h = snac_halo(cfg)
    a, w = cfg.vq_strides[0], cfg.attn_window_size or 1
    _check_shape(h, a * w // gcd(a, w))
    more = dataclasses.replace(cfg, encoder_rates=tuple(cfg.encoder_rates) + (2,), decoder_rates=tuple(cfg.decoder_rates) + (2,),
                               latent_dim=cfg.resolved_latent_dim)
    ho = snac_halo(more)
    for k in FIELDS:
        assert ho[k] >= h[k], (k, h, ho)
    if cfg.attn_window_size:   # the attention window only widens the reach
        hn = snac_halo(dataclasses.replace(cfg, attn_window_size=None))
        for k in FIELDS:
            assert h[k] >= hn[k], (k, h, hn)


def test_halo_rejects_bad_configs():
    with pytest.raises(ValueError):
        dac_halo(dataclasses.replace(DACConfig(), encoder_rates=(2, 0, 8, 8)))
    with pytest.raises(ValueError):
        snac_halo(dataclasses.replace(SNACConfig(), vq_strides=(0, 2, 1)))


def _moved_frames(a, b):
    """frames (last axis) where two [B, C, T] arrays differ"""
    return np.nonzero(np.any(a != b, axis=(0, 1)))[0]


def _assert_within(moved, centre, left, right, what):
    assert moved.size, f"{what}: the change moved nothing (the probe is broken)"
    assert moved.min() >= centre - left and moved.max() <= centre + right, \
        f"{what}: moved frames {moved.min()}..{moved.max()} outside [{centre - left}, {centre + right}]"


def test_dac_small_halo_is_sufficient_against_the_oracle():
    cfg, seed = _small_dac()
    h = dac_halo(cfg)
    hop, halo = cfg.hop_length, max(h[k] for k in FIELDS)
    frames = (4 * halo + 9) * h["align"]
    ref = c_oracle.RefDAC(cfg, save_blob(dac_synthetic_state_dict(cfg, seed=seed)))
    pcm = synthetic_pcm(1, 1, frames * hop, cfg.sample_rate, seed=5)
    zq, codes, lat, ze = ref.encode(pcm)
    for x in (frames // 2 * hop, frames // 2 * hop + hop - 1):          # first / last sample of a mid-clip frame
        p2 = pcm.copy()
        p2[0, 0, x] += STEP
        zq2, codes2, lat2, ze2 = ref.encode(p2)
        for name, a, b in (("z_e", ze, ze2), ("latents", lat, lat2), ("z_q", zq, zq2), ("codes", codes, codes2)):
            if name == "codes" and not np.any(a != b):
                continue
            _assert_within(_moved_frames(a, b), x // hop, h["enc_left"], h["enc_right"], f"dac encoder {name} sample {x}")
    H = int(np.prod(cfg.decoder_rates))
    audio = ref.decode(zq)
    f = frames // 2
    z2 = zq.copy()
    z2[0, :, f] += STEP
    moved = np.unique(_moved_frames(audio, ref.decode(z2)) // H)
    _assert_within(moved, f, h["dec_left"], h["dec_right"], "dac decoder")


@pytest.mark.parametrize("name", ["snac_small", "snac_small_attn"])
def test_snac_small_halo_is_sufficient_against_the_oracle(name):
    cfg, seed = _small_snac(name)
    h = snac_halo(cfg)
    hop, halo, W = cfg.hop_length, max(h[k] for k in FIELDS), cfg.attn_window_size or 1
    frames = (4 * halo + 9) * h["align"]
    ref = c_oracle.RefSNAC(cfg, save_blob(snac_synthetic_state_dict(cfg, seed=seed)))
    pcm = synthetic_pcm(1, 1, frames * hop, cfg.sampling_rate, seed=6)
    z, zq, codes = ref.encode(pcm)
    w0 = frames // 2 // h["align"] * h["align"]                        # a mid-clip attention window / pooling block starts here
    probes = [w0 * hop, (w0 + W - 1) * hop + hop - 1] if W > 1 else [w0 * hop + 3, (w0 + 1) * hop - 1]
    for x in probes:                                                    # first / last position of the window
        p2 = pcm.copy()
        p2[0, 0, x] += STEP
        z2, zq2, codes2 = ref.encode(p2)
        _assert_within(_moved_frames(z, z2), x // hop, h["enc_left"], h["enc_right"], f"{name} encoder z sample {x}")
        if np.any(zq != zq2):
            _assert_within(_moved_frames(zq, zq2), x // hop, h["enc_left"], h["enc_right"], f"{name} encoder zq sample {x}")
        for s, c, c2 in zip(cfg.vq_strides, codes, codes2):
            d = np.nonzero(np.any(c != c2, axis=0))[0]
            if d.size:
                assert d.min() * s >= x // hop - h["enc_left"] and d.max() * s + s - 1 <= x // hop + h["enc_right"], (name, s, d)
    noises = snac_noise(cfg, 1, frames, seed=9)
    audio = ref.decode_latents(zq, noises)
    for f in ([w0, w0 + W - 1] if W > 1 else [w0]):
        q2 = zq.copy()
        q2[0, :, f] += STEP
        moved = np.unique(_moved_frames(audio, ref.decode_latents(q2, noises)) // hop)
        _assert_within(moved, f, h["dec_left"], h["dec_right"], f"{name} decoder frame {f}")
