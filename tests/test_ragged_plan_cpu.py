"""CPU suite: nc_dac_ragged_windows / nc_snac_ragged_windows -- the window layout of the ragged (unequal-length) batch calls.

Host functions on a config alone, no device.  Small fixture configs and the 44.1 kHz presets, both directions; seeded random frame lists
that always hold F < W, F == W, F == W + align and F >> W; kept widths C in {align, 3 * align, max_halo + align}."""
import numpy as np
import pytest

from conftest import dac_cfg_from_meta, load_golden, snac_cfg_from_meta
from neuralcodecs_amd import DACConfig, SNACConfig, dac_halo, dac_ragged_windows, snac_halo, snac_ragged_windows

FIELDS = ("enc_left", "enc_right", "dec_left", "dec_right")
CFGS = {
    "dac_small": (lambda: dac_cfg_from_meta(load_golden("dac_small")["meta"]), dac_halo, dac_ragged_windows),
    "dac_44khz": (DACConfig.dac_44khz, dac_halo, dac_ragged_windows),
    "snac_small": (lambda: snac_cfg_from_meta(load_golden("snac_small")["meta"]), snac_halo, snac_ragged_windows),
    "snac_small_attn": (lambda: snac_cfg_from_meta(load_golden("snac_small_attn")["meta"]), snac_halo, snac_ragged_windows),
    "snac_44khz": (SNACConfig.snac_44khz, snac_halo, snac_ragged_windows),
}
MAX_WINDOWS = 5


def _halos(h, decode):
    """halo_left / halo_right as the chunk planner assigns them: a window needs to its left what a change reaches to its right"""
    return (h["dec_right"], h["dec_left"]) if decode else (h["enc_right"], h["enc_left"])


def _kept_widths(h):
    a = h["align"]
    return [a, 3 * a, max(h[k] for k in FIELDS) + a]


def _frames(h, decode, C, seed):
    a = h["align"]
    hl, hr = _halos(h, decode)
    W = C + hl + hr
    rng = np.random.default_rng(seed)
    short = [int(rng.integers(1, W // a)) * a for _ in range(3)] if W > a else []
    fixed = [W, W + a, 40 * W + 3 * a] + ([W - a] if W > a else [])
    mid = [W + int(rng.integers(1, 6 * W // a)) * a for _ in range(4)]
    fr = short + short[:1] + fixed + mid                       # short[:1] again: a group of two clips
    return [fr[i] for i in rng.permutation(len(fr))], W


@pytest.mark.parametrize("decode", [False, True])
@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("name", sorted(CFGS))
def test_window_layout(name, which, decode):
    make, halo, windows = CFGS[name]
    cfg = make()
    h = halo(cfg)
    a = h["align"]
    C = _kept_widths(h)[which]
    hl, hr = _halos(h, decode)
    frames, W = _frames(h, decode, C, seed=which)
    plan, rows = windows(cfg, frames, decode, C, MAX_WINDOWS)
    assert (plan["window_frames"], plan["kept_frames"], plan["halo_left"], plan["halo_right"]) == (W, C, hl, hr)
    assert plan["n_rows"] == len(rows) and plan["total_frames"] == sum(frames)
    kept = [np.zeros(f, np.int32) for f in frames]
    per_batch = {}
    for r in rows:
        F = frames[r["clip"]]
        per_batch.setdefault(r["batch"], []).append(r)
        assert r["start"] % a == 0 and r["width"] % a == 0 and r["keep_start"] % a == 0 and r["keep_frames"] % a == 0
        assert 0 <= r["start"] and r["start"] + r["width"] <= F                                   # lies inside the clip
        k0, k1 = r["keep_start"], r["keep_start"] + r["keep_frames"]
        assert r["start"] <= k0 < k1 <= r["start"] + r["width"]
        kept[r["clip"]][k0:k1] += 1
        if F >= W:
            assert r["width"] == W                                                                   # every window of a long clip is exactly W wide
            if r["start"] > 0:
                assert k0 - r["start"] >= hl                                                         # clear of the interior left edge
            if r["start"] + W < F:
                assert r["start"] + W - k1 >= hr                                                     # clear of the interior right edge
        else:
            assert (r["start"], r["width"], k0, k1) == (0, F, 0, F)                                # a short clip is not cut
    for b, k in enumerate(kept):
        assert np.all(k == 1), f"clip {b} ({frames[b]} frames): a frame is kept {k.min()}..{k.max()} times"
    long_clips = [f for f in frames if f >= W]
    n_windows = sum(1 + -(-(f - W) // C) for f in long_clips)
    assert plan["n_windows"] == n_windows == sum(1 for r in rows if frames[r["clip"]] >= W)
    assert plan["n_window_batches"] == -(-n_windows // MAX_WINDOWS)
    assert plan["n_batches"] == len(per_batch)
    for bi, rs in per_batch.items():
        assert len(rs) <= MAX_WINDOWS                                                                # no batch exceeds max_windows
        assert len({r["width"] for r in rs}) == 1                                                    # a batch is uniform
        if rs[0]["width"] < W:                                                                       # short clips: grouped by exact length
            assert len({frames[r["clip"]] for r in rs}) == 1
    short = [f for f in frames if f < W]
    assert plan["n_exact_groups"] == len(set(short))
    for f in set(short):                                                                             # one group, split only by max_windows
        batches = {r["batch"] for r in rows if frames[r["clip"]] == f}
        assert len(batches) == -(-short.count(f) // MAX_WINDOWS)
    # first window left-aligned, last right-aligned: both outer edges are true clip edges
    for b, F in enumerate(frames):
        mine = [r for r in rows if r["clip"] == b]
        assert min(r["start"] for r in mine) == 0 and max(r["start"] + r["width"] for r in mine) == F


@pytest.mark.parametrize("name", sorted(CFGS))
def test_arena_is_independent_of_batch_size_and_clip_length(name):
    make, halo, windows = CFGS[name]
    cfg = make()
    h = halo(cfg)
    a, C = h["align"], 3 * h["align"]
    for decode in (False, True):
        hl, hr = _halos(h, decode)
        W = C + hl + hr
        base, _ = windows(cfg, [W, 2 * W], decode, C, MAX_WINDOWS)
        more, _ = windows(cfg, [W, 2 * W] * 20 + [a], decode, C, MAX_WINDOWS)
        longer, _ = windows(cfg, [W, 1000 * W + a], decode, C, MAX_WINDOWS)
        assert 0 < base["arena_bytes"] == more["arena_bytes"] == longer["arena_bytes"]
        wider, _ = windows(cfg, [W, 2 * W], decode, C, 2 * MAX_WINDOWS)
        assert wider["arena_bytes"] == 2 * base["arena_bytes"]                                      # it is max_windows x W


def test_defaults_totals_and_refusals():
    cfg = DACConfig.dac_44khz()
    plan, rows = dac_ragged_windows(cfg, [100, 1000, 1000, 7])
    assert plan["kept_frames"] == 128 and plan["window_frames"] == 128 + plan["halo_left"] + plan["halo_right"]
    assert plan["n_exact_groups"] == 2 and plan["total_codes"] == cfg.n_codebooks * 2107
    assert plan["total_samples"] == 2107 * cfg.hop_length
    s = SNACConfig.snac_44khz()
    a = snac_halo(s)["align"]
    plan, _ = snac_ragged_windows(s, [a, 5 * a], decode=True)
    assert plan["kept_frames"] == 256
    assert plan["total_codes"] == sum(6 * a // v for v in s.vq_strides) and plan["total_samples"] == 6 * a * s.hop_length
    with pytest.raises(ValueError):
        snac_ragged_windows(s, [a + 1])                                                              # not whole pooling blocks / attention windows
    for bad in ([], [0], [5, -1]):
        with pytest.raises(ValueError):
            dac_ragged_windows(cfg, bad)
    with pytest.raises(ValueError):
        dac_ragged_windows(cfg, [5], kept_frames=-1)
