"""CPU suite: the planner of the causal Encodec streams (nc_encodec_causal_plan, host arithmetic) -- its closed forms against a brute-force
dependency model, the schedule invariants over random push schedules, the causality of the judge (the C oracle), and the refusals."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from conftest import encodec_cfg_from_meta, load_golden
from neuralcodecs_amd import _lib, encodec_causal_plan
from neuralcodecs_amd.config import EncodecConfig
from neuralcodecs_amd.encodec import _c_config
from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob, synthetic_pcm
from oracle import c_oracle

CFGS = {"encodec_small24": lambda: encodec_cfg_from_meta(load_golden("encodec_small24")["meta"]), "preset24": lambda: EncodecConfig()}


# ---- brute force: which outputs of a window can its left edge (or its own left reflect pad) reach --------------------------------------
def _conv(t, L, k, s):
    """a causal convolution on L inputs of which the set t is reached: (reached outputs, L_out); no extra right pad (L % s == 0)"""
    pad = k - s
    out = set()
    for j in range(L // s):
        idx = range(j * s - pad, j * s + s)
        if any(i < 0 or i in t for i in idx):                           # a padded position (the window's own reflect pad) or a reached input
            out.add(j)
    return out, L // s


def _convT(t, L, K, s):
    """a transposed convolution trimmed by K - s on the right; on a window that starts inside the stream input -1 is missing"""
    out = set()
    for p in range(L * s):
        lo = -(-(p - K + 1) // s)
        if any(i < 0 or i in t for i in range(lo, p // s + 1)):
            out.add(p)
    return out, L * s


def brute_encoder(cfg, frames):
    L = frames * cfg.hop_length
    t, L = _conv(set(), L, cfg.kernel_size, 1)
    for r in reversed(cfg.ratios):
        t, L = _conv(t, L, cfg.residual_kernel_size, 1)
        t, L = _conv(t, L, 2 * r, r)
    assert L == frames
    return t


def brute_decoder(cfg, frames):
    t, L = set(), frames
    for r in cfg.ratios:
        t, L = _convT(t, L, 2 * r, r)
        t, L = _conv(t, L, cfg.residual_kernel_size, 1)
    t, L = _conv(t, L, cfg.last_kernel_size, 1)
    assert L == frames * cfg.hop_length
    return t


def _small_input(L, k, s):
    """SConv1d's pad plan on a causal row of L inputs (SConv1d.cs:245-274): (takes the small-input path, L_out)"""
    pt = k - s
    nf = np.float32(L - k + pt) / np.float32(s) + np.float32(1.0)
    extra = (int(np.ceil(nf)) - 1) * s + (k - pt) - L
    return L <= max(pt, extra), (L + pt + extra - k) // s + 1


def takes_small_input_path(cfg, frames, decode):
    """does any layer of the one-clip call on `frames` frames (encode: frames * hop samples) zero-extend its row?"""
    hit = False
    if not decode:
        L = frames * cfg.hop_length
        plan = [(cfg.kernel_size, 1)] + [p for r in reversed(cfg.ratios) for p in ((cfg.residual_kernel_size, 1), (2 * r, r))] + [(cfg.last_kernel_size, 1)]
        for k, s in plan:
            d9, L = _small_input(L, k, s)
            hit = hit or d9
        return hit
    d9, L = _small_input(frames, cfg.kernel_size, 1)
    hit = d9
    for r in cfg.ratios:
        d9, L = _small_input(L * r, cfg.residual_kernel_size, 1)
        hit = hit or d9
    return hit or _small_input(L, cfg.last_kernel_size, 1)[0]


@pytest.mark.parametrize("name", sorted(CFGS))
def test_closed_forms_against_the_dependency_model(name):
    cfg = CFGS[name]()
    info = encodec_causal_plan(cfg)[0]
    hop = cfg.hop_length
    assert info["hop"] == hop
    te = brute_encoder(cfg, info["halo_e"] + 6)
    assert te == set(range(len(te)))                                      # a prefix: everything behind it is the one-clip call's
    # sufficient and necessary: exactly halo_e leading frames are reached, so dropping one less leaves frame halo_e - 1 in the output
    assert len(te) == info["taint_e"] == info["halo_e"] and info["halo_e"] - 1 in te
    td = brute_decoder(cfg, info["halo_d"] + 3)
    assert td == set(range(len(td))) and len(td) == info["taint_d"]
    assert info["halo_d"] * hop >= len(td) > (info["halo_d"] - 1) * hop   # sufficient, and one frame less is not
    # minimum first window, against the pad plans: at the minimum no layer of the one-clip call takes SConv1d's small-input path, one
    # frame less and some layer does (the k-tap stride-1 convolutions at frame rate: their left pad k - 1 is not shorter than the row)
    for decode, key in ((False, "min_frames_e"), (True, "min_frames_d")):
        assert not takes_small_input_path(cfg, info[key], decode) and not takes_small_input_path(cfg, info[key] + 1, decode)
        assert takes_small_input_path(cfg, info[key] - 1, decode)
    assert info["carry_e"] == cfg.last_kernel_size - 1 and info["carry_d"] == max(cfg.kernel_size - 1, info["min_frames_d"] - 1)
    if name == "preset24":
        assert (info["halo_e"], info["halo_d"], info["taint_d"], info["min_frames_e"], info["min_frames_d"]) == (2, 2, 478, 7, 7)


@pytest.mark.parametrize("decode", [False, True])
def test_schedule_invariants(decode):
    cfg = CFGS["encodec_small24"]()
    info = encodec_causal_plan(cfg)[0]
    hop, mn = cfg.hop_length, info["min_frames_d" if decode else "min_frames_e"]
    rng = np.random.default_rng(11 + decode)
    for trial in range(150):
        total = int(rng.integers(1, 40 if decode else 40 * hop))
        T = E = 0
        out = 0
        while True:
            n = int(min(total - T, rng.choice([0, 1, 2, 5, 9] if decode else [0, 1, hop - 1, hop, hop + 1, 3 * hop + 7, 11 * hop])))
            flush = T + n == total and (n == 0 or bool(rng.integers(0, 2)))
            try:
                _, nb, rows, n_out = encodec_causal_plan(cfg, [T], [E], [n], [flush], decode=decode)
            except ValueError as err:                                     # a flush below the minimum answers what the one-clip call answers
                assert flush and E == 0 and (T + n) // hop < mn and "segment too short" in str(err)
                break
            T += n
            frames = T if decode else T // hop
            new = rows[0]["new_frames"] if rows else 0
            if flush:                                                     # everything that remains, whatever the minimum
                want_total = T if decode else -(-T // hop)
                if rows and rows[0]["one_clip"]:
                    assert E == 0 and frames < mn
                else:
                    assert E + new == want_total
                    assert n_out[0] == (new * hop if decode else new)
                out += n_out[0]
                if not (rows and rows[0]["one_clip"]):
                    assert out == (total * hop if decode else -(-total // hop))   # every frame | sample exactly once
                break
            want_E = frames if frames >= mn else 0
            assert E + new == want_E and nb == len(rows) <= 1             # every frame exactly once, in order
            assert n_out[0] == (new * hop if decode else new)
            if rows:
                r = rows[0]
                first = E == 0
                if decode:
                    assert (r["start"], r["width"]) == ((0, T) if first else (T - n - info["carry_d"], info["carry_d"] + n))
                else:
                    start = 0 if first else (E - info["halo_e"]) * hop
                    assert (r["start"], r["width"]) == (start, frames * hop - start) and start >= 0
            E = want_E
            out += n_out[0]
            pending = (T - E) if decode else (T - E * hop)
            assert 0 <= pending < (mn if decode else max(mn, 1) * hop)


def test_lock_step_entries_share_a_batch():
    cfg = CFGS["encodec_small24"]()
    hop = cfg.hop_length
    _, nb, rows, n_out = encodec_causal_plan(cfg, [9 * hop] * 3 + [0, 20 * hop + 5], [9, 9, 9, 0, 20], [hop, hop, hop, 8 * hop, 2 * hop], None)
    assert nb == 3 and n_out == [1, 1, 1, 8, 2]
    assert len({r["batch"] for r in rows if r["entry"] < 3}) == 1 and sorted(r["row"] for r in rows if r["entry"] < 3) == [0, 1, 2]
    widths = [r["width"] for r in rows]
    assert widths == sorted(widths, reverse=True)                        # keys in descending order
    _, nb, rows, _ = encodec_causal_plan(cfg, [9 * hop] * 3, [9, 9, 9], [hop] * 3, None, max_rows=2)
    assert nb == 2                                                       # at most max_rows rows per batch


def test_the_judge_is_causal():
    """encode(x[:k*hop]) == the first k frames of encode(x) and decode(codes[:, :k]) == the first k*hop samples of decode(codes), bit for
    bit, on the C oracle: the premise of the whole path."""
    g = load_golden("encodec_small24")
    cfg = encodec_cfg_from_meta(g["meta"])
    blob = save_blob(encodec_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"]))
    ref = c_oracle.RefEncodec(cfg, blob)
    hop = cfg.hop_length
    x = synthetic_pcm(1, cfg.channels, 30 * hop + 17, cfg.sampling_rate, seed=5)
    (codes, _, emb), = ref.encode(x, want_emb=True)
    pcm = ref.decode([(codes, None)])
    for k in (7, 8, 19, 30):
        (ck, _, ek), = ref.encode(x[:, :, :k * hop], want_emb=True)
        assert np.array_equal(ck, codes[:, :, :k]) and np.array_equal(ek, emb[:, :, :k])
        assert np.array_equal(ref.decode([(np.ascontiguousarray(codes[:, :, :k]), None)]), pcm[:, :, :k * hop])


def test_refusals_of_the_bare_export():
    L = _lib.lib()
    cfg = CFGS["encodec_small24"]()
    c = _c_config(cfg)
    one, zero = _lib.i64_array([1]), _lib.i64_array([0])
    n_out = (C.c_int64 * 1)()
    call = lambda cc, n, r=zero, e=zero, ni=one: L.nc_encodec_causal_plan(cc, 0, n, r, e, ni, None, 0, None, None, 0, None, None, n_out)  # noqa: E731
    assert call(C.byref(c), 1) == _lib.NC_OK
    assert call(None, 1) == _lib.NC_EINVAL
    assert call(C.byref(c), 1, None) == _lib.NC_EINVAL and call(C.byref(c), 1, zero, None) == _lib.NC_EINVAL
    assert call(C.byref(c), 1, zero, zero, None) == _lib.NC_EINVAL
    assert call(C.byref(c), 0) == _lib.NC_EINVAL and call(C.byref(c), -3) == _lib.NC_EINVAL
    assert call(C.byref(c), 1, zero, one) == _lib.NC_EINVAL             # a stream that has received nothing has emitted nothing
    unsupported = _lib.NC_EUNSUPPORTED
    for change, word in ((dict(segment_seconds=0.25), "segmented"), (dict(normalize=True), "normalises"), (dict(causal=False), "not causal"),
                         (dict(norm="time_group_norm", causal=False), "not causal")):
        bad = _c_config(dataclasses.replace(cfg, **change))
        assert call(C.byref(bad), 1) == unsupported
        assert word in L.nc_last_error().decode()
    bad = _c_config(cfg)
    bad.time_group_norm = 1                                              # causal + time_group_norm is no Encodec config at all (NormConv1d.cs:143-147)
    assert call(C.byref(bad), 1) == _lib.NC_EINVAL and "GroupNorm" in L.nc_last_error().decode()
