"""GPU suite: the Encodec ragged calls (nc_encodec_{encode,decode}_ragged[_dev]) -- the segments of clips of unequal lengths pooled into
uniform batches.  Every clip's codes, scales, encoder output and decoded PCM must equal, bit for bit, the one-clip call on that clip and
the C oracle on that clip alone."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import encodec_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import Encodec, _lib, encodec_ragged_rows  # noqa: E402
from neuralcodecs_amd.config import EncodecConfig  # noqa: E402
from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402
from oracle import c_oracle  # noqa: E402

LENGTHS = {
    # shorter than a segment (own window) | one segment | an exact stride multiple | 40- and 30-sample tails (SConv1d's small-input path)
    # | shared 180-sample tails | duplicates | four segments
    "encodec_small48": [8100, 4000, 3990, 100, 9000, 8100, 47, 3960, 4140, 12000, 5000, 48],
    "encodec_small24": [3001, 3001, 1000, 48, 2999, 1000],
}
_CACHE = {}


def _model(name):
    g = load_golden(name)
    cfg = encodec_cfg_from_meta(g["meta"])
    blob = save_blob(encodec_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"]))
    m = Encodec(cfg)
    m.load_blob(blob)
    return cfg, blob, m


def _clips(cfg, lengths):
    return [synthetic_pcm(1, cfg.channels, T, cfg.sampling_rate, seed=1000 + 7 * i + T)[0] for i, T in enumerate(lengths)]


def _reference(name):
    """Per clip, computed once: the one-clip calls' frames, encoder outputs and PCM, each checked against the C oracle on that clip."""
    if name in _CACHE:
        return _CACHE[name]
    cfg, blob, m = _model(name)
    ref = c_oracle.RefEncodec(cfg, blob)
    clips = _clips(cfg, LENGTHS[name])
    per = []
    for x in clips:
        frames, embs = m.encode(x[None], return_emb=True)                       # (the one-clip call accepts every length of the list,
        audio = m.decode(frames, x.shape[-1])                                     #  4140 and 12000 included: it raises otherwise)
        rframes = ref.encode(x[None], want_emb=True)
        assert len(frames) == len(rframes)
        for f, e, (rc, rs, re) in zip(frames, embs, rframes):
            assert np.array_equal(f.codes, rc) and np.array_equal(e, re)
            assert rs is None or np.array_equal(f.scale, rs)
        assert np.array_equal(audio, ref.decode([(rc, rs) for rc, rs, _ in rframes]))
        per.append((frames, embs, audio[0]))
    m.dispose()
    _CACHE[name] = (cfg, blob, clips, per)
    return _CACHE[name]


def _same_frames(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.codes.dtype == np.int64 and a.codes.shape == b.codes.shape and np.array_equal(a.codes, b.codes)
        assert (a.scale is None) == (b.scale is None)
        if a.scale is not None:
            assert a.scale.shape == b.scale.shape and np.array_equal(a.scale, b.scale)


@pytest.mark.parametrize("max_rows", [2, 3, 0])
@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_ragged_equals_one_clip_calls_and_oracle(name, max_rows):
    cfg, blob, clips, per = _reference(name)
    lengths = LENGTHS[name]
    m = Encodec(cfg)
    m.load_blob(blob)
    m.set_ragged_rows(max_rows)
    for decode in (False, True):                                                  # the plan a handle reports is the config-only planner's
        assert m.ragged_rows(lengths, decode) == encodec_ragged_rows(cfg, lengths, decode, max_rows)
    if name == "encodec_small24":                                                 # the two pairs run as two-row batches
        _, rows = m.ragged_rows(lengths)
        sizes = {}
        for r in rows:
            sizes.setdefault(r["batch"], []).append(r["clip"])
        assert sorted(sizes.values()) == [[0, 1], [2, 5], [3], [4]]
    out, embs = m.encode_ragged(clips, return_emb=True)
    assert len(out) == len(clips)
    for b, (frames, es) in enumerate(zip(out, embs)):
        _same_frames(frames, per[b][0])
        assert len(es) == len(per[b][1]) and all(np.array_equal(a, e) for a, e in zip(es, per[b][1])), f"clip {b}: emb"
    audio = m.decode_ragged(out, lengths)
    for b, a in enumerate(audio):
        assert a.shape == per[b][2].shape and np.array_equal(a, per[b][2]), f"clip {b}: pcm"
    inferred = m.decode_ragged(out)                                               # lengths from the frames alone, as decode() infers them
    assert all(np.array_equal(a, c) for a, c in zip(inferred, audio))
    m.dispose()


def test_device_form_b1_and_no_stale_state():
    import torch
    cfg, blob, clips, per = _reference("encodec_small48")
    lengths = LENGTHS["encodec_small48"]
    m = Encodec(cfg)
    m.load_blob(blob)
    uni_pcm = synthetic_pcm(3, cfg.channels, 5000, cfg.sampling_rate, seed=1)
    uni_frames = m.encode(uni_pcm)
    uni_audio = m.decode(uni_frames, 5000)
    # host and device (torch tensor) forms agree
    dout = m.encode_ragged([torch.from_numpy(c).cuda() for c in clips])
    daudio = m.decode_ragged(dout, lengths)
    torch.cuda.synchronize()
    m.check_errors()
    for b in range(len(clips)):
        _same_frames([dataclasses.replace(f, codes=f.codes.cpu().numpy(), scale=None if f.scale is None else f.scale.cpu().numpy()) for f in dout[b]], per[b][0])
        assert np.array_equal(daudio[b].cpu().numpy(), per[b][2])
    # B = 1 equals the uniform call
    one = m.encode_ragged([clips[4]])
    _same_frames(one[0], per[4][0])
    assert np.array_equal(m.decode_ragged(one, [lengths[4]])[0], per[4][2])
    # a uniform call after ragged calls still gives its earlier result: no stale table state
    again = m.encode(uni_pcm)
    _same_frames(again, uni_frames)
    assert np.array_equal(m.decode(again, 5000), uni_audio)
    # after a bandwidth switch the packed sizes follow the new n_q
    m.set_target_bandwidth(3.0)
    nq = m.query(1)[1]
    sub = [clips[0], clips[3], clips[8]]
    low = m.encode_ragged(sub)
    plan, _ = m.ragged_rows([c.shape[-1] for c in sub])
    assert plan["total_codes"] == nq * plan["total_code_frames"] == sum(f.codes.size for fl in low for f in fl)
    for fl, x in zip(low, sub):
        want = m.encode(x[None])
        assert fl[0].codes.shape[1] == nq < per[0][0][0].codes.shape[1]
        _same_frames(fl, want)
    for a, fl, x in zip(m.decode_ragged(low, [c.shape[-1] for c in sub]), low, sub):
        assert np.array_equal(a, m.decode(fl, x.shape[-1])[0])
    m.dispose()


def test_refusals_name_the_clip_and_touch_nothing():
    cfg, blob, clips, per = _reference("encodec_small48")
    m = Encodec(cfg)
    m.load_blob(blob)
    with pytest.raises(ValueError):
        m.encode_ragged([])
    with pytest.raises(ValueError):
        m.encode_ragged([np.zeros((cfg.channels, 0), np.float32)])
    with pytest.raises(ValueError, match="max_rows"):
        m.set_ragged_rows(4097)
    # a batch holding a 1-sample clip: the one-clip call's answer, for the batch, with the clip's index, before anything is written
    with pytest.raises(ValueError, match="too short"):
        m.encode(np.zeros((1, cfg.channels, 1), np.float32))
    with pytest.raises(ValueError, match=r"clip 2: .*too short"):
        m.encode_ragged([clips[0], clips[3], np.zeros((cfg.channels, 1), np.float32), clips[1]])
    L = _lib.lib()
    lens = [100, 1, 4000]
    flat = np.zeros(cfg.channels * sum(lens), np.float32)
    sentinel = np.full(4096, -7, np.int64)
    scales = np.full(16, -7.0, np.float32)
    st = L.nc_encodec_encode_ragged(m._h, flat.ctypes.data, 3, _lib.i64_array(lens), sentinel.ctypes.data, scales.ctypes.data, None)
    assert st == _lib.NC_EINVAL and b"clip 1" in L.nc_last_error()
    assert np.all(sentinel == -7) and np.all(scales == -7.0)
    for args in ((None, 3, _lib.i64_array(lens), sentinel.ctypes.data), (flat.ctypes.data, 0, _lib.i64_array(lens), sentinel.ctypes.data),
                 (flat.ctypes.data, 3, None, sentinel.ctypes.data), (flat.ctypes.data, 3, _lib.i64_array(lens), None),
                 (flat.ctypes.data, 3, _lib.i64_array([100, 0, 4000]), sentinel.ctypes.data)):
        assert L.nc_encodec_encode_ragged(m._h, args[0], args[1], args[2], args[3], scales.ctypes.data, None) == _lib.NC_EINVAL
    assert np.all(sentinel == -7)
    # the window calls of DAC / SNAC keep refusing Encodec handles
    with pytest.raises(_lib.NcError):
        m.set_ragged_window(0, 0)
    # frames that do not match their clip's layout
    good = m.encode_ragged([clips[0], clips[1]])
    with pytest.raises(ValueError, match="clip 1"):
        m.decode_ragged(good, [8100, 8100])
    m.dispose()


def test_full_size_48khz():
    """encodec_48khz, stereo, 12 kbps: half a second, 1.3 s and 2 s -- the persistent LSTM, the aligned streaming kernels and the
    960-sample tail of a 2 s clip; 62000 leaves a 14480-sample tail."""
    cfg = dataclasses.replace(EncodecConfig.encodec_48khz(), bandwidth=12.0)
    blob = save_blob(encodec_synthetic_state_dict(cfg, seed=42))
    lengths = [24000, 62000, 96000]
    clips = _clips(cfg, lengths)
    with Encodec(cfg) as m:
        m.load_blob(blob)
        out = m.encode_ragged(clips)
        audio = m.decode_ragged(out, lengths)
        for b, x in enumerate(clips):
            want = m.encode(x[None])
            _same_frames(out[b], want)
            assert np.array_equal(audio[b], m.decode(want, lengths[b])[0])
        assert m.lstm_stats() == (False, 0)
    ref = c_oracle.RefEncodec(cfg, blob)
    rframes = ref.encode(clips[0][None])
    for f, (rc, rs) in zip(out[0], rframes):
        assert np.array_equal(f.codes, rc) and np.array_equal(f.scale, rs)
    assert np.array_equal(audio[0], ref.decode(rframes)[0])
