"""GPU suite: causal Encodec streams (nc_encodec_causal_pool_*) -- live 24 kHz-style streams encoded hop by hop and decoded frame by frame with
the LSTM's (h, c) carried.  Truth is the one-clip encode() / decode() on the whole stream (checked once against the C oracle): everything
a slot emits, laid end to end, must equal it bit for bit -- codes, the emb hook and PCM -- whatever the pushes were and whoever shared the
step."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import encodec_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import FLUSH, Encodec, _lib, encodec_causal_plan, ops  # noqa: E402
from neuralcodecs_amd.config import EncodecConfig  # noqa: E402
from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402
from oracle import c_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 48
T_CLIP = 41 * HOP + 123
_CACHE = {}


def enc_pushes(T, hop=HOP):
    sizes = [1, hop - 1, hop, hop + 1, 7 * hop + 5, 0]
    return sizes + [T - sum(sizes)]


def dec_pushes(F):
    sizes = [1, 1, 2, 7, 0]
    return sizes + [F - sum(sizes)]


def reference():
    """Computed once: the model, two clips, and per clip the one-clip call's codes, encoder output and PCM, checked against the C oracle."""
    if _CACHE:
        return _CACHE["ref"]
    g = load_golden("encodec_small24")
    cfg = encodec_cfg_from_meta(g["meta"])
    blob = save_blob(encodec_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"]))
    ref = c_oracle.RefEncodec(cfg, blob)
    clips = [synthetic_pcm(1, cfg.channels, T, cfg.sampling_rate, seed=4100 + i)[0] for i, T in enumerate([T_CLIP, 23 * HOP + 7, 9 * HOP, 30 * HOP + 47])]
    per = []
    with Encodec(cfg) as m:
        m.load_blob(blob)
        assert cfg.hop_length == HOP
        for x in clips:
            frames, embs = m.encode(x[None], return_emb=True)
            audio = m.decode(frames, x.shape[-1])
            (rc, _, re), = ref.encode(x[None], want_emb=True)
            assert np.array_equal(frames[0].codes, rc) and np.array_equal(embs[0], re)
            assert np.array_equal(audio, ref.decode([(rc, None)]))
            per.append((frames[0].codes, embs[0], audio[0]))
    _CACHE["ref"] = (cfg, blob, clips, per)
    return _CACHE["ref"]


def _model(cfg, blob):
    m = Encodec(cfg)
    m.load_blob(blob)
    return m


def run_encode_session(m, x, sizes):
    """-> (codes [1, n_q, F], emb [1, D, F]) of everything the session emitted"""
    cs, es, pos = [], [], 0
    with m.causal_encode_session() as s:
        for n in sizes:
            c, e = s.push(x[:, pos:pos + n], return_emb=True)
            pos += n
            assert s.pending() == pos - sum(a.shape[-1] for a in cs + [c]) * m.config.hop_length
            cs.append(c); es.append(e)
        c, e = s.flush(return_emb=True)
        assert s.pending() == 0
        cs.append(c); es.append(e)
    return np.concatenate(cs, -1), np.concatenate(es, -1)


def run_decode_session(m, codes, sizes, min_frames):
    outs, pos, hop = [], 0, m.config.hop_length
    with m.causal_decode_session() as s:
        for n in sizes:
            y = s.push(codes[:, :, pos:pos + n])
            pos += n
            outs.append(y)
            emitted = sum(o.shape[-1] for o in outs)
            assert emitted == (hop * pos if pos >= min_frames else 0)      # no latency once past the minimum window
            assert s.pending() == (0 if pos >= min_frames else pos)
        outs.append(s.flush())
    return np.concatenate(outs, -1)


def test_encode_session_equals_the_one_clip_call():
    cfg, blob, clips, per = reference()
    with _model(cfg, blob) as m:
        codes, emb = run_encode_session(m, clips[0], enc_pushes(T_CLIP))
    assert codes.dtype == np.int64 and np.array_equal(codes, per[0][0]) and np.array_equal(emb, per[0][1])


def test_decode_session_equals_the_one_clip_call():
    cfg, blob, clips, per = reference()
    info = encodec_causal_plan(cfg)[0]
    with _model(cfg, blob) as m:
        pcm = run_decode_session(m, per[0][0], dec_pushes(per[0][0].shape[-1]), info["min_frames_d"])
    assert np.array_equal(pcm, per[0][2])


def _cut(src, sizes):
    """the pushes of one stream: src cut along its last axis into pieces of `sizes` (cycled); the last piece carries the flush"""
    total, pos, i, out = src.shape[-1], 0, 0, []
    while pos < total:
        n = min(sizes[i % len(sizes)], total - pos)
        out.append(src[..., pos:pos + n])
        pos += n
        i += 1
    return out


def _run_pool(pool, streams, resets):
    """streams: (slot, first step, pushes, abandoned_after or None); resets: {step: slot} -- reset_slot before that step's entries.
    -> per stream the list of what the pool returned for each of its pushes"""
    got = [[] for _ in streams]
    batched = 0
    last = max(t0 + len(p) for _, t0, p, _ in streams)
    for step in range(last):
        if step in resets:
            pool.reset_slot(resets[step])
        entries, who = {}, {}
        for k, (slot, t0, pushes, stop) in enumerate(streams):
            i = step - t0
            if i < 0 or i >= len(pushes) or (stop is not None and i >= stop):
                continue
            assert slot not in entries
            entries[slot] = (pushes[i], FLUSH) if i == len(pushes) - 1 else pushes[i]
            who[slot] = k
        if not entries:
            continue
        lock = [list(entries).index(s) for s in (0, 1) if s in entries and not isinstance(entries[s], tuple)]
        if len(lock) == 2 and step >= 8:                       # slots 0 and 1 run in lock step: one batch, two rows of it
            _, rows = pool.plan(entries)
            mine = [r for r in rows if r["entry"] in lock]
            assert len(mine) == 2 and mine[0]["batch"] == mine[1]["batch"] and mine[0]["row"] != mine[1]["row"]
            batched += 1
        for slot, y in pool.step(entries).items():
            got[who[slot]].append(y)
    assert batched >= 3
    return got


def _run_session(sess, pushes, stop):
    out = []
    for i, x in enumerate(pushes if stop is None else pushes[:stop]):
        out.append(sess.flush(x) if i == len(pushes) - 1 else sess.push(x))
    return out


@pytest.mark.parametrize("decode", [False, True])
def test_pool_equals_sessions_and_batches_lock_step_entries(decode):
    """Five slots: 0 and 1 in lock step (one batch, asserted through plan), 2 idle for three steps, 3 at its own pace, 4 abandoned
    mid-stream, reset and reused for a second clip.  Every push of every slot returns what a single session returns for the same pushes,
    and every finished stream equals the one-clip call."""
    cfg, blob, clips, per = reference()
    if decode:
        src = [p[0] for p in per]                              # codes [1, n_q, F]
        want = [p[2] for p in per]
        cut = lambda ci, sizes: _cut(src[ci], sizes)  # noqa: E731
        streams = [(0, 0, cut(0, [1]), None), (1, 0, cut(0, [1]), None), (2, 3, cut(2, [4]), None), (3, 1, cut(3, [3, 1]), None),
                   (4, 0, cut(1, [2]), 6), (4, 9, cut(2, [5, 1]), None)]
    else:
        src = clips
        want = [p[0] for p in per]
        cut = lambda ci, sizes: _cut(src[ci], sizes)  # noqa: E731
        streams = [(0, 0, cut(0, [HOP]), None), (1, 0, cut(0, [HOP]), None), (2, 3, cut(2, [5 * HOP + 1, 17]), None),
                   (3, 1, cut(3, [2 * HOP - 1, 1]), None), (4, 0, cut(1, [HOP + 5]), 10), (4, 12, cut(2, [3 * HOP, 7]), None)]
    clip_of = [0, 0, 2, 3, 1, 2]
    with _model(cfg, blob) as m:
        make_pool = m.causal_decode_pool if decode else m.causal_encode_pool
        make_sess = m.causal_decode_session if decode else m.causal_encode_session
        with make_pool(5) as pool:
            got = _run_pool(pool, streams, {streams[5][1]: 4})
        for k, (slot, _, pushes, stop) in enumerate(streams):
            with make_sess() as sess:
                alone = _run_session(sess, pushes, stop)
            assert len(alone) == len(got[k])
            for i, (a, b) in enumerate(zip(alone, got[k])):
                assert a.shape == b.shape and np.array_equal(a, b), f"stream {k} (slot {slot}) push {i}"
            if stop is None:
                assert np.array_equal(np.concatenate(got[k], -1).reshape(want[clip_of[k]].shape), want[clip_of[k]]), f"stream {k} (slot {slot})"
            else:
                assert sum(g.shape[-1] for g in got[k]) > 0    # the abandoned stream had emitted before its slot was reset


def test_below_the_minimum():
    cfg, blob, clips, per = reference()
    info = encodec_causal_plan(cfg)[0]
    tiny = clips[0][:, :3 * HOP + 5]
    few = np.ascontiguousarray(per[0][0][:, :, :4])
    assert tiny.shape[-1] // HOP < info["min_frames_e"] and few.shape[-1] < info["min_frames_d"]
    with _model(cfg, blob) as m:
        want_c, want_e = m.encode(tiny[None], return_emb=True)
        want_p = c_oracle.RefEncodec(cfg, blob).decode([(few, None)])[0]       # (no clip length yields 4 frames: the oracle's DecodeFrame is the one-clip call)
        with m.causal_encode_session() as s:
            c = s.push(tiny)
            assert c.shape[-1] == 0 and s.pending() == tiny.shape[-1]
            c, e = s.flush(return_emb=True)
            assert np.array_equal(c, want_c[0].codes) and np.array_equal(e, want_e[0])
        with m.causal_decode_session() as s:
            y = s.push(few)
            assert y.shape[-1] == 0 and s.pending() == few.shape[-1]
            assert np.array_equal(s.flush(), want_p)
        # a stream too short for the one-clip call: the flush answers that call's error
        with pytest.raises(ValueError, match="segment too short") as one:
            m.encode(tiny[None, :, :2])
        with m.causal_encode_session() as s:
            with pytest.raises(ValueError, match="segment too short"):
                s.flush(tiny[:, :2])
            assert s.push(tiny[:, :2]).shape[-1] == 0                  # the refused flush left the slot as it was: it still takes pushes


@pytest.mark.parametrize("N", [1, 3])
def test_lstm_carried_hook(N):
    """T = 24 as splits (1, 5, 18) with carried state == the one-shot run == the oracle's LSTM (its tap elu(x + lstm(x)) on the tap before)."""
    cfg, blob, clips, per = reference()
    n_st = len(cfg.ratios)
    pcm = np.stack([clips[0][:, i * 211:i * 211 + 24 * HOP] for i in range(N)])
    taps = c_oracle.RefEncodec(cfg, blob).trace(pcm)
    x, want = taps[4 * n_st][0], taps[4 * n_st + 1][0]                 # the last down-convolution's output, the LSTM tap
    assert x.shape[0] == N and x.shape[-1] == 24
    with _model(cfg, blob) as m:
        y_all, st_all = ops.encodec_lstm_carried(m, x)
        parts, st, t0 = [], None, 0
        for n in (1, 5, 18):
            y, st = ops.encodec_lstm_carried(m, x[:, :, t0:t0 + n], st)
            parts.append(y)
            t0 += n
    assert np.array_equal(y_all, want)
    assert np.array_equal(np.concatenate(parts, -1), y_all)
    assert np.array_equal(st[0], st_all[0]) and np.array_equal(st[1], st_all[1])
    assert N == 1 or not np.array_equal(st[0][0], st[0][1])            # distinct state rows


@pytest.mark.parametrize("form", ["seq", "step"])
def test_against_both_one_clip_lstm_forms_in_child_processes(form, tmp_path):
    """The session tests in a fresh process whose one-clip calls take the persistent LSTM form (`lstm seq` in the launch log; encodec_small24
    has C = 64, which qualifies) and in one where NC_LSTM_STEPWISE=1 forces the step-wise form (`lstm step`).  The child
    asserts from its launch log which form its one-clip reference took, that the other never ran, and that the sessions ran `lstm carried`."""
    env = dict(os.environ, NC_LAUNCH_LOG=str(tmp_path / f"launch_{form}.log"))
    env.pop("NC_LSTM_STEPWISE", None)
    if form == "step":
        env["NC_LSTM_STEPWISE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_encodec_causal_child.py"), form], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_refusals_leave_the_slots_as_they_were():
    cfg, blob, clips, per = reference()
    g48 = load_golden("encodec_small48")
    cfg48 = encodec_cfg_from_meta(g48["meta"])
    with Encodec(cfg48) as m48:
        with pytest.raises(_lib.NcError, match="not causal"):             # NC_EUNSUPPORTED, naming the condition
            m48.causal_encode_pool(1)
    x = clips[1]
    with _model(cfg, blob) as m, m.causal_encode_pool(2) as p:
        import ctypes as C
        got = [p.step({0: x[:, :10 * HOP + 3]})[0]]
        L = _lib.lib()
        slots, n_in = (C.c_int32 * 2)(0, 0), _lib.i64_array([HOP, HOP])
        buf = np.zeros(2 * HOP, np.float32)
        out = np.zeros(64, np.int64)
        assert L.nc_encodec_causal_pool_step(p._p, 2, slots, n_in, None, buf.ctypes.data, out.ctypes.data, None, 64, None) == _lib.NC_EINVAL
        assert "named twice" in L.nc_last_error().decode()
        got.append(p.step({0: x[:, 10 * HOP + 3:12 * HOP]})[0])
        one = (C.c_int32 * 1)(0)
        nxt = np.ascontiguousarray(x[:, 12 * HOP:15 * HOP])
        assert L.nc_encodec_causal_pool_step(p._p, 1, one, _lib.i64_array([3 * HOP]), None, nxt.ctypes.data, out.ctypes.data, None, 1, None) == _lib.NC_EINVAL
        assert "out_cap" in L.nc_last_error().decode()
        got.append(p.step({0: nxt})[0])
        p.step({1: (x[:, :8 * HOP], FLUSH)})
        with pytest.raises(ValueError, match="slot 1 has been flushed"):
            p.step({0: x[:, 15 * HOP:16 * HOP], 1: x[:, :HOP]})
        got.append(p.step({0: (x[:, 15 * HOP:], FLUSH)})[0])
        assert np.array_equal(np.concatenate(got, -1), per[1][0])


def test_full_width_preset_once():
    """The 24 kHz preset, seeded weights: 1 s + 777 samples in 20 ms pieces through encode then decode sessions == the one-clip calls."""
    cfg = EncodecConfig()
    assert cfg.sampling_rate == 24000 and cfg.causal and cfg.hop_length == 320
    blob = save_blob(encodec_synthetic_state_dict(cfg, seed=24))
    x = synthetic_pcm(1, 1, 24000 + 777, 24000, seed=77)[0]
    piece = 480
    with _model(cfg, blob) as m:
        frames = m.encode(x[None])
        audio = m.decode(frames, x.shape[-1])[0]
        cs = []
        with m.causal_encode_session() as s:
            for p0 in range(0, x.shape[-1], piece):
                cs.append(s.push(x[:, p0:p0 + piece]))
            cs.append(s.flush())
        codes = np.concatenate(cs, -1)
        assert np.array_equal(codes, frames[0].codes)
        ys = []
        with m.causal_decode_session() as s:
            for c in cs:
                if c.shape[-1]:
                    ys.append(s.push(c))
            ys.append(s.flush())
        assert np.array_equal(np.concatenate(ys, -1), audio)
