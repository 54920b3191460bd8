"""GPU suite: the Encodec stream pool (nc_encodec_stream_pool_*) -- live streams encoded segment by segment as their PCM arrives and decoded
frame by frame.  Truth is the one-clip encode() / decode() on the whole stream (checked once per clip against the C oracle): everything a
slot emits, laid end to end, must equal it bit for bit -- codes, scales, encoder output and PCM -- whatever the pushes were, whoever
shared the step, and equally for a one-slot pool fed the same pushes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import encodec_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import FLUSH, Encodec, _lib  # noqa: E402
from neuralcodecs_amd.config import EncodecConfig  # noqa: E402
from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402
from oracle import c_oracle  # noqa: E402

SEG, STRIDE, HOP = 4000, 3960, 48
F_FULL = -(-SEG // HOP)
# shorter than a segment (own window) twice | a full segment and a 40-sample tail | an exact stride multiple | a full segment and a
# 180-sample tail | full + short 3990 + 30: two short tails | four segments
LENGTHS = [47, 100, 4000, 3960, 4140, 7950, 12000]
# per stream: idle steps before it starts, sizes of its pushes (cycled), whether the flush carries the last push
PUSHES = [
    (0, [47], True),                                   # a flush-only stream
    (2, [30], False),                                  # pushes that complete nothing; the flush comes alone
    (0, [SEG], False),                                 # a push that lands exactly on a segment end
    (1, [STRIDE - 3, 1, 1, 1], True),                  # an exact stride multiple, the last samples one by one; the flush carries the last
    (3, [SEG - 2, 1, 1, 1, 1, 200], False),            # single-sample pushes across a segment end
    (0, [1 << 20], True),                              # everything in the flush: three rows of three different keys
    (1, [2 * STRIDE + SEG + 5, 1000], False),          # one push completes three segments
]
_CACHE = {}


def _model(cfg, blob, max_rows=0):
    m = Encodec(cfg)
    m.load_blob(blob)
    m.set_ragged_rows(max_rows)
    return m


def _reference():
    """Per clip, computed once: the one-clip calls' frames, encoder outputs and PCM, each checked against the C oracle on that clip."""
    if _CACHE:
        return _CACHE["ref"]
    g = load_golden("encodec_small48")
    cfg = encodec_cfg_from_meta(g["meta"])
    blob = save_blob(encodec_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"]))
    ref = c_oracle.RefEncodec(cfg, blob)
    clips = [synthetic_pcm(1, cfg.channels, T, cfg.sampling_rate, seed=2000 + 7 * i + T)[0] for i, T in enumerate(LENGTHS)]
    per = []
    with _model(cfg, blob) as m:
        assert (m.segment_length, m.segment_stride, cfg.hop_length) == (SEG, STRIDE, HOP)
        for x in clips:
            frames, embs = m.encode(x[None], return_emb=True)                     # (the one-clip call accepts every length of the list: it raises otherwise)
            audio = m.decode(frames, x.shape[-1])
            rframes = ref.encode(x[None], want_emb=True)
            assert len(frames) == len(rframes)
            for f, e, (rc, rs, re) in zip(frames, embs, rframes):
                assert np.array_equal(f.codes, rc) and np.array_equal(e, re)
                assert rs is None or np.array_equal(f.scale, rs)
            assert np.array_equal(audio, ref.decode([(rc, rs) for rc, rs, _ in rframes]))
            per.append((frames, embs, audio[0]))
    _CACHE["ref"] = (cfg, blob, clips, per)
    return _CACHE["ref"]


def _np(a):
    return np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)


def _same_frames(got, want, what=""):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        ac = _np(a.codes)
        assert ac.dtype == np.int64 and ac.shape == b.codes.shape and np.array_equal(ac, b.codes), what
        assert (a.scale is None) == (b.scale is None)
        if a.scale is not None:
            assert np.array_equal(_np(a.scale).reshape(b.scale.shape), b.scale), what


def _encode_steps(x, delay, sizes, with_last):
    """the steps of one stream: None = idle, else the value of its entry"""
    T, pos, i, steps = x.shape[-1], 0, 0, [None] * delay
    while pos < T:
        n = min(T - pos, sizes[i % len(sizes)])
        steps.append(x[:, pos:pos + n])
        pos += n
        i += 1
    if with_last:
        steps[-1] = (steps[-1], FLUSH)
    else:
        steps.append(FLUSH)
    return steps


def _decode_steps(frames, delay, chunk, with_last):
    """full frames in pushes of `chunk`; the last two frames (the ones that may be short) come with the flush -- or, with_last == False,
    a full-length one among them comes before it and the flush brings the rest"""
    full, tail = list(frames[:-2]), list(frames[-2:])
    steps = [None] * delay + [full[i:i + chunk] for i in range(0, len(full), chunk)]
    if not with_last and len(tail) == 2 and tail[0].codes.shape[-1] == F_FULL:
        steps.append([tail.pop(0)])
    steps.append((tail, FLUSH))
    return steps


def _run(pool, streams, slots, wrap=lambda v: v, **kw):
    """streams[i]: the steps of the stream in slot slots[i] -> per stream everything its slot emitted, in order"""
    got = [[] for _ in streams]
    for t in range(max(len(s) for s in streams)):
        entries = {slots[i]: wrap(s[t]) for i, s in enumerate(streams) if t < len(s) and s[t] is not None}
        if not entries:
            continue
        out = pool.step(entries, **kw)
        for i, s in enumerate(slots):
            if s in entries:
                got[i].append(out[s] if not isinstance(out, tuple) else (out[0][s], out[1][s]))
    return got


def _check_encode(got, per, b, what):
    frames = [f for step in got for f in step[0]]
    embs = [e for step in got for e in step[1]]
    _same_frames(frames, per[b][0], what)
    assert len(embs) == len(per[b][1]) and all(np.array_equal(_np(a), e) for a, e in zip(embs, per[b][1])), f"{what}: emb"


def _check_decode(got, per, b, what):
    pcm = np.concatenate([_np(p) for p in got], axis=-1)
    assert pcm.shape == per[b][2].shape and np.array_equal(pcm, per[b][2]), f"{what}: pcm"


@pytest.mark.parametrize("max_rows", [2, 0])
def test_staggered_streams_equal_the_one_clip_call_and_a_one_slot_pool(max_rows):
    cfg, blob, clips, per = _reference()
    n = len(LENGTHS)
    slots = [5, 0, 6, 2, 7, 1, 3]                                                   # (slot 4 stays unused)
    with _model(cfg, blob, max_rows) as m:
        enc = [_encode_steps(x, *PUSHES[b]) for b, x in enumerate(clips)]
        with m.encode_pool(8) as pool:
            got = _run(pool, enc, slots, return_emb=True)
            assert all(pool.pending(s) == 0 for s in range(8))
        for b in range(n):
            _check_encode(got[b], per, b, f"encode, clip {b}")
            with m.encode_pool(1) as one:                                           # the same pushes, alone
                alone = _run(one, [enc[b]], [0], return_emb=True)[0]
            assert len(alone) == len(got[b])
            for a, g in zip(alone, got[b]):                                         # step by step the same pieces
                _same_frames(a[0], g[0], f"one-slot pool, clip {b}")
                assert all(np.array_equal(x, y) for x, y in zip(a[1], g[1]))
        dec = [_decode_steps(per[b][0], PUSHES[b][0], 1 + b % 2, b % 2 == 0) for b in range(n)]
        with m.decode_pool(8) as pool:
            got = _run(pool, dec, slots)
        for b in range(n):
            _check_decode(got[b], per, b, f"decode, clip {b}")
            with m.decode_pool(1) as one:
                alone = _run(one, [dec[b]], [0])[0]
            assert len(alone) == len(got[b]) and all(np.array_equal(a, g) for a, g in zip(alone, got[b])), f"one-slot pool, clip {b}"
        # a full frame makes exactly one stride final
        first = [g for g in got[6] if g.shape[-1]]
        assert first[0].shape == (cfg.channels, (1 + 6 % 2) * STRIDE)
        assert m.lstm_stats() == (False, 0)


def test_sessions_and_device_forms_equal_the_host_forms():
    import torch
    cfg, blob, clips, per = _reference()
    dev = lambda v: (None if v is None else v if v is FLUSH else (dev(v[0]), FLUSH) if isinstance(v, tuple) else  # noqa: E731
                     [dataclasses.replace(f, codes=torch.from_numpy(f.codes).cuda(), scale=None if f.scale is None else torch.from_numpy(f.scale).cuda()) for f in v]
                     if isinstance(v, list) else torch.from_numpy(np.ascontiguousarray(v)).cuda())
    with _model(cfg, blob) as m:
        order = [6, 5, 4, 0]
        enc = [_encode_steps(clips[b], *PUSHES[b]) for b in order]
        with m.encode_pool(4) as pool:
            got = _run(pool, enc, [0, 1, 2, 3], wrap=dev, return_emb=True)
            torch.cuda.synchronize()
            m.check_errors()
        for i, b in enumerate(order):
            assert all(hasattr(f.codes, "cpu") for step in got[i] for f in step[0])
            _check_encode(got[i], per, b, f"device encode, clip {b}")
        dec = [_decode_steps(per[b][0], 0, 2, i % 2 == 0) for i, b in enumerate(order)]
        with m.decode_pool(4) as pool:
            got = _run(pool, dec, [3, 2, 1, 0], wrap=dev)
            torch.cuda.synchronize()
            m.check_errors()
        for i, b in enumerate(order):
            _check_decode(got[i], per, b, f"device decode, clip {b}")
        # the one-stream session is a pool with one slot
        x = clips[4]
        with m.encode_session() as s:
            frames = s.push(x[:, :1000]) + s.push(x[:, 1000:4100]) + s.flush(x[:, 4100:])
            assert s.pending() == 0
            _same_frames(frames, per[4][0], "session")
            s.reset()
            _same_frames(s.flush(clips[0]), per[0][0], "session, second stream")
        with m.decode_session() as s:
            pcm = np.concatenate([s.push(per[4][0][:1]), s.flush(per[4][0][1:])], axis=-1)
            assert np.array_equal(pcm, per[4][2])
        # fewer codebooks than the handle's bandwidth: fixed at create
        nq = 2
        low = [dataclasses.replace(f, codes=np.ascontiguousarray(f.codes[:, :nq])) for f in per[6][0]]
        with m.decode_session(n_q=nq) as s:
            pcm = np.concatenate([s.push(low[:2]), s.flush(low[2:])], axis=-1)
        assert np.array_equal(pcm, m.decode(low, LENGTHS[6])[0])


def test_a_reset_slot_shows_no_stale_carry():
    cfg, blob, clips, per = _reference()
    with _model(cfg, blob) as m:
        with m.encode_pool(2) as pool:
            pool.step({0: clips[6][:, :5000], 1: clips[4][:, :300]})              # both slots hold samples of streams that are dropped
            assert pool.pending(0) == 5000 - STRIDE and pool.pending(1) == 300
            pool.reset_slot(0)
            pool.reset_slot(1)
            assert pool.pending(0) == pool.pending(1) == 0
            got = _run(pool, [_encode_steps(clips[5], 0, [4100], False), _encode_steps(clips[2], 0, [2500], True)], [0, 1], return_emb=True)
            _check_encode(got[0], per, 5, "after a reset")
            _check_encode(got[1], per, 2, "after a reset")
            with pytest.raises(ValueError, match="slot 0 has been flushed"):
                pool.step({0: clips[0]})
            pool.reset_slot(0)                                                      # a flushed slot is new again
            _check_encode(_run(pool, [_encode_steps(clips[3], 0, [SEG], True)], [0], return_emb=True)[0], per, 3, "after a flush and a reset")
        with m.decode_pool(2) as pool:
            pool.step({0: per[6][0][:2], 1: per[5][0][:1]})                         # carried tails of dropped streams
            assert pool.pending(0) == pool.pending(1) == F_FULL * HOP - STRIDE
            pool.reset_slot(0)
            pool.reset_slot(1)
            got = _run(pool, [_decode_steps(per[5][0], 0, 1, True), _decode_steps(per[6][0], 0, 3, False)], [0, 1])
            _check_decode(got[0], per, 5, "after a reset")
            _check_decode(got[1], per, 6, "after a reset")


def _launches(m, fn):
    m.profile_enable(True)
    m.profile_reset()
    out = fn()
    n = sum(v["launches"] for v in m.profile_read().values())
    m.profile_enable(False)
    return out, n


def test_a_lockstep_step_is_one_launch_sequence_and_a_handle_without_a_pool_is_unchanged():
    cfg, blob, clips, per = _reference()
    n = 4
    x = synthetic_pcm(n, cfg.channels, SEG + STRIDE, cfg.sampling_rate, seed=5)
    with _model(cfg, blob) as fresh, _model(cfg, blob) as m:
        # a handle that never had a pool: the counts of the one-clip and ragged calls, before anything else
        base = [_launches(fresh, lambda: fresh.encode(x[:, :, :STRIDE]))[1], _launches(fresh, lambda: fresh.encode(clips[6][None]))[1],
                _launches(fresh, lambda: fresh.decode(per[6][0], LENGTHS[6]))[1], _launches(fresh, lambda: fresh.encode_ragged(clips))[1]]
        uni_frames, n_uni = _launches(m, lambda: m.encode(x[:, :, :STRIDE]))      # n one-segment clips as one uniform batch
        _, n_uni_dec = _launches(m, lambda: m.decode(uni_frames, STRIDE))
        with m.encode_pool(n) as pool:
            pool.step({k: x[k, :, :100] for k in range(n)})                         # completes nothing: no launch but the gather
            _, n_idle = _launches(m, lambda: pool.step({k: x[k, :, 100:200] for k in range(n)}))
            assert n_idle == 1
            plan, rows = pool.plan({k: x[k, :, 200:SEG] for k in range(n)})           # one batch of n rows
            assert (plan["n_rows"], plan["n_batches"]) == (n, 1) and sorted(r["clip"] for r in rows) == list(range(n))
            out, n_pool = _launches(m, lambda: pool.step({k: x[k, :, 200:SEG] for k in range(n)}))
            assert all(len(out[k]) == 1 for k in range(n))
            # the step's own table-driven launches, counted: the gather (what the idle step launched) and one copy per packed output of
            # the one batch -- the codes, and the scales where the model normalises (no emb was asked for)
            own = n_idle + 1 + int(cfg.normalize)
            assert n_pool - own <= n_uni, (n_pool, own, n_uni)
            out2, n_pool2 = _launches(m, lambda: pool.step({k: x[k, :, SEG:] for k in range(n)}))
            assert n_pool2 == n_pool and all(len(out2[k]) == 1 for k in range(n))
        whole = [m.encode(x[k:k + 1]) for k in range(n)]
        for k in range(n):
            _same_frames(out[k] + out2[k], whole[k][:2], f"row {k}")
        with m.decode_pool(n) as pool:
            res, n_dec = _launches(m, lambda: pool.step({k: whole[k][:1] for k in range(n)}))
            # its own launches, counted: one copy per packed input of the one batch (the codes, and the scales where the model normalises)
            # and the one overlap-add (the one-clip call's own overlap-add is not a profiled launch)
            own = 1 + int(cfg.normalize) + 1
            assert n_dec - own <= n_uni_dec, (n_dec, own, n_uni_dec)
            assert all(np.array_equal(res[k], m.decode(whole[k], SEG + STRIDE)[0][:, :STRIDE]) for k in range(n))
        after = [_launches(m, lambda: m.encode(x[:, :, :STRIDE]))[1], _launches(m, lambda: m.encode(clips[6][None]))[1],
                 _launches(m, lambda: m.decode(per[6][0], LENGTHS[6]))[1], _launches(m, lambda: m.encode_ragged(clips))[1]]
        assert after == base and n_uni == base[0]                                   # pools leave no trace on the other calls


def test_refusals_name_the_slot_and_leave_every_slot_as_it_was():
    cfg, blob, clips, per = _reference()
    L = _lib.lib()
    i32 = lambda v: (C.c_int32 * len(v))(*v)  # noqa: E731
    with Encodec(cfg) as bare:                                                      # a handle without weights
        with bare.encode_pool(1) as pool, pytest.raises(RuntimeError, match="weights not loaded"):
            pool.step({0: clips[2]})
    small24 = encodec_cfg_from_meta(load_golden("encodec_small24")["meta"])
    with Encodec(small24) as m24:
        p = C.c_void_p()
        assert L.nc_encodec_stream_pool_create(m24._h, 0, 1, 0, C.byref(p)) == _lib.NC_EUNSUPPORTED and b"not segmented" in L.nc_last_error()
        assert not p.value
    with _model(cfg, blob) as m:
        for bad in (0, -1, 70000):
            with pytest.raises(ValueError):
                m.encode_pool(bad)
        with pytest.raises(ValueError):
            m.decode_pool(1, n_q=99)
        with m.encode_pool(3) as pool:
            x = clips[4]
            pool.step({0: x[:, :3000], 2: clips[6][:, :4100]})
            state = [pool.pending(s) for s in range(3)]
            sentinel, sc = np.full(8192, -7, np.int64), np.full(16, -7.0, np.float32)
            flat = np.zeros(cfg.channels * 8000, np.float32)

            def raw(slots, n_in, flush=None, n=None, in_=flat, out=sentinel, cap=8192):
                return L.nc_encodec_stream_pool_step(pool._p, (1 if slots is None else len(slots)) if n is None else n, i32(slots) if slots is not None else None,
                                                     _lib.i64_array(n_in) if n_in is not None else None, i32(flush) if flush else None, None,
                                                     in_.ctypes.data if in_ is not None else None, None, out.ctypes.data if out is not None else None,
                                                     sc.ctypes.data, None, cap, None, None)
            for args, word in ((dict(slots=[0, 1], n_in=[10, 10], n=0), b"n must be positive"), (dict(slots=None, n_in=[10]), b"null"),
                               (dict(slots=[0], n_in=None), b"null"), (dict(slots=[0], n_in=[2000], in_=None), b"null"),
                               (dict(slots=[0], n_in=[2000], out=None), b"null"), (dict(slots=[0, 3], n_in=[10, 10]), b"slot 3 is out of range"),
                               (dict(slots=[0, -1], n_in=[10, 10]), b"slot -1"), (dict(slots=[1, 0, 1], n_in=[10, 10, 10]), b"slot 1 is named twice"),
                               (dict(slots=[1, 0], n_in=[10, -5]), b"slot 0: n_in is negative"), (dict(slots=[0, 1], n_in=[10, 0], flush=[0, 1]), b"slot 1: a flush"),
                               (dict(slots=[0, 2], n_in=[2000, 4000], cap=10), b"out_cap"),
                               # the tail the one-clip call refuses: flushing slot 2 one sample behind a segment start leaves a 1-sample segment
                               (dict(slots=[0, 2], n_in=[2000, 2 * STRIDE + 1 - 4100], flush=[0, 1]), b"slot 2: ")):
                assert raw(**args) == _lib.NC_EINVAL and word in L.nc_last_error(), (args, L.nc_last_error())
                assert [pool.pending(s) for s in range(3)] == state and np.all(sentinel == -7) and np.all(sc == -7.0)
            with pytest.raises(ValueError, match="too short"):                      # (that tail is what the one-clip call refuses)
                m.encode(np.zeros((1, cfg.channels, 1), np.float32))
            assert L.nc_encodec_stream_pool_pending(pool._p, 3, C.byref(C.c_int64())) == _lib.NC_EINVAL
            assert L.nc_encodec_stream_pool_reset_slot(pool._p, -1) == _lib.NC_EINVAL
            assert L.nc_encodec_stream_pool_query(pool._p, 1, i32([0]), _lib.i64_array([10]), None, None, None, None, None) == _lib.NC_OK
            # push on: the refused steps have changed nothing
            _same_frames(pool.step({0: (x[:, 3000:], FLUSH)})[0], per[4][0], "after the refusals")
            with pytest.raises(ValueError, match="slot 0 has been flushed"):        # a push to an ended slot
                pool.step({0: x[:, :10], 1: x[:, :10]})
            assert pool.pending(1) == 0
            rest = pool.step({2: (clips[6][:, 4100:], FLUSH)})
            _same_frames(rest[2], per[6][0][1:], "slot 2 after the refusals")
        with m.decode_pool(2) as pool:
            fr = per[6][0]
            a = pool.step({0: fr[:1]})[0]
            short = dataclasses.replace(fr[3])
            for entries, word in (({0: [short]}, "a full segment has"), ({0: ([short, fr[1], short], FLUSH)}, "a full segment has"),
                                  ({0: ([short, short], FLUSH)}, "no clip length"), ({1: FLUSH}, "received nothing"),
                                  ({0: [dataclasses.replace(fr[1], codes=fr[1].codes[:, :1])]}, "Invalid frame codes")):
                with pytest.raises(ValueError, match=word):
                    pool.step(entries)
                assert pool.pending(0) == F_FULL * HOP - STRIDE and pool.pending(1) == 0
            codes = np.ascontiguousarray(fr[1].codes.reshape(-1))
            out = np.zeros(cfg.channels * STRIDE, np.float32)
            args = (pool._p, 1, i32([0]), _lib.i64_array([1]), None, None, codes.ctypes.data)
            assert L.nc_encodec_stream_pool_step(*args, None, out.ctypes.data, None, None, out.size, None, None) == _lib.NC_EINVAL      # no scales
            assert L.nc_encodec_stream_pool_step(*args, fr[1].scale.ctypes.data, out.ctypes.data, None, None, out.size - 1, None, None) == _lib.NC_EINVAL
            assert b"out_cap" in L.nc_last_error() and not out.any()
            b = pool.step({0: (fr[1:], FLUSH)})[0]
            assert np.array_equal(np.concatenate([a, b], axis=-1), per[6][2])


def test_full_size_48khz_two_streams_three_segments():
    """encodec_48khz, stereo, 12 kbps: two live streams of 3 s pushed a second at a time (the persistent LSTM and the aligned streaming
    kernels on two-row batches); the second stream starts a step later.  Against the one-shot calls on the whole streams."""
    cfg = dataclasses.replace(EncodecConfig.encodec_48khz(), bandwidth=12.0)
    blob = save_blob(encodec_synthetic_state_dict(cfg, seed=42))
    T = 144000
    clips = [synthetic_pcm(1, cfg.channels, T, cfg.sampling_rate, seed=77 + i)[0] for i in range(2)]
    with _model(cfg, blob) as m:
        want = [m.encode(x[None]) for x in clips]
        audio = [m.decode(w, T)[0] for w in want]
        assert [len(w) for w in want] == [4, 4]                                     # three full segments and the 1440-sample tail
        enc = [_encode_steps(x, d, [48000], False) for d, x in enumerate(clips)]
        with m.encode_pool(2) as pool:
            got = _run(pool, enc, [0, 1])
        for b in range(2):
            _same_frames([f for step in got[b] for f in step], want[b], f"stream {b}")
        dec = [_decode_steps(want[b], b, 1, True) for b in range(2)]
        with m.decode_pool(2) as pool:
            got = _run(pool, dec, [1, 0])
        for b in range(2):
            pcm = np.concatenate(got[b], axis=-1)
            assert pcm.shape == audio[b].shape and np.array_equal(pcm, audio[b]), f"stream {b}"
        assert m.lstm_stats() == (False, 0)
