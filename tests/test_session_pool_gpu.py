"""GPU suite: the session pool of DAC and SNAC -- many independent streams stepped in one call.  Every piece a slot returns == the piece a
B = 1 session returns for the same pushes, and every clip's concatenation == the one-shot call on that clip alone, bit for bit
(np.array_equal only: a mismatch means a kernel instance depends on the row or the batch it runs in, which is a finding).

Shapes (the reduced-width fixture configs and the clip recipe of tests/test_session_gpu.py): frames = 2 * max(halos) + 4 * align less a
few aligns per stream, so every stream has windows at the clip's true left edge, windows cut on both sides and the flush window at the
true right edge, and the streams differ in length; PCM lengths are no multiple of the hop."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import dac_cfg_from_meta, load_golden, snac_cfg_from_meta  # noqa: E402
from neuralcodecs_amd import DAC, FLUSH, SNAC, DACConfig, Encodec, EncodecConfig, SNACConfig, _lib, dac_halo, snac_halo  # noqa: E402
from neuralcodecs_amd.weights import (dac_synthetic_state_dict, save_blob, snac_noise, snac_synthetic_state_dict,  # noqa: E402
                                      synthetic_pcm)

N = 4                                                                       # streams
FIELDS = ("enc_left", "enc_right", "dec_left", "dec_right")
PATTERN_OF_SLOT = ("constant", "irregular", "one_large_push", "shorter_than_hr")   # slot 3 flushes early, is reset and runs a second clip


def _pushes(h, decode, frames, which):
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
    return [a] * max(1, (hr - a) // a)


def _sample_pushes(pushes, hop, T):
    out, left = [], T
    for n in pushes:
        k = min(left, n * hop)
        if k > 0:
            out.append(k)
        left -= k
    if left > 0:
        out.append(left)
    return out


def _launches(m, fn):
    m.profile_enable(True)
    m.profile_reset()
    out = fn()
    n = sum(v["launches"] for v in m.profile_read().values())
    m.profile_enable(False)
    return out, n


def _parts(x):
    """a piece as a list of numpy arrays (SNAC encode returns one per level)"""
    xs = x if isinstance(x, (list, tuple)) else [x]
    return [np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in xs]


def _same(a, b):
    a, b = _parts(a), _parts(b)
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _cat(pieces):
    cols = list(zip(*[_parts(p) for p in pieces]))
    return [np.concatenate(c, axis=-1) for c in cols]


# ----------------------------------------------------------------------------------------------------------------------- fixtures
class Rig:
    """One model with N clips of its own: cut(k, o, n) -> (what stream k pushes for units [o, o + n), its noise or None)."""

    def __init__(self, name):
        g = load_golden(name)
        self.snac = name.startswith("snac")
        if self.snac:
            self.cfg = snac_cfg_from_meta(g["meta"])
            self.h = snac_halo(self.cfg)
            self.m = SNAC(self.cfg)
            self.m.load_blob(save_blob(snac_synthetic_state_dict(self.cfg, seed=g["meta"]["weight_seed"])))
            self.rate = self.cfg.sampling_rate
        else:
            self.cfg = dac_cfg_from_meta(g["meta"])
            self.h = dac_halo(self.cfg)
            self.m = DAC(self.cfg)
            self.m.load_blob(save_blob(dac_synthetic_state_dict(self.cfg, seed=g["meta"]["weight_seed"])))
            self.rate = self.cfg.sample_rate
        self.m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        self.hop, a = self.cfg.hop_length, self.h["align"]
        self.frames = 2 * max(self.h[k] for k in FIELDS) + 4 * a
        self.F = [self.frames - k * a for k in (2, 1, 0, 3)]                # clip lengths differ (slot 2: one_large_push needs them all)
        self.T = [f * self.hop - 5 if self.snac else (f - 1) * self.hop + 17 for f in self.F]      # no multiple of the hop; f frames
        self.pcm = synthetic_pcm(N, 1, self.frames * self.hop, self.rate, seed=51)
        self.noise = self.snac and bool(self.cfg.noise)
        if self.snac:
            self.codes = [np.ascontiguousarray(c) for c in self.m.encode(self.pcm)]
            self.nz = snac_noise(self.cfg, N, self.frames, seed=53) if self.noise else None
        else:
            self.codes = self.m.encode(self.pcm)[1]

    def cut(self, decode, k, o, n):
        if not decode:
            return np.ascontiguousarray(self.pcm[k:k + 1, :, o:o + n]), None
        if not self.snac:
            return np.ascontiguousarray(self.codes[k:k + 1, :, o:o + n]), None
        c = [np.ascontiguousarray(lv[k:k + 1, o // s:(o + n) // s]) for lv, s in zip(self.codes, self.cfg.vq_strides)]
        z = [np.ascontiguousarray(b[k:k + 1, :, o * (b.shape[-1] // self.frames):(o + n) * (b.shape[-1] // self.frames)]) for b in self.nz] if self.noise else None
        return c, z

    def one_shot(self, decode, k, total):
        x, z = self.cut(decode, k, 0, total)
        if not decode:
            return self.m.encode(x) if self.snac else self.m.encode(x)[1]
        return self.m.decode(x, z) if self.snac else self.m.decode(self.m.from_codes(x))

    def session(self, decode):
        return self.m.decode_session(1) if decode else self.m.encode_session(1)

    def pool(self, decode, n=N):
        return self.m.decode_pool(n) if decode else self.m.encode_pool(n)

    def clips(self, decode):
        """per slot: the clips it runs, each (stream row k, pushes in units); slot 3: a clip shorter than hr, then a second clip"""
        out = []
        for k, which in enumerate(PATTERN_OF_SLOT):
            fr = _pushes(self.h, decode, self.F[k], which)
            if which == "shorter_than_hr":
                second = _pushes(self.h, decode, self.F[k], "irregular")
                out.append([(k, self._units(decode, fr, sum(fr) * self.hop - 3)), (k, self._units(decode, second, self.T[k]))])
            else:
                out.append([(k, self._units(decode, fr, self.T[k]))])
        return out

    def _units(self, decode, frame_pushes, T):
        return list(frame_pushes) if decode else _sample_pushes(frame_pushes, self.hop, T)


_RIGS = {}


def _rig(name):
    if name not in _RIGS:
        _RIGS[name] = Rig(name)
    return _RIGS[name]


def _run_pool(r, decode, to=None, with_noise=True):
    """Slot k joins at step k.  -> per slot, per clip: the pieces the pool returned"""
    clips = r.clips(decode)
    todo = []                                                               # per slot: [(clip index, k, offset, n | FLUSH)]
    for sl, cl in enumerate(clips):
        items = []
        for ci, (k, pushes) in enumerate(cl):
            o = 0
            for n in pushes:
                items.append((ci, k, o, n))
                o += n
            items.append((ci, k, o, FLUSH))
        todo.append(items)
    got = [[[] for _ in cl] for cl in clips]
    with r.pool(decode) as pool:
        t = 0
        while any(t - sl < len(items) for sl, items in enumerate(todo)):
            entries, noise, meta = {}, {}, {}
            for sl, items in enumerate(todo):
                i = t - sl
                if not 0 <= i < len(items):
                    continue
                ci, k, o, n = items[i]
                if i > 0 and items[i - 1][3] is FLUSH:
                    assert pool.pending(sl) == 0
                    pool.reset(sl)
                if n is FLUSH:
                    entries[sl] = FLUSH
                else:
                    x, z = r.cut(decode, k, o, n)
                    if to:
                        x = [to(a) for a in x] if isinstance(x, list) else to(x)
                        z = [to(a) for a in z] if z is not None else None
                    entries[sl] = x
                    if z is not None:
                        noise[sl] = z
                meta[sl] = ci
            out = pool.step(entries, noise if (noise and with_noise) else None)
            assert set(out) == set(entries)
            for sl, piece in out.items():
                got[sl][meta[sl]].append(piece)
            t += 1
    return clips, got


def _run_sessions(r, decode, clips):
    """the same pushes, clip by clip, on a B = 1 session"""
    ref = []
    for cl in clips:
        per = []
        for k, pushes in cl:
            pieces, o = [], 0
            with r.session(decode) as s:
                for n in pushes:
                    x, z = r.cut(decode, k, o, n)
                    pieces.append(s.push(x, z) if (decode and r.snac) else s.push(x))
                    o += n
                pieces.append(s.flush())
            per.append(pieces)
        ref.append(per)
    return ref


# ------------------------------------------------------------------------------------------------- 1. staggered streams == sessions
@pytest.mark.parametrize("decode", [True, False], ids=["decode", "encode"])
@pytest.mark.parametrize("name", ["dac_small", "snac_small", "snac_small_attn"])
def test_staggered_streams_equal_single_sessions_and_one_shot(name, decode):
    r = _rig(name)
    clips, got = _run_pool(r, decode)
    ref = _run_sessions(r, decode, clips)
    for sl, cl in enumerate(clips):
        for ci, (k, pushes) in enumerate(cl):
            assert len(got[sl][ci]) == len(ref[sl][ci]) == len(pushes) + 1
            for i, (a, b) in enumerate(zip(got[sl][ci], ref[sl][ci])):
                assert _same(a, b), (name, decode, sl, ci, i)
            want = _parts(r.one_shot(decode, k, sum(pushes)))
            have = _cat(got[sl][ci])
            assert len(have) == len(want)
            for a, b in zip(have, want):
                assert a.shape == b.shape and np.array_equal(a, b), (name, decode, sl, ci)
    short = got[3][0]
    assert all(_parts(p)[0].shape[-1] == 0 for p in short[:-1]), "a clip shorter than hr emitted before its flush"
    assert any(_parts(p)[0].shape[-1] > 0 for p in got[0][0][:-1]), "nothing was emitted before the flush"


# ----------------------------------------------------------------------------------------------------------- 2. batching is real
@pytest.mark.parametrize("name", ["dac_small", "snac_small_attn"])
def test_a_lockstep_step_launches_no_more_than_a_lockstep_session(name):
    r = _rig(name)
    m, a = r.m, r.h["align"]
    hl, hr = r.h["dec_right"], r.h["dec_left"]
    warm = (hl + hr) // a + 2                                               # pushes of `a` frames until the window is hl + a + hr wide
    B4 = lambda o, n: _cut_rows(r, o, n)  # noqa: E731

    with m.decode_session(N) as s:
        for i in range(warm):
            x, z = B4(i * a, a)
            s.push(x, z) if r.snac else s.push(x)
        x, z = B4(warm * a, a)
        ref, n_session = _launches(m, lambda: s.push(x, z) if r.snac else s.push(x))
    with r.pool(True) as pool:
        step = lambda o, slots: pool.step({k: r.cut(True, k, o, a)[0] for k in slots},  # noqa: E731
                                          {k: r.cut(True, k, o, a)[1] for k in slots} if r.noise else None)
        for i in range(warm):
            step(i * a, range(N))
        out, n_pool = _launches(m, lambda: step(warm * a, range(N)))
        assert all(np.array_equal(_parts(out[k])[0][0], np.asarray(ref)[k]) for k in range(N))
        assert np.asarray(ref).shape[-1] > 0
        assert n_pool <= n_session, (n_pool, n_session)                     # one batch of 4 rows, never 4 sequences
    with r.pool(True) as pool:                                              # two window widths in one step: two sequences, one assembly
        step = lambda o, slots: pool.step({k: r.cut(True, k, o, a)[0] for k in slots},  # noqa: E731
                                          {k: r.cut(True, k, o, a)[1] for k in slots} if r.noise else None)
        early = hr // a + 1                                                 # slots 2, 3 join `late` steps later and are still growing
        late = warm - early
        for i in range(late):
            step(i * a, (0, 1))
        for i in range(early):
            step((late + i) * a, (0, 1))
            step(i * a, (2, 3))
        widths = {k: pool.pending(k) for k in range(N)}
        assert widths[0] == widths[1] and widths[2] == widths[3]
        out, n_two = _launches(m, lambda: pool.step(
            {k: r.cut(True, k, (warm if k < 2 else early) * a, a)[0] for k in range(N)},
            {k: r.cut(True, k, (warm if k < 2 else early) * a, a)[1] for k in range(N)} if r.noise else None))
        assert all(_parts(out[k])[0].shape[-1] > 0 for k in range(N))
        n_assemble = 2 if r.noise else 1
        assert n_two == 2 * n_pool - n_assemble, (n_two, n_pool)


def _cut_rows(r, o, n):
    """units [o, o + n) of all N streams as one B = N push"""
    xs = [r.cut(True, k, o, n) for k in range(N)]
    if r.snac:
        x = [np.concatenate([x[0][i] for x in xs]) for i in range(len(xs[0][0]))]
        z = [np.concatenate([x[1][i] for x in xs]) for i in range(len(xs[0][1]))] if r.noise else None
        return x, z
    return np.concatenate([x[0] for x in xs]), None


# ------------------------------------------------------------------------------------------------- 3. device-pointer forms
@pytest.mark.parametrize("name", ["dac_small", "snac_small_attn"])
def test_device_pointer_forms_equal_the_host_forms(name):
    import torch
    r = _rig(name)
    dev = torch.device("cuda", r.m.device_index)
    to = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    for decode in (True, False):
        clips, host = _run_pool(r, decode)
        _, got = _run_pool(r, decode, to=to)                                # shapes are read below before any synchronisation
        shapes = lambda g: [[[tuple(a.shape) for a in (p if isinstance(p, list) else [p])] for p in c] for s in g for c in s]  # noqa: E731
        assert shapes(got) == shapes(host)
        torch.cuda.synchronize()
        for sl in range(len(clips)):
            for ci in range(len(clips[sl])):
                # a step of flushes alone answers in the form of the last step with data, so every piece here is a device tensor
                assert all(torch.is_tensor(a) and a.is_cuda for p in got[sl][ci] for a in (p if isinstance(p, list) else [p]))
                assert all(_same(a, b) for a, b in zip(got[sl][ci], host[sl][ci])), (name, decode, sl, ci)


# ----------------------------------------------------------------------------------------------------------- 4. SNAC seeded noise
def test_snac_slot_seed_equals_a_single_session_with_that_seed():
    r = _rig("snac_small_attn")
    assert r.noise
    pushes = _pushes(r.h, True, r.F[1], "irregular")
    runs = {}
    for seed in (7, 8):
        parts, o = [], 0
        with r.m.decode_session(1) as s:
            s.set_seed(seed)
            for n in pushes:
                parts.append(s.push(r.cut(True, 1, o, n)[0]))
                o += n
            parts.append(s.flush())
        runs[seed] = parts
    with r.pool(True, 3) as pool:                                           # slot 2 runs stream 1 with seed 7, slot 0 the same stream with seed 8
        pool.set_seed(2, 7)
        pool.set_seed(0, 8)
        got, o = {0: [], 2: []}, 0
        for n in pushes:
            out = pool.step({0: r.cut(True, 1, o, n)[0], 2: r.cut(True, 1, o, n)[0]})
            o += n
            for k in got:
                got[k].append(out[k])
        out = pool.step({0: FLUSH, 2: FLUSH})
        for k in got:
            got[k].append(out[k])
    assert all(_same(a, b) for a, b in zip(got[2], runs[7])) and all(_same(a, b) for a, b in zip(got[0], runs[8]))
    assert not np.array_equal(_cat(got[0])[0], _cat(got[2])[0])


# ----------------------------------------------------------------------------------------------------------- 5. error conventions
def test_error_conventions():
    L = _lib.lib()
    with Encodec(EncodecConfig()) as e:
        out = C.c_void_p()
        assert L.nc_session_pool_create(e._h, 1, 4, 0, C.byref(out)) == _lib.NC_EUNSUPPORTED and not out.value
        assert L.nc_session_pool_create(e._h, 0, 4, 0, C.byref(out)) == _lib.NC_EUNSUPPORTED
    r = _rig("dac_small")
    with pytest.raises(ValueError):
        r.m.decode_pool(0)
    sn = _rig("snac_small")
    a = sn.h["align"]
    assert a > 1
    with sn.pool(True, 2) as pool:                                          # a decode push that is no multiple of align
        n = (C.c_int64 * 2)(-1, -1)
        flat = np.zeros(8 * a, np.int64)
        outb = np.zeros(1 << 16, np.float32)
        slots, nin = (C.c_int32 * 2)(0, 1), _lib.i64_array([a, a + 1])
        assert L.nc_session_pool_step(pool._p, 2, slots, nin, flat.ctypes.data, None, outb.ctypes.data, outb.size, n) == _lib.NC_EINVAL
        assert L.nc_session_pool_query(pool._p, 2, slots, nin, n) == _lib.NC_EINVAL
        assert pool.pending(0) == 0 and pool.pending(1) == 0
    hr = r.h["dec_left"]
    first = hr + 2                                                          # a first push that emits
    with r.pool(True, 3) as pool, r.m.decode_session(1) as s:
        x0, x1 = r.cut(True, 0, 0, first)[0], r.cut(True, 1, 0, 1)[0]
        want0 = s.push(x0)
        assert want0.shape[-1] > 0
        nq = r.cfg.n_codebooks
        packed = np.ascontiguousarray(np.concatenate([x0.reshape(-1), x1.reshape(-1)]))
        n_out = pool.query({0: first, 1: 1})
        assert n_out == {0: want0.shape[-1], 1: 0}
        cap = sum(n_out.values())
        outb = np.full(cap, np.nan, np.float32)
        n = (C.c_int64 * 3)(-1, -1, -1)
        S = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
        call = lambda k, slots, nin, cap_: L.nc_session_pool_step(pool._p, k, slots, _lib.i64_array(nin), packed.ctypes.data, None,  # noqa: E731
                                                                  outb.ctypes.data, cap_, n)
        assert call(2, S(0, 0), [first, 1], cap) == _lib.NC_EINVAL                       # duplicate slot
        assert call(2, S(0, 3), [first, 1], cap) == _lib.NC_EINVAL                       # slot out of range
        assert call(2, S(0, -1), [first, 1], cap) == _lib.NC_EINVAL
        assert call(2, S(0, 1), [first, 1], cap - 1) == _lib.NC_EINVAL                   # out_cap one short
        assert call(2, S(0, 1), [first, 0], cap) == _lib.NC_EINVAL                       # flush of an empty slot
        assert call(2, S(0, 1), [first, -1], cap) == _lib.NC_EINVAL
        assert L.nc_session_pool_step(pool._p, 2, S(0, 1), _lib.i64_array([first, 1]), None, None, outb.ctypes.data, cap, n) == _lib.NC_EINVAL
        assert L.nc_session_pool_step(pool._p, 2, S(0, 1), _lib.i64_array([first, 1]), packed.ctypes.data, None, None, cap, n) == _lib.NC_EINVAL
        assert [pool.pending(k) for k in range(3)] == [0, 0, 0] and list(n) == [-1, -1, -1] and np.isnan(outb).all()   # no slot moved
        out = pool.step({0: x0, 1: x1})                                                  # ... and the valid step is exact
        assert np.array_equal(out[0], want0) and out[1].shape[-1] == 0
        assert (pool.pending(0), pool.pending(1)) == (s.pending(), 1)
        out = pool.step({0: FLUSH})
        assert np.array_equal(out[0], s.flush())
        x2 = r.cut(True, 0, first, 2)[0]
        before = [pool.pending(k) for k in range(3)]
        with pytest.raises(ValueError):                                                  # push after flush without reset: slot 1 must not move either
            pool.step({1: r.cut(True, 1, 1, 2)[0], 0: x2})
        with pytest.raises(ValueError):
            pool.step({0: FLUSH})
        assert [pool.pending(k) for k in range(3)] == before
        pool.reset(0)
        s.reset()
        assert np.array_equal(pool.step({0: x0})[0], s.push(x0))
        assert nq == x0.shape[1]
    with DAC(r.cfg) as unloaded:                                                         # no weights: NC_ESTATE
        with unloaded.decode_pool(2) as pool:
            with pytest.raises(RuntimeError):
                pool.step({0: np.zeros((1, r.cfg.n_codebooks, 4), np.int64)})
            assert pool.pending(0) == 0


# ------------------------------------------------------------------------------------------- 6. nothing changes without a pool
# Launches of one-shot encode / decode (profiled kernel classes), as tests/test_session_gpu.py records them
PARENT_LAUNCHES = {"dac_small": (39, 30), "snac_small": (44, 44)}


def test_a_handle_without_a_pool_launches_what_it_launched_before():
    B = 2
    r = _rig("dac_small")
    cfg, h = r.cfg, r.h
    frames = 6 * max(h[k] for k in FIELDS) + 5 * h["align"]
    pcm = synthetic_pcm(B, 1, (frames - 1) * cfg.hop_length + 17, cfg.sample_rate, seed=21)
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=load_golden("dac_small")["meta"]["weight_seed"])))
        (z, codes, _, _, _), n_enc = _launches(m, lambda: m.encode(pcm))
        audio, n_dec = _launches(m, lambda: m.decode(z))
        assert (n_enc, n_dec) == PARENT_LAUNCHES["dac_small"]
        with m.decode_pool(2) as pool:                                      # ... and a pool, used and destroyed, leaves them as they were
            pool.step({1: np.ascontiguousarray(codes[:1, :, :h["dec_left"] + 4])})
            pool.step({1: FLUSH})
        (z2, _, _, _, _), n_enc2 = _launches(m, lambda: m.encode(pcm))
        audio2, n_dec2 = _launches(m, lambda: m.decode(z2))
        assert (n_enc2, n_dec2) == (n_enc, n_dec) and np.array_equal(audio2, audio)
    sr = _rig("snac_small")
    scfg, sh = sr.cfg, sr.h
    frames = 6 * max(sh[k] for k in FIELDS) + 5 * sh["align"]
    pcm = synthetic_pcm(B, 1, frames * scfg.hop_length - 5, scfg.sampling_rate, seed=22)
    with SNAC(scfg) as m:
        m.load_blob(save_blob(snac_synthetic_state_dict(scfg, seed=load_golden("snac_small")["meta"]["weight_seed"])))
        codes, n_enc = _launches(m, lambda: m.encode(pcm))
        nz = snac_noise(scfg, B, frames, seed=23)
        audio, n_dec = _launches(m, lambda: m.decode([np.ascontiguousarray(c) for c in codes], nz))
        assert (n_enc, n_dec) == PARENT_LAUNCHES["snac_small"]
        with m.encode_pool(2) as pool:
            pool.step({0: np.ascontiguousarray(pcm[:1, :, :5000])})
            pool.step({0: FLUSH})
        codes2, n_enc2 = _launches(m, lambda: m.encode(pcm))
        audio2, n_dec2 = _launches(m, lambda: m.decode([np.ascontiguousarray(c) for c in codes2], nz))
        assert (n_enc2, n_dec2) == (n_enc, n_dec) and np.array_equal(audio2, audio)


def test_fixtures_are_released():
    for r in _RIGS.values():
        r.m.dispose()
    _RIGS.clear()


# ---------------------------------------------------------------------------------------------------------- 7. full-size instances
def _staggered_decode(pool, clips, push, cut):
    """slot k joins at step k and pushes `push` frames per step; -> per slot the pieces"""
    n_steps = [-(-f // push) + 1 for f in clips]
    got = [[] for _ in clips]
    for t in range(max(k + n for k, n in enumerate(n_steps))):
        entries, noise = {}, {}
        for k, f in enumerate(clips):
            i = t - k
            if 0 <= i < n_steps[k] - 1:
                entries[k], z = cut(k, i * push, min(push, f - i * push))
                if z is not None:
                    noise[k] = z
            elif i == n_steps[k] - 1:
                entries[k] = FLUSH
        out = pool.step(entries, noise or None)
        for k, p in out.items():
            got[k].append(p)
    return got


def test_dac44k_pool_equals_one_shot():
    """Engine against itself: instance selection changes with the batch and the width here."""
    cfg = DACConfig.dac_44khz()
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=3)))
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        pcm = synthetic_pcm(3, 1, int(1.5 * cfg.sample_rate), cfg.sample_rate, seed=34)
        codes = m.encode(pcm)[1]
        F = [codes.shape[-1] - 3 * k for k in range(3)]
        want = [m.decode(m.from_codes(np.ascontiguousarray(codes[k:k + 1, :, :F[k]]))) for k in range(3)]
        with m.decode_pool(3) as pool:
            got = _staggered_decode(pool, F, 32, lambda k, o, n: (np.ascontiguousarray(codes[k:k + 1, :, o:o + n]), None))
        for k in range(3):
            assert sum(g.shape[-1] > 0 for g in got[k]) >= 2
            have = np.concatenate(got[k], axis=-1)
            assert have.shape == want[k].shape and np.array_equal(have, want[k]), k


def test_snac24k_pool_equals_one_shot():
    cfg = SNACConfig.snac_24khz()
    frames = 2 * 16 + 3 * 4 + 64
    with SNAC(cfg) as m:
        m.load_blob(save_blob(snac_synthetic_state_dict(cfg, seed=4)))
        m.set_chunk_frames(_lib.NC_CHUNK_OFF)
        pcm = synthetic_pcm(2, 1, frames * cfg.hop_length, cfg.sampling_rate, seed=35)
        codes = [np.ascontiguousarray(c) for c in m.encode(pcm)]
        a = snac_halo(cfg)["align"]
        F = [frames, frames - 2 * a]
        nz = snac_noise(cfg, 2, frames, seed=36) if cfg.noise else None

        def cut(k, o, n):
            c = [np.ascontiguousarray(lv[k:k + 1, o // s:(o + n) // s]) for lv, s in zip(codes, cfg.vq_strides)]
            z = [np.ascontiguousarray(b[k:k + 1, :, o * (b.shape[-1] // frames):(o + n) * (b.shape[-1] // frames)]) for b in nz] if nz else None
            return c, z

        want = [m.decode(*cut(k, 0, F[k])) for k in range(2)]
        with m.decode_pool(2) as pool:
            got = _staggered_decode(pool, F, 16, cut)
        for k in range(2):
            have = np.concatenate(got[k], axis=-1)
            assert have.shape == want[k].shape and np.array_equal(have, want[k]), k
