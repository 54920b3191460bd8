"""GPU suite: Dia's prompt stage on the device (csrc/nc_dia.hip) -- voice prompts to the delayed prefill in one call.

Truth for the kernels is the numpy restatement tests/dia_prompt_ref.py (which tests/test_dia_prompt_cpu.py holds to a torch-CPU
transcription of the reference); truth for the codes is the existing engine on every prompt alone (encode_to_code_matrix) and the C
oracle on every prompt.  np.array_equal everywhere, no tolerance.  The reduced-width DAC fixture of tests/test_dia_output_gpu.py
(4 codebooks of 64 entries, synthetic weights)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dia_prompt_ref as R  # noqa: E402
from conftest import dac_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import DAC, DACConfig, _lib, dia, dia_prefill_pack, mix_to_mono_ragged  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402
from oracle import c_oracle  # noqa: E402

BOS, SENTINEL = 1026, -777
PATTERNS = {"dia": [0, 8, 9, 10, 11, 12, 13, 14, 15], "zero": [0] * 9, "one_channel": [3], "descending": [7, 5, 2, 0],
            "repeats": [2, 0, 2, 5, 5, 0, 1], "wide": [(7 * i) % 13 for i in range(32)]}
EDGES = (0, 1, 63, 64, 65, 129)                                                  # frames around the tile of 64 steps
DELAY = [0, 2, 3, 5]                                                             # on the fixture's 4 codebooks


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _launches(m, fn):
    m.profile_enable(True)
    m.profile_reset()
    out = fn()
    p = m.profile_read()
    m.profile_enable(False)
    return out, sum(v["launches"] for v in p.values()), p["elem"]["launches"]


# ---- the prefill kernel alone -----------------------------------------------------------------------------------------------------------
def _packed_codes(B, Cn, seed, last_longest):
    """random codes up to 2^31 - 1 for B items whose frame counts run through EDGES; the last item of every group of 32 is the longest"""
    rng = np.random.default_rng(seed)
    frames = [EDGES[(b + b // 6) % 6] for b in range(B)]
    for b in last_longest:
        frames = [min(f, 65) if b - b % 32 <= i < b else f for i, f in enumerate(frames)]
        frames[b] = 129
    items = []
    for f in frames:
        c = rng.integers(0, 2 ** 31, (Cn, f)).astype(np.int64)
        if c.size:
            c.reshape(-1)[rng.integers(0, c.size, max(1, c.size // 9))] = rng.choice([2 ** 31 - 1, 0, BOS, SENTINEL], max(1, c.size // 9))
        items.append(c if f else None)
    return items, frames


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_prefill_kernel_equals_the_restatement(name):
    delay = PATTERNS[name]
    md, Cn = max(delay), len(delay)
    for B, last_longest, extra in ((33, (31, 32), 0), (70, (63, 69), 70)):
        items, frames = _packed_codes(B, Cn, 100 * B + Cn, last_longest)
        assert set(EDGES) <= set(frames) and max(frames) == 129
        T = 129 + md + extra
        got = dia_prefill_pack(items, delay, BOS, SENTINEL, T_max=T if extra else None)
        want = R.prefill_closed_form(items, delay, BOS, T_max=T)
        assert got.dtype == np.int32 and got.shape == want.shape == (B, T, Cn)
        assert np.array_equal(got, want), (name, B, np.argwhere(got != want)[:4].tolist())
        assert (got == 2 ** 31 - 1).any()
        if not extra:                                                            # the reference's own composition at its own T_max
            literal, _ = R.prepare_audio_prompt([None if c is None else c.T for c in items], B, delay, BOS, SENTINEL)
            assert np.array_equal(got, literal), (name, B)
    import torch
    dev_items = [None if c is None else torch.from_numpy(c).cuda() for c in items[:5]]
    t = dia_prefill_pack(dev_items, delay, BOS)
    assert t.is_cuda and t.dtype == torch.int32
    torch.cuda.synchronize()
    assert np.array_equal(_np(t), R.prefill_closed_form(items[:5], delay, BOS))


def test_prefill_without_any_prompt_and_its_refusals():
    for name, delay in PATTERNS.items():
        if max(delay) == 0:
            with pytest.raises(ValueError):                                      # T_max == 0: nothing holds the BOS row
                dia_prefill_pack([None, None], delay, BOS)
            continue
        got = dia_prefill_pack([None] * 3, delay, BOS)
        assert got.shape == (3, max(delay), len(delay)) and np.array_equal(got, R.prefill_closed_form([None] * 3, delay, BOS))
        assert np.all(got[:, 0, :] == BOS)
    one = [np.zeros((4, 6), np.int64)]
    with pytest.raises(ValueError):
        dia_prefill_pack(one, [0, 1, -1, 2], BOS)
    with pytest.raises(ValueError):
        dia_prefill_pack(one, DELAY, 2 ** 31)
    with pytest.raises(ValueError):
        dia_prefill_pack(one, DELAY, BOS, pad=-2 ** 31 - 1)
    with pytest.raises(ValueError):
        dia_prefill_pack(one, DELAY, BOS, T_max=10)                              # below 6 + 5
    assert np.array_equal(dia_prefill_pack(one, DELAY, BOS, T_max=11), R.prefill_closed_form(one, DELAY, BOS))


# ---- the ragged mix kernel --------------------------------------------------------------------------------------------------------------
def test_mix_ragged_kernel_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(8)
    ch = [(1, 2, 3, 6)[b % 4] for b in range(33)]
    n = [(1, 255, 256, 257)[(b // 4 + b) % 4] for b in range(33)]
    assert len({(c, f) for c, f in zip(ch, n)}) == 16                            # every channel count meets every frame count
    prompts = [(rng.standard_normal(f * c) * 2).astype(np.float32) for c, f in zip(ch, n)]
    prompts[0][0] = -0.0                                                         # one channel is a copy: the sign of zero survives
    got = mix_to_mono_ragged(prompts, ch)
    assert [g.shape[0] for g in got] == n
    for b, (g, p, c) in enumerate(zip(got, prompts, ch)):
        assert g.dtype == np.float32 and g.tobytes() == R.mix_mono32(p, c).tobytes(), (b, c, n[b])
    import torch
    dev = mix_to_mono_ragged([torch.from_numpy(p).cuda() for p in prompts[:6]], ch[:6])
    assert all(t.is_cuda for t in dev)
    torch.cuda.synchronize()
    assert all(_np(t).tobytes() == R.mix_mono32(p, c).tobytes() for t, p, c in zip(dev, prompts, ch))
    with pytest.raises(ValueError):
        mix_to_mono_ragged(prompts[:2], [1, 0])
    with pytest.raises(ValueError):
        mix_to_mono_ragged([prompts[1][:5]], [2])                                # not whole frames


# ---- encode_dia_prompts -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dac():
    g = load_golden("dac_small")
    cfg = dac_cfg_from_meta(g["meta"])
    m = DAC(cfg)
    m.blob = save_blob(dac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"]))
    m.load_blob(m.blob)
    m.set_chunk_frames(_lib.NC_CHUNK_OFF)
    assert cfg.n_codebooks == 4 and cfg.codebook_size == 64
    yield m
    m.dispose()


@pytest.fixture(scope="module")
def case(dac):
    """the prompts, the codes of every prompt alone from the engine and from the C oracle, the restated prefill -- computed once"""
    hop, sr = dac.hop_length, dac.config.sample_rate
    lens = [hop - 1, hop, hop + 1, 3 * hop + 5]
    prompts = [synthetic_pcm(1, 1, t, sr, seed=70 + i)[0, 0] for i, t in enumerate(lens)]
    prompts.insert(2, None)
    batch = len(prompts) + 2
    solo = [None if p is None else _np(dac.encode_to_code_matrix(p[None, :])) for p in prompts]          # [F, C]
    ref = c_oracle.RefDAC(dac.config, dac.blob)
    ora = [None if p is None else np.ascontiguousarray(np.asarray(ref.encode(p[None, None])[1][0]).T) for p in prompts]
    frames = [0 if s is None else s.shape[0] for s in solo] + [0, 0]
    assert frames == [1, 1, 0, 2, 4, 0, 0]
    want, steps = R.prepare_audio_prompt(solo, batch, DELAY, BOS, SENTINEL)
    want_ora, _ = R.prepare_audio_prompt(ora, batch, DELAY, BOS, SENTINEL)
    return dict(prompts=prompts, batch=batch, solo=solo, frames=frames, want=want, want_ora=want_ora, steps=steps)


def test_encode_dia_prompts_equals_every_prompt_alone_and_the_oracle(dac, case):
    k = case
    got, steps = dac.encode_dia_prompts(k["prompts"], k["batch"], DELAY, BOS, SENTINEL)
    assert got.dtype == np.int32 and got.shape == (7, 4 + 5, 4)
    assert np.array_equal(got, k["want"]), "differs from PrepareAudioPrompt on encode_to_code_matrix of every prompt alone"
    assert np.array_equal(got, k["want_ora"]), "differs from PrepareAudioPrompt on the C oracle's codes"
    assert steps == k["steps"] == [f + 1 for f in k["frames"]]
    assert not np.any(got == SENTINEL)
    fewer, st = dac.encode_dia_prompts(k["prompts"], 2, DELAY, BOS)              # batch_size below the prompt count
    assert np.array_equal(fewer, k["want"][:5]) and st == k["steps"][:5]


def test_a_stereo_prompt_equals_its_mono_mix(dac, case):
    k = case
    rng = np.random.default_rng(4)
    n = k["prompts"][4].shape[0]
    stereo = (rng.standard_normal(2 * n) * 0.3).astype(np.float32)
    three = (rng.standard_normal(3 * (dac.hop_length + 1)) * 0.3).astype(np.float32)
    mixed = list(k["prompts"])
    mixed[3], mixed[4] = three, stereo
    mono = list(k["prompts"])
    mono[3], mono[4] = R.mix_mono32(three, 3), R.mix_mono32(stereo, 2)
    (a, sa), n_mix, _ = _launches(dac, lambda: dac.encode_dia_prompts(mixed, k["batch"], DELAY, BOS, channels=[1, 1, 1, 3, 2]))
    (b, sb), n_mono, _ = _launches(dac, lambda: dac.encode_dia_prompts(mono, k["batch"], DELAY, BOS))
    assert np.array_equal(a, b) and sa == sb == k["steps"]
    assert n_mix == n_mono + 1                                                   # one mix launch, and none where every prompt is mono
    solo = [None if p is None else _np(dac.encode_to_code_matrix(p[None, :])) for p in mono]
    assert np.array_equal(a, R.prepare_audio_prompt(solo, k["batch"], DELAY, BOS)[0])


def test_no_prompt_at_all_runs_no_encode(dac):
    for prompts, batch in (([None] * 3, None), (None, 3), ([], 3)):
        (got, steps), n_all, n_elem = _launches(dac, lambda: dac.encode_dia_prompts(prompts, batch, DELAY, BOS, SENTINEL))
        assert got.shape == (3, max(DELAY), 4) and steps == [1, 1, 1]
        assert np.array_equal(got, R.prepare_audio_prompt(prompts, 3, DELAY, BOS)[0])
        assert np.all(got[:, 0, :] == BOS) and set(np.unique(got)) <= {BOS, -1}
        assert (n_all, n_elem) == (1, 1)                                         # the prefill launch alone


def test_device_tensors_stay_on_the_device_and_the_launches_are_the_ragged_ones(dac, case):
    import torch
    k = case
    dev = torch.device("cuda", dac.device_index)
    stream = torch.cuda.Stream(dev)
    clips = [torch.from_numpy(p).to(dev) for p in k["prompts"] if p is not None]
    prompts = [None if p is None else torch.from_numpy(p).to(dev) for p in k["prompts"]]
    rng = np.random.default_rng(4)
    stereo_np = (rng.standard_normal(2 * k["prompts"][4].shape[0]) * 0.3).astype(np.float32)
    with_stereo = list(prompts)
    with_stereo[4] = torch.from_numpy(stereo_np).to(dev)
    many = prompts + [None] * 30                                                 # 35 items: two item groups
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        _, n_ragged, e_ragged = _launches(dac, lambda: dac.encode_ragged(clips))
        (got, steps), n_call, e_call = _launches(dac, lambda: dac.encode_dia_prompts(prompts, k["batch"], DELAY, BOS, SENTINEL))
        (mixed, _), n_mixed, e_mixed = _launches(dac, lambda: dac.encode_dia_prompts(with_stereo, k["batch"], DELAY, BOS, channels=[1, 1, 1, 1, 2]))
        (wide, _), n_wide, _ = _launches(dac, lambda: dac.encode_dia_prompts(many, None, DELAY, BOS))
    stream.synchronize()
    dac.check_errors()
    assert got.is_cuda and mixed.is_cuda and wide.is_cuda and got.dtype == torch.int32
    assert (n_call, e_call) == (n_ragged + 1, e_ragged + 1)                      # one prefill launch behind the ragged sequence
    assert (n_mixed, e_mixed) == (n_ragged + 2, e_ragged + 2)                    # and one mix launch in front of it
    assert n_wide == n_ragged + 2                                                # one prefill launch per group of 32 items
    assert np.array_equal(_np(got), k["want"]) and steps == k["steps"]
    assert np.array_equal(_np(wide)[:7], k["want"]) and np.array_equal(_np(wide)[7:], np.broadcast_to(_np(wide)[2], (28, 9, 4)))
    solo = list(k["solo"])
    solo[4] = _np(dac.encode_to_code_matrix(R.mix_mono32(stereo_np, 2)[None, :]))
    assert np.array_equal(_np(mixed), R.prepare_audio_prompt(solo, k["batch"], DELAY, BOS)[0])


# ---- query and refusals -----------------------------------------------------------------------------------------------------------------
def _i32(v):
    return (C.c_int32 * len(v))(*v)


def test_prompt_query_values_and_every_refusal(dac, case):
    L, k, hop = _lib.lib(), case, dac.hop_length
    lens = [0 if p is None else p.shape[0] for p in k["prompts"]] + [0, 0]
    assert dia.prompt_query(dac, lens, DELAY) == (k["frames"], k["steps"], 4 + 5)
    assert dia.prompt_query(dac, [0, 0], DELAY) == ([0, 0], [1, 1], 5)
    assert dia.prompt_query(dac, [1, hop, hop + 1, 0], [0, 0, 0, 0]) == ([1, 1, 2, 0], [2, 2, 3, 1], 2)
    assert L.nc_dia_prompt_query(dac._h, 7, 4, _i32(DELAY), _lib.i64_array(lens), None, None, None) == _lib.NC_OK   # outputs nullable
    fr, st, tm = (C.c_int64 * 7)(), (C.c_int32 * 7)(), C.c_int64()

    def q(B=7, Cn=4, d=DELAY, n=lens, h=None):
        return L.nc_dia_prompt_query(dac._h if h is None else h, B, Cn, _i32(list(d)) if d is not None else None,
                                     _lib.i64_array(n) if n is not None else None, fr, st, C.byref(tm))

    E = _lib.NC_EINVAL
    assert q() == _lib.NC_OK and list(fr) == k["frames"] and list(st) == k["steps"] and tm.value == 9
    assert q(B=0) == E and q(B=-1) == E and q(n=None) == E and q(d=None) == E
    assert q(Cn=3, d=DELAY[:3]) == E and b"codebooks" in L.nc_last_error()      # C != n_codebooks
    assert q(Cn=5, d=DELAY + [1]) == E
    assert q(d=[0, 2, -1, 5]) == E                                               # a negative delay
    assert q(n=[hop, -1] + lens[2:]) == E                                        # a negative length
    assert q(d=[0, 0, 0, 0], n=[0] * 7) == E                                     # T_max == 0
    with DAC(DACConfig(n_codebooks=33)) as wide:                                 # C > 32, on a handle that has that many
        assert L.nc_dia_prompt_query(wide._h, 1, 33, _i32([0] * 33), _lib.i64_array([5]), fr, st, C.byref(tm)) == E

    pcm = np.ascontiguousarray(np.concatenate([p for p in k["prompts"] if p is not None]))
    out = np.full(7 * 9 * 4 + 8, SENTINEL, np.int32)
    steps = _i32([SENTINEL] * 7)
    with DAC(dac.config) as empty:                                               # no weights
        assert L.nc_dia_encode_prompts(empty._h, pcm.ctypes.data, 7, _lib.i64_array(lens), None, 4, _i32(DELAY), BOS, -1, out.ctypes.data,
                                       steps) == _lib.NC_ESTATE
    for fn in (L.nc_dia_encode_prompts, L.nc_dia_encode_prompts_dev):
        def call(p=pcm.ctypes.data, B=7, n=lens, ch=None, Cn=4, d=DELAY, bos=BOS, pad=-1, o=out.ctypes.data):
            return fn(dac._h, p, B, _lib.i64_array(n) if n is not None else None, _i32(list(ch)) if ch is not None else None, Cn,
                      _i32(list(d)) if d is not None else None, bos, pad, o, steps)

        assert call(p=None) == E and call(o=None) == E and call(n=None) == E and call(d=None) == E          # null pointers
        assert call(B=0) == E
        assert call(Cn=3, d=DELAY[:3]) == E and call(Cn=5, d=DELAY + [1]) == E                             # C != n_codebooks
        assert call(d=[0, 2, -1, 5]) == E
        assert call(n=[hop, -1] + lens[2:]) == E
        assert call(ch=[1, 1, 1, 0, 1, 1, 1]) == E and call(ch=[1, -2, 1, 1, 1, 1, 1]) == E                 # channels[b] <= 0
        assert call(d=[0, 0, 0, 0], n=[0] * 7) == E                                                         # T_max == 0
        assert call(bos=2 ** 31) == E and call(bos=-2 ** 31 - 1) == E and call(pad=2 ** 31) == E and call(pad=-2 ** 40) == E
        assert call(n=[2 ** 30 + 1] + lens[1:]) == E                                                        # longer than the ragged encode takes
    assert np.all(out == SENTINEL) and list(steps) == [SENTINEL] * 7
    codes = np.zeros(4 * 4, np.int64)
    assert L.nc_dia_prefill_pack_dev(dac.device_index, codes.ctypes.data, 1, _lib.i64_array([2 ** 38]), 4, _i32(DELAY), BOS, -1, 2 ** 38 + 5,
                                     out.ctypes.data, None) == E                                            # a grid that does not fit
    dac.synchronize()
    dac.check_errors()
    got, steps = dac.encode_dia_prompts(k["prompts"], k["batch"], DELAY, BOS, SENTINEL)
    assert np.array_equal(got, k["want"]) and steps == k["steps"]


# ---- round trip -------------------------------------------------------------------------------------------------------------------------
def test_prefill_fed_to_the_output_stage_decodes_the_prompt(dac, case):
    """The two stages' index conventions tied together.  The prefill is P[t, c] = codes[c][t - d_c - 1] for 1 <= t - d_c <= F (row 0 is
    BOS); the output stage reverts G to out[t, c] = G[min(t + d_c, T_gen - 1), c] for t < F.  With the BOS row dropped, G = P[1:],
    G[t + d_c, c] = P[t + d_c + 1, c] = codes[c][t]: the revert reads rows up to F - 1 + maxd of G, so the item's valid rows are
    P[1 : F + maxd + 1] -- F + maxd rows, which the prefill holds for every item shorter than the longest (T_max = max F + maxd cuts the
    longest item's own last row, as the reference does).  maxd arbitrary rows appended behind them are never read (T_gen = F + 2 maxd,
    t + d_c <= F - 1 + maxd < T_gen - 1): they stand for what the language model generates next."""
    k, md = case, max(DELAY)
    item, F = 3, 2                                                               # the prompt of hop + 1 samples; the longest has 4 frames
    assert k["frames"][item] == F and max(k["frames"]) > F
    prefill, steps = dac.encode_dia_prompts(k["prompts"], k["batch"], DELAY, BOS)
    assert steps[item] == F + 1
    G = prefill[item, 1:F + md + 1, :].astype(np.int64)
    assert G.shape == (F + md, 4)
    junk = np.random.default_rng(1).integers(-5, 2000, (md, 4)).astype(np.int64)
    delayed = np.concatenate([G, junk])[None]
    pcm = dac.decode_dia_output(delayed, [F], DELAY, valid_range=(0, 63))[0]
    want = dac.decode_codes_ragged([np.ascontiguousarray(k["solo"][item].T)])[0]
    assert pcm.shape == want.shape == (dac.decoded_length(F),) and np.array_equal(_np(pcm), _np(want))
