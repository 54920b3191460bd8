"""CPU suite: Dia's sampling stage (include/nc_mi355x.h "Dia sampling stage") without a device.

nc_dia_sample_host -- the serial C++ twin of the kernel and the bit judge of the GPU suite -- is held to
  * meaning: a torch-CPU transcription of Dia.cs:424-501, 538-548 (every token has non-zero probability in its finalProbs) and a binary64
    inverse CDF (tests/dia_sample_ref.py) wherever no binary64 cumulative value lies within DELTA of top_p or of u.  DELTA = 1e-5 covers the
    binary32 chain behind the survivors: 2 ulp of exp, at most 64 sequential additions and one division, about 67 * 2^-24 = 4e-6.  At
    most 2 % of the rows may be left out by that rule;
  * the definition: the binary32 restatement, exactly, at every edge the header names;
  * the loop: a host emulation of the step's closed form against a torch transcription of Dia.cs:681-801, position for position.
nc_dia_generate_lengths is held to the transcription, and every refusal of the header is raised."""
import ctypes as C

import numpy as np
import pytest
import torch

import dia_sample_ref as R
from neuralcodecs_amd import _lib, dia_sample_host
from neuralcodecs_amd.dia import generate_lengths

DELTA = 1e-5
EDGES = R.edge_cases()
LOOPS = R.loop_cases()


def test_random_logits_mean_what_the_reference_means():
    rows = left_out = 0
    for name, lg, p, u in R.random_cases():
        tok, bad = dia_sample_host(lg, u, **p)
        assert not bad.any() and tok.min() >= 0, name
        B, Cn = tok.shape
        _, probs = R.torch_sample_next_token(R.torch_guided_logits(lg, p["cfg_scale"], p["eos"]).reshape(B * Cn, -1), p["temperature"], p["top_p"],
                                             p["top_k"], p["eos"])
        chosen = probs.numpy().reshape(B, Cn, -1)[np.arange(B)[:, None], np.arange(Cn)[None, :], tok]
        assert (chosen > 0).all(), (name, np.argwhere(chosen <= 0)[:4].tolist())
        for b in range(B):
            for c in range(Cn):
                want, margin = R.sample_row64(lg[2 * b, c], lg[2 * b + 1, c], c, p, u[b, c])
                rows += 1
                if margin is not None and margin <= DELTA:
                    left_out += 1
                    continue
                assert tok[b, c] == want, (name, b, c, int(tok[b, c]), want, margin)
    print(f"rows {rows}, left out by the DELTA rule {left_out}")
    assert rows == 864 and left_out <= 0.02 * rows, (rows, left_out)


def test_greedy_equals_torch_argmax_nan_rows_included():
    rng = np.random.default_rng(5)
    lg = (rng.standard_normal((8, 9, 70)) * 3).astype(np.float32)
    lg[1, 0, 3] = lg[1, 0, 40] = np.nan                 # two NaNs below eos on a conditional row: the first wins
    lg[3, 2, 11] = np.inf
    lg[4, 4, :] = 1.5                                    # all equal: the first maximum
    lg[5, 4, :] = 1.5
    lg[6, 5, :] = -np.inf
    lg[7, 5, :] = -np.inf                               # inf - inf: a row of NaN
    p = dict(R.DEFAULTS, eos=64, pad=65, temperature=0.0)
    tok, bad = dia_sample_host(lg, rng.random((4, 9)).astype(np.float32), **p)
    want = torch.argmax(R.torch_guided_logits(lg, p["cfg_scale"], p["eos"]), dim=-1).numpy()
    assert np.array_equal(tok, want) and not bad.any()
    assert tok[0, 0] == 3 and tok[3, 5] == 0


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_definition_edges_equal_the_binary32_restatement(case):
    name, lg, p, u = case
    want_tok, want_bad = R.sample32(lg, p, u)
    tok, bad = dia_sample_host(lg, u, **p)
    assert np.array_equal(tok, want_tok) and np.array_equal(bad, want_bad), (name, tok.tolist(), want_tok.tolist())
    if name == "bad_rows":
        assert tok[:, 1].tolist() == [-1, -1] and tok[0, 2] == -1 and tok[1, 0] == -1 and tok[1, 2] >= 0 and bad.tolist() == [1, 1]
    if name.startswith("no_survivor"):                      # all -inf and no NaN: the n == 0 exit, not the NaN one
        assert tok[0, 0] == -1 and tok[0, 2] == -1 and tok[0, 1] >= 0 and (tok[1] >= 0).all() and bad.tolist() == [1, 0]
    if name == "overflow_through_the_division":
        assert (tok == -1).all() and bad.tolist() == [1, 1]
    if name == "nan_on_eos":
        assert tok[0, 0] == -1 and bad.tolist() == [1, 0]
    if name == "top_p_tiny_only_the_first" or name == "top_k_1":
        q = dict(p, temperature=0.0)
        strike = R.sample32(lg, q, u)[0]                 # with one survivor the token is the argmax behind the EOS rule
        assert np.array_equal(tok[:, 1:], strike[:, 1:])
    if name == "eos_highest_on_channel_0":
        assert (dia_sample_host(lg, u, **dict(p, top_k=1))[0][:, 0] == p["eos"]).all()
    if name == "eos_not_highest_on_channel_0":
        assert not (tok[:, 0] == p["eos"]).any()


def _emulate(k, sampler):
    """the loop through a sampler of [2B, C, V] -> tokens and the closed form of the step on numpy arrays"""
    B, Cn, M, delay = k["B"], k["C"], k["max_tokens"], k["delay"]
    generated = np.full((B, M, Cn), -1, np.int32)
    generated[:, :k["prefill"].shape[1]] = k["prefill"]
    state, active = R.new_state(B), np.ones(B, bool)
    dec_step, bos_over, snaps = min(k["prefill_steps"]) - 1, False, []
    p = dict(R.DEFAULTS, eos=k["eos"], pad=k["pad"], temperature=0.0)
    while dec_step < M and active.any():
        s = dec_step + 1
        tok = sampler(k["tables"][s], p)
        if not bos_over:
            bos_over = all(dec_step - q > max(delay) for q in k["prefill_steps"])
        active = R.step_closed_form(state, generated, tok, s, M, delay, k["eos"], k["pad"], not bos_over)
        dec_step += 1
        snaps.append((generated.copy(), state[0].copy(), state[1].copy(), state[2].copy()))
    return snaps, state, generated, dec_step + 1


@pytest.mark.parametrize("case", LOOPS, ids=[c[0] for c in LOOPS])
def test_loop_closed_form_equals_the_transcribed_generate(case):
    name, k = case
    want = R.torch_generate(k["tables"], k["delay"], k["max_tokens"], k["prefill"], k["prefill_steps"], k["eos"], k["pad"])
    snaps, state, generated, final_step = _emulate(k, lambda lg, p: dia_sample_host(lg, np.zeros((k["B"], k["C"]), np.float32), **p)[0])
    assert len(snaps) == want["steps"] and final_step == want["final_step"]
    if name == "dia_pattern":
        assert want["steps"] == 40
    masked = unmasked = False
    for i, (a, b) in enumerate(zip(snaps, want["snaps"])):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (name, i)
    for i in range(1, len(snaps)):                          # both sides of apply_mask were taken over the prefilled buffer
        s = min(k["prefill_steps"]) + i
        kept = (snaps[i - 1][0][:, s] != -1) & (snaps[i][0][:, s] == snaps[i - 1][0][:, s])
        masked = masked or bool(kept.any())
        unmasked = unmasked or bool((snaps[i - 1][0][:, s] == -1).all())
    assert unmasked and (masked or max(k["delay"]) == 0 or name == "one_channel")
    lens, T_gen = generate_lengths(state[2].tolist(), k["prefill_steps"], final_step, max(k["delay"]))
    assert lens == want["lengths"] == R.lengths(state[2], k["prefill_steps"], final_step, max(k["delay"]))[0]
    assert T_gen == want["codes"].shape[1]
    assert np.array_equal(R.collect(generated, k["prefill_steps"], lens, max(k["delay"]), k["pad"]), want["codes"])
    if name == "dia_pattern":                               # ends early; EOS during another's countdown; ends by max_tokens - D
        assert state[2].tolist() == [6, 12, 42 - 15] and (state[1] == 0).all()


def test_generate_lengths_unfinished_items():
    assert generate_lengths([-1, 7, -1, 3], [2, 9, 40, 1], 30, 5) == ([23, 0, 0, 2], 28)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _i32(v):
    return (C.c_int32 * len(v))(*v)


def test_every_refusal_of_the_sampling_calls():
    L, E = _lib.lib(), _lib.NC_EINVAL
    B, Cn, V = 2, 3, 68
    lg = np.zeros((2 * B, Cn, V), np.float32)
    u = np.zeros((B, Cn), np.float32)
    tok, bad = np.full((B, Cn), -7, np.int64), np.full(B, -7, np.int32)
    state, gen, act = np.zeros((3, B), np.int64), np.full((B, 50, Cn), -1, np.int32), np.zeros(B, np.int32)
    good = dict(cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos=64, pad=65)

    def params(**kw):
        return _lib.NcDiaSampleParams(*[dict(good, **kw)[f] for f, _ in _lib.NcDiaSampleParams._fields_])

    def host(lg_=lg.ctypes.data, B_=B, C_=Cn, V_=V, p=params(), u_=u.ctypes.data, t=tok.ctypes.data, bd=bad.ctypes.data):
        return L.nc_dia_sample_host(lg_, B_, C_, V_, None if p is None else C.byref(p), u_, t, bd)

    def dev(lg_=lg.ctypes.data, B_=B, C_=Cn, V_=V, p=params(), u_=u.ctypes.data, t=tok.ctypes.data, bd=bad.ctypes.data):
        return L.nc_dia_sample_dev(0, lg_, B_, C_, V_, None if p is None else C.byref(p), u_, t, bd, None)

    def step(lg_=lg.ctypes.data, B_=B, C_=Cn, V_=V, p=params(), u_=u.ctypes.data, d=(0, 1, 2), s=3, M=50, st=state.ctypes.data, g=gen.ctypes.data,
             Ln=50, a=act.ctypes.data, bd=bad.ctypes.data):
        return L.nc_dia_generate_step_dev(0, lg_, B_, C_, V_, None if p is None else C.byref(p), u_, None if d is None else _i32(list(d)), s, M, 1, st, g,
                                          Ln, a, bd, None)

    for fn in (host, dev, step):
        assert fn(lg_=None) == E and fn(p=None) == E and fn(u_=None) == E and fn(bd=None) == E            # null pointers
        assert fn(B_=0) == E and fn(B_=-1) == E
        assert fn(C_=0) == E and fn(C_=33) == E
        assert fn(p=params(eos=-1)) == E and fn(p=params(eos=V)) == E
        assert fn(V_=4097, p=params(eos=0)) == E
        assert fn(p=params(top_k=0)) == E and fn(p=params(top_k=65)) == E
        for f in ("temperature", "top_p", "cfg_scale"):
            assert fn(p=params(**{f: float("nan")})) == E and fn(p=params(**{f: float("inf")})) == E, f
        assert fn(p=params(temperature=-0.5)) == E
        assert fn(p=params(top_p=0.0)) == E and fn(p=params(top_p=-1.0)) == E
    assert host(t=None) == E and dev(t=None) == E
    assert step(d=None) == E and step(st=None) == E and step(g=None) == E and step(a=None) == E
    assert step(d=(0, -1, 2)) == E                                                                        # a negative delay
    assert step(s=-1) == E and step(s=50) == E                                                            # step outside [0, L)
    assert step(M=51) == E                                                                                # max_tokens > L
    assert L.nc_dia_generate_state_init_dev(0, 0, state.ctypes.data, None) == E
    assert L.nc_dia_generate_state_init_dev(0, 2, None, None) == E
    assert (tok == -7).all() and (bad == -7).all() and (gen == -1).all()                                  # refused before anything is written
    assert host() == _lib.NC_OK and (tok >= 0).all()
    # lengths and collect
    ln, tg = (C.c_int64 * 2)(), C.c_int64()
    fin = _lib.i64_array([5, -1])
    assert L.nc_dia_generate_lengths(2, fin, _i32([1, 2]), 20, 3, ln, None) == _lib.NC_OK and list(ln) == [4, 15]     # T_gen_out nullable
    assert L.nc_dia_generate_lengths(0, fin, _i32([1, 2]), 20, 3, ln, C.byref(tg)) == E
    assert L.nc_dia_generate_lengths(2, None, _i32([1, 2]), 20, 3, ln, C.byref(tg)) == E
    assert L.nc_dia_generate_lengths(2, fin, None, 20, 3, ln, C.byref(tg)) == E
    assert L.nc_dia_generate_lengths(2, fin, _i32([1, 2]), 20, 3, None, C.byref(tg)) == E
    assert L.nc_dia_generate_lengths(2, fin, _i32([1, 2]), 20, -1, ln, C.byref(tg)) == E
    out = np.zeros((B, 60, Cn), np.int64)

    def coll(g=gen.ctypes.data, B_=B, Ln=50, C_=Cn, ps=(1, 2), n=(4, 15), md=3, o=out.ctypes.data):
        return L.nc_dia_generate_collect_dev(0, g, B_, Ln, C_, None if ps is None else _i32(list(ps)), None if n is None else _lib.i64_array(n), md, 65, o, None)

    assert coll(g=None) == E and coll(ps=None) == E and coll(n=None) == E and coll(o=None) == E
    assert coll(B_=0) == E and coll(C_=0) == E and coll(C_=33) == E and coll(md=-1) == E
    assert coll(n=(4, -1)) == E and coll(ps=(-1, 2)) == E
    assert coll(n=(0, 0), md=0) == E                                                                      # nothing was generated
    assert coll(n=(4, 46)) == E                                                                           # 2 + 46 + 3 > 50


@pytest.mark.skipif(_lib.lib().nc_device_count() > 0, reason="GPU present: covered by the gpu suite")
def test_device_calls_fail_loudly_without_a_device():
    L = _lib.lib()
    lg, u = np.zeros((2, 1, 8), np.float32), np.zeros((1, 1), np.float32)
    tok, bad = np.zeros((1, 1), np.int64), np.zeros(1, np.int32)
    p = _lib.NcDiaSampleParams(3.0, 1.2, 0.95, 4, 5, 6)
    assert L.nc_dia_sample_dev(0, lg.ctypes.data, 1, 1, 8, C.byref(p), u.ctypes.data, tok.ctypes.data, bad.ctypes.data, None) == _lib.NC_EDEVICE
    assert L.nc_dia_sample_host(lg.ctypes.data, 1, 1, 8, C.byref(p), u.ctypes.data, tok.ctypes.data, bad.ctypes.data) == _lib.NC_OK   # the host twin runs
