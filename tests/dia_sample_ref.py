"""Numpy restatements of Dia's sampling stage (include/nc_mi355x.h "Dia sampling stage"), the truth of
tests/test_dia_sample_cpu.py and tests/test_dia_sample_gpu.py.

    sample_row32   the definition operation by operation in binary32 (numpy float32 scalars, nc_expf rebuilt on fma32): exact
    sample_row64   guidance, masks and the division as the definition rounds them (they ARE the definition), then softmax, cumulative sums
                   and the inverse CDF in binary64; also returns how close a cumulative value comes to top_p and to u
    step_closed_form / lengths / collect   the bookkeeping of one generation step and the final copy, on numpy arrays
"""
import numpy as np

from dia_output_ref import fma32

F = np.float32
NINF = F(-np.inf)


def expf32(x):
    """nc_expf (csrc/nc_math.h) on binary32 values, element by element"""
    x = np.clip(np.asarray(x, F), F(-87.0), F(88.0))
    n = np.rint((x * F(float.fromhex("0x1.715476p+0"))).astype(F)).astype(F)
    r = fma32(n, F(float.fromhex("-0x1.62e400p-1")), x)
    r = fma32(n, F(float.fromhex("-0x1.7f7d1cp-20")), r)
    q = np.full(x.shape, F(float.fromhex("0x1.6d5accp-10")), F)
    for k in ("0x1.121f36p-7", "0x1.5554d8p-5", "0x1.5554cap-3", "0x1.000000p-1"):
        q = fma32(q, r, F(float.fromhex(k)))
    e = (fma32((r * r).astype(F), q, r) + F(1.0)).astype(F)
    sc = ((n.astype(np.int32) + 127) << 23).astype(np.uint32).view(F)
    return (e * sc).astype(F)


def guided(uncond, cond, c, cfg_scale, eos):
    """steps 1 and 2 on one row, binary32"""
    uncond, cond = np.asarray(uncond, F), np.asarray(cond, F)
    with np.errstate(invalid="ignore", over="ignore"):
        g = (cond + (F(cfg_scale) * (cond - uncond)).astype(F)).astype(F)
        v = np.arange(g.shape[0])
        g[v > eos] = NINF
        if c >= 1:
            g[v >= eos] = NINF
        else:
            g[eos] = F(g[eos] * F(0.8))
    return g


def argmax_aten(g):
    """first maximum; a NaN beats every number, first NaN wins"""
    nan = np.isnan(g)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(g))


def _survivors(uncond, cond, c, p, want_greedy=True):
    """steps 1-6: (token, None) where the row is decided already (greedy: token; bad: -1), else (None, (x of the survivors, indices))"""
    g = guided(uncond, cond, c, p["cfg_scale"], p["eos"])
    top = argmax_aten(g)
    if F(p["temperature"]) < F(1e-5):
        return top, None
    if np.isnan(g).any():
        return -1, None
    if top != p["eos"]:
        g[p["eos"]] = NINF
    with np.errstate(over="ignore"):
        x = (g / F(p["temperature"])).astype(F)
    idx = np.flatnonzero(x > NINF)
    idx = idx[np.argsort(-x[idx].astype(np.float64), kind="stable")][:p["top_k"]]      # value descending, index ascending
    if idx.size == 0 or x[idx[0]] == F(np.inf):
        return -1, None
    return None, (x[idx], idx)


def sample_row32(uncond, cond, c, p, u):
    """the token of one row by the definition, every operation in binary32; p: dict of cfg_scale, temperature, top_p, top_k, eos"""
    tok, sv = _survivors(uncond, cond, c, p)
    if sv is None:
        return tok
    x, idx = sv
    e = expf32((x - x[0]).astype(F))
    kept = [True] * len(e)
    if F(p["top_p"]) < F(1.0):
        S = F(0.0)
        for ej in e:
            S = F(S + ej)
        cum = F(0.0)
        for j, ej in enumerate(e):
            if j >= 1 and cum > F(p["top_p"]):
                kept[j] = False
            cum = F(cum + F(ej / S))
    S2 = F(0.0)
    for j, ej in enumerate(e):
        if kept[j]:
            S2 = F(S2 + ej)
    d, last = F(0.0), 0
    for j, ej in enumerate(e):
        if not kept[j]:
            continue
        d = F(d + F(ej / S2))
        last = j
        if F(u) < d:
            return int(idx[j])
    return int(idx[last])


def sample_row64(uncond, cond, c, p, u):
    """(token, margin): the inverse-CDF token with softmax and cumulative sums in binary64, and the least distance of a cumulative value
    from top_p (where a nucleus is cut) or from u; margin None: the row is decided without a draw"""
    tok, sv = _survivors(uncond, cond, c, p)
    if sv is None:
        return tok, None
    x, idx = sv
    e = np.exp(x.astype(np.float64) - np.float64(x[0]))
    margin = np.inf
    kept = np.ones(e.size, bool)
    if F(p["top_p"]) < F(1.0):
        cum = np.cumsum(e / e.sum())
        kept[1:] = ~(cum[:-1] > np.float64(F(p["top_p"])))
        margin = min(margin, float(np.abs(cum - np.float64(F(p["top_p"]))).min()))
    q = np.where(kept, e, 0.0)
    d = np.cumsum(q / q.sum())
    margin = min(margin, float(np.abs(d[kept] - np.float64(F(u))).min()))
    hit = np.flatnonzero(kept & (np.float64(F(u)) < d))
    j = int(hit[0]) if hit.size else int(np.flatnonzero(kept)[-1])
    return int(idx[j]), margin


def sample32(logits, p, uniform):
    """every row of logits [2B, C, V] by sample_row32 -> (tokens int64 [B, C], bad int32 [B])"""
    B, Cn = logits.shape[0] // 2, logits.shape[1]
    tok = np.array([[sample_row32(logits[2 * b, c], logits[2 * b + 1, c], c, p, uniform[b, c]) for c in range(Cn)] for b in range(B)], np.int64)
    return tok, (tok < 0).any(axis=1).astype(np.int32)


# ---- bookkeeping ------------------------------------------------------------------------------------------------------------------------
def new_state(B):
    return np.stack([np.zeros(B, np.int64), np.full(B, -1, np.int64), np.full(B, -1, np.int64)])


def step_closed_form(state, generated, tok, step, max_tokens, delay, eos, pad, apply_mask):
    """one generation step on numpy arrays, in place: state int64 [3, B], generated int32 [B, L, C], tok int64 [B, C] -> active [B]"""
    D = max(delay)
    for b in range(tok.shape[0]):
        det, cdn, fin = (int(v) for v in state[:, b])
        t = [int(v) for v in tok[b]]
        trigger = cdn != 0 and ((not det and t[0] == eos) or step >= max_tokens - D)
        det = 1 if (det or trigger) else 0
        if trigger and cdn < 0:
            cdn, fin = D, step
        if cdn > 0:
            a = D - cdn
            t = [eos if a == dc else pad if a > dc else v for v, dc in zip(t, delay)]
            cdn -= 1
        for c, v in enumerate(t):
            if not apply_mask or generated[b, step, c] == -1:
                generated[b, step, c] = v
        state[:, b] = (det, cdn, fin)
    return state[1] != 0


def lengths(finished, prefill_steps, final_step, maxd):
    f = np.where(np.asarray(finished) == -1, final_step - maxd, np.asarray(finished))
    n = np.maximum(0, f - np.asarray(prefill_steps))
    return [int(v) for v in n], int(n.max()) + maxd


def collect(generated, prefill_steps, lens, maxd, pad):
    T = max(lens) + maxd
    out = np.full((generated.shape[0], T, generated.shape[2]), pad, np.int64)
    for b, (s, n) in enumerate(zip(prefill_steps, lens)):
        out[b, :n + maxd] = generated[b, s:s + n + maxd]
    return out


# ---- the cases both suites run --------------------------------------------------------------------------------------------------------
DEFAULTS = dict(cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos=1024, pad=1025)
RANDOM_PARAMS = ((1.3, 0.95, 45, 3.0), (1.0, 0.8, 45, 3.0), (0.7, 0.5, 64, 1.0), (1.8, 0.99, 10, 5.0))     # (T, p, k, s)


def random_cases():
    """N(0, 3) logits, V = 1028, B = 8, C = 9: three draws per parameter set, 864 rows in all"""
    out = []
    for i, (T, tp, k, s) in enumerate(RANDOM_PARAMS):
        for seed in range(3):
            rng = np.random.default_rng(1000 + 10 * i + seed)
            lg = (rng.standard_normal((16, 9, 1028)) * 3).astype(F)
            out.append((f"random_T{T}_p{tp}_k{k}_s{s}_{seed}", lg, dict(DEFAULTS, temperature=T, top_p=tp, top_k=k, cfg_scale=s),
                        rng.random((8, 9)).astype(F)))
    return out


def edge_cases():
    """(name, logits [2B, C, V], params, uniform [B, C]) at the edges of the definition; small: V in {65, 68, 70}"""
    out = []
    base = dict(DEFAULTS, eos=64, pad=65)

    def rows(seed, B=2, Cn=3, V=68, scale=3.0):
        rng = np.random.default_rng(seed)
        return (rng.standard_normal((2 * B, Cn, V)) * scale).astype(F), rng.random((B, Cn)).astype(F)

    for k in (1, 45, 64):
        lg, u = rows(10 + k)
        out.append((f"top_k_{k}", lg, dict(base, top_k=k), u))
    lg, u = rows(20, V=70)
    out.append(("top_k_above_the_finite_logits", lg, dict(base, eos=10, pad=11, top_k=45), u))
    lg, u = rows(21)
    out.append(("top_p_1_no_nucleus", lg, dict(base, top_p=1.0), u))
    out.append(("top_p_2_no_nucleus", lg, dict(base, top_p=2.0), u))
    out.append(("top_p_tiny_only_the_first", lg, dict(base, top_p=1e-6), u))
    rng = np.random.default_rng(22)                                                      # few levels, uncond == cond: g == cond, ties everywhere
    lv = rng.integers(-2, 3, (2, 3, 68)).astype(F)
    lg = np.repeat(lv, 2, axis=0)
    for k, tp in ((5, 0.95), (20, 0.5), (45, 0.9), (64, 1.0)):
        out.append((f"ties_k{k}_p{tp}", lg, dict(base, top_k=k, top_p=tp, temperature=1.0), rng.random((2, 3)).astype(F)))
    lg, u = rows(23)
    hi = lg.copy()
    hi[1::2, 0, 64] = 40.0                                                               # EOS the highest on channel 0 (and guided up)
    out.append(("eos_highest_on_channel_0", hi, base, u))
    out.append(("eos_highest_greedy", hi, dict(base, temperature=0.0), u))
    lo = lg.copy()
    lo[1::2, 0, 64] = lg[1::2, 0, :64].max(axis=-1) - F(0.5)                             # a likely EOS that is not the argmax: struck out
    out.append(("eos_not_highest_on_channel_0", lo, dict(base, cfg_scale=0.0), u))
    out.append(("u_zero", lg, base, np.zeros_like(u)))
    out.append(("u_just_below_one", lg, base, np.full_like(u, np.nextafter(F(1.0), F(0.0)))))
    out.append(("u_just_below_one_no_nucleus", lg, dict(base, top_p=1.0, top_k=64), np.full_like(u, np.nextafter(F(1.0), F(0.0)))))
    lg, u = rows(24, V=65)
    out.append(("V_65", lg, dict(base, eos=64), u))
    out.append(("V_65_eos_low", lg, dict(base, eos=33, pad=34), u))
    lg, u = rows(25)
    out.append(("greedy", lg, dict(base, temperature=0.0), u))
    out.append(("greedy_below_the_threshold", lg, dict(base, temperature=9e-6), u))
    out.append(("temperature_at_the_threshold", lg, dict(base, temperature=1e-5), u))   # sampled, not greedy: x is about 1e6, nothing overflows
    bad = lg.copy()
    bad[:, 1, :] = -np.inf                                                               # both rows -inf: (-inf) - (-inf), a row of NaN
    bad[1, 2, 5] = np.inf                                                                # one +inf
    bad[3, 0, 7] = np.nan                                                                # a NaN
    bad[2, 2, 66] = np.nan                                                               # a NaN behind eos: masked, harmless
    out.append(("bad_rows", bad, base, u))
    out.append(("bad_rows_greedy", bad, dict(base, temperature=0.0), u))
    none = lg.copy()                                                                     # conditional -inf, unconditional finite, cfg_scale > 0:
    none[1, 0, :] = -np.inf                                                              # every guided logit is -inf, no NaN -- no survivor; on
    none[1, 2, :] = -np.inf                                                              # channel 0 (the EOS entry -inf * 0.8 too) and on channel 2
    assert np.isfinite(none[0]).all() and (guided(none[0, 0], none[1, 0], 0, 3.0, 64) == NINF).all() and (guided(none[0, 2], none[1, 2], 2, 3.0, 64) == NINF).all()
    out.append(("no_survivor", none, base, u))
    out.append(("no_survivor_no_nucleus", none, dict(base, top_p=1.0, top_k=1), u))
    over = np.clip(lg, -3, 3) * F(1e35)                                                  # finite g, the division overflows: item 0 to -inf
    over[0:2] = -np.abs(over[0:2]) - F(1e35)                                             # everywhere (no survivor), item 1 to +inf survivors
    over[2:4, :, 3] = F(3e35)
    out.append(("overflow_through_the_division", over.astype(F), dict(base, cfg_scale=0.0, temperature=1e-4), u))
    nan_eos = lg.copy()
    nan_eos[1, 0, 64] = np.nan                                                           # the only NaN sits on eos
    out.append(("nan_on_eos", nan_eos, base, u))
    lg, u = rows(26, B=1, Cn=32, V=68)
    out.append(("C_32", lg, base, u))
    lg, u = rows(27, B=8, Cn=9, V=70, scale=2.0)
    out.append(("B_8", lg, base, u))
    lg, u = rows(28, B=1, Cn=1, V=65)
    out.append(("C_1", lg, dict(base, eos=0, pad=1, top_k=1), u))
    return out


# ---- the reference, statement by statement, on torch CPU tensors (Models/Dia.cs) ------------------------------------------------------
def torch_guided_logits(logits, cfg_scale, eos):
    """Dia.cs:531-548: logits float32 [2B, C, V] -> the guided and masked logits [B, C, V]"""
    import torch
    lg = torch.as_tensor(logits).view(logits.shape[0] // 2, 2, logits.shape[1], logits.shape[2])
    uncond, cond = lg[:, 0, :, :], lg[:, 1, :, :]
    out = cond + (cfg_scale * (cond - uncond))
    out[:, :, eos + 1:].fill_(float("-inf"))
    out[:, 1:, eos:].fill_(float("-inf"))
    out[:, 0, eos].mul_(0.8)
    return out


def torch_sample_next_token(logits, temperature, top_p, top_k, eos):
    """Dia.cs:424-501 up to the draw: logits [N, V] -> ("greedy", argmax) or ("probs", finalProbs)"""
    import torch
    if temperature < 1e-5:
        return "greedy", torch.argmax(logits, dim=-1)
    top = torch.argmax(logits, dim=-1)
    mask = torch.zeros_like(logits, dtype=torch.bool)
    mask[top.ne(eos), eos] = True
    logits = logits.masked_fill(mask, float("-inf"))
    logits = logits.div(temperature)
    _, indices = torch.topk(logits, k=top_k, dim=-1)
    mask = torch.ones_like(logits, dtype=torch.bool)
    mask.scatter_(-1, indices, torch.zeros_like(indices, dtype=torch.bool))
    logits.masked_fill_(mask, float("-inf"))
    if top_p < 1.0:
        probs = torch.softmax(logits, dim=-1)
        sorted_probs, sorted_indices = torch.sort(probs, dim=-1, descending=True)
        cumulative = torch.cumsum(sorted_probs, dim=-1)
        remove = cumulative.gt(top_p)
        remove = torch.roll(remove, shifts=1, dims=-1)
        remove[..., 0] = False
        to_remove = torch.zeros_like(remove)
        to_remove.scatter_(-1, sorted_indices, remove)
        logits.masked_fill_(to_remove, float("-inf"))
    return "probs", torch.softmax(logits, dim=-1)


def torch_generate(tables, delay, max_tokens, prefill, prefill_steps, eos, pad, cfg_scale=3.0):
    """The loop of Dia.Generate (Dia.cs:664-801) at temperature 0 around a fake language model: tables[s] holds the logits
    [2B, C, V] of step s (currentStepIdx).  generated is DecoderOutput.GeneratedTokens of max_tokens steps with the prefill copied in.
    -> dict(snapshots = per step (generated, detected, countdown, finished), steps, lengths, codes)"""
    import torch
    B, Cn = prefill.shape[0], len(delay)
    D = max(delay)
    delay_t = torch.tensor(delay, dtype=torch.int64)
    generated = torch.full((B, max_tokens, Cn), -1, dtype=torch.int32)
    generated[:, :prefill.shape[1], :] = torch.as_tensor(prefill)
    dec_step = min(prefill_steps) - 1
    detected = torch.zeros(B, dtype=torch.bool)
    countdown = torch.full((B,), -1, dtype=torch.int64)
    finished = torch.full((B,), -1, dtype=torch.int64)
    bos_over, snaps = False, []
    while dec_step < max_tokens:
        if bool(countdown.eq(0).all()):
            break
        s = dec_step + 1
        guided_l = torch_guided_logits(tables[s], cfg_scale, eos)
        _, pred = torch_sample_next_token(guided_l.reshape(B * Cn, -1).to(torch.float32), 0.0, 0.95, 45, eos)
        pred = pred.view(B, Cn)
        active = countdown.ne(0)
        trigger = torch.zeros_like(active)
        if bool(active.any()):
            is_eos = detected[active].logical_not().logical_and(pred[active, 0].eq(eos))
            is_max = s >= max_tokens - D
            trigger[active] = is_eos.logical_or(torch.tensor(is_max))
        detected = detected.logical_or(trigger)
        start = trigger.logical_and(countdown.lt(0))
        if bool(start.any()):
            countdown[start] = D
            finished[start] = s
        padding = countdown.gt(0)
        if bool(padding.any()):
            pa = pred[padding].clone()
            after = (D - countdown[padding]).unsqueeze(1)
            pa[after.eq(delay_t.unsqueeze(0))] = eos
            pa[after.gt(delay_t.unsqueeze(0))] = pad
            pred[padding] = pa
            countdown[padding] -= 1
        if not bos_over:
            bos_over = all(dec_step - p > D for p in prefill_steps)
        dec = pred.to(generated.dtype)                                                   # DecoderOutput.UpdateOne
        if not bos_over:
            cur = generated[:, s, :]
            generated[:, s, :] = torch.where(cur.eq(-1), dec, cur)
        else:
            generated[:, s, :] = dec
        dec_step += 1
        snaps.append((generated.numpy().copy(), detected.numpy().astype(np.int64), countdown.numpy().copy(), finished.numpy().copy()))
    final_step = dec_step + 1
    finished = finished.clone()
    finished[finished == -1] = final_step - D
    lens = torch.clamp(finished - torch.tensor(prefill_steps), min=0)
    max_len = int(lens.max()) + D
    codes = torch.full((B, max_len, Cn), pad, dtype=torch.int64)
    for i in range(B):
        n = int(lens[i]) + D
        if n > 0:
            codes[i, :n, :] = generated[i, prefill_steps[i]:prefill_steps[i] + n, :]
    return dict(snaps=snaps, steps=len(snaps), final_step=final_step, lengths=[int(v) for v in lens], codes=codes.numpy())


def loop_cases():
    """(name, dict) of the generation loops both suites run: fake-LM tables with EOS on channel 0 held down except at chosen steps"""
    out = []
    eos, pad, bos, V = 64, 65, 66, 68
    for name, delay, frames, M, eos_at in (
            ("dia_pattern", [0, 8, 9, 10, 11, 12, 13, 14, 15], [2, 1, 3], 42, {0: 6, 1: 12}),      # early, during 0's countdown, by max_tokens - D
            ("no_delay", [0, 0, 0, 0], [2, 0, 1], 42, {0: 5, 1: 9, 2: 30}),
            ("one_channel", [3], [1, 4], 42, {0: 7})):
        rng = np.random.default_rng(len(delay) * 100 + M)
        B, Cn, D = len(frames), len(delay), max(delay)
        T = max(frames) + D
        prefill = np.full((B, max(T, 1), Cn), -1, np.int32)
        for b, Fb in enumerate(frames):
            for c, dc in enumerate(delay):
                for t in range(prefill.shape[1]):
                    s = t - dc
                    prefill[b, t, c] = bos if s <= 0 else int(rng.integers(0, 64)) if s <= Fb else -1
        tables = (rng.standard_normal((M + 1, 2 * B, Cn, V)) * 2).astype(F)
        tables[:, :, 0, eos] = -300.0
        for b, s in eos_at.items():
            tables[s, 2 * b:2 * b + 2, 0, eos] = 300.0
        out.append((name, dict(delay=delay, max_tokens=M, prefill=prefill, prefill_steps=[f + 1 for f in frames], tables=tables, eos=eos, pad=pad,
                               V=V, B=B, C=Cn)))
    return out
