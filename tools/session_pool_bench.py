#!/usr/bin/env python3
"""Session-pool benchmark: N independent decode streams advanced tick by tick, three ways on the same build.

    python tools/session_pool_bench.py --out profiles/session_pool_bench.json

Workloads (synthetic weights, seeded; device-pointer calls on torch tensors):
  DAC 44.1 kHz decode, 8 and 32 streams, pushes of 16 and 32 frames, staggered starts (stream k joins at tick k mod 8)
  SNAC 24 kHz decode, 8 streams, pushes of 16 frames
Arms, alternated round by round:
  (a) sessions   one B = 1 nc_session per stream, pushed one after another every tick -- what a caller had before the pool: the baseline
  (b) pool       one nc_session_pool, one step per tick
  (c) lockstep   one nc_session with B = N on streams that all start at tick 0: the floor (no grouping, no tables)
  (b') SNAC only: the pool with noise == NULL, every entry drawing its own block (the cost of the per-entry draws)
One tick = every live stream pushes n frames; host clock around the tick with a stream synchronise behind it.  Only ticks in which every
stream is in steady state count (window = hl + n + hr frames).  Per round and arm: the median over those ticks; reported: median, min
and max over the rounds.  The bar of DESIGN.md 4g: (a) - (b) must exceed (a)'s min-max spread; `clears_bar` records it per workload."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralcodecs_amd import DAC, SNAC, DACConfig, SNACConfig, dac_halo, snac_halo  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob, snac_noise, snac_synthetic_state_dict, synthetic_pcm  # noqa: E402

STEADY_TICKS = 12


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3), "rounds": len(v)}


def _ticks(h, n, stagger):
    warm = -(-(h["dec_right"] + h["dec_left"]) // n) + 1            # pushes until a stream's window has both halos
    return warm + stagger, warm + stagger + STEADY_TICKS            # steady ticks: [first, last)


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _arm_sessions(m, N, n, first, last, join, cut):
    out = []
    ss = [m.decode_session(1) for _ in range(N)]
    try:
        for t in range(last):
            live = [k for k in range(N) if t >= join[k]]
            args = [cut(k, (t - join[k]) * n, n) for k in live]

            def tick():
                for k, (x, z) in zip(live, args):
                    ss[k].push(x, z) if z is not None else ss[k].push(x)
            dt = _timed(tick)
            if t >= first:
                out.append(dt)
    finally:
        for s in ss:
            s.close()
    return float(np.median(out))


def _arm_pool(m, N, n, first, last, join, cut, drawn=False):
    out = []
    with m.decode_pool(N) as pool:
        for t in range(last):
            live = [k for k in range(N) if t >= join[k]]
            args = {k: cut(k, (t - join[k]) * n, n) for k in live}
            entries = {k: a[0] for k, a in args.items()}
            noise = None if (drawn or args[live[0]][1] is None) else {k: a[1] for k, a in args.items()}
            dt = _timed(lambda: pool.step(entries, noise))
            if t >= first:
                out.append(dt)
    return float(np.median(out))


def _arm_lockstep(m, N, n, first, last, cut_all):
    out = []
    with m.decode_session(N) as s:
        for t in range(last):
            x, z = cut_all(t * n, n)
            dt = _timed(lambda: s.push(x, z) if z is not None else s.push(x))
            if t >= first:
                out.append(dt)
    return float(np.median(out))


def _workload(model, m, h, N, n, cut, cut_all, rounds, extra_drawn=False):
    join = [k % 8 for k in range(N)]
    first, last = _ticks(h, n, max(join))
    arms = {"sessions": [], "pool": [], "lockstep": []}
    if extra_drawn:
        arms["pool_drawn_noise"] = []
    for r in range(rounds + 1):                                     # round 0 warms every arm up and is dropped
        vals = {"sessions": _arm_sessions(m, N, n, first, last, join, cut), "pool": _arm_pool(m, N, n, first, last, join, cut),
                "lockstep": _arm_lockstep(m, N, n, first - max(join), last - max(join), cut_all)}
        if extra_drawn:
            vals["pool_drawn_noise"] = _arm_pool(m, N, n, first, last, join, cut, drawn=True)
        if r:
            for k, v in vals.items():
                arms[k].append(v)
    res = {"model": model, "streams": N, "push_frames": n, "halo_left": h["dec_right"], "halo_right": h["dec_left"],
           "steady_ticks": STEADY_TICKS, **{k: _stats(v) for k, v in arms.items()}}
    a, b = res["sessions"], res["pool"]
    res["sessions_spread_ms"] = round(a["max_ms"] - a["min_ms"], 3)
    res["gain_ms"] = round(a["median_ms"] - b["median_ms"], 3)
    res["speedup"] = round(a["median_ms"] / b["median_ms"], 3)
    res["clears_bar"] = bool(res["gain_ms"] > res["sessions_spread_ms"])
    print(json.dumps(res), flush=True)
    return res


def bench_dac(rounds):
    import torch
    cfg = DACConfig.dac_44khz()
    h = dac_halo(cfg)
    dev = torch.device("cuda", 0)
    out = []
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=3)))
        for N in (8, 32):
            for n in (16, 32):
                _, last = _ticks(h, n, 7)
                pcm = torch.from_numpy(synthetic_pcm(N, 1, last * n * cfg.hop_length, cfg.sample_rate, seed=31)).to(dev)
                codes = m.encode(pcm)[1].contiguous()
                out.append(_workload("dac_44khz", m, h, N, n, lambda k, o, c: (codes[k:k + 1, :, o:o + c], None),
                                     lambda o, c: (codes[:, :, o:o + c], None), rounds))
    return out


def bench_snac(rounds):
    import torch
    cfg = SNACConfig.snac_24khz()
    h = snac_halo(cfg)
    dev = torch.device("cuda", 0)
    N, n = 8, 16
    with SNAC(cfg) as m:
        m.load_blob(save_blob(snac_synthetic_state_dict(cfg, seed=4)))
        _, last = _ticks(h, n, 7)
        frames = last * n
        pcm = torch.from_numpy(synthetic_pcm(N, 1, frames * cfg.hop_length, cfg.sampling_rate, seed=32)).to(dev)
        codes = [c.contiguous() for c in m.encode(pcm)]
        noises = [torch.from_numpy(z).to(dev) for z in snac_noise(cfg, N, frames, seed=33)] if cfg.noise else None

        def cut(k, o, c, rows=1):
            x = [lv[k:k + rows, o // s:(o + c) // s] for lv, s in zip(codes, cfg.vq_strides)]
            z = [b[k:k + rows, :, o * (b.shape[-1] // frames):(o + c) * (b.shape[-1] // frames)] for b in noises] if noises else None
            return x, z

        return [_workload("snac_24khz", m, h, N, n, cut, lambda o, c: cut(0, o, c, N), rounds, extra_drawn=bool(noises))]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_pool_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if a.rounds < 7:
        raise SystemExit("at least 7 rounds")
    import torch
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "results": bench_dac(a.rounds) + bench_snac(a.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
