#!/usr/bin/env python3
"""Dia prompt-stage benchmark: voice prompts of a batch to the delayed prefill, two ways on the same build.

    python tools/dia_prompt_bench.py --out profiles/dia_prompt_bench.json

Workload (synthetic weights, seeded): DAC 44.1 kHz, Dia's delay pattern [0, 8, 9, ..., 15] on 9 codebooks, 16 mono prompts of 1 to 10 s
(drawn once), batch size 16.  Both arms start from the prompts in device memory and end with the int32 prefill [B, T_max, C] in device
memory, timed to a device synchronise, alternated round by round:
  (a) loop   what the reference's structure implies for a caller of this library: one encode_to_code_matrix per prompt at batch 1, the
             codes downloaded, PrepareAudioPrompt composed on the host (numpy: full(-1), the BOS row, the copies, the delay gather), the
             prefill uploaded
  (b) call   DAC.encode_dia_prompts on the device tensors: the ragged encode of all prompts and one prefill launch, nothing downloaded
Per round and arm one timed call behind one untimed; reported: median, min and max over the rounds.
The prefill kernel on its own (nc_dia_prefill_pack_dev on the packed codes of the same prompts): HIP events around `reps` back-to-back
launches, the time of one launch and the bytes it moves (8 * C * sum F read, 4 * B * T_max * C written).  A measurement, not a bar."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralcodecs_amd import DAC, DACConfig, _lib  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402

DELAY = [0, 8, 9, 10, 11, 12, 13, 14, 15]
BOS = 1026


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3), "rounds": len(v)}


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _host_prepare(prompts_TC, batch, delay, bos):
    """Dia.PrepareAudioPrompt on the host: [F, C] codes per prompt -> int32 [B, T_max, C]"""
    Cn, md = len(delay), max(delay)
    B = max(batch, len(prompts_TC))
    T = max(p.shape[0] for p in prompts_TC) + md
    prefill = np.full((B, T, Cn), -1, np.int32)
    prefill[:, 0, :] = bos
    for i, p in enumerate(prompts_TC):
        n = min(p.shape[0], T - 1)
        prefill[i, 1:n + 1, :] = p[:n]
    out = np.empty_like(prefill)
    for c in range(Cn):
        t = np.arange(T) - delay[c]
        out[:, :, c] = np.where(t < 0, bos, prefill[:, np.clip(t, 0, T - 1), c])
    return out


def _arm_loop(m, prompts, dev):
    import torch
    codes = [m.encode_to_code_matrix(p[None, :]) for p in prompts]
    host = [c.cpu().numpy() for c in codes]
    return torch.from_numpy(_host_prepare(host, len(prompts), DELAY, BOS)).to(dev)


def _kernel_alone(codes_CF, reps):
    """one prefill launch on the packed codes of the prompts: ms per launch from HIP events around `reps` launches"""
    import torch
    L = _lib.lib()
    frames = [int(c.shape[1]) for c in codes_CF]
    B, Cn, T = len(frames), len(DELAY), max(frames) + max(DELAY)
    flat = torch.cat([c.reshape(-1) for c in codes_CF]).contiguous()
    out = torch.empty((B, T, Cn), dtype=torch.int32, device=flat.device)
    fr, dl = _lib.i64_array(frames), (C.c_int32 * Cn)(*DELAY)
    stream = torch.cuda.current_stream(flat.device).cuda_stream

    def launch():
        _lib.check(L.nc_dia_prefill_pack_dev(flat.device.index or 0, flat.data_ptr(), B, fr, Cn, dl, BOS, -1, T, out.data_ptr(), stream))

    for _ in range(10):
        launch()
    per = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) / reps)
    read, written = 8 * Cn * sum(frames), 4 * B * T * Cn
    ms = float(np.median(per))
    return {"launch_us_median": round(ms * 1e3, 3), "launch_us_min": round(min(per) * 1e3, 3), "launch_us_max": round(max(per) * 1e3, 3), "reps": reps,
            "bytes_read": read, "bytes_written": written, "gb_per_s": round((read + written) / (ms * 1e-3) / 1e9, 2), "T_max": T}


def bench(rounds):
    import torch
    cfg = DACConfig.dac_44khz()
    dev = torch.device("cuda", 0)
    B = 16
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=3)))
        rng = np.random.default_rng(56)
        lens = [int(s * cfg.sample_rate) for s in rng.uniform(1.0, 10.0, B)]
        prompts = [torch.from_numpy(synthetic_pcm(1, 1, t, cfg.sample_rate, seed=90 + i)[0, 0]).to(dev) for i, t in enumerate(lens)]
        fns = {"loop": lambda: _arm_loop(m, prompts, dev), "call": lambda: m.encode_dia_prompts(prompts, B, DELAY, BOS)[0]}
        arms = {k: [] for k in fns}
        last = {}
        for r in range(rounds + 1):                                 # round 0 warms every arm up and is dropped
            for k, fn in fns.items():
                fn()
                dt, last[k] = _timed(fn)
                if r:
                    arms[k].append(dt)
        same = bool(torch.equal(last["loop"], last["call"]))
        frames = [m.frames(t) for t in lens]
        res = {"model": "dac_44khz", "items": B, "samples_min": min(lens), "samples_max": max(lens), "frames_total": sum(frames),
               "arms_agree": same, **{k: _stats(v) for k, v in arms.items()}}
        res["loop_spread_ms"] = round(res["loop"]["max_ms"] - res["loop"]["min_ms"], 3)
        res["speedup_call"] = round(res["loop"]["median_ms"] / res["call"]["median_ms"], 3)
        res["prefill_kernel"] = _kernel_alone(m.encode_ragged(prompts), 200)
        print(json.dumps(res), flush=True)
    return [res]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dia_prompt_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if a.rounds < 7:
        raise SystemExit("at least 7 rounds")
    import torch
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "results": bench(a.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
