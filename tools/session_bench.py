#!/usr/bin/env python3
"""Incremental-session benchmark: what a decode session costs per push, beside the one-shot decode of the same sequence.

    python tools/session_bench.py --out profiles/session_bench.json

Workloads (synthetic weights, seeded; device-pointer calls on torch tensors):
  DAC 44.1 kHz decode, B = 1 and B = 8, pushes of 16, 32 and 64 frames
  SNAC 24 kHz decode, B = 1, pushes of 16 and 32 frames
One measurement = the whole sequence (--seconds of audio) pushed piece by piece, host clock around every push with a stream
synchronise behind it (what a caller that plays the audio waits for), then the flush.  Recorded per workload: the audio duration of one
push, the median / min / max milliseconds of the pushes in steady state (the ones whose window has both halos), the session's total,
the one-shot decode of the same codes (from_codes + decode for DAC: the baseline, unchanged by sessions) and the expected ratio of work
(hl + n + hr) / n.  No threshold is applied: the figures are a record."""
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


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3), "n": len(v)}


def _run(model, rate, hop, h, B, frames, n, push_args, one_shot, warmup, reps):
    """push_args(o, n) -> (x, noise) for frames [o, o + n); one_shot() decodes the whole sequence"""
    import torch
    hl, hr = h["dec_right"], h["dec_left"]
    steady, totals, ones = [], [], []
    for it in range(warmup + reps):
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        with model.decode_session(B) as s:
            for o in range(0, frames, n):
                k = min(n, frames - o)
                x, nz = push_args(o, k)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.push(x, nz)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if it >= warmup and k == n and o >= hl + hr + n:
                    steady.append(dt)
            s.flush()
            torch.cuda.synchronize()
        if it >= warmup:
            totals.append((time.perf_counter() - t_all) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_shot()
        torch.cuda.synchronize()
        if it >= warmup:
            ones.append((time.perf_counter() - t0) * 1e3)
    return {"B": B, "push_frames": n, "frames": frames, "halo_left": hl, "halo_right": hr,
            "push_audio_ms": round(1e3 * n * hop / rate, 3), "latency_audio_ms": round(1e3 * hr * hop / rate, 3),
            "expected_work_ratio": round((hl + n + hr) / n, 3), "push": _stats(steady), "session_total": _stats(totals),
            "one_shot": _stats(ones), "total_over_one_shot": round(float(np.median(totals) / np.median(ones)), 3)}


def bench_dac(seconds, warmup, reps):
    import torch
    cfg = DACConfig.dac_44khz()
    h = dac_halo(cfg)
    dev = torch.device("cuda", 0)
    out = []
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=3)))
        for B in (1, 8):
            pcm = torch.from_numpy(synthetic_pcm(B, 1, int(seconds * cfg.sample_rate), cfg.sample_rate, seed=31)).to(dev)
            codes = m.encode(pcm)[1].contiguous()
            frames = int(codes.shape[-1])
            for n in (16, 32, 64):
                r = _run(m, cfg.sample_rate, cfg.hop_length, h, B, frames, n, lambda o, k: (codes[:, :, o:o + k], None),
                         lambda: m.decode(m.from_codes(codes)), warmup, reps)
                out.append(dict(model="dac_44khz", **r))
                print(json.dumps(out[-1]), flush=True)
    return out


def bench_snac(seconds, warmup, reps):
    import torch
    cfg = SNACConfig.snac_24khz()
    h = snac_halo(cfg)
    dev = torch.device("cuda", 0)
    out = []
    with SNAC(cfg) as m:
        m.load_blob(save_blob(snac_synthetic_state_dict(cfg, seed=4)))
        frames = int(seconds * cfg.sampling_rate) // cfg.hop_length // 32 * 32
        pcm = torch.from_numpy(synthetic_pcm(1, 1, frames * cfg.hop_length, cfg.sampling_rate, seed=32)).to(dev)
        codes = [c.contiguous() for c in m.encode(pcm)]
        noises = [torch.from_numpy(z).to(dev) for z in snac_noise(cfg, 1, frames, seed=33)] if cfg.noise else None

        def args(o, k):
            c = [lv[:, o // s:(o + k) // s] for lv, s in zip(codes, cfg.vq_strides)]
            z = [b[:, :, o * (b.shape[-1] // frames):(o + k) * (b.shape[-1] // frames)] for b in noises] if noises else None
            return c, z

        for n in (16, 32):
            r = _run(m, cfg.sampling_rate, cfg.hop_length, h, 1, frames, n, args, lambda: m.decode(codes, noises), warmup, reps)
            out.append(dict(model="snac_24khz", **r))
            print(json.dumps(out[-1]), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_bench.json"))
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "seconds": a.seconds, "warmup": a.warmup, "reps": a.reps,
           "results": bench_dac(a.seconds, a.warmup, a.reps) + bench_snac(a.seconds, a.warmup, a.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
