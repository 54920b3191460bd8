#!/usr/bin/env python3
"""Dia output-stage benchmark: delayed codes of a batch of generations to waveforms, two ways on the same build.

    python tools/dia_output_bench.py --out profiles/dia_output_bench.json

Workload (synthetic weights, seeded): DAC 44.1 kHz, Dia's delay pattern [0, 8, 9, ..., 15] on 9 codebooks, 8 and 32 items of 2 to 10 s
(172 to 861 frames, drawn once per batch size), every item slowed to speed 0.9.
Arms, alternated round by round, both from the delayed codes in host memory to the waveforms in host memory:
  (a) loop       what the reference's structure implies for a caller of this library: the delay reverted, cut and masked on the host
                 (numpy), one decode_code_matrix per item at batch 1, the speed adjustment by numpy interpolation on the host
  (b) call       DAC.decode_dia_output on the host array: one upload, revert-and-pack, the ragged decode, one interpolation launch,
                 one download
  (b') call_dev  the same call on a device tensor, the waveforms left on the device (what a caller whose language model runs on the GPU
                 sees), timed to a device synchronise
Per round and arm one timed call behind one untimed; reported: median, min and max over the rounds.  A measurement, not a bar."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralcodecs_amd import DAC, DACConfig  # noqa: E402
from neuralcodecs_amd.dia import adjust_speed_len  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob  # noqa: E402

DELAY = [0, 8, 9, 10, 11, 12, 13, 14, 15]
SPEED = 0.9


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3), "rounds": len(v)}


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _host_revert(codes, delay):
    B, T, C = codes.shape
    md = max(delay)
    out = np.empty((B, T - md, C), np.int64)
    for c in range(C):
        out[:, :, c] = codes[:, np.minimum(np.arange(T - md) + delay[c], T - 1), c]
    out[(out < 0) | (out > 1023)] = 0
    return out


def _host_interp(fp, speed):
    """Dia.AdjustSpeed on the host in binary32 (positions in binary64 here: this arm is timed, not compared)"""
    L = fp.shape[0]
    T = adjust_speed_len(L, speed)
    if T == L:
        return fp
    x = np.linspace(0, L - 1, T).astype(np.float32)
    idx = np.clip(np.ceil(x).astype(np.int64) - 1, 0, L - 2)
    offset = fp[idx + 1] - fp[idx]
    return offset * x + (fp[idx] - offset * idx.astype(np.float32))


def _arm_loop(m, codes, lens):
    rev = _host_revert(codes, DELAY)
    return [_host_interp(m.decode_code_matrix(np.ascontiguousarray(rev[b, :n, :])), SPEED) for b, n in enumerate(lens)]


def bench(rounds):
    import torch
    cfg = DACConfig.dac_44khz()
    fps = cfg.sample_rate / cfg.hop_length
    dev = torch.device("cuda", 0)
    out = []
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=3)))
        for B in (8, 32):
            rng = np.random.default_rng(40 + B)
            lens = [int(s * fps) for s in rng.uniform(2.0, 10.0, B)]
            codes = rng.integers(0, cfg.codebook_size, (B, max(lens) + max(DELAY), len(DELAY))).astype(np.int64)
            codes_dev = torch.from_numpy(codes).to(dev)
            fns = {"loop": lambda: _arm_loop(m, codes, lens),
                   "call": lambda: m.decode_dia_output(codes, lens, DELAY, speed=SPEED),
                   "call_dev": lambda: m.decode_dia_output(codes_dev, lens, DELAY, speed=SPEED)}
            arms = {k: [] for k in fns}
            for r in range(rounds + 1):                                 # round 0 warms every arm up and is dropped
                for k, fn in fns.items():
                    fn()
                    dt, _ = _timed(fn)
                    if r:
                        arms[k].append(dt)
            res = {"model": "dac_44khz", "items": B, "frames_min": min(lens), "frames_max": max(lens), "frames_total": sum(lens), "speed": SPEED,
                   **{k: _stats(v) for k, v in arms.items()}}
            res["loop_spread_ms"] = round(res["loop"]["max_ms"] - res["loop"]["min_ms"], 3)
            res["speedup_call"] = round(res["loop"]["median_ms"] / res["call"]["median_ms"], 3)
            res["speedup_call_dev"] = round(res["loop"]["median_ms"] / res["call_dev"]["median_ms"], 3)
            print(json.dumps(res), flush=True)
            out.append(res)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dia_output_bench.json"))
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
