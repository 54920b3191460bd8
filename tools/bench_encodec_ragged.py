#!/usr/bin/env python3
"""Encodec ragged-batch benchmark: clips of unequal lengths through one ragged call against the loop of one-clip calls.

    python tools/bench_encodec_ragged.py --out profiles/encodec_ragged_bench.json

Workload (synthetic weights, seeded): Encodec 48 kHz, stereo, 12 kbps, 16 clips with lengths drawn once, uniformly from 0.5..10 s.
Device-pointer calls on preallocated buffers; one measurement = encode of every clip + decode of every clip's frames, host clock around
work that ends in a stream synchronise.  Variants:
  solo      the loop of B = 1 calls (nc_encodec_encode_dev, then nc_encodec_decode_dev): the code path before the ragged calls, the baseline
  uniform   for scale: one uniform call on B clips of total / B samples (the same amount of audio, no raggedness)
  ragged    one nc_encodec_encode_ragged_dev + one nc_encodec_decode_ragged_dev, for every rows-per-batch setting
The ragged outputs are asserted equal, bit for bit, to the solo outputs for every setting BEFORE anything is timed.  Every variant is
warmed up, then the variants are timed in turn, `--reps` rounds, so drift hits all of them alike; the JSON holds every sample, the median
and min / max."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralcodecs_amd import Encodec, EncodecConfig, _lib  # noqa: E402
from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402


def _time_variants(variants, sync, warmup, reps):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
        sync()
    samples = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            samples[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"ms": [round(x, 3) for x in v], "median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3),
                "max_ms": round(max(v), 3)} for k, v in samples.items()}


def _ok(st):
    _lib.check(st)


def bench(B, rows, warmup, reps, seed):
    import torch
    cfg = dataclasses.replace(EncodecConfig.encodec_48khz(), bandwidth=12.0)
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    sr, Cn = cfg.sampling_rate, cfg.channels
    lens = [int(v) for v in np.random.default_rng(seed).integers(sr // 2, 10 * sr + 1, B)]
    with Encodec(cfg) as m:
        m.load_blob(save_blob(encodec_synthetic_state_dict(cfg, seed=42)))
        m._bind_torch_stream()
        nq = m.query(1)[1]
        nfs, frs, dls = m.ragged_query(lens)
        pcm = torch.from_numpy(np.concatenate([synthetic_pcm(1, Cn, t, sr, seed=300 + i)[0].reshape(-1) for i, t in enumerate(lens)])).to(dev)
        ioff, coff, soff, ooff = (np.concatenate([[0], np.cumsum(v)]) for v in ([Cn * t for t in lens], [nq * f for f in frs], nfs, [Cn * d for d in dls]))
        codes_solo = torch.zeros(int(coff[-1]), dtype=torch.int64, device=dev)
        scales_solo = torch.zeros(int(soff[-1]), dtype=torch.float32, device=dev)
        out_solo = torch.zeros(int(ooff[-1]), dtype=torch.float32, device=dev)
        codes_rg, scales_rg, out_rg = torch.zeros_like(codes_solo), torch.zeros_like(scales_solo), torch.zeros_like(out_solo)
        c_lens = _lib.i64_array(lens)
        Tu = sum(lens) // B
        nfu, _, lu, du = m.query(Tu)
        cu = torch.zeros(B * nq * sum(lu), dtype=torch.int64, device=dev)
        su = torch.zeros(B * nfu, dtype=torch.float32, device=dev)
        ou = torch.empty(B * Cn * du, dtype=torch.float32, device=dev)

        def solo():
            for b in range(B):
                _ok(L.nc_encodec_encode_dev(m._h, pcm.data_ptr() + 4 * int(ioff[b]), 1, lens[b], codes_solo.data_ptr() + 8 * int(coff[b]),
                                            scales_solo.data_ptr() + 4 * int(soff[b]), None))
            for b in range(B):
                _ok(L.nc_encodec_decode_dev(m._h, codes_solo.data_ptr() + 8 * int(coff[b]), scales_solo.data_ptr() + 4 * int(soff[b]), 1, lens[b], nq,
                                            out_solo.data_ptr() + 4 * int(ooff[b])))

        def ragged(r):
            def run():
                _ok(L.nc_encodec_set_ragged_rows(m._h, r))
                _ok(L.nc_encodec_encode_ragged_dev(m._h, pcm.data_ptr(), B, c_lens, codes_rg.data_ptr(), scales_rg.data_ptr(), None))
                _ok(L.nc_encodec_decode_ragged_dev(m._h, codes_rg.data_ptr(), scales_rg.data_ptr(), B, c_lens, nq, out_rg.data_ptr()))
            return run

        def uniform():
            _ok(L.nc_encodec_encode_dev(m._h, pcm.data_ptr(), B, Tu, cu.data_ptr(), su.data_ptr(), None))
            _ok(L.nc_encodec_decode_dev(m._h, cu.data_ptr(), su.data_ptr(), B, Tu, nq, ou.data_ptr()))

        solo()
        torch.cuda.synchronize()
        plans = {}
        for r in rows:                                  # faster and different is not faster: equal before anything is timed
            codes_rg.zero_(); scales_rg.zero_(); out_rg.zero_()
            ragged(r)()
            torch.cuda.synchronize()
            assert torch.equal(codes_rg, codes_solo) and torch.equal(scales_rg, scales_solo), f"max_rows {r}: codes / scales differ from the one-clip calls"
            assert torch.equal(out_rg, out_solo), f"max_rows {r}: decoded PCM differs from the one-clip calls"
            plans[f"R{r}"] = {"encode": m.ragged_rows(lens, False)[0], "decode": m.ragged_rows(lens, True)[0]}
        m.check_errors()
        variants = {"solo": solo, "uniform": uniform}
        for r in rows:
            variants[f"ragged_R{r}"] = ragged(r)
        res = _time_variants(variants, torch.cuda.synchronize, warmup, reps)
        m.check_errors()
        stepwise, timeouts = m.lstm_stats()
    return {"codec": "encodec_48khz", "channels": Cn, "bandwidth_kbps": 12.0, "clips": B, "lengths": lens, "audio_seconds": round(sum(lens) / sr, 3),
            "segments": int(sum(nfs)), "timings": res, "ragged_equals_solo": True, "plans": plans, "lstm_stepwise": stepwise, "lstm_timeouts": timeouts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encodec_ragged_bench.json"))
    ap.add_argument("--max-rows", type=int, nargs="+", default=[8, 16, 32, 64, 128])
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    if _lib.lib().nc_device_count() <= 0:
        sys.exit("bench_encodec_ragged.py needs a GPU: there is no CPU path to time")
    w = bench(a.clips, a.max_rows, a.warmup, a.reps, a.seed)
    t = w["timings"]
    best = min((k for k in t if k.startswith("ragged")), key=lambda k: t[k]["median_ms"])
    w["best_ragged"] = best
    w["solo_spread_ms"] = round(t["solo"]["max_ms"] - t["solo"]["min_ms"], 3)
    w["best_ragged_spread_ms"] = round(t[best]["max_ms"] - t[best]["min_ms"], 3)
    w["solo_over_best_ragged"] = round(t["solo"]["median_ms"] / t[best]["median_ms"], 3)
    out = {"tool": "tools/bench_encodec_ragged.py", "library_sha256": _lib.lib_sha256(), "warmup": a.warmup, "reps": a.reps, "seed": a.seed, "workloads": [w]}
    print(f"{w['codec']}: {w['clips']} clips, {w['audio_seconds']} s of audio in {w['segments']} segments; solo {t['solo']['median_ms']} ms "
          f"(spread {w['solo_spread_ms']}), uniform {t['uniform']['median_ms']} ms, best {best} {t[best]['median_ms']} ms")
    for k, v in t.items():
        print(f"    {k:14s} median {v['median_ms']:9.3f}  min {v['min_ms']:9.3f}  max {v['max_ms']:9.3f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
