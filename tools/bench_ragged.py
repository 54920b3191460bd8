#!/usr/bin/env python3
"""Ragged-batch benchmark: clips of unequal lengths through one ragged call against the loop of one-clip calls.

    python tools/bench_ragged.py --out profiles/ragged_bench.json

Workloads (synthetic weights, seeded): DAC 44.1 kHz with 32 clips and SNAC 44 kHz with 8 clips, lengths drawn uniformly from 1..10 s.
Device-pointer calls on preallocated buffers; one measurement = encode of every clip + decode of every clip's codes, host clock around
work that ends in a stream synchronise.  Variants:
  solo      the loop of B = 1 calls (nc_*_encode_dev; nc_dac_from_codes_dev + nc_dac_decode_dev / nc_snac_decode_dev): the reference
  ragged    one nc_*_encode_ragged_dev + one nc_*_decode*_ragged_dev, for kept widths C x rows per launch batch
  uniform   for scale: one uniform call on B clips of total / B samples (the same audio, no raggedness)
Every variant is warmed up, then the variants are timed in turn, `--reps` rounds, so drift hits all of them alike; the JSON holds every
sample, the median, and min / max.  The ragged outputs are compared bit for bit with the solo outputs at these sizes."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralcodecs_amd import DAC, SNAC, DACConfig, SNACConfig, _lib  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob, snac_synthetic_state_dict, synthetic_pcm  # noqa: E402


def _lengths(n, rate, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(rate, 10 * rate + 1, n)]


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


def bench_dac(B, kept, maxw, warmup, reps, seed):
    import torch
    cfg = DACConfig.dac_44khz()
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    lens = _lengths(B, cfg.sample_rate, seed)
    with DAC(cfg) as m:
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=3)))
        m._bind_torch_stream()
        nq, hop = cfg.n_codebooks, cfg.hop_length
        frames = [m.frames(t) for t in lens]
        pcm = torch.from_numpy(np.concatenate([synthetic_pcm(1, 1, t, cfg.sample_rate, seed=100 + i)[0, 0] for i, t in enumerate(lens)])).to(dev)
        ioff, coff = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum([nq * f for f in frames])])
        codes_solo = torch.zeros(int(coff[-1]), dtype=torch.int64, device=dev)
        codes_rg = torch.zeros_like(codes_solo)
        out_solo = torch.zeros(sum(frames) * hop, dtype=torch.float32, device=dev)
        out_rg = torch.zeros_like(out_solo)
        ooff = np.concatenate([[0], np.cumsum([f * hop for f in frames])])
        z = torch.empty(m.latent_dim * max(frames), dtype=torch.float32, device=dev)
        c_lens, c_frames = _lib.i64_array(lens), _lib.i64_array(frames)
        Tu = int(ioff[-1]) // B
        cu = torch.zeros(B * nq * m.frames(Tu), dtype=torch.int64, device=dev)
        zu = torch.empty(B * m.latent_dim * m.frames(Tu), dtype=torch.float32, device=dev)
        ou = torch.empty(B * m.frames(Tu) * hop, dtype=torch.float32, device=dev)

        def solo():
            for b in range(B):
                _ok(L.nc_dac_encode_dev(m._h, pcm.data_ptr() + 4 * int(ioff[b]), 1, lens[b], 0, 0, codes_solo.data_ptr() + 8 * int(coff[b]), None, None))
            for b in range(B):
                _ok(L.nc_dac_from_codes_dev(m._h, codes_solo.data_ptr() + 8 * int(coff[b]), 1, nq, frames[b], z.data_ptr()))
                _ok(L.nc_dac_decode_dev(m._h, z.data_ptr(), 1, frames[b], out_solo.data_ptr() + 4 * int(ooff[b])))

        def ragged(c, w):
            def run():
                _ok(L.nc_codec_set_ragged_window(m._h, c, w))
                _ok(L.nc_dac_encode_ragged_dev(m._h, pcm.data_ptr(), B, c_lens, 0, 0, codes_rg.data_ptr()))
                _ok(L.nc_dac_decode_codes_ragged_dev(m._h, codes_rg.data_ptr(), B, c_frames, nq, out_rg.data_ptr()))
            return run

        def uniform():
            _ok(L.nc_dac_encode_dev(m._h, pcm.data_ptr(), B, Tu, 0, 0, cu.data_ptr(), None, None))
            _ok(L.nc_dac_from_codes_dev(m._h, cu.data_ptr(), B, nq, m.frames(Tu), zu.data_ptr()))
            _ok(L.nc_dac_decode_dev(m._h, zu.data_ptr(), B, m.frames(Tu), ou.data_ptr()))

        variants = {"solo": solo, "uniform": uniform}
        for c in kept:
            for w in maxw:
                variants[f"ragged_C{c}_W{w}"] = ragged(c, w)
        res = _time_variants(variants, torch.cuda.synchronize, warmup, reps)
        exact = {}
        for c in kept:                                  # faster and different is not faster
            ragged(c, maxw[0])()
            torch.cuda.synchronize()
            exact[f"C{c}"] = bool(torch.equal(codes_rg, codes_solo) and torch.equal(out_rg, out_solo))
        m.check_errors()
        plans = {f"C{c}_W{w}": (m.set_ragged_window(c, w), m.ragged_plan(frames, True))[1] for c in kept for w in maxw}
    return {"codec": "dac_44khz", "clips": B, "lengths": lens, "audio_seconds": round(sum(lens) / cfg.sample_rate, 3), "timings": res,
            "ragged_equals_solo": exact, "decode_plans": plans}


def bench_snac(B, kept, maxw, warmup, reps, seed):
    import torch
    cfg = SNACConfig.snac_44khz()
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    lens = _lengths(B, cfg.sampling_rate, seed)
    with SNAC(cfg) as m:
        m.load_blob(save_blob(snac_synthetic_state_dict(cfg, seed=4)))
        m._bind_torch_stream()
        c_lens = _lib.i64_array(lens)
        fr, per, dl = (C.c_int64 * B)(), (C.c_int64 * B)(), (C.c_int64 * B)()
        _ok(L.nc_snac_ragged_query(m._h, B, c_lens, fr, per, dl))
        frames = list(fr)
        pcm = torch.from_numpy(np.concatenate([synthetic_pcm(1, 1, t, cfg.sampling_rate, seed=200 + i)[0, 0] for i, t in enumerate(lens)])).to(dev)
        ioff, coff, ooff = (np.concatenate([[0], np.cumsum(v)]) for v in (lens, list(per), list(dl)))
        codes_solo = torch.zeros(int(coff[-1]), dtype=torch.int64, device=dev)
        codes_rg = torch.zeros_like(codes_solo)
        out_solo = torch.zeros(int(ooff[-1]), dtype=torch.float32, device=dev)
        out_rg = torch.zeros_like(out_solo)
        Tu = int(ioff[-1]) // B
        _, Fu, wu, Lu = m.query(Tu)
        cu = torch.zeros(B * sum(wu), dtype=torch.int64, device=dev)
        ou = torch.empty(B * Lu, dtype=torch.float32, device=dev)

        def solo():   # noise drawn on the device: clip b from seed 5 + b, as the ragged call draws it
            for b in range(B):
                _ok(L.nc_snac_encode_dev(m._h, pcm.data_ptr() + 4 * int(ioff[b]), 1, lens[b], codes_solo.data_ptr() + 8 * int(coff[b]), None, None))
            for b in range(B):
                _ok(L.nc_snac_decode_dev(m._h, codes_solo.data_ptr() + 8 * int(coff[b]), 1, frames[b], None, 5 + b, out_solo.data_ptr() + 4 * int(ooff[b])))

        def ragged(c, w):
            def run():
                _ok(L.nc_codec_set_ragged_window(m._h, c, w))
                _ok(L.nc_snac_encode_ragged_dev(m._h, pcm.data_ptr(), B, c_lens, codes_rg.data_ptr()))
                _ok(L.nc_snac_decode_ragged_dev(m._h, codes_rg.data_ptr(), B, fr, None, 5, out_rg.data_ptr()))
            return run

        def uniform():
            _ok(L.nc_snac_encode_dev(m._h, pcm.data_ptr(), B, Tu, cu.data_ptr(), None, None))
            _ok(L.nc_snac_decode_dev(m._h, cu.data_ptr(), B, Fu, None, 5, ou.data_ptr()))

        variants = {"solo": solo, "uniform": uniform}
        for c in kept:
            for w in maxw:
                variants[f"ragged_C{c}_W{w}"] = ragged(c, w)
        res = _time_variants(variants, torch.cuda.synchronize, warmup, reps)
        exact = {}
        for c in kept:
            ragged(c, maxw[0])()
            torch.cuda.synchronize()
            exact[f"C{c}"] = bool(torch.equal(codes_rg, codes_solo) and torch.equal(out_rg, out_solo))
        m.check_errors()
        plans = {f"C{c}_W{w}": (m.set_ragged_window(c, w), m.ragged_plan(frames, True))[1] for c in kept for w in maxw}
    return {"codec": "snac_44khz", "clips": B, "lengths": lens, "audio_seconds": round(sum(lens) / cfg.sampling_rate, 3), "timings": res,
            "ragged_equals_solo": exact, "decode_plans": plans}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_bench.json"))
    ap.add_argument("--kept", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--max-windows", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--codecs", nargs="+", default=["dac", "snac"], choices=["dac", "snac"])
    ap.add_argument("--dac-clips", type=int, default=32)
    ap.add_argument("--snac-clips", type=int, default=8)
    a = ap.parse_args()
    if _lib.lib().nc_device_count() <= 0:
        sys.exit("bench_ragged.py needs a GPU: there is no CPU path to time")
    out = {"tool": "tools/bench_ragged.py", "library_sha256": _lib.lib_sha256(), "warmup": a.warmup, "reps": a.reps, "seed": a.seed, "workloads": []}
    if "dac" in a.codecs:
        out["workloads"].append(bench_dac(a.dac_clips, a.kept, a.max_windows, a.warmup, a.reps, a.seed))
    if "snac" in a.codecs:
        out["workloads"].append(bench_snac(a.snac_clips, a.kept, a.max_windows, a.warmup, a.reps, a.seed))
    for w in out["workloads"]:
        t = w["timings"]
        best = min((k for k in t if k.startswith("ragged")), key=lambda k: t[k]["median_ms"])
        w["best_ragged"] = best
        w["solo_spread_ms"] = round(t["solo"]["max_ms"] - t["solo"]["min_ms"], 3)
        w["solo_over_best_ragged"] = round(t["solo"]["median_ms"] / t[best]["median_ms"], 3)
        print(f"{w['codec']}: {w['clips']} clips, {w['audio_seconds']} s of audio; solo {t['solo']['median_ms']} ms "
              f"(spread {w['solo_spread_ms']}), uniform {t['uniform']['median_ms']} ms, best {best} {t[best]['median_ms']} ms; "
              f"bit-exact {w['ragged_equals_solo']}")
        for k, v in t.items():
            print(f"    {k:22s} median {v['median_ms']:9.3f}  min {v['min_ms']:9.3f}  max {v['max_ms']:9.3f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
