#!/usr/bin/env python3
"""Loudness benchmark: 32 mono rows x 1 s and x 10 s at 44.1 kHz, two ways on the same GPU.

    python tools/loudness_bench.py --out profiles/loudness_bench.json [--kernel-stats <rocprofv3 kernel_stats.csv or results .db>]
    python tools/loudness_bench.py --out profiles/loudness_bench.json --merge --kernel-stats <...>      # add the statistics later, no device
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/loudness_bench.py --only-engine 20      # the run the csv comes from

  (a) torch  the same quantity composed on torch device tensors the way the reference's device path intends it: two 512-tap conv1d (the
             truncated impulse responses of the two biquads), unfold into 400 ms blocks with 75 % overlap, both gates, the formulas
  (b) engine nc_loudness_dev and nc_loudness_normalize_dev on the same device tensor: the exact recursion, block-parallel on the fp32
             matrix cores (kweight_mfma_kernel), the serial state scan and the finish kernels
Both arms are timed between two device events over `iters` calls, alternated round by round; round 0 warms up and is dropped (>= 20 timed
calls per figure with the defaults).  filter_gemm_tflops: 2 x 80 x 64 FLOP per 64-sample block over the kweight_mfma_kernel time of the
kernel statistics, when they are given; kernel_share: each kernel's part of the summed kernel time of the call.
A measurement, not a bar: the comparison side is torch, not an earlier build."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralcodecs_amd import LoudnessConfig  # noqa: E402
from neuralcodecs_amd import loudness as L  # noqa: E402

SR, ROWS = 44100, 32
KERNELS = ("kweight_mfma_kernel", "kweight_scan_kernel", "kweight_out_kernel", "loud_sub_kernel", "loud_cell_kernel", "loud_block_kernel",
           "loud_finish_kernel", "gain_kernel")


def _timed(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _med(v):
    return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def _fir(b, a, taps=512):
    h, s0, s1 = [], 0.0, 0.0
    for i in range(taps):
        v = 1.0 if i == 0 else 0.0
        o = b[0] * v + s0
        s0, s1 = b[1] * v - a[1] * o + s1, b[2] * v - a[2] * o
        h.append(o)
    return h


def _signal(torch, seconds):
    rng = np.random.default_rng(0)
    return torch.from_numpy((0.1 * rng.standard_normal((ROWS, SR * seconds))).astype(np.float32)).cuda()


def _torch_arm(torch, x):
    b, a = L.kweight_coeffs(SR, "reference")
    firs = [torch.tensor(_fir(b[s], a[s])[::-1], dtype=torch.float32, device=x.device).reshape(1, 1, -1) for s in range(2)]
    N, S = int(np.float32(0.4) * np.float32(SR)), int(np.float32(0.4) * np.float32(SR) * np.float32(0.25))

    def run():
        y = x[:, None]
        for f in firs:
            y = torch.nn.functional.conv1d(torch.nn.functional.pad(y, (511, 0)), f)
        z = y[:, 0].unfold(1, N, S).pow(2).sum(2) / N
        l = -0.691 + 10.0 * torch.log10(z)
        pa = l > -70.0
        za = (z * pa).sum(1) / pa.sum(1).clamp(min=1)
        pr = pa & (l > (-0.691 + 10.0 * torch.log10(za) - 10.0)[:, None])
        zr = (z * pr).sum(1) / pr.sum(1).clamp(min=1)
        return torch.maximum(-0.691 + 10.0 * torch.log10(zr), torch.full_like(zr, -70.0))
    return run


def _kernel_stats(path):
    rows = {}
    if path.endswith(".db"):                      # rocprofv3's default output: a SQLite database with a `kernels` view
        import sqlite3
        for name, total in sqlite3.connect(path).execute("select name, sum(duration) from kernels group by name"):
            for k in KERNELS:
                if k in name:
                    rows[k] = rows.get(k, 0.0) + float(total)
        return rows
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for k in KERNELS:
                if k in name:
                    rows[k] = rows.get(k, 0.0) + float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
    return rows


def _stats_entry(stats, stats_calls, stats_seconds):
    ns = _kernel_stats(stats)
    total = sum(ns.values()) or 1.0
    e = {"calls": stats_calls, "seconds": stats_seconds, "us_per_call": {k: round(v / 1e3 / stats_calls, 2) for k, v in ns.items()},
         "kernel_share": {k: round(v / total, 4) for k, v in ns.items()}}
    if ns.get("kweight_mfma_kernel"):
        flop = 2.0 * 80 * 64 * ROWS * ((SR * stats_seconds + 63) // 64) * stats_calls
        e["filter_gemm_tflops"] = round(flop / (ns["kweight_mfma_kernel"] * 1e-9) / 1e12, 3)
    return e


def merge_stats(out, stats, stats_calls, stats_seconds):
    """add the kernel statistics of a trace to an existing result file (no device needed)"""
    with open(out) as f:
        res = json.load(f)
    res["kernel_stats"] = _stats_entry(stats, stats_calls, stats_seconds)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["kernel_stats"]))


def only_engine(calls, seconds):
    import torch
    x = _signal(torch, seconds).reshape(-1)
    lens = [SR * seconds] * ROWS
    for _ in range(calls):
        L.loudness_packed(x, SR, lens)
    torch.cuda.synchronize()
    print("ran", calls, "calls of nc_loudness_dev on", ROWS, "rows x", seconds, "s")


def main(out, iters, rounds, stats, stats_calls, stats_seconds):
    import torch
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "sample_rate": SR, "iters": iters, "rounds": rounds, "workloads": []}
    for seconds in (1, 10):
        x = _signal(torch, seconds)
        flat, lens = x.reshape(-1), [SR * seconds] * ROWS
        work = flat.clone()
        arms = {"torch_fir512": _torch_arm(torch, x), "nc_loudness_dev": lambda: L.loudness_packed(flat, SR, lens),
                "nc_loudness_normalize_dev": lambda: L.normalize_loudness_packed(work, SR, lens, config=LoudnessConfig("reference", -24.0), in_place=True)}
        times = {k: [] for k in arms}
        for r in range(rounds + 1):
            for k, fn in arms.items():
                dt = _timed(torch, fn, iters)
                if r:
                    times[k].append(dt)
        blocks = ROWS * ((SR * seconds + 63) // 64)
        w = {"seconds": seconds, "filter_gemm_gflop": round(2.0 * 80 * 64 * blocks / 1e9, 4), **{k: _med(v) for k, v in times.items()}}
        w["engine_over_torch"] = round(w["nc_loudness_dev"]["ms_median"] / w["torch_fir512"]["ms_median"], 3)
        twin = L.loudness_packed(flat.cpu().numpy()[:SR * seconds * 2], SR, lens[:2], host=True)["lufs"]
        w["first_rows_equal_host_twin"] = bool(np.array_equal(L.loudness_packed(flat, SR, lens)["lufs"][:2].cpu().numpy(), twin))
        res["workloads"].append(w)
        print(json.dumps(w), flush=True)
    if stats:
        res["kernel_stats"] = _stats_entry(stats, stats_calls, stats_seconds)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.json"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--only-engine", type=int, default=0, help="run this many nc_loudness_dev calls and exit (for a kernel trace)")
    ap.add_argument("--seconds", type=int, default=10, help="row length of the --only-engine / --kernel-stats run")
    ap.add_argument("--kernel-stats", default="", help="kernel_stats.csv or results .db of a rocprofv3 --kernel-trace --stats run of --only-engine")
    ap.add_argument("--merge", action="store_true", help="only add --kernel-stats to the existing --out file")
    ap.add_argument("--kernel-stats-calls", type=int, default=20)
    a = ap.parse_args()
    if a.only_engine:
        only_engine(a.only_engine, a.seconds)
    elif a.merge:
        merge_stats(a.out, a.kernel_stats, a.kernel_stats_calls, a.seconds)
    else:
        main(a.out, a.iters, a.rounds, a.kernel_stats, a.kernel_stats_calls, a.seconds)
