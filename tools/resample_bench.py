#!/usr/bin/env python3
"""Resampling benchmark: 32 mono rows x 10 s for 48 k -> 44.1 k, 44.1 k -> 48 k, 48 k -> 24 k and 24 k -> 48 k, three ways on the same GPU.

    python tools/resample_bench.py --out profiles/resample_bench.json

  (a) engine  nc_audio_resample_sinc_dev on one packed device tensor (resample_mfma_kernel, or resample_vec_kernel for small U)
  (b) torch   the SAME table applied by torch.nn.functional.conv1d: weight [U, 1, K], stride D, on the edge-padded rows, then transposed
              to time order -- what a caller without the engine would write
  (c) linear  audio.resample_linear (nc_audio_resample_linear_dev): no anti-alias filter, two taps per output
Every pair runs in a child process of its own under a time limit, and the driver stops at the first child that fails.  Arms are timed
between two device events over `iters` calls, alternated round by round; round 0 warms up and is dropped.  Per call the result carries the
arithmetic (2 K4 FLOP per output sample) and the bytes a call must move (input read once + output written once + the table once).
A measurement, not a bar: the comparison side is torch, not an earlier build."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, SECONDS = 32, 10
PAIRS = [(48000, 44100), (44100, 48000), (48000, 24000), (24000, 48000)]
STEP_LIMIT_S = 240


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


def one_pair(src, dst, iters, rounds):
    import torch
    from neuralcodecs_amd import audio, resample_sinc_geom, resample_sinc_len, resample_sinc_packed, resample_sinc_table
    g = resample_sinc_geom(src, dst)
    U, D, W, K, K4 = (g[k] for k in ("U", "D", "W", "K", "K4"))
    n = src * SECONDS
    no = resample_sinc_len(n, src, dst)
    rng = np.random.default_rng(0)
    x = torch.from_numpy((0.1 * rng.standard_normal((ROWS, n))).astype(np.float32)).cuda()
    flat, lens = x.reshape(-1), [n] * ROWS
    out = torch.empty(ROWS * no, dtype=torch.float32, device="cuda")
    weight = torch.from_numpy(np.ascontiguousarray(resample_sinc_table(src, dst)[:, :K])).cuda().reshape(U, 1, K)
    frames = -(-no // U)

    def torch_arm():
        xp = torch.nn.functional.pad(x[:, None], (W, frames * D + W - n), mode="replicate")
        y = torch.nn.functional.conv1d(xp, weight, stride=D)                       # [rows, U, frames]
        return y.transpose(1, 2).reshape(ROWS, -1)[:, :no].contiguous()

    arms = {"nc_audio_resample_sinc_dev": lambda: resample_sinc_packed(flat, src, dst, lens, out=out),
            "torch_conv1d_same_table": torch_arm,
            "nc_audio_resample_linear_dev": lambda: audio.resample_linear(x, src, dst)}
    times = {k: [] for k in arms}
    for r in range(rounds + 1):
        for k, fn in arms.items():
            dt = _timed(torch, fn, iters)
            if r:
                times[k].append(dt)
    got = resample_sinc_packed(flat, src, dst, lens, out=out)[0].reshape(ROWS, no)
    ref = torch_arm()
    twin = resample_sinc_packed(x[0].cpu().numpy()[:D * 64], src, dst, [D * 64], host=True)[0]
    head = resample_sinc_packed(x[0, :D * 64].contiguous(), src, dst, [D * 64])[0].cpu().numpy()
    w = {"src": src, "dst": dst, "U": U, "D": D, "K": K, "K4": K4, "rows": ROWS, "seconds": SECONDS, "n_out": no,
         "table_kb": round(U * K4 * 4 / 1024, 1), "gflop_per_call": round(2.0 * K4 * no * ROWS / 1e9, 3),
         "mbytes_per_call": round((ROWS * (n + no) * 4 + U * K4 * 4) / 1e6, 2), **{k: _med(v) for k, v in times.items()}}
    ms = w["nc_audio_resample_sinc_dev"]["ms_median"]
    w["engine_tflops"] = round(w["gflop_per_call"] / ms, 3)
    w["engine_gbytes_per_s"] = round(w["mbytes_per_call"] / ms, 1)
    w["engine_over_torch"] = round(ms / w["torch_conv1d_same_table"]["ms_median"], 3)
    w["engine_over_linear"] = round(ms / w["nc_audio_resample_linear_dev"]["ms_median"], 3)
    w["max_abs_diff_to_torch"] = float((got - ref).abs().max())
    w["head_equals_host_twin"] = bool(np.array_equal(head.view(np.uint32), twin.view(np.uint32)))
    return w


def main(out, iters, rounds):
    res = {"rows": ROWS, "seconds": SECONDS, "iters": iters, "rounds": rounds, "workloads": []}
    for src, dst in PAIRS:
        cmd = [sys.executable, os.path.abspath(__file__), "--pair", str(src), str(dst), "--iters", str(iters), "--rounds", str(rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{src} -> {dst}: no result within {STEP_LIMIT_S} s; stopping", flush=True)
            sys.exit(2)
        if p.returncode != 0:
            print(f"{src} -> {dst}: the child ended with status {p.returncode}; stopping\n{p.stderr[-2000:]}", flush=True)
            sys.exit(p.returncode if p.returncode > 0 else 1)
        w = json.loads(p.stdout.strip().splitlines()[-1])
        res.setdefault("device", w.pop("device"))
        res["workloads"].append(w)
        print(json.dumps(w), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--pair", type=int, nargs=2, default=None, help="run one src dst pair in this process and print its JSON line")
    a = ap.parse_args()
    if a.pair:
        import torch
        w = one_pair(a.pair[0], a.pair[1], a.iters, a.rounds)
        w["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(w))
    else:
        main(a.out, a.iters, a.rounds)
