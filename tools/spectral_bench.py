#!/usr/bin/env python3
"""Measure the inverse STFT next to torch.istft on the same device and inputs: 32 rows x 1 s at 44.1 kHz at the seven
dac_eval windows with H = W / 4.  Writes profiles/spectral_bench.json.

Per window: the whole nc_audio_istft_dev call (both launches), the same call with one output sample per row (the matrix-core launch with a
gather that has nothing to do), their difference (the gather), the achieved TFLOP/s of direct-DFT arithmetic (2 W (W + 2) flops per
frame) on the matrix-core launch, and torch.istft.  Medians of `--iters` timed calls after `--warmup` untimed ones, HIP events around
each call, the device idle before each."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from neuralcodecs_amd import spectral as S  # noqa: E402
from neuralcodecs_amd.quality import QualityConfig, stft_packed  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_bench.json"))
    a = ap.parse_args()
    n = int(a.seconds * a.rate)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((a.rows, n)).astype(np.float32) * 0.1).cuda()
    res = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "samples": n, "warmup": a.warmup, "iters": a.iters, "windows": []}
    for W in QualityConfig.dac_eval().windows:
        H = W // 4
        lens = [n] * a.rows
        spec, so, shapes = stft_packed(x.reshape(-1), W, H, "hann", lens)
        fr = [f for _, f in shapes]
        out = torch.empty(a.rows * n, dtype=torch.float32, device=x.device)
        oo = [r * n for r in range(a.rows)]
        whole = timed(lambda: S.istft_packed(spec, W, H, "hann", fr, so, lens, oo, out=out), a.warmup, a.iters)
        mfma = timed(lambda: S.istft_packed(spec, W, H, "hann", fr, so, [1] * a.rows, oo, out=out), a.warmup, a.iters)
        X = torch.view_as_complex(spec[:2 * a.rows * (W // 2 + 1) * fr[0]].reshape(a.rows, W // 2 + 1, fr[0], 2))
        win = torch.hann_window(W, device=x.device)
        th = timed(lambda: torch.istft(X, W, H, window=win, center=True, length=n), a.warmup, a.iters)
        flops = 2.0 * W * (W + 2) * sum(fr)
        res["windows"].append({"W": W, "H": H, "frames_per_row": fr[0], "istft_call_ms": whole, "mfma_launch_ms": mfma, "gather_ms": max(whole - mfma, 0.0),
                               "direct_dft_tflops": flops / (mfma * 1e-3) / 1e12, "torch_istft_ms": th, "ratio_to_torch": whole / th})
        print(res["windows"][-1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
