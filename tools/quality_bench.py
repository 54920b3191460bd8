#!/usr/bin/env python3
"""Round-trip quality benchmark: the DAC paper's evaluation scales on 32 rows x 1 s at 44.1 kHz, two ways on the same GPU.

    python tools/quality_bench.py --out profiles/quality_bench.json

  (a) torch  the same metrics composed on torch device tensors: L1, SI-SDR, and per scale torch.stft (an FFT) + abs + matmul with the mel
             table + the two L1 terms; one batch of [32, 44100]
  (b) engine quality_metrics on the same device tensors: nc_quality_metrics_dev, a direct windowed DFT on the fp32 matrix cores
Both arms are timed between two device events over `iters` calls, alternated round by round; round 0 warms up and is dropped.
per_scale: the STFT launch of each scale alone (nc_audio_stft_dev on the 64 signal rows of the call, complex output), its time and the
achieved rate 2 x 2 (W/2 + 1) x W x frames x rows FLOP / time, and the mel-spectrogram call (STFT + band chains) of that scale.
A measurement, not a bar: the comparison side is torch, not an earlier build."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralcodecs_amd import QualityConfig, mel_filterbank  # noqa: E402
from neuralcodecs_amd.quality import mel_spectrogram_packed, quality_metrics, stft_packed  # noqa: E402

SR, ROWS, N = 44100, 32, 44100


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


def main(out, iters, rounds):
    import torch
    dev = torch.device("cuda", 0)
    cfg = QualityConfig.dac_eval()
    rng = np.random.default_rng(0)
    ref = torch.from_numpy((0.3 * rng.standard_normal((ROWS, N))).astype(np.float32)).to(dev)
    est = (0.9 * ref + 0.03 * torch.randn_like(ref)).contiguous()
    tables = [(W, W // 4, torch.from_numpy(mel_filterbank(SR, M, W)[0]).to(dev), torch.hann_window(W, device=dev)) for W, M in zip(cfg.windows, cfg.n_mels)]

    def arm_torch():
        res = [(est - ref).abs().mean(dim=1)]
        y, x = ref - ref.mean(dim=1, keepdim=True), est - est.mean(dim=1, keepdim=True)
        scale = ((x * y).sum(1) + 1e-8) / ((y * y).sum(1) + 1e-8)
        t = scale[:, None] * y
        res.append(10 * torch.log10((t * t).sum(1) / (((x - t) ** 2).sum(1) + 1e-8) + 1e-8))
        for W, H, fb, win in tables:
            mels = []
            for s in (est, ref):
                p = torch.nn.functional.pad(s[:, None], (W // 2, W // 2), mode="reflect")[:, 0]
                mels.append(torch.matmul(fb, torch.stft(p, W, H, window=win, center=False, return_complex=True).abs()))
            X, Y = mels
            res.append((X - Y).abs().mean(dim=(1, 2)) + (X.clamp(1e-5).pow(2).log10() - Y.clamp(1e-5).pow(2).log10()).abs().mean(dim=(1, 2)))
        return res

    def arm_engine():
        return quality_metrics(ref, est, sample_rate=SR, scales=cfg)

    arms = {"torch": [], "engine": []}
    for r in range(rounds + 1):
        for k, fn in (("torch", arm_torch), ("engine", arm_engine)):
            dt = _timed(torch, fn, iters)
            if r:
                arms[k].append(dt)
    both = torch.cat([est.reshape(-1), ref.reshape(-1)])
    lens = [N] * (2 * ROWS)
    per_scale = []
    for W, M in zip(cfg.windows, cfg.n_mels):
        H = W // 4
        stft_ms = [_timed(torch, lambda: stft_packed(both, W, H, lengths=lens), iters) for _ in range(rounds + 1)][1:]
        mel_ms = [_timed(torch, lambda: mel_spectrogram_packed(both, SR, W, H, M, lengths=lens), iters) for _ in range(rounds + 1)][1:]
        flop = 2.0 * 2 * (W // 2 + 1) * W * (1 + N // H) * 2 * ROWS
        per_scale.append({"W": W, "H": H, "n_mels": M, "stft": _med(stft_ms), "stft_gflop": round(flop / 1e9, 3),
                          "stft_tflops": round(flop / (float(np.median(stft_ms)) * 1e-3) / 1e12, 3), "mel_spectrogram": _med(mel_ms)})
        print(json.dumps(per_scale[-1]), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "samples": N, "sample_rate": SR, "iters": iters, "rounds": rounds,
           "whole_call": {k: _med(v) for k, v in arms.items()}, "per_scale": per_scale,
           "note": "stft / mel_spectrogram times include the output allocation (torch.zeros) and the table upload of each call"}
    res["speedup_whole_call"] = round(res["whole_call"]["torch"]["ms_median"] / res["whole_call"]["engine"]["ms_median"], 3)
    print(json.dumps(res["whole_call"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_bench.json"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    main(a.out, a.iters, a.rounds)
