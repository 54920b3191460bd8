#!/usr/bin/env python3
"""Soak of the fence-free hand-offs (runs ON THE GPU BOX; test infrastructure).  VERDICT r4 item 7.

The persistent LSTM's h exchange (csrc/nc_lstm.hip lstm_seq_kernel: write-through payload -> drain -> barrier -> relaxed flag; the
consumer polls the flags and reads the payload with agent-scope loads, NO acquire fence) and the in-launch GroupNorm finish (csrc/nc_gn.h)
are validated empirically: a stale read would be a silently wrong h / mean, not a timeout.  This tool runs `--iters` Encodec 48 kHz stereo
encode + decode steps at the BASELINE C3 shape (16 x 2 s; ~300 LSTM time steps x 4 LSTM sections and ~130 GroupNorm finishes per step) and
compares EVERY iteration's codes, scales and PCM with the first iteration's on the device (bitwise; a running mismatch count read back every
`--check-every` iterations, so the launches stay back to back), then prints one JSON record.  Run it once in the default build and once with
NC_SYNC_ACQUIRE=1 (the textbook acquire form): equal SHA-256 of codes / PCM between the two runs and zero mismatching iterations in both is
the evidence; a single mismatch makes the acquire form the default.

    python tools/soak.py --iters 10000 [--out gpurun_out/soak_default.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--check-every", type=int, default=250)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from neuralcodecs_amd import Encodec
    from neuralcodecs_amd.config import EncodecConfig
    from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob, synthetic_pcm
    cfg = EncodecConfig.encodec_48khz()
    m = Encodec(cfg)
    m.load_blob(save_blob(encodec_synthetic_state_dict(cfg, seed=42)))
    B, T = 16, 2 * cfg.sampling_rate
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(synthetic_pcm(B, cfg.channels, T, cfg.sampling_rate, seed=1234)).to(dev)

    def step():
        fr = m.encode(x)
        return fr, m.decode(fr, T)

    fr0, au0 = step()
    torch.cuda.synchronize()
    m.check_errors()
    ref = [f.codes.clone() for f in fr0] + [f.scale.clone() for f in fr0 if f.scale is not None] + [au0.clone()]
    h = hashlib.sha256()
    for f in fr0:
        h.update(np.ascontiguousarray(f.codes.cpu().numpy()).tobytes())
    codes_sha = h.hexdigest()
    pcm_sha = hashlib.sha256(np.ascontiguousarray(au0.cpu().numpy()).tobytes()).hexdigest()
    bad = torch.zeros((), dtype=torch.int64, device=dev)      # iterations with ANY differing element (device-side; test infrastructure)
    bad_iters, first_bad, t0 = 0, None, time.time()
    for i in range(1, a.iters):
        fr, au = step()
        got = [f.codes for f in fr] + [f.scale for f in fr if f.scale is not None] + [au]
        diff = torch.zeros((), dtype=torch.bool, device=dev)
        for g, r in zip(got, ref):
            diff |= (g != r).any()
        bad += diff.to(torch.int64)
        if i % a.check_every == 0 or i == a.iters - 1:
            n = int(bad.item())                                   # (synchronises)
            m.check_errors()
            if n != bad_iters and first_bad is None:
                first_bad = [i - a.check_every + 1, i]
            bad_iters = n
    dt = time.time() - t0
    sw, tmo = m.lstm_stats()
    rec = {"what": "Encodec 48 kHz stereo 16 x 2 s encode+decode, every iteration's codes / scales / PCM compared bitwise with iteration 0",
           "iterations": a.iters, "mismatching_iterations": bad_iters, "first_mismatch_window": first_bad, "seconds": round(dt, 1),
           "ms_per_iteration_incl_compare": round(dt / max(a.iters - 1, 1) * 1e3, 3), "lstm_stepwise": sw, "lstm_timeouts": tmo,
           "NC_SYNC_ACQUIRE": os.environ.get("NC_SYNC_ACQUIRE", ""), "codes_sha256": codes_sha, "pcm_sha256": pcm_sha,
           "lstm_steps_exchanged": a.iters * 4 * 150 + a.iters * 4 * 4, "library": os.environ.get("NC_MI355X_LIB", "neuralcodecs_amd/libnc_mi355x.so")}
    m.dispose()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rec, open(a.out, "w"), indent=1)
    sys.exit(1 if bad_iters or tmo else 0)


if __name__ == "__main__":
    main()
