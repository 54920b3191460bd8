#!/usr/bin/env python3
"""Causal Encodec streams at the 24 kHz preset (seeded weights): wall time of one pool step, device tensors in and out, synchronised.

    python tools/encodec_causal_bench.py [--out profiles/encodec_causal_bench.json] [--repeats 3]

Per direction (encode, decode), pool size (1, 16 slots, lock step: one batch) and push size (1, 5, 75 frames): the step's wall time after
2 s and after 20 s of history -- the claim under test is that it does not depend on the history -- as the median over `--steps` steps,
repeated `--repeats` times from a fresh pool (the spread is the min / max of those medians).  Beside it the baseline a caller has
without the pool: the one-clip call on the whole prefix at the same points (B = 1 per stream, so 16 streams are 16 calls).  The baseline
runs in this process on this build, not on the parent commit: the one-clip launch sequences are the parent's, unchanged.  Also the
kernel-class profile of a step (HIP events): the LSTM class is the per-time-step launches; the share of halo recompute is stated from
the frame counts, halo / (n + halo)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encodec_causal_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    import torch
    from neuralcodecs_amd import Encodec, encodec_causal_plan
    from neuralcodecs_amd.encodec import EncodedFrame
    from neuralcodecs_amd.config import EncodecConfig
    from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob, synthetic_pcm
    cfg = EncodecConfig()
    hop = cfg.hop_length
    info = encodec_causal_plan(cfg)[0]
    m = Encodec(cfg)
    m.load_blob(save_blob(encodec_synthetic_state_dict(cfg, seed=24)))
    sec = cfg.sampling_rate // hop                                        # 75 frames
    total = 20 * sec + 75 * (a.steps + 2)
    x = torch.from_numpy(synthetic_pcm(16, 1, total * hop, cfg.sampling_rate, seed=3)).cuda()
    codes = torch.stack([m.encode(x[i:i + 1, :, :])[0].codes[0] for i in range(16)])   # [16, n_q, total]
    sync = torch.cuda.synchronize

    def timed(fn):
        sync(); t0 = time.perf_counter(); fn(); sync()
        return (time.perf_counter() - t0) * 1e3

    def pool_point(decode, slots, n, hist_s):
        pool = m.causal_decode_pool(slots) if decode else m.causal_encode_pool(slots)
        src, unit = (codes, 1) if decode else (x, hop)
        pos = 0
        def push(k):
            nonlocal pos
            ent = {s: (src[s, :, pos * unit:(pos + k) * unit]) for s in range(slots)}
            pool.step(ent)
            pos += k
        while pos < hist_s * sec:
            push(sec)
        push(n)                                                          # warm-up at this shape
        ts = [timed(lambda: push(n)) for _ in range(a.steps)]
        pool.close()
        return statistics.median(ts)

    def baseline_point(decode, slots, frames):
        def run():
            for s in range(slots):
                if decode:
                    m.decode([EncodedFrame(codes[s:s + 1, :, :frames])], frames * hop)
                else:
                    m.encode(x[s:s + 1, :, :frames * hop])
        run()
        return statistics.median([timed(run) for _ in range(3)])

    res = {"config": "Encodec 24 kHz preset, seeded weights, device tensors, wall time incl. synchronisation", "info": info,
           "baseline_note": "one-clip calls measured in the same process on the same build as the pool (their launch sequences are unchanged from the parent commit); not a separate run of the parent commit",
           "points": [], "baseline": []}
    for decode in (False, True):
        for slots in (1, 16):
            for n in (1, 5, 75):
                row = {"direction": "decode" if decode else "encode", "slots": slots, "push_frames": n}
                for hist in (2, 20):
                    meds = [pool_point(decode, slots, n, hist) for _ in range(a.repeats)]
                    row[f"ms_after_{hist}s"] = {"median": statistics.median(meds), "min": min(meds), "max": max(meds)}
                halo = info["halo_d"] if decode else info["halo_e"]
                row["halo_share_of_conv_frames"] = halo / (n + halo)
                res["points"].append(row)
                print(json.dumps(row), flush=True)
            for hist in (2, 20):
                meds = [baseline_point(decode, slots, hist * sec) for _ in range(a.repeats)]
                b = {"direction": "decode" if decode else "encode", "slots": slots, "prefix_s": hist,
                     "one_clip_calls_ms": {"median": statistics.median(meds), "min": min(meds), "max": max(meds)}}
                res["baseline"].append(b)
                print(json.dumps(b), flush=True)
    # kernel-class profile of one-slot steps of 5 frames: the share of the per-time-step LSTM launches
    prof = {}
    for decode in (False, True):
        pool = m.causal_decode_pool(1) if decode else m.causal_encode_pool(1)
        src, unit = (codes, 1) if decode else (x, hop)
        pool.step({0: src[0, :, :sec * unit]})
        m.profile_enable(True)
        m.profile_reset()
        pos = sec
        for _ in range(10):
            pool.step({0: src[0, :, pos * unit:(pos + 5) * unit]})
            pos += 5
        sync()
        p = m.profile_read()
        m.profile_enable(False)
        tot = sum(v["ms"] for v in p.values()) or 1.0
        prof["decode" if decode else "encode"] = {k: {"ms_per_step": v["ms"] / 10, "share": v["ms"] / tot} for k, v in p.items() if v["ms"] > 0}
        pool.close()
    res["profile_push5_1slot"] = prof
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
