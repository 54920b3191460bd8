"""Long-clip record (not a gate): one-shot against chunked Encode / Decode on 60 s clips, and one DAC-44.1k clip past the one-shot limit.

    python tools/long_clip_check.py --out profiles/long_clip.json

Every step runs in a child process of its own under a time limit; the first step that fails, faults or times out ends the run (nothing
more is started on the GPU after it) and is recorded as such.  Steps:
  latency   DAC-44.1k B=1, 1 s and 60 s: encode+decode latency (median of 10 after 3 warm-ups) with launch counts
  dac60     DAC-44.1k B=1 60 s: one-shot vs chunked at the built-in chunk size, encode and decode, device-memory high-water marks
  snac60    SNAC-44k  B=1 60 s: the same
  past      one DAC-44.1k clip just past the one-shot limit (length from the inequality (512 + 4) * L + L >= 2^31 the planner uses)
            under NC_CHUNK_AUTO: status, n_chunks, wall time, and the codes of a 2 s window cut from the middle against a one-shot
            encode of that window extended by the halo on both sides
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("latency", 120), ("dac60", 240), ("snac60", 240), ("past", 180))


def _median_ms(fn, sync, n=10, warm=3):
    for _ in range(warm):
        fn()
    sync()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 3)


def _launches(m, fn):
    m.profile_enable(True)
    m.profile_reset()
    fn()
    n = sum(v["launches"] for v in m.profile_read().values())
    m.profile_enable(False)
    return int(n)


def _builtin_chunk(halo, decode):
    h = max(halo["dec_left"], halo["dec_right"]) if decode else max(halo["enc_left"], halo["enc_right"])
    c = max(1024, 16 * h)
    return -(-c // halo["align"]) * halo["align"]


def _codec(kind):
    from neuralcodecs_amd import DAC, SNAC, DACConfig, SNACConfig, dac_halo, snac_halo
    from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob, snac_synthetic_state_dict
    if kind == "dac":
        cfg = DACConfig.dac_44khz()
        m = DAC(cfg)
        m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=3)))
        return cfg, m, dac_halo(cfg), cfg.sample_rate
    cfg = SNACConfig.snac_44khz()
    m = SNAC(cfg)
    m.load_blob(save_blob(snac_synthetic_state_dict(cfg, seed=4)))
    return cfg, m, snac_halo(cfg), cfg.sampling_rate


def step_latency():
    import torch
    from neuralcodecs_amd.weights import synthetic_pcm
    cfg, m, halo, sr = _codec("dac")
    out = {}
    for sec in (1, 60):
        x = torch.from_numpy(synthetic_pcm(1, 1, sec * sr, sr, seed=40 + sec)).cuda()
        z = m.encode(x)[0]
        out[f"{sec}s"] = {"encode_ms": _median_ms(lambda: m.encode(x), torch.cuda.synchronize), "decode_ms": _median_ms(lambda: m.decode(z), torch.cuda.synchronize),
                          "encode_launches": _launches(m, lambda: m.encode(x)), "decode_launches": _launches(m, lambda: m.decode(z))}
    return out


def step_60(kind):
    import numpy as np
    import torch
    from neuralcodecs_amd import _lib
    from neuralcodecs_amd.weights import snac_noise, synthetic_pcm
    out = {}
    for mode in ("chunked", "one_shot"):             # chunked first: its high-water mark is read before the one-shot arena exists
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()                          # HIP's own accounting: the engine allocates with hipMalloc
        cfg, m, halo, sr = _codec(kind)
        x = torch.from_numpy(synthetic_pcm(1, 1, 60 * sr, sr, seed=50)).cuda()
        frames = -(-x.shape[-1] // cfg.hop_length)
        r = {}
        for decode in (False, True):
            chunk = _builtin_chunk(halo, decode)
            m.set_chunk_frames(chunk if mode == "chunked" else _lib.NC_CHUNK_OFF)
            plan = m.chunk_plan(frames, decode, 1)
            if kind == "dac":
                enc = lambda: m.encode(x)
                z = m.encode(x)[0]
                dec = lambda: m.decode(z)
                keep = lambda: [t.cpu().numpy() for t in m.encode(x)[:3]] + [m.decode(z).cpu().numpy()]
            else:
                enc = lambda: m.encode(x, return_latents=True)
                codes = m.encode(x)
                nz = m.flat_noise(snac_noise(cfg, 1, codes[-1].shape[-1] * cfg.vq_strides[-1], seed=51), device=x.device)
                dec = lambda: m.decode(codes, nz)
                keep = lambda: [c.cpu().numpy() for c in m.encode(x)] + [m.decode(codes, nz).cpu().numpy()]
            fn = dec if decode else enc
            key = "decode" if decode else "encode"
            r[key] = {"n_chunks": plan["n_chunks"], "chunk_frames": plan["chunk_frames"], "halo": [plan["halo_left"], plan["halo_right"]],
                      "plan_arena_bytes": plan["arena_bytes"], "ms": _median_ms(fn, torch.cuda.synchronize),
                      "launches": _launches(m, fn)}
            if mode == "chunked":
                r[key]["expected_ratio"] = round((chunk + plan["halo_left"] + plan["halo_right"]) / chunk, 4)
        torch.cuda.synchronize()
        r["device_bytes_high_water"] = int(free0 - torch.cuda.mem_get_info()[0])   # weights + clip + arena + outputs (all grow-only)
        r["_out"] = keep()
        out[mode] = r
        m.dispose()
        del m, x
        torch.cuda.empty_cache()
    a, b = out["chunked"].pop("_out"), out["one_shot"].pop("_out")
    out["bit_identical"] = bool(all(np.array_equal(p, q) for p, q in zip(a, b)))
    for key in ("encode", "decode"):
        out[key + "_measured_ratio"] = round(out["chunked"][key]["ms"] / out["one_shot"][key]["ms"], 4)
    return out


def step_past():
    import numpy as np
    from neuralcodecs_amd import _lib
    cfg, m, halo, sr = _codec("dac")
    hop = cfg.hop_length
    T = (-(-(1 << 31) // 517) // hop + 2) * hop                       # first hop multiples past (512 + 4) * L + L >= 2^31
    rng = np.random.default_rng(60)
    pcm = (0.3 * rng.standard_normal((1, 1, T))).astype(np.float32)
    frames = T // hop
    plan = m.chunk_plan(frames, False, 1)
    t0 = time.perf_counter()
    _, codes, _, _, _ = m.encode(pcm)                                  # host-pointer API under NC_CHUNK_AUTO: upload / download per chunk
    wall = time.perf_counter() - t0
    f0, n = frames // 2, 2 * sr // hop
    lo, hi = f0 - halo["enc_right"], f0 + n + halo["enc_left"]
    m.set_chunk_frames(_lib.NC_CHUNK_OFF)
    _, ref, _, _, _ = m.encode(np.ascontiguousarray(pcm[:, :, lo * hop:hi * hop]))
    same = bool(np.array_equal(codes[:, :, f0:f0 + n], ref[:, :, f0 - lo:f0 - lo + n]))
    return {"samples": int(T), "seconds_of_audio": round(T / sr, 2), "status": "NC_OK", "n_chunks": plan["n_chunks"], "chunk_frames": plan["chunk_frames"],
            "plan_arena_bytes": plan["arena_bytes"], "wall_s": round(wall, 3), "middle_2s_codes_equal_one_shot_window": same}


def child(step):
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")
    r = {"latency": step_latency, "dac60": lambda: step_60("dac"), "snac60": lambda: step_60("snac"), "past": step_past}[step]()
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_clip.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:
        return child(a.step)
    rec = {}
    for step, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            rec[step] = {"failed": f"time limit of {limit} s"}
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            rec[step] = {"failed": f"exit status {p.returncode}", "stderr_tail": p.stderr[-800:]}
            break                                                       # nothing more is started after a failure
        rec[step] = json.loads(line[-1][7:])
        with open(a.out, "w") as f:                                      # partial results survive a later failure
            json.dump(rec, f, indent=1)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return 0 if all("failed" not in v for v in rec.values()) and len(rec) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
