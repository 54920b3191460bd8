#!/usr/bin/env python3
"""Encodec stream pool benchmark: n live 48 kHz stereo streams, each pushing one second per step, encode and decode.

    python tools/encodec_stream_bench.py --out profiles/encodec_stream_bench.json

Variants, per direction and n in (1, 8, 32), device-pointer calls on preallocated buffers (synthetic weights, seeded):
  pool      one nc_encodec_stream_pool_step_dev on n entries: the code under test
  solo      (a) the loop of n one-slot pools, one step each: the same launch sequences, one row at a time
  one_clip  (b) the one-clip call per stream and segment: nc_encodec_encode_dev(B = 1, T = 48000) / nc_encodec_decode_dev(B = 1) on the
            frame of a 47520-sample clip (149 code frames; no one-segment clip has a full frame's 150) -- the launch sequences a caller
            without the pool runs per second of every stream, WITHOUT the caller's own ring and overlap-add
One sample = `--steps` consecutive steps from freshly reset slots (one complete segment per stream and step), host clock around work that
ends in a stream synchronise, divided by the number of steps.  Every variant is warmed up, then the variants are timed in turn for
`--reps` rounds, so drift hits all alike.  append_only: a step in which every stream pushes half a second and completes nothing -- the
host cost of a step call that launches the gather kernel and nothing else (slot resets, table upload, one launch), `--append-loops`
such steps per sample.

The two new kernels' own times come from a kernel trace, taken in a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --stats -d DIR -o p -- python tools/encodec_stream_bench.py --trace
    python tools/encodec_stream_bench.py --merge-trace DIR/.../p_results.db --out profiles/encodec_stream_bench.json

--trace runs, per width, `--trace-steps` pool steps of each direction and nothing else: every encode step launches
encodec_stream_gather_kernel once and every decode step overlap_add_stream_kernel once, so dispatch i of a kernel belongs to width
i // trace_steps.  --merge-trace reads the dispatches' durations from the trace's database (the first `--trace-skip` of every width
dropped as warm-up) and adds them to the JSON as `kernels`, with the bytes each launch reads and writes and the rate that follows."""
import argparse
import ctypes as C
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
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encodec_stream_bench.json"))
    ap.add_argument("--widths", default="1,8,32")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--append-loops", type=int, default=200)
    ap.add_argument("--trace", action="store_true", help="only the pool steps, to run under rocprofv3 --kernel-trace")
    ap.add_argument("--trace-steps", type=int, default=8)
    ap.add_argument("--trace-skip", type=int, default=3)
    ap.add_argument("--merge-trace", metavar="DB", help="add the two kernels' times from the database of a --trace run to --out")
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a)
    if a.trace:
        a.steps = a.trace_steps
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this benchmark measures nothing without one")
    cfg = dataclasses.replace(EncodecConfig.encodec_48khz(), bandwidth=12.0)
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    m = Encodec(cfg)
    m.load_blob(save_blob(encodec_synthetic_state_dict(cfg, seed=42)))
    m._bind_torch_stream()
    Cn, seg, stride, S = cfg.channels, m.segment_length, m.segment_stride, a.steps
    nq, F = m.query(seg)[1], m.query(seg)[2][0]
    F1 = m.query(stride)[2][0]
    sync = torch.cuda.synchronize
    ok = _lib.check
    i32 = lambda v: (C.c_int32 * len(v))(*v)  # noqa: E731
    result = {"config": "encodec_48khz stereo 12 kbps", "n_q": nq, "steps_per_sample": S, "reps": a.reps, "unit": "ms per step", "widths": {}}

    def pool_of(decode, n):
        p = C.c_void_p()
        ok(L.nc_encodec_stream_pool_create(m._h, decode, n, 0, C.byref(p)))
        return p

    for n in [int(w) for w in a.widths.split(",")]:
        pcm = torch.from_numpy(synthetic_pcm(n, Cn, S * seg, cfg.sampling_rate, seed=3)).to(dev)
        # encode: the packed push of step t, [n][C, seg]; per stream its own buffer for the baselines
        packed = [pcm[:, :, t * seg:(t + 1) * seg].contiguous() for t in range(S)]
        codes = torch.empty((n * nq * F,), dtype=torch.int64, device=dev)
        scales = torch.empty((n,), dtype=torch.float32, device=dev)
        slots, n_in, one, n_one = i32(list(range(n))), _lib.i64_array([seg] * n), i32([0]), _lib.i64_array([seg])
        big, solo = pool_of(0, n), [pool_of(0, 1) for _ in range(n)]

        def enc_pool():
            for k in range(n):
                ok(L.nc_encodec_stream_pool_reset_slot(big, k))
            for t in range(S):
                ok(L.nc_encodec_stream_pool_step_dev(big, n, slots, n_in, None, None, packed[t].data_ptr(), None, codes.data_ptr(), scales.data_ptr(), None,
                                                     codes.numel(), None, None))

        def enc_solo():
            for k in range(n):
                ok(L.nc_encodec_stream_pool_reset_slot(solo[k], 0))
            for t in range(S):
                for k in range(n):
                    ok(L.nc_encodec_stream_pool_step_dev(solo[k], 1, one, n_one, None, None, packed[t][k].data_ptr(), None, codes.data_ptr() + 8 * k * nq * F,
                                                         scales.data_ptr() + 4 * k, None, nq * F, None, None))

        tail = torch.empty((nq * F + 64,), dtype=torch.int64, device=dev)
        tsc = torch.empty((4,), dtype=torch.float32, device=dev)

        def enc_one_clip():
            for t in range(S):
                for k in range(n):   # T = 48000 is two segments for the one-clip call (the second: the 480-sample overlap); the caller wants the first
                    ok(L.nc_encodec_encode_dev(m._h, packed[t][k].data_ptr(), 1, stride, tail.data_ptr(), tsc.data_ptr(), None))

        half = _lib.i64_array([seg // 2] * n)

        def append_only():
            for _ in range(a.append_loops):
                for k in range(n):
                    ok(L.nc_encodec_stream_pool_reset_slot(big, k))
                ok(L.nc_encodec_stream_pool_step_dev(big, n, slots, half, None, None, packed[0].data_ptr(), None, codes.data_ptr(), scales.data_ptr(), None,
                                                     codes.numel(), None, None))

        if a.trace:   # the pool's steps alone: one gather launch per encode step
            enc_pool(); sync()
            enc, g = None, None
        else:
            enc = _time_variants({"pool": enc_pool, "solo": enc_solo, "one_clip": enc_one_clip}, sync, a.warmup, a.reps)
            g = _time_variants({"append_only": append_only}, sync, a.warmup, a.reps)
        if not a.trace:   # the pool's codes of the last step equal the one-slot pools'
            enc_pool(); sync(); c_pool = codes.clone(); enc_solo(); sync()
            same_enc = bool(torch.equal(c_pool, codes))
        for p in [big] + solo:
            ok(L.nc_encodec_stream_pool_destroy(p))

        # decode: every stream pushes one full frame per step
        fr = torch.randint(0, cfg.codebook_size, (n, nq, F), dtype=torch.int64, device=dev)
        fsc = torch.ones((n,), dtype=torch.float32, device=dev)
        out = torch.empty((n, Cn, stride), dtype=torch.float32, device=dev)
        fr1 = fr[:, :, :F1].contiguous()
        out1 = torch.empty((Cn * m.query(stride)[3] + 64,), dtype=torch.float32, device=dev)
        n_fr, n_fr1 = _lib.i64_array([1] * n), _lib.i64_array([1])
        big, solo = pool_of(1, n), [pool_of(1, 1) for _ in range(n)]

        def dec_pool():
            for k in range(n):
                ok(L.nc_encodec_stream_pool_reset_slot(big, k))
            for t in range(S):
                ok(L.nc_encodec_stream_pool_step_dev(big, n, slots, n_fr, None, None, fr.data_ptr(), fsc.data_ptr(), out.data_ptr(), None, None, out.numel(),
                                                     None, None))

        def dec_solo():
            for k in range(n):
                ok(L.nc_encodec_stream_pool_reset_slot(solo[k], 0))
            for t in range(S):
                for k in range(n):
                    ok(L.nc_encodec_stream_pool_step_dev(solo[k], 1, one, n_fr1, None, None, fr[k].data_ptr(), fsc.data_ptr() + 4 * k, out[k].data_ptr(), None,
                                                         None, Cn * stride, None, None))

        def dec_one_clip():
            for t in range(S):
                for k in range(n):
                    ok(L.nc_encodec_decode_dev(m._h, fr1[k].data_ptr(), fsc.data_ptr() + 4 * k, 1, stride, nq, out1.data_ptr()))

        if a.trace:   # one overlap-add launch per decode step
            dec_pool(); sync()
            for p in [big] + solo:
                ok(L.nc_encodec_stream_pool_destroy(p))
            m.check_errors()
            print("traced", n, "streams:", S, "steps per direction", flush=True)
            continue
        dec = _time_variants({"pool": dec_pool, "solo": dec_solo, "one_clip": dec_one_clip}, sync, a.warmup, a.reps)
        dec_pool(); sync(); o_pool = out.clone(); dec_solo(); sync()
        same_dec = bool(torch.equal(o_pool, out))
        for p in [big] + solo:
            ok(L.nc_encodec_stream_pool_destroy(p))
        m.check_errors()

        def stats(samples, per):
            v = [x / per for x in samples]
            return {"ms": [round(x, 3) for x in v], "median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        result["widths"][str(n)] = {
            "encode": {k: stats(v, S) for k, v in enc.items()}, "decode": {k: stats(v, S) for k, v in dec.items()},
            "append_only": stats(g["append_only"], a.append_loops), "append_only_bytes": 8 * n * Cn * (seg // 2),
            "pool_equals_solo": {"encode": same_enc, "decode": same_dec},
        }
        print(n, json.dumps(result["widths"][str(n)]), flush=True)
    if a.trace:
        return
    result["lstm_stats"] = list(m.lstm_stats())
    if os.path.exists(a.out):   # keep the kernel times of an earlier --merge-trace
        try:
            old = json.load(open(a.out))
            if "kernels" in old:
                result["kernels"] = old["kernels"]
        except ValueError:
            pass
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


def merge_trace(a):
    """the durations of the two kernels' dispatches from a rocprofv3 database (view `kernels`: name, start, end in ns) into the JSON"""
    import sqlite3
    cfg = EncodecConfig.encodec_48khz()
    Cn, seg = cfg.channels, int(cfg.segment_seconds * cfg.sampling_rate)
    stride = max(1, int((1 - cfg.overlap) * seg))
    widths = [int(w) for w in a.widths.split(",")]
    db = sqlite3.connect(a.merge_trace)
    out = {"source": "rocprofv3 --kernel-trace --stats of `--trace` (a run of its own)", "unit": "us per launch", "trace_steps": a.trace_steps,
           "skipped_per_width": a.trace_skip}
    # bytes a launch reads and writes per stream, ov = seg - stride.  gather: a row [C, seg] and the kept overlap [C, ov], each once in and
    # once out (a stream that pushes whole seconds also keeps the ov samples it runs ahead by per step: not counted, a lower bound);
    # overlap-add: [C, stride] samples out and as many read from the new frame, the carried tail [C, ov] read, the new tail read and written
    ov = seg - stride
    per_stream = {"encodec_stream_gather_kernel": 8 * Cn * (seg + ov), "overlap_add_stream_kernel": 4 * Cn * (2 * stride + 3 * ov)}
    for name, bytes_1 in per_stream.items():
        d = [(e - s0) / 1e3 for s0, e in db.execute("select start, end from kernels where name like ? order by start", (f"%{name}%",))]
        if len(d) != len(widths) * a.trace_steps:
            sys.exit(f"{name}: {len(d)} dispatches in the trace, expected {len(widths)} widths x {a.trace_steps} steps")
        out[name] = {}
        for i, n in enumerate(widths):
            v = d[i * a.trace_steps + a.trace_skip:(i + 1) * a.trace_steps]
            med = float(np.median(v))
            out[name][str(n)] = {"us": [round(x, 2) for x in v], "median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                                 "bytes": n * bytes_1, "GB_per_s_at_median": round(n * bytes_1 / med / 1e3, 1)}
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result["kernels"] = out
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
