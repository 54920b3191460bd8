#!/usr/bin/env python3
"""DAC from_latents against the composition a caller had to build before it existed.

    python tools/probe/from_latents_probe.py --out profiles/from_latents_probe.json

DAC 44.1 kHz (synthetic weights, seeded), Gaussian latents [B, n_q * D, frames], two shapes: B = 32 x 87 frames and B = 1 x 8700 frames.
Variants, each ending in a device synchronise under a host clock:
  composed     n_q calls of the test hook nc_op_vq_argmin on the per-codebook slices (host arrays, cut out and made contiguous BEFORE the
               clock starts; every call uploads its slice and its codebook and downloads the indices), the codes stacked on the host and
               uploaded, then nc_dac_from_codes_dev on the same handle: 2 n_q + 1 launches and a host gather
  host         nc_dac_from_latents: host latents in, z / projected / codes back on the host (the like-for-like of `composed`, which also
               starts on the host; it brings back more: z and the raw rows)
  dev          nc_dac_from_latents_dev on device tensors: n_q + 2 launches, nothing crosses the bus
Every variant is warmed up; then `--reps` rounds time all of them, the order reversed every other round; the JSON keeps every sample,
medians, and min / max as the run-to-run spread.  The outputs of the three variants are compared bit for bit at these sizes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from neuralcodecs_amd import DAC, DACConfig, _lib  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob  # noqa: E402


def _stats(v):
    return {"ms": [round(x, 4) for x in v], "median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def probe(m, sd, cfg, B, T, warmup, reps):
    import torch
    L = _lib.lib()
    nq, D = cfg.n_codebooks, cfg.codebook_dim
    lat = np.random.default_rng(B * 100003 + T).standard_normal((B, nq * D, T)).astype(np.float32)
    slices = [np.ascontiguousarray(lat[:, i * D:(i + 1) * D, :]) for i in range(nq)]
    books = [np.ascontiguousarray(sd[f"quantizer.quantizers.{i}.codebook.weight"], dtype=np.float32) for i in range(nq)]
    idx = [np.empty((B, T), np.int64) for _ in range(nq)]
    st = np.empty((B, D, T), np.float32)
    z_c = torch.empty((B, m.latent_dim, T), dtype=torch.float32, device="cuda")
    x_d = torch.from_numpy(lat).cuda()
    z_d, p_d, c_d = (torch.empty((B, m.latent_dim, T), dtype=torch.float32, device="cuda"), torch.empty((B, nq * D, T), dtype=torch.float32, device="cuda"),
                     torch.empty((B, nq, T), dtype=torch.int64, device="cuda"))
    z_h, p_h, c_h = np.empty((B, m.latent_dim, T), np.float32), np.empty((B, nq * D, T), np.float32), np.empty((B, nq, T), np.int64)
    m._bind_torch_stream()
    keep = {}

    def composed():
        for i in range(nq):
            _lib.check(L.nc_op_vq_argmin(0, slices[i].ctypes.data, B, D, T, books[i].ctypes.data, books[i].shape[0], idx[i].ctypes.data, st.ctypes.data))
        keep["codes"] = torch.from_numpy(np.stack(idx, axis=1)).cuda()
        _lib.check(L.nc_dac_from_codes_dev(m._h, keep["codes"].data_ptr(), B, nq, T, z_c.data_ptr()))

    def host():
        _lib.check(L.nc_dac_from_latents(m._h, lat.ctypes.data, B, nq * D, T, z_h.ctypes.data, p_h.ctypes.data, c_h.ctypes.data))

    def dev():
        _lib.check(L.nc_dac_from_latents_dev(m._h, x_d.data_ptr(), B, nq * D, T, z_d.data_ptr(), p_d.data_ptr(), c_d.data_ptr()))

    variants = {"composed": composed, "host": host, "dev": dev}
    for fn in variants.values():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for r in range(reps):
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for k in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            variants[k]()
            torch.cuda.synchronize()
            samples[k].append((time.perf_counter() - t0) * 1e3)
    m.profile_enable(True)
    m.profile_reset()
    dev()
    torch.cuda.synchronize()
    launches = {k: int(v["launches"]) for k, v in m.profile_read().items() if v["launches"]}
    kernel_ms = {k: round(float(v["ms"]), 4) for k, v in m.profile_read().items() if v["launches"]}
    m.profile_enable(False)
    same = bool(torch.equal(keep["codes"], c_d) and torch.equal(z_c, z_d) and np.array_equal(c_h, c_d.cpu().numpy())
                and np.array_equal(z_h, z_d.cpu().numpy()) and np.array_equal(p_h, p_d.cpu().numpy()))
    return {"B": B, "frames": T, "timings": {k: _stats(v) for k, v in samples.items()}, "dev_launches_by_class": launches,
            "dev_kernel_ms_by_class": kernel_ms, "composed_launches": 2 * nq + 1, "outputs_identical": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    cfg = DACConfig.dac_44khz()
    sd = dac_synthetic_state_dict(cfg, seed=3)
    res = {"codec": "dac_44khz", "lib_sha256": _lib.lib_sha256(), "shapes": []}
    with DAC(cfg) as m:
        m.load_blob(save_blob(sd))
        for B, T in ((32, 87), (1, 8700)):
            res["shapes"].append(probe(m, sd, cfg, B, T, a.warmup, a.reps))
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    for s in res["shapes"]:
        print(json.dumps({"B": s["B"], "frames": s["frames"], "identical": s["outputs_identical"], "launches": s["dev_launches_by_class"],
                          **{k: (v["median_ms"], v["min_ms"], v["max_ms"]) for k, v in s["timings"].items()}}))


if __name__ == "__main__":
    main()
