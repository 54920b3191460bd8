#!/usr/bin/env python3
"""Dia sampling-stage benchmark: the language model's logits to the next row of the delayed code matrix, two ways on the same GPU.

    python tools/dia_sample_bench.py --out profiles/dia_sample_bench.json

Workload: B in {1, 8, 32}, C = 9, V = 1028, Dia's delay pattern, the reference's sampling defaults (cfg 3.0, temperature 1.2, top_p 0.95,
top_k 45), N(0, 3) logits fixed in device memory with EOS held down, `steps` generation steps per timed window (500), max_tokens above
steps + max(delay) so no item ends inside a window.  Both arms start from the logits in device memory and end with the row written into
generated [B, L, C], timed with a host clock to a device synchronise behind the last step, alternated round by round:
  (a) torch  the reference's step transcribed onto torch device tensors (Dia.cs:538-548, 424-501, 706-755): about twenty small launches
             and the reference's own .item() round trips per step, torch.multinomial for the draw
  (b) step   DiaGeneration.step: torch.rand for the uniform and ONE nc_dia_generate_step_dev launch, no synchronisation inside the window
  (c) step_u the same with the uniform drawn beforehand: the launch alone, as a caller with its own generator runs it
Reported per arm: median, min and max microseconds per step over the rounds.  events_back_to_back: arm (c) between two HIP events
instead of the host clock -- `steps` Python-driven steps, so it is the kernel's time only while the host enqueues faster than the kernel
runs (it does where this figure equals step_u).  The torch arm always writes unmasked; the one-launch arms mask while the reference would.  A measurement, not a bar: the comparison side is torch, not an earlier build."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralcodecs_amd import DiaGeneration  # noqa: E402

DELAY = [0, 8, 9, 10, 11, 12, 13, 14, 15]
EOS, PAD, BOS, V = 1024, 1025, 1026, 1028
CFG, TEMP, TOP_P, TOP_K = 3.0, 1.2, 0.95, 45


def _stats(v, steps):
    us = [x * 1e3 / steps for x in v]
    return {"us_per_step_median": round(float(np.median(us)), 2), "us_per_step_min": round(min(us), 2), "us_per_step_max": round(max(us), 2),
            "rounds": len(v)}


class TorchLoop:
    """the reference's step on torch device tensors, its host round trips included"""

    def __init__(self, B, L, M, prefill, dev):
        import torch
        self.t, self.B, self.M, self.D = torch, B, M, max(DELAY)
        self.generated = torch.full((B, L, len(DELAY)), -1, dtype=torch.int32, device=dev)
        self.generated[:, :prefill.shape[1]] = prefill
        self.delay = torch.tensor(DELAY, dtype=torch.int64, device=dev)
        self.detected = torch.zeros(B, dtype=torch.bool, device=dev)
        self.countdown = torch.full((B,), -1, dtype=torch.int64, device=dev)
        self.finished = torch.full((B,), -1, dtype=torch.int64, device=dev)
        self.dec_step = 0

    def step(self, logits):
        t = self.t
        B, Cn = self.B, len(DELAY)
        s = self.dec_step + 1
        lg = logits.view(B, 2, Cn, -1)
        uncond, cond = lg[:, 0], lg[:, 1]
        g = cond + (CFG * (cond - uncond))
        g[:, :, EOS + 1:].fill_(float("-inf"))
        g[:, 1:, EOS:].fill_(float("-inf"))
        g[:, 0, EOS].mul_(0.8)
        x = g.view(B * Cn, -1).to(t.float32)
        top = t.argmax(x, dim=-1)
        m = t.zeros_like(x, dtype=t.bool)
        m[top.ne(EOS), EOS] = True
        x = x.masked_fill(m, float("-inf")).div(TEMP)
        _, idx = t.topk(x, k=TOP_K, dim=-1)
        m = t.ones_like(x, dtype=t.bool)
        m.scatter_(-1, idx, t.zeros_like(idx, dtype=t.bool))
        x.masked_fill_(m, float("-inf"))
        probs = t.softmax(x, dim=-1)
        sp, si = t.sort(probs, dim=-1, descending=True)
        rm = t.roll(t.cumsum(sp, dim=-1).gt(TOP_P), shifts=1, dims=-1)
        rm[..., 0] = False
        x.masked_fill_(t.zeros_like(rm).scatter_(-1, si, rm), float("-inf"))
        pred = t.multinomial(t.softmax(x, dim=-1), num_samples=1).squeeze_(1).view(B, Cn)
        active = self.countdown.ne(0)
        trigger = t.zeros_like(active)
        if active.any().item():
            is_eos = self.detected[active].logical_not().logical_and(pred[active, 0].eq(EOS))
            trigger[active] = is_eos.logical_or(t.tensor(s >= self.M - self.D, device=is_eos.device))
        self.detected = self.detected.logical_or(trigger)
        start = trigger.logical_and(self.countdown.lt(0))
        if start.any().item():
            self.countdown[start] = self.D
            self.finished[start] = s
        padding = self.countdown.gt(0)
        if padding.any().item():
            pa = pred[padding].clone()
            after = (self.D - self.countdown[padding]).unsqueeze(1)
            pa[after.eq(self.delay.unsqueeze(0))] = EOS
            pa[after.gt(self.delay.unsqueeze(0))] = PAD
            pred[padding] = pa
            self.countdown[padding] -= 1
        self.generated[:, s, :] = pred.to(t.int32)                  # (bosOver: the prefill is one BOS row behind max(delay) steps)
        self.dec_step += 1


def bench(B, steps, rounds):
    import torch
    dev = torch.device("cuda", 0)
    L = M = steps + max(DELAY) + 64
    rng = np.random.default_rng(B)
    lg = (rng.standard_normal((2 * B, len(DELAY), V)) * 3).astype(np.float32)
    lg[:, 0, EOS] = -300.0
    logits = torch.from_numpy(lg).to(dev)
    prefill = torch.full((B, 1, len(DELAY)), BOS, dtype=torch.int32, device=dev)
    uniforms = torch.rand((steps, B, len(DELAY)), dtype=torch.float32, device=dev)

    def arm_torch():
        loop = TorchLoop(B, L, M, prefill, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loop.step(logits)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def arm_step(supplied):
        gen = DiaGeneration(B, DELAY, M, prefill, [1] * B, CFG, TEMP, TOP_P, TOP_K, EOS, PAD, audio_length=L)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            gen.step(logits, uniforms[i] if supplied else None)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        assert gen.active().all() and not gen.bad().any()
        return dt

    def events_back_to_back():
        gen = DiaGeneration(B, DELAY, M, prefill, [1] * B, CFG, TEMP, TOP_P, TOP_K, EOS, PAD, audio_length=L)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(steps):
            gen.step(logits, uniforms[i])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fns = {"torch": arm_torch, "step": lambda: arm_step(False), "step_u": lambda: arm_step(True), "events_back_to_back": events_back_to_back}
    arms = {k: [] for k in fns}
    for r in range(rounds + 1):                                      # round 0 warms every arm up and is dropped
        for k, fn in fns.items():
            dt = fn()
            if r:
                arms[k].append(dt)
    res = {"B": B, "C": len(DELAY), "V": V, "steps": steps, **{k: _stats(v, steps) for k, v in arms.items()}}
    res["speedup_step"] = round(res["torch"]["us_per_step_median"] / res["step"]["us_per_step_median"], 2)
    res["speedup_step_u"] = round(res["torch"]["us_per_step_median"] / res["step_u"]["us_per_step_median"], 2)
    res["logit_bytes_per_step"] = 4 * 2 * B * len(DELAY) * V
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dia_sample_bench.json"))
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "results": [bench(B, a.steps, a.rounds) for B in (1, 8, 32)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
