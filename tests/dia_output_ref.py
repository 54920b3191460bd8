"""TEST INFRASTRUCTURE: Dia's output stage restated in plain numpy, written from the index formulas (no torch, no engine).

    revert_delay / mask_invalid   Modules/Dia/AudioUtils.cs:108-176 and Models/Dia.cs:1039-1044
    apply_delay                   Modules/Dia/AudioUtils.cs:19-94
    adjust_speed_len / linspace32 / adjust_speed     Models/Dia.cs:947-966, Utils/TorchUtils.cs:58-82 in explicit np.float32 steps

tests/test_dia_output_cpu.py holds these to a torch-CPU transcription of the reference; the GPU suite holds the kernels to these."""
import numpy as np

F = np.float32


def revert_delay(codes, delay):
    """[B, T, C] -> [B, T - max(delay), C]: out[b, t, c] = in[b, min(t + delay[c], T - 1), c] (the pad mask behind the clamp is dead)."""
    codes = np.asarray(codes, np.int64)
    B, T, C = codes.shape
    maxd = int(max(delay))
    out = np.empty((B, T - maxd, C), np.int64)
    for c in range(C):
        t = np.minimum(np.arange(T - maxd) + int(delay[c]), T - 1)
        out[:, :, c] = codes[:, t, c]
    return out


def mask_invalid(codes, lo=0, hi=1023):
    codes = np.asarray(codes, np.int64)
    return np.where((codes < lo) | (codes > hi), 0, codes)


def apply_delay(codes, delay, bos, pad=0):
    """out[b, t, c] = bos where t - delay[c] < 0, else in[b, t - delay[c], c]; `pad` (for t - delay[c] >= T) can never be written."""
    codes = np.asarray(codes, np.int64)
    B, T, C = codes.shape
    out = np.empty_like(codes)
    for c in range(C):
        t = np.arange(T) - int(delay[c])
        out[:, :, c] = np.where(t < 0, bos, codes[:, np.clip(t, 0, T - 1), c])
    return out


def pack_items(reverted, lengths):
    """the packed ragged layout: item b as [C, F_b] row-major, item after item"""
    return np.concatenate([np.ascontiguousarray(reverted[b, :int(n), :].T).reshape(-1) for b, n in enumerate(lengths)])


def adjust_speed_len(L, speed):
    """`(int)(originalLen / speedFactor)` in binary32 with AdjustSpeed's early returns"""
    speed = F(speed)
    if abs(F(speed - F(1.0))) < F(1e-5):
        return int(L)
    T = int(F(L) / speed)             # truncates toward zero, as the C# cast
    return int(L) if T <= 0 or T == L else T


def fma32(a, b, c):
    """round32(a * b + c) with ONE rounding, for binary32 a, b, c.  The product is exact in binary64; the sum is taken there with its
    rounding error (two-sum), and the error decides the one case double rounding gets wrong: a binary64 sum that sits exactly half way
    between two binary32 neighbours."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(F)
    d = s - r.astype(np.float64)
    nb = np.nextafter(r, np.where(d > 0, F(np.inf), F(-np.inf)).astype(F))
    tie = (d != 0) & (np.abs(d) * 2 == np.abs(nb.astype(np.float64) - r.astype(np.float64)))
    return np.where(tie & (err != 0) & ((err > 0) == (d > 0)), nb, r).astype(F)


def linspace32(L, T):
    """torch.linspace(0, L - 1, T) in binary32: step = (end - start) / (steps - 1); the first half start + i * step, the second
    end - (steps - 1 - i) * step; one step: start.  ATen's CPU kernels are built with contraction wherever the instruction set has a fused
    multiply-add, so each position is one fused operation (fma32), not a rounded product and a rounded sum."""
    if T == 1:
        return np.zeros(1, F)
    start, end = F(0), F(L - 1)
    step = F(F(end - start) / F(T - 1))
    i = np.arange(T, dtype=np.int64)
    first = fma32(step, i.astype(F), start)
    second = fma32(-step, (T - 1 - i).astype(F), end)
    return np.where(i < T // 2, first, second).astype(F)


def interp32(x, fp):
    """TorchUtils.Interp(x, arange(L), fp), linear: y = offset * x + slope, two roundings"""
    fp = np.asarray(fp, F)
    L = fp.shape[0]
    idx = np.clip(np.ceil(x).astype(np.int64) - 1, 0, L - 2)            # searchsorted_left(arange(L), x) - 1, clamped
    offset = (fp[idx + 1] - fp[idx]).astype(F)                           # diff(fp) / diff(xp), diff(xp) = 1
    slope = (fp[idx] - (offset * idx.astype(F)).astype(F)).astype(F)
    return ((offset * x).astype(F) + slope).astype(F)


def adjust_speed(fp, speed):
    fp = np.asarray(fp, F)
    L = fp.shape[0]
    T = adjust_speed_len(L, speed)
    if T == L:
        return fp.copy()
    return interp32(linspace32(L, T), fp)
