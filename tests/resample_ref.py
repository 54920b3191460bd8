"""Binary64 statement of the band-limited resampler, written from include/nc_mi355x.h ("band-limited resampling": ratio, geom, table, pad,
chain, length) in numpy -- the judge of the serial host twin in tests/test_resample_cpu.py.  Plain module, not a conftest."""
import math

import numpy as np

PI = float.fromhex("0x1.921fb54442d18p+1")
PAIRS = [(48000, 44100), (44100, 48000), (48000, 24000), (24000, 48000), (16000, 44100), (44100, 16000)]
GEOM = {(48000, 44100): (147, 160, 28, 216), (44100, 48000): (160, 147, 26, 199), (48000, 24000): (1, 2, 51, 104),
        (24000, 48000): (2, 1, 26, 53), (16000, 44100): (441, 160, 26, 212), (44100, 16000): (160, 441, 70, 581)}   # U, D, W, K


def geom(src, dst, zeros=24, rolloff=None):
    g = math.gcd(src, dst)
    U, D = dst // g, src // g
    base = min(U, D) * (0.945 if rolloff is None else float(np.float32(rolloff)))   # the default is julius' binary64 0.945
    W = math.ceil(zeros * D / base)
    K = 2 * W + D
    return dict(U=U, D=D, W=W, K=K, K4=(K + 3) // 4 * 4, base=base, zeros=zeros)


def n_out(n, src, dst):
    g = math.gcd(src, dst)
    return -(-n * (dst // g) // (src // g))


def table64(src, dst, zeros=24, rolloff=None):
    """h [U, K] in binary64, every row divided by its own sum"""
    q = geom(src, dst, zeros, rolloff)
    i = np.arange(q["U"], dtype=np.float64)[:, None]
    k = np.arange(q["K"], dtype=np.float64)[None, :]
    t = ((-i) / q["U"] + (k - q["W"]) / q["D"]) * q["base"]
    t = np.clip(t, -float(zeros), float(zeros))
    a = PI * t
    c = np.cos(a / (2.0 * zeros))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(a == 0.0, 1.0, np.sin(a) / a) * c * c
    return q, v / v.sum(axis=1, keepdims=True)


def table32(src, dst, zeros=24, rolloff=None):
    """the table as the library exports it: [U, K4] binary32, +0 behind K"""
    q, h = table64(src, dst, zeros, rolloff)
    out = np.zeros((q["U"], q["K4"]), np.float32)
    out[:, :q["K"]] = h.astype(np.float32)
    return q, out


def windows(x, q, frames):
    """xpad[m D + k] for m < frames, k < K: the edge sample repeated"""
    idx = np.arange(frames)[:, None] * q["D"] + np.arange(q["K"])[None, :] - q["W"]
    return np.asarray(x, np.float64)[np.clip(idx, 0, len(x) - 1)]


def resample64(x, src, dst, zeros=24, rolloff=None):
    """(y in binary64 from the unrounded table, sum_k |h_k| |xpad_k| per output sample, geometry)"""
    q, h = table64(src, dst, zeros, rolloff)
    no = n_out(len(x), src, dst)
    if no == 0:
        return np.zeros(0), np.zeros(0), q
    frames = -(-no // q["U"])
    X = windows(x, q, frames)
    return (X @ h.T).reshape(-1)[:no], (np.abs(X) @ np.abs(h).T).reshape(-1)[:no], q


def chain_bound(mag, q):
    """|binary32 fmaf chain of K4 steps on the once-rounded table - binary64| per output: each step rounds once (2^-24 relative to a partial
    sum that sum |h| |x| bounds) and every tap carries its one rounding (2^-24 relative); second-order terms are covered by the + 2"""
    return (q["K4"] + 2) * 2.0 ** -24 * mag


def ulp_distance(a, b):
    """distance in representable binary32 values, elementwise"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def signal(n, seed, amp=0.5):
    """a reproducible test row: noise plus two tones, |x| < amp"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.5 * rng.uniform(-1, 1, n) + 0.3 * np.sin(0.05 * t + seed) + 0.2 * np.sin(1.3 * t)
    return (amp * x).astype(np.float32)


def tone(f, rate, n, amp=0.5, phase=0.3):
    return amp * np.sin(2 * np.pi * f * np.arange(n) / rate + phase)
