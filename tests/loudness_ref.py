"""The judge of the loudness tests: numpy / Python binary64, not part of the product and sharing nothing with it.  A serial lfilter loop,
the BS.1770 gating with real log10 comparisons (as LoudnessMeter.cs:127-190 writes them) and the normalise formula; the coefficient design
and the block tables of include/nc_mi355x.h "loudness" evaluated here on their own; the fixture signals and the measured twin-vs-binary64
gaps of tests/golden/loudness_bounds.json."""
import json
import math
import os

import numpy as np

import quality_ref as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loudness_bounds.json")
GAIN_FACTOR = math.log(10.0) / 20.0
G = (1.0, 1.0, 1.0, float(np.float32(1.41)), float(np.float32(1.41)))
RATE = 8000                       # the fixtures' sample rate
REF_B = [[1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -2.0, 1.0]]                  # LoudnessMeter.cs:41-52
REF_A = [[1.0, -1.69065929318241, 0.73248077421585], [1.0, -1.99004745483398, 0.99007225036621]]


# ------------------------------------------------------------------------------------------------------------------ coefficients, tables
def coeffs64(rate, filt):
    """(b [2][3], a [2][3]) as Python floats"""
    if filt == "reference":
        f = lambda rows: [[float(np.float32(v)) for v in r] for r in rows]
        return f(REF_B), f(REF_A)
    out_b, out_a = [], []
    for f0, Q, G in ((1681.974450955533, 0.7071752369554196, 3.999843853973347), (38.13547087602444, 0.5003270373238773, None)):
        K = math.tan(math.pi * f0 / rate)
        a0 = 1.0 + K / Q + K * K
        out_a.append([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
        if G is None:
            out_b.append([1.0, -2.0, 1.0])
        else:
            Vh = 10.0 ** (G / 20.0)
            Vb = Vh ** 0.4996667741545416
            out_b.append([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    return out_b, out_a


def state_space(b, a):
    """the cascade of two transposed direct form II biquads as s' = A s + B x, y = C s + D x"""
    (b0, b1, b2), (c0, c1, c2) = b
    (_, a1, a2), (_, d1, d2) = a
    e1, e2 = c1 - d1 * c0, c2 - d2 * c0
    A = [[-a1, 1.0, 0.0, 0.0], [-a2, 0.0, 0.0, 0.0], [e1, 0.0, -d1, 1.0], [e2, 0.0, -d2, 0.0]]
    return A, [b1 - a1 * b0, b2 - a2 * b0, e1 * b0, e2 * b0], [c0, 0.0, 1.0, 0.0], c0 * b0


def _dot(p, q):
    acc = p[0] * q[0]
    for k in range(1, 4):
        acc = acc + p[k] * q[k]
    return acc


def tables64(rate, filt, L=64):
    """Hm, Cm (rounded to binary32), Gs, M in the evaluation order the header states"""
    A, B, Cv, D = state_space(*coeffs64(rate, filt))
    col = lambda m, k: [m[i][k] for i in range(4)]
    AkB = [B]
    for _ in range(1, L):
        AkB.append([_dot(A[i], AkB[-1]) for i in range(4)])
    h = [D] + [_dot(Cv, AkB[k - 1]) for k in range(1, L)]
    Hm = np.zeros((L, L), np.float32)
    for r in range(L):
        for j in range(r + 1):
            Hm[r, j] = np.float32(h[r - j])
    Cm = np.array([[AkB[L - 1 - j][i] for j in range(L)] for i in range(4)], np.float64).astype(np.float32)
    Gs = [Cv]
    for _ in range(1, L):
        Gs.append([_dot(Gs[-1], col(A, i)) for i in range(4)])
    P = [row[:] for row in A]
    for _ in range(1, L):
        P = [[_dot(A[i], col(P, k)) for k in range(4)] for i in range(4)]
    return {"Hm": Hm, "Cm": Cm, "Gs": np.array(Gs, np.float64), "M": np.array(P, np.float64)}


# ------------------------------------------------------------------------------------------------------------------ filter and gating
def lfilter(b, a, x):
    """one biquad, sample by sample, binary64, zero initial state"""
    b0, b1, b2 = (v / a[0] for v in b)
    a1, a2 = a[1] / a[0], a[2] / a[0]
    y = np.empty(len(x), np.float64)
    s0 = s1 = 0.0
    for i, v in enumerate(np.asarray(x, np.float64).tolist()):
        o = b0 * v + s0
        s0 = b1 * v - a1 * o + s1
        s1 = b2 * v - a2 * o
        y[i] = o
    return y


def kweight64(x, rate, filt):
    b, a = coeffs64(rate, filt)
    return lfilter(b[1], a[1], lfilter(b[0], a[0], x))


def geometry(rate):
    block = np.float32(0.4) * np.float32(rate)
    return int(block), int(block * np.float32(0.25))


def gating64(ys, rate):
    """ys: [C][n] filtered channels -> lufs (unclamped below -70 only by the clamp itself), the counts and the block loudness with its
    distances to both thresholds in dB"""
    ys = np.atleast_2d(np.asarray(ys, np.float64))
    C, n = ys.shape
    N, S = geometry(rate)
    J = (n - N) // S + 1 if n >= N else 0
    out = {"n_blocks": J, "n_pass_abs": 0, "n_pass_rel": 0, "lufs": -70.0, "margin_db": math.inf, "block_db": np.zeros(0)}
    if J == 0:
        return out
    z = np.array([[np.sum(ys[c, j * S:j * S + N] ** 2) / N for j in range(J)] for c in range(C)])
    g = np.array(G[:C])[:, None]
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10((g * z).sum(0))
        pa = l > -70.0
        za = (z * pa).sum(1) / max(int(pa.sum()), 1)
        gamma_r = -0.691 + 10.0 * np.log10((g[:, 0] * za).sum()) - 10.0
        pr = pa & (l > gamma_r)
        zr = (z * pr).sum(1) / max(int(pr.sum()), 1)
        W = (g[:, 0] * zr).sum()
        lufs = -0.691 + 10.0 * np.log10(W) if W > 0 else -math.inf
    margins = np.concatenate([np.abs(l - -70.0), np.abs(l - gamma_r) if np.isfinite(gamma_r) else np.full(J, math.inf)])
    out.update(n_pass_abs=int(pa.sum()), n_pass_rel=int(pr.sum()), lufs=max(float(lufs), -70.0), margin_db=float(np.nanmin(margins)), block_db=l)
    return out


def loudness64(clip, rate, filt):
    """clip [n] or [C, n] binary32 -> gating64 of its K-weighted channels"""
    clip = np.atleast_2d(clip)
    return gating64([kweight64(ch, rate, filt) for ch in clip], rate)


def gain64(target_db, lufs):
    return math.exp((target_db - lufs) * GAIN_FACTOR)


# ------------------------------------------------------------------------------------------------------------------ fixtures and bounds
def fixtures(rate=RATE):
    """name -> binary32 mono clip: two plain signals of quality_ref.signal and the three shaped ones"""
    out = {"tones": np.float32(0.5) * Q.signal(12000, rate, 1), "soft": np.float32(0.1) * Q.signal(9001, rate, 2)}
    z = np.float32(0.4) * Q.signal(14000, rate, 3)
    z[4000:9000] = 0.0
    out["zeros"] = z
    q = np.float32(0.4) * Q.signal(14000, rate, 4)
    q[7000:] *= np.float32(10.0 ** (-15.0 / 20.0))
    out["quiet"] = q
    out["dc"] = (np.float32(0.3) * Q.signal(12000, rate, 5) + np.float32(0.2)).astype(np.float32)
    return out


FILTERS = ("reference", "designed")


def measure(twin_kweight, twin_loudness, twin_normalize):
    """the twin against this judge on every fixture and both filters: relative filter gap, |delta LUFS| and the level after normalising
    to -16.  twin_kweight(x, rate, filt) -> y; twin_loudness(x, rate, filt) -> lufs; twin_normalize(x, rate, filt, target) -> levelled x"""
    doc = {"kweight_rel": {}, "lufs_abs": 2.0 ** -19, "normalize_abs": 2.0 ** -19}     # binary32 results near -16 .. -32: never held closer than one ulp32
    for name, x in fixtures().items():
        for filt in FILTERS:
            y64 = kweight64(x, RATE, filt)
            y = np.asarray(twin_kweight(x, RATE, filt), np.float64)
            doc["kweight_rel"][f"{name}/{filt}"] = max(float(np.abs(y - y64).max() / np.abs(y64).max()), 2.0 ** -24)
            want = gating64([y64], RATE)["lufs"]
            doc["lufs_abs"] = max(doc["lufs_abs"], abs(float(twin_loudness(x, RATE, filt)) - want))
            lev = twin_normalize(x, RATE, filt, -16.0)
            doc["normalize_abs"] = max(doc["normalize_abs"], abs(float(twin_loudness(lev, RATE, filt)) - -16.0))
    return doc


def write_bounds(twin_kweight, twin_loudness, twin_normalize):
    """tests/golden/loudness_bounds.json.  Run by hand when the canonical arithmetic changes:
        python -c "import sys; sys.path[:0] = ['tests', '.']; import test_loudness_cpu as t; t.regenerate()" """
    doc = measure(twin_kweight, twin_loudness, twin_normalize)
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc


def bounds():
    with open(GOLDEN) as f:
        return json.load(f)
