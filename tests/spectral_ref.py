"""A plain float64 restatement of the inverse STFT, the spectral masks and the MFCC (include/nc_mi355x.h "inverse STFT, spectral masks, MFCC"):
numpy.fft.irfft per frame, times the window, overlap-add, the envelope division and the length rule -- the recipe of torch.istft with
center = True, which tests/test_spectral_cpu.py holds to torch.istft on complex128.  Also the derived error bounds of the binary32 chains
and the deterministic test inputs the CPU and GPU suites share."""
import numpy as np

U = 2.0 ** -24   # the unit roundoff of binary32


def gamma(m):
    return m * U / (1.0 - m * U)


def signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.4 * np.sin(2 * np.pi * 440.0 * t + seed) + 0.2 * rng.standard_normal(n)).astype(np.float32)


def spectrum(W, F, seed):
    """float32 (re, im) pairs [W/2+1, F, 2], every part set (the imaginary parts of bins 0 and W/2 included)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((W // 2 + 1, F, 2)).astype(np.float32)


def window64(W, window):
    return np.ones(W) if window == "ones" else 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)


def default_len(F, H):
    return H * (F - 1)


def overlap_add(frames, W, H):
    """frames [F, W] -> [W + H (F - 1)]"""
    F = frames.shape[0]
    y = np.zeros(W + H * (F - 1))
    for t in range(F):
        y[t * H:t * H + W] += frames[t]
    return y


def envelope64(W, H, F, window):
    w = window64(W, window)
    return overlap_add(np.tile(w * w, (F, 1)), W, H)


def istft64(X, W, H, window="hann", length=None):
    """X complex [W/2+1, F] -> float64 [length]; samples past the covered span are 0"""
    X = np.asarray(X, np.complex128)
    F = X.shape[1]
    L = default_len(F, H) if not length else int(length)
    w = window64(W, window)
    frames = np.fft.irfft(X.T, n=W, axis=1) * w[None, :]
    y, env = overlap_add(frames, W, H), envelope64(W, H, F, window)
    span = W + H * (F - 1)
    out = np.zeros(L)
    n = max(0, min(L, span - W // 2))
    out[:n] = y[W // 2:W // 2 + n] / env[W // 2:W // 2 + n]
    return out


def idft_basis64(W, window):
    """T [W, W + 2] in float64 as the header defines it"""
    w = window64(W, window)
    n, k = np.arange(W)[:, None], np.arange(W // 2 + 1)[None, :]
    c = np.where((k == 0) | (k == W // 2), 1.0, 2.0)
    ang = 2.0 * np.pi * ((k * n) % W) / W
    T = np.zeros((W, W + 2))
    T[:, 0::2] = w[:, None] * c * np.cos(ang) / W
    T[:, 1::2] = -w[:, None] * c * np.sin(ang) / W
    T[:, 1] = 0.0
    T[:, W + 1] = 0.0
    return T


def flat(X32):
    """(re, im) pairs [K, F, 2] -> Xflat [2 K, F] float64"""
    K, F, _ = X32.shape
    return np.asarray(X32, np.float64).transpose(0, 2, 1).reshape(2 * K, F)


def istft_bound(X32, W, H, window, length, x_true, e_X=None):
    """The derived bound on |twin - exact| per output sample, u = 2^-24, gamma_m = m u / (1 - m u):
      frame   the chain of J = W + 2 fmaf on table entries rounded once from binary64: |y^ - y*| <= gamma_(J+1) S, S = sum_j |T||X|
              ((1 + u)(1 + gamma_J) - 1 <= gamma_(J+1))
      sum     m = ceil(W / H) covering frames at most, m additions from +0: |num - num*| <= (gamma_(J+1) (1 + gamma_m) + gamma_m) sum_t S
      env     w32 = w (1 + d), |d| <= u, squared: 2 u + u^2; the binary64 sum adds nothing visible; one rounding: env32 = env* (1 + e), |e| <= 4 u
      divide  out = fl(num / env32): |out - x*| <= ((E_num / env* + 4 u |x*|) / (1 - 4 u)) (1 + u) + u |x*|
    plus 64 eps64 sum S / env* for the float64 restatement itself.  e_X (optional, [2 K, F]): a bound on the error of X itself, carried
    through the exact inverse: sum_t (|T| e_X) / env*."""
    F = X32.shape[1]
    J, m = W + 2, -(-W // H)
    T = np.abs(idft_basis64(W, window))
    S = overlap_add((T @ np.abs(flat(X32))).T, W, H)
    env = envelope64(W, H, F, window)
    span = W + H * (F - 1)
    L = len(x_true)
    n = max(0, min(L, span - W // 2))
    sl = slice(W // 2, W // 2 + n)
    e_num = (gamma(J + 1) * (1 + gamma(m)) + gamma(m)) * S[sl]
    ax = np.abs(x_true[:n])
    b = ((e_num / env[sl] + 4 * U * ax) / (1 - 4 * U)) * (1 + U) + U * ax + 64 * np.finfo(np.float64).eps * S[sl] / env[sl]
    if e_X is not None:
        b = b + overlap_add((T @ e_X).T, W, H)[sl] / env[sl]
    out = np.zeros(L)
    out[:n] = b
    return out


def stft_error_bound(x32, W, H, window):
    """|X^ - X*| per part [2 K, F] of the forward transform (header, "round-trip quality"): a chain of W fmaf on table entries rounded once:
    gamma_(W+1) sum_n |basis||x_pad|"""
    x = np.asarray(x32, np.float64)
    n = len(x)
    F = 1 + n // H
    xp = np.pad(x, W // 2, mode="reflect")
    w = window64(W, window)
    idx = np.arange(F)[:, None] * H + np.arange(W)[None, :]
    fr = np.abs(xp[idx]) * w[None, :]            # [F, W]
    k, nn = np.arange(W // 2 + 1)[:, None], np.arange(W)[None, :]
    ang = 2.0 * np.pi * ((k * nn) % W) / W
    E = np.zeros((W + 2, F))
    E[0::2] = np.abs(np.cos(ang)) @ fr.T
    E[1::2] = np.abs(np.sin(ang)) @ fr.T
    return gamma(W + 1) * E


def dct64(n_mfcc, n_mels):
    c, m = np.arange(n_mfcc)[:, None], np.arange(n_mels)[None, :]
    d = np.cos(np.pi * c * (2 * m + 1) / (2.0 * n_mels)) * np.sqrt(2.0 / n_mels)
    d[0] *= 1.0 / np.sqrt(2.0)
    return d


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def ragged_spectra(W, frames, seed):
    """(packed float32 buffer of (re, im) pairs, COMPLEX element offsets): rows at ODD complex offsets with NaN-filled gaps"""
    K = W // 2 + 1
    offs, o = [], 1
    for f in frames:
        offs.append(o)
        o += K * f + (2 if (o + K * f) % 2 else 3)
    buf = np.full(2 * o, np.nan, np.float32)
    for i, (at, f) in enumerate(zip(offs, frames)):
        buf[2 * at:2 * (at + K * f)] = spectrum(W, f, seed + i).reshape(-1)
    return buf, offs


def out_canvas(lens):
    """(NaN canvas, offsets): rows at multiples of four elements and at odd offsets in turn, a NaN gap behind each"""
    oo, o = [], 1
    for i, n in enumerate(lens):
        o += (-o) % 4 if i % 2 else (0 if o % 2 else 1)
        oo.append(o)
        o += n + 3
    return np.full(o + 4, np.nan, np.float32), oo
