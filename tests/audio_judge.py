"""Shared by the audio pre/post and bit-packing op tests (plain module, not a conftest): inputs, truths written independently of the
kernels, the exact judge of the linear resampler with its derived bound, the contraction sentinels, the Python-integer BitPacker, and
the canary-filled device buffers the GPU tests run the `_dev` entry points on.

Nothing here imports the engine; torch is imported only by Canvas, which only the GPU tests construct.
"""
import functools
import json
import os

import numpy as np

from oracle import audio_ref as R

BLOCK = 256                                       # threads per block of every element-wise kernel in nc_audio.hip / nc_pack.hip
LENGTHS = (1, 255, 256, 257, 3001)                # one element, either side of one block, a dozen blocks with a partial last one
F32_CANARY, I16_CANARY, U8_CANARY, I64_CANARY = 0x7FC00000, 0x5A5A, 0xA5, 0x5A5A5A5A5A5A5A5A
_UINT = {np.dtype(np.float32): (np.uint32, F32_CANARY), np.dtype(np.int16): (np.uint16, I16_CANARY),
         np.dtype(np.uint8): (np.uint8, U8_CANARY), np.dtype(np.int64): (np.uint64, I64_CANARY)}


TABLE = []


def report(kernel, **kw):
    TABLE.append(dict(kernel=kernel, **kw))
    print("\nOPREPORT " + json.dumps(TABLE[-1], sort_keys=True))


def write_table():
    path = os.environ.get("NC_AUDIO_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(what="cases and compared values per test of tests/test_audio_gpu.py and tests/test_containers_gpu.py on an MI355X; "
                                "the resampler rows hold the largest error / allowed against the exact interpolant.  A record: no test reads it.",
                           rows=TABLE), f, indent=1, sort_keys=True)
            f.write("\n")


def bits_of(a):
    """The array's bit patterns: -0.0 and NaN payloads count in a comparison of these."""
    a = np.ascontiguousarray(a)
    return a.view(_UINT[a.dtype][0])


def f32_from_bits(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def same_bits(got, want, what, created_nan=False):
    """Equal bit for bit.  created_nan: where the arithmetic itself makes a NaN (0 * inf, inf - inf) x86 and the GPU return different
    default NaNs, so NaN is required at the same positions and equal bits everywhere else."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits_of(got), bits_of(want)
    if created_nan:
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN at other positions"
        keep = ~np.isnan(want)
        g, w = g[keep], w[keep]
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} differ, first at {int(bad[0])}: got {int(g[bad[0]]):#x}, want {int(w[bad[0]]):#x}"
    return int(got.size)


class Canvas:
    """n elements inside a larger device buffer that is pre-filled with a canary (NaN for float, 0x5A5A for int16, 0xA5 for bytes).
    An input's neighbours would show in the output if a kernel read them; an output's neighbours must be untouched after the call.
    skew moves the payload by that many elements: a byte payload then starts skew bytes behind a 16-byte boundary."""
    PAD = 64

    def __init__(self, dtype, n, data=None, skew=0):
        import torch
        self.dtype, self.n, self.lo = np.dtype(dtype), int(n), self.PAD + skew
        utype, canary = _UINT[self.dtype]
        host = np.empty(self.lo + self.n + self.PAD, self.dtype)
        host.view(utype)[:] = canary
        if data is not None:
            host[self.lo:self.lo + self.n] = np.ascontiguousarray(data, self.dtype).reshape(-1)
        self.before = host.copy()
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lo * self.dtype.itemsize

    def read(self, what="output"):
        """The payload, after asserting that nothing outside it changed."""
        import torch
        torch.cuda.synchronize()
        host = self.t.cpu().numpy()
        b, a = bits_of(self.before), bits_of(host)
        assert np.array_equal(a[:self.lo], b[:self.lo]) and np.array_equal(a[self.lo + self.n:], b[self.lo + self.n:]), \
            f"{what}: the call wrote outside its output"
        return host[self.lo:self.lo + self.n].copy()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return np.array_equal(bits_of(self.t.cpu().numpy()), bits_of(self.before))


# ------------------------------------------------------------------------------------------------------------------ float -> pcm16
QUIET_NANS = (0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFD54321)            # both signs, two with a payload


@functools.lru_cache(maxsize=None)
def pcm16_inputs():
    """For every k in [-32767, 32767] the binary32 nearest k / 32767 and its two neighbours (every truncation boundary from both sides),
    +-0, the smallest subnormal and normal, +-1 with their neighbours, +-FLT_MAX, +-inf, and quiet NaNs of both signs."""
    f, inf = np.float32, np.float32(np.inf)
    c = (np.arange(-32767, 32768, dtype=np.float64) / 32767.0).astype(np.float32)
    tiny, small, big, one = f(2.0 ** -149), np.finfo(np.float32).tiny, np.finfo(np.float32).max, f(1.0)
    edges = np.array([0.0, -0.0, tiny, -tiny, small, -small, one, np.nextafter(one, f(0)), np.nextafter(one, f(2)), -one,
                      -np.nextafter(one, f(0)), -np.nextafter(one, f(2)), big, -big, inf, -inf], np.float32)
    x = np.concatenate([np.nextafter(c, -inf), c, np.nextafter(c, inf), edges, f32_from_bits(QUIET_NANS)]).astype(np.float32)
    x.setflags(write=False)
    return x


def pcm16_truth(x):
    """The kernel's one rounding, restated: c = clamp(x, -1, 1) (NaN -> 0), the product c * 32767 in binary64 is exact (24 x 15 bits),
    one rounding to binary32, truncation toward zero.  Not the oracle's statements: tests/test_audio_cpu.py shows the two agree."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    c = np.where(np.isnan(x64), 0.0, np.clip(x64, -1.0, 1.0))
    return np.trunc((c * 32767.0).astype(np.float32)).astype(np.int16)


# ------------------------------------------------------------------------------------------------------------------ linear resampler
RATES = ((1, 1), (2, 1), (1, 2), (3, 4), (4, 3), (44100, 48000), (48000, 44100), (8000, 48000), (48000, 8000), (1, 100), (100, 1))
N_IN = (1, 2, 3, 257, 3001)
ROWS = (1, 3)
RESAMPLE_CASES = tuple((s, d, n, B) for (s, d) in RATES for n in N_IN for B in ROWS if R.resample_len(n, s, d) > 0)
RESAMPLE_EMPTY = tuple((s, d, n) for (s, d) in RATES for n in N_IN if R.resample_len(n, s, d) == 0)   # these belong with the refusals


def resample_id(case):
    return "%dto%d-n%d-B%d" % tuple(case)


@functools.lru_cache(maxsize=None)
def resample_case(src, dst, n_in, B):
    """(x [B, n_in] binary32 with a full mantissa, the oracle's rows), computed once per process: read-only."""
    x = (np.random.default_rng([src, dst, n_in, B]).standard_normal((B, n_in)) * 0.7).astype(np.float32)
    y = np.stack([R.resample_linear(x[b], src, dst) for b in range(B)])
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


_POW2 = np.array([1 << k for k in range(256)], dtype=object)


def _scaled_int(a):
    """Finite binary32 values times 2^149 as Python integers, exactly (an object array)."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.int64)
    e, m = (b >> 23) & 0xFF, b & 0x7FFFFF
    assert not (e == 255).any(), "finite values only"
    v = np.where(e == 0, m, m | 0x800000).astype(object) * _POW2[np.where(e == 0, 0, e - 1)]
    return np.where((b >> 31) != 0, -v, v)


def resample_judge(y, x, src, dst, what):
    """One row y of the resampler against the exact rational interpolant, in integers; returns the largest error / allowed.

    Exact: p = o * src / dst, i = floor(p), r = o * src mod dst, value x[i] + (r / dst) (x[i+1] - x[i]), and x[n-1] once i >= n - 1.

    Allowed: |y - exact| <= 2^-24 |exact| + S p 2^-51 + 2^-50 max|x| + 2^-149, with S = max |x[i+1] - x[i]|, because
      * the code computes ratio = fl(dst / src) and position = fl(o / ratio): two binary64 roundings, each at most 2^-53 relative, so
        |position - p| <= p 2^-51 with room to spare;
      * the piecewise-linear interpolant (held at x[n-1] behind the last sample) is Lipschitz with constant S, so evaluating it at
        `position` instead of p moves the value by at most S p 2^-51 -- including where `position` falls on the other side of an
        integer than p, or into the `index >= n - 1` branch one output early;
      * fraction = position - index is exact; (1 - fraction), the two products and the sum are binary64 operations on magnitudes of at
        most max|x|, each at most 2^-53 relative: together below 2^-50 max|x|;
      * the one rounding to binary32 is at most 2^-24 relative (what it adds through the terms above is far inside the room the third
        term leaves), or half of 2^-149 in the subnormal range.
    Everything is scaled by dst * 2^149 * 2^51 and compared as Python integers, so the judgement itself does not round."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    n_in, n_out = len(x), len(y)
    assert n_out == int(n_in * (dst / src)) and np.isfinite(y).all(), what
    num = np.arange(n_out, dtype=np.int64) * src                                    # p * dst
    idx, rem = num // dst, num % dst
    held = idx >= n_in - 1
    i0, i1 = np.minimum(idx, n_in - 1), np.minimum(idx + 1, n_in - 1)
    rem = np.where(held, 0, rem).astype(object)
    X, Y = _scaled_int(x), _scaled_int(y)
    exact = X[i0] * (dst - rem) + X[i1] * rem                                       # exact * dst * 2^149
    err = np.abs(Y * dst - exact) * (1 << 51)
    S = max((abs(int(d)) for d in X[1:] - X[:-1]), default=0)
    M = max(abs(int(v)) for v in X)
    allowed = np.abs(exact) * (1 << 27) + S * num.astype(object) + 2 * M * dst + (dst << 51)
    over = np.nonzero(err > allowed)[0]
    assert over.size == 0, f"{what}: {over.size} outputs outside the bound, first o={int(over[0])}: {float(y[over[0]])!r}"
    return max(float(e / a) for e, a in zip(err, allowed))


def branch_edge(src, dst, n_in):
    """The first output whose exact position has floor(p) >= n_in - 1 (None if no output gets there)."""
    o = -(-(n_in - 1) * dst // src)
    return o if o < R.resample_len(n_in, src, dst) else None


def blend_forms(src, dst, o, x0, x1):
    """The binary32 result of output o between binary32 samples x0, x1 as (unfused, first product fused, second product fused), and the
    index: the kernel's statements with every rounding done by hand on fractions.  `a * b + c * d` contracts to fma(a, b, c * d) or to
    fma(c, d, a * b); which one is the compiler's choice, so a sentinel has to tell the unfused form from both."""
    from fractions import Fraction as Q
    ratio = float(dst) / float(src)
    position = o / ratio
    index = int(position)
    fraction = position - index
    rest = 1.0 - fraction
    pa, pb = Q(rest) * Q(float(x0)), Q(fraction) * Q(float(x1))                     # the exact products
    a, b = float(pa), float(pb)                                                     # int / int division: correctly rounded
    unfused, fused_a, fused_b = float(Q(a) + Q(b)), float(pa + Q(b)), float(Q(a) + pb)
    assert unfused == (rest * float(x0)) + (fraction * float(x1))
    return tuple(np.float32(v) for v in (unfused, fused_a, fused_b)), index


# (src, dst, o, bits of x0, bits of x1): found by a seeded search over x0 in +-[0.5, 1) with x1 next to -x0 (1 - f) / f, where the blend
# cancels and a binary64 rounding of a product is worth many binary32 ulps of the result (about one try in fifty hits; random audio does
# about once in 2^29).  tests/test_audio_cpu.py re-proves that each one tells the unfused form from both fused forms.
SENTINELS = ((4, 3, 1, 3204487092, 1065392052), (44100, 48000, 1, 3212730617, 1035204603), (48000, 44100, 1, 1057038459, 3232129024),
             (8000, 48000, 1, 1060102196, 3227244609))


# ------------------------------------------------------------------------------------------------------------------------ bit packing
def ref_bitpack(values, bits):
    """Modules/Encodec/BitPacker.cs:66-90 (Push) + :48-62 (Flush), restated with Python integers."""
    out = bytearray()
    cur, nb = 0, 0
    for v in values:
        cur |= int(v) << nb
        nb += bits
        while nb >= 8:
            out.append(cur & 0xFF)
            cur >>= 8
            nb -= 8
    if nb > 0:
        out.append(cur & 0xFF)
    return bytes(out)


def ref_bitunpack(data, bits, count):
    """Modules/Encodec/BitUnpacker.cs Pull."""
    vals, cur, nb, pos = [], 0, 0, 0
    for _ in range(count):
        while nb < bits:
            cur |= data[pos] << nb
            pos += 1
            nb += 8
        vals.append(cur & ((1 << bits) - 1))
        cur >>= bits
        nb -= bits
    return vals


# The six shapes of the issue have K * T = 1, 7, 15, 32, 783, 96: only 0, 1 and 7 mod 8.  An odd width can end a row on any bit of a byte,
# so five more shapes (K * T = 2 .. 6) complete the residues; every width then runs all eleven.
PACK_SHAPES = ((1, 1), (1, 7), (3, 5), (8, 4), (9, 87), (32, 3)) + ((1, 2), (1, 3), (2, 2), (5, 1), (2, 3))
PACK_ROWS = (1, 3)


def tail_residues(bits, shapes=PACK_SHAPES):
    return {(K * T * bits) % 8 for K, T in shapes}


def possible_residues(bits):
    return {(n * bits) % 8 for n in range(8)}


def slot_bytes(v, bits):
    """How many bytes value v of the stream touches."""
    return (v * bits + bits - 1) // 8 - (v * bits) // 8 + 1


def first_slot_spanning(nbytes, bits, n):
    return next((v for v in range(n) if slot_bytes(v, bits) == nbytes), None)


def to_codes(stream, K, T):
    """[B, K*T] in stream order (t outer, codebook inner: EncodecCompressor.cs:170-181) -> codes [B, K, T]."""
    s = np.asarray(stream, np.int64)
    return np.ascontiguousarray(s.reshape(s.shape[0], T, K).transpose(0, 2, 1))


def to_stream(codes):
    c = np.asarray(codes)
    return c.transpose(0, 2, 1).reshape(c.shape[0], -1)


def pack_patterns(bits, K, T, B):
    """(name, stream [B, K*T]): seeded random values, and the patterns that show a shift leaking into a neighbour -- all ones,
    alternating all-ones and zero in both phases, and one all-ones value among zeros at the first slot, the last slot, the first slot
    that straddles two bytes and the first that straddles three (where the shape has one)."""
    n, full = K * T, (1 << bits) - 1
    rng = np.random.default_rng([bits, K, T, B])
    yield "random", rng.integers(0, 1 << bits, (B, n), dtype=np.int64)
    yield "ones", np.full((B, n), full, np.int64)
    even = np.where(np.arange(n) % 2 == 0, full, 0).astype(np.int64)
    yield "alternating", np.tile(even, (B, 1))
    yield "alternating-odd", np.tile(full - even, (B, 1))
    slots = {"first": 0, "last": n - 1, "two-bytes": first_slot_spanning(2, bits, n), "three-bytes": first_slot_spanning(3, bits, n)}
    for name, v in slots.items():
        if v is not None:
            s = np.zeros((B, n), np.int64)
            s[:, v] = full
            yield "single-" + name, s


def ref_pack_rows(stream, bits):
    """uint8 [B, ceil(n * bits / 8)] of the reference packer, row by row."""
    return np.stack([np.frombuffer(ref_bitpack(row, bits), np.uint8) for row in np.asarray(stream)])
