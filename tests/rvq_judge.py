"""Shared by the quantizer op tests (plain module, not a conftest): the seeded inputs of a DAC quantizer case, the C oracle's stage
loop composed from its existing ops, and the binary64 judgement of one stage.

The stage loop is ResidualVectorQuantizer.forward (ResidualVectorQuantizer.cs:54-103 over VectorQuantizer.cs:67-125) as the oracle's
RefDAC.encode runs it: tests/test_oracle_ops_f64_cpu.py holds the composition to RefDAC.encode bit for bit, tests/test_rvq_ops_gpu.py
holds the engine's two forms of the quantizer to the composition.
"""
import functools
import itertools

import numpy as np

import ref64
from oracle import c_oracle

D = 8                                             # codebook dimension of every case (the one-launch kernel's instantiation)
LATENTS = (256, 512, 768, 1024)                   # what launch_dac_rvq_fused admits
BOOKS = (64, 128, 320, 1024)                      # N % 64 == 0: one, two, five and sixteen codes per lane
STAGES = (1, 3, 9)
# (clips, frames per clip).  A workgroup of the one-launch kernel owns 16 consecutive frames of the flattened (clip, frame) axis:
# (1,1) / (1,15) one partial block, (1,16) one full block, (1,17) a block and one frame, (3,11) and (5,13) clip boundaries inside a block
# and a partial last block, (2,40) five full blocks with the boundary inside the third.
LAYOUTS = ((1, 1), (1, 15), (1, 16), (1, 17), (3, 11), (2, 40), (5, 13))
SHIPPED = (1024, 1024, 9, 4, 300)                 # DAC 44.1 kHz: L, N, n_q of the shipped preset, 1 200 frames


def _thinned():
    """28 of the 4 x 4 x 3 x 7 cells: every latent width with every layout, the book and the stage count rotated so that every value
    of each axis meets every value of each other axis (asserted below)."""
    cases = []
    for f, (B, T) in enumerate(LAYOUTS):
        for l, L in enumerate(LATENTS):
            cases.append((L, BOOKS[(l + f) % 4], STAGES[(l + 2 * f) % 3], B, T))
    return cases


CASES = _thinned()
for _a, _b in itertools.combinations(range(4), 2):
    _axes = (LATENTS, BOOKS, STAGES, LAYOUTS)
    _val = lambda c, k: (c[3], c[4]) if k == 3 else c[k]
    assert {(_val(c, _a), _val(c, _b)) for c in CASES} == set(itertools.product(_axes[_a], _axes[_b])), (_a, _b)


def case_id(case):
    return "L%d-N%d-q%d-B%dxT%d" % tuple(case)


def inputs(L, N, n_q, B, T, seed=None, dim=D):
    """residual ~ N(0,1), w_in ~ N(0, 1/L), w_out ~ N(0, 1/D), biases ~ 0.1 N(0,1), codebooks ~ N(0,1); binary32, seeded by the shape."""
    rng = np.random.default_rng([L, N, n_q, B, T, dim] if seed is None else seed)
    f = lambda *shape, scale=1.0: (rng.standard_normal(shape) * scale).astype(np.float32)
    return dict(r=f(B, L, T), w_in=f(n_q, dim, L, scale=1.0 / np.sqrt(L)), b_in=f(n_q, dim, scale=0.1), cb=f(n_q, N, dim),
                w_out=f(n_q, L, dim, scale=1.0 / np.sqrt(dim)), b_out=f(n_q, L, scale=0.1))


def oracle_stages(r, w_in, b_in, cb, w_out, b_out):
    """The oracle's quantizer on residual r [B,L,T]: per stage z_e = in_proj(r), (idx, st) = nearest code and its straight-through value,
    q = out_proj(st), then zq = zq + q and r = r - q in binary32 (one rounding each).  Returns (stages, codes [B,n_q,T], latents
    [B,n_q*D,T], zq [B,L,T]); stages[i] holds that stage's r_in, z_e, idx, st and q."""
    r = np.ascontiguousarray(r, np.float32).copy()
    zq = np.zeros_like(r)
    stages = []
    for i in range(len(cb)):
        z_e = c_oracle.conv1d(r, w_in[i][:, :, None], None if b_in is None else b_in[i])
        idx, st = c_oracle.vq_argmin(z_e, cb[i])[:2]
        q = c_oracle.conv1d(st, w_out[i][:, :, None], None if b_out is None else b_out[i])
        stages.append(dict(r_in=r, z_e=z_e, idx=idx, st=st, q=q))
        with np.errstate(invalid="ignore"):       # inf - inf of the non-finite cases
            zq = zq + q
            r = r - q
    codes = np.stack([s["idx"] for s in stages], axis=1)
    lat = np.concatenate([s["z_e"] for s in stages], axis=1)
    return stages, codes, lat, zq


@functools.lru_cache(maxsize=None)
def case(L, N, n_q, B, T):
    """(inputs, oracle_stages of them) of a case, computed once per process and shared by the tests that need it: read-only."""
    x = inputs(L, N, n_q, B, T)
    out = oracle_stages(**x)
    for a in list(x.values()) + [out[1], out[2], out[3]] + [v for s in out[0] for v in s.values()]:
        a.setflags(write=False)
    return x, out


def _worst(err, allowed):
    return float((err / np.maximum(allowed, 1e-300)).max())


def judge_projection(got, x, w, b, what):
    """A 1x1 projection got = w . x + b (binary32) against binary64 within the derived bound of its chain; returns worst error / allowed."""
    want = ref64.conv1d(x, w[:, :, None], b)
    bound = ref64.conv1d_bound(x, w[:, :, None], b)
    err = np.abs(got.astype(np.float64) - want)
    assert got.shape == want.shape
    assert np.all(err <= bound), f"{what}: |binary32 - binary64| is {_worst(err, bound):.3g} x the allowed error at its worst element"
    return _worst(err, bound)


def judge_choice(idx, z_e, book, what):
    """The chosen codes against binary64 distances: the kernel chose c over the true nearest m, so its binary32 distances satisfied
    d32(c) <= d32(m), hence d64(c) - d64(m) <= bound(c) + bound(m) with ref64.vq_distances' bound of a binary32 distance.  Frames whose
    index differs from the binary64 argmin are counted, not capped.  Returns (worst excess / room, differing frames)."""
    dist, want, _, bound = ref64.vq_distances(z_e, book, "dac")
    pick = lambda a, i: np.take_along_axis(a, i[..., None], -1)[..., 0]
    excess = pick(dist, idx) - pick(dist, want)
    room = pick(bound, idx) + pick(bound, want)
    differ = int((idx != want).sum())
    if differ:
        print(f"{what}: {differ} of {idx.size} frames differ from the binary64 argmin; worst excess / room {_worst(excess, room):.3g}")
    assert np.all(excess <= room), f"{what}: a chosen code is farther than the binary32 bound allows ({_worst(excess, room):.3g} x)"
    return _worst(excess, room), differ
