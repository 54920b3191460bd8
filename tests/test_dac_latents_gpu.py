"""GPU suite: DAC.from_latents (nc_dac_from_latents[_dev]) -- continuous latents back to codes, raw codebook rows and z.

Judges as elsewhere: the C oracle for bits (codes == oracle codes, z == oracle.from_codes at max-abs 0, projected == the state dict's
codebook rows) and binary64 for meaning (tests/ref64.py vq_distances: the chosen code is a nearest code up to the binary32 error bound of
a distance).  Two configurations: the small golden one (64 codes: one code per lane) and the same with 256 codes (four codes per lane, the
scan loop of the lookup kernel).  A workgroup of the lookup holds 16 frames, a wavefront 4."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import dac_cfg_from_meta, snac_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import DAC, SNAC, _lib, ops  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob, snac_synthetic_state_dict, synthetic_pcm  # noqa: E402
from oracle import c_oracle  # noqa: E402

FRAMES = (1, 15, 16, 17, 63, 64, 65, 130)


class Model:
    def __init__(self, cfg, seed, edit=None):
        self.cfg = cfg
        self.sd = dac_synthetic_state_dict(cfg, seed=seed)
        if edit:
            edit(self.sd)
        blob = save_blob(self.sd)
        self.m = DAC(cfg)
        self.m.load_blob(blob)
        self.ref = c_oracle.RefDAC(cfg, blob)
        self.D, self.nq = cfg.codebook_dim, cfg.n_codebooks
        self.books = [np.asarray(self.sd[f"quantizer.quantizers.{i}.codebook.weight"], np.float32) for i in range(self.nq)]
        self._enc = {}

    def encoded(self, frames, B):
        """(latents, codes) of the ORACLE's encode of B seeded clips of `frames` frames; the oracle runs clip by clip, so the B = 3
        result is computed once per length and its first rows serve B = 1."""
        if frames not in self._enc:
            pcm = synthetic_pcm(3, 1, frames * self.cfg.hop_length, self.cfg.sample_rate, seed=100 + frames)
            _, codes, lat, _ = self.ref.encode(pcm)
            self._enc[frames] = (lat, codes)
        lat, codes = self._enc[frames]
        return np.ascontiguousarray(lat[:B]), np.ascontiguousarray(codes[:B])

    def rows(self, codes):
        """the raw codebook rows of codes [B, n_q, T] -> [B, n_q * D, T], by numpy indexing of the state dict"""
        return np.concatenate([self.books[i][codes[:, i, :]].transpose(0, 2, 1) for i in range(codes.shape[1])], axis=1)


@pytest.fixture(scope="module")
def small(golden_small):
    s = Model(dac_cfg_from_meta(golden_small["meta"]), golden_small["meta"]["weight_seed"])
    yield s
    s.m.dispose()


@pytest.fixture(scope="module")
def wide(golden_small):
    s = Model(dataclasses.replace(dac_cfg_from_meta(golden_small["meta"]), codebook_size=256), 23)
    yield s
    s.m.dispose()


def free_latents(s, B, T, scale, seed, C_lat=None):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, C_lat or s.nq * s.D, T)) * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ 1. round trip
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("B", (1, 3))
def test_round_trip_of_the_encoders_latents(small, B, frames):
    lat, rcodes = small.encoded(frames, B)
    z, proj, codes = small.m.from_latents(lat)
    assert codes.dtype == np.int64 and codes.shape == (B, small.nq, frames) and proj.shape == lat.shape
    assert np.array_equal(codes, rcodes)
    want = small.ref.from_codes(rcodes)
    assert z.shape == want.shape and float(np.abs(z - want).max()) == 0.0
    assert np.array_equal(proj, small.rows(rcodes))


# ---------------------------------------------------------------------------------------------------------------- 2. free latents
@pytest.mark.parametrize("scale", (1.0, 1e-3))
@pytest.mark.parametrize("which", ("small", "wide"))
def test_free_latents_choose_a_nearest_code(request, which, scale):
    """Per codebook slice the codes are the C oracle's argmin; in binary64 the chosen code is as near as the nearest one up to what two
    binary32 distances may be off by: each is (|e|^2 + |c|^2) - 2 e.c, three D-term chains and two additions, bounded in
    ref64.vq_distances by gamma(D + 2) * sum (|e_d| + |c_d|)^2.  The kernel chose c over the true nearest m, so its binary32 distances
    satisfy d32(c) <= d32(m), hence d64(c) - bound(c) <= d64(m) + bound(m)."""
    import ref64
    s = request.getfixturevalue(which)
    B, T = 2, 37
    lat = free_latents(s, B, T, scale, seed=5)
    z, proj, codes = s.m.from_latents(lat)
    for i in range(s.nq):
        sl = lat[:, i * s.D:(i + 1) * s.D, :]
        assert np.array_equal(codes[:, i, :], c_oracle.vq_argmin(sl, s.books[i])[0]), f"codebook {i}"
        dist, want, _, bound = ref64.vq_distances(sl, s.books[i], "dac")
        pick = lambda a, idx: np.take_along_axis(a, idx[..., None], -1)[..., 0]
        got = codes[:, i, :]
        excess = pick(dist, got) - pick(dist, want)
        room = pick(bound, got) + pick(bound, want)
        print(f"{which} scale {scale} codebook {i}: max excess {excess.max():.3e}, least room {room.min():.3e}, differing frames {int((got != want).sum())}")
        assert np.all(excess <= room), f"codebook {i}: a chosen code is farther than the binary32 bound allows"
    assert np.array_equal(proj, s.rows(codes))
    assert np.array_equal(z, s.ref.from_codes(codes))


# ---------------------------------------------------------------------------------------------------------------- 3. channel rule
def test_channel_rule(small):
    s, T = small, 21
    full = free_latents(s, 2, T, 1.0, seed=9, C_lat=(s.nq + 1) * s.D)
    base = s.m.from_latents(np.ascontiguousarray(full[:, :s.nq * s.D]))
    more = s.m.from_latents(np.ascontiguousarray(full[:, :s.nq * s.D + 5]))          # 5 channels that fit no codebook: ignored
    for a, b in zip(base, more):
        assert np.array_equal(a, b)
    z1, p1, c1 = s.m.from_latents(np.ascontiguousarray(full[:, :s.D]))               # one codebook
    assert c1.shape == (2, 1, T) and p1.shape == (2, s.D, T)
    assert np.array_equal(c1, base[2][:, :1]) and np.array_equal(p1, base[1][:, :s.D]) and np.array_equal(z1, s.ref.from_codes(c1))
    zn, pn, cn = s.m.from_latents(full)                                              # one slice more than there are codebooks
    assert cn.shape == (2, s.nq, T)
    for a, b in zip(base, (zn, pn, cn)):
        assert np.array_equal(a, b)
    few = np.ascontiguousarray(full[:, :s.D - 1])
    z = np.full((2, s.m.latent_dim, T), 7.0, np.float32); p = np.full((2, s.D, T), 7.0, np.float32); c = np.full((2, 1, T), 7, np.int64)
    st = _lib.lib().nc_dac_from_latents(s.m._h, few.ctypes.data, 2, s.D - 1, T, z.ctypes.data, p.ctypes.data, c.ctypes.data)
    assert st == _lib.NC_EINVAL
    assert np.all(z == 7.0) and np.all(p == 7.0) and np.all(c == 7)                  # nothing written
    with pytest.raises(ValueError):
        s.m.from_latents(few)


# ------------------------------------------------------------------------------------------------------------------------ 4. ties
@pytest.mark.parametrize("N", (64, 256))
def test_ties_go_to_the_first_index(golden_small, N):
    """Every row of every codebook twice (row n + N/2 == row n): each distance occurs twice, bit for bit, and the first index wins."""
    cfg = dataclasses.replace(dac_cfg_from_meta(golden_small["meta"]), codebook_size=N)

    def twice(sd):
        for k in sd:
            if k.endswith("codebook.weight"):
                sd[k] = np.concatenate([sd[k][:N // 2], sd[k][:N // 2]]).astype(np.float32)
    s = Model(cfg, 31, edit=twice)
    lat = free_latents(s, 3, 45, 1.0, seed=2)
    z, proj, codes = s.m.from_latents(lat)
    s.m.dispose()
    assert codes.max() < N // 2
    for i in range(s.nq):
        assert np.array_equal(codes[:, i, :], c_oracle.vq_argmin(lat[:, i * s.D:(i + 1) * s.D, :], s.books[i][:N // 2])[0])
    assert np.array_equal(proj, s.rows(codes))


# ------------------------------------------------------------------------------------------------------------------ 5. non-finite
def test_non_finite_latents_follow_the_argmin_op_and_stay_in_their_frames(wide):
    s, T = wide, 40
    lat = free_latents(s, 2, T, 1.0, seed=13)
    clean = s.m.from_latents(lat)
    bad = lat.copy()
    hits = [(0, 3, 5, np.nan), (0, s.D + 1, 16, np.inf), (1, 2 * s.D, 17, -np.inf), (1, 3 * s.D + 7, 39, np.nan), (1, 0, 0, np.inf)]
    for b, ch, t, v in hits:
        bad[b, ch, t] = v
    z, proj, codes = s.m.from_latents(bad)
    for i in range(s.nq):
        want, _ = ops.vq_argmin(bad[:, i * s.D:(i + 1) * s.D, :], s.books[i])
        assert np.array_equal(codes[:, i, :], want), f"codebook {i}"
    assert np.array_equal(proj, s.rows(codes))
    touched = np.zeros((2, T), bool)
    for b, _, t, _ in hits:
        touched[b, t] = True
    keep = ~touched
    for got, want in zip((z, proj, codes), clean):
        assert np.array_equal(got.transpose(0, 2, 1)[keep], want.transpose(0, 2, 1)[keep])


# ------------------------------------------------------------------------------------------------------------ 6. batch invariance
def test_rows_of_a_batch_equal_the_single_calls(small):
    lat, _ = small.encoded(65, 3)
    full = small.m.from_latents(lat)
    for b in range(3):
        one = small.m.from_latents(lat[b:b + 1])
        for a, o in zip(full, one):
            assert np.array_equal(a[b:b + 1], o)


# ------------------------------------------------------------------------------------------------------------------ 7. device form
def test_device_tensors_on_a_side_stream_equal_the_host_form(small):
    import torch
    lat, _ = small.encoded(130, 3)
    host = small.m.from_latents(lat)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.from_numpy(lat).cuda()
        dev = small.m.from_latents(x)
    side.synchronize()
    assert all(t.is_cuda for t in dev) and dev[2].dtype == torch.int64
    for d, h in zip(dev, host):
        assert np.array_equal(d.cpu().numpy(), h)


# --------------------------------------------------------------------------------------------------------------- 8. output subsets
def test_each_single_output_equals_the_full_call_and_launch_counts(small):
    import torch
    s = small
    lat, _ = s.encoded(63, 3)
    B, Cl, T = lat.shape
    full = s.m.from_latents(lat)
    L = _lib.lib()
    for k in range(3):
        outs = [np.empty_like(a) for a in full]
        ptrs = [outs[j].ctypes.data if j == k else None for j in range(3)]
        _lib.check(L.nc_dac_from_latents(s.m._h, lat.ctypes.data, B, Cl, T, *ptrs))
        assert np.array_equal(outs[k], full[k]), "host form, output %d alone" % k
    x = torch.from_numpy(lat).cuda()
    s.m._bind_torch_stream()
    s.m.profile_enable(True)
    launches = []
    for k in range(3):
        outs = [torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device="cuda") for a in full]
        ptrs = [outs[j].data_ptr() if j == k else None for j in range(3)]
        s.m.profile_reset()
        _lib.check(L.nc_dac_from_latents_dev(s.m._h, x.data_ptr(), B, Cl, T, *ptrs))
        torch.cuda.synchronize()
        launches.append(sum(v["launches"] for v in s.m.profile_read().values()))
        assert np.array_equal(outs[k].cpu().numpy(), full[k]), "device form, output %d alone" % k
    s.m.profile_enable(False)
    assert launches == [1 + s.nq, 1, 1]          # z: the lookup and n_q out-projections (and a memset); projected / codes: the lookup alone
    assert L.nc_dac_from_latents(s.m._h, lat.ctypes.data, B, Cl, T, None, None, None) == _lib.NC_EINVAL


# ---------------------------------------------------------------------------------------------------------------- 9. packed ragged
def test_clips_packed_end_to_end_are_one_call(small):
    clips = [small.encoded(f, 1)[0] for f in (15, 17, 63)]
    clips = [clips[0][:, :, :5], clips[1], clips[2][:, :, :40]]                      # 5, 17 and 40 frames
    packed = small.m.from_latents(np.ascontiguousarray(np.concatenate(clips, axis=2)))
    single = [small.m.from_latents(np.ascontiguousarray(c)) for c in clips]
    for k in range(3):
        assert np.array_equal(packed[k], np.concatenate([one[k] for one in single], axis=2))


# ------------------------------------------------------------------------------------------------------------------ 10. downstream
def test_decode_of_z_equals_decode_of_from_codes(small):
    lat, rcodes = small.encoded(17, 3)
    z, _, codes = small.m.from_latents(lat)
    assert np.array_equal(small.m.decode(z), small.m.decode(small.m.from_codes(codes)))
    assert np.array_equal(small.m.decode(z), small.ref.decode(small.ref.from_codes(rcodes)))


# ------------------------------------------------------------------------------------------- the out-projection in pieces, refusals
def test_cut_out_projection_equals_the_one_launch_form(small):
    """Rows too long for one convolution launch are out-projected piece by piece (the plan of from_codes); a chunk setting forces it."""
    import torch
    lat, _ = small.encoded(130, 3)
    whole = small.m.from_latents(lat)
    small.m.set_chunk_frames(48)
    try:
        cut = small.m.from_latents(lat)
        dev = small.m.from_latents(torch.from_numpy(lat).cuda())
        torch.cuda.synchronize()
    finally:
        small.m.set_chunk_frames(_lib.NC_CHUNK_AUTO)
    for w, c, d in zip(whole, cut, dev):
        assert np.array_equal(w, c) and np.array_equal(w, d.cpu().numpy())


def test_refusals_come_before_any_launch(small):
    import torch
    s, L = small, _lib.lib()
    lat, _ = s.encoded(16, 1)
    Cl, T = lat.shape[1], lat.shape[2]
    host = np.zeros(1 << 16, np.float32)
    dev = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    s.m.profile_enable(True)
    s.m.profile_reset()
    for fn, src, buf in ((L.nc_dac_from_latents, lat.ctypes.data, host.ctypes.data), (L.nc_dac_from_latents_dev, dev.data_ptr(), dev.data_ptr())):
        p = C.c_void_p(buf)
        assert fn(None, src, 1, Cl, T, p, p, p) == _lib.NC_EINVAL
        assert fn(s.m._h, None, 1, Cl, T, p, p, p) == _lib.NC_EINVAL
        assert fn(s.m._h, src, 0, Cl, T, p, p, p) == _lib.NC_EINVAL
        assert fn(s.m._h, src, 1, Cl, 0, p, p, p) == _lib.NC_EINVAL
        assert fn(s.m._h, src, 1, s.D - 1, T, p, p, p) == _lib.NC_EINVAL
        assert fn(s.m._h, src, 1, Cl, (1 << 30) + 1, p, p, p) == _lib.NC_EINVAL
        assert fn(s.m._h, src, 1, Cl, T, None, None, None) == _lib.NC_EINVAL
    torch.cuda.synchronize()
    assert sum(v["launches"] for v in s.m.profile_read().values()) == 0
    s.m.profile_enable(False)
    assert not host.any()
    fresh = DAC(s.cfg)
    with pytest.raises(RuntimeError):
        fresh.from_latents(lat)                                                       # NC_ESTATE: no weights
    fresh.dispose()
    g = load_golden("snac_small")
    scfg = snac_cfg_from_meta(g["meta"])
    snac = SNAC(scfg)
    snac.load_blob(save_blob(snac_synthetic_state_dict(scfg, seed=g["meta"]["weight_seed"])))
    p = C.c_void_p(host.ctypes.data)
    assert L.nc_dac_from_latents(snac._h, lat.ctypes.data, 1, Cl, T, p, p, p) == _lib.NC_EINVAL
    snac.dispose()
    with pytest.raises(ValueError):
        s.m.from_latents(None)
    with pytest.raises(ValueError):
        s.m.from_latents(lat[0])
