"""GPU suite: the host-pointer entries of DAC / SNAC that keep a staging of their own (nc_snac_encode_tensor, nc_snac_process_audio: never
cut into windows, on the handle's window buffers), and the status every DAC / SNAC entry returns for an empty batch, an empty clip and
a null required pointer.  Bit-exact comparisons except where the golden vector itself is a torch result (the tolerance of
test_snac_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import audit_snac_levels, dac_cfg_from_meta, load_golden, snac_cfg_from_meta  # noqa: E402
from neuralcodecs_amd import DAC, SNAC, _lib  # noqa: E402
from neuralcodecs_amd.weights import (dac_synthetic_state_dict, save_blob, snac_noise, snac_synthetic_state_dict,  # noqa: E402
                                      synthetic_pcm)
from oracle import c_oracle  # noqa: E402

LATENT_TOL, GAP_TOL = 3e-5, 1e-4   # test_snac_gpu.py
B = 2


def _snac(name):
    g = load_golden(name)
    cfg = snac_cfg_from_meta(g["meta"])
    blob = save_blob(snac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"]))
    m = SNAC(cfg)
    m.load_blob(blob)
    return g, cfg, blob, m


def test_snac_encode_tensor_host_equals_golden_and_device_form():
    import torch
    g, cfg, blob, m = _snac("snac24k_tensor_b1")
    meta = g["meta"]
    pcm = synthetic_pcm(B, 1, meta["T"], cfg.sampling_rate, seed=meta["pcm_seed"])
    codes, z, zq = m.encode_tensor(pcm, return_latents=True)
    rz, rzq, rcodes = c_oracle.RefSNAC(cfg, blob).encode_tensor(pcm)
    assert [c.shape for c in codes] == [(B, 11), (B, 22), (B, 44)]
    for a, b in zip(codes, rcodes):
        assert np.array_equal(a, b)
    assert np.array_equal(z, rz) and np.array_equal(zq, rzq)
    assert audit_snac_levels([c[:1] for c in codes], g, GAP_TOL) == 0
    assert np.abs(zq[:1, ::16, :] - g["zq_slice"]).max() < LATENT_TOL
    dcodes, dz, dzq = m.encode_tensor(torch.from_numpy(pcm).cuda(), return_latents=True)
    torch.cuda.synchronize()
    for a, b in zip(dcodes, codes):
        assert np.array_equal(a.cpu().numpy(), b)
    assert np.array_equal(dz.cpu().numpy(), z) and np.array_equal(dzq.cpu().numpy(), zq)
    want = np.concatenate(codes, axis=1)
    only = np.full_like(want, -1)                                     # z = NULL, zq = NULL
    _lib.check(_lib.lib().nc_snac_encode_tensor(m._h, pcm.ctypes.data, B, pcm.shape[-1], only.ctypes.data, None, None))
    assert np.array_equal(only, want)
    m.dispose()


def test_snac_process_audio_equals_the_device_pointer_composition():
    """resample -> encode -> decode -> narrow through the device-pointer calls, at the model's rate and at another one."""
    import torch
    g, cfg, blob, m = _snac("snac_small")
    x = synthetic_pcm(1, 1, 1777, cfg.sampling_rate, seed=31)[0, 0]
    for src in (cfg.sampling_rate, cfg.sampling_rate * 2 // 3):
        xd = torch.from_numpy(x).cuda()
        xr = xd if src == cfg.sampling_rate else m.resample_linear(xd, src, cfg.sampling_rate)
        n = int(xr.shape[-1])
        _, frames, _, _ = m.query(n)
        nz = snac_noise(cfg, 1, frames, seed=9)
        audio = m.decode(m.encode(xr.reshape(1, 1, -1)), [torch.from_numpy(a).cuda() for a in nz])
        torch.cuda.synchronize()
        want = audio.cpu().numpy().reshape(-1)[:n]
        got = m.process_audio(x, src, noise=nz)
        assert got.shape == (n,) and np.array_equal(got, want), src
        seeded = m.decode(m.encode(xr.reshape(1, 1, -1)), None, seed=5)
        torch.cuda.synchronize()
        assert np.array_equal(m.process_audio(x, src, seed=5), seeded.cpu().numpy().reshape(-1)[:n]), src
    m.dispose()


# ---------------------------------------------------------------------------------------------------------------- status codes
# (entry, arguments after the handle).  "B" / "N" mark the batch and the length argument, "p:<name>" a required pointer, "o" an optional
# one, anything else is passed as it is.  Each entry is called with B = 0, with N = 0 and with each required pointer null, in its
# host-pointer and in its device-pointer form; everything else is valid.
def _entries(dac, snac, T_dac, fr_dac, T_snac, fr_snac):
    nq = dac.config.n_codebooks
    return [
        (dac, "nc_dac_encode", ["p:pcm", "B", ("N", T_dac), 0, 0, "p:codes", "o", "o"]),
        (dac, "nc_dac_decode", ["p:z", "B", ("N", fr_dac), "p:pcm"]),
        (dac, "nc_dac_from_codes", ["p:codes", "B", nq, ("N", fr_dac), "p:z"]),
        (dac, "nc_dac_decode_code_matrix", ["p:codes", "B", ("N", fr_dac), nq, "p:pcm"]),
        (dac, "nc_dac_encode_code_matrix", ["p:pcm", "B", ("N", T_dac), 0, "p:codes"]),
        (snac, "nc_snac_encode", ["p:pcm", "B", ("N", T_snac), "p:codes", "o", "o"]),
        (snac, "nc_snac_encode_tensor", ["p:pcm", "B", ("N", T_snac), "p:codes", "o", "o"]),
        (snac, "nc_snac_from_codes", ["p:codes", "B", ("N", fr_snac), "p:zq"]),
        (snac, "nc_snac_decode", ["p:codes", "B", ("N", fr_snac), "o", 3, "p:pcm"]),
    ]


def status_table(dac, snac, T_dac, fr_dac, T_snac, fr_snac):
    """{"<entry>:<case>": status} for every DAC / SNAC entry, host and device form, plus nc_snac_process_audio."""
    import torch
    L = _lib.lib()
    host = np.zeros(1 << 20, np.float32)
    dev = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    out = {}
    for m, name, spec in _entries(dac, snac, T_dac, fr_dac, T_snac, fr_snac):
        for suffix, ptr in (("", host.ctypes.data), ("_dev", dev.data_ptr())):
            cases = ["B=0", "N=0"] + [a for a in spec if isinstance(a, str) and a.startswith("p:")]
            for case in cases:
                args = []
                for a in spec:
                    if a == "B":
                        args.append(0 if case == "B=0" else B)
                    elif isinstance(a, tuple):
                        args.append(0 if case == "N=0" else a[1])
                    elif isinstance(a, str):
                        args.append(None if a in ("o", case) else C.c_void_p(ptr))
                    else:
                        args.append(a)
                out[f"{name}{suffix}:{case}"] = int(getattr(L, name + suffix)(m._h, *args))
    hp = C.c_void_p(host.ctypes.data)
    for case, args in (("n=0", (hp, 0, snac.config.sampling_rate, None, 3, hp)), ("p:audio", (None, 100, snac.config.sampling_rate, None, 3, hp)),
                       ("p:out", (hp, 100, snac.config.sampling_rate, None, 3, None)), ("rate=0", (hp, 100, 0, None, 3, hp))):
        out[f"nc_snac_process_audio:{case}"] = int(L.nc_snac_process_audio(snac._h, *args))
    torch.cuda.synchronize()
    return out


def status_models():
    g = load_golden("dac_small")
    dcfg = dac_cfg_from_meta(g["meta"])
    dac = DAC(dcfg)
    dac.load_blob(save_blob(dac_synthetic_state_dict(dcfg, seed=g["meta"]["weight_seed"])))
    g, scfg, _, snac = _snac("snac_small")
    fr_snac = 2 * max(scfg.vq_strides)
    return dac, snac, (3 * dcfg.hop_length + 17, 4, fr_snac * scfg.hop_length - 5, fr_snac)


# The table as status_table() returned it on commit 3541718, the last one with the hand-written host staging (1 = NC_EINVAL).
EXPECTED_STATUS = {
    "nc_dac_decode:B=0": 1,
    "nc_dac_decode:N=0": 1,
    "nc_dac_decode:p:pcm": 1,
    "nc_dac_decode:p:z": 1,
    "nc_dac_decode_code_matrix:B=0": 1,
    "nc_dac_decode_code_matrix:N=0": 1,
    "nc_dac_decode_code_matrix:p:codes": 1,
    "nc_dac_decode_code_matrix:p:pcm": 1,
    "nc_dac_decode_code_matrix_dev:B=0": 1,
    "nc_dac_decode_code_matrix_dev:N=0": 1,
    "nc_dac_decode_code_matrix_dev:p:codes": 1,
    "nc_dac_decode_code_matrix_dev:p:pcm": 1,
    "nc_dac_decode_dev:B=0": 1,
    "nc_dac_decode_dev:N=0": 1,
    "nc_dac_decode_dev:p:pcm": 1,
    "nc_dac_decode_dev:p:z": 1,
    "nc_dac_encode:B=0": 1,
    "nc_dac_encode:N=0": 1,
    "nc_dac_encode:p:codes": 1,
    "nc_dac_encode:p:pcm": 1,
    "nc_dac_encode_code_matrix:B=0": 1,
    "nc_dac_encode_code_matrix:N=0": 1,
    "nc_dac_encode_code_matrix:p:codes": 1,
    "nc_dac_encode_code_matrix:p:pcm": 1,
    "nc_dac_encode_code_matrix_dev:B=0": 1,
    "nc_dac_encode_code_matrix_dev:N=0": 1,
    "nc_dac_encode_code_matrix_dev:p:codes": 1,
    "nc_dac_encode_code_matrix_dev:p:pcm": 1,
    "nc_dac_encode_dev:B=0": 1,
    "nc_dac_encode_dev:N=0": 1,
    "nc_dac_encode_dev:p:codes": 1,
    "nc_dac_encode_dev:p:pcm": 1,
    "nc_dac_from_codes:B=0": 1,
    "nc_dac_from_codes:N=0": 1,
    "nc_dac_from_codes:p:codes": 1,
    "nc_dac_from_codes:p:z": 1,
    "nc_dac_from_codes_dev:B=0": 1,
    "nc_dac_from_codes_dev:N=0": 1,
    "nc_dac_from_codes_dev:p:codes": 1,
    "nc_dac_from_codes_dev:p:z": 1,
    "nc_snac_decode:B=0": 1,
    "nc_snac_decode:N=0": 1,
    "nc_snac_decode:p:codes": 1,
    "nc_snac_decode:p:pcm": 1,
    "nc_snac_decode_dev:B=0": 1,
    "nc_snac_decode_dev:N=0": 1,
    "nc_snac_decode_dev:p:codes": 1,
    "nc_snac_decode_dev:p:pcm": 1,
    "nc_snac_encode:B=0": 1,
    "nc_snac_encode:N=0": 1,
    "nc_snac_encode:p:codes": 1,
    "nc_snac_encode:p:pcm": 1,
    "nc_snac_encode_dev:B=0": 1,
    "nc_snac_encode_dev:N=0": 1,
    "nc_snac_encode_dev:p:codes": 1,
    "nc_snac_encode_dev:p:pcm": 1,
    "nc_snac_encode_tensor:B=0": 1,
    "nc_snac_encode_tensor:N=0": 1,
    "nc_snac_encode_tensor:p:codes": 1,
    "nc_snac_encode_tensor:p:pcm": 1,
    "nc_snac_encode_tensor_dev:B=0": 1,
    "nc_snac_encode_tensor_dev:N=0": 1,
    "nc_snac_encode_tensor_dev:p:codes": 1,
    "nc_snac_encode_tensor_dev:p:pcm": 1,
    "nc_snac_from_codes:B=0": 1,
    "nc_snac_from_codes:N=0": 1,
    "nc_snac_from_codes:p:codes": 1,
    "nc_snac_from_codes:p:zq": 1,
    "nc_snac_from_codes_dev:B=0": 1,
    "nc_snac_from_codes_dev:N=0": 1,
    "nc_snac_from_codes_dev:p:codes": 1,
    "nc_snac_from_codes_dev:p:zq": 1,
    "nc_snac_process_audio:n=0": 1,
    "nc_snac_process_audio:p:audio": 1,
    "nc_snac_process_audio:p:out": 1,
    "nc_snac_process_audio:rate=0": 1,
}


def test_rejected_calls_return_the_recorded_status_and_launch_nothing():
    dac, snac, shape = status_models()
    for m in (dac, snac):
        m.profile_enable(True)
        m.profile_reset()
    got = status_table(dac, snac, *shape)
    assert got == EXPECTED_STATUS, {k: (v, EXPECTED_STATUS.get(k)) for k, v in got.items() if EXPECTED_STATUS.get(k) != v}
    for m in (dac, snac):
        assert sum(v["launches"] for v in m.profile_read().values()) == 0
        m.dispose()
