"""GPU suite: Dia's output stage on the device (csrc/nc_dia.hip) -- delayed codes to PCM in one ragged call.

Truth for the kernels is the numpy restatement tests/dia_output_ref.py (which tests/test_dia_output_cpu.py holds to a torch-CPU
transcription of the reference); truth for the decode is the existing engine on the host-reverted codes: decode_codes_ragged on the
packed codes and decode_code_matrix on every item alone.  np.array_equal everywhere, no tolerance.  The reduced-width DAC fixture of
tests/test_ragged_gpu.py (4 codebooks of 64 entries, a decoder stride of 5): the decode tests mask to [0, 63], the codebook it has."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dia_output_ref as R  # noqa: E402
from conftest import dac_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import DAC, DACConfig, _lib, adjust_speed, dia, dia_apply_delay, dia_revert_delay  # noqa: E402
from neuralcodecs_amd.weights import dac_synthetic_state_dict, save_blob  # noqa: E402

PAD, BOS = 1025, 1026
PATTERNS = {"zero": [0, 0, 0, 0], "increasing": [0, 2, 3, 5], "non_monotone": [3, 0, 5, 1]}
SPEEDS = (0.5, 0.8, 0.99999, 1.0, 1.25, 3.0)
LENGTHS = (2, 3, 17, 1000)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _codes(B, T, Cn, seed, hi=1024):
    """codes in [0, hi) with -1, 1024, the pad and the bos value sprinkled in; the last step of every channel is one of them too"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, hi, (B, T, Cn)).astype(np.int64)
    n = max(4, c.size // 6)
    c.reshape(-1)[rng.integers(0, c.size, n)] = rng.choice([-1, 1024, PAD, BOS], n)
    c[:, -1, 0] = BOS
    return c


def _launches(m, fn):
    m.profile_enable(True)
    m.profile_reset()
    out = fn()
    p = m.profile_read()
    m.profile_enable(False)
    return out, sum(v["launches"] for v in p.values()), p["elem"]["launches"]


@pytest.fixture(scope="module")
def dac():
    g = load_golden("dac_small")
    cfg = dac_cfg_from_meta(g["meta"])
    m = DAC(cfg)
    m.load_blob(save_blob(dac_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"])))
    m.set_chunk_frames(_lib.NC_CHUNK_OFF)
    assert cfg.n_codebooks == 4 and cfg.codebook_size == 64
    yield m
    m.dispose()


# ---- the code kernels -------------------------------------------------------------------------------------------------------------
def _lengths(B, T, md, k):
    """valid lengths of a batch: the longest allowed, 1 and an odd one in turn (odd F: rows 1 and 3 of an item start at odd offsets)"""
    full = T - md
    return [(full, 1, max(1, full - 1 - (full % 2 == 1)))[(b + k) % 3] for b in range(B)]


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_revert_pack_apply_kernels_equal_the_restatement(name):
    delay = PATTERNS[name]
    md, Cn = max(delay), len(delay)
    odd_rows = 0
    for k, T in enumerate([md + 1, md + 2, 63, 64, 65, 257]):
        for B in (1, 3):
            c = _codes(B, T, Cn, 1000 * T + B)
            want = R.mask_invalid(R.revert_delay(c, delay))
            got = dia_revert_delay(c, delay)
            assert got.shape == want.shape and np.array_equal(got, want), ("revert", name, T, B)
            assert np.array_equal(dia_revert_delay(c, delay, (5, 40)), R.mask_invalid(R.revert_delay(c, delay), 5, 40))
            lens = _lengths(B, T, md, k)
            packed = dia.dia_revert_pack(c, lens, delay)
            flat = np.concatenate([p.reshape(-1) for p in packed])
            assert np.array_equal(flat, R.pack_items(want, lens)), ("pack", name, T, B, lens)
            off = np.cumsum([0] + [Cn * n for n in lens])
            odd_rows += sum(1 for b, n in enumerate(lens) for ch in range(Cn) if (off[b] + ch * n) % 2)
            got = dia_apply_delay(c, delay, BOS, PAD)
            assert np.array_equal(got, R.apply_delay(c, delay, BOS, PAD)), ("apply", name, T, B)
            if T > md:
                assert np.array_equal(dia_revert_delay(got, delay, (-10, 5000)), c[:, :T - md, :])   # delay, then revert: the clip back
    assert odd_rows > 0
    c = _codes(2, 70, Cn, 9)
    assert np.array_equal(dia_revert_delay(c[0], delay), R.mask_invalid(R.revert_delay(c[:1], delay))[0])   # [T, C] form


def test_revert_pack_many_items_and_a_long_one():
    """more items than one launch carries (32), and an item of several tiles next to items of one step"""
    delay = PATTERNS["non_monotone"]
    md, Cn, B, T = max(delay), 4, 37, 300
    c = _codes(B, T, Cn, 77)
    lens = [1 + (13 * b) % (T - md) for b in range(B)]
    lens[5], lens[33] = T - md, T - md
    packed = dia.dia_revert_pack(c, lens, delay)
    want = R.mask_invalid(R.revert_delay(c, delay))
    assert np.array_equal(np.concatenate([p.reshape(-1) for p in packed]), R.pack_items(want, lens))


# ---- the decode -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decode_case(dac):
    """delayed codes of 5 items, host-reverted codes, the per-item truth -- computed once"""
    delay = PATTERNS["increasing"]
    md, T = max(delay), 40
    lens = [1, T - md, 17, 17, 30]
    c = _codes(len(lens), T, 4, 123, hi=64)
    rev = R.mask_invalid(R.revert_delay(c, delay), 0, 63)
    solo = [_np(dac.decode_code_matrix(np.ascontiguousarray(rev[b, :n, :]))) for b, n in enumerate(lens)]
    ragged = [_np(p) for p in dac.decode_codes_ragged([np.ascontiguousarray(rev[b, :n, :].T) for b, n in enumerate(lens)])]
    return dict(delay=delay, T=T, lens=lens, codes=c, solo=solo, ragged=ragged)


def test_decode_dia_output_equals_the_ragged_decode_and_every_item_alone(dac, decode_case):
    k = decode_case
    got = dac.decode_dia_output(k["codes"], k["lens"], k["delay"], valid_range=(0, 63))
    assert len(got) == len(k["lens"])
    for b, (g, r, s) in enumerate(zip(got, k["ragged"], k["solo"])):
        assert g.shape == r.shape == s.shape == (dac.decoded_length(k["lens"][b]),)
        assert np.array_equal(g, r), f"item {b}: differs from decode_codes_ragged on the host-reverted codes"
        assert np.array_equal(g, s), f"item {b}: differs from decode_code_matrix on the item alone"
    fr, dl, ol = dia.output_query(dac, k["T"], k["lens"], k["delay"])
    assert fr == k["lens"] and dl == ol == [dac.decoded_length(n) for n in k["lens"]]


def test_decode_dia_output_with_speed_equals_the_restatement_on_the_decoded_items(dac, decode_case):
    k = decode_case
    speeds = [1.0, 0.8, 1.25, 0.99999, 3.0]
    got = dac.decode_dia_output(k["codes"], k["lens"], k["delay"], speed=speeds, valid_range=(0, 63))
    _, dl, ol = dia.output_query(dac, k["T"], k["lens"], k["delay"], speeds)
    for b, (g, s, sp) in enumerate(zip(got, k["solo"], speeds)):
        want = R.adjust_speed(s, sp)
        assert ol[b] == want.shape[0] == R.adjust_speed_len(dl[b], sp)
        assert g.shape == want.shape and np.array_equal(g, want), (b, sp)
    one = dac.decode_dia_output(k["codes"], k["lens"], k["delay"], speed=0.8, valid_range=(0, 63))     # one factor for all
    assert all(np.array_equal(g, R.adjust_speed(s, 0.8)) for g, s in zip(one, k["solo"]))


def test_device_tensors_stay_on_the_device_and_the_launches_are_the_ragged_ones(dac, decode_case):
    import torch
    k = decode_case
    dev = torch.device("cuda", dac.device_index)
    ct = torch.from_numpy(k["codes"]).to(dev)
    rev = R.mask_invalid(R.revert_delay(k["codes"], k["delay"]), 0, 63)
    packed = [torch.from_numpy(np.ascontiguousarray(rev[b, :n, :].T)).to(dev) for b, n in enumerate(k["lens"])]
    _, n_ragged, e_ragged = _launches(dac, lambda: dac.decode_codes_ragged(packed))
    plain, n_plain, e_plain = _launches(dac, lambda: dac.decode_dia_output(ct, k["lens"], k["delay"], valid_range=(0, 63)))
    sped, n_sped, e_sped = _launches(dac, lambda: dac.decode_dia_output(ct, k["lens"], k["delay"], speed=[1.0, 0.8, 1.25, 1.0, 3.0], valid_range=(0, 63)))
    same, n_same, _ = _launches(dac, lambda: dac.decode_dia_output(ct, k["lens"], k["delay"], speed=1.0, valid_range=(0, 63)))
    torch.cuda.synchronize()
    dac.check_errors()
    assert all(t.is_cuda for t in plain + sped + same)
    assert (n_plain, e_plain) == (n_ragged + 1, e_ragged + 1)          # one revert-pack launch in front of the ragged sequence
    assert (n_sped, e_sped) == (n_ragged + 2, e_ragged + 2)            # and one adjust launch behind it
    assert n_same == n_ragged + 1                                      # no row changes its length: nothing to adjust
    for g, s in zip(plain, k["solo"]):
        assert np.array_equal(_np(g), s)
    for g, s, sp in zip(sped, k["solo"], [1.0, 0.8, 1.25, 1.0, 3.0]):
        assert np.array_equal(_np(g), R.adjust_speed(s, sp))
    d = PATTERNS["non_monotone"]
    c = _codes(2, 65, 4, 5)
    tc = torch.from_numpy(c).to(dev)
    a, r = dia_apply_delay(tc, d, BOS, PAD), dia_revert_delay(tc, d)
    w = adjust_speed([torch.from_numpy(k["solo"][1]).to(dev)], 1.25)
    assert a.is_cuda and r.is_cuda and w[0].is_cuda
    torch.cuda.synchronize()
    assert np.array_equal(_np(a), R.apply_delay(c, d, BOS, PAD)) and np.array_equal(_np(r), R.mask_invalid(R.revert_delay(c, d)))
    assert np.array_equal(_np(w[0]), R.adjust_speed(k["solo"][1], 1.25))


# ---- the speed kernel -------------------------------------------------------------------------------------------------------------
def _wave(L, seed):
    return np.random.default_rng(seed).standard_normal(L).astype(np.float32)


def test_adjust_speed_kernel_equals_the_restatement():
    for L in LENGTHS:
        fp = _wave(L, 11 * L)
        got = adjust_speed([fp] * len(SPEEDS), SPEEDS)                   # the six speeds as six rows of one call
        for g, sp in zip(got, SPEEDS):
            want = R.adjust_speed(fp, sp)
            assert g.shape == want.shape and np.array_equal(g, want), (L, sp, int((g != want).sum()) if g.shape == want.shape else None)
    long_row = _wave(100003, 3)
    for sp in (0.99999, 0.8, 1.25):
        got = adjust_speed(long_row, sp)
        want = R.adjust_speed(long_row, sp)
        assert got.shape == want.shape and np.array_equal(got, want), (sp, int((got != want).sum()))
    assert adjust_speed(long_row, 0.99999).shape == (100004,)


def test_adjust_speed_mixed_rows_in_one_call_and_more_rows_than_one_launch():
    rows = [_wave(n, n) for n in (1000, 17, 333, 2, 1)]
    speeds = [1.0, 0.5, 3.0, 0.5, 1.0]                                   # unchanged, stretched, shrunk, the shortest row, one sample
    got = adjust_speed(rows, speeds)
    for g, r, sp in zip(got, rows, speeds):
        assert np.array_equal(g, R.adjust_speed(r, sp))
    assert [g.shape[0] for g in got] == [1000, 34, 111, 4, 1]
    many = [_wave(5 + b, 100 + b) for b in range(40)]
    sp = [(0.5, 1.0, 1.25, 3.0)[b % 4] for b in range(40)]
    for g, r, s in zip(adjust_speed(many, sp), many, sp):
        assert np.array_equal(g, R.adjust_speed(r, s))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_output_query_values_and_every_refusal(dac):
    L = _lib.lib()
    delay = PATTERNS["increasing"]
    i32 = lambda v: (C.c_int32 * len(v))(*v)                              # noqa: E731
    f32 = lambda v: (C.c_float * len(v))(*v)                              # noqa: E731
    fr, dl, ol = (C.c_int64 * 3)(), (C.c_int64 * 3)(), (C.c_int64 * 3)()

    def q(B=3, T=40, Cn=4, d=delay, lens=(1, 35, 17), speed=None, h=None):
        return L.nc_dia_output_query(dac._h if h is None else h, B, T, Cn, i32(list(d)) if d is not None else None,
                                     _lib.i64_array(lens) if lens is not None else None, f32(list(speed)) if speed is not None else None, fr, dl, ol)

    assert q() == _lib.NC_OK
    assert list(fr) == [1, 35, 17] and list(dl) == list(ol) == [dac.decoded_length(n) for n in (1, 35, 17)]
    assert q(speed=(0.5, 1.0, 3.0)) == _lib.NC_OK
    assert list(ol) == [R.adjust_speed_len(n, s) for n, s in zip(dl, (0.5, 1.0, 3.0))] and ol[0] == 2 * dl[0] and ol[1] == dl[1]
    assert L.nc_dia_output_query(dac._h, 3, 40, 4, i32(delay), _lib.i64_array((1, 35, 17)), None, None, None, None) == _lib.NC_OK   # outputs nullable
    E = _lib.NC_EINVAL
    assert q(Cn=3, d=delay[:3]) == E and b"codebooks" in L.nc_last_error()          # C != n_codebooks
    assert q(Cn=5, d=delay + [1]) == E
    assert q(d=[0, 2, -1, 5]) == E                                                    # a negative delay
    assert q(T=5) == E and q(T=4) == E                                                # T_gen <= max(delay)
    assert q(T=6, lens=(1, 1, 1)) == _lib.NC_OK
    assert q(lens=(1, 0, 17)) == E and q(lens=(1, -3, 17)) == E                       # a length <= 0
    assert q(lens=(1, 36, 17)) == E                                                   # > T_gen - max(delay)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert q(speed=(1.0, bad, 1.0)) == E, bad                                     # a speed that is not finite or <= 0
    assert q(B=0) == E and q(lens=None) == E and q(d=None) == E
    with DAC(DACConfig(n_codebooks=33)) as wide:                                      # C > 32, on a handle that has that many
        assert L.nc_dia_output_query(wide._h, 1, 40, 33, i32([0] * 33), _lib.i64_array([5]), None, fr, dl, ol) == E


def test_refusals_leave_the_handle_usable(dac, decode_case):
    L, k = _lib.lib(), decode_case
    c = np.ascontiguousarray(k["codes"])
    B, T, Cn = c.shape
    delay = (C.c_int32 * 4)(*k["delay"])
    lens = _lib.i64_array(k["lens"])
    out = np.full(sum(s.shape[0] for s in k["solo"]) + 8, -7.0, np.float32)
    for fn in (L.nc_dia_decode_output, L.nc_dia_decode_output_dev):
        assert fn(dac._h, c.ctypes.data, B, T, 3, delay, lens, 0, 63, None, out.ctypes.data) == _lib.NC_EINVAL              # a wrong C
        assert fn(dac._h, c.ctypes.data, B, T, Cn, delay, _lib.i64_array([1, T, 17, 17, 30]), 0, 63, None, out.ctypes.data) == _lib.NC_EINVAL   # too long
        assert fn(dac._h, None, B, T, Cn, delay, lens, 0, 63, None, out.ctypes.data) == _lib.NC_EINVAL                      # null pointers
        assert fn(dac._h, c.ctypes.data, B, T, Cn, delay, lens, 0, 63, None, None) == _lib.NC_EINVAL
        assert fn(dac._h, c.ctypes.data, B, T, Cn, None, lens, 0, 63, None, out.ctypes.data) == _lib.NC_EINVAL
        assert fn(dac._h, c.ctypes.data, B, T, Cn, delay, None, 0, 63, None, out.ctypes.data) == _lib.NC_EINVAL
        assert fn(dac._h, c.ctypes.data, B, T, Cn, delay, lens, 0, 1023, None, out.ctypes.data) == _lib.NC_EINVAL           # codes past the codebook
        assert fn(dac._h, c.ctypes.data, B, T, Cn, delay, lens, -1, 63, None, out.ctypes.data) == _lib.NC_EINVAL
        assert fn(dac._h, c.ctypes.data, B, T, Cn, delay, lens, 0, 63, (C.c_float * 5)(1, 1, 0, 1, 1), out.ctypes.data) == _lib.NC_EINVAL
    assert np.all(out == -7.0)
    with pytest.raises(ValueError):
        adjust_speed([np.zeros(1, np.float32)], 0.5)                                  # one sample cannot be interpolated
    with pytest.raises(ValueError):
        dia_revert_delay(np.zeros((1, 5, 4), np.int64), [0, 2, 3, 5])                 # nothing behind the delay
    with pytest.raises(ValueError):
        dia_apply_delay(np.zeros((1, 5, 4), np.int64), [0, 2, -3, 5], BOS)
    dac.synchronize()
    dac.check_errors()
    got = dac.decode_dia_output(k["codes"], k["lens"], k["delay"], valid_range=(0, 63))
    assert all(np.array_equal(g, s) for g, s in zip(got, k["solo"]))
