"""CPU suite: the schedule of the incremental sessions (nc_session_schedule) -- a host function, no device.

For the halos of every shipped preset and of the small test configs, and for every push pattern, the steps must partition the clip: every
frame kept by exactly one step, in order; every kept frame clear of a cut window edge by the halo of that side; bounds on multiples of
align; the resident history bounded by hl + hr + align frames."""
import ctypes as C

import pytest

from conftest import dac_cfg_from_meta, load_golden, snac_cfg_from_meta
from neuralcodecs_amd import DACConfig, SNACConfig, _lib, dac_halo, session_schedule, snac_halo


def _halos():
    out = [("dac_44khz", dac_halo(DACConfig.dac_44khz())), ("dac_44khz_16kbps", dac_halo(DACConfig.dac_44khz_16kbps())),
           ("dac_24khz", dac_halo(DACConfig.dac_24khz())), ("dac_16khz", dac_halo(DACConfig.dac_16khz())),
           ("snac_24khz", snac_halo(SNACConfig.snac_24khz())), ("snac_32khz", snac_halo(SNACConfig.snac_32khz())),
           ("snac_44khz", snac_halo(SNACConfig.snac_44khz())),
           ("dac_small", dac_halo(dac_cfg_from_meta(load_golden("dac_small")["meta"])))]
    for name in ("snac_small", "snac_small_attn"):
        out.append((name, snac_halo(snac_cfg_from_meta(load_golden(name)["meta"]))))
    return out


HALOS = _halos()


def _hl_hr(h, decode):
    return (h["dec_right"], h["dec_left"]) if decode else (h["enc_right"], h["enc_left"])     # as nc_codec_chunk_plan reports them


def _patterns(h, decode):
    """name -> pushes (frames); total = 2 * max(halos) + 4 * align unless the pattern says otherwise"""
    a = h["align"]
    hl, hr = _hl_hr(h, decode)
    total = 2 * max(hl, hr) + 4 * a
    irregular, left, i = [], total, 0
    while left > 0:
        n = min(left, a * (1, 3, 2, 7, 1, 5)[i % 6])
        irregular.append(n)
        left -= n
        i += 1
    pats = {"constant": [a] * (total // a), "irregular": irregular, "one_large_push": [a, hl + hr + 2 * a, a, a],
            "all_in_one": [total]}
    if hr > a:
        pats["shorter_than_hr"] = [a] * ((hr - a) // a)
    return pats


def _check(h, decode, pushes, steps):
    a = h["align"]
    hl, hr = _hl_hr(h, decode)
    total = sum(pushes)
    assert len(steps) == len(pushes) + 1
    P = E = 0
    for i, st in enumerate(steps):
        flush = i == len(pushes)
        if not flush:
            P += pushes[i]
        for k in ("w0", "w1", "k0", "k1"):
            assert st[k] % a == 0 or (flush and st[k] == total), (i, k, st)
        assert st["k0"] == E and st["k1"] >= st["k0"], (i, st)              # in order, no gap, no frame twice
        if st["k1"] > st["k0"]:
            assert st["w0"] == max(0, E - hl) and st["w1"] == P, (i, st)
            assert st["w0"] == 0 or st["k0"] - st["w0"] >= hl, (i, st)        # a cut left edge is hl away
            assert flush or st["w1"] - st["k1"] >= hr, (i, st)                # a cut right edge is hr away
            if not flush:
                assert st["k1"] == (P - hr) // a * a                        # nothing final is held back
        else:
            assert st["w0"] == st["w1"] and not flush, (i, st)
            assert P - hr < E + a                                           # nothing more could have been emitted
        E = st["k1"]
        assert st["resident"] == (0 if flush else P - max(0, E - hl)), (i, st)
        assert st["resident"] <= hl + hr + a, (i, st)
    assert E == total


@pytest.mark.parametrize("decode", [True, False])
@pytest.mark.parametrize("name,h", HALOS, ids=[n for n, _ in HALOS])
def test_every_pattern_partitions_the_clip(name, h, decode):
    assert all(h[k] % h["align"] == 0 and h[k] > 0 for k in ("enc_left", "enc_right", "dec_left", "dec_right"))
    for pname, pushes in _patterns(h, decode).items():
        steps = session_schedule(h, pushes, decode=decode, flush=True)
        _check(h, decode, pushes, steps)
        if pname == "shorter_than_hr":
            assert all(st["k1"] == 0 and st["w0"] == st["w1"] for st in steps[:-1]), "a clip shorter than hr emitted before the flush"
            assert (steps[-1]["w0"], steps[-1]["w1"], steps[-1]["k0"], steps[-1]["k1"]) == (0, sum(pushes), 0, sum(pushes))
        if pname == "all_in_one":                                           # one push: its window is the whole clip
            assert (steps[0]["w0"], steps[0]["w1"], steps[0]["k0"]) == (0, pushes[0], 0)
            assert (steps[-1]["w0"], steps[-1]["w1"]) == (max(0, steps[0]["k1"] - _hl_hr(h, decode)[0]), pushes[0])
        without = session_schedule(h, pushes, decode=decode, flush=False)
        assert without == steps[:-1]


@pytest.mark.parametrize("name,h", HALOS, ids=[n for n, _ in HALOS])
def test_single_push_shorter_than_the_halo_and_flush_is_one_window_of_the_whole_clip(name, h):
    for decode in (True, False):
        n = h["align"]
        steps = session_schedule(h, [n], decode=decode)
        assert steps[0]["k1"] == 0 and steps[0]["resident"] == n
        assert (steps[1]["w0"], steps[1]["w1"], steps[1]["k0"], steps[1]["k1"], steps[1]["resident"]) == (0, n, 0, n, 0)


def test_steady_state_window_is_hl_plus_push_plus_hr():
    for _, h in HALOS:
        for decode in (True, False):
            hl, hr = _hl_hr(h, decode)
            n = 2 * h["align"]
            steps = session_schedule(h, [n] * ((hl + hr) // n + 6), decode=decode, flush=False)
            assert steps[-1]["w1"] - steps[-1]["w0"] == hl + n + hr and steps[-1]["k1"] - steps[-1]["k0"] == n


def test_refusals_do_not_crash():
    L = _lib.lib()
    h = _lib.NcHalo(enc_left=4, enc_right=4, dec_left=4, dec_right=4, align=4)
    steps = (_lib.NcSessionStep * 4)()
    one = _lib.i64_array([4])
    assert L.nc_session_schedule(C.byref(h), 1, 0, None, 1, steps) == _lib.NC_EINVAL          # nothing to flush
    assert L.nc_session_schedule(C.byref(h), 1, 0, one, 1, steps) == _lib.NC_EINVAL
    assert L.nc_session_schedule(None, 1, 1, one, 1, steps) == _lib.NC_EINVAL
    assert L.nc_session_schedule(C.byref(h), 1, 1, None, 1, steps) == _lib.NC_EINVAL
    assert L.nc_session_schedule(C.byref(h), 1, 1, one, 1, None) == _lib.NC_EINVAL
    assert L.nc_session_schedule(C.byref(h), 1, -1, one, 0, steps) == _lib.NC_EINVAL
    assert L.nc_session_schedule(C.byref(h), 0, 1, _lib.i64_array([6]), 1, steps) == _lib.NC_EINVAL   # not a multiple of align
    assert L.nc_session_schedule(C.byref(h), 0, 1, _lib.i64_array([0]), 1, steps) == _lib.NC_EINVAL
    bad = _lib.NcHalo(enc_left=4, enc_right=4, dec_left=4, dec_right=4, align=0)
    assert L.nc_session_schedule(C.byref(bad), 1, 1, one, 1, steps) == _lib.NC_EINVAL
    assert L.nc_session_schedule(C.byref(h), 1, 1, one, 1, steps) == _lib.NC_OK
    with pytest.raises(ValueError):
        session_schedule({"enc_left": 4, "enc_right": 4, "dec_left": 4, "dec_right": 4, "align": 4}, [], flush=True)
    # the session entry points on null handles
    out = C.c_void_p()
    n = C.c_int64()
    assert L.nc_session_create(None, 1, 1, 0, C.byref(out)) == _lib.NC_EINVAL and not out.value
    assert L.nc_session_create(None, 1, 1, 0, None) == _lib.NC_EINVAL
    assert L.nc_session_reset(None) == _lib.NC_EINVAL and L.nc_session_pending(None, C.byref(n)) == _lib.NC_EINVAL
    assert L.nc_session_query(None, 4, C.byref(n)) == _lib.NC_EINVAL
    assert L.nc_session_push(None, None, 4, None, None, 0, C.byref(n)) == _lib.NC_EINVAL
    assert L.nc_session_flush_dev(None, None, 0, C.byref(n)) == _lib.NC_EINVAL
    assert L.nc_session_destroy(None) == _lib.NC_OK
