"""CPU suite: the grouping rule of the session pool (nc_session_pool_plan) -- a host function, no device.

For the halos of every shipped DAC and SNAC preset (and of the small test configs), both directions, and random staggered push scripts:
the step the planner gives every stream is the step nc_session_schedule gives that stream run on its own; the entries of one group share
a window width; no group has more than max_rows rows; an entry without a window has group -1."""
import ctypes as C
import random
import zlib

import pytest

from conftest import dac_cfg_from_meta, load_golden, snac_cfg_from_meta
from neuralcodecs_amd import DACConfig, SNACConfig, _lib, dac_halo, session_pool_plan, session_schedule, snac_halo


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


def _script(rng, h, decode, n_streams, n_ticks):
    """per stream: the tick it joins at and its pushes (frames; 0 = the flush, after which the stream starts over)"""
    a = h["align"]
    hl, hr = (h["dec_right"], h["dec_left"]) if decode else (h["enc_right"], h["enc_left"])
    sizes = [a, a, 2 * a, 4 * a, hl + hr + 2 * a]          # few distinct sizes, so that equal widths do meet
    streams = []
    for k in range(n_streams):
        pushes = []
        for _ in range(n_ticks):
            r = rng.random()
            pushes.append(0 if (r < 0.1 and pushes and pushes[-1] != 0) else (None if r < 0.2 else rng.choice(sizes)))
        streams.append((k % 4, pushes))
    return streams


@pytest.mark.parametrize("decode", [True, False])
@pytest.mark.parametrize("name,h", HALOS, ids=[n for n, _ in HALOS])
def test_plan_is_the_schedule_stream_by_stream_and_groups_share_a_width(name, h, decode):
    rng = random.Random(zlib.crc32(f"{name}:{decode}".encode()))
    n_streams, n_ticks, max_rows = 9, 14, 3
    streams = _script(rng, h, decode, n_streams, n_ticks)
    P, E, hist = [0] * n_streams, [0] * n_streams, [[] for _ in range(n_streams)]      # hist: the pushes of the stream's running clip
    seen_windows = seen_none = 0
    for t in range(n_ticks):
        who, push = [], []
        for k, (join, pushes) in enumerate(streams):
            f = pushes[t] if t >= join else None
            if f is None or (f == 0 and P[k] == 0):
                continue
            who.append(k)
            push.append(f)
        if not who:
            continue
        steps, group_of, n_groups = session_pool_plan(h, [P[k] for k in who], [E[k] for k in who], push, decode=decode, max_rows=max_rows)
        members = {}
        for i, k in enumerate(who):
            # the same stream on its own: nc_session_schedule over its whole clip so far; the last step is this one
            alone = session_schedule(h, hist[k] + ([push[i]] if push[i] else []), decode=decode, flush=push[i] == 0)[-1]
            assert steps[i] == alone, (name, t, k, steps[i], alone)
            if steps[i]["k1"] > steps[i]["k0"]:
                assert 0 <= group_of[i] < n_groups
                members.setdefault(group_of[i], []).append(steps[i]["w1"] - steps[i]["w0"])
            else:
                assert group_of[i] == -1
                seen_none += 1
        assert sorted(members) == list(range(n_groups))
        widths = [members[g][0] for g in range(n_groups)]
        for g, ws in members.items():
            assert len(set(ws)) == 1 and len(ws) <= max_rows, (name, t, g, ws)
        assert widths == sorted(widths)                                             # narrowest first
        for w in set(widths):                                                       # a width is split only where it overflows
            n_rows = sum(len(members[g]) for g in range(n_groups) if widths[g] == w)
            assert widths.count(w) == -(-n_rows // max_rows)
        seen_windows += len(members)
        for i, k in enumerate(who):
            if push[i] == 0:
                P[k], E[k], hist[k] = 0, 0, []
            else:
                P[k] += push[i]
                E[k] = steps[i]["k1"]
                hist[k].append(push[i])
    assert seen_windows > 0 and seen_none > 0


@pytest.mark.parametrize("name,h", HALOS, ids=[n for n, _ in HALOS])
def test_a_group_of_more_than_max_rows_streams_is_split(name, h):
    for decode in (True, False):
        a = h["align"]
        hl, hr = (h["dec_right"], h["dec_left"]) if decode else (h["enc_right"], h["enc_left"])
        P = hl + hr + 4 * a                                                         # seven streams in the same steady state, one idle
        E = (P - hr) // a * a
        steps, group_of, n_groups = session_pool_plan(h, [P] * 7 + [0], [E] * 7 + [0], [2 * a] * 8, decode=decode, max_rows=3)
        assert all(st["w1"] - st["w0"] == hl + 2 * a + hr + (P - hr - E) for st in steps[:7])
        assert group_of[:7] == [0, 0, 0, 1, 1, 1, 2] and n_groups == 3
        assert (group_of[7] == -1) == (steps[7]["k1"] == 0) and group_of[7] not in (0, 1, 2)   # the newcomer's window, if any, is narrower
        assert session_pool_plan(h, [P] * 7, [E] * 7, [2 * a] * 7, decode=decode)[2] == 1   # the default holds them all


def test_flush_and_push_windows_of_equal_width_share_a_group():
    h = {"enc_left": 4, "enc_right": 4, "dec_left": 4, "dec_right": 4, "align": 2}
    # stream 0: 12 pushed, 8 emitted, pushes 2 -> window [4, 14); stream 1: 14 pushed, 8 emitted, flushes -> window [4, 14)
    steps, group_of, n_groups = session_pool_plan(h, [12, 14, 2], [8, 8, 0], [2, 0, 2])
    assert (steps[0]["w0"], steps[0]["w1"], steps[0]["k1"]) == (4, 14, 10) and (steps[1]["w0"], steps[1]["w1"], steps[1]["k1"]) == (4, 14, 14)
    assert group_of == [0, 0, -1] and n_groups == 1
    assert steps[2]["w0"] == steps[2]["w1"] and steps[2]["resident"] == 4


def test_refusals_do_not_crash():
    L = _lib.lib()
    h = _lib.NcHalo(enc_left=4, enc_right=4, dec_left=4, dec_right=4, align=4)
    steps = (_lib.NcSessionStep * 2)()
    grp = (C.c_int32 * 2)()
    ng = C.c_int32()
    P, E, F = _lib.i64_array([8, 0]), _lib.i64_array([4, 0]), _lib.i64_array([4, 4])
    ok = lambda *a: L.nc_session_pool_plan(*a)  # noqa: E731
    assert ok(C.byref(h), 1, 2, P, E, F, 0, steps, grp, C.byref(ng)) == _lib.NC_OK
    for args in ((None, 1, 2, P, E, F, 0, steps, grp, C.byref(ng)), (C.byref(h), 1, 2, None, E, F, 0, steps, grp, C.byref(ng)),
                 (C.byref(h), 1, 2, P, None, F, 0, steps, grp, C.byref(ng)), (C.byref(h), 1, 2, P, E, None, 0, steps, grp, C.byref(ng)),
                 (C.byref(h), 1, 2, P, E, F, 0, None, grp, C.byref(ng)), (C.byref(h), 1, 2, P, E, F, 0, steps, None, C.byref(ng)),
                 (C.byref(h), 1, 2, P, E, F, 0, steps, grp, None), (C.byref(h), 1, 0, P, E, F, 0, steps, grp, C.byref(ng)),
                 (C.byref(h), 1, -1, P, E, F, 0, steps, grp, C.byref(ng)), (C.byref(h), 1, 2, P, E, F, -1, steps, grp, C.byref(ng))):
        assert ok(*args) == _lib.NC_EINVAL, args
    bad = _lib.NcHalo(enc_left=4, enc_right=4, dec_left=4, dec_right=4, align=0)
    assert ok(C.byref(bad), 1, 2, P, E, F, 0, steps, grp, C.byref(ng)) == _lib.NC_EINVAL
    for p, e, f in (([6, 0], [4, 0], [4, 4]),        # pushed not a multiple of align
                    ([8, 0], [12, 0], [4, 4]),       # more emitted than pushed
                    ([8, 0], [4, 0], [4, 6]),        # a misaligned push
                    ([8, 0], [4, 0], [4, 0]),        # a flush of nothing
                    ([8, 0], [4, 0], [-4, 4]), ([-8, 0], [4, 0], [4, 4])):
        assert ok(C.byref(h), 1, 2, _lib.i64_array(p), _lib.i64_array(e), _lib.i64_array(f), 0, steps, grp, C.byref(ng)) == _lib.NC_EINVAL, (p, e, f)
    # the pool entry points on null handles
    out = C.c_void_p()
    n = C.c_int64()
    slots = (C.c_int32 * 1)(0)
    nin = _lib.i64_array([4])
    assert L.nc_session_pool_create(None, 1, 4, 0, C.byref(out)) == _lib.NC_EINVAL and not out.value
    assert L.nc_session_pool_create(None, 1, 4, 0, None) == _lib.NC_EINVAL
    assert L.nc_session_pool_reset_slot(None, 0) == _lib.NC_EINVAL and L.nc_session_pool_set_seed(None, 0, 1) == _lib.NC_EINVAL
    assert L.nc_session_pool_pending(None, 0, C.byref(n)) == _lib.NC_EINVAL
    assert L.nc_session_pool_query(None, 1, slots, nin, C.byref(n)) == _lib.NC_EINVAL
    assert L.nc_session_pool_step(None, 1, slots, nin, None, None, None, 0, C.byref(n)) == _lib.NC_EINVAL
    assert L.nc_session_pool_step_dev(None, 1, slots, nin, None, None, None, 0, C.byref(n)) == _lib.NC_EINVAL
    assert L.nc_session_pool_destroy(None) == _lib.NC_OK
