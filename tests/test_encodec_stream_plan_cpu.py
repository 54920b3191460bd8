"""CPU suite: nc_encodec_stream_plan -- which rows a step of an Encodec stream pool runs, and what every entry emits.

A host function on a config alone, no device.  Driven here as a stream pool drives it: every stream keeps (pushed, emitted), a step
brings n_in / flush per stream, and the rows of all steps of a stream, put together, must be the rows nc_encodec_ragged_rows gives for
the whole clip -- each once, in segment order -- with the emitted counts adding up to the whole clip's (the sums of nc_encodec_query, which
the ragged planner reports from the config alone)."""
import ctypes as C

import pytest

from conftest import encodec_cfg_from_meta, load_golden
from neuralcodecs_amd import EncodecConfig, _lib, encodec_ragged_rows, encodec_stream_plan
from neuralcodecs_amd.encodec import _c_config

SEG, STRIDE, HOP = 4000, 3960, 48
LENGTHS = [47, 100, 4000, 3960, 4140, 7950, 12000, 3990, 8100, 9000]
# sizes of the successive pushes (cycled until the clip is through); the last entry of a pattern decides how the stream ends:
# True = the flush carries the last push, False = the flush comes alone
PATTERNS = {
    "small pushes that complete nothing for a long time": ([700], False),
    "exactly a segment, then exactly a stride": ([SEG, STRIDE], False),
    "one push completes two or more segments": ([2 * STRIDE + SEG + 5], True),
    "single samples across the segment end": ([SEG - 2, 1, 1, 1, 1, STRIDE - 6, 1, 1, 1, 1, 1, 1, 5000], False),
    "everything in the flush": ([1 << 20], True),
    "odd sizes": ([1234, 1, 4321, 17], True),
}


def _cfg():
    return encodec_cfg_from_meta(load_golden("encodec_small48")["meta"])


def _pushes(T, sizes):
    out, i = [], 0
    while T > 0:
        n = min(T, sizes[i % len(sizes)])
        out.append(n)
        T -= n
        i += 1
    return out


def _whole(cfg, T, decode):
    plan, rows = encodec_ragged_rows(cfg, [T], decode)
    return plan, sorted(((r["segment"], r["offset"], r["length"], r["frames"]) for r in rows))


def _drive(cfg, streams, decode, max_rows=0):
    """streams: per stream the list of steps (n_in, flush, frame_lens or None); None = idle in that step.  -> per stream the rows and the
    emitted sums, per step the plan and the rows."""
    n = len(streams)
    pushed, emitted = [0] * n, [0] * n
    got = [[] for _ in range(n)]
    sums = [dict(n_frames=0, code_frames=0, n_samples=0) for _ in range(n)]
    steps = []
    for t in range(max(len(s) for s in streams)):
        who = [i for i in range(n) if t < len(streams[i]) and streams[i][t] is not None]
        if not who:
            continue
        ent = [streams[i][t] for i in who]
        lens = [f for e in ent for f in (e[2] or [])] if decode else None
        plan, rows, per = encodec_stream_plan(cfg, [pushed[i] for i in who], [emitted[i] for i in who], [e[0] for e in ent], [e[1] for e in ent],
                                              lens, decode, max_rows)
        steps.append((plan, rows, who))
        assert plan["n_rows"] == len(rows) == sum(p["n_frames"] for p in per)
        for j, i in enumerate(who):
            mine = [r for r in rows if r["clip"] == j]
            assert len(mine) == per[j]["n_frames"] and sum(r["frames"] for r in mine) == per[j]["code_frames"]
            got[i] += sorted((r["segment"], r["offset"], r["length"], r["frames"]) for r in mine)
            for k in sums[i]:
                sums[i][k] += per[j][k]
            pushed[i] += ent[j][0]
            if decode:
                emitted[i] += per[j]["n_samples"]
            elif not ent[j][1]:
                emitted[i] += per[j]["n_frames"]
                assert per[j]["n_samples"] == pushed[i] - emitted[i] * STRIDE < SEG      # what the slot keeps
    return got, sums, steps


def _encode_steps(T, sizes, with_last):
    ps = _pushes(T, sizes)
    if with_last:
        return [(p, False, None) for p in ps[:-1]] + [(ps[-1], True, None)]
    return [(p, False, None) for p in ps] + [(0, True, None)]


def _decode_steps(frames, chunk, with_last):
    """the clip's frames in pushes of `chunk`; the last two (the ones that may be short) come with the flush, or -- where they are as long as
    a full frame -- may come before it"""
    full, tail = frames[:-2], frames[-2:]
    steps = [(len(full[i:i + chunk]), False, full[i:i + chunk]) for i in range(0, len(full), chunk)]
    if with_last:
        return steps + [(len(tail), True, tail)]
    F = -(-SEG // HOP)
    early = [f for f in tail[:-1] if f == F]                                           # a full-length frame needs no flush to be pushed
    rest = tail[len(early):]
    return steps + [(len(early), False, early)] * bool(early) + [(len(rest), True, rest)]


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_encode_rows_of_all_steps_are_the_whole_clips_rows(pattern):
    cfg = _cfg()
    sizes, with_last = PATTERNS[pattern]
    streams = [_encode_steps(T, sizes, with_last) for T in LENGTHS]
    got, sums, _ = _drive(cfg, streams, False)
    for T, rows, s in zip(LENGTHS, got, sums):
        plan, want = _whole(cfg, T, False)
        assert rows == want, f"T = {T}"                                                  # each row once, in segment order
        assert s["n_frames"] == plan["n_rows"] and s["code_frames"] == plan["total_code_frames"]


@pytest.mark.parametrize("chunk,with_last", [(1, True), (2, False), (5, True)])
def test_decode_rows_of_all_steps_are_the_whole_clips_rows(chunk, with_last):
    cfg = _cfg()
    streams, wants = [], []
    for T in LENGTHS:
        plan, want = _whole(cfg, T, True)
        wants.append((plan, want))
        streams.append(_decode_steps([w[3] for w in want], chunk, with_last))
    got, sums, _ = _drive(cfg, streams, True)
    for T, rows, s, (plan, want) in zip(LENGTHS, got, sums, wants):
        assert rows == want, f"T = {T}"
        assert s["n_frames"] == plan["n_rows"] and s["code_frames"] == plan["total_code_frames"]
        assert s["n_samples"] == plan["total_samples"], f"T = {T}"                       # the decoded length of the whole clip


def test_decode_emits_a_stride_per_full_frame():
    cfg = _cfg()
    F = -(-SEG // HOP)
    plan, rows, per = encodec_stream_plan(cfg, [0, 3], [0, 3 * STRIDE], [2, 1], [False, False], None, decode=True)
    assert [p["n_samples"] for p in per] == [2 * STRIDE, STRIDE] and [p["code_frames"] for p in per] == [2 * F, F]
    assert sorted((r["clip"], r["segment"], r["offset"]) for r in rows) == [(0, 0, 0), (0, 1, STRIDE), (1, 3, 3 * STRIDE)]
    assert all(r["frames"] == F and r["length"] == F * HOP for r in rows) and plan["n_batches"] == 1


@pytest.mark.parametrize("max_rows", [2, 0])
def test_rows_of_one_key_share_batches_of_at_most_max_rows(max_rows):
    cfg = _cfg()
    # five streams in lock step complete a segment each; two more flush 180-sample tails; one is idle (pushes too little)
    pushed = [0, STRIDE + 40, 100, 3000, 2 * STRIDE + 40, STRIDE + 100, STRIDE + 50, 10]
    emitted = [0, 1, 0, 0, 2, 1, 1, 0]
    n_in = [SEG, STRIDE, SEG - 100, 1000, STRIDE, 80, 130, 5]
    flush = [0, 0, 0, 0, 0, 1, 1, 0]
    plan, rows, per = encodec_stream_plan(cfg, pushed, emitted, n_in, flush, None, False, max_rows)
    assert [p["n_frames"] for p in per] == [1, 1, 1, 1, 1, 1, 1, 0]
    by_batch = {}
    for r in rows:
        by_batch.setdefault(r["batch"], []).append(r)
    keys = [b[0]["length"] for _, b in sorted(by_batch.items())]
    assert keys == sorted(keys, reverse=True)                                             # keys in descending order
    for b in by_batch.values():
        assert len({r["length"] for r in b}) == 1 and sorted(r["row"] for r in b) == list(range(len(b)))
    full = sorted(len(b) for b in by_batch.values() if b[0]["length"] == SEG)
    tails = sorted(len(b) for b in by_batch.values() if b[0]["length"] == 180)
    if max_rows == 2:
        assert full == [1, 2, 2] and tails == [2]
    else:
        assert full == [5] and tails == [2] and plan["n_batches"] == 2                    # a lock-step step is ONE launch sequence
    assert plan["max_rows"] == (max_rows or plan["max_rows"]) and plan["n_keys"] == 2


def test_refusals_return_a_status():
    cfg = _cfg()
    F = -(-SEG // HOP)
    with pytest.raises(ValueError, match="negative"):
        encodec_stream_plan(cfg, [0], [0], [-1])
    with pytest.raises(ValueError, match="received nothing"):
        encodec_stream_plan(cfg, [0], [0], [0], [True])
    with pytest.raises(ValueError, match="has emitted"):
        encodec_stream_plan(cfg, [SEG], [0], [10])                                        # a stream at 4000 samples has emitted one segment
    with pytest.raises(ValueError, match="has emitted"):
        encodec_stream_plan(cfg, [2], [STRIDE], [1], decode=True)
    with pytest.raises(ValueError, match="max_rows"):
        encodec_stream_plan(cfg, [0], [0], [10], max_rows=5000)
    with pytest.raises(ValueError, match="full segment"):
        encodec_stream_plan(cfg, [0], [0], [1], [False], [F - 1], decode=True)            # a push that is not a full frame
    with pytest.raises(ValueError, match="full segment"):
        encodec_stream_plan(cfg, [0], [0], [3], [True], [F - 1, F, 1], decode=True)       # only the last two may be short
    with pytest.raises(ValueError, match="no clip length"):
        encodec_stream_plan(cfg, [1], [STRIDE], [1], [True], [F + 1], decode=True)        # tail frames that no clip produces
    with pytest.raises(ValueError, match="no clip length"):
        encodec_stream_plan(cfg, [1], [STRIDE], [2], [True], [1, 1], decode=True)         # (a 1-frame segment is never followed by another)
    # the 24 kHz preset is not segmented: there is nothing to stream
    with pytest.raises(_lib.NcError, match="not segmented"):
        encodec_stream_plan(EncodecConfig.encodec_24khz(), [0], [0], [1000])
    # null pointers and n <= 0 through the bare export
    L, c, one, p = _lib.lib(), _c_config(cfg), _lib.i64_array([0]), _lib.NcEncodecRaggedPlan()
    assert L.nc_encodec_stream_plan(None, 0, 1, one, one, one, None, None, 0, C.byref(p), None, 0, None, None, None) == _lib.NC_EINVAL
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert L.nc_encodec_stream_plan(C.byref(c), 0, 1, *args, None, None, 0, C.byref(p), None, 0, None, None, None) == _lib.NC_EINVAL
    assert L.nc_encodec_stream_plan(C.byref(c), 0, 0, one, one, one, None, None, 0, C.byref(p), None, 0, None, None, None) == _lib.NC_EINVAL
    # every output is optional
    assert L.nc_encodec_stream_plan(C.byref(c), 0, 1, one, one, _lib.i64_array([SEG]), None, None, 0, None, None, 0, None, None, None) == _lib.NC_OK


def test_full_size_preset_one_second_per_step():
    cfg = EncodecConfig.encodec_48khz()
    seg, stride = 48000, 47520
    pushed = emitted = 0
    total = []
    for step in range(4):
        plan, rows, per = encodec_stream_plan(cfg, [pushed], [emitted], [48000])
        total += [(r["segment"], r["offset"], r["length"]) for r in rows]
        pushed += 48000
        emitted += per[0]["n_frames"]
    assert total == [(k, k * stride, seg) for k in range(4)] and emitted == 4             # 4 s hold 4 complete segments (4 * stride + seg > 192000)
    plan, rows, per = encodec_stream_plan(cfg, [pushed], [emitted], [0], [True])
    assert [(r["segment"], r["offset"], r["length"]) for r in rows] == [(4, 4 * stride, 192000 - 4 * stride)]
