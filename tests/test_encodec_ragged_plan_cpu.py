"""CPU suite: nc_encodec_ragged_rows -- how the Encodec ragged calls pool the segments of clips of unequal lengths into uniform batches.

A host function on a config alone, no device.  The reduced 48 kHz-style fixture (segment 4000, stride 3960, hop 48), the reduced
24 kHz-style one (no segmentation) and the 48 kHz preset, both directions."""
import numpy as np
import pytest

from conftest import encodec_cfg_from_meta, load_golden
from neuralcodecs_amd import EncodecConfig, encodec_ragged_rows

CFGS = {
    "encodec_small48": lambda: encodec_cfg_from_meta(load_golden("encodec_small48")["meta"]),
    "encodec_small24": lambda: encodec_cfg_from_meta(load_golden("encodec_small24")["meta"]),
    "encodec_48khz": EncodecConfig.encodec_48khz,
}
SMALL48 = [8100, 4000, 3990, 100, 9000, 8100, 47, 3960, 4140, 12000, 5000, 48]


def _segments(cfg, T):
    """Encodec.cs:278-282: (offset, length) of every segment of a T-sample clip"""
    if cfg.segment_seconds is None:
        return [(0, T)]
    seg = int(cfg.segment_seconds * cfg.sampling_rate)
    stride = max(1, int((1 - cfg.overlap) * seg))
    return [(off, min(off + seg, T) - off) for off in range(0, T, stride)]


def _lengths(cfg, seed):
    if cfg.segment_seconds is None:
        return [3001, 3001, 1000, 48, 2999, 1000]
    seg = int(cfg.segment_seconds * cfg.sampling_rate)
    stride = max(1, int((1 - cfg.overlap) * seg))
    rng = np.random.default_rng(seed)
    fixed = [seg, stride, 2 * stride, 2 * stride + 180, stride + 180, seg // 40, 3 * seg]
    return fixed + [int(rng.integers(1, 4 * seg)) for _ in range(5)]


@pytest.mark.parametrize("decode", [False, True])
@pytest.mark.parametrize("max_rows", [2, 3, 0])
@pytest.mark.parametrize("name", sorted(CFGS))
def test_row_layout(name, max_rows, decode):
    cfg = CFGS[name]()
    lengths = SMALL48 if name == "encodec_small48" else _lengths(cfg, seed=max_rows)
    plan, rows = encodec_ragged_rows(cfg, lengths, decode, max_rows)
    cap = plan["max_rows"]
    assert cap == max_rows or (max_rows == 0 and 0 < cap <= 4096)
    want = {(b, s): seg for b, T in enumerate(lengths) for s, seg in enumerate(_segments(cfg, T))}
    got = {(r["clip"], r["segment"]): r for r in rows}
    assert len(rows) == len(got) == plan["n_rows"] and set(got) == set(want)          # every (clip, segment) exactly once
    hop = cfg.hop_length
    for k, r in got.items():
        off, ln = want[k]
        assert r["offset"] == off
        if not decode:
            assert r["length"] == ln
        if ln >= 10 * hop:                                                               # away from the small-input path: one frame per hop
            assert r["frames"] == -(-ln // hop)
            if decode:
                assert r["length"] == r["frames"] * hop
    key = (lambda r: r["frames"]) if decode else (lambda r: r["length"])
    batches = {}
    for r in rows:
        batches.setdefault(r["batch"], []).append(r)
    assert sorted(batches) == list(range(plan["n_batches"]))
    for bi, rs in batches.items():
        assert len(rs) <= cap                                                            # no batch exceeds max_rows
        assert len({key(r) for r in rs}) == 1                                            # all rows of a batch share the key
        assert len({r["frames"] for r in rs}) == 1 and len({r["length"] for r in rs}) == 1
        assert sorted(r["row"] for r in rs) == list(range(len(rs)))
    counts = {}
    for r in rows:
        counts[key(r)] = counts.get(key(r), 0) + 1
    assert plan["n_keys"] == len(counts)
    assert plan["n_batches"] == sum(-(-n // cap) for n in counts.values())
    # totals: the sums of the per-clip figures, through the planner's own per-row frames
    assert plan["total_code_frames"] == sum(r["frames"] for r in rows)
    assert plan["total_scales"] == len(rows)
    nq = max(1, int(cfg.bandwidth * 1000 // (np.log2(cfg.codebook_size) * int(np.ceil(cfg.sampling_rate / hop)))))
    assert plan["total_codes"] == nq * plan["total_code_frames"]
    if decode:
        per_clip = {}
        for r in rows:
            per_clip.setdefault(r["clip"], []).append(r)
        total = 0
        for b, rs in per_clip.items():
            last = max(rs, key=lambda r: r["segment"])
            total += last["offset"] + last["length"]                                     # (n - 1) * stride + decoded(last frame)
        assert plan["total_samples"] == total


def test_shared_tails_and_uniform_grouping():
    cfg = CFGS["encodec_small48"]()
    plan, rows = encodec_ragged_rows(cfg, [8100, 4140], False, 0)
    tails = [r for r in rows if r["length"] == 180]
    assert [(r["clip"], r["segment"]) for r in tails] == [(1, 1), (0, 2)] and len({r["batch"] for r in tails}) == 1   # segment-major
    assert plan["n_keys"] == 2 and plan["n_batches"] == 2
    # equal lengths: the uniform call's grouping -- the full segments of all clips one batch, segment-major, the tails the other
    plan, rows = encodec_ragged_rows(cfg, [8100] * 3, False, 0)
    assert plan["n_batches"] == 2
    assert [(r["batch"], r["row"], r["segment"], r["clip"]) for r in rows] == \
        [(0, 3 * s + b, s, b) for s in range(2) for b in range(3)] + [(1, b, 2, b) for b in range(3)]
    for decode in (False, True):
        _, a = encodec_ragged_rows(cfg, [9000, 9000], decode, 0)
        assert [r["batch"] for r in a] == sorted(r["batch"] for r in a)                  # launch order, keys descending
        keys = [r["frames"] if decode else r["length"] for r in a]
        assert keys == sorted(keys, reverse=True)


def test_unsegmented_models_pool_only_equal_lengths():
    cfg = CFGS["encodec_small24"]()
    lengths = [3001, 3001, 1000, 48, 2999, 1000]
    plan, rows = encodec_ragged_rows(cfg, lengths, False, 0)
    assert plan["n_rows"] == 6 and plan["n_keys"] == 4 and plan["n_batches"] == 4
    by_batch = {}
    for r in rows:
        assert r["segment"] == 0 and r["offset"] == 0 and r["length"] == lengths[r["clip"]]
        by_batch.setdefault(r["batch"], []).append(r["clip"])
    assert sorted(by_batch.values()) == [[0, 1], [2, 5], [3], [4]]
    plan, _ = encodec_ragged_rows(cfg, [1000] * 5, False, 2)
    assert plan["n_keys"] == 1 and plan["n_batches"] == 3


def test_refusals():
    cfg = CFGS["encodec_small48"]()
    for bad in ([], [0], [100, 0], [100, -5]):
        with pytest.raises(ValueError):
            encodec_ragged_rows(cfg, bad)
    with pytest.raises(ValueError):
        encodec_ragged_rows(cfg, [100], max_rows=-1)
    with pytest.raises(ValueError):
        encodec_ragged_rows(cfg, [100], max_rows=4097)
    plan, _ = encodec_ragged_rows(cfg, [100], max_rows=4096)
    assert plan["max_rows"] == 4096
