"""GPU suite: the launch sequence of Encodec held to a recorded fixture.

tests/test_encodec_gpu.py holds the RESULTS of the engine to the oracle bit for bit and tests/test_conv_plan_gpu.py the decisions of
launch_conv; neither sees a launch of the SEANet driver, the LSTM or the quantizer that was added, dropped or moved to another class.
The handle's profiler does: per kernel class (NC_KC_*) it counts the profiled launches of a call and adds up the flops and bytes the
host computes for them from the shapes alone.  This test reads that table for one encode and one decode per case, in the default
environment, and compares it with tests/golden/encodec_launches.json: launch counts equal, flops and bytes equal to 1e-12 relative
(they are host arithmetic on shapes).

The fixture was recorded at commit 82419e0, with the engine as it stood before nc_encodec.hip was split into the LSTM, Euclidean-RVQ and model units, so
a figure that differs is a change of behaviour: it is fixed in the engine, never in the fixture.  The test never writes;
`python tests/test_encodec_launches_gpu.py <file.json>` is the recorder (the same reader, its table written to <file.json>).
"""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

from conftest import encodec_cfg_from_meta, load_golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "encodec_launches.json")
REL_TOL = 1e-12


# case -> (golden that fixes config and weights, clip): None = the golden's own pcm array, (B, T, seed) = synthetic_pcm(B, channels, T,
# rate, seed) with T / seed None = the golden's meta["T"] / meta["pcm_seed"]
CASES = {
    "encodec_small48": ("encodec_small48", None),
    "encodec_small24": ("encodec_small24", None),
    # segments of 4000 samples at stride 3960: two equal segments (one batched group on the handle's stream) and a 1080-sample tail
    # (a group of its own on a side stream)
    "encodec_small48 T=9000": ("encodec_small48", (1, 9000, 9000)),
    # full width, two clips, one 1 s segment of 75 frames: the two LSTM layers run as the layer-pipelined persistent form.  The golden
    # holds ONE clip, so its own array is not used: the two clips are synthesised from its T and pcm_seed, as tests/test_encodec_gpu.py does
    "encodec24k_b1 B=2": ("encodec24k_b1", (2, None, None)),
}


def _table(m, fn):
    """The profiler exactly as _launches of tests/test_chunked_gpu.py uses it, keeping the whole per-class table."""
    m.profile_enable(True)
    m.profile_reset()
    out = fn()
    tab = {k: {f: v[f] for f in ("launches", "flops", "bytes")} for k, v in m.profile_read().items()}
    m.profile_enable(False)
    return out, tab


def read_case(case):
    from neuralcodecs_amd import Encodec
    from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob, synthetic_pcm
    name, clip = CASES[case]
    g = load_golden(name)
    cfg = encodec_cfg_from_meta(g["meta"])
    if clip is None:
        pcm = g["pcm"]
    else:
        B, T, seed = clip
        pcm = synthetic_pcm(B, cfg.channels, T or g["meta"]["T"], cfg.sampling_rate, seed=g["meta"]["pcm_seed"] if seed is None else seed)
    with Encodec(cfg) as m:
        m.load_blob(save_blob(encodec_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"])))
        frames, enc = _table(m, lambda: m.encode(pcm))
        _, dec = _table(m, lambda: m.decode(frames, pcm.shape[-1]))
    return {"encode": enc, "decode": dec}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_the_cases(recorded):
    assert set(recorded) == set(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_encodec_launch_table_matches_the_recorded_parent(case, recorded):
    got, want = read_case(case), recorded[case]
    print("\nENCODEC_LAUNCHES " + json.dumps({case: got}))
    for call in ("encode", "decode"):
        assert set(got[call]) == set(want[call]), (case, call, "the kernel classes differ")
        assert sum(v["launches"] for v in want[call].values()) > 0, (case, call, "the fixture recorded no launch")
        for kc, w in want[call].items():
            h = got[call][kc]
            assert h["launches"] == w["launches"], (case, call, kc, "launches", h["launches"], w["launches"])
            for f in ("flops", "bytes"):
                assert abs(h[f] - w[f]) <= REL_TOL * max(abs(h[f]), abs(w[f])), (case, call, kc, f, h[f], w[f])


if __name__ == "__main__":
    with open(sys.argv[1], "w") as out:
        json.dump({case: read_case(case) for case in CASES}, out, indent=1, sort_keys=True)
        out.write("\n")
