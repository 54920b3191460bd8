"""Child process of tests/test_encodec_causal_gpu.py (a fresh interpreter, the tests/_gpu_child.py pattern): the encode and decode session
tests under the diagnostic switches the parent put into the environment (they are read once per process).

    python tests/_encodec_causal_child.py seq|step      with NC_LAUNCH_LOG set

seq: the one-clip reference must have taken the persistent LSTM form; step: the step-wise form (NC_LSTM_STEPWISE=1).  Prints CHILD_OK."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")
os.environ.setdefault("GOMP_SPINCOUNT", "0")


def main():
    form = sys.argv[1]
    assert form in ("seq", "step") and os.environ.get("NC_LAUNCH_LOG")
    import test_encodec_causal_gpu as t
    t.reference()                                         # the one-clip calls of THIS process, held to the C oracle
    lines = [ln for ln in open(os.environ["NC_LAUNCH_LOG"]).read().splitlines() if ln.startswith("lstm ")]
    other = "step" if form == "seq" else "seq"
    assert any(ln.startswith(f"lstm {form} C=64 ") and " layers=2 " in ln for ln in lines), lines[:8]
    assert not any(ln.startswith(f"lstm {other}") or ln.startswith("lstm carried") for ln in lines), lines[:8]
    t.test_encode_session_equals_the_one_clip_call()
    t.test_decode_session_equals_the_one_clip_call()
    after = [ln for ln in open(os.environ["NC_LAUNCH_LOG"]).read().splitlines() if ln.startswith("lstm ")][len(lines):]
    assert after and all(ln.startswith("lstm carried C=64 layers=2") for ln in after), after[:8]
    print("CHILD_OK")


if __name__ == "__main__":
    main()
