"""Child process of tests/test_lds_token_paths.py: drives the library named by DEXSIM_LIB_PATH (the -DDEXSIM_DEBUG_SPIN twin, whose
token waits are bounded) through the cases of tests/lds_token_cases.py named on the command line, free-running for STEPS control
steps each, and prints one JSON line: per case the spin-timeout word of the counters block and a digest of the end state.  The
test computes the same digest in its own process on the product build (run_case)."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import lds_token_cases as lc  # noqa: E402
from tests import physics_rig as pr  # noqa: E402

CNT_SPIN_TIMEOUT = 20     # csrc/dexsim_device.h
DIGEST_FIELDS = ("q", "qd", "box_pos", "box_quat", "box_lin", "box_ang", "cforce", "ncontact", "wgen")


def run_case(case):
    """{"spin_word", "digest"} of a case on the library this process has loaded."""
    import torch
    n, start = lc.state(case)
    sc, _, ms = pr.setup("BlindGrasping", n)
    b = pr.hip(sc, ms)
    pr.load(b, start)
    for _ in range(lc.STEPS):
        b.physics_step()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for f in DIGEST_FIELDS:
        h.update(b.core.field(f).cpu().numpy().tobytes())
    return {"spin_word": int(b.core.counters[CNT_SPIN_TIMEOUT].item()), "digest": h.hexdigest()}


if __name__ == "__main__":
    print(json.dumps({case: run_case(case) for case in sys.argv[1:]}))
