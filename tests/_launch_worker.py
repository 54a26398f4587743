"""Child of tests/test_launch_coverage.py for cases that need an environment knob the library reads once per
process.  The launch ledger is per process too, so the child arms its own, prints it, and the parent unions it.

    python tests/_launch_worker.py N OUT.npz     (parent sets FHESPEAR_ENCODE_UNFUSED=1)

Encodes _launch_matrix.encode_rows(N) -- with the knob set, through k_encode's reduction into every limb and the
in-place k_ntt_fwd_ptrs -- checks every plaintext against the extended-precision reference, saves the limbs as
pt0, pt1, ... for the parent to compare with the fused encoder's, and prints "LEDGER <json list of names>"."""
import json
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent / "fhe-spear_amd" / "python"), str(HERE)]
os.environ.setdefault("FHESPEAR_PARITY_RNG", "1")


def main():
    N, out = int(sys.argv[1]), sys.argv[2]
    assert os.environ.get("FHESPEAR_ENCODE_UNFUSED"), "the parent sets FHESPEAR_ENCODE_UNFUSED"
    import pyPhantom as ph
    from oracle import oracle as orc
    import _launch_matrix as lm
    orc.build()
    ph.debug_launch_ledger("arm")
    try:
        r = lm._Ring(ph, orc, N, [59] * 4, seed=lm.SEED)
        limbs = lm.encode_and_check(r)
    finally:
        ph.debug_launch_ledger("disarm")
    np.savez(out, **{f"pt{k}": a for k, a in enumerate(limbs)})
    print("LEDGER " + json.dumps(ph.debug_launch_ledger("read")), flush=True)


if __name__ == "__main__":
    main()
