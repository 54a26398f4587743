"""bench.py's legs on the GPU at test size: the measured RWKV-block leg with its CPU limb check
(VERDICT r2 next #1), so the code path the driver's bench line takes is covered by the suite."""
import argparse
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


@pytest.mark.gpu
def test_block_leg_with_cpu_limb_check(require_gpu):
    """bench.run_block on a small block (N=4096, L0=6, D=64, F=256): timing fields, the decrypted output
    against the plaintext block, and the r projection's server call recorded in the block and
    recomputed by the CPU port (cpu_check_block_projection) -- limb for limb."""
    import bench
    import pyPhantom as ph
    args = argparse.Namespace(split=False, block_dealt=False, config="cfg2")
    res = bench.run_block(args, ph, None, 0, 1, 0, 1, 1, capture=True, config="block_small")
    cap = res.pop("_capture")
    assert res["sec_per_block"] > 0 and set(res["stages_ms"]) == {"server_rkv", "server_wo", "server_ffn_key",
                                                                   "server_ffn_val", "client_encrypt",
                                                                   "client_decrypt", "client_numpy"}
    assert res["client_ms"] > 0 and res["server_ms"] > 0
    assert cap["ct_in"].shape == (2, 6, 4096) and cap["ct_out"].shape == (2, 5, 4096) and len(cap["pts"]) == 64
    par = bench.cpu_check_block_projection(cap)
    assert par["r_projection_limbs_match_cpu_port"], par


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_oracle_limbs(require_gpu, tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` without --full at the smoke size (N=4096, L0=6, D=256):
    K timed steps, ms_per_step consistent with them, none of the --full records, and the dumped limbs of the
    last timed step (two exact float64 halves) hash to the C oracle's digest of this workload
    (tests/golden/manifest.json bench_digests.small)."""
    import hashlib
    import json
    import subprocess

    import numpy as np
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "small", "--dump-outputs", str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 3 and len(res["step_ms_sorted"]) == 3 and res["full"] is False
    assert res["unit"] == "matvec/s" and res["higher_is_better"] is True and res["dtype"] == "u64"
    # value = 1000 / median step ms; the line rounds both to 3 decimals (the median is a fraction of a ms here)
    m = res["median_ms_per_step"]
    assert 1000.0 / (m + 0.0005) - 0.001 <= res["value"] <= 1000.0 / (m - 0.0005) + 0.001
    # the wall time of the K steps brackets their device times (same stream, one after the other)
    assert res["ms_per_step"] * 3 >= 0.9 * sum(res["step_ms_sorted"])
    assert not {"roofline", "kernels", "cpu_baseline", "parity", "sustained", "seal_mode", "rwkv_block",
                "cfg5_chain"} & set(res)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["y_limbs_hi.npy", "y_limbs_lo.npy"]
    hi, lo = np.load(tmp_path / "y_limbs_hi.npy"), np.load(tmp_path / "y_limbs_lo.npy")
    assert hi.dtype == lo.dtype == np.float64 and hi.shape == lo.shape == (2, 5, 4096)
    limbs = hi.astype(np.uint64) * np.uint64(2 ** 32) + lo.astype(np.uint64)
    want = json.loads((REPO / "tests" / "golden" / "manifest.json").read_text())["bench_digests"]["small"]["sha256"]
    assert hashlib.sha256(limbs.tobytes()).hexdigest() == want
