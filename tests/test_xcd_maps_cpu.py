"""The block-index maps of the key-switch kernels (fhe-spear_amd/csrc/fhs_xcdmap.h) proved on the host: the very
functions the kernels call, compiled into tools/debug/xcd_map_check.cpp with the address and undefined-behaviour
sanitizers.  No GPU needed."""
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def test_every_map_covers_its_domain_once_and_balances_the_xcds(tmp_path):
    """For E = 1..48, M in {1, 2, 3, 12, 45, 64, 528}, NB in {1, 2, 64}: every (limb, item) pair of a map's domain
    comes from exactly one block of its grid and no block gives a pair outside it; per XCD (block b runs on XCD
    b & 7) the plain map is within one block, the map of the hoisted key products within one limb with all blocks
    of a limb on one XCD, and ModUp's real workgroups (its own-limb skips taken out) within 1
    wherever the special pairs suffice to level the data limbs' spread, never wider than that spread, and within one
    target limb's worth for P = 3."""
    exe = tmp_path / "xcd_map_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'fhe-spear_amd/csrc'}", str(REPO / "tools/debug/xcd_map_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    for name in ("plain_tm", "xcd_tinner", "xcd_touter", "modup_map"):
        assert any(line.startswith(name) and " ok " in line for line in r.stdout.splitlines()), name
