"""The reference's ct_pt_dot for many columns: the per-column head against multiply_plain_rescale_many.

    python tools/ct_pt_dot_bench.py --leg dot          # ct_pt_dot_many: the head of every column, then inner_sum_many
    python tools/ct_pt_dot_bench.py --leg head-loop    # per column: multiply_plain, rescale_to_next (fri:69-70)
    python tools/ct_pt_dot_bench.py --leg head-fused   # multiply_plain_rescale_many: one call over all columns

One leg per process.  The ring of the reference's RWKV inference (fhe_rwkv_inference.py:29-54): N = 32768,
create_coeff_modulus(N, [60] + [40] * 9 + [60]) with P = 1, the input at chain index 1; one ciphertext of seeded
uniform residues against n = 64 plaintexts of seeded uniform residues, dim = 256 (8 rotation steps).  The dot leg
runs on any build that has ct_pt_dot_many (before multiply_plain_rescale_many existed its head was the per-column
loop), so the same command times both.  Timed with HIP events on the context stream after warm-up, median / min / max
over --steps calls.  The fused head leg then reads the rescale's per-kernel timer in a pass of its own and compares
its first and last result with the loop's, limb for limb.  The GPU's clocks are sampled before and after.

Prints one JSON line; --out appends it to a file (profiles/ct_pt_dot/)."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "fhe-spear_amd" / "python"))
sys.path.insert(0, str(REPO))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("dot", "head-loop", "head-fused"), required=True)
    ap.add_argument("--N", type=int, default=32768)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--chain-index", type=int, default=1)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--tag", default=None, help="copied into the line (which build this is)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pyPhantom as ph
    from bench import gpu_clocks

    N, n = a.N, a.n
    bits = [60] + [40] * a.depth + [60]
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    primes = ph.create_coeff_modulus(N, bits)
    parms.set_coeff_modulus(primes)
    parms.set_special_modulus_size(1)
    steps = []
    s = 1
    while s < a.dim:
        steps.append(s)
        s *= 2
    parms.set_galois_elts(sorted(set(ph.get_elts_from_steps(steps, N))) if a.leg == "dot" else [])
    ctx = ph.context(parms)
    sk = ph.secret_key(ctx, seed=a.seed)
    gk = sk.create_galois_keys(ctx) if a.leg == "dot" else None
    l = ctx.limbs(a.chain_index)
    rng = np.random.default_rng(a.seed)

    def limbs():
        return np.stack([rng.integers(0, int(primes[i]), N, dtype=np.uint64) for i in range(l)])

    ct = ph.ciphertext_from_numpy(ctx, np.stack([limbs(), limbs()]), a.chain_index, 2.0 ** 40)
    pts = [ph.plaintext_from_numpy(ctx, limbs(), a.chain_index, 2.0 ** 40) for _ in range(n)]
    bus = ph.device_pci_bus_id(ctx.device)
    clocks_start = gpu_clocks(bus)

    def head_loop(pp):
        return [ph.rescale_to_next(ctx, ph.multiply_plain(ctx, ct, p)) for p in pp]

    if a.leg == "dot":
        call = lambda: ph.ct_pt_dot_many(ctx, ct, pts, a.dim, gk)
    elif a.leg == "head-loop":
        call = lambda: head_loop(pts)
    else:
        call = lambda: ph.multiply_plain_rescale_many(ctx, ct, pts)

    def timed(fn, count):
        ms = []
        out = None
        for k in range(a.warmup + count):
            del out
            e0 = ph.Event(ctx)
            out = fn()
            e1 = ph.Event(ctx)
            t = e0.elapsed_ms(e1)
            if k >= a.warmup:
                ms.append(t)
        return ms, out

    ms, out = timed(call, a.steps)
    line = {
        "tool": "ct_pt_dot_bench", "leg": a.leg, "tag": a.tag, "N": N, "bits": bits, "P": 1, "chain_index": a.chain_index,
        "l": l, "n": n, "dim": a.dim, "steps": a.steps, "warmup": a.warmup,
        "head": "multiply_plain_rescale_many" if hasattr(ph, "multiply_plain_rescale_many") else "per-column loop",
        "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
        "library": os.path.relpath(ph.LIB_PATH, REPO),
    }
    if a.leg == "head-fused":
        ph.kernel_timer_arm(ctx, ["rescale"])
        ph.kernel_timer_read(ctx, reset=True)
        for _ in range(a.steps):
            del out
            out = call()
        kms, kn = ph.kernel_timer_read(ctx, reset=True)["rescale"]
        ph.kernel_timer_arm(ctx, [])
        line["rescale_ms_per_call"] = round(kms / a.steps, 4)
        line["rescale_launches_per_call"] = kn / a.steps
        want = head_loop([pts[0], pts[-1]])
        line["limbs_equal_loop"] = bool(np.array_equal(out[0].to_numpy(), want[0].to_numpy()) and
                                        np.array_equal(out[-1].to_numpy(), want[1].to_numpy()))
    line["clocks_start"], line["clocks_end"] = clocks_start, gpu_clocks(bus)
    s = json.dumps(line)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    if a.leg == "head-fused" and not line["limbs_equal_loop"]:
        raise SystemExit("multiply_plain_rescale_many differs from the multiply_plain / rescale_to_next loop")


if __name__ == "__main__":
    main()
