"""CT x CT multiply, relinearize and rescale for many ciphertexts: the per-column loop against multiply_relin_many.

    python tools/multiply_bench.py --leg loop           # per column: multiply, relinearize, rescale_to_next (fri:97-101)
    python tools/multiply_bench.py --leg fused-square   # square_many: one call over all columns, operands read once
    python tools/multiply_bench.py --leg fused-pairs    # multiply_relin_many over n pairs of distinct ciphertexts

One leg per process.  The ring of the reference's RWKV inference (fhe_rwkv_inference.py:29-54): N = 32768,
create_coeff_modulus(N, [60] + [40] * 9 + [60]) with P = 1, inputs at chain index 2 (after ct_pt_dot's rescale);
n = 64 columns of seeded uniform residues.  The loop leg squares (as ct_ct_square is written); --loop-pairs makes it
multiply the pairs of the fused-pairs leg instead.  Timed with HIP events on the context stream after warm-up,
median / min / max over --steps calls.  Then the stages, each in a pass of its own so that no event sits inside a
timed call: the loop leg times its n multiplies, n relinearizations and n rescales as three loops; a fused leg times
the tensor stage as a call without key and rescale, and the key switch's kernels and the rescale with the
per-kernel timers.  Each fused leg compares its first and last result with the loop's, limb for limb.  The GPU's
clocks are sampled before and after.

Prints one JSON line; --out appends it to a file (profiles/multiply_many/)."""
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
KS_KERNELS = ("k_ks_intt", "k_modup", "k_ks_ip", "k_ks_special_intt", "k_moddown", "rescale")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("loop", "fused-square", "fused-pairs"), required=True)
    ap.add_argument("--N", type=int, default=32768)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--chain-index", type=int, default=2)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--loop-pairs", action="store_true")
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
    parms.set_galois_elts([])
    ctx = ph.context(parms)
    sk = ph.secret_key(ctx, seed=a.seed)
    rk = sk.gen_relinkey(ctx)
    l = ctx.limbs(a.chain_index)
    rng = np.random.default_rng(a.seed)
    pairs = a.leg == "fused-pairs" or (a.leg == "loop" and a.loop_pairs)

    def uniform():
        limbs = np.stack([np.stack([rng.integers(0, int(primes[i]), N, dtype=np.uint64) for i in range(l)])
                          for _ in range(2)])
        return ph.ciphertext_from_numpy(ctx, limbs, a.chain_index, 2.0 ** 40)

    xs = [uniform() for _ in range(n)]
    ys = [uniform() for _ in range(n)] if pairs else xs
    bus = ph.device_pci_bus_id(ctx.device)
    clocks_start = gpu_clocks(bus)

    def loop(aa, bb):
        return [ph.rescale_to_next(ctx, ph.relinearize(ctx, ph.multiply(ctx, x, y), rk)) for x, y in zip(aa, bb)]

    def fused(aa, bb, key=rk, rescale=True):
        return ph.multiply_relin_many(ctx, aa, bb if pairs else None, key, rescale)

    fn = loop if a.leg == "loop" else fused

    def timed(call):
        ms = []
        out = None
        for k in range(a.warmup + a.steps):
            del out
            e0 = ph.Event(ctx)
            out = call()
            e1 = ph.Event(ctx)
            t = e0.elapsed_ms(e1)
            if k >= a.warmup:
                ms.append(t)
        return ms, out

    ms, out = timed(lambda: fn(xs, ys))
    line = {
        "tool": "multiply_bench", "leg": a.leg, "operands": "pairs" if pairs else "squares", "N": N, "bits": bits, "P": 1,
        "chain_index": a.chain_index, "l": l, "n": n, "steps": a.steps, "warmup": a.warmup,
        "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
        "library": os.path.relpath(ph.LIB_PATH, REPO),
    }
    stage = {}
    if a.leg == "loop":
        prods = [ph.multiply(ctx, x, y) for x, y in zip(xs, ys)]
        relins = [ph.relinearize(ctx, p, rk) for p in prods]
        for name, call in (("multiply", lambda: [ph.multiply(ctx, x, y) for x, y in zip(xs, ys)]),
                           ("relinearize", lambda: [ph.relinearize(ctx, p, rk) for p in prods]),
                           ("rescale_to_next", lambda: [ph.rescale_to_next(ctx, r) for r in relins])):
            stage[name + "_ms_median"] = round(statistics.median(timed(call)[0]), 4)
    else:
        stage["tensor_ms_median"] = round(statistics.median(timed(lambda: fused(xs, ys, None, False))[0]), 4)
        ph.kernel_timer_arm(ctx, list(KS_KERNELS))
        ph.kernel_timer_read(ctx, reset=True)
        for _ in range(a.steps):
            del out
            out = fused(xs, ys)
        kt = ph.kernel_timer_read(ctx, reset=True)
        ph.kernel_timer_arm(ctx, [])
        for name in KS_KERNELS:
            kms, kn = kt[name]
            stage[name + "_ms_per_call"] = round(kms / a.steps, 4)
            stage[name + "_launches_per_call"] = kn / a.steps
        want = loop([xs[0], xs[-1]], [ys[0], ys[-1]])
        line["limbs_equal_loop"] = bool(np.array_equal(out[0].to_numpy(), want[0].to_numpy()) and
                                        np.array_equal(out[-1].to_numpy(), want[1].to_numpy()))
    line["stages"] = stage
    line["clocks_start"], line["clocks_end"] = clocks_start, gpu_clocks(bus)
    s = json.dumps(line)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    if a.leg != "loop" and not line["limbs_equal_loop"]:
        raise SystemExit("multiply_relin_many differs from the multiply / relinearize / rescale loop")


if __name__ == "__main__":
    main()
