"""Rotate-and-sum of the slots for many ciphertexts: the per-op loops against the batched inner_sum_many.

    python tools/inner_sum_bench.py --leg loop          # per column: rotate + add per step (fri:71-75 as written)
    python tools/inner_sum_bench.py --leg rotate_many   # per step: one rotate_many over all columns, then an add each
    python tools/inner_sum_bench.py --leg fused         # inner_sum_many: one key switch per step, adds in its ModDown

One leg per process.  The ring of the reference's RWKV inference (fhe_rwkv_inference.py:29-54): N = 32768,
create_coeff_modulus(N, [60] + [40] * 9 + [60]) with P = 1, inputs at chain index 2 (after ct_pt_dot's rescale);
dim = 256 (8 steps), n = 64 columns of seeded uniform residues.  Timed with HIP events on the context stream after
warm-up, median / min / max over --steps calls; the fused leg then times k_ks_ip and ModDown with the per-kernel
timers in a pass of their own (so their events do not sit inside the timed calls) and compares its first and last
results with the loop's, limb for limb.  The GPU's clocks are sampled before and after.

Prints one JSON line; --out appends it to a file (profiles/inner_sum/)."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "fhe-spear_amd" / "python"))
sys.path.insert(0, str(REPO))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("loop", "rotate_many", "fused"), required=True)
    ap.add_argument("--N", type=int, default=32768)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--chain-index", type=int, default=2)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pyPhantom as ph
    from bench import gpu_clocks

    N, n, dim = a.N, a.n, a.dim
    bits = [60] + [40] * a.depth + [60]
    rot = []
    s = 1
    while s < dim:
        rot.append(s)
        s *= 2
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    primes = ph.create_coeff_modulus(N, bits)
    parms.set_coeff_modulus(primes)
    parms.set_special_modulus_size(1)
    parms.set_galois_elts(sorted(set(ph.get_elts_from_steps(rot, N))))
    ctx = ph.context(parms)
    sk = ph.secret_key(ctx, seed=a.seed)
    gk = sk.create_galois_keys(ctx)
    l = ctx.limbs(a.chain_index)
    rng = np.random.default_rng(a.seed)
    cts = []
    for _ in range(n):
        limbs = np.stack([np.stack([rng.integers(0, int(primes[i]), N, dtype=np.uint64) for i in range(l)])
                          for _ in range(2)])
        cts.append(ph.ciphertext_from_numpy(ctx, limbs, a.chain_index, 2.0 ** 40))
    del limbs
    bus = ph.device_pci_bus_id(ctx.device)
    clocks_start = gpu_clocks(bus)

    def loop(xs):
        out = []
        for x in xs:
            for st in rot:
                x = ph.add(ctx, x, ph.rotate(ctx, x, st, gk))
            out.append(x)
        return out

    def rotate_many(xs):
        xs = list(xs)
        for st in rot:
            ins = (C.c_void_p * n)(*[x._h for x in xs])
            steps = (C.c_int * n)(*([st] * n))
            outs = (C.c_void_p * n)()
            ph._check(ph._lib.fhs_rotate_many(ctx._h, ins, steps, n, gk._h, outs), "rotate_many")
            rots = [ph.ciphertext(ctx, C.c_void_p(outs[i])) for i in range(n)]
            xs = [ph.add(ctx, x, r) for x, r in zip(xs, rots)]
        return xs

    def fused(xs):
        return ph.inner_sum_many(ctx, xs, dim, gk)

    fn = {"loop": loop, "rotate_many": rotate_many, "fused": fused}[a.leg]
    ms = []
    for k in range(a.warmup + a.steps):
        e0 = ph.Event(ctx)
        out = fn(cts)
        e1 = ph.Event(ctx)
        t = e0.elapsed_ms(e1)
        if k >= a.warmup:
            ms.append(t)
        if k + 1 < a.warmup + a.steps:
            del out
    line = {
        "tool": "inner_sum_bench", "leg": a.leg, "N": N, "bits": bits, "P": 1, "chain_index": a.chain_index, "l": l,
        "dim": dim, "n": n, "rotation_steps": rot, "steps": a.steps, "warmup": a.warmup,
        "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
        "key_switches_per_call": len(rot) * n, "key_switch_launch_groups_per_call": len(rot) * (n if a.leg == "loop" else 1),
    }
    if a.leg == "fused":
        ph.kernel_timer_arm(ctx, ["k_ks_ip", "k_moddown"])
        ph.kernel_timer_read(ctx, reset=True)
        for _ in range(a.steps):
            del out
            out = fused(cts)
        kt = ph.kernel_timer_read(ctx, reset=True)
        ph.kernel_timer_arm(ctx, [])
        for name in ("k_ks_ip", "k_moddown"):
            kms, kn = kt[name]
            line[name + "_ms_per_call"] = round(kms / a.steps, 4)
            line[name + "_launches_per_call"] = kn / a.steps
        want = loop([cts[0], cts[-1]])
        line["limbs_equal_loop"] = bool(np.array_equal(out[0].to_numpy(), want[0].to_numpy()) and
                                        np.array_equal(out[-1].to_numpy(), want[1].to_numpy()))
    line["clocks_start"], line["clocks_end"] = clocks_start, gpu_clocks(bus)
    s = json.dumps(line)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    if a.leg == "fused" and not line["limbs_equal_loop"]:
        raise SystemExit("inner_sum_many differs from the rotate + add loop")


if __name__ == "__main__":
    main()
