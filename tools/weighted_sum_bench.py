"""Plaintext-weighted sums of ciphertexts: the reference's per-term loop against weighted_sums.

    python tools/weighted_sum_bench.py --leg reference  # per term: encode a constant, mod_switch_to, multiply_plain,
                                                        # rescale_to_next, add (fri:79-94, ct_pt_weighted_sum per column)
    python tools/weighted_sum_bench.py --leg loop       # the same loop over plaintexts encoded beforehand
    python tools/weighted_sum_bench.py --leg fused      # weighted_sums: one call over all columns

One leg per process.  The ring of the reference's RWKV inference (fhe_rwkv_inference.py:29-54): N = 32768,
create_coeff_modulus(N, [60] + [40] * 9 + [60]) with P = 1, inputs at chain index 3 (the squared FFN columns); F = 256
inputs of seeded uniform residues, E = 64 outputs (--E 1: one column).  The weights take --distinct values (256), weight
(j, i) being value (i F + j) mod distinct, so that the loop leg holds 256 encoded plaintexts (604 MB), not F E of them
(39 GB); every term is still its own multiply_plain, rescale_to_next and add.  The loop legs' plaintexts are the exact
constants round(w 2^40) imported as limbs (the loop leg) or the GPU encoder's (the reference leg, which may differ from
them where w 2^40 lies within the encoder's error of a half-integer; its limbs are not compared).  Timed with HIP
events on the context stream, median / min / max over --steps calls after --warmup (defaults: 3 after 0 for the
loops, 20 after 3 for the fused call).  Then the stages, in passes of their own: the loop leg times its F E
multiply_plain, rescale_to_next and add calls as three loops; the fused leg reads the per-stage timers (last-limb
INTTs, rounding sums, their residues + NTT, weighted sums).  The fused leg compares its first and last result with the
loop's, limb for limb.  The GPU's clocks are sampled before and after.

Prints one JSON line; --out appends it to a file (profiles/weighted_sum/)."""
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
SCALE = 2.0 ** 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("reference", "loop", "fused"), required=True)
    ap.add_argument("--N", type=int, default=32768)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--chain-index", type=int, default=3)
    ap.add_argument("--F", type=int, default=256)
    ap.add_argument("--E", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pyPhantom as ph
    from bench import gpu_clocks

    fused = a.leg == "fused"
    steps = a.steps if a.steps is not None else (20 if fused else 3)
    warmup = a.warmup if a.warmup is not None else (3 if fused else 0)
    N, F, E, ci = a.N, a.F, a.E, a.chain_index
    bits = [60] + [40] * a.depth + [60]
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    primes = [int(q) for q in ph.create_coeff_modulus(N, bits)]
    parms.set_coeff_modulus(primes)
    parms.set_special_modulus_size(1)
    parms.set_galois_elts([])
    ctx = ph.context(parms)
    l = ctx.limbs(ci)
    rng = np.random.default_rng(a.seed)
    xs = [ph.ciphertext_from_numpy(ctx, np.stack([np.stack([rng.integers(0, primes[i], N, dtype=np.uint64) for i in range(l)])
                                                  for _ in range(2)]), ci, SCALE) for _ in range(F)]
    vals = rng.normal(0.0, 1.0, a.distinct)
    which = (np.arange(E)[None, :] * F + np.arange(F)[:, None]) % a.distinct   # [j, i]
    W = vals[which]

    def const_pt(w):
        x = float(w) * SCALE
        c = int(np.copysign(np.floor(abs(x) + 0.5), x))
        return ph.plaintext_from_numpy(ctx, np.stack([np.full(N, c % primes[m], dtype=np.uint64) for m in range(l)]), ci, SCALE)

    pts = [const_pt(w) for w in vals] if a.leg == "loop" or fused else None
    enc = ph.ckks_encoder(ctx)
    slots = N // 2

    def term_reference(j, i):
        pt = ph.mod_switch_to(ctx, enc.encode_double_vector(ctx, [float(W[j, i])] * slots, SCALE), ci)
        return ph.rescale_to_next(ctx, ph.multiply_plain(ctx, xs[j], pt))

    def term_loop(j, i):
        return ph.rescale_to_next(ctx, ph.multiply_plain(ctx, xs[j], pts[which[j, i]]))

    def loop(term, cols=range(E)):
        outs = []
        for i in cols:
            acc = term(0, i)
            for j in range(1, F):
                acc = ph.add(ctx, acc, term(j, i))
            outs.append(acc)
        return outs

    call = {"reference": lambda: loop(term_reference), "loop": lambda: loop(term_loop),
            "fused": lambda: ph.weighted_sums(ctx, xs, W, SCALE)}[a.leg]
    bus = ph.device_pci_bus_id(ctx.device)
    clocks_start = gpu_clocks(bus)

    def timed(fn, n_steps=steps, n_warm=warmup):
        ms, out = [], None
        for k in range(n_warm + n_steps):
            del out
            e0 = ph.Event(ctx)
            out = fn()
            e1 = ph.Event(ctx)
            t = e0.elapsed_ms(e1)
            if k >= n_warm:
                ms.append(t)
        return ms, out

    ms, out = timed(call)
    line = {
        "tool": "weighted_sum_bench", "leg": a.leg, "N": N, "bits": bits, "P": 1, "chain_index": ci, "l": l, "F": F, "E": E,
        "distinct_weights": a.distinct, "steps": steps, "warmup": warmup,
        "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
        "library": os.path.relpath(ph.LIB_PATH, REPO),
    }
    stage = {}
    if a.leg == "loop":
        prods = [ph.multiply_plain(ctx, xs[j], pts[which[j, 0]]) for j in range(F)]
        terms = [ph.rescale_to_next(ctx, p) for p in prods]

        def each(fn, count):
            for k in range(count):
                fn(k)                                   # the result is dropped at once: its block goes back to the cache
        for name, fn in (("multiply_plain", lambda: each(lambda k: ph.multiply_plain(ctx, xs[k % F], pts[which[k % F, k // F]]), E * F)),
                         ("rescale_to_next", lambda: each(lambda k: ph.rescale_to_next(ctx, prods[k % F]), E * F)),
                         ("add", lambda: each(lambda k: ph.add(ctx, terms[k % F], terms[(k + 1) % F]), E * (F - 1)))):
            stage[name + "_ms_median"] = round(statistics.median(timed(fn, 3, 0)[0]), 4)
    elif fused:
        names = list(ph.STAGE_IDS)
        ph.kernel_timer_arm(ctx, names)
        ph.stage_timer_read(ctx, reset=True)
        for _ in range(steps):
            del out
            out = call()
        st = ph.stage_timer_read(ctx, reset=True)
        ph.kernel_timer_arm(ctx, [])
        for name in names:
            stage[name + "_ms_per_call"] = round(st[name][0] / steps, 4)
            stage[name + "_brackets_per_call"] = st[name][1] / steps
        want = loop(term_loop, [0, E - 1] if E > 1 else [0])
        line["limbs_equal_loop"] = bool(np.array_equal(out[0].to_numpy(), want[0].to_numpy()) and
                                        np.array_equal(out[-1].to_numpy(), want[-1].to_numpy()))
    line["stages"] = stage
    line["clocks_start"], line["clocks_end"] = clocks_start, gpu_clocks(bus)
    s = json.dumps(line)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    if fused and not line["limbs_equal_loop"]:
        raise SystemExit("weighted_sums differs from the multiply_plain / rescale_to_next / add loop")


if __name__ == "__main__":
    main()
