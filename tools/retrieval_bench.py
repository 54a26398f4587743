"""Encrypted retrieval scoring: the reference's per-op similarity join against the fused dot_product_many.

    python tools/retrieval_bench.py --shape A            # the reference demo: 64-d, 10 000 docs (J = 32, C = 3)
    python tools/retrieval_bench.py --shape B            # 1 000 000 docs (C = 245, ~3.1 GB of ciphertexts)

One shape per process.  Synthetic seeded unit-norm embeddings, N = 8192, create_coeff_modulus(N, [60, 40, 40,
60]) with P = 1 (ct_ct_search.py:27-30), complex packing as EncryptedSimilarityJoins (two dimensions per slot,
one document per slot, J = dim / 2 ciphertexts per chunk of N / 2 documents).  Encrypting the database is
outside every timed region.  Timed with HIP events on the context stream, after warm-up, median over --queries:

  loop   ct_ct_search.py:92-106 op for op: multiply, relinearize, rescale_to_next per term, then add --
         ops the fused path does not touch, so this is what the engine did before dot_product_many existed;
  fused  dot_product_many(query, chunks, rk);
  k_dot_tensor  the kernel's own time (per-kernel timer, a separate pass so its events do not sit inside the
         timed queries) and its C J 2 l N 8 database bytes over that time as a fraction of 8 TB/s;
  decrypt + decode of the C score ciphertexts (host wall time, reported apart), and both paths' max score
  error against float64 docs @ q.

Prints one JSON line; --out appends it to a file (profiles/retrieval/)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "fhe-spear_amd" / "python"))

SHAPES = {"A": 10_000, "B": 1_000_000}
HBM_PEAK = 8.0e12            # bytes / s, MI355X


def unit_rows(rng, n, d):
    v = rng.normal(size=(n, d))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="A")
    ap.add_argument("--docs", type=int, default=None, help="override the shape's document count")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--queries", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pyPhantom as ph

    N, dim = a.N, a.dim
    docs_n = a.docs or SHAPES[a.shape]
    slots, J = N // 2, dim // 2
    C = (docs_n + slots - 1) // slots
    scale = 2.0 ** 40
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(ph.create_coeff_modulus(N, [60, 40, 40, 60]))
    parms.set_special_modulus_size(1)
    ctx = ph.context(parms)
    sk = ph.secret_key(ctx, seed=a.seed)
    rk = sk.gen_relinkey(ctx)
    l = ctx.L0

    rng = np.random.default_rng(a.seed)
    docs = unit_rows(rng, docs_n, dim)
    queries = unit_rows(rng, a.warmup + a.queries, dim)
    t0 = time.perf_counter()
    chunks = []
    for c in range(C):                                  # ct_ct_search.py:39-75, one chunk at a time
        v = np.zeros((slots, dim))
        part = docs[c * slots:(c + 1) * slots]
        v[:len(part)] = part
        packed = (v[:, 0::2] + 1j * v[:, 1::2]).T       # [J][slots]
        chunks.append(sk.encode_encrypt_batch(ctx, np.ascontiguousarray(packed), scale))
    ctx.synchronize()
    encrypt_db_s = time.perf_counter() - t0

    def encrypt_query(qv):                              # ct_ct_search.py:79-90: the conjugate, in every slot
        z = qv[0::2] - 1j * qv[1::2]
        return sk.encode_encrypt_batch(ctx, np.ascontiguousarray(np.repeat(z[:, None], slots, axis=1)), scale)

    def loop(q):                                        # ct_ct_search.py:92-106
        out = []
        for ch in chunks:
            res = None
            for j in range(J):
                p = ph.rescale_to_next(ctx, ph.relinearize(ctx, ph.multiply(ctx, q[j], ch[j]), rk))
                res = p if res is None else ph.add(ctx, res, p)
            out.append(res)
        return out

    def fused(q):
        return ph.dot_product_many(ctx, q, chunks, rk)

    def scores_of(cts):
        z = sk.decrypt_decode_batch(ctx, cts)
        return np.real(z).reshape(-1)[:docs_n]

    def timed(fn):
        ms, err = [], 0.0
        for k, qv in enumerate(queries):
            q = encrypt_query(qv)
            e0 = ph.Event(ctx)
            out = fn(q)
            e1 = ph.Event(ctx)
            t = e0.elapsed_ms(e1)
            if k >= a.warmup:
                ms.append(t)
                if k == a.warmup:                       # one accuracy check per path, outside the clock
                    err = float(np.max(np.abs(scores_of(out) - docs @ qv)))
            del out, q
        return ms, err

    loop_ms, loop_err = timed(loop)
    fused_ms, fused_err = timed(fused)

    ph.kernel_timer_arm(ctx, ["k_dot_tensor"])
    ph.kernel_timer_read(ctx, reset=True)
    outs = None
    for qv in queries[a.warmup:]:
        outs = fused(encrypt_query(qv))
    kms, kn = ph.kernel_timer_read(ctx, reset=True)["k_dot_tensor"]
    ph.kernel_timer_arm(ctx, [])
    t0 = time.perf_counter()
    scores_of(outs)
    decode_ms = (time.perf_counter() - t0) * 1e3

    db_bytes = C * J * 2 * l * N * 8
    k_ms = kms / max(1, kn) * (-(-J // 64))             # launches per query: one per 64-term window
    med_loop, med_fused = statistics.median(loop_ms), statistics.median(fused_ms)
    line = {
        "tool": "retrieval_bench", "shape": a.shape, "N": N, "dim": dim, "docs": docs_n, "J": J, "C": C, "l": l,
        "bits": [60, 40, 40, 60], "P": 1, "queries": a.queries, "warmup": a.warmup,
        "loop_ms_median": round(med_loop, 4), "loop_ms_min": round(min(loop_ms), 4), "loop_ms_max": round(max(loop_ms), 4),
        "fused_ms_median": round(med_fused, 4), "fused_ms_min": round(min(fused_ms), 4),
        "fused_ms_max": round(max(fused_ms), 4), "speedup_median": round(med_loop / med_fused, 2),
        "k_dot_tensor_ms": round(k_ms, 4), "k_dot_tensor_launches": kn, "db_bytes": db_bytes,
        "k_dot_tensor_hbm_fraction": round(db_bytes / (k_ms * 1e-3) / HBM_PEAK, 4) if k_ms > 0 else None,
        "max_err_loop": loop_err, "max_err_fused": fused_err,
        "decrypt_decode_ms": round(decode_ms, 3), "encrypt_db_s": round(encrypt_db_s, 3),
        "loop_ops": {"multiply": C * J, "relinearize": C * J, "rescale_to_next": C * J, "add": C * (J - 1)},
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    if not med_fused < med_loop:
        raise SystemExit("fused path is not faster than the per-op loop")


if __name__ == "__main__":
    main()
