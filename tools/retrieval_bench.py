"""Encrypted retrieval scoring: the reference's per-op similarity join against the fused dot_product_many.

    python tools/retrieval_bench.py --shape A            # the reference demo: 64-d, 10 000 docs (J = 32, C = 3)
    python tools/retrieval_bench.py --shape B            # 1 000 000 docs (C = 245, ~3.1 GB of ciphertexts)
    python tools/retrieval_bench.py --client pk          # database and queries encrypted with the public key only

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

--client chooses who encrypts the database and every query (the scoring above is the same for all three):
  sk       sk.encode_encrypt_batch (symmetric; the default, and the line of the earlier records);
  pk       pk.encode_encrypt_batch: the reference's client, which holds only the public key (ct_ct_search.py:54-90),
           through the fused batch;
  pk-loop  encode_complex_vector_batch, then one pk.encrypt_asymmetric per plaintext -- calls every build has, so
           --engine can point this leg at the build of an earlier commit.
The pk modes add encrypt_query_ms_median / min / max (HIP events around the J encryptions of each timed query of the
fused pass) and, from the kernel-timer pass, the encrypt_pk launches' time per query with the bytes they move
(the transforms out and back, the result, the message, the key) over that time as a fraction of 8 TB/s.  pk also times its own per-ciphertext loop once (encode batch + J single
calls) and exits non-zero if the batch is not faster.

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
    ap.add_argument("--client", choices=("sk", "pk", "pk-loop"), default="sk")
    ap.add_argument("--engine", default=None,
                    help="fhe-spear_amd directory of another build (python/ and lib/): A/B against an earlier commit")
    a = ap.parse_args()
    if a.engine:
        sys.path.insert(0, str(Path(a.engine).resolve() / "python"))
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
    pk = sk.gen_publickey(ctx) if a.client != "sk" else None
    enc = ph.ckks_encoder(ctx)
    l = ctx.L0

    def pk_loop(mat):                                   # the calls every build has: encode, then one by one
        return [pk.encrypt_asymmetric(ctx, p) for p in enc.encode_complex_vector_batch(ctx, mat, scale)]

    def encrypt_rows(mat):
        if a.client == "sk":
            return sk.encode_encrypt_batch(ctx, mat, scale)
        return pk.encode_encrypt_batch(ctx, mat, scale) if a.client == "pk" else pk_loop(mat)

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
        chunks.append(encrypt_rows(np.ascontiguousarray(packed)))
    ctx.synchronize()
    encrypt_db_s = time.perf_counter() - t0

    def query_rows(qv):                                 # ct_ct_search.py:79-90: the conjugate, in every slot
        z = qv[0::2] - 1j * qv[1::2]
        return np.ascontiguousarray(np.repeat(z[:, None], slots, axis=1))

    def encrypt_query(qv):
        return encrypt_rows(query_rows(qv))

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

    enc_ms = []

    def timed(fn):
        ms, err = [], 0.0
        del enc_ms[:]                                   # the last pass's (fused) stay
        for k, qv in enumerate(queries):
            if a.client == "sk":                        # the default line: no further events
                q = encrypt_query(qv)
            else:
                rows = query_rows(qv)
                ea = ph.Event(ctx)
                q = encrypt_rows(rows)
                eb = ph.Event(ctx)
                if k >= a.warmup:
                    enc_ms.append(ea.elapsed_ms(eb))
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

    time_pk = a.client != "sk" and "encrypt_pk" in ph.KERNEL_IDS     # an earlier build has no such timer
    ph.kernel_timer_arm(ctx, ["k_dot_tensor"] + (["encrypt_pk"] if time_pk else []))
    ph.kernel_timer_read(ctx, reset=True)
    outs = None
    for qv in queries[a.warmup:]:
        outs = fused(encrypt_query(qv))
    ktimes = ph.kernel_timer_read(ctx, reset=True)
    kms, kn = ktimes["k_dot_tensor"]
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
    line["client"] = a.client
    batch_slower = False
    if a.client != "sk":
        med_enc = statistics.median(enc_ms)
        line.update({"encrypt_query_ms_median": round(med_enc, 4), "encrypt_query_ms_min": round(min(enc_ms), 4),
                     "encrypt_query_ms_max": round(max(enc_ms), 4)})
        if time_pk:
            pms, pn = ktimes["encrypt_pk"]
            p_ms = pms / a.queries                      # per query: one batch (pk) or J (pk-loop)
            ct_bytes = 2 * l * N * 8 * J
            # what the launches move per query: the three transforms written and read back (3 l N words each way),
            # the result, the message (N doubles fused, l N words of plaintext otherwise) and the key once
            moved = (6 + 2) * l * N * 8 * J + (N if a.client == "pk" else l * N) * 8 * J + 2 * l * N * 8
            line.update({"encrypt_pk_ms": round(p_ms, 4), "encrypt_pk_batches": pn, "query_ct_bytes": ct_bytes,
                         "encrypt_pk_moved_bytes": moved,
                         "encrypt_pk_hbm_fraction": round(moved / (p_ms * 1e-3) / HBM_PEAK, 4) if p_ms > 0 else None})
        if a.client == "pk":                            # the batch against its own per-ciphertext loop, timed once
            rows = query_rows(queries[-1])
            pk_loop(rows)
            ea = ph.Event(ctx)
            q = pk_loop(rows)
            eb = ph.Event(ctx)
            own = ea.elapsed_ms(eb)
            del q
            line["encrypt_query_own_loop_ms"] = round(own, 4)
            batch_slower = not med_enc < own
    s = json.dumps(line)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    if not med_fused < med_loop:
        raise SystemExit("fused path is not faster than the per-op loop")
    if batch_slower:
        raise SystemExit("pk.encode_encrypt_batch is not faster than one encrypt_asymmetric per ciphertext")


if __name__ == "__main__":
    main()
