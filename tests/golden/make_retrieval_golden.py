"""Generate the retrieval fixture by running the REFERENCE's own encrypted similarity join
(/root/reference/gpu/ct_ct_search.py EncryptedSimilarityJoins: encrypt_database, encrypt_query, search,
decrypt_scores -- imported read-only, bytecode writing disabled) on the C parity oracle, installed as
`pyPhantom` (oracle/pyphantom_oracle.py), on its own parameter set create_coeff_modulus(N, [60, 40, 40, 60]),
P = 1.  Run in the build container only (the reference does not travel to the GPU box):

    python tests/golden/make_retrieval_golden.py

Outputs tests/golden/retrieval_ctct_n512.npz + retrieval_manifest.json.  The archive is written with fixed
member timestamps, so a rerun reproduces it byte for byte.  tests/test_retrieval_dot.py replays it on the GPU.
"""
import hashlib
import io
import json
import sys
import zipfile
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[2]
REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
from oracle import pyphantom_oracle as php  # noqa: E402

sys.modules["pyPhantom"] = php
sys.path.insert(0, str(REF))
sys.path.insert(0, str(REF / "gpu"))
import ct_ct_search as cs  # noqa: E402

NAME = "retrieval_ctct_n512"
N, DIM, DOCS = 512, 16, 300
MIN_GAP = 1e-6            # the float64 top-11 scores must be further apart than this (a stable top-10)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def unit_rows(rng, n, d):
    v = rng.normal(size=(n, d))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def pick_data():
    """First seed from 2025 whose float64 top-11 scores are separated by more than MIN_GAP."""
    for seed in range(2025, 2125):
        rng = np.random.default_rng(seed)
        docs, query = unit_rows(rng, DOCS, DIM), unit_rows(rng, 1, DIM)[0]
        top = np.sort(docs @ query)[::-1][:11]
        if np.min(-np.diff(top)) > MIN_GAP:
            return seed, docs, query
    raise SystemExit("no seed with a separated top-11")


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    seed, docs, query = pick_data()
    esj = cs.EncryptedSimilarityJoins(embed_dim=DIM, poly_degree=N)
    pts = []                                        # every encoded plaintext, in encryption order
    enc_a = php.public_key.encrypt_asymmetric

    def encrypt(self, ctx, pt):
        pts.append(pt.data.copy())
        return enc_a(self, ctx, pt)
    php.public_key.encrypt_asymmetric = encrypt
    php.OP_COUNTS.clear()
    try:
        db = esj.encrypt_database(docs)
        q = esj.encrypt_query(query)
        scores_ct = esj.search(q, db)
        dec = esj.decrypt_scores(scores_ct, DOCS)
    finally:
        php.public_key.encrypt_asymmetric = enc_a
    counts = dict(php.OP_COUNTS)
    J, C = esj.n_cts_per_vec, db["n_chunks"]
    assert (J, C, len(pts)) == (8, 2, 24) and DOCS < C * esj.slot_count        # the second chunk is padded
    exact = docs @ query
    max_err_loop = float(np.max(np.abs(dec - exact)))
    assert list(np.argsort(-dec)[:10]) == list(np.argsort(-exact)[:10])
    primes = np.array(esj.ctx.o.primes, dtype=np.uint64)
    print(f"[{NAME}] seed={seed} J={J} C={C} primes={[int(p).bit_length() for p in primes]} "
          f"max|score - docs@q|={max_err_loop:.3e} ops={counts}")
    write_npz(OUT / f"{NAME}.npz", {
        "primes": primes, "docs": docs, "query": query,
        "sk_seed": np.array(esj.sk.seed, dtype=np.int64),
        "pts": np.stack(pts),                              # [24][3][N]: chunk 0 (8), chunk 1 (8), query (8)
        "scores_ct": np.stack([c.data for c in scores_ct]),   # [2][2][2][N]
        "scores": dec, "max_err_loop": np.array(max_err_loop)})
    size = (OUT / f"{NAME}.npz").stat().st_size
    assert size < 600_000, size
    manifest = {
        "file": f"{NAME}.npz", "generator": "tests/golden/make_retrieval_golden.py",
        "reference": "gpu/ct_ct_search.py EncryptedSimilarityJoins(embed_dim=16, poly_degree=512): "
                     "encrypt_database, encrypt_query, search, decrypt_scores",
        "N": N, "embed_dim": DIM, "docs": DOCS, "J": J, "C": C, "bits": [60, 40, 40, 60], "P": 1,
        "data_seed": seed, "sk_seed": esj.sk.seed, "pk_enc_counter": 1 << 20, "scale": esj.scale,
        "pts_order": "chunk 0 (J), chunk 1 (J), query (J); asymmetric encryptions in that order",
        "chain_index_out": scores_ct[0].chain_index(), "scale_out": scores_ct[0].scale(),
        "max_err_loop": max_err_loop, "min_top11_gap": float(np.min(-np.diff(np.sort(exact)[::-1][:11]))),
        "op_counts": counts, "secret_sha256": sha(esj.sk.s), "scores_ct_sha256": sha(np.stack([c.data for c in scores_ct])),
        "npz_sha256": hashlib.sha256((OUT / f"{NAME}.npz").read_bytes()).hexdigest(), "npz_bytes": size,
    }
    (OUT / "retrieval_manifest.json").write_text(json.dumps(manifest, indent=1) + "\n")


if __name__ == "__main__":
    main()
