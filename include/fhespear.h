/*
 * fhespear.h -- C ABI of libfhespear_hip.so, the MI355X-native CKKS engine behind FHE-SPEAR's
 * BSGS diagonal matrix-vector path.
 *
 * It replaces gpu/phantom_binding.cu (the pybind11 module `pyPhantom`, pb) and the un-vendored
 * PhantomFHE arithmetic under it.  Each entry point names the reference binding/call site it
 * stands in for.  The Python module fhe-spear_amd/python/pyPhantom binds these with ctypes
 * (INTEGRATION.md shows the binding and the fhe_common.py switch).
 *
 * Conventions
 *  - Plain pointers and sizes only; objects are opaque handles freed with *_destroy.
 *  - Every function returns an fhs_status (0 = OK); fhs_last_error() returns a thread-local
 *    message for the last failure.  FHS_ERR_OOM messages contain "out of memory" (the reference
 *    string-matches that text, scripts/bootstrap_generation.py:1164-1166).
 *  - Ciphertexts/plaintexts are device-resident in HBM: [comp][limb][N] uint64, NTT form,
 *    bit-reversed evaluation order.  chain_index c holds L0 + 1 - c data limbs (pb:144, tf:33).
 *  - All work is ordered on one HIP stream per context; calls are serialised per context and
 *    are safe from several host threads (bg:223-249).  Functions that return host data
 *    synchronise the stream.
 */
#ifndef FHESPEAR_H
#define FHESPEAR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int fhs_status;
enum {
    FHS_OK = 0,
    FHS_ERR_INVALID = 1,      /* bad argument / unsupported parameter */
    FHS_ERR_OOM = 2,          /* device or host allocation failed ("out of memory") */
    FHS_ERR_HIP = 3,          /* HIP runtime error */
    FHS_ERR_LEVEL = 4,        /* operands at different chain indices / no level left */
    FHS_ERR_SCALE = 5,        /* scale mismatch on add */
    FHS_ERR_KEY = 6,          /* missing Galois key for a rotation step */
    FHS_ERR_NODEVICE = 7      /* no HIP device available */
};

typedef struct fhs_context fhs_context;
typedef struct fhs_ciphertext fhs_ciphertext;
typedef struct fhs_plaintext fhs_plaintext;
typedef struct fhs_secret_key fhs_secret_key;
typedef struct fhs_public_key fhs_public_key;
typedef struct fhs_relin_key fhs_relin_key;
typedef struct fhs_galois_keys fhs_galois_keys;

const char* fhs_last_error(void);
const char* fhs_version(void);
int fhs_device_count(void);
/* PCI bus id of HIP device `device` (e.g. "0000:05:00.0"), for the multi-rank line's device check.  Replaces
 * no pb symbol (extension). */
fhs_status fhs_device_pci_bus_id(int device, char* buf, int len);
/* Testing hook (extension, replaces no pb symbol): the next `count` flushes of queued rotations on `ctx` fail as
 * out of memory before launching, so the drop-the-queue path (queued outputs marked lost, later uses rejected)
 * can be exercised without exhausting HBM. */
fhs_status fhs_debug_fail_next_flushes(fhs_context* ctx, int count);
/* Testing hook (extension, replaces no pb symbol): nth >= 0 arms it -- the (nth+1)-th device allocation `ctx` makes
 * from now on (cache hits included) fails once as out of memory, before the block cache is consulted and before any
 * hipMalloc; nth < 0 disarms it.  *was_armed (may be NULL) receives whether an arming was still pending.  Launches
 * nothing and touches no device state: every failure path can be walked without exhausting HBM. */
fhs_status fhs_debug_fail_alloc(fhs_context* ctx, int nth, int* was_armed);
/* Testing hook (extension, replaces no pb symbol): on > 0 makes every giant-step launch of `ctx` at N >= 512 take
 * its forked form (the special limbs' chain on the context's side stream), whatever its size; on == 0 restores the
 * size threshold; on < 0 changes nothing.  *forked (may be NULL) receives the number of launches of `ctx` that have
 * taken the forked form so far.  Results are the same limbs either way. */
fhs_status fhs_debug_force_fork(fhs_context* ctx, int on, uint64_t* forked);
/* Testing hook (extension, replaces no pb symbol): the launch ledger, one per process.  Every kernel launch of the
 * library passes one macro; while the ledger is armed that macro records which kernel was launched (disarmed it
 * costs one relaxed atomic load).  The tests use it to prove that each compiled kernel has an oracle-checked case.
 *   FHS_LEDGER_ARM     clears the ledger and arms it
 *   FHS_LEDGER_DISARM  stops recording; what was recorded stays readable
 *   FHS_LEDGER_READ    writes the launched kernels to buf as sorted names, each followed by '\n', NUL-terminated:
 *                      the kernel with its template arguments and nothing else ("k_modup_h<12, 3, true>").  *needed
 *                      (may be NULL) receives the byte count including the NUL; a buffer shorter than that (or NULL)
 *                      is FHS_ERR_INVALID with *needed still set.  An empty ledger reads as "".
 * buf, len and needed are ignored by ARM and DISARM. */
enum { FHS_LEDGER_ARM = 0, FHS_LEDGER_DISARM = 1, FHS_LEDGER_READ = 2 };
fhs_status fhs_debug_launch_ledger(int op, char* buf, uint64_t len, uint64_t* needed);
/* Testing hook (extension, replaces no pb symbol): the state of `ctx`'s host allocator, so that a test which bounds
 * a cache can see the bound being applied.  Writes the first min(n, FHS_ALLOC_STATS_COUNT) of these to out:
 *   FHS_ALLOC_CACHED_BYTES     bytes of freed device blocks kept in the block cache
 *   FHS_ALLOC_CACHE_CAP        the bound on them (a quarter of the device's memory, or FHESPEAR_CACHE_BYTES as read
 *                              when the context was created)
 *   FHS_ALLOC_EVICTED          cached blocks returned to the device so far because the cache was over its bound
 *                              (one per hipFree; the trims on out-of-memory and at destruction are not counted)
 *   FHS_ALLOC_FIT              batch allocations so far that took a cached block larger than their request whole
 *                              (up to 1.5x; an exact-size hit is not counted)
 *   FHS_ALLOC_SEAL_CORR_BYTES  bytes of SEAL-convention hoisting corrections kept per (Galois key, level)
 *   FHS_ALLOC_SEAL_CORR_CAP    the bound on them (1/16 of the device's memory, or FHESPEAR_SEAL_CORR_BYTES)
 *   FHS_ALLOC_SEAL_CORR_DROPS  times a flush emptied a non-empty correction cache because its own corrections did
 *                              not fit under the bound (a key's corrections leaving with the key are not counted)
 * Read-only: it launches nothing, flushes no queued rotation and touches no device state. */
enum {
    FHS_ALLOC_CACHED_BYTES = 0,
    FHS_ALLOC_CACHE_CAP = 1,
    FHS_ALLOC_EVICTED = 2,
    FHS_ALLOC_FIT = 3,
    FHS_ALLOC_SEAL_CORR_BYTES = 4,
    FHS_ALLOC_SEAL_CORR_CAP = 5,
    FHS_ALLOC_SEAL_CORR_DROPS = 6,
    FHS_ALLOC_STATS_COUNT = 7
};
fhs_status fhs_debug_alloc_stats(fhs_context* ctx, uint64_t* out, int n);

/* ---- parameters (pb:78-98) ---- */
/* pb:81 create_coeff_modulus: SEAL CoeffModulus::Create (largest primes = 1 mod 2N per size) */
fhs_status fhs_create_coeff_modulus(uint64_t N, const int* bit_sizes, int n, uint64_t* primes_out);
/* pb:124-126 get_elt_from_step(s): 5^s mod 2N (s<0 -> 5^(N/2-|s|), s=0 -> 2N-1) */
uint64_t fhs_galois_elt_from_step(int step, uint64_t N);

/* pb:85-98 params + context(params).  primes: key-level list, the last `special` are the
 * special primes; galois_elts: the set create_galois_keys will generate (NULL/0 = default
 * power-of-two steps + conjugation, as Phantom does when set_galois_elts is not called). */
fhs_status fhs_context_create(uint64_t N, const uint64_t* primes, int nprimes, int special,
                              const uint64_t* galois_elts, int n_elts, int device, fhs_context** out);
fhs_status fhs_context_destroy(fhs_context* ctx);
fhs_status fhs_context_info(const fhs_context* ctx, uint64_t* N, int* L0, int* P, int* n_elts);
fhs_status fhs_context_galois_elts(const fhs_context* ctx, uint64_t* elts_out);
fhs_status fhs_synchronize(fhs_context* ctx);
/* bytes currently held by the context's device pool (diagnostics) */
fhs_status fhs_memory_in_use(fhs_context* ctx, uint64_t* bytes);

/* ---- keys (pb:100-124) ---- */
/* pb:100 secret_key(ctx).  All secret randomness is ChaCha20 keyed by key32:
 * deterministic for a caller-supplied key (tests: the integer seed, 32 bytes little-endian). */
fhs_status fhs_secret_key_create(fhs_context* ctx, const uint8_t* key32 /* 32 bytes, NULL: /dev/urandom */,
                                 fhs_secret_key** out);
fhs_status fhs_secret_key_destroy(fhs_secret_key* sk);
fhs_status fhs_gen_public_key(fhs_context* ctx, fhs_secret_key* sk, fhs_public_key** out);      /* pb:102 */
fhs_status fhs_gen_relin_key(fhs_context* ctx, fhs_secret_key* sk, fhs_relin_key** out);        /* pb:103 */
/* pb:104 create_galois_keys: keys for elts (NULL/0 = the context's set) */
fhs_status fhs_create_galois_keys(fhs_context* ctx, fhs_secret_key* sk, const uint64_t* elts, int n,
                                  fhs_galois_keys** out);
fhs_status fhs_public_key_destroy(fhs_public_key* pk);
fhs_status fhs_relin_key_destroy(fhs_relin_key* rk);
fhs_status fhs_galois_keys_destroy(fhs_galois_keys* gk);
fhs_status fhs_galois_keys_has(const fhs_galois_keys* gk, uint64_t elt, int* has);
/* export one switching key [dnum][2][L0+P][N] (parity tests) */
fhs_status fhs_galois_key_export(fhs_context* ctx, const fhs_galois_keys* gk, uint64_t elt, uint64_t* host);
fhs_status fhs_relin_key_export(fhs_context* ctx, const fhs_relin_key* rk, uint64_t* host);
fhs_status fhs_secret_key_export(fhs_context* ctx, const fhs_secret_key* sk, uint64_t* host /* [L0+P][N] */);
/* Key import in the export layout ("identical Galois keys": a key set made elsewhere, e.g. SEAL's
 * KSwitchKeys with key_vector[j].data(0|1), P = 1).  Residues must be canonical.  Imported keys keep
 * their a_j explicitly (generated keys regenerate them from seeds).  Replaces no pb symbol: the
 * binding had no import; TenSEAL's key loading is the analogue. */
fhs_status fhs_galois_keys_import(fhs_context* ctx, const uint64_t* elts, int n,
                                  const uint64_t* host /* [n][dnum][2][L0+P][N] */, fhs_galois_keys** out);
fhs_status fhs_relin_key_import(fhs_context* ctx, const uint64_t* host /* [dnum][2][L0+P][N] */, fhs_relin_key** out);
fhs_status fhs_secret_key_import(fhs_context* ctx, const uint64_t* host /* [L0+P][N], NTT form */,
                                 fhs_secret_key** out);
/* Key-switch convention: FHS_KS_EXACT (default; exact centred ModUp, ModDown without
 * rounding, hoistable) or FHS_KS_SEAL (P = 1 only: SEAL's switch_key_inplace -- per-limb lift without
 * centring, automorphism before the decomposition, ModDown rounded by adding floor(p/2)). */
#define FHS_KS_EXACT 0
#define FHS_KS_SEAL 1
fhs_status fhs_context_set_key_switch_mode(fhs_context* ctx, int mode);
fhs_status fhs_context_key_switch_mode(const fhs_context* ctx, int* mode);
/* SEAL convention: batched rotations of one ciphertext share one decomposition (the same limbs as SEAL's
 * per-rotation decomposition via a per-(Galois key, level) correction); a digit coefficient
 * equal to 0 falls back to the per-rotation path, and so does a flush whose corrections could not be allocated
 * (out of memory).  Counts of flushes taken each way. */
fhs_status fhs_seal_hoist_stats(fhs_context* ctx, uint64_t* hoisted, uint64_t* fallback);
fhs_status fhs_public_key_export(fhs_context* ctx, const fhs_public_key* pk, uint64_t* host /* [2][L0][N] */);
fhs_status fhs_galois_keys_bytes(const fhs_galois_keys* gk, uint64_t* bytes);

/* ---- objects (pb:157-163) ---- */
fhs_status fhs_ciphertext_destroy(fhs_ciphertext* ct);
fhs_status fhs_plaintext_destroy(fhs_plaintext* pt);
fhs_status fhs_ciphertext_info(const fhs_ciphertext* ct, int* ncomp, int* chain_index, int* nlimbs, double* scale);
fhs_status fhs_ciphertext_set_scale(fhs_ciphertext* ct, double scale);                              /* pb:163 */
fhs_status fhs_plaintext_info(const fhs_plaintext* pt, int* chain_index, int* nlimbs, double* scale);
fhs_status fhs_ciphertext_export(fhs_context* ctx, const fhs_ciphertext* ct, uint64_t* host);
fhs_status fhs_ciphertext_import(fhs_context* ctx, const uint64_t* host, int ncomp, int chain_index, double scale,
                                 fhs_ciphertext** out);
fhs_status fhs_plaintext_export(fhs_context* ctx, const fhs_plaintext* pt, uint64_t* host);
fhs_status fhs_plaintext_import(fhs_context* ctx, const uint64_t* host, int chain_index, double scale,
                                fhs_plaintext** out);
/* device pointer of the limb data (zero-copy interop with torch / RCCL) */
fhs_status fhs_ciphertext_device_ptr(const fhs_ciphertext* ct, void** dptr, uint64_t* bytes);

/* ---- CKKS encoder (pb:128-156) ---- */
/* values: n complex numbers interleaved (re, im); n <= N/2, zero padded.  pb:141-149 */
fhs_status fhs_encode(fhs_context* ctx, const double* re_im, size_t n, double scale, int chain_index,
                      fhs_plaintext** out);
/* batch: count vectors of n complex values each (bg:382 encode_*_vector_batch).
 * Lifetime (every batch creator: encode batches, random_plaintexts, upload_plaintexts, encode_matrix_diagonals):
 * the plaintexts of one call share one device block (a slab of up to 1.5x the request, reused from the cache),
 * returned to the cache only when the LAST of them is destroyed -- keeping one diagonal of a batch keeps the whole
 * batch's HBM, and fhs_context memory_in_use counts the slab as long as any of them lives.  Destroy batches as
 * a whole, or create plaintexts that must outlive their batch with a single-plaintext call. */
fhs_status fhs_encode_batch(fhs_context* ctx, const double* re_im, size_t count, size_t n, double scale,
                            int chain_index, fhs_plaintext** out_array);
/* real-valued fast paths: values are n doubles */
fhs_status fhs_encode_real(fhs_context* ctx, const double* values, size_t n, double scale, int chain_index,
                           fhs_plaintext** out);
fhs_status fhs_encode_real_batch(fhs_context* ctx, const double* values, size_t count, size_t n, double scale,
                                 int chain_index, fhs_plaintext** out_array);
/* pb:150-156 decode: writes N/2 complex (re, im) */
fhs_status fhs_decode(fhs_context* ctx, const fhs_plaintext* pt, double* re_im_out);
/* decode of `count` plaintexts with one device synchronisation (the client's decrypt_vec of a block
 * stage, bg:784-892): the first `nslots` slots of each, re_im_out = count x nslots x (re, im); the same
 * doubles as fhs_decode */
fhs_status fhs_decode_batch(fhs_context* ctx, const fhs_plaintext* const* pts, int count, int nslots,
                            double* re_im_out);

/* ---- encryption (pb:105-116) ---- */
fhs_status fhs_encrypt_symmetric(fhs_context* ctx, fhs_secret_key* sk, const fhs_plaintext* pt, fhs_ciphertext** out);
/* `count` symmetric encryptions in one pass (the client's inputs of a block stage, bg:784-892): the same
 * ciphertexts as `count` fhs_encrypt_symmetric calls in order (each takes the key's next encryption
 * counter); the samplers and NTTs run once over the whole batch */
fhs_status fhs_encrypt_symmetric_batch(fhs_context* ctx, fhs_secret_key* sk, const fhs_plaintext* const* pts, int count,
                                       fhs_ciphertext** out_array);
/* Extension: encode `count` vectors of n values (is_real: n doubles each; else n interleaved (re, im)) at
 * `scale` / `chain_index` and encrypt them with sk in one pass -- the same ciphertexts as
 * fhs_encode[_real]_batch + fhs_encrypt_symmetric_batch (no plaintext objects; count <= 4096) */
fhs_status fhs_encode_encrypt_symmetric_batch(fhs_context* ctx, fhs_secret_key* sk, const double* values, size_t count,
                                              size_t n, int is_real, double scale, int chain_index,
                                              fhs_ciphertext** out_array);
/* Extension: decrypt `count` ciphertexts with sk and decode the first `nslots` slots of each (re_im_out =
 * count x nslots x (re, im)) -- the doubles of fhs_decrypt + fhs_decode_batch, without the plaintexts */
fhs_status fhs_decrypt_decode_batch(fhs_context* ctx, fhs_secret_key* sk, const fhs_ciphertext* const* cts, int count,
                                    int nslots, double* re_im_out);
/* pb:112-116: c0 = u pk0 + e0 + m, c1 = u pk1 + e1 with the key's next encryption counter (the count = 1 case of
 * the batch below) */
fhs_status fhs_encrypt_asymmetric(fhs_context* ctx, fhs_public_key* pk, const fhs_plaintext* pt, fhs_ciphertext** out);
/* `count` public-key encryptions in one pass (the client that holds only the public key: pb:112-116 once per
 * plaintext; ct_ct_search.py:54-90 encrypts its database and its query that way): the same ciphertexts as
 * `count` fhs_encrypt_asymmetric calls in order (each takes the key's next encryption counter).  The small
 * polynomials u, e0, e1 are drawn once per coefficient (not once per limb), and the sampler, the three NTTs and the
 * combine are each one launch over the whole batch instead of seven launches per ciphertext.  On failure nothing stays allocated and
 * out_array is untouched; the counters the call had taken are not given back (a mask stream is never reused) */
fhs_status fhs_encrypt_asymmetric_batch(fhs_context* ctx, fhs_public_key* pk, const fhs_plaintext* const* pts, int count,
                                        fhs_ciphertext** out_array);
/* Extension: encode `count` vectors of n values (is_real: n doubles each; else n interleaved (re, im)) at
 * `scale` / `chain_index` and encrypt them with pk in one pass -- the same ciphertexts as
 * fhs_encode[_real]_batch + fhs_encrypt_asymmetric_batch (no plaintext objects; count <= 4096).  Failure as
 * above: a failed call has used `count` counters */
fhs_status fhs_encode_encrypt_asymmetric_batch(fhs_context* ctx, fhs_public_key* pk, const double* values, size_t count,
                                               size_t n, int is_real, double scale, int chain_index,
                                               fhs_ciphertext** out_array);
fhs_status fhs_decrypt(fhs_context* ctx, fhs_secret_key* sk, const fhs_ciphertext* ct, fhs_plaintext** out);

/* ---- evaluator (pb:165-205); every op returns a NEW object ---- */
fhs_status fhs_add(fhs_context* ctx, const fhs_ciphertext* a, const fhs_ciphertext* b, fhs_ciphertext** out);       /* pb:167 */
fhs_status fhs_sub(fhs_context* ctx, const fhs_ciphertext* a, const fhs_ciphertext* b, int negate, fhs_ciphertext** out); /* pb:173 */
fhs_status fhs_negate(fhs_context* ctx, const fhs_ciphertext* a, fhs_ciphertext** out);                            /* pb:165 */
fhs_status fhs_add_plain(fhs_context* ctx, const fhs_ciphertext* a, const fhs_plaintext* p, fhs_ciphertext** out);  /* pb:169 */
fhs_status fhs_sub_plain(fhs_context* ctx, const fhs_ciphertext* a, const fhs_plaintext* p, fhs_ciphertext** out);  /* pb:175 */
fhs_status fhs_multiply_plain(fhs_context* ctx, const fhs_ciphertext* a, const fhs_plaintext* p, fhs_ciphertext** out); /* pb:181 */
fhs_status fhs_multiply(fhs_context* ctx, const fhs_ciphertext* a, const fhs_ciphertext* b, fhs_ciphertext** out);  /* pb:177 */
fhs_status fhs_relinearize(fhs_context* ctx, const fhs_ciphertext* a, const fhs_relin_key* rk, fhs_ciphertext** out); /* pb:183 */
fhs_status fhs_rescale_to_next(fhs_context* ctx, const fhs_ciphertext* a, fhs_ciphertext** out);                   /* pb:185 */
fhs_status fhs_mod_switch_to_next(fhs_context* ctx, const fhs_ciphertext* a, fhs_ciphertext** out);                /* pb:191-193 */
fhs_status fhs_mod_switch_to(fhs_context* ctx, const fhs_ciphertext* a, int chain_index, fhs_ciphertext** out);    /* pb:198-199 */
fhs_status fhs_plain_mod_switch_to_next(fhs_context* ctx, const fhs_plaintext* a, fhs_plaintext** out);            /* pb:187-189 */
fhs_status fhs_plain_mod_switch_to(fhs_context* ctx, const fhs_plaintext* a, int chain_index, fhs_plaintext** out);/* pb:195-196 */
/* pb:203 rotate: left rotation of the N/2 slots by `step` (bg:219, bg:479) */
fhs_status fhs_rotate(fhs_context* ctx, const fhs_ciphertext* a, int step, const fhs_galois_keys* gk, fhs_ciphertext** out);
/* pb:201 apply_galois with an explicit element */
fhs_status fhs_apply_galois(fhs_context* ctx, const fhs_ciphertext* a, uint64_t elt, const fhs_galois_keys* gk,
                            fhs_ciphertext** out);
/* batch of rotations of possibly different inputs: out[i] = rotate(in[i], steps[i]).  On failure nothing is handed
 * out: out[0..n) are null and the outputs already made are destroyed. */
fhs_status fhs_rotate_many(fhs_context* ctx, const fhs_ciphertext* const* in, const int* steps, int n,
                           const fhs_galois_keys* gk, fhs_ciphertext** out);
/* Extension (fri:71-75): out[i] = x_K, where x_0 = in[i] and x_{k+1} = x_k + rotate(x_k, stride * 2^k),
 * for every k with 2^k < dim. Limb-identical to that loop of fhs_rotate + fhs_add per ciphertext.
 * The batched rotate-and-sum of the slots (ct_pt_dot's tail for every FFN column at once; the server-side slot sum
 * of a retrieval score): per step ONE key switch over all n ciphertexts, its ModDown adding x_k as well, following
 * the context's key-switch mode.  n >= 1, dim >= 1, stride >= 1; dim = 1 copies the inputs; a dim that is no power
 * of two takes the loop's steps (dim = 3: steps 1 and 2); the largest step must be < N/2 (else FHS_ERR_INVALID).
 * Inputs have 2 components (else FHS_ERR_INVALID) and share one chain index (else FHS_ERR_LEVEL); scales may differ,
 * each output keeps its input's scale and chain index.  A Galois key missing for any step is FHS_ERR_KEY, found
 * before anything is allocated or launched.  On failure nothing stays allocated and out_array is untouched.
 * Lifetime: the n results share one device block (as the plaintexts of a batch creator do), returned to the cache
 * when the LAST of them is destroyed.  The inputs are not written and may be destroyed as soon as the call returns. */
fhs_status fhs_inner_sum_many(fhs_context* ctx, const fhs_ciphertext* const* in, int n, int dim, int stride,
                              const fhs_galois_keys* gk, fhs_ciphertext** out_array);

/* ---- fused BSGS (fork-only pyPhantom symbols, bg:459, bg:515) ----
 * Semantics identical, limb for limb, to the loop scripts/bootstrap_generation.py:464-485:
 *   out = rescale( sum_g rot_{gG}( sum_{b: gG+b<D} baby[b] (.) pts[gG+b] ) )
 * baby: G ciphertexts (baby[b] = rot_b(x)); pts: D plaintexts at the baby steps' level. */
fhs_status fhs_bsgs_multiply_accumulate(fhs_context* ctx, const fhs_ciphertext* const* baby, int G,
                                        const fhs_plaintext* const* pts, int D, int B,
                                        const fhs_galois_keys* gk, fhs_ciphertext** out);
/* host staging of pre-encoded diagonals (bg:336-358: offload_plaintexts / upload_plaintexts).
 * host buffer holds count x nlimbs x N uint64 (pinned when allocated by fhs_host_alloc). */
fhs_status fhs_offload_plaintexts(fhs_context* ctx, const fhs_plaintext* const* pts, int count, uint64_t* host);
fhs_status fhs_upload_plaintexts(fhs_context* ctx, const uint64_t* host, int count, int chain_index, double scale,
                                 fhs_plaintext** out_array);
/* bg:449 bsgs_from_cpu: streams diagonals from host memory through the BSGS */
fhs_status fhs_bsgs_from_cpu(fhs_context* ctx, const fhs_ciphertext* const* baby, int G, const uint64_t* host,
                             int D, int B, int chain_index, double scale, const fhs_galois_keys* gk,
                             fhs_ciphertext** out);
fhs_status fhs_host_alloc(uint64_t bytes, void** ptr);   /* pinned host memory */
fhs_status fhs_host_free(void* ptr);

/* ---- CKKS bootstrapping primitives (ckks_bootstrapper, bg:72-74, 110-116, 149-154; tf:243-262;
 * the fork's C++ bootstrapper behind pb is un-vendored) ----
 * Generalised fused BSGS linear transform (CoeffToSlot / SlotToCoeff groups):
 *   out = [rescale]( sum_{g<B} galois_{giant_elts[g]}( sum_{b<G} baby[b] (.) pts[g G + b] ) )
 * D = B * G plaintexts; giant_elts[0] must be 1 (identity group).  rescale = 0 keeps the product
 * scale (baby scale x plaintext scale) and the level. */
fhs_status fhs_linear_transform(fhs_context* ctx, const fhs_ciphertext* const* baby, int G,
                                const fhs_plaintext* const* pts, int D, int B, const uint64_t* giant_elts,
                                const fhs_galois_keys* gk, int rescale, fhs_ciphertext** out);
/* Extension (no reference symbol): the Hadamard half of fhs_bsgs_multiply_accumulate on its own --
 * outs[g] = sum_{b < G} baby[b] (.) pts[g G + b] for g < B (bg:465-476 per giant group), NOT rotated and
 * NOT rescaled (scale baby * pt).  The baby-step-sharded latency mode (fhespear_dist.bsgs_baby_sharded)
 * forms every giant group's partial inner product over a rank's share of the baby steps with it.
 * outs: B new ciphertexts. */
fhs_status fhs_bsgs_inner_products(fhs_context* ctx, const fhs_ciphertext* const* baby, int G,
                                   const fhs_plaintext* const* pts, int B, fhs_ciphertext** outs);
/* Extension (no reference symbol): the giant-step half of fhs_bsgs_multiply_accumulate (bg:478-483):
 * out = sum_j rot_{elts[j]}(inners[j]) for k 2-component ciphertexts at one chain index and scale, the k
 * key switches summed before one ModDown, NOT rescaled.  elts[0] may be 1 (unrotated term); no other.
 * The baby-step-sharded latency mode finishes a rank's giant groups with it.  out: 1 new ciphertext. */
fhs_status fhs_bsgs_giant_steps(fhs_context* ctx, const fhs_ciphertext* const* inners, int k, const uint64_t* elts,
                                const fhs_galois_keys* gk, fhs_ciphertext** out);
/* Extensions (no reference symbol): the two halves over caller device memory, for the grid-sharded
 * latency mode's reduce-scatter buffers -- fhs_bsgs_inner_products writing group g at dst + g 2 l N words,
 * and fhs_bsgs_giant_steps reading term j at src + j 2 l N words (l = L0 + 1 - chain_index).  Both are
 * ordered on the context's stream (fhs_context_stream); the caller orders its own streams around them. */
fhs_status fhs_bsgs_inner_products_device(fhs_context* ctx, const fhs_ciphertext* const* baby, int G,
                                          const fhs_plaintext* const* pts, int B, uint64_t* dst);
fhs_status fhs_bsgs_giant_steps_device(fhs_context* ctx, const uint64_t* src, int k, int chain_index, double scale,
                                       const uint64_t* elts, const fhs_galois_keys* gk, fhs_ciphertext** out);
/* Extension (ct_ct_search.py:92-106, fc:169-194): encrypted dot-product scores of one query against C chunks.
 *   outs[c] = [rescale]( [relinearize]( sum_{j<J} q[j] (x) db[c*J + j] ) ),  c < C
 * limb-identical to  t = multiply(q[0], db[cJ]); t = add(t, multiply(q[j], db[cJ+j])) ...;
 * relinearize(t, rk); rescale_to_next.  rk = NULL: 3-component result.  rescale = 0: product scale kept.
 * Every input has 2 components; all inputs share one chain index (else FHS_ERR_LEVEL), all q one scale and all db
 * one scale (else FHS_ERR_SCALE); J >= 1, 1 <= C <= 21845, J (C + 1) <= 65536; rescale at the last level is
 * FHS_ERR_LEVEL.
 * The relinearization follows the context's key-switch mode.  On failure nothing is left allocated and outs is
 * untouched.  Lifetime: the C results share one device block (as the plaintexts of a batch creator do), returned
 * to the cache when the LAST of them is destroyed. */
fhs_status fhs_dot_product_many(fhs_context* ctx, const fhs_ciphertext* const* q, int J,
                                const fhs_ciphertext* const* db, int C, const fhs_relin_key* rk,
                                int rescale, fhs_ciphertext** outs);
/* Extension (fri:97-108, ct_ct_square per FFN column and ct_ct_multiply per channel): n element-wise products.
 *   out_array[i] = [rescale]( [relinearize]( a[i] (x) b[i] ) ),  i < n
 * limb-identical to fhs_multiply, fhs_relinearize, fhs_rescale_to_next per pair, with ONE tensor launch, ONE batched
 * key switch and ONE rescale launch per chunk of pairs (chunks bound the scratch, not n).  b = NULL squares: b = a.
 * A non-null b[i] may be the same handle as a[i], and a handle may appear in several pairs.  rk = NULL: 3-component
 * results.  rescale = 0: product scale and level kept.  n >= 1; every input has 2 components (else FHS_ERR_INVALID)
 * and all inputs share one chain index (else FHS_ERR_LEVEL); scales may differ per pair: output i has scale
 * a[i].scale * b[i].scale, divided by the dropped prime when rescaled; rescale at the last level is FHS_ERR_LEVEL.
 * The relinearization follows the context's key-switch mode.  On failure nothing stays allocated and out_array is
 * untouched.  Lifetime: the n results share one device block (as the plaintexts of a batch creator do), returned to
 * the cache when the LAST of them is destroyed.  The inputs are not written and may be destroyed as soon as the
 * call returns. */
fhs_status fhs_multiply_relin_many(fhs_context* ctx, const fhs_ciphertext* const* a,
                                   const fhs_ciphertext* const* b, int n, const fhs_relin_key* rk,
                                   int rescale, fhs_ciphertext** out_array);
/* Extension (fri:67-70 for every column at once): out_array[i] = rescale_to_next( multiply_plain( a[i], p[i] ) ), i < n,
 * limb-identical to the two calls per pair, in two launches per chunk with no product stored.
 * p = NULL: out_array[i] = rescale_to_next( a[i] ).
 * n >= 1; every a[i] has 2 components (else FHS_ERR_INVALID); all a[i] and p[i] share one chain index (else
 * FHS_ERR_LEVEL); at the last level the call is FHS_ERR_LEVEL.  A handle may appear any number of times in a or p
 * (ct_pt_dot passes one ciphertext n times).  Output i has scale a[i].scale * p[i].scale / q_{l-1} (p = NULL:
 * a[i].scale / q_{l-1}), computed as the two single calls compute it, and chain index + 1.  Queued rotation outputs
 * used as inputs are flushed first; a lost input is rejected; a compact-only plaintext gets its dense limbs first.
 * Every allocation precedes the first launch of the call's own kernels; on failure nothing stays allocated and
 * out_array is untouched.  The inputs are not written and may be destroyed as soon as the call returns.  Lifetime: the
 * n results share one device block, returned to the cache when the LAST of them is destroyed. */
fhs_status fhs_multiply_plain_rescale_many(fhs_context* ctx, const fhs_ciphertext* const* a,
                                           const fhs_plaintext* const* p, int n, fhs_ciphertext** out_array);
/* Extension (fri:79-94, ct_pt_weighted_sum for every output column at once):
 *   out_array[i] = sum_{j<F} rescale_to_next( multiply_plain( in[j], P_ij ) ),   i < E
 * P_ij: the plaintext at in's chain index and scale `scale` whose every slot is W[j*ldw + i].
 * Limb-identical to the reference's loop -- every term rescaled on its own, then added (not "sum, then one rescale",
 * which gives other limbs) -- in a constant number of launches per chunk of outputs, whatever F and E.  P_ij is the
 * constant polynomial c_ij = round(W[j*ldw + i] * scale), half away from zero (fhs_multiply_const's rounding); its NTT
 * image is c_ij mod q_m in every position of limb m, which is what an exact encoder gives for a constant vector.  The
 * GPU's float64 encoder (fhs_encode*) can differ from it where W * scale lies within its FFT error of a half-integer.
 * Result i has scale in.scale * scale / q_{l-1} and chain index + 1.  Inputs have 2 components (else
 * FHS_ERR_INVALID), share one chain index (else FHS_ERR_LEVEL) and one scale as fhs_add judges it (else
 * FHS_ERR_SCALE); 1 <= F <= 4096, E >= 1, ldw >= E, `scale` finite and > 0, every weight finite with
 * |c_ij| < 2^62 (else FHS_ERR_INVALID); at the last level the call is FHS_ERR_LEVEL.  A handle may appear several
 * times in `in`.  Queued rotation outputs used as inputs are flushed first; a lost input is rejected.  The inputs are
 * not written and may be destroyed as soon as the call returns.  Every allocation precedes the first launch; on
 * failure nothing stays allocated and out_array is untouched.  Lifetime: the E results share one device block,
 * returned to the cache when the LAST of them is destroyed. */
fhs_status fhs_weighted_sums(fhs_context* ctx, const fhs_ciphertext* const* in, int F,
                             const double* W, int64_t ldw, int E, double scale,
                             fhs_ciphertext** out_array);
/* Extension (no reference symbol): bg:198-203 + bg:361-432 on the device -- the D diagonals of the
 * D x D row-major matrix M1 (complex: M1 + i M2; M2 = NULL for real), group g = k / G rolled by g G,
 * tiled to N/2 slots, encoded at `scale` / `chain_index`.  Limb-identical to encode_*_vector_batch
 * of the host-prepared rows; uploads D^2 doubles instead of D x N/2.  out_array: D plaintexts. */
fhs_status fhs_encode_diagonals(fhs_context* ctx, const double* M1, const double* M2, int D, int G, double scale,
                                int chain_index, fhs_plaintext** out_array);
/* the same for a strided or transposed view: row r of the D x D block starts at A + r * ld (ld >= D);
 * trans = 1 means the block holds M^T (M[m][c] = A[c * ld + m]), e.g. numpy's W[:, lo:hi].T */
fhs_status fhs_encode_diagonals_ex(fhs_context* ctx, const double* A1, const double* A2, int64_t ld, int trans, int D,
                                   int G, double scale, int chain_index, fhs_plaintext** out_array);
/* only the diagonals rows[0..nrows) (indices < D, any order; out_array[k] is diagonal rows[k]): the rows one
 * rank of a sharded matvec needs (fhespear_dist giant_groups / grid_rows) -- limb-identical to the same
 * plaintexts of the full encode */
fhs_status fhs_encode_diagonals_rows(fhs_context* ctx, const double* A1, const double* A2, int64_t ld, int trans, int D,
                                     int G, double scale, int chain_index, const int* rows, int nrows,
                                     fhs_plaintext** out_array);
/* encode_complex_vector_batch with an extended-precision (long double) canonical-embedding FFT on the
 * host and exact 128-bit rounding: for constant plaintexts whose f64 encoding error (~2^-52 log n
 * relative) matters -- the bootstrap's CoeffToSlot / SlotToCoeff diagonals.  |values x scale| < 2^126. */
fhs_status fhs_encode_precise(fhs_context* ctx, const double* re_im, size_t count, size_t n, double scale,
                              int chain_index, fhs_plaintext** out_array);
/* out = a * c with the integer c = round(value * const_scale) (half away from zero, exact for any
 * finite double); out scale = a.scale * const_scale */
fhs_status fhs_multiply_const(fhs_context* ctx, const fhs_ciphertext* a, double value, double const_scale,
                              fhs_ciphertext** out);
/* out = a + round(value * a.scale) (added to component 0; scale unchanged) */
fhs_status fhs_add_const(fhs_context* ctx, const fhs_ciphertext* a, double value, fhs_ciphertext** out);
/* ModRaise: limb q0 of a (any level) lifted centred to all L0 data limbs; out at chain index 1,
 * same scale (decrypts to m + q0 I) */
fhs_status fhs_mod_raise(fhs_context* ctx, const fhs_ciphertext* a, fhs_ciphertext** out);
/* ckks_bootstrapper EvalMod (pyPhantom/bootstrap.py Bootstrapper._evalmod, the same op sequence):
 * cos / sin Chebyshev series cc, cs (ncoef coefficients each, scale-exact split, landing at chain
 * index y + cheb_depth at y's scale) on one basis, then r complex squarings; out = sin(2 pi K y) */
fhs_status fhs_bootstrap_evalmod(fhs_context* ctx, const fhs_ciphertext* y, const fhs_relin_key* rk,
                                 const double* cc, const double* cs, int ncoef, int r, int cheb_depth,
                                 fhs_ciphertext** out);

/* ---- measurement hooks (bench.py) ---- */
/* fill n plaintexts with i.i.d. uniform limbs mod q_i (SURVEY.md §8d throughput workload) */
fhs_status fhs_random_plaintexts(fhs_context* ctx, uint64_t seed, int count, int chain_index, double scale,
                                 fhs_plaintext** out_array);
/* HIP events on the context stream: record returns an opaque id usable with fhs_event_elapsed */
fhs_status fhs_event_record(fhs_context* ctx, void** ev);
fhs_status fhs_event_elapsed(void* start, void* stop, float* ms);
fhs_status fhs_event_destroy(void* ev);
/* Per-kernel device time from HIP events recorded on the context stream around each launch.
 * Kernel ids: 0 k_bsgs_inner (ct x pt Hadamard-accumulate), 1 k_modup (ModUp + NTT), 2 k_ks_ip
 * (key inner product), 3 k_moddown, 4 k_ks_intt, 5 k_ks_special_intt, 6 k_giant_sum,
 * 7 k_giant_final, 8 rescale, 9 k_dot_tensor (ct x ct dot-product tensor sums), 10 encrypt_pk
 * (public-key encryption: the sampler, NTT and combine launches of a batch).  arm(mask) enables
 * ids (bit i); timer() reports kernel_id's accumulated ms / launch count and optionally resets every
 * accumulator. */
fhs_status fhs_kernel_timer_arm(fhs_context* ctx, uint32_t mask);
fhs_status fhs_kernel_timer(fhs_context* ctx, int kernel_id, float* ms, int* launches, int reset);
/* device-to-device copies of ciphertext limbs to / from caller-owned HBM (RCCL gather in bench.py) */
fhs_status fhs_ciphertext_copy_to_device(fhs_context* ctx, const fhs_ciphertext* ct, void* dst);
fhs_status fhs_ciphertext_from_device(fhs_context* ctx, const void* src, int ncomp, int chain_index, double scale,
                                      fhs_ciphertext** out);
/* Stream-ordered variants for callers that order their own streams against the context stream
 * (fhespear_dist: torch / RCCL buffers): the copy is enqueued on the context stream and the call
 * returns without waiting; the caller makes the context stream wait for the buffer's producer and
 * its own stream wait for the copy (HIP events; torch.cuda.ExternalStream on fhs_context_stream). */
fhs_status fhs_ciphertext_copy_to_device_async(fhs_context* ctx, const fhs_ciphertext* ct, void* dst);
fhs_status fhs_ciphertext_from_device_async(fhs_context* ctx, const void* src, int ncomp, int chain_index,
                                            double scale, fhs_ciphertext** out);
/* the context's HIP stream (hipStream_t), on which every library call is ordered */
fhs_status fhs_context_stream(fhs_context* ctx, void** stream);
/* staging-ring statistics: how often the pinned descriptor ring re-entered a segment, and how many of
 * those re-entries had to wait for the GPU (should stay 0: the host never drains the queue) */
fhs_status fhs_staging_stats(fhs_context* ctx, uint64_t* reentries, uint64_t* blocked);
/* Host-side diagnostic of the device reduction arithmetic (no GPU needed): reduces hi:lo mod q with
 * the pseudo-Mersenne folds the kernels use when q qualifies (*pm_used = 1), else *pm_used = 0 and
 * *out = (hi:lo) mod q.  Exists so the CPU test suite can check the fold bounds against big ints. */
fhs_status fhs_debug_reduce128(uint64_t q, uint64_t lo, uint64_t hi, uint64_t* out, int* pm_used);
/* Test hook: ModUp's X form (k_centered_x + modup_convert3x arithmetic, run on the host) of the 3-limb
 * digit residues y3 over primes q3 into target prime m; *out = the centred digit value mod m. */
fhs_status fhs_debug_modup_xform(const uint64_t* q3, const uint64_t* y3, uint64_t m, uint64_t* out);
/* Test hook: ModDown's X form (k_special_x + moddown_convert3x arithmetic, on the host): special residues y3
 * over primes p3 (< 2^59) into target prime q; *out = (sum_k y3[k] P/p3[k]) mod q. */
fhs_status fhs_debug_moddown_xform(const uint64_t* p3, const uint64_t* y3, uint64_t q, uint64_t* out);
/* Test hook: k_dot_tensor's per-coefficient schedule (split-30 accumulate, Acc3 folds, 128-bit sums, one reduction
 * per sum, windows of 64 terms adding their reduced sums -- the kernel's own __host__ __device__ routines) run on
 * the host for one coefficient of prime q < 2^60: out3 = (sum a0 b0, sum a0 b1 + a1 b0, sum a1 b1) mod q over J
 * terms.  Operands must be < q. */
fhs_status fhs_debug_dot_accumulate(uint64_t q, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                    const uint64_t* b1, int J, uint64_t* out3);
/* Test hooks: the per-coefficient routines of fhs_weighted_sums' two pointwise stages (the kernel's own
 * __host__ __device__ routines) run on the host.  round: the rounding sum S = sum_j centre(k[j] d[j] mod qL),
 * centre(u) = ((u + (qL >> 1)) mod qL) - (qL >> 1), as the signed 128-bit integer *hi 2^64 + *lo.  accumulate:
 * *out = (sum_j kprime[j] c[j] + wT t) mod q with split-30 partial sums, Acc3 folds and one reduction per window of
 * 64 products.  q odd and < 2^60, operands < q, 1 <= F <= 4096. */
fhs_status fhs_debug_wsum_round(uint64_t qL, const uint64_t* k, const uint64_t* d, int F, int64_t* hi, uint64_t* lo);
fhs_status fhs_debug_wsum_accumulate(uint64_t q, const uint64_t* kprime, const uint64_t* c, int F, uint64_t wT,
                                     uint64_t t, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif
