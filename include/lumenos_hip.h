/*
 * lumenos_hip.h -- C ABI of the MI355X-native (gfx950) server-side homomorphic
 * Ligero prover.  This is the drop-in boundary: plain pointers and sizes, no
 * C++/torch types.  Every entry point names the reference interface it
 * replaces (paths relative to the ChainSafe/lumenos tree; Lattigo calls are
 * the ones made at those lines).  The Go-side cgo binding a maintainer would
 * add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - return value: 0 = OK, non-zero = error; lumen_last_error() gives text
 *     (the reference's cgo convention in vdec/prover.go:121-232 is mirrored:
 *     Create/Destroy pairs, opaque handles checked for NULL).
 *   - residues are canonical u64 in [0, q_i), NTT domain, non-Montgomery --
 *     exactly what rlwe.Ciphertext.Value[k].Coeffs[i] holds.
 *   - a ciphertext is [poly(2)][limb(nl)][N] u64; a "set" is an HBM-resident
 *     array [ct][poly][limb][N].  Host buffers passed in/out use the same
 *     layout (the Go shim stages Lattigo's per-limb slices into it).
 *   - threading: every entry point that takes a context locks it, so
 *     concurrent calls on ONE context are safe and run one after the other
 *     (host side and on the context's HIP stream).  To run concurrently -- the
 *     reference evaluates the R and Z inner products on two goroutines
 *     (fhe/ligero.go:231-242), each with its own backend.CopyNew() -- give each
 *     goroutine pool a lumen_ctx_clone(): clones share parameters, twiddles,
 *     field table and keys (read-only, like Evaluator.ShallowCopy) and own their
 *     streams, scratch and storage pool.  A set may be read by any context of
 *     the same device (lumen_sync the producer first); it is destroyed through
 *     the context that created it.  Configuration calls (lumen_field_set,
 *     lumen_load_*_key, lumen_encoder_set, lumen_leaf_format_set) must not race
 *     with compute calls on a clone of the same context.
 *   - calls return after the work is enqueued unless they hand back host data;
 *     lumen_sync() waits.
 */
#ifndef LUMENOS_HIP_H
#define LUMENOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LUMEN_ABI_VERSION 4
#define LUMEN_MAX_LIMBS 24

typedef struct lumen_ctx lumen_ctx;
typedef struct lumen_set lumen_set;
typedef struct lumen_group lumen_group;

/* What fhe.NewBackendBFV (fhe/bfv.go:23-28) captures from bgv.Parameters:
 * ring degree, the Q and P moduli chains, the plaintext modulus, and for
 * every modulus the primitive 2N-th root psi its NTT tables are built from
 * (Lattigo: SubRing.RootsForward; standard form here). */
typedef struct lumen_params_desc {
    uint32_t abi_version; /* LUMEN_ABI_VERSION */
    uint32_t log_n; /* 8, 10 .. 14: every entry point; 15: transforms, rescale, products, Encode / Commit / gather / wire
                     * format, key loading, InnerSum, rotations, relinearisation -- lumen_keygen_*, lumen_encrypt_*,
                     * lumen_ct_expand_seeded, lumen_decrypt, lumen_verify_columns, lumen_batch_ciphertexts,
                     * lumen_vdec_witness and lumen_ring_switch fail there with an error that names the degree */
    uint32_t num_q; /* L */
    uint32_t num_p; /* K (alpha) */
    uint64_t plaintext_modulus;
    uint64_t moduli[LUMEN_MAX_LIMBS]; /* q_0..q_{L-1}, p_0..p_{K-1} */
    uint64_t psi[LUMEN_MAX_LIMBS];    /* primitive 2N-th root per modulus */
    int32_t device;                   /* HIP device ordinal */
} lumen_params_desc;

/* ---- context: replaces fhe.ServerBFV / NewBackendBFV / CopyNew (fhe/bfv.go:13-58) */
int lumen_ctx_create(const lumen_params_desc *desc, lumen_ctx **out);
void lumen_ctx_destroy(lumen_ctx *ctx);
/* ServerBFV.CopyNew (fhe/bfv.go:56-58: Evaluator.ShallowCopy per goroutine, fhe/ligero.go:142,315):
 * a context on the same device that shares src's tables and keys and owns its streams and scratch.
 * Destroy clones and source in any order; the shared tables go with the last one. */
int lumen_ctx_clone(lumen_ctx *src, lumen_ctx **out);
/* ctx's stream waits -- on the device, the host does not block -- for everything enqueued so far on `other`
 * (same device): the hand-over between a producer context and the clone that serialises / downloads its
 * results while the producer goes on (the reference's R and Z goroutines, fhe/ligero.go:231-242). */
int lumen_ctx_wait(lumen_ctx *ctx, lumen_ctx *other);
/* The library's tuning switches (A/B tools; every default is the measured best; DESIGN.md "Run-time
 * switches") are read from the environment ONCE, by lumen_ctx_create; clones inherit them.  This setter is
 * the in-process form for tests and tools: name = "LUMEN_KS_BATCH", "LUMEN_KS_LANES",
 * "LUMEN_KS_PAIR" (1: on one lane lumen_inner_sum / lumen_matrix_inner_sum send two consecutive batches through a rotation
 * as one pair; 0: single batches; 2: pairs with the second half extended first, for measurements; value < 0: by ring
 * degree, the default -- 1 at LogN 14; same residues),
 * "LUMEN_KS_FUSED_DIGITS" (value < 0: derived default), "LUMEN_KS_CLOSE_FUSED" (1, the default: the last rotation of
 * lumen_matrix_inner_sum writes the rescale's coefficient-form input itself; 0: ModDown and the whole rescale; same
 * residues), "LUMEN_KS_C0_FOLD" (1, the default: on that route the doublings before the last rotation run ModDown for
 * polynomial 1 alone and polynomial 0's lifts are taken once, at the close; 0: ModDown for both; same residues),
 * "LUMEN_DEBUG", "LUMEN_MODUP_TGROUP",
 * "LUMEN_MODDOWN_TGROUP" (work-list order of the key switch's two transform kernels), "LUMEN_KS_PLACEMENT" (candidate
 * blocks per key-switch scratch buffer among which a context's first key switch picks by measurement, 0 = none:
 * takes effect when the buffers are next allocated, e.g. after lumen_ctx_trim), "LUMEN_BATCH_CHUNKS" (chunks of columns
 * per limb in lumen_batch_ciphertexts, 0 .. 4096, 0 = derived from the CU count; the residues do not depend on it),
 * "LUMEN_DOT_PAIRS" (coefficient pairs per block of the dot product's tensor kernel, 256 or 512, 0 = by the size of the
 * launch; same residues), "LUMEN_DOT_PARTS" (blocks the terms of one sum are split over there, 1 .. 256, 0 = by the size
 * of the launch; same residues), "LUMEN_ALLOC_FILL" (a testing mode; 0, the default: off, nothing changes; 1 .. 255:
 * every device block the library draws from then on -- tables, keys, temporaries, scratch, set storage, fresh or out of
 * the pool -- is filled with this byte before its first use and, when freshly drawn, has a 4 KiB guard band of another
 * byte behind it; setting a non-zero value on a live context, the current one as well, waits for the context's
 * streams and fills every scratch buffer and pooled block again, and is refused while a lumen_leaf_digests_begin job
 * is in flight; results must not depend on it; see lumen_ctx_alloc_check).  An
 * unknown name or a value out of a switch's range is an error and changes nothing. */
int lumen_ctx_set_tuning(lumen_ctx *ctx, const char *name, long value);
/* TEST HOOK (not a tuning switch, never read from the environment): lumen_group_create then lets LUMEN_TRANSPORT_RCCL
 * through although ranks share a device, so that the library's RCCL call sequence can be run with W > 1 on a one-GPU
 * box against the test double tests/cpp/fake_rccl.cpp (real RCCL refuses such a communicator). */
int lumen_test_allow_shared_device_rccl(lumen_ctx *ctx, int on);
/* Freed set storage is pooled per context and scratch buffers persist (a prover run allocates the same sizes
 * every time; mapping 25 GB per call costs 0.2 s).  lumen_ctx_trim hands all of it back to the driver -- between
 * jobs of different shapes, or when several contexts share one GPU.  Waits for the context's work first. */
int lumen_ctx_trim(lumen_ctx *ctx);
const char *lumen_last_error(const lumen_ctx *ctx); /* ctx may be NULL */
int lumen_sync(lumen_ctx *ctx);
/* number of ct x scalar multiplications issued: ServerBFV.MulCounter (bfv.go:44-46) */
uint64_t lumen_mul_counter(const lumen_ctx *ctx);

/* ---- HBM-resident ciphertext sets ([]*rlwe.Ciphertext on the Go side) */
int lumen_set_create(lumen_ctx *ctx, uint32_t count, uint32_t num_limbs, lumen_set **out);
void lumen_set_destroy(lumen_ctx *ctx, lumen_set *set);
uint32_t lumen_set_count(const lumen_set *set);
uint32_t lumen_set_limbs(const lumen_set *set);
/* non-owning view of ciphertexts [first, first+n) of `set` (a Go sub-slice
 * matrix[a:b]); destroy the view before the parent */
int lumen_set_slice(lumen_ctx *ctx, const lumen_set *set, uint32_t first, uint32_t n,
                    lumen_set **view);
/* device pointer of the set's storage (for callers that own HIP interop) */
void *lumen_set_device_ptr(const lumen_set *set);
/* Host <-> device staging.  The Go shim's stage() copies Lattigo's per-limb slices
 * (ct.Value[k].Coeffs[i]) into ONE flat buffer anyway: allocate that buffer with
 * lumen_host_alloc (page-locked) and upload/download move it by DMA with no further copy.  Ordinary
 * (pageable) host pointers are accepted too and are pipelined through two pinned bounce buffers of the
 * context.  Both calls return when the host buffer may be reused / holds the data. */
void *lumen_host_alloc(size_t bytes);
void lumen_host_free(void *p);
/* The staging copy itself, for a host that cannot avoid it: `limbs` = n separately allocated arrays of `words`
 * u64 each (Lattigo: ct.Value[k].Coeffs[i], pinned with runtime.Pinner and listed in a C array, in the order
 * [ct][poly][limb]); ONE call gathers them into the flat buffer (scatter: the way back) on `threads` host
 * threads (0: min(16, cores)) -- a single goroutine's copy() loop moves ~10 GB/s, the PCIe link ~55.
 * INTEGRATION.md section 2 shows how to make the copy disappear instead (limb slices that alias one
 * lumen_host_alloc block). */
int lumen_host_gather(uint64_t *dst, const uint64_t *const *limbs, size_t n, size_t words, uint32_t threads);
int lumen_host_scatter(const uint64_t *src, uint64_t *const *limbs, size_t n, size_t words, uint32_t threads);
int lumen_set_upload(lumen_ctx *ctx, lumen_set *set, uint32_t first, uint32_t n,
                     const uint64_t *host);
int lumen_set_download(lumen_ctx *ctx, const lumen_set *set, uint32_t first, uint32_t n,
                       uint64_t *host);
/* synthetic input: residues uniform in [0,q_i) from a counter-based RNG
 * (benchmark inputs) */
int lumen_set_fill_random(lumen_ctx *ctx, lumen_set *set, uint64_t seed);

/* ---- polynomial NTT per limb: Lattigo SubRing.NTT / INTT as used inside
 * Rescale and key-switching.  In place on every limb of
 * every ciphertext of the set.  inverse: 0 = NTT, 1 = INTT. */
int lumen_set_ntt(lumen_ctx *ctx, lumen_set *set, int inverse);

/* ---- plaintext field table: backend.Field().RootForwardUint64(i)
 * (core/field.go:45-47), fieldN = 2*cols entries, raw Montgomery-form words. */
int lumen_field_set(lumen_ctx *ctx, const uint64_t *roots_forward, uint32_t field_n);

/* ---- fhe.NTT(values, size, backend) (fhe/ntt.go:12-18): in place on the set,
 * including the final ciphertext permutation the Go pointer swaps produce. */
int lumen_ct_ntt(lumen_ctx *ctx, lumen_set *values, uint32_t size);

/* ---- fhe.Encode(matrix, rows, rhoInv, backend) (fhe/code.go:8-34).
 * zero_ct: the one fresh encryption of the zero vector (code.go:15-22), made by
 * the host Encryptor, host layout [2][nl][N].  Returns a new set of
 * cols*rho_inv ciphertexts; `matrix` is not modified. */
int lumen_encode(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *zero_ct,
                 uint32_t rho_inv, lumen_set **encoded);

/* ---- multi-GPU Commit: the same transform, of which rank `rank` of `world` keeps only the encoded
 * columns its share of the final pass produces (every rank holds the whole input matrix; no exchange
 * is needed before the leaf digests are all-gathered).  col_index: room for cols*rho_inv entries;
 * receives the global indices (ascending) of the *n_cols columns returned in `encoded`. */
int lumen_encode_shard(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *zero_ct,
                       uint32_t rho_inv, uint32_t rank, uint32_t world, lumen_set **encoded,
                       uint32_t *col_index, uint32_t *n_cols);

/* ---- multi-GPU Commit, lane-sharded: the ciphertext-axis transform never mixes lanes, so rank g
 * of W = 2^log_world encodes coefficients [g*N/W, (g+1)*N/W) of every limb of EVERY ciphertext (a "lane
 * shard": a set whose limbs are N/W words wide), and owns whole ciphertexts of a contiguous block of
 * columns everywhere else.  Per step and rank: two all-to-alls over xGMI, done by the host with RCCL on the
 * sets' device pointers -- both layouts are ct-major, so every block that travels is a contiguous slice:
 *     own input columns --lumen_lanes_split--> W blocks --all-to-all--> lane shard of all columns
 *     --lumen_encode (on the lane shard, with the same slice of the one Enc(0))--> lane shard of the S
 *     encoded columns --all-to-all--> W blocks of own encoded columns --lumen_lanes_assemble--> full width.
 * A rank uploads 1/W of the matrix and no work is replicated.  Lane sets are accepted by create /
 * destroy / slice / upload / download / fill_random / gather, lumen_encode and the elementwise lumen_add / _sub /
 * _mul_scalar / _mul_scalar_then_add / _linear_combination only.
 * These are the building blocks; a host program uses the group entry points further down
 * (lumen_group_encode runs the whole sequence, exchange included, inside the library). */
int lumen_set_create_lanes(lumen_ctx *ctx, uint32_t count, uint32_t num_limbs, uint32_t log_world, lumen_set **out);
uint32_t lumen_set_log_world(const lumen_set *set);
/* full-width columns [n] -> lane set of W*n ciphertexts, block g (lane ciphertexts [g*n, (g+1)*n)) for rank g */
int lumen_lanes_split(lumen_ctx *ctx, const lumen_set *columns, uint32_t log_world, lumen_set **lanes);
/* lane set of W*n ciphertexts, block g received from rank g -> full-width columns [n] */
int lumen_lanes_assemble(lumen_ctx *ctx, const lumen_set *lanes, lumen_set **columns);

/* ---- Evaluator.Rescale looped `for ct.Level() > target` (fhe/ligero.go:149-155,
 * 271-273, 331-333).  out is a new set with target_limbs limbs. */
int lumen_rescale(lumen_ctx *ctx, const lumen_set *in, uint32_t target_limbs, lumen_set **out);

/* ---- rlwe.Ciphertext.WriteTo (fhe/ligero.go:156-157 for the leaves, 664-691 for the proof) as a layout
 *     head | for each polynomial: poly_head | for each limb: limb_head | N little-endian u64
 * The three byte strings are cut by the host out of ONE real ct.WriteTo of a ciphertext of the level
 * being serialised (INTEGRATION.md section 4 shows the Go code): they hold Lattigo's MetaData block
 * and the length words of structs.Vector / structs.Matrix, which this library does not hard-code.
 * All three NULL: back to the default, the recalled framing with an empty MetaData block
 * (head = LE64(2), poly_head = LE64(limbs), limb_head = LE64(N)) -- NOT byte-compatible with a
 * Lattigo peer; a root computed under it verifies only against this library's own serialisation.
 * lumen_ct_serialize writes ciphertexts [first, first+n) of a set in the current format into `out`
 * (n * lumen_ct_serialized_size(ctx, limbs) bytes): the proof marshaller (EncryptedProof.WriteTo,
 * fhe/ligero.go:659-705, is metadata | MatR | MatZ | QueriedCols | paths | root with every ciphertext through
 * ct.WriteTo), and the shim's one-off byte comparison with Lattigo before it trusts device digests.
 * The wire image is assembled on the device and crosses PCIe as contiguous DMA: hand it page-locked
 * memory (lumen_host_alloc; a Go []byte over it feeds the HTTP response with no further copy).
 * lumen_ct_serialize_async is the same without the wait: `out` must be page-locked, the bytes are valid
 * after lumen_sync(ctx) -- call it on a lumen_ctx_clone to move MatR while MatZ is computed. */
int lumen_leaf_format_set(lumen_ctx *ctx, const uint8_t *head, uint32_t head_len, const uint8_t *poly_head,
                          uint32_t poly_head_len, const uint8_t *limb_head, uint32_t limb_head_len);
size_t lumen_ct_serialized_size(lumen_ctx *ctx, uint32_t num_limbs);
int lumen_ct_serialize(lumen_ctx *ctx, const lumen_set *set, uint32_t first, uint32_t n, uint8_t *out,
                       size_t cap);
int lumen_ct_serialize_async(lumen_ctx *ctx, const lumen_set *set, uint32_t first, uint32_t n, uint8_t *out,
                             size_t cap);
/* The way back: EncryptedProof.ReadFrom (fhe/ligero.go:707-753: rlwe.Ciphertext.ReadFrom for every entry of MatR,
 * MatZ and the queried columns).  `bytes`: n serialised ciphertexts of num_limbs limbs back to back in the current
 * format (len = n * lumen_ct_serialized_size).  The image crosses PCIe as it is and is taken apart on the
 * device into a new set -- what a client that owns a GPU feeds to lumen_decrypt.  The format's byte strings
 * are compared with the image: any difference (another level or ring degree, a corrupt proof) is an error. */
int lumen_ct_deserialize(lumen_ctx *ctx, const uint8_t *bytes, size_t len, uint32_t n, uint32_t num_limbs,
                         lumen_set **out);

/* ---- leaves of the commitment: serialize every ciphertext of a level-1 set in the current format
 * (ct.WriteTo, fhe/ligero.go:156-157) and SHA-256 it (core/tree.go:96-111).
 * digests: host buffer, count*32 bytes. */
int lumen_leaf_digests(lumen_ctx *ctx, const lumen_set *level1, uint8_t *digests);
/* The same, split in two so that the caller can overlap it with the inner products: Prove does
 * not write the root to the transcript before sampling r (fhe/ligero.go:198-199), so nothing of
 * matrixInnerSumEval depends on the leaves.  _begin enqueues the hashing of `level1` on a side
 * stream of the context, behind everything already enqueued, and returns; `level1` must stay alive
 * and unmodified until _end, which waits and writes count*32 bytes.  One job in flight per context. */
int lumen_leaf_digests_begin(lumen_ctx *ctx, const lumen_set *level1);
int lumen_leaf_digests_end(lumen_ctx *ctx, uint8_t *digests);
/* the same job ended without bringing the digests to the host: *dev_digests = count*32 bytes of device
 * memory (valid until the next _begin), what an RCCL all-gather reads; and core.NewTree's root over
 * digests that sit in device memory (the all-gathered leaves): only the root crosses PCIe */
int lumen_leaf_digests_end_device(lumen_ctx *ctx, void **dev_digests);
int lumen_merkle_root_device(lumen_ctx *ctx, const void *dev_leaf_digests, uint32_t n_leaves, uint8_t *root);
/* core.NewTree over leaf digests (core/tree.go:113-163): nodes = all levels,
 * bottom-up, (returns node count through n_nodes); root: 32 bytes. */
int lumen_merkle_build(lumen_ctx *ctx, const uint8_t *leaf_digests, uint32_t n_leaves,
                       uint8_t *nodes, size_t nodes_cap, size_t *n_nodes, uint8_t *root);

/* ---- server-side witness encryption: server.EncryptNew per column
 * (cmd/server/main.go:199-208; fhe/bfv.go:13-58 holds the rlwe.Encryptor with the public key).
 * pk: [2][L+K][N], NTT domain, over the whole basis QP -- rlwe.PublicKey.Value[0..1] are ringqp.Poly
 * {Q, P}: flatten the Q limbs then the P limbs of each.  Encryption follows rlwe.Encryptor.encryptZeroPk
 * [LATTIGO-RECALL]: u*pk_w + e_w is formed over QP and divided by P (ModDownQPtoQ), which leaves a
 * fresh noise of a few units; fhe.Encode's unrescaled scalar multiplications need that.
 * plaintexts: host, [count][L][N] NTT-domain RNS plaintexts as Encoder.Encode leaves them
 * (m * T^-1 form), or NULL for encryptions of zero (fhe/code.go:21-25).
 * The reference's encryption is randomised; this one is deterministic in (seed, first_index + i):
 * ciphertext i draws its ternary u and Gaussian e0, e1 from ChaCha20(seed, first_index + i), so a
 * column encrypts to the same bits on whichever GPU it lands.  The seed is key material: take it from
 * the OS CSPRNG (crypto/rand).  out: new set of `count` ciphertexts at the top level. */
int lumen_load_public_key(lumen_ctx *ctx, const uint64_t *pk);
/* The same from the raw witness: Encoder.Encode + EncryptNew for `count` columns of `rows` slot
 * values each (cmd/server/main.go:188-208), host [count][rows]; 8*rows bytes cross PCIe per column
 * instead of the 8*L*N of an encoded plaintext.  lumen_encoder_set hands over the primitive 2N-th
 * root of unity modulo T of the encoder's Z_T ring (Lattigo: params.RingT()), like `psi` for the
 * limbs.  Encoding [LATTIGO-RECALL bgv.Encoder]: slot i of row 0 at the evaluation point 5^i, row 1
 * at -5^i; INTT over Z_T; scale by T^-1 mod q_l; NTT (fused here into the encryption's transforms). */
int lumen_encoder_set(lumen_ctx *ctx, uint64_t psi_t);
int lumen_encrypt_values(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count,
                         const uint8_t seed[32], uint64_t first_index, lumen_set **out);
int lumen_encrypt_pk(lumen_ctx *ctx, const uint64_t *plaintexts, uint32_t count, const uint8_t seed[32],
                     uint64_t first_index, lumen_set **out);

/* ---- P(z) over a block of witness columns (cmd/server/main.go:255-258, core/poly.go:13-45): the claimed value the
 * server answers GET /prove?point=z with next to the proof, which the client checks as InnerProduct(MatZ, a) == value,
 * a = [1, z, z^2, ...] (fhe/ligero.go:569).  P = core.NewDensePolyFromMatrix(matrix): the witness flattened row-major,
 * coefficient i*cols + j = M[i][j].  values: host, `count` columns of `rows` values each, [count][rows] -- exactly what
 * lumen_encrypt_values takes -- of which the first is column `first_column` of a matrix of `cols` columns:
 *     partial = sum_{j<count} sum_{i<rows} (values[j][i] mod T) * z^(i*cols + first_column + j)   (mod T)
 * T is the context's plaintext modulus; values >= T count as their residue, as in lumen_encrypt_values.  The partials
 * of disjoint column blocks sum mod T to P(z), so a caller batches the columns as it batches lumen_encrypt_values.
 * One pass over the 8*rows*count bytes on the device (page-locked values: lumen_host_alloc; pageable ones are
 * bounced).  Refused with a message: rows outside [1, N], first_column + count > cols, a context without a
 * plaintext modulus (or one of 2^60 and more), NULL pointers. */
int lumen_poly_eval_columns(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count,
                            uint64_t first_column, uint32_t cols, uint64_t z, uint64_t *partial);

/* ---- client-side decryption of the proof's ciphertexts: EncryptedProof.Decrypt /
 * decryptBatchedParallel (fhe/ligero.go:381-502, 577-636) = Decryptor.DecryptNew + Encoder.Decode.
 * For a client that owns a GPU and for end-to-end tests: the proving server never holds sk.
 * sk: [L][N], NTT domain.  set: ciphertexts at any level (level <= 1 is what Prove returns; deeper ones,
 * e.g. the unrescaled output of Encode that TestEncode decrypts, go through an exact mixed-radix CRT).
 * scale: the ciphertexts' Scale, i.e. the product of the dropped moduli's inverses modulo T that the
 * rescales left behind (1 if none); values: host, [count][nvalues] slot values.
 * Needs lumen_encoder_set. */
int lumen_load_secret_key(lumen_ctx *ctx, const uint64_t *sk);
int lumen_decrypt(lumen_ctx *ctx, const lumen_set *set, uint64_t scale, uint32_t nvalues, uint64_t *values);

/* ---- the client's check of the opened columns: the per-column loop of Proof.Verify (fhe/ligero.go:554-567) over
 * the `count` opened level-1 ciphertexts of `opened` (what lumen_ct_deserialize or lumen_gather produced), on a
 * context that holds the secret key and encoder tables.  For every column i, without its values leaving the device:
 *   core.VerifyMerklePath(Ct_i, paths[i], root, leaf_index[i]) (core/tree.go:225-268): the leaf is SHA-256 of the
 *     ciphertext in the CONTEXT's serialisation format (lumen_leaf_format_set), hashed up `depth` siblings,
 *     cur = H(cur | sib) for an even running index, H(sib | cur) for an odd one;
 *   InnerProduct(Values_i, r) == want_r[i]  with want_r[i] = core.Encode(MatR)[leaf_index[i]]  (ligero.go:559);
 *   InnerProduct(Values_i, b) == want_z[i]  with b = [1, w, w^2, ...], w = z^cols mod T      (ligero.go:564),
 * Values_i = the first `rows` slot values lumen_decrypt(ctx, opened, scale, rows, .) gives.  r: host, [rows], the
 * transcript's words as sampled (reduced mod T inside); b is built on the device from w.
 * Returns 0 when the checks RAN: a failing column is no error, it is a non-zero status[i], the OR of the bits below.
 * All three checks are evaluated for every column, so walking status[] in query order and testing PATH, R, B in
 * that order reproduces the reference's first error.  got (or NULL): host, [count][2] = the two inner products,
 * canonical mod T; values (or NULL): host, [count][rows], exactly lumen_decrypt's output (Proof.QueriedCols[i].Values).
 * want_r / want_z are compared as given: a word >= T never matches.  count == 0 succeeds and touches nothing.
 * The leaves are hashed by a lumen_leaf_digests_begin job on the context's side stream, under the decryption: no
 * such job of the caller's may be in flight on the context (one job per context).
 * Refused with a message, before any device work: NULL ctx / opened / r / want_r / want_z / leaf_index / root /
 * status; NULL paths with depth > 0; rows outside [1, N]; depth > 32; a leaf_index[i] >= 2^depth; scale = 0 mod T;
 * no secret key; no encoder tables; T >= 2^60; a lane-sharded set; a limb count outside [1, L]. */
#define LUMEN_VERIFY_BAD_PATH 1u /* "failed to verify merkle path for column %d" */
#define LUMEN_VERIFY_BAD_R 2u    /* "well-formedness R check failed for column %d" */
#define LUMEN_VERIFY_BAD_B 4u    /* "well-formedness B check failed for column %d" */
int lumen_verify_columns(lumen_ctx *ctx, const lumen_set *opened, uint64_t scale, uint32_t rows, const uint64_t *r,
                         uint64_t w, const uint64_t *want_r, const uint64_t *want_z, const uint32_t *leaf_index,
                         const uint8_t *paths /* [count][depth][32] */, uint32_t depth, const uint8_t root[32],
                         uint32_t *status, uint64_t *got, uint64_t *values);

/* ---- the plain prover on the same kernels: LigeroProveReference (fhe/ligero.go:799-953),
 * what the client runs to check a decrypted proof.  A plain matrix over F_T is a set of a context whose
 * ONE modulus is T (num_q = 1, num_p = 0, 2N = rows): column j is one "ciphertext" of 2 x 1 x N words.
 * Then core.Encode of every row = lumen_encode (zero_ct all zero), the Merkle leaves = lumen_leaf_digests
 * with an empty serialisation format (non-NULL strings of length 0: the leaf is the column's bytes,
 * ligero.go:866-872), queries = lumen_gather, and the two inner products (ligero.go:886-897, 909-918):
 * out[j] = sum_i columns[j][i] * vec[i] mod q_0, vec: host, 2N raw u64 words (reduced here). */
int lumen_plain_inner_products(lumen_ctx *ctx, const lumen_set *columns, const uint64_t *vec, uint64_t *out);

/* ---- Galois keys: rlwe.EvaluationKeySet entries used by InnerSum.
 * evk host layout [digit(beta)][b|a][limb(L+K)][N], NTT domain, standard form
 * (the Go shim converts from Lattigo's Montgomery-form GadgetCiphertext). */
int lumen_load_galois_key(lumen_ctx *ctx, uint64_t gal_el, const uint64_t *evk);
/* The same with flags.  LUMEN_KEY_MONTGOMERY: the words are in Lattigo's Montgomery form (x * 2^64 mod q_i), i.e.
 * GadgetCiphertext.Value[d][0][0..1] copied as it is -- no IMForm pass over 2.75 M words per key on the Go side.
 * Either way the conversion to the form the gadget product multiplies with runs on the device (0.35 GB of keys
 * per client at the headline size). */
#define LUMEN_KEY_MONTGOMERY 1u
int lumen_load_galois_key_ex(lumen_ctx *ctx, uint64_t gal_el, const uint64_t *evk, uint32_t flags);
/* Galois elements InnerSum(ct, 1, n) needs, in the order it uses them
 * (params.GaloisElementsForInnerSum(1, rows), fhe/ligero_test.go:53) */
uint32_t lumen_inner_sum_galois_elements(const lumen_ctx *ctx, uint32_t n, uint64_t *gal_els);

/* ---- matrixInnerSumEval (fhe/ligero.go:299-370) without the ring switch:
 * for every ciphertext j of `matrix`:
 *   MulNew(matrix[j], pt) -> InnerSum(., 1, rows) -> Rescale to level 1.
 * pt: host, [nl][N], NTT domain (bgv.Encoder.Encode output).  out: new level-1 set. */
int lumen_matrix_inner_sum(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt,
                           uint32_t rows, lumen_set **out);
/* building blocks of the above, exposed for parity tests */
int lumen_mul_plain(lumen_ctx *ctx, const lumen_set *in, const uint64_t *pt, lumen_set **out);
int lumen_inner_sum(lumen_ctx *ctx, const lumen_set *in, uint32_t n, lumen_set **out);

/* ---- the same at every level of the modulus chain.  The two entry points above serve the top level, where the path
 * calls them, and refuse any other set; these take a set with 1 <= nl <= L limbs.  The hybrid key switch then runs on
 * the ceil(nl / K) digits of that level over its nl Q limbs and the K limbs modulo P, with the Galois keys as they
 * are loaded (lumen_load_galois_key[_ex]: the RNS gadget does not depend on the level).  Preconditions as above: n /
 * rows a power of two <= N, 1 or 2 special primes, a full-width set. */
/* Evaluator.InnerSum(ct, 1, n) at the level of `in`: 1 <= in->nl <= L.  With in->nl == L the result equals
   lumen_inner_sum's word for word. */
int lumen_inner_sum_at_level(lumen_ctx *ctx, const lumen_set *in, uint32_t n, lumen_set **out);
/* matrixInnerSumEval (ligero.go:299-370) at the level of `matrix`: pt is [matrix->nl][N]; out has
   min(matrix->nl, 2) limbs.  With matrix->nl == L: lumen_matrix_inner_sum's words. */
int lumen_matrix_inner_sum_at_level(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt,
                                    uint32_t rows, lumen_set **out);

/* ---- InnerSum for any length and batch size: Evaluator.InnerSum(ct, batch_size, n), the lazy double-and-add.  The
 * rotations of the odd bits of n are accumulated over Q and P and take ONE ModDown together; the doublings are the
 * rotations of the entry points above.  out[j] = sum_{i < n} in[j + i * batch_size] on the slots of each row.
 * Accepted: a full-width set at any level, 1 <= in->nl <= L; batch_size >= 1, n >= 1 and batch_size * n <= N / 2 (the
 * sum stays inside one slot row); and batch_size == 1 with n a power of two <= N, where the result is
 * lumen_inner_sum_at_level's word for word (the row swap at n == N included).  1 or 2 special primes.  The Galois keys
 * of lumen_inner_sum_general_elements must be loaded.  Output: canonical residues.
 * The entry points above keep their ranges and their refusals. */
int lumen_inner_sum_general(lumen_ctx *ctx, const lumen_set *in, uint32_t batch_size, uint32_t n, lumen_set **out);
/* lumen_matrix_inner_sum_at_level for the same range of rows (batch size 1); a power of two makes exactly its calls */
int lumen_matrix_inner_sum_general(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt, uint32_t rows,
                                   lumen_set **out);
/* the Galois elements lumen_inner_sum_general(., batch_size, n) applies, in order of first use, without duplicates or
 * the identity: a subset of params.GaloisElementsForInnerSum(batch_size, n).  gal_els: room for 64.  Returns the count;
 * 0 for arguments the call refuses. */
uint32_t lumen_inner_sum_general_elements(const lumen_ctx *ctx, uint32_t batch_size, uint32_t n, uint64_t *gal_els);

/* ---- ciphertext x ciphertext: Evaluator.MulRelinNew(ct, ct) -- ServerBFV.MulNew / Mul take an rlwe.Operand, which may
 * be a ciphertext (fhe/bfv.go:34-42) -- with the relinearisation key the client generates and posts in the /keys body
 * (cmd/client/main.go:74-81; lumen_keygen_relin).  For two degree-1 ciphertexts a = (a0, a1), b = (b0, b1) of the same
 * nl limbs, 1 <= nl <= L, for every Q limb i < nl, coefficient-wise mod q_i:
 *     d0 = T a0 b0      d1 = T (a0 b1 + a1 b0)      d2 = T a1 b1
 *     (k0, k1) = the hybrid key switch (gadget product + ModDown at level nl) of d2 under the relinearisation key
 *     out = (d0 + k0, d1 + k1)                                               (canonical residues)
 * T mod q_i is the factor lumen_mul_plain gives its plaintext: ciphertexts encrypt m * T^-1 + e, and the product of two
 * keeps that form with one T.  The result's scale is scale_a * scale_b mod T: the caller tracks it.  The noise of a
 * product is about T^2 * N * B (B: the operands' noise), so it only decrypts where that stays under Q_level / 2
 * (T = 0x3ee0001: from two limbs; the 57-bit T of cmd/server: three).
 * lumen_load_relin_key: evk in lumen_keygen_relin's layout, [digit(beta)][b|a][limb(L+K)][N], NTT domain, standard form or,
 * with LUMEN_KEY_MONTGOMERY, Lattigo's; converted on the device like a Galois key and shared read-only with clones;
 * loading again replaces it.  It is no Galois key: lumen_load_galois_key(1, .) and it do not see each other.
 * lumen_mul_relin: b has as many ciphertexts as a (pairwise) or one (every ciphertext of a times it); a == b (squares)
 * is allowed.  out: a new set of a's count and level.  lumen_mul_counter grows by a's count.
 * lumen_mul_tensor: the degree-2 triple (d0, d1, d2) before relinearisation, for parity tests, like lumen_mul_plain: host,
 * [count][3][nl][N]; needs no key; leaves lumen_mul_counter as it is.
 * Where lumen_mul_relin is a context's first key switch, the key-switch scratch is placed by timed rotations under the
 * relinearisation key, as a first InnerSum places it under a Galois key: the order of the calls does not matter.
 * Refused with a message: NULL arguments; unknown flags; no special primes (K = 0) or more than two; no relinearisation
 * key loaded; operands of different levels; a count mismatch; a lane-sharded set; a limb count outside [1, L]. */
int lumen_load_relin_key(lumen_ctx *ctx, const uint64_t *evk, uint32_t flags);
int lumen_mul_relin(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, lumen_set **out);
int lumen_mul_tensor(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, uint64_t *host_out /* [count][3][nl][N] */);

/* ---- sums of ciphertext products with ONE relinearisation per sum: the dot product of two encrypted vectors, or an
 * encrypted matrix times an encrypted vector, on the *bgv.Evaluator that ServerBFV embeds (fhe/bfv.go:13-21; the product is
 * fhe/bfv.go:34-42 with ciphertext operands).  It stands for the Lattigo sequence ([LATTIGO-RECALL])
 *     acc = MulNew(a_0, b_0)            (no relinearisation: degree 2)
 *     MulThenAdd(a_i, b_i, acc)         for 0 < i < n
 *     Relinearize(acc)
 * in which the degree-2 terms add up and the hybrid key switch runs once per sum.  `a` holds groups * n ciphertexts of one
 * level, 1 <= nl <= L; term i of group g is a[g n + i].  `b` holds as many (pairwise: b[g n + i]) or exactly n (one vector
 * against every group, matrix x vector: b[i]); with a's count == n the two forms coincide.  a == b is allowed (sums of
 * squares).  With e = g n + i, for every Q limb l < nl, coefficient-wise mod q_l:
 *     D0 = T sum_i a0_e b0_e      D1 = T sum_i (a0_e b1_e + a1_e b0_e)      D2 = T sum_i a1_e b1_e
 *     (k0, k1) = the hybrid key switch of D2 at level nl under the relinearisation key
 *     out[g] = (D0 + k0, D1 + k1)                                            (canonical residues)
 * out: a new set of `groups` ciphertexts at the level of a; a's count == 0 gives an empty set.  The scale is
 * scale_a * scale_b mod T as for lumen_mul_relin (all terms of a sum must share it: the caller tracks it).
 * NOISE: one key-switch term per sum, where n calls of lumen_mul_relin added up carry n; the products' own noise adds,
 * about n * T^2 * N * B, and must stay under Q_level / 2.  The words differ from the sum of n lumen_mul_relin results
 * (the key switch is not linear in its digits' rounding); both decrypt alike.
 * lumen_mul_counter grows by a's count (the products formed).  Batching, lanes and scratch are lumen_mul_relin's, over
 * the `groups` outputs.  Every ring degree lumen_mul_relin serves is served, 2^15 included.
 * lumen_mul_tensor_dot: (D0, D1, D2) before relinearisation, for parity tests: host, [groups][3][nl][N]; needs no key and
 * no special prime; leaves lumen_mul_counter as it is.
 * Refused with a message, before any device work: NULL arguments; n == 0; a's count no multiple of n; b's count neither
 * a's nor n; operands of different levels; a lane-sharded set; a limb count outside [1, L]; and, lumen_mul_relin_dot alone:
 * no special primes (K = 0) or more than two; no relinearisation key loaded. */
int lumen_mul_relin_dot(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, uint32_t n, lumen_set **out);
int lumen_mul_tensor_dot(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, uint32_t n,
                         uint64_t *host_out /* [groups][3][nl][N] */);

/* ---- rotations: Evaluator.Automorphism, RotateColumnsNew, RotateRowsNew and RotateHoistedNew of the *bgv.Evaluator that
 * ServerBFV embeds (fhe/bfv.go:13-21), with the Galois keys lumen_load_galois_key[_ex] loaded (lumen_keygen_galois makes
 * one for any odd element).  `in`: a set of `count` ciphertexts at one level, 1 <= nl <= L; it is not modified.  With
 * (k0, k1) the hybrid key switch of c1 at that level under the key of g and index_g the NTT-domain table of X -> X^g
 * ([LATTIGO-RECALL] ring.AutomorphismNTTIndex), for d = (c0 + k0, k1):
 *     out[w][l][j] = d[w][l][index_g[j]]                                     (canonical residues)
 * in a new set of the same count and level.  On the slots of a BGV plaintext (two rows of N/2): g = 5^k rotates both rows
 * by k to the left (slot i takes the value of slot i + k mod N/2), g = 2N - 1 swaps the rows.
 * lumen_galois_element: 5^(k mod N/2) mod 2N (rlwe.Parameters.GaloisElement; k may be negative; 0 and N/2 give 1); the row
 * swap is 2N - 1 (GaloisElementForRowRotation).  0 for a NULL context.
 * lumen_rotate_columns(k) = lumen_automorphism(lumen_galois_element(k)); lumen_rotate_rows = lumen_automorphism(2N - 1).
 * lumen_rotate_hoisted: outs[i] = lumen_automorphism(in, gal_els[i]) word for word, i < n_els <= 64, with the
 * decomposition of c1 (inverse transform, digit extension) done once and shared by the elements.  An element equal to 1 and
 * repeated elements are allowed; each gets its own set.  n_els == 0 does nothing.  On failure every outs[i] is NULL.
 * gal_el == 1 is a copy and needs no key.  count == 0 gives an empty set.  lumen_mul_counter does not move.
 * Refused with a message, before any device work: NULL arguments; an even element or one >= 2N; no key loaded for the
 * element; no special primes (K = 0) or more than two; a lane-sharded set; a limb count outside [1, L]; n_els > 64. */
uint64_t lumen_galois_element(const lumen_ctx *ctx, int64_t k);
int lumen_automorphism(lumen_ctx *ctx, const lumen_set *in, uint64_t gal_el, lumen_set **out);
int lumen_rotate_columns(lumen_ctx *ctx, const lumen_set *in, int64_t k, lumen_set **out);
int lumen_rotate_rows(lumen_ctx *ctx, const lumen_set *in, lumen_set **out);
int lumen_rotate_hoisted(lumen_ctx *ctx, const lumen_set *in, const uint64_t *gal_els, uint32_t n_els,
                         lumen_set **outs /* [n_els] new sets */);

/* ---- the diagonal linear transform: a plaintext matrix times an encrypted vector by the diagonal method,
 *     out = sum_k diag_k (.) Rot_k(ct)
 * [LATTIGO-RECALL] Evaluator.MultiplyByDiagMatrix, the non-BSGS branch of LinearTransformation / LinearTransformationsNew
 * of the lintrans evaluator, which sits on the *bgv.Evaluator that ServerBFV embeds (fhe/bfv.go:13-21).  Single-hoisted:
 * one decomposition of c1, per non-zero diagonal one gadget product and one multiply-accumulate over Q and P, and ONE
 * ModDown for the whole sum -- where lumen_rotate_hoisted followed by lumen_mul_plain_then_add pays one ModDown, one
 * output set and one product pass per diagonal.  lumen_lintrans_load_bsgs gives the double-hoisted (baby-step / giant-step)
 * form of the same transform, below.  Limits: column rotations only (no row swap among the diagonals); 1 or 2 special
 * primes.  Prove does not use the transform.
 * lumen_lintrans_load (LinearTransformation's encoding, NewLinearTransformation + Encode): n >= 1 diagonals at the level of
 * nl limbs, 1 <= nl <= L.  k[d]: the diagonal's index, |k| < N/2, taken modulo N/2; its Galois element is
 * lumen_galois_element(k).  pts: host [n][nl + K][N], diagonal d as a plaintext over Q and P -- limbs 0..nl-1 residues
 * modulo q_0..q_{nl-1}, limbs nl..nl+K-1 residues modulo the special primes, NTT domain, canonical, in the form
 * Encoder.Encode leaves and lumen_mul_plain takes (m * T^-1).  The multiplier is m_k = pt_k * T per limb, as MulNew's; it
 * is formed once, here, and stays on the device until lumen_lintrans_destroy (ctx: the loading context or a clone; NULL
 * after the context is gone).  A transform serves the context that loaded it and its clones.
 * lumen_lintrans_galois_elements: the elements of the non-zero diagonals in the order given -- of a double-hoisted
 * transform: of its babies i != 0, ascending, then of its giants j != 0, ascending -- into gal_els (room for 2n: a
 * double-hoisted transform may need a baby's and a giant's key per diagonal); returns their number.  The keys of exactly
 * these must be loaded (lumen_load_galois_key[_ex]).
 * lumen_linear_transform (LinearTransformationNew): `in`, a set of any count at the transform's level, is not modified.
 * With dig = the digits of c1, (u0, u1)_k = the gadget product of dig under the key of g_k over the nl limbs of Q and the
 * K of P, and sigma_g the NTT-domain permutation of lumen_automorphism:
 *     acc = sum_{k != 0} m_k (.) sigma_{g_k}(u0_k + (P c0 on Q, 0 on P), u1_k)          (over Q and P, no ModDown)
 *     out = ModDown(acc) (+ m_0 (.) (c0, c1) when 0 is among the diagonals)            (canonical residues)
 * in a new set of the same count and level.  The scale is lumen_mul_plain's.  The words differ from those of the rotations
 * multiplied and added up one by one (the floor of ModDown does not commute with the sum); both decrypt alike.
 * A transform with diagonal 0 alone needs no key, runs no key switch and gives lumen_mul_plain's words.  count == 0 gives
 * an empty set and looks no key up.  lumen_mul_counter does not move (it counts the Mul / MulNew wrappers, as for the
 * rotations).  Batching, lanes and scratch are the key switch's; every ring degree is served, 2^15 included.
 * lumen_linear_transforms (LinearTransformationsNew): outs[i] = lumen_linear_transform(in, lts[i]) word for word, with the
 * decomposition of c1 done once per batch and shared by the transforms.  n_lts == 0 does nothing.  On failure every
 * outs[i] is NULL.
 * Refused with a message, before anything is allocated or enqueued: NULL arguments; n == 0; nl outside [1, L]; |k| >= N/2;
 * two diagonals equal modulo N/2; a residue >= its modulus; no special primes (K = 0) or more than two; a set at another
 * level than the transform's; a transform of another context; a lane-sharded set; no key loaded for a diagonal's element.
 *
 * The double-hoisted form ([LATTIGO-RECALL] MultiplyByDiagMatrixBSGS).  lumen_lintrans_load_bsgs takes lumen_lintrans_load's
 * arguments -- the diagonals are NOT pre-rotated by the caller -- and n1 >= 1 baby steps.  With e = k mod N/2 a diagonal is
 * e = j + i, i = e mod n1 its baby, j = e - i its giant; the load forms m'_e = sigma_{g_j}^-1(m_e) on the device.  Then
 *     baby_0 = (P c0, P c1) on Q, 0 on P;   baby_i = sigma_{g_i}(gadget(dig, key g_i) + (P c0 on Q, 0))        (i != 0, no ModDown)
 *     tmp_j  = sum_i m'_{j+i} (.) baby_i                                                  (over Q and P, both polynomials)
 *     acc    = tmp_0 + sum_{j != 0} sigma_{g_j}(gadget(decompose(ModDown(tmp_j)[1]), key g_j) + (tmp_j[0], 0))
 *     out    = ModDown(acc)                                                              (ONE, canonical residues)
 * so D diagonals cost about n1 + D / n1 gadget products and keys instead of D; a giant adds one decomposition and a
 * ModDown of one polynomial.  lumen_linear_transform and lumen_linear_transforms take such an object wherever they take a
 * single-hoisted one, mixed freely; outs[i] still equals the single call word for word (a double-hoisted transform with
 * giants decomposes c1 for itself, the single-hoisted ones of a call keep sharing one decomposition).  When every
 * diagonal is a baby (n1 above the largest e) the words are the single-hoisted transform's; n1 = 1 makes every diagonal
 * a giant; diagonal 0 alone needs no key and gives lumen_mul_plain's words.  Levels, ring degrees, K, counts, the
 * counter and the refusals are lumen_lintrans_load's and lumen_linear_transform's; n1 == 0 is refused by name.  Each
 * giant that occurs holds one more block of the gadget product's size per lane while a batch runs;
 * the batch of such a call is halved until the blocks fit a quarter of the device's memory.
 * lumen_lintrans_best_baby_steps (host only): the power of two n1 in [1, N/2], N = 2^log_n, that minimises the number of
 * keys, (distinct babies != 0) + (distinct giants != 0); the smaller on a tie; 0 for NULL, n == 0, a log_n outside
 * [1, 31] or a k outside (-N/2, N/2). */
typedef struct lumen_lintrans lumen_lintrans;
int lumen_lintrans_load(lumen_ctx *ctx, const int64_t *k, const uint64_t *pts /* host [n][nl+K][N] */, uint32_t n,
                        uint32_t nl, lumen_lintrans **out);
void lumen_lintrans_destroy(lumen_ctx *ctx, lumen_lintrans *lt);
int lumen_lintrans_load_bsgs(lumen_ctx *ctx, const int64_t *k, const uint64_t *pts /* host [n][nl+K][N] */, uint32_t n,
                             uint32_t nl, uint32_t n1, lumen_lintrans **out);
uint32_t lumen_lintrans_best_baby_steps(uint32_t log_n, const int64_t *k, uint32_t n);
uint32_t lumen_lintrans_galois_elements(const lumen_lintrans *lt, uint64_t *gal_els /* room for 2n */);
int lumen_linear_transform(lumen_ctx *ctx, const lumen_set *in, const lumen_lintrans *lt, lumen_set **out);
int lumen_linear_transforms(lumen_ctx *ctx, const lumen_set *in, const lumen_lintrans *const *lts, uint32_t n_lts,
                            lumen_set **outs /* [n_lts] new sets */);

/* ---- the evaluator's linear operations: Evaluator.Add / Sub / Mul(ct, uint64) / MulThenAdd of the *bgv.Evaluator that
 * ServerBFV embeds (fhe/bfv.go:13-21), with a ciphertext, a scalar or a plaintext operand -- the calls fhe/ntt.go:27-236 and
 * vdec/batching.go:24-34 make one ciphertext at a time, here on whole sets, so that a caller can write another butterfly
 * network, another code or another batching on resident sets.  Inputs are canonical NTT-domain words; outputs are
 * canonical.  The library is scale-agnostic here as everywhere: the caller tracks the scale.
 * SCALARS.  A scalar word w is what Evaluator.Mul(ct, uint64) sees: limb i is multiplied by centre_T(w mod T) mod q_i, the
 * representative of w mod T in (-T/2, T/2] taken modulo q_i.  The raw Montgomery-form words of RootForwardUint64 that
 * fhe/ntt.go passes go in as they are.  On a plain context, whose one modulus is T, that is w mod T.
 * lumen_linear_combination: out = sum_{t<n} w[t] * in[t], 1 <= n <= 8, in ONE pass: every input word is read once and every
 * output word written once.  w[t] == 1 and w[t] == -1 (mod T) are additions and subtractions with no multiply.
 * lumen_add (AddNew / Add), lumen_sub, lumen_mul_scalar (Mul(ct, uint64)) and lumen_mul_scalar_then_add (MulThenAdd:
 * acc += w * a) are its cases n <= 2 -- the same code.
 * COUNTS.  Every ciphertext operand has the result's count or count 1: one ciphertext combines with every ciphertext of
 * the other operands, as in lumen_mul_relin.
 * LEVELS.  Operands may have different limb counts; the result has the smallest and each operand contributes its first
 * limbs (Lattigo's min-level rule: dropping a level is taking a prefix).  A plaintext pt is host [a's limbs][N] raw
 * residues in the form lumen_mul_plain takes (Encoder.Encode's output); a residue >= q_l is refused the same way.
 * lumen_add_plain / lumen_sub_plain: out = (c0 +- pt, c1).  lumen_mul_plain_then_add: acc += a (.) (pt * T), i.e.
 * lumen_mul_plain followed by lumen_add, word for word; the accumulator takes the first limbs of a and pt where they are
 * deeper than it.
 * DESTINATION.  *out == NULL on entry: a new set.  Otherwise *out is an existing set of exactly the result's count, limb
 * count and lane width, and is written.  It may BE one of the operands (the same ciphertexts, limbs and storage): the
 * operations work in place, and an in-place butterfly over a resident set allocates nothing.  Any other overlap of an
 * operand's device range with the destination's -- an overlapping but unequal lumen_set_slice, say -- is refused.  a == b
 * is allowed.  `acc` of the two _then_add forms is read and written in place and may not overlap a.
 * Lane-sharded sets (lumen_set_create_lanes) are accepted by the five scalar forms: all operands and the destination must
 * have one lane width.  The three plaintext forms take full-width sets.  Sets created by another context of the same
 * device are accepted, as elsewhere.  Every ring degree a context can have is served, 2^15 included.
 * lumen_mul_counter grows by the result's count in lumen_mul_scalar (the counter lives in the ServerBFV.Mul / MulNew
 * wrappers, bfv.go:34-42); the other seven calls are the embedded evaluator's own and leave it alone.
 * Refused with a message, before any launch: NULL arguments; n == 0 or n > 8; counts that are neither equal nor 1; a
 * destination of another count, limb count or lane width than the result; mixed lane widths; a forbidden overlap; a
 * plaintext residue out of range; a context without a plaintext modulus. */
int lumen_add(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, lumen_set **out);
int lumen_sub(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, lumen_set **out);
int lumen_mul_scalar(lumen_ctx *ctx, const lumen_set *a, uint64_t w, lumen_set **out);
int lumen_mul_scalar_then_add(lumen_ctx *ctx, const lumen_set *a, uint64_t w, lumen_set *acc);
int lumen_linear_combination(lumen_ctx *ctx, const lumen_set *const *in, const uint64_t *w, uint32_t n, lumen_set **out);
int lumen_add_plain(lumen_ctx *ctx, const lumen_set *a, const uint64_t *pt, lumen_set **out);
int lumen_sub_plain(lumen_ctx *ctx, const lumen_set *a, const uint64_t *pt, lumen_set **out);
int lumen_mul_plain_then_add(lumen_ctx *ctx, const lumen_set *a, const uint64_t *pt, lumen_set *acc);

/* ---- fhe.RingSwitchServer (fhe/ring_switch.go:93-113): Evaluator.ApplyEvaluationKey of every
 * ciphertext of `in` into the ring of degree 2^log_n_small with the single modulus q_0, at level 0.
 * key: the rlwe.EvaluationKey of NewRingSwitchClient (ring_switch.go:43-56) as the client posts it
 * (cmd/client/main.go:124-131): GadgetCiphertext.Value flattened
 *     [rns digit][power-of-two digit][b|a][limb: q_0..q_{L-1}, p_0..p_{K-1}][N],  NTT domain, standard form
 * with lumen_ringswitch_rns_digits() x lumen_ringswitch_digits(w) entries.  Level 0 reads RNS digit 0
 * only, so a caller may pass just that first block (evk.Value[0]); key_words = the number of u64 words at
 * `key`, which must be one of those two sizes (anything else is refused before a word is read).
 * base_two_w = BaseTwoDecomposition (13).  Which gadget product runs follows the key's LevelP, as in
 * rlwe.Evaluator.GadgetProductLazy [LATTIGO-RECALL]:
 *   K >= 2 special primes (what GenerateBGVParamsForNTT always produces, fhe/bfv.go:172-178): the hybrid
 *     key switch with RNS digits only; base_two_w is ignored and lumen_ringswitch_digits() = 1 -- the
 *     reference's "Marshaled keys length" logs show the key is exactly one Galois key's size
 *     (results/experimental/client/bench_*.txt:20 against results/baseline/client/bench_*.txt:19);
 *   K <= 1 (TestRingSwitch's LogQ = [58] without P, fhe/ring_switch_test.go:14-18): unsigned base-2^w
 *     digits, lumen_ringswitch_digits() = ceil(bits(q_0) / w); no ModDown when K = 0.
 * out: host, [count][2][2^log_n_small] residues mod q_0 in the small ring's NTT domain. */
uint32_t lumen_ringswitch_rns_digits(const lumen_ctx *ctx);
uint32_t lumen_ringswitch_digits(const lumen_ctx *ctx, uint32_t base_two_w);
int lumen_load_ringswitch_key(lumen_ctx *ctx, uint32_t log_n_small, uint32_t base_two_w,
                              const uint64_t *key, size_t key_words);
int lumen_ring_switch(lumen_ctx *ctx, const lumen_set *in, uint64_t *out);

/* ---- the client's keys, generated on the device (cmd/client/main.go:74-81, fhe/ring_switch.go:16-57):
 * kgen.GenKeyPairNew(), GenRelinearizationKeyNew(sk), GenGaloisKeysNew(galEls, sk), GenEvaluationKeyNew(sk, skNew).
 * Every key is an array of gadget entries (b, a) = (NTT(e) - a*s_out + fac*s_in, a) over the whole basis QP, in exactly
 * the layout its loader takes (lumen_load_public_key, lumen_load_galois_key[_ex], lumen_load_ringswitch_key), so a
 * generated key goes straight into them -- or, with LUMEN_KEY_MONTGOMERY, into Lattigo's GadgetCiphertext as it is.
 * SAMPLING CONTRACT.  Deterministic in (seed, key id, entry, limb, coefficient): keys generated one at a time, in one
 * batched call or on another GPU are the same bytes.
 *   keystream(I, s) = ChaCha20(key = seed, nonce = LE64(I) || LE32(s), counter = 0, 1, ...), the encryptor's;
 *   sample index I(key_id, e) = key_id * 4096 + e, e = i * pw2 + j the gadget entry (RNS digit i, power-of-two digit j;
 *     pw2 = 1 everywhere except the ring-switch key with K <= 1);
 *   key ids: secret 0, public 1, relinearisation 2, ring switch 3, Galois key of element g: 0x10000 + g;
 *   ternary secret s: stream 0 of I(0, 0), 32-bit word w -> ((w * 3) >> 32) - 1; the ring switch's small secret: the
 *     first 2^log_n_small coefficients of stream 0 of I(3, 0);
 *   Gaussian error of entry e: stream 1 of I(key_id, e), the encryptor's CDT rule, one N-coefficient sample per entry
 *     extended to every limb;
 *   uniform a of limb m (Q limbs, then P limbs) of entry e: stream 16 + m of I(key_id, e) read as little-endian 64-bit
 *     words; attempt t = 0, 1, ... for coefficient k is word number t * N + k; the first attempt with
 *     x < 2^64 - (2^64 mod q_m) is kept and a[k] = x mod q_m (unbiased).  a is sampled in the NTT domain.
 * The seed is key material: take it from the OS CSPRNG and use it for nothing else.  Streams 0-2 of an index are the
 * ones lumen_encrypt_* would draw: a keygen seed MUST NOT be passed to lumen_encrypt_*.
 * lumen_keygen_secret generates s on the device, installs it as the context's secret key (the first L limbs, exactly
 * what lumen_load_secret_key would hold) and keeps its L+K-limb table for the other four calls, which need it and take
 * the same seed; clones share it like the other key tables.  sk leaves the device only when a buffer is given.
 * fac = P * 2^(w j) mod q_m on the Q limbs m of the entry's RNS digit (i * alpha <= m < (i+1) * alpha, alpha = max(K, 1)),
 * 0 elsewhere.  public key: one entry, fac = 0, s_out = s.  Galois key of g: s_out = pi_{g^-1}(s), s_in = s.
 * relinearisation key: s_out = s, s_in = s^2.  ring-switch key: s_out = skNew(X^(N/n)), s_in = s, shape
 * lumen_ringswitch_rns_digits() x lumen_ringswitch_digits(w) (K >= 2: w ignored).
 * flags: LUMEN_KEY_MONTGOMERY = both halves leave multiplied by 2^64 mod q_m (what lumen_load_galois_key_ex accepts).
 * All keys of a call are produced by one launch of each kernel and reach `evk` in one transfer (page-locked memory
 * from lumen_host_alloc directly, pageable memory through the bounce buffers).
 * Refused with a message, before any device work: no generated secret on the context; NULL ctx / seed / output; an even
 * gal_el or one >= 2N; K = 0 for Galois and relinearisation keys; a wrong key_words; log_n_small >= logN; unknown flag
 * bits.  count == 0 succeeds and touches nothing. */
int lumen_keygen_secret(lumen_ctx *ctx, const uint8_t seed[32], uint64_t *sk /* NULL or host [L+K][N], NTT */);
int lumen_keygen_public(lumen_ctx *ctx, const uint8_t seed[32], uint64_t *pk /* [2][L+K][N] */);
int lumen_keygen_galois(lumen_ctx *ctx, const uint8_t seed[32], const uint64_t *gal_els, uint32_t count,
                        uint64_t *evk /* [count][beta][b|a][L+K][N] */, uint32_t flags);
int lumen_keygen_relin(lumen_ctx *ctx, const uint8_t seed[32], uint64_t *evk /* [beta][b|a][L+K][N] */, uint32_t flags);
int lumen_keygen_ringswitch(lumen_ctx *ctx, const uint8_t seed[32], uint32_t log_n_small, uint32_t base_two_w,
                            uint64_t *key, size_t key_words /* the full [rns][pw2][b|a][L+K][N] size */,
                            int8_t *sk_small /* host [2^log_n_small] */);

/* ---- seeded switching keys: the Galois keys and the relinearisation key travel as their b halves and ONE public
 * 32-byte seed (cmd/client/main.go:74-81 generates and marshals the whole set; the `/keys` handler of
 * cmd/server/main.go:66 receives it -- 16 Galois keys and one relinearisation key of 22 MB each at the headline shape,
 * half of which is the pseudorandom `a`).  The client keeps `a` out of memory altogether and posts
 * [digit(beta)][limb(L+K)][N] words per key; the server draws `a` where it converts the key anyway.
 * ADDITION TO THE SAMPLING CONTRACT.  A seeded key takes two seeds:
 *   seed: key material, as above.  The error of entry e is stream 1 of I(key_id, e) under seed; the secret is the
 *     context's generated secret;
 *   a_seed: PUBLIC.  a of limb m of entry e is stream 16 + m of the SAME index I(key_id, e) under a_seed, by the rule
 *     above: attempt t of coefficient k is word t * N + k, the first x < 2^64 - (2^64 mod q_m) is kept as x mod q_m;
 *   b = NTT(e) - a*s_out + fac*s_in as above.
 * So a seeded key expanded by the server is word for word the pair (b, a), and with a_seed == seed b would be exactly
 * what lumen_keygen_galois / lumen_keygen_relin return -- which the device refuses, because it would publish the secret
 * seed.
 * ONE `a` PER KEY.  The error depends on (seed, key id, entry) alone, not on a_seed: generating a key again under the same
 * two seeds gives the same words, which is harmless.  What MUST NOT happen is the same key -- one (keygen seed, key id) --
 * published under two different `a`: its seeded form under two a_seeds, or its full form (lumen_keygen_galois /
 * lumen_keygen_relin draw a under the keygen seed) beside a seeded one.  The two b differ by (a2 - a1) * s_out
 * coefficient by coefficient, both a are public, and whoever sees both keys has the secret.  So: draw ONE a_seed from the
 * OS CSPRNG together with the keygen seed, keep it for as long as that seed lives, use it for nothing else, and publish
 * each key in one of the two forms only.  The library sees one call at a time and cannot enforce this; the host
 * mirror's fhe::KeyGenerator does.
 * lumen_keygen_galois_seeded / lumen_keygen_relin_seeded work like their siblings: all keys of a call come from one
 * launch of each kernel and one download of half the size; LUMEN_KEY_MONTGOMERY applies to b.  `a` is drawn inside
 * the transform's storer and never written.  Refused like their siblings (no generated secret, K = 0, an even element or
 * one >= 2N, unknown flags, NULL arguments, a split ring degree), and when the two seeds are equal.
 * lumen_load_galois_key_seeded / lumen_load_relin_key_seeded need no secret, no keygen state and no encoder.  flags
 * describes b (LUMEN_KEY_MONTGOMERY: b is in Lattigo's form); a is always drawn canonical.  b takes the conversion and
 * the range check of lumen_load_galois_key_ex ("key residue out of range (digit, limb)"); a is drawn straight into the
 * gadget product's layout.  The installed key is the one lumen_load_galois_key_ex(gal_el, (b, a)) installs: shared with
 * clones, replaced in place when loaded again, and a full and a seeded key of one element replace each other.  They
 * serve every ring degree their siblings serve, 2^15 included. */
int lumen_keygen_galois_seeded(lumen_ctx *ctx, const uint8_t seed[32], const uint8_t a_seed[32], const uint64_t *gal_els,
                               uint32_t count, uint64_t *b_out /* [count][beta][L+K][N] */, uint32_t flags);
int lumen_keygen_relin_seeded(lumen_ctx *ctx, const uint8_t seed[32], const uint8_t a_seed[32],
                              uint64_t *b_out /* [beta][L+K][N] */, uint32_t flags);
int lumen_load_galois_key_seeded(lumen_ctx *ctx, uint64_t gal_el, const uint64_t *b /* [beta][L+K][N] */,
                                 const uint8_t a_seed[32], uint32_t flags);
int lumen_load_relin_key_seeded(lumen_ctx *ctx, const uint64_t *b /* [beta][L+K][N] */, const uint8_t a_seed[32],
                                uint32_t flags);

/* ---- the client's encryptor: witness encryption under the SECRET key, and seeded ciphertexts (fhe/bfv.go:77: the
 * rlwe.NewEncryptor(paramsFHE, sk) that ClientBFV embeds; client.EncryptNew, vdec/batching_test.go:56).  In the protocol
 * the witness belongs to the client; a client that holds its secret on the device (lumen_load_secret_key or
 * lumen_keygen_secret) encrypts under it: `count` columns of `rows` slot values, host [count][rows], exactly what
 * lumen_encrypt_values takes, to top-level ciphertexts
 *     c1[l] = a_l,    c0[l] = NTT_l(e) + pt_l - a_l (.) NTT_l(s)      (canonical residues)
 * -- L limb transforms per ciphertext against the (L+K) + 2K + 2L of the public-key path, and no public key at all.
 * c1 is pure randomness regenerated from a PUBLIC 32-byte seed, so a ciphertext travels as its c0 half and that seed:
 * lumen_encrypt_sk_seeded returns only the c0 halves (half the bytes over PCIe and the network) and the server rebuilds
 * the set with lumen_ct_expand_seeded, which needs no key of any kind.
 * CONTRACT.  Deterministic in (seeds, first_index + i, limb, coefficient): chunked, one ciphertext at a time or on
 * another GPU the bits are the same.
 *   keystream(I, s) = ChaCha20(key, nonce = LE64(I) || LE32(s), counter = 0, 1, ...), the library's one keystream;
 *     ciphertext i has index I = first_index + i;
 *   error e: stream 3 of keystream(I, .) under secret_seed, the encryptor's CDT rule (sigma 3.2, |e| <= 19), one
 *     N-coefficient sample per ciphertext extended to every limb.  The public-key encryptor draws streams 0-2 and key
 *     generation streams 16 + m, so the stream number separates the domains; a seed is still key material taken from
 *     the OS CSPRNG and used for ONE purpose only;
 *   c1[l] = a_l: uniform mod q_l, sampled in the NTT domain from stream 16 + l of keystream(I, .) under a_seed by key
 *     generation's exact rule: attempt t of coefficient k is 64-bit word t * N + k, the first x < 2^64 - (2^64 mod q_l)
 *     is kept as x mod q_l.  Q limbs only;
 *   pt: the plaintext bits lumen_encrypt_values encrypts (slot scatter, INTT over Z_T, m * T^-1 mod q_l: Encoder.Encode);
 *   s: the context's secret key, loaded or generated.
 * The three calls agree: lumen_encrypt_sk_seeded returns the c0 halves of the very set lumen_encrypt_sk_values would
 * return, and lumen_ct_expand_seeded rebuilds that set bit for bit on any context with the same moduli (the c0 words are
 * taken as given, like lumen_set_upload; page-locked c0: one strided DMA, pageable: the bounce buffers).
 * a_seed is public, secret_seed is key material: equal seeds are refused (the server could regenerate e).  A pair
 * (a_seed, index) MUST NOT encrypt two messages under one key -- the same a twice leaks the difference of the
 * plaintexts: take a fresh a_seed from the OS CSPRNG per call (or keep first_index moving) and use it for nothing else.
 * The fresh noise is e itself, larger than the few units the public-key path leaves after its division by P
 * (tools/noise_budget.py: every BASELINE shape tolerates it).
 * Refused with a message, before any device work: NULL arguments; no secret key; no encoder tables; rows outside
 * [1, N]; equal seeds.  count == 0 succeeds and touches nothing. */
/* Encoder.Encode + Encryptor(sk).EncryptNew of `count` columns of `rows` slot values: full ciphertexts on the device */
int lumen_encrypt_sk_values(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count,
                            const uint8_t secret_seed[32], const uint8_t a_seed[32], uint64_t first_index,
                            lumen_set **out);
/* the same ciphertexts in seeded form: only the c0 halves leave the device; c0: host, [count][L][N] */
int lumen_encrypt_sk_seeded(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count,
                            const uint8_t secret_seed[32], const uint8_t a_seed[32], uint64_t first_index,
                            uint64_t *c0);
/* the server's side: c0 halves + public seed -> the full top-level set.  Needs no key of any kind. */
int lumen_ct_expand_seeded(lumen_ctx *ctx, const uint64_t *c0, uint32_t count, const uint8_t a_seed[32],
                           uint64_t first_index, lumen_set **out);

/* ---- the front end of the proof of decryption (cmd/client/main.go:203-208: Proof.ProveDecrypt ->
 * vdec.ProveBfvDecBatched, vdec/prover.go:50-98, vdec/batching.go): what the client computes on its own ciphertexts
 * before the call into lazer.  lazer itself is out of scope: these two calls produce the arguments of ProveVdecLnpTbox.
 *
 * lumen_batch_ciphertexts = vdec.BatchCiphertexts: each row alpha_j of `alphas` (host [count][rows], count = the set's)
 * is encoded as a plaintext at scale pt_scale (Encoder.Encode: alpha_j * pt_scale mod T into the slots, inverse transform
 * over Z_T -- the scale is applied modulo T, ahead of the transform) and the result is ONE ciphertext of the set's limb
 * count,
 *     out = sum_j MulNew(ct_j, pt(alpha_j))                                   (canonical residues)
 * A word of `alphas` >= T counts as its residue (the transcript samples raw 64-bit words).  The result's scale is the
 * ciphertexts' scale * pt_scale mod T: the caller tracks it (the reference copies the ciphertexts' MetaData into the
 * plaintexts, so pt_scale is the ciphertexts' scale there).  lumen_mul_counter grows by count.
 * THE BUDGET.  Multiplying by a full-size plaintext costs about N * T in noise, so the batch only decrypts where
 *     T * count * N * T * (B + 1) < Q_level / 2,
 * B the noise of the inputs in the form phase = m * T^-1 + e.  The reference's vdec tests use T = 0x3ee0001 for exactly
 * that reason; with the 57-bit T of cmd/server its own -vdec path overflows at level 1.  The library computes what it is
 * asked to compute: tools/noise_budget.py --vdec COUNT says whether a shape fits.
 * Refused with a message, before any device work: NULL arguments; count == 0; rows outside [1, N]; a lane-sharded set;
 * a limb count outside [1, L]; no encoder tables; pt_scale == 0 mod T; T >= 2^60.
 *
 * lumen_vdec_witness = the witness generation of prover.go:104-119 (core/utils.go:12-33) on ONE ciphertext of ONE limb
 * (run lumen_rescale(., 1) first), N centred coefficients each, host arrays:
 *     sk       the secret key, in {-1, 0, 1} (anything else is an error)
 *     c0, c1   the ciphertext's halves, coefficient domain, in (-q_0/2, q_0/2]
 *     m_delta  the message m (host [rows] slot values) at `scale`: Encode(m * scale mod T) * T^-1 mod q_0, coefficient
 *              domain, centred
 *     err      (or NULL) c0 + c1 * sk - m_delta mod q_0, centred: the e whose smallness lazer proves.  The decryption
 *              is right exactly when |err| * 2T < q_0.
 * Recorded deviation: prover.go:119 passes isNTT = false for an NTT-domain plaintext, i.e. it hands lazer limb 0's
 * NTT-domain words as if they were coefficients.  That is not reproduced: m_delta is in the coefficient domain, like
 * c0 and c1.  The reference takes only the first `degree` (2048) coefficients (prover.go:92,138-143); here all N are
 * returned and the caller slices.
 * Refused in addition: a set of other than one ciphertext or other than one limb; no secret key; scale == 0 mod T. */
int lumen_batch_ciphertexts(lumen_ctx *ctx, const lumen_set *cts, const uint64_t *alphas /* host [count][rows] */,
                            uint32_t rows, uint64_t pt_scale, lumen_set **out /* 1 ciphertext, cts' limb count */);
int lumen_vdec_witness(lumen_ctx *ctx, const lumen_set *ct, const uint64_t *m /* host [rows] */, uint32_t rows,
                       uint64_t scale, int8_t *sk /* [N] */, int64_t *c0, int64_t *c1, int64_t *m_delta,
                       int64_t *err /* or NULL */);

/* ---- query loop of Prove (fhe/ligero.go:268-279): gather ciphertexts idx[i]
 * of a set into a new set (duplicates allowed). */
int lumen_gather(lumen_ctx *ctx, const lumen_set *src, const uint32_t *idx, uint32_t n,
                 lumen_set **out);

/* ---- several GPUs behind ONE call sequence: the reference is one Go process that owns the whole
 * request (cmd/server/main.go:187-266) and spreads its work over goroutine pools (fhe/ligero.go:136-162,
 * 231-242); a lumen_group is that process's set of W = 2^log_world "ranks", one lumen_ctx per GPU, with the
 * exchange steps of the sharded Commit inside the library:
 *     rank r holds input columns [r*cols/W, (r+1)*cols/W) and everything derived from them (MatR / MatZ
 *     blocks r), the encoded columns [r*S/W, (r+1)*S/W) with their level-1 leaves, and during Encode the lane
 *     shard r (coefficients [r*N/W, (r+1)*N/W) of every limb of every ciphertext).
 * Transport, chosen at creation:
 *     LUMEN_TRANSPORT_COPY  stream-ordered device copies (hipMemcpyAsync on one device, hipMemcpyPeerAsync
 *                           across devices) pulled by the destination rank's stream; every rank must be a
 *                           context of this process.  The only transport possible when several ranks share a
 *                           device (the one-GPU test mode: RCCL refuses two ranks on one device).
 *     LUMEN_TRANSPORT_RCCL  RCCL over xGMI, loaded at run time (librccl.so.1): grouped ncclSend / ncclRecv
 *                           for the two all-to-alls, ncclAllGather for the digests.  One communicator per
 *                           rank: ncclCommInitAll for a process that owns all W devices (lumen_group_create),
 *                           ncclCommInitRank for one process per GPU (lumen_group_create_rank).
 *     LUMEN_TRANSPORT_AUTO  RCCL when the W contexts sit on W distinct devices, COPY otherwise -- and COPY as well
 *                           when RCCL cannot be loaded or refuses to initialise (a host without librccl, an IPC
 *                           mode RCCL does not support): the W devices of one process can always exchange by
 *                           (peer) copies.  lumen_group_transport() / _note() say what was chosen and why;
 *                           LUMEN_TRANSPORT_RCCL asked for by name fails instead of falling back.
 * Every array argument below has lumen_group_local() entries, one per context of THIS process, in the order
 * the contexts were given (ascending global rank).  Collectives are enqueued on the contexts' own streams
 * and ordered against the work already enqueued there; nothing blocks the host unless it returns host data
 * (temporaries of lumen_group_encode / _gather go back to their contexts' pools in stream order).
 * Errors: non-zero return, text through lumen_last_error(NULL) on the calling thread. */
#define LUMEN_TRANSPORT_AUTO 0
#define LUMEN_TRANSPORT_COPY 1
#define LUMEN_TRANSPORT_RCCL 2
/* one process, all W ranks: ctxs[r] is rank r (contexts of the same parameters; clones of one context are
 * fine and share its keys when they share its device). */
int lumen_group_create(lumen_ctx *const *ctxs, uint32_t log_world, uint32_t transport, lumen_group **out);
/* one process per GPU (what `torch.distributed.run bench.py` starts): rank 0 draws a 128-byte id
 * (ncclGetUniqueId), the host hands it to every rank by any means, each rank joins with its own context. */
int lumen_group_unique_id(uint8_t id[128]);
int lumen_group_create_rank(lumen_ctx *ctx, uint32_t rank, uint32_t log_world, const uint8_t id[128],
                            lumen_group **out);
/* destroy a group BEFORE its contexts: it waits for their streams and returns its events to them */
void lumen_group_destroy(lumen_group *g);
uint32_t lumen_group_world(const lumen_group *g);
uint32_t lumen_group_local(const lumen_group *g);
/* what actually moves the blocks: "rccl"; "copy" (all ranks on one device); "copy-peer" (several devices, peer
 * access enabled between every pair: hipMemcpyPeerAsync goes device to device over xGMI); "copy-staged" (several
 * devices of which at least one pair has NO peer access: the runtime stages those copies through host memory --
 * correct, but PCIe-bound; check the topology).  _note: one line on how the transport was chosen (the librccl
 * version and init call, or why LUMEN_TRANSPORT_AUTO fell back, or the peer-access census). */
const char *lumen_group_transport(const lumen_group *g);
const char *lumen_group_transport_note(const lumen_group *g);
/* ranks the RCCL communicator reports (ncclCommCount); 0 for the copy transports */
uint32_t lumen_group_rccl_ranks(const lumen_group *g);
/* waits for everything enqueued on every local context */
int lumen_group_sync(lumen_group *g);
/* every local rank's whole set from / to its host buffer (hosts[i]: the layout of lumen_set_upload), all transfers
 * enqueued before any is waited for: a process that owns W GPUs moves its W blocks over W PCIe links at once
 * (page-locked buffers; pageable ones are bounced rank by rank).  Returns when the host buffers may be reused /
 * hold the data. */
int lumen_group_upload(lumen_group *g, lumen_set *const *sets, const uint64_t *const *hosts);
int lumen_group_download(lumen_group *g, const lumen_set *const *sets, uint64_t *const *hosts);
/* block p of send[.] (its p-th run of count/W ciphertexts: every layout is ct-major, so a contiguous slice)
 * goes to rank p; block q of recv[.] comes from rank q.  send[i] and recv[i] have the same size. */
int lumen_group_all_to_all(lumen_group *g, const lumen_set *const *send, lumen_set *const *recv);
/* fhe.Encode (fhe/code.go:8-34) of a matrix whose columns are spread over the ranks: matrix[i] = the local
 * rank's block of cols/W full-width columns; encoded[i] receives ITS block of S/W encoded columns, full width.
 * zero_ct: the ONE fresh encryption of zero (code.go:15-22), host [2][nl][N], the same on every rank.
 * Inside: lumen_lanes_split, all-to-all, Encode on the lane shard, all-to-all, lumen_lanes_assemble; for
 * W = 1 plain lumen_encode.  Byte-identical to lumen_encode of the whole matrix on one GPU. */
int lumen_group_encode(lumen_group *g, const lumen_set *const *matrix, const uint64_t *zero_ct,
                       uint32_t rho_inv, lumen_set **encoded);
/* Commit's one exchange (north_star: "a single RCCL all-gather ... to assemble the Merkle leaves"): ends the
 * lumen_leaf_digests_begin job of every local context (same leaf count n on every rank) and all-gathers the
 * digests in rank order = column order; afterwards every rank holds the W*n digests in device memory.
 * lumen_group_merkle_root builds core.NewTree's root over them on the first local rank's device (only the
 * root crosses PCIe); lumen_group_digests copies the W*n*32 bytes to the host, for the process that keeps
 * the tree to answer Merkle paths (core/tree.go:113-163 via lumen_merkle_build). */
int lumen_group_all_gather_digests(lumen_group *g);
int lumen_group_merkle_root(lumen_group *g, uint8_t root[32]);
int lumen_group_digests(lumen_group *g, uint8_t *digests, size_t cap, uint32_t *n_leaves);
/* the query loop of Prove (fhe/ligero.go:268-279) over column-sharded leaves: src[i] = the local rank's block
 * of S/W level-1 columns, idx = n GLOBAL column indices (duplicates allowed).  The owners gather their
 * columns and send them to rank 0, which returns them in query order as *out (a set of rank 0's context);
 * on a process that does not hold rank 0, *out = NULL.
 * Every rank must pass the SAME n and idx[] (each builds its half of the send / receive plan from them; the
 * reference samples them from the one transcript, fhe/ligero.go:261-267).  With one process per GPU
 * (lumen_group_create_rank) the call first all-gathers a fingerprint of (n, idx[]) and fails on every rank that
 * sees a difference, instead of hanging inside RCCL -- in that form it therefore blocks the host for one tiny
 * collective; with all ranks in one process it only enqueues.  The other collectives take their sizes from their
 * arguments' shapes (block size, leaf count), which the ranks of a sharded Commit / Prove share by construction;
 * passing different shapes on different processes is a caller error the library cannot see. */
int lumen_group_gather(lumen_group *g, const lumen_set *const *src, const uint32_t *idx, uint32_t n,
                       lumen_set **out);
/* P(z) over a matrix whose columns are spread over the ranks (lumen_poly_eval_columns, cmd/server/main.go:255-258,
 * core/poly.go:13-45): values[i] / counts[i] = the local rank's block of columns, host [counts[i]][rows], as
 * ServerGroup's witness encryption splits them (rank r's block follows rank r-1's); the counts of all ranks sum to
 * cols.  Every rank evaluates its own block; the partials are summed mod T inside the library and *value = P(z) on
 * every rank.  With one process per GPU (lumen_group_create_rank) the partials, the counts and a fingerprint of
 * (rows, cols, z) travel in one fixed-size all-gather, and a rank whose own arguments or evaluation fail still takes
 * part in it: then every rank returns non-zero, none blocks.  Every rank must pass the same rows, cols and z. */
int lumen_group_poly_eval(lumen_group *g, const uint64_t *const *values, uint32_t rows, const uint32_t *counts,
                          uint32_t cols, uint64_t z, uint64_t *value);
/* HIP-event time of the collectives since the last reset: name = "all_to_all" (lumen_group_all_to_all),
 * "all_to_all_1" / "all_to_all_2" (the two exchanges inside lumen_group_encode), "all_gather", "gather_to_root";
 * ms = sum over calls of the slowest local rank's time on its stream (it includes waiting for the peers to
 * arrive), bytes = what ONE rank sent to other ranks, summed over calls. */
int lumen_group_stats(lumen_group *g, const char *name, double *ms, uint64_t *bytes, uint64_t *calls);
int lumen_group_stats_reset(lumen_group *g);

/* ---- placement diagnostics (tools/ks_mac_placement.py; not on the product path).
 * lumen_ctx_scratch_info: device address and size of one of the context's named scratch buffers ("ks_ext", "ks_u",
 * "ks_coef", "ks_acc2", "ks_acc", ...); *ptr = NULL if it has not been allocated.
 * lumen_ks_mac_probe: HIP-event time of the gadget-product kernel of a key switch (step 3 of Lattigo's hybrid
 * key switching as InnerSum runs it, fhe/ligero.go:325) alone, on caller-chosen device blocks of at least -- ext
 * batch * beta * (L+K) * N, acc batch * 2 * L * N, key beta * 2 * (L+K) * N, u batch * 2 * (L+K) * N words; NULL = the
 * block the library itself uses (batch 0 = the library's batch size).  Contents are irrelevant (data-independent
 * kernel). */
int lumen_ctx_scratch_info(lumen_ctx *ctx, const char *name, void **ptr, size_t *bytes);
/* The fill-and-fence mode of the tests ("LUMEN_ALLOC_FILL", see lumen_ctx_set_tuning): waits for the context's streams
 * and reads back the guard band behind every live guarded block of the context -- its scratch buffers, the sets in its
 * pool and the sets the caller holds.  Fails naming the first damaged block, its size and the offset of the first
 * changed byte behind its end.  With the mode off it returns 0 and touches nothing.  The same check runs, reporting on
 * stderr, whenever a guarded block is released and at lumen_ctx_destroy. */
int lumen_ctx_alloc_check(lumen_ctx *ctx);
int lumen_ks_mac_probe(lumen_ctx *ctx, uint32_t batch, const void *ext, const void *acc, const void *key, void *u,
                       uint32_t reps, float *ms_per_launch);

/* ---- timing on the context's stream (bench.py / roofline) */
int lumen_timer_start(lumen_ctx *ctx);
int lumen_timer_stop(lumen_ctx *ctx, float *elapsed_ms);
/* accumulated HIP-event time and launch count of the limb-NTT kernels since
 * the last reset (measured only while profiling is enabled) */
int lumen_prof_enable(lumen_ctx *ctx, int on);
int lumen_prof_read(lumen_ctx *ctx, const char *kernel, double *total_ms, uint64_t *launches,
                    uint64_t *units);
int lumen_prof_reset(lumen_ctx *ctx);
/* comma-separated names of the kernels that have profile entries; returns the
 * length needed (excluding NUL) */
size_t lumen_prof_names(lumen_ctx *ctx, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
