/* schnorr_sig_amd.h -- C ABI of the MI355X-native batched Schnorr verification engine.
 *
 * Drop-in boundary for the verification path of toposware/schnorr-sig.  The reference has
 * no FFI (`#![deny(unsafe_code)]`, src/lib.rs:152); these entry points are what a Rust
 * `-sys` shim would bind to replace, one for one:
 *
 *   ssa_verify              <- Signature::verify            src/signature.rs:181-205
 *                              (KeyPair::verify_signature   src/signature.rs:159-165,
 *                               PublicKey::verify_signature src/signature.rs:170-176,
 *                               KeyedSignature::verify      src/signature.rs:232-234)
 *   ssa_verify_batch        <- verify_batch                 src/batch.rs:31-50
 *   ssa_verify_batch_msm    <- verify_batch, the reference's own algorithm (random linear
 *                              combination + 2n-point MSM)     src/batch.rs:56-130
 *   ssa_verify_many         <- n x Signature::verify (the per-signature accept/reject vector
 *                              BASELINE.json's north_star asks for)
 *   ssa_verify_many_dedup   <- the same over a slice in which keys repeat: each distinct key is checked once
 *   ssa_verify_many_screened <- the same vector at about the price of one MSM: segments of the batch are screened by
 *                              a random linear combination, each distinct key's subgroup check runs once
 *   ssa_verify_many_cached   <- the same call with a key cache on the device: every distinct public key is checked once,
 *                              not once per batch (ssa_keycache_create).
 *   ssa_verify_keyed_many_cached <- n x KeyedSignature::{from_bytes, verify} (src/signature.rs:230-271) on the 130-byte
 *                              wire records, through a key cache whose key identity is the 49 bytes of
 *                              PublicKey::to_bytes (src/public.rs:49-56): the decompression's square root, the subgroup
 *                              check and the key's table run once per key (SSA_KEYCACHE_WIRE).
 *   ssa_verify_keyed_many_device <- ssa_verify_keyed_many on device buffers
 *   ssa_hash_message_many   <- hash_message                 src/signature.rs:274-306
 *   ssa_rescue_hash_many    <- RescueHash::hash_field       src/signature.rs:303
 *   ssa_verify_keyed_many   <- KeyedSignature::{from_bytes, verify}  src/signature.rs:232-271
 *   ssa_decompress_many     <- PublicKey::from_bytes / AffinePoint::from_compressed
 *                                                           src/public.rs:54-56, src/batch.rs:104
 *   ssa_keygen_sign_many    <- KeyPair::new / KeyPair::sign src/keypair.rs:57-65,
 *                                                           src/signature.rs:114-129
 *   ssa_keygen_sign_many_ex <- the same, constant-time (SSA_FLAG_SIGN_CT) and / or as KeyedSignature records
 *                              (sign_and_bind_pkey + KeyedSignature::to_bytes, src/signature.rs:132-156,237-245)
 *   ssa_pubkey_many         <- PublicKey::from(&PrivateKey) src/public.rs:26-32
 *   ssa_compress_many       <- PublicKey::to_bytes          src/public.rs:49-51
 *   ssa_xprv_master_many    <- ExtendedPrivateKey::generate_master_key   src/derivation.rs:66-82
 *   ssa_xprv_derive_many    <- ExtendedPrivateKey::derive_private / derive_public
 *                                                           src/derivation.rs:88-174
 *   ssa_xpub_derive_many    <- ExtendedPublicKey::derive_normal_public   src/derivation.rs:235-260
 *   ssa_sign_many_indexed   <- KeyPair::sign / sign_and_bind_pkey over a signer set (key pairs held on the device)
 *                                                           src/signature.rs:114-156
 *   status codes            <- SignatureError               src/error.rs:13-18
 *   record sizes            <- src/constants.rs:12-30
 *
 * Data layout (all little-endian, canonical limbs -- pinned by the reference's fixtures,
 * src/signature.rs:387-404, :430-460):
 *   signature  81 B = R.x c0..c5 (6 x u64) | flag byte (ignored by verify, src/signature.rs:186)
 *                     | e (32 B, < q)
 *   public key 96 B = affine x c0..c5 | y c0..c5   (PublicKey.0 is an AffinePoint in memory,
 *                     src/public.rs:24); the 49-B compressed wire form (src/public.rs:49-56) goes through
 *                     ssa_decompress_many / ssa_compress_many, or directly into ssa_verify_keyed_many
 *   messages   either a dense array with a fixed stride, or concatenated bytes + (n+1) offsets
 *
 * Ownership: the caller owns every buffer for the duration of the call; the library keeps
 * no pointer.  A context owns its device memory and one HIP stream; calls on one context
 * must be serialised by the caller, several contexts may be used concurrently.
 * No entry point aborts: inputs on which the reference would panic (non-canonical limbs,
 * src/signature.rs:186; e >= q) get status SSA_MALFORMED.
 */
#ifndef SCHNORR_SIG_AMD_H
#define SCHNORR_SIG_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSA_SIGNATURE_LENGTH 81   /* src/constants.rs:27 */
#define SSA_AFFINE_PK_LENGTH 96   /* 2 x BASEFIELD_LENGTH, src/constants.rs:18 */
#define SSA_SCALAR_LENGTH 32      /* src/constants.rs:12 */
#define SSA_PUBLIC_KEY_LENGTH 49  /* compressed wire form, src/constants.rs:21 */
#define SSA_DIGEST_LENGTH 32      /* hash_message output, src/signature.rs:274 */
#define SSA_PARAMS_LENGTH 2816

/* per-signature status (src/error.rs:13-18) */
#define SSA_OK 0
#define SSA_INVALID_PUBLIC_KEY 1  /* SignatureError::InvalidPublicKey */
#define SSA_INVALID_SIGNATURE 2   /* SignatureError::InvalidSignature */
#define SSA_MALFORMED 3           /* the reference would panic on this input */

/* API return codes (negative = the call itself failed) */
#define SSA_ERR_ARG (-1)
#define SSA_ERR_HIP (-2)
#define SSA_ERR_PARAMS (-3)
#define SSA_ERR_NO_DEVICE (-4)
#define SSA_ERR_TABLE (-5)        /* a precomputed table failed its self-check (ssa_ctx_selfcheck) */

/* flags */
#define SSA_MAX_BATCH ((size_t)1 << 30)   /* signatures per call; larger n returns SSA_ERR_ARG.  Device memory does not grow
                                             with n, for device-pointer AND host-buffer entry points: workspaces and
                                             staging are sized for slices of 2^20 lanes (4.4 GB of tables + 0.3 GB of
                                             staging per slice in flight, at most two; SSA_LANE_SLICE), resp. 2^23
                                             signatures of the MSM form (SSA_MSM_SLICE).  The host-buffer entry points
                                             copy the caller's bytes through page-locked bounce buffers of the library's,
                                             the size of one slice's inputs (0.3 GB, resp. 2.2 GB for a full MSM slice);
                                             the caller's memory is never registered with the runtime */
#define SSA_FLAG_FORCE_LANE 2u    /* always the throughput kernels (one signature per lane) */
#define SSA_FLAG_FORCE_COOP 4u    /* always the low-latency kernel (one wave per signature) */
#define SSA_FLAG_CHECK_TORSION 1u /* Signature::verify semantics (src/signature.rs:182-184);
                                     off = verify_batch semantics (src/batch.rs has no check) */
#define SSA_FLAG_SIG_FLAG_BYTE 8u /* verify_batch semantics for byte 48 of the signature: the reference decompresses R
                                     with its flag byte (from_compressed(&sig.x).unwrap(), src/batch.rs:104), so a
                                     signature only verifies for the R the flags select: wrong sort bit (bit 6) or an
                                     infinity bit (bit 7) that does not match the recomputed R -> SSA_INVALID_SIGNATURE,
                                     an undecodable flag byte -> SSA_MALFORMED (the reference panics).  Off =
                                     Signature::verify, which ignores the byte (src/signature.rs:186) */

typedef struct ssa_ctx ssa_ctx;

/* Parameter blob (Rescue-Prime instance + generator), see schnorr-sig_amd/params/gen_params.py.
 *   char magic[8] = "SSAPARM1"; u32 n_rounds, rate_off; i32 cap_len_idx; u32 pad_mode,
 *   digest_off, flags; u64 mds[144]; u64 ark1[8][12]; u64 ark2[8][12]; u64 gen_x[6], gen_y[6]
 * params == NULL selects the built-in default blob -- the builder's own Rescue constants and generator, NOT
 * upstream's (they live in un-vendored crates; DESIGN.md "parity unpinned"): such a context rejects every genuine
 * toposware signature and ssa_ctx_uses_default_params() returns 1 for it.  tools/blob_from_upstream.py builds the
 * blob from upstream's constants.  The generator is validated on the device (on the curve, [q]G == O):
 * SSA_ERR_PARAMS otherwise.  Device memory: the fixed-base comb table of the generator (the reference's const
 * BASEPOINT_TABLE, src/signature.rs:20,116, src/batch.rs:98-100) is sized by the context -- see ssa_ctx_create_ex --,
 * one per device, generator and geometry, shared by all the contexts of the process; the per-lane workspaces grow to
 * 4.4 GB with the first large batch (slices of 2^20 lanes, whatever the batch size), twice that once a call of more than
 * one slice has used the second internal stream. */
int ssa_ctx_create(ssa_ctx **out, int device, const void *params, size_t params_len);
/* The same with the speed-for-memory trade chosen by the caller.
 *   gtab_bits         window width of the comb for G: 24 (11 windows, 17.7 GB: [e]G = 11 additions), 22 (12, 4.8 GB),
 *                     20 (13, 1.3 GB) or 16 (16, 100 MB; ssa_k_verify +1.9 %); 0 = the widest whose table fits the budget
 *                     (environment: SSA_GTAB_BITS).  Results are identical for every width.
 *   hbm_budget_bytes  what the tables that only buy speed may take on the device -- the comb for G, the per-key combs of
 *                     an SSA_KEYSET_AUTO key set; 0 = a tenth of the memory that is free when the context is created
 *                     (environment: SSA_HBM_BUDGET_MB).
 * An allocation that fails is not an error while a smaller table exists: the context falls back width by width down
 * to the 100 MB comb (ssa_ctx_info says what it got). */
int ssa_ctx_create_ex(ssa_ctx **out, int device, const void *params, size_t params_len, uint32_t gtab_bits,
                      uint64_t hbm_budget_bytes);
/* What the context holds on the device: out[0] window bits and out[1] windows of the comb for G, out[2] its bytes,
 * out[3] bytes of this context's workspaces and staging buffers as reserved so far, out[4] lanes per slice of the
 * per-lane kernels, out[5] signatures per slice of the MSM form, out[6] the HBM budget, out[7] 1 when calls of more than
 * one slice alternate their slices between two internal streams (SSA_TWO_STREAMS=0 turns that off). */
int ssa_ctx_info(const ssa_ctx *ctx, uint64_t out[8]);
/* Exact self-check of the context's precomputed tables, on the context's stream; returns when it is done.  Every row of
 * the comb for G (the table every verification, the throughput signer and xpub derivation walk) and, once the first
 * constant-time signature has built it, every row of the constant-time signer's table is checked against the rows
 * before it: a clean result proves each row equal to its multiple of G.  flags must be 0.
 * Returns SSA_OK when both are clean, SSA_ERR_TABLE when a row is wrong, SSA_ERR_ARG / SSA_ERR_HIP as usual.
 *   out[0] comb rows checked (windows x 2^bits)      out[4] constant-time rows that fail
 *   out[1] comb rows that fail                       out[5] first failing constant-time row (UINT64_MAX: none)
 *   out[2] first failing comb row (UINT64_MAX: none) out[6] builds the comb took (1; 2 after a rebuild at creation)
 *   out[3] constant-time rows checked (0 before it is built, or while the comb fails; else 1026)
 *                                                    out[7] window bits of the comb
 * Tables are checked when they are built, too: ssa_ctx_create_ex rebuilds a comb that fails once, falls back to the
 * next smaller width when it fails again and returns SSA_ERR_TABLE when no width gives a clean table; a constant-time
 * table that fails twice makes the signing call return SSA_ERR_TABLE.  A comb that fails here is RETIRED: contexts
 * created afterwards build and check a new one.  Contexts that hold the failed comb (this one and any other of the
 * process on the same device and geometry) keep computing with it -- destroy them.  A constant-time table that fails
 * here is rebuilt (and checked) by the next constant-time call.  Long-lived services should run this periodically
 * (INTEGRATION.md gives its cost per width). */
int ssa_ctx_selfcheck(ssa_ctx *ctx, uint32_t flags, uint64_t out[8]);
/* 1 when the context was created from the built-in blob (parity with upstream unpinned), 0 for a caller-supplied one */
int ssa_ctx_uses_default_params(const ssa_ctx *ctx);
void ssa_ctx_destroy(ssa_ctx *ctx);
const char *ssa_strerror(int rc);
/* the built-in blob (SSA_PARAMS_LENGTH bytes) */
const void *ssa_default_params(void);
/* Ordering against a stream of the caller WITHOUT a host synchronisation.  Every *_device entry point only ENQUEUES
 * on the context's stream (its own non-blocking stream unless ssa_ctx_set_stream changed it): its outputs are valid for
 * other streams only after one of ssa_ctx_sync, ssa_ctx_stream_release, or a shared stream.
 *   ssa_ctx_stream_release(ctx, s): stream s waits for everything enqueued on the context so far (publish outputs to s);
 *   ssa_ctx_stream_acquire(ctx, s): the context's stream waits for everything enqueued on s so far (inputs written on s,
 *                                   e.g. by a collective, are visible to the next call on the context). */
int ssa_ctx_stream_release(ssa_ctx *ctx, void *consumer_hip_stream);
int ssa_ctx_stream_acquire(ssa_ctx *ctx, void *producer_hip_stream);
/* make the context issue its work on an existing hipStream_t.  NULL = back to the context's own (non-blocking)
 * stream; to select the legacy null stream pass HIP's own handle for it, hipStreamLegacy (or hipStreamPerThread). */
int ssa_ctx_set_stream(ssa_ctx *ctx, void *hip_stream);
/* average duration (ms) of the `ssa_k_verify` launches since the last call, measured with
 * hipEvents on the context's stream when profiling is on; resets the statistics.  A one-slice call that ran as two
 * parts on two streams counts as ONE launch per key: its entry runs from the earlier start to
 * the later end of the two launches of that kernel.  The ssa_k_hash and ssa_k_verify entries of such a call overlap
 * by design, so they do not add up to the call's time and neither describes an exclusive launch. */
int ssa_ctx_enable_timing(ssa_ctx *ctx, int on);
int ssa_ctx_read_timing(ssa_ctx *ctx, const char *kernel, double *avg_ms, uint64_t *launches);

/* ---- host-buffer entry points (what the Rust shim binds) ----------------------------- */

/* Signature::verify for one signature.  Returns a status code. */
int ssa_verify(ssa_ctx *ctx, const uint8_t sig[SSA_SIGNATURE_LENGTH],
               const uint8_t pk[SSA_AFFINE_PK_LENGTH], const uint8_t *msg, size_t msg_len,
               uint32_t flags);

/* n independent verifications; status_out[i] in {0,1,2,3}; *n_fail_out = #(status != 0).
 * msg_off != NULL: message i = msgs[msg_off[i] .. msg_off[i+1]);
 * msg_off == NULL: message i = msgs[i*msg_stride .. i*msg_stride + msg_len).
 * pk_inf (optional, n bytes): non-zero marks pk i as the identity. */
int ssa_verify_many(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                    const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                    size_t msg_len, size_t n, uint32_t flags, uint8_t *status_out,
                    uint64_t *n_fail_out);

/* verify_batch: one verdict for the batch = AND of the per-signature verdicts (equal to the
 * reference's MSM verdict on honest and on corrupted-but-well-formed inputs; divergence
 * classes are listed in DESIGN.md).  Returns SSA_OK, SSA_INVALID_SIGNATURE (or
 * SSA_INVALID_PUBLIC_KEY with SSA_FLAG_CHECK_TORSION, SSA_MALFORMED) -- the smallest
 * non-zero status present.  n == 0 returns SSA_OK like the reference.  SSA_FLAG_SIG_FLAG_BYTE is always on
 * here (the reference's verify_batch honours the flag byte); pk_inf as in ssa_verify_many: an identity key is a
 * valid PublicKey (src/public.rs:95-101) and contributes nothing to the equation (src/batch.rs:106). */
int ssa_verify_batch(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                     const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                     size_t n, uint32_t flags);

/* verify_batch exactly as src/batch.rs:31-130: sum s_i R_i - sum (s_i h_i) P_i ?= [sum s_i e_i] G with
 * R_i decompressed from sig.x (flag byte honoured), a 2n-point bucket MSM on the GPU and an x-only
 * comparison.  coeffs: n x 32-byte scalars standing in for Scalar::random(rng) (reduced mod q), or
 * NULL for 128-bit coefficients from a ChaCha20 stream (RFC 8439) generated on the device and keyed per
 * call with getrandom(2).  Returns SSA_OK, SSA_INVALID_SIGNATURE, or
 * SSA_MALFORMED where the reference panics (undecodable sig.x, src/batch.rs:67,104).  No torsion
 * check, like the reference.  Any n <= SSA_MAX_BATCH: above 2^23 signatures (SSA_MSM_SLICE) the batch runs slice after slice,
 * each reduced to its record like a shard, the records added up (src/batch.rs:98-129) -- bounded device memory. */
int ssa_verify_batch_msm(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                         const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                         size_t n, const uint8_t *coeffs);

/* Screened batch verification: a per-signature status vector at close to the price of one MSM verdict (DESIGN.md
 * section 13).  The MSM of ssa_verify_batch_msm, with its buckets keyed by (window, segment, digit), gives one sum per
 * contiguous segment of the batch in one pass.  A segment whose sum is the identity is accepted as a whole; only the
 * lanes of failing segments run the exact per-lane check, on the challenge scalars the MSM already computed.
 * status_out[i] is 0, 2 or 3 with verify_batch semantics: the flag byte is honoured (SSA_FLAG_SIG_FLAG_BYTE), there is
 * no subgroup check, and pk_inf marks identity keys, exactly as ssa_verify_batch.
 *   - 3 (SSA_MALFORMED) exactly on the lanes where ssa_verify_many(..., SSA_FLAG_SIG_FLAG_BYTE) says 3: non-canonical
 *     limbs, e >= q, a key off the curve, an undecodable sig.x or flag byte.  Such lanes add nothing to any segment.
 *   - A lane the per-lane check accepts is never rejected: its E_i = R_i - [h_i]P_i - [e_i]G is exactly O, so a segment
 *     of valid lanes always passes, and a lane in a failing segment gets its per-lane status.
 *   - A lane the per-lane check rejects gets that status (2, or 3 as above) UNLESS its segment's random combination
 *     vanishes, sum s_i E_i = O over the segment: the soundness of the reference's verify_batch (DESIGN.md section 1,
 *     divergence class 1) -- about 2^-128 for an error with a prime-order component, but 1/l for an error of pure small
 *     order l (2, 5, ...: reachable only with keys or R outside the prime-order subgroup).  A small-order part of P_i
 *     enters the sum through the reduced scalar s_i h_i mod q, as in the reference (src/batch.rs:109-111): with a key
 *     P + T2 (T2 of order 2) the lane is reported exactly when s_i h_i mod q is odd.  A segment is checked as the
 *     point equation sum s_i R_i - sum s_i h_i P_i == [sum s_i e_i] G, not x-only: the global-sign divergence of the
 *     MSM form (class 2) does not occur, a segment in which every e is replaced by q - e fails.
 * coeffs: n x 32-byte coefficients (mod q, as ssa_verify_batch_msm), or NULL for 128-bit coefficients drawn on the
 * device (ChaCha20 keyed with getrandom(2)).  For given inputs and coefficients the result does not depend on the
 * number of segments.  n <= the context's small-batch bound (SSA_MSM_SMALL_MAX, 3072 by default): the exact per-lane
 * path, as ssa_verify_many with SSA_FLAG_SIG_FLAG_BYTE.  Above SSA_MSM_SLICE signatures the batch is screened slice by
 * slice; segments never straddle two slices.  n == 0 returns SSA_OK.  Return code and *n_fail_out (the number of
 * nonzero statuses) as ssa_verify_many.  Host buffers go through the library's staging, caller memory is not
 * registered. */
int ssa_verify_batch_screened(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                              const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                              size_t n, const uint8_t *coeffs, uint8_t *status_out, uint64_t *n_fail_out);

/* hash_message for n (R.x, pk, message) triples -> n x 32-byte digests */
int ssa_hash_message_many(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks,
                          const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                          size_t msg_len, size_t n, uint8_t *digests_out);

/* Rescue-Prime hash_field over n rows of `felts_per_row` canonical u64 -> n x 4 felts */
int ssa_rescue_hash_many(ssa_ctx *ctx, const uint64_t *felts, uint32_t felts_per_row, size_t n,
                         uint64_t *digests_out);

/* pk_i = [sk_i]G (affine, 96 B) and sig_i = sign(sk_i, nonce_i, msg_i).  Secret keys and nonces are 32-byte LE
 * CANONICAL scalars in [1, q): 0 and values >= q return SSA_ERR_ARG (PrivateKey::new / Scalar::random never
 * produce them, src/private.rs:49-57).  Drawing them uniformly is the caller's job -- 64 random bytes reduced
 * mod q, as the C++ and Python mirrors do; 32 random bytes reduced mod q are biased (2^256 / q ~ 2.08) and leak the
 * key through the nonces.  The kernel is VARIABLE-TIME in the secrets (comb windows equal to zero are skipped and the
 * table is indexed by secret windows), like the reference's *_vartime verification calls but unlike its signing:
 * use it where timing side channels are out of scope (test-input generation, trusted hosts).
 * The _device form cannot report errors per lane: non-canonical inputs are reduced mod q there. */
int ssa_keygen_sign_many(ssa_ctx *ctx, const uint8_t *sks, const uint8_t *nonces,
                         const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                         size_t msg_len, size_t n, uint8_t *pks_out, uint8_t *sigs_out);

/* The signing side with options (KeyPair::sign / sign_and_bind_pkey, src/signature.rs:114-156; PrivateKey::sign,
 * :65-110).  flags:
 *   SSA_FLAG_SIGN_CT     constant-time in the secrets, like the reference's `&BASEPOINT_TABLE * r` and Scalar::from_bits
 *                        (src/signature.rs:67,116,123): fixed 4-bit windows over a 98 KB table that is read in full for
 *                        every window (the entry is selected, never indexed), no skipped window, generic additions from a
 *                        public offset point with no exceptional-case branch, masked scalar arithmetic, compiled (branch-
 *                        free) field blocks.  Same bytes out as the throughput signer; about 5x its time.  A lane whose
 *                        addition meets an exceptional input (probability ~2^-250; surely only for a scalar that reduces
 *                        to 0, which the host form refuses) is recomputed by the exact variable-time code.
 *   SSA_FLAG_SIGN_KEYED  sigs_out receives n x 130-byte KeyedSignature records pk(49, compressed) || sig(81)
 *                        (KeyedSignature::to_bytes, src/signature.rs:237-245) instead of n x 81 bytes; pks_out may be
 *                        NULL then.
 * The host form checks the scalars (canonical, non-zero: SSA_ERR_ARG otherwise) in time independent of their values
 * and wipes its device copies of them before it returns.  ssa_keygen_sign_many[_device] = flags 0. */
#define SSA_FLAG_SIGN_CT 16u
#define SSA_FLAG_SIGN_KEYED 32u
int ssa_keygen_sign_many_ex(ssa_ctx *ctx, const uint8_t *sks, const uint8_t *nonces, const uint8_t *msgs,
                            const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n, uint32_t flags,
                            uint8_t *pks_out, uint8_t *sigs_out);

/* PublicKey::from(&PrivateKey) (src/public.rs:26-32; KeyPair::from_bytes / from_seed re-derive the key the same way,
 * src/keypair.rs:73-103): pks_out[i] = [sks[i]]G as 96-byte affine points -- ONE constant-time base multiplication per
 * key (the signer's table and window code) and nothing else derived from the secret: no nonce, no response scalar.
 * The host form checks the scalars (canonical, non-zero: SSA_ERR_ARG otherwise) in time independent of their values and
 * wipes its device copy before it returns; the _device form computes [sk mod q]G for any 32 bytes, through the
 * variable-time fallback when sk reduces to 0. */
int ssa_pubkey_many(ssa_ctx *ctx, const uint8_t *sks, size_t n, uint8_t *pks_out);

/* PublicKey::to_bytes (AffinePoint::to_compressed, src/public.rs:49-51): n x 96-byte affine points -> n x 49 bytes
 * x || flag byte (bit 7: the identity, [0; 48] || 0x80, src/public.rs:95-101 -- marked by pk_inf[i] != 0, optional; bit 6:
 * the sort flag of y).  status_out (optional): 0, or SSA_MALFORMED for a limb that is not canonical. */
int ssa_compress_many(ssa_ctx *ctx, const uint8_t *pks, const uint8_t *pk_inf, size_t n, uint8_t *out,
                      uint8_t *status_out);

/* ---- hierarchical deterministic key derivation (src/derivation.rs) ---------------------------------------------
 * An extended private key is sk(32, little-endian, canonical, non-zero) || chain code(32); an extended public key is
 * the compressed key(49) || chain code(32).  An index is a uint32_t whose little-endian bytes are the reference's
 * &[u8; 4]; it is hardened when bit 31 is set.  Every child is one HMAC-SHA512 keyed by its parent's chain code (the
 * key's ipad / opad states are computed once per parent: two SHA-512 compressions per child) and one base
 * multiplication.  parse(I_L) = Scalar::from_bytes_non_canonical is read as the full reduction mod q of the 256-bit
 * little-endian value.
 * Parents: when parent_idx is NULL, m is 1 (every child of one parent) or n (child i of parent i); otherwise child i
 * derives from parent parent_idx[i], and an index >= m gives SSA_MALFORMED on that lane.
 * status_out[i]: 0 ok, 1 the reference's CtOption is none (child key 0, hardened index on an xpub, T = O),
 * SSA_MALFORMED the parent does not decode (ExtendedPrivateKey::from_bytes / ExtendedPublicKey::from_bytes is none).
 * Lanes whose status is not 0 get all-zero outputs.  n <= SSA_MAX_BATCH (n == 0 is a no-op). */
#define SSA_CHAIN_CODE_LENGTH 32
#define SSA_EXTENDED_PRIVATE_KEY_LENGTH 64
#define SSA_EXTENDED_PUBLIC_KEY_LENGTH 81
#define SSA_FLAG_DERIVE_PUBLIC 64u   /* xprv -> xpub children (derive_public) */

/* ExtendedPrivateKey::generate_master_key (src/derivation.rs:66-82): HMAC-SHA512(b"Cheetah - Master extended key
 * seed", seed) for n 32-byte seeds -> n x 64-byte xprvs; status 1 when the key reduces to 0.  Constant-time in the
 * seeds; the host form wipes its device copies of seeds and keys before it returns. */
int ssa_xprv_master_many(ssa_ctx *ctx, const uint8_t *seeds, size_t n, uint8_t *xprvs_out, uint8_t *status_out);

/* ExtendedPrivateKey::derive_private (src/derivation.rs:88-154) and, with SSA_FLAG_DERIVE_PUBLIC, derive_public
 * (:160-174): m parents (m x 64) -> n children, n x 64 bytes (sk || cc') or n x 81 (compress([sk]G) || cc').
 * Constant-time in every secret (keys, chain codes, the hardened bit selects the message without a branch); the
 * host form wipes its device copies of parents and children, and every call its per-parent records, before it
 * returns. */
int ssa_xprv_derive_many(ssa_ctx *ctx, const uint8_t *parents, size_t m, const uint32_t *parent_idx,
                         const uint32_t *indices, size_t n, uint32_t flags, uint8_t *children_out,
                         uint8_t *status_out);

/* ExtendedPublicKey::derive_normal_public (src/derivation.rs:235-260): m parents (m x 81) -> n x 81 children and,
 * optionally, the children's 96-byte affine keys (pks_out: what ssa_verify_many and key sets take; zero for the
 * identity) and identity flags (pk_inf_out: a child equal to the identity is valid and encodes as [0; 48] || 0x80).
 * Variable-time: everything here is public. */
int ssa_xpub_derive_many(ssa_ctx *ctx, const uint8_t *parents, size_t m, const uint32_t *parent_idx,
                         const uint32_t *indices, size_t n, uint8_t *children_out, uint8_t *pks_out,
                         uint8_t *pk_inf_out, uint8_t *status_out);

/* the SHA-512 / HMAC code of the derivation kernels on its own (not part of the reference API): n MACs
 * HMAC-SHA512(key, msgs[i]) -> n x 64 bytes.  key_len <= 256 (keys longer than 128 bytes are hashed first, RFC 2104),
 * msg_len <= 239 (messages of i * msg_len .. (i + 1) * msg_len). */
int ssa_debug_hmac_sha512(ssa_ctx *ctx, const uint8_t *key, size_t key_len, const uint8_t *msgs, size_t msg_len,
                          size_t n, uint8_t *out);

#define SSA_KEYED_SIGNATURE_LENGTH 130  /* src/constants.rs:30 */
/* n x KeyedSignature::verify on the 130-byte wire form pk(49, compressed) || sig(81)
 * (src/signature.rs:232-271): the key is decompressed on the GPU, then verified as ssa_verify_many.
 * A record whose key or scalar does not decode (KeyedSignature::from_bytes is_none) gets SSA_MALFORMED. */
int ssa_verify_keyed_many(ssa_ctx *ctx, const uint8_t *keyed, const uint8_t *msgs, const uint64_t *msg_off,
                          size_t msg_stride, size_t msg_len, size_t n, uint32_t flags, uint8_t *status_out,
                          uint64_t *n_fail_out);

/* PublicKey::from_bytes (src/public.rs:54-56): n x 49-byte compressed points (48 bytes of x, flag
 * byte: bit 7 = infinity, bit 6 = sort flag, other bits clear) -> n x 96-byte affine points.
 * status_out[i] = 0 ok, 1 "decompression failed" (CtOption is_none); pk_inf_out[i] (optional) = 1
 * for the identity encoding [0;48] || 0x80 (src/public.rs:95-101). */
int ssa_decompress_many(ssa_ctx *ctx, const uint8_t *compressed, size_t n, uint8_t *pks_out,
                        uint8_t *pk_inf_out, uint8_t *status_out);

/* ---- device-buffer entry points: same semantics, every pointer is a device pointer ----
 * (work is enqueued on the context's stream; outputs are valid after ssa_ctx_sync) */
int ssa_verify_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                           const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                           const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                           uint32_t flags, uint8_t *d_status_out, uint64_t *d_n_fail_out);
int ssa_hash_message_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                 const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                 size_t msg_stride, size_t msg_len, size_t n,
                                 uint8_t *d_digests_out);
int ssa_rescue_hash_many_device(ssa_ctx *ctx, const uint64_t *d_felts, uint32_t felts_per_row,
                                size_t n, uint64_t *d_digests_out);
int ssa_keygen_sign_many_device(ssa_ctx *ctx, const uint8_t *d_sks, const uint8_t *d_nonces,
                                const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                size_t msg_stride, size_t msg_len, size_t n, uint8_t *d_pks_out,
                                uint8_t *d_sigs_out);
int ssa_decompress_many_device(ssa_ctx *ctx, const uint8_t *d_compressed, size_t n, uint8_t *d_pks_out,
                               uint8_t *d_pk_inf_out, uint8_t *d_status_out);
/* (cannot report errors per lane: scalars are reduced mod q; d_pks_out may be NULL with SSA_FLAG_SIGN_KEYED.
 *  PRECONDITION of SSA_FLAG_SIGN_CT on device buffers: every sk and nonce is canonical and non-zero -- what the host form
 *  checks; a scalar that reduces to 0 is still signed correctly, but by the variable-time fallback) */
int ssa_keygen_sign_many_ex_device(ssa_ctx *ctx, const uint8_t *d_sks, const uint8_t *d_nonces, const uint8_t *d_msgs,
                                   const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                   uint32_t flags, uint8_t *d_pks_out, uint8_t *d_sigs_out);
int ssa_pubkey_many_device(ssa_ctx *ctx, const uint8_t *d_sks, size_t n, uint8_t *d_pks_out);
int ssa_compress_many_device(ssa_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t n, uint8_t *d_out,
                             uint8_t *d_status_out);
/* key derivation (src/derivation.rs): the device forms wipe the per-parent records, not the caller's buffers */
int ssa_xprv_master_many_device(ssa_ctx *ctx, const uint8_t *d_seeds, size_t n, uint8_t *d_xprvs_out,
                                uint8_t *d_status_out);
int ssa_xprv_derive_many_device(ssa_ctx *ctx, const uint8_t *d_parents, size_t m, const uint32_t *d_parent_idx,
                                const uint32_t *d_indices, size_t n, uint32_t flags, uint8_t *d_children_out,
                                uint8_t *d_status_out);
int ssa_xpub_derive_many_device(ssa_ctx *ctx, const uint8_t *d_parents, size_t m, const uint32_t *d_parent_idx,
                                const uint32_t *d_indices, size_t n, uint8_t *d_children_out, uint8_t *d_pks_out,
                                uint8_t *d_pk_inf_out, uint8_t *d_status_out);
/* coeff_bytes in 1..32: little-endian coefficient width (d_coeffs == NULL: the library draws 128-bit
 * coefficients as above); *d_verdict_out receives the status.  A 32-byte coefficient is taken mod q (Scalar::random,
 * src/batch.rs:75-78).  A narrower one is recoded into signed digits over its own windows only, so a value that fills
 * them to the top (above 0x7fff...7fff with 16-bit windows, n >= 4096; above 0x7f7f...7f with 8-bit ones) stands for
 * raw - 2^(8 coeff_bytes): the SAME value multiplies R_i, h_i and e_i, so the equation is the reference's with another,
 * equally random, coefficient (tests/test_gpu_round4.py pins the rule against the oracle). */
int ssa_verify_batch_msm_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                size_t msg_len, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                                uint32_t *d_verdict_out);
/* The device form of ssa_verify_batch_screened.  d_coeffs: n x coeff_bytes (1..32) as ssa_verify_batch_msm_device, or
 * NULL (library-drawn).  *d_n_fail_out (device, may be NULL) receives the number of nonzero statuses.  Unlike the other
 * _device forms this one SYNCHRONISES the context's stream once per slice of SSA_MSM_SLICE signatures (once for any
 * batch of up to 2^23), to read back the segment verdicts (at most 256 bytes) and size the re-check of the failing
 * segments; the statuses and the count are ordered on the context's stream like any other _device result. */
int ssa_verify_batch_screened_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                     const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                     size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes, uint8_t *d_status_out,
                                     uint64_t *d_n_fail_out);
int ssa_ctx_sync(ssa_ctx *ctx);

/* ---- keyed context: many signatures by few signers (validator sets) ---------------------------------
 * A key set runs once per KEY what Signature::verify runs per signature on the key: canonical-limb and on-curve
 * checks, the subgroup check [q]P == O (src/signature.rs:182-184) and the table of multiples the ladder needs.
 * ssa_verify_many_indexed then verifies signature i against key key_idx[i] starting at the ladder.  Same
 * statuses as ssa_verify_many (a key that failed its subgroup check gives SSA_INVALID_PUBLIC_KEY under
 * SSA_FLAG_CHECK_TORSION; an index >= m gives SSA_MALFORMED).  A key set belongs to the context it was created
 * on.  Destroy it before the context; one that outlives its context is orphaned by ssa_ctx_destroy (its tables are
 * freed there, every call on it but ssa_keyset_destroy returns SSA_ERR_ARG), never a dangling pointer. */
typedef struct ssa_keyset ssa_keyset;
/* table kind: SSA_KEYSET_LADDER keeps sixteen multiples per key (4 KB; verification runs the 250-doubling ladder),
 * SSA_KEYSET_COMB a comb of [d * 2^(16w)]P, w < 16, d < 65536 per key (100 MB; [h]P becomes 16 mixed additions, no
 * doublings -- about 8x less curve work per signature), SSA_KEYSET_AUTO the comb while all tables fit 16 GB (160 keys) */
#define SSA_KEYSET_AUTO 0u
#define SSA_KEYSET_COMB 1u
#define SSA_KEYSET_LADDER 2u
int ssa_keyset_create(ssa_ctx *ctx, const uint8_t *pks, const uint8_t *pk_inf, size_t m, uint32_t flags,
                      ssa_keyset **out);
int ssa_keyset_create_device(ssa_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t m, uint32_t flags,
                             ssa_keyset **out);
void ssa_keyset_destroy(ssa_keyset *ks);
/* per-key status (m bytes): 0 usable, 1 not in the prime subgroup, 3 malformed */
int ssa_keyset_status(ssa_keyset *ks, uint8_t *status_out);
int ssa_verify_many_indexed(ssa_ctx *ctx, ssa_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                            const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                            size_t n, uint32_t flags, uint8_t *status_out, uint64_t *n_fail_out);
int ssa_verify_many_indexed_device(ssa_ctx *ctx, ssa_keyset *ks, const uint32_t *d_key_idx, const uint8_t *d_sigs,
                                   const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                   size_t msg_len, size_t n, uint32_t flags, uint8_t *d_status_out,
                                   uint64_t *d_n_fail_out);

/* ---- ssa_verify_many with each DISTINCT public key of a slice checked once --------------
 * Real batches repeat keys (a block or a mempool holds many signatures by far fewer accounts; the reference's own batch
 * test reuses keys, src/batch.rs:152-175), and the subgroup check [q]P == O of SSA_FLAG_CHECK_TORSION -- about 40 % of
 * that mode's time -- depends on the key alone.  These calls take the arguments of ssa_verify_many[_device] and return
 * the same status vector, lane for lane, and the same *n_fail_out, for any flags: no key set, no handle, no index from
 * the caller, no allocation per call.  Per slice of at most SSA_LANE_SLICE lanes the device finds the distinct keys
 * (two lanes share a key only when their 96 key bytes are equal AND their pk_inf flags agree as booleans: equality is
 * decided on the bytes; a keyed 64-bit fingerprint only picks the candidates), runs the limb, curve and subgroup
 * checks and the table of sixteen multiples once per distinct key, and starts every lane at the ladder.
 * Non-canonical and off-curve keys take part like any other bytes: they are found malformed once, and every lane
 * that holds them is SSA_MALFORMED.
 *   - Policy per slice (u: its distinct keys), from the measured table of DESIGN.md section 14.  With
 *     SSA_FLAG_CHECK_TORSION the keyed route is taken whenever u < lanes: it was faster at every u measured below all-
 *     distinct (2^20 lanes: 34.7 ms against 56.7 at u = lanes / 16, 45.3 at lanes / 2); a slice of all-distinct keys
 *     takes the path of ssa_verify_many, having paid for the dedup (+0.2 ms per 2^20 lanes: why these calls are
 *     opt-in).  Without the flag there is no subgroup check to save and the keyed route measured slower at every u:
 *     every slice takes the path of ssa_verify_many, and the dedup runs only when stats_out asks for the count.
 *   - SSA_FLAG_FORCE_COOP, and batches that ssa_verify_many would hand to the cooperative kernel (n <= 7680, or
 *     n <= 10496 with SSA_FLAG_CHECK_TORSION, unless SSA_FLAG_FORCE_LANE is set), take the path of ssa_verify_many
 *     unchanged; their keys are counted only when stats_out is given.
 *   - Both forms read u back once per slice: the _device form synchronises the context's stream once per slice (as the
 *     screened form does) and runs the slices of a larger batch one after the other on that stream.
 * stats_out (optional, HOST memory in both forms): [0] distinct keys summed over the slices, [1] slices that took the
 * keyed route, [2] slices that fell back (or went to the cooperative kernel), [3] lanes that hit the probe bound of the
 * dedup table and became keys of their own -- always correct, it only costs time (0 on honest inputs). */
int ssa_verify_many_dedup(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                          const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                          uint32_t flags, uint8_t *status_out, uint64_t *n_fail_out, uint64_t stats_out[4]);
int ssa_verify_many_dedup_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                 const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                 size_t n, uint32_t flags, uint8_t *d_status_out, uint64_t *d_n_fail_out,
                                 uint64_t stats_out[4]);

/* ---- Signature::verify screened: the status vector of ssa_verify_many at about the price of one MSM (DESIGN.md
 * section 15) ------------------------------------------------------------------------------------------------------
 * The screen of ssa_verify_batch_screened under the semantics of ssa_verify_many.  flags: any combination of
 * SSA_FLAG_CHECK_TORSION and SSA_FLAG_SIG_FLAG_BYTE (any other bit: SSA_ERR_ARG).  SSA_FLAG_CHECK_TORSION alone is
 * Signature::verify (src/signature.rs:181-205).  SSA_FLAG_SIG_FLAG_BYTE alone IS ssa_verify_batch_screened: the call
 * is handed to it and stats_out stays zero.  For the other three settings, per slice of at most SSA_LANE_SLICE lanes
 * (2^20; segments never straddle slices):
 *   1. the distinct keys of the slice are found as ssa_verify_many_dedup finds them, and the limb, curve and subgroup
 *      checks and the table of sixteen multiples run once per distinct key;
 *   2. the segments of the slice (256 of 4096 lanes at 2^20) are screened by the segmented MSM, on points as in
 *      ssa_verify_batch_screened;
 *   3. the lanes of failing segments, and the lanes that could not be screened, run the exact keyed kernel (no subgroup
 *      work, no table build per lane) on the challenge scalars the screen hashed.  If they are more than half the
 *      slice, that kernel runs over the whole slice in place.
 * status_out[i] is the status ssa_verify_many gives lane i for the same inputs and flags (0, 1, 2 or 3, in the order
 * of src/signature.rs:182-186: the key first, then the signature), with one exception:
 *   - A lane the exact check accepts is never rejected.
 *   - The screen only ever ACCEPTS.  Every nonzero status is written by the exact kernel.
 *   - A lane that cannot be screened gets no status from the screen: it is left out of its segment's sums (it does not
 *     make the segment fail) and is re-checked exactly.  Those are the lanes whose key the per-key check refused
 *     (malformed, or outside the prime-order subgroup -- with or without SSA_FLAG_CHECK_TORSION: the per-key check
 *     computes [q]P == O anyway, so no key outside the subgroup ever enters a sum; without the flag the exact kernel
 *     then verifies the lane against that key as ssa_verify_many does) and the lanes whose signature gives no R to add
 *     up: non-canonical limbs, e >= q, an x that is not on the curve, a flag byte that does not decode.
 *   - A lane the exact check rejects keeps its exact status unless the random combination of its segment vanishes:
 *     about 2^-128 for an error with a prime-order component.  Every key that enters a sum has passed [q]P == O, so
 *     the key-side small-order case of ssa_verify_batch_screened (a key P + T2) cannot occur: such a lane gets its
 *     exact status (SSA_INVALID_PUBLIC_KEY with SSA_FLAG_CHECK_TORSION).  What remains is an R outside the prime-order subgroup,
 *     R = R' + T with T of small order l and e made for R': the exact status is 2, and the screen misses it with
 *     probability 1/l (for l = 2: exactly when the lane's coefficient, reduced mod q, is even).  Building such a lane
 *     appears to take the secret key, because h depends on R.x (changing R changes h, and solving for e is then the
 *     forgery problem itself): a signer spoiling their own signature, not a third party.  No reduction is claimed.
 * Without SSA_FLAG_SIG_FLAG_BYTE Signature::verify ignores byte 48 of the signature.  The screen still reads its sort
 * bit to choose between R and -R, since an honest signer sets it.  A valid signature with the wrong sort bit therefore
 * makes its segment fail and is then accepted by the re-check: correct, at the price of one segment's re-check.  A
 * byte that does not decode at all sends only its own lane to the re-check.
 * coeffs, n_fail_out, host staging, n == 0, SSA_MAX_BATCH: as ssa_verify_batch_screened.  Batches of at most
 * SSA_MSM_SMALL_MAX lanes (3072), and a trailing slice that small, take ssa_verify_many with the caller's flags.
 * stats_out (optional, HOST memory in both forms), summed over the slices: [0] distinct keys, [1] segments screened,
 * [2] segments that failed, [3] lanes sent to the exact re-check, [4] lanes that could not be screened, [5] slices
 * screened, [6] slices whose every lane ran the exact kernel (a re-check of more than half the slice, which was also
 * screened, or a slice of at most SSA_MSM_SMALL_MAX lanes, which was not), [7] lanes that hit the probe bound of the
 * dedup table.
 * Both forms synchronise the context's stream TWICE per slice: once to read the number of distinct keys, once to read
 * the segment verdicts together with the length of the re-check list.  No allocation per call once the workspaces
 * have grown.  Measured (2^20 signatures, SSA_FLAG_CHECK_TORSION): 18.2 ms by 65 536 signers
 * against 34.7 for ssa_verify_many_dedup, 40.9 ms by all-distinct signers against 56.8 for ssa_verify_many.  When every
 * segment fails the call costs the screen on top of the keyed kernel: 42.8 ms, 1.24x ssa_verify_many_dedup. */
int ssa_verify_many_screened(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                             const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                             uint32_t flags, const uint8_t *coeffs, uint8_t *status_out, uint64_t *n_fail_out,
                             uint64_t stats_out[8]);
int ssa_verify_many_screened_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                    const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                    size_t n, uint32_t flags, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                                    uint8_t *d_status_out, uint64_t *d_n_fail_out, uint64_t stats_out[8]);

/* ---- key cache: each public key checked once, not once per batch ------------------------
 * A key cache is a key set that fills itself.  ssa_verify_many_cached is ssa_verify_many_screened with its per-key
 * check (limbs, curve, [q]P == O, the table of sixteen multiples) behind a cache on the device: every distinct key of a
 * slice is looked up by its bytes, only the keys never seen are checked, and their statuses and tables stay for the
 * next slice and the next call.  The caller hands in no index and need not know the signers in advance.
 *
 * The object.  capacity = keys the cache can hold, 1 <= capacity <= 2^24 (anything else: SSA_ERR_ARG, *out = NULL).
 * ALL device memory is allocated by ssa_keycache_create, none per call: per key the 4 KB table of sixteen multiples,
 * the 96 key bytes, the pk_inf boolean and the status byte (the storage of a ladder-kind key set), and an
 * open-addressing table of 64-bit words with at least four slots per key: about 4.2 KB per key, 4.4 GB for 2^20 keys.
 * A failed allocation is SSA_ERR_HIP and leaves nothing behind.  ssa_keycache_clear empties the cache (one memset of
 * the slot words on the context's stream; the next call is cold).  ssa_keycache_info: out[0] capacity, [1] keys held,
 * [2] clears since creation (explicit and automatic), [3] device bytes.  A cache belongs to one context; the calls that
 * use it are serialised by the caller, as calls on a context are.  A cache that outlives its context is orphaned, not
 * dangling, as key sets are: its device memory is freed by ssa_ctx_destroy, every call on it but ssa_keycache_destroy
 * then returns SSA_ERR_ARG.  ssa_keycache_destroy(NULL) is a no-op.
 * A key's identity is the one of ssa_verify_many_dedup: the 96 key bytes and pk_inf as a boolean.  Equality is decided
 * on those bytes, never on the fingerprint that picks the slot (keyed SipHash-2-4 under the context's random key).
 * Keys with a nonzero status (malformed, or outside the prime-order subgroup) are cached like any other: a sender
 * cannot force the check again by repeating a bad key.
 *
 * The calls.  Arguments, flag rules (SSA_FLAG_CHECK_TORSION and SSA_FLAG_SIG_FLAG_BYTE only; any other bit is
 * SSA_ERR_ARG before anything else is looked at), coeffs, n == 0, SSA_MAX_BATCH, n_fail_out: those of
 * ssa_verify_many_screened.  SSA_FLAG_SIG_FLAG_BYTE alone is handed to ssa_verify_batch_screened, and batches and
 * trailing slices of at most SSA_MSM_SMALL_MAX lanes to ssa_verify_many: the cache is then not touched.  kc == NULL,
 * or a cache of another context (or an orphaned one), is SSA_ERR_ARG.
 * With the same coeffs the status vector is BYTE FOR BYTE the one ssa_verify_many_screened returns, in every state of
 * the cache -- cold, warm, partly warm, just cleared, bypassed: the same keys with the same statuses and tables enter
 * the same sums.  That is an equality, not a probability.
 * Per slice of at most SSA_LANE_SLICE lanes:
 *   1. the distinct keys of the slice, as in ssa_verify_many_dedup (u of them);
 *   2. one lane per distinct key probes the cache (queued behind the dedup, in front of its read-back): u, the number
 *      of lanes at the probe bound and the number of misses m come back in the dedup's one read-back;
 *   3. on the host, a pure function of (capacity, held, u, m) (ssa_debug_keycache_plan):
 *        held + m <= capacity   the m misses are inserted;
 *        else u <= capacity     the cache is cleared (whole-cache eviction: no entry is ever deleted alone, so an
 *                               empty slot always ends a probe chain) and all u keys of the slice are inserted;
 *        else                   the slice BYPASSES the cache and runs exactly as in ssa_verify_many_screened; the
 *                               cache is left as it was;
 *   4. the new keys' bytes are gathered into the next rows, ssa_k_keyset_build runs over those rows only, and a
 *      publishing launch claims a slot per new row by a vector compare-and-swap.  It is queued after the build: a row is
 *      complete before any later launch can find it.  A row that finds no empty slot within the probe bound is used by
 *      this call and is simply not found by the next one;
 *   5. every lane gets its key's cache row, and the mask, the segmented MSM and the keyed exact kernel run as in
 *      ssa_verify_many_screened, reading the cache's statuses and tables.
 * The slices of one call run IN ORDER ON THE CONTEXT'S STREAM IN BOTH FORMS: the host form does not alternate its
 * slices between the context and its second set of streams as the other host forms do, because two streams would
 * mutate one cache.  It gives up the ~2 % overlap of multi-slice host calls.  Two synchronisations per slice, as
 * ssa_verify_many_screened; no allocation per call once the context's workspaces have grown.
 * stats_out (optional, HOST memory in both forms, 12 words, summed over the slices): [0..7] as
 * ssa_verify_many_screened, with the rows that could not be published added to [7]; [8] distinct keys found in the
 * cache, [9] keys checked and inserted, [10] automatic clears, [11] slices that bypassed the cache.  [8] + [9] == [0]
 * over the slices that used the cache.
 * Timing keys beside those of ssa_verify_many_screened: keycache_lookup, keycache_insert (gather and publish),
 * keycache_map; ssa_k_keyset_build keeps its key, and a warm call launches none.  Measured: DESIGN.md section 16. */
typedef struct ssa_keycache ssa_keycache;
int ssa_keycache_create(ssa_ctx *ctx, size_t capacity, ssa_keycache **out);
void ssa_keycache_destroy(ssa_keycache *kc);
int ssa_keycache_clear(ssa_keycache *kc);
int ssa_keycache_info(ssa_keycache *kc, uint64_t out[4]);
int ssa_verify_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                           const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                           uint32_t flags, const uint8_t *coeffs, uint8_t *status_out, uint64_t *n_fail_out,
                           uint64_t stats_out[12]);
int ssa_verify_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_sigs, const uint8_t *d_pks,
                                  const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                  size_t msg_stride, size_t msg_len, size_t n, uint32_t flags, const uint8_t *d_coeffs,
                                  uint32_t coeff_bytes, uint8_t *d_status_out, uint64_t *d_n_fail_out,
                                  uint64_t stats_out[12]);

/* ---- KeyedSignature wire records through a key cache in wire mode -------------------------
 * ssa_keycache_create_ex(ctx, capacity, flags, &out): flags == 0 is exactly ssa_keycache_create; SSA_KEYCACHE_WIRE makes
 * the identity of a row the 49 compressed key bytes AS RECEIVED (any other flag bit: SSA_ERR_ARG before anything else is
 * looked at, *out = NULL).  A wire row holds everything an affine row holds -- the 96 key bytes, pk_inf, the status and
 * the table, produced by the decompression and then by the same key check -- and the 49 bytes it was built from (56 more
 * bytes per key; ssa_keycache_info reports the larger footprint).  Slot words, probe bound, clear-only eviction, the plan
 * of ssa_debug_keycache_plan, orphaning, clear / info / destroy and the statistics are those of an affine cache.
 * A key that does not decode -- a flag byte with one of its six low bits set, a limb >= p, an infinity bit with x != 0 or
 * with the sort bit, x^3 + x + u + 395 not a square -- is cached like any other key: its row holds the affine bytes
 * (0, 0), which the key check reports as SSA_MALFORMED, so a sender cannot force the square root again by repeating a
 * bad key.  Two different undecodable strings are two keys.
 * Every call checks the mode: ssa_verify_many_cached(_device) on a wire cache and the calls below on an affine cache
 * return SSA_ERR_ARG and leave the cache as it was.
 *
 * ssa_verify_keyed_many_cached(_device): keyed = n records of 130 bytes, pk (49) || signature (81).  Flags, coeffs,
 * n == 0, SSA_MAX_BATCH, the slice length, n_fail_out and stats_out are those of ssa_verify_many_cached, word for word;
 * stats[0], [8] and [9] count distinct 49-byte strings.
 * The contract is an equality.  Let P(keyed) be what ssa_verify_keyed_many unpacks a batch into: affine keys, (0, 0) for
 * undecodable ones, pk_inf, and the 81-byte signatures.  With the same coeffs the status vector equals
 * ssa_verify_many_screened on P(keyed) BYTE FOR BYTE, in every state of the cache; so it equals ssa_verify_keyed_many
 * lane for lane except with the probability the screen already allows.
 * Batches and trailing slices of at most SSA_MSM_SMALL_MAX lanes go to the exact keyed path (ssa_verify_keyed_many_device)
 * and flags == SSA_FLAG_SIG_FLAG_BYTE alone to unpacking plus ssa_verify_batch_screened_device: the cache is not touched.
 * Per slice: the 81 signature bytes are split into a dense array; the distinct 49-byte keys are found (the dedup of
 * section 14 on 49 bytes) and looked up against the rows' stored 49 bytes; one lane per MISS decompresses its key into
 * the next rows, the key check runs over those rows as it is, and the rows are published; every lane's 96 key bytes and
 * flag are then copied out of its row into a per-lane workspace, which is what the screen's MSM and challenge hash read.
 * From there on the slice is a slice of ssa_verify_many_cached.  Still two synchronisations per slice.  Under a bypass
 * the u keys are decompressed into the context's own workspaces.
 * The host form uploads the 130-byte records and the messages (130 B per lane in place of 177) and runs the device
 * slice; the challenge hash needs y, which exists only after the look-up, so the pipelined upload-and-hash is not used.
 * Slices run in order on the context's stream in both forms.
 * Timing keys beside those of ssa_verify_many_cached: keyed_split, ssa_k_keyed_decompress, keyed_expand; a warm call
 * launches neither ssa_k_keyed_decompress nor ssa_k_keyset_build.
 * ssa_verify_keyed_many_device: ssa_verify_keyed_many on device buffers (d_n_fail_out optional, device memory). */
#define SSA_KEYCACHE_WIRE 1u    /* ssa_keycache_create_ex: rows are identified by the 49 compressed key bytes */
int ssa_keycache_create_ex(ssa_ctx *ctx, size_t capacity, uint32_t flags, ssa_keycache **out);
int ssa_verify_keyed_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *keyed, const uint8_t *msgs,
                                 const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n, uint32_t flags,
                                 const uint8_t *coeffs, uint8_t *status_out, uint64_t *n_fail_out, uint64_t stats_out[12]);
int ssa_verify_keyed_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_keyed, const uint8_t *d_msgs,
                                        const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                        uint32_t flags, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                                        uint8_t *d_status_out, uint64_t *d_n_fail_out, uint64_t stats_out[12]);
int ssa_verify_keyed_many_device(ssa_ctx *ctx, const uint8_t *d_keyed, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                 size_t msg_stride, size_t msg_len, size_t n, uint32_t flags, uint8_t *d_status_out,
                                 uint64_t *d_n_fail_out);

/* ---- key cache eviction: keep the keys used most recently when the cache fills -----------
 * A cache clears itself when a slice's misses do not fit (step 3 above) until ssa_keycache_set_eviction(kc,
 * SSA_KEYCACHE_EVICT_RECENT) is called on it; SSA_KEYCACHE_EVICT_CLEAR goes back.  Both work on affine and wire
 * caches, empty or not.  The policy is no flag of ssa_keycache_create_ex.  A NULL or orphaned cache, or any other
 * policy value, is SSA_ERR_ARG.
 * SSA_KEYCACHE_EVICT_RECENT allocates, at that call, everything the policy will ever need: a 32-bit stamp per row and
 * the compaction's scratch (12 bytes per row and a little per 256 rows), sized for `capacity`.  ssa_keycache_info()[3]
 * reports the larger footprint from then on and it never changes again (going back to CLEAR keeps the memory).  A
 * failed allocation is SSA_ERR_HIP and leaves the policy as it was.  Rows already held count as used now.
 * Under SSA_KEYCACHE_EVICT_RECENT the cache has an epoch, one more for every slice that looks keys up in it.  The
 * look-up stores the epoch into the stamp of every row it hits; inserted rows get the current epoch.  The plan stays a
 * pure function of (capacity, held, u, m): insert if held + m <= capacity, else COMPACT (where the default policy clears)
 * if u <= capacity, else bypass.
 * A compaction: age(r) = epoch - stamp(r) (32-bit; 0 for the rows this slice hit); hist[a] = rows of age a for a in
 * 0..62, hist[63] = all older rows, never kept; budget = max(u - m, (capacity - m) / 2); a* = the largest a in 0..62
 * with hist[0] + .. + hist[a] <= budget and K = that sum (ssa_debug_keycache_keep: out[0] = a*, out[1] = K).  The K
 * rows of age <= a* survive and are packed into rows [0, K) -- survivors below K stay, the t-th survivor at a row >= K
 * moves whole into the t-th other row below K --, every slot is emptied and rows [0, K) are published again, the
 * slice's hits follow their rows, and the m misses are inserted at rows K .. K + m as ever: held = K + m <= capacity.
 * K < held, so a compaction always drops a row, and since at most half of the room beside the misses is kept the next
 * compaction is at least (capacity - m) / 2 insertions away.  No key that is still in use is checked twice.  Stamps alias
 * after 2^32 slices: that can change which rows are kept, never a status (should the aliased ages leave no a*, the
 * cache is cleared as under the default policy).
 * The contract of ssa_verify_many_cached / ssa_verify_keyed_many_cached is unchanged -- the status vector equals
 * ssa_verify_many_screened's BYTE FOR BYTE in every state of the cache, during and after a compaction included -- and
 * so are stats[0..9] and [11]; [10] counts automatic evictions: clears of a CLEAR cache, compactions of a RECENT one.
 * Rows that find no slot when they are published again are counted in [7].  ssa_keycache_info is unchanged (its clears
 * count clears only); ssa_keycache_selfcheck, its repair and ssa_debug_keytab_read work on rows [0, held) as before.
 * ssa_keycache_eviction_info: out[0] policy, [1] compactions since creation, [2] rows dropped by them, [3] rows kept
 * and [4] rows moved by the last one, [5] the epoch, [6] = [7] = 0.
 * A compaction costs two more read-backs in its slice.  Timing key: keycache_compact (ages, marking, move, publishing,
 * remapping). */
#define SSA_KEYCACHE_EVICT_CLEAR  0u   /* whole-cache eviction, the default */
#define SSA_KEYCACHE_EVICT_RECENT 1u   /* keep the rows used most recently */
int ssa_keycache_set_eviction(ssa_keycache *kc, uint32_t policy);
int ssa_keycache_eviction_info(ssa_keycache *kc, uint64_t out[8]);

/* Exact self-check of the per-key tables of a key set or a key cache, on the owning context's
 * stream; returns when it is done.  ssa_ctx_selfcheck covers the tables for G; these two cover what lives as long as a
 * validator set does: per key the 4 KB table of sixteen multiples, the status byte and, in comb mode, the 100 MB comb.
 * The root of trust of a row is what it was built from: its 96 stored key bytes and its pk_inf boolean (a key set keeps
 * both from its creation on).  What "a key passes" means depends on its stored status:
 *   0, finite key  the bytes are canonical and on the curve; entry 1P is the key bit for bit, 2P the tangent of 1P, mP
 *                  (3 <= m <= 16) the chord (m-1)P + P (section 11's two equations, no inversion), and the second line of
 *                  every entry is (x, -y).  A clean pass proves every entry exact.
 *   0, identity    all sixteen entries are the (0, 0) sentinel in both lines.
 *   1              the table is built again into scratch and the words the kernels read are compared (no [q]P).
 *   3              no kernel reads the table; the status itself is checked, always: the bytes must fail the limb or the
 *                  curve test.  Any other status byte fails.
 * Table words are compared as residues mod p (the builder stores loose limbs and every kernel reads them as such); the
 * key bytes, and entry 1P against them, bit for bit.  Words 12-15 and 28-31 of an entry are read by no kernel and are
 * not checked.  WITHOUT SSA_KEYCHECK_DEEP A STATUS BYTE FLIPPED BETWEEN 0 AND 1 IS NOT DETECTED: the table of such a key
 * is right.  DEEP recomputes [q]P from the proven table of every key of status 0 or 1 whose table passed -- exactly what
 * ssa_k_keyset_build computes -- and compares with the stored byte; it costs about one key check per key.
 * Key sets in comb mode: the comb of every key of status 0 is checked like the comb for G (16 windows of 16 bits, no
 * header word, row (0, 1) = the key; an identity key's comb is all sentinels).  COMBS OF KEYS OF STATUS 1 OR 3 ARE NOT
 * CHECKED; out[6] counts them.
 *   out[0] keys checked (m / keys held)              out[4] comb rows checked (key sets in comb mode)
 *   out[1] keys that fail (before any repair)        out[5] keys checked by rebuild-and-compare (status 1)
 *   out[2] first failing key (UINT64_MAX: none)      out[6] keys whose comb was skipped
 *   out[3] ladder-table entries checked by relations out[7] rows rebuilt (SSA_KEYCHECK_REPAIR)
 * bad_out (key sets; host, m bytes, optional) receives 1 per failing key, 0 otherwise: a key set is indexed by the
 * caller, who has to hand those keys in again (a new key set); it has no repair, because rebuilding position i from
 * device bytes that may themselves be what flipped would answer for another key under the caller's index.
 * SSA_KEYCHECK_REPAIR (key caches only) rebuilds every failing row in place from its stored bytes and pk_inf with
 * ssa_k_keyset_build and checks again.  That is safe in a cache even when the key bytes were what flipped: the row becomes
 * a correct row for the bytes it now holds, look-ups compare all 97 bytes, so the original key misses and is inserted
 * again, and the status vector stays byte for byte that of ssa_verify_many_screened.
 * A cache in WIRE mode (SSA_KEYCACHE_WIRE) trusts the 49 bytes a row was built from.  A row also fails when its stored
 * 96 bytes and pk_inf are not what those 49 bytes stand for -- x equal bit for bit, the sort bit equal to
 * lex_largest(y), the identity encoding, (0, 0) and no flag for a string that cannot decode; with the curve relation
 * above that fixes y, and no square root is computed -- and, under SSA_KEYCHECK_DEEP, when a row of status 3 decodes
 * after all (one decompression per such row).  Such rows are counted in out[1] and out[2] like any other.  REPAIR
 * rebuilds a failing row from its 49 bytes: the decompression, then the key check.  When the 49 bytes were what flipped
 * the row becomes a correct row for the string it now holds; the original key misses and is inserted again.
 * Returns SSA_OK when clean, or clean after repair (an empty cache: SSA_OK, all zero but out[2]); SSA_ERR_TABLE when a
 * key failed and was not repaired, or still fails after it; SSA_ERR_ARG for a NULL or orphaned object, an unknown flag
 * bit, REPAIR on a key set, or out == NULL; SSA_ERR_HIP as usual.  Both only read the object, but for repair.  Their
 * workspaces belong to the context: from the second call on nothing is allocated.  Timing keys: ssa_k_keytab_check,
 * ssa_k_keytab_rebuild, ssa_k_keytab_deep, ssa_k_keycomb_check, keycheck_repair (and ssa_k_keyset_build in a repair). */
#define SSA_KEYCHECK_DEEP   1u  /* also recompute [q]P per key from the proven table and compare with the stored status */
#define SSA_KEYCHECK_REPAIR 2u  /* key caches only: rebuild failing rows in place from their stored key bytes */
int ssa_keyset_selfcheck(ssa_keyset *ks, uint32_t flags, uint8_t *bad_out, uint64_t out[8]);
int ssa_keycache_selfcheck(ssa_keycache *kc, uint32_t flags, uint64_t out[8]);

/* ---- signer sets: many signatures by few signers (the signing twin of the key set) ---------------------------
 * A signer set holds m key pairs on the device: the secret key, the 96-byte affine public key, the 49-byte compressed
 * key and a per-key status.  Signature i is then KeyPair::sign (src/signature.rs:114-129) -- or, with
 * SSA_FLAG_SIGN_KEYED, KeyPair::sign_and_bind_pkey (:132-156) -- by key pair key_idx[i]: the public key the key pair
 * holds is hashed, so each signature costs ONE base multiplication, [r]G, where ssa_keygen_sign_many_ex (which is
 * PrivateKey::sign) computes [sk]G as well.  For every valid lane the output is byte-identical to
 * ssa_keygen_sign_many_ex with the same flags on the gathered rows sks[key_idx[i]].  Lifetime as for key sets: a set
 * belongs to its context; one that outlives it is orphaned by ssa_ctx_destroy (its secret keys are zeroed and its
 * memory freed there, every call on it but ssa_signer_set_destroy returns SSA_ERR_ARG).  ssa_signer_set_destroy zeroes
 * the secret keys on the device before it frees them. */
typedef struct ssa_signer_set ssa_signer_set;
/* KeyPair::from_bytes (src/keypair.rs:78-89) for m keys (m x 32): a zero or non-canonical key gives SSA_ERR_ARG (the
 * check takes the same time whatever the keys are); the staged copy of the keys is wiped before the call returns. */
int ssa_signer_set_create(ssa_ctx *ctx, const uint8_t *sks, size_t m, ssa_signer_set **out);
/* the same from device memory: key k is the first 32 bytes of d_sks + k * sk_stride (sk_stride >= 32; 64 takes the
 * key half of the ExtendedPrivateKey records key || chaincode, src/derivation.rs:177-184, that
 * ssa_xprv_derive_many_device writes).  Each key is checked on the device without a branch on its value: a zero or
 * non-canonical key gets status SSA_MALFORMED and signs nothing. */
int ssa_signer_set_create_device(ssa_ctx *ctx, const uint8_t *d_sks, size_t sk_stride, size_t m,
                                 ssa_signer_set **out);
void ssa_signer_set_destroy(ssa_signer_set *ss);
/* per-key status (m bytes): 0 usable, 3 malformed */
int ssa_signer_set_status(ssa_signer_set *ss, uint8_t *status_out);
/* PublicKey::from(&PrivateKey) (src/public.rs:26-32) as m x 96 affine bytes and PublicKey::to_bytes (:49-51) as m x 49,
 * byte for byte what ssa_pubkey_many and ssa_compress_many give (zero for a malformed key); either may be NULL */
int ssa_signer_set_public_keys(ssa_signer_set *ss, uint8_t *pks96_out, uint8_t *pks49_out);
/* KeyPair::sign / sign_and_bind_pkey for n messages: signature i by key pair key_idx[i] with nonce i.  flags:
 * SSA_FLAG_SIGN_CT and SSA_FLAG_SIGN_KEYED as for ssa_keygen_sign_many_ex, any other bit is SSA_ERR_ARG.  Messages,
 * limits and output layout (n x 81, or n x 130 keyed) are those of ssa_keygen_sign_many_ex.  SSA_ERR_ARG for an index
 * >= m, a key whose status is not 0, or a zero or non-canonical nonce; the device copy of the nonces is wiped. */
int ssa_sign_many_indexed(ssa_ctx *ctx, ssa_signer_set *ss, const uint32_t *key_idx, const uint8_t *nonces,
                          const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                          size_t n, uint32_t flags, uint8_t *sigs_out);
/* the same on device buffers, on the context's stream: nonces are reduced mod q; a lane whose index is >= m or whose
 * key is unusable gets an all-zero record and, when d_status_out is given, SSA_MALFORMED there (0 for the others).
 * PRECONDITION of SSA_FLAG_SIGN_CT: every nonce is canonical and non-zero, as for ssa_keygen_sign_many_ex_device. */
int ssa_sign_many_indexed_device(ssa_ctx *ctx, ssa_signer_set *ss, const uint32_t *d_key_idx,
                                 const uint8_t *d_nonces, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                 size_t msg_stride, size_t msg_len, size_t n, uint32_t flags,
                                 uint8_t *d_sigs_out, uint8_t *d_status_out);

/* ---- nonces and keys drawn on the device (Scalar::random(rng)) --------------------------
 * sign(message, rng) and sign_and_bind_pkey(message, rng) (src/signature.rs:65-156) with the nonces drawn by the GPU
 * itself, and KeyPair::new(rng) (src/keypair.rs:57-65) for a whole signer set.  Each call takes a fresh 44-byte seed from
 * getrandom(2) -- ChaCha20 key = seed[0:32], nonce = seed[32:44], RFC 8439 blocks with a 32-bit counter -- and lane i of
 * the call (counted over the whole call) gets Scalar::from_bytes_wide(block 2i), or from_bytes_wide(block 2i + 1) where
 * the first is 0, chosen by a constant-time select.  Neither the nonces nor the seed ever reach the host: the seed passes
 * through the library's page-locked buffer (wiped before the call returns) into device memory, and the device seed and
 * the drawn scalars are zeroed on the context's stream after the signing kernels.  Device memory for the draw is one
 * slice (SSA_LANE_SLICE lanes, 32 B each), whatever n is.  The _device forms wait for the seed upload (and so for the work
 * queued before it on the stream) before they enqueue the rest. */
/* ssa_keygen_sign_many_ex with nonces drawn on the device: flags, checks, limits and output layout are those of
 * ssa_keygen_sign_many_ex (SSA_FLAG_SIGN_CT, SSA_FLAG_SIGN_KEYED; any other bit is SSA_ERR_ARG), and the output is
 * byte-identical to it given the drawn nonces. */
int ssa_keygen_sign_many_rng(ssa_ctx *ctx, const uint8_t *sks, const uint8_t *msgs, const uint64_t *msg_off,
                             size_t msg_stride, size_t msg_len, size_t n, uint32_t flags, uint8_t *pks_out,
                             uint8_t *sigs_out);
int ssa_keygen_sign_many_rng_device(ssa_ctx *ctx, const uint8_t *d_sks, const uint8_t *d_msgs,
                                    const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                    uint32_t flags, uint8_t *d_pks_out, uint8_t *d_sigs_out);
/* ssa_sign_many_indexed[_device] with nonces drawn on the device: statuses, errors and orphan behaviour are theirs */
int ssa_sign_many_indexed_rng(ssa_ctx *ctx, ssa_signer_set *ss, const uint32_t *key_idx, const uint8_t *msgs,
                              const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n, uint32_t flags,
                              uint8_t *sigs_out);
int ssa_sign_many_indexed_rng_device(ssa_ctx *ctx, ssa_signer_set *ss, const uint32_t *d_key_idx,
                                     const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                     size_t msg_len, size_t n, uint32_t flags, uint8_t *d_sigs_out,
                                     uint8_t *d_status_out);
/* KeyPair::new(rng) for m key pairs (1 <= m <= SSA_MAX_BATCH): key j is the draw of lane j under a fresh seed; public
 * keys and statuses come from the path of ssa_signer_set_create_device */
int ssa_signer_set_generate(ssa_ctx *ctx, size_t m, ssa_signer_set **out);
/* KeyPair::to_bytes (src/keypair.rs:73-75) for the whole set: m x 32 bytes, zeros for a malformed key.  What makes a
 * generated set persistable -- and the one call that brings its secret keys to the host. */
int ssa_signer_set_secret_keys(ssa_signer_set *ss, uint8_t *sks_out);
/* TEST HOOKS.  ssa_debug_pin_rng makes every later draw on ctx use `seed` (44 bytes) instead of getrandom(2); NULL
 * unpins.  A PINNED CONTEXT REUSES ITS NONCES ON EVERY CALL, AND TWO SIGNATURES BY ONE KEY WITH ONE NONCE GIVE THE KEY
 * AWAY: for tests only, never in production.  ssa_debug_draw_scalars runs the device's draw rule on n caller-supplied
 * block pairs (B0 || B1, 128 bytes each) and writes n x 32 bytes. */
int ssa_debug_pin_rng(ssa_ctx *ctx, const uint8_t seed[44]);
int ssa_debug_draw_scalars(ssa_ctx *ctx, const uint8_t *blocks, size_t n, uint8_t *out);

/* ---- several GPUs of one node from a single process --------------------------------------------
 * The batch shards by signature (contiguous ranges, sizes differ by at most one) over the listed
 * devices -- one context and one host thread per device, no collective: every verification reads
 * only its own record (src/signature.rs:181-205).  Same semantics as ssa_verify_many. */
typedef struct ssa_multi ssa_multi;
int ssa_multi_create(ssa_multi **out, const int *devices, int n_devices, const void *params, size_t params_len);
void ssa_multi_destroy(ssa_multi *m);
int ssa_multi_verify_many(ssa_multi *m, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                          const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                          size_t n, uint32_t flags, uint8_t *status_out, uint64_t *n_fail_out);

/* verify_batch exactly as src/batch.rs (ssa_verify_batch_msm) with the batch sharded over the devices: each device
 * reduces its shard to one point and one scalar, device 0 adds the shards up (one point addition per shard), computes
 * [sum s_i e_i]G and compares x coordinates.  coeffs: n x 32 bytes or NULL (every device draws its own). */
int ssa_multi_verify_batch_msm(ssa_multi *m, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                               const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                               size_t n, const uint8_t *coeffs);

/* ---- MSM-form verify_batch across PROCESSES (one process per GPU, torch.distributed / RCCL) ----------------
 * The same split as ssa_multi_verify_batch_msm, with the exchange left to the caller ("in the MSM
 * form, one point addition per shard + one compare", src/batch.rs:98-129): every rank reduces ITS shard to one
 * record of SSA_MSM_PARTIAL_WORDS u64 --
 *     words 0..17  the shard's left-hand point  sum s_i R_i - sum (s_i h_i) P_i  as X, Y, Z in canonical limbs; the
 *                  library writes the canonical form -- affine (x, y, 1), or (0, 0, 0) for the identity -- so equal
 *                  shards give equal bytes; ssa_msm_combine accepts any Jacobian representative
 *     words 18..21 sum s_i e_i mod q            word 22  1: the shard holds an input the reference panics on, else 0
 *     word 23      SSA_MSM_RECORD_MAGIC -- every record the library produces carries it, the empty shard's too
 * -- the ranks all-gather the records (24 words per rank: the only traffic), and ssa_msm_combine adds the k points
 * up (one Jacobian addition per shard), computes [sum]G from the comb table and compares x coordinates exactly as
 * the single-context call does.  An empty shard (n == 0) gives the identity (all limbs 0), 0 and the magic word.
 * Coefficients as in ssa_verify_batch_msm_device (NULL: drawn per call on the device; every rank draws its own).
 *
 * ORDERING (the _device forms are asynchronous): ssa_verify_batch_msm_partial_device only enqueues on the context's
 * stream; the record is valid for a collective on another stream after ssa_ctx_stream_release(ctx, that stream) (or
 * ssa_ctx_sync, or a shared stream via ssa_ctx_set_stream), and the gathered records are visible to
 * ssa_msm_combine_device after ssa_ctx_stream_acquire(ctx, the collective's stream).  The combination FAILS CLOSED:
 * a record that was never written (all zero), comes from another format version, has a non-canonical limb or scalar,
 * or a point off the curve makes the verdict SSA_MALFORMED -- never SSA_OK. */
#define SSA_MSM_PARTIAL_WORDS 24
#define SSA_MSM_RECORD_MAGIC 0x5353415245430004ull   /* "SSAREC", format 4 */
int ssa_verify_batch_msm_partial_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                        const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                        size_t msg_stride, size_t msg_len, size_t n, const uint8_t *d_coeffs,
                                        uint32_t coeff_bytes, uint64_t *d_partial_out);
/* host-buffer form (coeffs: n x 32 bytes or NULL); out24 is host memory */
int ssa_verify_batch_msm_partial(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                 const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                 size_t n, const uint8_t *coeffs, uint64_t out24[SSA_MSM_PARTIAL_WORDS]);
/* k records (k x 24 words, device memory) -> *d_verdict_out = SSA_OK / SSA_INVALID_SIGNATURE / SSA_MALFORMED,
 * enqueued on the context's stream; 1 <= k <= 4096 */
int ssa_msm_combine_device(ssa_ctx *ctx, const uint64_t *d_parts24, size_t k, uint32_t *d_verdict_out);
/* the same from host memory; returns the status */
int ssa_msm_combine(ssa_ctx *ctx, const uint64_t *parts24, size_t k);

/* ---- half-aggregation of signatures -------------------------------------------------
 * "Non-interactive half-aggregation of EdDSA and variants of Schnorr signatures" (Chalkias, Garillot, Kondi,
 * Nikolaenko, CT-RSA 2021), which src/batch.rs:1-3 announces and does not ship: n signatures (R_i, e_i) become the n
 * R's and ONE scalar, 49 n + 32 bytes instead of 81 n,
 *     aggregate = R_0 || ... || R_(n-1) || e_agg,      e_agg = sum a_i e_i mod q   (32 bytes, little-endian, canonical)
 * where R_i is the first 49 bytes of signature i verbatim and the coefficients a_i are hashed out of a transcript that
 * binds every R_i (its flag byte too), key, message and the ORDER of the lanes (H = RescueHash::hash_field):
 *     d_i = the 4-felt digest of hash_message(R_i.x, P_i, m_i), before any reduction mod q
 *     leaf_i = H(d_i || flag byte of R_i || 0xA1);   node = H(left || right), an odd last node of a level moves up
 *     unchanged, until one node, top, is left;   root = H(top || n || 0xA2)
 *     a_i = the first 16 bytes of Digest::to_bytes(H(root || i || 0xA3)), little-endian, masked to 126 bits, 0 -> 1
 * The verifier recomputes the a_i and accepts iff
 *     sum a_i R_i - sum (a_i h_i mod q) P_i == [e_agg] G        AS POINTS (both coordinates; no x-only comparison)
 * -- the equation of ssa_verify_batch_msm with hash-derived coefficients, through the same bucket MSM.  Semantics are
 * those of verify_batch: the flag byte of R_i is honoured, pk_inf marks identity keys, and there is NO subgroup check
 * (keys or R's with a small-order component: the caveat of ssa_verify_batch_screened applies; take key statuses from a
 * key set or a key cache where it matters).  An aggregate verifies only if every input verified with
 * SSA_FLAG_SIG_FLAG_BYTE; a forgery succeeds with probability about 2^-126 per transcript tried.
 * n above the context's MSM slice (2^23, SSA_MSM_SLICE) is SSA_ERR_ARG in the calls of this section; the sliced,
 * sharded and multi-GPU forms are the calls of "sharded half-aggregation" below.
 *
 * ssa_aggregate_many: agg_out receives SSA_AGGREGATE_LENGTH(n) bytes.  flags: 0 or SSA_AGG_CHECK (any other bit:
 * SSA_ERR_ARG).  With SSA_AGG_CHECK the statuses of ssa_verify_batch_screened are computed first: if any is nonzero,
 * agg_out is zeroed, status_out names the lanes and the smallest nonzero status is returned.  Without it only inputs
 * the verifier would call malformed are refused (non-canonical limbs, e_i >= q, a key off the curve, an R that does not
 * decode): status_out[i] is then 0 or 3, agg_out is zeroed and SSA_MALFORMED is returned.  status_out (n bytes) and
 * n_fail_out may be NULL.  n == 0: 32 zero bytes, SSA_OK.  The _device form takes device pointers (d_n_fail_out too) and
 * SYNCHRONISES the context's stream, since the status it returns is read from the device.
 *
 * ssa_verify_aggregate returns SSA_OK, SSA_INVALID_SIGNATURE (the equation fails) or SSA_MALFORMED (a non-canonical
 * limb, an undecodable R_i or flag byte, a key off the curve, e_agg >= q).  n == 0: the 32 bytes must be zero.  The
 * _device form writes the status to *d_verdict_out and only enqueues on the context's stream, like
 * ssa_verify_batch_msm_device. */
#define SSA_AGGREGATE_LENGTH(n) ((size_t)49 * (size_t)(n) + 32)
#define SSA_AGG_CHECK 1u
int ssa_aggregate_many(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                       const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                       uint32_t flags, uint8_t *agg_out, uint8_t *status_out, uint64_t *n_fail_out);
int ssa_aggregate_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                              const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                              size_t n, uint32_t flags, uint8_t *d_agg_out, uint8_t *d_status_out,
                              uint64_t *d_n_fail_out);
int ssa_verify_aggregate(ssa_ctx *ctx, const uint8_t *agg, const uint8_t *pks, const uint8_t *pk_inf,
                         const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n);
int ssa_verify_aggregate_device(ssa_ctx *ctx, const uint8_t *d_agg, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                size_t n, uint32_t *d_verdict_out);
/* tests: the coefficients a_i of an aggregate's R's (rs49: n x 49 bytes, host), keys and messages -> n x 16 bytes */
int ssa_debug_aggregate_coeffs(ssa_ctx *ctx, const uint8_t *rs49, const uint8_t *pks, const uint8_t *pk_inf,
                               const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                               uint8_t *coeffs16_out);

/* ---- sharded half-aggregation: slices, devices, processes -----------------------------------
 * The same aggregate, byte for byte, and the same verdict as the calls above, for any n <= SSA_MAX_BATCH and with the
 * lanes spread over slices of one context, several devices or several processes.  The tree of the transcript is defined
 * level by level, so an aligned run of B = 2^t lanes is a whole subtree of it: a SHARD -- consecutive lanes whose first
 * stands on a multiple of B in the aggregate; every shard but the last holds whole blocks of B -- reduces its lanes to one
 * 32-byte TOP per block.  The tops of all shards, in lane order, give the root; the root goes back to the shards; each
 * derives its lanes' coefficients from the root and the lanes' places and returns 32 bytes (producer: its part of
 * e_agg) or one record of SSA_MSM_PARTIAL_WORDS words (validator: its part of the left-hand point).  Traffic: 32 bytes
 * per block in, 32 bytes out, 32 or 192 bytes per shard back.
 *
 * The primitives are device forms and only enqueue on the context's stream; ORDERING for collectives on other streams
 * is that of ssa_verify_batch_msm_partial_device above (ssa_ctx_stream_release / ssa_ctx_stream_acquire).  Tops, roots,
 * challenge scalars and partial scalars are read and written as 64-bit words: 8-byte aligned, else SSA_ERR_ARG.
 *   ssa_aggregate_shard_tops_device   n_s lanes at d_lanes -- signatures (lane_stride 81) or R's (lane_stride 49) -- with
 *       their keys and messages -> ceil(n_s / block_lanes) tops; d_h_out (or NULL): the n_s challenge scalars mod q, four
 *       words each, which ssa_verify_aggregate_shard_device takes.  block_lanes: a power of two, else SSA_ERR_ARG.
 *       One ssa_k_hash, one ag_k_leaf and log2(block_lanes) launches of ag_k_level per MSM slice of lanes.
 *   ssa_aggregate_root_device         n_tops tops of an aggregate of n lanes -> the 32-byte root.  block_lanes: 0, or the
 *       B the tops were made with; then n_tops must be ceil(n / B).  n == 0 (no root exists), n_tops == 0 or n_tops > n:
 *       SSA_ERR_ARG.
 *   ssa_aggregate_shard_fold_device   producer: n_s signatures whose first is lane `lane0` of the aggregate and the root
 *       -> d_e_out = sum a_i e_i mod q over them (32 bytes) and d_rs_out = their R's (49 n_s bytes).  d_status_out (or
 *       NULL: no checks, the keys are not read): the checks, status bytes and count of ssa_aggregate_many without
 *       SSA_AGG_CHECK; a lane that fails adds nothing to the sum.
 *   ssa_verify_aggregate_shard_device validator: n_s R's at stride 49, keys, pk_inf and messages, the challenge scalars
 *       from the tops call (d_h; NULL: hashed again), lane0 and the root -> one record in the format of
 *       ssa_verify_batch_msm_partial (words 18..21 are zero: e = 0 on every lane).  An empty shard gives the identity
 *       record.  The messages are read only by shards of at most SSA_MSM_SMALL_MAX lanes, whose kernel hashes for itself.
 *   ssa_aggregate_combine_device      k (1..4096) partial scalars -> e_agg (canonical).
 *   ssa_verify_aggregate_combine_device   k (1..4096) records, e_agg (32 bytes) and n -> the verdict of
 *       ssa_verify_aggregate: the records are added up and compared with [e_agg]G in BOTH coordinates.  FAILS CLOSED as
 *       ssa_msm_combine: a record without the magic word, with a set malformed word, a non-canonical limb or scalar or a
 *       point off the curve gives SSA_MALFORMED.  n == 0: the rule of the empty aggregate (records are not read).
 *
 * ssa_aggregate_many_sliced / ssa_verify_aggregate_sliced (and _device): arguments, flags and return values of
 * ssa_aggregate_many / ssa_verify_aggregate, on one context, for any n <= SSA_MAX_BATCH: the slices are the shards.  B is
 * the largest power of two not above the context's MSM slice (SSA_AGG_BLOCK overrides it, for tests).  The validator
 * keeps the challenge scalars of all n lanes (32 bytes per lane); every other workspace is one slice's.
 * ssa_multi_aggregate_many / ssa_multi_verify_aggregate: host buffers, the blocks dealt to the devices of an ssa_multi
 * in contiguous runs whose block counts differ by at most one (B from the first context); one host thread per device,
 * root and combination on device 0. */
int ssa_aggregate_shard_tops_device(ssa_ctx *ctx, const uint8_t *d_lanes, uint32_t lane_stride, const uint8_t *d_pks,
                                    const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                    size_t n_s, size_t block_lanes, uint8_t *d_tops_out, uint64_t *d_h_out);
int ssa_aggregate_root_device(ssa_ctx *ctx, const uint8_t *d_tops, size_t n_tops, size_t n, size_t block_lanes,
                              uint8_t *d_root_out);
int ssa_aggregate_shard_fold_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                    size_t n_s, size_t lane0, const uint8_t *d_root, uint8_t *d_e_out, uint8_t *d_rs_out,
                                    uint8_t *d_status_out, uint64_t *d_n_fail_out);
int ssa_verify_aggregate_shard_device(ssa_ctx *ctx, const uint8_t *d_rs49, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                      const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                      const uint64_t *d_h, size_t n_s, size_t lane0, const uint8_t *d_root,
                                      uint64_t *d_record_out);
int ssa_aggregate_combine_device(ssa_ctx *ctx, const uint8_t *d_partials32, size_t k, uint8_t *d_e_agg_out);
int ssa_verify_aggregate_combine_device(ssa_ctx *ctx, const uint64_t *d_records24, size_t k, const uint8_t *d_e_agg,
                                        size_t n, uint32_t *d_verdict_out);
int ssa_aggregate_many_sliced(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                              const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                              uint32_t flags, uint8_t *agg_out, uint8_t *status_out, uint64_t *n_fail_out);
int ssa_aggregate_many_sliced_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                     const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                     size_t n, uint32_t flags, uint8_t *d_agg_out, uint8_t *d_status_out,
                                     uint64_t *d_n_fail_out);
int ssa_verify_aggregate_sliced(ssa_ctx *ctx, const uint8_t *agg, const uint8_t *pks, const uint8_t *pk_inf,
                                const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n);
int ssa_verify_aggregate_sliced_device(ssa_ctx *ctx, const uint8_t *d_agg, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                       const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                       size_t n, uint32_t *d_verdict_out);
int ssa_multi_aggregate_many(ssa_multi *m, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                             const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                             uint32_t flags, uint8_t *agg_out, uint8_t *status_out, uint64_t *n_fail_out);
int ssa_multi_verify_aggregate(ssa_multi *m, const uint8_t *agg, const uint8_t *pks, const uint8_t *pk_inf,
                               const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n);
/* tests: the coefficients a_(lane0 + i), i < n_s, of an aggregate with this root (host) -> n_s x 16 bytes */
int ssa_debug_aggregate_shard_coeffs(ssa_ctx *ctx, const uint8_t root[32], size_t n_s, size_t lane0,
                                     uint8_t *coeffs16_out);

/* ---- many aggregates in one call --------------------------------------------------------
 * k aggregates, one verdict each: verdicts_out[j] is the value ssa_verify_aggregate returns for aggregate j handed in
 * alone with its own keys and messages -- SSA_OK, SSA_INVALID_SIGNATURE or SSA_MALFORMED; for n_j = 0 the 32 bytes must
 * be zero --, for every input and on every internal path.  The transcript is that of section 20, bit for bit.
 *   counts[j] = n_j, a HOST array in both forms (the library plans its launches from it without a read-back);
 *   aggs      = the k aggregates in their wire form, end to end: aggregate j starts at byte 49 (n_0 + ... + n_(j-1)) + 32 j;
 *   pks, pk_inf, messages belong to the N = sum n_j lanes, in the same order.
 * The return value reports errors only (a rejected aggregate is a result): SSA_ERR_ARG for an n_j above the context's
 * MSM slice, N above SSA_MAX_BATCH, or a null pointer the single call refuses.  k == 0: SSA_OK.  The _device form takes
 * device pointers but for counts, and only enqueues on the context's stream. */
int ssa_verify_aggregates_many(ssa_ctx *ctx, const uint8_t *aggs, const uint64_t *counts, size_t k, const uint8_t *pks,
                               const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                               size_t msg_len, uint32_t *verdicts_out);
int ssa_verify_aggregates_many_device(ssa_ctx *ctx, const uint8_t *d_aggs, const uint64_t *counts, size_t k,
                                      const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                      const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                      uint32_t *d_verdicts_out);
/* tests: the plan of such a call from its counts alone (host code, no device).  out[0..4) = lanes, tree passes, groups,
 * descriptors in all; six words per group (first aggregate, aggregates, first lane, lanes, padded segment length,
 * 1 = bucket path); then per pass its number of workgroups and four words each (first node, nodes, output slot, n_j if
 * the workgroup writes a root, else 0).  Returns the words the plan takes -- out receives them if out_words is enough --
 * or SSA_ERR_ARG. */
int64_t ssa_debug_aggregates_plan(const uint64_t *counts, size_t k, size_t msm_slice, size_t small_max, uint64_t *out,
                                  size_t out_words);
/* tests: the coefficients of all N lanes as ssa_verify_aggregates_many derives them (host buffers) -> N x 16 bytes */
int ssa_debug_aggregates_many_coeffs(ssa_ctx *ctx, const uint8_t *aggs, const uint64_t *counts, size_t k,
                                     const uint8_t *pks, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                     size_t msg_len, uint8_t *coeffs16_out);

/* ---- many aggregates produced in one call -----------------------------------------------
 * The producer's side of ssa_verify_aggregates_many: k batches of signatures become k aggregates, in the wire layout that
 * call reads.  The contract is one equality, per aggregate: the 49 n_j + 32 bytes of aggregate j, results_out[j] and the
 * status bytes of its lanes are what ssa_aggregate_many writes to agg_out, returns and writes to status_out for batch j
 * handed in alone with the same flags.
 *   counts[j] = n_j, a HOST array in both forms;
 *   sigs (stride 81), pks, pk_inf and the messages belong to the N = sum n_j lanes, in order;
 *   flags     = 0 or SSA_AGG_CHECK (any other bit: SSA_ERR_ARG);
 *   aggs_out  receives 49 N + 32 k bytes: aggregate j at byte 49 (n_0 + ... + n_(j-1)) + 32 j;
 *   results_out[j] = SSA_OK, SSA_MALFORMED or, with SSA_AGG_CHECK, the smallest nonzero status of the aggregate's lanes.
 * A refused aggregate (results_out[j] != 0) is zeroed, all 49 n_j + 32 bytes of it, and changes no byte of any other;
 * n_j = 0 gives 32 zero bytes and SSA_OK.  *n_fail_out = the failing lanes of the whole call.  status_out, n_fail_out and
 * results_out may be NULL.  The return value reports errors only: SSA_ERR_ARG for exactly the sizes and null pointers
 * ssa_verify_aggregates_many refuses (an n_j above the context's MSM slice, N above SSA_MAX_BATCH).  k == 0: SSA_OK.
 * The refusal is decided on the device, per aggregate: without SSA_AGG_CHECK the _device form only enqueues on the
 * context's stream, with it the call synchronises no more than ssa_verify_batch_screened_device over the N lanes does. */
int ssa_aggregates_many(ssa_ctx *ctx, const uint8_t *sigs, const uint64_t *counts, size_t k, const uint8_t *pks,
                        const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                        size_t msg_len, uint32_t flags, uint8_t *aggs_out, uint32_t *results_out, uint8_t *status_out,
                        uint64_t *n_fail_out);
int ssa_aggregates_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint64_t *counts, size_t k, const uint8_t *d_pks,
                               const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                               size_t msg_len, uint32_t flags, uint8_t *d_aggs_out, uint32_t *d_results_out,
                               uint8_t *d_status_out, uint64_t *d_n_fail_out);
/* tests: the partial sums of that call's fold from its counts alone (host code, no device).  out[0] = partials in all,
 * out[1 .. k + 2) = pfirst: aggregate j shares lanes with pfirst[j + 1] - pfirst[j] workgroups of 256 dense lanes (0 if it
 * is empty).  Returns the k + 2 words this takes -- out receives them if out_words is enough -- or SSA_ERR_ARG. */
int64_t ssa_debug_aggregates_fold_plan(const uint64_t *counts, size_t k, uint64_t *out, size_t out_words);

/* ---- many aggregates through a key cache, subgroup check included -----------------------
 * ssa_verify_aggregates_many with the key cache of sections 16, 18 and 19 in front: every distinct key is checked
 * (limbs, curve, [q]P) once and then found in the cache, a wire key is decompressed once, and an aggregate that holds a
 * key outside the prime-order subgroup is answered SSA_INVALID_PUBLIC_KEY -- the guarantee of Signature::verify
 * (src/signature.rs:182-186) for every lane of the aggregate.  aggs, counts (a HOST array in both forms), k and the
 * messages are those of ssa_verify_aggregates_many; N = sum counts[j].
 *   ssa_verify_aggregates_many_cached(_device)       N affine keys (96 bytes each, optional pk_inf), an affine cache;
 *   ssa_verify_aggregates_many_cached_wire(_device)  N dense 49-byte keys, a cache made with SSA_KEYCACHE_WIRE.
 * Let U be the keys as the aggregate verifier reads them: the caller's arrays, or for wire keys what
 * ssa_decompress_many gives (the affine key, (0, 0) for a key that does not decode, and pk_inf); V_j the value
 * ssa_verify_aggregate returns for aggregate j alone on U; ks_i the status byte ssa_keyset_status reports for key i
 * (0, SSA_INVALID_PUBLIC_KEY for a key on the curve outside the subgroup, else SSA_MALFORMED).  Then
 *   verdicts_out[j] = SSA_INVALID_PUBLIC_KEY   if some lane i of aggregate j has ks_i == SSA_INVALID_PUBLIC_KEY,
 *                   = V_j                      otherwise
 * -- an equality, not a probability (no screen is involved), in every state of the cache (cold, warm, cleared or
 * compacted in the middle of the call, bypassed) and on both group paths of section 21.  The key decides, as in the
 * reference and in ssa_verify_many.  A malformed key needs no rule: V_j is then SSA_MALFORMED.  An empty aggregate has no
 * key: V_j.
 * NOT added: a subgroup check of the R's.  Signature::verify makes none (its R is recomputed).  With every key in the
 * subgroup the sum of the a_i R_i is forced into it; small-order parts of single R's that cancel under the
 * transcript's coefficients remain possible.
 * Errors: a NULL cache, a cache of the other mode, of another context or orphaned is SSA_ERR_ARG, and the cache is left
 * untouched; every other argument error is that of ssa_verify_aggregates_many.  k == 0: SSA_OK.  The return value
 * reports errors only.  The cache is used for every N >= 1: there is no small-batch bypass.
 * stats_out (8 words, HOST memory in both forms, may be NULL), summed over the slices of SSA_LANE_SLICE lanes:
 *   [0] distinct keys  [1] keys found in the cache  [2] keys checked and inserted  [3] automatic clears or compactions
 *   [4] slices that bypassed the cache  [5] lanes at the probe bound plus rows that could not be published
 *   [6] aggregates answered SSA_INVALID_PUBLIC_KEY  [7] 0;   [1] + [2] == [0] over the slices that used the cache.
 * The _device forms take device pointers but for counts and stats_out.  They SYNCHRONISE the context's stream once per
 * slice of SSA_LANE_SLICE lanes -- the key dedup's one read-back, as in ssa_verify_many_cached_device; the aggregate
 * stages behind it are only enqueued.  A caller that passes stats_out waits once more, at the end, for words [5] and
 * [6], which the device counts. */
int ssa_verify_aggregates_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *aggs, const uint64_t *counts, size_t k,
                                      const uint8_t *pks, const uint8_t *pk_inf, const uint8_t *msgs,
                                      const uint64_t *msg_off, size_t msg_stride, size_t msg_len, uint32_t *verdicts_out,
                                      uint64_t stats_out[8]);
int ssa_verify_aggregates_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_aggs, const uint64_t *counts,
                                             size_t k, const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                             const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                             uint32_t *d_verdicts_out, uint64_t stats_out[8]);
int ssa_verify_aggregates_many_cached_wire(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *aggs, const uint64_t *counts,
                                           size_t k, const uint8_t *pks49, const uint8_t *msgs, const uint64_t *msg_off,
                                           size_t msg_stride, size_t msg_len, uint32_t *verdicts_out,
                                           uint64_t stats_out[8]);
int ssa_verify_aggregates_many_cached_wire_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_aggs,
                                                  const uint64_t *counts, size_t k, const uint8_t *d_pks49,
                                                  const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                                  size_t msg_len, uint32_t *d_verdicts_out, uint64_t stats_out[8]);

/* ---- filtering half-aggregation: drop the lanes that fail, aggregate the rest ----------
 * What a block producer needs: n signatures in, the aggregate of exactly the lanes that verify out, and the list of
 * those lanes.  Let S be the status vector ssa_verify_batch_screened (library-drawn coefficients) gives the input and
 * K = { i : S[i] == 0 } in ascending order.  Then
 *   *n_kept_out = |K|,  kept_out[0, |K|) = K,  status_out = S (status_out may be NULL),
 *   the first SSA_AGGREGATE_LENGTH(|K|) bytes of agg_out are byte for byte what ssa_aggregate_many (flags 0) returns
 *   for the lanes of K handed in alone in that order,
 *   the rest of agg_out (capacity SSA_AGGREGATE_LENGTH(n)) and of kept_out (capacity n words) is zero.
 * |K| == 0 gives 32 zero bytes: the empty aggregate, which ssa_verify_aggregate accepts for n = 0.  n == 0: SSA_OK,
 * *n_kept_out = 0, 32 zero bytes.  The return value reports errors only (a dropped lane is a result): SSA_ERR_ARG for a
 * null agg_out, kept_out or n_kept_out, and for n above the context's MSM slice.
 * The guarantee is that of SSA_AGG_CHECK: verify_batch semantics (the flag byte of R_i honoured, pk_inf marks identity
 * keys, NO subgroup check of keys or R's), and a lane that does not verify is kept only with the probability a
 * screened segment accepts it: about 2^-128 for an error with a prime-order component, 1/l for
 * an error of pure small order l, which needs a key or an R outside the prime-order subgroup.
 * The call hashes every message ONCE: the same launch gives the screen its challenge scalars and the transcript its
 * digests; only the digests and signatures of the kept lanes are moved, keys and messages never.
 * The _device form takes device pointers except n_kept_out, a HOST pointer in both forms: the call SYNCHRONISES the
 * context's stream twice -- once inside the screen (for its segment verdicts; not at all for a batch of at most
 * SSA_MSM_SMALL_MAX lanes) and once for |K|, by which it sizes its remaining launches and the caller whatever reads the
 * aggregate.  The remaining launches are only enqueued. */
int ssa_aggregate_valid_many(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                             const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                             uint8_t *agg_out, uint32_t *kept_out, uint64_t *n_kept_out, uint8_t *status_out);
int ssa_aggregate_valid_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                    const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                    size_t n, uint8_t *d_agg_out, uint32_t *d_kept_out, uint64_t *n_kept_out,
                                    uint8_t *d_status_out);
/* tests: the compaction alone.  status (n bytes, host) -> kept_out (the indices of the zero bytes, ascending, then zeros
 * up to n), *n_kept_out their number */
int ssa_debug_aggregate_keep(ssa_ctx *ctx, const uint8_t *status, size_t n, uint32_t *kept_out, uint64_t *n_kept_out);

/* ---- filtering half-aggregation through a key cache, subgroup check included -----------
 * ssa_aggregate_valid_many under the verdict the validator's call applies (ssa_verify_aggregates_many_cached, section
 * 23): a lane is kept iff ssa_verify_many_cached -- respectively ssa_verify_keyed_many_cached -- with
 * SSA_FLAG_CHECK_TORSION | SSA_FLAG_SIG_FLAG_BYTE and library-drawn coefficients gives it status 0, so a key outside
 * the prime-order subgroup drops its lane (status SSA_INVALID_PUBLIC_KEY; the key decides) instead of spoiling the
 * block.  Let S be that status vector and K = { i : S[i] == 0 } in ascending order.  Then, in every state of the cache
 * (cold, warm, partly warm, cleared or compacted in the middle of the call, bypassed):
 *   status_out = S, stats_out = the 12 words of that call, and the cache is left as that call leaves it: it is used
 *     exactly where that call uses it (not for a call, or a last slice, of at most SSA_MSM_SMALL_MAX lanes);
 *   *n_kept_out = |K|,  kept_out[0, |K|) = K;
 *   the first SSA_AGGREGATE_LENGTH(|K|) bytes of agg_out are byte for byte what ssa_aggregate_many (flags 0) returns
 *     for the lanes of K handed in alone in that order (for records: split into signatures and decompressed keys);
 *   pks_out (96 bytes per kept lane) and pk_inf_out (one byte per kept lane; all zero when pk_inf is NULL), or
 *     keys49_out (49 bytes per kept lane: the first 49 bytes of the lane's record), hold the kept lanes' keys
 *     verbatim, in that order;
 *   the rest of agg_out (capacity SSA_AGGREGATE_LENGTH(n)), kept_out (n words) and the key outputs (n keys) is zero.
 * agg_out and the key output, unchanged, with the kept lanes' messages, k = 1 and counts = { |K| }, are what
 * ssa_verify_aggregates_many_cached (respectively _cached_wire) takes, and on the same cache that call answers SSA_OK
 * without building a key table or decompressing a key: every kept key is in the cache, unless the call above bypassed
 * it or did not use it.
 *   ssa_aggregate_valid_many_cached(_device)        signatures and affine keys, an affine cache;
 *   ssa_aggregate_valid_keyed_many_cached(_device)  n x 130-byte KeyedSignature records (key 49 || signature 81), a
 *                                                   cache made with SSA_KEYCACHE_WIRE.
 * The MESSAGES of the kept lanes are NOT gathered: the caller has kept_out, and compacting messages of variable length
 * is a piece of work of its own.
 * Every message is hashed ONCE, as in ssa_aggregate_valid_many: the affine form hashes all n lanes in front of the
 * first slice, the keyed form hashes each slice behind its cache look-up (the affine key exists only then).
 * Errors: a NULL cache, a cache of the other mode, of another context or orphaned is SSA_ERR_ARG, as are a null
 * agg_out, kept_out or n_kept_out and n above the context's MSM slice (SSA_MSM_SLICE); the cache is then untouched.
 * n == 0: SSA_OK, *n_kept_out = 0, 32 zero bytes.  The return value reports errors only: a dropped lane is a result.
 * status_out, pks_out, pk_inf_out, keys49_out and stats_out may be NULL.  stats_out and n_kept_out are HOST memory in
 * both forms.  The _device forms synchronise the context's stream as ssa_verify_many_cached_device does, slice by
 * slice, and once more for |K|; the launches behind that are only enqueued. */
int ssa_aggregate_valid_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *sigs, const uint8_t *pks,
                                    const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                    size_t msg_len, size_t n, uint8_t *agg_out, uint32_t *kept_out, uint64_t *n_kept_out,
                                    uint8_t *status_out, uint8_t *pks_out, uint8_t *pk_inf_out, uint64_t stats_out[12]);
int ssa_aggregate_valid_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_sigs, const uint8_t *d_pks,
                                           const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                           size_t msg_stride, size_t msg_len, size_t n, uint8_t *d_agg_out,
                                           uint32_t *d_kept_out, uint64_t *n_kept_out, uint8_t *d_status_out,
                                           uint8_t *d_pks_out, uint8_t *d_pk_inf_out, uint64_t stats_out[12]);
int ssa_aggregate_valid_keyed_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *keyed, const uint8_t *msgs,
                                          const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                          uint8_t *agg_out, uint32_t *kept_out, uint64_t *n_kept_out, uint8_t *status_out,
                                          uint8_t *keys49_out, uint64_t stats_out[12]);
int ssa_aggregate_valid_keyed_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_keyed,
                                                 const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                                 size_t msg_len, size_t n, uint8_t *d_agg_out, uint32_t *d_kept_out,
                                                 uint64_t *n_kept_out, uint8_t *d_status_out, uint8_t *d_keys49_out,
                                                 uint64_t stats_out[12]);

/* ---- streaming aggregator: push signatures as they arrive, finish at block time ----------
 * Every producer call above takes the whole batch when the block is closed.  A block producer receives its signatures
 * over the whole slot; only the coefficients have to wait for block time, because they need the root and the root needs
 * every leaf.  An ssa_aggregator holds, on the device and in arrival order, the lanes admitted so far -- their R's in the
 * aggregate's wire layout, their scalars, their leaves and the top of every complete block of block_lanes leaves -- so
 * that the challenge hash, the admission check, the leaves and most of the tree are paid on arrival, and block time pays
 * one permutation, one multiplication and a sum per lane.  It belongs to the context it was created on, like a key cache.
 *   create   capacity: 1 .. SSA_MAX_BATCH lanes; block_lanes: 0 (the default, 512) or a power of two from 2 to 512 (small
 *            values let tests reach every path of the tree at a few thousand lanes); flags: 0 or any of
 *            SSA_AGGR_HOLD_KEYS49, SSA_AGGR_HOLD_ADMISSION and SSA_AGGR_HOLD_INDEX (below).  Anything else: SSA_ERR_ARG.  All device memory is allocated here -- 49 capacity + 32 bytes of R's, 32 bytes of scalar and 32
 *            bytes of leaf per lane, 32 bytes per block: about 113 bytes per lane -- and is the object's own: destroy
 *            releases it, or ssa_ctx_destroy (the handle then stays valid for destroy and is refused everywhere else).
 *   push     the arguments of ssa_aggregate_valid_many.  Let S be the status vector: with flags == 0 the one
 *            ssa_verify_batch_screened (library-drawn coefficients) gives THIS batch alone, with its guarantee and its
 *            exact path for small batches; with SSA_AGGR_NO_SCREEN, S[i] is 0 or SSA_MALFORMED by exactly the checks
 *            ssa_aggregate_many makes without SSA_AGG_CHECK (e < q, canonical limbs, key on the curve, R decodable) -- for
 *            a producer that made the signatures itself.  The lanes with S[i] == 0 are appended in lane order;
 *            status_out (may be NULL) = S, *n_kept_out (HOST memory in both forms) = their number.  A dropped lane is a
 *            result: the return value reports errors only.  SSA_ERR_ARG: a context other than the object's, an unknown
 *            flag, n above the context's MSM slice, or n > capacity - held -- by n, not by the kept count, so that a push
 *            is never applied in part; the object is then unchanged.  n == 0: SSA_OK.  The same signature pushed twice
 *            is held twice.  Every message is hashed ONCE.  The _device form synchronises the context's stream as
 *            ssa_aggregate_valid_many_device does: once inside the screen (never with SSA_AGGR_NO_SCREEN) and once for
 *            the kept count, which the object keeps on the host from then on.
 *   finish   writes SSA_AGGREGATE_LENGTH(n_take) bytes: byte for byte what ssa_aggregate_many (flags 0) returns for the
 *            first n_take admitted lanes handed in alone in that order.  n_take == SIZE_MAX: all lanes held;
 *            n_take > held: SSA_ERR_ARG; n_take == 0: 32 zero bytes.  n_take is the block-size limit: a producer whose
 *            pool exceeds the block takes a prefix.  finish changes NO state of the object but a counter: it may be
 *            repeated, called with another n_take, and followed by more pushes.  The _device form only enqueues.
 *   reset    empties the object (counters included) and keeps its memory.
 *   info     [0] lanes held  [1] capacity  [2] block_lanes  [3] pushes  [4] lanes offered  [5] lanes dropped
 *            [6] blocks whose top is stored  [7] finishes.
 *   drop_front, remove   take lanes OUT of the object in place: the lanes a block took from the
 *            front, or lanes withdrawn anywhere.  Let L be the lanes held and K the ascending list of the kept ones: after
 *            the call the object is indistinguishable from one that admitted L[K[0]], L[K[1]], ... in that order --
 *            info [0] == |K|, [6] == |K| / block_lanes, every finish(n_take <= |K|) is byte for byte the ssa_aggregate_many
 *            of the first n_take kept lanes handed in alone, later pushes append behind lane |K|.  The counters pushes,
 *            offered, dropped and finishes do not move ("dropped" counts refused admissions, not withdrawals).  No
 *            message, key or signature is touched again: the stored R, scalar and leaf of a lane do not depend on its
 *            place, so the kept lanes are moved and only the blocks that changed are reduced again.
 *            drop_front(n) removes the first n held lanes; n == SIZE_MAX or n == held: all of them; n == 0: SSA_OK,
 *            nothing is launched; n > held: SSA_ERR_ARG.  It only enqueues, as finish_device does.
 *            remove takes one byte per held lane: n_bytes must equal the lanes held, and lane i is removed iff
 *            drop[i] != 0 -- the status-vector convention, so the status_out of a screen can be handed in as it is; every
 *            byte vector is valid.  *n_kept_out (HOST memory in both forms) = |K|.  The _device form synchronises the
 *            context's stream once, for that count.
 *            SSA_ERR_ARG, with the object, its info and every later finish unchanged: a context other than the object's,
 *            an orphaned object, a NULL mask with lanes held, a NULL n_kept_out, the length and range errors above.
 *            A move in place cannot be undone: a runtime error (SSA_ERR_HIP) once the move has begun leaves the object
 *            EMPTY (0 lanes held, counters as they were), never half-moved.
 *   push_cached, push_keyed_cached   admission through a key cache, under the verdict validators apply (DESIGN.md
 *            section 31).  push_cached takes the lanes of push and an AFFINE cache, push_keyed_cached n 130-byte
 *            KeyedSignature records (key 49 || signature 81) and a WIRE cache.  Two equalities, in every state of the
 *            cache (cold, warm, partly warm, cleared or compacted between two slices of the push, bypassed):
 *            the admission -- status_out (may be NULL), the 12 words of stats_out (HOST memory, may be NULL) and the state
 *            of the cache afterwards are exactly those ssa_aggregate_valid_many_cached (for records:
 *            ssa_aggregate_valid_keyed_many_cached) gives THIS batch alone on the same cache: SSA_FLAG_CHECK_TORSION |
 *            SSA_FLAG_SIG_FLAG_BYTE, library-drawn coefficients, the cache used exactly where that call uses it (not for
 *            a push, or a last slice, of at most the context's small-batch bound), and the key deciding over a bad
 *            signature in the same lane;
 *            the object -- the lanes of status 0 are appended in lane order, and every later finish(n_take) is byte for
 *            byte ssa_aggregate_many (flags 0) on the first n_take admitted lanes handed in alone (records: split into
 *            signatures and decompressed keys), whichever kind of push admitted each lane: plain, cached and keyed pushes
 *            may be mixed in one object, the stored R, scalar and leaf do not depend on how a lane came in.
 *            Everything else follows push: every message is hashed ONCE; a push is refused by n; n == 0 counts a push
 *            and touches neither cache nor object; *n_kept_out is HOST memory in both forms; the return value reports
 *            errors only.  SSA_ERR_ARG, with object and cache untouched: a NULL cache, a cache of the other mode, of
 *            another context or orphaned, and everything push refuses.  The _device forms synchronise as
 *            ssa_aggregate_valid_many_cached_device does.
 *   SSA_AGGR_HOLD_KEYS49 (create flag)   the object also holds the 49 wire bytes of every admitted lane's key, in arrival
 *            order: 49 more bytes per lane, about 162 in all.  Such an object takes push_keyed_cached ONLY -- the other
 *            pushes carry no wire key: SSA_ERR_ARG, the object unchanged.  keys(n_take) writes the first n_take held
 *            lanes' keys, 49 n_take bytes -- the first 49 bytes of each lane's record, verbatim -- by the conventions of
 *            finish: SIZE_MAX = all lanes held, n_take > held is SSA_ERR_ARG, n_take == 0 writes nothing, the _device form
 *            only enqueues, no state of the object changes.  On an object created without the flag: SSA_ERR_ARG.
 *            drop_front, remove and reset treat the key column as they treat the R's: after a removal the object is
 *            indistinguishable, keys included, from one that admitted the kept lanes alone.  The outputs of finish and
 *            keys, unchanged, with the kept messages, k = 1 and counts = {n}, are what
 *            ssa_verify_aggregates_many_cached_wire takes; on the same cache that call finds every key (stats[2] == 0)
 *            unless the push bypassed the cache or did not use it.
 *   SSA_AGGR_HOLD_ADMISSION (create flag)   the object also records HOW each lane was admitted: one
 *            more byte per lane, `adm`, written by the library behind every push and by nobody else:
 *              SSA_ADM_UNSCREENED (0)    a push with SSA_AGGR_NO_SCREEN: the caller's own word;
 *              SSA_ADM_SCREENED (1)      the plain screened push: the lane's equation is established, its key has had
 *                                        no subgroup check;
 *              SSA_ADM_KEY_CHECKED (2)   push_cached or push_keyed_cached, with or without the key column: the equation
 *                                        and the subgroup check of the key.
 *            The byte moves with its lane under drop_front, remove and remove_indices (after a removal the object is
 *            indistinguishable, classes included, from one that admitted the kept lanes alone by the same kinds of
 *            push); reset forgets it; finish, finish_select and keys neither read nor write it.  admission(n_take)
 *            writes the first n_take held lanes' classes, n_take bytes, by the conventions of keys: SIZE_MAX = all lanes
 *            held, n_take > held is SSA_ERR_ARG, n_take == 0 writes nothing, the _device form only enqueues, no state of
 *            the object changes.  On an object created without the flag: SSA_ERR_ARG.  Such an object allocates what
 *            it did before the flag existed and enqueues exactly the launches and copies it did.  The classes are what
 *            ssa_aggverifier_push_mixed_cached requires of the lanes it takes from the pool.
 *   finish_select, remove_indices   CHOOSE among the held lanes: a producer fills its block with the
 *            lanes it wants, in an order of its own, and keeps the rest.  Let L be the lanes held; order[0, m) names m
 *            DISTINCT places < held.  finish_select writes SSA_AGGREGATE_LENGTH(m) bytes: byte for byte what
 *            ssa_aggregate_many (flags 0) returns for L[order[0]], ..., L[order[m - 1]] handed in alone in that order.
 *            Like finish it changes no state of the object but the `finishes` counter (every call that passes the
 *            argument checks counts): it may be repeated, mixed with finish, and followed by pushes and removals.
 *            keys49_out (may be NULL; otherwise the object must have SSA_AGGR_HOLD_KEYS49, else SSA_ERR_ARG) receives the
 *            selected lanes' 49 key bytes in the same order, 49 m bytes; the two outputs, with the selected messages,
 *            k = 1 and counts = {m}, are what ssa_verify_aggregates_many_cached_wire takes.  m == 0: 32 zero bytes.  No
 *            message, key or signature is touched: the call gathers the stored leaves, scalars, R's and keys, runs the
 *            tree over the gathered leaves and the coefficient fold of finish.
 *            SSA_ERR_ARG before anything is launched: m > held, m above the context's MSM slice, a NULL order with
 *            m > 0, a NULL agg_out, an object of another context or an orphaned one, a device list that is not 4-byte
 *            aligned, a NULL d_result_out.
 *            Whether the list is valid -- every index < held, no index twice -- is decided ON THE DEVICE.  An invalid list
 *            zeroes the outputs (SSA_AGGREGATE_LENGTH(m) bytes, and 49 m bytes of keys), the way ssa_aggregates_many
 *            refuses an aggregate, and no lane outside [0, held) is read.  The host form then returns SSA_ERR_ARG; the
 *            _device form only enqueues and writes *d_result_out (DEVICE memory, required): 0 valid, 1 invalid.  Either
 *            way the object is unchanged and a later finish gives the bytes it gave before.
 *            remove_indices is remove with a list in place of a mask: the lanes named are removed, everything else stays
 *            in arrival order, and the object then equals the one remove leaves for the equivalent mask.  The list obeys
 *            the rules above (any m <= held: no slice limit); an invalid one is SSA_ERR_ARG with the object unchanged --
 *            the device's verdict is read before the move begins.  *n_kept_out (HOST memory in both forms) = the lanes
 *            kept (for a refused list: the lanes held).  m == 0: SSA_OK, nothing is launched.  The _device form
 *            synchronises the context's stream once, as remove_device does.
 *   leaves, leaves_select   the LEAF column.  Every held lane has a 32-byte leaf,
 *            H(d || flag byte of R || 0xA1) of its challenge digest: the one value that binds (R, key, message) and that
 *            the aggregator and the aggregate verifier compute identically.  It is the lane's ID.  Both calls work on
 *            every aggregator, whatever its flags, and change no state.  leaves(n_take) writes the first n_take held
 *            lanes' leaves, 32 n_take bytes, by the conventions of keys: SIZE_MAX = all lanes held, n_take > held is
 *            SSA_ERR_ARG, n_take == 0 writes nothing, the _device form is one device-to-device copy.  leaves_select
 *            writes the leaves at the places order[0], ..., order[m - 1] in that order, 32 m bytes: the id column that
 *            goes beside finish_select on the same list.  An index >= held is refused and no lane outside [0, held) is
 *            read: the host form zeroes the 32 m bytes and returns SSA_ERR_ARG; the _device form only enqueues, zeroes
 *            them and writes *d_result_out (DEVICE memory, 4-byte aligned, required) = 1, else 0.  A place named twice
 *            is written twice: whether a list may repeat a place is finish_select's decision.  m == 0: SSA_OK, nothing
 *            is launched or written.  SSA_ERR_ARG before anything is launched: NULL arguments with m > 0,
 *            m > SSA_MAX_BATCH, an object of another context or an orphaned one, a device list that is not 4-byte aligned.
 *   SSA_AGGR_HOLD_INDEX (create flag)   the object also holds a LEAF INDEX: a table on the device,
 *            8 bytes per slot with at least four slots per lane of the capacity (a power of two, at least 1024) and one
 *            8-byte counter, that answers "which of my places holds this leaf?".  It is what a validator needs to
 *            receive a compact block -- ids plus the few lanes it lacks -- since the pool's places move under every
 *            removal, some of them by masks that exist on the device only.  Combinable with the other create flags.
 *            lookup(ids32, n): places_out[i] = the LOWEST place p < held whose leaf equals the 32 bytes
 *            ids32[32 i, 32 i + 32), or SSA_AGGV_UNKNOWN; an id that occurs several times gets the same answer each
 *            time.  *n_unknown_out = the number of SSA_AGGV_UNKNOWN answers: with places_out, exactly what
 *            ssa_aggverifier_push_mixed* takes as places and as the count of lanes that come with the call.  The
 *            _device form only enqueues on the context's stream; d_ids32 may lie at any byte alignment (read by 64-bit
 *            words when 8-aligned, byte by byte otherwise), d_places_out and d_n_unknown_out (ONE uint32, device memory)
 *            are 4-byte aligned, else SSA_ERR_ARG.  The host form stages and copies back like every host form;
 *            *n_unknown_out is then a uint64 in host memory.  n == 0: SSA_OK, count 0, nothing is launched;
 *            n > SSA_MAX_BATCH, NULL arguments, an object created without the flag, of another context or orphaned:
 *            SSA_ERR_ARG with nothing written.
 *            THE INDEX IS LAZY.  push*, finish*, keys, admission, drop_front, remove*, and reset enqueue on an object
 *            with the flag exactly what they enqueue on one without.  The object keeps on the host how many lanes the
 *            table covers (`indexed`) and whether it is `stale`: a removal that changed the object, a reset, and a
 *            removal that failed with SSA_ERR_HIP after its move began make it stale.  All index work is enqueued by
 *            index_sync and, identically, in front of every lookup: for a stale table one clear (slots to all-ones,
 *            the counter to zero), then ONE insert launch over the lanes [indexed, held).  So after pushes the insert
 *            is incremental, after a removal it is a rebuild, and a caller takes the rebuild off its critical path by
 *            calling index_sync right behind the removal.  index_sync only enqueues.
 *            FAIL-OPEN.  A returned place is always right: all 32 bytes of the stored leaf were compared, the table's
 *            fingerprint (SipHash-2-4 under the context's random key) only picks slots.  SSA_AGGV_UNKNOWN for an id
 *            the pool DOES hold can happen only for a lane whose insert ran into the probe bound (128 slots by
 *            default, at a load of at most 1/4; index_info word [4] counts such lanes).  The mixed push then treats
 *            that lane as unknown and verifies it from the block body: that costs time and never changes a verdict.
 *            index_info: out[0] slots, [1] lanes indexed, [2] stale (0 / 1), [3] clears of the table so far (rebuilds,
 *            the first build included), [4] lanes that hit the probe bound since the last clear, [5] lookup calls that
 *            launched, [6] ids looked up, [7] 0.  Word [4] is a counter on the device: the call SYNCHRONISES the
 *            context's stream once (not when the table is stale: then it reports 0).
 * NOT here: selections above one MSM slice, reuse of the stored tops for a selection, a column of affine keys, the
 * messages, ssa_multi forms, dropping duplicate leaves on push, short ids, an index on the verifier object.  The
 * validator's counterpart is ssa_aggverifier, below. */
typedef struct ssa_aggregator ssa_aggregator;
#define SSA_AGGR_NO_SCREEN 1u      /* push flag */
#define SSA_AGGR_HOLD_KEYS49 2u    /* create flag */
#define SSA_AGGR_HOLD_ADMISSION 8u /* create flag */
#define SSA_AGGR_HOLD_INDEX 32u    /* create flag */
#define SSA_ADM_UNSCREENED 0u      /* the admission classes of SSA_AGGR_HOLD_ADMISSION */
#define SSA_ADM_SCREENED 1u
#define SSA_ADM_KEY_CHECKED 2u
int ssa_aggregator_create(ssa_ctx *ctx, size_t capacity, size_t block_lanes, uint32_t flags, ssa_aggregator **out);
void ssa_aggregator_destroy(ssa_aggregator *ag);
int ssa_aggregator_reset(ssa_aggregator *ag);
int ssa_aggregator_info(ssa_aggregator *ag, uint64_t out[8]);
int ssa_aggregator_push(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                        const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                        uint32_t flags, uint8_t *status_out, uint64_t *n_kept_out);
int ssa_aggregator_push_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *d_sigs, const uint8_t *d_pks,
                               const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                               size_t msg_len, size_t n, uint32_t flags, uint8_t *d_status_out, uint64_t *n_kept_out);
int ssa_aggregator_push_cached(ssa_ctx *ctx, ssa_aggregator *ag, ssa_keycache *kc, const uint8_t *sigs, const uint8_t *pks,
                               const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                               size_t msg_len, size_t n, uint8_t *status_out, uint64_t *n_kept_out, uint64_t stats_out[12]);
int ssa_aggregator_push_cached_device(ssa_ctx *ctx, ssa_aggregator *ag, ssa_keycache *kc, const uint8_t *d_sigs,
                                      const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                      const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                      uint8_t *d_status_out, uint64_t *n_kept_out, uint64_t stats_out[12]);
int ssa_aggregator_push_keyed_cached(ssa_ctx *ctx, ssa_aggregator *ag, ssa_keycache *kc, const uint8_t *keyed,
                                     const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                     size_t n, uint8_t *status_out, uint64_t *n_kept_out, uint64_t stats_out[12]);
int ssa_aggregator_push_keyed_cached_device(ssa_ctx *ctx, ssa_aggregator *ag, ssa_keycache *kc, const uint8_t *d_keyed,
                                            const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                            size_t msg_len, size_t n, uint8_t *d_status_out, uint64_t *n_kept_out,
                                            uint64_t stats_out[12]);
int ssa_aggregator_finish(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *agg_out);
int ssa_aggregator_finish_device(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *d_agg_out);
int ssa_aggregator_keys(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *keys49_out);
int ssa_aggregator_keys_device(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *d_keys49_out);
/* tests: the bytes create allocates for an object of this capacity, block size and flags (host code, no device):
 * out[0] the R's, [1] the scalars, [2] the leaves, [3] the tops, [4] the key column (0 without SSA_AGGR_HOLD_KEYS49).
 * SSA_ERR_ARG for anything create would refuse. */
int ssa_debug_aggregator_bytes(size_t capacity, size_t block_lanes, uint32_t flags, uint64_t out[5]);
/* tests: the same five words (SSA_AGGR_HOLD_ADMISSION and SSA_AGGR_HOLD_INDEX are accepted by both and change none of
 * them), out[5] the admission column (0 without SSA_AGGR_HOLD_ADMISSION), out[6] the leaf index, 8 bytes per slot and
 * the 8-byte counter (0 without SSA_AGGR_HOLD_INDEX), out[7] = 0. */
int ssa_debug_aggregator_bytes_ex(size_t capacity, size_t block_lanes, uint32_t flags, uint64_t out[8]);
int ssa_aggregator_admission(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *adm_out);
int ssa_aggregator_admission_device(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *d_adm_out);
int ssa_aggregator_leaves(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *ids32_out);
int ssa_aggregator_leaves_device(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *d_ids32_out);
int ssa_aggregator_leaves_select(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *order, size_t m, uint8_t *ids32_out);
int ssa_aggregator_leaves_select_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *d_order, size_t m,
                                        uint8_t *d_ids32_out, uint32_t *d_result_out);
int ssa_aggregator_index_sync(ssa_ctx *ctx, ssa_aggregator *ag);
int ssa_aggregator_lookup(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *ids32, size_t n, uint32_t *places_out,
                          uint64_t *n_unknown_out);
int ssa_aggregator_lookup_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *d_ids32, size_t n, uint32_t *d_places_out,
                                 uint32_t *d_n_unknown_out);
int ssa_aggregator_index_info(ssa_ctx *ctx, ssa_aggregator *ag, uint64_t out[8]);
/* tests: what a push of m kept lanes onto `held` lanes completes with blocks of block_lanes (0: 512) lanes (host code, no
 * device): out[0] the first completed block, out[1] the number of completed blocks, out[2] the first lane of the ragged
 * tail, out[3] its length.  SSA_ERR_ARG for a block size create would refuse or held + m above SSA_MAX_BATCH. */
int ssa_debug_aggregator_plan(uint64_t held, uint64_t m, uint64_t block_lanes, uint64_t out[4]);
int ssa_aggregator_drop_front(ssa_ctx *ctx, ssa_aggregator *ag, size_t n);
int ssa_aggregator_remove(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *drop, size_t n_bytes, uint64_t *n_kept_out);
int ssa_aggregator_remove_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *d_drop, size_t n_bytes,
                                 uint64_t *n_kept_out);
int ssa_aggregator_finish_select(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *order, size_t m, uint8_t *agg_out,
                                 uint8_t *keys49_out);
int ssa_aggregator_finish_select_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *d_order, size_t m,
                                        uint8_t *d_agg_out, uint8_t *d_keys49_out, uint32_t *d_result_out);
int ssa_aggregator_remove_indices(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *order, size_t m, uint64_t *n_kept_out);
int ssa_aggregator_remove_indices_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *d_order, size_t m,
                                         uint64_t *n_kept_out);
/* tests: what a removal does to the stored tops (host code, no device).  held: the lanes held before; first_changed: the
 * first place whose content changes -- the first removed lane; new_held: the lanes kept; first_changed <= new_held <=
 * held.  first_changed == 0 stands for drop_front(held - new_held), the one removal the library plans with that value (a
 * mask that removes lane 0 is planned with every block reduced again).  out[0]: blocks [0, out[0]) keep their tops;
 * out[1]: the tops of blocks [0, out[1]) are MOVED from blocks (held - new_held) / block_lanes onwards (a front drop by a
 * multiple of block_lanes only); blocks [out[2], out[2] + out[3]) are reduced again from the moved leaves.  Every
 * complete block of the new object is in exactly one of the three.  SSA_ERR_ARG for a block size create would refuse,
 * held above SSA_MAX_BATCH, or an order other than the above. */
int ssa_debug_aggregator_remove_plan(uint64_t held, uint64_t first_changed, uint64_t new_held, uint64_t block_lanes,
                                     uint64_t out[4]);

/* ---- streaming aggregate verifier: push a block body as it arrives, finish with e_agg ----
 * The validator's counterpart of the streaming aggregator.  A block body -- the R's, keys and messages of a half-aggregate
 * -- arrives before the verdict can be asked for, and only the coefficients have to wait for the last R.  An
 * ssa_aggverifier holds, on the device and in arrival order, what ssa_verify_aggregate computes per lane without knowing
 * the lane's place: R decompressed and -P as the MSM's point rows, the challenge scalar, the leaf, a "failed a check"
 * byte, and the top of every complete block of block_lanes leaves.  finish pays one permutation and one multiplication
 * per lane, the bucket MSM and the exact comparison.  It belongs to the context it was created on, like a key cache.
 *   create   capacity: 1 .. SSA_MAX_BATCH lanes; block_lanes: 0 (the default, 512) or a power of two from 2 to 512;
 *            flags: 0.  Anything else: SSA_ERR_ARG.  All device memory is allocated here -- 96 + 96 + 32 + 32 + 1 + 1 + 1
 *            bytes per lane and 32 bytes per block: about 259 bytes per lane -- and is the object's own: destroy releases it,
 *            or ssa_ctx_destroy (the handle then stays valid for destroy and is refused everywhere else).
 *   push     n R's at stride 49 (the aggregate's wire layout), their keys, pk_inf (may be NULL) and messages, as
 *            ssa_verify_aggregate takes them.  ALL n lanes are appended: a validator cannot drop a lane, its place is
 *            part of the transcript; a lane that fails a check (non-canonical limbs, key off the curve, R not decodable)
 *            is held as such and makes every finish that takes it SSA_MALFORMED.  SSA_ERR_ARG: a context other than the
 *            object's, n above the context's MSM slice, n > capacity - held, bad message arguments; the object is then
 *            unchanged -- a push is never applied in part.  n == 0: SSA_OK.  Every message is hashed ONCE.  The _device
 *            form only enqueues on the context's stream: it never synchronises.
 *   finish   the status ssa_verify_aggregate returns for the first n_take held lanes handed in at once as
 *            R_0 || ... || R_(n_take-1) || e_agg (e_agg32 / d_e_agg: 32 bytes).  n_take == SIZE_MAX: all lanes held;
 *            n_take > held: SSA_ERR_ARG; n_take == 0: the rule of the empty aggregate (valid iff e_agg is zero).  finish
 *            changes NO state of the object but a counter: it may be repeated, take prefixes, and be followed by more
 *            pushes.  The host form returns the status; the _device form only enqueues and the status lands in the
 *            uint32 at d_verdict_out.  Always the bucket MSM, whatever n_take is.
 *   reset    empties the object (counters included) and keeps its memory.
 *   info     [0] lanes held  [1] capacity  [2] block_lanes  [3] pushes  [4] lanes pushed  [5] lanes pushed through a key
 *            cache (below; 0 for an object that sees plain pushes only.  Lanes that failed a check are known on the
 *            device alone: nothing is read back)  [6] blocks whose top is stored  [7] finishes.
 * NOT here: ssa_multi forms, removing lanes from the front.
 *
 * Through a key cache, subgroup check included.  The plain push verifies under verify_batch
 * semantics: a key P + T with T of small order can pass.  The cached pushes put the key cache of sections 16, 18, 19 and
 * 23 in front: every distinct key is checked (limbs, curve, [q]P) once and then found, a wire key is decompressed once,
 * and the object keeps ONE MORE byte per lane, the key's status.
 *   push_cached(_device)       n affine keys (96 bytes each, optional pk_inf), an affine cache;
 *   push_cached_wire(_device)  n dense 49-byte keys, a cache made with SSA_KEYCACHE_WIRE: the host form uploads 49
 *                              bytes per key instead of 97, and U (section 23) is what ssa_decompress_many gives.
 * The contract is section 23's equality.  If the first n held lanes were all pushed through a cache,
 *   finish(e_agg, n) == ssa_verify_aggregates_many_cached(_wire) with k = 1, counts = {n} and
 *                       aggs = R_0 || ... || R_(n-1) || e_agg on the same keys and messages:
 * SSA_INVALID_PUBLIC_KEY if some lane i < n has key status SSA_INVALID_PUBLIC_KEY, else exactly what finish returns
 * without the cache.  The key decides, also over a malformed R or a wrong e_agg in the same prefix; n_take == 0 keeps
 * the rule of the empty aggregate; exact (no screen), in every state of the cache (cold, warm, partly warm, cleared or
 * compacted between two slices of one push, bypassed).  finish, finish_device and ssa_debug_aggverifier_record keep
 * their signatures, and the record is the same: the key status never enters the MSM.
 * MIXING: plain and cached pushes may be mixed in one object.  A lane of a plain push carries key status 0, "not
 * checked": it never answers SSA_INVALID_PUBLIC_KEY, whatever its key is, and the equality above speaks only of prefixes
 * whose lanes all came through a cache (info word [5] == word [4] says so for the whole object).  An object that never
 * sees a cached push enqueues exactly what it did before these entry points existed.
 * Errors, all SSA_ERR_ARG, the object, the cache and info unchanged: a NULL cache, a cache of the other mode, of
 * another context or orphaned, and everything the plain push refuses.  n == 0 counts a push and touches neither the
 * cache nor the object.  A push is never applied in part (the cache may have taken keys from a push that then failed
 * with SSA_ERR_HIP: the state ssa_verify_many_cached leaves too, and harmless).
 * stats_out (8 words, HOST memory in both forms, may be NULL): words [0] .. [5] of section 23, summed over the slices of
 * this push; [6] = [7] = 0, nothing about verdicts is known before finish.
 * The _device forms SYNCHRONISE the context's stream once per slice of SSA_LANE_SLICE lanes (the key dedup's read-back,
 * as in ssa_verify_aggregates_many_cached_device) and only enqueue behind that; a caller that passes stats_out waits
 * once more, at the end, for the device's part of word [5].  The plain push_device stays enqueue-only. */
typedef struct ssa_aggverifier ssa_aggverifier;
int ssa_aggverifier_create(ssa_ctx *ctx, size_t capacity, size_t block_lanes, uint32_t flags, ssa_aggverifier **out);
void ssa_aggverifier_destroy(ssa_aggverifier *av);
int ssa_aggverifier_reset(ssa_aggverifier *av);
int ssa_aggverifier_info(ssa_aggverifier *av, uint64_t out[8]);
int ssa_aggverifier_push(ssa_ctx *ctx, ssa_aggverifier *av, const uint8_t *rs49, const uint8_t *pks, const uint8_t *pk_inf,
                         const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n);
int ssa_aggverifier_push_device(ssa_ctx *ctx, ssa_aggverifier *av, const uint8_t *d_rs49, const uint8_t *d_pks,
                                const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                size_t msg_stride, size_t msg_len, size_t n);
int ssa_aggverifier_finish(ssa_ctx *ctx, ssa_aggverifier *av, const uint8_t *e_agg32, size_t n_take);
int ssa_aggverifier_finish_device(ssa_ctx *ctx, ssa_aggverifier *av, const uint8_t *d_e_agg, size_t n_take,
                                  uint32_t *d_verdict_out);
/* tests: the 24-word record finish compares with [e_agg]G -- the sum of the pieces' records -- at device address
 * d_record24_out (8-byte aligned), without the comparison.  Only enqueues.  n_take == 0 (no record): SSA_ERR_ARG. */
int ssa_debug_aggverifier_record(ssa_ctx *ctx, ssa_aggverifier *av, size_t n_take, uint64_t *d_record24_out);
int ssa_aggverifier_push_cached(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const uint8_t *rs49, const uint8_t *pks,
                                const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                size_t msg_len, size_t n, uint64_t stats_out[8]);
int ssa_aggverifier_push_cached_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const uint8_t *d_rs49,
                                       const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                       const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                       uint64_t stats_out[8]);
int ssa_aggverifier_push_cached_wire(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const uint8_t *rs49,
                                     const uint8_t *pks49, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                     size_t msg_len, size_t n, uint64_t stats_out[8]);
int ssa_aggverifier_push_cached_wire_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const uint8_t *d_rs49,
                                            const uint8_t *d_pks49, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                            size_t msg_stride, size_t msg_len, size_t n, uint64_t stats_out[8]);
/* tests: the lanes of key statuses one workgroup of finish's fold takes (AGV_KST_SPAN): its edges are where a fold of a
 * long prefix can lose a byte */
size_t ssa_debug_aggverifier_key_span(void);

/* ---- a block against the pool: known lanes by scalar, the rest by MSM ----
 * A validator that follows a chain holds most lanes of an incoming block already: it received, screened and admitted
 * them into an ssa_aggregator, which keeps each lane's leaf and scalar s_i.  For a lane with s_i G = R_i + h_i P_i
 * established, the term a_i (R_i + h_i P_i) of the aggregate's equation is [a_i s_i]G, so
 *     [e_agg - S]G = sum over the unknown lanes of a_i (R_i + h_i P_i),   S = sum over the known lanes of a_i s_i mod q.
 * A known lane costs a gather of 64 bytes, its share of the tree and one coefficient permutation; only the unknown
 * lanes pay the challenge hash, the decompression and the MSM.
 *   push_mixed   appends n lanes.  places[i] is SSA_AGGV_UNKNOWN or a place < held of `ag`, a streaming aggregator of
 *                the same context.  The u unknown lanes come with the call, side by side in block order -- R's at stride
 *                49, keys, pk_inf (may be NULL), messages, exactly as ssa_aggverifier_push takes them -- and are
 *                treated exactly as that call treats them.  A known lane takes the leaf and the scalar of the pool's
 *                lane, COPIED: a later remove or drop_front on the pool does not reach the verifier.  It holds the
 *                (0, 0) rows, no "failed a check" mark and key status "not checked" (the pool's cached push checked its
 *                key on admission).  A place may be named more than once.  push_known is the case u == 0.
 *   finish       unchanged in signature; for a prefix that holds a known lane it answers what ssa_verify_aggregate
 *                answers for the block in which every known lane is replaced by the (R, key, message) the pool admitted
 *                it with, PROVIDED every known lane's stored scalar satisfies its own verification equation.
 * THE CONTRACT IS THE CALLER'S on these entry points, which have no `require` argument.  Lanes admitted by a screened or
 * cached push of the aggregator meet it; a lane pushed with SSA_AGGR_NO_SCREEN is the caller's own word.  A wrong stored
 * scalar makes honest blocks fail, and somebody who knows of such a lane in a validator's pool could craft a block that
 * this path accepts and ssa_verify_aggregate refuses.  Do not name such lanes as known -- or let the library refuse
 * them: ssa_aggverifier_push_mixed_cached (below) with require >= 1 on a pool that records its admissions.
 * Host forms: SSA_ERR_ARG, the object unchanged, for a place >= ag->held that is not the sentinel, u different from the
 * number of sentinels, objects of different contexts or orphaned, n > capacity - held, n or u above the context's MSM
 * slice, bad message arguments, NULL objects, a NULL list with n != 0.
 * _device forms: only enqueue, never synchronise.  d_places (4-byte aligned) and *d_result_out (required) are DEVICE
 * memory; u is the caller's (the size of its compact arrays).  The device decides whether the list is valid and fails
 * closed: a place out of range holds a lane marked as failed, a sentinel count other than u marks every lane of the
 * push so, *d_result_out becomes 1 (0 for a valid list), and every finish whose prefix reaches such a lane answers
 * SSA_MALFORMED.  The lanes are appended either way: reset the object after a refused push.
 * ssa_debug_aggverifier_record gives the record of the prefix's unknown lanes alone (SSA_ERR_ARG when it has none);
 * ssa_debug_aggverifier_known_sum writes S of the first n_take lanes, 32 bytes little-endian, to DEVICE memory (zero
 * without a known lane).  An object that never sees a mixed push enqueues exactly what it did before these entry points
 * existed; it holds one more byte per lane (259 in all).
 * NOT here: ssa_multi forms, known lanes taken from another verifier.  (Mixed pushes through a key cache and the
 * admission class of a pool's lane: the next block.) */
#define SSA_AGGV_UNKNOWN 0xFFFFFFFFu
int ssa_aggverifier_push_mixed(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, const uint32_t *places, size_t n,
                               const uint8_t *rs49, const uint8_t *pks, const uint8_t *pk_inf, const uint8_t *msgs,
                               const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t u);
int ssa_aggverifier_push_mixed_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, const uint32_t *d_places,
                                      size_t n, const uint8_t *d_rs49, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                      const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                      size_t u, uint32_t *d_result_out);
int ssa_aggverifier_push_known(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, const uint32_t *places, size_t m);
int ssa_aggverifier_push_known_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, const uint32_t *d_places,
                                      size_t m, uint32_t *d_result_out);
int ssa_debug_aggverifier_known_sum(ssa_ctx *ctx, ssa_aggverifier *av, size_t n_take, uint8_t *d_s32_out);

/* ---- a block against the pool through the key cache, with a required admission class ----
 * push_mixed with the guarantee of ssa_verify_aggregates_many_cached(_wire), and with its soundness condition checked
 * by the library.  The arguments of push_mixed, a key cache `kc`, and `require`:
 *   unknown lanes   are treated exactly as ssa_aggverifier_push_cached (_wire: push_cached_wire) treats them: the u
 *                compact keys -- affine with pk_inf and an AFFINE cache, or 49-byte wire keys and a WIRE cache -- go
 *                through the cache in slices of the context's lane slice, each distinct key is checked (a wire key
 *                decompressed) once, and each lane's key status is held at the lane's true place in the block.  The
 *                first such push makes the object keyed, as a cached push does.  stats_out (HOST memory, may be NULL):
 *                the eight words of push_cached over the u unknown lanes.
 *   known lanes  require is 0, 1 or 2 (anything else: SSA_ERR_ARG), and a known lane whose admission class in the pool
 *                (SSA_ADM_*, above) is BELOW require is refused exactly as a place out of range is.  require > 0 needs
 *                a pool created with SSA_AGGR_HOLD_ADMISSION, else SSA_ERR_ARG.  require == 0 is push_mixed's contract
 *                on any pool.  A known lane that passes is stored as push_mixed stores it, key status 0.
 * THE CONTRACT.  Take a prefix of n lanes, all pushed through a cache or known lanes of class 2 pushed with
 * require == 2.  finish(e_agg, n) equals ssa_verify_aggregates_many_cached (_wire) with k = 1, counts = {n} on the block
 * in which every known lane is replaced by the (R, key, message) the pool admitted it with -- in every state of the
 * cache, and with nothing owed by the caller beyond having looked up the right places.  What remains is the error
 * probability of the screen that admitted the pool's lanes, stated once.  With require == 1 the
 * equality is with ssa_verify_aggregate, as for push_mixed, now without its proviso; with require == 0 it is push_mixed's.
 * The result word (*d_result_out; the host forms read it themselves): bit 0 = the list is invalid (a place out of range,
 * a sentinel miscount), bit 1 = a known lane was below the required class.
 * Host forms refuse before anything is applied: everything push_mixed and push_cached refuse on the host, and, with
 * require > 0, a pre-check launch over the uploaded places whose word the host reads before the cache or the object is
 * touched -- nonzero: SSA_ERR_ARG, with object, cache and info unchanged.  A push is never applied in part.
 * _device forms fail closed as push_mixed_device does: a refused lane is held as failed, every finish that reaches it
 * is SSA_MALFORMED; reset the object after a refusal.  They are NOT enqueue-only: they synchronise the context's stream
 * once per cache slice, as push_cached_device does (and once more for stats_out, if given).
 * The existing push_mixed / push_known entry points, and an object that never sees these calls, enqueue exactly what
 * they did. */
int ssa_aggverifier_push_mixed_cached(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, ssa_keycache *kc,
                                      const uint32_t *places, size_t n, const uint8_t *rs49, const uint8_t *pks,
                                      const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                      size_t msg_len, size_t u, uint32_t require, uint64_t stats_out[8]);
int ssa_aggverifier_push_mixed_cached_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, ssa_keycache *kc,
                                             const uint32_t *d_places, size_t n, const uint8_t *d_rs49, const uint8_t *d_pks,
                                             const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                             size_t msg_stride, size_t msg_len, size_t u, uint32_t require,
                                             uint32_t *d_result_out, uint64_t stats_out[8]);
int ssa_aggverifier_push_mixed_cached_wire(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, ssa_keycache *kc,
                                           const uint32_t *places, size_t n, const uint8_t *rs49, const uint8_t *pks49,
                                           const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                           size_t u, uint32_t require, uint64_t stats_out[8]);
int ssa_aggverifier_push_mixed_cached_wire_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, ssa_keycache *kc,
                                                  const uint32_t *d_places, size_t n, const uint8_t *d_rs49,
                                                  const uint8_t *d_pks49, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                                  size_t msg_stride, size_t msg_len, size_t u, uint32_t require,
                                                  uint32_t *d_result_out, uint64_t stats_out[8]);

/* ---- ABI version -------------------------------------------------------------------------------------------
 * Bumped whenever an exported signature changes (round 2 inserted pk_inf into the batch entry points under the same
 * symbol names: a shim built against the older header would still link and pass msgs as pk_inf).  A binding checks
 * ssa_abi_version() == SSA_ABI_VERSION at load; the Python and C++ mirrors do. */
#define SSA_ABI_VERSION 5
int ssa_abi_version(void);

/* ---- arithmetic probes (unit parity with the oracle; not part of the reference API) --- */
/* op: 0 = Fp6 mul, 1 = Fp6 sqr, 2 = Fp6 inv, 3 = point add (affine 12+12 -> 12 felts + inf),
 *     4 = scalar mul [k]P (k in a[0..4], P in b), 5 = Fp mul (a[0]*b[0]), 6 = Fp inv,
 *     7 = the cooperative (one wave per point) operations: a = (x, y, inf, mode), b = (x, y, inf);
 *         mode 0 mixed addition, 1 general addition of two scaled Jacobian points, 2 doubling of a
 *     8..14 = products fused with linear terms, a = (u, v) 12 felts, b = (x, y) 12 felts -> 6 felts:
 *         8 u^2 - x - y, 9 u^2 + 3x, 10 u^2 - 4x, 11 u*v - 8x, 12 u*v - x, 13 u^2 - x - 2y, 14 u*v + x*y
 *     15..17 = the generated point operations of the ladder on RAW loose limbs (any 64-bit values, nothing is
 *         canonicalised on the way in or out): a = X, Y, Z (18 words), a[18] = act, a[19] = n; b = x2, y2 (12 words)
 *         -> X, Y, Z (18 words) + out[18] = flag.  15 one ladder window (n doublings, then the mixed addition where
 *         act != 0; flag 0 = the addition met a possible exceptional input and was left to the caller),
 *         16 mixed addition with its exact fallback, 17 n doublings
 *     18 = the Rescue S-boxes on raw loose values: a = (x, y) -> x^7, y^7, x^(1/7), y^(1/7) (canonical) and the flags of
 *         the two generated blocks (non-zero: the block reported its rare reduction borrow and the lane was recomputed) */
int ssa_debug_arith(ssa_ctx *ctx, int op, const uint64_t *a, const uint64_t *b, size_t n,
                    size_t a_stride, size_t b_stride, uint64_t *out, size_t out_stride);
/* error-path tests: the next pipelined host-buffer upload on this context fails with SSA_ERR_HIP after chunk `chunk`
 * has been enqueued (one shot; chunk < 0 disarms).  Replaces round 3's SSA_FAULT_AFTER_CHUNK environment variable: the
 * production path reads no environment per call. */
int ssa_debug_fault_after_chunk(ssa_ctx *ctx, int chunk);
/* call-order tests: fills every workspace and staging buffer of the context (and of its second set, once a call of more
 * than one slice has made it) with `byte` (0..255), up to each buffer's full capacity, and the page-locked host buffers
 * too; waits for the context's stream first and returns when the fill is done.  The constant-time signer's table is
 * left alone (it is state that persists between calls, not a workspace), and so is everything a context shares or
 * hands out: the comb for G, the parameters, key sets, key caches, signer sets.  Results of later calls must not change. */
int ssa_debug_poison_workspaces(ssa_ctx *ctx, int byte);
/* self-check tests.  which: 0 the comb for G, 1 the constant-time table (SSA_ERR_ARG before it is built).  Rows are 12
 * words (x[6], y[6]); rows and words outside the table are SSA_ERR_ARG, nothing is read or written out of bounds.
 *   ssa_debug_table_read  copies rows [first_row, first_row + n) to rows_out (n x 12 words)
 *   ssa_debug_table_xor   XORs `mask` into word `word` of row `row` ON THE DEVICE.  The comb is shared by every context of
 *                         the process on this device and geometry: this corrupts all of them.  Run no verification,
 *                         signing or derivation on any of them afterwards -- a poked header word (row 0, word 0)
 *                         misdirects the comb walk itself; ssa_ctx_selfcheck and ssa_ctx_destroy are what is left.
 *   ssa_debug_corrupt_table_builds  the next n comb builds of this process (any context, any width) get one fixed word
 *                         of a mid-table row flipped after the build and before its check (n = 0 disarms). */
int ssa_debug_table_read(ssa_ctx *ctx, int which, uint64_t first_row, uint64_t n, uint64_t *rows_out);
int ssa_debug_table_xor(ssa_ctx *ctx, int which, uint64_t row, uint32_t word, uint64_t mask);
int ssa_debug_corrupt_table_builds(int n);
/* key-table self-check tests: one key of a key set or of a key cache (exactly one of ks, kc non-NULL; key < m / keys
 * held).  what: 0 the ladder table (512 words), 1 the status byte, 2 the key bytes (12 words), 3 the pk_inf byte, 4 the
 * key's comb (key sets in comb mode: 12 words per row, word = 12 row + word of the row), 5 the 49 compressed bytes of a
 * row of a key cache in wire mode (7 words: the six of x, and one holding the flag byte).  Anything outside the object
 * is SSA_ERR_ARG, nothing is read or written out of bounds.
 *   ssa_debug_keytab_xor   XORs `mask` into word `word` ON THE DEVICE (a byte target: word 0, mask < 256).  Afterwards
 *                          only the self-check, its repair and the destroy call may run on the object.
 *   ssa_debug_keytab_read  copies the target to words_out: 512 words, 12 words, one word holding the byte, (what 4)
 *                          rows (0, 0) and (0, 1) of the comb, 24 words, or (what 5) 7 words. */
int ssa_debug_keytab_xor(ssa_keyset *ks, ssa_keycache *kc, int what, uint64_t key, uint32_t word, uint64_t mask);
int ssa_debug_keytab_read(ssa_keyset *ks, ssa_keycache *kc, int what, uint64_t key, uint64_t *words_out);
/* host logic of ssa_k_verify's end game, no context and no device needed: the launch plan for n lanes when `waves`
 * waves are resident (pieces / gens / uniform / min_main: what SSA_TAIL_PIECES, _GENS, _UNIFORM, _MIN_MAIN set).
 * out: number of pieces (0: no end game), 64-lane tail groups, ordinary workgroups, workgroups of the grid, the eight
 * piece descriptors (pass | first-of-pass << 1 | last-of-pass << 2 | first window << 8 | end window << 16) and the two
 * whole-pass descriptors ([q]P of the subgroup check, [h]P). */
int ssa_debug_tail_plan(unsigned waves, unsigned pieces, unsigned gens, int uniform, unsigned min_main, size_t n,
                        uint32_t flags, uint32_t out[14]);
/* One-slice calls of the lane kernels as two unequal parts on the context's two streams (SSA_SPLIT_FRAC, SSA_SPLIT_MIN;
 * DESIGN.md section 33).  ssa_debug_split_plan is the host logic, no context and no device needed: for a call of n lanes
 * with `flags`, the knobs as given (split_frac: the short part's share in 1/16ths, 0 = off; the two crossovers of the
 * cooperative kernel; twin: a second stream exists), out[0] = nA lanes stay on the caller's stream and out[1] = nB run
 * on the twin's: nA + nB = n, nA a multiple of 256, nB <= nA, nB = 0 when the call is not split.
 * ssa_debug_split_config sets the knobs on this context (negative: leave that one as it is; tail_b: part B runs with an
 * end game of its own; alone = 0: calls are split also while the process has other contexts on the device, which the
 * tests' processes always have).  ssa_debug_split_timing reads, and leaves in place, the last entry of timing key `kernel` that a
 * split call recorded: out[0] the span ssa_ctx_read_timing will count (earlier start to later end), out[1] and out[2]
 * the launches of part A and part B alone, in ms; SSA_ERR_ARG when there is none. */
int ssa_debug_split_plan(size_t n, uint32_t flags, size_t split_min, unsigned split_frac, size_t coop_max_n,
                         size_t coop_max_n_torsion, int twin, uint64_t out[2]);
int ssa_debug_split_config(ssa_ctx *ctx, int64_t split_min, int split_frac, int tail_b, int alone);
int ssa_debug_split_timing(ssa_ctx *ctx, const char *kernel, double out[3]);
/* host logic of the screened form, no context and no device needed: the plan for n signatures with coeff_bytes-wide
 * coefficients (0: library-drawn, 128-bit) at the default SSA_MSM_SLICE.  out: segments K of the first slice, lanes per
 * segment (a multiple of 256; only the last segment of a slice is ragged), window bits c, windows, windows that carry
 * R (the coefficient's), buckets per window (K * 2^(c-1)), slices, segments over all slices.  A context runs the exact
 * per-lane path instead for batches up to its small-batch bound. */
int ssa_debug_screen_plan(size_t n, uint32_t coeff_bytes, uint64_t out[8]);
/* tests: the screened form on this context uses k segments per slice (k in 1..256, fewer where the slice has fewer
 * 256-lane blocks; 0 = automatic).  The statuses do not depend on k. */
int ssa_debug_screen_segments(ssa_ctx *ctx, uint32_t k);
/* tests of the key dedup.  ssa_debug_dedup_device runs the dedup alone over ONE slice (1 <= n <= SSA_LANE_SLICE) of
 * device keys and optional flags: out[0] = u, out[1] = lanes that hit the probe bound; d_key_idx_out (optional, device,
 * n words) receives each lane's key index (< u; equal for two lanes only if their 97 bytes are equal).  Returns when it is
 * done.  ssa_debug_dedup_config sets the policy of ssa_verify_many_dedup on this context, for both flag settings: a
 * slice takes the keyed route when u < max_distinct_ratio * lanes (0 forces the fallback, anything above 1 the keyed
 * route; negative: the measured defaults), a lane probes at most probe_bound slots (0: the default, 128).  The statuses
 * depend on neither. */
int ssa_debug_dedup_device(ssa_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t n,
                           uint32_t *d_key_idx_out, uint64_t out[2]);
int ssa_debug_dedup_config(ssa_ctx *ctx, double max_distinct_ratio, uint32_t probe_bound);
/* host logic of the key cache, no context and no device needed: what a slice with u distinct keys, m of them not in the
 * cache, does to a cache of `capacity` rows holding `held`.  *plan_out: 0 insert the m misses, 1 clear the cache and
 * insert all u keys, 2 bypass the cache.  SSA_ERR_ARG for a capacity outside 1..2^24, held > capacity, m > u or
 * u > SSA_MAX_BATCH. */
int ssa_debug_keycache_plan(uint64_t capacity, uint64_t held, uint64_t u, uint64_t m, uint32_t *plan_out);
/* host logic of a compaction (SSA_KEYCACHE_EVICT_RECENT), no context and no device needed: hist[a] = rows of age a (a < 63),
 * hist[63] = older rows; out[0] = a*, out[1] = K as defined with ssa_keycache_set_eviction.  SSA_ERR_ARG for a capacity
 * outside 1..2^24, m > u, u > capacity, more rows in hist than capacity, or hist[0] above the budget (more rows of age 0
 * than the slice has hits: no a* exists). */
int ssa_debug_keycache_keep(uint64_t capacity, uint64_t u, uint64_t m, const uint64_t hist[64], uint64_t out[2]);
/* n_blocks 64-byte blocks of the ChaCha20 keystream the MSM coefficients come from (RFC 8439 known answers) */
int ssa_debug_chacha20(ssa_ctx *ctx, const uint8_t key[32], const uint8_t nonce[12], uint32_t counter0,
                       size_t n_blocks, uint8_t *out);
/* register-resident Fp-mul throughput probe: returns Fp multiplications per second (variants 0..2: fp_mul chains
 * with 1/4/8 independent streams, 3: the lazy Fp6 product + square, 4 / 5: squaring chains with the four- / three-
 * multiply square); variants 10..12: dependent
 * cooperative doublings / mixed additions / general additions per second (one wave) */
int ssa_bench_fpmul(ssa_ctx *ctx, int variant, double *fpmul_per_s);

#ifdef __cplusplus
}
#endif
#endif /* SCHNORR_SIG_AMD_H */
