// schnorr_sig.hpp -- C++17 host-side mirror of the reference's Rust API over the C ABI
// (include/schnorr_sig_amd.h).  Rust is not available in this image; this header keeps the
// reference's names, argument meaning and error behaviour so that a Rust `-sys` shim (see
// INTEGRATION.md) and these classes are interchangeable callers of the same entry points.
//
//   schnorr_sig::Signature::verify          <- src/signature.rs:181-205
//   schnorr_sig::KeyPair::{create, sign, sign_and_bind_pkey, verify_signature}
//                                           <- src/keypair.rs:57-65, src/signature.rs:114-165 (signing is CONSTANT-TIME,
//                                              SSA_FLAG_SIGN_CT, like the reference's `&BASEPOINT_TABLE * r`)
//   schnorr_sig::PublicKey::{to_bytes, from_bytes}          <- src/public.rs:49-56
//   schnorr_sig::KeyedSignature::{to_bytes, from_bytes, verify}  <- src/signature.rs:232-271
//   schnorr_sig::PublicKey::verify_signature <- src/signature.rs:170-176
//   schnorr_sig::verify_batch               <- src/batch.rs:31-50
//   schnorr_sig::SignatureError             <- src/error.rs:13-31
//   schnorr_sig::SignerSet::{sign, sign_and_bind_pkey}  <- KeyPair::sign / sign_and_bind_pkey over many messages by few
//                                              key pairs held on the device, src/signature.rs:114-156
//   schnorr_sig::{ChainCode, ExtendedPrivateKey, ExtendedPublicKey}, PrivateKey / PublicKey derivation
//                                           <- src/derivation.rs:30-317 (Context::xprv_derive_many & co. batched)
//
// All compute happens on the GPU behind ssa_*; nothing here does field or curve arithmetic.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <functional>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/schnorr_sig_amd.h"

namespace schnorr_sig {

constexpr size_t SCALAR_LENGTH = 32, BASEFIELD_LENGTH = 48, PUBLIC_KEY_LENGTH = 49, SIGNATURE_LENGTH = 81,
                 KEYED_SIGNATURE_LENGTH = 130, AFFINE_PUBLIC_KEY_LENGTH = 96, PRIVATE_KEY_LENGTH = SCALAR_LENGTH,
                 KEY_PAIR_LENGTH = PRIVATE_KEY_LENGTH;  // src/constants.rs:12-30

enum class SignatureError { InvalidPublicKey = 1, InvalidSignature = 2 };  // src/error.rs:13-18
inline const char *to_string(SignatureError e) {                           // src/error.rs:20-31
    return e == SignatureError::InvalidPublicKey ? "The public key is not an element of the prime subgroup."
                                                 : "The signature is invalid or was incorrectly computed.";
}
// Result<(), SignatureError>: empty optional == Ok(())
using Result = std::optional<SignatureError>;

// Inputs the reference panics on (src/signature.rs:186, src/batch.rs:37-44,67,104)
struct Panic : std::runtime_error {
    using std::runtime_error::runtime_error;
};

using Rng = std::function<void(uint8_t *, size_t)>;  // fills a buffer with random bytes
// the `rng` that has the GPU draw the nonces (and the keys of SignerSet::generate) itself: no nonce exists on the host
// (ssa_*_rng)
struct DeviceRng {};
inline constexpr DeviceRng device_rng{};

// ssa_ctx_selfcheck's out[8] by name; ok == false is a failing table (SSA_ERR_TABLE), not an exception
struct SelfCheck {
    uint64_t rows, bad, first_bad, ctab_rows, ctab_bad, ctab_first_bad, builds, bits;
    bool ok;
};

// ssa_keyset_selfcheck's / ssa_keycache_selfcheck's out[8] by name; ok == false means keys fail (SSA_ERR_TABLE), not an
// exception.  bad: one byte per key of a key set, 1 for a failing key (empty for a key cache).
struct KeyCheck {
    uint64_t keys_checked, keys_bad, first_bad_key, ladder_entries_checked, comb_rows_checked, keys_rebuilt_and_compared,
        combs_skipped, rows_repaired;
    bool ok;
    std::vector<uint8_t> bad;
};
inline KeyCheck keycheck_result(int rc, const uint64_t o[8], const char *what, std::vector<uint8_t> bad = {}) {
    if (rc != SSA_OK && rc != SSA_ERR_TABLE) throw std::runtime_error(std::string(what) + ": " + ssa_strerror(rc));
    return KeyCheck{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], rc == SSA_OK, std::move(bad)};
}

class Context {
  public:
    // gtab_bits / hbm_budget_bytes: the comb for G (the reference's const BASEPOINT_TABLE) as a speed-for-memory choice of
    // the context -- 0 / 0 = the widest table that fits a tenth of the free device memory (ssa_ctx_create_ex)
    explicit Context(int device = 0, const void *params = nullptr, size_t params_len = 0, uint32_t gtab_bits = 0,
                     uint64_t hbm_budget_bytes = 0) {
        // a library from another revision of the header links just as well and reads its arguments shifted
        if (ssa_abi_version() != SSA_ABI_VERSION)
            throw std::runtime_error("schnorr_sig_amd: library ABI version " + std::to_string(ssa_abi_version()) +
                                     ", header " + std::to_string(SSA_ABI_VERSION));
        int rc = ssa_ctx_create_ex(&ctx_, device, params, params_len, gtab_bits, hbm_budget_bytes);
        if (rc != 0) throw std::runtime_error(std::string("ssa_ctx_create: ") + ssa_strerror(rc));
    }
    ~Context() { ssa_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    ssa_ctx *get() const { return ctx_; }
    // the exact check of the comb for G and (once built) the constant-time table; a comb that fails is retired: destroy
    // this context and create a new one
    SelfCheck selfcheck() {
        uint64_t o[8] = {};
        const int rc = ssa_ctx_selfcheck(ctx_, 0, o);
        if (rc != SSA_OK && rc != SSA_ERR_TABLE) throw std::runtime_error(std::string("ssa_ctx_selfcheck: ") + ssa_strerror(rc));
        return SelfCheck{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], rc == SSA_OK};
    }

  private:
    ssa_ctx *ctx_ = nullptr;
};

inline Result status_to_result(int st) {
    if (st == SSA_OK) return std::nullopt;
    if (st == SSA_INVALID_PUBLIC_KEY) return SignatureError::InvalidPublicKey;
    if (st == SSA_INVALID_SIGNATURE) return SignatureError::InvalidSignature;
    if (st == SSA_MALFORMED) throw Panic("undecodable field element or scalar (the reference panics)");
    throw std::runtime_error(std::string("schnorr_sig_amd: ") + ssa_strerror(st));
}

struct Signature;
struct KeyedSignature;
struct PublicKey;

// a little-endian integer of 64 bytes reduced mod q (Scalar::from_bytes_wide): binary long division, host glue
inline void reduce_wide_mod_q(const uint8_t wide[64], uint64_t r[4]) {
    static const uint64_t Q[4] = {0xd443623eaed4accfULL, 0x327aa72330157722ULL, 0x563fbf0f990a37b5ULL, 0x7af2599b3b3f22d0ULL};
    r[0] = r[1] = r[2] = r[3] = 0;
    for (int bit = 511; bit >= 0; bit--) {
        const uint64_t top = r[3] >> 63;
        r[3] = (r[3] << 1) | (r[2] >> 63);
        r[2] = (r[2] << 1) | (r[1] >> 63);
        r[1] = (r[1] << 1) | (r[0] >> 63);
        r[0] = (r[0] << 1) | ((wide[bit >> 3] >> (bit & 7)) & 1u);
        bool ge = top != 0;
        if (!ge) {
            ge = true;
            for (int i = 3; i >= 0; i--) {
                if (r[i] != Q[i]) {
                    ge = r[i] > Q[i];
                    break;
                }
            }
        }
        if (ge) {
            unsigned __int128 borrow = 0;
            for (int i = 0; i < 4; i++) {
                const unsigned __int128 d = (unsigned __int128)r[i] - Q[i] - borrow;
                r[i] = (uint64_t)d;
                borrow = (d >> 64) & 1;
            }
        }
    }
}

struct PrivateKey {  // src/private.rs:25
    std::array<uint8_t, SCALAR_LENGTH> bytes{};
    bool operator==(const PrivateKey &o) const { return bytes == o.bytes; }
    std::array<uint8_t, PRIVATE_KEY_LENGTH> to_bytes() const { return bytes; }  // src/private.rs:69-71
    // PrivateKey::from_bytes, src/private.rs:74-76: nullopt for a non-canonical or zero scalar
    static std::optional<PrivateKey> from_bytes(const std::array<uint8_t, PRIVATE_KEY_LENGTH> &b) {
        static const uint64_t Q[4] = {0xd443623eaed4accfULL, 0x327aa72330157722ULL, 0x563fbf0f990a37b5ULL, 0x7af2599b3b3f22d0ULL};
        uint64_t w[4] = {0, 0, 0, 0};
        for (int i = 0; i < 32; i++) w[i / 8] |= (uint64_t)b[i] << (8 * (i % 8));
        if ((w[0] | w[1] | w[2] | w[3]) == 0) return std::nullopt;
        for (int i = 3; i >= 0; i--) {
            if (w[i] != Q[i]) {
                if (w[i] > Q[i]) return std::nullopt;
                PrivateKey k;
                k.bytes = b;
                return k;
            }
        }
        return std::nullopt;   // == q
    }
    // PrivateKey::from_seed, src/private.rs:79-82
    static std::optional<PrivateKey> from_seed(const std::array<uint8_t, 64> &seed) {
        uint64_t r[4];
        reduce_wide_mod_q(seed.data(), r);
        if ((r[0] | r[1] | r[2] | r[3]) == 0) return std::nullopt;
        PrivateKey k;
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 8; j++) k.bytes[8 * i + j] = (uint8_t)(r[i] >> (8 * j));
        return k;
    }
    // PrivateKey::sign / sign_and_bind_pkey, src/signature.rs:62-110 ("it is faster to sign with a KeyPair": the public key
    // is recomputed first, PublicKey::from(self)) -- defined after KeyPair
    Signature sign(Context &cx, const uint8_t *msg, size_t len, Rng rng) const;
    KeyedSignature sign_and_bind_pkey(Context &cx, const uint8_t *msg, size_t len, Rng rng) const;
    Signature sign(Context &cx, const uint8_t *msg, size_t len, DeviceRng) const;
    KeyedSignature sign_and_bind_pkey(Context &cx, const uint8_t *msg, size_t len, DeviceRng) const;
};

struct PublicKey {  // src/public.rs:24 -- the in-memory AffinePoint (x, y), canonical LE limbs
    std::array<uint8_t, AFFINE_PUBLIC_KEY_LENGTH> affine{};
    bool is_identity = false;  // AffinePoint::identity() is a valid PublicKey (src/public.rs:95-101)
    bool operator==(const PublicKey &o) const { return affine == o.affine && is_identity == o.is_identity; }
    static PublicKey from_private(Context &cx, const PrivateKey &sk);   // impl From<&PrivateKey>, src/public.rs:26-32
    Result verify_signature(Context &cx, const Signature &sig, const uint8_t *msg, size_t len) const;
    // PublicKey::to_bytes, src/public.rs:49-51: the 49-byte compressed wire form
    std::array<uint8_t, PUBLIC_KEY_LENGTH> to_bytes(Context &cx) const {
        std::array<uint8_t, PUBLIC_KEY_LENGTH> out{};
        const uint8_t inf = is_identity ? 1 : 0;
        uint8_t st = SSA_MALFORMED;
        const int rc = ssa_compress_many(cx.get(), affine.data(), &inf, 1, out.data(), &st);
        if (rc != 0) throw std::runtime_error(std::string("ssa_compress_many: ") + ssa_strerror(rc));
        if (st != SSA_OK) throw Panic("PublicKey holds a non-canonical limb");
        return out;
    }
    // PublicKey::from_bytes, src/public.rs:54-56: nullopt when decompression fails (CtOption is_none)
    static std::optional<PublicKey> from_bytes(Context &cx, const std::array<uint8_t, PUBLIC_KEY_LENGTH> &b) {
        PublicKey pk;
        uint8_t inf = 0, st = 1;
        const int rc = ssa_decompress_many(cx.get(), b.data(), 1, pk.affine.data(), &inf, &st);
        if (rc != 0) throw std::runtime_error(std::string("ssa_decompress_many: ") + ssa_strerror(rc));
        if (st != 0) return std::nullopt;
        pk.is_identity = inf != 0;
        return pk;
    }
};

struct Signature {  // src/signature.rs:34-40, wire layout :208-214
    std::array<uint8_t, SIGNATURE_LENGTH> bytes{};
    // Signature::verify, src/signature.rs:181-205
    Result verify(Context &cx, const uint8_t *msg, size_t len, const PublicKey &pk) const {
        uint8_t st = SSA_MALFORMED;
        const uint8_t inf = pk.is_identity ? 1 : 0, dummy = 0;
        const int rc = ssa_verify_many(cx.get(), bytes.data(), pk.affine.data(), &inf, len ? msg : &dummy, nullptr, len,
                                       len, 1, SSA_FLAG_CHECK_TORSION, &st, nullptr);
        return status_to_result(rc != 0 ? rc : (int)st);
    }
    std::array<uint8_t, SIGNATURE_LENGTH> to_bytes() const { return bytes; }
};

inline Result PublicKey::verify_signature(Context &cx, const Signature &sig, const uint8_t *msg, size_t len) const {
    return sig.verify(cx, msg, len, *this);
}

struct KeyedSignature {  // src/signature.rs:55-60; wire form pk(49) || sig(81), :236-271
    PublicKey public_key;
    Signature signature;
    Result verify(Context &cx, const uint8_t *msg, size_t len) const { return signature.verify(cx, msg, len, public_key); }
    std::array<uint8_t, KEYED_SIGNATURE_LENGTH> to_bytes(Context &cx) const {
        std::array<uint8_t, KEYED_SIGNATURE_LENGTH> out{};
        const auto pk = public_key.to_bytes(cx);
        std::memcpy(out.data(), pk.data(), PUBLIC_KEY_LENGTH);
        std::memcpy(out.data() + PUBLIC_KEY_LENGTH, signature.bytes.data(), SIGNATURE_LENGTH);
        return out;
    }
    // nullopt unless both halves decode (the scalar e must be canonical: Signature::from_bytes, src/signature.rs:217-227)
    static std::optional<KeyedSignature> from_bytes(Context &cx, const std::array<uint8_t, KEYED_SIGNATURE_LENGTH> &b) {
        std::array<uint8_t, PUBLIC_KEY_LENGTH> pkb;
        std::memcpy(pkb.data(), b.data(), PUBLIC_KEY_LENGTH);
        const auto pk = PublicKey::from_bytes(cx, pkb);
        static const uint8_t q_le[32] = {0xcf, 0xac, 0xd4, 0xae, 0x3e, 0x62, 0x43, 0xd4, 0x22, 0x77, 0x15,
                                         0x30, 0x23, 0xa7, 0x7a, 0x32, 0xb5, 0x37, 0x0a, 0x99, 0x0f, 0xbf,
                                         0x3f, 0x56, 0xd0, 0x22, 0x3f, 0x3b, 0x9b, 0x59, 0xf2, 0x7a};
        int cmp = 0;
        for (int k = 31; k >= 0 && cmp == 0; k--)
            if (b[PUBLIC_KEY_LENGTH + 49 + k] != q_le[k]) cmp = b[PUBLIC_KEY_LENGTH + 49 + k] < q_le[k] ? -1 : 1;
        if (!pk || cmp >= 0) return std::nullopt;
        KeyedSignature ks;
        ks.public_key = *pk;
        std::memcpy(ks.signature.bytes.data(), b.data() + PUBLIC_KEY_LENGTH, SIGNATURE_LENGTH);
        return ks;
    }
};

struct KeyPair {  // src/keypair.rs:48-53
    PrivateKey private_key;
    PublicKey public_key;

    // Scalar::random(rng): 64 random bytes reduced mod q (statistical distance from uniform < 2^-256), never 0.
    // (A 32-byte draw reduced mod q, or a masked 254-bit draw, is biased -- fatal for nonces: hidden-number problem.)
    static void random_scalar(Rng &rng, uint8_t out[32]) {
        for (;;) {
            uint8_t wide[64];
            rng(wide, sizeof wide);
            uint64_t r[4];
            reduce_wide_mod_q(wide, r);
            if ((r[0] | r[1] | r[2] | r[3]) == 0) continue;   // PrivateKey::new rejects 0 (src/private.rs:49-57)
            for (int i = 0; i < 4; i++)
                for (int k = 0; k < 8; k++) out[8 * i + k] = (uint8_t)(r[i] >> (8 * k));
            return;
        }
    }
    bool operator==(const KeyPair &o) const { return private_key == o.private_key && public_key == o.public_key; }
    // impl From<&PrivateKey> for KeyPair, src/keypair.rs:21-32: the public key is [sk]G -- one constant-time base
    // multiplication (ssa_pubkey_many) and nothing else derived from the secret
    static KeyPair from_private(Context &cx, const PrivateKey &sk) {
        KeyPair kp;
        kp.private_key = sk;
        int rc = ssa_pubkey_many(cx.get(), sk.bytes.data(), 1, kp.public_key.affine.data());
        if (rc != 0) throw std::runtime_error(std::string("ssa_pubkey_many: ") + ssa_strerror(rc));
        return kp;
    }
    // KeyPair::to_bytes / from_bytes / from_seed, src/keypair.rs:73-103: the private key only, the public key is rebuilt
    std::array<uint8_t, KEY_PAIR_LENGTH> to_bytes() const { return private_key.to_bytes(); }
    static std::optional<KeyPair> from_bytes(Context &cx, const std::array<uint8_t, KEY_PAIR_LENGTH> &b) {
        const auto sk = PrivateKey::from_bytes(b);
        if (!sk) return std::nullopt;
        return from_private(cx, *sk);
    }
    static std::optional<KeyPair> from_seed(Context &cx, const std::array<uint8_t, 64> &seed) {
        const auto sk = PrivateKey::from_seed(seed);
        if (!sk) return std::nullopt;
        return from_private(cx, *sk);
    }
    // KeyPair::new, src/keypair.rs:57-65
    static KeyPair create(Context &cx, Rng rng) {
        PrivateKey sk;
        random_scalar(rng, sk.bytes.data());
        return from_private(cx, sk);
    }
    // KeyPair::sign, src/signature.rs:114-129 (constant-time in the key and the nonce, like the reference)
    Signature sign(Context &cx, const uint8_t *msg, size_t len, Rng rng) const {
        uint8_t nonce[32], pk[AFFINE_PUBLIC_KEY_LENGTH];
        random_scalar(rng, nonce);
        Signature s;
        uint8_t dummy = 0;
        int rc = ssa_keygen_sign_many_ex(cx.get(), private_key.bytes.data(), nonce, len ? msg : &dummy, nullptr, len,
                                         len, 1, SSA_FLAG_SIGN_CT, pk, s.bytes.data());
        if (rc != 0) throw std::runtime_error(std::string("ssa_keygen_sign_many_ex: ") + ssa_strerror(rc));
        return s;
    }
    // KeyPair::sign_and_bind_pkey, src/signature.rs:132-156: the engine emits the 130-byte record itself
    // (SSA_FLAG_SIGN_KEYED); the public key inside it is this pair's
    KeyedSignature sign_and_bind_pkey(Context &cx, const uint8_t *msg, size_t len, Rng rng) const {
        uint8_t nonce[32], rec[KEYED_SIGNATURE_LENGTH], dummy = 0;
        random_scalar(rng, nonce);
        int rc = ssa_keygen_sign_many_ex(cx.get(), private_key.bytes.data(), nonce, len ? msg : &dummy, nullptr, len,
                                         len, 1, SSA_FLAG_SIGN_CT | SSA_FLAG_SIGN_KEYED, nullptr, rec);
        if (rc != 0) throw std::runtime_error(std::string("ssa_keygen_sign_many_ex: ") + ssa_strerror(rc));
        KeyedSignature ks;
        ks.public_key = public_key;
        std::memcpy(ks.signature.bytes.data(), rec + PUBLIC_KEY_LENGTH, SIGNATURE_LENGTH);
        return ks;
    }
    // the same two with the nonce drawn on the device (ssa_keygen_sign_many_rng)
    Signature sign(Context &cx, const uint8_t *msg, size_t len, DeviceRng) const {
        uint8_t pk[AFFINE_PUBLIC_KEY_LENGTH], dummy = 0;
        Signature s;
        int rc = ssa_keygen_sign_many_rng(cx.get(), private_key.bytes.data(), len ? msg : &dummy, nullptr, len, len, 1,
                                          SSA_FLAG_SIGN_CT, pk, s.bytes.data());
        if (rc != 0) throw std::runtime_error(std::string("ssa_keygen_sign_many_rng: ") + ssa_strerror(rc));
        return s;
    }
    KeyedSignature sign_and_bind_pkey(Context &cx, const uint8_t *msg, size_t len, DeviceRng) const {
        uint8_t rec[KEYED_SIGNATURE_LENGTH], dummy = 0;
        int rc = ssa_keygen_sign_many_rng(cx.get(), private_key.bytes.data(), len ? msg : &dummy, nullptr, len, len, 1,
                                          SSA_FLAG_SIGN_CT | SSA_FLAG_SIGN_KEYED, nullptr, rec);
        if (rc != 0) throw std::runtime_error(std::string("ssa_keygen_sign_many_rng: ") + ssa_strerror(rc));
        KeyedSignature ks;
        ks.public_key = public_key;
        std::memcpy(ks.signature.bytes.data(), rec + PUBLIC_KEY_LENGTH, SIGNATURE_LENGTH);
        return ks;
    }
    Result verify_signature(Context &cx, const Signature &sig, const uint8_t *msg, size_t len) const {
        return sig.verify(cx, msg, len, public_key);  // src/signature.rs:159-165
    }
};

inline PublicKey PublicKey::from_private(Context &cx, const PrivateKey &sk) { return KeyPair::from_private(cx, sk).public_key; }
inline Signature PrivateKey::sign(Context &cx, const uint8_t *msg, size_t len, Rng rng) const {
    return KeyPair::from_private(cx, *this).sign(cx, msg, len, rng);
}
inline KeyedSignature PrivateKey::sign_and_bind_pkey(Context &cx, const uint8_t *msg, size_t len, Rng rng) const {
    return KeyPair::from_private(cx, *this).sign_and_bind_pkey(cx, msg, len, rng);
}
inline Signature PrivateKey::sign(Context &cx, const uint8_t *msg, size_t len, DeviceRng r) const {
    return KeyPair::from_private(cx, *this).sign(cx, msg, len, r);
}
inline KeyedSignature PrivateKey::sign_and_bind_pkey(Context &cx, const uint8_t *msg, size_t len, DeviceRng r) const {
    return KeyPair::from_private(cx, *this).sign_and_bind_pkey(cx, msg, len, r);
}

// Many signatures by few signers (validator sets; the reference's own batch test reuses keys, src/batch.rs:152-175):
// the key checks of Signature::verify -- canonical limbs, on the curve, subgroup check (src/signature.rs:182-184) --
// and the tables the verification needs are computed once per key (ssa_keyset_create); verify() then checks
// signature i against key key_idx[i] with Signature::verify's semantics.
class KeySet {
  public:
    KeySet(Context &cx, const std::vector<PublicKey> &keys, uint32_t kind = SSA_KEYSET_AUTO) : cx_(cx), m_(keys.size()) {
        std::vector<uint8_t> pks(m_ * AFFINE_PUBLIC_KEY_LENGTH), inf(m_);
        for (size_t i = 0; i < m_; i++) {
            std::memcpy(&pks[i * AFFINE_PUBLIC_KEY_LENGTH], keys[i].affine.data(), AFFINE_PUBLIC_KEY_LENGTH);
            inf[i] = keys[i].is_identity ? 1 : 0;
        }
        int rc = ssa_keyset_create(cx.get(), pks.data(), inf.data(), m_, kind, &ks_);
        if (rc != 0) throw std::runtime_error(std::string("ssa_keyset_create: ") + ssa_strerror(rc));
    }
    ~KeySet() { ssa_keyset_destroy(ks_); }
    KeySet(const KeySet &) = delete;
    KeySet &operator=(const KeySet &) = delete;
    size_t size() const { return m_; }
    // the exact check of every key's table, status and (comb mode) comb against the stored key bytes; deep: also [q]P
    // per key (without it a status flipped between 0 and 1 is not seen).  Keys with bad[i] == 1 go into a new key set.
    KeyCheck selfcheck(bool deep = false) {
        uint64_t o[8] = {};
        std::vector<uint8_t> bad(m_, 0);
        const int rc = ssa_keyset_selfcheck(ks_, deep ? SSA_KEYCHECK_DEEP : 0u, bad.data(), o);
        return keycheck_result(rc, o, "ssa_keyset_selfcheck", std::move(bad));
    }
    // one Result per signature (a Panic for inputs the reference would panic on)
    std::vector<Result> verify(const std::vector<Signature> &signatures, const std::vector<uint32_t> &key_idx,
                               const std::vector<std::pair<const uint8_t *, size_t>> &messages) const {
        const size_t n = signatures.size();
        if (key_idx.size() != n || messages.size() != n) throw Panic("one key index and one message per signature");
        std::vector<Result> out(n);
        if (n == 0) return out;
        std::vector<uint8_t> sigs(n * SIGNATURE_LENGTH), flat, status(n);
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(&sigs[i * SIGNATURE_LENGTH], signatures[i].bytes.data(), SIGNATURE_LENGTH);
            flat.insert(flat.end(), messages[i].first, messages[i].first + messages[i].second);
            off[i + 1] = flat.size();
        }
        flat.push_back(0);
        int rc = ssa_verify_many_indexed(cx_.get(), ks_, key_idx.data(), sigs.data(), flat.data(), off.data(), 0, 0, n,
                                         SSA_FLAG_CHECK_TORSION, status.data(), nullptr);
        if (rc != 0) throw std::runtime_error(std::string("ssa_verify_many_indexed: ") + ssa_strerror(rc));
        for (size_t i = 0; i < n; i++) out[i] = status_to_result(status[i]);
        return out;
    }

  private:
    Context &cx_;
    size_t m_;
    ssa_keyset *ks_ = nullptr;
};

// Many signatures by few key pairs (a service's keys, derived deposit addresses): the key pairs stay on the device
// (ssa_signer_set_create) and sign() is KeyPair::sign (src/signature.rs:114-129) -- constant-time, one base
// multiplication per signature -- of message i by key pair key_idx[i]; sign_and_bind_pkey() gives the KeyedSignature
// records (:132-156).  The destructor zeroes the secret keys on the device.  SignerSet(cx, m, device_rng) is
// KeyPair::new(rng) for m key pairs drawn on the device (ssa_signer_set_generate); secret_keys() exports them.
class SignerSet {
  public:
    SignerSet(Context &cx, const std::vector<KeyPair> &pairs) : cx_(cx), m_(pairs.size()) {
        std::vector<uint8_t> sks(pairs.size() * PRIVATE_KEY_LENGTH);
        for (size_t i = 0; i < pairs.size(); i++) {
            std::memcpy(&sks[i * PRIVATE_KEY_LENGTH], pairs[i].private_key.bytes.data(), PRIVATE_KEY_LENGTH);
            pks_.push_back(pairs[i].public_key);
        }
        int rc = ssa_signer_set_create(cx.get(), sks.data(), pairs.size(), &ss_);
        std::fill(sks.begin(), sks.end(), 0);
        if (rc != 0) throw std::runtime_error(std::string("ssa_signer_set_create: ") + ssa_strerror(rc));
    }
    SignerSet(Context &cx, size_t m, DeviceRng) : cx_(cx), m_(m) {
        int rc = ssa_signer_set_generate(cx.get(), m, &ss_);
        if (rc != 0) throw std::runtime_error(std::string("ssa_signer_set_generate: ") + ssa_strerror(rc));
        pks_ = public_keys();
    }
    ~SignerSet() { ssa_signer_set_destroy(ss_); }
    SignerSet(const SignerSet &) = delete;
    SignerSet &operator=(const SignerSet &) = delete;
    size_t size() const { return m_; }
    // KeyPair::to_bytes of every key pair (src/keypair.rs:73-75): the one call that brings the keys to the host
    std::vector<std::array<uint8_t, KEY_PAIR_LENGTH>> secret_keys() const {
        std::vector<std::array<uint8_t, KEY_PAIR_LENGTH>> out(size());
        int rc = ssa_signer_set_secret_keys(ss_, size() ? out[0].data() : nullptr);
        if (rc != 0) throw std::runtime_error(std::string("ssa_signer_set_secret_keys: ") + ssa_strerror(rc));
        return out;
    }
    // the public keys as the set computed them: 96-byte affine and 49-byte compressed
    std::vector<PublicKey> public_keys() const {
        std::vector<uint8_t> pks(size() * AFFINE_PUBLIC_KEY_LENGTH);
        int rc = ssa_signer_set_public_keys(ss_, pks.data(), nullptr);
        if (rc != 0) throw std::runtime_error(std::string("ssa_signer_set_public_keys: ") + ssa_strerror(rc));
        std::vector<PublicKey> out(size());
        for (size_t i = 0; i < size(); i++) std::memcpy(out[i].affine.data(), &pks[i * AFFINE_PUBLIC_KEY_LENGTH], AFFINE_PUBLIC_KEY_LENGTH);
        return out;
    }
    std::vector<Signature> sign(const std::vector<uint32_t> &key_idx,
                                const std::vector<std::pair<const uint8_t *, size_t>> &messages, Rng rng) const {
        return sigs(run(key_idx, messages, &rng, SSA_FLAG_SIGN_CT, SIGNATURE_LENGTH));
    }
    std::vector<KeyedSignature> sign_and_bind_pkey(const std::vector<uint32_t> &key_idx,
                                                   const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                   Rng rng) const {
        return keyed(key_idx, run(key_idx, messages, &rng, SSA_FLAG_SIGN_CT | SSA_FLAG_SIGN_KEYED, KEYED_SIGNATURE_LENGTH));
    }
    // the same two with the nonces drawn on the device (ssa_sign_many_indexed_rng)
    std::vector<Signature> sign(const std::vector<uint32_t> &key_idx,
                                const std::vector<std::pair<const uint8_t *, size_t>> &messages, DeviceRng) const {
        return sigs(run(key_idx, messages, nullptr, SSA_FLAG_SIGN_CT, SIGNATURE_LENGTH));
    }
    std::vector<KeyedSignature> sign_and_bind_pkey(const std::vector<uint32_t> &key_idx,
                                                   const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                   DeviceRng) const {
        return keyed(key_idx, run(key_idx, messages, nullptr, SSA_FLAG_SIGN_CT | SSA_FLAG_SIGN_KEYED, KEYED_SIGNATURE_LENGTH));
    }

  private:
    static std::vector<Signature> sigs(const std::vector<uint8_t> &recs) {
        std::vector<Signature> out(recs.size() / SIGNATURE_LENGTH);
        for (size_t i = 0; i < out.size(); i++)
            std::memcpy(out[i].bytes.data(), &recs[i * SIGNATURE_LENGTH], SIGNATURE_LENGTH);
        return out;
    }
    std::vector<KeyedSignature> keyed(const std::vector<uint32_t> &key_idx, const std::vector<uint8_t> &recs) const {
        std::vector<KeyedSignature> out(key_idx.size());
        for (size_t i = 0; i < out.size(); i++) {
            out[i].public_key = pks_[key_idx[i]];
            std::memcpy(out[i].signature.bytes.data(), &recs[i * KEYED_SIGNATURE_LENGTH + PUBLIC_KEY_LENGTH],
                        SIGNATURE_LENGTH);
        }
        return out;
    }
    // rng == nullptr: the nonces are drawn on the device
    std::vector<uint8_t> run(const std::vector<uint32_t> &key_idx,
                             const std::vector<std::pair<const uint8_t *, size_t>> &messages, Rng *rng, uint32_t flags,
                             size_t rec_len) const {
        const size_t n = key_idx.size();
        if (messages.size() != n) throw Panic("one key index per message");
        for (uint32_t k : key_idx)
            if (k >= size()) throw Panic("key index out of range");
        std::vector<uint8_t> nonces(rng ? n * SCALAR_LENGTH : 0), flat, recs(n * rec_len);
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) {
            if (rng) KeyPair::random_scalar(*rng, &nonces[i * SCALAR_LENGTH]);
            flat.insert(flat.end(), messages[i].first, messages[i].first + messages[i].second);
            off[i + 1] = flat.size();
        }
        flat.push_back(0);
        if (!rng) {
            int rc = ssa_sign_many_indexed_rng(cx_.get(), ss_, key_idx.data(), flat.data(), off.data(), 0, 0, n, flags,
                                               recs.data());
            if (rc != 0) throw std::runtime_error(std::string("ssa_sign_many_indexed_rng: ") + ssa_strerror(rc));
            return recs;
        }
        int rc = ssa_sign_many_indexed(cx_.get(), ss_, key_idx.data(), nonces.data(), flat.data(), off.data(), 0, 0, n,
                                       flags, recs.data());
        std::fill(nonces.begin(), nonces.end(), 0);
        if (rc != 0) throw std::runtime_error(std::string("ssa_sign_many_indexed: ") + ssa_strerror(rc));
        return recs;
    }
    Context &cx_;
    size_t m_;
    std::vector<PublicKey> pks_;
    ssa_signer_set *ss_ = nullptr;
};

// (signature, public key, message) triples as the batch entry points take them: 81-byte signatures, 96-byte affine keys,
// identity flags, the messages back to back with their n + 1 offsets.  The length checks of the reference's verify_batch.
struct PackedTriples {
    std::vector<uint8_t> sigs, pks, inf, flat;
    std::vector<uint64_t> off;
};
inline PackedTriples pack_triples(const std::vector<Signature> &signatures, const std::vector<PublicKey> &public_keys,
                                  const std::vector<std::pair<const uint8_t *, size_t>> &messages) {
    if (signatures.size() != public_keys.size())
        throw Panic("We should have the same number of signatures than public keys");
    if (messages.size() != public_keys.size())
        throw Panic("We should have the same number of messages than public keys");
    const size_t n = signatures.size();
    PackedTriples t;
    t.sigs.resize(n * SIGNATURE_LENGTH);
    t.pks.resize(n * AFFINE_PUBLIC_KEY_LENGTH);
    t.inf.resize(n);
    t.off.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        std::memcpy(&t.sigs[i * SIGNATURE_LENGTH], signatures[i].bytes.data(), SIGNATURE_LENGTH);
        std::memcpy(&t.pks[i * AFFINE_PUBLIC_KEY_LENGTH], public_keys[i].affine.data(), AFFINE_PUBLIC_KEY_LENGTH);
        t.inf[i] = public_keys[i].is_identity ? 1 : 0;
        t.flat.insert(t.flat.end(), messages[i].first, messages[i].first + messages[i].second);
        t.off[i + 1] = t.flat.size();
    }
    t.flat.push_back(0);
    return t;
}

// The tail the *_statuses functions share: one status byte per triple (none for an empty slice), Scalar::random(rng)
// coefficients when there is an rng, call(statuses, coefficients or nullptr), and an ABI error thrown under `what`.
template <class F>
inline std::vector<uint8_t> statuses_of(size_t n, Rng rng, const char *what, F &&call) {
    std::vector<uint8_t> status(n, 0), coeffs;
    if (n == 0) return status;
    if (rng) {
        coeffs.resize(n * SCALAR_LENGTH);
        for (size_t i = 0; i < n; i++) KeyPair::random_scalar(rng, &coeffs[i * SCALAR_LENGTH]);
    }
    const int rc = call(status.data(), rng ? coeffs.data() : nullptr);
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + ssa_strerror(rc));
    return status;
}

// verify_batch, src/batch.rs:31-50.
//   msm = false: AND of exact per-signature checks (`rng` unused; DESIGN.md lists the divergence classes)
//   msm = true : the reference's own algorithm on the GPU (random linear combination + 2n-point MSM), the
//                coefficients are Scalar::random(rng) per signature (src/batch.rs:75-78); rng == nullptr lets the
//                library draw them (ChaCha20 keyed with getrandom(2))
inline Result verify_batch(Context &cx, const std::vector<Signature> &signatures,
                           const std::vector<PublicKey> &public_keys,
                           const std::vector<std::pair<const uint8_t *, size_t>> &messages, Rng rng = nullptr,
                           bool msm = false) {
    const PackedTriples t = pack_triples(signatures, public_keys, messages);     // (its length checks: src/batch.rs:37-44)
    const size_t n = signatures.size();
    if (n == 0) return std::nullopt;
    if (msm) {
        std::vector<uint8_t> coeffs;
        if (rng) {
            coeffs.resize(n * SCALAR_LENGTH);
            for (size_t i = 0; i < n; i++) KeyPair::random_scalar(rng, &coeffs[i * SCALAR_LENGTH]);
        }
        return status_to_result(ssa_verify_batch_msm(cx.get(), t.sigs.data(), t.pks.data(), t.inf.data(), t.flat.data(),
                                                     t.off.data(), 0, 0, n, rng ? coeffs.data() : nullptr));
    }
    return status_to_result(
        ssa_verify_batch(cx.get(), t.sigs.data(), t.pks.data(), t.inf.data(), t.flat.data(), t.off.data(), 0, 0, n, 0));
}

// verify_batch semantics per signature, screened on the GPU: statuses 0 (Ok), 2 (invalid
// signature) or 3 (malformed: the reference would panic), with the same coefficients as verify_batch(msm = true).  A
// rejected lane is reported except with the probability the header states (random combination of its segment vanishes).
inline std::vector<uint8_t> verify_batch_statuses(Context &cx, const std::vector<Signature> &signatures,
                                                  const std::vector<PublicKey> &public_keys,
                                                  const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                  Rng rng = nullptr) {
    const PackedTriples t = pack_triples(signatures, public_keys, messages);
    const size_t n = signatures.size();
    return statuses_of(n, rng, "ssa_verify_batch_screened", [&](uint8_t *status, const uint8_t *coeffs) {
        return ssa_verify_batch_screened(cx.get(), t.sigs.data(), t.pks.data(), t.inf.data(), t.flat.data(), t.off.data(), 0,
                                         0, n, coeffs, status, nullptr);
    });
}

class KeyCache;

// The half-aggregate of n signatures: their R's, 49 bytes each, and e_agg = sum a_i e_i mod q with
// coefficients hashed out of every R, key, message and the order of the lanes -- 49 n + 32 bytes for 81 n.  verify_batch
// semantics: the flag byte of R is honoured, there is no subgroup check.
struct AggregateSignature {
    std::vector<uint8_t> bytes;                 // SSA_AGGREGATE_LENGTH(n)
    size_t size() const { return (bytes.size() - 32) / 49; }
    // check: every signature is verified first (SSA_AGG_CHECK) and a slice with a bad one yields its error instead of an
    // aggregate; without it only inputs the verifier would call malformed are refused (Panic)
    static std::optional<AggregateSignature> aggregate(Context &cx, const std::vector<Signature> &signatures,
                                                       const std::vector<PublicKey> &public_keys,
                                                       const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                       bool check = true, bool sliced = false) {
        const PackedTriples t = pack_triples(signatures, public_keys, messages);
        const size_t n = signatures.size();
        AggregateSignature a;
        a.bytes.assign(SSA_AGGREGATE_LENGTH(n), 0);
        const int rc = (sliced ? ssa_aggregate_many_sliced : ssa_aggregate_many)(
            cx.get(), t.sigs.data(), t.pks.data(), t.inf.data(), t.flat.data(), t.off.data(), 0, 0, n,
            check ? SSA_AGG_CHECK : 0u, a.bytes.data(), nullptr, nullptr);
        if (rc < 0) throw std::runtime_error(std::string("ssa_aggregate_many: ") + ssa_strerror(rc));
        if (rc == SSA_MALFORMED) throw Panic("undecodable signature in batch (the reference panics here)");
        if (rc != SSA_OK) return std::nullopt;
        return a;
    }
    // The same aggregate, byte for byte, for any number of signatures up to SSA_MAX_BATCH: slice after slice of the
    // context in bounded workspaces (ssa_aggregate_many_sliced)
    static std::optional<AggregateSignature> aggregate_sliced(Context &cx, const std::vector<Signature> &signatures,
                                                              const std::vector<PublicKey> &public_keys,
                                                              const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                              bool check = true) {
        return aggregate(cx, signatures, public_keys, messages, check, true);
    }
    // Many aggregates from one call (ssa_aggregates_many): the triples of all slices in order,
    // counts[j] of them for aggregate j.  Element j is what aggregate() gives slice j alone, byte for byte, and nullopt
    // where it would refuse (also where it would throw Panic: nothing is thrown for one slice among many); *results_out
    // (optional) receives the k statuses -- SSA_OK, SSA_MALFORMED or, with check, the smallest nonzero status of the
    // slice's signatures.
    static std::vector<std::optional<AggregateSignature>>
    aggregate_many(Context &cx, const std::vector<uint64_t> &counts, const std::vector<Signature> &signatures,
                   const std::vector<PublicKey> &public_keys, const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                   bool check = true, std::vector<uint32_t> *results_out = nullptr) {
        const PackedTriples t = pack_triples(signatures, public_keys, messages);
        const size_t n = signatures.size(), k = counts.size();
        size_t total = 0;
        for (uint64_t c : counts) total += c;
        if (total != n) throw Panic("We should have the same number of signatures than the counts say");
        std::vector<std::optional<AggregateSignature>> out(k);
        std::vector<uint32_t> results(k, SSA_MALFORMED);
        if (k) {
            std::vector<uint8_t> wire(49 * n + 32 * k, 0);
            const int rc = ssa_aggregates_many(cx.get(), t.sigs.data(), counts.data(), k, t.pks.data(), t.inf.data(),
                                               t.flat.data(), t.off.data(), 0, 0, check ? SSA_AGG_CHECK : 0u, wire.data(),
                                               results.data(), nullptr, nullptr);
            if (rc != 0) throw std::runtime_error(std::string("ssa_aggregates_many: ") + ssa_strerror(rc));
            size_t lo = 0;
            for (size_t j = 0; j < k; lo += SSA_AGGREGATE_LENGTH(counts[j]), j++) {
                if (results[j] != SSA_OK) continue;
                out[j].emplace();
                out[j]->bytes.assign(wire.begin() + lo, wire.begin() + lo + SSA_AGGREGATE_LENGTH(counts[j]));
            }
        }
        if (results_out) *results_out = std::move(results);
        return out;
    }
    // Filtering half-aggregation: the aggregate of exactly the triples that verify under
    // verify_batch semantics, and their indices in ascending order.  A triple that does not verify is dropped, not
    // reported as an error; with none kept the aggregate is the empty one (32 zero bytes).
    static std::pair<AggregateSignature, std::vector<uint32_t>>
    aggregate_valid(Context &cx, const std::vector<Signature> &signatures, const std::vector<PublicKey> &public_keys,
                    const std::vector<std::pair<const uint8_t *, size_t>> &messages) {
        const PackedTriples t = pack_triples(signatures, public_keys, messages);
        const size_t n = signatures.size();
        AggregateSignature a;
        a.bytes.assign(SSA_AGGREGATE_LENGTH(n), 0);
        std::vector<uint32_t> kept(n ? n : 1, 0u);
        uint64_t n_kept = 0;
        const int rc = ssa_aggregate_valid_many(cx.get(), t.sigs.data(), t.pks.data(), t.inf.data(), t.flat.data(),
                                                t.off.data(), 0, 0, n, a.bytes.data(), kept.data(), &n_kept, nullptr);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregate_valid_many: ") + ssa_strerror(rc));
        a.bytes.resize(SSA_AGGREGATE_LENGTH(n_kept));
        kept.resize(n_kept);
        return {std::move(a), std::move(kept)};
    }
    // The same through a key cache: a triple is kept iff Signature::verify accepts it -- the
    // subgroup check of its key included, once per key and cache -- so verify_many on the same cache accepts the result.
    // An Affine cache takes the objects and hands the kept keys back in *kept_keys; a Wire cache takes n 130-byte
    // KeyedSignature records (key 49 || signature 81) side by side and hands back the kept lanes' 49 key bytes, which
    // the wire-key overload of verify_many takes.  stats_out: 12 words, optional.  (Defined behind KeyCache.)
    static std::pair<AggregateSignature, std::vector<uint32_t>>
    aggregate_valid(Context &cx, KeyCache &cache, const std::vector<Signature> &signatures,
                    const std::vector<PublicKey> &public_keys, const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                    std::vector<PublicKey> *kept_keys = nullptr, uint64_t *stats_out = nullptr);
    static std::pair<AggregateSignature, std::vector<uint32_t>>
    aggregate_valid(Context &cx, KeyCache &cache, const std::vector<uint8_t> &keyed_records,
                    const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                    std::vector<uint8_t> *kept_keys49 = nullptr, uint64_t *stats_out = nullptr);
    Result verify(Context &cx, const std::vector<PublicKey> &public_keys,
                  const std::vector<std::pair<const uint8_t *, size_t>> &messages, bool sliced = false) const {
        if (public_keys.size() != size() || messages.size() != size())
            throw Panic("We should have the same number of messages than public keys");
        const PackedTriples t = pack_triples(std::vector<Signature>(size()), public_keys, messages);
        return status_to_result((sliced ? ssa_verify_aggregate_sliced : ssa_verify_aggregate)(
            cx.get(), bytes.data(), t.pks.data(), t.inf.data(), t.flat.data(), t.off.data(), 0, 0, size()));
    }
    // the same verdict for any size up to SSA_MAX_BATCH (ssa_verify_aggregate_sliced)
    Result verify_sliced(Context &cx, const std::vector<PublicKey> &public_keys,
                         const std::vector<std::pair<const uint8_t *, size_t>> &messages) const {
        return verify(cx, public_keys, messages, true);
    }
    // Many aggregates in one call: the keys and messages of all their lanes, in order.  One status
    // per aggregate -- SSA_OK, SSA_INVALID_SIGNATURE or SSA_MALFORMED (where verify() panics) --, each the value verify()
    // stands for on that aggregate alone.
    static std::vector<uint32_t> verify_many(Context &cx, const std::vector<AggregateSignature> &aggregates,
                                             const std::vector<PublicKey> &public_keys,
                                             const std::vector<std::pair<const uint8_t *, size_t>> &messages) {
        std::vector<uint64_t> counts;
        std::vector<uint8_t> wire;
        size_t n = 0;
        for (const AggregateSignature &a : aggregates) {
            counts.push_back(a.size());
            n += a.size();
            wire.insert(wire.end(), a.bytes.begin(), a.bytes.end());
        }
        if (public_keys.size() != n || messages.size() != n)
            throw Panic("We should have the same number of messages than public keys");
        std::vector<uint32_t> verdicts(aggregates.size(), SSA_MALFORMED);
        if (aggregates.empty()) return verdicts;
        const PackedTriples t = pack_triples(std::vector<Signature>(n), public_keys, messages);
        const int rc = ssa_verify_aggregates_many(cx.get(), wire.data(), counts.data(), counts.size(), t.pks.data(),
                                                  t.inf.data(), t.flat.data(), t.off.data(), 0, 0, verdicts.data());
        if (rc != 0) throw std::runtime_error(std::string("ssa_verify_aggregates_many: ") + ssa_strerror(rc));
        return verdicts;
    }
    // The same through a key cache, the subgroup check of every key included: an aggregate that
    // holds a key outside the prime-order subgroup gets SSA_INVALID_PUBLIC_KEY, every other status is verify_many's, in
    // every state of the cache; each distinct key is checked once per cache.  An Affine cache takes PublicKey objects; a
    // Wire cache takes the keys as they arrive, 49 bytes each side by side, and decompresses each distinct one once.
    // stats_out: 8 words, optional.  (Defined behind KeyCache.)
    static std::vector<uint32_t> verify_many(Context &cx, KeyCache &cache, const std::vector<AggregateSignature> &aggregates,
                                             const std::vector<PublicKey> &public_keys,
                                             const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                             uint64_t *stats_out = nullptr);
    static std::vector<uint32_t> verify_many(Context &cx, KeyCache &cache, const std::vector<AggregateSignature> &aggregates,
                                             const std::vector<uint8_t> &wire_keys,
                                             const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                             uint64_t *stats_out = nullptr);
    const std::vector<uint8_t> &to_bytes() const { return bytes; }
    // nullopt when the length is not 49 n + 32 or e_agg is not canonical
    static std::optional<AggregateSignature> from_bytes(const std::vector<uint8_t> &b) {
        static const uint64_t Q[4] = {0xd443623eaed4accfULL, 0x327aa72330157722ULL, 0x563fbf0f990a37b5ULL, 0x7af2599b3b3f22d0ULL};
        if (b.size() < 32 || (b.size() - 32) % 49) return std::nullopt;
        for (int k = 3; k >= 0; k--) {
            uint64_t w = 0;
            for (int j = 7; j >= 0; j--) w = (w << 8) | b[b.size() - 32 + 8 * k + j];
            if (w < Q[k]) break;
            if (w > Q[k] || k == 0) return std::nullopt;
        }
        AggregateSignature a;
        a.bytes = b;
        return a;
    }
};

// Signature::verify (src/signature.rs:181-205) over a slice of signatures in which public keys repeat: one status per
// signature (0 Ok, 1 InvalidPublicKey, 2 InvalidSignature, 3 malformed: the reference would panic), the same vector as n
// single calls, with each DISTINCT key's subgroup check and table run once on the GPU.
inline std::vector<uint8_t> verify_many_statuses(Context &cx, const std::vector<Signature> &signatures,
                                                 const std::vector<PublicKey> &public_keys,
                                                 const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                 uint64_t *stats_out = nullptr) {
    const PackedTriples t = pack_triples(signatures, public_keys, messages);
    const size_t n = signatures.size();
    return statuses_of(n, nullptr, "ssa_verify_many_dedup", [&](uint8_t *status, const uint8_t *) {
        return ssa_verify_many_dedup(cx.get(), t.sigs.data(), t.pks.data(), t.inf.data(), t.flat.data(), t.off.data(), 0, 0,
                                     n, SSA_FLAG_CHECK_TORSION, status, nullptr, stats_out);
    });
}

// The same vector as verify_many_statuses at about the price of one MSM for an honest slice: each
// distinct key checked once, the segments of the slice screened by a random linear combination (coefficients from `rng`,
// or drawn on the device), only the lanes of failing segments and the lanes that could not be screened checked exactly.
// A rejected signature is reported except with the probability the header states.  stats_out: 8 words, optional.
inline std::vector<uint8_t> verify_many_screened_statuses(Context &cx, const std::vector<Signature> &signatures,
                                                          const std::vector<PublicKey> &public_keys,
                                                          const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                          Rng rng = nullptr, uint64_t *stats_out = nullptr) {
    const PackedTriples t = pack_triples(signatures, public_keys, messages);
    const size_t n = signatures.size();
    return statuses_of(n, rng, "ssa_verify_many_screened", [&](uint8_t *status, const uint8_t *coeffs) {
        return ssa_verify_many_screened(cx.get(), t.sigs.data(), t.pks.data(), t.inf.data(), t.flat.data(), t.off.data(), 0,
                                        0, n, SSA_FLAG_CHECK_TORSION, coeffs, status, nullptr, stats_out);
    });
}

// A key cache on the device (ssa_keycache_create): the checks and tables of the public keys that
// verify_many_cached_statuses has seen, kept across slices and calls.  Belongs to the context it was made on.
class KeyCache {
  public:
    struct Info {
        uint64_t capacity, held, clears, device_bytes;
    };
    // Wire (SSA_KEYCACHE_WIRE): a key is identified by its 49 compressed bytes as received; such a
    // cache serves verify_keyed_many_cached_statuses / verify_keyed_many_cached_device and the wire-key overload of
    // AggregateSignature::verify_many, and no other call
    enum Mode : uint32_t { Affine = 0u, Wire = SSA_KEYCACHE_WIRE };
    KeyCache(Context &cx, size_t capacity, Mode mode = Affine) : wire_(mode == Wire) {
        const int rc = ssa_keycache_create_ex(cx.get(), capacity, (uint32_t)mode, &kc_);
        if (rc != 0) throw std::runtime_error(std::string("ssa_keycache_create_ex: ") + ssa_strerror(rc));
    }
    bool wire() const { return wire_; }
    ~KeyCache() { ssa_keycache_destroy(kc_); }
    KeyCache(const KeyCache &) = delete;
    KeyCache &operator=(const KeyCache &) = delete;
    ssa_keycache *get() const { return kc_; }
    void clear() {
        const int rc = ssa_keycache_clear(kc_);
        if (rc != 0) throw std::runtime_error(std::string("ssa_keycache_clear: ") + ssa_strerror(rc));
    }
    Info info() const {
        uint64_t v[4] = {0, 0, 0, 0};
        const int rc = ssa_keycache_info(kc_, v);
        if (rc != 0) throw std::runtime_error(std::string("ssa_keycache_info: ") + ssa_strerror(rc));
        return {v[0], v[1], v[2], v[3]};
    }
    // What a full cache does: Clear (the default) empties it; Recent keeps the rows used most
    // recently.  Recent allocates the rows' stamps and the compaction's scratch, once: info().device_bytes grows here.
    enum Eviction : uint32_t { Clear = SSA_KEYCACHE_EVICT_CLEAR, Recent = SSA_KEYCACHE_EVICT_RECENT };
    struct EvictionInfo {
        uint64_t policy, compactions, dropped, last_kept, last_moved, epoch;
    };
    void set_eviction(Eviction policy) {
        const int rc = ssa_keycache_set_eviction(kc_, (uint32_t)policy);
        if (rc != 0) throw std::runtime_error(std::string("ssa_keycache_set_eviction: ") + ssa_strerror(rc));
    }
    EvictionInfo eviction_info() const {
        uint64_t v[8] = {};
        const int rc = ssa_keycache_eviction_info(kc_, v);
        if (rc != 0) throw std::runtime_error(std::string("ssa_keycache_eviction_info: ") + ssa_strerror(rc));
        return {v[0], v[1], v[2], v[3], v[4], v[5]};
    }
    // the exact check of every held row against its stored key bytes; deep: also [q]P per key; repair: failing rows are
    // rebuilt in place from their stored bytes and checked again (ok: clean afterwards)
    KeyCheck selfcheck(bool deep = false, bool repair = false) {
        uint64_t o[8] = {};
        const int rc = ssa_keycache_selfcheck(kc_, (deep ? SSA_KEYCHECK_DEEP : 0u) | (repair ? SSA_KEYCHECK_REPAIR : 0u), o);
        return keycheck_result(rc, o, "ssa_keycache_selfcheck");
    }

  private:
    ssa_keycache *kc_ = nullptr;
    bool wire_ = false;
};

// A streaming aggregator on the device (ssa_aggregator_create): push signatures as they arrive,
// finish at block time.  push admits a slice of triples and appends the ones that pass, in order; finish gives the
// aggregate of the first n_take admitted triples -- byte for byte AggregateSignature::aggregate(check = false) of those
// triples alone -- and changes nothing, so it may be repeated, called with another n_take, and followed by more pushes.
// The KeyCache overloads admit through a key cache, under the verdict validators apply, and an object made with HoldKeys
// keeps the admitted lanes' wire keys.  Belongs to the context it was made on.
class Aggregator {
  public:
    struct Info {
        uint64_t held, capacity, block_lanes, pushes, offered, dropped, blocks, finishes;
    };
    static constexpr size_t All = SIZE_MAX;       // finish: every triple held
    // HoldKeys (SSA_AGGR_HOLD_KEYS49): the object also holds the 49 wire bytes of every admitted lane's key, for keys();
    // it then takes push_keyed alone.  HoldAdmission (SSA_AGGR_HOLD_ADMISSION): the object also
    // records the class of the push that admitted each lane, for admission() and for the KeyCache overloads of
    // AggregateVerifier::push_mixed.  HoldIndex (SSA_AGGR_HOLD_INDEX): the object also holds a leaf
    // index, for lookup().  The options combine with | (below).
    enum Options : uint32_t {
        None = 0u,
        HoldKeys = SSA_AGGR_HOLD_KEYS49,
        HoldAdmission = SSA_AGGR_HOLD_ADMISSION,
        HoldKeysAndAdmission = SSA_AGGR_HOLD_KEYS49 | SSA_AGGR_HOLD_ADMISSION,
        HoldIndex = SSA_AGGR_HOLD_INDEX
    };
    friend constexpr Options operator|(Options a, Options b) { return (Options)((uint32_t)a | (uint32_t)b); }
    // the words of index_info(), and what lookup() returns
    struct IndexInfo {
        uint64_t slots, indexed, stale, rebuilds, overflowed, lookups, ids, reserved;
    };
    struct Lookup {
        std::vector<uint32_t> places;      // the lowest place that holds the id, or SSA_AGGV_UNKNOWN
        uint64_t n_unknown;
    };
    // how a lane was admitted: by push(screen = false), by the plain screened push, or through a key cache
    enum class Admission : uint8_t {
        Unscreened = SSA_ADM_UNSCREENED,
        Screened = SSA_ADM_SCREENED,
        KeyChecked = SSA_ADM_KEY_CHECKED
    };
    // block_lanes: 0 (512) or a power of two from 2 to 512.  All device memory, about 113 bytes per lane (162 with
    // HoldKeys), is allocated here.
    Aggregator(Context &cx, size_t capacity, size_t block_lanes = 0, Options options = None) : cx_(cx) {
        const int rc = ssa_aggregator_create(cx.get(), capacity, block_lanes, (uint32_t)options, &ag_);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_create: ") + ssa_strerror(rc));
    }
    ~Aggregator() { ssa_aggregator_destroy(ag_); }
    Aggregator(const Aggregator &) = delete;
    Aggregator &operator=(const Aggregator &) = delete;
    ssa_aggregator *get() const { return ag_; }
    // One status byte per triple; the triples whose byte is zero were appended.  screen: the statuses of
    // verify_batch_statuses on this slice alone (library-drawn coefficients); without it 0 or SSA_MALFORMED by the checks
    // aggregate(check = false) makes (SSA_AGGR_NO_SCREEN: for a producer that made the signatures itself).  A slice that
    // does not fit what is left of the capacity throws and changes nothing.
    std::vector<uint8_t> push(const std::vector<Signature> &signatures, const std::vector<PublicKey> &public_keys,
                              const std::vector<std::pair<const uint8_t *, size_t>> &messages, bool screen = true,
                              uint64_t *n_kept_out = nullptr) {
        const PackedTriples t = pack_triples(signatures, public_keys, messages);
        const size_t n = signatures.size();
        std::vector<uint8_t> status(n, 0);
        uint64_t n_kept = 0;
        const int rc = ssa_aggregator_push(cx_.get(), ag_, t.sigs.data(), t.pks.data(), t.inf.data(), t.flat.data(),
                                           t.off.data(), 0, 0, n, screen ? 0u : SSA_AGGR_NO_SCREEN,
                                           n ? status.data() : nullptr, &n_kept);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_push: ") + ssa_strerror(rc));
        if (n_kept_out) *n_kept_out = n_kept;
        return status;
    }
    // Through a key cache, subgroup check included: statuses and stats_out (12 words, or nullptr)
    // are those of ssa_aggregate_valid_many_cached on this slice alone and the same cache -- a triple whose key lies
    // outside the prime-order subgroup is dropped with SSA_INVALID_PUBLIC_KEY.  An Affine cache here, a Wire cache for
    // push_keyed.  Lanes of every kind of push may be mixed in one object.
    std::vector<uint8_t> push(KeyCache &cache, const std::vector<Signature> &signatures,
                              const std::vector<PublicKey> &public_keys,
                              const std::vector<std::pair<const uint8_t *, size_t>> &messages, uint64_t *n_kept_out = nullptr,
                              uint64_t *stats_out = nullptr) {
        if (cache.wire()) throw std::invalid_argument("a Wire key cache takes KeyedSignature records (push_keyed)");
        const PackedTriples t = pack_triples(signatures, public_keys, messages);
        const size_t n = signatures.size();
        std::vector<uint8_t> status(n, 0);
        uint64_t n_kept = 0;
        const int rc = ssa_aggregator_push_cached(cx_.get(), ag_, cache.get(), t.sigs.data(), t.pks.data(), t.inf.data(),
                                                  t.flat.data(), t.off.data(), 0, 0, n, n ? status.data() : nullptr, &n_kept,
                                                  stats_out);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_push_cached: ") + ssa_strerror(rc));
        if (n_kept_out) *n_kept_out = n_kept;
        return status;
    }
    // keyed: messages.size() records side by side, 130 bytes each (key 49 || signature 81), as a mempool receives them;
    // statuses and stats_out are those of ssa_aggregate_valid_keyed_many_cached on this slice alone and the same cache
    std::vector<uint8_t> push_keyed(KeyCache &cache, const std::vector<uint8_t> &keyed,
                                    const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                    uint64_t *n_kept_out = nullptr, uint64_t *stats_out = nullptr) {
        if (!cache.wire()) throw std::invalid_argument("an Affine key cache takes triples (push), not KeyedSignature records");
        const size_t n = messages.size();
        if (keyed.size() != n * KEYED_SIGNATURE_LENGTH)
            throw std::invalid_argument("We should have the same number of messages than keyed signatures");
        std::vector<uint8_t> flat;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) {
            flat.insert(flat.end(), messages[i].first, messages[i].first + messages[i].second);
            off[i + 1] = flat.size();
        }
        flat.push_back(0);
        std::vector<uint8_t> status(n, 0);
        uint64_t n_kept = 0;
        const int rc = ssa_aggregator_push_keyed_cached(cx_.get(), ag_, cache.get(), n ? keyed.data() : nullptr, flat.data(),
                                                        off.data(), 0, 0, n, n ? status.data() : nullptr, &n_kept, stats_out);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_push_keyed_cached: ") + ssa_strerror(rc));
        if (n_kept_out) *n_kept_out = n_kept;
        return status;
    }
    // the same over KeyedSignature objects: each is put on the wire (KeyedSignature::to_bytes) first
    std::vector<uint8_t> push_keyed(KeyCache &cache, const std::vector<KeyedSignature> &records,
                                    const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                    uint64_t *n_kept_out = nullptr, uint64_t *stats_out = nullptr) {
        std::vector<uint8_t> keyed;
        keyed.reserve(records.size() * KEYED_SIGNATURE_LENGTH);
        for (const KeyedSignature &r : records) {
            const auto b = r.to_bytes(cx_);
            keyed.insert(keyed.end(), b.begin(), b.end());
        }
        return push_keyed(cache, keyed, messages, n_kept_out, stats_out);
    }
    // the wire keys of the first n_take held triples, 49 bytes each, in arrival order (an object made with HoldKeys; any
    // other throws): with finish(n_take) the block body AggregateSignature::verify_many's wire-key overload takes
    std::vector<uint8_t> keys(size_t n_take = All) const {
        const size_t n = n_take == All ? (size_t)info().held : n_take;
        std::vector<uint8_t> out(n * PUBLIC_KEY_LENGTH + 1, 0);
        const int rc = ssa_aggregator_keys(cx_.get(), ag_, n, out.data());
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_keys: ") + ssa_strerror(rc));
        out.resize(n * PUBLIC_KEY_LENGTH);
        return out;
    }
    // the admission classes (Admission, as bytes) of the first n_take held triples, in arrival order (an object made with
    // HoldAdmission; any other throws).  Changes nothing.
    std::vector<uint8_t> admission(size_t n_take = All) const {
        const size_t n = n_take == All ? (size_t)info().held : n_take;
        std::vector<uint8_t> out(n + 1, 0);
        const int rc = ssa_aggregator_admission(cx_.get(), ag_, n, out.data());
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_admission: ") + ssa_strerror(rc));
        out.resize(n);
        return out;
    }
    // ---- the leaf column and the leaf index.  A lane's 32-byte leaf is its id.
    // the leaves of the first n_take held triples, 32 bytes each, in arrival order (every object has them)
    std::vector<uint8_t> leaves(size_t n_take = All) const {
        const size_t n = n_take == All ? (size_t)info().held : n_take;
        std::vector<uint8_t> out(32 * n + 1, 0);
        const int rc = ssa_aggregator_leaves(cx_.get(), ag_, n, out.data());
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_leaves: ") + ssa_strerror(rc));
        out.resize(32 * n);
        return out;
    }
    // the leaves at the places order[0], order[1], ... in that order: the id column beside finish_select(order).  An index
    // that is not below the triples held throws.
    std::vector<uint8_t> leaves_select(const std::vector<uint32_t> &order) const {
        const size_t m = order.size();
        std::vector<uint8_t> out(32 * m + 1, 0);
        const int rc = ssa_aggregator_leaves_select(cx_.get(), ag_, m ? order.data() : nullptr, m, out.data());
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_leaves_select: ") + ssa_strerror(rc));
        out.resize(32 * m);
        return out;
    }
    // brings the index up to date with the triples held (only enqueues; a lookup does the same in front of its query)
    void index_sync() {
        const int rc = ssa_aggregator_index_sync(cx_.get(), ag_);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_index_sync: ") + ssa_strerror(rc));
    }
    // ids32: n ids side by side, 32 bytes each -> for each the lowest place that holds it, or SSA_AGGV_UNKNOWN, and the
    // number of the latter: what AggregateVerifier::push_mixed takes.  An object made without HoldIndex throws.
    Lookup lookup(const std::vector<uint8_t> &ids32) {
        if (ids32.size() % 32) throw std::invalid_argument("ids are 32 bytes each");
        const size_t n = ids32.size() / 32;
        Lookup r{std::vector<uint32_t>(n + 1, SSA_AGGV_UNKNOWN), 0};
        const int rc = ssa_aggregator_lookup(cx_.get(), ag_, n ? ids32.data() : nullptr, n, r.places.data(), &r.n_unknown);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_lookup: ") + ssa_strerror(rc));
        r.places.resize(n);
        return r;
    }
    // synchronises the context's stream once (the overflow counter lives on the device)
    IndexInfo index_info() const {
        uint64_t w[8] = {0};
        const int rc = ssa_aggregator_index_info(cx_.get(), ag_, w);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_index_info: ") + ssa_strerror(rc));
        return IndexInfo{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
    }
    AggregateSignature finish(size_t n_take = All) const {
        const size_t n = n_take == All ? (size_t)info().held : n_take;
        AggregateSignature a;
        a.bytes.assign(SSA_AGGREGATE_LENGTH(n), 0);
        const int rc = ssa_aggregator_finish(cx_.get(), ag_, n, a.bytes.data());
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_finish: ") + ssa_strerror(rc));
        return a;
    }
    // Removing triples in place: the object is then what it would be had it admitted the remaining
    // triples alone, in their order; only `held` and `blocks` of the counters move.  drop_front: the first n (All: every
    // one); more than are held throws and changes nothing.
    void drop_front(size_t n = All) {
        const int rc = ssa_aggregator_drop_front(cx_.get(), ag_, n);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_drop_front: ") + ssa_strerror(rc));
    }
    // drop: one byte per held triple; triple i is removed iff drop[i] != 0 (a status vector can be handed in as it is).
    // -> the number of triples kept.  Another length throws and changes nothing.
    uint64_t remove(const std::vector<uint8_t> &drop) {
        uint64_t n_kept = 0;
        const int rc = ssa_aggregator_remove(cx_.get(), ag_, drop.empty() ? nullptr : drop.data(), drop.size(), &n_kept);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_remove: ") + ssa_strerror(rc));
        return n_kept;
    }
    // the same over a mask in device memory; synchronises the context's stream once, for the count
    uint64_t remove_device(const uint8_t *d_drop, size_t n_bytes) {
        uint64_t n_kept = 0;
        const int rc = ssa_aggregator_remove_device(cx_.get(), ag_, d_drop, n_bytes, &n_kept);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_remove_device: ") + ssa_strerror(rc));
        return n_kept;
    }
    // finish(n_take), then drop_front of the same triples: they leave the object, the rest stays for the next block
    AggregateSignature take(size_t n_take = All) {
        const size_t n = n_take == All ? (size_t)info().held : n_take;
        AggregateSignature a = finish(n);
        drop_front(n);
        return a;
    }
    // A block of the producer's choosing: the aggregate of the held triples at the places
    // order[0], order[1], ... -- distinct, below the triples held -- in THAT order: byte for byte
    // AggregateSignature::aggregate(check = false) of those triples alone.  Changes nothing, like finish.  keys49_out (an
    // object made with HoldKeys; any other throws): their wire keys in the same order, 49 bytes each.  A list the device
    // refuses (an index out of range or named twice) throws, and the object is as it was.
    AggregateSignature finish_select(const std::vector<uint32_t> &order, std::vector<uint8_t> *keys49_out = nullptr) const {
        const size_t m = order.size();
        AggregateSignature a;
        a.bytes.assign(SSA_AGGREGATE_LENGTH(m), 0);
        if (keys49_out) keys49_out->assign(m * PUBLIC_KEY_LENGTH + 1, 0);
        const int rc = ssa_aggregator_finish_select(cx_.get(), ag_, m ? order.data() : nullptr, m, a.bytes.data(),
                                                    keys49_out ? keys49_out->data() : nullptr);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_finish_select: ") + ssa_strerror(rc));
        if (keys49_out) keys49_out->resize(m * PUBLIC_KEY_LENGTH);
        return a;
    }
    // remove with a list in place of a mask: the named triples leave, the rest stays in arrival order -> the number kept.
    // A list the device refuses throws and changes nothing.
    uint64_t remove_indices(const std::vector<uint32_t> &order) {
        uint64_t n_kept = 0;
        const int rc = ssa_aggregator_remove_indices(cx_.get(), ag_, order.empty() ? nullptr : order.data(), order.size(), &n_kept);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_remove_indices: ") + ssa_strerror(rc));
        return n_kept;
    }
    // finish_select(order), then remove_indices(order): the chosen triples leave as a block body, the rest stays for the
    // next slot
    AggregateSignature take_select(const std::vector<uint32_t> &order, std::vector<uint8_t> *keys49_out = nullptr) {
        AggregateSignature a = finish_select(order, keys49_out);
        remove_indices(order);
        return a;
    }
    void reset() {
        const int rc = ssa_aggregator_reset(ag_);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_reset: ") + ssa_strerror(rc));
    }
    Info info() const {
        uint64_t v[8] = {};
        const int rc = ssa_aggregator_info(ag_, v);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggregator_info: ") + ssa_strerror(rc));
        return {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
    }

  private:
    Context &cx_;
    ssa_aggregator *ag_ = nullptr;
};

// A streaming aggregate verifier on the device (ssa_aggverifier_create): push the R's, keys and
// messages of a block body as they arrive, finish with e_agg.  push appends EVERY lane -- a validator cannot drop one, its
// place is part of the transcript --; finish gives what AggregateSignature::verify gives the first n_take lanes handed in
// at once with that scalar, and changes nothing, so it may be repeated, take prefixes, and be followed by more pushes.
// Belongs to the context it was made on.
class AggregateVerifier {
  public:
    struct Info {
        uint64_t held, capacity, block_lanes, pushes, pushed, reserved, blocks, finishes;     // reserved: lanes pushed
    };                                                                                        // through a key cache
    static constexpr size_t All = SIZE_MAX;       // finish: every lane held
    // block_lanes: 0 (512) or a power of two from 2 to 512.  All device memory, about 259 bytes per lane, is allocated here.
    AggregateVerifier(Context &cx, size_t capacity, size_t block_lanes = 0) : cx_(cx) {
        const int rc = ssa_aggverifier_create(cx.get(), capacity, block_lanes, 0u, &av_);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_create: ") + ssa_strerror(rc));
    }
    ~AggregateVerifier() { ssa_aggverifier_destroy(av_); }
    AggregateVerifier(const AggregateVerifier &) = delete;
    AggregateVerifier &operator=(const AggregateVerifier &) = delete;
    ssa_aggverifier *get() const { return av_; }
    // rs49: the R's of public_keys.size() lanes side by side, 49 bytes each (the head of an aggregate's bytes).  A slice
    // that does not fit what is left of the capacity throws and changes nothing.
    void push(const uint8_t *rs49, const std::vector<PublicKey> &public_keys,
              const std::vector<std::pair<const uint8_t *, size_t>> &messages) {
        const size_t n = public_keys.size();
        const PackedTriples t = pack_triples(std::vector<Signature>(n), public_keys, messages);
        const int rc = ssa_aggverifier_push(cx_.get(), av_, rs49, t.pks.data(), t.inf.data(), t.flat.data(), t.off.data(),
                                            0, 0, n);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_push: ") + ssa_strerror(rc));
    }
    // the R's of an aggregate; its scalar is not kept: hand it to finish
    void push(const AggregateSignature &agg, const std::vector<PublicKey> &public_keys,
              const std::vector<std::pair<const uint8_t *, size_t>> &messages) {
        if (agg.size() != public_keys.size()) throw Panic("We should have the same number of signatures than public keys");
        push(agg.bytes.data(), public_keys, messages);
    }
    // Through a key cache, subgroup check included: every distinct key is checked once, and a finish
    // that takes a lane whose key lies outside the prime-order subgroup answers SSA_INVALID_PUBLIC_KEY -- the guarantee of
    // Signature::verify.  An Affine cache here, a Wire cache for push_wire.  stats_out: 8 words (ssa_aggverifier_push_cached)
    // or nullptr.  Lanes of the plain push are "not checked"; both kinds may be mixed in one object.
    void push(KeyCache &cache, const uint8_t *rs49, const std::vector<PublicKey> &public_keys,
              const std::vector<std::pair<const uint8_t *, size_t>> &messages, uint64_t *stats_out = nullptr) {
        if (cache.wire()) throw std::invalid_argument("a Wire key cache takes 49-byte keys (push_wire), not PublicKey objects");
        const size_t n = public_keys.size();
        const PackedTriples t = pack_triples(std::vector<Signature>(n), public_keys, messages);
        const int rc = ssa_aggverifier_push_cached(cx_.get(), av_, cache.get(), rs49, t.pks.data(), t.inf.data(),
                                                   t.flat.data(), t.off.data(), 0, 0, n, stats_out);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_push_cached: ") + ssa_strerror(rc));
    }
    void push(KeyCache &cache, const AggregateSignature &agg, const std::vector<PublicKey> &public_keys,
              const std::vector<std::pair<const uint8_t *, size_t>> &messages, uint64_t *stats_out = nullptr) {
        if (agg.size() != public_keys.size()) throw Panic("We should have the same number of signatures than public keys");
        push(cache, agg.bytes.data(), public_keys, messages, stats_out);
    }
    // wire_keys: messages.size() keys side by side, 49 bytes each, as a block body carries them
    void push_wire(KeyCache &cache, const uint8_t *rs49, const std::vector<uint8_t> &wire_keys,
                   const std::vector<std::pair<const uint8_t *, size_t>> &messages, uint64_t *stats_out = nullptr) {
        if (!cache.wire()) throw std::invalid_argument("an Affine key cache takes PublicKey objects (push), not 49-byte keys");
        const size_t n = messages.size();
        if (wire_keys.size() != n * PUBLIC_KEY_LENGTH) throw Panic("We should have the same number of messages than public keys");
        std::vector<uint8_t> flat;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) {
            flat.insert(flat.end(), messages[i].first, messages[i].first + messages[i].second);
            off[i + 1] = flat.size();
        }
        flat.push_back(0);
        const int rc = ssa_aggverifier_push_cached_wire(cx_.get(), av_, cache.get(), rs49, wire_keys.data(), flat.data(),
                                                        off.data(), 0, 0, n, stats_out);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_push_cached_wire: ") + ssa_strerror(rc));
    }
    // A block against the pool: places[i] is the place in `pool` of lane i of the block, or Unknown
    // for a lane the pool does not hold.  The unknown lanes come with the call, side by side in block order -- rs49 their
    // R's, 49 bytes each, then their keys and messages as push takes them --; a known lane takes leaf and scalar from the
    // pool, copied.  finish then answers as for the block with every known lane replaced by what the pool admitted it
    // with, PROVIDED the pool's scalar of every known lane satisfies its verification equation: name only lanes that a
    // screened or cached push admitted.  An invalid list throws and changes nothing.
    static constexpr uint32_t Unknown = SSA_AGGV_UNKNOWN;
    void push_mixed(Aggregator &pool, const std::vector<uint32_t> &places, const uint8_t *rs49,
                    const std::vector<PublicKey> &public_keys,
                    const std::vector<std::pair<const uint8_t *, size_t>> &messages) {
        const size_t u = public_keys.size();
        const PackedTriples t = pack_triples(std::vector<Signature>(u), public_keys, messages);
        const int rc = ssa_aggverifier_push_mixed(cx_.get(), av_, pool.get(), places.data(), places.size(), rs49, t.pks.data(),
                                                  t.inf.data(), t.flat.data(), t.off.data(), 0, 0, u);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_push_mixed: ") + ssa_strerror(rc));
    }
    // The same through a key cache, with a required admission class: the unknown lanes are treated
    // as push(cache, ...) / push_wire treat them, and a known lane whose class in the pool is below `require` is refused
    // -- the call throws and changes nothing.  Above Require::None the pool must be made with HoldAdmission.  With
    // Require::KeyChecked on lanes the pool admitted through a cache, finish answers what
    // AggregateSignature::verify_many's cached form answers for the whole block: the caller owes nothing but the places.
    // An Affine cache here, a Wire cache for push_mixed_wire.  stats_out: 8 words over the unknown lanes, or nullptr.
    enum class Require : uint32_t {
        None = SSA_ADM_UNSCREENED,
        Screened = SSA_ADM_SCREENED,
        KeyChecked = SSA_ADM_KEY_CHECKED
    };
    void push_mixed(Aggregator &pool, KeyCache &cache, const std::vector<uint32_t> &places, const uint8_t *rs49,
                    const std::vector<PublicKey> &public_keys,
                    const std::vector<std::pair<const uint8_t *, size_t>> &messages, Require require = Require::None,
                    uint64_t *stats_out = nullptr) {
        if (cache.wire()) throw std::invalid_argument("a Wire key cache takes 49-byte keys (push_mixed_wire)");
        const size_t u = public_keys.size();
        const PackedTriples t = pack_triples(std::vector<Signature>(u), public_keys, messages);
        const int rc = ssa_aggverifier_push_mixed_cached(cx_.get(), av_, pool.get(), cache.get(), places.data(), places.size(),
                                                         rs49, t.pks.data(), t.inf.data(), t.flat.data(), t.off.data(), 0, 0, u,
                                                         (uint32_t)require, stats_out);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_push_mixed_cached: ") + ssa_strerror(rc));
    }
    // wire_keys: the unknown lanes' keys side by side, 49 bytes each (messages.size() of them)
    void push_mixed_wire(Aggregator &pool, KeyCache &cache, const std::vector<uint32_t> &places, const uint8_t *rs49,
                         const std::vector<uint8_t> &wire_keys,
                         const std::vector<std::pair<const uint8_t *, size_t>> &messages, Require require = Require::None,
                         uint64_t *stats_out = nullptr) {
        if (!cache.wire()) throw std::invalid_argument("an Affine key cache takes PublicKey objects (push_mixed)");
        const size_t u = messages.size();
        if (wire_keys.size() != u * PUBLIC_KEY_LENGTH) throw Panic("We should have the same number of messages than public keys");
        std::vector<uint8_t> flat;
        std::vector<uint64_t> off(u + 1, 0);
        for (size_t i = 0; i < u; i++) {
            flat.insert(flat.end(), messages[i].first, messages[i].first + messages[i].second);
            off[i + 1] = flat.size();
        }
        flat.push_back(0);
        const int rc = ssa_aggverifier_push_mixed_cached_wire(cx_.get(), av_, pool.get(), cache.get(), places.data(),
                                                              places.size(), u ? rs49 : nullptr, u ? wire_keys.data() : nullptr,
                                                              flat.data(), off.data(), 0, 0, u, (uint32_t)require, stats_out);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_push_mixed_cached_wire: ") + ssa_strerror(rc));
    }
    // every lane of the block is held by the pool
    void push_known(Aggregator &pool, const std::vector<uint32_t> &places) {
        const int rc = ssa_aggverifier_push_known(cx_.get(), av_, pool.get(), places.data(), places.size());
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_push_known: ") + ssa_strerror(rc));
    }
    // the status word: SSA_OK, SSA_INVALID_SIGNATURE or SSA_MALFORMED; SSA_INVALID_PUBLIC_KEY after pushes through a cache
    int finish_status(const uint8_t e_agg[32], size_t n_take = All) const {
        const int rc = ssa_aggverifier_finish(cx_.get(), av_, e_agg, n_take);
        if (rc < 0) throw std::runtime_error(std::string("ssa_aggverifier_finish: ") + ssa_strerror(rc));
        return rc;
    }
    // as AggregateSignature::verify: nullopt (Ok), InvalidSignature, or Panic thrown for a malformed lane or scalar
    Result finish(const uint8_t e_agg[32], size_t n_take = All) const { return status_to_result(finish_status(e_agg, n_take)); }
    void reset() {
        const int rc = ssa_aggverifier_reset(av_);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_reset: ") + ssa_strerror(rc));
    }
    Info info() const {
        uint64_t v[8] = {};
        const int rc = ssa_aggverifier_info(av_, v);
        if (rc != 0) throw std::runtime_error(std::string("ssa_aggverifier_info: ") + ssa_strerror(rc));
        return {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
    }

  private:
    Context &cx_;
    ssa_aggverifier *av_ = nullptr;
};

// AggregateSignature::verify_many through a key cache
namespace detail {
struct PackedAggregates {
    std::vector<uint64_t> counts;
    std::vector<uint8_t> wire;
    size_t n = 0;
};
inline PackedAggregates pack_aggregates(const std::vector<AggregateSignature> &aggregates) {
    PackedAggregates p;
    for (const AggregateSignature &a : aggregates) {
        p.counts.push_back(a.size());
        p.n += a.size();
        p.wire.insert(p.wire.end(), a.bytes.begin(), a.bytes.end());
    }
    return p;
}
// n messages end to end and their n + 1 offsets
struct PackedMessages {
    std::vector<uint8_t> flat;
    std::vector<uint64_t> off;
};
inline PackedMessages pack_messages(const std::vector<std::pair<const uint8_t *, size_t>> &messages) {
    PackedMessages m;
    m.off.assign(messages.size() + 1, 0);
    for (size_t i = 0; i < messages.size(); i++) {
        m.flat.insert(m.flat.end(), messages[i].first, messages[i].first + messages[i].second);
        m.off[i + 1] = m.flat.size();
    }
    m.flat.push_back(0);
    return m;
}
}  // namespace detail

inline std::vector<uint32_t> AggregateSignature::verify_many(Context &cx, KeyCache &cache,
                                                             const std::vector<AggregateSignature> &aggregates,
                                                             const std::vector<PublicKey> &public_keys,
                                                             const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                             uint64_t *stats_out) {
    if (cache.wire()) throw std::invalid_argument("a Wire key cache takes 49-byte keys, not PublicKey objects");
    const detail::PackedAggregates p = detail::pack_aggregates(aggregates);
    if (public_keys.size() != p.n || messages.size() != p.n)
        throw Panic("We should have the same number of messages than public keys");
    std::vector<uint32_t> verdicts(aggregates.size(), SSA_MALFORMED);
    if (aggregates.empty()) return verdicts;
    std::vector<uint8_t> pks(p.n * AFFINE_PUBLIC_KEY_LENGTH + 1), inf(p.n + 1);
    for (size_t i = 0; i < p.n; i++) {
        std::memcpy(&pks[i * AFFINE_PUBLIC_KEY_LENGTH], public_keys[i].affine.data(), AFFINE_PUBLIC_KEY_LENGTH);
        inf[i] = public_keys[i].is_identity ? 1 : 0;
    }
    const detail::PackedMessages m = detail::pack_messages(messages);
    const int rc = ssa_verify_aggregates_many_cached(cx.get(), cache.get(), p.wire.data(), p.counts.data(), p.counts.size(),
                                                     pks.data(), inf.data(), m.flat.data(), m.off.data(), 0, 0,
                                                     verdicts.data(), stats_out);
    if (rc != 0) throw std::runtime_error(std::string("ssa_verify_aggregates_many_cached: ") + ssa_strerror(rc));
    return verdicts;
}

inline std::vector<uint32_t> AggregateSignature::verify_many(Context &cx, KeyCache &cache,
                                                             const std::vector<AggregateSignature> &aggregates,
                                                             const std::vector<uint8_t> &wire_keys,
                                                             const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                             uint64_t *stats_out) {
    if (!cache.wire()) throw std::invalid_argument("an Affine key cache takes PublicKey objects, not 49-byte keys");
    const detail::PackedAggregates p = detail::pack_aggregates(aggregates);
    if (wire_keys.size() != p.n * PUBLIC_KEY_LENGTH || messages.size() != p.n)
        throw Panic("We should have the same number of messages than public keys");
    std::vector<uint32_t> verdicts(aggregates.size(), SSA_MALFORMED);
    if (aggregates.empty()) return verdicts;
    const detail::PackedMessages m = detail::pack_messages(messages);
    const int rc = ssa_verify_aggregates_many_cached_wire(cx.get(), cache.get(), p.wire.data(), p.counts.data(),
                                                          p.counts.size(), wire_keys.data(), m.flat.data(), m.off.data(), 0, 0,
                                                          verdicts.data(), stats_out);
    if (rc != 0) throw std::runtime_error(std::string("ssa_verify_aggregates_many_cached_wire: ") + ssa_strerror(rc));
    return verdicts;
}

// AggregateSignature::aggregate_valid through a key cache
inline std::pair<AggregateSignature, std::vector<uint32_t>>
AggregateSignature::aggregate_valid(Context &cx, KeyCache &cache, const std::vector<Signature> &signatures,
                                    const std::vector<PublicKey> &public_keys,
                                    const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                    std::vector<PublicKey> *kept_keys, uint64_t *stats_out) {
    if (cache.wire()) throw std::invalid_argument("a Wire key cache takes KeyedSignature records, not objects");
    const PackedTriples t = pack_triples(signatures, public_keys, messages);
    const size_t n = signatures.size();
    AggregateSignature a;
    a.bytes.assign(SSA_AGGREGATE_LENGTH(n), 0);
    std::vector<uint32_t> kept(n ? n : 1, 0u);
    std::vector<uint8_t> pks(n * AFFINE_PUBLIC_KEY_LENGTH + 1), inf(n + 1);
    uint64_t n_kept = 0;
    const int rc = ssa_aggregate_valid_many_cached(cx.get(), cache.get(), t.sigs.data(), t.pks.data(), t.inf.data(),
                                                   t.flat.data(), t.off.data(), 0, 0, n, a.bytes.data(), kept.data(), &n_kept,
                                                   nullptr, pks.data(), inf.data(), stats_out);
    if (rc != 0) throw std::runtime_error(std::string("ssa_aggregate_valid_many_cached: ") + ssa_strerror(rc));
    a.bytes.resize(SSA_AGGREGATE_LENGTH(n_kept));
    kept.resize(n_kept);
    if (kept_keys) {
        kept_keys->assign(n_kept, PublicKey{});
        for (size_t i = 0; i < n_kept; i++) {
            std::memcpy((*kept_keys)[i].affine.data(), &pks[i * AFFINE_PUBLIC_KEY_LENGTH], AFFINE_PUBLIC_KEY_LENGTH);
            (*kept_keys)[i].is_identity = inf[i] != 0;
        }
    }
    return {std::move(a), std::move(kept)};
}

inline std::pair<AggregateSignature, std::vector<uint32_t>>
AggregateSignature::aggregate_valid(Context &cx, KeyCache &cache, const std::vector<uint8_t> &keyed_records,
                                    const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                    std::vector<uint8_t> *kept_keys49, uint64_t *stats_out) {
    constexpr size_t RECORD = KEYED_SIGNATURE_LENGTH;
    if (!cache.wire()) throw std::invalid_argument("an Affine key cache takes objects, not KeyedSignature records");
    if (keyed_records.size() % RECORD || keyed_records.size() / RECORD != messages.size())
        throw Panic("We should have the same number of messages than public keys");
    const size_t n = messages.size();
    const detail::PackedMessages m = detail::pack_messages(messages);
    AggregateSignature a;
    a.bytes.assign(SSA_AGGREGATE_LENGTH(n), 0);
    std::vector<uint32_t> kept(n ? n : 1, 0u);
    std::vector<uint8_t> keys(n * PUBLIC_KEY_LENGTH + 1);
    uint64_t n_kept = 0;
    const int rc = ssa_aggregate_valid_keyed_many_cached(cx.get(), cache.get(), keyed_records.data(), m.flat.data(),
                                                         m.off.data(), 0, 0, n, a.bytes.data(), kept.data(), &n_kept, nullptr,
                                                         keys.data(), stats_out);
    if (rc != 0) throw std::runtime_error(std::string("ssa_aggregate_valid_keyed_many_cached: ") + ssa_strerror(rc));
    a.bytes.resize(SSA_AGGREGATE_LENGTH(n_kept));
    kept.resize(n_kept);
    if (kept_keys49) kept_keys49->assign(keys.begin(), keys.begin() + (std::ptrdiff_t)(n_kept * PUBLIC_KEY_LENGTH));
    return {std::move(a), std::move(kept)};
}

// verify_many_screened_statuses with each public key's check done once per cache, not once per slice: byte for byte the
// same vector for the same coefficients, whatever the cache holds.  stats_out: 12 words, optional.
inline std::vector<uint8_t> verify_many_cached_statuses(Context &cx, KeyCache &cache, const std::vector<Signature> &signatures,
                                                        const std::vector<PublicKey> &public_keys,
                                                        const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                        Rng rng = nullptr, uint64_t *stats_out = nullptr) {
    const PackedTriples t = pack_triples(signatures, public_keys, messages);
    const size_t n = signatures.size();
    return statuses_of(n, rng, "ssa_verify_many_cached", [&](uint8_t *status, const uint8_t *coeffs) {
        return ssa_verify_many_cached(cx.get(), cache.get(), t.sigs.data(), t.pks.data(), t.inf.data(), t.flat.data(),
                                      t.off.data(), 0, 0, n, SSA_FLAG_CHECK_TORSION, coeffs, status, nullptr, stats_out);
    });
}

// KeyedSignature::verify (src/signature.rs:232-234) over n wire records of 130 bytes, pk (49) || signature (81), as they
// arrive from the network, through a key cache in Wire mode: a key seen before -- one that does not
// decode included -- is neither decompressed nor checked again.  The statuses of verify_many_cached_statuses on the
// unpacked records, byte for byte for the same coefficients; a record whose key does not decode gets 3.  stats_out: 12
// words, optional.
inline std::vector<uint8_t> verify_keyed_many_cached_statuses(Context &cx, KeyCache &cache, const std::vector<uint8_t> &keyed,
                                                              const std::vector<std::pair<const uint8_t *, size_t>> &messages,
                                                              Rng rng = nullptr, uint64_t *stats_out = nullptr) {
    if (keyed.size() != messages.size() * KEYED_SIGNATURE_LENGTH)
        throw std::invalid_argument("We should have the same number of messages than keyed signatures");
    const size_t n = messages.size();
    std::vector<uint8_t> flat;
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        flat.insert(flat.end(), messages[i].first, messages[i].first + messages[i].second);
        off[i + 1] = flat.size();
    }
    flat.push_back(0);
    return statuses_of(n, rng, "ssa_verify_keyed_many_cached", [&](uint8_t *status, const uint8_t *coeffs) {
        return ssa_verify_keyed_many_cached(cx.get(), cache.get(), keyed.data(), flat.data(), off.data(), 0, 0, n,
                                            SSA_FLAG_CHECK_TORSION, coeffs, status, nullptr, stats_out);
    });
}

// the device forms as they are: n records and n messages of msg_len bytes, side by side, in device memory
inline int verify_keyed_many_cached_device(Context &cx, KeyCache &cache, const uint8_t *d_keyed, const uint8_t *d_msgs,
                                           size_t msg_len, size_t n, uint32_t flags, const uint8_t *d_coeffs,
                                           uint32_t coeff_bytes, uint8_t *d_status_out, uint64_t *d_n_fail_out,
                                           uint64_t *stats_out = nullptr) {
    return ssa_verify_keyed_many_cached_device(cx.get(), cache.get(), d_keyed, d_msgs, nullptr, msg_len, msg_len, n, flags,
                                               d_coeffs, coeff_bytes, d_status_out, d_n_fail_out, stats_out);
}
inline int verify_keyed_many_device(Context &cx, const uint8_t *d_keyed, const uint8_t *d_msgs, size_t msg_len, size_t n,
                                    uint32_t flags, uint8_t *d_status_out, uint64_t *d_n_fail_out) {
    return ssa_verify_keyed_many_device(cx.get(), d_keyed, d_msgs, nullptr, msg_len, msg_len, n, flags, d_status_out,
                                        d_n_fail_out);
}

// ---- hierarchical deterministic key derivation (src/derivation.rs) ---------------------------------------------------
constexpr size_t CHAIN_CODE_LENGTH = SSA_CHAIN_CODE_LENGTH, EXTENDED_PRIVATE_KEY_LENGTH = SSA_EXTENDED_PRIVATE_KEY_LENGTH,
                 EXTENDED_PUBLIC_KEY_LENGTH = SSA_EXTENDED_PUBLIC_KEY_LENGTH;
using Index = std::array<uint8_t, 4>;   // the reference's &[u8; 4], little-endian; hardened when bit 7 of i[3] is set
inline uint32_t index_value(const Index &i) {
    return (uint32_t)i[0] | (uint32_t)i[1] << 8 | (uint32_t)i[2] << 16 | (uint32_t)i[3] << 24;
}
inline void derive_check(int rc, const char *what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + ssa_strerror(rc));
}

struct ChainCode {  // src/derivation.rs:30-31
    std::array<uint8_t, CHAIN_CODE_LENGTH> bytes{};
    bool operator==(const ChainCode &o) const { return bytes == o.bytes; }
};

struct ExtendedPublicKey;

struct ExtendedPrivateKey {  // src/derivation.rs:46-52; wire form sk(32) || cc(32)
    PrivateKey key;
    ChainCode chaincode;
    bool operator==(const ExtendedPrivateKey &o) const { return key == o.key && chaincode == o.chaincode; }
    std::array<uint8_t, EXTENDED_PRIVATE_KEY_LENGTH> to_bytes() const {  // :177-184
        std::array<uint8_t, EXTENDED_PRIVATE_KEY_LENGTH> b{};
        std::memcpy(b.data(), key.bytes.data(), 32);
        std::memcpy(b.data() + 32, chaincode.bytes.data(), 32);
        return b;
    }
    // :187-203: nullopt for a non-canonical or zero key
    static std::optional<ExtendedPrivateKey> from_bytes(const std::array<uint8_t, EXTENDED_PRIVATE_KEY_LENGTH> &b) {
        std::array<uint8_t, PRIVATE_KEY_LENGTH> k{};
        std::memcpy(k.data(), b.data(), 32);
        auto sk = PrivateKey::from_bytes(k);
        if (!sk) return std::nullopt;
        ExtendedPrivateKey x{*sk, {}};
        std::memcpy(x.chaincode.bytes.data(), b.data() + 32, 32);
        return x;
    }
    // :66-82 (ssa_xprv_master_many)
    static std::optional<ExtendedPrivateKey> generate_master_key(Context &cx, const std::array<uint8_t, 32> &seed) {
        std::array<uint8_t, EXTENDED_PRIVATE_KEY_LENGTH> out{};
        uint8_t st = 0xff;
        derive_check(ssa_xprv_master_many(cx.get(), seed.data(), 1, out.data(), &st), "ssa_xprv_master_many");
        if (st != SSA_OK) return std::nullopt;
        return from_bytes(out);
    }
    // :88-154 (ssa_xprv_derive_many): nullopt when the child key is 0
    std::optional<ExtendedPrivateKey> derive_private(Context &cx, const Index &i) const {
        const auto par = to_bytes();
        const uint32_t idx = index_value(i);
        std::array<uint8_t, EXTENDED_PRIVATE_KEY_LENGTH> out{};
        uint8_t st = 0xff;
        derive_check(ssa_xprv_derive_many(cx.get(), par.data(), 1, nullptr, &idx, 1, 0, out.data(), &st),
                     "ssa_xprv_derive_many");
        if (st != SSA_OK) return std::nullopt;
        return from_bytes(out);
    }
    // :160-174 (SSA_FLAG_DERIVE_PUBLIC)
    std::optional<ExtendedPublicKey> derive_public(Context &cx, const Index &i) const;
};

struct ExtendedPublicKey {  // src/derivation.rs:207-213; wire form compressed key(49) || cc(32)
    PublicKey key;
    ChainCode chaincode;
    bool operator==(const ExtendedPublicKey &o) const { return key == o.key && chaincode == o.chaincode; }
    static ExtendedPublicKey from_extended_private_key(Context &cx, const ExtendedPrivateKey &x) {  // :225-230
        return ExtendedPublicKey{PublicKey::from_private(cx, x.key), x.chaincode};
    }
    std::array<uint8_t, EXTENDED_PUBLIC_KEY_LENGTH> to_bytes(Context &cx) const {  // :263-270
        std::array<uint8_t, EXTENDED_PUBLIC_KEY_LENGTH> b{};
        const auto k = key.to_bytes(cx);
        std::memcpy(b.data(), k.data(), PUBLIC_KEY_LENGTH);
        std::memcpy(b.data() + PUBLIC_KEY_LENGTH, chaincode.bytes.data(), 32);
        return b;
    }
    // :273-290: nullopt when decompression fails or for the identity
    static std::optional<ExtendedPublicKey> from_bytes(Context &cx, const std::array<uint8_t, EXTENDED_PUBLIC_KEY_LENGTH> &b) {
        std::array<uint8_t, PUBLIC_KEY_LENGTH> k{};
        std::memcpy(k.data(), b.data(), PUBLIC_KEY_LENGTH);
        auto pk = PublicKey::from_bytes(cx, k);
        if (!pk || pk->is_identity) return std::nullopt;
        ExtendedPublicKey x{*pk, {}};
        std::memcpy(x.chaincode.bytes.data(), b.data() + PUBLIC_KEY_LENGTH, 32);
        return x;
    }
    // :235-260 (ssa_xpub_derive_many): nullopt for a hardened index or T = O; the child may be the identity
    std::optional<ExtendedPublicKey> derive_normal_public(Context &cx, const Index &i) const {
        const auto par = to_bytes(cx);
        const uint32_t idx = index_value(i);
        std::array<uint8_t, EXTENDED_PUBLIC_KEY_LENGTH> out{};
        ExtendedPublicKey child;
        uint8_t inf = 0, st = 0xff;
        derive_check(ssa_xpub_derive_many(cx.get(), par.data(), 1, nullptr, &idx, 1, out.data(), child.key.affine.data(),
                                          &inf, &st), "ssa_xpub_derive_many");
        if (st == SSA_MALFORMED) throw Panic("ExtendedPublicKey does not encode");
        if (st != SSA_OK) return std::nullopt;
        child.key.is_identity = inf != 0;
        std::memcpy(child.chaincode.bytes.data(), out.data() + PUBLIC_KEY_LENGTH, 32);
        return child;
    }
};

inline std::optional<ExtendedPublicKey> ExtendedPrivateKey::derive_public(Context &cx, const Index &i) const {
    const auto par = to_bytes();
    const uint32_t idx = index_value(i);
    std::array<uint8_t, EXTENDED_PUBLIC_KEY_LENGTH> out{};
    uint8_t st = 0xff;
    derive_check(ssa_xprv_derive_many(cx.get(), par.data(), 1, nullptr, &idx, 1, SSA_FLAG_DERIVE_PUBLIC, out.data(), &st),
                 "ssa_xprv_derive_many");
    if (st != SSA_OK) return std::nullopt;
    return ExtendedPublicKey::from_bytes(cx, out);
}

// PrivateKey::derive_private (src/derivation.rs:291-302): the reference unwraps -- Panic on a none child
inline std::pair<PrivateKey, ChainCode> derive_private(Context &cx, const PrivateKey &sk, const ChainCode &cc,
                                                       const Index &i) {
    auto c = ExtendedPrivateKey{sk, cc}.derive_private(cx, i);
    if (!c) throw Panic("derive_private is none (child key 0)");
    return {c->key, c->chaincode};
}
// PublicKey::derive_public (src/derivation.rs:305-316): Panic on a hardened index (the reference's unwrap)
inline std::pair<PublicKey, ChainCode> derive_public(Context &cx, const PublicKey &pk, const ChainCode &cc, const Index &i) {
    auto c = ExtendedPublicKey{pk, cc}.derive_normal_public(cx, i);
    if (!c) throw Panic("derive_normal_public is none (hardened index or T = O)");
    return {c->key, c->chaincode};
}

}  // namespace schnorr_sig
