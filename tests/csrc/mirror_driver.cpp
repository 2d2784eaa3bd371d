// Replay tool for the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp): `mirror_driver <scenario file> <output file>`.
// tests/test_gpu_cxx_mirror.py writes a scenario -- a list of steps, each a name and byte-string arguments -- this program
// performs every step through the mirror's classes and writes what came back; the test compares it byte for byte with the
// oracle, the models and the Python mirror.  Nothing is judged here.
//   g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include mirror_driver.cpp -L../../schnorr-sig_amd/csrc
//       -lschnorr_sig_amd -L/opt/rocm/lib -lamdhip64 -o mirror_driver
// (the HIP runtime only for the device buffers of the two *_device pass-throughs; the one raw ssa_* call is the rng pin)
//
// Both files: records of  u32 name length, name, u32 number of blobs, then per blob u64 length and the bytes.
// An output record answers the step of the same position: blob 0 is one byte -- 0 returned, 1 Panic, 2
// std::invalid_argument, 3 any other std::runtime_error -- blob 1 the exception's text, blob 2 the bytes the replaying Rng
// handed out during the step (u64), the rest is the step's own results.  A missing optional is the single byte 0, a
// present one the byte 1 followed by its blobs; a Result is one byte: 0 Ok, 1 InvalidPublicKey, 2 InvalidSignature.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <fstream>
#include <memory>

#include "../../schnorr-sig_amd/host/schnorr_sig.hpp"

using namespace schnorr_sig;
using Blob = std::vector<uint8_t>;
using Msgs = std::vector<std::pair<const uint8_t *, size_t>>;

struct Record {
    std::string name;
    std::vector<Blob> blobs;
};

static bool read_record(std::istream &in, Record &r) {
    uint32_t len = 0, nb = 0;
    if (!in.read((char *)&len, 4)) return false;
    r.name.resize(len);
    in.read(&r.name[0], len);
    in.read((char *)&nb, 4);
    r.blobs.assign(nb, {});
    for (auto &b : r.blobs) {
        uint64_t l = 0;
        in.read((char *)&l, 8);
        b.resize(l);
        if (l) in.read((char *)b.data(), (std::streamsize)l);
    }
    if (!in) throw std::runtime_error("truncated scenario");
    return true;
}
static void write_record(std::ostream &out, const Record &r) {
    const uint32_t len = (uint32_t)r.name.size(), nb = (uint32_t)r.blobs.size();
    out.write((const char *)&len, 4);
    out.write(r.name.data(), len);
    out.write((const char *)&nb, 4);
    for (const auto &b : r.blobs) {
        const uint64_t l = b.size();
        out.write((const char *)&l, 8);
        if (l) out.write((const char *)b.data(), (std::streamsize)l);
    }
}

template <class V>
static Blob blob(const V &v) { return Blob(v.begin(), v.end()); }
static Blob words(const uint64_t *w, size_t n) { return Blob((const uint8_t *)w, (const uint8_t *)(w + n)); }
static Blob byte(unsigned v) { return Blob(1, (uint8_t)v); }
static Blob key_blob(const PublicKey &p) {   // affine(96) || identity flag
    Blob b = blob(p.affine);
    b.push_back(p.is_identity ? 1 : 0);
    return b;
}
static Blob result_blob(const Result &r) { return byte(r ? (unsigned)*r : 0u); }
template <size_t N>
static std::array<uint8_t, N> fixed(const Blob &b) {
    if (b.size() != N) throw std::logic_error("scenario: a blob of the wrong length");
    std::array<uint8_t, N> a;
    std::copy(b.begin(), b.end(), a.begin());
    return a;
}
static uint64_t u64_of(const Blob &b) {
    uint64_t v = 0;
    std::memcpy(&v, b.data(), std::min<size_t>(8, b.size()));
    return v;
}
static void hip_ok(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::logic_error(std::string(what) + ": " + hipGetErrorString(e));
}

struct State {
    Context cx{0};
    Blob stream;          // what the replaying Rng hands out
    size_t pos = 0;
    Rng rng = [this](uint8_t *p, size_t n) {
        if (pos + n > stream.size()) throw std::logic_error("scenario: rng stream exhausted");
        std::memcpy(p, stream.data() + pos, n);
        pos += n;
    };
    KeyPair kp;
    std::unique_ptr<SignerSet> ss;
    std::vector<uint32_t> idx;
    std::vector<Signature> sigs;
    std::vector<PublicKey> pks;
    Blob flat, keyed;
    Msgs msgs;
    std::unique_ptr<KeyCache> kc;
    std::unique_ptr<KeySet> ks;
    AggregateSignature agg;
    ExtendedPrivateKey xprv;
    ExtendedPublicKey xpub;
};

static void put_keyed(State &s, std::vector<Blob> &o, const KeyedSignature &k) {
    o.push_back(key_blob(k.public_key));
    o.push_back(blob(k.signature.bytes));
    o.push_back(blob(k.to_bytes(s.cx)));
}
static void put_keycheck(std::vector<Blob> &o, const KeyCheck &k) {
    const uint64_t w[8] = {k.keys_checked, k.keys_bad, k.first_bad_key, k.ladder_entries_checked, k.comb_rows_checked,
                           k.keys_rebuilt_and_compared, k.combs_skipped, k.rows_repaired};
    o.push_back(words(w, 8));
    o.push_back(byte(k.ok));
    o.push_back(k.bad);
}
static void put_xprv(std::vector<Blob> &o, const std::optional<ExtendedPrivateKey> &x) {
    o.push_back(byte(x.has_value()));
    if (x) o.push_back(blob(x->to_bytes()));
}
static void put_xpub(State &s, std::vector<Blob> &o, const std::optional<ExtendedPublicKey> &x) {
    o.push_back(byte(x.has_value()));
    if (x) o.push_back(blob(x->to_bytes(s.cx)));
}

// a: the step's arguments; o: its results
static void step(State &s, const std::string &op, const std::vector<Blob> &a, std::vector<Blob> &o) {
    const uint8_t *m = a.size() ? a[0].data() : nullptr;
    const size_t ml = a.size() ? a[0].size() : 0;
    // ---- inputs ---------------------------------------------------------------------------------------------------
    if (op == "rng") {
        s.stream = a[0];
        s.pos = 0;
    } else if (op == "pin") {
        const int rc = ssa_debug_pin_rng(s.cx.get(), a[0].empty() ? nullptr : a[0].data());
        if (rc != 0) throw std::logic_error("ssa_debug_pin_rng failed");
    } else if (op == "sigs") {
        s.sigs.assign(a[0].size() / SIGNATURE_LENGTH, {});
        for (size_t i = 0; i < s.sigs.size(); i++) std::memcpy(s.sigs[i].bytes.data(), &a[0][i * SIGNATURE_LENGTH], SIGNATURE_LENGTH);
    } else if (op == "pks") {   // n x 96 affine bytes, n identity flags
        s.pks.assign(a[1].size(), {});
        for (size_t i = 0; i < s.pks.size(); i++) {
            std::memcpy(s.pks[i].affine.data(), &a[0][i * AFFINE_PUBLIC_KEY_LENGTH], AFFINE_PUBLIC_KEY_LENGTH);
            s.pks[i].is_identity = a[1][i] != 0;
        }
    } else if (op == "msgs") {   // n + 1 offsets (u64), the bytes
        s.flat = a[1];
        s.flat.push_back(0);     // (so that an empty list of bytes still has an address)
        s.msgs.clear();
        for (size_t i = 0; i + 1 < a[0].size() / 8; i++) {
            uint64_t lo, hi;
            std::memcpy(&lo, &a[0][8 * i], 8);
            std::memcpy(&hi, &a[0][8 * i + 8], 8);
            s.msgs.push_back({s.flat.data() + lo, (size_t)(hi - lo)});
        }
    } else if (op == "idx") {
        s.idx.assign(a[0].size() / 4, 0);
        if (!s.idx.empty()) std::memcpy(s.idx.data(), a[0].data(), a[0].size());
    } else if (op == "keyed") {
        s.keyed = a[0];
        // ---- key pairs and single signatures ------------------------------------------------------------------------
    } else if (op == "kp_create") {
        s.kp = KeyPair::create(s.cx, s.rng);
        o.push_back(blob(s.kp.to_bytes()));
        o.push_back(key_blob(s.kp.public_key));
    } else if (op == "kp_from_bytes") {
        const auto k = KeyPair::from_bytes(s.cx, fixed<32>(a[0]));
        o.push_back(byte(k.has_value()));
        if (k) {
            s.kp = *k;
            o.push_back(key_blob(k->public_key));
        }
    } else if (op == "kp_sign") {
        o.push_back(blob(s.kp.sign(s.cx, m, ml, s.rng).to_bytes()));
    } else if (op == "kp_sign_bind") {
        put_keyed(s, o, s.kp.sign_and_bind_pkey(s.cx, m, ml, s.rng));
    } else if (op == "sk_sign") {
        o.push_back(blob(s.kp.private_key.sign(s.cx, m, ml, s.rng).to_bytes()));
    } else if (op == "sk_sign_bind") {
        put_keyed(s, o, s.kp.private_key.sign_and_bind_pkey(s.cx, m, ml, s.rng));
    } else if (op == "kp_sign_dev") {
        o.push_back(blob(s.kp.sign(s.cx, m, ml, device_rng).to_bytes()));
    } else if (op == "kp_sign_bind_dev") {
        put_keyed(s, o, s.kp.sign_and_bind_pkey(s.cx, m, ml, device_rng));
    } else if (op == "sk_sign_dev") {
        o.push_back(blob(s.kp.private_key.sign(s.cx, m, ml, device_rng).to_bytes()));
    } else if (op == "sk_sign_bind_dev") {
        put_keyed(s, o, s.kp.private_key.sign_and_bind_pkey(s.cx, m, ml, device_rng));
    } else if (op == "keyed_from_bytes") {
        const auto k = KeyedSignature::from_bytes(s.cx, fixed<KEYED_SIGNATURE_LENGTH>(a[0]));
        o.push_back(byte(k.has_value()));
        if (k) put_keyed(s, o, *k);
        // ---- signer sets ----------------------------------------------------------------------------------------------
    } else if (op == "ss_pairs") {   // m x 32 secret keys -> KeyPair::from_bytes each -> SignerSet(cx, pairs)
        std::vector<KeyPair> pairs;
        for (size_t i = 0; i < a[0].size() / 32; i++) {
            std::array<uint8_t, 32> b;
            std::memcpy(b.data(), &a[0][32 * i], 32);
            pairs.push_back(*KeyPair::from_bytes(s.cx, b));
        }
        s.ss.reset();
        s.ss = std::make_unique<SignerSet>(s.cx, pairs);
        o.push_back(words(std::array<uint64_t, 1>{s.ss->size()}.data(), 1));
    } else if (op == "ss_generate") {
        s.ss.reset();
        s.ss = std::make_unique<SignerSet>(s.cx, (size_t)u64_of(a[0]), device_rng);
        o.push_back(words(std::array<uint64_t, 1>{s.ss->size()}.data(), 1));
    } else if (op == "ss_secret_keys") {
        Blob b;
        for (const auto &k : s.ss->secret_keys()) b.insert(b.end(), k.begin(), k.end());
        o.push_back(b);
    } else if (op == "ss_public_keys") {
        Blob b;
        for (const auto &p : s.ss->public_keys()) {
            const Blob k = key_blob(p);
            b.insert(b.end(), k.begin(), k.end());
        }
        o.push_back(b);
    } else if (op == "ss_sign" || op == "ss_sign_dev") {
        Blob b;
        for (const auto &g : op == "ss_sign" ? s.ss->sign(s.idx, s.msgs, s.rng) : s.ss->sign(s.idx, s.msgs, device_rng))
            b.insert(b.end(), g.bytes.begin(), g.bytes.end());
        o.push_back(b);
    } else if (op == "ss_sign_bind" || op == "ss_sign_bind_dev") {
        Blob keys, sg;
        for (const auto &k : op == "ss_sign_bind" ? s.ss->sign_and_bind_pkey(s.idx, s.msgs, s.rng)
                                                   : s.ss->sign_and_bind_pkey(s.idx, s.msgs, device_rng)) {
            const Blob kb = key_blob(k.public_key);
            keys.insert(keys.end(), kb.begin(), kb.end());
            sg.insert(sg.end(), k.signature.bytes.begin(), k.signature.bytes.end());
        }
        o.push_back(keys);
        o.push_back(sg);
        // ---- status vectors -------------------------------------------------------------------------------------------
    } else if (op == "verify_many_statuses") {
        uint64_t st[4] = {};
        o.push_back(verify_many_statuses(s.cx, s.sigs, s.pks, s.msgs, st));
        o.push_back(words(st, 4));
    } else if (op == "verify_many_screened_statuses") {   // a[0]: 1 = coefficients from the replayed Rng, 0 = nullptr
        uint64_t st[8] = {};
        o.push_back(verify_many_screened_statuses(s.cx, s.sigs, s.pks, s.msgs, a[0][0] ? s.rng : Rng(nullptr), st));
        o.push_back(words(st, 8));
    } else if (op == "verify_batch_statuses") {
        o.push_back(verify_batch_statuses(s.cx, s.sigs, s.pks, s.msgs, a[0][0] ? s.rng : Rng(nullptr)));
    } else if (op == "verify_batch") {                    // a[0]: rng or not, a[1]: msm or not
        o.push_back(result_blob(verify_batch(s.cx, s.sigs, s.pks, s.msgs, a[0][0] ? s.rng : Rng(nullptr), a[1][0] != 0)));
        // ---- key caches -----------------------------------------------------------------------------------------------
    } else if (op == "kc_create") {   // capacity (u64), 1 = Wire
        s.kc.reset();
        s.kc = std::make_unique<KeyCache>(s.cx, (size_t)u64_of(a[0]), a[1][0] ? KeyCache::Wire : KeyCache::Affine);
        o.push_back(byte(s.kc->wire()));
    } else if (op == "kc_info") {
        const KeyCache::Info i = s.kc->info();
        const uint64_t w[4] = {i.capacity, i.held, i.clears, i.device_bytes};
        o.push_back(words(w, 4));
    } else if (op == "kc_clear") {
        s.kc->clear();
    } else if (op == "kc_set_eviction") {   // by NAME, so that the enumerators' values are under test
        s.kc->set_eviction(a[0][0] == 'R' ? KeyCache::Recent : KeyCache::Clear);
    } else if (op == "kc_eviction_info") {
        const KeyCache::EvictionInfo i = s.kc->eviction_info();
        const uint64_t w[6] = {i.policy, i.compactions, i.dropped, i.last_kept, i.last_moved, i.epoch};
        o.push_back(words(w, 6));
    } else if (op == "kc_selfcheck") {
        put_keycheck(o, s.kc->selfcheck(a[0][0] != 0, a[1][0] != 0));
    } else if (op == "verify_many_cached_statuses") {
        uint64_t st[12] = {};
        o.push_back(verify_many_cached_statuses(s.cx, *s.kc, s.sigs, s.pks, s.msgs, a[0][0] ? s.rng : Rng(nullptr), st));
        o.push_back(words(st, 12));
    } else if (op == "verify_keyed_many_cached_statuses") {
        uint64_t st[12] = {};
        o.push_back(verify_keyed_many_cached_statuses(s.cx, *s.kc, s.keyed, s.msgs, a[0][0] ? s.rng : Rng(nullptr), st));
        o.push_back(words(st, 12));
    } else if (op == "verify_keyed_many_device" || op == "verify_keyed_many_cached_device") {
        // a[0]: n x msg_len message bytes side by side, a[1]: msg_len (u64), a[2]: flags (u64); the records are `keyed`
        const size_t n = s.keyed.size() / KEYED_SIGNATURE_LENGTH, msg_len = (size_t)u64_of(a[1]);
        uint8_t *d_keyed = nullptr, *d_msgs = nullptr, *d_status = nullptr;
        uint64_t *d_nfail = nullptr, nfail = ~0ull, st[12] = {};
        Blob status(n, 0xee);
        hip_ok(hipMalloc((void **)&d_keyed, s.keyed.size()), "hipMalloc");
        hip_ok(hipMalloc((void **)&d_msgs, a[0].size() + 1), "hipMalloc");
        hip_ok(hipMalloc((void **)&d_status, n), "hipMalloc");
        hip_ok(hipMalloc((void **)&d_nfail, 8), "hipMalloc");
        hip_ok(hipMemcpy(d_keyed, s.keyed.data(), s.keyed.size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_ok(hipMemcpy(d_msgs, a[0].data(), a[0].size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_ok(hipMemcpy(d_status, status.data(), n, hipMemcpyHostToDevice), "hipMemcpy");
        hip_ok(hipMemcpy(d_nfail, &nfail, 8, hipMemcpyHostToDevice), "hipMemcpy");
        const int rc = op == "verify_keyed_many_device"
                           ? verify_keyed_many_device(s.cx, d_keyed, d_msgs, msg_len, n, (uint32_t)u64_of(a[2]), d_status, d_nfail)
                           : verify_keyed_many_cached_device(s.cx, *s.kc, d_keyed, d_msgs, msg_len, n, (uint32_t)u64_of(a[2]),
                                                             nullptr, 0, d_status, d_nfail, st);
        // the results are ordered on the context's own stream, a non-blocking one that a plain hipMemcpy does not wait for
        hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_ok(hipMemcpy(status.data(), d_status, n, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_ok(hipMemcpy(&nfail, d_nfail, 8, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_ok(hipFree(d_keyed), "hipFree");
        hip_ok(hipFree(d_msgs), "hipFree");
        hip_ok(hipFree(d_status), "hipFree");
        hip_ok(hipFree(d_nfail), "hipFree");
        const uint64_t w[2] = {(uint64_t)(int64_t)rc, nfail};
        o.push_back(words(w, 2));
        o.push_back(status);
        o.push_back(words(st, 12));
        // ---- aggregates -----------------------------------------------------------------------------------------------
    } else if (op == "aggregate") {
        const auto g = AggregateSignature::aggregate(s.cx, s.sigs, s.pks, s.msgs, a[0][0] != 0);
        o.push_back(byte(g.has_value()));
        if (g) {
            s.agg = *g;
            o.push_back(g->to_bytes());
            o.push_back(words(std::array<uint64_t, 1>{g->size()}.data(), 1));
        }
    } else if (op == "agg_from_bytes") {
        const auto g = AggregateSignature::from_bytes(a[0]);
        o.push_back(byte(g.has_value()));
        if (g) s.agg = *g;
    } else if (op == "agg_set_bytes") {   // the struct's public member, no check
        s.agg.bytes = a[0];
    } else if (op == "agg_verify") {
        o.push_back(result_blob(s.agg.verify(s.cx, s.pks, s.msgs)));
        // ---- self-checks ----------------------------------------------------------------------------------------------
    } else if (op == "ctx_selfcheck") {
        const SelfCheck c = s.cx.selfcheck();
        const uint64_t w[8] = {c.rows, c.bad, c.first_bad, c.ctab_rows, c.ctab_bad, c.ctab_first_bad, c.builds, c.bits};
        o.push_back(words(w, 8));
        o.push_back(byte(c.ok));
    } else if (op == "keyset_create") {   // of the current keys; a[0]: 'L' ladder, 'C' comb, else auto
        s.ks.reset();
        s.ks = std::make_unique<KeySet>(s.cx, s.pks, a[0][0] == 'L' ? SSA_KEYSET_LADDER : a[0][0] == 'C' ? SSA_KEYSET_COMB : SSA_KEYSET_AUTO);
        o.push_back(words(std::array<uint64_t, 1>{s.ks->size()}.data(), 1));
    } else if (op == "keyset_selfcheck") {
        put_keycheck(o, s.ks->selfcheck(a[0][0] != 0));
        // ---- derivation -----------------------------------------------------------------------------------------------
    } else if (op == "xprv_master") {
        const auto x = ExtendedPrivateKey::generate_master_key(s.cx, fixed<32>(a[0]));
        if (x) s.xprv = *x;
        put_xprv(o, x);
    } else if (op == "xprv_from_bytes") {
        const auto x = ExtendedPrivateKey::from_bytes(fixed<EXTENDED_PRIVATE_KEY_LENGTH>(a[0]));
        if (x) s.xprv = *x;
        put_xprv(o, x);
    } else if (op == "xprv_derive_private") {   // the current xprv moves to the child
        const auto x = s.xprv.derive_private(s.cx, fixed<4>(a[0]));
        if (x) s.xprv = *x;
        put_xprv(o, x);
    } else if (op == "xprv_derive_public") {    // the current xprv stays; the child becomes the current xpub
        const auto x = s.xprv.derive_public(s.cx, fixed<4>(a[0]));
        if (x) s.xpub = *x;
        put_xpub(s, o, x);
    } else if (op == "xpub_from_xprv") {
        s.xpub = ExtendedPublicKey::from_extended_private_key(s.cx, s.xprv);
        put_xpub(s, o, s.xpub);
    } else if (op == "xpub_derive_normal_public") {   // the current xpub moves to the child
        const auto x = s.xpub.derive_normal_public(s.cx, fixed<4>(a[0]));
        if (x) s.xpub = *x;
        put_xpub(s, o, x);
    } else if (op == "xpub_from_bytes") {
        const auto x = ExtendedPublicKey::from_bytes(s.cx, fixed<EXTENDED_PUBLIC_KEY_LENGTH>(a[0]));
        if (x) s.xpub = *x;
        put_xpub(s, o, x);
        if (x) {   // the decoded key, and whether decoding its own encoding gives an equal object
            o.push_back(key_blob(x->key));
            const auto again = ExtendedPublicKey::from_bytes(s.cx, x->to_bytes(s.cx));
            o.push_back(byte(again && *again == *x && again->chaincode == x->chaincode));
        }
    } else if (op == "free_derive_private") {   // PrivateKey::derive_private on the current xprv's two halves
        const auto c = derive_private(s.cx, s.xprv.key, s.xprv.chaincode, fixed<4>(a[0]));
        o.push_back(blob(c.first.to_bytes()));
        o.push_back(blob(c.second.bytes));
    } else if (op == "free_derive_public") {    // PublicKey::derive_public on the current xpub's two halves
        const auto c = derive_public(s.cx, s.xpub.key, s.xpub.chaincode, fixed<4>(a[0]));
        o.push_back(blob(c.first.to_bytes(s.cx)));
        o.push_back(blob(c.second.bytes));
    } else {
        throw std::logic_error("scenario: unknown step " + op);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: mirror_driver <scenario file> <output file>\n");
        return 2;
    }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        std::ofstream out(argv[2], std::ios::binary);
        if (!in || !out) throw std::logic_error("cannot open the scenario or the output file");
        State s;
        Record r;
        while (read_record(in, r)) {
            Record res;
            res.name = r.name;
            std::vector<Blob> o;
            unsigned outcome = 0;
            std::string what;
            const size_t before = s.pos;
            try {
                step(s, r.name, r.blobs, o);
            } catch (const Panic &e) {
                outcome = 1, what = e.what();
            } catch (const std::invalid_argument &e) {
                outcome = 2, what = e.what();
            } catch (const std::runtime_error &e) {
                outcome = 3, what = e.what();
            }
            if (outcome) o.clear();
            const uint64_t used = r.name == "rng" ? 0 : s.pos - before;
            res.blobs = {byte(outcome), Blob(what.begin(), what.end()), words(&used, 1)};
            res.blobs.insert(res.blobs.end(), o.begin(), o.end());
            write_record(out, res);
        }
        out.flush();
        if (!out) throw std::logic_error("writing the output failed");
    } catch (const std::exception &e) {   // a scenario or set-up mistake, not a result
        std::fprintf(stderr, "mirror_driver: %s\n", e.what());
        return 3;
    }
    std::printf("mirror_driver done\n");
    return 0;
}
