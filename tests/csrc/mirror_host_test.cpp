// The host-only arithmetic and marshalling of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp), run for real: a
// line-driven tool that tests/test_cxx_mirror_host.py feeds with cases and whose answers it compares with Python integers.
// It links WITHOUT the library (the functions used here reach no ssa_* entry point but the error-string lookup, which is
// stubbed below), so it runs without a GPU and under the sanitizers:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all mirror_host_test.cpp -o mirror_host_test
//
// stdin: one case per line, `op arg...`, byte strings in hex ("-" for the empty string); stdout: one answer line per case.
#include <cstdio>
#include <iostream>
#include <sstream>

#include "../../schnorr-sig_amd/host/schnorr_sig.hpp"

// status_to_result names an ABI error through the library; the stand-in keeps this program free of it
extern "C" const char *ssa_strerror(int code) { return code < 0 ? "stub-abi-error" : "stub-status"; }

using namespace schnorr_sig;

static std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    if (s.size() % 2) throw std::invalid_argument("odd hex");
    for (size_t i = 0; i < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return out;
}
static std::string hex(const uint8_t *p, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) {
        s.push_back(d[p[i] >> 4]);
        s.push_back(d[p[i] & 15]);
    }
    return n ? s : "-";
}
template <class V>
static std::string hex(const V &v) { return hex(v.data(), v.size()); }
template <size_t N>
static std::array<uint8_t, N> fixed(const std::string &s) {
    const auto v = unhex(s);
    if (v.size() != N) throw std::invalid_argument("wrong length for " + std::to_string(N) + " bytes");
    std::array<uint8_t, N> a;
    std::copy(v.begin(), v.end(), a.begin());
    return a;
}

static std::string one_case(std::istringstream &in, const std::string &op) {
    std::string a;
    if (op == "reduce") {
        in >> a;
        const auto w = fixed<64>(a);
        uint64_t r[4];
        reduce_wide_mod_q(w.data(), r);
        uint8_t b[32];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 8; j++) b[8 * i + j] = (uint8_t)(r[i] >> (8 * j));
        return hex(b, 32);
    }
    if (op == "seed") {
        in >> a;
        const auto k = PrivateKey::from_seed(fixed<64>(a));
        return k ? hex(k->to_bytes()) : "none";
    }
    if (op == "skbytes") {
        in >> a;
        const auto k = PrivateKey::from_bytes(fixed<32>(a));
        return k ? hex(k->to_bytes()) : "none";
    }
    if (op == "xprv") {
        in >> a;
        const auto x = ExtendedPrivateKey::from_bytes(fixed<64>(a));
        if (!x) return "none";
        const auto again = ExtendedPrivateKey::from_bytes(x->to_bytes());
        if (!again || !(*again == *x)) return "round trip differs";
        return hex(x->to_bytes()) + " " + hex(x->key.bytes) + " " + hex(x->chaincode.bytes);
    }
    if (op == "rand") {   // one KeyPair::random_scalar under an Rng that replays the stream and counts what it hands out
        in >> a;
        const auto stream = unhex(a);
        size_t pos = 0;
        Rng rng = [&](uint8_t *p, size_t n) {
            if (pos + n > stream.size()) throw std::out_of_range("rng stream exhausted");
            std::memcpy(p, stream.data() + pos, n);
            pos += n;
        };
        uint8_t sc[32];
        KeyPair::random_scalar(rng, sc);
        return hex(sc, 32) + " " + std::to_string(pos);
    }
    if (op == "agg") {
        in >> a;
        const auto b = unhex(a);
        const auto g = AggregateSignature::from_bytes(b);
        if (!g) return "none";
        return std::to_string(g->size()) + " " + hex(g->to_bytes());
    }
    if (op == "index") {
        in >> a;
        return std::to_string(index_value(fixed<4>(a)));
    }
    if (op == "status") {
        int st = 0;
        in >> st;
        try {
            const Result r = status_to_result(st);
            if (!r) return "ok";
            return std::string(*r == SignatureError::InvalidPublicKey ? "InvalidPublicKey|" : "InvalidSignature|") + to_string(*r);
        } catch (const Panic &e) {
            return std::string("panic|") + e.what();
        } catch (const std::runtime_error &e) {
            return std::string("runtime_error|") + e.what();
        }
    }
    if (op == "pack") {   // pack ns nk nm, then ns signatures, nk keys as affine:identity-flag, nm messages
        size_t ns = 0, nk = 0, nm = 0;
        in >> ns >> nk >> nm;
        std::vector<Signature> sigs(ns);
        std::vector<PublicKey> pks(nk);
        std::vector<std::vector<uint8_t>> store(nm);
        std::vector<std::pair<const uint8_t *, size_t>> msgs;
        for (auto &s : sigs) {
            in >> a;
            s.bytes = fixed<81>(a);
        }
        for (auto &p : pks) {
            in >> a;
            p.affine = fixed<96>(a.substr(0, 192));
            p.is_identity = a.substr(192) == ":1";
        }
        for (auto &m : store) {
            in >> a;
            m = unhex(a);
            msgs.push_back({m.data(), m.size()});
        }
        try {
            const PackedTriples t = pack_triples(sigs, pks, msgs);
            std::string off;
            for (uint64_t o : t.off) off += (off.empty() ? "" : ",") + std::to_string(o);
            return "sigs=" + hex(t.sigs) + " pks=" + hex(t.pks) + " inf=" + hex(t.inf) + " off=" + off + " flat=" + hex(t.flat);
        } catch (const Panic &e) {
            return std::string("panic|") + e.what();
        }
    }
    throw std::invalid_argument("unknown op " + op);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string op;
        in >> op;
        std::string out;
        try {
            out = one_case(in, op);
        } catch (const std::exception &e) {
            std::printf("ERROR %s: %s\n", op.c_str(), e.what());
            return 2;
        }
        std::printf("%s\n", out.c_str());
    }
    std::printf("done\n");
    return 0;
}
