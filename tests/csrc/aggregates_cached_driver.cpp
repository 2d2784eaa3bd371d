// Driver of tests/test_gpu_aggregates_cached_cxx.py: the key-cache overloads of AggregateSignature::verify_many of the C++
// mirror on one case written by the test, in both cache modes.  Input file: u64 k, k x u64 counts, the aggregates' wire
// bytes end to end, N x 96 key bytes, N identity flags, N x 49 compressed key bytes, N x u64 message lengths, the message
// bytes.  Output file: k x u32 verdicts through an Affine cache, k x u32 through a Wire cache, then each call's 8
// statistics words (u64).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

#include "../../schnorr-sig_amd/host/schnorr_sig.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> d((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    auto need = [&](size_t bytes) {
        if (d.size() - pos < bytes) {
            std::fprintf(stderr, "short input\n");
            std::exit(2);
        }
        const uint8_t *p = d.data() + pos;
        pos += bytes;
        return p;
    };
    auto u64 = [&]() {
        uint64_t v;
        std::memcpy(&v, need(8), 8);
        return v;
    };
    const size_t k = u64();
    std::vector<uint64_t> counts(k);
    size_t n = 0;
    for (auto &c : counts) n += (c = u64());
    std::vector<schnorr_sig::AggregateSignature> aggs(k);
    for (size_t j = 0; j < k; j++) {
        const uint8_t *p = need(SSA_AGGREGATE_LENGTH(counts[j]));
        aggs[j].bytes.assign(p, p + SSA_AGGREGATE_LENGTH(counts[j]));
    }
    std::vector<schnorr_sig::PublicKey> pks(n);
    for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
    for (auto &pk : pks) pk.is_identity = *need(1) != 0;
    const uint8_t *w = need(49 * n);
    const std::vector<uint8_t> wire_keys(w, w + 49 * n);
    std::vector<uint64_t> lens(n);
    for (auto &l : lens) l = u64();
    std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
    for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    try {
        schnorr_sig::Context cx(0);
        schnorr_sig::KeyCache affine(cx, 256), wire(cx, 256, schnorr_sig::KeyCache::Wire);
        uint64_t sa[8] = {}, sw[8] = {};
        const std::vector<uint32_t> va = schnorr_sig::AggregateSignature::verify_many(cx, affine, aggs, pks, msgs, sa);
        const std::vector<uint32_t> vw = schnorr_sig::AggregateSignature::verify_many(cx, wire, aggs, wire_keys, msgs, sw);
        bool refused = false;      // each overload refuses the other mode's cache
        try {
            (void)schnorr_sig::AggregateSignature::verify_many(cx, wire, aggs, pks, msgs);
        } catch (const std::invalid_argument &) {
            refused = true;
        }
        if (!refused) return 3;
        std::ofstream out(argv[2], std::ios::binary);
        out.write((const char *)va.data(), (std::streamsize)(va.size() * sizeof(uint32_t)));
        out.write((const char *)vw.data(), (std::streamsize)(vw.size() * sizeof(uint32_t)));
        out.write((const char *)sa, sizeof sa);
        out.write((const char *)sw, sizeof sw);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
