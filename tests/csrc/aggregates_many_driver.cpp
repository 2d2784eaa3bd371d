// Driver of tests/test_gpu_aggregates_many_cxx.py: AggregateSignature::verify_many of the C++ mirror on one case written by
// the test.  Input file: u64 k, k x u64 counts, the aggregates' wire bytes end to end, N x 96 key bytes, N identity flags,
// N x u64 message lengths, the message bytes.  Output file: k x u32 verdicts.
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
    std::vector<uint64_t> lens(n);
    for (auto &l : lens) l = u64();
    std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
    for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    try {
        schnorr_sig::Context cx(0);
        const std::vector<uint32_t> v = schnorr_sig::AggregateSignature::verify_many(cx, aggs, pks, msgs);
        std::ofstream out(argv[2], std::ios::binary);
        out.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(uint32_t)));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
