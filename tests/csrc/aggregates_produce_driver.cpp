// Driver of tests/test_gpu_aggregates_produce_cxx.py: AggregateSignature::aggregate_many of the C++ mirror on one case
// written by the test.  Input file: u64 k, k x u64 counts, u64 check, N x 81 signature bytes, N x 96 key bytes, N identity
// flags, N x u64 message lengths, the message bytes.  Output file: k x u32 results, then the aggregates end to end (a
// refused one as 49 n_j + 32 zero bytes).
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
    const bool check = u64() != 0;
    std::vector<schnorr_sig::Signature> sigs(n);
    for (auto &s : sigs) std::memcpy(s.bytes.data(), need(81), 81);
    std::vector<schnorr_sig::PublicKey> pks(n);
    for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
    for (auto &pk : pks) pk.is_identity = *need(1) != 0;
    std::vector<uint64_t> lens(n);
    for (auto &l : lens) l = u64();
    std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
    for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    try {
        schnorr_sig::Context cx(0);
        std::vector<uint32_t> results;
        const auto aggs = schnorr_sig::AggregateSignature::aggregate_many(cx, counts, sigs, pks, msgs, check, &results);
        std::ofstream out(argv[2], std::ios::binary);
        out.write((const char *)results.data(), (std::streamsize)(results.size() * sizeof(uint32_t)));
        for (size_t j = 0; j < k; j++) {
            const std::vector<uint8_t> zero(SSA_AGGREGATE_LENGTH(counts[j]), 0);
            const std::vector<uint8_t> &b = aggs[j] ? aggs[j]->bytes : zero;
            out.write((const char *)b.data(), (std::streamsize)b.size());
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
