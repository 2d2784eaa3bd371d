// Driver of tests/test_gpu_aggregate_sliced_cxx.py: AggregateSignature::aggregate_sliced / verify_sliced of the C++ mirror
// on one case written by the test.  Input file: u64 n, n x 81 signature bytes, n x 96 key bytes, n identity flags, n x u64
// message lengths, the message bytes.  Output file: the aggregate (49 n + 32 bytes), then two u32: the status verify_sliced
// gives the aggregate, and the one it gives the aggregate with its first two R's swapped (0 Ok, 2 InvalidSignature).
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
    const size_t n = u64();
    std::vector<schnorr_sig::Signature> sigs(n);
    for (auto &s : sigs) std::memcpy(s.bytes.data(), need(81), 81);
    std::vector<schnorr_sig::PublicKey> pks(n);
    for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
    for (auto &pk : pks) pk.is_identity = *need(1) != 0;
    std::vector<uint64_t> lens(n);
    for (auto &l : lens) l = u64();
    std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
    for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    auto status = [](const schnorr_sig::Result &r) { return r ? (uint32_t)*r : 0u; };
    try {
        schnorr_sig::Context cx(0);
        const auto agg = schnorr_sig::AggregateSignature::aggregate_sliced(cx, sigs, pks, msgs);
        if (!agg) {
            std::fprintf(stderr, "aggregate_sliced refused an honest batch\n");
            return 1;
        }
        uint32_t v[2] = {status(agg->verify_sliced(cx, pks, msgs)), 0u};
        schnorr_sig::AggregateSignature swapped = *agg;
        if (n >= 2) std::swap_ranges(swapped.bytes.begin(), swapped.bytes.begin() + 49, swapped.bytes.begin() + 49);
        v[1] = status(swapped.verify_sliced(cx, pks, msgs));
        std::ofstream out(argv[2], std::ios::binary);
        out.write((const char *)agg->bytes.data(), (std::streamsize)agg->bytes.size());
        out.write((const char *)v, sizeof v);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
