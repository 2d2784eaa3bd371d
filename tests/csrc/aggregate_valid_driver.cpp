// Driver of tests/test_gpu_aggregate_valid_cxx.py: AggregateSignature::aggregate_valid of the C++ mirror on one case written
// by the test.  Input file: u64 n, n x 81 signature bytes, n x 96 key bytes, n identity flags, n x u64 message lengths, the
// message bytes.  Output file: u64 |K|, |K| x u32 kept lanes, the aggregate's 49 |K| + 32 bytes.
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
    try {
        schnorr_sig::Context cx(0);
        const auto r = schnorr_sig::AggregateSignature::aggregate_valid(cx, sigs, pks, msgs);
        const uint64_t m = r.second.size();
        std::ofstream out(argv[2], std::ios::binary);
        out.write((const char *)&m, sizeof m);
        out.write((const char *)r.second.data(), (std::streamsize)(m * sizeof(uint32_t)));
        out.write((const char *)r.first.bytes.data(), (std::streamsize)r.first.bytes.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
