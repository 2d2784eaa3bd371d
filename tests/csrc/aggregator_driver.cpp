// Driver of tests/test_gpu_aggregator_cxx.py: schnorr_sig::Aggregator of the C++ mirror on one case written by the test.
// Input file: u64 n, u64 screen (0 / 1), u64 block_lanes, u64 k, k x u64 push sizes (their sum is n), n x 81 signature
// bytes, n x 96 key bytes, n identity flags, n x u64 message lengths, the message bytes.  Output file: per push its n_j
// status bytes and u64 kept count; then the eight info words, the aggregate of all held lanes (49 held + 32 bytes) and the
// aggregate of the first held / 2 of them.
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
    const bool screen = u64() != 0;
    const size_t block_lanes = u64(), k = u64();
    std::vector<uint64_t> cuts(k);
    for (auto &c : cuts) c = u64();
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
        schnorr_sig::Aggregator ag(cx, n, block_lanes);
        std::ofstream out(argv[2], std::ios::binary);
        size_t lo = 0;
        for (uint64_t c : cuts) {
            if (c > n - lo) return 2;
            uint64_t kept = 0;
            const std::vector<uint8_t> status =
                ag.push({sigs.begin() + lo, sigs.begin() + lo + c}, {pks.begin() + lo, pks.begin() + lo + c},
                        {msgs.begin() + lo, msgs.begin() + lo + c}, screen, &kept);
            out.write((const char *)status.data(), (std::streamsize)status.size());
            out.write((const char *)&kept, sizeof kept);
            lo += c;
        }
        const schnorr_sig::Aggregator::Info info = ag.info();
        out.write((const char *)&info, sizeof info);
        const schnorr_sig::AggregateSignature whole = ag.finish(), half = ag.finish(info.held / 2);
        out.write((const char *)whole.bytes.data(), (std::streamsize)whole.bytes.size());
        out.write((const char *)half.bytes.data(), (std::streamsize)half.bytes.size());
        if (ag.info().held != info.held) return 3;            // finish changes no lane
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
