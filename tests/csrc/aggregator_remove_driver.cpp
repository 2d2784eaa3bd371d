// Driver of tests/test_gpu_aggregator_remove_cxx.py: drop_front, remove and take of schnorr_sig::Aggregator of the C++
// mirror on one case written by the test.
// Input file: u64 n, u64 block_lanes, u64 d (front drop), u64 t (take), n x 81 signature bytes, n x 96 key bytes, n
// identity flags, n x u64 message lengths, the message bytes, then n - d mask bytes.  The n triples are pushed at once,
// unscreened.  Output file: the aggregate of all lanes after drop_front(d); the u64 kept count of remove(mask) and the
// aggregate of all lanes after it; the aggregate take(t) returns and the aggregate of all that is left; the eight info
// words.
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
    const size_t n = u64(), block_lanes = u64(), front = u64(), take = u64();
    if (front > n) return 2;
    std::vector<schnorr_sig::Signature> sigs(n);
    for (auto &s : sigs) std::memcpy(s.bytes.data(), need(81), 81);
    std::vector<schnorr_sig::PublicKey> pks(n);
    for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
    for (auto &pk : pks) pk.is_identity = *need(1) != 0;
    std::vector<uint64_t> lens(n);
    for (auto &l : lens) l = u64();
    std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
    for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    const uint8_t *m = need(n - front);
    const std::vector<uint8_t> mask(m, m + (n - front));
    try {
        schnorr_sig::Context cx(0);
        schnorr_sig::Aggregator ag(cx, n, block_lanes);
        std::ofstream out(argv[2], std::ios::binary);
        auto put = [&](const schnorr_sig::AggregateSignature &a) {
            out.write((const char *)a.bytes.data(), (std::streamsize)a.bytes.size());
        };
        uint64_t kept = 0;
        ag.push(sigs, pks, msgs, false, &kept);
        if (kept != n) return 3;
        ag.drop_front(front);
        put(ag.finish());
        kept = ag.remove(mask);
        out.write((const char *)&kept, sizeof kept);
        put(ag.finish());
        if (ag.info().held != kept) return 3;
        put(ag.take(take));
        put(ag.finish());
        const schnorr_sig::Aggregator::Info info = ag.info();
        out.write((const char *)&info, sizeof info);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
