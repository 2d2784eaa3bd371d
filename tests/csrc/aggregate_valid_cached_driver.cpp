// Driver of tests/test_gpu_aggregate_valid_cached_cxx.py: the KeyCache overloads of AggregateSignature::aggregate_valid of the
// C++ mirror on one case written by the test, and the validator's call on what came out, on the same cache.
// Input file: u64 mode (0 objects and an Affine cache, 1 records and a Wire cache), u64 n, n x 81 signature bytes, n x 96 key
// bytes, n identity flags, n x 49 wire keys, n x u64 message lengths, the message bytes.
// Output file: u64 |K|, |K| x u32 kept lanes, the aggregate's 49 |K| + 32 bytes, the kept keys (96 + 1 bytes each: key,
// flag; or 49 bytes each), 12 x u64 statistics, u32 the validator's verdict.
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
    const bool wire = u64() != 0;
    const size_t n = u64();
    std::vector<schnorr_sig::Signature> sigs(n);
    for (auto &s : sigs) std::memcpy(s.bytes.data(), need(81), 81);
    std::vector<schnorr_sig::PublicKey> pks(n);
    for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
    for (auto &pk : pks) pk.is_identity = *need(1) != 0;
    std::vector<uint8_t> records(n * 130);
    for (size_t i = 0; i < n; i++) {
        std::memcpy(&records[130 * i], need(49), 49);
        std::memcpy(&records[130 * i + 49], sigs[i].bytes.data(), 81);
    }
    std::vector<uint64_t> lens(n);
    for (auto &l : lens) l = u64();
    std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
    for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    try {
        using schnorr_sig::AggregateSignature;
        using schnorr_sig::KeyCache;
        schnorr_sig::Context cx(0);
        KeyCache cache(cx, 4096, wire ? KeyCache::Wire : KeyCache::Affine);
        uint64_t stats[12] = {};
        std::vector<schnorr_sig::PublicKey> kept_keys;
        std::vector<uint8_t> kept49;
        const auto r = wire ? AggregateSignature::aggregate_valid(cx, cache, records, msgs, &kept49, stats)
                            : AggregateSignature::aggregate_valid(cx, cache, sigs, pks, msgs, &kept_keys, stats);
        std::vector<std::pair<const uint8_t *, size_t>> kept_msgs;
        for (uint32_t i : r.second) kept_msgs.push_back(msgs[i]);
        const std::vector<uint32_t> v = wire ? AggregateSignature::verify_many(cx, cache, {r.first}, kept49, kept_msgs)
                                             : AggregateSignature::verify_many(cx, cache, {r.first}, kept_keys, kept_msgs);
        const uint64_t m = r.second.size();
        std::ofstream out(argv[2], std::ios::binary);
        out.write((const char *)&m, sizeof m);
        out.write((const char *)r.second.data(), (std::streamsize)(m * sizeof(uint32_t)));
        out.write((const char *)r.first.bytes.data(), (std::streamsize)r.first.bytes.size());
        if (wire) {
            out.write((const char *)kept49.data(), (std::streamsize)kept49.size());
        } else {
            for (const auto &pk : kept_keys) {
                const char flag = pk.is_identity ? 1 : 0;
                out.write((const char *)pk.affine.data(), 96);
                out.write(&flag, 1);
            }
        }
        out.write((const char *)stats, sizeof stats);
        out.write((const char *)v.data(), sizeof(uint32_t));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
