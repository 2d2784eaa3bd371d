// Driver of tests/test_gpu_aggregator_cached_cxx.py: the KeyCache overloads of schnorr_sig::Aggregator of the C++ mirror
// (push through an affine cache, push_keyed through a wire cache, keys, HoldKeys) on one case written by the test.
// Input file: u64 n, u64 n_affine, u64 block_lanes, u64 n_objects (KeyedSignature objects), u64 mask_a, u64 mask_b (the
// lengths of the two masks), n x 81 signature bytes, n x 96 key bytes, n identity flags, n x 49 wire keys, n x u64 message
// lengths, the message bytes, then the two masks.
// Object A (no key column): the first n_affine triples through the affine cache, then all n records through the wire
// cache; remove(mask a).  Object B (HoldKeys): all n records; remove(mask b).  Object C (HoldKeys): the first n_objects
// lanes as KeyedSignature objects.
// Output file: per push its n status bytes, the u64 kept count and the 12 statistics words; A: finish, the u64 kept count
// of remove, finish; B: keys, finish, the u64 kept count of remove, keys, finish; C: keys, finish; the eight info words of
// A, B and C.
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
    const size_t n = u64(), n_affine = u64(), block_lanes = u64(), n_objects = u64(), len_a = u64(), len_b = u64();
    if (n_affine > n || n_objects > n) return 2;
    std::vector<schnorr_sig::Signature> sigs(n);
    for (auto &s : sigs) std::memcpy(s.bytes.data(), need(81), 81);
    std::vector<schnorr_sig::PublicKey> pks(n);
    for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
    for (auto &pk : pks) pk.is_identity = *need(1) != 0;
    const uint8_t *wire = need(49 * n);
    std::vector<uint64_t> lens(n);
    for (auto &l : lens) l = u64();
    std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
    for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    const uint8_t *ma = need(len_a), *mb = need(len_b);
    const std::vector<uint8_t> mask_a(ma, ma + len_a), mask_b(mb, mb + len_b);
    std::vector<uint8_t> keyed(130 * n);
    for (size_t i = 0; i < n; i++) {
        std::memcpy(keyed.data() + 130 * i, wire + 49 * i, 49);
        std::memcpy(keyed.data() + 130 * i + 49, sigs[i].bytes.data(), 81);
    }
    try {
        using schnorr_sig::Aggregator;
        schnorr_sig::Context cx(0);
        schnorr_sig::KeyCache affine(cx, 4096), wire_cache(cx, 4096, schnorr_sig::KeyCache::Wire);
        Aggregator a(cx, n_affine + n, block_lanes), b(cx, n, block_lanes, Aggregator::HoldKeys),
            c(cx, n_objects + 1, block_lanes, Aggregator::HoldKeys);
        std::ofstream out(argv[2], std::ios::binary);
        auto bytes = [&](const std::vector<uint8_t> &v) { out.write((const char *)v.data(), (std::streamsize)v.size()); };
        auto word = [&](uint64_t v) { out.write((const char *)&v, sizeof v); };
        auto pushed = [&](const std::vector<uint8_t> &status, uint64_t kept, const uint64_t *stats) {
            bytes(status);
            word(kept);
            out.write((const char *)stats, 12 * sizeof(uint64_t));
        };
        uint64_t kept = 0, stats[12];
        std::vector<uint8_t> status;
        const std::vector<schnorr_sig::Signature> s0(sigs.begin(), sigs.begin() + (std::ptrdiff_t)n_affine);
        const std::vector<schnorr_sig::PublicKey> p0(pks.begin(), pks.begin() + (std::ptrdiff_t)n_affine);
        const std::vector<std::pair<const uint8_t *, size_t>> m0(msgs.begin(), msgs.begin() + (std::ptrdiff_t)n_affine);
        // A: both kinds of cached push on one object
        status = a.push(affine, s0, p0, m0, &kept, stats);
        pushed(status, kept, stats);
        status = a.push_keyed(wire_cache, keyed, msgs, &kept, stats);
        pushed(status, kept, stats);
        bytes(a.finish().bytes);
        word(a.remove(mask_a));
        bytes(a.finish().bytes);
        // B: the key column
        status = b.push_keyed(wire_cache, keyed, msgs, &kept, stats);
        pushed(status, kept, stats);
        bytes(b.keys());
        bytes(b.finish().bytes);
        word(b.remove(mask_b));
        bytes(b.keys());
        bytes(b.finish().bytes);
        // C: KeyedSignature objects
        std::vector<schnorr_sig::KeyedSignature> objects(n_objects);
        for (size_t i = 0; i < n_objects; i++) {
            objects[i].public_key = pks[i];
            objects[i].signature = sigs[i];
        }
        const std::vector<std::pair<const uint8_t *, size_t>> mc(msgs.begin(), msgs.begin() + (std::ptrdiff_t)n_objects);
        status = c.push_keyed(wire_cache, objects, mc, &kept, stats);
        pushed(status, kept, stats);
        bytes(c.keys());
        bytes(c.finish().bytes);
        // what the mirror refuses itself: a cache of the other mode, keys of an object without a key column
        int refused = 0;
        try {
            a.push(wire_cache, s0, p0, m0);
        } catch (const std::invalid_argument &) {
            refused++;
        }
        try {
            a.push_keyed(affine, keyed, msgs);
        } catch (const std::invalid_argument &) {
            refused++;
        }
        try {
            a.keys();
        } catch (const std::runtime_error &) {
            refused++;
        }
        if (refused != 3) return 3;
        for (const Aggregator *o : {&a, &b, &c}) {
            const Aggregator::Info info = o->info();
            out.write((const char *)&info, sizeof info);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
