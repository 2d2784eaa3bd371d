// Driver of tests/test_gpu_aggregator_select_cxx.py: finish_select, remove_indices and take_select of
// schnorr_sig::Aggregator of the C++ mirror on one case written by the test.
// Input file: u64 n, u64 block_lanes, u64 m1, u64 m2, u64 m3 (the lengths of three lists), n x 81 signature bytes,
// n x 49 wire keys, n x u64 message lengths, the message bytes, then the three lists as u32.  List 1 and list 2 are valid
// for the lanes held when they are used; list 3 is one the device refuses.
// Object A (HoldKeys): all n records through a wire cache; finish_select(list 1) with keys; take_select(list 2) with keys;
// keys and finish of what is left.  Object B (no key column): the same push; finish_select(list 1); remove_indices(list 2);
// finish.
// Output file: the n status bytes and the u64 kept count of A's push; A: keys, aggregate of list 1; keys, aggregate of
// list 2; keys, finish; B: aggregate of list 1, the u64 kept count of remove_indices, finish; the eight info words of A
// and B.
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
    const size_t n = u64(), block_lanes = u64(), m1 = u64(), m2 = u64(), m3 = u64();
    const uint8_t *sigs = need(81 * n), *wire = need(49 * n);
    std::vector<uint64_t> lens(n);
    for (auto &l : lens) l = u64();
    std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
    for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    auto list = [&](size_t m) {
        std::vector<uint32_t> v(m);
        if (m) std::memcpy(v.data(), need(4 * m), 4 * m);
        return v;
    };
    const std::vector<uint32_t> l1 = list(m1), l2 = list(m2), l3 = list(m3);
    std::vector<uint8_t> keyed(130 * n);
    for (size_t i = 0; i < n; i++) {
        std::memcpy(keyed.data() + 130 * i, wire + 49 * i, 49);
        std::memcpy(keyed.data() + 130 * i + 49, sigs + 81 * i, 81);
    }
    try {
        using schnorr_sig::Aggregator;
        schnorr_sig::Context cx(0);
        schnorr_sig::KeyCache cache(cx, 4096, schnorr_sig::KeyCache::Wire);
        Aggregator a(cx, n, block_lanes, Aggregator::HoldKeys), b(cx, n, block_lanes);
        std::ofstream out(argv[2], std::ios::binary);
        auto bytes = [&](const std::vector<uint8_t> &v) { out.write((const char *)v.data(), (std::streamsize)v.size()); };
        auto word = [&](uint64_t v) { out.write((const char *)&v, sizeof v); };
        uint64_t kept = 0;
        std::vector<uint8_t> keys;
        // A: the block body of a selection, then of a selection that leaves
        bytes(a.push_keyed(cache, keyed, msgs, &kept));
        word(kept);
        schnorr_sig::AggregateSignature agg = a.finish_select(l1, &keys);
        bytes(keys);
        bytes(agg.bytes);
        agg = a.take_select(l2, &keys);
        bytes(keys);
        bytes(agg.bytes);
        bytes(a.keys());
        bytes(a.finish().bytes);
        // B: no key column
        b.push_keyed(cache, keyed, msgs, &kept);
        bytes(b.finish_select(l1).bytes);
        word(b.remove_indices(l2));
        bytes(b.finish().bytes);
        // what is refused: a list the device refuses, by either call; the keys of an object that holds none
        int refused = 0;
        const Aggregator::Info before = a.info();
        try {
            a.finish_select(l3, &keys);
        } catch (const std::runtime_error &) {
            refused++;
        }
        try {
            a.remove_indices(l3);
        } catch (const std::runtime_error &) {
            refused++;
        }
        try {
            b.finish_select(std::vector<uint32_t>{0}, &keys);
        } catch (const std::runtime_error &) {
            refused++;
        }
        if (refused != 3 || a.info().held != before.held) return 3;
        for (const Aggregator *o : {&a, &b}) {
            const Aggregator::Info info = o->info();
            out.write((const char *)&info, sizeof info);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
