// Driver of tests/test_gpu_aggregator_index_cxx.py: the leaf column and the leaf index of schnorr_sig::Aggregator
// (HoldIndex; leaves, leaves_select, index_sync, lookup, index_info) of the C++ mirror on one scenario written by the
// test.  Input file: u64 pool capacity, u64 block_lanes, u64 options (the create flags), then u64 k operations, each a
// u64 code and its arguments:
//   1 push         u64 screen, u64 lanes, lanes x 81 signature bytes, lanes x 96 key bytes, lanes x u64 message lengths,
//                  the message bytes                               -> the status bytes
//   2 lookup       u64 n, n x 32 id bytes                          -> one byte (1: it threw), n x u32 places, u64 n_unknown
//   3 leaves       u64 n_take (all ones: every lane held)          -> one byte (1: it threw), the leaves
//   4 leaves_select u64 m, m x u32 places                          -> one byte (1: it threw), the leaves
//   5 drop_front   u64 n                                           -> nothing
//   6 index_sync                                                   -> one byte (1: it threw)
//   7 index_info                                                   -> one byte (1: it threw), the eight words
// What a call that threw would have written is left out.
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
    using Msgs = std::vector<std::pair<const uint8_t *, size_t>>;
    try {
        schnorr_sig::Context cx(0);
        std::ofstream out(argv[2], std::ios::binary);
        auto put = [&](const void *p, size_t bytes) { out.write((const char *)p, (std::streamsize)bytes); };
        // (one statement per call that may throw: the byte in front says whether the bytes behind it exist)
        auto guarded = [&](auto &&call) {
            uint8_t threw = 0;
            try {
                call();
            } catch (const std::runtime_error &) {
                threw = 1;
            }
            return threw;
        };
        const size_t capacity = u64(), block_lanes = u64();
        const auto options = (schnorr_sig::Aggregator::Options)u64();
        schnorr_sig::Aggregator pool(cx, capacity, block_lanes, options);
        for (uint64_t k = u64(); k; k--) {
            const uint64_t op = u64();
            if (op == 1) {
                const bool screen = u64() != 0;
                const size_t lanes = u64();
                std::vector<schnorr_sig::Signature> sigs(lanes);
                for (auto &s : sigs) std::memcpy(s.bytes.data(), need(81), 81);
                std::vector<schnorr_sig::PublicKey> pks(lanes);
                for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
                std::vector<uint64_t> lens(lanes);
                for (auto &l : lens) l = u64();
                Msgs msgs(lanes);
                for (size_t i = 0; i < lanes; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
                const std::vector<uint8_t> status = pool.push(sigs, pks, msgs, screen);
                put(status.data(), status.size());
            } else if (op == 2) {
                const size_t n = u64();
                const uint8_t *ids = need(32 * n);
                schnorr_sig::Aggregator::Lookup r{};
                const uint8_t threw = guarded([&] { r = pool.lookup(std::vector<uint8_t>(ids, ids + 32 * n)); });
                put(&threw, 1);
                if (!threw) {
                    put(r.places.data(), 4 * r.places.size());
                    put(&r.n_unknown, 8);
                }
            } else if (op == 3) {
                const uint64_t n_take = u64();
                std::vector<uint8_t> leaves;
                const uint8_t threw =
                    guarded([&] { leaves = pool.leaves(n_take == ~0ull ? schnorr_sig::Aggregator::All : (size_t)n_take); });
                put(&threw, 1);
                if (!threw) put(leaves.data(), leaves.size());
            } else if (op == 4) {
                const size_t m = u64();
                std::vector<uint32_t> order(m);
                if (m) std::memcpy(order.data(), need(4 * m), 4 * m);
                std::vector<uint8_t> leaves;
                const uint8_t threw = guarded([&] { leaves = pool.leaves_select(order); });
                put(&threw, 1);
                if (!threw) put(leaves.data(), leaves.size());
            } else if (op == 5) {
                pool.drop_front((size_t)u64());
            } else if (op == 6) {
                const uint8_t threw = guarded([&] { pool.index_sync(); });
                put(&threw, 1);
            } else if (op == 7) {
                schnorr_sig::Aggregator::IndexInfo info{};
                const uint8_t threw = guarded([&] { info = pool.index_info(); });
                put(&threw, 1);
                if (!threw) put(&info, sizeof info);
            } else {
                std::fprintf(stderr, "unknown operation\n");
                return 2;
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
