// Driver of tests/test_gpu_aggverifier_admission.py (the _cxx test): schnorr_sig::Aggregator with HoldAdmission and the
// KeyCache overloads of schnorr_sig::AggregateVerifier::push_mixed / push_mixed_wire of the C++ mirror on one scenario
// written by the test.  Input file: u64 pool capacity, u64 pool block_lanes, u64 pool pushes; per pool push u64 kind
// (0: push without the screen, 1: the screened push, 2: push through an Affine cache), u64 lanes, lanes x 81 signature
// bytes, lanes x 96 key bytes, lanes x u64 message lengths, the message bytes; u64 n (the capacity of the verifier),
// u64 block_lanes, u64 k pushes; per push u64 wire (0: affine keys, 1: 49-byte keys), u64 require, u64 lanes,
// lanes x u32 places (all ones: unknown), u64 u, and the u unknown lanes: u x 49 bytes of R's, u x 96 (wire: 49) key
// bytes, u x u64 message lengths, the message bytes; then u64 m, m x (u64 n_take -- all ones: every lane held --, 32
// bytes of e_agg).  Output file: the pool's status bytes, its admission classes, one byte per verifier push (1: it
// threw), the m status words (i32) of finish_status and the eight info words.
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
    auto read_keys = [&](size_t n, std::vector<schnorr_sig::PublicKey> &pks) {
        pks.resize(n);
        for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
    };
    auto read_msgs = [&](size_t n, Msgs &msgs) {
        std::vector<uint64_t> lens(n);
        for (auto &l : lens) l = u64();
        msgs.resize(n);
        for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    };
    try {
        schnorr_sig::Context cx(0);
        std::ofstream out(argv[2], std::ios::binary);
        schnorr_sig::KeyCache affine(cx, 4096), wire(cx, 4096, schnorr_sig::KeyCache::Wire);
        const size_t capacity = u64(), pool_block = u64();
        schnorr_sig::Aggregator pool(cx, capacity, pool_block, schnorr_sig::Aggregator::HoldAdmission);
        for (uint64_t k = u64(); k; k--) {
            const uint64_t kind = u64();
            const size_t lanes = u64();
            std::vector<schnorr_sig::Signature> sigs(lanes);
            for (auto &s : sigs) std::memcpy(s.bytes.data(), need(81), 81);
            std::vector<schnorr_sig::PublicKey> pks;
            Msgs msgs;
            read_keys(lanes, pks);
            read_msgs(lanes, msgs);
            const std::vector<uint8_t> status = kind == 2 ? pool.push(affine, sigs, pks, msgs) : pool.push(sigs, pks, msgs, kind == 1);
            out.write((const char *)status.data(), status.size());
        }
        const std::vector<uint8_t> classes = pool.admission();
        out.write((const char *)classes.data(), classes.size());
        const size_t n = u64(), block_lanes = u64();
        schnorr_sig::AggregateVerifier av(cx, n, block_lanes);
        for (uint64_t k = u64(); k; k--) {
            const bool is_wire = u64() != 0;
            const auto require = (schnorr_sig::AggregateVerifier::Require)u64();
            const size_t lanes = u64();
            std::vector<uint32_t> places(lanes);
            if (lanes) std::memcpy(places.data(), need(4 * lanes), 4 * lanes);
            const size_t u = u64();
            const uint8_t *rs = need(49 * u);
            std::vector<schnorr_sig::PublicKey> pks;
            std::vector<uint8_t> keys49;
            Msgs msgs;
            if (is_wire) {
                const uint8_t *k49 = need(49 * u);
                keys49.assign(k49, k49 + 49 * u);
            } else {
                read_keys(u, pks);
            }
            read_msgs(u, msgs);
            uint8_t threw = 0;
            try {
                if (is_wire) av.push_mixed_wire(pool, wire, places, rs, keys49, msgs, require);
                else av.push_mixed(pool, affine, places, rs, pks, msgs, require);
            } catch (const std::runtime_error &) {
                threw = 1;
            }
            out.write((const char *)&threw, 1);
        }
        for (uint64_t m = u64(); m; m--) {
            const uint64_t n_take = u64();
            const int32_t st = av.finish_status(need(32), n_take == ~0ull ? schnorr_sig::AggregateVerifier::All : (size_t)n_take);
            out.write((const char *)&st, sizeof st);
        }
        const schnorr_sig::AggregateVerifier::Info info = av.info();
        out.write((const char *)&info, sizeof info);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
