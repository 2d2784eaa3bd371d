// Driver of tests/test_gpu_aggverifier_mixed.py (the _cxx test): schnorr_sig::AggregateVerifier::push_mixed and
// push_known of the C++ mirror on one scenario written by the test.  Input file: u64 p, the pool's lanes -- p x 81
// signature bytes, p x 96 key bytes, p x u64 message lengths, the message bytes --, u64 pool block_lanes; u64 n (the
// capacity of the verifier), u64 block_lanes, u64 k pushes; per push u64 lanes, lanes x u32 places (all ones: unknown),
// u64 u, and the u unknown lanes: u x 49 bytes of R's, u x 96 key bytes, u x u64 message lengths, the message bytes;
// then u64 m, m x (u64 n_take -- all ones: every lane held --, 32 bytes of e_agg).  The pool admits its lanes by ONE
// screened push; a push without unknown lanes goes through push_known.  Output file: the pool's status bytes, the m status
// words (i32) of finish_status and the eight info words.
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
    auto keys_and_msgs = [&](size_t n, std::vector<schnorr_sig::PublicKey> &pks, Msgs &msgs) {
        pks.resize(n);
        for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
        std::vector<uint64_t> lens(n);
        for (auto &l : lens) l = u64();
        msgs.resize(n);
        for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
    };
    try {
        schnorr_sig::Context cx(0);
        std::ofstream out(argv[2], std::ios::binary);
        const size_t p = u64();
        std::vector<schnorr_sig::Signature> sigs(p);
        for (auto &s : sigs) std::memcpy(s.bytes.data(), need(81), 81);
        std::vector<schnorr_sig::PublicKey> pool_pks;
        Msgs pool_msgs;
        keys_and_msgs(p, pool_pks, pool_msgs);
        schnorr_sig::Aggregator pool(cx, p, u64());
        const std::vector<uint8_t> status = pool.push(sigs, pool_pks, pool_msgs);
        out.write((const char *)status.data(), status.size());
        const size_t n = u64(), block_lanes = u64();
        schnorr_sig::AggregateVerifier av(cx, n, block_lanes);
        for (uint64_t k = u64(); k; k--) {
            const size_t lanes = u64();
            std::vector<uint32_t> places(lanes);
            if (lanes) std::memcpy(places.data(), need(4 * lanes), 4 * lanes);
            const size_t u = u64();
            const uint8_t *rs = need(49 * u);
            std::vector<schnorr_sig::PublicKey> pks;
            Msgs msgs;
            keys_and_msgs(u, pks, msgs);
            if (u) av.push_mixed(pool, places, rs, pks, msgs);
            else av.push_known(pool, places);
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
