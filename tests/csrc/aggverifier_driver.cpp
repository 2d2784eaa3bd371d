// Driver of tests/test_gpu_aggverifier_cxx.py: schnorr_sig::AggregateVerifier of the C++ mirror on the cases written by the
// test, one verifier per case on one context.  Input file: u64 cases; per case u64 n, u64 block_lanes, u64 k, k x u64 push
// sizes (their sum is n), n x 49 bytes of R's, n x 96 key bytes, n identity flags, n x u64 message lengths, the message
// bytes, u64 m, m x (u64 n_take -- all ones: every lane held --, 32 bytes of e_agg).  Output file: per case the m status
// words (i32) of finish_status and then the eight info words.
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
    try {
        schnorr_sig::Context cx(0);
        std::ofstream out(argv[2], std::ios::binary);
        for (uint64_t cases = u64(); cases; cases--) {
            const size_t n = u64(), block_lanes = u64(), k = u64();
            std::vector<uint64_t> cuts(k);
            for (auto &c : cuts) c = u64();
            const uint8_t *rs = need(49 * n);
            std::vector<schnorr_sig::PublicKey> pks(n);
            for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
            for (auto &pk : pks) pk.is_identity = *need(1) != 0;
            std::vector<uint64_t> lens(n);
            for (auto &l : lens) l = u64();
            std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
            for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
            schnorr_sig::AggregateVerifier av(cx, n, block_lanes);
            size_t lo = 0;
            for (uint64_t c : cuts) {
                if (c > n - lo) return 2;
                av.push(rs + 49 * lo, {pks.begin() + lo, pks.begin() + lo + c}, {msgs.begin() + lo, msgs.begin() + lo + c});
                lo += c;
            }
            for (uint64_t m = u64(); m; m--) {
                const uint64_t n_take = u64();
                const int32_t st = av.finish_status(need(32), n_take == ~0ull ? schnorr_sig::AggregateVerifier::All : (size_t)n_take);
                out.write((const char *)&st, sizeof st);
            }
            const schnorr_sig::AggregateVerifier::Info info = av.info();
            out.write((const char *)&info, sizeof info);
            if (info.held != n) return 3;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
