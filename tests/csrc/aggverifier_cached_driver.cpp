// Driver of tests/test_gpu_aggverifier_cached_cxx.py: the KeyCache overloads of schnorr_sig::AggregateVerifier (push
// through an Affine cache, push_wire through a Wire cache, and the plain push beside them) on the cases written by the
// test, one verifier and one fresh cache per case on one context.  Input file: u64 cases; per case u64 n, u64 wire (0 /
// 1), u64 k, k x (u64 push size, u64 through the cache 0 / 1) (the sizes sum to n), n x 49 bytes of R's, n x 96 affine key
// bytes, n identity flags, n x 49 wire key bytes, n x u64 message lengths, the message bytes, u64 m, m x (u64 n_take --
// all ones: every lane held --, 32 bytes of e_agg).  A plain push takes the affine keys in both modes.  Output file: per
// case k x 8 statistics words (zeros for a plain push), the m status words (i32) of finish_status and the eight info words.
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
            const size_t n = u64();
            const bool wire = u64() != 0;
            std::vector<std::pair<uint64_t, uint64_t>> cuts(u64());
            for (auto &c : cuts) {
                c.first = u64();
                c.second = u64();
            }
            const uint8_t *rs = need(49 * n);
            std::vector<schnorr_sig::PublicKey> pks(n);
            for (auto &pk : pks) std::memcpy(pk.affine.data(), need(96), 96);
            for (auto &pk : pks) pk.is_identity = *need(1) != 0;
            const uint8_t *w49 = need(49 * n);
            std::vector<uint64_t> lens(n);
            for (auto &l : lens) l = u64();
            std::vector<std::pair<const uint8_t *, size_t>> msgs(n);
            for (size_t i = 0; i < n; i++) msgs[i] = {need(lens[i]), (size_t)lens[i]};
            schnorr_sig::AggregateVerifier av(cx, n);
            schnorr_sig::KeyCache cache(cx, 256, wire ? schnorr_sig::KeyCache::Wire : schnorr_sig::KeyCache::Affine);
            size_t lo = 0;
            for (const auto &c : cuts) {
                const size_t cnt = c.first;
                if (cnt > n - lo) return 2;
                uint64_t stats[8] = {};
                const std::vector<std::pair<const uint8_t *, size_t>> m(msgs.begin() + lo, msgs.begin() + lo + cnt);
                if (!c.second)
                    av.push(rs + 49 * lo, {pks.begin() + lo, pks.begin() + lo + cnt}, m);
                else if (wire)
                    av.push_wire(cache, rs + 49 * lo, std::vector<uint8_t>(w49 + 49 * lo, w49 + 49 * (lo + cnt)), m, stats);
                else
                    av.push(cache, rs + 49 * lo, {pks.begin() + lo, pks.begin() + lo + cnt}, m, stats);
                out.write((const char *)stats, sizeof stats);
                lo += cnt;
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
