// Host-side compile of what identifies a key on the device (tests only): the loaders of an affine lane and the lane
// and row sources of ssa_dedup.hpp, and the fingerprint over their words.  Reads one case per line from standard input and prints the key's words and its
// fingerprint in hex; tests/test_key_identity_host.py compares them with a SipHash-2-4 written in Python.
//   hipcc --cuda-host-only -x hip -O2 key_identity_main.cpp -o key_identity_main.out
// A case is   KIND k0 k1 index misalign bytes [flags]   (numbers and bytes in hex; "-" for no flags):
//   AL  affine lanes: `bytes` are 96-byte keys placed `misalign` bytes behind an 8-byte boundary, `flags` the pk_inf bytes
//   AR  affine rows:  `bytes` are the rows' 96 bytes each (c_pks), `flags` the c_inf bytes
//   WL  wire lanes:   `bytes` are 130-byte records placed `misalign` bytes behind an 8-byte boundary
//   WR  wire rows:    `bytes` are the rows' seven words each (c_wire)
#define SSA_NO_KERNELS 1
#define SSA_NO_COOP 1
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../schnorr-sig_amd/csrc/ssa_keyed.hpp"

using namespace ssa;

// `hex` as bytes, `misalign` bytes behind the start of an 8-byte aligned store
struct Bytes {
    std::vector<u64> store;
    u8 *p;
    size_t len;
    Bytes(const std::string &hex, size_t misalign) : store((hex.size() / 2 + misalign + 7) / 8 + 1, 0), len(hex.size() / 2) {
        p = reinterpret_cast<u8 *>(store.data()) + misalign;
        for (size_t i = 0; i < len; i++) p[i] = (u8)std::stoul(hex.substr(2 * i, 2), nullptr, 16);
    }
};

// an affine lane as dd_k_insert and kc_k_lookup read it: dd_key_word (aligned or byte-wise, decided once) and dd_key_flag
struct AffineLanes {
    static constexpr int WORDS = 13, BYTES = 97;
    const u8 *pks, *pk_inf;
    u64 word(size_t i, int k) const {
        return k < 12 ? dd_key_word(pks, i, k, ((size_t)pks & 7u) == 0) : (u64)dd_key_flag(pk_inf, i);
    }
};

template <class Src>
static void show(const Src &src, size_t index, u64 k0, u64 k1) {
    u64 w[Src::WORDS];
    dd_load(src, index, w);
    for (int k = 0; k < Src::WORDS; k++) std::printf("%016llx ", (unsigned long long)w[k]);
    std::printf("%016llx %d\n", (unsigned long long)dd_fingerprint_of<Src>(w, k0, k1), dd_same_key(src, index, w) ? 1 : 0);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, bytes, flags;
        u64 k0, k1;
        size_t index, misalign;
        if (!(in >> kind >> std::hex >> k0 >> k1 >> index >> misalign >> bytes)) continue;
        if (!(in >> flags)) flags = "-";
        const Bytes b(bytes, misalign), f(flags == "-" ? "" : flags, 0);
        const u8 *fl = flags == "-" ? nullptr : f.p;
        const size_t per = kind == "WL" ? 130 : kind == "WR" ? 8 * KY_WIRE_WORDS : 96;
        if (misalign > 7 || (index + 1) * per > b.len || (fl && index >= f.len) || ((kind[1] == 'R') && misalign)) {
            std::printf("bad case\n");
            return 2;
        }
        if (kind == "AL") {
            const AffineLanes lanes{b.p, fl};
            u64 w[13];
            dd_load(lanes, index, w);
            if (dd_fingerprint(w, (u32)w[12], k0, k1) != dd_fingerprint_of<AffineLanes>(w, k0, k1)) return 3;
            show(lanes, index, k0, k1);
        }
        else if (kind == "AR" && fl) show(DdAffineRows{reinterpret_cast<const u64 *>(b.p), fl}, index, k0, k1);
        else if (kind == "WL") show(DdWireLanes{b.p}, index, k0, k1);
        else if (kind == "WR") show(DdWireRows{reinterpret_cast<const u64 *>(b.p)}, index, k0, k1);
        else {
            std::printf("bad case\n");
            return 2;
        }
    }
    return 0;
}
