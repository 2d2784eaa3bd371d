// Host-side compile of the key-table check's per-key device functions (tests only): what
// kck_k_tables decides for one key, run on the CPU over the table build_ptab builds -- the table builder and the check
// are the library's own code, so a disagreement between them shows without a GPU.  The shipped library never runs this.
//   hipcc --cuda-host-only -x hip -O2 -shared -fPIC keycheck_host.cpp -o libkeycheck_host.so
#define SSA_NO_KERNELS 1
#define SSA_NO_COOP 1
#define SSA_CHECK_FUNCTIONS_ONLY 1
#include "../../schnorr-sig_amd/csrc/ssa_kernels.hpp"
#include "../../schnorr-sig_amd/csrc/ssa_selfcheck.hpp"
#include "../../schnorr-sig_amd/csrc/ssa_keycheck.hpp"

using namespace ssa;

extern "C" {
// the table ssa_k_keyset_build stores for a well-formed key (512 words) -> the status it stores (0 / 1)
int kh_build(const uint64_t *key12, int inf, uint64_t *tab512) {
    bool canon;
    const aff P = kck_ld_key(key12, 0, canon);
    build_ptab(tab512, P, inf != 0);
    sc256 q;
    for (int j = 0; j < 4; j++) q.w[j] = SC_Q(j);
    return jac_is_identity(mul_ptab(tab512, q, true)) ? 0 : 1;
}
// kck_k_tables' decision for one key of stored status st: 0 passes, 1 fails, 2 goes to the rebuild list
int kh_light(const uint64_t *key12, int inf, int st, const uint64_t *tab512) {
    bool canon;
    const aff P = kck_ld_key(key12, 0, canon);
    const bool wellformed = canon && (inf || aff_on_curve(P));
    if (st == (int)ST_MALFORMED) return wellformed ? 1 : 0;
    if (st < 0 || st > (int)ST_INVALID_PK || !wellformed) return 1;
    if (st == (int)ST_INVALID_PK) return 2;
    if (inf) {
        for (int e = 0; e < PTAB_ENTRIES; e++)
            if (!kck_entry_sentinel(tab512 + e * PTAB_ENTRY_U64)) return 1;
        return 0;
    }
    return kck_chain_ok(tab512, P) ? 0 : 1;
}
}
