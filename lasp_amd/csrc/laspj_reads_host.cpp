// The host's half of the one-pass reads (no GPU involved, no lock taken): the wave-item
// layout of k_read_check's descriptors and the fold of read_any/3 over the met bytes the
// kernel answered.  laspj_nif_waiters.hip builds the descriptors around these and applies the fold
// to the variables' waiter and lazy lists; tests/c/reads_host_check.cpp drives them alone.

#include "laspj_internal.h"

namespace laspj {

uint64_t read_lay_items(ReadDesc* rds, uint32_t n, const uint64_t* tiles) {
    uint64_t items = 0;
    for (uint32_t i = 0; i < n; ++i) {
        rds[i].item0 = items;
        items += tiles[i];
    }
    return items;
}

void read_fold(uint32_t n, const uint32_t* var_of, uint32_t nvars, const uint32_t* nlazy,
               const uint8_t* const* ans, ReadFold* out) {
    out->found = -1;
    out->total = 0;
    out->fired.assign(n, {});
    out->blocked.assign(n, 0);
    out->still.assign(nvars, {});
    // present[v][j]: lazy entry j of variable v is still in its list
    std::vector<std::vector<uint8_t>> present(nvars);
    for (uint32_t v = 0; v < nvars; ++v) present[v].assign(nlazy[v], 1);
    for (uint32_t i = 0; i < n && out->found < 0; ++i) {
        const uint32_t v = var_of[i];
        // reply_to_all(LazyThreads, {ok, Threshold}) over the list as this read finds it
        for (uint32_t j = 0; j < nlazy[v]; ++j)
            if (present[v][j] && ans[i][1 + j]) out->fired[i].push_back(j);
        out->total += out->fired[i].size();
        if (ans[i][0]) {
            out->found = (int32_t)i;          // met: nothing is stored, the fired entries stay
        } else {
            out->blocked[i] = 1;              // V#dv{waiting_threads=WT, lazy_threads=StillLazy}
            for (uint32_t j : out->fired[i]) present[v][j] = 0;
        }
    }
    for (uint32_t v = 0; v < nvars; ++v)
        for (uint32_t j = 0; j < nlazy[v]; ++j)
            if (present[v][j]) out->still[v].push_back(j);
}

}  // namespace laspj
