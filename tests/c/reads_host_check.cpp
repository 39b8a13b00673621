// The host's half of the one-pass reads (laspj_reads_host.cpp: the wave-item layout and the
// fold of read_any/3) as a program of its own, so that it can be built with the host
// sanitizers (tests/test_reads_host.py builds and runs it; nothing here touches a GPU).
//
// read_fold is compared with the fold written the way lasp_core.erl:372-414 writes it —
// lists of entries edited read by read — over random calls: up to 20 reads of up to 5
// variables (named again at random) with up to 20 lazy entries each, every met byte in a
// heap block of exactly its length (a read past it is the sanitizer's to find).

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../lasp_amd/csrc/laspj_internal.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

int main() {
    int bad = 0, rounds = 0;
    // the layout: tiles of 128 units of two words, an odd last word is a unit
    const uint64_t words[] = {0, 1, 2, 255, 256, 257, 258, 512, 513};
    const uint64_t want[] = {0, 1, 1, 1, 1, 2, 2, 2, 3};
    for (int k = 0; k < 9; ++k)
        if (laspj::read_tiles(words[k]) != want[k]) {
            std::printf("read_tiles(%llu) = %llu\n", (unsigned long long)words[k],
                        (unsigned long long)laspj::read_tiles(words[k]));
            ++bad;
        }
    {
        std::vector<laspj::ReadDesc> d(4);
        const uint64_t tiles[4] = {2, 0, 3, 1};
        const uint64_t items = laspj::read_lay_items(d.data(), 4, tiles);
        if (items != 6 || d[0].item0 != 0 || d[1].item0 != 2 || d[2].item0 != 2 || d[3].item0 != 5) {
            std::printf("read_lay_items\n");
            ++bad;
        }
        if (laspj::read_lay_items(nullptr, 0, nullptr) != 0) ++bad;
    }
    for (; rounds < 4000; ++rounds) {
        const uint32_t nvars = 1 + rnd(5), n = 1 + rnd(20);
        std::vector<uint32_t> nlazy(nvars), var_of(n);
        for (uint32_t& x : nlazy) x = rnd(4) == 0 ? 0 : rnd(21);
        std::vector<std::vector<uint8_t>> ans(n);
        std::vector<const uint8_t*> ap(n);
        const uint32_t p_met = rnd(4);          // 0: no read is met
        for (uint32_t i = 0; i < n; ++i) {
            var_of[i] = rnd(nvars);
            ans[i].resize(1 + nlazy[var_of[i]]);
            ans[i][0] = p_met && rnd(8) < p_met ? 1 : 0;
            for (size_t j = 1; j < ans[i].size(); ++j) ans[i][j] = (uint8_t)rnd(2);
            ap[i] = ans[i].data();
        }
        laspj::ReadFold f;
        laspj::read_fold(n, var_of.data(), nvars, nlazy.data(), ap.data(), &f);
        // the reference's shape: each variable's list of entries, edited read by read
        std::vector<std::vector<uint32_t>> lists(nvars);
        for (uint32_t v = 0; v < nvars; ++v)
            for (uint32_t j = 0; j < nlazy[v]; ++j) lists[v].push_back(j);
        int32_t found = -1;
        uint64_t total = 0;
        bool same = true;
        for (uint32_t i = 0; i < n; ++i) {
            std::vector<uint32_t> fired, still;
            uint8_t blocked = 0;
            if (found < 0) {
                for (uint32_t j : lists[var_of[i]]) (ans[i][1 + j] ? fired : still).push_back(j);
                if (ans[i][0]) {
                    found = (int32_t)i;
                } else {
                    blocked = 1;
                    lists[var_of[i]] = still;
                }
            }
            total += fired.size();
            same = same && fired == f.fired[i] && blocked == f.blocked[i];
        }
        same = same && found == f.found && total == f.total && lists == f.still;
        if (!same) {
            std::printf("round %d: fold differs\n", rounds);
            ++bad;
        }
    }
    std::printf("%d rounds, %d bad\n", rounds, bad);
    return bad ? 1 : 0;
}
