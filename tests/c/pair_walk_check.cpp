// The pair-mode list walk (laspj_host.cpp list_walk_pairs: the images of a pair-keyed list
// variable, include/laspj.h "pair-keyed list variables") driven from a file of images, as a
// program of its own so that it can be built with the host sanitizers
// (tests/test_lvar_products_abi.py writes the file, builds and runs this; nothing here touches
// a GPU).
//
// Lines of the file: `V <hex>` an image the walk takes — its items must carry the pair bits,
// and list_write must give the image back byte for byte; `R <hex>` one it refuses — the
// dictionary then holds what it held before (elements and token bytes).  Every image goes
// through a fresh dictionary and through one shared by all lines.

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../lasp_amd/csrc/laspj_internal.h"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return out;
}

struct Mark {
    uint32_t n = 0;
    uint64_t eb = 0, tb = 0;
    bool operator==(const Mark& o) const { return n == o.n && eb == o.eb && tb == o.tb; }
};

static Mark mark(const laspj_dict* d) {
    Mark m;
    laspj_dict_info(d, &m.n, &m.eb, &m.tb);
    return m;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string kind, hex;
    laspj_dict* shared = nullptr;
    if (laspj_dict_create(&shared) != LASPJ_OK) return 2;
    int lines = 0, bad = 0;
    while (in >> kind >> hex) {
        ++lines;
        // a heap copy of exactly the image's length: a read past it is the sanitizer's to find
        const std::vector<uint8_t> img = unhex(hex);
        laspj_dict* fresh = nullptr;
        if (laspj_dict_create(&fresh) != LASPJ_OK) return 2;
        for (laspj_dict* d : {fresh, shared}) {
            const Mark before = mark(d);
            laspj::ListItems it;
            const int st = laspj::list_walk_pairs(d, img.data(), img.size(), &it);
            if (kind == "V") {
                std::string back;
                bool ok = st == LASPJ_DEC_OK && it.toff.size() == it.keys.size() + 1 &&
                          it.toff.back() == it.toks.size();
                for (uint64_t k : it.keys) ok = ok && (k & LASPJ_LIST_PAIR);
                for (uint64_t t : it.toks) ok = ok && (t & LASPJ_LIST_COMPOUND);
                ok = ok && laspj::list_write(d, LASPJ_KIND_ORSET, it, &back) == LASPJ_OK &&
                     back.size() == img.size() && std::equal(img.begin(), img.end(), back.begin(),
                                                             [](uint8_t a, char b) { return a == (uint8_t)b; });
                if (!ok) {
                    std::printf("line %d: a valid image did not round-trip (st %d)\n", lines, st);
                    ++bad;
                }
            } else if (st == LASPJ_DEC_OK || !(mark(d) == before)) {
                std::printf("line %d: a refused image was taken or left registrations (st %d)\n",
                            lines, st);
                ++bad;
            }
        }
        laspj_dict_destroy(fresh);
    }
    laspj_dict_destroy(shared);
    std::printf("%d lines, %d bad\n", lines, bad);
    return bad ? 1 : 0;
}
