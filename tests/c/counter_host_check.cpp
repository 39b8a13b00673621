// The counter image codec (laspj_counter_host.cpp over laspj_host.cpp) driven from a file of
// images, as a program of its own so that it can be built with the host sanitizers
// (tests/test_counter_host.py builds and runs it; nothing here touches a GPU).
//
// Lines of the file: `V <hex>` an image the parser takes (it must parse, and encode back
// byte for byte), `R <hex>` one it refuses, `T <hex>` a truncated one; after a refusal the
// dictionary holds what it held before.  Every image also goes through the threshold
// planner, as a threshold of both kinds.

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/laspj.h"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return out;
}

static uint32_t size_of(const laspj_dict* d) {
    uint32_t e = 0;
    uint64_t eb = 0, tb = 0;
    laspj_dict_info(d, &e, &eb, &tb);
    return e;
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
        const std::vector<uint8_t> img = unhex(hex == "-" ? "" : hex);
        laspj_dict* fresh = nullptr;
        if (laspj_dict_create(&fresh) != LASPJ_OK) return 2;
        for (laspj_dict* d : {fresh, shared}) {
            const uint32_t before = size_of(d);
            std::vector<uint32_t> slots(4096);
            std::vector<uint64_t> counts(4096);
            uint32_t n = 0;
            int32_t st = -1;
            const int rc = laspj_gcounter_etf_parse(d, img.empty() ? (const uint8_t*)"" : img.data(),
                                                    img.size(), slots.data(), counts.data(), 4096,
                                                    &n, &st);
            if (kind == "V") {
                std::vector<uint8_t> back(img.size() + 16);
                uint64_t len = 0;
                // (the shared dictionary may refuse an actor `==` to another image's: not here)
                if (rc != LASPJ_OK || st != LASPJ_DEC_OK ||
                    laspj_gcounter_etf_encode(d, slots.data(), counts.data(), n, back.data(),
                                              back.size(), &len) != LASPJ_OK ||
                    len != img.size() || !std::equal(img.begin(), img.end(), back.begin())) {
                    if (d == fresh || st != LASPJ_DEC_EQUAL_TERMS) {
                        std::printf("line %d: a valid image did not round-trip (rc %d st %d)\n", lines, rc, st);
                        ++bad;
                    }
                }
            } else if (rc != LASPJ_OK || st == LASPJ_DEC_OK || n != 0 || size_of(d) != before) {
                std::printf("line %d: a refused image was taken (rc %d st %d)\n", lines, rc, st);
                ++bad;
            }
        }
        laspj_dict_destroy(fresh);
        for (int strict = 0; strict < 2; ++strict) {
            int32_t plan = -1;
            uint64_t t = 0;
            laspj_gcounter_threshold_plan(img.empty() ? (const uint8_t*)"" : img.data(), img.size(),
                                          strict, &plan, &t);
        }
    }
    laspj_dict_destroy(shared);
    std::printf("%d lines, %d bad\n", lines, bad);
    return bad || !lines ? 1 : 0;
}
