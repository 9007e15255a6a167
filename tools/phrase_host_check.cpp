// phrase_host_check.cpp -- csrc/phrase_host.h (the ranges and the trie compiler of hotword boosting, DESIGN.md
// §5.7) as a stand-alone program, with no device and no Python: tests/test_phrase_host.py holds its output to the
// brute-force numpy rule, and a build with -fsanitize=address,undefined runs the same cases under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -Iqwen3-asr.cpp_amd/csrc tools/phrase_host_check.cpp -o phrase_host_check
//   ./phrase_host_check cases.txt [--no-ranges]
// --no-ranges hands the lists to the compiler unchecked (its own limits are then what refuses one).
// Input, whitespace separated, any number of cases (floats as the hex of their fp32 bits):
//   n_phrases vocab n_hist
//   per phrase:   len boost ids[len]
//   per history:  t ids[t]
// Output per case: "case ok <nodes> <edges>" or "case err <message>" (then nothing more for the case); per
// history "hist <pairs> | token:bonus ..." in ascending token order, as the trie's "deepest node decides" gives.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "phrase_host.h"

static float bits_f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t f_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char **argv) {
    const bool ranges = !(argc == 3 && !strcmp(argv[2], "--no-ranges"));
    if (argc != 2 && ranges) {
        fprintf(stderr, "usage: %s cases.txt [--no-ranges]\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    long long n, vocab, n_hist;
    while (in >> n >> vocab >> n_hist) {
        if (n < 0 || n > 1000000 || n_hist < 0) {
            fprintf(stderr, "bad case header\n");
            return 2;
        }
        std::vector<int32_t> ids, len;
        std::vector<float> boost;
        for (long long k = 0; k < n; k++) {
            long long l;
            std::string b;
            if (!(in >> l >> b) || l < 0 || l > 1000) {
                fprintf(stderr, "short case\n");
                return 2;
            }
            len.push_back((int32_t)l);
            boost.push_back(bits_f((uint32_t)std::stoul(b, nullptr, 16)));
            for (long long j = 0; j < l; j++) {
                long long x;
                if (!(in >> x)) {
                    fprintf(stderr, "short case\n");
                    return 2;
                }
                ids.push_back((int32_t)x);
            }
        }
        std::vector<std::vector<int32_t>> hist((size_t)n_hist);
        for (auto &h : hist) {
            long long t;
            if (!(in >> t) || t < 0) {
                fprintf(stderr, "short case\n");
                return 2;
            }
            h.resize((size_t)t);
            for (int32_t &x : h) {
                long long v;
                if (!(in >> v)) {
                    fprintf(stderr, "short case\n");
                    return 2;
                }
                x = (int32_t)v;
            }
        }
        qasr::PhraseTrieHost tr;
        std::string err = ranges ? qasr::phrase_check((int)n, ids.data(), len.data(), boost.data(), (int)vocab) : std::string();
        if (err.empty()) err = qasr::phrase_compile((int)n, ids.data(), len.data(), boost.data(), tr);
        if (!err.empty()) {
            printf("case err %s\n", err.c_str());
            continue;
        }
        printf("case ok %d %d\n", tr.nodes(), tr.edges());
        for (const auto &h : hist) {
            const auto got = qasr::phrase_bonuses(tr, h.data(), (int)h.size());
            printf("hist %zu |", got.size());
            for (const auto &p : got) printf(" %d:%08x", p.first, f_bits(p.second));
            printf("\n");
        }
    }
    return 0;
}
