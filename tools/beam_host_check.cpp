// beam_host_check.cpp -- csrc/beam_host.h (the back-tracking and ranking of a beam run) as a stand-alone
// program, with no device and no Python: tests/test_beam_host.py holds its output to the numpy rule, and a
// build with -fsanitize=address,undefined runs the same cases under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -Iqwen3-asr.cpp_amd/csrc tools/beam_host_check.cpp -o beam_host_check
//   ./beam_host_check cases.txt
// Input, whitespace separated, any number of cases (floats as the hex of their fp32 bits):
//   W row0 T stride n_fin done
//   h_par[T * stride]  h_id[T * stride]  h_lp[T * stride]
//   cum[row0 + W]  fin_row[row0 + W]  fin_t[row0 + W]  fin_sum[row0 + W]  fin_lp[row0 + W]
// Output per case: "case <hypotheses>", then per hypothesis "finished n sum n_tokens | tokens | logprobs".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "beam_host.h"

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

template <class T>
static bool read_ints(std::istream &in, std::vector<T> &v, size_t n) {
    v.resize(n);
    for (T &x : v) {
        long long k;
        if (!(in >> k)) return false;
        x = (T)k;
    }
    return true;
}
static bool read_floats(std::istream &in, std::vector<float> &v, size_t n) {
    v.resize(n);
    for (float &x : v) {
        std::string s;
        if (!(in >> s)) return false;
        x = bits_f((uint32_t)std::stoul(s, nullptr, 16));
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    qasr::BeamGroup g;
    while (in >> g.W >> g.row0 >> g.T >> g.stride >> g.n_fin >> g.done) {
        if (g.W < 1 || g.W > 8 || g.row0 < 0 || g.T < 0 || g.stride < g.row0 + g.W || g.n_fin < 0 || g.n_fin > g.W) {
            fprintf(stderr, "bad case header\n");
            return 2;
        }
        const size_t H = (size_t)g.T * g.stride, R = (size_t)g.row0 + g.W;
        std::vector<int> h_par, fin_row, fin_t;
        std::vector<int32_t> h_id;
        std::vector<float> h_lp, cum, fin_sum, fin_lp;
        if (!read_ints(in, h_par, H) || !read_ints(in, h_id, H) || !read_floats(in, h_lp, H) || !read_floats(in, cum, R) ||
            !read_ints(in, fin_row, R) || !read_ints(in, fin_t, R) || !read_floats(in, fin_sum, R) || !read_floats(in, fin_lp, R)) {
            fprintf(stderr, "short case\n");
            return 2;
        }
        g.h_par = h_par.data(); g.h_id = h_id.data(); g.h_lp = h_lp.data(); g.cum = cum.data();
        g.fin_row = fin_row.data(); g.fin_t = fin_t.data(); g.fin_sum = fin_sum.data(); g.fin_lp = fin_lp.data();
        const std::vector<qasr::BeamHyp> hs = qasr::beam_hypotheses(g);
        printf("case %zu\n", hs.size());
        for (const qasr::BeamHyp &h : hs) {
            printf("%d %d %08x %zu |", h.finished, h.n, f_bits(h.sum), h.tokens.size());
            for (int32_t t : h.tokens) printf(" %d", t);
            printf(" |");
            for (float l : h.logprobs) printf(" %08x", f_bits(l));
            printf("\n");
        }
    }
    return 0;
}
