// score_host_check.cpp -- csrc/score_host.h (the sequence grouping, slot plan and row / target tables of
// qasr_score) as a stand-alone program, with no device and no Python: tests/test_score_host.py reads its
// output, and a build with -fsanitize=address,undefined runs the same code under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -Iqwen3-asr.cpp_amd/csrc tools/score_host_check.cpp -o score_host_check
//   ./score_host_check --self 2000          fixed cases + 2000 randomised plans, every one checked (exit 0 = clean)
//   ./score_host_check cases.txt            print the plans of the cases in the file
// A case, whitespace separated:  S include_eos pool max_batch eos_id  clips[S]  n_tokens[S]  P[pool]  tokens[sum n_tokens]
// (P[i]: prompt length of staged clip i).  Output per case: "error <message>", or
//   plan D G n_out
//   seq s group slot out_off n_out            (S lines)
//   p1 row target out                         (pass 1: rows of the prompts' prefill)
//   chunk seq len slot pos0                   (pass 2: the chunk prefill's sequences)
//   p2 row target out                         (pass 2 rows)
//   fork parent from to                       (D * G lines)
// Every printed plan is also checked (check_plan below); a failed check exits 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <random>
#include <string>

#include "score_host.h"

using namespace qasr;

static int fail_at(const char *what, int s) {
    fprintf(stderr, "check failed: %s (sequence %d)\n", what, s);
    return 1;
}

// every (context row, target) pair exactly once; every slot inside its group and used once; offsets contiguous
static int check_plan(const ScorePlan &p, const std::vector<int> &clips, const std::vector<int> &nt, const std::vector<int> &Pclip,
                      const std::vector<int32_t> &tokens, int32_t eos_id, int max_batch) {
    const int S = (int)clips.size();
    if (p.S != S || p.D <= 0 || p.G <= 0 || p.G > kScoreMaxHyp || p.D * p.G > max_batch) return fail_at("plan shape", -1);
    std::vector<int> P(p.D);
    for (int d = 0; d < p.D; d++) P[d] = Pclip[p.clip[d]];
    std::vector<char> slot_used((size_t)p.D * p.G, 0);
    long off = 0, toff = 0;
    for (int s = 0; s < S; s++) {
        const int d = p.group[s];
        if (d < 0 || d >= p.D || p.clip[d] != clips[s]) return fail_at("group", s);
        if (p.slot[s] < d * p.G || p.slot[s] >= (d + 1) * p.G) return fail_at("slot outside its group", s);
        if (slot_used[p.slot[s]]++) return fail_at("slot used twice", s);
        if (p.out_off[s] != off || p.tok_off[s] != toff) return fail_at("offsets not contiguous", s);
        off += nt[s] + p.eos;
        toff += nt[s];
    }
    if (p.out_off[S] != off) return fail_at("output total", -1);
    for (int d = 0; d < p.D; d++)
        for (int e = 0; e < d; e++)
            if (p.clip[d] == p.clip[e]) return fail_at("a clip in two groups", -1);
    // expected (context, target) of every output entry: context = (sequence, tokens fed before it)
    std::vector<int> seen((size_t)off, 0);
    const ScoreRows r1 = score_rows_prompt(p, P.data(), tokens.data(), nt.data(), eos_id);
    std::vector<int> last(p.D);
    int acc = 0;
    for (int d = 0; d < p.D; d++) { acc += P[d]; last[d] = acc - 1; }
    for (size_t i = 0; i < r1.size(); i++) {
        int s = 0;
        while (s < S && !(p.out_off[s] == r1.out[i] && p.n_out(s) > 0)) s++;
        if (s == S) return fail_at("pass 1 output not a sequence's first entry", -1);
        if (r1.row[i] != last[p.group[s]]) return fail_at("pass 1 row", s);
        if (r1.target[i] != (nt[s] > 0 ? tokens[p.tok_off[s]] : eos_id)) return fail_at("pass 1 target", s);
        seen[r1.out[i]]++;
    }
    const ScoreChunk ch = score_chunk(p, P.data(), tokens.data(), nt.data(), eos_id);
    int row0 = 0;
    size_t ri = 0;
    for (size_t k = 0; k < ch.len.size(); k++) {
        const int s = ch.seq[k];
        if (ch.slot[k] != p.slot[s] || ch.pos0[k] != P[p.group[s]]) return fail_at("chunk slot / pos0", s);
        if (ch.len[k] != (p.eos ? nt[s] : nt[s] - 1) || ch.len[k] <= 0) return fail_at("chunk length", s);
        for (int t = 0; t < ch.len[k]; t++, ri++) {
            if (ch.ids[row0 + t] != tokens[p.tok_off[s] + t]) return fail_at("chunk token", s);
            if (ri >= ch.rows.size() || ch.rows.row[ri] != row0 + t) return fail_at("pass 2 row", s);
            if (ch.rows.target[ri] != (t + 1 < nt[s] ? tokens[p.tok_off[s] + t + 1] : eos_id)) return fail_at("pass 2 target", s);
            if (ch.rows.out[ri] != p.out_off[s] + t + 1) return fail_at("pass 2 output", s);
            seen[ch.rows.out[ri]]++;
        }
        row0 += ch.len[k];
    }
    if (ri != ch.rows.size() || row0 != (int)ch.ids.size()) return fail_at("pass 2 totals", -1);
    for (long o = 0; o < off; o++)
        if (seen[o] != 1) return fail_at("an output entry not produced exactly once", (int)o);
    std::vector<int> parent, from, to;
    score_fork(p, P.data(), parent, from, to);
    for (int b = 0; b < p.D * p.G; b++) {
        const int d = b / p.G, j = b % p.G;
        if (parent[b] != d * p.G || from[b] != 0) return fail_at("fork parent", b);
        if (to[b] != ((j > 0 && j < p.count[d]) ? P[d] : 0)) return fail_at("fork range", b);
    }
    return 0;
}

static void print_plan(const ScorePlan &p, const std::vector<int> &Pclip, const std::vector<int> &nt, const std::vector<int32_t> &tokens,
                       int32_t eos_id) {
    std::vector<int> P(p.D);
    for (int d = 0; d < p.D; d++) P[d] = Pclip[p.clip[d]];
    printf("plan %d %d %ld\n", p.D, p.G, p.out_off[p.S]);
    for (int s = 0; s < p.S; s++) printf("seq %d %d %d %ld %d\n", s, p.group[s], p.slot[s], p.out_off[s], p.n_out(s));
    const ScoreRows r1 = score_rows_prompt(p, P.data(), tokens.data(), nt.data(), eos_id);
    for (size_t i = 0; i < r1.size(); i++) printf("p1 %d %d %d\n", r1.row[i], r1.target[i], r1.out[i]);
    const ScoreChunk ch = score_chunk(p, P.data(), tokens.data(), nt.data(), eos_id);
    for (size_t k = 0; k < ch.len.size(); k++) printf("chunk %d %d %d %d\n", ch.seq[k], ch.len[k], ch.slot[k], ch.pos0[k]);
    for (size_t i = 0; i < ch.rows.size(); i++) printf("p2 %d %d %d\n", ch.rows.row[i], ch.rows.target[i], ch.rows.out[i]);
    std::vector<int> parent, from, to;
    score_fork(p, P.data(), parent, from, to);
    for (size_t b = 0; b < parent.size(); b++) printf("fork %d %d %d\n", parent[b], from[b], to[b]);
}

// 0 = as expected (a valid plan that passes its checks, or an error where want_error)
static int one(const std::vector<int> &clips, const std::vector<int> &nt, int eos, int pool, int max_batch, bool want_error,
               const char *name) {
    std::vector<int> Pclip(pool);
    for (int i = 0; i < pool; i++) Pclip[i] = 20 + 3 * i;
    long total = 0;
    for (int v : nt) total += v > 0 ? v : 0;
    std::vector<int32_t> tokens((size_t)total);
    for (long i = 0; i < total; i++) tokens[i] = (int32_t)(1000 + i);
    ScorePlan p;
    std::string err;
    const bool ok = score_plan(clips.data(), nt.data(), (int)clips.size(), eos, pool, max_batch, p, err);
    if (ok == want_error) {
        fprintf(stderr, "case %s: %s\n", name, ok ? "accepted, an error was expected" : err.c_str());
        return 1;
    }
    if (!ok) return 0;
    if (check_plan(p, clips, nt, Pclip, tokens, 7, max_batch)) {
        fprintf(stderr, "case %s failed its checks\n", name);
        return 1;
    }
    return 0;
}

static int self_check(int n_random) {
    int bad = 0;
    // sequences of one clip not adjacent in the input
    bad += one({2, 0, 2, 1, 0, 2}, {3, 1, 4, 1, 5, 9}, 1, 3, 16, false, "interleaved");
    // 1, 8 and 9 hypotheses of a clip
    bad += one({0}, {5}, 1, 1, 1, false, "one");
    bad += one(std::vector<int>(8, 1), {1, 2, 3, 4, 5, 6, 7, 8}, 0, 2, 8, false, "eight");
    bad += one(std::vector<int>(9, 1), std::vector<int>(9, 2), 1, 2, 64, true, "nine");
    // D x G against max_batch: 2 clips x 3 = 6
    bad += one({0, 1, 0, 0}, {1, 1, 1, 1}, 1, 2, 6, false, "fits");
    bad += one({0, 1, 0, 0}, {1, 1, 1, 1}, 1, 2, 5, true, "too many slots");
    // an empty hypothesis with and without EOS
    bad += one({0, 0}, {0, 3}, 1, 1, 2, false, "empty with eos");
    bad += one({0, 0}, {0, 3}, 0, 1, 2, false, "empty without eos");
    bad += one({0}, {0}, 0, 1, 1, false, "nothing to score");
    bad += one({0, 0}, {1, 1}, 0, 1, 2, false, "single tokens without eos");
    // bad clip indices and counts
    bad += one({0, 3}, {1, 1}, 1, 3, 8, true, "clip outside the pool");
    bad += one({-1}, {1}, 1, 3, 8, true, "negative clip");
    bad += one({0}, {-2}, 1, 3, 8, true, "negative count");
    std::mt19937 rng(12345);
    for (int it = 0; it < n_random; it++) {
        const int pool = 1 + (int)(rng() % 6), S = 1 + (int)(rng() % 24), eos = (int)(rng() % 2);
        std::vector<int> clips(S), nt(S), per(pool, 0);
        for (int s = 0; s < S; s++) {
            clips[s] = (int)(rng() % pool);
            nt[s] = (int)(rng() % 7) == 0 ? 0 : (int)(rng() % 12);
            per[clips[s]]++;
        }
        int D = 0, G = 0;
        for (int v : per) { D += v > 0; G = v > G ? v : G; }
        const int max_batch = 1 + (int)(rng() % 48);
        const bool want_error = G > kScoreMaxHyp || D * G > max_batch;
        bad += one(clips, nt, eos, pool, max_batch, want_error, "random");
    }
    if (bad) fprintf(stderr, "%d case(s) failed\n", bad);
    else printf("score_host_check: 13 fixed cases and %d random plans clean\n", n_random);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && std::string(argv[1]) == "--self") return self_check(atoi(argv[2]));
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.txt | --self <random plans>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int S, eos, pool, max_batch, eos_id;
    while (in >> S >> eos >> pool >> max_batch >> eos_id) {
        if (S <= 0 || S > 4096 || pool <= 0 || pool > 4096) {
            fprintf(stderr, "bad case header\n");
            return 2;
        }
        std::vector<int> clips(S), nt(S), Pclip(pool);
        for (int &v : clips) in >> v;
        for (int &v : nt) in >> v;
        for (int &v : Pclip) in >> v;
        long total = 0;
        for (int v : nt) total += v > 0 ? v : 0;
        std::vector<int32_t> tokens((size_t)total);
        for (int32_t &v : tokens) in >> v;
        if (!in) {
            fprintf(stderr, "short case\n");
            return 2;
        }
        ScorePlan p;
        std::string err;
        if (!score_plan(clips.data(), nt.data(), S, eos, pool, max_batch, p, err)) {
            printf("error %s\n", err.c_str());
            continue;
        }
        if (check_plan(p, clips, nt, Pclip, tokens, eos_id, max_batch)) return 1;
        print_plan(p, Pclip, nt, tokens, eos_id);
    }
    return 0;
}
