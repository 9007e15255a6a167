// align_path_host_check.cpp -- csrc/align_path_host.h (the rule of the forced aligner's monotone path, DESIGN.md
// §5.11) as a stand-alone program, with no device and no Python, so the host sanitizers can run over it:
//   g++ -std=c++17 -g -fsanitize=address,undefined -Iqwen3-asr.cpp_amd/csrc tools/align_path_host_check.cpp -o align_path_host_check
//   ./align_path_host_check
// It runs the rule on fixed inputs in exactly sized buffers, so a read or write outside them is the sanitizer's to
// report, against a naive restatement (every prefix maximum scanned from scratch, in float64 on logits whose sums
// are exact): NT = 0, 1, 2 and 9; C = 1, C = classify_num and C in between; an all-equal row and an all-equal
// input (every tie to the smallest class); ld larger than classify_num; the refused argument ranges; the class
// bound of a clip's duration.  Prints "align_path_host_check OK" and returns 0, or the failures and 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "align_path_host.h"

using namespace qasr;

static int fails = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::fprintf(stderr, "FAIL %s: ", #cond);      \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
            fails++;                                       \
        }                                                  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// multiples of 0.25 in [-4, 4]: every add of the programme is exact in fp32 and fp64 alike
static std::vector<float> logits(int NT, int ld) {
    std::vector<float> z((size_t)NT * ld);
    for (auto &v : z) v = 0.25f * (float)((int)(next_u32() % 33u) - 16);
    return z;
}

// the rule once more: float64, every maximum from scratch, the path from the stored arg-maxima
static void rule_again(const std::vector<float> &z, int ld, int NT, int C, std::vector<int> &path, double &score) {
    std::vector<double> dp((size_t)NT * C);
    std::vector<int> bp((size_t)NT * C, 0);
    for (int c = 0; c < C; c++) dp[c] = z[c];
    for (int i = 1; i < NT; i++)
        for (int c = 0; c < C; c++) {
            int arg = 0;
            for (int k = 1; k <= c; k++)
                if (dp[(size_t)(i - 1) * C + k] > dp[(size_t)(i - 1) * C + arg]) arg = k;
            bp[(size_t)i * C + c] = arg;
            dp[(size_t)i * C + c] = (double)z[(size_t)i * ld + c] + dp[(size_t)(i - 1) * C + arg];
        }
    int cur = 0;
    for (int c = 1; c < C; c++)
        if (dp[(size_t)(NT - 1) * C + c] > dp[(size_t)(NT - 1) * C + cur]) cur = c;
    score = dp[(size_t)(NT - 1) * C + cur];
    path.assign(NT, 0);
    for (int i = NT - 1; i >= 0; i--) {
        path[i] = cur;
        if (i) cur = bp[(size_t)i * C + cur];
    }
}

static void one_case(int NT, int N, int ld, int C, int flat_row) {
    std::vector<float> z = logits(NT, ld);
    if (flat_row >= 0 && flat_row < NT)
        for (int c = 0; c < ld; c++) z[(size_t)flat_row * ld + c] = 1.25f;
    std::vector<int32_t> path((size_t)NT);
    std::vector<float> lp((size_t)NT);
    float score = -1.0f;
    CHECK(align_path_host(NT ? z.data() : nullptr, ld, NT, N, C, NT ? path.data() : nullptr, NT ? lp.data() : nullptr, &score),
          "NT %d N %d C %d", NT, N, C);
    if (NT == 0) {
        CHECK(score == -1.0f, "NT 0 wrote a score");
        return;
    }
    std::vector<int> want;
    double wscore = 0.0;
    rule_again(z, ld, NT, C, want, wscore);
    CHECK((double)score == wscore, "NT %d C %d: score %g, want %g", NT, C, (double)score, wscore);
    for (int i = 0; i < NT; i++) {
        CHECK(path[i] == want[i], "NT %d C %d row %d: class %d, want %d", NT, C, i, path[i], want[i]);
        CHECK(i == 0 || path[i] >= path[i - 1], "NT %d C %d row %d: not monotone", NT, C, i);
        double mx = z[(size_t)i * ld], s = 0.0;
        for (int c = 1; c < N; c++) mx = std::max(mx, (double)z[(size_t)i * ld + c]);
        for (int c = 0; c < N; c++) s += std::exp((double)z[(size_t)i * ld + c] - mx);
        const double ref = (double)z[(size_t)i * ld + path[i]] - (mx + std::log(s));
        CHECK(std::fabs((double)lp[i] - ref) <= 1e-5 && lp[i] <= 0.0f, "NT %d C %d row %d: logprob %g, want %g", NT, C, i, (double)lp[i], ref);
    }
}

int main() {
    for (int NT : {0, 1, 2, 9})
        for (int C : {1, 5, 12}) {
            one_case(NT, 12, 12, C, -1);
            one_case(NT, 12, 17, C, 1);   // ld past classify_num, row 1 all equal
        }
    {   // all equal: every tie to the smallest class, the score the sum, the log-probability -log(N)
        const int NT = 6, N = 8;
        std::vector<float> z((size_t)NT * N, 0.5f);
        std::vector<int32_t> path(NT);
        std::vector<float> lp(NT);
        float score = 0.f;
        CHECK(align_path_host(z.data(), N, NT, N, N, path.data(), lp.data(), &score), "all equal");
        for (int i = 0; i < NT; i++) CHECK(path[i] == 0 && std::fabs(lp[i] + std::log(8.0f)) < 1e-6f, "all equal row %d: %d %g", i, path[i], (double)lp[i]);
        CHECK(score == 3.0f, "all equal score %g", (double)score);
        CHECK(align_path_host(z.data(), N, NT, N, N, nullptr, nullptr, nullptr), "null outputs");
    }
    {
        std::vector<float> z(2 * 6, 0.f);
        int32_t p[2];
        CHECK(!align_path_host(z.data(), 6, 2, 6, 0, p, nullptr, nullptr), "C = 0 accepted");
        CHECK(!align_path_host(z.data(), 6, 2, 6, 7, p, nullptr, nullptr), "C > classify_num accepted");
        CHECK(!align_path_host(z.data(), 6, 2, 9, 3, p, nullptr, nullptr), "classify_num > ld accepted");
        CHECK(!align_path_host(z.data(), 6, -1, 6, 3, p, nullptr, nullptr), "NT < 0 accepted");
        CHECK(!align_path_host(nullptr, 6, 2, 6, 3, p, nullptr, nullptr), "null logits accepted");
    }
    // 30 s at 80 ms a class: classes 0 .. 376; 300 s: 0 .. 3751; a head of 5000 classes bounds a long clip
    CHECK(align_path_classes(5000, 30 * 16000, 80) == 377, "%d", align_path_classes(5000, 30 * 16000, 80));
    CHECK(align_path_classes(5000, 300 * 16000, 80) == 3752, "%d", align_path_classes(5000, 300 * 16000, 80));
    CHECK(align_path_classes(5000, 2000000000, 80) == 5000, "%d", align_path_classes(5000, 2000000000, 80));
    CHECK(align_path_classes(5000, 1, 80) == 2, "%d", align_path_classes(5000, 1, 80));
    if (fails) {
        std::fprintf(stderr, "align_path_host_check: %d failure(s)\n", fails);
        return 1;
    }
    std::printf("align_path_host_check OK\n");
    return 0;
}
