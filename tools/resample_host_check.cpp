// resample_host_check.cpp -- csrc/resample_host.h (the plan, the tap table and the reference filter of the
// resampler to 16 kHz) as a stand-alone program, with no device and no Python, so the host
// sanitizers can run over it:
//   g++ -std=c++17 -g -fsanitize=address,undefined -Iqwen3-asr.cpp_amd/csrc tools/resample_host_check.cpp -o resample_host_check
//   ./resample_host_check
// It checks, for every supported common rate and 16000: the plan against the rule's integers, the refused rates,
// the output length around n_in = 0, 1, M - 1, M, M + 1, every phase of the table (sum 1 within fp32 rounding,
// zero phase symmetric), and the filter at the edge sizes n_in = 0, 1, 2, H, H + 1, 2H + 1 and a few hundred samples
// against a second, independently indexed evaluation of the rule (exact buffers, so a read or write outside them
// is the sanitizer's to report).  Prints "resample_host_check OK" and returns 0, or the first failure and 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "resample_host.h"

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

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// the rule once more, from the input's side: sample j of x reaches output n through tap k = j - i + H
static void filter_again(const std::vector<float> &x, const ResamplePlan &pl, const std::vector<float> &h, std::vector<float> &out) {
    const int64_t n_in = (int64_t)x.size(), n_out = resample_len64(n_in, pl);
    out.assign((size_t)n_out, 0.f);
    const int T = pl.taps();
    for (int64_t n = 0; n < n_out; n++) {
        const int64_t q = n * pl.M, i = q / pl.L, p = q % pl.L;
        double acc = 0.0;
        for (int64_t j = i - pl.H; j <= i + pl.H; j++) {   // ascending j is ascending k
            const double xv = j >= 0 && j < n_in ? (double)x[(size_t)j] : 0.0;
            acc = acc + (double)h[(size_t)p * T + (size_t)(j - i + pl.H)] * xv;
        }
        out[(size_t)n] = (float)acc;
    }
}

int main() {
    const int rates[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000};
    const int taps_want[] = {69, 69, 69, 1, 93, 103, 135, 185, 203, 369, 403, 737, 803};
    for (int bad : {44101, 0, -1, 3999, 200000, 192001, 16001}) {
        ResamplePlan pl;
        const std::string e = resample_plan(bad, pl);
        CHECK(!e.empty() && e.find(std::to_string(bad)) != std::string::npos, "rate %d not refused by name", bad);
    }
    uint64_t lcg = 12345;
    auto rnd = [&]() {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((double)(lcg >> 11) / 9007199254740992.0 * 2.0 - 1.0);
    };
    for (size_t ri = 0; ri < sizeof rates / sizeof rates[0]; ri++) {
        const int sr = rates[ri];
        ResamplePlan pl;
        CHECK(resample_plan(sr, pl).empty(), "rate %d refused", sr);
        const int g = resample_gcd(16000, sr);
        CHECK(pl.L == 16000 / g && pl.M == sr / g && pl.taps() == taps_want[ri], "rate %d: L %d M %d taps %d", sr, pl.L, pl.M, pl.taps());
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)pl.M - 1, (int64_t)pl.M, (int64_t)pl.M + 1, (int64_t)2147483647}) {
            if (n < 0) continue;
            const int64_t want = (n * pl.L + pl.M - 1) / pl.M;
            CHECK(resample_len64(n, pl) == want && (n == 0) == (want == 0), "rate %d: len(%lld)", sr, (long long)n);
        }
        std::vector<float> h;
        resample_taps(sr, pl, h);
        const int T = pl.taps();
        CHECK((int)h.size() == pl.L * T, "rate %d: table size", sr);
        for (int p = 0; p < pl.L; p++) {
            double sum = 0.0;
            for (int k = 0; k < T; k++) sum += (double)h[(size_t)p * T + k];
            CHECK(std::fabs(sum - 1.0) < 1e-5, "rate %d phase %d: sum %.9g", sr, p, sum);
        }
        for (int k = 0; k < T; k++) CHECK(bits(h[k]) == bits(h[T - 1 - k]), "rate %d: phase 0 not symmetric at %d", sr, k);
        std::vector<float> dev;
        resample_taps_device(pl, h, dev);
        for (int n = 0; n < 3 * pl.L; n += 7)
            CHECK(bits(dev[(size_t)(T / 2) * pl.L + n % pl.L]) == bits(h[(size_t)((int64_t)n * pl.M % pl.L) * T + T / 2]), "rate %d: device layout", sr);
        for (int n_in : {0, 1, 2, pl.H, pl.H + 1, 2 * pl.H + 1, 777}) {
            std::vector<float> x((size_t)n_in), out((size_t)resample_len64(n_in, pl)), again;
            for (float &v : x) v = rnd();
            if (n_in > 0) { x.front() = 1.f; x.back() = 1.f; }
            resample_filter(x.data(), n_in, pl, h.data(), out.data());
            filter_again(x, pl, h, again);
            CHECK(out.size() == again.size(), "rate %d n %d: sizes", sr, n_in);
            for (size_t n = 0; n < out.size(); n++)
                if (bits(out[n]) != bits(again[n])) {
                    CHECK(false, "rate %d n_in %d: output %zu differs", sr, n_in, n);
                    break;
                }
            if (pl.copy())
                for (size_t n = 0; n < out.size(); n++) CHECK(bits(out[n]) == bits(x[n]), "copy differs at %zu", n);
        }
    }
    if (fails) return 1;
    std::printf("resample_host_check OK\n");
    return 0;
}
