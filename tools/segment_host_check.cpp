// segment_host_check.cpp -- csrc/segment_host.h (the rule of the pause segmentation of long recordings, DESIGN.md
// §5.9) as a stand-alone program, with no device and no Python, so the host sanitizers can run over it:
//   g++ -std=c++17 -g -fsanitize=address,undefined -Iqwen3-asr.cpp_amd/csrc tools/segment_host_check.cpp -o segment_host_check
//   ./segment_host_check
// It checks every range of the validation, and the rule against a naive restatement (each window and each segment
// scanned from scratch, differently indexed) over random and degenerate inputs in exact buffers, so a read or write
// outside them is the sanitizer's to report: (max, min, H) = (8, 3, 2) for F = 0 .. 25 and 100 with and without a
// 37-sample tail, H = 0 and 64, digital silence (the larger-frame tie: a cut every max_frames), a planted pause
// (the cut is frame 154), the segment invariants (min .. max frames each, the samples tiled exactly) and the silent
// flags at skip_ratio -1, 0, 1e-6.  Prints "segment_host_check OK" and returns 0, or the failures and 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "segment_host.h"

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

static uint64_t bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, [0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

// samples whose amplitude spans several decades, in an exactly sized buffer
static std::vector<float> recording(int64_t n) {
    std::vector<float> x((size_t)n);
    for (auto &v : x) v = (float)((uniform() * 2.0 - 1.0) * std::exp(-6.0 * uniform()));
    return x;
}

// the rule once more: e from the sample's side, s from the term's side, every window and segment from scratch
static void rule_again(const std::vector<float> &x, const SegmentParams &p, SegmentTable &t, std::vector<double> &s) {
    const int64_t n = (int64_t)x.size(), F = n / 160;
    std::vector<double> e((size_t)F, 0.0);
    for (int64_t j = 0; j < F * 160; j++) e[(size_t)(j / 160)] = e[(size_t)(j / 160)] + (double)x[(size_t)j] * (double)x[(size_t)j];
    s.assign((size_t)F, 0.0);
    for (int64_t d = -p.smooth_half; d <= p.smooth_half; d++)   // ascending d is ascending k for every f
        for (int64_t f = 0; f < F; f++)
            if (f + d >= 0 && f + d < F) s[(size_t)f] = s[(size_t)f] + e[(size_t)(f + d)];
    t = SegmentTable();
    t.cuts.push_back(0);
    while (F - t.cuts.back() > p.max_frames) {
        const int64_t a = t.cuts.back(), lo = a + p.min_frames, hi = std::min<int64_t>(a + p.max_frames, F - p.min_frames);
        int64_t c = hi;
        for (int64_t f = hi; f >= lo; f--)   // from the top: only a strictly smaller value moves the cut down
            if (s[(size_t)f] < s[(size_t)c]) c = f;
        t.cuts.push_back((int)c);
    }
    for (double v : s) t.peak_rec = std::max(t.peak_rec, v);
    for (size_t k = 0; k < t.cuts.size(); k++) {
        const int64_t b = t.cuts[k], e2 = k + 1 < t.cuts.size() ? t.cuts[k + 1] : F;
        double m = 0.0;
        for (int64_t f = e2 - 1; f >= b; f--) m = std::max(m, s[(size_t)f]);
        t.peak.push_back(m);
        t.silent.push_back(p.skip_ratio >= 0.0 && m <= p.skip_ratio * t.peak_rec ? 1 : 0);
    }
}

static void compare(const std::vector<float> &x, const SegmentParams &p, const char *what) {
    SegmentTable a, b;
    std::vector<double> e, s, s2;
    segment_rule(x.data(), (int64_t)x.size(), p, a, &e, &s);
    rule_again(x, p, b, s2);
    const int64_t n = (int64_t)x.size(), F = n / 160;
    CHECK((int64_t)s.size() == F && (int64_t)e.size() == F, "%s n %lld", what, (long long)n);
    for (int64_t f = 0; f < F; f++) CHECK(bits(s[(size_t)f]) == bits(s2[(size_t)f]), "%s n %lld frame %lld", what, (long long)n, (long long)f);
    CHECK(a.cuts == b.cuts, "%s n %lld: cuts differ", what, (long long)n);
    CHECK(a.silent == b.silent, "%s n %lld: silent flags differ", what, (long long)n);
    CHECK(a.peak.size() == b.peak.size() && bits(a.peak_rec) == bits(b.peak_rec), "%s n %lld: peaks differ", what, (long long)n);
    for (size_t k = 0; k < std::min(a.peak.size(), b.peak.size()); k++) CHECK(bits(a.peak[k]) == bits(b.peak[k]), "%s n %lld peak %zu", what, (long long)n, k);
    // the invariants: at least one segment, the samples tiled exactly, min .. max frames each when there are several
    const size_t K = a.cuts.size();
    CHECK(K >= 1 && a.cuts[0] == 0 && (int64_t)K <= segment_cap(n, p), "%s n %lld: %zu segments", what, (long long)n, K);
    int64_t at = 0;
    for (size_t k = 0; k < K; k++) {
        CHECK(segment_start(a, k) == at, "%s n %lld segment %zu starts at %lld", what, (long long)n, k, (long long)segment_start(a, k));
        at = segment_end(a, k, n);
        const int64_t fr = (k + 1 < K ? a.cuts[k + 1] : F) - a.cuts[k];
        if (K > 1) CHECK(fr >= p.min_frames && fr <= p.max_frames, "%s n %lld segment %zu has %lld frames", what, (long long)n, k, (long long)fr);
    }
    CHECK(at == n, "%s n %lld: the segments end at %lld", what, (long long)n, (long long)at);
    CHECK((K == 1) == (F <= p.max_frames), "%s n %lld: %zu segments of %lld frames", what, (long long)n, K, (long long)F);
}

int main() {
    // validation
    SegmentParams d;
    CHECK(segment_validate(d).empty() && d.max_frames == 3000 && d.min_frames == 1000 && d.smooth_half == 5 && d.skip_ratio == -1.0, "defaults");
    struct { int mx, mn, h; double r; bool ok; } cases[] = {
        {2, 1, 0, 0.0, true}, {1 << 20, 1 << 19, 64, 1e9, true}, {8, 3, 2, -1.0, true},
        {8, 0, 2, -1.0, false}, {8, -1, 2, -1.0, false}, {5, 3, 2, -1.0, false}, {(1 << 20) + 1, 3, 2, -1.0, false},
        {8, 3, -1, -1.0, false}, {8, 3, 65, -1.0, false}, {8, 3, 2, std::numeric_limits<double>::quiet_NaN(), false},
        {2147483647, 1073741824, 2, -1.0, false}};
    for (const auto &c : cases) {
        SegmentParams p;
        p.max_frames = c.mx; p.min_frames = c.mn; p.smooth_half = c.h; p.skip_ratio = c.r;
        CHECK(segment_validate(p).empty() == c.ok, "validate(%d, %d, %d, %g): %s", c.mx, c.mn, c.h, c.r, segment_validate(p).c_str());
    }
    // random recordings
    SegmentParams small;
    small.max_frames = 8; small.min_frames = 3; small.smooth_half = 2;
    for (int tail : {0, 37})
        for (int F = 0; F <= 101; F++) {
            if (F > 25 && F != 100) continue;
            for (double r : {-1.0, 0.0, 0.25}) {
                small.skip_ratio = r;
                compare(recording(160 * (int64_t)F + tail), small, "random (8, 3, 2)");
            }
        }
    for (int H : {0, 1, 64})
        for (int F : {1, 63, 64, 65, 128, 129, 300}) {
            SegmentParams p;
            p.max_frames = 40; p.min_frames = 10; p.smooth_half = H; p.skip_ratio = 0.01;
            compare(recording(160 * (int64_t)F + 159), p, "random (40, 10, H)");
        }
    compare(std::vector<float>(), small, "empty");
    compare(std::vector<float>(159, 1.0f), small, "no frame");
    // digital silence: the longest segments
    {
        small.skip_ratio = -1.0;
        const std::vector<float> z(160 * 100 + 5, 0.0f);
        SegmentTable t;
        segment_rule(z.data(), (int64_t)z.size(), small, t);
        CHECK(t.cuts.size() == 13, "silence: %zu segments", t.cuts.size());
        for (size_t k = 0; k < t.cuts.size(); k++) CHECK(t.cuts[k] == (int)(8 * k), "silence: cut %zu at %d", k, t.cuts[k]);
        for (int sflag : t.silent) CHECK(sflag == 0, "silence: skip_ratio -1 is never silent");
        compare(z, small, "silence");
        small.skip_ratio = 0.0;
        segment_rule(z.data(), (int64_t)z.size(), small, t);
        for (int sflag : t.silent) CHECK(sflag == 1, "silence: 0 <= 0 * 0 is silent");
    }
    // a planted pause over frames 140 .. 159 of 300: s = 0 on 145 .. 154, the cut is frame 154
    {
        std::vector<float> x = recording(160 * 300);
        for (auto &v : x) v = v == 0.0f ? 0.5f : v;
        for (int j = 160 * 140; j < 160 * 160; j++) x[(size_t)j] = 0.0f;
        SegmentParams p;
        p.max_frames = 200; p.min_frames = 80; p.smooth_half = 5;
        for (double r : {-1.0, 0.0, 1e-6}) {
            p.skip_ratio = r;
            SegmentTable t;
            std::vector<double> s;
            segment_rule(x.data(), (int64_t)x.size(), p, t, nullptr, &s);
            for (int f = 140; f < 160; f++) CHECK((s[(size_t)f] == 0.0) == (f >= 145 && f <= 154), "pause: s[%d] = %g", f, s[(size_t)f]);
            CHECK(t.cuts.size() == 2 && t.cuts[1] == 154, "pause: %zu segments, cut %d", t.cuts.size(), t.cuts.size() > 1 ? t.cuts[1] : -1);
            CHECK(t.silent[0] == 0 && t.silent[1] == 0, "pause: both segments carry signal");
            compare(x, p, "pause");
        }
        // the pause as a segment of its own: silent at 0 and 1e-6, not at -1
        p.max_frames = 20; p.min_frames = 10; p.smooth_half = 0;
        std::vector<float> y(x.begin() + 160 * 120, x.begin() + 160 * 180);   // frames 20 .. 39 of 60 are zero
        for (int j = 160 * 40; j < 160 * 41; j++) y[(size_t)j] = 0.0f;            // ... and frame 40: the tie among 30 .. 40 goes to 40
        for (double r : {-1.0, 0.0, 1e-6}) {
            p.skip_ratio = r;
            SegmentTable t;
            segment_rule(y.data(), (int64_t)y.size(), p, t);
            CHECK(t.cuts.size() == 3 && t.cuts[1] == 20 && t.cuts[2] == 40, "pause segment: cuts");
            if (t.cuts.size() == 3) {
                CHECK(t.peak[1] == 0.0 && t.silent[1] == (r >= 0.0 ? 1 : 0), "pause segment: silent flag at %g", r);
                CHECK(t.silent[0] == 0 && t.silent[2] == 0, "pause segment: its neighbours at %g", r);
            }
            compare(y, p, "pause segment");
        }
    }
    if (fails) {
        std::fprintf(stderr, "%d failure(s)\n", fails);
        return 1;
    }
    std::printf("segment_host_check OK\n");
    return 0;
}
