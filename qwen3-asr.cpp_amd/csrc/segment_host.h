// segment_host.h -- the host side of the pause segmentation of long recordings: the rule in full
// and a plain reference of it, pure C++ with no device code (tools/segment_host_check.cpp builds it alone).
//
// The rule.  The input is a recording of n samples at 16 kHz, fp32, finite.  F = n / 160 frames (the mel hop, so a
// cut is a mel-frame boundary).  Parameters: max_frames, min_frames, smooth_half = H, skip_ratio.
//   1. frame energy     e[f] = sum_{i = 0 .. 159} double(x[160 f + i])^2, fp64, in ascending i.  The square of an
//                       fp32 is exact in fp64, so a fused multiply-add gives the bits of a multiply and an add.
//   2. smoothed energy  s[f] = sum_{k = max(0, f - H) .. min(F - 1, f + H)} e[k], fp64, in ascending k.
//   3. cuts             a = 0, cuts = [0]; while F - a > max_frames:
//                         lo = a + min_frames, hi = min(a + max_frames, F - min_frames),
//                         c = the frame of [lo, hi] with the smallest s, EQUAL VALUES TO THE LARGER f,
//                         append c, a = c.
//                       (Digital silence then yields the longest segments: all-zero input with (8, 3, 2) cuts every
//                       8 frames.  This differs on purpose from argmax_key's lower-id tie.)
//   4. segments         segment k covers samples [160 cuts[k], 160 cuts[k + 1]), the last one ends at n (the n % 160
//                       tail samples are its).  Every recording has at least one segment, n < 160 and n = 0 included.
//   5. peaks, silence   peak[k] = the maximum of s over the segment's frames (0 when it has none), peak_rec = the
//                       maximum of s over the recording.  With skip_ratio >= 0 segment k is silent iff
//                       peak[k] <= skip_ratio * peak_rec (one fp64 multiply, one compare); skip_ratio < 0: never.
// Ranges: 1 <= min_frames, 2 min_frames <= max_frames <= 2^20, 0 <= smooth_half <= 64, skip_ratio not NaN.  With
// 2 min <= max the window [lo, hi] is never empty (F - a > max gives F - min >= a + max - min >= a + min), every
// segment of a multi-segment recording has min .. max frames, and the loop ends.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace qasr {

constexpr int kSegmentHop = 160;
constexpr int kSegmentMaxFramesCap = 1 << 20, kSegmentSmoothCap = 64;

struct SegmentParams {
    int max_frames = 3000, min_frames = 1000, smooth_half = 5;
    double skip_ratio = -1.0;
};

// an empty string, or the message naming the violated range
inline std::string segment_validate(const SegmentParams &p) {
    if (p.min_frames < 1) return "segment: min_frames " + std::to_string(p.min_frames) + " outside 1 <= min_frames";
    if (p.max_frames > kSegmentMaxFramesCap || (int64_t)p.max_frames < 2 * (int64_t)p.min_frames)
        return "segment: max_frames " + std::to_string(p.max_frames) + " outside 2 * min_frames <= max_frames <= 1048576";
    if (p.smooth_half < 0 || p.smooth_half > kSegmentSmoothCap)
        return "segment: smooth_half " + std::to_string(p.smooth_half) + " outside 0 <= smooth_half <= 64";
    if (std::isnan(p.skip_ratio)) return "segment: skip_ratio is NaN";
    return "";
}

inline int64_t segment_frames(int64_t n) { return n / kSegmentHop; }
// an upper bound of a recording's segments (every segment but the last has at least min_frames)
inline int64_t segment_cap(int64_t n, const SegmentParams &p) { return segment_frames(n) / p.min_frames + 1; }

inline void segment_energy(const float *x, int64_t n, std::vector<double> &e) {
    const int64_t F = segment_frames(n);
    e.assign((size_t)F, 0.0);
    for (int64_t f = 0; f < F; f++) {
        double acc = 0.0;
        for (int i = 0; i < kSegmentHop; i++) {
            const double d = (double)x[f * kSegmentHop + i];
            acc = acc + d * d;
        }
        e[(size_t)f] = acc;
    }
}

inline void segment_smooth(const std::vector<double> &e, int H, std::vector<double> &s) {
    const int64_t F = (int64_t)e.size();
    s.assign((size_t)F, 0.0);
    for (int64_t f = 0; f < F; f++) {
        double acc = 0.0;
        for (int64_t k = std::max<int64_t>(0, f - H); k <= std::min<int64_t>(F - 1, f + H); k++) acc = acc + e[(size_t)k];
        s[(size_t)f] = acc;
    }
}

struct SegmentTable {
    std::vector<int> cuts;       // first frame of every segment (cuts[0] = 0)
    std::vector<double> peak;    // per segment
    std::vector<int> silent;     // per segment, 0 / 1
    double peak_rec = 0.0;
};

// the silent flag of a peak (step 5)
inline int segment_silent(double peak, double peak_rec, double skip_ratio) {
    return skip_ratio >= 0.0 && peak <= skip_ratio * peak_rec ? 1 : 0;
}

// steps 3 and 5 over a recording's smoothed energy
inline void segment_cuts(const std::vector<double> &s, const SegmentParams &p, SegmentTable &t) {
    const int64_t F = (int64_t)s.size();
    t = SegmentTable();
    int64_t a = 0;
    t.cuts.push_back(0);
    while (F - a > p.max_frames) {
        const int64_t lo = a + p.min_frames, hi = std::min<int64_t>(a + p.max_frames, F - p.min_frames);
        int64_t c = lo;
        for (int64_t f = lo + 1; f <= hi; f++)
            if (s[(size_t)f] <= s[(size_t)c]) c = f;
        t.cuts.push_back((int)c);
        a = c;
    }
    const size_t K = t.cuts.size();
    t.peak.assign(K, 0.0);
    for (size_t k = 0; k < K; k++) {
        const int64_t b = t.cuts[k], e = k + 1 < K ? t.cuts[k + 1] : F;
        double m = 0.0;
        for (int64_t f = b; f < e; f++) m = s[(size_t)f] > m ? s[(size_t)f] : m;
        t.peak[k] = m;
        t.peak_rec = m > t.peak_rec ? m : t.peak_rec;
    }
    t.silent.resize(K);
    for (size_t k = 0; k < K; k++) t.silent[k] = segment_silent(t.peak[k], t.peak_rec, p.skip_ratio);
}

// the whole rule: x[n] -> the segment table (and e, s when asked for)
inline void segment_rule(const float *x, int64_t n, const SegmentParams &p, SegmentTable &t, std::vector<double> *e_out = nullptr,
                         std::vector<double> *s_out = nullptr) {
    std::vector<double> e, s;
    segment_energy(x, n, e);
    segment_smooth(e, p.smooth_half, s);
    segment_cuts(s, p, t);
    if (e_out) e_out->swap(e);
    if (s_out) s_out->swap(s);
}

// samples of segment k of a recording of n samples
inline int64_t segment_start(const SegmentTable &t, size_t k) { return (int64_t)t.cuts[k] * kSegmentHop; }
inline int64_t segment_end(const SegmentTable &t, size_t k, int64_t n) {
    return k + 1 < t.cuts.size() ? (int64_t)t.cuts[k + 1] * kSegmentHop : n;
}

}  // namespace qasr
