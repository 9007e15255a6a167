// resample_host.h -- the host side of the resampler to 16 kHz: the plan of a rate, its tap table
// and a plain reference filter, pure C++ with no device code (tools/resample_host_check.cpp builds it alone).
//
// The rule, for an input rate sr (every quantity below in fp64 unless said otherwise):
//   g = gcd(16000, sr), L = 16000 / g, M = sr / g.  sr == 16000 is a plain copy (no filter).
//   supported: 4000 <= sr <= 192000 with L <= 640.
//   s = min(1, 16000 / sr) * ROLL, H = ceil(Z / s), with Z = 32, BETA = 9.0, ROLL = 0.96.
//   n_out = (n_in * L + M - 1) / M in 64-bit arithmetic.
//   tap table h[p][k], p = 0 .. L-1, k = 0 .. 2H:
//     d = (k - H) - p / L, u = d / (H + 1),
//     w = I0(BETA * sqrt(1 - u^2)) / I0(BETA) for |u| < 1, else 0,
//     raw = s * sinc(s * d) * w, sinc(x) = sin(pi x) / (pi x);
//     a phase is divided by the sum of its raw values (summed in order of k), then rounded to fp32.
//   output n: q = n * M (64-bit), i = q / L, p = q % L; acc = 0; for k = 0 .. 2H in this order
//     acc = acc + (double)h[p][k] * (double)x[i + k - H], x zero outside [0, n_in); the result is (float)acc.
// Both factors are fp32, so the fp64 product is exact and an fma gives the bits of a multiply and an add.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace qasr {

constexpr int kResampleOutRate = 16000;
constexpr int kResampleRateMin = 4000, kResampleRateMax = 192000, kResampleLMax = 640;
constexpr double kResampleZ = 32.0, kResampleBeta = 9.0, kResampleRoll = 0.96;

struct ResamplePlan {
    int L = 1, M = 1, H = 0;
    bool copy() const { return L == 1 && M == 1; }
    int taps() const { return 2 * H + 1; }
};

inline int resample_gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

// the plan of a rate; an empty string, or the message naming the refused rate
inline std::string resample_plan(int rate, ResamplePlan &out) {
    const std::string bad = "resample: unsupported sample rate " + std::to_string(rate) +
                            " Hz (4000..192000 with 16000 / gcd(16000, rate) <= 640)";
    if (rate < kResampleRateMin || rate > kResampleRateMax) return bad;
    const int g = resample_gcd(kResampleOutRate, rate);
    out.L = kResampleOutRate / g;
    out.M = rate / g;
    if (out.L > kResampleLMax) return bad;
    if (out.copy()) { out.H = 0; return ""; }
    const double s = std::fmin(1.0, (double)kResampleOutRate / (double)rate) * kResampleRoll;
    out.H = (int)std::ceil(kResampleZ / s);
    return "";
}

// output samples of n_in input samples (n_in >= 0), 64-bit
inline int64_t resample_len64(int64_t n_in, const ResamplePlan &pl) { return (n_in * pl.L + pl.M - 1) / pl.M; }

// modified Bessel function of the first kind, order 0: its power series sum ((x/2)^j / j!)^2 until a term no
// longer changes the sum
inline double resample_i0(double x) {
    const double y = x * x / 4.0;
    double sum = 1.0, term = 1.0;
    for (int j = 1; j < 1000; j++) {
        term *= y / ((double)j * (double)j);
        const double next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}

// the tap table h[p][k] of a rate ([L][2H + 1], fp32); a copy plan has the one tap 1
inline void resample_taps(int rate, const ResamplePlan &pl, std::vector<float> &h) {
    const int T = pl.taps();
    h.assign((size_t)pl.L * T, 0.f);
    if (pl.copy()) { h[0] = 1.f; return; }
    const double pi = 3.14159265358979323846;
    const double s = std::fmin(1.0, (double)kResampleOutRate / (double)rate) * kResampleRoll;
    const double i0b = resample_i0(kResampleBeta);
    std::vector<double> raw(T);
    for (int p = 0; p < pl.L; p++) {
        double sum = 0.0;
        for (int k = 0; k < T; k++) {
            const double d = (double)(k - pl.H) - (double)p / (double)pl.L;
            const double u = d / (double)(pl.H + 1);
            double w = 0.0;
            if (std::fabs(u) < 1.0) w = resample_i0(kResampleBeta * std::sqrt(1.0 - u * u)) / i0b;
            const double x = s * d;
            const double sinc = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
            raw[k] = s * sinc * w;
            sum += raw[k];
        }
        for (int k = 0; k < T; k++) h[(size_t)p * T + k] = (float)(raw[k] / sum);
    }
}

// the table as the kernel reads it (kernels.h ResampleClip): [2H + 1][L], entry [k][r] = h[(r * M) % L][k]
inline void resample_taps_device(const ResamplePlan &pl, const std::vector<float> &h, std::vector<float> &dev) {
    const int T = pl.taps();
    dev.resize(h.size());
    for (int k = 0; k < T; k++)
        for (int r = 0; r < pl.L; r++) dev[(size_t)k * pl.L + r] = h[(size_t)((int64_t)r * pl.M % pl.L) * T + k];
}

// the rule, output by output: x[n_in] at the plan's rate -> out[resample_len64(n_in)] with the table h
inline void resample_filter(const float *x, int64_t n_in, const ResamplePlan &pl, const float *h, float *out) {
    const int64_t n_out = resample_len64(n_in, pl);
    if (pl.copy()) {
        for (int64_t n = 0; n < n_out; n++) out[n] = x[n];
        return;
    }
    const int T = pl.taps();
    for (int64_t n = 0; n < n_out; n++) {
        const int64_t q = n * pl.M, i = q / pl.L;
        const float *hp = h + (size_t)(q % pl.L) * T;
        double acc = 0.0;
        for (int k = 0; k < T; k++) {
            const int64_t j = i + k - pl.H;
            const double xv = j >= 0 && j < n_in ? (double)x[j] : 0.0;
            acc = acc + (double)hp[k] * xv;
        }
        out[n] = (float)acc;
    }
}

}  // namespace qasr
