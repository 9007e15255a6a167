// align_path_host.h -- the host side of the forced aligner's monotone path: the rule in full and a
// plain reference of it, pure C++ with no device code (tools/align_path_host_check.cpp builds it alone).
//
// The rule.  One clip has NT timestamp rows in prompt order; z[i][c] is the fp32 classify-head logit of row i and
// class c, 0 <= c < classify_num, finite (a -0 counts as +0).  C classes are allowed (align_path_classes below).
//   dp[0][c] = z[0][c]                                                   for c < C
//   dp[i][c] = z[i][c] + m[i][c], one fp32 add, m[i][c] = max_{c' <= c} dp[i-1][c'],
//   bp[i][c] = the SMALLEST c' attaining that maximum
//   path[NT-1] = the smallest c attaining max_c dp[NT-1][c]; path[i-1] = bp[i][path[i]]; score = dp[NT-1][path[NT-1]]
//   logprob[i] = z[i][path[i]] - lse_i, lse_i = mx + log(sum_c exp(z[i][c] - mx)) over ALL classify_num classes, fp32,
//                mx the row's maximum
// path and score are exact functions of z; lse alone depends on the order of its sum.  NT = 0 yields nothing.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace qasr {

constexpr int kAlignPathMaxClasses = 8192;

// the classes a clip of n_samples at 16 kHz may take: the last one is the first class at or past the audio's end
inline int align_path_classes(int classify_num, int n_samples, int ts_segment_ms) {
    return (int)std::min<int64_t>(classify_num, (int64_t)n_samples / (16 * (int64_t)ts_segment_ms) + 2);
}

// the rule on the CPU.  logits [NT][ld], ld >= classify_num >= C >= 1.  path [NT], logprob [NT], score [1] (each
// may be null); false (nothing written) for arguments outside those ranges
inline bool align_path_host(const float *logits, int64_t ld, int NT, int classify_num, int C, int32_t *path, float *logprob,
                            float *score) {
    if (NT < 0 || C < 1 || C > classify_num || classify_num > ld || (NT > 0 && !logits)) return false;
    if (NT == 0) return true;
    std::vector<float> dp(logits, logits + C);
    std::vector<int32_t> bp((size_t)NT * C, 0);
    for (int i = 1; i < NT; i++) {
        const float *z = logits + (int64_t)i * ld;
        float m = dp[0];
        int arg = 0;
        for (int c = 0; c < C; c++) {
            if (dp[c] > m) { m = dp[c]; arg = c; }   // strict: equal values keep the smaller class
            bp[(size_t)i * C + c] = arg;
            dp[c] = z[c] + m;                        // (dp[c] is read above before it is replaced)
        }
    }
    int cur = 0;
    for (int c = 1; c < C; c++)
        if (dp[c] > dp[cur]) cur = c;
    if (score) *score = dp[cur];
    std::vector<int32_t> p(NT);
    for (int i = NT - 1; i >= 0; i--) {
        p[i] = cur;
        if (i) cur = bp[(size_t)i * C + cur];
    }
    for (int i = 0; i < NT; i++) {
        if (path) path[i] = p[i];
        if (!logprob) continue;
        const float *z = logits + (int64_t)i * ld;
        float mx = z[0];
        for (int c = 1; c < classify_num; c++) mx = std::max(mx, z[c]);
        float s = 0.0f;
        for (int c = 0; c < classify_num; c++) s += std::exp(z[c] - mx);
        logprob[i] = z[p[i]] - (mx + std::log(s));
    }
    return true;
}

}  // namespace qasr
