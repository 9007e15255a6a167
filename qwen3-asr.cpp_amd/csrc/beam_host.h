// beam_host.h -- the host end of a beam run: the back-pointer history and the finished table a
// group left on the device, back-tracked into token sequences and ranked (DESIGN.md "Beam search").
// Plain C++ with no device dependency: tools/beam_host_check.cpp runs it under the sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace qasr {

struct BeamHyp {
    std::vector<int32_t> tokens;   // a finished hypothesis' EOS is popped ...
    std::vector<float> logprobs;   // ... with its value, one per token
    float sum = 0.f;               // summed log-probability, the EOS step included
    int n = 0;                     // steps summed (tokens + the popped EOS)
    int finished = 0;
};

// what one group (rows row0 .. row0 + W - 1) left after T beam steps, as host copies of the device arrays
struct BeamGroup {
    int W = 0, row0 = 0, T = 0;
    int stride = 0;                        // rows of one history slot
    const int *h_par = nullptr;            // [T][stride] parent row (absolute)
    const int32_t *h_id = nullptr;
    const float *h_lp = nullptr;
    const float *cum = nullptr;            // [rows]
    const int *fin_row = nullptr, *fin_t = nullptr;   // [rows], this group's entries at row0
    const float *fin_sum = nullptr, *fin_lp = nullptr;
    int n_fin = 0, done = 0;
};

// row `row` as it stood after step t: its t + 1 tokens and their log-probabilities, oldest first
inline void beam_backtrack(const BeamGroup &g, int row, int t, std::vector<int32_t> &tok, std::vector<float> &lp) {
    tok.assign((size_t)t + 1, 0);
    lp.assign((size_t)t + 1, 0.f);
    for (int s = t; s >= 0; s--) {
        const size_t at = (size_t)s * g.stride + row;
        tok[s] = g.h_id[at];
        lp[s] = g.h_lp[at];
        row = g.h_par[at];
    }
}

// The group's hypotheses, best first, at most W: the finished table in record order, then -- unless the
// table filled (done) -- the live rows by row as unfinished ones with sum = cum and n = T; ranked by
// sum / n in fp32, descending, ties in the order just given (a stable sort).
inline std::vector<BeamHyp> beam_hypotheses(const BeamGroup &g) {
    std::vector<BeamHyp> all;
    for (int e = 0; e < g.n_fin; e++) {
        BeamHyp h;
        const int t = g.fin_t[g.row0 + e];
        // (the EOS itself is popped: its step is counted in n and sum only)
        if (t > 0) beam_backtrack(g, g.fin_row[g.row0 + e], t - 1, h.tokens, h.logprobs);
        h.sum = g.fin_sum[g.row0 + e];
        h.n = t + 1;
        h.finished = 1;
        all.push_back(std::move(h));
    }
    if (!g.done && g.T > 0)
        for (int b = 0; b < g.W; b++) {
            BeamHyp h;
            beam_backtrack(g, g.row0 + b, g.T - 1, h.tokens, h.logprobs);
            h.sum = g.cum[g.row0 + b];
            h.n = g.T;
            all.push_back(std::move(h));
        }
    std::stable_sort(all.begin(), all.end(), [](const BeamHyp &a, const BeamHyp &b) { return a.sum / (float)a.n > b.sum / (float)b.n; });
    if ((int)all.size() > g.W) all.resize(g.W);
    return all;
}

}  // namespace qasr
