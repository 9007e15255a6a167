// score_host.h -- the host arithmetic of qasr_score (DESIGN.md "Teacher-forced scoring"): the grouping of
// the caller's sequences by clip, the KV-cache slot plan and the (row, target, output) tables of the two
// scoring passes.  Plain C++ with no device dependency: tools/score_host_check.cpp runs it under the
// sanitizers.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace qasr {

constexpr int kScoreMaxHyp = 8;   // hypotheses of one clip a call (launch_kv_fork's largest group)

// Sequence s = n_tokens[s] tokens of clip clips[s].  The D distinct clips, in order of first appearance,
// each own a group of G consecutive cache slots, G = the largest number of hypotheses of one clip: the
// clip's prompt is prefilled into the group's first slot, hypothesis j of the clip continues in slot
// d * G + j.
struct ScorePlan {
    int S = 0, D = 0, G = 0, eos = 0;   // eos: 1 = every sequence ends with a scored EOS
    std::vector<int> clip;              // [D] the distinct clips
    std::vector<int> count;             // [D] hypotheses of each
    std::vector<int> group, slot;       // [S] the sequence's group d and cache slot d * G + j
    std::vector<long> tok_off;          // [S] first token of the sequence in the caller's tokens
    std::vector<long> out_off;          // [S + 1] first output entry of the sequence; [S] = their number
    int n_out(int s) const { return (int)(out_off[s + 1] - out_off[s]); }
};

// false: the arguments are not valid (err says why), the plan is unspecified.  pool: staged clips.
inline bool score_plan(const int *clips, const int *n_tokens, int S, int include_eos, int pool, int max_batch, ScorePlan &p,
                       std::string &err) {
    p = ScorePlan();
    if (!clips || !n_tokens || S <= 0) { err = "bad arguments"; return false; }
    p.S = S;
    p.eos = include_eos ? 1 : 0;
    p.group.resize(S); p.slot.resize(S); p.tok_off.resize(S); p.out_off.resize((size_t)S + 1);
    std::vector<int> which;   // [S] index of the hypothesis inside its clip
    which.resize(S);
    long toks = 0, outs = 0;
    for (int s = 0; s < S; s++) {
        if (n_tokens[s] < 0) { err = "negative token count"; return false; }
        if (clips[s] < 0 || clips[s] >= pool) { err = "staged clip index out of range"; return false; }
        int d = 0;
        while (d < p.D && p.clip[d] != clips[s]) d++;
        if (d == p.D) { p.clip.push_back(clips[s]); p.count.push_back(0); p.D++; }
        if (p.count[d] == kScoreMaxHyp) { err = "more than 8 hypotheses of one clip"; return false; }
        which[s] = p.count[d]++;
        p.group[s] = d;
        p.tok_off[s] = toks;
        p.out_off[s] = outs;
        toks += n_tokens[s];
        outs += n_tokens[s] + p.eos;
    }
    p.out_off[S] = outs;
    for (int d = 0; d < p.D; d++) p.G = p.count[d] > p.G ? p.count[d] : p.G;
    if ((long)p.D * p.G > max_batch) { err = "distinct clips x hypotheses of one clip exceed the context's max_batch"; return false; }
    for (int s = 0; s < S; s++) p.slot[s] = p.group[s] * p.G + which[s];
    return true;
}

// one scoring pass: hidden row `row` of the pass's prefill against `target`, the result to output entry `out`
struct ScoreRows {
    std::vector<int> row, out;
    std::vector<int32_t> target;
    size_t size() const { return row.size(); }
};

// Pass 1, after the prompts' prefill (clip d's prompt the d-th sequence, P[d] rows): the last row of
// clip d's prompt against the first token of each of its hypotheses (the EOS for an empty one).
inline ScoreRows score_rows_prompt(const ScorePlan &p, const int *P, const int32_t *tokens, const int *n_tokens, int32_t eos_id) {
    ScoreRows r;
    std::vector<int> last(p.D);
    int acc = 0;
    for (int d = 0; d < p.D; d++) { acc += P[d]; last[d] = acc - 1; }
    for (int s = 0; s < p.S; s++) {
        if (p.n_out(s) == 0) continue;
        r.row.push_back(last[p.group[s]]);
        r.target.push_back(n_tokens[s] > 0 ? tokens[p.tok_off[s]] : eos_id);
        r.out.push_back((int)p.out_off[s]);
    }
    return r;
}

// Pass 2, one chunk prefill after the prompts: the sequences that feed tokens, in input order, each in its
// own slot at positions P[group] ..; a sequence feeds its first n_tokens - 1 tokens, and the last one too
// when the EOS is scored.  Row t of a sequence is scored against its token t + 1 (the EOS after the last).
struct ScoreChunk {
    std::vector<int32_t> ids;        // the chunks' tokens back to back
    std::vector<int> len, slot, pos0, seq;   // per chunk: rows, cache slot, cached positions, the sequence
    ScoreRows rows;
};
inline ScoreChunk score_chunk(const ScorePlan &p, const int *P, const int32_t *tokens, const int *n_tokens, int32_t eos_id) {
    ScoreChunk c;
    for (int s = 0; s < p.S; s++) {
        const int n = n_tokens[s], feed = p.eos ? n : n - 1;
        if (feed <= 0) continue;
        const int row0 = (int)c.ids.size();
        for (int t = 0; t < feed; t++) {
            c.ids.push_back(tokens[p.tok_off[s] + t]);
            c.rows.row.push_back(row0 + t);
            c.rows.target.push_back(t + 1 < n ? tokens[p.tok_off[s] + t + 1] : eos_id);
            c.rows.out.push_back((int)p.out_off[s] + t + 1);
        }
        c.len.push_back(feed);
        c.slot.push_back(p.slot[s]);
        c.pos0.push_back(P[p.group[s]]);
        c.seq.push_back(s);
    }
    return c;
}

// the fork that gives every hypothesis its clip's prompt: rows of D * G slots in groups of G
inline void score_fork(const ScorePlan &p, const int *P, std::vector<int> &parent, std::vector<int> &from, std::vector<int> &to) {
    const int B = p.D * p.G;
    parent.assign(B, 0); from.assign(B, 0); to.assign(B, 0);
    for (int b = 0; b < B; b++) {
        const int d = b / p.G, j = b % p.G;
        parent[b] = d * p.G;
        if (j > 0 && j < p.count[d]) to[b] = P[d];   // (the others: from == to, a no-op)
    }
}

}  // namespace qasr
