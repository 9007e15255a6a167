// phrase_host.h -- the host side of hotword boosting: the ranges of a phrase list and its
// compiler, pure C++ with no device code (tools/phrase_host_check.cpp builds it alone).
//   phrase_check     the ranges of a list; an empty string, or the message naming the violated range
//   phrase_compile   the trie over the phrases, flattened to CSR in breadth-first order (root = node 0): per node
//                    its children child_off[u] .. child_off[u + 1), per edge the token (ascending within a node), the
//                    node it leads to and its bonus.  An edge's raw bonus is the largest boost of the phrases that
//                    run through it; its bonus eff(u, x) is the largest raw bonus of (w, x) over u and every node w
//                    that spells a proper suffix of u's string and has a child x (the Aho-Corasick suffix links,
//                    taken in breadth-first order so a shallower node's eff is final before a deeper one reads it).
//   phrase_bonuses   what the device does with the trie: the nodes the last tokens of a history spell, deepest first,
//                    each child token taken from the deepest node that has it.  With eff this equals the rule's
//                    maximum over all matching (phrase, position) pairs.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace qasr {

constexpr int kPhraseMax = 4096, kPhraseLenMax = 16;
constexpr int kPhraseNodeMax = 65536 + 1, kPhraseEdgeMax = 65536;
constexpr float kPhraseBoostMax = 100.f;

struct PhraseTrieHost {
    std::vector<int32_t> child_off;   // [nodes + 1]
    std::vector<int32_t> tok, dst;    // [edges]
    std::vector<float> bonus;         // [edges] eff
    int nodes() const { return child_off.empty() ? 0 : (int)child_off.size() - 1; }
    int edges() const { return (int)tok.size(); }
};

// vocab <= 0: the ids' upper bound is not checked
inline std::string phrase_check(int n, const int32_t *ids, const int32_t *len, const float *boost, int vocab) {
    if (n < 0 || n > kPhraseMax) return "phrases: n_phrases must be in 0..4096";
    if (n > 0 && (!ids || !len || !boost)) return "phrases: n_phrases > 0 without ids, len and boost";
    size_t at = 0;
    for (int k = 0; k < n; k++) {
        if (len[k] < 1 || len[k] > kPhraseLenMax) return "phrases: the length of phrase " + std::to_string(k) + " must be in 1..16";
        for (int j = 0; j < len[k]; j++, at++)
            if (ids[at] < 0 || (vocab > 0 && ids[at] >= vocab))
                return "phrases: id " + std::to_string(ids[at]) + " of phrase " + std::to_string(k) + " outside the vocabulary";
        if (!(boost[k] > 0.f && boost[k] <= kPhraseBoostMax)) return "phrases: the boost of phrase " + std::to_string(k) + " must be in (0, 100]";
    }
    return "";
}

// a checked list (phrase_check) -> its trie; an empty string, or the message of the limit it exceeds
inline std::string phrase_compile(int n, const int32_t *ids, const int32_t *len, const float *boost, PhraseTrieHost &out) {
    out = PhraseTrieHost();
    if (n <= 0) return "";
    struct Edge { int dst; float raw; };
    std::vector<std::map<int32_t, Edge>> kids(1);
    std::vector<int> parent(1, -1);
    std::vector<int32_t> via(1, -1);
    size_t at = 0;
    for (int k = 0; k < n; k++) {
        int u = 0;
        for (int j = 0; j < len[k]; j++, at++) {
            auto it = kids[u].find(ids[at]);
            if (it == kids[u].end()) {
                if ((int)kids.size() - 1 >= kPhraseEdgeMax || (int)kids.size() >= kPhraseNodeMax)
                    return "phrases: the trie exceeds 65536 edges (65537 nodes)";
                it = kids[u].emplace(ids[at], Edge{(int)kids.size(), boost[k]}).first;
                kids.emplace_back();
                parent.push_back(u);
                via.push_back(ids[at]);
            } else if (boost[k] > it->second.raw) {
                it->second.raw = boost[k];
            }
            u = it->second.dst;
        }
    }
    const int N = (int)kids.size();
    // breadth-first order and the suffix links
    std::vector<int> order(1, 0), link(N, 0);
    order.reserve(N);
    for (size_t i = 0; i < order.size(); i++)
        for (const auto &e : kids[order[i]]) order.push_back(e.second.dst);
    for (int i = 1; i < N; i++) {
        const int v = order[i], u = parent[v];
        int w = u;
        link[v] = 0;
        while (w != 0) {
            w = link[w];
            auto it = kids[w].find(via[v]);
            if (it != kids[w].end()) { link[v] = it->second.dst; break; }
        }
    }
    // eff along the suffix links: the nearest proper suffix of u that has a child x holds the maximum below it
    std::vector<std::map<int32_t, float>> eff(N);
    for (int i = 0; i < N; i++) {
        const int u = order[i];
        for (const auto &e : kids[u]) {
            float b = e.second.raw;
            for (int w = u; w != 0;) {
                w = link[w];
                auto it = eff[w].find(e.first);
                if (it != eff[w].end()) { b = std::max(b, it->second); break; }
            }
            eff[u][e.first] = b;
        }
    }
    // CSR, the nodes renumbered in breadth-first order
    std::vector<int> id(N);
    for (int i = 0; i < N; i++) id[order[i]] = i;
    out.child_off.assign(N + 1, 0);
    out.tok.reserve(N - 1); out.dst.reserve(N - 1); out.bonus.reserve(N - 1);
    for (int i = 0; i < N; i++) {
        const int u = order[i];
        for (const auto &e : kids[u]) {
            out.tok.push_back(e.first);
            out.dst.push_back(id[e.second.dst]);
            out.bonus.push_back(eff[u][e.first]);
        }
        out.child_off[i + 1] = (int32_t)out.tok.size();
    }
    return "";
}

// child x of node u, or -1 (a binary search, as the device's)
inline int phrase_child(const PhraseTrieHost &tr, int u, int32_t x) {
    int lo = tr.child_off[u], hi = tr.child_off[u + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tr.tok[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < tr.child_off[u + 1] && tr.tok[lo] == x ? lo : -1;
}

// the (token, bonus) pairs of history h[0 .. t), in ascending token order: "the deepest matched node that has
// child x decides"
inline std::vector<std::pair<int32_t, float>> phrase_bonuses(const PhraseTrieHost &tr, const int32_t *h, int t) {
    std::map<int32_t, float> got;
    if (tr.nodes() == 0) return {};
    const int m = std::min(t, kPhraseLenMax - 1);
    for (int j = m; j >= 0; j--) {   // deepest first
        int u = 0;
        for (int i = 0; i < j && u >= 0; i++) {
            const int e = phrase_child(tr, u, h[t - j + i]);
            u = e < 0 ? -1 : tr.dst[e];
        }
        if (u < 0) continue;
        for (int e = tr.child_off[u]; e < tr.child_off[u + 1]; e++) got.emplace(tr.tok[e], tr.bonus[e]);   // (a marked token is skipped)
    }
    return std::vector<std::pair<int32_t, float>>(got.begin(), got.end());
}

}  // namespace qasr
