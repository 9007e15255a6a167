// main.cpp -- qwen3-asr-cli: the three modes of src/main.cpp (transcription
// :361-414, forced alignment --align :301-359, transcribe + align -a :416-500)
// with the same flags and output, plus MI355X additions: --device, batch file
// lists (-f may repeat, --file-list, transcription mode), --devices to shard a
// file list over several GPUs (one host thread and model replica per GPU,
// longest-first assignment: the sharded counterpart of the reference's shell
// loop, docs/usage.md:240-252), --synthetic to write a synthetic GGUF
// (tiny|full|aligner|aligner-tiny) for testing.
#include <algorithm>
#include <atomic>
#include <cctype>
#include <climits>
#include <cmath>
#include <chrono>
#include <sys/stat.h>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "forced_aligner.h"
#include "qasr_capi.h"
#include "qwen3_asr.h"

struct cli_params {
    std::string model_path = "models/qwen3-asr-0.6b-f16.gguf";
    std::string aligner_model_path;
    std::vector<std::string> audio_paths;
    std::string output_path, language, synthetic, align_text;
    int32_t max_tokens = 1024, n_threads = 4, device = 0, batch = 16;
    std::vector<int> devices;   // --devices: shard the files over these GPUs
    bool print_progress = false, print_timing = true, print_tokens = false, profile = false;
    bool resample = false;   // --resample: files at other rates go through the device resampler
    bool logprobs = false;   // --logprobs: per-token log-probabilities (transcribe_params::token_logprobs)
    int32_t top_k = 0;       // --top-k: alternatives per token (transcribe_params::top_k)
    int32_t beam_width = 0;  // --beam-width: beam search of this width (transcribe_params::beam_width)
    bool beams = false;      // --beams: list every hypothesis of a beam run
    float temperature = 0.f, min_p = 0.f;   // --temperature / --min-p / --seed / --n-best: sampling (transcribe_params)
    uint64_t seed = 0;
    int32_t n_best = 1;
    // --no-repeat-ngram / --repetition-penalty / --penalty-last-n / --suppress-tokens / --token-bias: decoding constraints
    int32_t no_repeat_ngram = 0, penalty_last_n = 0;
    float repetition_penalty = 1.f;
    std::vector<int32_t> suppress_tokens;
    std::vector<std::pair<int32_t, float>> token_bias;
    // --hotword / --hotwords-file / --hotword-boost: hotword boosting (a boost <= 0: --hotword-boost's)
    std::vector<std::string> hotwords;
    std::vector<float> hotword_boosts;
    float hotword_boost = 5.f;
    // --long / --segment-max / --segment-min / --skip-silence / --segments: one -f recording of any length, cut at its
    // pauses on the device (Qwen3ASR::transcribe_long)
    bool long_mode = false, print_segments = false;
    double segment_max_s = 30.0, segment_min_s = 10.0, skip_silence_db = 1.0;   // (skip_silence_db > 0: nothing skipped)
    std::vector<std::string> score_texts;   // --score: texts scored as transcripts of the -f file (Qwen3ASR::score)
    bool align_mode = false, transcribe_align_mode = false;
};

static void usage(const char *prog) {
    fprintf(stderr, "Usage: %s [options]\n\nOptions:\n", prog);
    fprintf(stderr, "  -m, --model <path>     Path to GGUF model (default: models/qwen3-asr-0.6b-f16.gguf)\n");
    fprintf(stderr, "  -f, --audio <path>     Path to audio file (WAV, 16kHz mono) [required; repeat for a batch]\n");
    fprintf(stderr, "  -o, --output <path>    Output file path (default: stdout)\n");
    fprintf(stderr, "  -l, --language <code>  Language code (optional, e.g. 'korean' for Korean word splitting)\n");
    fprintf(stderr, "  -t, --threads <n>      Number of threads (accepted for compatibility)\n");
    fprintf(stderr, "  --max-tokens <n>       Maximum tokens to generate (default: 1024)\n");
    fprintf(stderr, "  --progress             Print progress during transcription\n");
    fprintf(stderr, "  --no-timing            Don't print timing information\n");
    fprintf(stderr, "  --resample             Accept WAV files at 8 / 11.025 / 12 / 22.05 / 24 / 32 / 44.1 / 48 / 88.2 / 96 / 176.4 / 192 kHz:\n");
    fprintf(stderr, "                         resampled to 16 kHz on the GPU (transcription, --align, --transcribe-align, --file-list, --devices)\n");
    fprintf(stderr, "  --tokens               Print token IDs\n");
    fprintf(stderr, "  --logprobs             Per-token log-probabilities: avg / min per file, and with --tokens each token's\n");
    fprintf(stderr, "  --top-k <n>            The n (1..8) most likely tokens of every step; with --tokens, listed under each token\n");
    fprintf(stderr, "  --beam-width <n>       Beam search of width n (2..8) instead of greedy decoding\n");
    fprintf(stderr, "  --beams                With --beam-width: list every hypothesis with its summed log-probability\n");
    fprintf(stderr, "  --temperature <T>      Sample every token from softmax(logits / T), 0 < T <= 100, instead of greedy decoding\n");
    fprintf(stderr, "  --min-p <p>            With --temperature: only tokens at least p (0..1) times as probable as the greedy one\n");
    fprintf(stderr, "  --seed <n>             With --temperature: the 64-bit seed of the draws (default: 0)\n");
    fprintf(stderr, "  --n-best <n>           With --temperature: n (1..8) samples a file; n > 1 lists every sample with its\n");
    fprintf(stderr, "                         summed log-probability (the output is sample 0's text)\n");
    fprintf(stderr, "  --no-repeat-ngram <n>  No n-gram (1..8) of tokens occurs twice in a transcript (0: off)\n");
    fprintf(stderr, "  --repetition-penalty <p>  Penalise tokens already emitted, 0 < p <= 10 (1: off)\n");
    fprintf(stderr, "  --penalty-last-n <n>   With --repetition-penalty: only the last n tokens count (0: all)\n");
    fprintf(stderr, "  --suppress-tokens <id,id,...>  Token ids never emitted\n");
    fprintf(stderr, "  --token-bias <id:val,...>  Add val to the logit of token id before every choice\n");
    fprintf(stderr, "  --hotword <text>       Prefer this word or phrase (repeatable; at most 16 tokens each)\n");
    fprintf(stderr, "  --hotwords-file <path> One hotword a line, optionally a tab and its own boost; lines starting with # are comments\n");
    fprintf(stderr, "  --hotword-boost <b>    Added to the next token's logit while a hotword is being spelled, 0 < b <= 100 (default 5)\n");
    fprintf(stderr, "  --long                 Take the one -f file at any length: cut at its quietest points on the GPU into segments\n");
    fprintf(stderr, "                         that are decoded from the uploaded recording (any --resample rate is accepted)\n");
    fprintf(stderr, "  --segment-max <s>      With --long: the longest segment in seconds (default 30)\n");
    fprintf(stderr, "  --segment-min <s>      With --long: the shortest segment in seconds, at most half of --segment-max (default 10)\n");
    fprintf(stderr, "  --skip-silence <dB>    With --long: do not decode segments whose peak energy is <dB> (<= 0) or more below the recording's\n");
    fprintf(stderr, "  --segments             With --long: one '[start --> end] text' line a segment instead of the joined text\n");
    fprintf(stderr, "  --score <text>         Score <text> as a transcript of the -f file instead of transcribing (repeatable):\n");
    fprintf(stderr, "                         per text the summed log-probability, the mean per token and the token count\n");
    fprintf(stderr, "                         (the EOS included); with --tokens every token's id, text and log-probability,\n");
    fprintf(stderr, "                         and the model's own greedy token where it differs.  The text is scored as\n");
    fprintf(stderr, "                         given: the real model's reply carries its 'language ...<asr_text>' prefix,\n");
    fprintf(stderr, "                         so a text without it is scored as a reply that lacks it\n");
    fprintf(stderr, "  --profile              Print timing profile\n");
    fprintf(stderr, "  --device <n>           HIP device index (default: 0)\n");
    fprintf(stderr, "  --file-list <path>     Text file with one audio path per line (added to the -f files)\n");
    fprintf(stderr, "  --devices <i,j,...>    Shard the audio files over these HIP devices (one replica each)\n");
    fprintf(stderr, "  --batch <n>            KV-cache slots per GPU (continuous batching) with --devices / several files (default: 16)\n");
    fprintf(stderr, "  --synthetic <cfg>      Write a synthetic GGUF (tiny|full|aligner|aligner-tiny) to --model and exit\n");
    fprintf(stderr, "\nForced Alignment:\n");
    fprintf(stderr, "  --align                Enable forced alignment mode\n");
    fprintf(stderr, "  --text <text>          Reference transcript for alignment\n");
    fprintf(stderr, "\nTranscribe + Align:\n");
    fprintf(stderr, "  -a, --transcribe-align Run ASR then forced alignment\n");
    fprintf(stderr, "  --aligner-model <path> Path to forced aligner GGUF model (required with --transcribe-align)\n");
    fprintf(stderr, "\n  -h, --help             Show this help message\n");
}

static bool parse(int argc, char **argv, cli_params &p) {
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        auto val = [&](std::string &dst) {
            if (i + 1 >= argc) { fprintf(stderr, "Error: %s requires an argument\n", a); return false; }
            dst = argv[++i];
            return true;
        };
        std::string v;
        if (!strcmp(a, "-m") || !strcmp(a, "--model")) { if (!val(p.model_path)) return false; }
        else if (!strcmp(a, "-f") || !strcmp(a, "--audio")) { if (!val(v)) return false; p.audio_paths.push_back(v); }
        else if (!strcmp(a, "-o") || !strcmp(a, "--output")) { if (!val(p.output_path)) return false; }
        else if (!strcmp(a, "-l") || !strcmp(a, "--language") || !strcmp(a, "--lang")) { if (!val(p.language)) return false; }
        else if (!strcmp(a, "-t") || !strcmp(a, "--threads")) { if (!val(v)) return false; p.n_threads = atoi(v.c_str()); }
        else if (!strcmp(a, "--max-tokens")) { if (!val(v)) return false; p.max_tokens = atoi(v.c_str()); }
        else if (!strcmp(a, "--device")) { if (!val(v)) return false; p.device = atoi(v.c_str()); }
        else if (!strcmp(a, "--batch")) { if (!val(v)) return false; p.batch = std::max(1, atoi(v.c_str())); }
        else if (!strcmp(a, "--devices")) {
            if (!val(v)) return false;
            for (size_t k = 0; k < v.size();) {
                const size_t e = v.find(',', k);
                p.devices.push_back(atoi(v.substr(k, e == std::string::npos ? std::string::npos : e - k).c_str()));
                if (e == std::string::npos) break;
                k = e + 1;
            }
        }
        else if (!strcmp(a, "--file-list")) {
            if (!val(v)) return false;
            std::ifstream f(v);
            if (!f) { fprintf(stderr, "Error: cannot read file list %s\n", v.c_str()); return false; }
            for (std::string line; std::getline(f, line);) {
                while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
                if (!line.empty()) p.audio_paths.push_back(line);
            }
        }
        else if (!strcmp(a, "--synthetic")) { if (!val(p.synthetic)) return false; }
        else if (!strcmp(a, "--progress")) p.print_progress = true;
        else if (!strcmp(a, "--no-timing")) p.print_timing = false;
        else if (!strcmp(a, "--resample")) p.resample = true;
        else if (!strcmp(a, "--long")) p.long_mode = true;
        else if (!strcmp(a, "--segments")) p.print_segments = true;
        else if (!strcmp(a, "--segment-max")) { if (!val(v)) return false; p.segment_max_s = atof(v.c_str()); }
        else if (!strcmp(a, "--segment-min")) { if (!val(v)) return false; p.segment_min_s = atof(v.c_str()); }
        else if (!strcmp(a, "--skip-silence")) {
            if (!val(v)) return false;
            p.skip_silence_db = atof(v.c_str());
            if (!(p.skip_silence_db <= 0.0)) { fprintf(stderr, "Error: --skip-silence takes a level in dB <= 0\n"); return false; }
        }
        else if (!strcmp(a, "--tokens")) p.print_tokens = true;
        else if (!strcmp(a, "--logprobs")) p.logprobs = true;
        else if (!strcmp(a, "--top-k")) {
            if (!val(v)) return false;
            p.top_k = atoi(v.c_str());
            if (p.top_k < 1 || p.top_k > 8) { fprintf(stderr, "Error: --top-k takes 1..8\n"); return false; }
        }
        else if (!strcmp(a, "--beam-width")) {
            if (!val(v)) return false;
            p.beam_width = atoi(v.c_str());
            if (p.beam_width < 2 || p.beam_width > 8) { fprintf(stderr, "Error: --beam-width takes 2..8\n"); return false; }
        }
        else if (!strcmp(a, "--beams")) p.beams = true;
        else if (!strcmp(a, "--temperature")) {
            if (!val(v)) return false;
            p.temperature = (float)atof(v.c_str());
            if (!(p.temperature > 0.f && p.temperature <= 100.f)) { fprintf(stderr, "Error: --temperature takes 0 < T <= 100\n"); return false; }
        }
        else if (!strcmp(a, "--min-p")) {
            if (!val(v)) return false;
            p.min_p = (float)atof(v.c_str());
            if (!(p.min_p >= 0.f && p.min_p <= 1.f)) { fprintf(stderr, "Error: --min-p takes 0..1\n"); return false; }
        }
        else if (!strcmp(a, "--seed")) { if (!val(v)) return false; p.seed = strtoull(v.c_str(), nullptr, 0); }
        else if (!strcmp(a, "--n-best")) {
            if (!val(v)) return false;
            p.n_best = atoi(v.c_str());
            if (p.n_best < 1 || p.n_best > 8) { fprintf(stderr, "Error: --n-best takes 1..8\n"); return false; }
        }
        else if (!strcmp(a, "--no-repeat-ngram")) {
            if (!val(v)) return false;
            p.no_repeat_ngram = atoi(v.c_str());
            if (p.no_repeat_ngram < 0 || p.no_repeat_ngram > 8) { fprintf(stderr, "Error: --no-repeat-ngram takes 0..8\n"); return false; }
        }
        else if (!strcmp(a, "--repetition-penalty")) {
            if (!val(v)) return false;
            p.repetition_penalty = (float)atof(v.c_str());
            if (!(p.repetition_penalty > 0.f && p.repetition_penalty <= 10.f)) { fprintf(stderr, "Error: --repetition-penalty takes 0 < p <= 10\n"); return false; }
        }
        else if (!strcmp(a, "--hotword")) {
            if (!val(v)) return false;
            if (v.find_first_not_of(" \t\r\n") == std::string::npos) { fprintf(stderr, "Error: --hotword takes a non-empty text\n"); return false; }
            p.hotwords.push_back(v);
            p.hotword_boosts.push_back(0.f);
        }
        else if (!strcmp(a, "--hotword-boost")) {
            if (!val(v)) return false;
            char *tail = nullptr;
            p.hotword_boost = strtof(v.c_str(), &tail);
            if (*tail != 0 || !(p.hotword_boost > 0.f && p.hotword_boost <= 100.f)) { fprintf(stderr, "Error: --hotword-boost takes 0 < b <= 100\n"); return false; }
        }
        else if (!strcmp(a, "--hotwords-file")) {
            if (!val(v)) return false;
            std::ifstream f(v);
            if (!f) { fprintf(stderr, "Error: cannot read hotwords file %s\n", v.c_str()); return false; }
            int no = 0;
            for (std::string line; std::getline(f, line);) {
                no++;
                while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
                if (line.empty() || line[0] == '#') continue;
                float b = 0.f;
                const size_t tab = line.find('\t');
                if (tab != std::string::npos) {
                    char *tail = nullptr;
                    b = strtof(line.c_str() + tab + 1, &tail);
                    if (tail == line.c_str() + tab + 1 || *tail != 0 || !(b > 0.f && b <= 100.f)) {
                        fprintf(stderr, "Error: %s line %d: the boost after the tab takes 0 < b <= 100\n", v.c_str(), no);
                        return false;
                    }
                    line.resize(tab);
                }
                if (line.find_first_not_of(" \t") == std::string::npos) { fprintf(stderr, "Error: %s line %d: no text before the boost\n", v.c_str(), no); return false; }
                p.hotwords.push_back(line);
                p.hotword_boosts.push_back(b);
            }
        }
        else if (!strcmp(a, "--penalty-last-n")) {
            if (!val(v)) return false;
            p.penalty_last_n = atoi(v.c_str());
            if (p.penalty_last_n < 0) { fprintf(stderr, "Error: --penalty-last-n takes 0 or more\n"); return false; }
        }
        else if (!strcmp(a, "--suppress-tokens") || !strcmp(a, "--token-bias")) {
            const bool sup = a[2] == 's';
            if (!val(v)) return false;
            size_t at = 0;
            while (at <= v.size()) {   // id[,id...] or id:val[,id:val...]
                const size_t end = std::min(v.find(',', at), v.size());
                const std::string item = v.substr(at, end - at);
                char *rest = nullptr;
                const long id = strtol(item.c_str(), &rest, 10);
                bool ok = !item.empty() && rest != item.c_str() && id >= 0 && id <= INT32_MAX;
                float b = 0.f;
                if (ok && sup) ok = *rest == 0;
                if (ok && !sup) {
                    char *tail = nullptr;
                    ok = *rest == ':' && rest[1] != 0;
                    if (ok) { b = strtof(rest + 1, &tail); ok = *tail == 0 && (std::isfinite(b) || b == -INFINITY); }
                }
                if (!ok) { fprintf(stderr, sup ? "Error: --suppress-tokens takes id,id,...\n" : "Error: --token-bias takes id:val,...\n"); return false; }
                if (sup) p.suppress_tokens.push_back((int32_t)id);
                else p.token_bias.push_back({(int32_t)id, b});
                at = end + 1;
            }
        }
        else if (!strcmp(a, "--score")) { if (!val(v)) return false; p.score_texts.push_back(v); }
        else if (!strcmp(a, "--profile")) p.profile = true;
        else if (!strcmp(a, "--align")) p.align_mode = true;
        else if (!strcmp(a, "-a") || !strcmp(a, "--transcribe-align")) p.transcribe_align_mode = true;
        else if (!strcmp(a, "--aligner-model")) { if (!val(p.aligner_model_path)) return false; }
        else if (!strcmp(a, "--text")) { if (!val(p.align_text)) return false; }
        else if (!strcmp(a, "-h") || !strcmp(a, "--help")) { usage(argv[0]); exit(0); }
        else { fprintf(stderr, "Error: Unknown argument: %s\n", a); return false; }
    }
    if (!p.synthetic.empty()) return true;
    if (p.audio_paths.empty()) { fprintf(stderr, "Error: Audio file path is required (-f/--audio)\n"); return false; }
    if (!p.score_texts.empty() && (p.audio_paths.size() != 1 || p.align_mode || p.transcribe_align_mode || !p.devices.empty())) {
        fprintf(stderr, "Error: --score takes one -f file and no alignment or --devices\n");
        return false;
    }
    if (p.long_mode && (p.audio_paths.size() != 1 || p.align_mode || p.transcribe_align_mode || !p.devices.empty() || !p.score_texts.empty())) {
        fprintf(stderr, "Error: --long takes one -f file and no alignment, --score or --devices\n");
        return false;
    }
    // src/main.cpp:76-90
    if (p.align_mode && p.align_text.empty()) {
        fprintf(stderr, "Error: Reference text is required for alignment mode (--text)\n");
        return false;
    }
    if (p.align_mode && p.transcribe_align_mode) {
        fprintf(stderr, "Error: --align and --transcribe-align cannot be used together\n");
        return false;
    }
    if (p.transcribe_align_mode && p.aligner_model_path.empty()) {
        fprintf(stderr, "Error: --aligner-model is required for --transcribe-align\n");
        return false;
    }
    if ((p.align_mode || p.transcribe_align_mode) && p.audio_paths.size() != 1) {
        fprintf(stderr, "Error: alignment takes exactly one audio file\n");
        return false;
    }
    return true;
}

// src/main.cpp:163-189: "language Xxxx..." prefix of the ASR text
static std::string detect_language(const std::string &asr_text) {
    const std::string prefix = "language ";
    if (asr_text.size() < prefix.size() || asr_text.compare(0, prefix.size(), prefix) != 0) return "";
    size_t pos = prefix.size();
    if (pos >= asr_text.size() || !std::isupper((unsigned char)asr_text[pos])) return "";
    ++pos;
    while (pos < asr_text.size() && std::islower((unsigned char)asr_text[pos])) ++pos;
    std::string lang = asr_text.substr(prefix.size(), pos - prefix.size());
    std::transform(lang.begin(), lang.end(), lang.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    return lang;
}

// src/main.cpp:191-228
static std::string extract_transcript(const std::string &asr_text) {
    const std::string prefix = "language ";
    if (asr_text.size() < prefix.size() || asr_text.compare(0, prefix.size(), prefix) != 0) return asr_text;
    size_t pos = prefix.size();
    if (pos >= asr_text.size()) return "";
    if (!std::isupper((unsigned char)asr_text[pos])) return asr_text;
    ++pos;
    while (pos < asr_text.size() && std::islower((unsigned char)asr_text[pos])) ++pos;
    while (pos < asr_text.size()) {
        const unsigned char c = (unsigned char)asr_text[pos];
        if (c >= 0x80 || !std::isspace(c)) break;
        ++pos;
    }
    return asr_text.substr(pos);
}

// src/main.cpp:230-276
static std::string escape_json_string(const std::string &s) {
    std::string r;
    for (char c : s) {
        switch (c) {
            case '"': r += "\\\""; break;
            case '\\': r += "\\\\"; break;
            case '\b': r += "\\b"; break;
            case '\f': r += "\\f"; break;
            case '\n': r += "\\n"; break;
            case '\r': r += "\\r"; break;
            case '\t': r += "\\t"; break;
            default:
                if ((unsigned char)c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", (unsigned char)c); r += b; }
                else r += c;
        }
    }
    return r;
}

static std::string alignment_to_json(const qwen3_asr::alignment_result &result) {
    std::string json = "{\n  \"words\": [\n";
    for (size_t i = 0; i < result.words.size(); ++i) {
        const auto &w = result.words[i];
        char buf[64];
        snprintf(buf, sizeof buf, "\"start\": %.3f, \"end\": %.3f}", w.start, w.end);
        json += "    {\"word\": \"" + escape_json_string(w.word) + "\", " + buf;
        if (i + 1 < result.words.size()) json += ",";
        json += "\n";
    }
    json += "  ]\n}";
    return json;
}

// src/main.cpp:278-299
static std::string find_korean_dict(const std::string &model_path) {
    auto dir_of = [](const std::string &path) -> std::string {
        const size_t pos = path.find_last_of("/\\");
        return pos != std::string::npos ? path.substr(0, pos) : ".";
    };
    for (const std::string &p : {dir_of(model_path) + "/../assets/korean_dict_jieba.dict",
                                 dir_of(model_path) + "/assets/korean_dict_jieba.dict", std::string("assets/korean_dict_jieba.dict")}) {
        std::ifstream f(p);
        if (f.good()) return p;
    }
    return "";
}

static int write_output(const cli_params &p, const std::string &text) {
    if (p.output_path.empty()) {
        printf("%s", text.c_str());
        return 0;
    }
    std::ofstream out(p.output_path);
    if (!out) { fprintf(stderr, "Error: Failed to open output file: %s\n", p.output_path.c_str()); return 1; }
    out << text;
    fprintf(stderr, "Output written to: %s\n", p.output_path.c_str());
    return 0;
}

static bool load_aligner(qwen3_asr::ForcedAligner &al, const std::string &path, const std::string &lang, int device) {
    al.set_device(device);
    if (!al.load_model(path)) { fprintf(stderr, "Error (Aligner): %s\n", al.get_error().c_str()); return false; }
    if (lang == "korean") {
        const std::string dict = find_korean_dict(path);
        if (dict.empty()) fprintf(stderr, "Warning: Korean dictionary not found. Falling back to whitespace splitting.\n");
        else if (!al.load_korean_dict(dict)) fprintf(stderr, "Warning: Failed to load Korean dictionary from %s\n", dict.c_str());
    }
    return true;
}

static int run_alignment(const cli_params &p) {
    fprintf(stderr, "qwen3-asr-cli (Forced Alignment Mode)\n  Model: %s\n  Audio: %s\n  Text: %s\n", p.model_path.c_str(),
            p.audio_paths[0].c_str(), p.align_text.c_str());
    if (!p.language.empty()) fprintf(stderr, "  Language: %s\n", p.language.c_str());
    fprintf(stderr, "\n");
    qwen3_asr::ForcedAligner al;
    if (!load_aligner(al, p.model_path, p.language, p.device)) return 1;
    al.set_resample(p.resample);
    fprintf(stderr, "Model loaded. Running alignment...\n");
    auto r = al.align(p.audio_paths[0], p.align_text, p.language);
    if (!r.success) { fprintf(stderr, "Error: %s\n", r.error_msg.c_str()); return 1; }
    if (p.print_timing) {
        fprintf(stderr, "\nTiming:\n");
        fprintf(stderr, "  Mel spectrogram: %lld ms\n", (long long)r.t_mel_ms);
        fprintf(stderr, "  Audio encoding:  %lld ms\n", (long long)r.t_encode_ms);
        fprintf(stderr, "  Text decoding:   %lld ms\n", (long long)r.t_decode_ms);
        fprintf(stderr, "  Total:           %lld ms\n", (long long)r.t_total_ms);
        fprintf(stderr, "  Words aligned:   %zu\n", r.words.size());
    }
    return write_output(p, alignment_to_json(r) + "\n");
}

static int run_transcribe_and_align(const cli_params &p) {
    fprintf(stderr, "qwen3-asr-cli (Transcribe + Align Mode)\n  ASR Model: %s\n  Aligner Model: %s\n  Audio: %s\n  Threads: %d\n\n",
            p.model_path.c_str(), p.aligner_model_path.c_str(), p.audio_paths[0].c_str(), p.n_threads);
    fprintf(stderr, "--- Phase 1: Transcription ---\n");
    qwen3_asr::Qwen3ASR asr;
    asr.set_device(p.device);
    if (!asr.load_model(p.model_path)) { fprintf(stderr, "Error (ASR): %s\n", asr.get_error().c_str()); return 1; }
    qwen3_asr::transcribe_params tp;
    tp.max_tokens = p.max_tokens;
    tp.language = p.language;
    tp.n_threads = p.n_threads;
    tp.print_progress = p.print_progress;
    tp.print_timing = p.print_timing;
    tp.resample = p.resample;
    auto ar = asr.transcribe(p.audio_paths[0], tp);
    if (!ar.success) { fprintf(stderr, "Error (ASR): %s\n", ar.error_msg.c_str()); return 1; }
    const std::string detected = detect_language(ar.text);
    const std::string lang = p.language.empty() ? detected : p.language;
    const std::string transcript = extract_transcript(ar.text);
    fprintf(stderr, "  Detected language: %s\n", detected.empty() ? "(none)" : detected.c_str());
    if (!p.language.empty()) fprintf(stderr, "  Language override: %s\n", p.language.c_str());
    fprintf(stderr, "  Alignment language: %s\n", lang.empty() ? "(none)" : lang.c_str());
    fprintf(stderr, "  Transcript: %s\n", transcript.c_str());
    fprintf(stderr, "\n--- Phase 2: Forced Alignment ---\n");
    qwen3_asr::ForcedAligner al;
    if (!load_aligner(al, p.aligner_model_path, lang, p.device)) return 1;
    al.set_resample(p.resample);
    auto r = al.align(p.audio_paths[0], transcript, lang);
    if (!r.success) { fprintf(stderr, "Error (Aligner): %s\n", r.error_msg.c_str()); return 1; }
    if (p.print_timing) {
        fprintf(stderr, "\nCombined Timing:\n");
        fprintf(stderr, "  ASR:           %lld ms\n", (long long)ar.t_total_ms);
        fprintf(stderr, "  Alignment:     %lld ms\n", (long long)r.t_total_ms);
        fprintf(stderr, "  Total:         %lld ms\n", (long long)(ar.t_total_ms + r.t_total_ms));
        fprintf(stderr, "  Words aligned: %zu\n", r.words.size());
    }
    return write_output(p, alignment_to_json(r) + "\n");
}

// the sample rate a WAV file's header states (fmt chunk first, as write_wav and most encoders lay it out); 16000
// where the file cannot be read that way -- only an estimate of the clip's length hangs on it
static int wav_header_rate(const std::string &path) {
    unsigned char h[28];
    FILE *f = fopen(path.c_str(), "rb");
    const size_t k = f ? fread(h, 1, sizeof h, f) : 0;
    if (f) fclose(f);
    if (k < sizeof h || memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4) || memcmp(h + 12, "fmt ", 4)) return 16000;
    const int sr = h[24] | h[25] << 8 | h[26] << 16 | h[27] << 24;
    return sr > 0 ? sr : 16000;
}

// --devices: one host thread per GPU, each with its own model replica and
// context (the reference's objects are single-threaded; so are ours), pulling
// files from one shared queue (longest first) into its continuous-batching
// stream of --batch slots: a device that finishes early takes the next file,
// so the tail stays balanced whatever the decode lengths; output in input order
static int run_transcription_sharded(const cli_params &p) {
    const size_t N = p.audio_paths.size();
    const int G = (int)p.devices.size();
    std::vector<long long> size(N);
    for (size_t i = 0; i < N; i++) {
        struct stat st;
        size[i] = stat(p.audio_paths[i].c_str(), &st) == 0 ? (long long)st.st_size : 0;
        // --resample: the queue order, the stream's cap and its context go by the samples at 16 kHz
        if (p.resample) size[i] = size[i] * 16000 / wav_header_rate(p.audio_paths[i]);
    }
    std::vector<size_t> order(N);
    for (size_t i = 0; i < N; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return size[a] > size[b]; });
    fprintf(stderr, "qwen3-asr-cli (sharded)\n  Model: %s\n  Files: %zu over %d GPU(s), %d slots each, shared queue\n\n",
            p.model_path.c_str(), N, G, p.batch);
    // the stream's context: the longest file's prompt + the budget (16-bit PCM:
    // at most size / 2 samples), capped at kStreamSecs of audio -- every slot
    // gets that length, so one long file must not multiply the whole cache
    // (ADVICE r4).  Longer files go to a second queue that the device threads
    // take one at a time after their streams, each in a context sized to that
    // file as the reference sizes its context per clip (src/qwen3_asr.cpp:223).
    constexpr long long kStreamSecs = 120;
    std::vector<size_t> longq;
    while (!order.empty() && size[order.front()] / 2 > kStreamSecs * 16000) {
        longq.push_back(order.front());
        order.erase(order.begin());
    }
    const size_t NS = order.size();
    const long long max_samples = NS ? size[order[0]] / 2 : 0;
    const int n_ctx = qasr_prompt_len(qasr_encoder_frames(qasr_mel_frames((int)std::min<long long>(max_samples, 1LL << 30)))) +
                      p.max_tokens + 64;
    std::atomic<size_t> next_long{0};
    std::vector<qwen3_asr::transcribe_result> results(N);
    std::vector<std::string> errors(G);
    std::atomic<size_t> next{0};
    std::atomic<long long> samples{0};
    std::mutex res_mu;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int g = 0; g < G; g++) {
        th.emplace_back([&, g] {
            qwen3_asr::Qwen3ASR asr;
            asr.set_device(p.devices[g]);
            asr.set_max_batch(p.batch);
            if (!asr.load_model(p.model_path)) { errors[g] = asr.get_error(); return; }
            qwen3_asr::transcribe_params tp;
            tp.max_tokens = p.max_tokens;
            tp.language = p.language;
            tp.print_timing = false;
            tp.resample = p.resample;
            auto fetch = [&](int &id, std::vector<float> &pcm, int &sr) {
                for (;;) {
                    const size_t k = next++;
                    if (k >= NS) return false;
                    const size_t i = order[k];
                    sr = 0;
                    if (qwen3_asr::load_audio_file(p.audio_paths[i], pcm, sr) && (sr == 16000 || (p.resample && sr > 0))) {
                        samples += (long long)pcm.size() * 16000 / sr;
                        id = (int)i;
                        return true;
                    }
                    std::lock_guard<std::mutex> lk(res_mu);   // this file fails alone
                    results[i].error_msg = "Failed to load audio file: " + p.audio_paths[i];
                }
            };
            auto sink = [&](int id, qwen3_asr::transcribe_result r) {
                std::lock_guard<std::mutex> lk(res_mu);
                results[id] = std::move(r);
            };
            if (NS && !asr.transcribe_stream_rate(fetch, sink, tp, n_ctx)) { errors[g] = asr.get_error(); return; }
            for (size_t k; (k = next_long++) < longq.size();) {   // files past the stream's cap, one at a time
                const size_t i = longq[k];
                qwen3_asr::transcribe_result r = asr.transcribe(p.audio_paths[i], tp);
                std::lock_guard<std::mutex> lk(res_mu);
                if (r.success) samples += size[i] / 2;
                results[i] = std::move(r);
            }
        });
    }
    for (auto &t : th) t.join();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int g = 0; g < G; g++)
        if (!errors[g].empty()) { fprintf(stderr, "Error (device %d): %s\n", p.devices[g], errors[g].c_str()); return 1; }
    std::string all;
    for (size_t i = 0; i < N; i++) {
        if (!results[i].success) { fprintf(stderr, "Error (%s): %s\n", p.audio_paths[i].c_str(), results[i].error_msg.c_str()); return 1; }
        all += results[i].text + "\n";
    }
    if (p.print_timing)
        fprintf(stderr, "Sharded timing: %.1f s of audio in %.3f s over %d GPU(s) (RTFx %.1f, model loads included)\n",
                samples.load() / 16000.0, wall, G, samples.load() / 16000.0 / wall);
    return write_output(p, all);
}

// --long: the one recording through Qwen3ASR::transcribe_long
static int run_long(const cli_params &p, qwen3_asr::Qwen3ASR &asr, const qwen3_asr::transcribe_params &tp) {
    std::vector<float> pcm;
    int sr = 0;
    if (!qwen3_asr::load_audio_file(p.audio_paths[0], pcm, sr)) { fprintf(stderr, "Error: Failed to load audio file: %s\n", p.audio_paths[0].c_str()); return 1; }
    if (sr != 16000 && !p.resample) { fprintf(stderr, "Error: Audio must be 16kHz, got %d Hz\n", sr); return 1; }
    // seconds -> frames of 10 ms; dB -> the energy ratio 10^(dB / 10) the engine compares with
    qasr_segment_params sp{(int32_t)std::llround(p.segment_max_s * 100.0), (int32_t)std::llround(p.segment_min_s * 100.0), 5,
                           p.skip_silence_db <= 0.0 ? std::pow(10.0, p.skip_silence_db / 10.0) : -1.0};
    asr.set_max_batch(p.batch);
    const qwen3_asr::long_result r = asr.transcribe_long(pcm.data(), (int)pcm.size(), sr, tp, &sp);
    if (!r.success) { fprintf(stderr, "Error: %s\n", r.error_msg.c_str()); return 1; }
    std::string all;
    size_t n_silent = 0;
    for (const auto &s : r.segments) {
        n_silent += s.silent;
        if (!p.print_segments) continue;
        char head[64];
        snprintf(head, sizeof head, "[%.2f --> %.2f] ", s.start_s, s.end_s);
        all += head + s.result.text + "\n";
    }
    if (!p.print_segments) all = r.text + "\n";
    fprintf(stderr, "%s: %.1f s in %zu segments (%zu silent, not decoded)\n", p.audio_paths[0].c_str(), pcm.size() / (double)sr, r.segments.size(), n_silent);
    const int rc = write_output(p, all);
    if (p.profile) fprintf(stderr, "%s", asr.profile_report().c_str());
    return rc;
}

static int run_transcription(const cli_params &p) {
    fprintf(stderr, "qwen3-asr-cli\n  Model: %s\n", p.model_path.c_str());
    for (auto &a : p.audio_paths) fprintf(stderr, "  Audio: %s\n", a.c_str());
    fprintf(stderr, "  Threads: %d\n\n", p.n_threads);
    qwen3_asr::Qwen3ASR asr;
    asr.set_device(p.device);
    asr.set_profile(p.profile);
    if (!asr.load_model(p.model_path)) { fprintf(stderr, "Error: %s\n", asr.get_error().c_str()); return 1; }
    qwen3_asr::transcribe_params tp;
    tp.max_tokens = p.max_tokens;
    tp.language = p.language;
    tp.n_threads = p.n_threads;
    tp.print_progress = p.print_progress;
    tp.print_timing = p.print_timing;
    tp.token_logprobs = p.logprobs;
    tp.top_k = p.top_k;
    tp.beam_width = p.beam_width;
    tp.temperature = p.temperature;
    tp.min_p = p.min_p;
    tp.seed = p.seed;
    tp.n_best = p.n_best;
    tp.no_repeat_ngram = p.no_repeat_ngram;
    tp.repetition_penalty = p.repetition_penalty;
    tp.penalty_last_n = p.penalty_last_n;
    tp.suppress_tokens = p.suppress_tokens;
    tp.token_bias = p.token_bias;
    tp.hotwords = p.hotwords;
    tp.hotword_boost = p.hotword_boost;
    tp.hotword_boosts = p.hotword_boosts;
    tp.resample = p.resample;
    if (p.long_mode) return run_long(p, asr, tp);
    std::vector<qwen3_asr::transcribe_result> results;
    if (p.audio_paths.size() == 1) {
        results.push_back(asr.transcribe(p.audio_paths[0], tp));
    } else {
        std::vector<std::vector<float>> clips;
        std::vector<int> rates;
        for (auto &a : p.audio_paths) {
            std::vector<float> s;
            int sr = 0;
            if (!qwen3_asr::load_audio_file(a, s, sr) || (sr != 16000 && !p.resample)) { fprintf(stderr, "Error: bad audio %s\n", a.c_str()); return 1; }
            clips.push_back(std::move(s));
            rates.push_back(sr);
        }
        asr.set_max_batch(p.batch);
        results = p.resample ? asr.transcribe_batch(clips, rates, tp) : asr.transcribe_batch(clips, tp);
    }
    std::string all;
    for (size_t f = 0; f < results.size(); f++) {
        const auto &r = results[f];
        if (!r.success) { fprintf(stderr, "Error: %s\n", r.error_msg.c_str()); return 1; }
        const bool lp = p.logprobs && r.token_logprobs.size() == r.tokens.size();
        if (p.print_tokens) {
            fprintf(stderr, "\nTokens (%zu):\n", r.tokens.size());
            for (size_t k = 0; k < r.tokens.size(); ++k) {
                if (lp) fprintf(stderr, "  [%zu] %d %.4f\n", k, r.tokens[k], r.token_logprobs[k]);
                else fprintf(stderr, "  [%zu] %d\n", k, r.tokens[k]);
                if (p.top_k > 0 && r.alt_tokens.size() == r.tokens.size() * p.top_k)
                    for (int j = 0; j < p.top_k; j++) {
                        const int32_t id = r.alt_tokens[k * p.top_k + j];
                        fprintf(stderr, "        %d  %.4f  \"%s\"\n", id, r.alt_logprobs[k * p.top_k + j], asr.token_text(id).c_str());
                    }
            }
            fprintf(stderr, "\n");
        }
        if (p.beams && !r.beams.empty()) {
            fprintf(stderr, "%s: %zu hypotheses\n", p.audio_paths[f].c_str(), r.beams.size());
            for (size_t i = 0; i < r.beams.size(); ++i) {
                const auto &h = r.beams[i];
                fprintf(stderr, "  [%zu] %.4f  %zu tokens%s  \"%s\"\n", i, h.sum_logprob, h.tokens.size(), h.finished ? "" : " (unfinished)",
                        h.text.c_str());
            }
        }
        if (r.samples.size() > 1) {   // --n-best > 1: every sample, in the layout of --beams
            fprintf(stderr, "%s: %zu samples\n", p.audio_paths[f].c_str(), r.samples.size());
            for (size_t i = 0; i < r.samples.size(); ++i) {
                const auto &h = r.samples[i];
                fprintf(stderr, "  [%zu] %.4f  %zu tokens  \"%s\"\n", i, h.sum_logprob, h.tokens.size(), h.text.c_str());
            }
        }
        if (lp && !r.tokens.empty()) {
            double sum = 0.0;
            float mn = r.token_logprobs[0];
            for (float v : r.token_logprobs) { sum += v; mn = std::min(mn, v); }
            fprintf(stderr, "%s: avg_logprob %.4f min_logprob %.4f\n", p.audio_paths[f].c_str(), sum / r.tokens.size(), mn);
        }
        all += r.text + "\n";
    }
    const int rc = write_output(p, all);
    if (p.profile) fprintf(stderr, "%s", asr.profile_report().c_str());   // src/main.cpp:409-411
    return rc;
}

// --score: every text as a transcript of the one audio file, one line per text on the output
static int run_scoring(const cli_params &p) {
    qwen3_asr::Qwen3ASR asr;
    asr.set_device(p.device);
    if (!asr.load_model(p.model_path)) { fprintf(stderr, "Error: %s\n", asr.get_error().c_str()); return 1; }
    std::vector<float> pcm;
    int sr = 0;
    if (!qwen3_asr::load_audio_file(p.audio_paths[0], pcm, sr) || sr != 16000) { fprintf(stderr, "Error: bad audio %s\n", p.audio_paths[0].c_str()); return 1; }
    const std::vector<qwen3_asr::score_result> rs = asr.score(pcm.data(), (int)pcm.size(), p.score_texts);
    std::string all;
    for (size_t i = 0; i < rs.size(); i++) {
        const qwen3_asr::score_result &r = rs[i];
        if (!r.success) { fprintf(stderr, "Error: %s\n", r.error_msg.c_str()); return 1; }
        char line[160];
        snprintf(line, sizeof line, "%.4f\t%.4f\t%zu\t", r.sum_logprob, r.sum_logprob / (float)r.tokens.size(), r.tokens.size());
        all += line + p.score_texts[i] + "\n";
        if (p.print_tokens) {
            fprintf(stderr, "\nScore [%zu] \"%s\" (%zu tokens):\n", i, p.score_texts[i].c_str(), r.tokens.size());
            for (size_t k = 0; k < r.tokens.size(); ++k) {
                fprintf(stderr, "  [%zu] %d \"%s\" %.4f", k, r.tokens[k], asr.token_text(r.tokens[k]).c_str(), r.token_logprobs[k]);
                if (r.greedy_tokens[k] != r.tokens[k])
                    fprintf(stderr, "   (greedy %d \"%s\" %.4f)", r.greedy_tokens[k], asr.token_text(r.greedy_tokens[k]).c_str(), r.greedy_logprobs[k]);
                fprintf(stderr, "\n");
            }
        }
    }
    return write_output(p, all);
}

int main(int argc, char **argv) {
    cli_params p;
    if (!parse(argc, argv, p)) { fprintf(stderr, "\n"); usage(argv[0]); return 1; }
    if (!p.synthetic.empty()) {
        if (qasr_write_synthetic_gguf(p.model_path.c_str(), p.synthetic.c_str(), 42, 1) != 0) {
            fprintf(stderr, "Error: %s\n", qasr_last_error());
            return 1;
        }
        fprintf(stderr, "wrote synthetic %s model to %s\n", p.synthetic.c_str(), p.model_path.c_str());
        return 0;
    }
    if (p.transcribe_align_mode) return run_transcribe_and_align(p);
    if (p.align_mode) return run_alignment(p);
    if (!p.devices.empty()) return run_transcription_sharded(p);
    if (!p.score_texts.empty()) return run_scoring(p);
    return run_transcription(p);
}
