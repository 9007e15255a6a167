// engine_segment.hip -- long recordings: the host-only entry points over csrc/segment_host.h
// (validation, the rule on the CPU), the segment stage (recordings in HBM -> seg_energy_kernel -> seg_cut_kernel ->
// counts, cuts and peaks back, nothing else) and the entry points over it: qasr_segment (stage level),
// qasr_stage_long (the pool becomes the segments, each an (offset, length) pair into the recording as uploaded) and
// qasr_get_segments.  No existing path launches anything of this unit.
#include <climits>

#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

static SegmentParams params_of(const qasr_segment_params *p) {
    SegmentParams o;
    if (p) { o.max_frames = p->max_frames; o.min_frames = p->min_frames; o.smooth_half = p->smooth_half; o.skip_ratio = p->skip_ratio; }
    return o;
}

// ------------------------------------------------------------ host only
extern "C" int qasr_segment_validate(const qasr_segment_params *p) {
    const std::string e = segment_validate(params_of(p));
    return e.empty() ? 0 : fail(QASR_ERR_ARG, e);
}

// (a count on success, so errors are minus the code, as qasr_resample_len)
extern "C" int qasr_segment_host(const float *pcm, int n, const qasr_segment_params *p, int *cuts, double *peak, int *silent, int cap) {
    const SegmentParams prm = params_of(p);
    const std::string e = segment_validate(prm);
    if (!e.empty()) return -fail(QASR_ERR_ARG, e);
    if (n < 0 || (n > 0 && !pcm) || cap < 0) return -fail(QASR_ERR_ARG, "bad arguments");
    SegmentTable t;
    segment_rule(pcm, n, prm, t);
    const int K = (int)t.cuts.size();
    for (int k = 0; k < std::min(K, cap); k++) {
        if (cuts) cuts[k] = t.cuts[k];
        if (peak) peak[k] = t.peak[k];
        if (silent) silent[k] = t.silent[k];
    }
    return K;
}

// ------------------------------------------------------------ the stage
int qasr::eng::run_segment(qasr_ctx *c, const float *d_pcm, const std::vector<long> &off, const std::vector<int> &n,
                           const SegmentParams &p, bool want_e, bool timed, SegmentRun &out) {
    const int B = (int)n.size(), tile = segment_tile();
    std::vector<SegmentRec> recs(B);
    std::vector<int2> blocks;
    long frames = 0, slots = 0;
    out = SegmentRun();
    out.frame_off.resize(B);
    for (int b = 0; b < B; b++) {
        const int F = (int)segment_frames(n[b]), cap = (int)segment_cap(n[b], p);
        recs[b] = SegmentRec{off[b], frames, slots, F, cap};
        out.frame_off[b] = frames;
        for (int f = 0; f < F; f += tile) blocks.push_back(make_int2(b, f));
        frames += F;
        slots += cap;
    }
    out.frames = frames;
    // the cut kernel's outputs in one buffer: peak [slots] | peak_rec [B] (doubles), then cuts [slots] | n_seg [B]
    const size_t dbl = (size_t)(slots + B) * 8, all = dbl + (size_t)(slots + B) * 4;
    int rc;
    if ((rc = upload(c, c->sgrecs, recs)) || (rc = upload(c, c->sgblocks, blocks)) ||
        (rc = ensure(c, c->sg_s, std::max<long>(frames, 1) * 8)) || (want_e && (rc = ensure(c, c->sg_e, std::max<long>(frames, 1) * 8))) ||
        (rc = ensure(c, c->sg_out, all)))
        return rc;
    double *d_peak = c->sg_out.as<double>(), *d_prec = d_peak + slots;
    int *d_cuts = (int *)(d_prec + B), *d_nseg = d_cuts + slots;
    if (timed) HIPCHK(hipEventRecord(c->sg_ev[0], c->st));
    launch_segment(d_pcm, c->sgrecs.as<SegmentRec>(), B, blocks.empty() ? nullptr : c->sgblocks.as<int2>(), (int)blocks.size(),
                   p.max_frames, p.min_frames, p.smooth_half, want_e ? c->sg_e.as<double>() : nullptr, c->sg_s.as<double>(), d_cuts,
                   d_peak, d_nseg, d_prec, c->st, timed ? c->sg_ev[1] : nullptr);
    if (timed) HIPCHK(hipEventRecord(c->sg_ev[2], c->st));
    HIPCHK(hipGetLastError());
    std::vector<char> host(all);
    HIPCHK(hipMemcpyAsync(host.data(), c->sg_out.p, all, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    const double *h_peak = (const double *)host.data(), *h_prec = h_peak + slots;
    const int *h_cuts = (const int *)(h_prec + B), *h_nseg = h_cuts + slots;
    out.tab.resize(B);
    for (int b = 0; b < B; b++) {
        SegmentTable &t = out.tab[b];
        const int K = h_nseg[b];
        if (K < 1 || K > recs[b].cap) return fail(QASR_ERR_DEVICE, "segment: the cut kernel returned an impossible segment count");
        t.cuts.assign(h_cuts + recs[b].seg_off, h_cuts + recs[b].seg_off + K);
        t.peak.assign(h_peak + recs[b].seg_off, h_peak + recs[b].seg_off + K);
        t.peak_rec = h_prec[b];
        t.silent.resize(K);
        for (int k = 0; k < K; k++) t.silent[k] = segment_silent(t.peak[k], t.peak_rec, p.skip_ratio);
    }
    return 0;
}

// ------------------------------------------------------------ entry points
extern "C" int qasr_segment(qasr_ctx *c, const float *const *pcm, const int *n, int B, const qasr_segment_params *p, double *e, double *s,
                            int *cuts, double *peak, int *silent, int *n_seg, double *peak_rec, int cap) {
    if (!c || !pcm || !n || B <= 0 || !n_seg || cap < 0) return fail(QASR_ERR_ARG, "bad arguments");
    const SegmentParams prm = params_of(p);
    const std::string err = segment_validate(prm);
    if (!err.empty()) return fail(QASR_ERR_ARG, err);
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    for (hipEvent_t &ev : c->sg_ev)
        if (!ev) HIPCHK(hipEventCreate(&ev));
    c->sg_timed = false;
    // the recordings back to back in c->rsin: the staged pool (c->pcm) stays as it is
    std::vector<long> off(B);
    long tot = 0;
    for (int b = 0; b < B; b++) {
        if (n[b] < 0) return fail(QASR_ERR_ARG, "negative length");
        if (n[b] && !pcm[b]) return fail(QASR_ERR_ARG, "bad arguments");
        off[b] = tot;
        tot += n[b];
    }
    int rc;
    if ((rc = ensure(c, c->rsin, std::max<long>(tot, 1) * 4))) return rc;
    for (int b = 0; b < B; b++)
        if (n[b]) HIPCHK(hipMemcpyAsync(c->rsin.as<float>() + off[b], pcm[b], (size_t)n[b] * 4, hipMemcpyHostToDevice, c->st));
    SegmentRun r;
    if ((rc = run_segment(c, c->rsin.as<float>(), off, std::vector<int>(n, n + B), prm, e != nullptr, true, r))) return rc;
    c->sg_timed = true;
    if (e && r.frames) HIPCHK(hipMemcpy(e, c->sg_e.p, (size_t)r.frames * 8, hipMemcpyDeviceToHost));
    if (s && r.frames) HIPCHK(hipMemcpy(s, c->sg_s.p, (size_t)r.frames * 8, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; b++) {
        const SegmentTable &t = r.tab[b];
        const int K = (int)t.cuts.size();
        n_seg[b] = K;
        if (peak_rec) peak_rec[b] = t.peak_rec;
        if ((cuts || peak || silent) && K > cap)
            return fail(QASR_ERR_ARG, "segment: recording " + std::to_string(b) + " has " + std::to_string(K) + " segments, cap is " + std::to_string(cap));
        for (int k = 0; k < K; k++) {
            if (cuts) cuts[(size_t)b * cap + k] = t.cuts[k];
            if (peak) peak[(size_t)b * cap + k] = t.peak[k];
            if (silent) silent[(size_t)b * cap + k] = t.silent[k];
        }
    }
    return 0;
}

// (a count on success, so errors are minus the code)
extern "C" int qasr_segment_last_us(qasr_ctx *c, int *cut_us) {
    if (!c) return -fail(QASR_ERR_ARG, "null context");
    if (!c->sg_timed) return -fail(QASR_ERR_STATE, "no qasr_segment call has launched the kernels on this context");
    float all = 0.f, cut = 0.f;
    if (hipEventElapsedTime(&all, c->sg_ev[0], c->sg_ev[2]) != hipSuccess || hipEventElapsedTime(&cut, c->sg_ev[1], c->sg_ev[2]) != hipSuccess)
        return -fail(QASR_ERR_DEVICE, "hipEventElapsedTime failed");
    if (cut_us) *cut_us = (int)(cut * 1000.f + 0.5f);
    return (int)(all * 1000.f + 0.5f);
}

extern "C" int qasr_stage_long(qasr_ctx *c, const float *const *pcm, const int *n, const int *rate, int B, const qasr_segment_params *p) {
    if (!c || !pcm || !n || B <= 0) return -fail(QASR_ERR_ARG, "bad arguments");
    if (c->m->hp.aligner) return -fail(QASR_ERR_STATE, "qasr_stage_long: an aligner model transcribes nothing");
    const SegmentParams prm = params_of(p);
    const std::string err = segment_validate(prm);
    if (!err.empty()) return -fail(QASR_ERR_ARG, err);
    // the recordings into c->pcm at 16 kHz: as qasr_stage_audio, or through the resampler as qasr_stage_audio_rate
    int rc = rate ? qasr_stage_audio_rate(c, pcm, n, rate, B) : qasr_stage_audio(c, pcm, n, B);
    if (rc) return -rc;
    c->pin_used = 0;
    const std::vector<long> rec_off = c->staged_off;
    const std::vector<int> rec_n = c->staged_n;
    c->staged_off.clear();   // (a failure below leaves no pool behind)
    c->staged_n.clear();
    SegmentRun r;
    if ((rc = run_segment(c, c->pcm.as<float>(), rec_off, rec_n, prm, false, false, r))) return -rc;
    long total = 0;
    for (int b = 0; b < B; b++) total += (long)r.tab[b].cuts.size();
    if (total > INT_MAX) return -fail(QASR_ERR_ARG, "segment: the segment count does not fit int");
    c->seg_first.clear();
    c->seg_peak.clear();
    c->seg_silent.clear();
    for (int b = 0; b < B; b++) {
        const SegmentTable &t = r.tab[b];
        c->seg_first.push_back((int)c->staged_n.size());
        for (size_t k = 0; k < t.cuts.size(); k++) {
            const int64_t s0 = segment_start(t, k), s1 = segment_end(t, k, rec_n[b]);
            c->staged_off.push_back(rec_off[b] + (long)s0);   // into the recording where it lies: no PCM moves
            c->staged_n.push_back((int)(s1 - s0));
            c->seg_peak.push_back(t.peak[k]);
            c->seg_silent.push_back(t.silent[k]);
        }
    }
    c->seg_first.push_back((int)c->staged_n.size());
    c->seg_rec_off = rec_off;
    c->seg_valid = true;
    return (int)total;
}

extern "C" int qasr_get_segments(qasr_ctx *c, int rec, long long *start, int *n_samples, double *peak, int *silent, int cap) {
    if (!c || cap < 0) return -fail(QASR_ERR_ARG, "bad arguments");
    if (c->m->hp.aligner) return -fail(QASR_ERR_STATE, "qasr_get_segments: an aligner model has no segments");
    if (!c->seg_valid) return -fail(QASR_ERR_STATE, "qasr_get_segments: the pool is not a qasr_stage_long's");
    const int B = (int)c->seg_first.size() - 1;
    if (rec < 0 || rec >= B) return -fail(QASR_ERR_ARG, "recording index out of range");
    const int k0 = c->seg_first[rec], K = c->seg_first[rec + 1] - k0;
    for (int k = 0; k < std::min(K, cap); k++) {
        if (start) start[k] = (long long)(c->staged_off[k0 + k] - c->seg_rec_off[rec]);
        if (n_samples) n_samples[k] = c->staged_n[k0 + k];
        if (peak) peak[k] = c->seg_peak[k0 + k];
        if (silent) silent[k] = c->seg_silent[k0 + k];
    }
    return K;
}
