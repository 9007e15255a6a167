// engine_resample.hip -- audio at any common sample rate: the host-only entry points over
// csrc/resample_host.h (plan, length, taps, reference filter), the per-context tap-table cache, the resample stage
// in front of the mel (raw clips -> c->rsin -> launch_resample -> the buffer the mel kernel reads) and the entry
// points that take a rate per clip: qasr_resample, qasr_stage_audio_rate, qasr_transcribe_batch_rate.
// (qasr_run_stream_rate is engine_run.hip's, beside the stream it drives.)
#include <climits>

#include "engine_impl.h"

using namespace qasr;
using namespace qasr::eng;

// ------------------------------------------------------------ host only
extern "C" int qasr_resample_plan(int rate, int *L, int *M, int *H) {
    ResamplePlan pl;
    const std::string e = resample_plan(rate, pl);
    if (!e.empty()) return fail(QASR_ERR_ARG, e);
    if (L) *L = pl.L;
    if (M) *M = pl.M;
    if (H) *H = pl.H;
    return 0;
}

// (a count on success, so errors are minus the code, as qasr_align_json)
extern "C" int qasr_resample_len(int n_in, int rate) {
    ResamplePlan pl;
    const std::string e = resample_plan(rate, pl);
    if (!e.empty()) return -fail(QASR_ERR_ARG, e);
    if (n_in < 0) return -fail(QASR_ERR_ARG, "negative length");
    const int64_t n = resample_len64(n_in, pl);
    if (n > INT_MAX) return -fail(QASR_ERR_ARG, "resample: the output of " + std::to_string(n_in) + " samples at " + std::to_string(rate) + " Hz does not fit int");
    return (int)n;
}

extern "C" int qasr_resample_taps(int rate, float *out, int cap) {
    ResamplePlan pl;
    const std::string e = resample_plan(rate, pl);
    if (!e.empty()) return -fail(QASR_ERR_ARG, e);
    const int need = pl.L * pl.taps();
    if (cap < 0 || (cap > 0 && !out)) return -fail(QASR_ERR_ARG, "bad arguments");
    if (cap == 0) return need;   // (the size a caller allocates)
    if (cap < need) return -fail(QASR_ERR_ARG, "buffer shorter than the tap table");
    std::vector<float> h;
    resample_taps(rate, pl, h);
    memcpy(out, h.data(), h.size() * 4);
    return need;
}

extern "C" int qasr_resample_host(const float *pcm, int n, int rate, float *out) {
    const int n_out = qasr_resample_len(n, rate);
    if (n_out < 0) return n_out;
    if ((n > 0 && !pcm) || (n_out > 0 && !out)) return -fail(QASR_ERR_ARG, "bad arguments");
    ResamplePlan pl;
    (void)resample_plan(rate, pl);
    std::vector<float> h;
    resample_taps(rate, pl, h);
    resample_filter(pcm, n, pl, h.data(), out);
    return n_out;
}

// ------------------------------------------------------------ the stage
// the plan and the device table of a rate, built once per context
int qasr::eng::resample_table(qasr_ctx *c, int rate, ResampleTab &out) {
    auto it = c->rs_tabs.find(rate);
    if (it != c->rs_tabs.end()) { out = it->second; return 0; }
    ResampleTab t;
    const std::string e = resample_plan(rate, t.pl);
    if (!e.empty()) return fail(QASR_ERR_ARG, e);
    if (!resample_fits(t.pl.L, t.pl.M, t.pl.H)) return fail(QASR_ERR_STATE, "resample: the kernel's window does not hold rate " + std::to_string(rate));
    if (!t.pl.copy()) {
        std::vector<float> h, dev;
        resample_taps(rate, t.pl, h);
        resample_taps_device(t.pl, h, dev);
        int rc;
        if ((rc = dev_alloc(c, (void **)&t.d_taps, dev.size() * 4))) return rc;
        HIPCHK(hipMemcpy(t.d_taps, dev.data(), dev.size() * 4, hipMemcpyHostToDevice));
    }
    c->rs_tabs[rate] = t;
    out = t;
    return 0;
}

// where B raw clips (n[b] samples at rate[b]; rate null: 16000) lie back to back, before and after the resampler
int qasr::eng::resample_layout(const int *n, const int *rate, int B, ResampleLayout &o) {
    o = ResampleLayout();
    o.in_off.resize(B); o.out_off.resize(B); o.n_in.assign(n, n + B); o.n_out.resize(B); o.rate.resize(B);
    for (int b = 0; b < B; b++) {
        o.rate[b] = rate ? rate[b] : kResampleOutRate;
        if (n[b] < 0) return fail(QASR_ERR_ARG, "negative length");
        const int no = qasr_resample_len(n[b], o.rate[b]);
        if (no < 0) return -no;
        o.in_off[b] = o.in_tot; o.out_off[b] = o.out_tot; o.n_out[b] = no;
        o.in_tot += n[b]; o.out_tot += no;
    }
    return 0;
}

// clips of a layout already at d_in -> d_out (both hold the layout's totals), one launch on the context stream
// (timed: between the events c->rs_ev)
int qasr::eng::run_resample(qasr_ctx *c, const ResampleLayout &o, const float *d_in, float *d_out, bool timed) {
    const int B = (int)o.n_in.size();
    std::vector<ResampleClip> clips(B);
    std::vector<int2> blocks;
    const int tile = resample_tile();
    int rc;
    for (int b = 0; b < B; b++) {
        ResampleTab t;
        if ((rc = resample_table(c, o.rate[b], t))) return rc;
        clips[b] = ResampleClip{o.in_off[b], o.out_off[b], o.n_in[b], o.n_out[b], t.pl.L, t.pl.M, t.pl.H, t.d_taps};
        for (long f = 0; f < o.n_out[b]; f += tile) blocks.push_back(make_int2(b, (int)f));
    }
    if (blocks.empty()) return 0;
    if ((rc = upload(c, c->rsclips, clips)) || (rc = upload(c, c->rsblocks, blocks))) return rc;
    if (timed) HIPCHK(hipEventRecord(c->rs_ev[0], c->st));
    launch_resample(d_in, c->rsclips.as<ResampleClip>(), c->rsblocks.as<int2>(), (int)blocks.size(), d_out, c->st);
    if (timed) HIPCHK(hipEventRecord(c->rs_ev[1], c->st));
    HIPCHK(hipGetLastError());
    return 0;
}

// B host clips -> c->rsin (copies on the context stream) -> resampled into dst, grown to hold them
static int resample_host_clips(qasr_ctx *c, const float *const *pcm, const ResampleLayout &o, DevBuf &dst, bool timed = false) {
    const int B = (int)o.n_in.size();
    int rc;
    if ((rc = ensure(c, c->rsin, std::max<long>(o.in_tot, 1) * 4)) || (rc = ensure(c, dst, std::max<long>(o.out_tot, 1) * 4))) return rc;
    for (int b = 0; b < B; b++) {
        if (o.n_in[b] && !pcm[b]) return fail(QASR_ERR_ARG, "bad arguments");
        if (o.n_in[b]) HIPCHK(hipMemcpyAsync(c->rsin.as<float>() + o.in_off[b], pcm[b], (size_t)o.n_in[b] * 4, hipMemcpyHostToDevice, c->st));
    }
    return run_resample(c, o, c->rsin.as<float>(), dst.as<float>(), timed);
}

// ------------------------------------------------------------ entry points
extern "C" int qasr_resample(qasr_ctx *c, const float *const *pcm, const int *n, const int *rate, int B, float *out) {
    if (!c || !pcm || !n || B <= 0 || !out) return fail(QASR_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    ResampleLayout o;
    int rc;
    for (hipEvent_t &e : c->rs_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    c->rs_timed = false;
    if ((rc = resample_layout(n, rate, B, o)) || (rc = resample_host_clips(c, pcm, o, c->pcm, true))) return rc;
    c->rs_timed = o.out_tot > 0;
    if (o.out_tot) HIPCHK(hipMemcpyAsync(out, c->pcm.p, (size_t)o.out_tot * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

// (a count on success, so errors are minus the code)
extern "C" int qasr_resample_last_us(qasr_ctx *c) {
    if (!c) return -fail(QASR_ERR_ARG, "null context");
    if (!c->rs_timed) return -fail(QASR_ERR_STATE, "no qasr_resample call has launched the kernel on this context");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->rs_ev[0], c->rs_ev[1]) != hipSuccess) return -fail(QASR_ERR_DEVICE, "hipEventElapsedTime failed");
    return (int)(ms * 1000.f + 0.5f);
}

extern "C" int qasr_stage_audio_rate(qasr_ctx *c, const float *const *pcm, const int *n, const int *rate, int B) {
    if (!rate) return qasr_stage_audio(c, pcm, n, B);
    if (!c || !pcm || !n || B <= 0) return fail(QASR_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->st));
    c->pin_used = 0;
    ResampleLayout o;
    int rc;
    if ((rc = resample_layout(n, rate, B, o)) || (rc = resample_host_clips(c, pcm, o, c->pcm))) return rc;
    HIPCHK(hipStreamSynchronize(c->st));
    c->seg_valid = false;
    c->staged_n = o.n_out;   // the pool holds 16 kHz clips from here on
    c->staged_off = o.out_off;
    return 0;
}

extern "C" int qasr_transcribe_batch_rate(qasr_ctx *c, const float *const *pcm, const int *n, const int *rate, int B, int max_tokens,
                                          int ignore_eos, int32_t *tokens, int *n_tokens, qasr_timings *t) {
    int rc = qasr_stage_audio_rate(c, pcm, n, rate, B);
    if (rc) return rc;
    return qasr_run(c, max_tokens, ignore_eos, tokens, n_tokens, t);
}
