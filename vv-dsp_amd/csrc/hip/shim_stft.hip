// shim_stft.hip -- STFT handles (device window, per-device copies, host-path
// staging) over the STFT units (stft_kernels.hip routes to them; istft_kernels.hip)
// and mixed_fft.hip, and the framing entry points
// (framing_kernels.hip).
#include "shim_common.hpp"

using namespace vvh;

namespace vvh {

const float* stft_window_here(vvhip_stft* h) {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return nullptr;
    if (d == h->dev) return h->d_win;
    std::lock_guard<std::mutex> lk(h->win_mu);
    for (auto& w : h->other_wins)
        if (w.first == d) return w.second;
    float* p = nullptr;
    if (hipMalloc(&p, sizeof(float) * (h->nfft + 2)) != hipSuccess) return nullptr;
    if (hipMemcpy(p, h->h_win.data(), sizeof(float) * h->nfft, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p);
        return nullptr;
    }
    h->other_wins.push_back({d, p});
    return p;
}

int stft_frames_run(vvhip_stft* h, const float* sig, size_t n, size_t nch, size_t ch_stride, void* out,
                    size_t out_ch_stride, int out_kind, hipStream_t s, size_t frame0, size_t nframes) {
    size_t frames = vvhip_stft_num_frames(n, h->nfft, h->hop);
    const float* win = stft_window_here(h);
    if (!win) return fail(ST_INTERNAL, "stft window on the current device");
    if (out_kind < 0 || out_kind > 2) return fail(ST_RANGE, "stft output kind");
    if (frame0 != 0 || nframes != SIZE_MAX) {
        if (frame0 > frames || (nframes != SIZE_MAX && nframes > frames - frame0))
            return fail(ST_RANGE, "stft frame range past the last frame");
        if (nframes == SIZE_MAX) nframes = frames - frame0;
        if (nframes == 0) return ST_OK;
        const size_t off = frame0 * h->hop;   // < n for every existing frame but a wholly padded last one
        sig += off < n ? off : n;
        n -= off < n ? off : n;
        frames = nframes;
    }
    const long long NF = (long long)h->nfft;
    if (stft_fused_supported(NF)) {
        HIPCHK(launch_stft(NF, (long long)h->hop, out_kind, sig, (long long)n, (long long)nch, (long long)ch_stride,
                           (long long)frames, win, out, (long long)out_ch_stride, s),
               ST_INTERNAL);
        return ST_OK;
    }
    if (knob(KNOB_NO_MIXED, 0) != 1 && stft_mixed_supported(NF)) {   // 7-smooth nfft <= 4096: one kernel
        HIPCHK(launch_stft_mixed(NF, (long long)h->hop, out_kind, sig, (long long)n, (long long)nch,
                                 (long long)ch_stride, (long long)frames, win, out, (long long)out_ch_stride, s),
               ST_INTERNAL);
        return ST_OK;
    }
    const int complex_out = out_kind == 1;
    // generic nfft: gather windowed complex frames, batched C2C, magnitude
    for (size_t c = 0; c < nch; ++c) {
        Scratch fr(s);
        const size_t cnt = frames * h->nfft;
        HIPCHK(fr.alloc(8 * cnt), ST_INTERNAL);
        HIPCHK(launch_frame_gather(NF, (long long)h->hop, sig + c * ch_stride, (long long)n, 1, 0,
                                   (long long)frames, win, (float2*)fr.p, s),
               ST_INTERNAL);
        if (complex_out) {
            int st = fft_run(h->nfft, 0, 1, fr.p, (float2*)out + c * out_ch_stride, frames, s);
            if (st) return st;
        } else {
            int st = fft_run(h->nfft, 0, 1, fr.p, fr.p, frames, s);
            if (st) return st;
            if (out_kind == 2)
                HIPCHK(launch_power_half((const float2*)fr.p, (float*)out + c * out_ch_stride, NF, (long long)frames,
                                         s),
                       ST_INTERNAL);
            else
                HIPCHK(launch_magnitude((const float2*)fr.p, (float*)out + c * out_ch_stride, (long long)cnt, s),
                       ST_INTERNAL);
        }
    }
    return ST_OK;
}

}  // namespace vvh

extern "C" {

size_t vvhip_stft_num_frames(size_t n, size_t nfft, size_t hop) {
    if (hop == 0) return 0;
    return (n < nfft) ? 1 : 1 + (n - nfft + hop) / hop;
}

int vvhip_stft_create(size_t nfft, size_t hop, const float* window, vvhip_stft** out) {
    if (!out || !window) return ST_NULL;
    *out = nullptr;
    if (nfft == 0 || hop == 0 || hop > nfft) return ST_SIZE;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    vvhip_stft* h = new (std::nothrow) vvhip_stft;
    if (!h) return ST_INTERNAL;
    h->nfft = nfft;
    h->hop = hop;
    h->h_win.assign(window, window + nfft);
    if (hipGetDevice(&h->dev) != hipSuccess) h->dev = 0;
    if (hipMalloc(&h->d_win, sizeof(float) * (nfft + 2)) != hipSuccess ||
        hipMemcpy(h->d_win, window, sizeof(float) * nfft, hipMemcpyHostToDevice) != hipSuccess) {
        vvhip_stft_destroy(h);
        return fail(ST_INTERNAL, "stft window upload");
    }
    *out = h;
    return ST_OK;
}

void vvhip_stft_destroy(vvhip_stft* h) {
    if (!h) return;
    h->host.release();
    if (h->d_win) (void)hipFree(h->d_win);
    for (auto& w : h->other_wins) (void)hipFree(w.second);
    h->b0.release();
    h->b1.release();
    h->b2.release();
    delete h;
}

int vvhip_stft_spectrogram_device(vvhip_stft* h, const float* d_signal, size_t n, size_t nch,
                                  size_t ch_stride, void* d_out, size_t out_ch_stride, int complex_out,
                                  void* stream) {
    if (!h || !d_signal || !d_out) return ST_NULL;
    if (nch == 0) return ST_OK;
    return stft_frames_run(h, d_signal, n, nch, ch_stride, d_out, out_ch_stride, complex_out,
                           (hipStream_t)stream);
}

// power rows [ch][frame][nfft/2+1] with rows row_pitch floats apart: in the
// kernel for power-of-two nfft; other lengths write packed rows to scratch and
// place them with one strided copy (the same values)
int vvhip_stft_power_pitched_device(vvhip_stft* h, const float* d_signal, size_t n, size_t nch, size_t ch_stride,
                                    float* d_out, size_t out_ch_stride, size_t row_pitch, void* stream) {
    if (!h || !d_signal || !d_out) return ST_NULL;
    const size_t nb = h->nfft / 2 + 1, frames = vvhip_stft_num_frames(n, h->nfft, h->hop);
    if (row_pitch < nb) return fail(ST_SIZE, "power row pitch below nfft/2+1");
    if (nch > 1 && out_ch_stride < frames * row_pitch) return fail(ST_SIZE, "channel stride below frames x row pitch");
    if (nch == 0) return ST_OK;
    const hipStream_t s = (hipStream_t)stream;
    if (row_pitch == nb)
        return stft_frames_run(h, d_signal, n, nch, ch_stride, d_out, out_ch_stride, 2, s);
    const float* win = stft_window_here(h);
    if (!win) return fail(ST_INTERNAL, "stft window on the current device");
    if (stft_fused_supported((long long)h->nfft)) {
        HIPCHK(launch_stft((long long)h->nfft, (long long)h->hop, 2, d_signal, (long long)n, (long long)nch,
                           (long long)ch_stride, (long long)frames, win, d_out, (long long)out_ch_stride, s,
                           (long long)row_pitch),
               ST_INTERNAL);
        return ST_OK;
    }
    Scratch pw(s);
    HIPCHK(pw.alloc(sizeof(float) * nch * frames * nb), ST_INTERNAL);
    if (int st = stft_frames_run(h, d_signal, n, nch, ch_stride, pw.p, frames * nb, 2, s)) return st;
    for (size_t c = 0; c < nch; ++c)
        HIPCHK(hipMemcpy2DAsync(d_out + c * out_ch_stride, sizeof(float) * row_pitch, (const float*)pw.p + c * frames * nb,
                                sizeof(float) * nb, sizeof(float) * nb, frames, hipMemcpyDeviceToDevice, s),
               ST_INTERNAL);
    return ST_OK;
}

int vvhip_stft_spectrogram_range_device(vvhip_stft* h, const float* d_signal, size_t n, size_t nch,
                                        size_t ch_stride, size_t frame0, size_t nframes, void* d_out,
                                        size_t out_ch_stride, int out_kind, void* stream) {
    if (!h || !d_signal || !d_out) return ST_NULL;
    if (nch == 0) return ST_OK;
    if (nframes == SIZE_MAX) return fail(ST_RANGE, "stft frame count");
    return stft_frames_run(h, d_signal, n, nch, ch_stride, d_out, out_ch_stride, out_kind, (hipStream_t)stream,
                           frame0, nframes);
}

int vvhip_stft_spectrogram_host(vvhip_stft* h, const float* signal, size_t n, float* out_mag) {
    if (!h || !signal || !out_mag) return ST_NULL;
    std::lock_guard<std::mutex> host_lock(h->host.mu);
    DevGuard on_dev(h->dev);   // the handle's stream, buffers and window live on its creation device
    HIPCHK(h->host.stream_or_create(), ST_INTERNAL);
    const hipStream_t s = h->host.stream;
    const size_t frames = vvhip_stft_num_frames(n, h->nfft, h->hop);
    const size_t ob = sizeof(float) * frames * h->nfft;
    const size_t row = sizeof(float) * h->nfft;
    size_t per = (host_chunk_bytes() / row) & ~(size_t)1;   // even: frames pair up as in one launch
    if (per < 2) per = 2;
    if (n >= h->nfft && frames >= 2 * per && stft_fused_supported((long long)h->nfft)) {
        // pipelined over frame chunks; chunk c reads its own span (with the nfft-hop overlap)
        const long long nchunks = (long long)((frames + per - 1) / per);
        return run_lanes(h->host.lanes, nchunks, [&](long long c, HostLane& L) -> int {
            const size_t f0 = (size_t)c * per, fc = (frames - f0) < per ? (frames - f0) : per;
            const size_t start = f0 * h->hop;
            const size_t want = (fc - 1) * h->hop + h->nfft;
            const size_t len = (n - start) < want ? (n - start) : want;
            HIPCHK(L.a.ensure(sizeof(float) * ((per - 1) * h->hop + h->nfft)), ST_INTERNAL);
            HIPCHK(L.b.ensure(row * per), ST_INTERNAL);
            HIPCHK(hipMemcpyAsync(L.a.p, signal + start, sizeof(float) * len, hipMemcpyHostToDevice, L.s),
                   ST_INTERNAL);
            HIPCHK(launch_stft((long long)h->nfft, (long long)h->hop, 0, (const float*)L.a.p, (long long)len, 1, 0,
                               (long long)fc, h->d_win, L.b.p, (long long)(fc * h->nfft), L.s),
                   ST_INTERNAL);
            HIPCHK(hipMemcpyAsync(out_mag + f0 * h->nfft, L.b.p, row * fc, hipMemcpyDeviceToHost, L.s),
                   ST_INTERNAL);
            return ST_OK;
        });
    }
    HIPCHK(h->b0.ensure(sizeof(float) * (n ? n : 1)), ST_INTERNAL);
    HIPCHK(h->b1.ensure(ob), ST_INTERNAL);
    if (n) HIPCHK(hipMemcpyAsync(h->b0.p, signal, sizeof(float) * n, hipMemcpyHostToDevice, s), ST_INTERNAL);
    int st = stft_frames_run(h, (const float*)h->b0.p, n, 1, 0, h->b1.p, frames * h->nfft, 0, s);
    if (st) return st;
    HIPCHK(hipMemcpyAsync(out_mag, h->b1.p, ob, hipMemcpyDeviceToHost, s), ST_INTERNAL);
    HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
    return ST_OK;
}

int vvhip_stft_process_device(vvhip_stft* h, const float* d_frames, size_t count, float* d_spec,
                              void* stream) {
    if (!h || !d_frames || !d_spec) return ST_NULL;
    // explicit frames laid back to back: hop = nfft over a count*nfft signal
    const size_t n = count * h->nfft;
    const long long NF = (long long)h->nfft;
    hipStream_t s = (hipStream_t)stream;
    const float* win = stft_window_here(h);
    if (!win) return fail(ST_INTERNAL, "stft window on the current device");
    if (stft_fused_supported(NF)) {
        HIPCHK(launch_stft(NF, NF, 1, d_frames, (long long)n, 1, 0, (long long)count, win, d_spec, 0, s),
               ST_INTERNAL);
        return ST_OK;
    }
    Scratch fr(s);
    HIPCHK(fr.alloc(8 * n), ST_INTERNAL);
    HIPCHK(launch_frame_gather(NF, NF, d_frames, (long long)n, 1, 0, (long long)count, win,
                               (float2*)fr.p, s),
           ST_INTERNAL);
    return fft_run(h->nfft, 0, 1, fr.p, d_spec, count, s);
}

int vvhip_stft_process_host(vvhip_stft* h, const float* frame, float* spec_out) {
    if (!h || !frame || !spec_out) return ST_NULL;
    std::lock_guard<std::mutex> host_lock(h->host.mu);
    DevGuard on_dev(h->dev);   // the handle's stream, buffers and window live on its creation device
    HIPCHK(h->host.stream_or_create(), ST_INTERNAL);
    const hipStream_t s = h->host.stream;
    HIPCHK(h->b0.ensure(sizeof(float) * h->nfft), ST_INTERNAL);
    HIPCHK(h->b1.ensure(8 * h->nfft), ST_INTERNAL);
    HIPCHK(hipMemcpyAsync(h->b0.p, frame, sizeof(float) * h->nfft, hipMemcpyHostToDevice, s), ST_INTERNAL);
    int st = vvhip_stft_process_device(h, (const float*)h->b0.p, 1, (float*)h->b1.p, s);
    if (st) return st;
    HIPCHK(hipMemcpyAsync(spec_out, h->b1.p, 8 * h->nfft, hipMemcpyDeviceToHost, s), ST_INTERNAL);
    HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
    return ST_OK;
}

int vvhip_stft_reconstruct_device(vvhip_stft* h, const float* d_spec, size_t count, size_t hop,
                                  float* d_out_add, float* d_norm_add, void* stream) {
    if (!h || !d_spec || !d_out_add) return ST_NULL;
    if (hop == 0) return ST_SIZE;
    hipStream_t s = (hipStream_t)stream;
    const float* win = stft_window_here(h);
    if (!win) return fail(ST_INTERNAL, "stft window on the current device");
    // knob ISTFT_OLD = 1 (A/B, scripts/kbench.py): IFFT to scratch + k_ola
    if (istft_fused_supported((long long)h->nfft, (long long)hop) && knob(KNOB_ISTFT_OLD, 0) != 1) {
        HIPCHK(launch_istft_fused((long long)h->nfft, (long long)hop, (const float2*)d_spec, (long long)count,
                                  win, d_out_add, d_norm_add, s),
               ST_INTERNAL);
        return ST_OK;
    }
    Scratch tf(s);
    HIPCHK(tf.alloc(8 * h->nfft * count), ST_INTERNAL);
    int st = fft_run(h->nfft, 0, -1, d_spec, tf.p, count, s);
    if (st) return st;
    HIPCHK(launch_ola((long long)h->nfft, (long long)hop, (const float2*)tf.p, (long long)count, win,
                      d_out_add, d_norm_add, s),
           ST_INTERNAL);
    return ST_OK;
}

int vvhip_stft_reconstruct_host(vvhip_stft* h, const float* spec, float* out_add, float* norm_add) {
    if (!h || !spec || !out_add) return ST_NULL;
    std::lock_guard<std::mutex> host_lock(h->host.mu);
    DevGuard on_dev(h->dev);   // the handle's stream, buffers and window live on its creation device
    HIPCHK(h->host.stream_or_create(), ST_INTERNAL);
    const hipStream_t s = h->host.stream;
    const size_t nb = sizeof(float) * h->nfft;
    HIPCHK(h->b0.ensure(2 * nb), ST_INTERNAL);
    HIPCHK(h->b1.ensure(nb), ST_INTERNAL);
    HIPCHK(h->b2.ensure(nb), ST_INTERNAL);
    HIPCHK(hipMemcpyAsync(h->b0.p, spec, 2 * nb, hipMemcpyHostToDevice, s), ST_INTERNAL);
    HIPCHK(hipMemcpyAsync(h->b1.p, out_add, nb, hipMemcpyHostToDevice, s), ST_INTERNAL);
    if (norm_add) HIPCHK(hipMemcpyAsync(h->b2.p, norm_add, nb, hipMemcpyHostToDevice, s), ST_INTERNAL);
    int st = vvhip_stft_reconstruct_device(h, (const float*)h->b0.p, 1, h->nfft, (float*)h->b1.p,
                                           norm_add ? (float*)h->b2.p : nullptr, s);
    if (st) return st;
    HIPCHK(hipMemcpyAsync(out_add, h->b1.p, nb, hipMemcpyDeviceToHost, s), ST_INTERNAL);
    if (norm_add) HIPCHK(hipMemcpyAsync(norm_add, h->b2.p, nb, hipMemcpyDeviceToHost, s), ST_INTERNAL);
    HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
    return ST_OK;
}

// ---------------------------------------------------------------------------
// Framing (framing.c:58-146)
// ---------------------------------------------------------------------------
int vvhip_fetch_frames_device(const float* d_signal, size_t n, float* d_frames, size_t frame_len, size_t hop,
                              size_t frame0, size_t count, int center, const float* d_window, void* stream) {
    if (!d_signal || !d_frames) return ST_NULL;
    if (n == 0 || frame_len == 0 || hop == 0) return ST_SIZE;
    HIPCHK(launch_fetch_frames(d_signal, 0, (long long)n, d_frames, (long long)frame_len, (long long)hop,
                               (long long)frame0, (long long)count, center, d_window, (hipStream_t)stream),
           ST_INTERNAL);
    return ST_OK;
}

int vvhip_overlap_add_device(const float* d_frames, size_t count, float* d_out, size_t out_len, size_t frame_len,
                             size_t hop, size_t frame0, void* stream) {
    if (!d_frames || !d_out) return ST_NULL;
    if (out_len == 0 || frame_len == 0 || hop == 0) return ST_SIZE;
    HIPCHK(launch_overlap_add(d_frames, (long long)count, d_out, (long long)out_len, (long long)frame_len,
                              (long long)hop, (long long)frame0, (hipStream_t)stream),
           ST_INTERNAL);
    return ST_OK;
}

// One frame through the device: only the span of samples the frame reads
// goes up (for a centred frame near an end, the reflected indices' span).
int vvhip_fetch_frame_host(const float* signal, size_t n, float* frame, size_t frame_len, size_t hop,
                           size_t frame_index, int center, const float* window) {
    if (!signal || !frame) return ST_NULL;
    if (n == 0 || frame_len == 0 || hop == 0) return ST_SIZE;
    HostCall c("fetch_frame");
    if (!c.ok()) return c.st;
    const long long N = (long long)n, L = (long long)frame_len;
    const long long start = (long long)(frame_index * hop) - (center ? L / 2 : 0);
    long long lo = N, hi = 0;   // sample span [lo, hi) the frame reads
    if (center) {
        for (long long i = 0; i < L; ++i) {
            const long long k = reflect_sample(start + i, N);
            lo = k < lo ? k : lo;
            hi = k + 1 > hi ? k + 1 : hi;
        }
    } else {
        lo = start < 0 ? 0 : (start < N ? start : N);
        hi = start + L < N ? (start + L > lo ? start + L : lo) : N;
    }
    const long long span = hi > lo ? hi - lo : 0;
    const float* dsig = (const float*)c.in(signal + lo, sizeof(float) * span);
    const float* dwin = (const float*)c.in(window, sizeof(float) * L);
    float* dfr = (float*)c.out(frame, sizeof(float) * L);
    if (!c.ok()) return c.st;
    const hipError_t e = launch_fetch_frames(dsig, lo, N, dfr, L, (long long)hop, (long long)frame_index, 1, center,
                                             dwin, c.s);
    return c.finish(e == hipSuccess ? ST_OK : fail(ST_INTERNAL, "fetch_frame run", e));
}

// One frame added into out[s0, s0 + frame_len) (clipped to out_len) on the device.
int vvhip_overlap_add_host(const float* frame, float* out, size_t out_len, size_t frame_len, size_t hop,
                           size_t frame_index) {
    if (!frame || !out) return ST_NULL;
    if (out_len == 0 || frame_len == 0 || hop == 0) return ST_SIZE;
    HostCall c("overlap_add");
    const size_t s0 = frame_index * hop;
    if (!c.ok() || s0 >= out_len) return c.st;   // nothing lands inside the output (framing.c:137-144)
    const size_t span = out_len - s0 < frame_len ? out_len - s0 : frame_len;
    const float* dfr = (const float*)c.in(frame, sizeof(float) * frame_len);
    float* dout = (float*)c.inout(out + s0, sizeof(float) * span);
    if (!c.ok()) return c.st;
    const hipError_t e = launch_overlap_add(dfr, 1, dout, (long long)span, (long long)frame_len, (long long)hop, 0, c.s);
    return c.finish(e == hipSuccess ? ST_OK : fail(ST_INTERNAL, "overlap_add run", e));
}

}  // extern "C"
