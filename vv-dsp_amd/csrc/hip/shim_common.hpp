// shim_common.hpp -- what the translation units of the extern "C" HIP shim
// (shim_*.hip, include/vv_dsp_hip.h) share: status codes, the per-thread error
// text, device buffers and the host-buffer staging helpers.  Not part of the
// public C ABI; the library is built with hidden visibility.
#pragma once
#include "../../../include/vv_dsp_hip.h"
#include "vvhip_internal.hpp"

#include <cstdint>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace vvh {

enum { ST_OK = 0, ST_NULL = 1, ST_SIZE = 2, ST_RANGE = 3, ST_INTERNAL = 4, ST_NAN = 5, ST_UNSUP = 6 };

// The text behind vvhip_last_error(): one object per thread for the whole
// library, whichever translation unit raised the failure.
inline thread_local std::string g_err;

inline int fail(int code, const char* what, hipError_t e = hipSuccess) {
    g_err = what;
    if (e != hipSuccess) {
        g_err += ": ";
        g_err += hipGetErrorString(e);
    }
    return code;
}

#define HIPCHK(expr, code)                                           \
    do {                                                             \
        hipError_t e__ = (expr);                                     \
        if (e__ != hipSuccess) return fail((code), #expr, e__);      \
    } while (0)

inline int device_count() {
    static int cnt = -1;
    static std::once_flag once;
    std::call_once(once, [] {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
        cnt = c;
    });
    return cnt;
}

inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }

// Growable device buffer.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Makes device `d` current for a scope and restores the caller's device after
// (host-buffer calls of a handle run on the handle's creation device: its
// stream, staging buffers and window live there).
struct DevGuard {
    int prev = -1;
    explicit DevGuard(int d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev >= 0 && prev != d && hipSetDevice(d) != hipSuccess) prev = -1;
        if (prev == d) prev = -1;
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DevGuard(const DevGuard&) = delete;
    DevGuard& operator=(const DevGuard&) = delete;
};

// Stream-ordered scratch for multi-kernel paths on device pointers.
struct Scratch {
    void* p = nullptr;
    hipStream_t s;
    explicit Scratch(hipStream_t st) : s(st) {}
    hipError_t alloc(size_t bytes) { return hipMallocAsync(&p, bytes ? bytes : 16, s); }
    ~Scratch() {
        if (p) (void)hipFreeAsync(p, s);
    }
};

// Host-buffer pipeline (the reference API's host pointers).  A large call is
// cut into chunks that alternate between two lanes; each lane is a host thread
// with its own stream and device buffers and runs host->device copy, kernels
// and device->host copy for its chunks.  PCIe is full duplex, so one lane's
// device->host copy overlaps the other lane's host->device copy; a pageable
// hipMemcpy blocks its calling thread, hence two threads rather than two
// streams issued from one.
struct HostLane {
    hipStream_t s = nullptr;
    DevBuf a, b;
    hipError_t init() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    void release() {
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
        s = nullptr;
        a.release();
        b.release();
    }
};

inline size_t host_chunk_bytes() {
    const long long mb = knob(KNOB_HOST_CHUNK_MB, 16);
    return (size_t)(mb > 0 ? mb : 16) << 20;
}

// fn(chunk, lane) enqueues one chunk on lane.s and returns a status; the lane
// synchronises its stream after every chunk, so the caller's host buffers are
// complete when this returns.
template <class F>
int run_lanes(HostLane* lanes, long long nchunks, F&& fn) {
    for (int l = 0; l < 2; ++l) HIPCHK(lanes[l].init(), ST_INTERNAL);
    int dev = 0;
    HIPCHK(hipGetDevice(&dev), ST_INTERNAL);
    int st1 = ST_OK;
    std::string err1;
    std::thread worker([&] {
        if (hipSetDevice(dev) != hipSuccess) {
            st1 = ST_INTERNAL;
            err1 = "host pipeline: hipSetDevice";
            return;
        }
        for (long long c = 1; c < nchunks && st1 == ST_OK; c += 2) {
            st1 = fn(c, lanes[1]);
            if (st1 == ST_OK && hipStreamSynchronize(lanes[1].s) != hipSuccess) st1 = ST_INTERNAL;
        }
        if (st1 != ST_OK) err1 = g_err.empty() ? "host pipeline lane 1" : g_err;
    });
    int st0 = ST_OK;
    for (long long c = 0; c < nchunks && st0 == ST_OK; c += 2) {
        st0 = fn(c, lanes[0]);
        if (st0 == ST_OK) HIPCHK(hipStreamSynchronize(lanes[0].s), ST_INTERNAL);
    }
    worker.join();
    if (st0 != ST_OK) return st0;
    if (st1 != ST_OK) return fail(st1, err1.c_str());
    return ST_OK;
}

// The host-buffer state of a plan handle (FFT, STFT, FIR, mel): its stream,
// created on the first host-buffer call, the two pipeline lanes of the handles
// that cut large calls into chunks, and the mutex under which host-buffer
// calls on one handle take turns (they share the stream and the handle's
// staging buffers; the reference's execute takes a const plan and Kiss is
// reentrant, fft.h:227).
struct HostStage {
    hipStream_t stream = nullptr;
    HostLane lanes[2];
    std::mutex mu;
    hipError_t stream_or_create() {
        return stream ? hipSuccess : hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    }
    void release() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        stream = nullptr;
        lanes[0].release();
        lanes[1].release();
    }
};

// One host-buffer call without a handle through the device: a stream of its
// own, stream-ordered device buffers, the copies up, the caller's launches on
// `s`, the copies down.  Everything is released on every path.
//
//     HostCall c("cepstrum");
//     const float* dx = (const float*)c.in(x, 4 * n);
//     float* dc = (float*)c.out(cep, 4 * n);
//     if (!c.ok()) return c.st;
//     return c.finish(vvhip_cepstrum_device(dx, n, 1, dc, c.s));
struct HostCall {
    hipStream_t s = nullptr;   // valid once a buffer exists
    int st = ST_OK;            // the first failure: no device, stream, allocation or copy up

    explicit HostCall(const char* what_) : what(what_) {
        if (device_count() <= 0) st = fail(ST_UNSUP, "no HIP device");
    }
    ~HostCall() {
        for (int i = 0; i < nbuf; ++i)
            if (bufs[i].dev) (void)hipFreeAsync(bufs[i].dev, s);
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    }
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;
    bool ok() const { return st == ST_OK; }

    // A device copy of `bytes` of host memory; a null `host` (an optional
    // input) gives a null device pointer, a zero length a buffer nothing is
    // copied into.
    void* in(const void* host, size_t bytes) { return host ? buffer(host, nullptr, bytes) : nullptr; }
    // A device buffer that finish() copies to `host`.
    void* out(void* host, size_t bytes) { return buffer(nullptr, host, bytes); }
    // Both: a read-modify-write buffer.
    void* inout(void* host, size_t bytes) { return buffer(host, host, bytes); }

    // After the launches, which returned `status`: copies the outputs down when
    // copy_back holds (by default on success only; a callee that wrote its
    // output and then reports ST_NAN passes true), waits for the stream and
    // returns the status, or ST_INTERNAL when a copy or the stream failed.
    int finish(int status) { return finish(status, status == ST_OK); }
    int finish(int status, bool copy_back) {
        if (!ok()) return st;
        if (!copy_back) return status;
        hipError_t e = hipSuccess;
        for (int i = 0; i < nbuf && e == hipSuccess; ++i)
            if (bufs[i].down && bufs[i].bytes)
                e = hipMemcpyAsync(bufs[i].down, bufs[i].dev, bufs[i].bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return e == hipSuccess ? status : fail(ST_INTERNAL, what, e);
    }

private:
    struct Buf {
        void* dev;
        void* down;   // host destination of finish(), or null
        size_t bytes;
    };
    static constexpr int MAX_BUFS = 6;
    const char* what;
    Buf bufs[MAX_BUFS];
    int nbuf = 0;

    void* buffer(const void* up, void* down, size_t bytes) {
        if (!ok()) return nullptr;
        if (nbuf == MAX_BUFS) {
            st = fail(ST_INTERNAL, what);
            return nullptr;
        }
        hipError_t e = s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        void* d = nullptr;
        if (e == hipSuccess) e = hipMallocAsync(&d, bytes ? bytes : 16, s);
        if (e == hipSuccess) bufs[nbuf++] = {d, down, bytes};
        if (e == hipSuccess && up && bytes) e = hipMemcpyAsync(d, up, bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) st = fail(ST_INTERNAL, what, e);
        return e == hipSuccess ? d : nullptr;
    }
};

// ---- the rows of a per-frame entry point (shim_lpc / shim_stats / shim_pitch):
// the FrameSrc (vvhip_internal.hpp) of `batch` rows of n samples ...
inline FrameSrc rows_src(const float* d_x, size_t n, size_t batch, size_t row_stride) {
    FrameSrc src;
    src.x = d_x;
    src.len = (long long)n;
    src.rows = src.frames = (long long)batch;
    src.row_stride = (long long)row_stride;
    return src;
}
// ... and of the frames of nch channels of signal [nch][n]
inline FrameSrc frames_src(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                           size_t hop, size_t frames, int center, const float* d_window) {
    FrameSrc src;
    src.x = d_signal;
    src.len = (long long)frame_len;
    src.frames = (long long)frames;
    src.rows = (long long)(nch * frames);
    src.sig_n = (long long)n;
    src.ch_stride = (long long)ch_stride;
    src.hop = (long long)hop;
    src.framed = 1;
    src.center = center != 0;
    src.win = d_window;
    return src;
}
// The size checks of the framed entry point `who`, in the order every one of
// them makes them; an entry point's own checks stand between the steps, and
// that order is part of its contract (statuses are asserted by the tests).
struct FramesCall {
    const char* who;
    size_t n, nch, frame_len, hop, frames;
    // first, after the null pointers
    int shape() const { return hop == 0 || frame_len == 0 ? ST_SIZE : ST_OK; }
    // what one call and FrameSrc's 32-bit row split take
    int limits() const {
        if (frame_len >= ((size_t)1 << 32) || n >= ((size_t)1 << 40) || nch >= ((size_t)1 << 31) ||
            frames >= ((size_t)1 << 31) || nch * frames >= ((size_t)1 << 31))
            return fail(ST_SIZE, (std::string(who) + ": too many frames for one call").c_str());
        return ST_OK;
    }
    // last: true when there are rows to launch, else *st is what the call returns
    bool start(int* st) const {
        *st = ST_OK;
        if (device_count() <= 0) *st = fail(ST_UNSUP, "no HIP device");
        else if (frames == 0 || nch == 0) return false;
        else if (n == 0) *st = ST_SIZE;   // frames of an empty signal (center): nothing to reflect
        return *st == ST_OK;
    }
};

// ---- shim_lsf.hip: channels per group of the signal -> LSF / formant calls,
// whose LPC rows take per_ch bytes of scratch a channel (knob LSF_GROUP) ----
size_t lsf_group(size_t per_ch, size_t nch);

// ---- shim_fft.hip: the FFT dispatch every other module transforms through ----
// Non-power-of-two DFT: the mixed-radix kernel for 7-smooth n <= 4096, else the
// exact-angle f64 O(n^2) kernel for short lengths and Bluestein over the
// power-of-two kernels from BLUESTEIN_MIN on.  Knob NO_MIXED = 1 skips the
// mixed-radix kernel (A/B and the tests that compare the two).
bool use_mixed(long long n);
hipError_t dft_any(long long n, int fwd, const void* in, int real_in, float2* out, long long nout, long long batch,
                   long long in_dist, long long out_dist, float scale, hipStream_t s);
// Core device dispatch: `batch` transforms, contiguous, device pointers.
int fft_run(size_t n, int type, int dir, const void* in, void* out, size_t batch, hipStream_t s);

}  // namespace vvh

// ---- shim_stft.hip: the STFT handle, which the fused signal -> mel entry
// point (shim_mel.hip) reads as well ------------------------------------------
struct vvhip_stft {
    size_t nfft = 0, hop = 0;
    float* d_win = nullptr;   // on device `dev` (current at create)
    int dev = 0;
    std::vector<float> h_win;
    std::mutex win_mu;        // per-device window copies for device-pointer calls on other GPUs
    std::vector<std::pair<int, float*>> other_wins;
    vvh::HostStage host;
    vvh::DevBuf b0, b1, b2;
};

namespace vvh {

// The handle's window on the calling thread's current device: a device-pointer
// call may run on any GPU of the node (one handle, several shards), so the
// window is copied once to each device that uses it.
const float* stft_window_here(vvhip_stft* h);
// out_kind: 0 magnitude rows [frame][nfft], 1 complex rows [frame][nfft],
// 2 power rows [frame][nfft/2+1]
// frame0/nframes: rows of frames [frame0, frame0 + nframes) only (nframes =
// SIZE_MAX: all).  The signal is viewed from frame0's first sample on: frame
// f >= frame0 of the whole signal is frame f - frame0 of that view, and the
// zero padding past n is the same.
int stft_frames_run(vvhip_stft* h, const float* sig, size_t n, size_t nch, size_t ch_stride, void* out,
                    size_t out_ch_stride, int out_kind, hipStream_t s, size_t frame0 = 0,
                    size_t nframes = SIZE_MAX);

}  // namespace vvh
