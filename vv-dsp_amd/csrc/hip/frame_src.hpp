// frame_src.hpp -- the device side of FrameSrc (vvhip_internal.hpp): which
// samples a row of a per-frame kernel reads.  The frame gather k_fetch_frames
// (framing_kernels.hip) and the fused LPC, statistics and pitch kernels all take
// a sample through frame_sample below, so "frame f as the gather delivers it"
// is one piece of text: x_frames == x(fetch_frames) holds by construction.
//
//   reflect_index   the reflection of centred frames (framing.c:21-56)
//   frame_sample    sample i of a row: zero padding, reflection, the window
//   frame_row       where a row's samples are (FrameRow), of either kind of row
#pragma once
#include "vvhip_internal.hpp"

namespace vvh {

// reflection about the ends, period 2n for far indices
__host__ __device__ __forceinline__ long long reflect_index(long long idx, long long n) {
    if (idx < 0) {
        long long a = -idx - 1;
        if (a >= n) {
            const long long period = 2 * n;
            a %= period;
            if (a >= n) a = period - 1 - a;
        }
        return a;
    }
    if (idx >= n) {
        long long r = n - 1 - (idx - n);
        if (r < 0) {
            r = -r - 1;
            if (r >= n) {
                const long long period = 2 * n;
                r %= period;
                if (r >= n) r = period - 1 - r;
            }
        }
        return r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
    }
    return idx;
}

// A row of a FrameSrc: sample i is frame_sample<inside>(s, r, i), which for an
// inside row is p[start + i] (times the window).  at: where the module's
// outputs for the row go, a type of the module's own (NoAt: nowhere from here).
struct NoAt {};
template <class At = NoAt>
struct FrameRow {
    const float* p;
    long long start;
    bool inside;
    At at;
};

// Sample i of the row that starts at sample `start` of the signal p of s.sig_n
// samples: zero outside the signal, or the reflected sample when s.center, then
// one rounded multiply by s.win[i] (win not null).  INSIDE: the caller knows
// that every sample of the row is inside the signal.  p holds samples [base, ..)
// of the signal (k_fetch_frames under a host call; 0 for everyone else).
template <bool INSIDE>
__device__ __forceinline__ float frame_sample(const FrameSrc& s, const float* p, long long start, long long i,
                                              long long base = 0) {
    float v;
    if (INSIDE) {
        v = p[start + i - base];
    } else {
        const long long k = start + i;
        if (s.center) v = p[reflect_index(k, s.sig_n) - base];
        else v = (k < 0 || k >= s.sig_n) ? 0.0f : p[k - base];
    }
    if (s.win) v = v * s.win[i];
    return v;
}
template <bool INSIDE, class At>
__device__ __forceinline__ float frame_sample(const FrameSrc& s, const FrameRow<At>& r, long long i) {
    return frame_sample<INSIDE>(s, r.p, r.start, i);
}
// for a caller that does not specialise its loop on the row's kind
template <class At>
__device__ __forceinline__ float frame_sample(const FrameSrc& s, const FrameRow<At>& r, long long i) {
    return r.inside ? frame_sample<true>(s, r, i) : frame_sample<false>(s, r, i);
}

// Row `row`: row `row` of a batch (its pointer, start 0, inside) or frame f of
// channel ch (the channel's pointer, the frame's first sample, and whether all
// of it is inside the signal).  at_row() / at_frame(ch, f) give the module's
// At; it is formed inside the kind's branch so that it folds into the branch.
// Rows and frames are below 2^31 (the shim checks): the (channel, frame) split
// is a 32-bit division, unless the caller steps (ch, f) = (row / frames,
// row % frames) itself and passes them (stepped; k_lpc_wave).
template <class RowFn, class FrameFn, class I = unsigned>
__device__ __forceinline__ auto frame_row(const FrameSrc& s, long long row, RowFn at_row, FrameFn at_frame,
                                          bool stepped = false, I ch = 0, I f = 0) -> FrameRow<decltype(at_row())> {
    if (!s.framed) return {s.x + row * s.row_stride, 0, true, at_row()};
    if (!stepped) {
        ch = (unsigned)row / (unsigned)s.frames;
        f = (unsigned)row - ch * (unsigned)s.frames;
    }
    const long long start = (long long)f * s.hop - (s.center ? s.len / 2 : 0);
    return {s.x + ch * s.ch_stride, start, start >= 0 && start + s.len <= s.sig_n, at_frame(ch, f)};
}
// ... of a module that places its outputs by other means
struct NoAtFn {
    __device__ NoAt operator()() const { return {}; }
    __device__ NoAt operator()(long long, long long) const { return {}; }
};
__device__ __forceinline__ FrameRow<> frame_row(const FrameSrc& s, long long row) {
    return frame_row(s, row, NoAtFn(), NoAtFn());
}
__device__ __forceinline__ FrameRow<> frame_row(const FrameSrc& s, long long row, long long ch, long long f) {
    return frame_row(s, row, NoAtFn(), NoAtFn(), true, ch, f);
}

}  // namespace vvh
