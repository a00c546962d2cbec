// pitch_track_kernels.hip -- one f0 contour per channel from the YIN curves of its
// frames: a Viterbi path over (lag, frame) with an unvoiced state, for gfx950.
// include/vv_dsp/features/pitch_track.h states the definition; this file states
// how it is computed.  Every cost is an f64 add of two rounded values and every
// decision a strict comparison in the header's order, so the result does not
// depend on how the states are spread over lanes.
//
// Forward pass (k_ptrack_fwd<P, REG, ONE>).  Sequential in t, parallel over the S
// lags and over channels: one wave per channel up to 64 states (ONE), one workgroup
// per channel beyond: one state per thread and a wave per SIMD up to 256 states,
// ceil(S / 256) waves of four states per thread above.  Thread i owns the states i, i + NT, ...: neighbouring lanes read
// neighbouring doubles of the D vector, which sits in LDS twice (step t reads one
// copy and writes the other), with 8 entries of +inf either side, so the band of a
// state at the edge of the range reads +inf, which no strict comparison takes,
// instead of clipping.  One synchronisation per step: wave_sync() for one wave, a
// barrier beyond.  The curve row of step t + 1 is loaded into registers before
// step t's candidates are examined.  The lowest lag of the smallest D (s*) is an
// xor butterfly on (value, lag) that prefers the lower lag, run on the values a
// step has just produced; waves exchange their results through LDS behind the
// step's barrier.
// Penalties.  REG (up to 256 states and max_step == 8, the default): fl(k r(tau)), k = 0 .. 8,
// of every owned state are computed once into registers before the frame loop, and
// the 17 candidates of the band are unrolled.  Other max_step, or more states: the
// loop over the clipped band computes the product per candidate.  Either way the
// product is pinned behind an empty asm, so it is rounded before the add (no FMA).
// A predecessor is one byte per state and frame (0: U, 1: jump to s*, 2 + k: lag
// tau - B + k), rows of ptrack_row_bytes(S) bytes (state S is U); s* is stored
// once per frame.
//
// Backtrace (k_ptrack_back).  One workgroup per channel walks the frames from the
// last block of L = ptrack_block(S) frames to the first: the block's predecessor
// rows and s* values are staged in LDS with 16-byte loads by all threads, one
// thread walks the block there (dependent LDS reads, not HBM), then every thread
// writes the outputs of one frame of the block (lag, the parabola of pitch.h for
// f0) and the waves take the unvoiced frames' curve minima in turn.
#include "vvhip_internal.hpp"
#include "wave_sync.hpp"

#include <climits>
#include <cmath>

namespace vvh {

namespace {

constexpr int PT_PAD = 8;        // +inf entries either side of a D vector
constexpr int PT_REG_B = 8;      // the max_step whose penalties sit in registers
constexpr int PT_MAX_WAVES = 16;
constexpr size_t PT_LDS_SMALL = 64u << 10;

struct PtK {
    const float* q;              // curves
    long long F, row_stride, cmnd_ch_stride;
    unsigned char* pred;         // [nch][F][PS]
    unsigned* sstar;             // [nch][F]
    unsigned* endst;             // [nch]
    double* cost;                // [nch] or null
    double lambda, jump, sw, uc;
    int tau_min, S, B, PS, dstride;
};

__device__ __forceinline__ double pt_obs(float v) {
    const double x = (double)v;
    return x != x ? (double)INFINITY : x;
}

// fl((double)k * r), rounded before anything is added to it
__device__ __forceinline__ double pt_penalty(int k, double r) {
#pragma clang fp contract(off)
    double p = (double)k * r;
    asm volatile("" : "+v"(p));
    return p;
}

// (bv, bi) <- the smaller of (bv, bi) and (ov, oi): by value, then by lag (selects, no branch)
__device__ __forceinline__ void pt_take(double& bv, int& bi, double ov, int oi) {
    const bool take = (ov < bv) | ((ov == bv) & (oi < bi));
    bv = take ? ov : bv;
    bi = take ? oi : bi;
}

// the smallest of a thread's D values and its lowest lag, then over the wave
template <int P>
__device__ __forceinline__ void pt_wave_min(const double (&d)[P], const bool (&act)[P], const int (&s)[P],
                                            int tau_min, double& bv, int& bi) {
    bv = INFINITY;
    bi = INT_MAX;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const bool take = act[j] & ((bi == INT_MAX) | (d[j] < bv));
        bv = take ? d[j] : bv;
        bi = take ? tau_min + s[j] : bi;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const double ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        pt_take(bv, bi, ov, oi);
    }
}

template <int P, bool REG, bool ONE>
__global__ void __launch_bounds__(ONE ? 64 : 1024) k_ptrack_fwd(PtK k) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char pt_lds[];
    double* Dv = reinterpret_cast<double*>(pt_lds);
    double* wv = Dv + 2 * k.dstride;                       // [2][PT_MAX_WAVES]
    int* wl = reinterpret_cast<int*>(wv + 2 * PT_MAX_WAVES);   // [2][PT_MAX_WAVES]
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = NT >> 6;
    const long long ch = blockIdx.x, F = k.F;
    const int S = k.S, B = k.B;
    const float* q = k.q + ch * k.cmnd_ch_stride + k.tau_min;
    unsigned char* pred = k.pred + (size_t)ch * (size_t)F * (size_t)k.PS;
    unsigned* sstar = k.sstar + ch * F;

    for (int i = tid; i < 2 * k.dstride; i += NT) Dv[i] = INFINITY;
    if (ONE) wave_sync();
    else __syncthreads();

    int s[P], sr[P];   // the owned states; sr: the state whose band is read (an unowned slot reads the last state's)
    bool act[P];
    double r[P], d[P];
    double pen[REG ? P : 1][PT_REG_B + 1];
    float qn[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        s[j] = tid + j * NT;
        act[j] = s[j] < S;
        sr[j] = act[j] ? s[j] : S - 1;
        r[j] = k.lambda / (double)(k.tau_min + sr[j]);
        if constexpr (REG) {
#pragma unroll
            for (int m = 0; m <= PT_REG_B; ++m) pen[j][m] = pt_penalty(m, r[j]);
        }
        qn[j] = q[sr[j]];
    }
    if (!REG) pen[0][0] = 0.0;

    // Step t reads D(t - 1) from one copy and writes D(t) to the other.  One wave: the
    // butterfly over D(t - 1) stands inside step t, where nothing but the jump and U
    // candidates waits for it: the band's candidates, which come after them in the
    // header's order, are reduced first (from +inf, strictly smaller in ascending order)
    // and their winner replaces min(U, jump) only where strictly smaller, which is the
    // same decision.  The P bands of a thread are independent chains with no branch
    // between them, so they overlap each other and the butterfly.
    double DU = k.uc, bv = INFINITY;
    int bi = INT_MAX, cur = 0;
    for (long long t = 0; t < F; ++t) {
        const double* prev = Dv + cur * k.dstride + PT_PAD;
        double* nxt = Dv + (cur ^ 1) * k.dstride + PT_PAD;
        double o[P];
#pragma unroll
        for (int j = 0; j < P; ++j) o[j] = pt_obs(qn[j]);
        if (t + 1 < F) {   // the next row, in flight while this one is reduced
            const float* qr = q + (t + 1) * k.row_stride;
#pragma unroll
            for (int j = 0; j < P; ++j) qn[j] = qr[sr[j]];
        }
        if (t == 0) {
#pragma unroll
            for (int j = 0; j < P; ++j) d[j] = o[j];
        } else {
            double bb[P];
            int bc[P];
#pragma unroll
            for (int j = 0; j < P; ++j) {
                bb[j] = INFINITY;
                bc[j] = 0;
            }
            if constexpr (REG) {
#pragma unroll
                for (int m = 0; m <= 2 * PT_REG_B; ++m) {
                    const int a = m < PT_REG_B ? PT_REG_B - m : m - PT_REG_B;
#pragma unroll
                    for (int j = 0; j < P; ++j) {
                        const double c = prev[sr[j] - PT_REG_B + m] + pen[j][a];
                        const bool take = c < bb[j];
                        bb[j] = take ? c : bb[j];
                        bc[j] = take ? 2 + m : bc[j];
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    if (!act[j]) continue;
                    const int lo = s[j] - B > 0 ? s[j] - B : 0, hi = s[j] + B < S - 1 ? s[j] + B : S - 1;
                    for (int sp = lo; sp <= hi; ++sp) {
                        const int m = sp - s[j];
                        const double c = prev[sp] + pt_penalty(m < 0 ? -m : m, r[j]);
                        if (c < bb[j]) {
                            bb[j] = c;
                            bc[j] = 2 + m + B;
                        }
                    }
                }
            }
            if (ONE) pt_wave_min<P>(d, act, s, k.tau_min, bv, bi);   // of D(t - 1)
            const double cU = DU + k.sw, cJ = bv + k.jump;
            const bool jump = cJ < cU;
            const double b0 = jump ? cJ : cU;
            unsigned char* prow = pred + (size_t)t * (size_t)k.PS;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const bool band = bb[j] < b0;
                d[j] = (band ? bb[j] : b0) + o[j];
                if (act[j]) prow[s[j]] = (unsigned char)(band ? bc[j] : jump ? 1 : 0);
            }
            const double cS = bv + k.sw;
            const bool from_voiced = cS < DU;
            if (tid == 0) {
                prow[S] = (unsigned char)(from_voiced ? 1 : 0);
                sstar[t] = (unsigned)bi;
            }
            DU = (from_voiced ? cS : DU) + k.uc;
        }
#pragma unroll
        for (int j = 0; j < P; ++j)
            if (act[j]) nxt[s[j]] = d[j];
        cur ^= 1;
        if (ONE) {
            wave_sync();
        } else {   // the waves' minima through LDS, behind the step's one barrier
            pt_wave_min<P>(d, act, s, k.tau_min, bv, bi);
            if (lane == 0) {
                wv[cur * PT_MAX_WAVES + wave] = bv;
                wl[cur * PT_MAX_WAVES + wave] = bi;
            }
            __syncthreads();
            bv = wv[cur * PT_MAX_WAVES];
            bi = wl[cur * PT_MAX_WAVES];
            for (int w = 1; w < NW; ++w) pt_take(bv, bi, wv[cur * PT_MAX_WAVES + w], wl[cur * PT_MAX_WAVES + w]);
        }
    }
    if (ONE) pt_wave_min<P>(d, act, s, k.tau_min, bv, bi);   // of D(F - 1)
    if (tid == 0) {
        const bool voiced = bv < DU;
        k.endst[ch] = voiced ? (unsigned)bi : 0u;
        if (k.cost) k.cost[ch] = voiced ? bv : DU;
    }
}

struct PtBack {
    const float* q;
    long long F, row_stride, cmnd_ch_stride, ch_stride;
    const unsigned char* pred;
    const unsigned* sstar;
    const unsigned* endst;
    unsigned* lag;
    float* f0;
    float* ap;
    double fs;
    int tau_min, tau_max, S, B, PS, L;
};

constexpr int PT_BACK_THREADS = 256;

__global__ void __launch_bounds__(PT_BACK_THREADS) k_ptrack_back(PtBack k) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_lds[];
    unsigned char* rows = pb_lds;                                            // [L][PS]
    unsigned* ss = reinterpret_cast<unsigned*>(pb_lds + (size_t)k.L * k.PS);   // [L]
    unsigned* st = ss + k.L;                                                 // [L]: the path's lag, 0 = U
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long ch = blockIdx.x, F = k.F;
    const unsigned char* pred = k.pred + (size_t)ch * (size_t)F * (size_t)k.PS;
    const unsigned* sstar = k.sstar + ch * F;
    const float* q = k.q + ch * k.cmnd_ch_stride;
    unsigned state = k.endst[ch];   // thread 0 carries it from block to block
    const long long nb = (F + k.L - 1) / k.L;
    for (long long b = nb - 1; b >= 0; --b) {
        const long long t0 = b * k.L;
        const int cnt = (int)(F - t0 < k.L ? F - t0 : k.L);
        {   // the block's rows are one run of bytes; PS is a multiple of 16
            const uint4* src = reinterpret_cast<const uint4*>(pred + (size_t)t0 * k.PS);
            uint4* dst = reinterpret_cast<uint4*>(rows);
            const int n16 = cnt * (k.PS / 16);
            for (int i = tid; i < n16; i += PT_BACK_THREADS) dst[i] = src[i];
            for (int i = tid; i < cnt; i += PT_BACK_THREADS) ss[i] = sstar[t0 + i];
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = cnt - 1; i >= 0; --i) {
                st[i] = state;
                if (t0 + i > 0) {
                    const unsigned code = rows[(size_t)i * k.PS + (state ? state - (unsigned)k.tau_min : (unsigned)k.S)];
                    state = code == 0 ? 0u : code == 1 ? ss[i] : state + (code - 2u) - (unsigned)k.B;
                }
            }
        }
        __syncthreads();
        if (tid < cnt) {
            const long long t = t0 + tid;
            const unsigned tau = st[tid];
            const float* qr = q + t * k.row_stride;
            if (k.lag) k.lag[ch * k.ch_stride + t] = tau;
            if (tau && (k.f0 || k.ap)) {
                const float qb = qr[tau];
                if (k.ap) k.ap[ch * k.ch_stride + t] = qb;
                if (k.f0) {
                    const double bq = (double)qb;
                    double off = 0.0;
                    if ((int)tau - 1 >= 1 && (int)tau + 1 <= k.tau_max) {
                        const double a = (double)qr[tau - 1], c = (double)qr[tau + 1];
                        const double den = (a - 2.0 * bq) + c;
                        if (a >= bq && c >= bq && den > 0.0) off = (a - c) / (2.0 * den);
                    }
                    k.f0[ch * k.ch_stride + t] = (float)(k.fs / ((double)tau + off));
                }
            } else if (!tau && k.f0) {
                k.f0[ch * k.ch_stride + t] = 0.0f;
            }
        }
        if (k.ap) {   // unvoiced frames: the first minimum of the row, NaN skipped
            for (int i = wave; i < cnt; i += PT_BACK_THREADS / 64) {
                if (st[i]) continue;
                const float* qr = q + (t0 + i) * k.row_stride;
                float mv = INFINITY;
                int mi = INT_MAX;
                for (int tau = k.tau_min + lane; tau <= k.tau_max; tau += 64) {
                    const float v = qr[tau];
                    if (v == v && (mi == INT_MAX || v < mv)) {
                        mv = v;
                        mi = tau;
                    }
                }
#pragma unroll
                for (int m = 32; m > 0; m >>= 1) {
                    const float ov = __shfl_xor(mv, m);
                    const int oi = __shfl_xor(mi, m);
                    if (oi != INT_MAX && (mi == INT_MAX || ov < mv || (ov == mv && oi < mi))) {
                        mv = ov;
                        mi = oi;
                    }
                }
                if (lane == 0) k.ap[ch * k.ch_stride + t0 + i] = mi == INT_MAX ? NAN : mv;
            }
        }
        __syncthreads();
    }
}

template <int P, bool REG, bool ONE>
hipError_t ptrack_fwd_launch(const PtK& k, long long nch, int threads, size_t lds, hipStream_t s) {
    auto kern = k_ptrack_fwd<P, REG, ONE>;
    if (lds > PT_LDS_SMALL) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)nch), dim3((unsigned)threads), lds, s, k);
    return hipGetLastError();
}

template <bool REG>
hipError_t ptrack_fwd(const PtK& k, long long nch, hipStream_t s) {
    const size_t lds = (size_t)2 * k.dstride * sizeof(double) + 2 * PT_MAX_WAVES * (sizeof(double) + sizeof(int));
    const int waves = (k.S + 63) / 64;
    if (waves == 1) return ptrack_fwd_launch<1, REG, true>(k, nch, 64, lds, s);
    // up to 256 states: one state per thread, a wave per SIMD.  A wave alone on its SIMD issues
    // one dependent instruction every few cycles, so P states per lane take P times as long;
    // four waves of one state each run side by side and meet at the step's barrier.
    if (waves <= 4) return ptrack_fwd_launch<1, REG, false>(k, nch, 64 * waves, lds, s);
    // 16 waves leave a thread 128 VGPRs: the wide form keeps no penalty table
    return ptrack_fwd_launch<4, false, false>(k, nch, 64 * ((k.S + 255) / 256), lds, s);
}

}  // namespace

hipError_t launch_pitch_track(const PtrackCfg& cfg, const PtrackArgs& a, hipStream_t s) {
    const int S = cfg.S();
    if (a.nch <= 0 || a.F <= 0 || a.nch >= (1LL << 31) || a.F >= (1LL << 31) || cfg.tau_min < 1 || S < 2 ||
        S > PTRACK_MAX_STATES || cfg.B < 0 || cfg.B > PTRACK_MAX_STEP || a.row_stride < cfg.tau_max + 1 || !a.work)
        return hipErrorInvalidValue;
    const size_t PS = ptrack_row_bytes(S);
    unsigned char* pred = a.work;
    unsigned* sstar = reinterpret_cast<unsigned*>(pred + (size_t)a.nch * (size_t)a.F * PS);
    unsigned* endst = sstar + (size_t)a.nch * (size_t)a.F;

    PtK k;
    k.q = a.q;
    k.F = a.F;
    k.row_stride = a.row_stride;
    k.cmnd_ch_stride = a.cmnd_ch_stride;
    k.pred = pred;
    k.sstar = sstar;
    k.endst = endst;
    k.cost = a.cost;
    k.lambda = cfg.lambda;
    k.jump = cfg.jump;
    k.sw = cfg.sw;
    k.uc = cfg.uc;
    k.tau_min = cfg.tau_min;
    k.S = S;
    k.B = cfg.B;
    k.PS = (int)PS;
    k.dstride = S + 2 * PT_PAD;
    hipError_t e = cfg.B == PT_REG_B ? ptrack_fwd<true>(k, a.nch, s) : ptrack_fwd<false>(k, a.nch, s);
    if (e != hipSuccess) return e;
    if (!a.lag && !a.f0 && !a.aperiodicity) return hipSuccess;

    PtBack b;
    b.q = a.q;
    b.F = a.F;
    b.row_stride = a.row_stride;
    b.cmnd_ch_stride = a.cmnd_ch_stride;
    b.ch_stride = a.ch_stride;
    b.pred = pred;
    b.sstar = sstar;
    b.endst = endst;
    b.lag = a.lag;
    b.f0 = a.f0;
    b.ap = a.aperiodicity;
    b.fs = cfg.sample_rate;
    b.tau_min = cfg.tau_min;
    b.tau_max = cfg.tau_max;
    b.S = S;
    b.B = cfg.B;
    b.PS = (int)PS;
    b.L = ptrack_block(S);
    const size_t lds = (size_t)b.L * PS + (size_t)b.L * 2 * sizeof(unsigned);
    hipLaunchKernelGGL(k_ptrack_back, dim3((unsigned)a.nch), dim3(PT_BACK_THREADS), lds, s, b);
    return hipGetLastError();
}

}  // namespace vvh
