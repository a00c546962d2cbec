// stft_small.hip -- STFT analysis for the sizes whose last FFT pass cannot be
// mirror-paired in registers (nfft = 256 and 4096): k_stft_pair_lds reads the
// mirror bins back through LDS; magnitude rows have a kernel of their own per
// size (k_stft_stage<256>, k_stft_one<4096>).
#include "stft_common.hpp"
#include "stft_launch.hpp"

namespace vvh {

// Frame pairs for the lengths whose last FFT pass cannot be mirror-paired in
// registers (N = 256 = 16 x 16, 4096 = 16^3: one last-pass butterfly per
// thread): two windowed real frames per complex FFT as k_stft_pair, then the
// spectrum goes through the (idle) LDS exchange buffer in natural order, and
// each thread reads Z[k], Z[N-k] for bins k = t + T j -- so both rows leave
// as lane-contiguous, full-line stores.  Persistent XCD walk with the next
// pair's samples loaded into registers while this pair is transformed.
// (Bounded to three waves per SIMD at N = 256 -- 168 VGPRs, no spills -- its
// magnitude rows ran 4 % slower: profiles/r06_ab_stft_sizes_stage.jsonl; they
// now run in k_stft_stage.)
template <int N, int MODE>
__global__ void __launch_bounds__(Wg<N>::value)
k_stft_pair_lds(const float* sig, long long n, long long nch, long long ch_stride, long long frames,
                long long hop, const float* win, void* out, long long out_ch_stride, long long row_pitch,
                const float2* gpass, const float2* gtab) {
    using G = Geo<N>;
    constexpr int WG = Wg<N>::value, F = Wg<N>::F;
    __shared__ float2 lds[F * G::LDS];
    __shared__ float2 ltab[TwLayout<N>::ENTRIES];
    stage_twiddles<N, WG>(ltab, gpass, gtab);
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T;
    float2* my = lds + slot * G::LDS;
    float w[G::P];   // 0.5 w: Xa = Z[k] + conj Z[N-k] needs no further scaling (pair_post)
#pragma unroll
    for (int r = 0; r < G::P; ++r) w[r] = 0.5f * win[t + r * G::T];
    __syncthreads();
    const TwTab<N> tw{ltab};
    constexpr long long ES = MODE == 1 ? 8 : 4;
    constexpr long long ROW = MODE == 2 ? N / 2 + 1 : N;
    const long long ppc = (frames + 1) / 2, pairs = nch * ppc;
    long long p, p_end, p_step;
    xcd_walk(pairs, F, slot, &p, &p_end, &p_step);
    p = uni<G::T>(p);
    p_end = uni<G::T>(p_end);
    p_step = uni<G::T>(p_step);
    float xa[G::P], xb[G::P];
    auto load = [&](long long q) {
        const long long c = q / ppc, fa = 2 * (q - c * ppc);
        const float* s = sig + c * ch_stride;
        const long long sa = fa * hop, sb = sa + hop;
        const bool hb = fa + 1 < frames;
        if (sb + N <= n) {   // both frames inside the signal
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                xa[r] = s[sa + t + r * G::T];
                xb[r] = s[sb + t + r * G::T];
            }
        } else {
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                const long long i = t + r * G::T;
                xa[r] = sa + i < n ? s[sa + i] : 0.0f;
                xb[r] = hb && sb + i < n ? s[sb + i] : 0.0f;
            }
        }
    };
    if (p < p_end) load(p);
    for (; p < p_end; p += p_step) {
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = make_float2(xa[r] * w[r], xb[r] * w[r]);
        const long long c = p / ppc, fa = 2 * (p - c * ppc);
        const bool hb = fa + 1 < frames;
        if (p + p_step < p_end) load(p + p_step);   // in flight across this pair's FFT and stores
        fft_regs<N, true>(v, t, my, tw);
#pragma unroll
        for (int q = 0; q < G::P; ++q) my[G::pad(out_pos<N>(t, q))] = v[q];
        xsync<G::T>();
        const long long rp = MODE == 2 ? row_pitch : ROW;   // power rows: row_pitch floats apart
        char* rowa = reinterpret_cast<char*>(out) + (c * out_ch_stride + fa * rp) * ES;
        char* rowb = rowa + rp * ES;
        if constexpr (N == 4096 && MODE == 0) {
            // bins k = t + T j <= N/2 only: bin N - k of a real frame is the
            // conjugate of bin k, bit for bit (pair_post with Z[k], Z[N-k] swapped
            // gives conj(A), conj(B) exactly: the sums commute and negation is
            // exact), so each post serves both bins -- half the posts and LDS
            // reads: 5.48 -> 5.17 ms for 32 ch x 10 min.  (At N = 256 the mirror
            // halves are 16-lane, one-float-misaligned 64 B segments whose
            // streaming stores leave partial lines: 2x slower there, and complex
            // rows at 4096 +16 %: not used; profiles/r06_ab_fir_run_stft_sizes.jsonl.)
#pragma unroll
            for (int j = 0; j <= G::P / 2; ++j) {
                const int k = t + G::T * j;
                if (j == G::P / 2 && t != 0) continue;   // bin N/2 (its own mirror): thread 0
                float2 A, B;
                pair_post<MODE>(my[G::pad(k)], my[G::pad((N - k) & (N - 1))], &A, &B);
                const bool mir = MODE != 2 && k != 0 && k != N / 2;   // bin N - k is another bin
                // bases at bins t and N - t: bin k = t + T j and N - k at -T j
                if constexpr (MODE == 1) {
                    float2* ra = reinterpret_cast<float2*>(rowa) + t;
                    float2* rm = reinterpret_cast<float2*>(rowa) + (N - t);
                    st_nt(A, ra + G::T * j);
                    if (mir) st_nt(cconj(A), rm - G::T * j);
                    if (hb) {
                        st_nt(B, ra + (rowb - rowa) / 8 + G::T * j);
                        if (mir) st_nt(cconj(B), rm + (rowb - rowa) / 8 - G::T * j);
                    }
                } else {
                    float* ra = reinterpret_cast<float*>(rowa) + t;
                    float* rm = reinterpret_cast<float*>(rowa) + (N - t);
                    __builtin_nontemporal_store(A.x, ra + G::T * j);
                    if (mir) __builtin_nontemporal_store(A.x, rm - G::T * j);
                    if (hb) {
                        __builtin_nontemporal_store(B.x, ra + rp + G::T * j);
                        if (mir) __builtin_nontemporal_store(B.x, rm + rp - G::T * j);
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < G::P; ++j) {
                const int k = t + G::T * j;
                if (MODE == 2 && k > N / 2) continue;
                float2 A, B;
                pair_post<MODE>(my[G::pad(k)], my[G::pad((N - k) & (N - 1))], &A, &B);
                if constexpr (MODE == 1) {
                    st_nt(A, reinterpret_cast<float2*>(rowa) + k);
                    if (hb) st_nt(B, reinterpret_cast<float2*>(rowb) + k);
                } else {
                    __builtin_nontemporal_store(A.x, reinterpret_cast<float*>(rowa) + k);
                    if (hb) __builtin_nontemporal_store(B.x, reinterpret_cast<float*>(rowb) + k);
                }
            }
        }
        xsync<G::T>();   // the next pair's FFT exchange reuses `my`
    }
}

// ------------------------------------------------------------------------
// k_stft_one<N>: magnitude rows with ONE frame pair per transform slot and no
// loop (N = 4096) -- no prefetch registers, no persistent walk: the occupancy
// hides the latency and the dispatcher balances the CUs (k_c2c ONE's shape,
// which took c2c 4096 from 0.72 to 0.775).  Slot s of block b takes pair
// (b % 8) per8 + (b / 8) F + s: each XCD (block b runs on XCD b % 8) walks its
// own contiguous eighth of the pairs, so the N + hop - 2 hop overlap of
// neighbouring spans comes from that XCD's L2.  The frames are windowed on load
// (zero past the end of the signal), two per complex FFT; the spectrum goes to
// LDS in natural order and each post serves bin k and its mirror N - k (bit for
// bit the same magnitude), as k_stft_pair_lds<4096>.
// ------------------------------------------------------------------------
// Twiddles of a one-transform kernel whose threads own one last-pass butterfly
// each (T = N/16, e.g. N = 4096): the passes before the last read the LDS
// pass-major table (its first tw_off(LAST) entries: 240 at 4096); the last
// pass' W_N^{t r} (j = t) are powers of W = W_N^t -- one L2 load per thread,
// each power a product of W, W^2, W^4, W^8 (at most four roundings deep) --
// instead of the two-level table's two LDS reads, index arithmetic and complex
// multiply per twiddle.
template <int N>
struct TwPow {
    using G = Geo<N>;
    static constexpr int LAST = G::NPASS - 1, RL = G::RL, NS = G::ns(LAST);
    static_assert(G::T == NS && G::P == RL, "one last-pass butterfly per thread, j = t");
    const float2* tab;
    float2 w[RL - 1];   // w[r - 1] = W^r
    template <int p>
    __device__ __forceinline__ float2 at(int j, int r, int /*i*/ = 0) const {
        if constexpr (p == LAST) return w[r - 1];
        else return tab[G::tw_off(p) + (r - 1) * G::ns(p) + j];
    }
    __device__ __forceinline__ void init(float2 W) {
        w[0] = W;
#pragma unroll
        for (int r = 2; r < RL; ++r) {
            const int hp = 1 << (31 - __builtin_clz(r));   // the highest power of two <= r
            w[r - 1] = r == hp ? cmul(w[hp / 2 - 1], w[hp / 2 - 1]) : cmul(w[hp - 1], w[r - hp - 1]);
        }
    }
};

template <int N, int VAR>
__global__ void __launch_bounds__(Wg<N>::value)
k_stft_one(const float* sig, long long n, long long nch, long long ch_stride, long long frames, long long hop,
           const float* win, float* out, long long out_ch_stride, const float2* gpass, const float2* gtab,
           long long per8) {
    // VAR bits: 1 the samples loaded before the twiddles are staged; 2 the
    // half-size real/imaginary exchange (and spectrum pass), half the LDS per
    // transform; 4 the last pass' twiddles as powers in registers (TwPow)
    // instead of the two-level lo * hi table
    using G = Geo<N>;
    static_assert(G::T >= 64 && G::T % 64 == 0, "whole waves per transform");
    constexpr bool EARLY = VAR & 1, RI = VAR & 2, TLR = VAR & 4;
    constexpr int WG = Wg<N>::value, F = Wg<N>::F, JH = G::P / 2;
    constexpr int XF = RI ? (ri_floats<N>() + 3) / 4 * 2 : G::LDS;   // float2 per transform
    __shared__ __attribute__((aligned(16))) float2 lds[F * XF];
    using TW = std::conditional_t<TLR, TwPow<N>, TwTab<N>>;
    __shared__ float2 ltab[TLR ? G::tw_off(G::NPASS - 1) : TwLayout<N>::ENTRIES];
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T;
    float2* my = lds + slot * XF;
    const long long b = blockIdx.x;
    const long long ppc = (frames + 1) / 2, pairs = nch * ppc;
    const long long p = uni<G::T>((b & 7) * per8 + (b >> 3) * F + slot);
    const bool act = p < pairs;   // uniform per transform
    const long long pc = act ? p : 0;   // an idle slot (F > 1) transforms pair 0 and stores nothing
    // (channel, first frame): 32-bit division (the launcher keeps pairs < 2^31)
    const unsigned cu = (unsigned)pc / (unsigned)ppc;
    const long long c = cu, fa = 2 * (pc - (long long)cu * ppc);
    const float* s = sig + c * ch_stride;
    const long long sa = fa * hop, sb = sa + hop;
    const bool hb = fa + 1 < frames;
    float2 v[G::P];
    auto load = [&]() {
        if (sb + N <= n) {   // both frames inside the signal
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                const float w = 0.5f * win[t + r * G::T];
                v[r] = make_float2(s[sa + t + r * G::T] * w, s[sb + t + r * G::T] * w);
            }
        } else {
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                const long long i = t + r * G::T;
                const float w = 0.5f * win[i];
                const float xa = sa + i < n ? s[sa + i] : 0.0f;
                const float xb = hb && sb + i < n ? s[sb + i] : 0.0f;
                v[r] = make_float2(xa * w, xb * w);
            }
        }
    };
    if constexpr (EARLY) load();
    TW tw{ltab};
    float2 w1 = make_float2(1.0f, 0.0f);
    if constexpr (TLR) {
        w1 = gtab[t];   // W_N^t
        for (int i = threadIdx.x; i < G::tw_off(G::NPASS - 1); i += WG) ltab[i] = gpass[i];
    } else {
        stage_twiddles<N, WG>(ltab, gpass, gtab);
    }
    __syncthreads();
    if constexpr (F == 1) {
        if (!act) return;
    }
    if constexpr (!EARLY) load();
    if constexpr (TLR) tw.init(w1);
    fft_regs<N, true, false, RI, TW>(v, t, my, tw);
    float* ra = out + c * out_ch_stride + fa * N;
    float* rb = ra + N;
    // each post stores bin k and its mirror N - k at once (k <= N/2; the
    // mirror blocks one float off the 256 B grid)
    auto post = [&](const float2* z, const float2* zm) {
#pragma unroll
        for (int j = 0; j <= JH; ++j) {
            const int k = t + G::T * j;
            if (j == JH && t != 0) continue;   // bin N/2 (its own mirror): thread 0
            float2 A, B;
            pair_post<0>(z[j], zm[j], &A, &B);
            const bool mir = k != 0 && k != N / 2;   // bin N - k is another bin
            __builtin_nontemporal_store(A.x, ra + k);
            if (mir) __builtin_nontemporal_store(A.x, ra + N - k);
            if (hb) {
                __builtin_nontemporal_store(B.x, rb + k);
                if (mir) __builtin_nontemporal_store(B.x, rb + N - k);
            }
        }
    };
    float2 z[JH + 1], zm[JH + 1];
    if constexpr (RI) {
        // the spectrum in natural order through the half-size buffer: real
        // parts, then imaginary parts, of bins k and N - k
        float* lf = reinterpret_cast<float*>(my);
#pragma unroll
        for (int q = 0; q < G::P; ++q) lf[G::pad(out_pos<N>(t, q))] = v[q].x;
        xsync<G::T>();
#pragma unroll
        for (int j = 0; j <= JH; ++j) {
            const int k = j < JH ? t + G::T * j : N / 2;
            z[j].x = lf[G::pad(k)];
            zm[j].x = lf[G::pad((N - k) & (N - 1))];
        }
        xsync<G::T>();
#pragma unroll
        for (int q = 0; q < G::P; ++q) lf[G::pad(out_pos<N>(t, q))] = v[q].y;
        xsync<G::T>();
#pragma unroll
        for (int j = 0; j <= JH; ++j) {
            const int k = j < JH ? t + G::T * j : N / 2;
            z[j].y = lf[G::pad(k)];
            zm[j].y = lf[G::pad((N - k) & (N - 1))];
        }
    } else {
#pragma unroll
        for (int q = 0; q < G::P; ++q) my[G::pad(out_pos<N>(t, q))] = v[q];
        xsync<G::T>();
#pragma unroll
        for (int j = 0; j <= JH; ++j) {
            const int k = j < JH ? t + G::T * j : N / 2;
            z[j] = my[G::pad(k)];
            zm[j] = my[G::pad((N - k) & (N - 1))];
        }
    }
    if (!act) return;   // after the last barrier
    post(z, zm);
}

// ------------------------------------------------------------------------
// k_stft_stage<N>: magnitude rows for N = 256 (T = 16 threads per transform,
// four transforms per wave) with every global access a coalesced 16 B per
// lane.  k_stft_pair_lds reads each frame as 16 dword loads of 64 B per slot
// (four frames of four pairs per instruction) and writes each row the same
// way.  Here the four slots of a wave take four consecutive frame pairs of one
// channel (xcd_walk gives a wave's slots consecutive pairs), so the wave's
// eight frames are ONE span of 7 hop + N samples: it comes in as <= 3
// dwordx4 per lane (issued one step ahead, 12 VGPRs instead of 32), is laid
// into the wave's idle exchange buffers, and each slot reads its two frames
// from there.  After the transforms and the mirror-bin posts (bins k <= N/2,
// bin N - k its mirror) the wave's eight rows -- 2048 contiguous floats --
// go back through the same buffers and leave as eight dwordx4 streaming
// stores per lane.  Steps whose four pairs cross a channel, reach past the
// end of the signal (zero padding) or would need an unaligned span take the
// per-slot path with the padding rule, in the same loop (a wave-uniform
// branch).  Bit-identical to k_stft_pair_lds<N, 0> (same transform, same posts).
// ------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(256, 3)
k_stft_stage(const float* sig, long long n, long long nch, long long ch_stride, long long frames, long long hop,
             const float* win, float* out, long long out_ch_stride, const float2* gpass, const float2* gtab) {
    using G = Geo<N>;
    constexpr int T = G::T, NT = 64 / T, F = 256 / T;
    constexpr int WF = NT * G::LDS * 2;        // floats of one wave's exchange buffers
    constexpr int ROWS = 2 * NT * N;           // floats of the wave's eight rows
    constexpr int U = 3;                       // span pieces of 256 floats: 7 hop + N <= 768
    static_assert(T == 16 && ROWS <= WF && U * 256 <= WF, "N = 256: four transforms per wave");
    __shared__ __attribute__((aligned(16))) float2 lds[F * G::LDS];
    __shared__ float2 ltab[TwLayout<N>::ENTRIES];
    stage_twiddles<N, 256>(ltab, gpass, gtab);
    const int lt = threadIdx.x, slot = lt / T, t = lt % T, lane = lt & 63, ws = slot % NT;
    float2* my = lds + slot * G::LDS;
    float* wb = reinterpret_cast<float*>(lds + (slot - ws) * G::LDS);   // the wave's buffers (16 B aligned)
    float w[G::P];   // 0.5 w (pair_post)
#pragma unroll
    for (int r = 0; r < G::P; ++r) w[r] = 0.5f * win[t + r * T];
    __syncthreads();
    const TwTab<N> tw{ltab};
    const long long ppc = (frames + 1) / 2, pairs = nch * ppc;
    long long p, p_end, p_step;
    xcd_walk(pairs, F, slot, &p, &p_end, &p_step);
    long long p0 = uni<64>(p - ws);   // the wave's first pair (its slots hold p0 .. p0 + NT - 1)
    p_end = uni<64>(p_end);
    p_step = uni<64>(p_step);
    const int span = (int)(2 * NT - 1) * (int)hop + N;   // the launcher keeps it <= U * 256
    // wave-uniform: the NT pairs from q0 lie in one channel, all 2 NT frames
    // inside the signal, and their span starts 16 B aligned
    auto staged_ok = [&](long long q0) -> bool {
        if (q0 + NT > p_end) return false;
        const long long c = q0 / ppc, q = q0 - c * ppc;
        if (q + NT > ppc) return false;
        const long long f0 = 2 * q;
        if (f0 + 2 * NT > frames || (f0 + 2 * NT - 1) * hop + N > n) return false;
        return ((c * ch_stride + f0 * hop) & 3) == 0;
    };
    vf4_t pre[U];
    auto issue = [&](long long q0) {
        const long long c = q0 / ppc, f0 = 2 * (q0 - c * ppc);
        const vf4_t* s = reinterpret_cast<const vf4_t*>(sig + c * ch_stride + f0 * hop);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = 4 * lane + 256 * u;
            pre[u] = e < span ? s[e >> 2] : vf4_t{0.0f, 0.0f, 0.0f, 0.0f};   // plain loads: the span overlaps the next wave's (L2)
        }
    };
    bool stg = p0 < p_end && staged_ok(p0);
    if (stg) issue(p0);
    for (; p0 < p_end; p0 += p_step) {
        const long long qq = p0 + ws, q = qq < p_end ? qq : p_end - 1;   // invalid slots redo a valid pair
        const bool qv = qq < p_end;
        const long long c = q / ppc, fa = 2 * (q - c * ppc);
        const bool hb = fa + 1 < frames;
        float xa[G::P], xb[G::P];
        const bool stg0 = stg;
        if (stg0 && hop == 64) {
            // hop 64 (nfft / 4): the span laid out with 16 floats of pad per 128, so
            // the four slots' frames (128 floats apart) read from four distinct bank
            // quarters: unpadded, slots ws and ws + 1 of a 32-lane group hit the
            // same 16 banks on every frame read (a 2-way conflict per instruction)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (4 * lane + 256 * u < span)
                    *reinterpret_cast<vf4_t*>(wb + 4 * lane + 256 * u + 16 * (lane >> 5) + 32 * u) = pre[u];
            xsync<64>();
            const float* fsa = wb + 144 * ws + t;   // element e at e + 16 (e >> 7)
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                xa[r] = fsa[T * r + 16 * (r >> 3)];
                xb[r] = fsa[64 + T * r + 16 * ((r + 4) >> 3)];
            }
            xsync<64>();
        } else if (stg0) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (4 * lane + 256 * u < span) *reinterpret_cast<vf4_t*>(wb + 4 * lane + 256 * u) = pre[u];
            xsync<64>();
            const float* fsa = wb + 2 * ws * hop + t;
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                xa[r] = fsa[T * r];
                xb[r] = fsa[hop + T * r];
            }
            xsync<64>();
        } else {
            const float* sg = sig + c * ch_stride;
            const long long sa = fa * hop, sb = sa + hop;
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                const long long i = t + r * T;
                xa[r] = sa + i < n ? sg[sa + i] : 0.0f;
                xb[r] = hb && sb + i < n ? sg[sb + i] : 0.0f;
            }
        }
        // the next step's span, in flight across this step's transforms and stores
        stg = p0 + p_step < p_end && staged_ok(p0 + p_step);
        if (stg) issue(p0 + p_step);
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = make_float2(xa[r] * w[r], xb[r] * w[r]);
        fft_regs<N, true>(v, t, my, tw);
#pragma unroll
        for (int k = 0; k < G::P; ++k) my[G::pad(out_pos<N>(t, k))] = v[k];
        xsync<T>();
        float A[G::P / 2 + 1], B[G::P / 2 + 1];
#pragma unroll
        for (int j = 0; j <= G::P / 2; ++j) {
            const int k = t + T * j;
            float2 a, b;
            pair_post<0>(my[G::pad(k & (N - 1))], my[G::pad((N - k) & (N - 1))], &a, &b);
            A[j] = a.x;
            B[j] = b.x;
        }
        xsync<64>();   // every slot of the wave has read its spectrum: the buffers take the rows
        if (stg0) {
            float* ra = wb + 2 * ws * N;
#pragma unroll
            for (int j = 0; j <= G::P / 2; ++j) {
                const int k = t + T * j;
                if (j == G::P / 2 && t != 0) continue;   // bin N/2: thread 0
                ra[k] = A[j];
                ra[N + k] = B[j];
                if (k != 0 && k != N / 2) {
                    ra[N - k] = A[j];
                    ra[2 * N - k] = B[j];
                }
            }
            xsync<64>();
            const long long cw = p0 / ppc, f0 = 2 * (p0 - cw * ppc);
            vf4_t* dst = reinterpret_cast<vf4_t*>(out + cw * out_ch_stride + f0 * N);
#pragma unroll
            for (int u = 0; u < ROWS / 256; ++u)
                __builtin_nontemporal_store(*reinterpret_cast<const vf4_t*>(wb + 4 * lane + 256 * u), dst + lane + 64 * u);
        } else if (qv) {
            float* rowa = out + c * out_ch_stride + fa * N;
            float* r0 = rowa + t;
            float* rm = rowa + (N - t);
#pragma unroll
            for (int j = 0; j <= G::P / 2; ++j) {
                const int k = t + T * j;
                if (j == G::P / 2 && t != 0) continue;
                const bool mir = k != 0 && k != N / 2;
                __builtin_nontemporal_store(A[j], r0 + T * j);
                if (mir) __builtin_nontemporal_store(A[j], rm - T * j);
                if (hb) {
                    __builtin_nontemporal_store(B[j], r0 + N + T * j);
                    if (mir) __builtin_nontemporal_store(B[j], rm + N - T * j);
                }
            }
        }
        xsync<64>();   // the next step's span / exchange reuses the buffers
    }
}

template <int N, int MODE>
hipError_t run_stft_small(const StftJob& j) {
    static_assert(!Geo<N>::CAN_PAIR, "the mirror-paired sizes: stft_pair.hip");
    const float* const sig = j.sig;
    const long long n = j.n, nch = j.nch, ch_stride = j.ch_stride, frames = j.frames, hop = j.hop,
                    out_ch_stride = j.out_ch_stride;
    const float2* tN = twiddle_table(N);
    const float2* pN = pass_twiddles(N);
    if (!tN || !pN) return hipErrorOutOfMemory;
    constexpr int WG = Wg<N>::value, F = Wg<N>::F;
    const long long pairs = nch * ((frames + 1) / 2);
    if constexpr (MODE == 0 && N == 4096) {
        // one frame pair per transform slot, no loop (k_stft_one VAR 5: the loads
        // before the twiddle staging, the last pass' twiddles as powers in
        // registers): 5.07 -> 4.13 ms for 32 ch x 10 min against k_stft_pair_lds
        // (0.454 -> 0.558 of HBM; profiles/r06_ab_stft4096_one.jsonl: the
        // half-size exchange at five workgroups per CU, the lane-0 trade for
        // aligned mirror blocks and the two-level twiddle table were slower).
        // Knob STFT_ONE = 0 keeps k_stft_pair_lds (A/B)
        if (knob(KNOB_STFT_ONE, 1) != 0 && pairs < (1LL << 31)) {
            const long long per8 = ((pairs + 8 * F - 1) / (8 * F)) * F;   // pairs per XCD, whole blocks
            const long long grid = 8 * (per8 / F);
            if (pairs < 1) return hipSuccess;
            hipLaunchKernelGGL((k_stft_one<N, 5>), dim3((unsigned)grid), dim3(WG), 0, j.s, sig, n, nch, ch_stride,
                               frames, hop, j.win, (float*)j.out, out_ch_stride, pN, tN, per8);
            return hipGetLastError();
        }
    }
    if constexpr (N == 256 && MODE == 0) {
        // magnitude rows with every global access 16 B per lane (k_stft_stage);
        // knob STFT_STAGE = 0 keeps k_stft_pair_lds (A/B)
        if (7 * hop + N <= 768 && hop % 4 == 0 && ((uintptr_t)sig & 15) == 0 && ((uintptr_t)j.out & 15) == 0 &&
            (out_ch_stride & 3) == 0 && knob(KNOB_STFT_STAGE, 1) != 0) {
            static std::atomic<int> caps;
            const int grid = capped_grid(caps, (const void*)k_stft_stage<N>, 256, (pairs + F - 1) / F);
            if (grid < 1) return hipSuccess;
            hipLaunchKernelGGL((k_stft_stage<N>), dim3(grid), dim3(256), 0, j.s, sig, n, nch, ch_stride, frames, hop,
                               j.win, (float*)j.out, out_ch_stride, pN, tN);
            return hipGetLastError();
        }
    }
    // frame pairs with the mirror bins read back through LDS
    static std::atomic<int> capl;
    const int grid = capped_grid(capl, (const void*)k_stft_pair_lds<N, MODE>, WG, (pairs + F - 1) / F);
    if (grid < 1) return hipSuccess;
    hipLaunchKernelGGL((k_stft_pair_lds<N, MODE>), dim3(grid), dim3(WG), 0, j.s, sig, n, nch, ch_stride, frames, hop,
                       j.win, j.out, out_ch_stride, j.row_pitch, pN, tN);
    return hipGetLastError();
}

#define VVH_INST(NN, M) template hipError_t run_stft_small<NN, M>(const StftJob&);
VVH_INST(256, 0) VVH_INST(256, 1) VVH_INST(256, 2) VVH_INST(4096, 0) VVH_INST(4096, 1) VVH_INST(4096, 2)
#undef VVH_INST

}  // namespace vvh
