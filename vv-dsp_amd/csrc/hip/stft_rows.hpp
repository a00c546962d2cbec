// stft_rows.hpp -- the row emitters of the one-wave-per-transform kernels
// (N = 1024): magnitude / complex / power rows straight from the FFT registers
// (direct_rows), and the fused log-mel / MFCC rows (mel_rows for k_stft_pair,
// mel_tail also for k_stft_r32).
#pragma once
#include "stft_common.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// Rows of one frame pair straight from the FFT registers (N = 1024: one wave
// per transform, mirror-paired last pass; see k_stft_pair).  Issues exactly
// the kernel's NST stores per pair (rows of a missing second frame go to the
// sink), so the caller's hand-counted vmcnt stays exact.
template <int N, int MODE>
__device__ __forceinline__ void direct_rows(const float2* v, int t, char* rowa, char* rowb, bool has_b,
                                            float* sink) {
    using G = Geo<N>;
    using Mi = Mirror<N>;
    constexpr int R = G::RL;
    if constexpr (MODE == 1) {
        // as the DIRECT block below, with complex bins: a mirror block holds
        // conj(X[k]) (real frames), lane 0's rotated partner conj of its own
        // bin in slot j + 1, or in the last slot its self-mirrored bin as is.
        // Byte offsets reach 8 KB: blocks past 4 KB use the base + 4096.
        constexpr int J = G::NPT / 2, NB = G::NB, T = G::T;
        const unsigned ve = 8u * (unsigned)t;
        const unsigned vo = 8u * (unsigned)(t == 0 ? 0 : T - t);
        const char* ra = rowa;
        const char* rb = has_b ? rowb : reinterpret_cast<const char*>(sink);   // counted stores must all issue
        const char* ra2 = ra + 4096;
        const char* rb2 = rb + 4096;
        auto st = [&](auto imm, unsigned off, float2 val, const char* b1, const char* b2) {
            constexpr int I = decltype(imm)::value;
            if constexpr (I < 4096) st8_nt_sbase<I>(off, val, b1);
            else st8_nt_sbase<I - 4096>(off, val, b2);
        };
        float2 nxa[R], nxb[R];   // lane 0's partner values for slot j: conj of slot j+1's own bins
        static_for<0, J>([&](auto jc) {
            constexpr int j = J - 1 - decltype(jc)::value;   // last slot first: its partners are the specials
            static_for<0, R>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                constexpr int q = 2 * j * R + r;
                float2 A, B;
                pair_post<1>(v[q], mirror_of<N, true>(v, t, q), &A, &B);
                float2 pa, pb;
                if constexpr (j == J - 1) {
                    const int qm = Mi::normal(r);
                    pair_post<1>(v[qm], v[Mi::special(qm)], &pa, &pb);
                } else {
                    pa = nxa[r];
                    pb = nxb[r];
                }
                const float2 oa = select2(t == 0, pa, cconj(A)), ob = select2(t == 0, pb, cconj(B));
                nxa[r] = cconj(A);
                nxb[r] = cconj(B);
                constexpr int IE = 8 * (T * j + r * NB), IO = 8 * ((R - 1 - r) * NB - T * j + NB - T);
                st(std::integral_constant<int, IE>{}, ve, A, ra, ra2);
                st(std::integral_constant<int, IE>{}, ve, B, rb, rb2);
                st(std::integral_constant<int, IO>{}, vo, oa, ra, ra2);
                st(std::integral_constant<int, IO>{}, vo, ob, rb, rb2);
            });
        });
    } else {
        // Even slot j holds bins k = t + T j + r NB (lane-contiguous, 256 B
        // aligned per store); its partner slot holds N - k, which for lanes
        // t >= 1 covers N - k of the same magnitude.  Lane 0's partner bins
        // are shifted by one slot (lane 0 writes the mirror of its own bin in
        // slot j + 1, or its self-mirrored bin NB/2 + .. in the last slot), so
        // that every store instruction covers one aligned 256 B block: full
        // 128 B lines for the streaming stores, no LDS staging.
        constexpr int J = G::NPT / 2, NB = G::NB, T = G::T;
        constexpr int PM = MODE == 2 ? 2 : 0;   // magnitude or power post
        float ea[J][R], eb[J][R], sa[R], sb[R];
#pragma unroll
        for (int j = 0; j < J; ++j) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int q = 2 * j * R + r;
                float2 A, B;
                pair_post<PM>(v[q], mirror_of<N, true>(v, t, q), &A, &B);
                ea[j][r] = A.x;
                eb[j][r] = B.x;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {   // lane 0's odd slot 1: bins NB/2 + (R-1-r) NB, their own mirrors
            const int qm = Mi::normal(r);
            float2 A2, B2;
            pair_post<PM>(v[qm], v[Mi::special(qm)], &A2, &B2);
            sa[r] = A2.x;
            sb[r] = B2.x;
        }
        const unsigned ve = 4u * (unsigned)t;
        const unsigned vo = 4u * (unsigned)(t == 0 ? NB - T : NB - t);
        const void* ra = rowa;
        const void* rb = has_b ? rowb : (void*)sink;   // counted stores must all issue
        // Power rows (n/2+1 floats, so not line-aligned): a block is stored
        // only if it lies below N/2, with plain stores (partial lines merge
        // in L2; streaming stores of partial lines measured 1.65x slower)
        auto st = [&](auto imm, unsigned off, float val, const void* base) {
            constexpr int I = decltype(imm)::value;
            if constexpr (MODE == 2) {
                if constexpr (I < 4 * (N / 2)) st4_sbase<I>(off, val, base);
            } else {
                // streaming stores with sc0 sc1 (write-through, not kept in L2):
                // 0.6 % faster than nt alone on the config-5 shard (same-box A/B,
                // six alternating runs each)
                st4_pol_sbase<I, 2>(off, val, base);
            }
        };
        // The N/T blocks of a row in ascending address order, row a then
        // row b (measured 0.5 % faster than interleaving the rows).  Block
        // m is an even block (slot j = m % (NB/T) < J, r = m / (NB/T)) or
        // the mirror block of (j, r) with (N/T - 1) - m = r (NB/T) + j.
        auto val = [&](auto mc, const float (&e)[J][R], const float (&sp)[R]) -> float {
            constexpr int m = decltype(mc)::value;
            constexpr int je = m % (NB / T), re = m / (NB / T);
            if constexpr (je < J) {
                return e[je][re];
            } else {
                constexpr int mm = (N / T - 1) - m, rm = mm / (NB / T), jm = mm % (NB / T);
                if constexpr (jm + 1 < J) return t == 0 ? e[jm + 1][rm] : e[jm][rm];
                else return t == 0 ? sp[rm] : e[jm][rm];
            }
        };
        auto row = [&](const float (&e)[J][R], const float (&sp)[R], const void* base) {
            static_for<0, N / T>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                if constexpr (m % (NB / T) < J) st(std::integral_constant<int, 4 * T * m>{}, ve, val(mc, e, sp), base);
                else st(std::integral_constant<int, 4 * T * m>{}, vo - 4u * (NB - T), val(mc, e, sp), base);
            });
        };
        row(ea, sa, ra);
        row(eb, sb, rb);
        if constexpr (MODE == 2) {
            // bin N/2 = NB * (R/2): even slot j = 0, r = R/2, lane 0 (one
            // lane-0 store per row, counted; rb is the sink for a missing frame)
            static_assert(N / 2 == NB * (R / 2), "Nyquist bin in lane 0 of an even block");
            st4_lane0_counted((float*)ra + N / 2, ea[0][R / 2]);
            st4_lane0_counted((float*)rb + N / 2, eb[0][R / 2]);
        }
    }
}

// Log-mel (MODE 3) or MFCC (MODE 4) rows of one frame pair from the FFT
// registers (N = 1024, one wave per transform).  The power of bins 0..N/2 of
// both frames (pair_post<2>: the power rows' arithmetic) goes to the
// transform's idle exchange buffer P, the two rows interleaved bin by bin; then k_mel_grp's steps
// with FR = 2 frames: chunk partials (FMA in bin order; lane c % 64 holds chunk
// c in round c / 64), per-filter sums of the partials in chunk order (fetched
// across lanes by ds_bpermute), logf(e + eps), and for MODE 4 the DCT-II and
// lifter over the log-mel rows (kept in P's spare tail) -- the same operations
// in the same order, so the rows equal launch_stft mode 2 followed by
// launch_mel_grp bit for bit.  The plan's tables sit in dynamic LDS (about
// 4-8 KB), paid for by spans of N + 256 floats (hop <= 256), so 3 workgroups
// per CU still fit; no compiler-generated global load enters the hand-counted
// pipeline.  Stores: MODE 3 four counted dword stores (rows a, b x filters
// t, t + 64; M <= 128), MODE 4 two ((frame, coefficient) pairs t, t + 64;
// C <= 64); lanes without a row element write to the sink.
constexpr int MEL_MAX_ROUNDS = 4;   // chunks <= 256
constexpr int MEL_LM_OFF = 1028;    // MODE 4: log-mel rows in P past the two power rows (16 B aligned)
// MelArgs::W2: the zeros at bins N/2 + 1 .. N/2 + 3 (P floats below MEL_ZERO_END) alias the first log-mel floats, so
// every transform must rewrite them before its tail's window reads, and those reads must end (xsync) before lm is written
constexpr int MEL_ZERO_END = 2 * (1024 / 2 + 4);
static_assert(!MelArgs::W2 || (2 * (1024 / 2 + 1) <= MEL_LM_OFF && MEL_LM_OFF < MEL_ZERO_END),
              "the zero tail overlaps the log-mel rows: the order above is what keeps it safe");
template <int MODE, bool COUNTED>
__device__ __forceinline__ void mel_tail(int t, float* P, float* fa, float* fb, bool has_b, float* sink,
                                         const float* sW, const int* sCh, const int* sCb, const float* sD,
                                         const float* sL, const MelArgs& mel);
template <int N, int MODE>
__device__ __forceinline__ void mel_rows(const float2* v, int t, float* fa, float* fb, bool has_b, float* sink,
                                         float* P, const float* sW, const int* sCh, const int* sCb,
                                         const float* sD, const float* sL, const MelArgs& mel) {
    using G = Geo<N>;
    using Mi = Mirror<N>;
    constexpr int R = G::RL, J = G::NPT / 2, NB = G::NB, T = G::T, RW = N / 2 + 1;
    static_assert(T == 64, "one wave per transform");
    static_assert(2 * RW <= MEL_LM_OFF, "log-mel rows past the (interleaved) power rows");
    float ea[J][R], eb[J][R], sa[R], sb[R];
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int q = 2 * j * R + r;
            float2 A, B;
            pair_post<2>(v[q], mirror_of<N, true>(v, t, q), &A, &B);
            ea[j][r] = A.x;
            eb[j][r] = B.x;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int qm = Mi::normal(r);
        float2 A2, B2;
        pair_post<2>(v[qm], v[Mi::special(qm)], &A2, &B2);
        sa[r] = A2.x;
        sb[r] = B2.x;
    }
    // block m of 64 bins: an even block (lane t: bin 64 m + t) or the mirror
    // block of slot (jm, rm) (lane t: bin 64 m + (64 - t) % 64), as direct_rows.
    // The two rows go to P interleaved, P[2k] = |Xa[k]|^2, P[2k + 1] = |Xb[k]|^2:
    // one ds_write_b64 per bin here and one ds_read_b64 per bin in the chunk sums
    // below, the pair landing in one register pair for a packed FMA (two rows
    // RW floats apart took two b32 accesses and v_movs to re-pair them)
    auto put = [&](int bin, float va, float vb) { *reinterpret_cast<vf2_t*>(P + 2 * bin) = vf2_t{va, vb}; };
    static_for<0, N / T>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        if constexpr (T * m < N / 2) {
            constexpr int je = m % (NB / T), re = m / (NB / T);
            if constexpr (je < J) {
                put(T * m + t, ea[je][re], eb[je][re]);
            } else {
                constexpr int mm = (N / T - 1) - m, rm = mm / (NB / T), jm = mm % (NB / T);
                float va, vb;
                if constexpr (jm + 1 < J) {
                    va = t == 0 ? ea[jm + 1][rm] : ea[jm][rm];
                    vb = t == 0 ? eb[jm + 1][rm] : eb[jm][rm];
                } else {
                    va = t == 0 ? sa[rm] : ea[jm][rm];
                    vb = t == 0 ? sb[rm] : eb[jm][rm];
                }
                put(T * m + (t == 0 ? 0 : T - t), va, vb);
            }
        }
    });
    if (t == 0) {
        put(N / 2, ea[0][R / 2], eb[0][R / 2]);
        if constexpr (MelArgs::W2) {   // bins N/2 + 1 .. N/2 + 3: zeros under the last windows' tails
            put(N / 2 + 1, 0.0f, 0.0f);
            put(N / 2 + 2, 0.0f, 0.0f);
            put(N / 2 + 3, 0.0f, 0.0f);
        }
    }
    xsync<T>();
    mel_tail<MODE, true>(t, P, fa, fb, has_b, sink, sW, sCh, sCb, sD, sL, mel);
}

// The mel stage of one frame pair (MODE 3 log-mel, MODE 4 MFCC) over the 64
// lanes of a wave, from the pair's power rows in LDS interleaved bin by bin,
// P[2k] = |Xa[k]|^2, P[2k + 1] = |Xb[k]|^2 (k <= N/2): k_mel_grp's steps with
// FR = 2 frames -- chunk partials (FMA in bin order; lane c % 64 holds chunk c
// in round c / 64), per-filter sums of the partials in chunk order (fetched
// across lanes by ds_bpermute), logf(e + eps), and for MODE 4 the DCT-II and
// lifter over the log-mel rows (kept at P + MEL_LM_OFF) -- the same operations
// in the same order, so the rows equal the power rows followed by
// launch_mel_grp bit for bit.  Stores: MODE 3 rows a, b x filters t, t + 64
// (M <= 128), MODE 4 (frame, coefficient) pairs t, t + 64 (C <= 64).
template <int MODE, bool COUNTED>
__device__ __forceinline__ void mel_tail(int t, float* P, float* fa, float* fb, bool has_b, float* sink,
                                         const float* sW, const int* sCh, const int* sCb, const float* sD,
                                         const float* sL, const MelArgs& mel) {
    constexpr int T = 64;
    const int nc = mel.nc, M = mel.M, C = mel.C, lc = mel.lc, lcs = mel.lcs;
    float pa[MEL_MAX_ROUNDS], pb[MEL_MAX_ROUNDS];
    int dc[MEL_MAX_ROUNDS];   // the chunk a slot computes (windows: the host's bank-aware order)
#pragma unroll
    for (int u = 0; u < MEL_MAX_ROUNDS; ++u) {
        pa[u] = pb[u] = 0.0f;
        const int c = t + T * u;
        dc[u] = c;
        if (MODE == 3 || mel.cw == 0) {   // the chunk windows (log-mel; MFCC where the table fits three workgroups per CU)
            if (c >= nc) continue;
            // log-mel: the chunk's window of lc bins, the same lc for every lane (a
            // uniform loop: scalar trip count, immediate offsets); its zero weights
            // add exact zeros to the (row a, row b) partials, so the sums equal the
            // non-zero range's FMAs in bin order (3.053 -> 2.990 ms, 32 ch x 10 min).
            // Rows lcs = window_stride(lc) floats apart (16 B aligned, lcs / 4 odd: a
            // lane's four weights are one ds_read_b128 and the lanes' reads cover
            // distinct bank blocks; the host deals the chunks to lanes so that the
            // power reads' start banks collide least).  MFCC takes them where the windows' larger table
            // still leaves three workgroups per CU (with the register last-pass
            // twiddles, 6 KB less static LDS: the 40-mel / 13-coefficient plan);
            // otherwise the packed table (a workgroup per CU fewer: +17 %)
            const float* wr = sW + c * lcs;
            const int bits = __float_as_int(wr[lc]);   // window start | chunk << 16
            dc[u] = bits >> 16;
            const vf2_t* pp = reinterpret_cast<const vf2_t*>(P) + (bits & 0xffff);
            vf2_t ab = {0.0f, 0.0f};
            if constexpr (MelArgs::W2) {   // even starts: two bins' (row a, row b) pairs per 16 B read
                const vf4_t* p4 = reinterpret_cast<const vf4_t*>(pp);
                for (int j = 0; j < lc; j += 4) {
                    const vf4_t wq = *reinterpret_cast<const vf4_t*>(wr + j);
                    const vf4_t q0 = p4[j / 2], q1 = p4[j / 2 + 1];
                    ab = __builtin_elementwise_fma(vf2_t{q0[0], q0[1]}, vf2_t{wq[0], wq[0]}, ab);
                    ab = __builtin_elementwise_fma(vf2_t{q0[2], q0[3]}, vf2_t{wq[1], wq[1]}, ab);
                    ab = __builtin_elementwise_fma(vf2_t{q1[0], q1[1]}, vf2_t{wq[2], wq[2]}, ab);
                    ab = __builtin_elementwise_fma(vf2_t{q1[2], q1[3]}, vf2_t{wq[3], wq[3]}, ab);
                }
            } else {
                for (int j = 0; j < lc; j += 4) {
                    const vf4_t wq = *reinterpret_cast<const vf4_t*>(wr + j);   // rows 16 B aligned (lcs % 4 == 0)
#pragma unroll
                    for (int i = 0; i < 4; ++i) ab = __builtin_elementwise_fma(pp[j + i], vf2_t{wq[i], wq[i]}, ab);
                }
            }
            pa[u] = ab.x;
            pb[u] = ab.y;
        } else if (c < nc) {   // the packed layout, each chunk's own length
            const int lo = sCh[3 * c], len = sCh[3 * c + 1], off = sCh[3 * c + 2];
            vf2_t ab = {0.0f, 0.0f};   // (row a, row b) partials: fma per element, bin order
            const vf2_t* pp = reinterpret_cast<const vf2_t*>(P) + lo;
#pragma unroll 4
            for (int j = 0; j < len; ++j) {
                const float w = sW[off + j];
                ab = __builtin_elementwise_fma(pp[j], vf2_t{w, w}, ab);
            }
            pa[u] = ab.x;
            pb[u] = ab.y;
        }
    }
    // the chunk partials go to LDS over P (every lane has read its power bins
    // above), pair c at P[2c], P[2c + 1]; then lane m adds its filter's chunks
    // in chunk order -- independent ds_read_b64s instead of a chain of
    // cross-lane permutes (2 per round per chunk), the same sums bit for bit
    xsync<T>();
#pragma unroll
    for (int u = 0; u < MEL_MAX_ROUNDS; ++u) {
        const int c = t + T * u;
        if (c < nc) *reinterpret_cast<vf2_t*>(P + 2 * dc[u]) = vf2_t{pa[u], pb[u]};
    }
    xsync<T>();
    const vf2_t* part = reinterpret_cast<const vf2_t*>(P);
    float la[2] = {0.0f, 0.0f}, lb[2] = {0.0f, 0.0f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (T * u >= M) break;   // no filter in this round (M <= 64): skip its sums and logf
        const int m = t + T * u;
        const bool on = m < M;
        const int cb = on ? sCb[m] : 0, ce = on ? sCb[m + 1] : 0;
        float e0 = 0.0f, e1 = 0.0f;
#pragma unroll 4
        for (int c = cb; c < ce; ++c) {   // this lane's filter's chunks, in order
            const vf2_t q = part[c];
            e0 += q.x;
            e1 += q.y;
        }
        la[u] = on ? logf(e0 + mel.eps) : 0.0f;
        lb[u] = on ? logf(e1 + mel.eps) : 0.0f;
    }
    float* const snk = COUNTED ? sink + t : nullptr;
    // COUNTED: every lane issues each store (the sink when it has no element) so
    // k_stft_pair's hand-counted vmcnt stays exact; otherwise predicated stores
    auto put_out = [&](bool on, float* dst, float v) {
        if constexpr (COUNTED) st4_counted(on ? dst : snk, v);
        else if (on) *dst = v;
    };
    if constexpr (MODE == 3) {
        put_out(t < M, fa + t, la[0]);
        put_out(t + T < M, fa + t + T, la[1]);
        put_out(has_b && t < M, fb + t, lb[0]);
        put_out(has_b && t + T < M, fb + t + T, lb[1]);
    } else {
        float* const lm = P + MEL_LM_OFF;   // [2][M], M <= (ri_floats - MEL_LM_OFF) / 2
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = t + T * u;
            if (m < M) {
                lm[m] = la[u];
                lm[M + m] = lb[u];
            }
        }
        xsync<T>();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = t + T * u;
            float res = 0.0f;
            float* dst = snk;   // COUNTED: the sink; otherwise nullptr (no store)
            if (idx < 2 * C) {
                const int f = idx >= C ? 1 : 0, i = idx - f * C;
                const float* l = lm + f * M;
                const float* d = sD + i * M;
                float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
                int m = 0;
                if ((M & 3) == 0) {   // as k_mel_grp: four partial sums
#pragma unroll 5
                    for (; m < M; m += 4) {
                        const vf4_t a = *reinterpret_cast<const vf4_t*>(l + m);
                        const vf4_t b = *reinterpret_cast<const vf4_t*>(d + m);   // 16 B aligned: M % 4 == 0
                        c0 = __builtin_fmaf(a[0], b[0], c0);
                        c1 = __builtin_fmaf(a[1], b[1], c1);
                        c2 = __builtin_fmaf(a[2], b[2], c2);
                        c3 = __builtin_fmaf(a[3], b[3], c3);
                    }
                } else {
                    for (; m + 1 < M; m += 2) {
                        c0 = __builtin_fmaf(l[m], d[m], c0);
                        c1 = __builtin_fmaf(l[m + 1], d[m + 1], c1);
                    }
                    if (m < M) c0 = __builtin_fmaf(l[m], d[m], c0);
                }
                res = ((c0 + c1) + (c2 + c3)) * sL[i];
                if (f == 0) dst = fa + i;
                else if (has_b) dst = fb + i;
            }
            if constexpr (COUNTED) st4_counted(dst, res);
            else if (dst) *dst = res;
        }
    }
}

}  // namespace vvh
