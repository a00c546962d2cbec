// stft_pair.hpp -- k_stft_pair<N, MODE, VAR>: fused STFT analysis for the sizes
// whose last FFT pass is mirror-paired (Geo<N>::CAN_PAIR).
//
// TWO real frames a, b share one complex N-point FFT of z = w*a + i*w*b.  With
// the mirror-paired last pass each thread holds Z[k] and Z[N-k], so
// Xa[k] = (Z[k] + conj Z[N-k])/2 and Xb[k] = (Z[k] - conj Z[N-k])/2i
// come straight from registers -- no split twiddles, no LDS post pass -- and
// every bin 0..N-1 of both rows is produced in place (Hermitian symmetry is
// automatic).
//
// Scheduling: the bulk variant (VAR 0) is launched non-persistently, one
// workgroup per 16 consecutive frame pairs per transform slot, the slots of a
// workgroup interleaved, so the nfft-hop overlap of neighbouring frames is
// re-read from the same CU's L1/L2 and the dispatcher balances the CUs (no
// straggler tail).  VAR 1 (unaligned hops / channel strides) and VAR 2 (the
// zero-padded tail frames) are persistent and walk XCD-aware shares
// (xcd_walk).  VAR 0 streams each pair's input span (N + hop samples) into LDS
// with global_load_lds_dwordx4 one pair ahead and waits on hand-counted
// vmcnt.  For N = 1024 (one wave per transform) the magnitudes go straight
// from registers as full-line dword streaming stores and the FFT exchanges
// through a half-size real/imaginary buffer (3 workgroups per CU); other N
// stage the rows through LDS for 16-byte stores.  Window values are
// per-thread constants in registers; twiddles live in LDS.
//
// Modes 0..2 are launched from stft_pair.hip, modes 3 / 4 (N = 1024) from
// stft_mel.hip.
#pragma once
#include "stft_rows.hpp"

// N = 2048 magnitude rows (R2048): both last-pass butterflies' twiddles in
// registers (TwLastRegA, 166 VGPRs, three waves per SIMD as before) instead of
// TwLastRegP's mirror half read from LDS: -1.5 %, bit-identical
// (profiles/r06_ab_twregs_mfcc_windows.jsonl); 0 restores TwLastRegP (A/B)
#ifndef VVH_R2048_RA
#define VVH_R2048_RA 1
#endif

namespace vvh {

// Frame pairs (2j, 2j+1) of one channel, j in [pair0, pair0 + ppc): pairs never
// span channels, so a channel's rows do not depend on how channels are grouped
// into calls or shards.
//   VAR 0: bulk (both frames inside the signal), input spans by LDS-DMA,
//          magnitude rows as full-line streaming stores (16 B aligned rows)
//   VAR 1: bulk, stores straight from registers
//   VAR 2: tail -- the last few pairs, zero-padded past the end / odd last frame
// N = 1024 bulk: 3 waves per SIMD (<= 168 VGPRs) -- the LDS budget allows 3 workgroups per CU
template <int N, int MODE, int VAR>
__global__ void __launch_bounds__(Wg<N>::value, ((N == 1024 && (VAR == 0 || VAR == 3 || VAR == 4 || VAR == 5)) ||
                                                 (N == 2048 && MODE == 0 && VAR == 0))
                                                    ? 3
                                                    : 1)
k_stft_pair(const float* sig, long long n, long long nch, long long ch_stride, long long frames,
            long long hop, long long pair0, long long ppc, const float* win, void* out,
            long long out_ch_stride, long long row_pitch, const float2* gpass, const float2* gtab, long long chunk,
            float* sink, unsigned* ctrs, MelArgs mel) {
    using G = Geo<N>;
    using Mi = Mirror<N>;
    // MODE 3 / 4: log-mel / MFCC rows from the power rows, which stay in LDS
    // (launch_stft_mel; the tables of the MFCC plan in dynamic LDS)
    constexpr bool MEL = MODE == 3 || MODE == 4;
    constexpr bool TAIL = VAR == 2;
    constexpr bool BULK = VAR == 0 || VAR == 3 || VAR == 4 || VAR == 5;
    // VAR 3: VAR 0 with each wave walking a contiguous run of pairs and its
    // span kept as a ring of 256-float chunks (hop % 256 == 0): a pair DMAs only
    // its 2*hop new samples instead of the whole N + hop span
    // VAR 5: the dynamic walk below handing out runs of `rl` consecutive pairs
    // per counter value, each run walked with VAR 3's ring
    constexpr bool DRING = VAR == 5;
    constexpr bool RING = VAR == 3 || DRING;
    // VAR 4 / 5: the dynamic band walk -- each wave takes its next pair (run) from
    // a counter of its (XCD group, slot) stream, so the chip works on one moving
    // band and neighbouring pairs share an L2 while waves balance dynamically;
    // a persistent grid, counters from stream_counters().  The counter atomics
    // are hand-counted VMEM ops like the spans and stores.
    constexpr bool DYN = VAR == 4 || DRING;
    constexpr bool STAGE = BULK && MODE == 0 && G::NPASS > 1 && G::T > 1;
    // power rows (N = 1024): the DIRECT stores below, keeping only the
    // 64-bin blocks under N/2 plus one lane for bin N/2
    constexpr bool POWD = BULK && (MODE == 2 || MEL) && G::T == 64 && G::NPASS > 1;
    static_assert(!MEL || POWD, "log-mel / MFCC rows: the one-wave-per-transform bulk kernel (N = 1024)");
    // complex rows (N = 1024): DIRECT with 8 B/lane stores, conj() for the mirror blocks
    constexpr bool CPXD = BULK && MODE == 1 && G::T == 64 && G::NPASS > 1;
    constexpr bool GLDS = (STAGE || POWD || CPXD) && G::T >= 64;   // input spans by LDS-DMA (launcher checks hop/alignment)
    // floats per transform: hop <= N/2 (MEL: hop <= 256)
    // (MEL: hop <= 256; the ring walks VAR 3 / VAR 5: hop == 256 -- so N + 256
    // floats per span; for the ring walks that makes 40.8 KB of LDS per workgroup
    // with the register last-pass twiddles: four per CU, -2.5 % for power rows,
    // -2..-3 % for the headline's magnitude rows)
    constexpr int SPAN = GLDS ? ((MEL || VAR == 3 || VAR == 5) ? N + 256 : N + N / 2) : 1;
    // T == 64 (one wave per transform): magnitudes go straight from registers as
    // full-line dword stores (DIRECT); otherwise they are staged through LDS and
    // written as 16 B/lane stores
    constexpr bool DIRECT = GLDS && G::T == 64;
    static_assert(!RING || DIRECT, "ring spans: one wave per transform on the LDS-DMA path");
    // stores per pair (both rows): power rows keep half the blocks + bin N/2
    constexpr int NST = MEL ? (MODE == 3 ? 4 : 2)
                            : DIRECT ? (MODE == 2 ? G::P + 2 : 2 * G::P)
                                                                  : 2 * (G::P / 4);
    constexpr int WG = Wg<N>::value, F = Wg<N>::F, R = G::RL;
    // N = 2048 magnitude rows (two waves per transform, LDS-DMA spans, rows
    // staged for 16 B stores): the same half-size exchange, the last pass'
    // twiddles of each thread's first butterfly held in registers (TwLastRegP:
    // 1136 table entries in LDS instead of 2032) and the two rows staged one
    // after the other through the half-size buffer -- 51 KB of LDS per
    // workgroup instead of 75.6 KB, so 3 workgroups (3 waves per SIMD) fit per
    // CU instead of 2
    constexpr bool R2048 = N == 2048 && STAGE && GLDS;
    // DIRECT needs no staging buffer: the exchange goes through a half-size
    // (real, then imaginary) buffer, so 3 workgroups fit per CU instead of 2
    constexpr bool RI = DIRECT || R2048;
    constexpr int XF = RI ? (ri_floats<N>() + 3) / 4 * 2 : G::LDS;   // float2 per transform (16 B multiple)
    constexpr int LDSN = G::NPASS > 1 ? F * XF : 1;
    __shared__ __attribute__((aligned(16))) float2 lds[LDSN];   // 16 B: pass_exchange_ri's b128 writes
    // N = 1024 one-wave transforms (DIRECT): every last-pass twiddle of a
    // thread in registers (TwLastRegA: 24 VGPRs), only the first two passes'
    // 240 entries in LDS -- 6 KB less LDS per workgroup, 12 fewer LDS reads per
    // pair, the table's own values (bit-identical)
    // (Not for magnitude rows' VAR 0, the launch of small jobs: config 3's single
    // 60 s call measured +2 % with the per-workgroup twiddle loads.)
    constexpr bool RA = (DIRECT && N == 1024 && !(MODE == 0 && VAR == 0)) || (R2048 && VVH_R2048_RA);
    constexpr int TWE = RA       ? G::tw_off(G::NPASS - 1)
                        : R2048 ? G::tw_off(G::NPASS - 1) + (G::RL - 1) * (G::ns(G::NPASS - 1) / 2)   // TwLastRegP's
                                : TwLayout<N>::ENTRIES;
    __shared__ float2 ltab[TWE];
    __shared__ float span_all[GLDS ? F * SPAN : 1];
    const TwTab<N> tw{ltab};
    using TwL = std::conditional_t<RA, TwLastRegA<N, true>, std::conditional_t<R2048, TwLastRegP<N>, TwTab<N>>>;
    TwL twl{};
    if constexpr (RA) {
        twl.tab = ltab;
        twl.load(gpass, (int)threadIdx.x % Geo<N>::T);
    } else if constexpr (R2048) {
        twl.tab = ltab;
        twl.hi = ltab + Geo<N>::tw_off(Geo<N>::NPASS - 1);
        twl.load(gpass, (int)threadIdx.x % Geo<N>::T);
    }
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T;
    float2* my = lds + (G::NPASS > 1 ? slot * XF : 0);
    // window values 0.5 w[t + r T], packed two per VGPR pair (pk_mul_bcast)
    vf2_t wp[(G::P + 1) / 2];
#pragma unroll
    for (int r = 0; r < G::P; ++r) {
        const float wr = 0.5f * win[t + r * G::T];
        if (r & 1) wp[r / 2].y = wr;
        else wp[r / 2] = vf2_t{wr, 0.0f};
    }

    int kb[G::NPT];   // last-pass butterfly of each slot (loop invariant)
#pragma unroll
    for (int i = 0; i < G::NPT; ++i) kb[i] = bfly<N, G::NPASS - 1, true>(t, i);
    constexpr long long ES = MODE == 1 ? 8 : 4;            // bytes per bin
    constexpr long long ROW = MODE == 2 ? N / 2 + 1 : N;   // bins per row
    // floats (MODE 1: complex values) from one row's start to the next: power rows
    // may sit `row_pitch` floats apart (>= N/2 + 1, e.g. 544 = 17 whole lines)
    const long long ROWR = MODE == 3 ? (long long)mel.M : MODE == 4 ? (long long)mel.C : MODE == 2 ? row_pitch : ROW;
    // MEL: the plan's tables in dynamic LDS: W [nnz], chunks [3 nc], cbeg [M + 1], then (MODE 4) D [C M], lift [C]
    extern __shared__ __attribute__((aligned(16))) float mel_lds[];
    const int mel_dpos = MEL ? (mel.nnz + mel.cw * mel.nc + mel.M + 1 + 3) & ~3 : 0;
    // rows of one pair from the registers, plain stores (unaligned / tail pairs)
    auto store_generic = [&](float2* v, char* rowa, char* rowb, bool has_b) {
        if constexpr (G::T == 1) {
#pragma unroll
            for (int q = 0; q < G::P; ++q) {
                float2 A, B;
                pair_post<MODE>(v[q], mirror_of<N, true>(v, t, q), &A, &B);
                put_bin<MODE, N>(rowa, q, A);
                if (has_b) put_bin<MODE, N>(rowb, q, B);
            }
        } else {
            // even slots hold bins k, their partner slots hold N-k: one post
            // per (k, N-k) pair, stored at both (real input -> mirror = conj)
#pragma unroll
            for (int i = 0; i < G::NPT; i += 2) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int q = i * R + r, qm = Mi::normal(q);
                    float2 A, B;
                    pair_post<MODE>(v[q], mirror_of<N, true>(v, t, q), &A, &B);
                    float2 Am = MODE == 0 ? A : cconj(A), Bm = MODE == 0 ? B : cconj(B);
                    if (i == 0) {   // thread 0: slot 1 is butterfly NB/2, its own mirror
                        float2 A2, B2;
                        pair_post<MODE>(v[qm], v[Mi::special(qm)], &A2, &B2);
                        Am = select2(t == 0, A2, Am);
                        Bm = select2(t == 0, B2, Bm);
                    }
                    const int k = kb[i] + r * G::NB, km = kb[i + 1] + (R - 1 - r) * G::NB;
                    put_bin<MODE, N>(rowa, k, A);
                    put_bin<MODE, N>(rowa, km, Am);
                    if (has_b) {
                        put_bin<MODE, N>(rowb, k, B);
                        put_bin<MODE, N>(rowb, km, Bm);
                    }
                }
            }
        }
    };
    const long long pairs = nch * ppc;
    long long p, p_end, p_step;
    // RING: block b owns items [b*chunk, (b+1)*chunk) (chunk = the low 40 bits),
    // cut into groups of F runs of `rl` consecutive pairs (rl = the high bits);
    // slot s walks run s of every group
    const long long rl = RING ? (chunk >> 40) : 1;
    long long kk = 0;   // items this slot has done
    if constexpr (RING && !DRING) {
        const long long ch = chunk & ((1LL << 40) - 1);
        p = (long long)blockIdx.x * ch + slot * rl;
        p_end = (long long)(blockIdx.x + 1) * ch < pairs ? (long long)(blockIdx.x + 1) * ch : pairs;
        p_step = 1;
    } else if constexpr (DYN) {
        p = 0;   // set below from the XCD's counter
        p_end = pairs;
        p_step = 1;
    } else {
        work_walk(pairs, F, slot, chunk, &p, &p_end, &p_step);
    }
    p = uni<G::T>(p);
    p_end = uni<G::T>(p_end);
    p_step = uni<G::T>(p_step);
    // one counter per (XCD, slot): 32 streams, so no address takes more than one
    // atomic per workgroup of its XCD per pair
    const int stream = __builtin_amdgcn_readfirstlane((int)(blockIdx.x & 7) * F + slot);
    unsigned* const ctr = DYN ? ctrs + 32 * stream : nullptr;
    // DB = 2^dbs consecutive items per stream and band (VAR 5: log2 in chunk's low bits)
    const int dbs = DRING ? (int)(chunk & 15) : 6;
    // Each XCD group walks its own contiguous eighth of the runs (its F slot
    // streams banded inside it) -- the write probe's best layout (scripts/
    // membench.hip k_wprobe BAND 1: 0.896 of peak for pure writes against 0.840
    // for 2 MB chunks dealt round robin); a stream past its eighth is done.
    // 3.2967 -> 3.2556 ms for the config-5 shard, same buffers, bit-identical
    // (profiles/r04_kbench_xcd_eighths.jsonl).
    const long long nrun = DYN ? (pairs + rl - 1) / rl : 0, r8 = (nrun + 7) / 8;
    auto band_pair = [&](unsigned k) -> long long {
        const long long DB = 1LL << dbs;
        const long long g = stream / F, sl = stream % F;   // wave-uniform (stream is readfirstlane'd)
        const long long it = g * r8 + (long long)(k >> dbs) * (F * DB) + sl * DB + (long long)(k & (DB - 1));
        const long long ge = (g + 1) * r8 < nrun ? (g + 1) * r8 : nrun;
        return it < ge ? it : pairs;
    };
    unsigned rr = 0;   // lane 0: an issued counter atomic's result (valid after a vmcnt wait)
    auto grab = [&]() {
        if (t == 0) asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(rr) : "v"(ctr), "v"(1u) : "memory");
    };
    long long pn = 0;   // DYN: the pair after p
    if constexpr (DYN) {
        unsigned r0 = 0;
        if (t == 0)
            asm volatile("global_atomic_add %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=v"(r0) : "v"(ctr), "v"(1u) : "memory");
        if constexpr (DRING) {   // counter value k -> the run of pairs [rl b(k), rl b(k) + rl)
            p = rl * band_pair(__builtin_amdgcn_readfirstlane(r0));
        } else {
            grab();
            unsigned k1;
            asm volatile("s_waitcnt vmcnt(0)\n\tv_readfirstlane_b32 %0, %1" : "=s"(k1) : "v"(rr) : "memory");
            p = band_pair(__builtin_amdgcn_readfirstlane(r0));
            pn = band_pair(k1);
        }
    }
    const bool any = p < p_end;   // uniform per transform
    // (channel, first frame) of a pair; this launch covers frames
    // [2*pair0, 2*(pair0 + ppc)) of every channel
    auto locate = [&](long long q, long long* cc, long long* ff) {
        *cc = q / ppc;
        *ff = 2 * (pair0 + q - *cc * ppc);
    };
    long long c = 0, fa = 0;
    if (any) locate(p, &c, &fa);
    float xa[G::P], xb[G::P];
    // GLDS: the pair's span [fa*hop, fa*hop + hop + N) goes HBM/L2 -> LDS by
    // 16 B/lane LDS-DMA, issued right after the previous span was read, so it
    // lands while that pair is transformed -- no VGPRs held across iterations.
    float* span = span_all + (GLDS ? slot * SPAN : 0);
    // Pairs that reach past the end of the signal (the zero-padded tail, at
    // most a few per channel) fill the span with ordinary bounds-checked loads
    // and LDS stores instead: the compiler waits on those itself, and being
    // younger than every hand-counted operation they keep the counts valid.
    auto issue_span = [&](long long cc, long long ff) {
        const float* s0 = sig + cc * ch_stride + ff * hop;
        const int len = (int)(N + hop), lane = t & 63;
        if (ff * hop + len <= n) {
            for (int u = t >> 6; u * 256 < len; u += G::T / 64) {
                const int e = u * 256 + lane * 4;
                glds16(s0 + (e < len ? e : 0), span + u * 256);
            }
        } else {
            const long long left = n - ff * hop;   // samples of this span inside the signal
            for (int u = t >> 6; u * 256 < len; u += G::T / 64) {
                const int e = u * 256 + lane * 4;
                vf4_t q;
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = e + k < left ? s0[e + k] : 0.0f;
                *reinterpret_cast<vf4_t*>(span + u * 256 + lane * 4) = q;
            }
        }
    };
    // ring (VAR 3): chunk k of the current pair's span [fa*hop, fa*hop + N + hop)
    // sits in ring slot (rs + k) mod rc; the next pair of the same channel
    // reuses chunks h2.. and DMAs its last h2 into the slots of chunks 0..h2-1,
    // which this pair has read (into registers) before the DMA is issued
    const int rc = RING ? (int)((N + hop) >> 8) : 1, h2 = RING ? (int)((2 * hop) >> 8) : 0,
              hb = RING ? (int)(hop >> 8) : 0;
    int rs = 0, rsn = 0;
    auto issue_new = [&](long long cc, long long ff) {
        const float* s0 = sig + cc * ch_stride + ff * hop;
        rsn = rs + h2 >= rc ? rs + h2 - rc : rs + h2;
        for (int k = rc - h2; k < rc; ++k) {
            const int sl = rsn + k >= rc ? rsn + k - rc : rsn + k;
            glds16(s0 + k * 256 + (t & 63) * 4, span + sl * 256);
        }
    };
    auto load_pair = [&](long long cc, long long ff) {
        if constexpr (RING) rsn = 0;   // whole span, chunk k in slot k
        if constexpr (GLDS) {
            issue_span(cc, ff);
        } else if constexpr (TAIL) {
            const float* s = sig + cc * ch_stride;
            frame_load<N>(xa, s, ff * hop, n, t, true);
            frame_load<N>(xb, s, (ff + 1 < frames ? ff + 1 : ff) * hop, n, t, ff + 1 < frames);
        } else {   // both frames lie inside the signal: wave-uniform bases, plain loads
            const float* sa = sig + cc * ch_stride + ff * hop;
            const float* sb = sa + hop;
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                xa[r] = sa[t + r * G::T];
                xb[r] = sb[t + r * G::T];
            }
        }
    };
    // the first span's DMA is in flight while the block stages its twiddles
    if (any) load_pair(c, fa);
    if constexpr (DYN) {
        if constexpr (DRING) {
            if (any) grab();   // -> the next run
        } else {
            if (any && pn < pairs) grab();   // -> the pair after pn
        }
    }
    if constexpr (RA) {   // the passes before the last
        TwLastRegA<N, true>::template stage<WG>(ltab, gpass);
    } else if constexpr (R2048) {   // the passes before the last, and the last pass' upper half
        TwLastRegP<N>::template stage<WG>(ltab, ltab + Geo<N>::tw_off(Geo<N>::NPASS - 1), gpass);
    } else {
        stage_twiddles<N, WG>(ltab, gpass, gtab);
    }
    if constexpr (MEL) {
        int* const mi = reinterpret_cast<int*>(mel_lds);
        for (int i = threadIdx.x; i < mel.nnz; i += WG) mel_lds[i] = mel.W[i];
        for (int i = threadIdx.x; i < mel.cw * mel.nc; i += WG) mi[mel.nnz + i] = mel.chunks[i];
        for (int i = threadIdx.x; i <= mel.M; i += WG) mi[mel.nnz + mel.cw * mel.nc + i] = mel.cbeg[i];
        if constexpr (MODE == 4) {
            for (int i = threadIdx.x; i < mel.C * mel.M; i += WG) mel_lds[mel_dpos + i] = mel.D[i];
            for (int i = threadIdx.x; i < mel.C; i += WG) mel_lds[mel_dpos + mel.C * mel.M + i] = mel.lift[i];
        }
    }
    __syncthreads();
    if (!any && !DYN) return;
    if constexpr (GLDS) vm_wait<0>();
    if constexpr (RING) rs = rsn;
    for (; p < p_end; p += p_step) {
        if constexpr (DRING) {
            // the last grabbed run: its atomic is older than the previous pair's
            // NST stores (issued with the DMA of its run's first pair)
            unsigned kq;
            asm volatile("s_waitcnt vmcnt(%1)\n\tv_readfirstlane_b32 %0, %2" : "=s"(kq) : "n"(NST), "v"(rr) : "memory");
            const long long pq = p + 1 >= pairs ? pairs : kk + 1 < rl ? p + 1 : rl * band_pair(kq);
            p_step = uni<G::T>(pq - p);
        } else if constexpr (RING) {
            p_step = ((kk + 1) % rl) ? 1 : (long long)F * rl - rl + 1;
        }
        if constexpr (DYN && !DRING) p_step = pn - p;
        const bool more = p + p_step < p_end;
        long long cn = c, fn = fa;
        if constexpr (RING) {   // within a run: the next pair, or frame 2*pair0 of the next channel
            if (p_step == 1) {
                fn = fa + 2;
                if (fn >= 2 * (pair0 + ppc)) {
                    cn = c + 1;
                    fn = 2 * pair0;
                }
            } else if (more) {
                locate(p + p_step, &cn, &fn);
            }
        } else {
            if (more) locate(p + p_step, &cn, &fn);
        }
        if constexpr (RING) {
            if constexpr (!DRING) vm_wait<NST>();
            // chunk slots of frame a (chunks 0..3) and frame b (chunks hb..hb+3)
            int ca[4], cbk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int a = rs + k, b = rs + k + hb;
                ca[k] = __builtin_amdgcn_readfirstlane(a >= rc ? a - rc : a) * 256;
                cbk[k] = __builtin_amdgcn_readfirstlane(b >= rc ? b - rc : b) * 256;
            }
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                xa[r] = span[ca[r / 4] + t + 64 * (r % 4)];
                xb[r] = span[cbk[r / 4] + t + 64 * (r % 4)];
            }
            lgkm_wait0();   // span read before it is refilled
            if (more) {
                if (p_step == 1 && cn == c && fn * hop + (N + hop) <= n) issue_new(cn, fn);
                else load_pair(cn, fn);
                if constexpr (DRING) {
                    if (kk + 1 == rl) grab();   // the next pair starts a run: fetch the one after it
                }
            }
        } else if constexpr (DYN) {
            // this span's DMA and the counter atomic issued after it are older
            // than the previous pair's NST stores
            unsigned knn;
            asm volatile("s_waitcnt vmcnt(%1)\n\tv_readfirstlane_b32 %0, %2" : "=s"(knn) : "n"(NST), "v"(rr) : "memory");
            const long long pnn = more ? band_pair(knn) : pairs;
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                xa[r] = span[t + r * G::T];
                xb[r] = span[hop + t + r * G::T];
            }
            lgkm_wait0();   // span read before it is refilled
            if (more) {
                load_pair(cn, fn);
                if (pnn < pairs) grab();
            }
            pn = pnn;
        } else if constexpr (GLDS) {
            // younger than this span's DMA: only the previous pair's NST stores
            vm_wait<NST>();
            if constexpr (G::T > 64) lds_barrier();   // the other waves' pieces
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                xa[r] = span[t + r * G::T];
                xb[r] = span[hop + t + r * G::T];
            }
            lgkm_wait0();   // span read before it is refilled
            if constexpr (G::T > 64) lds_barrier();
            if (more) load_pair(cn, fn);
        }
        float2 v[G::P];
        if constexpr (BULK && G::T == 64) {
            // the span reads come in pairs (r, r + 1) of one frame (ds_read2st64: adjacent
            // registers); one v_pk_mov_b32 per (frame a, frame b) register pair instead of
            // two v_mov_b32.  With the exchange reads as single ds_read_b32 (RIV 1) the
            // loop's v_movs drop from 87 to 27 (power rows; VALU 419 -> 370 per pair),
            // bit-identical, 2.766 -> 2.741 ms power / 3.410 -> 3.399 ms magnitude
            // (profiles/r04_kbench_stft_movefree.jsonl).
#pragma unroll
            for (int i = 0; i < G::P / 2; ++i) {
                const vf2_t A = {xa[2 * i], xa[2 * i + 1]}, B = {xb[2 * i], xb[2 * i + 1]};
                v[2 * i] = upk(pk_mul_bcast<0>(pk_pair<0>(A, B), wp[i]));
                v[2 * i + 1] = upk(pk_mul_bcast<1>(pk_pair<1>(A, B), wp[i]));
            }
        } else {
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                const vf2_t x = {xa[r], xb[r]};
                v[r] = upk((r & 1) ? pk_mul_bcast<1>(x, wp[r / 2]) : pk_mul_bcast<0>(x, wp[r / 2]));
            }
        }
        if constexpr (GLDS) {
        } else if constexpr (TAIL) {
            if (more) load_pair(cn, fn);
        } else {
            load_pair(more ? cn : c, more ? fn : fa);   // last step re-reads its own pair
        }
        if constexpr (R2048 || RA) {
            twl.opaque();
            fft_regs<N, true, true, RI, TwL, false, false, 1>(v, t, my, twl);
        } else {
            fft_regs<N, true, true, RI, TwTab<N>, false, false, 1>(v, t, my, tw);
        }
        char* rowa = reinterpret_cast<char*>(out) + (c * out_ch_stride + fa * ROWR) * ES;
        char* rowb = rowa + ROWR * ES;
        const bool has_b = (TAIL || GLDS) ? fa + 1 < frames : true;
        if constexpr (MEL) {
            const int* mi = reinterpret_cast<const int*>(mel_lds);
            mel_rows<N, MODE>(v, t, reinterpret_cast<float*>(rowa), reinterpret_cast<float*>(rowb), has_b, sink,
                              reinterpret_cast<float*>(my), mel_lds, mi + mel.nnz, mi + mel.nnz + mel.cw * mel.nc,
                              mel_lds + mel_dpos, mel_lds + mel_dpos + mel.C * mel.M, mel);
        } else if constexpr (DIRECT) {
            direct_rows<N, MODE>(v, t, rowa, rowb, has_b, sink);
        } else if constexpr (R2048) {
            // row a, then row b, through the (now idle) half-size exchange buffer
            // (N floats each), each as full-line 16 B/lane streaming stores
            float* sf = reinterpret_cast<float*>(my);
            float bq[G::P];   // row b's magnitudes, staged after row a's stores
#pragma unroll
            for (int i = 0; i < G::NPT; i += 2) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int q = i * R + r, qm = Mi::normal(q);
                    float2 A, B;
                    pair_post<0>(v[q], mirror_of<N, true>(v, t, q), &A, &B);
                    float am = A.x, bm = B.x;
                    if (i == 0) {
                        float2 A2, B2;
                        pair_post<0>(v[qm], v[Mi::special(qm)], &A2, &B2);
                        am = t == 0 ? A2.x : am;
                        bm = t == 0 ? B2.x : bm;
                    }
                    const int k = kb[i] + r * G::NB, km = kb[i + 1] + (R - 1 - r) * G::NB;
                    sf[k] = A.x;
                    sf[km] = am;
                    bq[2 * (i / 2 * R + r)] = B.x;
                    bq[2 * (i / 2 * R + r) + 1] = bm;
                }
            }
            char* rb = has_b ? rowb : reinterpret_cast<char*>(sink);
            xsync<G::T>();
#pragma unroll
            for (int j = 0; j < G::P / 4; ++j) {   // N / (4 T) = P / 4 stores per row
                const int e = 4 * (t + G::T * j);
                st16_nt_counted(reinterpret_cast<vf4_t*>(rowa) + (t + G::T * j),
                                *reinterpret_cast<const vf4_t*>(sf + e));
            }
            xsync<G::T>();
#pragma unroll
            for (int i = 0; i < G::NPT; i += 2) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int k = kb[i] + r * G::NB, km = kb[i + 1] + (R - 1 - r) * G::NB;
                    sf[k] = bq[2 * (i / 2 * R + r)];
                    sf[km] = bq[2 * (i / 2 * R + r) + 1];
                }
            }
            xsync<G::T>();
#pragma unroll
            for (int j = 0; j < G::P / 4; ++j) {
                const int e = 4 * (t + G::T * j);
                st16_nt_counted(reinterpret_cast<vf4_t*>(rb) + (t + G::T * j), *reinterpret_cast<const vf4_t*>(sf + e));
            }
            xsync<G::T>();   // the next transform's first exchange reuses `my`
        } else if constexpr (STAGE) {
            // both magnitude rows through the (now idle) exchange buffer, then
            // full-line 16 B/lane streaming stores: 2N/(4T) instead of 2P per lane
            float* sf = reinterpret_cast<float*>(my);
#pragma unroll
            for (int i = 0; i < G::NPT; i += 2) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int q = i * R + r, qm = Mi::normal(q);
                    float2 A, B;
                    pair_post<0>(v[q], mirror_of<N, true>(v, t, q), &A, &B);
                    float am = A.x, bm = B.x;
                    if (i == 0) {
                        float2 A2, B2;
                        pair_post<0>(v[qm], v[Mi::special(qm)], &A2, &B2);
                        am = t == 0 ? A2.x : am;
                        bm = t == 0 ? B2.x : bm;
                    }
                    const int k = kb[i] + r * G::NB, km = kb[i + 1] + (R - 1 - r) * G::NB;
                    sf[k] = A.x;
                    sf[km] = am;
                    sf[N + k] = B.x;
                    sf[N + km] = bm;
                }
            }
            xsync<G::T>();
#pragma unroll
            for (int j = 0; j < G::P / 4; ++j) {
                const int e = 4 * (t + G::T * j);
                const vf4_t a = *reinterpret_cast<const vf4_t*>(sf + e);
                const vf4_t b = *reinterpret_cast<const vf4_t*>(sf + N + e);
                if constexpr (GLDS) {   // counted by the vm_wait<NST> above: exactly NST per pair
                    char* rb = has_b ? rowb : reinterpret_cast<char*>(sink);
                    st16_nt_counted(reinterpret_cast<vf4_t*>(rowa) + (t + G::T * j), a);
                    st16_nt_counted(reinterpret_cast<vf4_t*>(rb) + (t + G::T * j), b);
                } else {
                    __builtin_nontemporal_store(a, reinterpret_cast<vf4_t*>(rowa) + (t + G::T * j));
                    __builtin_nontemporal_store(b, reinterpret_cast<vf4_t*>(rowb) + (t + G::T * j));
                }
            }
            xsync<G::T>();   // the next transform's first exchange reuses `my`
        } else {
            store_generic(v, rowa, rowb, has_b);
        }
        c = cn;
        fa = fn;
        if constexpr (RING) {
            rs = rsn;
            if constexpr (DRING) kk = kk + 1 == rl ? 0 : kk + 1;
            else ++kk;
        }
    }
    if constexpr (DYN) {   // the XCD's last wave out resets its counters for the next launch
        vm_wait<0>();
        if (t == 0) {
            const unsigned nw = (unsigned)((gridDim.x - (blockIdx.x & 7) + 7) / 8);
            if (atomicAdd(ctr + 16, 1u) == nw - 1) {
                atomicExch(ctr, 0u);
                atomicExch(ctr + 16, 0u);
            }
        }
    }
}

}  // namespace vvh
