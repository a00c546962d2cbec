// stft_r32.hpp -- k_stft_r32<MODE>: nfft 1024 / hop 256 rows with the transform
// split 32 x 32 on half-waves (launch_r32 in stft_launch.hpp).  Mode 0 is
// launched from stft_pair.hip, modes 2..4 from stft_mel.hip.
#pragma once
#include "stft_rows.hpp"

namespace vvh {

// ------------------------------------------------------------------------
// k_stft_r32<MODE>: power rows (MODE 2) of nfft = 1024, hop = 256 frames with
// the transform split 32 x 32 on half-waves, as k_fir_r32: two frames per
// complex FFT (z = w/2 (a + i b)), two frame pairs per wave (one per half),
// ONE padded LDS transpose per FFT instead of k_stft_pair's two exchanges.
//   lane m2 (residue 2 (m & 15) + (m >> 4), the PAIRED layout): the pair's
//   1280-sample span as 20 dwordx2 loads re-laid by v_permlane16_swap -- frame
//   a = span rows 0..31, frame b = span rows 8..39 (hop = 8 rows) -- times the
//   window, DFT_32 over m1, twiddle W_1024^(m2 k1), transpose, DFT_32 over m2
//   -> Z[m + 32 k2] in register k2 of lane m.
// The mirror bins Z[N - k] (lane 32 - m, register 31 - k2; lane 0: register
// 32 - k2) come back through the same LDS buffer (16 writes, 16 reads), then
// pair_post<2> gives |Xa[k]|^2, |Xb[k]|^2 for bins 0..512 and each half stores
// its pair's two rows, 128 B per instruction.  Spans that reach past the end
// of the signal (the zero-padded tail) are staged through LDS with the zero
// rule, in the same loop.  Persistent grid, static XCD walk over frame-pair
// couples.
// ------------------------------------------------------------------------
// MODE 3 / 4 (log-mel / MFCC rows, launch_stft_mel): the power rows of each
// half's pair go to that half's (now idle) transpose buffer, interleaved bin by
// bin, and the wave runs mel_tail over its two pairs in turn -- the rows equal
// MODE 2's power rows followed by launch_mel_grp, bit for bit.  The plan's
// tables ride in dynamic LDS, so these modes take 8 transform slots per
// workgroup (512 threads, one workgroup and two waves per SIMD per CU) instead of
// two workgroups of 4: the same occupancy with one copy of the tables.
// 33 rows: the mirror read of lane 0 touches row 32; + 1 keeps every buffer 16 B
// aligned (the mel tail's 16 B reads of the power pairs in it)
constexpr int R33_BUF = 33 * R32_ROW + 1;
template <int MODE>
__global__ void __launch_bounds__(MODE >= 3 ? 512 : 256, MODE >= 3 ? 1 : 2)
k_stft_r32(const float* sig, long long n, long long nch, long long ch_stride, long long frames, const float* win,
           float* out, long long out_ch_stride, long long row_pitch, const float2* tw1024, MelArgs mel) {
    static_assert(MODE == 0 || MODE >= 2, "magnitude, power, log-mel or MFCC rows");
    constexpr bool MEL = MODE >= 3;
    constexpr int N = 1024, HOP = 256, F = MEL ? 8 : 4, WG = 64 * F, RW = MODE == 0 ? N : N / 2 + 1, SPAN = N + HOP;
    // floats from one output row's start to the next
    const long long RP = MODE == 2 ? row_pitch : MODE == 3 ? (long long)mel.M : MODE == 4 ? (long long)mel.C : RW;
    __shared__ __attribute__((aligned(16))) float2 xch[F * 2 * R33_BUF];
    __shared__ float2 ltw[32 * 32];   // [r][m] = W_1024^(m r)
    for (int i = threadIdx.x; i < 32 * 32; i += WG) ltw[i] = tw1024[((i & 31) * (i >> 5)) & (N - 1)];
    // MEL: the plan's tables in dynamic LDS: W [nnz], chunks [3 nc], cbeg [M + 1], then (MODE 4) D [C M], lift [C]
    extern __shared__ __attribute__((aligned(16))) float mel_lds[];
    const int mel_dpos = MEL ? (mel.nnz + mel.cw * mel.nc + mel.M + 1 + 3) & ~3 : 0;
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
    const int lt = threadIdx.x, slot = lt >> 6, lane = lt & 63, half = lane >> 5, m = lane & 31;
    const int mr = 2 * (m & 15) + (m >> 4);   // this lane's input residue
    float2* buf = xch + (2 * slot + half) * R33_BUF;
    // 0.5 w[32 r + mr], two rows per register pair (the 1/2 of the two-frame split rides in the window)
    vf2_t wp[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) wp[i] = vf2_t{0.5f * win[64 * i + mr], 0.5f * win[64 * i + 32 + mr]};
    __syncthreads();
    const long long ppc = (frames + 1) / 2, pairs = nch * ppc, couples = (pairs + 1) / 2;
    long long it, it_end, it_step;
    xcd_walk(couples, F, slot, &it, &it_end, &it_step);
    it = uni<64>(it);
    it_end = uni<64>(it_end);
    it_step = uni<64>(it_step);
    if (it >= it_end) return;
    // pair 2k = (channel c0, pair q0 of it), advanced incrementally (one division per wave)
    long long c0 = (2 * it) / ppc, q0 = 2 * it - c0 * ppc;
    const long long dc = (2 * it_step) / ppc, dq = 2 * it_step - dc * ppc;
    // a couple's rows as the stores see them: both pairs' row offsets (every lane
    // stores 256 B runs of ONE pair per instruction, see below), whether the second
    // pair exists, and whether each pair has its second frame
    struct Rows {
        long long oa, ob;
        bool two, ha, hb;
    };
    auto locate = [&](long long k, long long* c, long long* q, bool* valid, bool* edge_any, Rows* rw) {
        const bool two = 2 * k + 1 < pairs;
        const bool wrap = q0 + 1 == ppc;
        const long long c1 = two ? c0 + (wrap ? 1 : 0) : c0, q1 = two ? (wrap ? 0 : q0 + 1) : q0;
        *valid = !half || two;
        *c = half ? c1 : c0;
        *q = half ? q1 : q0;
        *edge_any = 2 * q0 * HOP + SPAN > n || 2 * q1 * HOP + SPAN > n;
        rw->oa = c0 * out_ch_stride + 2 * q0 * RP;
        rw->ob = c1 * out_ch_stride + 2 * q1 * RP;
        rw->two = two;
        rw->ha = 2 * q0 + 1 < frames;
        rw->hb = 2 * q1 + 1 < frames;
    };
    float xa[32], xt[8];   // span rows 0..31 (frame a) and 32..39 (frame b's rows 24..31)
    auto load_bulk = [&](long long c, long long q) {
        const float2* a = reinterpret_cast<const float2*>(sig + c * ch_stride + 2 * q * HOP) + m;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float2 u = ld_nt(a + 32 * i);
            xa[2 * i] = u.x;
            xa[2 * i + 1] = u.y;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 u = a[32 * (16 + i)];   // the next pair's span starts here: cached
            xt[2 * i] = u.x;
            xt[2 * i + 1] = u.y;
        }
    };
    // edge couples: the span through LDS with the zero rule (rolled loop), then the
    // residue layout directly (no swap)
    auto load_edge = [&](long long c, long long q) {
        const float* xs = sig + c * ch_stride;
        float* sf = reinterpret_cast<float*>(buf);
        const long long s0 = 2 * q * HOP;
#pragma unroll 1
        for (int k = m; k < SPAN; k += 32) sf[k] = s0 + k < n ? xs[s0 + k] : 0.0f;
        xsync<64>();
#pragma unroll
        for (int r = 0; r < 32; ++r) xa[r] = sf[32 * r + mr];
#pragma unroll
        for (int r = 0; r < 8; ++r) xt[r] = sf[N + 32 * r + mr];
        xsync<64>();
    };
    long long c, q;
    bool valid, edge;
    Rows rw;
    locate(it, &c, &q, &valid, &edge, &rw);
    if (!edge) load_bulk(c, q);
    for (; it < it_end; it += it_step) {
        if (edge) {
            load_edge(c, q);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) r32_pairswap(xa[2 * i], xa[2 * i + 1]);
#pragma unroll
            for (int i = 0; i < 4; ++i) r32_pairswap(xt[2 * i], xt[2 * i + 1]);
        }
        // v[r] = 0.5 w_r (a_r, b_r), b_r = span row r + 8
        float2 v[32];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const vf2_t A = {xa[2 * i], xa[2 * i + 1]};
            const vf2_t B = i < 12 ? vf2_t{xa[2 * i + 8], xa[2 * i + 9]} : vf2_t{xt[2 * i - 24], xt[2 * i - 23]};
            v[2 * i] = upk(pk_mul_bcast<0>(pk_pair<0>(A, B), wp[i]));
            v[2 * i + 1] = upk(pk_mul_bcast<1>(pk_pair<1>(A, B), wp[i]));
        }
        const long long itn = it + it_step;
        long long cn = c, qn = q;
        bool validn = valid, edgen = edge;
        Rows rwn = rw;
        if (itn < it_end) {   // the next couple's span, in flight across this one's transform
            q0 += dq;
            c0 += dc;
            if (q0 >= ppc) {
                q0 -= ppc;
                ++c0;
            }
            locate(itn, &cn, &qn, &validn, &edgen, &rwn);
            if (!edgen) load_bulk(cn, qn);
        }
        dft32<true>(v);
        r32_twiddle<true>(v, ltw + mr);
        r32_transpose(v, buf, mr, m);
        dft32<true>(v);
        // Z[N - k] (lane 32 - m, register 31 - r; lane 0: register 32 - r) through the
        // buffer: registers 16..31 for the power rows' bins 0..512, all 32 for the
        // magnitude rows, whose upper half each lane computes from its own
        // registers 16..31 (the same roundings as the mirror's: |X[N - k]| = |X[k]|
        // bit for bit), so every store has the lanes in address order
#pragma unroll
        for (int r = MODE == 0 ? 0 : 16; r < 32; ++r) buf[R32_ROW * r + m] = v[r];
        xsync<64>();
        float2 zm[16];   // zm[15 - k2] = Z[N - (m + 32 k2)], k2 < 16
        lds_rd64x16<0, 8 * R32_ROW>(buf + R32_ROW * (m == 0 ? 17 : 16) + ((32 - m) & 31), zm);
        float2 zu[16];   // MODE 0: zu[31 - r] = Z[N - (m + 32 r)], r >= 16 (lane 0, r = 16: Z[512] itself)
        if constexpr (MODE == 0) lds_rd64x16<0, 8 * R32_ROW>(buf + R32_ROW * (m == 0 ? 1 : 0) + ((32 - m) & 31), zu);
        xsync<64>();   // the next couple's transpose writes stay behind these reads
        if constexpr (MODE == 0) {
            // magnitude rows, all N bins: lane m holds bin m + 32 r of its pair's two
            // rows, r < 32.  Blocks 2j, 2j + 1 of one row are an aligned 256 B run: one
            // v_permlane32_swap per register pair moves half 0's block 2j + 1 up and half
            // 1's block 2j down, so each store writes 256 B of ONE pair's row (the first
            // pair's, then the second's) -- the 64-lane width of k_stft_pair's stores.
            float A[32], B[32];
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                float2 pa, pb;
                pair_post<0>(v[r], r < 16 ? ((r == 0 && m == 0) ? v[0] : zm[15 - r]) : zu[31 - r], &pa, &pb);
                A[r] = pa.x;
                B[r] = pb.x;
            }
            const int lo = half * 32 + m;   // this lane's float in a 256 B run
            float* ra = out + rw.oa + lo;
            float* rb = out + rw.ob + lo;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                r32_halfswap(A[2 * j], A[2 * j + 1]);
                r32_halfswap(B[2 * j], B[2 * j + 1]);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) __builtin_nontemporal_store(A[2 * j], ra + 64 * j);
            if (rw.two) {
#pragma unroll
                for (int j = 0; j < 16; ++j) __builtin_nontemporal_store(A[2 * j + 1], rb + 64 * j);
            }
            if (rw.ha) {
#pragma unroll
                for (int j = 0; j < 16; ++j) __builtin_nontemporal_store(B[2 * j], ra + RW + 64 * j);
            }
            if (rw.two && rw.hb) {
#pragma unroll
                for (int j = 0; j < 16; ++j) __builtin_nontemporal_store(B[2 * j + 1], rb + RW + 64 * j);
            }
        }
        if constexpr (MODE == 2) {
            const long long fa = 2 * q;
            float* rowa = out + c * out_ch_stride + fa * RP + m;
            float* rowb = rowa + RP;
            const bool hb = fa + 1 < frames;
            float A[16], B[16];
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                float2 pa, pb;
                pair_post<2>(v[k2], (k2 == 0 && m == 0) ? v[0] : zm[15 - k2], &pa, &pb);
                A[k2] = pa.x;
                B[k2] = pb.x;
            }
            float2 na, nb;   // bin 512: Z[512] is its own mirror (lane 0, register 16)
            pair_post<2>(v[16], v[16], &na, &nb);
            if (valid && m == 0) {   // each half's lane 0: its own pair's bin 512
                rowa[512] = na.x;
                if (hb) rowb[512] = nb.x;
            }
            // bins 0..511 as 256 B runs of one pair's row per store (v_permlane32_swap,
            // as the magnitude rows)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                r32_halfswap(A[2 * j], A[2 * j + 1]);
                r32_halfswap(B[2 * j], B[2 * j + 1]);
            }
            const int lo = half * 32 + m;
            float* pa = out + rw.oa + lo;
            float* pb = out + rw.ob + lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) pa[64 * j] = A[2 * j];
            if (rw.two) {
#pragma unroll
                for (int j = 0; j < 8; ++j) pb[64 * j] = A[2 * j + 1];
            }
            if (rw.ha) {
#pragma unroll
                for (int j = 0; j < 8; ++j) pa[RP + 64 * j] = B[2 * j];
            }
            if (rw.two && rw.hb) {
#pragma unroll
                for (int j = 0; j < 8; ++j) pb[RP + 64 * j] = B[2 * j + 1];
            }
        }
        if constexpr (MEL) {
            // this half's pair: power of bins m + 32 k2 (k2 < 16) and bin 512 (lane
            // 0) into its buffer as P[2k] = |Xa[k]|^2, P[2k + 1] = |Xb[k]|^2
            float* P = reinterpret_cast<float*>(buf);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                float2 pa, pb;
                pair_post<2>(v[k2], (k2 == 0 && m == 0) ? v[0] : zm[15 - k2], &pa, &pb);
                *reinterpret_cast<vf2_t*>(P + 2 * (m + 32 * k2)) = vf2_t{pa.x, pb.x};
            }
            float2 na, nb;   // bin 512: Z[512] is its own mirror (lane 0, register 16)
            pair_post<2>(v[16], v[16], &na, &nb);
            if (m == 0) {
                *reinterpret_cast<vf2_t*>(P + 2 * (N / 2)) = vf2_t{na.x, nb.x};
                if constexpr (MelArgs::W2) {   // zeros under the last windows' tails (as mel_rows)
#pragma unroll
                    for (int z = 1; z <= 3; ++z) *reinterpret_cast<vf2_t*>(P + 2 * (N / 2 + z)) = vf2_t{0.0f, 0.0f};
                }
            }
            xsync<64>();
            const int* mi = reinterpret_cast<const int*>(mel_lds);
            for (int h = 0; h < 2; ++h) {   // the two pairs in turn, each over the whole wave
                if (h == 1 && !rw.two) break;
                float* Ph = reinterpret_cast<float*>(xch + (2 * slot + h) * R33_BUF);
                float* fa_row = out + (h ? rw.ob : rw.oa);
                mel_tail<MODE, false>(lane, Ph, fa_row, fa_row + RP, h ? rw.hb : rw.ha, nullptr, mel_lds,
                                      mi + mel.nnz, mi + mel.nnz + mel.cw * mel.nc, mel_lds + mel_dpos,
                                      mel_lds + mel_dpos + mel.C * mel.M, mel);
            }
            xsync<64>();   // the next couple's transpose writes stay behind the tails' reads
        }
        c = cn;
        q = qn;
        valid = validn;
        edge = edgen;
        rw = rwn;
    }
}

}  // namespace vvh
