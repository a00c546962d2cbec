// shim_mel.hip -- Mel / MFCC plans (src/features/mel.c) over mel_kernels.hip:
// filterbank tables staged on the device, and the fused signal -> log-mel /
// MFCC entry point over an STFT handle.
#include "shim_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace vvh;

struct vvhip_mel {
    int n_mels = 0, nbins = 0, n_coeffs = 0, nnz = 0;
    float eps = 0.0f;
    float* W = nullptr;     // non-zero weight ranges of every filter, packed
    int* chunks = nullptr;  // balanced chunk schedule of the filters (mel_chunk_schedule)
    int* cbeg = nullptr;    // first chunk of each filter, [n_mels + 1]
    int nc = 0;
    float* Wf = nullptr;    // the fused kernels' chunk windows (MelArgs: rows of lc + 1 floats, lo last)
    int lc = 0;             // window length (0: no fused layout)
    float* D = nullptr;     // DCT-II table [n_coeffs][n_mels]
    float* lift = nullptr;  // lifter factors [n_coeffs]
    HostStage host;
    DevBuf bin, bout;
};

extern "C" {

void vvhip_mel_destroy(vvhip_mel* m) {
    if (!m) return;
    m->host.release();
    if (m->W) (void)hipFree(m->W);
    if (m->Wf) (void)hipFree(m->Wf);
    if (m->chunks) (void)hipFree(m->chunks);
    if (m->cbeg) (void)hipFree(m->cbeg);
    if (m->D) (void)hipFree(m->D);
    if (m->lift) (void)hipFree(m->lift);
    m->bin.release();
    m->bout.release();
    delete m;
}

int vvhip_mel_create(const float* fb, size_t n_mels, size_t nbins, size_t n_coeffs, float lifter, float eps,
                     vvhip_mel** out) {
    if (!out) return ST_NULL;
    *out = nullptr;
    if (n_mels == 0 || (fb && nbins == 0) || n_coeffs > n_mels) return ST_SIZE;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    vvhip_mel* m = new (std::nothrow) vvhip_mel;
    if (!m) return ST_INTERNAL;
    m->n_mels = (int)n_mels;
    m->nbins = fb ? (int)nbins : 0;
    m->n_coeffs = (int)n_coeffs;
    m->eps = eps;
    std::vector<float> w;
    std::vector<int> meta(3 * n_mels, 0);   // per filter: lo, len, offset into W (host: the chunk schedule)
    if (fb) {
        for (size_t f = 0; f < n_mels; ++f) {
            const float* r = fb + f * nbins;
            size_t lo = 0, hi = 0;
            for (size_t k = 0; k < nbins; ++k)
                if (r[k] != 0.0f) {
                    if (hi == 0) lo = k;
                    hi = k + 1;
                }
            meta[3 * f] = (int)lo;
            meta[3 * f + 1] = (int)(hi > lo ? hi - lo : 0);
            meta[3 * f + 2] = (int)w.size();
            for (size_t k = lo; k < hi; ++k) w.push_back(r[k]);
        }
    }
    m->nnz = (int)w.size();
    std::vector<int> chunks, cbeg;
    const int lc = mel_chunk_schedule(meta.data(), (int)n_mels, &chunks, &cbeg);
    m->nc = (int)(chunks.size() / 3);
    // The fused kernels' layout (MelArgs, cw = 0): one window of lcw bins per lane
    // slot, a row of MelArgs::window_stride(lcw) floats (the chunk's weights at its
    // own bins, zeros elsewhere, then start | chunk << 16 as int bits).
    // Bank-aware order: the kernel's 64 lanes read their windows' power pairs in
    // lockstep, so chunks whose windows start on the same bank residue (start mod
    // 32, in bins) within one lane group of the read instruction conflict.  Each
    // window may start anywhere in [lo + len - lc, lo] -- extra leading / trailing
    // zero weights add exact zeros, so the sums are bit-identical -- and any chunk
    // may sit in any lane slot, since each slot writes its partial to its chunk's
    // own index (the row's last float: start | chunk << 16).  With MelArgs::W2 the
    // windows are the schedule's lc + 4 bins and start on even bins (two bins per
    // ds_read_b128, whose lane groups are {0-3,12-15,20-27}, {4-11,16-19,28-31},
    // and the same + 32: MI355X_MICROARCH.md LDS table); otherwise ds_read_b64's
    // two 32-lane groups.  Greedy: chunks with the least slack first, each to the
    // (group, start) with the fewest windows on that residue.  The 40-mel /
    // 1024-point plan: 5 -> 2 extra LDS cycles per b64 bin step.
    std::vector<float> wf;
    const int lcw = MelArgs::W2 ? lc + 4 : lc, SS = MelArgs::W2 ? 2 : 1;
    if (fb && m->nc > 0 && lc % 4 == 0 && lcw <= (int)nbins && m->nc < 32768 && nbins < 65536 &&
        (!MelArgs::W2 || nbins == 513)) {   // W2: the fused kernel's rows (nfft 1024) only
        const int lcs = MelArgs::window_stride(lcw), nc = m->nc, nb = (int)nbins;
        // the lane groups of every round (64 slots), as slot lists
        std::vector<std::vector<int>> groups;
        for (int r = 0; 64 * r < nc; ++r) {
            auto add = [&](std::initializer_list<std::pair<int, int>> ranges) {
                std::vector<int> g;
                for (auto rg : ranges)
                    for (int l = rg.first; l <= rg.second; ++l)
                        if (64 * r + l < nc) g.push_back(64 * r + l);
                if (!g.empty()) groups.push_back(g);
            };
            if (MelArgs::W2) {
                for (int h = 0; h < 64; h += 32) {
                    add({{h + 0, h + 3}, {h + 12, h + 15}, {h + 20, h + 27}});
                    add({{h + 4, h + 11}, {h + 16, h + 19}, {h + 28, h + 31}});
                }
            } else {
                add({{0, 31}});
                add({{32, 63}});
            }
        }
        const int ng = (int)groups.size();
        std::vector<int> order(nc), used((size_t)ng * 32, 0), start(nc);
        std::vector<std::vector<int>> members(ng);
        auto smin = [&](int c) { const int v = chunks[3 * c] + chunks[3 * c + 1] - lcw; return v > 0 ? v : 0; };
        // W2: a window may reach 3 bins past the row (the kernel zeroes P's bins
        // nb .. nb + 2), so even the last chunk has an even start
        const int top = MelArgs::W2 ? nb + 3 - lcw : nb - lcw;
        auto smax = [&](int c) { return chunks[3 * c] < top ? chunks[3 * c] : top; };
        for (int c = 0; c < nc; ++c) order[c] = c;
        std::stable_sort(order.begin(), order.end(),
                         [&](int a, int b) { return smax(a) - smin(a) < smax(b) - smin(b); });
        bool ok_sched = true;
        for (int c : order) {
            int bg = -1, bs = 0, bu = 0, bn = 0;
            for (int g = 0; g < ng; ++g) {
                const int n = (int)members[g].size();
                if (n >= (int)groups[g].size()) continue;
                for (int st = smax(c) / SS * SS; st >= smin(c); st -= SS) {
                    const int u = used[(size_t)g * 32 + st % 32];
                    if (bg < 0 || u < bu || (u == bu && n < bn)) {
                        bg = g;
                        bs = st;
                        bu = u;
                        bn = n;
                    }
                }
            }
            if (bg < 0) {   // no start in range (not for lc <= nbins): no windows
                ok_sched = false;
                break;
            }
            ++used[(size_t)bg * 32 + bs % 32];
            members[bg].push_back(c);
            start[c] = bs;
        }
        if (ok_sched) {
            wf.assign((size_t)nc * lcs, 0.0f);
            for (int g = 0; g < ng; ++g)
                for (size_t q = 0; q < members[g].size(); ++q) {
                    const int c = members[g][q], slot = groups[g][q];
                    const int lo = chunks[3 * c], len = chunks[3 * c + 1], off = chunks[3 * c + 2], st = start[c];
                    for (int j = 0; j < lcw; ++j) {
                        const int k = st + j;
                        if (k >= lo && k < lo + len) wf[(size_t)slot * lcs + j] = w[(size_t)off + (k - lo)];
                    }
                    const int bits = st | (c << 16);
                    std::memcpy(&wf[(size_t)slot * lcs + lcw], &bits, sizeof bits);
                }
            m->lc = lcw;
        }
    }
    // DCT-II rows cos(pi (j + 1/2) i / M) (dct.c:21-30), and the lifter of mel.c:300-302
    std::vector<float> D(n_coeffs * n_mels), L(n_coeffs, 1.0f);
    for (size_t i = 0; i < n_coeffs; ++i)
        for (size_t j = 0; j < n_mels; ++j)
            D[i * n_mels + j] = (float)std::cos(M_PI * ((double)j + 0.5) * (double)i / (double)n_mels);
    if (lifter > 0.0f)
        for (size_t i = 1; i < n_coeffs; ++i)
            L[i] = 1.0f + (lifter / 2.0f) * sinf((float)M_PI * (float)i / lifter);
    bool ok = hipMalloc(&m->chunks, sizeof(int) * (chunks.size() + 1)) == hipSuccess &&
              (chunks.empty() ||
               hipMemcpy(m->chunks, chunks.data(), sizeof(int) * chunks.size(), hipMemcpyHostToDevice) == hipSuccess) &&
              hipMalloc(&m->cbeg, sizeof(int) * cbeg.size()) == hipSuccess &&
              hipMemcpy(m->cbeg, cbeg.data(), sizeof(int) * cbeg.size(), hipMemcpyHostToDevice) == hipSuccess &&
              hipMalloc(&m->W, sizeof(float) * (w.size() + 1)) == hipSuccess &&
              hipMalloc(&m->Wf, sizeof(float) * (wf.size() + 1)) == hipSuccess &&
              (wf.empty() || hipMemcpy(m->Wf, wf.data(), sizeof(float) * wf.size(), hipMemcpyHostToDevice) == hipSuccess) &&
              (w.empty() || hipMemcpy(m->W, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice) == hipSuccess) &&
              hipMalloc(&m->D, sizeof(float) * (D.size() + 1)) == hipSuccess &&
              (D.empty() || hipMemcpy(m->D, D.data(), sizeof(float) * D.size(), hipMemcpyHostToDevice) == hipSuccess) &&
              hipMalloc(&m->lift, sizeof(float) * (L.size() + 1)) == hipSuccess &&
              (L.empty() || hipMemcpy(m->lift, L.data(), sizeof(float) * L.size(), hipMemcpyHostToDevice) == hipSuccess);
    if (!ok) {
        vvhip_mel_destroy(m);
        return fail(ST_INTERNAL, "mel tables upload");
    }
    *out = m;
    return ST_OK;
}

static size_t mel_in_len(const vvhip_mel* m, int kind) { return kind == 2 ? (size_t)m->n_mels : (size_t)m->nbins; }
static size_t mel_out_len(const vvhip_mel* m, int kind) { return kind == 0 ? (size_t)m->n_mels : (size_t)m->n_coeffs; }

// row_pitch (kinds 0 / 1): floats from one power row's start to the next, >= nbins (0: nbins)
int vvhip_mel_pitched_device(vvhip_mel* m, const float* d_in, size_t frames, size_t row_pitch, float* d_out, int kind,
                             void* stream) {
    if (!m || !d_in || !d_out) return ST_NULL;
    if (kind < 0 || kind > 2) return fail(ST_RANGE, "mel output kind");
    if ((kind != 2 && m->nbins == 0) || (kind != 0 && m->n_coeffs == 0)) return fail(ST_RANGE, "mel plan lacks tables");
    if (kind == 2) row_pitch = 0;
    if (row_pitch != 0 && row_pitch < (size_t)m->nbins) return fail(ST_SIZE, "mel input row pitch below the row length");
    if (frames == 0) return ST_OK;
    const hipStream_t s = (hipStream_t)stream;
    // the kernel stages whole pitched rows (pad included) through LDS; a pad
    // past 64 floats would cost reads (and, far out, more LDS than a CU has):
    // such rows are packed first by one 2-D copy, then run as packed rows
    Scratch packed(s);
    if (row_pitch > (size_t)m->nbins + 64) {
        const size_t rb = sizeof(float) * (size_t)m->nbins;
        HIPCHK(packed.alloc(rb * frames), ST_INTERNAL);
        HIPCHK(hipMemcpy2DAsync(packed.p, rb, d_in, sizeof(float) * row_pitch, rb, frames, hipMemcpyDeviceToDevice, s),
               ST_INTERNAL);
        d_in = (const float*)packed.p;
        row_pitch = 0;
    }
    HIPCHK(launch_mel_grp(kind, d_in, (long long)frames, m->nbins, m->n_mels, m->n_coeffs, m->W, m->nnz, m->chunks,
                          m->nc, m->cbeg, m->D, m->lift, m->eps, d_out, s, (int)row_pitch),
           ST_INTERNAL);
    return ST_OK;
}
int vvhip_mel_device(vvhip_mel* m, const float* d_in, size_t frames, float* d_out, int kind, void* stream) {
    return vvhip_mel_pitched_device(m, d_in, frames, 0, d_out, kind, stream);
}

// Signal -> log-mel (kind 0) / MFCC (kind 1) rows [ch][frame][n_mels or
// n_coeffs]: one fused launch (launch_stft_mel) when the shape allows it, else
// the power rows into scratch and the plan's mel kernel -- the same values.
int vvhip_stft_mel_device(vvhip_stft* h, vvhip_mel* m, const float* d_signal, size_t n, size_t nch, size_t ch_stride,
                          float* d_out, size_t out_ch_stride, int kind, void* stream) {
    if (!h || !m || !d_signal || !d_out) return ST_NULL;
    if (kind != 0 && kind != 1) return fail(ST_RANGE, "stft mel output kind");
    if (m->nbins != (int)(h->nfft / 2 + 1)) return fail(ST_SIZE, "mfcc plan bins differ from the stft's nfft/2+1");
    if (kind == 1 && m->n_coeffs == 0) return fail(ST_RANGE, "mfcc plan lacks the DCT");
    if (nch == 0) return ST_OK;
    const hipStream_t s = (hipStream_t)stream;
    const size_t frames = vvhip_stft_num_frames(n, h->nfft, h->hop);
    const float* win = stft_window_here(h);
    if (!win) return fail(ST_INTERNAL, "stft window on the current device");
    if (knob(KNOB_MEL_FUSED, 1) != 0) {   // 0: the two launches (A/B)
        MelArgs a;
        a.W = m->W;
        a.chunks = m->chunks;
        a.Ww = m->lc > 0 ? m->Wf : nullptr;   // the chunk windows (launch_stft_mel's choice)
        a.lcw = m->lc;
        a.cbeg = m->cbeg;
        a.D = m->D;
        a.lift = m->lift;
        a.nnz = m->nnz;
        a.nc = m->nc;
        a.M = m->n_mels;
        a.C = m->n_coeffs;
        a.eps = m->eps;
        const hipError_t e = launch_stft_mel(kind, (long long)h->nfft, (long long)h->hop, d_signal, (long long)n,
                                             (long long)nch, (long long)ch_stride, (long long)frames, win, a, d_out,
                                             (long long)out_ch_stride, s);
        if (e == hipSuccess) {
            stat_inc(STAT_MEL_FUSED);
            return ST_OK;
        }
        if (e != hipErrorNotSupported) return fail(ST_INTERNAL, hipGetErrorString(e));
        (void)hipGetLastError();
    }
    stat_inc(STAT_MEL_SPLIT);
    const size_t nb = h->nfft / 2 + 1, width = kind == 0 ? (size_t)m->n_mels : (size_t)m->n_coeffs;
    Scratch pw(s);
    HIPCHK(pw.alloc(sizeof(float) * nch * frames * nb), ST_INTERNAL);
    int st = stft_frames_run(h, d_signal, n, nch, ch_stride, pw.p, frames * nb, 2, s);
    if (st) return st;
    if (out_ch_stride == frames * width) return vvhip_mel_device(m, (const float*)pw.p, nch * frames, d_out, kind, stream);
    for (size_t c = 0; c < nch && !st; ++c)
        st = vvhip_mel_device(m, (const float*)pw.p + c * frames * nb, frames, d_out + c * out_ch_stride, kind, stream);
    return st;
}

int vvhip_mel_host(vvhip_mel* m, const float* in, size_t frames, float* out, int kind) {
    if (!m || !in || !out) return ST_NULL;
    std::lock_guard<std::mutex> host_lock(m->host.mu);
    if (kind < 0 || kind > 2) return fail(ST_RANGE, "mel output kind");
    if (frames == 0) return ST_OK;
    HIPCHK(m->host.stream_or_create(), ST_INTERNAL);
    const hipStream_t s = m->host.stream;
    const size_t ib = sizeof(float) * frames * mel_in_len(m, kind), ob = sizeof(float) * frames * mel_out_len(m, kind);
    HIPCHK(m->bin.ensure(ib), ST_INTERNAL);
    HIPCHK(m->bout.ensure(ob), ST_INTERNAL);
    HIPCHK(hipMemcpyAsync(m->bin.p, in, ib, hipMemcpyHostToDevice, s), ST_INTERNAL);
    int st = vvhip_mel_device(m, (const float*)m->bin.p, frames, (float*)m->bout.p, kind, s);
    if (st) return st;
    HIPCHK(hipMemcpyAsync(out, m->bout.p, ob, hipMemcpyDeviceToHost, s), ST_INTERNAL);
    HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
    return ST_OK;
}

}  // extern "C"
