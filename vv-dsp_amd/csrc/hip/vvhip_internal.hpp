// vvhip_internal.hpp -- launchers shared between the kernel translation units
// and the extern "C" shim (shim_*.hip).  Not part of the public C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vvh {

// ---- A/B switches and path counters (debug.hip) ---------------------------
// Knob values come from vvhip_debug_set (or, with VVHIP_AB=1, from the
// environment read once per process); knob(k, dflt) returns dflt when unset.
enum Knob : int {
    KNOB_STFT_CPS, KNOB_STFT_RUN, KNOB_STFT_DBS, KNOB_POW_OLD, KNOB_STFT_RING, KNOB_STFT_DYN,
    KNOB_FS_VAR, KNOB_FS_CHUNK_MB, KNOB_FS_OLD, KNOB_BLUE_UNFUSED, KNOB_C2C_MAX, KNOB_STFT_SQ,
    KNOB_MIX_CHUNK_MB, KNOB_MIX_R2C_FULL, KNOB_FIR_OLD, KNOB_FIR_DYN, KNOB_FIR_DIRECT_LDS, KNOB_FIR_BLOCK,
    KNOB_HOST_CHUNK_MB, KNOB_NO_MIXED, KNOB_REAL_PROMOTE, KNOB_ISTFT_OLD, KNOB_MEL_FUSED, KNOB_CZT_UNFUSED,
    KNOB_CEPS_UNFUSED, KNOB_FIR_R32, KNOB_DIST_SLAB_KB, KNOB_POW_R32, KNOB_MAG_R32, KNOB_MEL_R32,
    KNOB_C2C_TPW, KNOB_C2C_ONE, KNOB_REAL_TPW, KNOB_ANA_TPW, KNOB_MIX_TPW, KNOB_C2C_SMALL, KNOB_DCT_SMALL, KNOB_HIL_SMALL, KNOB_REAL_SMALL, KNOB_R2C_SMALL, KNOB_STFT_STAGE, KNOB_STFT_ONE, KNOB_MFCC_WIN, KNOB_RESAMPLE_GENERIC, KNOB_LPC_GENERIC, KNOB_IIR_CHUNK, KNOB_STATS_LONG, KNOB_INTERP_ROWS, KNOB_PITCH_F32, KNOB_SHAPE_DWORD, KNOB_PVOC_GROUP, KNOB_PVOC_PLANE, KNOB_PTRACK_GROUP, KNOB_MEDIAN_SELECT, KNOB_HPSS_GROUP, KNOB_DENOISE_SEGMENT, KNOB_DENOISE_MIN, KNOB_DENOISE_GROUP, KNOB_LSF_GROUP, KNOB_LPC_SYNTH_CHUNK, KNOB_LPC_FILTER_GROUP, KNOB_COUNT
};
long long knob(Knob k, long long dflt);
// launches of the paths the tests must see taken (vvhip_debug_get("STAT_..."))
enum Stat : int { STAT_STFT_DYN, STAT_FIR_DYN, STAT_FIR_STATIC, STAT_MEL_FUSED, STAT_MEL_SPLIT, STAT_FIR_R32, STAT_POW_R32, STAT_MAG_R32, STAT_MEL_R32, STAT_RESAMPLE_TABLE, STAT_RESAMPLE_GENERIC, STAT_LPC_WAVE, STAT_LPC_GENERIC, STAT_IIR_EXACT, STAT_IIR_CHUNKED, STAT_STATS_WAVE, STAT_STATS_LONG, STAT_INTERP_ONE, STAT_INTERP_ROWS, STAT_PITCH_WAVE, STAT_SHAPE_WAVE, STAT_SHAPE_VEC16, STAT_PVOC_ROWS, STAT_PITCH_TRACK, STAT_DENOISE, STAT_LSF, STAT_FORMANT, STAT_LPC_RESIDUAL, STAT_LPC_SYNTH_EXACT, STAT_LPC_SYNTH_CHUNKED, STAT_COUNT };
void stat_inc(Stat s);

// Device-resident W_N^k = exp(-2*pi*i*k/N) table, k < N, f32 rounded from double.
// Cached per N for the process lifetime (per device).
const float2* twiddle_table(int n);
const double2* twiddle_table_d(long long n);
// Pass-major inter-pass twiddles of the length-n Stockham FFT (fft_core.hpp TwTab).
const float2* pass_twiddles(int n);

// Two-level table for large n (fourstep_fft.hip, fft_glue.hip): lo[2^lo_bits] ++ hi[n >> lo_bits].
const float2* twiddle_split(long long n, int* lo_bits);

// ---- large power-of-two C2C (fourstep_fft.hip): two HBM passes (fourstep.hpp)
// up to 2^20, five passes over the fused kernels above
bool c2c_large_supported(long long n);     // pow2, 8192 .. 2^24
hipError_t launch_c2c_large(long long n, int fwd, const float2* in, float2* out, long long batch,
                            hipStream_t s);
// Bluestein (bluestein.hip) for any n with pow2(2n-1) <= 2^24; same contract as
// launch_dft_naive (real_in promotes real input; nout bins written).
constexpr long long BLUESTEIN_MIN = 1025;   // below: the f64 O(n^2) DFT (exact-angle, faster at small n)
bool bluestein_supported(long long n);
hipError_t launch_bluestein(long long n, int fwd, const void* in, int real_in, float2* out, long long nout,
                            long long batch, long long in_dist, long long out_dist, float scale, hipStream_t s);
// Mixed-radix Stockham FFT (mixed_fft.hip routes to mixed_plan.hip, sq_rows.hip,
// sq_stft.hip, mixed_fourstep.hip) for 7-smooth non-power-of-two n; same contract as launch_dft_naive, and in == out is allowed.
bool mixed_supported(long long n);
bool stft_mixed_supported(long long n);
hipError_t launch_fft_mixed(long long n, int fwd, const void* in, int real_in, float2* out, long long nout,
                            long long batch, long long in_dist, long long out_dist, float scale, hipStream_t s);
// STFT rows through the mixed-radix kernel (frames gathered and windowed on
// load, |X| / complex / power bins 0..n/2 on store): kind as launch_stft.
hipError_t launch_stft_mixed(long long nfft, long long hop, int kind, const float* sig, long long n, long long nch,
                             long long ch_stride, long long frames, const float* win, void* out,
                             long long out_ch_stride, hipStream_t s);
// Real pow2 n = 2M above the fused kernels: split steps around an M-point C2C
// (fft_glue.hip).  fwd: Z [batch][M] -> X [batch][M+1]; inv: X -> V [batch][M].
hipError_t launch_real_split_fwd(const float2* Z, float2* X, long long M, long long batch, hipStream_t s);
hipError_t launch_real_split_inv(const float2* X, float2* V, long long M, long long batch, hipStream_t s);
// real[batch][n] -> complex[batch][n] (imaginary 0) (fft_glue.hip)
hipError_t launch_promote_real(const float* in, float2* out, long long count, hipStream_t s);

// ---- mel / MFCC (mel_kernels.hip) ---------------------------------------
// mode 0: power rows [frames][nbins] -> log-mel [frames][n_mels]
//      1: power rows -> MFCC [frames][n_coeffs];  2: log-mel rows -> MFCC
// in_pitch (modes 0 / 1): floats from one power row's start to the next (0: nbins)
hipError_t launch_mel_grp(int mode, const float* in, long long frames, int nbins, int n_mels, int n_coeffs,
                          const float* W, int nnz, const int* chunks, int nc, const int* cbeg, const float* D,
                          const float* lift, float eps, float* out, hipStream_t s, int in_pitch = 0);
// host: chunk schedule of the filters' non-zero ranges {lo, len, off}[n_mels] for
// launch_mel_grp (chunks {lo, len, off}, cbeg[n_mels+1]); returns the chunk length
int mel_chunk_schedule(const int* meta, int n_mels, std::vector<int>* chunks, std::vector<int>* cbeg);

// Write sink (SINK_FLOATS floats): destination of lanes that must issue a store
// with nothing to write, in kernels that hand-count their memory operations.
constexpr size_t SINK_FLOATS = 1u << 18;   // 1 MiB = 4096 waves x 64 lanes
float* store_sink();
// zeroed work counters of the dynamic walks (32 counter streams x 32 words) for a
// launch on stream s (tables.hip: per-(device, stream) pool blocks; a private,
// memset-on-replay block under graph capture); nullptr: take the static walk
constexpr size_t STFT_CTR_WORDS = 32 * 32;
unsigned* stream_counters(hipStream_t s);
// ---- batched framing (framing_kernels.hip), framing.c:58-146 semantics
long long reflect_sample(long long idx, long long n);   // framing.c:21-56, host side (span bounds)
hipError_t launch_fetch_frames(const float* sig, long long base, long long n, float* out, long long len,
                               long long hop, long long frame0, long long count, int center, const float* win,
                               hipStream_t s);
hipError_t launch_overlap_add(const float* frames, long long count, float* out, long long out_len, long long len,
                              long long hop, long long frame0, hipStream_t s);
// The rows a per-frame launch (LPC, statistics, pitch) reads, `rows` rows of
// len samples, of one of two kinds:
//   framed 0: row r is x + r * row_stride (frames = rows);
//   framed 1: row ch * frames + f is frame f of channel x + ch * ch_stride, an
//     n = sig_n sample signal, with exactly the value launch_fetch_frames gives
//     its sample i: sample f * hop - (center ? len / 2 : 0) + i of the signal,
//     zero outside it or, when center, reflected into it (framing.c:21-56), times
//     win[i] in one rounded multiply when win is not null.
// rows and frames are below 2^31.  frame_src.hpp is the device side: the one
// statement of that value, which the frame gather itself reads through.
struct FrameSrc {
    const float* x = nullptr;
    long long len = 0, rows = 0, frames = 0, row_stride = 0;
    long long sig_n = 0, ch_stride = 0, hop = 0;
    int framed = 0, center = 0;
    const float* win = nullptr;
};

// Persistent-grid sizing: resident blocks for `kernel` x CUs, capped by work.
// CUs x resident workgroups of `kernel` (capped at max_per_cu when > 0), at most work_blocks
int persistent_grid(const void* kernel, int block, size_t dyn_lds, long long work_blocks, int max_per_cu = 0);
// persistent_grid computed once per call site (a launcher's static cache);
// concurrent first calls compute the same value, the atomic keeps that race-free
inline int cached_grid(std::atomic<int>& cache, const void* kernel, int block, size_t dyn_lds, long long work_blocks,
                       int max_per_cu = 0) {
    int g = cache.load(std::memory_order_relaxed);
    if (g == 0) {
        g = persistent_grid(kernel, block, dyn_lds, work_blocks, max_per_cu);
        cache.store(g, std::memory_order_relaxed);
    }
    return g;
}
// Blocks of a persistent launch: the kernel's resident grid (computed once per
// call site, `cache`), at most the `need` blocks the work fills; < 1: nothing to launch.
inline int capped_grid(int cap, long long need) { return (int)(need < cap ? need : cap); }
inline int capped_grid(std::atomic<int>& cache, const void* kern, int wg, long long need) {
    return capped_grid(cached_grid(cache, kern, wg, 0, 1LL << 40), need);
}
// Blocks of a dynamic-walk launch (counters per XCD group): the same number in each of the 8 groups
inline long long dyn_grid(int cap) { return cap / 8 * 8; }
// Blocks of 256 threads for an element-wise kernel over `count` items, which
// walks them with VVH_GRID_STRIDE: one thread per item up to 65536 blocks
inline unsigned stride_blocks(long long count) {
    const long long b = (count + 255) / 256;
    return (unsigned)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}
#define VVH_GRID_STRIDE(i, count) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (count); i += (long long)gridDim.x * blockDim.x)

// ---- pow2 register/LDS FFTs (fft_c2c.hip, fft_real.hip; the naive DFT and glue: fft_glue.hip)
bool c2c_supported(long long n);           // pow2, 2..4096
// batch transforms of length n; element e of transform f at in[f*in_dist + e]
hipError_t launch_c2c(long long n, int fwd, const float2* in, float2* out, long long batch,
                      long long in_dist, long long out_dist, float scale, hipStream_t s);
bool r2c_supported(long long n);           // pow2 real length, 32..8192
hipError_t launch_r2c(long long n, const float* in, float2* out, long long batch,
                      long long in_dist, long long out_dist, hipStream_t s);
hipError_t launch_c2r(long long n, const float2* in, float* out, long long batch,
                      long long in_dist, long long out_dist, hipStream_t s);
// Any n: O(n^2) DFT with f64 accumulation (the reference's non-pow2 path,
// fft_kiss.c:76-92).  real_in: input is real[n] (R2C promotion); nout bins written.
hipError_t launch_dft_naive(long long n, int fwd, const void* in, int real_in, float2* out,
                            long long nout, long long batch, long long in_dist,
                            long long out_dist, float scale, hipStream_t s);
// Hermitian expansion used by C2R/Hilbert for non-pow2 n: half[n/2+1] -> full[n]
hipError_t launch_hermitian_expand(long long n, const float2* half, float2* full, long long batch,
                                   long long half_dist, int zero_dc_nyq_imag, hipStream_t s);
hipError_t launch_take_real(const float2* in, float* out, long long count, hipStream_t s);
hipError_t launch_zero_nyquist_imag(float2* out, long long n, long long batch, long long dist,
                                    hipStream_t s);

// ---- STFT analysis (stft_kernels.hip routes to stft_pair / stft_small /
// stft_r32.hip; stft_mel.hip, stft_generic.hip) and synthesis (istft_kernels.hip)
// mode 0: magnitude rows [frames][nfft]; 1: complex rows [frames][nfft];
// 2: power rows [frames][nfft/2+1], row_pitch floats apart (0: packed, nfft/2+1)
bool stft_fused_supported(long long nfft);
hipError_t launch_stft(long long nfft, long long hop, int mode, const float* sig, long long n,
                       long long nch, long long ch_stride, long long frames, const float* win,
                       void* out, long long out_ch_stride, hipStream_t s, long long row_pitch = 0);
// Mel filterbank / log / DCT tables of an MFCC plan (vvhip_mel, device
// pointers) for the fused signal -> log-mel / MFCC launch
struct MelArgs {
    const float* W = nullptr;      // non-zero filter weights, packed (nnz)
    const int* chunks = nullptr;   // {lo, len, off} per chunk (mel_chunk_schedule)
    const int* cbeg = nullptr;     // first chunk of each filter [M + 1]
    const float* D = nullptr;      // DCT-II rows [C][M]
    const float* lift = nullptr;   // lifter factors [C]
    int nnz = 0, nc = 0, M = 0, C = 0;
    // The layout the kernel reads: cw = 3 -- W packed with the chunk table above;
    // cw = 0 -- each chunk's window of lc bins as a row of lcs = window_stride(lc) floats in W,
    // [c lcs + j] the weight of bin lo_c + j (zero outside the chunk), [c lcs + lc]
    // lo_c's bits, the window inside the row (lo_c + lc <= n/2 + 1), lc % 4 == 0, no
    // chunk table.  The plan passes the packed layout plus the windows (Ww, lcw);
    // launch_stft_mel gives log-mel the windows and MFCC the packed layout.
    int lc = 0, lcs = 0, cw = 3;
    // row stride of the chunk windows for lc bins (lc % 4 == 0): the first multiple
    // of 4 above lc whose quarter is odd, so 16 lanes' 16 B weight reads (rows
    // lcs floats apart) cover 16 distinct 4-bank blocks
    static constexpr int window_stride(int lc) { return (lc / 4) % 2 == 0 ? lc + 4 : lc + 8; }
#ifndef VVH_MEL_W2
#define VVH_MEL_W2 1
#endif
    // VVH_MEL_W2: the chunk windows are 4 bins longer than the chunk schedule's
    // lc and start on even bins, so the kernel reads their power pairs two bins
    // per ds_read_b128 (half the read instructions; the 4 extra bins weigh 0)
    static constexpr bool W2 = VVH_MEL_W2;
    const float* Ww = nullptr;
    int lcw = 0;
    float eps = 0.0f;
};
// Log-mel (kind 0) or MFCC (kind 1) rows [ch][frame][M or C] straight from the
// signal: the power rows of launch_stft mode 2 feed k_mel_grp's arithmetic in
// the same kernel, never written to HBM (bit-identical to the two launches).
// hipErrorNotSupported when the fused kernel does not take this shape
// (nfft != 1024, hop / alignment, M > 128, more than 64 * MEL_MAX_ROUNDS chunks;
// MFCC also M > 60 or C > 64): the caller runs the two launches.
hipError_t launch_stft_mel(int kind, long long nfft, long long hop, const float* sig, long long n, long long nch,
                           long long ch_stride, long long frames, const float* win, const MelArgs& mel, float* out,
                           long long out_ch_stride, hipStream_t s);
// Frames given explicitly (stft_process batch): in real[count][nfft] -> cpx[count][nfft]
hipError_t launch_stft_frames(long long nfft, const float* frames_in, const float* win,
                              float2* out, long long count, hipStream_t s);
// Generic gather (any nfft): windowed complex frames for the generic FFT path
hipError_t launch_frame_gather(long long nfft, long long hop, const float* sig, long long n,
                               long long nch, long long ch_stride, long long frames,
                               const float* win, float2* out, hipStream_t s);
hipError_t launch_magnitude(const float2* in, float* out, long long count, hipStream_t s);
hipError_t launch_rows_half(const float* in, float* out, long long rows, long long n, int unpack, hipStream_t s);
hipError_t launch_power_half(const float2* in, float* out, long long nfft, long long rows, hipStream_t s);
// ISTFT accumulate (stft_reconstruct batch): out_add[i] += Re(t[f][i])*w[i] for frames at hop
hipError_t launch_ola(long long nfft, long long hop, const float2* time_frames, long long count,
                      const float* win, float* out_add, float* norm_add, hipStream_t s);
// the same from the spectra in one kernel (inverse FFT + window + overlap-add): nfft 1024, hop | nfft, hop >= 256
bool istft_fused_supported(long long nfft, long long hop);
hipError_t launch_istft_fused(long long nfft, long long hop, const float2* spec, long long count,
                              const float* win, float* out_add, float* norm_add, hipStream_t s);

// ---- FIR (fir_ols.hip routes to fir_1024.hip; fir_direct.hip, fir_long.hip) ----
bool fir_ols_supported(long long nfft);
// Overlap-save geometry of n samples per channel in blocks of nfft with history
// le (fir_pair.hpp): lout outputs per block, nblk blocks, ppc pairs of blocks;
// pairs [qf, ql) are the bulk pairs -- input span start 2q*lout - le >= 0 and both
// blocks' outputs (2q+2)*lout <= n -- or empty (qf = ql = ppc); nfft - le >= 1.
struct FirGeo {
    long long le, lout, nblk, ppc, qf, ql;
};
FirGeo fir_geometry(long long nfft, long long le, long long n);
// H: nfft complex bins of FFT(h zero-padded)/nfft.  prefix: [nch][taps-1] chronological or null.
hipError_t launch_fir_ols(long long nfft, long long taps, const float2* H, const float* x,
                          float* y, long long n, long long nch, long long x_stride,
                          long long y_stride, const float* prefix, hipStream_t s);
hipError_t launch_fir_direct(const float* h, long long taps, const float* x, float* y, long long n,
                             long long nch, long long x_stride, long long y_stride,
                             const float* prefix, hipStream_t s);
// vv_dsp_filtfilt_fir over nch rows (common.c:23-80); tmp: nch * (n + taps - 1) floats
hipError_t launch_filtfilt(const float* h, long long taps, const float* x, float* y, long long n, long long nch,
                           long long x_stride, long long y_stride, float* tmp, hipStream_t s);
// overlap-save glue for filters beyond the fused kernels (N > 8192, four-step FFTs;
// the product with H is launch_cmul_rows, chirp_glue.hip):
// rows q < rows of pair p0 + q over (channel, pair) items, ppc pairs per channel,
// row = z[e] = (x[2j*lout - le + e], x[(2j+1)*lout - le + e]) zero outside [0, n)
hipError_t launch_fir_long_gather(const float* x, long long n, long long x_stride, long long nfft, long long le,
                                  long long lout, long long ppc, long long p0, long long rows, float2* z,
                                  hipStream_t s);
hipError_t launch_fir_long_scatter(const float2* z, float* y, long long n, long long y_stride, long long nfft,
                                   long long le, long long lout, long long ppc, long long p0, long long rows,
                                   hipStream_t s);
hipError_t launch_scale_real(float* p, long long count, float s, hipStream_t st);
hipError_t launch_scale_cpx(float2* p, long long count, float s, hipStream_t st);

// ---- rational resampler (resample_kernels.hip), resampler.c:65-119 per row ----
// rows of in_n samples in_stride floats apart -> rows of out_n samples out_stride
// floats apart; ratio = (double)num / (double)den as the reference forms it.
hipError_t launch_resample_linear(const float* in, long long in_n, long long nch, long long in_stride, float* out,
                                  long long out_n, long long out_stride, double ratio, hipStream_t s);
// table kernel: W [phases][resample_row_stride(taps)] polyphase rows (phases = P + 1);
// a workgroup takes resample_run(...) consecutive outputs of one row.
constexpr int RESAMPLE_RUN = 1024;                     // outputs per workgroup, at most
constexpr size_t RESAMPLE_LDS_BYTES = 128u << 10;      // table + input span of one workgroup
constexpr size_t RESAMPLE_TABLE_BYTES = 96u << 10;     // larger tables take the generic kernel
// floats from one table row to the next in LDS: taps rounded up to a multiple of 4
// with an odd quarter, so 16 lanes' 16 B reads of 16 rows cover 16 distinct 4-bank blocks
constexpr int resample_row_stride(int taps) { return ((taps + 3) / 4) % 2 ? (taps + 3) / 4 * 4 : (taps + 3) / 4 * 4 + 4; }
// outputs per workgroup for this ratio and table (the span must fit beside the table); 0: generic kernel
int resample_run(long long phases, int taps, double ratio);
hipError_t launch_resample_table(const float* in, long long in_n, long long nch, long long in_stride, float* out,
                                 long long out_n, long long out_stride, double ratio, double cutoff, long long phases,
                                 int taps, const float* W, hipStream_t s);
// every output evaluates its own weights in f64 (any ratio; slow)
hipError_t launch_resample_generic(const float* in, long long in_n, long long nch, long long in_stride, float* out,
                                   long long out_n, long long out_stride, double ratio, double cutoff, int taps,
                                   hipStream_t s);

// ---- interpolation at arbitrary positions (interp_kernels.hip), interpolate.c:4-64 per output ----
constexpr int INTERP_LINEAR = 0, INTERP_CUBIC = 1;   // vv_dsp_interp_method
constexpr int INTERP_RUN = 2048;                     // consecutive outputs of one row per workgroup
// `batch` rows of n samples x_stride floats apart (0: one row read by every output
// row) at m positions per row -> rows of m outputs out_stride floats apart.
// Positions: pos not null -- rows of m floats pos_stride apart (0: one row for
// every signal row); pos null -- position k is (float)(start + (double)k * step),
// product and sum rounded separately.  n < 2^31.
struct InterpArgs {
    const float* x = nullptr;
    long long n = 0, batch = 0, x_stride = 0;
    const float* pos = nullptr;
    long long m = 0, pos_stride = 0;
    double start = 0.0, step = 0.0;
    float* out = nullptr;
    long long out_stride = 0;
};
// rows: signal rows one workgroup takes its run of positions through: 1, or
// INTERP_SHARED_ROWS where one position array serves every row (pos not null,
// pos_stride == 0), which reuses what each position decides
constexpr int INTERP_SHARED_ROWS = 8;
hipError_t launch_interp(const InterpArgs& a, int method, int rows, hipStream_t s);

// ---- LPC (lpc_kernels.hip), src/envelope/lpc.c ------------------------------
// The rows are described by a FrameSrc (above; rows of a batch have row_stride = len).
// Where the coefficient rows go: row (ch, f) = (row / frames, row % frames) at
// a + ch * a_ch_stride + f * (order + 1) and err + ch * err_ch_stride + f.
// flag (may be null): set to 1 when a row had r[0] <= 0.
struct LpcOut {
    float* a = nullptr;
    float* err = nullptr;
    long long frames = 0, a_ch_stride = 0, err_ch_stride = 0;
    int* flag = nullptr;
};
constexpr int LPC_WAVE_ORDER = 32;     // the wave kernel's orders and row lengths
constexpr int LPC_WAVE_LEN = 4096;
inline bool lpc_wave_supported(long long len, long long order) {
    return order <= LPC_WAVE_ORDER && len <= LPC_WAVE_LEN && order < len;
}
// wave kernel: autocorrelation rows into r [rows][order + 1] (r not null), or
// autocorrelation + Levinson into out; lpc_wave_supported shapes only
hipError_t launch_lpc_wave(const FrameSrc& src, int order, float* r, const LpcOut& out, hipStream_t s);
// any order < len: one workgroup per row, r [rows][order + 1]
hipError_t launch_autocorr_generic(const FrameSrc& src, long long order, float* r, hipStream_t s);
// r [rows][order + 1] -> out, the reference's recursion per row (lpc.c:24-38);
// generic 0 needs order <= LPC_WAVE_ORDER
hipError_t launch_levinson(const float* r, long long order, long long rows, int generic, const LpcOut& out,
                           hipStream_t s);
// a [batch][order + 1] -> mag [batch][nfft] = g / |1 -+ sum a[m] e^{-j 2 pi m k / nfft}|
// (plus 0: the reference's 1 - sum, lpc.c:60-69), g = gain[row] or gain1 when gain is null
hipError_t launch_lpspec(const float* a, long long order, const float* gain, float gain1, long long nfft,
                         long long batch, int plus, float* mag, hipStream_t s);

// ---- array statistics (stats_kernels.hip), src/core/core.c:42-108, stats.c:10-139 ----
// The rows are described by a FrameSrc (above).
// the outputs, in the order of vv_dsp_stats_out's members; bit k of a mask = output k
enum StatsBit : int {
    STATS_SUM, STATS_MEAN, STATS_VAR, STATS_RMS, STATS_MIN, STATS_MAX, STATS_CREST, STATS_SKEW, STATS_KURT,
    STATS_ZC, STATS_ARGMIN, STATS_ARGMAX, STATS_NOUT
};
constexpr int STATS_NFLOAT = 9;   // outputs [0, 9) are floats, [9, 12) uint32
// Value of row (ch, f) = (row / src.frames, row % src.frames) at p[k] + ch * ch_stride + f
// (rows that are not frames: at p[k] + row); p[k] null: output k not wanted.
struct StatsOut {
    void* p[STATS_NOUT] = {};
    long long ch_stride = 0;
    unsigned mask() const {
        unsigned m = 0;
        for (int k = 0; k < STATS_NOUT; ++k)
            if (p[k]) m |= 1u << k;
        return m;
    }
};
// outputs that need the f64 sum (and, from var on, the second pass about the mean)
constexpr unsigned STATS_MOMENT_MASK =
    1u << STATS_SUM | 1u << STATS_MEAN | 1u << STATS_VAR | 1u << STATS_SKEW | 1u << STATS_KURT;
constexpr unsigned STATS_CENTRAL_MASK = 1u << STATS_VAR | 1u << STATS_SKEW | 1u << STATS_KURT;
constexpr long long STATS_CHUNK = 4096;        // samples one wave reduces before its lanes combine
constexpr long long STATS_WAVE_LEN = 16384;    // rows up to here: one wave walks the row's chunks
// scratch of the long route: bytes per (row, chunk) and per row
size_t stats_part_bytes();
size_t stats_total_bytes();
// one wave per row (any len < 2^32; the shim sends len <= STATS_WAVE_LEN)
hipError_t launch_stats_wave(const FrameSrc& src, const StatsOut& out, hipStream_t s);
// one wave per (row, chunk), then the chunks' partial results combined per row in
// chunk order: the same sums in the same order as the wave kernel's.
// parts: rows * chunks * stats_part_bytes(), totals: rows * stats_total_bytes()
hipError_t launch_stats_long(const FrameSrc& src, const StatsOut& out, void* parts, void* totals, hipStream_t s);
// r [rows][r_len]: r[lag] = sum_i x[i] y[i + lag] in f64 over the `count` overlapping
// samples, over count (biased 0) or over nx (biased 1); 0 where count == 0.
// Rows of x / y are nx / ny floats apart.
hipError_t launch_xcorr(const float* x, long long nx, const float* y, long long ny, long long rows, long long r_len,
                        int biased, float* r, hipStream_t s);

// ---- per-frame pitch by YIN (pitch_kernels.hip), include/vv_dsp/features/pitch.h ----
// The rows are described by a FrameSrc (above).
constexpr long long PITCH_MAX_FRAME = 16384;     // samples of a row
constexpr int PITCH_MAX_LAG = 8191;              // tau_max
constexpr size_t PITCH_LDS_MAX = 128u << 10;     // the longest row as f32 and its lags as f64
// the lag range of a row of W + tau_max samples (shim_pitch.hip derives and checks
// it) and the parameters as the kernel compares with them
struct PitchCfg {
    double sample_rate = 0.0, threshold = 0.0;
    int tau_min = 0, tau_max = 0, W = 0;
};
// Value of row (ch, f) = (row / src.frames, row % src.frames) at plane + ch * ch_stride + f,
// its curve d'(0 .. tau_max) at cmnd + ch * cmnd_ch_stride + f * cmnd_row_stride (rows
// that are not frames: at plane + row and cmnd + row * cmnd_row_stride); null: not wanted.
struct PitchOut {
    float* f0 = nullptr;
    float* aperiodicity = nullptr;
    unsigned* lag = nullptr;
    float* cmnd = nullptr;
    long long ch_stride = 0, cmnd_ch_stride = 0, cmnd_row_stride = 0;
    bool any() const { return f0 || aperiodicity || lag || cmnd; }
};
// one wave per row, one launch; nothing wanted or no rows: nothing launched.
// The row sits in LDS as f64 where four rows fit 64 KiB, as f32 beyond or with
// f32_rows (knob PITCH_F32 = 1): the conversion is exact, the bits are the same.
hipError_t launch_pitch(const FrameSrc& src, const PitchCfg& cfg, const PitchOut& out, bool f32_rows, hipStream_t s);

// ---- f0 tracking over the YIN curves (pitch_track_kernels.hip), include/vv_dsp/features/pitch_track.h ----
constexpr int PTRACK_MAX_STEP = 126;             // VV_DSP_PITCH_TRACK_MAX_STEP: a predecessor code is one byte
constexpr int PTRACK_MAX_STATES = 4096;          // VV_DSP_PITCH_TRACK_MAX_STATES
constexpr int PTRACK_BLOCK = 64;                 // L: frames of predecessor rows the backtrace stages at most
struct PtrackCfg {
    double sample_rate = 0.0, lambda = 0.0, jump = 0.0, sw = 0.0, uc = 0.0;
    int tau_min = 0, tau_max = 0, B = 0;
    int S() const { return tau_max - tau_min + 1; }
};
// curves [nch][F][row_stride] (channels cmnd_ch_stride floats apart) -> planes [nch][F]
// (channels ch_stride values apart), cost [nch]; null: not wanted
struct PtrackArgs {
    const float* q = nullptr;
    long long nch = 0, F = 0, row_stride = 0, cmnd_ch_stride = 0, ch_stride = 0;
    unsigned* lag = nullptr;
    float* f0 = nullptr;
    float* aperiodicity = nullptr;
    double* cost = nullptr;
    // scratch of ptrack_scratch_bytes(): per channel F rows of predecessor bytes, F best
    // lags, the end state
    unsigned char* work = nullptr;
};
// bytes of a predecessor row: S voiced states and U, rounded up to 16
constexpr size_t ptrack_row_bytes(int S) { return ((size_t)S + 1 + 15) / 16 * 16; }
inline size_t ptrack_scratch_bytes(int S, long long nch, long long F) {
    return (size_t)nch * ((size_t)F * (ptrack_row_bytes(S) + 4) + 16);
}
// frames per staged block of the backtrace: PTRACK_BLOCK where that many rows fit 60 KiB
constexpr int ptrack_block(int S) {
    return (int)((60u << 10) / ptrack_row_bytes(S)) < PTRACK_BLOCK ? (int)((60u << 10) / ptrack_row_bytes(S))
                                                                    : PTRACK_BLOCK;
}
// forward pass (one wave per channel up to 64 states, one workgroup beyond) and
// backtrace on stream s; nch > 0, F > 0, checked sizes
hipError_t launch_pitch_track(const PtrackCfg& cfg, const PtrackArgs& a, hipStream_t s);

// ---- LSF and formants of LPC rows (lsf_kernels.hip, formant_kernels.hip),
// include/vv_dsp/envelope/lsf.h and include/vv_dsp/features/formant.h ----
constexpr int LSF_MAX_ORDER = 32;   // VV_DSP_LSF_MAX_ORDER = VV_DSP_FORMANT_MAX_ORDER
// a [rows] a_pitch floats apart -> lsf, rc [rows][order], flags [rows]; null: not wanted.
// One wave per row; 1 <= order <= LSF_MAX_ORDER, rows > 0.
hipError_t launch_lpc_to_lsf(const float* a, int order, long long rows, long long a_pitch, float* lsf, float* rc,
                             int* flags, hipStream_t s);
// lsf [rows][order] -> a [rows] a_pitch floats apart; one wave per row
hipError_t launch_lsf_to_lpc(const float* lsf, int order, long long rows, float* a, long long a_pitch, hipStream_t s);
struct FormantCfg {
    double sample_rate = 0.0, f_min = 0.0, f_max = 0.0, bw_max = 0.0;
    int n_formants = 0;
    double start[2 * LSF_MAX_ORDER];   // vvhip_formant_start_points(order)
};
struct FormantOut {
    float* freq = nullptr;
    float* bw = nullptr;
    int* count = nullptr;
    int* flags = nullptr;
    double* roots = nullptr;
};
// a [rows] a_pitch floats apart -> the planes of out, packed by row.  One lane
// per root, 8 / 4 / 2 rows per wave for orders up to 8 / 16 / 32.
hipError_t launch_formants(const float* a, int order, long long rows, long long a_pitch, const FormantCfg& cfg,
                           const FormantOut& out, hipStream_t s);

// ---- LPC residual and synthesis filters (lpc_filter_kernels.hip),
// include/vv_dsp/envelope/lpc_filter.h ----
constexpr int LPCF_MAX_ORDER = 32;                // VV_DSP_LPC_FILTER_MAX_ORDER
constexpr long long LPCF_EXACT_MAX = 8192;        // VV_DSP_LPC_SYNTH_EXACT_MAX
constexpr long long LPCF_CHUNK = 1024;            // VV_DSP_LPC_SYNTH_CHUNK
constexpr int LPCF_TILE = 1024;                   // samples of a channel per workgroup of the residual
// The signal [rows][n] and what governs it: row r reads coefficient rows
// a + r * a_ch_stride + f * a_pitch and gains gain + r * g_ch_stride + f (gain
// null: 1), f = clamp((t + offset) / seg_len, 0, frames - 1); state [rows][order]
// doubles, null: zeros in and nothing out.
struct LpcFilt {
    const float* x = nullptr;
    float* y = nullptr;
    long long n = 0, rows = 0, x_stride = 0, y_stride = 0;
    const float* a = nullptr;
    const float* gain = nullptr;
    long long frames = 0, a_pitch = 0, a_ch_stride = 0, g_ch_stride = 0, seg_len = 1, offset = 0;
    int order = 0;
    double* state = nullptr;
};
// residual: one workgroup per tile of LPCF_TILE samples of a row, then the state update
hipError_t launch_lpc_residual(const LpcFilt& f, hipStream_t s);
// The synthesis walk over rows * chunks sub-rows, one lane each: sub-row q = row *
// chunks + c is samples [c L, min(n, (c + 1) L)) and starts from zin[q * order + ..]
// (zin null: from f.state[row], chunks == 1); the last sub-row of a row leaves its
// end state in f.state[row].  This is the header's recursion, bit for bit.
hipError_t launch_lpc_synth_walk(const LpcFilt& f, long long chunks, long long L, const double* zin, hipStream_t s);
// per sub-row: the end state from zero state, z [q][order], and the transition
// phi [q][order (unit state i)][order (component r)]; one wave per sub-row
hipError_t launch_lpc_synth_phi(const LpcFilt& f, long long chunks, long long L, double* phi, double* z, hipStream_t s);
// per row: s_0 = f.state[row] (null: 0), s_{c+1} = phi_c s_c + z_c; zin[q][order] = s_c
hipError_t launch_lpc_synth_scan(const LpcFilt& f, long long chunks, const double* phi, const double* z, double* zin,
                                 hipStream_t s);

// ---- per-frame spectral shape (shape_kernels.hip), include/vv_dsp/features/spectral_shape.h ----
constexpr int SHAPE_MAX_BINS = 8193;             // K = n_fft / 2 + 1 of a row
// the outputs, in the order of vv_dsp_spectral_shape_out's members; bit k of a mask = output k
enum ShapeBit : int {
    SHAPE_ENERGY, SHAPE_CENTROID, SHAPE_SPREAD, SHAPE_SKEW, SHAPE_KURT, SHAPE_FLATNESS, SHAPE_ROLLOFF, SHAPE_FLUX,
    SHAPE_CREST, SHAPE_PEAK, SHAPE_NOUT
};
// the parameters as the kernel uses them (shim_shape.hip checks them)
struct ShapeCfg {
    int K = 0, k_min = 0, k_max = 0, magnitude = 0;
    double sample_rate = 0.0, n_fft = 0.0, rolloff = 0.0;
    float floor = 0.0f;
};
// Value of row r = g * rows_per_group + f at p[k] + g * group_stride + f; p[k] null: not wanted.
struct ShapeOut {
    void* p[SHAPE_NOUT] = {};
    long long group_stride = 0;
    unsigned mask() const {
        unsigned m = 0;
        for (int k = 0; k < SHAPE_NOUT; ++k)
            if (p[k]) m |= 1u << k;
        return m;
    }
};
// `rows` rows of cfg.K weights, row_pitch floats apart, in groups of rows_per_group
// (> 0) consecutive rows: one wave per run of rows of one group, one launch;
// nothing wanted or no rows: nothing launched.  dword (knob SHAPE_DWORD = 1):
// 4-byte loads even where the rows allow 16-byte ones (the same bits).
// whether rows at this base and pitch can be loaded 16 bytes at a time (every row 16-byte aligned)
bool shape_rows_vec16(const float* rows_ptr, long long row_pitch);
hipError_t launch_shape(const float* rows_ptr, long long rows, long long row_pitch, long long rows_per_group,
                        const ShapeCfg& cfg, const ShapeOut& out, bool dword, hipStream_t s);

// ---- phase vocoder (pvoc_kernels.hip), include/vv_dsp/spectral/phase_vocoder.h ----
constexpr int PVOC_SEGMENT = 32;                  // VV_DSP_PVOC_SEGMENT: output rows per segment of the phase sum
constexpr long long PVOC_MAX_FFT = 1ll << 24;     // VV_DSP_PVOC_MAX_FFT
constexpr float PVOC_NORM_FLOOR = 1e-8f;          // VV_DSP_PVOC_NORM_FLOOR
struct PvocArgs {
    const float2* in = nullptr;    // [nch][T][n_fft], channels in_ch_stride apart
    float2* out = nullptr;         // [nch][m][n_fft], channels out_ch_stride apart
    long long T = 0, n_fft = 0, nch = 0, m = 0, in_ch_stride = 0, out_ch_stride = 0;
    const float* pos = nullptr;    // m positions, or null: start + j * step
    double start = 0.0, step = 0.0;
    // scratch of pvoc_scratch_doubles(): [nch][nseg][K] segment totals, which the
    // scan turns into the segments' bases, then [nch][K] the phase of row 0
    double* work = nullptr;
    // null, or [nch][T][K] doubles for the rows' phases (knob PVOC_PLANE)
    const double* plane = nullptr;
};
constexpr long long pvoc_segments(long long m) { return (m + PVOC_SEGMENT - 1) / PVOC_SEGMENT; }
inline size_t pvoc_scratch_doubles(long long n_fft, long long nch, long long m) {
    return (size_t)nch * (size_t)(n_fft / 2 + 1) * (size_t)(pvoc_segments(m) + 1);
}
// whether one launch takes these sizes (the header's check 4 and the grid's limits)
bool pvoc_supported(long long T, long long n_fft, long long nch, long long m);
// whether the phase plane's kernel takes these sizes
bool pvoc_plane_supported(long long T, long long n_fft, long long nch);
// totals, scan, rows on stream s; m > 0, nch > 0, supported sizes
hipError_t launch_pvoc(const PvocArgs& a, hipStream_t s);
// y[c][i] = norm[c][i] > PVOC_NORM_FLOOR ? y[c][i] / norm[c][i] : 0 for i < len (norm rows contiguous)
hipError_t launch_pvoc_normalize(float* y, long long y_stride, const float* norm, long long len, long long nch,
                                 hipStream_t s);

// ---- running median and HPSS (median_kernels.hip), include/vv_dsp/filter/median.h,
// include/vv_dsp/spectral/hpss.h ----
constexpr int MED_MAX_WINDOW = 127;               // VV_DSP_MEDFILT_MAX_WINDOW
constexpr int MED_TILE = 256;                     // positions of a line per block (row direction)
constexpr int MED_RUN = 64;                       // rows of a group per block (column direction)
constexpr int MED_RADIX_FROM = 33;                // windows from here on: the bitwise select
constexpr int HPSS_MAX_BINS = 8193;               // VV_DSP_HPSS_MAX_BINS
enum MedMode : int { MED_REFLECT, MED_NEAREST, MED_ZERO };
enum HpssMask : int { HPSS_HARD, HPSS_SOFT, HPSS_WIENER };
// One launch of either direction.  Values x[line * x_pitch + i], i < n, lines in
// groups of rpg (> 0) consecutive lines; sqrt_w: the value is sqrtf(x).  Row
// direction: the window runs along i.  Column direction: along the lines of a group.
struct MedArgs {
    const float* x = nullptr;
    long long lines = 0, n = 0, x_pitch = 0, rpg = 0;
    int L = 1, mode = MED_REFLECT, sqrt_w = 0, radix = 0;
    float* y = nullptr;            // the medians [line * y_pitch + i], or null (row direction with masks)
    long long y_pitch = 0;
    // row direction with masks: the other median H [line * h_pitch + i] is read and the
    // masks that are wanted are written at y_pitch
    const float* H = nullptr;
    long long h_pitch = 0;
    float *mask_h = nullptr, *mask_p = nullptr;
    double margin_h = 1.0, margin_p = 1.0;
    int mask = HPSS_HARD;
};
// whether one launch takes these counts (flat grids below 2^31 blocks)
bool med_rows_supported(long long lines, long long n);
bool med_cols_supported(long long lines, long long n, long long rpg);
hipError_t launch_med_rows(const MedArgs& a, hipStream_t s);
hipError_t launch_med_cols(const MedArgs& a, hipStream_t s);
// spec rows [rows][n_fft] float pairs times mask [rows][K] (bin j >= K by mask[n_fft - j]) -> out
hipError_t launch_hpss_apply(const float2* spec, const float* mask, float2* out, long long rows, long long n_fft,
                             hipStream_t s);

// ---- spectral noise suppression (denoise_kernels.hip), include/vv_dsp/spectral/denoise.h ----
constexpr int DN_MAX_SMOOTH = 64;                 // VV_DSP_DENOISE_MAX_SMOOTH
constexpr int DN_MAX_REACH = 511;                 // VV_DSP_DENOISE_MAX_REACH
constexpr int DN_THREADS = 512;                   // eight waves share one halo of smoothed rows
constexpr int DN_DIRECT_BELOW = 64;               // windows below this: the direct minimum, else blockwise
enum DenoiseMode : int { DN_GATE, DN_WIENER, DN_SUBTRACT };
// One launch.  Powers p[row * p_pitch + k], k < K, rows in groups of rpg (> 0) consecutive rows.
// seg (0: chosen by the launcher) is the segment length L; direct: 1 the direct minimum, 0 blockwise.
struct DenoiseArgs {
    const float* p = nullptr;
    long long rows = 0, K = 0, p_pitch = 0, rpg = 0;
    int W = 1, back = 0, ahead = 0, mode = DN_WIENER;
    double bias = 1.0, floor = 0.0;               // (double) of the float parameters
    float *smooth = nullptr, *noise = nullptr, *gain = nullptr;   // each null (not wanted) or [row * o_pitch + k]
    long long o_pitch = 0;
    int seg = 0, direct = 0;
};
hipError_t launch_denoise(const DenoiseArgs& a, hipStream_t s);

// ---- biquad cascade (iir_kernels.hip), src/filter/iir.c:21-43 -----------------
constexpr int IIR_MAX_STAGES = 8;        // stages one walk holds in registers; longer cascades run in groups
constexpr int IIR_TILE = 32;             // samples of a sub-row per LDS tile: one 128 B line
constexpr long long IIR_EXACT_MAX = 8192;   // rows up to here run as one recurrence (N0)
constexpr long long IIR_CHUNK_LEN = 1024;   // chunk length of longer rows (L)
// One walk over rows * chunks sub-rows: sub-row (row, c) is samples [c L, min(n, (c + 1) L))
// of row `row`.  coef [stages][5] = b0 b1 b2 a1 a2 (device).  Sub-row q = row * chunks + c
// starts from zin[q * zin_stride + 2 s + {0, 1}] (zin null: zero).  write_y 0: no
// output, final state of every sub-row to zout[q * zout_stride + ..]; write_y 1: y
// written, and the final state of each row's last chunk to zout[row * zout_stride + ..]
// (zout null: none).
struct IirWalk {
    const float* x = nullptr;
    float* y = nullptr;
    long long n = 0, rows = 0, chunks = 1, L = 0, x_stride = 0, y_stride = 0;
    const float* coef = nullptr;
    const float* zin = nullptr;
    float* zout = nullptr;
    long long zin_stride = 0, zout_stride = 0;
};
hipError_t launch_iir_walk(const IirWalk& w, int stages, int write_y, hipStream_t s);
// phi [2 stages][2 stages] (f64, row-major): the cascade's L-step state transition,
// from the float coefficients by the homogeneous recurrence on unit states
hipError_t launch_iir_phi(const float* coef, int stages, long long L, double* phi, hipStream_t s);
// per row: z_0 = the row's incoming state (zrow [rows][zrow_stride], null: zero),
// z_{c+1} = phi z_c + zs_c in f64; zin[(row * chunks + c) * 2 stages + i] = (float)z_c
hipError_t launch_iir_scan(const double* phi, int stages, const float* zs, const float* zrow, long long zrow_stride,
                           long long rows, long long chunks, float* zin, hipStream_t s);

// ---- Savitzky-Golay (savgol_kernels.hip), src/filter/savgol.c:164-217 ---------
constexpr int SAVGOL_MAX_WINDOW = 257;
// h: m coefficients in host memory (passed as kernel arguments); flag (device int,
// policy 2 only): bit 0 a NaN/Inf sample read, bit 1 a NaN/Inf output
hipError_t launch_savgol(const float* x, long long n, long long batch, long long x_stride, const float* h, int m,
                         int mode, int policy, float* y, long long y_stride, int* flag, hipStream_t s);

// ---- DCT / Hilbert helpers (spectral_kernels.hip) ----------------------
// single-pass analytic signal / DCT-II (analytic_kernels.hip: hilbert_fused.hpp, dct2_fused.hpp): rows [batch][n]
bool hilbert_fused_supported(long long n);
hipError_t launch_hilbert_fused(long long n, const float* x, float2* z, long long batch, hipStream_t s);
// instantaneous phase / frequency rows (phase_kernels.hip, hilbert.c:77-113)
hipError_t launch_inst_phase(const float2* z, long long n, long long batch, float* phase, hipStream_t s);
hipError_t launch_phase_unwrap(const float* p, long long n, long long batch, float* out, hipStream_t s);
// spectral_utils_kernels.hip (src/spectral/utils.c)
hipError_t launch_fftshift(const void* in, void* out, long long n, long long batch, int cpx, int inverse,
                           hipStream_t s);
hipError_t launch_phase_wrap(const float* in, float* out, long long count, hipStream_t s);
hipError_t launch_inst_freq(const float* phase, long long n, long long batch, double scale, float* freq,
                            hipStream_t s);
bool dct2_fused_supported(long long n);
hipError_t launch_dct2_fused(long long n, const float* x, float* X, long long batch, int policy, hipStream_t s);
hipError_t launch_hilbert_mask(long long n, const float2* half, float2* full, long long batch,
                               long long half_dist, hipStream_t s);
hipError_t launch_dct2_pre(long long n, const float* x, float* v, long long batch, hipStream_t s);
hipError_t launch_dct2_post(long long n, const float2* V, float* X, long long batch,
                            const float2* tw4n, hipStream_t s);
hipError_t launch_dct3_pre(long long n, const float* X, float2* V, long long batch,
                           const float2* tw4n, hipStream_t s);
hipError_t launch_dct3_post(long long n, const float* v, float* x, long long batch, float scale,
                            hipStream_t s);
hipError_t launch_dct_naive(long long n, int type, int dir, const float* in, float* out,
                            long long batch, hipStream_t s);
hipError_t launch_nan_policy(float* p, long long count, int policy, int* flag, hipStream_t s);
// chirp_glue.hip: the element-wise stages of a chirp convolution through a
// p-point FFT pair (Bluestein, bluestein.hip; the chirp-z transform, czt.c:58-178)
//   pre:  u[r][i] = x[r][i] * tab[i] for i < n, 0 for n <= i < p (real_in: x is float rows)
//   cmul: a[r][i] *= B[i] (also the long FIR's product with H)
//   post: X[r][k] = y[r][off + k] * tab[k], k < nout; _scaled: times scale, rounded after the product
hipError_t launch_chirp_pre(const void* x, int real_in, long long n, long long p, long long rows, long long in_dist,
                            const float2* tab, float2* u, hipStream_t s);
hipError_t launch_cmul_rows(float2* a, const float2* B, long long p, long long rows, hipStream_t s);
hipError_t launch_chirp_post(const float2* y, long long off, long long p, long long nout, long long rows,
                             const float2* tab, float2* X, long long out_dist, hipStream_t s);
hipError_t launch_chirp_post_scaled(const float2* y, long long off, long long p, long long nout, long long rows,
                                    const float2* tab, float2* X, long long out_dist, float scale, hipStream_t s);
// ceps_stages.hip: the cepstrum family's element-wise stages (cepstrum.c, minphase.c)
hipError_t launch_log_magnitude(float2* Y, long long count, hipStream_t s);
hipError_t launch_cepstrum_fold(const float* c, long long n, long long rows, float2* C, hipStream_t s);
hipError_t launch_exp_real(float2* H, long long count, int dbl, hipStream_t s);
// czt_kernels.hip (czt_fused.hpp, ceps_fused.hpp):
// the whole chirp-z chain in one kernel for P <= 4096 (Bs = FFT_P(b) / P)
bool czt_fused_supported(long long p);
// the cepstrum family in one pass per row for pow2 n <= 4096 (kind 0 cepstrum,
// 1 icepstrum_minphase, 2 minphase_from_cepstrum with complex output rows)
bool ceps_fused_supported(long long n);
hipError_t launch_ceps_fused(int kind, long long n, const float* x, long long rows, float* y, hipStream_t s);
hipError_t launch_czt_fused(long long p, const void* x, int real_in, long long n, long long m, long long rows,
                            const float2* g, const float2* Bs, const float2* post, float2* X, hipStream_t s);

}  // namespace vvh
