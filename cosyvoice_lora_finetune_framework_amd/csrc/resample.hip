// resample.hip -- the polyphase resampler (include/cvft.h, "Resampler"): torchaudio's default sinc_interp_hann filter on
// a host-built compact tap table.  Bandwidth-bound (4 B in, 4 B out and a few tens of FMAs per sample), so the sums are
// plain fp32 FMAs on operands staged in LDS; no matrix cores, no atomics.
#include "common.h"

#define RS_TILE CVFT_RESAMPLE_TILE                      // consecutive output samples of one row per workgroup
#define RS_THREADS 256
#define RS_MAX_TAPS CVFT_RESAMPLE_MAX_TAPS              // floats of the compact table, n * span
#define RS_MAX_WINDOW CVFT_RESAMPLE_MAX_WINDOW          // floats of a tile's input window
#define RS_MAX_LDS (128 * 1024)                         // of the CU's 160 KB

// padded samples a tile's outputs can read: phases j0 .. jl with jl - j0 <= (RS_TILE - 1) / n + 1, each reading dense
// columns [j o, j o + 2 width + o)
static inline long long rs_window(int o, int n, int width) { return ((long long)(RS_TILE - 1) / n + 1) * o + 2LL * width + o; }
static inline long long rs_round4(long long v) { return (v + 3) & ~3LL; }

// LDS: taps [n][pitch] (pitch = span | 1: neighbouring lanes hold neighbouring phases, an odd pitch keeps their reads
// on distinct banks) | first [n] | the input window.  The window image starts at the 16-byte-aligned sample at or below
// the tile's first padded sample, so quads that lie inside the row are moved as one 16-byte load and one 16-byte write.
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(int Lmax, int ldw, const float* __restrict__ wav,
                                                              const int* __restrict__ len, int o, int n, int width, int span,
                                                              int pitch, const int* __restrict__ first,
                                                              const float* __restrict__ taps, int Mmax, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rs_sm[];
    const int tid = threadIdx.x;
    const int b = blockIdx.y, m0 = blockIdx.x * RS_TILE;
    const int L = min(max(len ? len[b] : Lmax, 0), Lmax);
    const int Mb = (int)min(((long long)n * L + o - 1) / o, (long long)Mmax);
    const int ntile = min(RS_TILE, Mmax - m0), nvalid = min(max(Mb - m0, 0), RS_TILE);
    float* y = out + (size_t)b * Mmax + m0;

    if (nvalid > 0) {
        float* tp = rs_sm;
        int* fs = reinterpret_cast<int*>(rs_sm + n * pitch);
        float* img = rs_sm + ((n * pitch + n + 3) & ~3);
        for (int i = tid / span, k = tid % span; i < n;) {
            tp[i * pitch + k] = taps[i * span + k];
            k += RS_THREADS % span;
            i += RS_THREADS / span;
            if (k >= span) { k -= span; ++i; }
        }
        for (int i = tid; i < n; i += RS_THREADS) fs[i] = min(max(first[i], 0), 2 * width + o - span);

        // ---- the tile's input window; every sample outside [0, L) is zero and nothing outside it is read
        const int j0 = m0 / n, jl = (m0 + nvalid - 1) / n;
        const int W = (jl - j0) * o + 2 * width + o;
        const int gs = j0 * o - width;                              // sample index of padded sample j0 * o
        const int a = gs & ~3, sh = gs - a;                         // (two's complement: rounds down for gs < 0 too)
        const float* w = wav + (size_t)b * ldw;
        const bool vec = (reinterpret_cast<uintptr_t>(w) & 15) == 0;
        for (int q = tid; 4 * q < W + sh; q += RS_THREADS) {
            const int s = a + 4 * q;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (vec && s >= 0 && s + 3 < L) {
                v = *reinterpret_cast<const f32x4*>(w + s);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (s + e >= 0 && s + e < L) v[e] = w[s + e];
            }
            *reinterpret_cast<f32x4*>(img + 4 * q) = v;
        }
        __syncthreads();

        // ---- output m = j n + i: span FMAs in ascending k over taps[i] and padded samples j o + first[i] + k
        const float* win = img + sh;
        const int dq = RS_THREADS / n, dr = RS_THREADS % n;
        int j = (m0 + tid) / n, i = (m0 + tid) - j * n;
        for (int r = tid; r < nvalid; r += RS_THREADS) {
            const float* t = tp + i * pitch;
            const float* x = win + (j - j0) * o + fs[i];
            float acc = 0.f;
            for (int k = 0; k < span; ++k) acc = fmaf(t[k], x[k], acc);
            y[r] = acc;
            i += dr;
            j += dq;
            if (i >= n) { i -= n; ++j; }
        }
    }
    for (int r = nvalid + tid; r < ntile; r += RS_THREADS) y[r] = 0.f;
}

extern "C" int cvft_resample(int B, int Lmax, int ldw, const float* wav, const int* len, int o, int n, int width, int span,
                             const int* first, const float* taps, int Mmax, float* out, void* stream) {
    CVFT_CHECK_ARG(B >= 1 && B <= 65535, "cvft_resample: B=%d outside [1, 65535]", B);
    CVFT_CHECK_ARG(o >= 1 && n >= 1 && width >= 1 && o <= (1 << 20) && n <= (1 << 20) && width <= (1 << 20),
                   "cvft_resample: o=%d n=%d width=%d", o, n, width);
    CVFT_CHECK_ARG(span >= 1 && span <= 2 * width + 1, "cvft_resample: span=%d outside [1, 2 * width + 1 = %d]", span,
                   2 * width + 1);
    CVFT_CHECK_ARG((long long)n * span <= RS_MAX_TAPS, "cvft_resample: n * span = %lld floats of taps exceed the budget of %d",
                   (long long)n * span, RS_MAX_TAPS);
    const long long window = rs_window(o, n, width);
    CVFT_CHECK_ARG(window <= RS_MAX_WINDOW, "cvft_resample: a tile's input window of %lld samples (o=%d n=%d) exceeds %d",
                   window, o, n, RS_MAX_WINDOW);
    const int pitch = span | 1;
    const long long lds = 4 * (rs_round4((long long)n * pitch + n) + rs_round4(window + 3));
    CVFT_CHECK_ARG(lds <= RS_MAX_LDS, "cvft_resample: %lld bytes of LDS (o=%d n=%d span=%d) exceed %d", lds, o, n, span, RS_MAX_LDS);
    CVFT_CHECK_ARG(Lmax >= 1 && Lmax <= (1 << 30) && ldw >= Lmax && Mmax >= 1 && Mmax <= (1 << 30),
                   "cvft_resample: Lmax=%d ldw=%d Mmax=%d", Lmax, ldw, Mmax);
    // the largest padded-sample index a thread forms: (Mmax / n + 1) * o + 2 * width + o
    CVFT_CHECK_ARG(((long long)Mmax / n + 2) * o + 2LL * width < (1LL << 31),
                   "cvft_resample: Mmax=%d o=%d n=%d: a sample index would pass 2^31", Mmax, o, n);
    CVFT_CHECK_ARG(wav && first && taps && out, "cvft_resample: null pointer");
    static int ready = 0;
    if (!ready) {
        CVFT_HIP_CHECK_RET(hipFuncSetAttribute((const void*)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RS_MAX_LDS),
                           "cvft_resample: reserving LDS");
        ready = 1;
    }
    hipLaunchKernelGGL(resample_kernel, dim3((Mmax + RS_TILE - 1) / RS_TILE, B), dim3(RS_THREADS), (size_t)lds, (hipStream_t)stream,
                       Lmax, ldw, wav, len, o, n, width, span, pitch, first, taps, Mmax, out);
    CVFT_LAUNCH_CHECK("cvft_resample");
    return 0;
}
