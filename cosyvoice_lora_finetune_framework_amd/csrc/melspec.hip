// melspec.hip -- the mel front-end (include/cvft.h, "Mel front-end"): waveform -> log-mel in one launch.  The 1024-point
// Hann DFT is a GEMM on the fp32-input matrix cores against a host-built table, the magnitude is formed in registers,
// the filterbank is a second small product per 16-bin chunk, and clamp / log / store are the epilogue.
#include "common.h"

#define MS_NFFT 1024
#define MS_HOP 256
#define MS_REFLECT 384                                  // (n_fft - hop) / 2 samples of reflect padding per side
#define MS_NMEL 80
#define MS_MT (MS_NMEL / 16)                            // band tiles of the filterbank product
#define MS_NT 4                                         // frame tiles per workgroup
#define MS_F (16 * MS_NT)                               // frames per workgroup
#define MS_SPAN (MS_HOP * (MS_F - 1) + MS_NFFT)         // padded samples the tile's frames cover (17152)
#define MS_BPITCH (MS_HOP + 4)                          // a 256-sample block is stored 260 floats apart: see below
#define MS_SIG (MS_SPAN / MS_HOP * MS_BPITCH)           // floats of the sample image
#define MS_WAVES 8
#define MS_THREADS (64 * MS_WAVES)
#define MS_MPITCH (MS_NMEL + 1)                         // mel image [frame][band], read both ways by the epilogue
#define MS_LDS_BYTES (MS_SIG * 4)
#define MS_MAX_CHUNKS 33                                // 513 bins in chunks of 16
#define MS_CLAMP 1e-5f
#define MS_LOG_CLAMP (-0x1.7069e2p+3f)                  // fp32(log(fp32(1e-5))) = -11.512925...: the clamped value's log

static_assert(MS_F * MS_MPITCH <= MS_SIG, "the mel image reuses the sample image");

// Sample image: padded sample j of the tile lives at j + 4 * (j >> 8).  Frame f reads j = 256 f + n, so for one n the 16
// frames of a tile sit 260 floats = 4 banks apart: the ds_read_b128 of a frame tile is conflict-free.  The k order of the
// DFT sum is permuted so that the four lane groups of an MFMA step read n 64 apart (the same banks, other frames' rows):
// step s of 64, lane group g, element e  ->  n = 256 (s >> 4) + 64 g + 4 (s & 15) + e.  The table is packed to match.
__global__ __launch_bounds__(MS_THREADS) void melspec_kernel(int Lmax, int ldw, const float* __restrict__ wav,
                                                             const int* __restrict__ len, const f32x4* __restrict__ tab,
                                                             const f32x4* __restrict__ basis, int nchunks, int Tmax,
                                                             int channel_last, float pad_value, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float ms_sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, fr = lane & 15;
    const int b = blockIdx.y, t0 = blockIdx.x * MS_F;
    const int L = min(len ? len[b] : Lmax, Lmax);
    const int T = L > MS_REFLECT ? min(L / MS_HOP, Tmax) : 0;
    const int nvalid = min(max(T - t0, 0), MS_F);

    if (nvalid > 0) {
        // ---- stage the tile's samples once, reflect map applied here; samples no valid frame reads are zero
        const float* w = wav + (size_t)b * ldw;
        const int p0 = t0 * MS_HOP;
        for (int q = tid; q < MS_SPAN; q += MS_THREADS) {
            const int p = p0 + q;
            float v = 0.f;
            if (p < L + 2 * MS_REFLECT) {
                int s = p - MS_REFLECT;
                s = s < 0 ? -s : (s >= L ? 2 * (L - 1) - s : s);
                v = w[s];
            }
            ms_sm[q + 4 * (q >> 8)] = v;
        }
        __syncthreads();

        f32x4 mel[MS_MT][MS_NT];
#pragma unroll
        for (int mt = 0; mt < MS_MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < MS_NT; ++nt) mel[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* sb = ms_sm + MS_BPITCH * fr + 64 * g;

        for (int c = wave; c < nchunks; c += MS_WAVES) {
            // ---- DFT of bins 16c .. 16c+15 for the tile's 64 frames: rows = bins (table), columns = frames (LDS)
            f32x4 re[MS_NT], im[MS_NT];
#pragma unroll
            for (int nt = 0; nt < MS_NT; ++nt) re[nt] = im[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4* tc = tab + (size_t)c * (64 * 2 * 64) + lane;
            f32x4 ca = tc[0], sa = tc[64];
#pragma unroll 2
            for (int s = 0; s < 64; ++s) {
                const int sn = s < 63 ? s + 1 : s;
                const f32x4 ca_n = tc[sn * 128], sa_n = tc[sn * 128 + 64];
                const float* sp = sb + MS_BPITCH * (s >> 4) + 4 * (s & 15);
                f32x4 x[MS_NT];
#pragma unroll
                for (int nt = 0; nt < MS_NT; ++nt) x[nt] = *reinterpret_cast<const f32x4*>(sp + nt * 16 * MS_BPITCH);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int nt = 0; nt < MS_NT; ++nt) {
                        re[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[e], x[nt][e], re[nt], 0, 0, 0);
                        im[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa[e], x[nt][e], im[nt], 0, 0, 0);
                    }
                ca = ca_n;
                sa = sa_n;
            }
            // ---- magnitude in registers: lane holds bins 16c + 4g + i of frames nt*16 + fr, which is the B operand of
            // the filterbank product with k = bin (step i takes bin 4g + i from lane group g; the basis is packed alike)
#pragma unroll
            for (int nt = 0; nt < MS_NT; ++nt)
#pragma unroll
                for (int i = 0; i < 4; ++i) re[nt][i] = sqrtf(re[nt][i] * re[nt][i] + im[nt][i] * im[nt][i] + 1e-9f);
#pragma unroll
            for (int mt = 0; mt < MS_MT; ++mt) {
                const f32x4 bw = basis[((size_t)c * MS_MT + mt) * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int nt = 0; nt < MS_NT; ++nt)
                        mel[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[i], re[nt][i], mel[mt][nt], 0, 0, 0);
            }
        }

        // ---- the waves' partial band sums, added in wave order (fixed, so results are bit-identical run to run)
        __syncthreads();
        for (int wv = 0; wv < MS_WAVES; ++wv) {
            if (wave == wv) {
#pragma unroll
                for (int mt = 0; mt < MS_MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < MS_NT; ++nt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float* p = ms_sm + (nt * 16 + fr) * MS_MPITCH + mt * 16 + g * 4 + i;
                            *p = wv == 0 ? mel[mt][nt][i] : *p + mel[mt][nt][i];
                        }
            }
            __syncthreads();
        }
    }

    // ---- clamp, log, store; frames past the row's own count get pad_value
    for (int e = tid; e < MS_F * MS_NMEL; e += MS_THREADS) {
        const int fl = channel_last ? e / MS_NMEL : e % MS_F, band = channel_last ? e % MS_NMEL : e / MS_F;
        const int t = t0 + fl;
        if (t >= Tmax) continue;
        float v = pad_value;
        if (fl < nvalid) {
            const float m = ms_sm[fl * MS_MPITCH + band];
            v = m > MS_CLAMP ? logf(m) : MS_LOG_CLAMP;
        }
        out[channel_last ? ((size_t)b * Tmax + t) * MS_NMEL + band : ((size_t)b * MS_NMEL + band) * Tmax + t] = v;
    }
}

extern "C" int cvft_melspec(int B, int Lmax, int ldw, const float* wav, const int* len, const float* dft_tab,
                            const float* basis_tab, int nchunks, int Tmax, int channel_last, float pad_value, float* out,
                            void* stream) {
    CVFT_CHECK_ARG(B >= 1 && B <= 65535, "cvft_melspec: B=%d outside [1, 65535]", B);
    CVFT_CHECK_ARG(Lmax > MS_REFLECT && Lmax <= (1 << 30) && ldw >= Lmax,
                   "cvft_melspec: Lmax=%d ldw=%d (reflect padding needs >= %d samples)", Lmax, ldw, MS_REFLECT + 1);
    CVFT_CHECK_ARG(Tmax >= 1 && Tmax <= (1 << 23) && nchunks >= 1 && nchunks <= MS_MAX_CHUNKS,
                   "cvft_melspec: Tmax=%d nchunks=%d", Tmax, nchunks);
    CVFT_CHECK_ARG(wav && dft_tab && basis_tab && out, "cvft_melspec: null pointer");
    CVFT_CHECK_ARG(((uintptr_t)dft_tab & 15) == 0 && ((uintptr_t)basis_tab & 15) == 0, "cvft_melspec: tables must be 16-byte aligned");
    static int ready = 0;
    if (!ready) {
        CVFT_HIP_CHECK_RET(hipFuncSetAttribute((const void*)melspec_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MS_LDS_BYTES),
                           "cvft_melspec: reserving LDS");
        ready = 1;
    }
    hipLaunchKernelGGL(melspec_kernel, dim3((Tmax + MS_F - 1) / MS_F, B), dim3(MS_THREADS), MS_LDS_BYTES, (hipStream_t)stream, Lmax,
                       ldw, wav, len, reinterpret_cast<const f32x4*>(dft_tab), reinterpret_cast<const f32x4*>(basis_tab), nchunks,
                       Tmax, channel_last, pad_value, out);
    CVFT_LAUNCH_CHECK("cvft_melspec");
    return 0;
}
