// feat16k.hip -- the 16 kHz front-ends (include/cvft.h, "16 kHz front-ends"): waveform -> the speech tokenizer's Whisper
// log-mel and the speaker encoder's Kaldi fbank.  Both are frames of 400 samples at hop 160, so one templated kernel in the
// shape of melspec.hip serves both: the frame's DFT is a k = 400 GEMM on the fp32-input matrix cores against a host-built
// table (for the fbank the table also carries mean removal, pre-emphasis and the Povey window, and the zero padding to 512
// drops out of the sum), the power is formed in registers, the filterbank is a second small product per 16-bin chunk, and
// floor / log / store are the epilogue.  Each feature ends in a reduction across a row's frames (whisper: the row's
// maximum; fbank: the per-band mean), so the main launch leaves one partial per workgroup and a small second launch
// finishes the row.  No atomics; every sum's order depends on the frame or the row alone.
#include "common.h"

#define FK_FRAME CVFT_FEAT16K_FRAME
#define FK_HOP CVFT_FEAT16K_HOP
#define FK_REFLECT (FK_FRAME / 2)                       // whisper: samples of reflect padding per side
#define FK_NT 4                                         // frame tiles per workgroup
#define FK_F CVFT_FEAT16K_TILE                          // frames per workgroup
#define FK_STEPS (FK_FRAME / 16)                        // MFMA k-steps of 16 samples
#define FK_SPAN (FK_HOP * (FK_F - 1) + FK_FRAME)        // samples the tile's frames cover (10480)
#define FK_BPITCH (FK_HOP + 4)                          // a 160-sample block is stored 164 floats apart: see below
#define FK_SIG (FK_SPAN + 4 * (FK_SPAN / FK_HOP))       // floats of the sample image (10740)
#define FK_WAVES 8
#define FK_THREADS (64 * FK_WAVES)
#define FK_FIN_THREADS 256
#define FK_W_FLOOR 1e-10f
#define FK_W_LOG_FLOOR (-10.0f)                         // log10 of the floor
#define FK_K_FLOOR 1.1920929e-07f                       // 2^-23
#define FK_K_LOG_FLOOR (-0x1.fe2804p+3f)                // fp32(log(fp32(2^-23))) = -15.942385

static_assert(FK_F == 16 * FK_NT, "a workgroup's frames are FK_NT MFMA tiles");
static_assert(FK_FRAME % 16 == 0 && FK_HOP % 16 == 0, "a k-step of 16 samples never straddles a 160-sample block");
static_assert(FK_F * (CVFT_FEAT16K_WHISPER_BANDS + 1) <= FK_SIG, "the band image reuses the sample image");

// Sample image: sample j of the tile lives at j + 4 * (j / 160).  Frame f reads j = 160 f + n, so for one n the 16 frames
// of an MFMA tile sit 164 floats = 41 sixteen-byte slots apart: 16 distinct slots of the 64-bank row (160 apart would put
// alternate frames on the same slot).  Quads never straddle a pad because 160 % 4 == 0.  Step s of 25, lane group g,
// element e read n = 16 s + 4 g + e; the groups are one slot apart, which leaves the ds_read_b128 two-way conflicted
// between lane groups -- 4 reads of 8 LDS cycles against 32 MFMAs of 32 cycles per step, so it is left alone.
template <int MT, int KIND>
__global__ __launch_bounds__(FK_THREADS) void feat16k_kernel(int Lmax, int ldw, const float* __restrict__ wav,
                                                             const int* __restrict__ len, const f32x4* __restrict__ tab,
                                                             const f32x4* __restrict__ basis, int nchunks, int Tmax,
                                                             float* __restrict__ out, float* __restrict__ work) {
    constexpr int NB = KIND == CVFT_FEAT16K_WHISPER ? CVFT_FEAT16K_WHISPER_BANDS : CVFT_FEAT16K_FBANK_BANDS;
    constexpr int MPITCH = NB + 1;                      // band image [frame][band], read both ways by the epilogue
    __shared__ __attribute__((aligned(16))) float sm[FK_SIG];
    __shared__ float red[FK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, fr = lane & 15;
    const int b = blockIdx.y, t0 = blockIdx.x * FK_F;
    const int L = min(len ? len[b] : Lmax, Lmax);
    const int T = KIND == CVFT_FEAT16K_WHISPER ? (L > FK_REFLECT ? min(L / FK_HOP, Tmax) : 0)
                                               : (L >= FK_FRAME ? min(1 + (L - FK_FRAME) / FK_HOP, Tmax) : 0);
    const int nvalid = min(max(T - t0, 0), FK_F);

    if (nvalid > 0) {
        // ---- stage the tile's samples once (whisper: reflect map applied here); samples outside the row are zero
        const float* w = wav + (size_t)b * ldw;
        const int p0 = t0 * FK_HOP;
        for (int q = tid; q < FK_SPAN; q += FK_THREADS) {
            const int p = p0 + q;
            float v = 0.f;
            if (KIND == CVFT_FEAT16K_WHISPER) {
                if (p < L + 2 * FK_REFLECT) {
                    int s = p - FK_REFLECT;
                    s = s < 0 ? -s : (s >= L ? 2 * (L - 1) - s : s);
                    v = w[s];
                }
            } else if (p < L) {
                v = w[p];
            }
            sm[q + 4 * (q / FK_HOP)] = v;
        }
        __syncthreads();

        f32x4 mel[MT][FK_NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < FK_NT; ++nt) mel[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* sb = sm + FK_BPITCH * fr + 4 * g;

        for (int c = wave; c < nchunks; c += FK_WAVES) {
            // ---- DFT of bins 16c .. 16c+15 for the tile's 64 frames: rows = bins (table), columns = frames (LDS)
            f32x4 re[FK_NT], im[FK_NT];
#pragma unroll
            for (int nt = 0; nt < FK_NT; ++nt) re[nt] = im[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4* tc = tab + (size_t)c * (FK_STEPS * 2 * 64) + lane;
            f32x4 ca = tc[0], sa = tc[64];
            for (int s = 0; s < FK_STEPS; ++s) {
                const int sn = s < FK_STEPS - 1 ? s + 1 : s;
                const f32x4 ca_n = tc[sn * 128], sa_n = tc[sn * 128 + 64];
                const float* sp = sb + 16 * s + 4 * (s / (FK_HOP / 16));
                f32x4 x[FK_NT];
#pragma unroll
                for (int nt = 0; nt < FK_NT; ++nt) x[nt] = *reinterpret_cast<const f32x4*>(sp + nt * 16 * FK_BPITCH);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int nt = 0; nt < FK_NT; ++nt) {
                        re[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[e], x[nt][e], re[nt], 0, 0, 0);
                        im[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa[e], x[nt][e], im[nt], 0, 0, 0);
                    }
                ca = ca_n;
                sa = sa_n;
            }
            // ---- power in registers: lane holds bins 16c + 4g + i of frames nt*16 + fr, which is the B operand of the
            // filterbank product with k = bin (step i takes bin 4g + i from lane group g; the basis is packed alike)
#pragma unroll
            for (int nt = 0; nt < FK_NT; ++nt)
#pragma unroll
                for (int i = 0; i < 4; ++i) re[nt][i] = re[nt][i] * re[nt][i] + im[nt][i] * im[nt][i];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const f32x4 bw = basis[((size_t)c * MT + mt) * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int nt = 0; nt < FK_NT; ++nt)
                        mel[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[i], re[nt][i], mel[mt][nt], 0, 0, 0);
            }
        }

        // ---- the waves' partial band sums, added in wave order (fixed, so results are bit-identical run to run)
        __syncthreads();
        for (int wv = 0; wv < FK_WAVES; ++wv) {
            if (wave == wv) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < FK_NT; ++nt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int band = mt * 16 + g * 4 + i;
                            if (band < NB) {
                                float* p = sm + (nt * 16 + fr) * MPITCH + band;
                                *p = wv == 0 ? mel[mt][nt][i] : *p + mel[mt][nt][i];
                            }
                        }
            }
            __syncthreads();
        }
    }

    if (KIND == CVFT_FEAT16K_WHISPER) {
        // ---- floor, log10, store [band][t]; frames past the row's count are 0; the tile's maximum goes to the workspace
        float mx = -INFINITY;
        for (int e = tid; e < FK_F * NB; e += FK_THREADS) {
            const int fl = e % FK_F, band = e / FK_F, t = t0 + fl;
            if (t >= Tmax) continue;
            float v = 0.f;
            if (fl < nvalid) {
                const float m = sm[fl * MPITCH + band];
                v = m > FK_W_FLOOR ? log10f(m) : FK_W_LOG_FLOOR;
                mx = fmaxf(mx, v);
            }
            out[((size_t)b * NB + band) * Tmax + t] = v;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        if (tid == 0) {
            for (int wv = 1; wv < FK_WAVES; ++wv) mx = fmaxf(mx, red[wv]);
            work[(size_t)b * gridDim.x + blockIdx.x] = mx;
        }
    } else {
        // ---- floor, log, store [t][band]; frames past the row's count are 0; the tile's per-band sums over its valid
        // frames, added in frame order, go to the workspace
        for (int e = tid; e < FK_F * NB; e += FK_THREADS) {
            const int fl = e / NB, band = e % NB, t = t0 + fl;
            float v = 0.f;
            if (fl < nvalid) {
                const float m = sm[fl * MPITCH + band];
                v = m > FK_K_FLOOR ? logf(m) : FK_K_LOG_FLOOR;
                sm[fl * MPITCH + band] = v;
            }
            if (t < Tmax) out[((size_t)b * Tmax + t) * NB + band] = v;
        }
        if (work) {
            __syncthreads();
            if (tid < NB) {
                float s = 0.f;
                for (int fl = 0; fl < nvalid; ++fl) s += sm[fl * MPITCH + tid];
                work[((size_t)b * gridDim.x + blockIdx.x) * NB + tid] = s;
            }
        }
    }
}

// whisper: x = max(x, rowmax - 8), then (x + 4) / 4 on the row's valid frames; rowmax from the tiles' maxima
__global__ __launch_bounds__(FK_FIN_THREADS) void feat16k_whisper_finish(int Lmax, const int* __restrict__ len, int Tmax,
                                                                         const float* __restrict__ work,
                                                                         float* __restrict__ out) {
    constexpr int NB = CVFT_FEAT16K_WHISPER_BANDS;
    const int b = blockIdx.y, t0 = blockIdx.x * FK_F;
    const int L = min(len ? len[b] : Lmax, Lmax);
    const int T = L > FK_REFLECT ? min(L / FK_HOP, Tmax) : 0;
    if (t0 >= T) return;
    const int ntiles = (T + FK_F - 1) / FK_F;
    float mx = -INFINITY;
    for (int i = 0; i < ntiles; ++i) mx = fmaxf(mx, work[(size_t)b * gridDim.x + i]);
    const float lo = mx - 8.0f;
    for (int e = threadIdx.x; e < FK_F * NB; e += FK_FIN_THREADS) {
        const int fl = e % FK_F, band = e / FK_F, t = t0 + fl;
        if (t >= T) continue;
        float* p = out + ((size_t)b * NB + band) * Tmax + t;
        *p = (fmaxf(*p, lo) + 4.0f) * 0.25f;
    }
}

// fbank: subtract each band's mean over the row's frames; the tiles' sums are added in tile order
__global__ __launch_bounds__(FK_FIN_THREADS) void feat16k_fbank_finish(int Lmax, const int* __restrict__ len, int Tmax,
                                                                       const float* __restrict__ work,
                                                                       float* __restrict__ out) {
    constexpr int NB = CVFT_FEAT16K_FBANK_BANDS;
    __shared__ float mean[NB];
    const int b = blockIdx.y, t0 = blockIdx.x * FK_F;
    const int L = min(len ? len[b] : Lmax, Lmax);
    const int T = L >= FK_FRAME ? min(1 + (L - FK_FRAME) / FK_HOP, Tmax) : 0;
    if (t0 >= T) return;
    const int ntiles = (T + FK_F - 1) / FK_F;
    if (threadIdx.x < NB) {
        float s = 0.f;
        for (int i = 0; i < ntiles; ++i) s += work[((size_t)b * gridDim.x + i) * NB + threadIdx.x];
        mean[threadIdx.x] = s / (float)T;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < FK_F * NB; e += FK_FIN_THREADS) {
        const int fl = e / NB, band = e % NB, t = t0 + fl;
        if (t >= T) continue;
        out[((size_t)b * Tmax + t) * NB + band] -= mean[band];
    }
}

static int feat16k_check(const char* fn, int kind, int B, int Lmax, int Tmax) {
    CVFT_CHECK_ARG(kind == CVFT_FEAT16K_WHISPER || kind == CVFT_FEAT16K_FBANK, "%s: kind=%d (0: whisper log-mel, 1: kaldi fbank)", fn, kind);
    CVFT_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d outside [1, 65535]", fn, B);
    const int need = kind == CVFT_FEAT16K_WHISPER ? FK_REFLECT + 1 : FK_FRAME;
    CVFT_CHECK_ARG(Lmax >= need && Lmax <= (1 << 30), "%s: Lmax=%d (this feature needs >= %d samples)", fn, Lmax, need);
    CVFT_CHECK_ARG(Tmax >= 1 && Tmax <= (1 << 23), "%s: Tmax=%d", fn, Tmax);
    return 0;
}

extern "C" int cvft_feat16k(int kind, int B, int Lmax, int ldw, const float* wav, const int* len, const float* dft_tab,
                            const float* basis_tab, int nchunks, int Tmax, float* out, float* work, void* stream) {
    if (int rc = feat16k_check("cvft_feat16k", kind, B, Lmax, Tmax)) return rc;
    const int maxc = kind == CVFT_FEAT16K_WHISPER ? CVFT_FEAT16K_WHISPER_CHUNKS : CVFT_FEAT16K_FBANK_CHUNKS;
    CVFT_CHECK_ARG(ldw >= Lmax, "cvft_feat16k: ldw=%d below Lmax=%d", ldw, Lmax);
    CVFT_CHECK_ARG(nchunks >= 1 && nchunks <= maxc, "cvft_feat16k: nchunks=%d outside [1, %d]", nchunks, maxc);
    CVFT_CHECK_ARG(wav && dft_tab && basis_tab && out, "cvft_feat16k: null pointer");
    CVFT_CHECK_ARG(work || kind == CVFT_FEAT16K_FBANK, "cvft_feat16k: the whisper log-mel needs its workspace");
    CVFT_CHECK_ARG(((uintptr_t)dft_tab & 15) == 0 && ((uintptr_t)basis_tab & 15) == 0, "cvft_feat16k: tables must be 16-byte aligned");
    const dim3 grid((Tmax + FK_F - 1) / FK_F, B);
    const f32x4* tab = reinterpret_cast<const f32x4*>(dft_tab);
    const f32x4* basis = reinterpret_cast<const f32x4*>(basis_tab);
    if (kind == CVFT_FEAT16K_WHISPER)
        hipLaunchKernelGGL((feat16k_kernel<CVFT_FEAT16K_WHISPER_BANDS / 16, CVFT_FEAT16K_WHISPER>), grid, dim3(FK_THREADS), 0,
                           (hipStream_t)stream, Lmax, ldw, wav, len, tab, basis, nchunks, Tmax, out, work);
    else
        hipLaunchKernelGGL((feat16k_kernel<CVFT_FEAT16K_FBANK_BANDS / 16, CVFT_FEAT16K_FBANK>), grid, dim3(FK_THREADS), 0,
                           (hipStream_t)stream, Lmax, ldw, wav, len, tab, basis, nchunks, Tmax, out, work);
    CVFT_LAUNCH_CHECK("cvft_feat16k");
    return 0;
}

extern "C" int cvft_feat16k_finish(int kind, int B, int Lmax, const int* len, int Tmax, const float* work, float* out,
                                   void* stream) {
    if (int rc = feat16k_check("cvft_feat16k_finish", kind, B, Lmax, Tmax)) return rc;
    CVFT_CHECK_ARG(work && out, "cvft_feat16k_finish: null pointer");
    const dim3 grid((Tmax + FK_F - 1) / FK_F, B);
    if (kind == CVFT_FEAT16K_WHISPER)
        hipLaunchKernelGGL(feat16k_whisper_finish, grid, dim3(FK_FIN_THREADS), 0, (hipStream_t)stream, Lmax, len, Tmax, work, out);
    else
        hipLaunchKernelGGL(feat16k_fbank_finish, grid, dim3(FK_FIN_THREADS), 0, (hipStream_t)stream, Lmax, len, Tmax, work, out);
    CVFT_LAUNCH_CHECK("cvft_feat16k_finish");
    return 0;
}
