// stream.hip -- the two stitching launches of streaming synthesis (include/cvft.h, "Streaming"): the mel side and the
// speech side of the reference's token2wav, each as ONE elementwise launch in place of a host round trip and 6-8 small
// slice / concat / multiply launches.  Bandwidth-trivial: no LDS, no atomics, every output element has one writer.
#include "common.h"

#define ST_THREADS 256

// The reference multiplies fp32 tensors by a float64 numpy window, so its fade is an fp64 sum rounded once to fp32.
// The products of two fp32 values are exact in fp64; what remains is the rounding of the window to fp32.
__device__ __forceinline__ float st_fade(float in, float w_in, float out, float w_out) {
    return (float)((double)in * (double)w_in + (double)out * (double)w_out);
}

// x * scale + shift as torch computes `mel * MEL_STD + MEL_MEAN`: a rounded product, then a rounded sum.  The compiler's
// default contracts a * b + c into one fma (one rounding), whatever the spelling, so contraction is switched off here.
__device__ __forceinline__ float st_affine(float v, float scale, float shift) {
#pragma clang fp contract(off)
    const float prod = v * scale;
    return prod + shift;
}

struct MelStitch {
    int Tn, ldx, trim, affine;
    float scale, shift;
    int ov, ldp, pcols, mc, ldc, total, Tout, ldo, mc_out;
    const float *x, *prev, *cache, *w;
    float *out, *nov, *ncache;
};

// column j of row c of [cache | faded chunk]
__device__ __forceinline__ float mel_value(const MelStitch& a, int c, int j) {
    if (j < a.mc) return a.cache[(size_t)c * a.ldc + j];
    const int k = j - a.mc;
    float v = a.x[(size_t)c * a.ldx + a.trim + k];
    if (a.affine) v = st_affine(v, a.scale, a.shift);
    if (a.prev != nullptr && k < a.ov) v = st_fade(v, a.w[k], a.prev[(size_t)c * a.ldp + a.pcols - a.ov + k], a.w[a.ov + k]);
    return v;
}

// grid (quads of columns, C): a thread owns columns j0 .. j0 + 3 of one row of [cache | faded chunk] and writes each to
// the vocoder input (j < Tout) or the new overlap (j >= Tout), and a second time where it is one of the last mc_out
// columns of the vocoder input (the new cached mel).
__global__ __launch_bounds__(ST_THREADS) void stream_mel_stitch_kernel(MelStitch a) {
    const int c = blockIdx.y;
    const int j0 = 4 * (blockIdx.x * ST_THREADS + threadIdx.x);
    if (j0 >= a.total) return;
    const int n = min(4, a.total - j0);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int k0 = j0 - a.mc;
    const float* xs = a.x + (size_t)c * a.ldx + a.trim + k0;
    if (n == 4 && k0 >= 0 && (a.prev == nullptr || k0 >= a.ov) && (reinterpret_cast<uintptr_t>(xs) & 15) == 0) {
        v = *reinterpret_cast<const f32x4*>(xs);                  // a quad of plain chunk columns: one 16-byte load
        if (a.affine) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = st_affine(v[e], a.scale, a.shift);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) v[e] = mel_value(a, c, j0 + e);
    }
    float* o = a.out + (size_t)c * a.ldo + j0;
    if (j0 + 3 < a.Tout && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        *reinterpret_cast<f32x4*>(o) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= n) break;
            const int j = j0 + e;
            if (j < a.Tout) o[e] = v[e];
            else a.nov[(size_t)c * a.ov + (j - a.Tout)] = v[e];
        }
    }
    if (a.ncache != nullptr) {
        const int first = a.Tout - a.mc_out;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + e;
            if (e < n && j >= first && j < a.Tout) a.ncache[(size_t)c * a.mc_out + (j - first)] = v[e];
        }
    }
}

extern "C" int cvft_stream_mel_stitch(int C, int Tn, int ldx, const float* x, int trim, int affine, float scale, float shift,
                                      int ov, const float* prev, int ldp, int prev_cols, int mc, const float* cache, int ldc,
                                      const float* window, int finalize, float* out, int ldo, float* new_overlap,
                                      float* new_cache, int mc_out, void* stream) {
    CVFT_CHECK_ARG(C >= 1 && C <= 65535, "cvft_stream_mel_stitch: C=%d outside [1, 65535]", C);
    CVFT_CHECK_ARG(Tn >= 1 && Tn <= (1 << 24) && ldx >= Tn && trim >= 0 && trim < Tn && ov >= 0 && mc >= 0 && mc <= (1 << 24),
                   "cvft_stream_mel_stitch: Tn=%d ldx=%d trim=%d ov=%d mc=%d", Tn, ldx, trim, ov, mc);
    CVFT_CHECK_ARG((finalize && prev == nullptr) || Tn - trim >= ov, "cvft_stream_mel_stitch: the chunk keeps %d columns after "
                   "trimming %d of %d, fewer than the overlap of %d", Tn - trim, trim, Tn, ov);
    CVFT_CHECK_ARG(prev == nullptr || (window != nullptr && ov >= 1 && prev_cols >= ov && ldp >= prev_cols),
                   "cvft_stream_mel_stitch: previous overlap of %d columns (pitch %d) for an overlap of %d, window %p", prev_cols,
                   ldp, ov, (const void*)window);
    CVFT_CHECK_ARG((mc == 0) == (cache == nullptr) && (cache == nullptr || ldc >= mc),
                   "cvft_stream_mel_stitch: cached mel of %d columns (pitch %d), pointer %p", mc, ldc, (const void*)cache);
    const int total = mc + (Tn - trim), Tout = total - (finalize ? 0 : ov);
    CVFT_CHECK_ARG(x != nullptr && (out != nullptr || Tout == 0), "cvft_stream_mel_stitch: null pointer");
    CVFT_CHECK_ARG(finalize || ov == 0 || new_overlap != nullptr, "cvft_stream_mel_stitch: no buffer for the new overlap");
    CVFT_CHECK_ARG(ldo >= Tout, "cvft_stream_mel_stitch: output pitch %d below its %d columns", ldo, Tout);
    CVFT_CHECK_ARG(new_cache == nullptr || (mc_out >= 1 && mc_out <= Tout), "cvft_stream_mel_stitch: new cache of %d columns "
                   "from a vocoder input of %d", mc_out, Tout);
    MelStitch a;
    a.Tn = Tn; a.ldx = ldx; a.trim = trim; a.affine = affine; a.scale = scale; a.shift = shift;
    a.ov = ov; a.ldp = ldp; a.pcols = prev_cols; a.mc = mc; a.ldc = ldc; a.total = total; a.Tout = Tout; a.ldo = ldo;
    a.mc_out = new_cache ? mc_out : 0;
    a.x = x; a.prev = prev; a.cache = cache; a.w = window; a.out = out; a.nov = new_overlap; a.ncache = new_cache;
    const int quads = (total + 3) / 4;
    hipLaunchKernelGGL(stream_mel_stitch_kernel, dim3((quads + ST_THREADS - 1) / ST_THREADS, C), dim3(ST_THREADS), 0,
                       (hipStream_t)stream, a);
    CVFT_LAUNCH_CHECK("cvft_stream_mel_stitch");
    return 0;
}

// 16-bit PCM as inference_joint.pcm16: a rounded fp32 product by 32767, round half to even, clip
__device__ __forceinline__ short st_pcm(float v) {
    const float r = rintf(__fmul_rn(v, 32767.0f));
    return (short)(int)fminf(fmaxf(r, -32768.0f), 32767.0f);
}

// a thread owns samples i0 .. i0 + 3: faded against the cache below sc, emitted below Nout, withheld from Nout on
__global__ __launch_bounds__(ST_THREADS) void stream_wav_stitch_kernel(int N, const float* __restrict__ speech, int sc,
                                                                       const float* __restrict__ cache,
                                                                       const float* __restrict__ w, int Nout,
                                                                       float* __restrict__ out, float* __restrict__ ncache,
                                                                       short* __restrict__ pcm) {
    const int i0 = 4 * (blockIdx.x * ST_THREADS + threadIdx.x);
    if (i0 >= N) return;
    const int n = min(4, N - i0);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n == 4 && (reinterpret_cast<uintptr_t>(speech + i0) & 15) == 0) {
        v = *reinterpret_cast<const f32x4*>(speech + i0);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) v[e] = speech[i0 + e];
    }
    if (cache != nullptr && i0 < sc) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n && i0 + e < sc) v[e] = st_fade(v[e], w[i0 + e], cache[i0 + e], w[sc + i0 + e]);
    }
    if (i0 + 3 < Nout && (reinterpret_cast<uintptr_t>(out + i0) & 15) == 0) {
        *reinterpret_cast<f32x4*>(out + i0) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= n) break;
            if (i0 + e < Nout) out[i0 + e] = v[e];
            else ncache[i0 + e - Nout] = v[e];
        }
    }
    if (pcm != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n && i0 + e < Nout) pcm[i0 + e] = st_pcm(v[e]);
    }
}

extern "C" int cvft_stream_wav_stitch(int N, const float* speech, int sc, const float* cache, const float* window,
                                      int finalize, float* out, float* new_cache, int16_t* pcm, void* stream) {
    CVFT_CHECK_ARG(N >= 1 && N <= (1 << 30) && sc >= 0, "cvft_stream_wav_stitch: N=%d sc=%d", N, sc);
    CVFT_CHECK_ARG(N >= sc, "cvft_stream_wav_stitch: %d samples of speech, fewer than the cache of %d", N, sc);
    CVFT_CHECK_ARG(speech != nullptr && (cache == nullptr || (window != nullptr && sc >= 1)),
                   "cvft_stream_wav_stitch: null pointer (speech %p, window %p, sc=%d)", (const void*)speech, (const void*)window, sc);
    const int Nout = N - (finalize ? 0 : sc);
    CVFT_CHECK_ARG(Nout == 0 || out != nullptr, "cvft_stream_wav_stitch: no buffer for the %d emitted samples", Nout);
    CVFT_CHECK_ARG(finalize || sc == 0 || new_cache != nullptr, "cvft_stream_wav_stitch: no buffer for the new speech cache");
    const int quads = (N + 3) / 4;
    hipLaunchKernelGGL(stream_wav_stitch_kernel, dim3((quads + ST_THREADS - 1) / ST_THREADS), dim3(ST_THREADS), 0,
                       (hipStream_t)stream, N, speech, sc, cache, window, Nout, out, new_cache, reinterpret_cast<short*>(pcm));
    CVFT_LAUNCH_CHECK("cvft_stream_wav_stitch");
    return 0;
}
