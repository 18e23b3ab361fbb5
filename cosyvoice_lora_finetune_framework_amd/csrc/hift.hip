// hift.hip -- the HiFT vocoder's inference kernels (include/cvft.h, "HiFT vocoder"): the tap-GEMM convolution on the
// matrix cores, the narrow direct convolution, the fp64 phase scan, the sine source, STFT and ISTFT.
#include "common.h"

// ---------------------------------------------------------------- cvft_hift_conv
#define HC_TM 64          // output positions per workgroup
#define HC_TN 64          // output channels per workgroup (16 per wave)
#define HC_KC 64          // input channels per staged slab
#define HC_SPAN 50        // max(tap_off) - min(tap_off): k = 11, d = 5
#define HC_ROWS (HC_TM + HC_SPAN)

// 16 bytes of k per lane and operand: fp32 = 4 k-steps of the 16x16x4 MFMA, bf16 = one 16x16x32 MFMA.  The k order
// inside a group is permuted the same way for both operands (lane group g holds k = VEC*g .. VEC*g + VEC-1).
template <typename T> struct HcOp;
template <> struct HcOp<float> {
    static constexpr int VEC = 4;
    typedef f32x4 V;
    static __device__ __forceinline__ void mma(f32x4& acc, V a, V b) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
    }
    static __device__ __forceinline__ void store4(float* p, float v0, float v1, float v2, float v3) {
        f32x4 v = {v0, v1, v2, v3};
        *reinterpret_cast<f32x4*>(p) = v;
    }
};
template <> struct HcOp<bf16_t> {
    static constexpr int VEC = 8;
    typedef bf16x8 V;
    static __device__ __forceinline__ void mma(f32x4& acc, V a, V b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
    static __device__ __forceinline__ void store4(bf16_t* p, float v0, float v1, float v2, float v3) {
        bf16x4 v = {(bf16_t)v0, (bf16_t)v1, (bf16_t)v2, (bf16_t)v3};
        *reinterpret_cast<bf16x4*>(p) = v;
    }
};

__device__ __forceinline__ float hc_pre(int pre, float x, float al, float slope) {
    if (pre == 1) {
        const float s = sinf(x * al);
        return x + (1.0f / (al + 1e-9f)) * (s * s);
    }
    if (pre == 2) return x > 0.f ? x : x * slope;
    return x;
}

template <typename T>
__global__ __launch_bounds__(256) void hift_conv_kernel(cvft_hift_conv_args a) {
    typedef HcOp<T> Op;
    constexpr int VEC = Op::VEC;
    constexpr int PITCH = HC_KC + VEC;          // 16 B of padding per row
    __shared__ __align__(16) T sA[HC_ROWS * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, q0 = blockIdx.x * HC_TM, n0 = blockIdx.y * HC_TN;
    int lo = a.tap_off[0], hi = a.tap_off[0];
    for (int j = 1; j < a.ntaps; ++j) { lo = min(lo, a.tap_off[j]); hi = max(hi, a.tap_off[j]); }
    const int nrows = HC_TM + hi - lo;          // <= HC_ROWS (checked by the host entry)
    const float* xb = a.x + (size_t)b * a.Tin * a.ldx;
    const T* W = reinterpret_cast<const T*>(a.W);
    f32x4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < a.Cin; c0 += HC_KC) {
        __syncthreads();
        // stage rows q0+lo .. q0+lo+nrows-1 of this 64-channel slab, pre-activation applied once per element
        const int c = (tid & 15) * 4;
        float al[4] = {1.f, 1.f, 1.f, 1.f};
        if (a.pre == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) al[e] = a.alpha[c0 + c + e];
        }
        for (int r = tid >> 4; r < nrows; r += 16) {
            const int t = q0 + lo + r;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (t >= 0 && t < a.Tin) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xb + (size_t)t * a.ldx + c0 + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = hc_pre(a.pre, xv[e], al[e], a.slope);
            }
            Op::store4(sA + r * PITCH + c, v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        for (int j = 0; j < a.ntaps; ++j) {
            const T* wj = W + ((size_t)j * a.CoutP + n0 + wave * 16 + (lane & 15)) * a.Cin + c0 + VEC * (lane >> 4);
            const T* aj = sA + (a.tap_off[j] - lo + (lane & 15)) * PITCH + VEC * (lane >> 4);
#pragma unroll
            for (int kg = 0; kg < HC_KC; kg += 4 * VEC) {
                const typename Op::V bf = *reinterpret_cast<const typename Op::V*>(wj + kg);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const typename Op::V af = *reinterpret_cast<const typename Op::V*>(aj + m * 16 * PITCH + kg);
                    Op::mma(acc[m], af, bf);
                }
            }
        }
    }

    const int n = n0 + wave * 16 + (lane & 15);
    if (n >= a.Cout) return;
    const float bias = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + m * 16 + (lane >> 4) * 4 + i;
            const int o = q * a.out_stride + a.out_off;
            if (q >= a.Tq || o >= a.Tout) continue;
            const size_t row = (size_t)b * a.Tout + o;
            float v = acc[m][i] + bias;
            if (a.elu) v = v > 0.f ? v : expm1f(v);
            if (a.res) v += a.res[row * a.ldr + n];
            if (a.res2) v += a.res2[row * a.ldr2 + n];
            if (a.accum) v += a.y[row * a.ldy + n];
            a.y[row * a.ldy + n] = v * a.scale;
        }
    }
}

extern "C" int cvft_hift_conv(const cvft_hift_conv_args* a, void* stream) {
    CVFT_CHECK_ARG(a, "cvft_hift_conv: null args");
    CVFT_CHECK_ARG(a->dtype == CVFT_F32 || a->dtype == CVFT_BF16, "cvft_hift_conv: dtype %d", a->dtype);
    CVFT_CHECK_ARG(a->B >= 1 && a->Tin >= 1 && a->Tq >= 1 && a->Tout >= 1 && a->out_stride >= 1 && a->out_off >= 0,
                   "cvft_hift_conv: B=%d Tin=%d Tq=%d Tout=%d out_stride=%d out_off=%d", a->B, a->Tin, a->Tq, a->Tout,
                   a->out_stride, a->out_off);
    CVFT_CHECK_ARG((long)(a->Tq - 1) * a->out_stride + a->out_off < a->Tout, "cvft_hift_conv: output rows exceed Tout=%d",
                   a->Tout);
    CVFT_CHECK_ARG(a->Cin >= 64 && a->Cin % HC_KC == 0, "cvft_hift_conv: Cin=%d (multiple of 64 required: pad the channels)",
                   a->Cin);
    CVFT_CHECK_ARG(a->Cout >= 1 && a->CoutP >= a->Cout && a->CoutP % HC_TN == 0, "cvft_hift_conv: Cout=%d CoutP=%d", a->Cout,
                   a->CoutP);
    CVFT_CHECK_ARG(a->ntaps >= 1 && a->ntaps <= 11, "cvft_hift_conv: ntaps=%d outside [1, 11]", a->ntaps);
    int lo = a->tap_off[0], hi = a->tap_off[0];
    for (int j = 1; j < a->ntaps; ++j) { lo = a->tap_off[j] < lo ? a->tap_off[j] : lo; hi = a->tap_off[j] > hi ? a->tap_off[j] : hi; }
    CVFT_CHECK_ARG(hi - lo <= HC_SPAN, "cvft_hift_conv: tap span %d > %d", hi - lo, HC_SPAN);
    CVFT_CHECK_ARG(a->x && a->W && a->y, "cvft_hift_conv: null pointer");
    CVFT_CHECK_ARG(a->ldx >= a->Cin && a->ldx % 4 == 0 && ((uintptr_t)a->x & 15) == 0 && ((uintptr_t)a->W & 15) == 0,
                   "cvft_hift_conv: x rows / W must be 16-byte aligned (ldx=%d)", a->ldx);
    CVFT_CHECK_ARG(a->ldy >= a->Cout && (!a->res || a->ldr >= a->Cout) && (!a->res2 || a->ldr2 >= a->Cout),
                   "cvft_hift_conv: bad output / residual strides");
    CVFT_CHECK_ARG(a->pre >= 0 && a->pre <= 2 && (a->pre != 1 || a->alpha), "cvft_hift_conv: pre=%d (Snake needs alpha)", a->pre);
    CVFT_CHECK_ARG(a->B <= 65535 && a->CoutP / HC_TN <= 65535, "cvft_hift_conv: grid too large");
    const dim3 grid((a->Tq + HC_TM - 1) / HC_TM, a->CoutP / HC_TN, a->B);
    hipStream_t s = (hipStream_t)stream;
    if (a->dtype == CVFT_F32) hipLaunchKernelGGL(hift_conv_kernel<float>, grid, dim3(256), 0, s, *a);
    else hipLaunchKernelGGL(hift_conv_kernel<bf16_t>, grid, dim3(256), 0, s, *a);
    CVFT_LAUNCH_CHECK("cvft_hift_conv");
    return 0;
}

// ---------------------------------------------------------------- cvft_hift_conv_small
__global__ __launch_bounds__(256) void hift_conv_small_kernel(int B, int Tin, int Tout, int Cin, int Cout, int k, int stride,
                                                              int pad, const float* x, int ldx, const float* W,
                                                              const float* bias, int absval, float* y, int ldy) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * Tout * Cout) return;
    const int n = (int)(idx % Cout);
    const long row = idx / Cout;
    const int t = (int)(row % Tout), b = (int)(row / Tout);
    float acc = bias ? bias[n] : 0.f;
    for (int j = 0; j < k; ++j) {
        const int ti = t * stride - pad + j;
        if (ti < 0 || ti >= Tin) continue;
        const float* xr = x + ((size_t)b * Tin + ti) * ldx;
        const float* wr = W + (size_t)j * Cin * Cout + n;
        for (int c = 0; c < Cin; ++c) acc += xr[c] * wr[(size_t)c * Cout];
    }
    y[row * ldy + n] = absval ? fabsf(acc) : acc;
}

extern "C" int cvft_hift_conv_small(int B, int Tin, int Tout, int Cin, int Cout, int k, int stride, int pad, const float* x,
                                    int ldx, const float* W, const float* bias, int absval, float* y, int ldy, void* stream) {
    CVFT_CHECK_ARG(B >= 1 && Tin >= 1 && Tout >= 1 && Cin >= 1 && Cout >= 1 && k >= 1 && stride >= 1 && pad >= 0,
                   "cvft_hift_conv_small: bad sizes");
    CVFT_CHECK_ARG((long)(Tout - 1) * stride - pad < Tin, "cvft_hift_conv_small: Tout=%d reads past Tin=%d", Tout, Tin);
    CVFT_CHECK_ARG(x && W && y && ldx >= Cin && ldy >= Cout, "cvft_hift_conv_small: bad pointers / strides");
    const long total = (long)B * Tout * Cout;
    hipLaunchKernelGGL(hift_conv_small_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, Tin,
                       Tout, Cin, Cout, k, stride, pad, x, ldx, W, bias, absval, y, ldy);
    CVFT_LAUNCH_CHECK("cvft_hift_conv_small");
    return 0;
}

// ---------------------------------------------------------------- cvft_hift_scan
#define SCAN_PER 16
__global__ __launch_bounds__(256) void hift_scan_kernel(int L, int rep, int Lx, const float* x, float div, float* y) {
    __shared__ double wsum[4];
    const float* xr = x + (size_t)blockIdx.x * Lx;
    float* yr = y + (size_t)blockIdx.x * L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double carry = 0.0;
    for (int base = 0; base < L; base += 256 * SCAN_PER) {
        const int n0 = base + tid * SCAN_PER;
        double v[SCAN_PER], loc = 0.0;
#pragma unroll
        for (int e = 0; e < SCAN_PER; ++e) {
            const int n = n0 + e;
            loc += n < L ? (double)__fdiv_rn(xr[n / rep], div) : 0.0;
            v[e] = loc;
        }
        double inc = loc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        __syncthreads();
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        double pre = carry;
        for (int w = 0; w < wave; ++w) pre += wsum[w];
        pre += inc - loc;
#pragma unroll
        for (int e = 0; e < SCAN_PER; ++e)
            if (n0 + e < L) yr[n0 + e] = (float)(pre + v[e]);
        carry += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    }
}

extern "C" int cvft_hift_scan(int R, int L, int rep, const float* x, float div, float* y, void* stream) {
    CVFT_CHECK_ARG(R >= 1 && L >= 1 && rep >= 1 && x && y && div != 0.f, "cvft_hift_scan: R=%d L=%d rep=%d", R, L, rep);
    hipLaunchKernelGGL(hift_scan_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, L, rep, (L + rep - 1) / rep, x, div, y);
    CVFT_LAUNCH_CHECK("cvft_hift_scan");
    return 0;
}

// ---------------------------------------------------------------- cvft_hift_source
__global__ __launch_bounds__(256) void hift_source_kernel(int H, int L, int rep, const float* f0, const float* cum,
                                                          const float* phase, const float* noise, const float* lw,
                                                          const float* lb, float thr, float* s, float* uv_out) {
    const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (n >= L) return;
    const int Lx = (L + rep - 1) / rep;
    const float uv = f0[(size_t)b * Lx + n / rep] > thr ? 1.f : 0.f;
    const float namp = uv * 0.003f + (1.f - uv) * 0.1f / 3.f;
    float acc = 0.f;
    for (int h = 0; h < H; ++h) {
        const size_t i = ((size_t)b * H + h) * L + n;
        const float c = cum[i];
        const float theta = 6.283185307179586f * (c - floorf(c));
        const float sine = 0.1f * sinf(theta + phase[b * H + h]);
        acc += (sine * uv + namp * noise[i]) * lw[h];
    }
    s[(size_t)b * L + n] = tanhf(acc + lb[0]);
    if (uv_out) uv_out[(size_t)b * L + n] = uv;
}

extern "C" int cvft_hift_source(int B, int H, int L, int rep, const float* f0, const float* cum, const float* phase,
                                const float* noise, const float* lw, const float* lb, float thr, float* s, float* uv_out,
                                void* stream) {
    CVFT_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && H <= 16 && L >= 1 && rep >= 1, "cvft_hift_source: B=%d H=%d L=%d rep=%d", B,
                   H, L, rep);
    CVFT_CHECK_ARG(f0 && cum && phase && noise && lw && lb && s, "cvft_hift_source: null pointer");
    hipLaunchKernelGGL(hift_source_kernel, dim3((L + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, H, L, rep, f0, cum, phase,
                       noise, lw, lb, thr, s, uv_out);
    CVFT_LAUNCH_CHECK("cvft_hift_source");
    return 0;
}

// ---------------------------------------------------------------- cvft_hift_stft / cvft_hift_istft
__device__ __forceinline__ float hann16(int m) { return 0.5f - 0.5f * cospif((float)m * 0.125f); }

__global__ __launch_bounds__(256) void hift_stft_kernel(int B, int L, const float* s, float* out) {
    const int F = L / 4 + 1;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * F * 18) return;
    const int c = (int)(idx % 18);
    const long row = idx / 18;
    const int f = (int)(row % F), b = (int)(row / F);
    const int k = c % 9;
    const float* sb = s + (size_t)b * L;
    float acc = 0.f;
    for (int m = 0; m < 16; ++m) {
        int j = 4 * f + m - 8;
        j = j < 0 ? -j : (j >= L ? 2 * (L - 1) - j : j);
        const float ang = (float)((k * m) & 15) * 0.125f;
        const float tw = c < 9 ? cospif(ang) : -sinpif(ang);
        acc += hann16(m) * sb[j] * tw;
    }
    out[idx] = acc;
}

extern "C" int cvft_hift_stft(int B, int L, const float* s, float* out, void* stream) {
    CVFT_CHECK_ARG(B >= 1 && L >= 16 && L % 4 == 0 && s && out, "cvft_hift_stft: B=%d L=%d (L %% 4 == 0, L >= 16)", B, L);
    const long total = (long)B * (L / 4 + 1) * 18;
    hipLaunchKernelGGL(hift_stft_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, L, s, out);
    CVFT_LAUNCH_CHECK("cvft_hift_stft");
    return 0;
}

__global__ __launch_bounds__(256) void hift_istft_kernel(int F, const float* x, int ldx, float limit, float* wav) {
    const int L = 4 * (F - 1);
    const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (n >= L) return;
    const int p = n + 8;
    const int f_lo = max(0, (p - 12) >> 2), f_hi = min(F - 1, p >> 2);     // 4f <= p <= 4f + 15
    float num = 0.f, den = 0.f;
    for (int f = f_lo; f <= f_hi; ++f) {
        const int m = p - 4 * f;
        const float* xr = x + ((size_t)b * F + f) * ldx;
        float v = 0.f;
        for (int k = 0; k <= 8; ++k) {
            const float mag = fminf(expf(xr[k]), 100.f);
            float sp, cp;
            sincosf(sinf(xr[9 + k]), &sp, &cp);
            const float ang = (float)((k * m) & 15) * 0.125f;
            // bins 0 and 8 contribute their real part only (the inverse real DFT drops their imaginary part)
            const float t = (k == 0 || k == 8) ? mag * cp * cospif(ang) : 2.f * mag * (cp * cospif(ang) - sp * sinpif(ang));
            v += t;
        }
        const float w = hann16(m);
        num += w * v * 0.0625f;
        den += w * w;
    }
    const float yv = num / den;
    wav[(size_t)b * L + n] = fminf(fmaxf(yv, -limit), limit);
}

__global__ __launch_bounds__(256) void hift_mag_kernel(long rows, const float* x, int ldx, float* mag) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * 9) return;
    mag[idx] = fminf(expf(x[(idx / 9) * ldx + idx % 9]), 100.f);
}

extern "C" int cvft_hift_istft(int B, int F, const float* x, int ldx, float limit, float* wav, float* mag_out, void* stream) {
    CVFT_CHECK_ARG(B >= 1 && B <= 65535 && F >= 5 && x && wav && ldx >= 18, "cvft_hift_istft: B=%d F=%d ldx=%d", B, F, ldx);
    const int L = 4 * (F - 1);
    hipLaunchKernelGGL(hift_istft_kernel, dim3((L + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, F, x, ldx, limit, wav);
    if (mag_out) {
        const long rows = (long)B * F;
        hipLaunchKernelGGL(hift_mag_kernel, dim3((unsigned)((rows * 9 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, x,
                           ldx, mag_out);
    }
    CVFT_LAUNCH_CHECK("cvft_hift_istft");
    return 0;
}
