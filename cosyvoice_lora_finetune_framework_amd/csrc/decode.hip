// decode.hip -- autoregressive speech-token decode of TransformerLM (llm.py:165-228): the M <= 16 weight-streaming
// linear, the rel-pos attention of a few new rows against a growing K/V cache (split over workgroups + combine), and the
// fused log_softmax / top-k / top-p / RAS sampler.  Activations and caches are fp32; weights fp32 or bf16.  Contract:
// include/cvft.h "Autoregressive decode".
#include "common.h"

namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_COLS = 4;        // output columns per workgroup (a 4 x 1024 bf16 slice = 8 KiB of weights)
constexpr int ATT_KEYS = 256;     // keys per attention workgroup (one per thread)
constexpr int MAX_LQ = 16;
constexpr int SMP_THREADS = 256;
constexpr int SMP_VMAX = 8192;
constexpr int SMP_KMAX = 64;
constexpr int SMP_TRIALS = 101;   // llm.py:147-163: the first draw + 100 re-draws, then RuntimeError

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// 8 consecutive weights of row n as fp32, read once with the non-temporal policy (MI355X_MICROARCH nt-weights)
__device__ __forceinline__ void load_w8(const float* W, size_t off, float* w) {
    const f32x4* p = reinterpret_cast<const f32x4*>(W + off);
    f32x4 a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + 1);
    w[0] = a[0]; w[1] = a[1]; w[2] = a[2]; w[3] = a[3]; w[4] = b[0]; w[5] = b[1]; w[6] = b[2]; w[7] = b[3];
}
__device__ __forceinline__ void load_w8(const bf16_t* W, size_t off, float* w) {
    bf16x8 a = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(W + off));
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (float)a[i];
}

// ---------------------------------------------------------------- decode linear
// The main loop of both decode linears (plain and with the per-row LoRA epilogue term): the K-sum of output (m, n) of
// this workgroup's DL_COLS columns, returned to thread t = c * MR + m (true when that thread owns a live output).
template <typename WT, int MR>
__device__ __forceinline__ bool decode_linear_dot(
    int M, int N, int K, const float* __restrict__ X, int ldx, const float* __restrict__ lg, const float* __restrict__ lb,
    float eps, const WT* __restrict__ W, int& m_out, int& n_out, float& y_out) {
    __shared__ float s_mean[MAX_LQ], s_rstd[MAX_LQ];
    __shared__ float s_red[DL_THREADS / WAVE][DL_COLS][MR];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    const bool ln = lg != nullptr;
    if (ln) {   // row statistics (two-pass) of the <= 16 input rows; every workgroup redoes them
        for (int m = wv; m < M; m += DL_THREADS / WAVE) {
            const float* x = X + (size_t)m * ldx;
            float s = 0.f;
            for (int k = lane; k < K; k += WAVE) s += x[k];
            const float mean = wave_sum(s) / K;
            float q = 0.f;
            for (int k = lane; k < K; k += WAVE) { const float d = x[k] - mean; q += d * d; }
            const float var = wave_sum(q) / K;
            if (lane == 0) { s_mean[m] = mean; s_rstd[m] = 1.0f / sqrtf(var + eps); }
        }
        __syncthreads();
    }
    const int n0 = blockIdx.x * DL_COLS;
    float acc[DL_COLS][MR];
#pragma unroll
    for (int c = 0; c < DL_COLS; ++c)
#pragma unroll
        for (int m = 0; m < MR; ++m) acc[c][m] = 0.f;
    const int NV = K / 8;
#pragma unroll 2
    for (int v = t; v < NV; v += DL_THREADS) {
        const int k = v * 8;
        float w[DL_COLS][8];
#pragma unroll
        for (int c = 0; c < DL_COLS; ++c) {
            const int n = min(n0 + c, N - 1);          // (columns past N: a valid row is read, the result is dropped)
            load_w8(W, (size_t)n * K + k, w[c]);
        }
        float g[8], be[8];
        if (ln) {
            const f32x4* gp = reinterpret_cast<const f32x4*>(lg + k);
            const f32x4* bp = reinterpret_cast<const f32x4*>(lb + k);
            f32x4 g0 = gp[0], g1 = gp[1], b0 = bp[0], b1 = bp[1];
            g[0] = g0[0]; g[1] = g0[1]; g[2] = g0[2]; g[3] = g0[3]; g[4] = g1[0]; g[5] = g1[1]; g[6] = g1[2]; g[7] = g1[3];
            be[0] = b0[0]; be[1] = b0[1]; be[2] = b0[2]; be[3] = b0[3]; be[4] = b1[0]; be[5] = b1[1]; be[6] = b1[2]; be[7] = b1[3];
        }
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            if (m < M) {
                const f32x4* xp = reinterpret_cast<const f32x4*>(X + (size_t)m * ldx + k);
                f32x4 x0 = xp[0], x1 = xp[1];
                float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
                if (ln) {
                    const float mu = s_mean[m], rs = s_rstd[m];
#pragma unroll
                    for (int i = 0; i < 8; ++i) x[i] = (x[i] - mu) * rs * g[i] + be[i];
                }
#pragma unroll
                for (int c = 0; c < DL_COLS; ++c)
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[c][m] = fmaf(w[c][i], x[i], acc[c][m]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < DL_COLS; ++c)
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const float s = wave_sum(acc[c][m]);
            if (lane == 0) s_red[wv][c][m] = s;
        }
    __syncthreads();
    if (t < DL_COLS * MR) {
        const int c = t / MR, m = t % MR, n = n0 + c;
        if (m < M && n < N) {
            float y = 0.f;
#pragma unroll
            for (int w = 0; w < DL_THREADS / WAVE; ++w) y += s_red[w][c][m];
            m_out = m; n_out = n; y_out = y;
            return true;
        }
    }
    return false;
}

template <typename WT, int MR>
__global__ __launch_bounds__(DL_THREADS) void decode_linear_kernel(
    int M, int N, int K, const float* __restrict__ X, int ldx, const float* __restrict__ lg, const float* __restrict__ lb,
    float eps, const WT* __restrict__ W, const float* __restrict__ bias, int act, const float* residual, int ldr, float* Y,
    int ldy) {
    int m, n;
    float y;
    if (!decode_linear_dot<WT, MR>(M, N, K, X, ldx, lg, lb, eps, W, m, n, y)) return;
    if (bias) y += bias[n];
    if (act == 1) y = fmaxf(y, 0.f);
    if (residual) y += residual[(size_t)m * ldr + n];
    Y[(size_t)m * ldy + n] = y;
}

// 8 consecutive adapter values as fp32.  The adapter stacks are a few MB re-read every step: plain loads, they stay cached.
__device__ __forceinline__ void load_a8(const float* A, size_t off, float* w) {
    const f32x4* p = reinterpret_cast<const f32x4*>(A + off);
    f32x4 a = p[0], b = p[1];
    w[0] = a[0]; w[1] = a[1]; w[2] = a[2]; w[3] = a[3]; w[4] = b[0]; w[5] = b[1]; w[6] = b[2]; w[7] = b[3];
}
__device__ __forceinline__ void load_a8(const bf16_t* A, size_t off, float* w) {
    bf16x8 a = *reinterpret_cast<const bf16x8*>(A + off);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (float)a[i];
}

// decode linear + the LoRA up-projection of the row's adapter: y = W.x + bias + scale[s] * Bst[s][n][:] . Z[m][g*R : g*R+R],
// s = slot[m], g = n / Ng; then the activation, then the residual.  A row without a valid slot takes the plain epilogue.
template <typename WT, int MR>
__global__ __launch_bounds__(DL_THREADS) void decode_linear_lora_kernel(
    int M, int N, int K, const float* __restrict__ X, int ldx, const float* __restrict__ lg, const float* __restrict__ lb,
    float eps, const WT* __restrict__ W, const float* __restrict__ bias, int act, const float* residual, int ldr, float* Y,
    int ldy, int S, int Ng, int R, const WT* __restrict__ Bst, const float* __restrict__ scale,
    const int32_t* __restrict__ slot, const float* __restrict__ Z, int ldz) {
    int m, n;
    float y;
    if (!decode_linear_dot<WT, MR>(M, N, K, X, ldx, lg, lb, eps, W, m, n, y)) return;
    if (bias) y += bias[n];
    const int s = slot[m];
    if (s >= 0 && s < S) {
        const float* z = Z + (size_t)m * ldz + (n / Ng) * R;
        const size_t boff = ((size_t)s * N + n) * R;
        float u = 0.f;
        for (int j = 0; j < R; j += 8) {
            float b[8];
            load_a8(Bst, boff + j, b);
            const f32x4 z0 = reinterpret_cast<const f32x4*>(z + j)[0], z1 = reinterpret_cast<const f32x4*>(z + j)[1];
            const float zz[8] = {z0[0], z0[1], z0[2], z0[3], z1[0], z1[1], z1[2], z1[3]};
#pragma unroll
            for (int i = 0; i < 8; ++i) u = fmaf(b[i], zz[i], u);
        }
        y += scale[s] * u;
    }
    if (act == 1) y = fmaxf(y, 0.f);
    if (residual) y += residual[(size_t)m * ldr + n];
    Y[(size_t)m * ldy + n] = y;
}

// LoRA down-projection of the decode rows: Z[m][g*R + j] = LN?(X)[m,:] . A[slot[m]][g][j][:].  One workgroup per
// (8 values of j, group g, row m), so a row's result depends on nothing but that row; operands go straight to VGPRs.
constexpr int LD_J = 8;
template <typename WT>
__global__ __launch_bounds__(DL_THREADS) void decode_lora_down_kernel(
    int K, int S, int G, int R, const float* __restrict__ X, int ldx, const float* __restrict__ lg,
    const float* __restrict__ lb, float eps, const WT* __restrict__ A, const int32_t* __restrict__ slot,
    float* __restrict__ Z, int ldz) {
    __shared__ float s_red[DL_THREADS / WAVE][LD_J];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    const int j0 = blockIdx.x * LD_J, g = blockIdx.y, m = blockIdx.z;
    float* zo = Z + (size_t)m * ldz + g * R + j0;
    const int s = slot[m];
    if (s < 0 || s >= S) {      // no adapter: zeros, and the stack is never indexed
        if (t < LD_J) zo[t] = 0.f;
        return;
    }
    const float* x = X + (size_t)m * ldx;
    const bool ln = lg != nullptr;
    float mu = 0.f, rs = 1.f;
    if (ln) {   // the two-pass row statistics of decode_linear_dot (every wave redoes them, in that order)
        float sm = 0.f;
        for (int k = lane; k < K; k += WAVE) sm += x[k];
        mu = wave_sum(sm) / K;
        float q = 0.f;
        for (int k = lane; k < K; k += WAVE) { const float d = x[k] - mu; q += d * d; }
        const float var = wave_sum(q) / K;
        rs = 1.0f / sqrtf(var + eps);
    }
    const WT* a = A + (((size_t)s * G + g) * R + j0) * K;
    float acc[LD_J];
#pragma unroll
    for (int j = 0; j < LD_J; ++j) acc[j] = 0.f;
    const int NV = K / 8;
    for (int v = t; v < NV; v += DL_THREADS) {
        const int k = v * 8;
        float xv[8];
        load_a8(x, (size_t)k, xv);
        if (ln) {
            float gm[8], be[8];
            load_a8(lg, (size_t)k, gm);
            load_a8(lb, (size_t)k, be);
#pragma unroll
            for (int i = 0; i < 8; ++i) xv[i] = (xv[i] - mu) * rs * gm[i] + be[i];
        }
#pragma unroll
        for (int j = 0; j < LD_J; ++j) {
            float w[8];
            load_a8(a, (size_t)j * K + k, w);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[j] = fmaf(w[i], xv[i], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < LD_J; ++j) {
        const float r = wave_sum(acc[j]);
        if (lane == 0) s_red[wv][j] = r;
    }
    __syncthreads();
    if (t < LD_J) {
        float z = 0.f;
#pragma unroll
        for (int w = 0; w < DL_THREADS / WAVE; ++w) z += s_red[w][t];
        zo[t] = z;
    }
}

template <typename WT>
int launch_linear(int M, int N, int K, const float* X, int ldx, const float* lg, const float* lb, float eps, const void* W,
                  const float* bias, int act, const float* res, int ldr, float* Y, int ldy, hipStream_t s) {
    const dim3 grid((N + DL_COLS - 1) / DL_COLS), blk(DL_THREADS);
    const WT* w = static_cast<const WT*>(W);
#define DL_CASE(MR)                                                                                                  \
    hipLaunchKernelGGL((decode_linear_kernel<WT, MR>), grid, blk, 0, s, M, N, K, X, ldx, lg, lb, eps, w, bias, act, \
                       res, ldr, Y, ldy)
    if (M <= 1) DL_CASE(1);
    else if (M <= 2) DL_CASE(2);
    else if (M <= 4) DL_CASE(4);
    else if (M <= 8) DL_CASE(8);
    else DL_CASE(16);
#undef DL_CASE
    return 0;
}

template <typename WT>
int launch_linear_lora(int M, int N, int K, const float* X, int ldx, const float* lg, const float* lb, float eps,
                       const void* W, const float* bias, int act, const float* res, int ldr, float* Y, int ldy, int S, int G,
                       int R, const void* Bst, const float* scale, const int32_t* slot, const float* Z, int ldz,
                       hipStream_t s) {
    const dim3 grid((N + DL_COLS - 1) / DL_COLS), blk(DL_THREADS);
    const WT* w = static_cast<const WT*>(W);
    const WT* b = static_cast<const WT*>(Bst);
#define DL_CASE(MR)                                                                                                       \
    hipLaunchKernelGGL((decode_linear_lora_kernel<WT, MR>), grid, blk, 0, s, M, N, K, X, ldx, lg, lb, eps, w, bias, act, \
                       res, ldr, Y, ldy, S, N / G, R, b, scale, slot, Z, ldz)
    if (M <= 1) DL_CASE(1);
    else if (M <= 2) DL_CASE(2);
    else if (M <= 4) DL_CASE(4);
    else if (M <= 8) DL_CASE(8);
    else DL_CASE(16);
#undef DL_CASE
    return 0;
}

// ---------------------------------------------------------------- decode attention
// One (key split s, head h) workgroup of the Lq new rows q0 .. q0+Lq-1 of `qkv` against cache row b: the body of both the
// uniform (B, Lq) launch (q0 = b * Lq) and the ragged one (a segment table).  Its slice of `part` is indexed per
// (query row, head, split): the Lq*H*nsplit*66 floats from q0*H*nsplit*66, laid out [h][s][r][66].
__device__ __forceinline__ void decode_attn_split_body(
    int b, int q0, int Lq, bool skip, int s, int h, int H, int cap, int nsplit, const float* __restrict__ qkv, int ldqkv,
    float* kc, float* vc, const int32_t* __restrict__ len, const float* __restrict__ P, int ldp,
    const float* __restrict__ pbu, const float* __restrict__ pbv, float scale, float* __restrict__ part) {
    __shared__ float s_qu[MAX_LQ][64], s_qv[MAX_LQ][64];
    __shared__ float s_p[MAX_LQ][ATT_KEYS];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    const int D = H * 64;
    float* pr = part + (((size_t)q0 * H + (size_t)h * Lq) * nsplit + (size_t)s * Lq) * 66;
    const int L0 = len[b];
    const int n = min(L0 + Lq, cap);
    const int j0 = s * ATT_KEYS;
    if (skip || j0 >= n) {
        for (int r = t; r < Lq; r += ATT_KEYS) { pr[r * 66 + 64] = -INFINITY; pr[r * 66 + 65] = 0.f; }
        return;
    }
    for (int i = t; i < Lq * 64; i += ATT_KEYS) {
        const int r = i / 64, d = i % 64;
        const float q = qkv[(size_t)(q0 + r) * ldqkv + h * 64 + d];
        s_qu[r][d] = q + pbu[h * 64 + d];
        s_qv[r][d] = q + pbv[h * 64 + d];
    }
    __syncthreads();
    const int j = j0 + t;
    const size_t crow = ((size_t)(b * H + h) * cap + j) * 64;
    if (j < n) {
        const float* kp = j < L0 ? kc + crow : qkv + (size_t)(q0 + (j - L0)) * ldqkv + D + h * 64;
        f32x4 k[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) k[i] = reinterpret_cast<const f32x4*>(kp)[i];
        for (int r = 0; r < Lq; ++r) {
            const int dlt = L0 + r - j;
            float sc = -INFINITY;
            if (dlt >= 0 && L0 + r < cap) {
                const f32x4* pp = reinterpret_cast<const f32x4*>(P + (size_t)dlt * ldp + h * 64);
                float ac = 0.f, bd = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const f32x4 pv = pp[i];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        ac = fmaf(s_qu[r][4 * i + e], k[i][e], ac);
                        bd = fmaf(s_qv[r][4 * i + e], pv[e], bd);
                    }
                }
                sc = (ac + bd) * scale;
            }
            s_p[r][t] = sc;
        }
        if (j >= L0) {        // append the new row's K/V (nobody reads cache rows >= len[b] in this launch)
            const float* vp = qkv + (size_t)(q0 + (j - L0)) * ldqkv + 2 * D + h * 64;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                reinterpret_cast<f32x4*>(kc + crow)[i] = k[i];
                reinterpret_cast<f32x4*>(vc + crow)[i] = reinterpret_cast<const f32x4*>(vp)[i];
            }
        }
    } else {
        for (int r = 0; r < Lq; ++r) s_p[r][t] = -INFINITY;
    }
    __syncthreads();
    for (int r = wv; r < Lq; r += ATT_KEYS / WAVE) {
        float mx = -INFINITY;
        for (int i = lane; i < ATT_KEYS; i += WAVE) mx = fmaxf(mx, s_p[r][i]);
        mx = wave_max(mx);
        float l = 0.f;
        for (int i = lane; i < ATT_KEYS; i += WAVE) {
            const float p = mx == -INFINITY ? 0.f : expf(s_p[r][i] - mx);
            s_p[r][i] = p;
            l += p;
        }
        l = wave_sum(l);
        if (lane == 0) { pr[r * 66 + 64] = mx; pr[r * 66 + 65] = l; }
    }
    __syncthreads();
    const int cnt = min(ATT_KEYS, n - j0);
    for (int i = t; i < Lq * 64; i += ATT_KEYS) {
        const int r = i / 64, d = i % 64;
        float o = 0.f;
        for (int jj = 0; jj < cnt; ++jj) {
            const int jk = j0 + jj;
            const float vv = jk < L0 ? vc[((size_t)(b * H + h) * cap + jk) * 64 + d]
                                     : qkv[(size_t)(q0 + (jk - L0)) * ldqkv + 2 * D + h * 64 + d];
            o = fmaf(s_p[r][jj], vv, o);
        }
        pr[r * 66 + d] = o;
    }
}

// The two-stage max / sum combine of query row q0 + r, head h over the splits (one thread per channel).
__device__ __forceinline__ void decode_attn_combine_body(int q0, int Lq, int r, bool skip, int h, int H, int nsplit,
                                                         const float* __restrict__ part, float* __restrict__ o, int ldo) {
    const int d = threadIdx.x;
    const float* pr = part + ((size_t)q0 * H + (size_t)h * Lq) * nsplit * 66 + r * 66;
    float mx = -INFINITY;
    for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, pr[(size_t)s * Lq * 66 + 64]);
    float l = 0.f, acc = 0.f;
    if (mx != -INFINITY && !skip) {
        for (int s = 0; s < nsplit; ++s) {
            const float* ps = pr + (size_t)s * Lq * 66;
            const float ms = ps[64];
            if (ms == -INFINITY) continue;
            const float w = expf(ms - mx);
            l += ps[65] * w;
            acc += ps[d] * w;
        }
    }
    o[(size_t)(q0 + r) * ldo + h * 64 + d] = l > 0.f ? acc / l : 0.f;
}

__global__ __launch_bounds__(ATT_KEYS) void decode_attn_split_kernel(
    int H, int Lq, int cap, int nsplit, const float* __restrict__ qkv, int ldqkv, float* kc, float* vc,
    const int32_t* __restrict__ len, const int32_t* __restrict__ done, const float* __restrict__ P, int ldp,
    const float* __restrict__ pbu, const float* __restrict__ pbv, float scale, float* __restrict__ part) {
    const int b = blockIdx.z;
    decode_attn_split_body(b, b * Lq, Lq, done && done[b], blockIdx.x, blockIdx.y, H, cap, nsplit, qkv, ldqkv, kc, vc, len, P,
                           ldp, pbu, pbv, scale, part);
}

__global__ __launch_bounds__(64) void decode_attn_combine_kernel(int H, int Lq, int nsplit, const int32_t* __restrict__ done,
                                                                 const float* __restrict__ part, float* __restrict__ o,
                                                                 int ldo) {
    const int b = blockIdx.z;
    decode_attn_combine_body(b * Lq, Lq, blockIdx.x, done && done[b], blockIdx.y, H, nsplit, part, o, ldo);
}

// Ragged form: sequence z is the segment seg[z] = (cache row b, first activation row q0, Lq).  A segment that does not fit
// the launch (b outside [0, nrows), rows outside [0, M)) is skipped whole, so a bad table reads and writes nothing.
__device__ __forceinline__ bool decode_attn_segment(const int32_t* __restrict__ seg, int z, int M, int nrows, int& b, int& q0,
                                                    int& Lq) {
    b = seg[3 * z];
    q0 = seg[3 * z + 1];
    Lq = seg[3 * z + 2];
    return b >= 0 && b < nrows && q0 >= 0 && Lq >= 1 && Lq <= MAX_LQ && q0 + Lq <= M;
}

__global__ __launch_bounds__(ATT_KEYS) void decode_attn_ragged_split_kernel(
    const int32_t* __restrict__ seg, int M, int nrows, int H, int cap, int nsplit, const float* __restrict__ qkv, int ldqkv,
    float* kc, float* vc, const int32_t* __restrict__ len, const float* __restrict__ P, int ldp,
    const float* __restrict__ pbu, const float* __restrict__ pbv, float scale, float* __restrict__ part) {
    int b, q0, Lq;
    if (!decode_attn_segment(seg, blockIdx.z, M, nrows, b, q0, Lq)) return;
    decode_attn_split_body(b, q0, Lq, false, blockIdx.x, blockIdx.y, H, cap, nsplit, qkv, ldqkv, kc, vc, len, P, ldp, pbu,
                           pbv, scale, part);
}

__global__ __launch_bounds__(64) void decode_attn_ragged_combine_kernel(
    const int32_t* __restrict__ seg, int M, int nrows, int H, int nsplit, const float* __restrict__ part,
    float* __restrict__ o, int ldo) {
    int b, q0, Lq;
    if (!decode_attn_segment(seg, blockIdx.z, M, nrows, b, q0, Lq) || (int)blockIdx.x >= Lq) return;
    decode_attn_combine_body(q0, Lq, blockIdx.x, false, blockIdx.y, H, nsplit, part, o, ldo);
}

// ---------------------------------------------------------------- sampler
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// uniform in [0, 1) with 24 bits, keyed by (request seed, step, trial, draw) -- never by batch row
__device__ __forceinline__ float draw_u(uint64_t seed, int step, int trial, int draw) {
    const uint64_t c = ((uint64_t)(uint32_t)step << 32) | ((uint64_t)(uint32_t)trial << 8) | (uint64_t)(uint32_t)draw;
    return (float)(splitmix64(seed ^ splitmix64(c)) >> 40) * (1.0f / 16777216.0f);
}

template <bool MAX>
__device__ float block_reduce(float v, float* s_tmp) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    v = MAX ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if (lane == 0) s_tmp[wv] = v;
    __syncthreads();
    float r = s_tmp[0];
    for (int i = 1; i < SMP_THREADS / WAVE; ++i) r = MAX ? fmaxf(r, s_tmp[i]) : r + s_tmp[i];
    return r;
}

// inverse CDF over pr[0..V) in index order (torch.multinomial over the full softmax); all threads call, all get the id
__device__ int full_draw(const float* pr, int V, float u, float* s_chunk, int* s_pick) {
    const int t = threadIdx.x;
    const int per = (V + SMP_THREADS - 1) / SMP_THREADS;
    const int a = min(V, t * per), e = min(V, a + per);
    float cs = 0.f;
    for (int i = a; i < e; ++i) cs += pr[i];
    __syncthreads();
    s_chunk[t] = cs;
    __syncthreads();
    if (t == 0) {
        float tot = 0.f;
        for (int i = 0; i < SMP_THREADS; ++i) tot += s_chunk[i];
        const float target = u * tot;
        float run = 0.f;
        int pick = V - 1;
        for (int c = 0; c < SMP_THREADS; ++c) {
            const int ca = min(V, c * per), ce = min(V, ca + per);
            if (ca >= ce) continue;
            if (run + s_chunk[c] > target) {
                pick = ce - 1;
                for (int i = ca; i < ce; ++i) {
                    run += pr[i];
                    if (run > target) { pick = i; break; }
                }
                break;
            }
            run += s_chunk[c];
        }
        while (pick > 0 && pr[pick] <= 0.f) --pick;     // (rounding at the very end: never a zero-mass id)
        *s_pick = pick;
    }
    __syncthreads();
    return *s_pick;
}

__global__ __launch_bounds__(SMP_THREADS) void decode_sample_kernel(
    int V, const float* __restrict__ logits, int ldl, float* logp, int eos, int mode, int top_k, float top_p, int win,
    int rep_thr, const uint64_t* __restrict__ seeds, const float* __restrict__ uniforms, int32_t* tok, int32_t* next_in,
    int32_t* hist, int hist_cap, int32_t* nhist, int32_t* step, const int32_t* __restrict__ min_len,
    const int32_t* __restrict__ max_len, int32_t* len, int32_t* done, int32_t* err) {
    __shared__ float s_lp[SMP_VMAX];
    __shared__ float s_tmp[SMP_THREADS / WAVE];
    __shared__ float s_chunk[SMP_THREADS];
    __shared__ float s_cp[SMP_KMAX];
    __shared__ int s_ci[SMP_KMAX];
    __shared__ float s_bv[SMP_THREADS / WAVE];
    __shared__ int s_bi[SMP_THREADS / WAVE];
    __shared__ int s_pick, s_ncand;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    if (mode != 3 && done[b]) return;
    const float* x = logits + (size_t)b * ldl;
    // log_softmax: (x - max) - log(sum(exp(x - max)))
    float mx = -INFINITY;
    for (int i = t; i < V; i += SMP_THREADS) mx = fmaxf(mx, x[i]);
    mx = block_reduce<true>(mx, s_tmp);
    float se = 0.f;
    for (int i = t; i < V; i += SMP_THREADS) se += expf(x[i] - mx);
    const float lse = logf(block_reduce<false>(se, s_tmp));
    for (int i = t; i < V; i += SMP_THREADS) {
        const float v = (x[i] - mx) - lse;
        s_lp[i] = v;
        if (logp) logp[(size_t)b * V + i] = v;
    }
    if (mode == 3) return;
    const int st = step[b];
    __syncthreads();
    if (st == 0 && t == 0) s_lp[eos] = -INFINITY;      // llm.py:217-218
    __syncthreads();
    // probabilities = softmax(logp): exp(lp - max) / sum, kept in s_lp
    float m2 = -INFINITY;
    for (int i = t; i < V; i += SMP_THREADS) m2 = fmaxf(m2, s_lp[i]);
    m2 = block_reduce<true>(m2, s_tmp);
    float s2 = 0.f;
    for (int i = t; i < V; i += SMP_THREADS) s2 += expf(s_lp[i] - m2);
    s2 = block_reduce<false>(s2, s_tmp);
    for (int i = t; i < V; i += SMP_THREADS) s_lp[i] = expf(s_lp[i] - m2) / s2;
    __syncthreads();
    // nucleus candidates: the stable descending order (ties -> lower id), taken while cum < top_p and count < top_k
    if (mode <= 1) {
        float pv = INFINITY, cum = 0.f;
        int pi = -1, nc = 0;
        while (cum < top_p && nc < top_k) {
            float bv = -1.f;
            int bi = V;
            for (int i = t; i < V; i += SMP_THREADS) {
                const float p = s_lp[i];
                const bool after = p < pv || (p == pv && i > pi);
                if (after && (p > bv || (p == bv && i < bi))) { bv = p; bi = i; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            __syncthreads();
            if (lane == 0) { s_bv[wv] = bv; s_bi[wv] = bi; }
            __syncthreads();
            bv = s_bv[0]; bi = s_bi[0];
            for (int w = 1; w < SMP_THREADS / WAVE; ++w)
                if (s_bv[w] > bv || (s_bv[w] == bv && s_bi[w] < bi)) { bv = s_bv[w]; bi = s_bi[w]; }
            if (bi >= V) break;
            if (t == 0) { s_cp[nc] = bv; s_ci[nc] = bi; }
            cum += bv;
            pv = bv; pi = bi;
            ++nc;
        }
        if (t == 0) s_ncand = nc;
        __syncthreads();
    }
    const bool ignore_eos = st < min_len[b];
    const uint64_t seed = seeds ? seeds[b] : 0ull;
    int id = -1, trial = 0;
    for (; trial < SMP_TRIALS; ++trial) {
        __syncthreads();     // every thread has its copy of the previous trial's s_pick before thread 0 rewrites it
        const float u0 = uniforms ? uniforms[((size_t)b * SMP_TRIALS + trial) * 2] : draw_u(seed, st, trial, 0);
        const float u1 = uniforms ? uniforms[((size_t)b * SMP_TRIALS + trial) * 2 + 1] : draw_u(seed, st, trial, 1);
        if (mode == 2) {
            id = full_draw(s_lp, V, u0, s_chunk, &s_pick);
        } else {
            if (t == 0) {
                const int nc = s_ncand;
                float tot = 0.f;
                for (int c = 0; c < nc; ++c) tot += s_cp[c];
                const float target = u0 * tot;
                float run = 0.f;
                int pick = s_ci[nc - 1];
                for (int c = 0; c < nc; ++c) {
                    run += s_cp[c];
                    if (run > target) { pick = s_ci[c]; break; }
                }
                int rep = 0;
                if (mode == 0 && win > 0) {
                    const int nh = nhist[b], w = min(win, nh);
                    for (int q = 1; q <= w; ++q) rep += hist[(size_t)b * hist_cap + (nh - q) % hist_cap] == pick;
                }
                s_pick = pick;
                s_ncand = nc | ((mode == 0 && win > 0 && rep >= rep_thr) ? (1 << 30) : 0);
            }
            __syncthreads();
            id = s_pick;
            const bool ras = (s_ncand >> 30) & 1;
            __syncthreads();
            if (t == 0) s_ncand &= (1 << 30) - 1;
            if (ras) id = full_draw(s_lp, V, u1, s_chunk, &s_pick);   // ras_sampling's random_sampling fallback
        }
        if (!(ignore_eos && id == eos)) break;
    }
    if (t != 0) return;
    if (trial == SMP_TRIALS) {     // still EOS after 100 re-draws
        err[b] = 1;
        done[b] = 1;
        next_in[b] = -1;
        return;
    }
    tok[b] = id;
    if (id == eos) {
        done[b] = 1;
        next_in[b] = -1;
        return;
    }
    next_in[b] = id;
    const int nh = nhist[b];
    hist[(size_t)b * hist_cap + nh % hist_cap] = id;
    nhist[b] = nh + 1;
    if (len) len[b] += 1;
    step[b] = st + 1;
    if (st + 1 >= max_len[b]) done[b] = 1;
}

}  // namespace

extern "C" int cvft_decode_linear(int wdtype, int M, int N, int K, const float* X, int ldx, const float* ln_g,
                                  const float* ln_b, float ln_eps, const void* W, const float* bias, int act,
                                  const float* residual, int ldr, float* Y, int ldy, void* stream) {
    CVFT_CHECK_ARG(M >= 1 && M <= MAX_LQ, "cvft_decode_linear: M=%d outside [1, 16]", M);
    CVFT_CHECK_ARG(N >= 1 && K >= 8 && K % 8 == 0, "cvft_decode_linear: N=%d K=%d (K %% 8 == 0 required)", N, K);
    CVFT_CHECK_ARG(X && W && Y && ldx >= K && ldy >= N && (!residual || ldr >= N), "cvft_decode_linear: bad pointers / strides");
    CVFT_CHECK_ARG(ldx % 4 == 0 && ((uintptr_t)X & 15) == 0, "cvft_decode_linear: X rows must be 16-byte aligned");
    CVFT_CHECK_ARG(!ln_g == !ln_b, "cvft_decode_linear: ln_g and ln_b go together");
    CVFT_CHECK_ARG(act == 0 || act == 1, "cvft_decode_linear: act %d (0 none, 1 relu)", act);
    CVFT_CHECK_ARG(wdtype == 0 || wdtype == 1, "cvft_decode_linear: wdtype %d", wdtype);
    hipStream_t s = (hipStream_t)stream;
    if (wdtype == 0) launch_linear<float>(M, N, K, X, ldx, ln_g, ln_b, ln_eps, W, bias, act, residual, ldr, Y, ldy, s);
    else launch_linear<bf16_t>(M, N, K, X, ldx, ln_g, ln_b, ln_eps, W, bias, act, residual, ldr, Y, ldy, s);
    CVFT_LAUNCH_CHECK("cvft_decode_linear");
    return 0;
}

extern "C" int cvft_decode_lora_down(int wdtype, int M, int K, int S, int G, int R, const float* X, int ldx,
                                     const float* ln_g, const float* ln_b, float ln_eps, const void* A,
                                     const int32_t* slot, float* Z, int ldz, void* stream) {
    CVFT_CHECK_ARG(M >= 1 && M <= MAX_LQ, "cvft_decode_lora_down: M=%d outside [1, 16]", M);
    CVFT_CHECK_ARG(K >= 8 && K % 8 == 0 && S >= 1, "cvft_decode_lora_down: K=%d S=%d (K %% 8 == 0 required)", K, S);
    CVFT_CHECK_ARG(G == 1 || G == 3, "cvft_decode_lora_down: G=%d (1 or 3)", G);
    CVFT_CHECK_ARG(R == 8 || R == 16 || R == 32 || R == 64, "cvft_decode_lora_down: R=%d (8, 16, 32 or 64)", R);
    CVFT_CHECK_ARG(X && A && slot && Z && ldx >= K && ldz >= G * R, "cvft_decode_lora_down: bad pointers / strides");
    CVFT_CHECK_ARG(ldx % 4 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)A & 15) == 0,
                   "cvft_decode_lora_down: X rows and A must be 16-byte aligned");
    CVFT_CHECK_ARG(!ln_g == !ln_b, "cvft_decode_lora_down: ln_g and ln_b go together");
    CVFT_CHECK_ARG(!ln_g || ((((uintptr_t)ln_g) | ((uintptr_t)ln_b)) & 15) == 0, "cvft_decode_lora_down: ln_g / ln_b alignment");
    CVFT_CHECK_ARG(wdtype == 0 || wdtype == 1, "cvft_decode_lora_down: wdtype %d", wdtype);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(R / LD_J, G, M), blk(DL_THREADS);
    if (wdtype == 0)
        hipLaunchKernelGGL(decode_lora_down_kernel<float>, grid, blk, 0, s, K, S, G, R, X, ldx, ln_g, ln_b, ln_eps,
                           static_cast<const float*>(A), slot, Z, ldz);
    else
        hipLaunchKernelGGL(decode_lora_down_kernel<bf16_t>, grid, blk, 0, s, K, S, G, R, X, ldx, ln_g, ln_b, ln_eps,
                           static_cast<const bf16_t*>(A), slot, Z, ldz);
    CVFT_LAUNCH_CHECK("cvft_decode_lora_down");
    return 0;
}

extern "C" int cvft_decode_linear_lora(int wdtype, int M, int N, int K, const float* X, int ldx, const float* ln_g,
                                       const float* ln_b, float ln_eps, const void* W, const float* bias, int act,
                                       const float* residual, int ldr, float* Y, int ldy, int S, int G, int R,
                                       const void* Bst, const float* scale, const int32_t* slot, const float* Z, int ldz,
                                       void* stream) {
    CVFT_CHECK_ARG(M >= 1 && M <= MAX_LQ, "cvft_decode_linear_lora: M=%d outside [1, 16]", M);
    CVFT_CHECK_ARG(N >= 1 && K >= 8 && K % 8 == 0, "cvft_decode_linear_lora: N=%d K=%d (K %% 8 == 0 required)", N, K);
    CVFT_CHECK_ARG(X && W && Y && ldx >= K && ldy >= N && (!residual || ldr >= N), "cvft_decode_linear_lora: bad pointers / strides");
    CVFT_CHECK_ARG(ldx % 4 == 0 && ((uintptr_t)X & 15) == 0, "cvft_decode_linear_lora: X rows must be 16-byte aligned");
    CVFT_CHECK_ARG(!ln_g == !ln_b, "cvft_decode_linear_lora: ln_g and ln_b go together");
    CVFT_CHECK_ARG(act == 0 || act == 1, "cvft_decode_linear_lora: act %d (0 none, 1 relu)", act);
    CVFT_CHECK_ARG(wdtype == 0 || wdtype == 1, "cvft_decode_linear_lora: wdtype %d", wdtype);
    CVFT_CHECK_ARG(S >= 1 && (G == 1 || G == 3) && N % G == 0, "cvft_decode_linear_lora: S=%d G=%d N=%d (G 1 or 3, N %% G == 0)", S, G, N);
    CVFT_CHECK_ARG(R == 8 || R == 16 || R == 32 || R == 64, "cvft_decode_linear_lora: R=%d (8, 16, 32 or 64)", R);
    CVFT_CHECK_ARG(Bst && scale && slot && Z && ldz >= G * R && ldz % 4 == 0 && ((uintptr_t)Z & 15) == 0 &&
                       ((uintptr_t)Bst & 15) == 0, "cvft_decode_linear_lora: bad adapter pointers / strides");
    hipStream_t s = (hipStream_t)stream;
    if (wdtype == 0)
        launch_linear_lora<float>(M, N, K, X, ldx, ln_g, ln_b, ln_eps, W, bias, act, residual, ldr, Y, ldy, S, G, R, Bst,
                                  scale, slot, Z, ldz, s);
    else
        launch_linear_lora<bf16_t>(M, N, K, X, ldx, ln_g, ln_b, ln_eps, W, bias, act, residual, ldr, Y, ldy, S, G, R, Bst,
                                   scale, slot, Z, ldz, s);
    CVFT_LAUNCH_CHECK("cvft_decode_linear_lora");
    return 0;
}

extern "C" int cvft_decode_attn(int B, int H, int Lq, int cap, int nsplit, const float* qkv, int ldqkv, float* kc,
                                float* vc, const int32_t* len, const int32_t* done, const float* P, int ldp,
                                const float* pos_bias_u, const float* pos_bias_v, float scale, float* part, float* o,
                                int ldo, void* stream) {
    CVFT_CHECK_ARG(B >= 1 && H >= 1 && Lq >= 1 && Lq <= MAX_LQ, "cvft_decode_attn: B=%d H=%d Lq=%d (Lq <= 16)", B, H, Lq);
    CVFT_CHECK_ARG(cap >= 1 && nsplit >= 1 && (long)nsplit * ATT_KEYS >= cap, "cvft_decode_attn: nsplit*256 < cap (%d, %d)",
                   nsplit, cap);
    CVFT_CHECK_ARG(qkv && kc && vc && len && P && pos_bias_u && pos_bias_v && part && o, "cvft_decode_attn: null pointer");
    CVFT_CHECK_ARG(ldqkv >= 3 * H * 64 && ldqkv % 4 == 0 && ldp >= H * 64 && ldp % 4 == 0 && ldo >= H * 64,
                   "cvft_decode_attn: bad strides");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(decode_attn_split_kernel, dim3(nsplit, H, B), dim3(ATT_KEYS), 0, s, H, Lq, cap, nsplit, qkv, ldqkv,
                       kc, vc, len, done, P, ldp, pos_bias_u, pos_bias_v, scale, part);
    hipLaunchKernelGGL(decode_attn_combine_kernel, dim3(Lq, H, B), dim3(64), 0, s, H, Lq, nsplit, done, part, o, ldo);
    CVFT_LAUNCH_CHECK("cvft_decode_attn");
    return 0;
}

extern "C" int cvft_decode_attn_ragged(int nseg, int M, int nrows, int H, int cap, int nsplit, const int32_t* seg,
                                       const float* qkv, int ldqkv, float* kc, float* vc, const int32_t* len,
                                       const float* P, int ldp, const float* pos_bias_u, const float* pos_bias_v,
                                       float scale, float* part, float* o, int ldo, void* stream) {
    CVFT_CHECK_ARG(nseg >= 1 && nseg <= MAX_LQ && M >= nseg && M <= MAX_LQ && nrows >= 1 && H >= 1,
                   "cvft_decode_attn_ragged: nseg=%d M=%d nrows=%d H=%d (1 <= nseg <= M <= 16)", nseg, M, nrows, H);
    CVFT_CHECK_ARG(cap >= 1 && nsplit >= 1 && (long)nsplit * ATT_KEYS >= cap,
                   "cvft_decode_attn_ragged: nsplit*256 < cap (%d, %d)", nsplit, cap);
    CVFT_CHECK_ARG(seg && qkv && kc && vc && len && P && pos_bias_u && pos_bias_v && part && o,
                   "cvft_decode_attn_ragged: null pointer");
    CVFT_CHECK_ARG(ldqkv >= 3 * H * 64 && ldqkv % 4 == 0 && ldp >= H * 64 && ldp % 4 == 0 && ldo >= H * 64,
                   "cvft_decode_attn_ragged: bad strides");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(decode_attn_ragged_split_kernel, dim3(nsplit, H, nseg), dim3(ATT_KEYS), 0, s, seg, M, nrows, H, cap,
                       nsplit, qkv, ldqkv, kc, vc, len, P, ldp, pos_bias_u, pos_bias_v, scale, part);
    hipLaunchKernelGGL(decode_attn_ragged_combine_kernel, dim3(MAX_LQ, H, nseg), dim3(64), 0, s, seg, M, nrows, H, nsplit,
                       part, o, ldo);
    CVFT_LAUNCH_CHECK("cvft_decode_attn_ragged");
    return 0;
}

extern "C" int cvft_decode_sample(int B, int V, const float* logits, int ldl, float* logp, int eos, int mode, int top_k,
                                  float top_p, int win, int rep_thr, const uint64_t* seeds, const float* uniforms,
                                  int32_t* tok, int32_t* next_in, int32_t* hist, int hist_cap, int32_t* nhist,
                                  int32_t* step, const int32_t* min_len, const int32_t* max_len, int32_t* len,
                                  int32_t* done, int32_t* err, void* stream) {
    CVFT_CHECK_ARG(B >= 1 && V >= 2 && V <= SMP_VMAX && ldl >= V, "cvft_decode_sample: B=%d V=%d (V <= 8192)", B, V);
    CVFT_CHECK_ARG(mode >= 0 && mode <= 3, "cvft_decode_sample: mode %d", mode);
    CVFT_CHECK_ARG(logits && (mode == 3 || (eos >= 0 && eos < V)), "cvft_decode_sample: eos %d", eos);
    CVFT_CHECK_ARG(mode == 3 || (tok && next_in && hist && nhist && step && min_len && max_len && done && err),
                   "cvft_decode_sample: null state pointer");
    CVFT_CHECK_ARG(mode >= 2 || (top_k >= 1 && top_k <= SMP_KMAX && top_p > 0.f),
                   "cvft_decode_sample: top_k %d outside [1, 64] or top_p %g <= 0", top_k, (double)top_p);
    CVFT_CHECK_ARG(mode != 0 || (win >= 0 && win <= hist_cap && hist_cap >= 1), "cvft_decode_sample: win %d > hist_cap %d",
                   win, hist_cap);
    CVFT_CHECK_ARG(mode == 3 || seeds || uniforms, "cvft_decode_sample: seeds or uniforms required");
    hipLaunchKernelGGL(decode_sample_kernel, dim3(B), dim3(SMP_THREADS), 0, (hipStream_t)stream, V, logits, ldl, logp, eos,
                       mode, top_k, top_p, win, rep_thr, seeds, uniforms, tok, next_in, hist, hist_cap, nhist, step,
                       min_len, max_len, len, done, err);
    CVFT_LAUNCH_CHECK("cvft_decode_sample");
    return 0;
}
