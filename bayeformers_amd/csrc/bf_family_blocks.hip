// bf_family_blocks.hip — the memory-bound ops of Gemma 1 / 2 / 3 and Qwen3 decoder layers that bf_decoder_blocks.hip's
// three do not cover: norm -> residual add -> norm in one pass with Gemma's (1 + weight) convention (the "sandwich" of
// Gemma 2 / 3: HF Gemma2DecoderLayer.forward's post_attention_layernorm, add, pre_feedforward_layernorm), the rotary
// embedding at head size 256 with an optional per-head RMSNorm of q and k in front of it (Qwen3Attention / Gemma3Attention's
// q_norm and k_norm), and gelu_tanh(gate) * up (Gemma's MLP).  The framework runs each as a chain of elementwise kernels.
//
// The manner of bf_decoder_blocks.hip: 16-byte loads and stores (bf_vec8.h), fp32 arithmetic in registers, one rounding
// into the output dtype unless a comment names another, no allocation, no host synchronisation (capturable), no
// trigonometry.
#include "bf_common.h"
#include "bf_device.h"
#include "bf_vec8.h"

namespace {

constexpr int kRowsPerBlock = 4;  // waves per workgroup of the norm kernel

template <typename T>
__device__ __forceinline__ void round8(float (&v)[8]) {
    if constexpr (!__is_same(T, float)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)(T)v[i];
    }
}

// A double rounded once into T, as a float: through fp32 rounded to odd (truncated, the last bit set when anything was cut
// off), which the second rounding to a format 13 or 16 bits narrower cannot double-round; T = float takes the plain cast.
template <typename T>
__device__ __forceinline__ float round_f64(double d) {
    float f = (float)d;
    if constexpr (!__is_same(T, float)) {
        if ((double)f != d) {
            unsigned b = __builtin_bit_cast(unsigned, f);
            if (fabs((double)f) > fabs(d)) --b;  // sign and magnitude: one step towards zero
            f = (float)(T)__builtin_bit_cast(float, b | 1u);
        } else {
            f = (float)(T)f;
        }
    }
    return f;
}

// ---- norm -> residual add -> norm ------------------------------------------------------------------------------------------
// u = gamma_pre ? round_T(x * rstd(x) * (woff + gamma_pre)) : x,  z = res ? round_T(res + u) : u,
// y = round_T(z * rstd(z) * (woff + gamma_out)),  rstd(v) = rsqrt(mean(v^2) + eps).
// G lanes own a row and V 8-element vectors each (N / 8 <= G * V): G = 64, one wave per row, or G = 32, half a wave per row
// and two rows per wave for N = 256 V (add_rmsnorm_half_kernel's layout, every lane busy).  The row is loaded once and stays
// in registers across both reductions; every lane reads its elements of x and the residual before it writes anything, and
// writes only where it read, which makes sum_out == res and out == x safe.  Algorithmic bytes per row: N * (2 reads +
// 2 writes) * sizeof(T) with a residual and a sum output.
template <typename T, typename GT, int G, int V>
__global__ __launch_bounds__(64 * kRowsPerBlock) void norm_add_rmsnorm_kernel(const T* x, const GT* __restrict__ gamma_pre,
                                                                              const T* res, const GT* __restrict__ gamma_out,
                                                                              T* sum_out, T* out, long long rows, int N,
                                                                              float woff, float eps_pre, float eps_out) {
    constexpr int kPerWave = 64 / G;  // rows of a wave
    const int lane = threadIdx.x & 63, gl = lane % G, sub = lane / G;
    const long long row_raw = ((long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6)) * kPerWave + sub;
    if (row_raw - sub >= rows) return;                    // the whole wave is past the end
    const bool live = row_raw < rows;
    const long long row = live ? row_raw : rows - 1;      // the idle half of the last wave reads a valid row, writes nothing
    const int nvec = N >> 3;
    const float inv_n = 1.0f / (float)N;
    const T* xr = x + row * N;
    float v[V][8];
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const int vi = gl + G * c;
        if (vi < nvec) {
            load8(xr + vi * 8, v[c]);
#pragma unroll
            for (int i = 0; i < 8; ++i) sq = fmaf(v[c][i], v[c][i], sq);
        }
    }
    if (gamma_pre) {  // (a kernel argument: the same way for every lane)
        // The first norm runs in fp64.  u is rounded to T and then feeds an add that is rounded again, so an fp32
        // evaluation error here (a few 2^-24) would carry about one u in 2^13 across a rounding boundary of a 16-bit T —
        // a whole spacing of u, where the framework's fp32 chain and a float64 restatement agree on the other side; in
        // fp64, rounded once (round_f64), u is the restatement's.  Some 6 fp64-rate instructions per element against 8 bytes of traffic.
        double sqd = 0.0;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            if (gl + G * c < nvec)
#pragma unroll
                for (int i = 0; i < 8; ++i) sqd = fma((double)v[c][i], (double)v[c][i], sqd);
        }
#pragma unroll
        for (int m = G / 2; m; m >>= 1) sqd += __shfl_xor(sqd, m);  // every lane of the row ends with the same sum
        const double rstd = 1.0 / sqrt(sqd / (double)N + (double)eps_pre);
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const int vi = gl + G * c;
            if (vi < nvec) {
                float g[8];
                load8(gamma_pre + vi * 8, g);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[c][i] = round_f64<T>(((double)v[c][i] * rstd) * ((double)woff + (double)g[i]));
            }
        }
    }
    if (res || gamma_pre) {  // z differs from x: add, and take the statistics again from the rounded z
        const T* rr = res ? res + row * N : nullptr;
        sq = 0.f;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const int vi = gl + G * c;
            if (vi < nvec) {
                if (rr) {
                    float r[8];
                    load8(rr + vi * 8, r);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[c][i] += r[i];
                    round8<T>(v[c]);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) sq = fmaf(v[c][i], v[c][i], sq);
            }
        }
    }
    if (sum_out && live) {
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const int vi = gl + G * c;
            if (vi < nvec) store8(sum_out + row * N + vi * 8, v[c]);
        }
    }
    if constexpr (G == 32) sq = half_sum(sq, lane);
    else sq = wave_sum(sq);
    const float rstd = 1.0f / sqrtf(sq * inv_n + eps_out);
    if (!live) return;
    T* orow = out + row * N;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const int vi = gl + G * c;
        if (vi < nvec) {
            float g[8], o[8];
            load8(gamma_out + vi * 8, g);
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = (v[c][i] * rstd) * (woff + g[i]);
            store8(orow + vi * 8, o);
        }
    }
}

template <typename T, typename GT>
int launch_norm_add(const void* x, const void* gpre, const void* res, const void* gout, void* sum_out, void* out, long long rows,
                    int N, float woff, float eps_pre, float eps_out, hipStream_t stream) {
    const int nvec = N >> 3;
    const dim3 block(64 * kRowsPerBlock);
#define BF_NAN_LAUNCH(G_, V_)                                                                                                 \
    hipLaunchKernelGGL((norm_add_rmsnorm_kernel<T, GT, G_, V_>), grid, block, 0, stream, (const T*)x, (const GT*)gpre,          \
                       (const T*)res, (const GT*)gout, (T*)sum_out, (T*)out, rows, N, woff, eps_pre, eps_out)
    if (nvec % 32 == 0 && nvec <= 128) {
        const dim3 grid((unsigned)((rows + 2 * kRowsPerBlock - 1) / (2 * kRowsPerBlock)));
        switch (nvec / 32) {
            case 1: BF_NAN_LAUNCH(32, 1); break;
            case 2: BF_NAN_LAUNCH(32, 2); break;
            case 3: BF_NAN_LAUNCH(32, 3); break;
            default: BF_NAN_LAUNCH(32, 4); break;
        }
    } else {
        const dim3 grid((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock));
        if (nvec <= 64) BF_NAN_LAUNCH(64, 1);
        else if (nvec <= 128) BF_NAN_LAUNCH(64, 2);
        else if (nvec <= 256) BF_NAN_LAUNCH(64, 4);
        else if (nvec <= 512) BF_NAN_LAUNCH(64, 8);
        else BF_NAN_LAUNCH(64, 16);
    }
#undef BF_NAN_LAUNCH
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int launch_norm_add_gt(const void* x, const void* gpre, const void* res, const void* gout, int param_dtype, void* sum_out,
                       void* out, long long rows, int N, float woff, float eps_pre, float eps_out, hipStream_t stream) {
    if (param_dtype == BF_DT_F32)
        return launch_norm_add<T, float>(x, gpre, res, gout, sum_out, out, rows, N, woff, eps_pre, eps_out, stream);
    return launch_norm_add<T, T>(x, gpre, res, gout, sum_out, out, rows, N, woff, eps_pre, eps_out, stream);
}

// ---- per-head RMSNorm of q and k, then the rotary embedding -------------------------------------------------------------------
// rope_qk_kernel's work split (bf_decoder_blocks.hip): one lane owns 8 elements of a head's first half and their 8 partners
// of the second, loads both, then stores both — the in-place form is safe — and lanes run over (token row, head of q then of
// k, vector) with the heads fastest.  NORM: the D / 16 lanes that own a head first normalise it,
// n = x * rsqrt(mean_D(x^2) + eps) * (woff + gamma), in fp32 and unrounded; the sum of squares crosses the lanes by xor
// shuffles.  Without NORM the arithmetic is rope_qk_kernel's, expression for expression.
struct qkrope_args_t {
    int T, H, Hkv, cos_batch;
    unsigned total;  // lanes of work: B * T * (H + Hkv) * D / 16
    float woff, eps;
    long long q[3], k[3], qo[3], ko[3];
};

template <typename T, typename CT, typename GT, int D, bool NORM>
__global__ __launch_bounds__(256) void qknorm_rope_kernel(const T* q, const T* k, const CT* __restrict__ cosp,
                                                          const CT* __restrict__ sinp, const GT* __restrict__ gamma_q,
                                                          const GT* __restrict__ gamma_k, T* q_out, T* k_out,
                                                          const qkrope_args_t a) {
    constexpr int kVec = D / 16;  // lanes per head: 4, 8 or 16, an aligned power-of-two group of a wave
    const unsigned per_row = (unsigned)(a.H + a.Hkv) * kVec;
    // idx % kVec is the lane's place in its head (per_row is a multiple of kVec) and, the workgroup's first idx and the
    // stride gridDim.x * 256 being multiples of 64, also threadIdx.x % kVec: a head's lanes are kVec neighbours of one wave.
    // total and the stride are both multiples of kVec (of 16 for every D: total = rows * heads * kVec, stride a multiple of
    // 256), so `idx < total` holds or fails for a whole group at once — the shuffles below never read a lane that left.
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.total; idx += gridDim.x * 256u) {
        const unsigned r = idx / per_row, l = idx - r * per_row;
        const unsigned b = r / (unsigned)a.T, t = r - b * (unsigned)a.T;
        const int hh = (int)(l / kVec), j = (int)(l % kVec);
        const bool is_q = hh < a.H;
        const int h = is_q ? hh : hh - a.H;
        const long long* si = is_q ? a.q : a.k;
        const long long* so = is_q ? a.qo : a.ko;
        const T* src = (is_q ? q : k) + b * si[0] + h * si[1] + t * si[2] + j * 8;
        T* dst = (is_q ? q_out : k_out) + b * so[0] + h * so[1] + t * so[2] + j * 8;
        const long long cs = ((long long)(a.cos_batch > 1 ? b : 0) * a.T + t) * D + j * 8;
        float x1[8], x2[8], c1[8], c2[8], s1[8], s2[8], o1[8], o2[8];
        load8(src, x1);
        load8(src + D / 2, x2);
        load8(cosp + cs, c1);
        load8(cosp + cs + D / 2, c2);
        load8(sinp + cs, s1);
        load8(sinp + cs + D / 2, s2);
        if constexpr (NORM) {
            float sq = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) sq = fmaf(x1[i], x1[i], sq);
#pragma unroll
            for (int i = 0; i < 8; ++i) sq = fmaf(x2[i], x2[i], sq);
#pragma unroll
            for (int m = kVec / 2; m; m >>= 1) sq += __shfl_xor(sq, m);  // every lane of the head ends with the same sum
            const GT* gm = is_q ? gamma_q : gamma_k;                     // (the same for the whole group)
            if (gm) {
                const float rstd = 1.0f / sqrtf(sq * (1.0f / (float)D) + a.eps);
                float g1[8], g2[8];
                load8(gm + j * 8, g1);
                load8(gm + j * 8 + D / 2, g2);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    x1[i] = (x1[i] * rstd) * (a.woff + g1[i]);
                    x2[i] = (x2[i] * rstd) * (a.woff + g2[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            o1[i] = fmaf(x1[i], c1[i], -(x2[i] * s1[i]));
            o2[i] = fmaf(x2[i], c2[i], x1[i] * s2[i]);
        }
        store8(dst, o1);
        store8(dst + D / 2, o2);
    }
}

template <typename T, typename CT, typename GT, bool NORM>
int launch_qkrope(const void* q, const void* k, const void* c, const void* s, const void* gq, const void* gk, void* qo, void* ko,
                  int D, const qkrope_args_t& a, hipStream_t stream) {
    const unsigned blocks = (a.total + 255u) / 256u;
    const dim3 grid(blocks < 4096u ? blocks : 4096u), block(256);
#define BF_QKR_LAUNCH(D_)                                                                                                     \
    hipLaunchKernelGGL((qknorm_rope_kernel<T, CT, GT, D_, NORM>), grid, block, 0, stream, (const T*)q, (const T*)k, (const CT*)c, \
                       (const CT*)s, (const GT*)gq, (const GT*)gk, (T*)qo, (T*)ko, a)
    if (D == 64) BF_QKR_LAUNCH(64);
    else if (D == 128) BF_QKR_LAUNCH(128);
    else BF_QKR_LAUNCH(256);
#undef BF_QKR_LAUNCH
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T, typename CT>
int launch_qkrope_gt(const void* q, const void* k, const void* c, const void* s, const void* gq, const void* gk, int param_dtype,
                     void* qo, void* ko, int D, const qkrope_args_t& a, hipStream_t stream) {
    if (!gq && !gk) return launch_qkrope<T, CT, float, false>(q, k, c, s, nullptr, nullptr, qo, ko, D, a, stream);
    if (param_dtype == BF_DT_F32) return launch_qkrope<T, CT, float, true>(q, k, c, s, gq, gk, qo, ko, D, a, stream);
    return launch_qkrope<T, CT, T, true>(q, k, c, s, gq, gk, qo, ko, D, a, stream);
}

template <typename T>
int launch_qkrope_ct(const void* q, const void* k, const void* c, const void* s, int cs_dtype, const void* gq, const void* gk,
                     int param_dtype, void* qo, void* ko, int D, const qkrope_args_t& a, hipStream_t stream) {
    if (cs_dtype == BF_DT_F32) return launch_qkrope_gt<T, float>(q, k, c, s, gq, gk, param_dtype, qo, ko, D, a, stream);
    return launch_qkrope_gt<T, T>(q, k, c, s, gq, gk, param_dtype, qo, ko, D, a, stream);
}

// ---- gelu_tanh(gate) * up -----------------------------------------------------------------------------------------------------
// 0.5 g (1 + tanh k) = g / (1 + exp(-2 k)) with k = sqrt(2/pi) (g + 0.044715 g^3): the quotient form has no 1 + tanh k that
// cancels for negative gates.  It is evaluated through e = exp(-|2k|) in (0, 1] — the sigmoid is 1 / (1 + e) for a positive
// gate and e / (1 + e) for a negative one — so nothing overflows: for negative gates the result follows e down through the
// subnormals to -0 instead of dropping to 0 where exp(88.8) would be inf while g u / exp(88.8) is still a normal number, and
// g^2 beyond fp32's range gives e = 0 and the two limits (g u and -0): finite wherever gate * up is.  The argument
// 2k = g (2c + 2c 0.044715 g^2) is formed in fp64 and rounded to fp32 once: where e dominates the result an absolute error of
// the argument is a relative error of y, and the argument passes 100 before e leaves the normal range — one rounding costs
// 100 * 2^-24, the four of an fp32 evaluation would cost most of the 2^-16 the result is held to.  Three fp64 operations per
// element, against 6 bytes of traffic.
// swiglu_kernel's grid: blockIdx.x: 256 vectors of a row, blockIdx.y: rows blockIdx.y, + gridDim.y, ...
template <typename T>
__global__ __launch_bounds__(256) void geglu_kernel(const T* gate, long long gate_stride, const T* up, long long up_stride, T* out,
                                                    long long out_stride, long long rows, int nvec) {
    constexpr double k2c = 1.5957691216057308;        // 2 sqrt(2 / pi)
    constexpr double k2ca = k2c * 0.044715;
    const int vi = blockIdx.x * 256 + threadIdx.x;
    if (vi >= nvec) return;
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        float g[8], u[8], o[8];
        load8(gate + row * gate_stride + vi * 8, g);
        load8(up + row * up_stride + vi * 8, u);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double gd = (double)g[i];
            const float arg = (float)(gd * fma(gd * gd, k2ca, k2c));  // 2k; +-inf beyond fp32's range
            const float e = expf(-fabsf(arg));
            const float s = (arg >= 0.f ? 1.0f : e) / (1.0f + e);
            o[i] = g[i] * s * u[i];
        }
        store8(out + row * out_stride + vi * 8, o);
    }
}

template <typename T>
int launch_geglu(const void* gate, long long gs, const void* up, long long us, void* out, long long os, long long rows, int N,
                 hipStream_t stream) {
    const int nvec = N >> 3;
    const unsigned gx = (unsigned)((nvec + 255) / 256);
    const long long want = 8192 / gx > 0 ? 8192 / gx : 1;  // about 8192 workgroups at most, the rest by the row loop
    const unsigned gy = (unsigned)(rows < want ? rows : want);
    hipLaunchKernelGGL((geglu_kernel<T>), dim3(gx, gy), dim3(256), 0, stream, (const T*)gate, gs, (const T*)up, us, (T*)out, os,
                       rows, nvec);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

bool strides_ok(const int64_t* s) { return s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && !((s[0] | s[1] | s[2]) & 7); }

}  // namespace

int bf_norm_add_rmsnorm(const void* d_x, const void* d_gamma_pre, const void* d_residual, const void* d_gamma_out,
                        int param_dtype, int weight_offset, void* d_sum_out, void* d_out, int dtype, int64_t rows, int N,
                        float eps_pre, float eps_out, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("bf_norm_add_rmsnorm: bad shape rows=%lld N=%d", (long long)rows, N);
    if (N % 8 || N > 8192) BF_FAIL("bf_norm_add_rmsnorm: N=%d must be a multiple of 8 and at most 8192", N);
    if (!d_x || !d_gamma_out || !d_out) BF_FAIL("bf_norm_add_rmsnorm: null pointer");
    if (rows > 0x7fffffffLL * kRowsPerBlock) BF_FAIL("bf_norm_add_rmsnorm: too many rows");
    const uintptr_t al = (uintptr_t)d_x | (uintptr_t)d_gamma_pre | (uintptr_t)d_residual | (uintptr_t)d_gamma_out |
                         (uintptr_t)d_sum_out | (uintptr_t)d_out;
    if (al & 15) BF_FAIL("bf_norm_add_rmsnorm: pointers must be 16-byte aligned");
    if (weight_offset != 0 && weight_offset != 1) BF_FAIL("bf_norm_add_rmsnorm: weight_offset=%d must be 0 or 1", weight_offset);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_norm_add_rmsnorm: unknown dtype %d", dtype);
    if (param_dtype != BF_DT_F32 && param_dtype != dtype)
        BF_FAIL("bf_norm_add_rmsnorm: the gammas must be fp32 or have the activation dtype");
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const float woff = (float)weight_offset;
#define BF_NAN_ARGS d_x, d_gamma_pre, d_residual, d_gamma_out, param_dtype, d_sum_out, d_out, rows, N, woff, eps_pre, eps_out, st
    switch (dtype) {
        case BF_DT_BF16: return launch_norm_add_gt<__bf16>(BF_NAN_ARGS);
        case BF_DT_F16: return launch_norm_add_gt<_Float16>(BF_NAN_ARGS);
        default: return launch_norm_add_gt<float>(BF_NAN_ARGS);
    }
#undef BF_NAN_ARGS
}

int bf_qknorm_rope(const void* d_q, const void* d_k, const void* d_cos, const void* d_sin, int cs_dtype,
                   const void* d_gamma_q, const void* d_gamma_k, int param_dtype, int weight_offset, float eps,
                   void* d_q_out, void* d_k_out, int dtype, const bf_rope_t* shape, void* stream) {
    if (!shape) BF_FAIL("bf_qknorm_rope: shape is NULL");
    const bf_rope_t& s = *shape;
    if (s.head_dim != 64 && s.head_dim != 128 && s.head_dim != 256)
        BF_FAIL("bf_qknorm_rope: head_dim=%d must be 64, 128 or 256", s.head_dim);
    if (s.B < 0 || s.T < 1 || s.H < 1 || s.Hkv < 1)
        BF_FAIL("bf_qknorm_rope: bad shape B=%d T=%d H=%d Hkv=%d", s.B, s.T, s.H, s.Hkv);
    if (s.cos_batch != 1 && s.cos_batch != s.B) BF_FAIL("bf_qknorm_rope: cos_batch=%d must be 1 or B=%d", s.cos_batch, s.B);
    if (!d_q || !d_k || !d_cos || !d_sin || !d_q_out || !d_k_out) BF_FAIL("bf_qknorm_rope: null pointer");
    const uintptr_t al = (uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_cos | (uintptr_t)d_sin | (uintptr_t)d_q_out |
                         (uintptr_t)d_k_out | (uintptr_t)d_gamma_q | (uintptr_t)d_gamma_k;
    if (al & 15) BF_FAIL("bf_qknorm_rope: pointers must be 16-byte aligned");
    if (!strides_ok(s.q_stride) || !strides_ok(s.k_stride) || !strides_ok(s.q_out_stride) || !strides_ok(s.k_out_stride))
        BF_FAIL("bf_qknorm_rope: strides must be non-negative multiples of 8 elements");
    if (weight_offset != 0 && weight_offset != 1) BF_FAIL("bf_qknorm_rope: weight_offset=%d must be 0 or 1", weight_offset);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_qknorm_rope: unknown dtype %d", dtype);
    if (cs_dtype != BF_DT_F32 && cs_dtype != dtype) BF_FAIL("bf_qknorm_rope: cos / sin must be fp32 or have the activation dtype");
    if ((d_gamma_q || d_gamma_k) && param_dtype != BF_DT_F32 && param_dtype != dtype)
        BF_FAIL("bf_qknorm_rope: the gammas must be fp32 or have the activation dtype");
    const long long total = (long long)s.B * s.T * (s.H + s.Hkv) * (s.head_dim / 16);
    if (total > 0x7fffffffLL) BF_FAIL("bf_qknorm_rope: B * T * (H + Hkv) * head_dim / 16 = %lld exceeds 2^31 - 1", total);
    if (total == 0) return 0;
    qkrope_args_t a;
    a.T = s.T, a.H = s.H, a.Hkv = s.Hkv, a.cos_batch = s.cos_batch, a.total = (unsigned)total;
    a.woff = (float)weight_offset, a.eps = eps;
    for (int i = 0; i < 3; ++i)
        a.q[i] = s.q_stride[i], a.k[i] = s.k_stride[i], a.qo[i] = s.q_out_stride[i], a.ko[i] = s.k_out_stride[i];
    hipStream_t st = (hipStream_t)stream;
#define BF_QKR_ARGS d_q, d_k, d_cos, d_sin, cs_dtype, d_gamma_q, d_gamma_k, param_dtype, d_q_out, d_k_out, s.head_dim, a, st
    switch (dtype) {
        case BF_DT_BF16: return launch_qkrope_ct<__bf16>(BF_QKR_ARGS);
        case BF_DT_F16: return launch_qkrope_ct<_Float16>(BF_QKR_ARGS);
        default: return launch_qkrope_ct<float>(BF_QKR_ARGS);
    }
#undef BF_QKR_ARGS
}

int bf_geglu(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, void* d_out,
             int64_t out_row_stride, int dtype, int64_t rows, int N, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("bf_geglu: bad shape rows=%lld N=%d", (long long)rows, N);
    if (N % 8) BF_FAIL("bf_geglu: N=%d must be a multiple of 8", N);
    if (!d_gate || !d_up || !d_out) BF_FAIL("bf_geglu: null pointer");
    if (((uintptr_t)d_gate | (uintptr_t)d_up | (uintptr_t)d_out) & 15) BF_FAIL("bf_geglu: pointers must be 16-byte aligned");
    if (gate_row_stride < N || up_row_stride < N || out_row_stride < N || ((gate_row_stride | up_row_stride | out_row_stride) & 7))
        BF_FAIL("bf_geglu: row strides (%lld, %lld, %lld) must be multiples of 8 and at least N=%d", (long long)gate_row_stride,
                (long long)up_row_stride, (long long)out_row_stride, N);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_geglu: unknown dtype %d", dtype);
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case BF_DT_BF16: return launch_geglu<__bf16>(d_gate, gate_row_stride, d_up, up_row_stride, d_out, out_row_stride, rows, N, st);
        case BF_DT_F16: return launch_geglu<_Float16>(d_gate, gate_row_stride, d_up, up_row_stride, d_out, out_row_stride, rows, N, st);
        default: return launch_geglu<float>(d_gate, gate_row_stride, d_up, up_row_stride, d_out, out_row_stride, rows, N, st);
    }
}
