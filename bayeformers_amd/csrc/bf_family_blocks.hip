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

// ==== the backward of the three ops ===========================================================================================
// bf_decoder_blocks.hip's backward half with the families' additions: the second norm in front of the add, the weight
// offset, the per-head norm in front of the rotation, the tanh-GELU gate.  No float atomics: every parameter gradient leaves
// a workgroup as one fp32 row of partial sums, and dgamma_rows_kernel adds the rows in a fixed order.
namespace {

constexpr int kBwdBlocks = 1024;      // workgroups at most (each leaves one row of partial sums)
constexpr int kBwdBlocksWide = 512;   // ... of the one-row-per-workgroup form of the norm (N > 2048)

template <int G>
__device__ __forceinline__ double group_sum_f64(double v) {
#pragma unroll
    for (int m = (G < 64 ? G : 64) / 2; m; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// out[n] = sum over the workgroups' partial rows [nblocks, W]; columns [0, N) go to out0, [N, W) to out1 (W = N or 2 N; a
// NULL output is skipped).  rmsnorm_dgamma_kernel's shape: 16 columns x 64 lanes over the workgroup axis; fixed order.
__global__ __launch_bounds__(1024) void dgamma_rows_kernel(const float* __restrict__ partial, int nblocks, int W, int N,
                                                           float* __restrict__ out0, float* __restrict__ out1) {
    __shared__ float sh[64][16];
    const int c = threadIdx.x & 15, n = blockIdx.x * 16 + c, cl = threadIdx.x >> 4;
    float acc = 0.f;
    if (n < W)
        for (int b = cl; b < nblocks; b += 64) acc += partial[(long long)b * W + n];
    sh[cl][c] = acc;
    __syncthreads();
    if (cl == 0 && n < W) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 64; ++i) t += sh[i][c];
        if (n < N) {
            if (out0) out0[n] = t;
        } else if (out1) {
            out1[n - N] = t;
        }
    }
}

// ---- norm -> residual add -> norm ------------------------------------------------------------------------------------------
// Stage 2, the norm behind the add, from the stored z, with r_z = rsqrt(mean(z^2) + eps_out), a = (woff + gamma_out) o dy:
//     dz = r_z a - z r_z^3 mean(z o a) + dz_in,      dgamma_out = sum_rows dy o z r_z
// (dy == NULL, only the sum was consumed: dz = dz_in, dgamma_out = 0).  dz is the gradient of the residual.
// Stage 1 (PRE), the norm in front of the add, with dz taken unrounded from the registers, b = (woff + gamma_pre) o dz:
//     dx = r_x b - x r_x^3 mean(x o b),              dgamma_pre = sum_rows dz o x r_x.
// add_rmsnorm_bwd_kernel's layouts (G lanes own a row, V vectors per lane: G = 32 for N = 256 .. 1024 in steps of 256,
// G = 64 up to N = 2048, the whole workgroup on one row up to 8192), its walk over the rows and its precision: both sums of
// squares in fp64, each dgamma term formed in fp64 and added to the fp32 partial with one rounding.  What it keeps in
// registers is the row (z, x, dy) and the two sets of dgamma partials, 5 x 8 V floats; the gammas are read again for every
// row (from L2: [N] values that every workgroup reads) instead of taking two more sets.  Every lane reads all it needs of a
// row before it writes, and writes only where it read: dz may be dy or dz_in, dx may be dz.  The workgroup's partials are
// one [W] row, W = N or (PRE) 2 N with dgamma_pre in the second half.  Algorithmic bytes per row: N * (2 reads + 1 write)
// * sizeof(T), + 1 read with dz_in, + 1 read and 1 write with gamma_pre.
template <typename T, typename GT, int G, int V, bool PRE>
__global__ __launch_bounds__(256) void norm_add_rmsnorm_bwd_kernel(const T* x, const T* z, const GT* __restrict__ gamma_pre,
                                                                   const GT* __restrict__ gamma_out, const T* dy,
                                                                   const T* dz_in, T* dz, T* dx, float* __restrict__ partial,
                                                                   long long rows, int N, float woff, float eps_pre,
                                                                   float eps_out) {
    constexpr int kGroups = 256 / G;  // rows in flight per workgroup
    extern __shared__ float sh[];     // [W] (kGroups > 1)
    __shared__ double red_sq[2][4];
    __shared__ float red_s[2][4];
    const int lane = threadIdx.x & 63, gl = threadIdx.x % G, sub = threadIdx.x / G;
    const int nvec = N >> 3;
    const int W = PRE ? 2 * N : N;
    float dgo[V][8], dgp[PRE ? V : 1][8];
#pragma unroll
    for (int c = 0; c < V; ++c)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            dgo[c][i] = 0.f;
            if constexpr (PRE) dgp[c][i] = 0.f;
        }
    const float inv_n = 1.0f / (float)N;
    for (long long base = (long long)blockIdx.x * kGroups; base < rows; base += (long long)gridDim.x * kGroups) {
        const bool live = base + sub < rows;
        const long long row = live ? base + sub : rows - 1;  // an idle group of the last round reads a valid row, writes nothing
        float v[V][8], g[V][8], xv[PRE ? V : 1][8];
        double sq = 0.0, sqx = 0.0;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const int vi = gl + G * c;
            if (vi < nvec) {
                load8(z + row * N + vi * 8, v[c]);
                if constexpr (PRE) {
                    load8(x + row * N + vi * 8, xv[c]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) sqx = fma((double)xv[c][i], (double)xv[c][i], sqx);
                }
                if (dy) {  // (a kernel argument: the same way for every lane)
                    float gm[8];
                    load8(dy + row * N + vi * 8, g[c]);
                    load8(gamma_out + vi * 8, gm);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        sq = fma((double)v[c][i], (double)v[c][i], sq);
                        s = fmaf(g[c][i] * (woff + gm[i]), v[c][i], s);
                    }
                }
            }
        }
        double rd = 0.0;
        float r = 0.f, k = 0.f;
        if (dy) {
            sq = group_sum_f64<G>(sq);
            if constexpr (G == 32) s = half_sum(s, lane);
            else s = wave_sum(s);
            if constexpr (G == 256) {
                if (lane == 0) red_sq[0][threadIdx.x >> 6] = sq, red_s[0][threadIdx.x >> 6] = s;
                __syncthreads();
                sq = ((red_sq[0][0] + red_sq[0][1]) + red_sq[0][2]) + red_sq[0][3];
                s = ((red_s[0][0] + red_s[0][1]) + red_s[0][2]) + red_s[0][3];
            }
            rd = 1.0 / sqrt(sq / (double)N + (double)eps_out);
            r = (float)rd;
            k = r * r * r * (s * inv_n);
        }
        // g becomes dz, unrounded; the dgamma_out terms leave with dy
        float sx = 0.f;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const int vi = gl + G * c;
            if (vi < nvec) {
                if (dy) {
                    float gm[8];
                    load8(gamma_out + vi * 8, gm);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        // dy z is exact in fp64, r unrounded: the one rounding of a step is the sum's, back to fp32
                        if (live) dgo[c][i] = (float)fma((double)g[c][i] * (double)v[c][i], rd, (double)dgo[c][i]);
                        g[c][i] = fmaf(-v[c][i], k, r * (g[c][i] * (woff + gm[i])));
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) g[c][i] = 0.f;
                }
                if (dz_in) {  // the sum had a second consumer: its gradient is added here, in fp32, not by a pass of its own
                    float h[8];
                    load8(dz_in + row * N + vi * 8, h);
#pragma unroll
                    for (int i = 0; i < 8; ++i) g[c][i] += h[i];
                }
                if constexpr (PRE) {
                    float gm[8];
                    load8(gamma_pre + vi * 8, gm);
#pragma unroll
                    for (int i = 0; i < 8; ++i) sx = fmaf(g[c][i] * (woff + gm[i]), xv[c][i], sx);
                }
            }
        }
        if constexpr (PRE) {
            sqx = group_sum_f64<G>(sqx);
            if constexpr (G == 32) sx = half_sum(sx, lane);
            else sx = wave_sum(sx);
            if constexpr (G == 256) {
                if (lane == 0) red_sq[1][threadIdx.x >> 6] = sqx, red_s[1][threadIdx.x >> 6] = sx;
                __syncthreads();
                sqx = ((red_sq[1][0] + red_sq[1][1]) + red_sq[1][2]) + red_sq[1][3];
                sx = ((red_s[1][0] + red_s[1][1]) + red_s[1][2]) + red_s[1][3];
            }
            const double rdx = 1.0 / sqrt(sqx / (double)N + (double)eps_pre);
            const float rx = (float)rdx;
            const float kx = rx * rx * rx * (sx * inv_n);
            if (live) {
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    const int vi = gl + G * c;
                    if (vi < nvec) {
                        float gm[8], o[8];
                        load8(gamma_pre + vi * 8, gm);
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            dgp[c][i] = (float)fma((double)g[c][i] * (double)xv[c][i], rdx, (double)dgp[c][i]);
                            o[i] = fmaf(-xv[c][i], kx, rx * (g[c][i] * (woff + gm[i])));
                        }
                        if (dz) store8(dz + row * N + vi * 8, g[c]);
                        store8(dx + row * N + vi * 8, o);
                    }
                }
            }
        } else if (live) {
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const int vi = gl + G * c;
                if (vi < nvec) store8(dz + row * N + vi * 8, g[c]);
            }
        }
        if constexpr (G == 256) __syncthreads();  // red_* are free for the next row
    }
    float* prow = partial + (long long)blockIdx.x * W;
    if constexpr (kGroups == 1) {
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const int vi = gl + G * c;
            if (vi < nvec)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    prow[vi * 8 + i] = dgo[c][i];
                    if constexpr (PRE) prow[N + vi * 8 + i] = dgp[c][i];
                }
        }
    } else {
        for (int grp = 0; grp < kGroups; ++grp) {  // group 0 stores, 1 .. kGroups - 1 add in turn: one fixed order
            if (sub == grp) {
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    const int vi = gl + G * c;
                    if (vi < nvec)
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const int n = vi * 8 + i;
                            sh[n] = grp ? sh[n] + dgo[c][i] : dgo[c][i];
                            if constexpr (PRE) sh[N + n] = grp ? sh[N + n] + dgp[c][i] : dgp[c][i];
                        }
                }
            }
            __syncthreads();
        }
        for (int n = threadIdx.x; n < W; n += 256) prow[n] = sh[n];
    }
}

// (lanes per row, workgroups) of a shape: what the launch and the workspace size both follow
void norm_bwd_layout(long long rows, int N, int* G, int* nblocks) {
    const int nvec = N >> 3;
    *G = (nvec % 32 == 0 && nvec <= 128) ? 32 : nvec <= 256 ? 64 : 256;
    const int groups = 256 / *G, cap = *G == 256 ? kBwdBlocksWide : kBwdBlocks;
    const long long need = (rows + groups - 1) / groups;
    *nblocks = (int)(need < cap ? (need < 1 ? 1 : need) : cap);
}

struct norm_bwd_args_t {
    const void *x, *z, *gpre, *gout, *dy, *dz_in;
    void *dz, *dx;
    float *partial, *dgpre, *dgout;
    long long rows;
    int N;
    float woff, eps_pre, eps_out;
};

template <typename T, typename GT, bool PRE>
int launch_norm_bwd(const norm_bwd_args_t& a, hipStream_t stream) {
    int G, nb;
    norm_bwd_layout(a.rows, a.N, &G, &nb);
    const int nvec = a.N >> 3, W = PRE ? 2 * a.N : a.N;
    const dim3 grid((unsigned)nb), block(256);
    const size_t lds = G == 256 ? 0 : (size_t)W * sizeof(float);
#define BF_NANB_LAUNCH(G_, V_)                                                                                               \
    hipLaunchKernelGGL((norm_add_rmsnorm_bwd_kernel<T, GT, G_, V_, PRE>), grid, block, lds, stream, (const T*)a.x,            \
                       (const T*)a.z, (const GT*)a.gpre, (const GT*)a.gout, (const T*)a.dy, (const T*)a.dz_in, (T*)a.dz,      \
                       (T*)a.dx, a.partial, a.rows, a.N, a.woff, a.eps_pre, a.eps_out)
    if (G == 32) {
        switch (nvec / 32) {
            case 1: BF_NANB_LAUNCH(32, 1); break;
            case 2: BF_NANB_LAUNCH(32, 2); break;
            case 3: BF_NANB_LAUNCH(32, 3); break;
            default: BF_NANB_LAUNCH(32, 4); break;
        }
    } else if (G == 64) {
        if (nvec <= 64) BF_NANB_LAUNCH(64, 1);
        else if (nvec <= 128) BF_NANB_LAUNCH(64, 2);
        else BF_NANB_LAUNCH(64, 4);
    } else {
        if (nvec <= 512) BF_NANB_LAUNCH(256, 2);
        else BF_NANB_LAUNCH(256, 4);
    }
#undef BF_NANB_LAUNCH
    BF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dgamma_rows_kernel, dim3((W + 15) / 16), dim3(1024), 0, stream, a.partial, nb, W, a.N, a.dgout, a.dgpre);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int launch_norm_bwd_gt(const norm_bwd_args_t& a, int param_dtype, hipStream_t stream) {
    if (param_dtype == BF_DT_F32)
        return a.gpre ? launch_norm_bwd<T, float, true>(a, stream) : launch_norm_bwd<T, float, false>(a, stream);
    return a.gpre ? launch_norm_bwd<T, T, true>(a, stream) : launch_norm_bwd<T, T, false>(a, stream);
}

// ---- the rotary embedding's transpose, then the per-head RMSNorm's backward ------------------------------------------------------
// qknorm_rope_kernel's work split and loop.  A lane loads its 8 + 8 elements of the incoming gradient and rotates them back,
//     dn1 = do1 c1 + do2 s2,   dn2 = do2 c2 - do1 s1
// (the transpose for tables whose halves differ as well).  NORM, for a tensor that has a gamma: with x the forward's input,
// r = rsqrt(mean_D(x^2) + eps) recomputed across the head's D / 16 lanes (the sum of squares in fp64) and b = (woff + g) o dn,
//     dx = r b - x r^3 mean_D(x o b),   dgamma = sum_{b, t, heads} dn o x r.
// A lane's columns are the same in every round of the loop (the stride is a multiple of 256), so it keeps the fp32 dgamma
// partials of its 16 columns in registers, one set for q and one for k, each term formed in fp64.  The workgroup combines
// them through LDS in a fixed order into one [2, D] row, which dgamma_rows_kernel sums.  The outputs are laid out
// [B, T, heads, D], and so is x.  Algorithmic bytes per element: 1 read + 1 write (+ 1 read with a gamma) * sizeof(T), and the
// tables once per token.
struct qkrope_bwd_args_t {
    int T, H, Hkv, cos_batch;
    unsigned total;
    float woff, eps;
    long long q[3], k[3];  // strides of the incoming gradients
};

template <typename T, typename CT, typename GT, int D, bool NORM>
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(const T* dqo, const T* dko, const T* xq, const T* xk,
                                                              const CT* __restrict__ cosp, const CT* __restrict__ sinp,
                                                              const GT* __restrict__ gamma_q, const GT* __restrict__ gamma_k,
                                                              T* dq, T* dk, float* __restrict__ partial,
                                                              const qkrope_bwd_args_t a) {
    constexpr int kVec = D / 16;  // lanes per head
    constexpr int kPad = 33;      // floats a lane owns in LDS: 2 x 16 partials and one of padding
    __shared__ float sh[NORM ? 256 * kPad : 1];
    const unsigned per_row = (unsigned)(a.H + a.Hkv) * kVec;
    float dg[NORM ? 2 : 1][16];
    if constexpr (NORM) {
#pragma unroll
        for (int i = 0; i < 16; ++i) dg[0][i] = dg[1][i] = 0.f;
    }
    // (as in the forward: `idx < total` holds or fails for all lanes of a head at once)
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < a.total; idx += gridDim.x * 256u) {
        const unsigned r = idx / per_row, l = idx - r * per_row;
        const unsigned b = r / (unsigned)a.T, t = r - b * (unsigned)a.T;
        const int hh = (int)(l / kVec), j = (int)(l % kVec);
        const bool is_q = hh < a.H;
        const int h = is_q ? hh : hh - a.H;
        const int heads = is_q ? a.H : a.Hkv;
        const long long* si = is_q ? a.q : a.k;
        const T* src = (is_q ? dqo : dko) + b * si[0] + h * si[1] + t * si[2] + j * 8;
        const long long off = (((long long)b * a.T + t) * heads + h) * D + j * 8;  // [B, T, heads, D]
        T* dst = (is_q ? dq : dk) + off;
        const long long cs = ((long long)(a.cos_batch > 1 ? b : 0) * a.T + t) * D + j * 8;
        float d1[8], d2[8], c1[8], c2[8], s1[8], s2[8], n1[8], n2[8];
        load8(src, d1);
        load8(src + D / 2, d2);
        load8(cosp + cs, c1);
        load8(cosp + cs + D / 2, c2);
        load8(sinp + cs, s1);
        load8(sinp + cs + D / 2, s2);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            n1[i] = fmaf(d1[i], c1[i], d2[i] * s2[i]);
            n2[i] = fmaf(d2[i], c2[i], -(d1[i] * s1[i]));
        }
        if constexpr (NORM) {
            const GT* gm = is_q ? gamma_q : gamma_k;  // (the same for the whole head)
            float x1[8], x2[8], g1[8], g2[8];
            double sq = 0.0;
            float sx = 0.f;
            if (gm) {
                const T* xs = (is_q ? xq : xk) + off;
                load8(xs, x1);
                load8(xs + D / 2, x2);
                load8(gm + j * 8, g1);
                load8(gm + j * 8 + D / 2, g2);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    sq = fma((double)x1[i], (double)x1[i], sq);
                    sq = fma((double)x2[i], (double)x2[i], sq);
                    sx = fmaf(n1[i] * (a.woff + g1[i]), x1[i], sx);
                    sx = fmaf(n2[i] * (a.woff + g2[i]), x2[i], sx);
                }
            }
#pragma unroll
            for (int m = kVec / 2; m; m >>= 1) {  // every lane of the head ends with the same sums
                sq += __shfl_xor(sq, m);
                sx += __shfl_xor(sx, m);
            }
            if (gm) {
                const double rd = 1.0 / sqrt(sq / (double)D + (double)a.eps);
                const float rr = (float)rd;
                const float kk = rr * rr * rr * (sx * (1.0f / (float)D));
                float* acc = dg[is_q ? 0 : 1];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    acc[i] = (float)fma((double)n1[i] * (double)x1[i], rd, (double)acc[i]);
                    acc[8 + i] = (float)fma((double)n2[i] * (double)x2[i], rd, (double)acc[8 + i]);
                    n1[i] = fmaf(-x1[i], kk, rr * (n1[i] * (a.woff + g1[i])));
                    n2[i] = fmaf(-x2[i], kk, rr * (n2[i] * (a.woff + g2[i])));
                }
            }
        }
        store8(dst, n1);
        store8(dst + D / 2, n2);
    }
    if constexpr (NORM) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sh[threadIdx.x * kPad + i] = dg[0][i];
            sh[threadIdx.x * kPad + 16 + i] = dg[1][i];
        }
        __syncthreads();
        // column c of the [2, D] row: tensor c / D, half (c % D) / (D / 2), vector j and element i within the half; the
        // lanes j, j + kVec, ... of the workgroup own it, added in that order
        for (int c = threadIdx.x; c < 2 * D; c += 256) {
            const int which = c / D, col = c % D, half = col / (D / 2), w = col % (D / 2);
            const int j = w >> 3, reg = which * 16 + half * 8 + (w & 7);
            float t = 0.f;
            for (int ln = j; ln < 256; ln += kVec) t += sh[ln * kPad + reg];
            partial[(long long)blockIdx.x * 2 * D + c] = t;
        }
    }
}

unsigned qkrope_bwd_blocks(long long total) {
    const long long blocks = (total + 255) / 256;
    return (unsigned)(blocks < kBwdBlocks ? blocks : kBwdBlocks);
}

struct qkrope_bwd_ptrs_t {
    const void *dqo, *dko, *xq, *xk, *c, *s, *gq, *gk;
    void *dq, *dk;
    float *partial, *dgq, *dgk;
};

template <typename T, typename CT, typename GT, bool NORM>
int launch_qkrope_bwd(const qkrope_bwd_ptrs_t& p, int D, const qkrope_bwd_args_t& a, hipStream_t stream) {
    const unsigned nb = qkrope_bwd_blocks(a.total);
    const dim3 grid(nb), block(256);
#define BF_QKRB_LAUNCH(D_)                                                                                                   \
    hipLaunchKernelGGL((qknorm_rope_bwd_kernel<T, CT, GT, D_, NORM>), grid, block, 0, stream, (const T*)p.dqo, (const T*)p.dko, \
                       (const T*)p.xq, (const T*)p.xk, (const CT*)p.c, (const CT*)p.s, (const GT*)p.gq, (const GT*)p.gk,        \
                       (T*)p.dq, (T*)p.dk, p.partial, a)
    if (D == 64) BF_QKRB_LAUNCH(64);
    else if (D == 128) BF_QKRB_LAUNCH(128);
    else BF_QKRB_LAUNCH(256);
#undef BF_QKRB_LAUNCH
    BF_HIP_CHECK(hipGetLastError());
    if constexpr (NORM) {
        hipLaunchKernelGGL(dgamma_rows_kernel, dim3((2 * D + 15) / 16), dim3(1024), 0, stream, p.partial, (int)nb, 2 * D, D,
                           p.dgq, p.dgk);
        BF_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

template <typename T, typename CT>
int launch_qkrope_bwd_gt(const qkrope_bwd_ptrs_t& p, int param_dtype, int D, const qkrope_bwd_args_t& a, hipStream_t stream) {
    if (!p.gq && !p.gk) return launch_qkrope_bwd<T, CT, float, false>(p, D, a, stream);
    if (param_dtype == BF_DT_F32) return launch_qkrope_bwd<T, CT, float, true>(p, D, a, stream);
    return launch_qkrope_bwd<T, CT, T, true>(p, D, a, stream);
}

template <typename T>
int launch_qkrope_bwd_ct(const qkrope_bwd_ptrs_t& p, int cs_dtype, int param_dtype, int D, const qkrope_bwd_args_t& a,
                         hipStream_t stream) {
    if (cs_dtype == BF_DT_F32) return launch_qkrope_bwd_gt<T, float>(p, param_dtype, D, a, stream);
    return launch_qkrope_bwd_gt<T, T>(p, param_dtype, D, a, stream);
}

// ---- gelu_tanh(gate) * up ---------------------------------------------------------------------------------------------------
// y = g s u with s = sigmoid(2k), 2k = g p, p = 2c + 2c 0.044715 g^2, and d(2k)/dg = q = 2c + 3 * 2c 0.044715 g^2:
//     dup = dy g s,      dgate = dy u s (1 + g q (1 - s)).
// s and 1 - s are both taken from e = exp(-|2k|) as swiglu_bwd_kernel takes them (2k formed as the forward forms it), so
// 1 - s keeps its relative precision where s rounds to 1.  g q is formed in fp64: g^3 leaves fp32's range at |g| = 7e12,
// where 1 - s (or s) has long been 0, and the fp64 product is finite up to the largest gate of any dtype (1e116), so no
// inf * 0 appears.  The bracket s (1 + g q (1 - s)) is bounded by 1.13; it is rounded to fp32 once and dy comes last.  The
// limits come out by themselves: g -> +inf gives s = 1, 1 - s = 0 and (dy u, dy g), g -> -inf gives s = 0 and (0, 0).
// The forward's grid.  Algorithmic bytes per element: (3 reads + 2 writes) * sizeof(T).
template <typename T>
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const T* gate, long long gate_stride, const T* up, long long up_stride,
                                                        const T* dy, long long dy_stride, T* dgate, long long dgate_stride,
                                                        T* dup, long long dup_stride, long long rows, int nvec) {
    constexpr double k2c = 1.5957691216057308;  // 2 sqrt(2 / pi)
    constexpr double k2ca = k2c * 0.044715;
    const int vi = blockIdx.x * 256 + threadIdx.x;
    if (vi >= nvec) return;
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        float g[8], u[8], d[8], og[8], ou[8];
        load8(gate + row * gate_stride + vi * 8, g);
        load8(up + row * up_stride + vi * 8, u);
        load8(dy + row * dy_stride + vi * 8, d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double gd = (double)g[i], g2 = gd * gd;
            const float arg = (float)(gd * fma(g2, k2ca, k2c));  // 2k; +-inf beyond fp32's range
            const float e = expf(-fabsf(arg));
            const float big = 1.0f / (1.0f + e), small = e * big;
            const float s = arg >= 0.f ? big : small, ms = arg >= 0.f ? small : big;
            const float f = (float)((double)s * fma(gd * fma(g2, 3.0 * k2ca, k2c), (double)ms, 1.0));
            og[i] = d[i] * (u[i] * f);
            ou[i] = d[i] * (g[i] * s);
        }
        store8(dgate + row * dgate_stride + vi * 8, og);
        store8(dup + row * dup_stride + vi * 8, ou);
    }
}

template <typename T>
int launch_geglu_bwd(const void* gate, long long gs, const void* up, long long us, const void* dy, long long ds, void* dgate,
                     long long dgs, void* dup, long long dus, long long rows, int N, hipStream_t stream) {
    const int nvec = N >> 3;
    const unsigned gx = (unsigned)((nvec + 255) / 256);
    const long long want = 8192 / gx > 0 ? 8192 / gx : 1;
    const unsigned gy = (unsigned)(rows < want ? rows : want);
    hipLaunchKernelGGL((geglu_bwd_kernel<T>), dim3(gx, gy), dim3(256), 0, stream, (const T*)gate, gs, (const T*)up, us,
                       (const T*)dy, ds, (T*)dgate, dgs, (T*)dup, dus, rows, nvec);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

size_t bf_norm_add_rmsnorm_bwd_workspace_bytes(int64_t rows, int N, int has_gamma_pre) {
    if (rows < 1 || N < 1) return 0;
    int G, nb;
    norm_bwd_layout(rows, N, &G, &nb);
    return (size_t)nb * N * (has_gamma_pre ? 2 : 1) * sizeof(float);
}

int bf_norm_add_rmsnorm_bwd(const void* d_x, const void* d_z, const void* d_gamma_pre, const void* d_gamma_out, int param_dtype,
                            int weight_offset, const void* d_dy, const void* d_dz_in, void* d_dz, void* d_dx,
                            float* d_dgamma_pre, float* d_dgamma_out, void* d_workspace, size_t workspace_bytes, int dtype,
                            int64_t rows, int N, float eps_pre, float eps_out, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("bf_norm_add_rmsnorm_bwd: bad shape rows=%lld N=%d", (long long)rows, N);
    if (N % 8 || N > 8192) BF_FAIL("bf_norm_add_rmsnorm_bwd: N=%d must be a multiple of 8 and at most 8192", N);
    if (!d_dgamma_out || (d_gamma_pre && !d_dgamma_pre)) BF_FAIL("bf_norm_add_rmsnorm_bwd: null parameter gradient");
    if (weight_offset != 0 && weight_offset != 1)
        BF_FAIL("bf_norm_add_rmsnorm_bwd: weight_offset=%d must be 0 or 1", weight_offset);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_norm_add_rmsnorm_bwd: unknown dtype %d", dtype);
    if (param_dtype != BF_DT_F32 && param_dtype != dtype)
        BF_FAIL("bf_norm_add_rmsnorm_bwd: the gammas must be fp32 or have the activation dtype");
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        BF_HIP_CHECK(hipMemsetAsync(d_dgamma_out, 0, (size_t)N * sizeof(float), st));
        if (d_gamma_pre) BF_HIP_CHECK(hipMemsetAsync(d_dgamma_pre, 0, (size_t)N * sizeof(float), st));
        return 0;
    }
    if (!d_z || !d_gamma_out || (!d_dy && !d_dz_in)) BF_FAIL("bf_norm_add_rmsnorm_bwd: null pointer");
    if (d_gamma_pre ? (!d_x || !d_dx) : !d_dz)
        BF_FAIL("bf_norm_add_rmsnorm_bwd: with gamma_pre x and dx are needed, without it dz");
    const uintptr_t al = (uintptr_t)d_x | (uintptr_t)d_z | (uintptr_t)d_gamma_pre | (uintptr_t)d_gamma_out | (uintptr_t)d_dy |
                         (uintptr_t)d_dz_in | (uintptr_t)d_dz | (uintptr_t)d_dx | (uintptr_t)d_dgamma_pre |
                         (uintptr_t)d_dgamma_out | (uintptr_t)d_workspace;
    if (al & 15) BF_FAIL("bf_norm_add_rmsnorm_bwd: pointers must be 16-byte aligned");
    const size_t need = bf_norm_add_rmsnorm_bwd_workspace_bytes(rows, N, d_gamma_pre != nullptr);
    if (!d_workspace || workspace_bytes < need)
        BF_FAIL("bf_norm_add_rmsnorm_bwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    norm_bwd_args_t a;
    a.x = d_x, a.z = d_z, a.gpre = d_gamma_pre, a.gout = d_gamma_out, a.dy = d_dy, a.dz_in = d_dz_in, a.dz = d_dz;
    a.dx = d_gamma_pre ? d_dx : nullptr, a.partial = reinterpret_cast<float*>(d_workspace);
    a.dgpre = d_gamma_pre ? d_dgamma_pre : nullptr, a.dgout = d_dgamma_out;
    a.rows = rows, a.N = N, a.woff = (float)weight_offset, a.eps_pre = eps_pre, a.eps_out = eps_out;
    switch (dtype) {
        case BF_DT_BF16: return launch_norm_bwd_gt<__bf16>(a, param_dtype, st);
        case BF_DT_F16: return launch_norm_bwd_gt<_Float16>(a, param_dtype, st);
        default: return launch_norm_bwd_gt<float>(a, param_dtype, st);
    }
}

size_t bf_qknorm_rope_bwd_workspace_bytes(const bf_rope_t* shape, int has_gamma) {
    if (!shape || !has_gamma) return 0;
    const long long total = (long long)shape->B * shape->T * (shape->H + shape->Hkv) * (shape->head_dim / 16);
    if (total < 1) return 0;
    return (size_t)qkrope_bwd_blocks(total) * 2 * shape->head_dim * sizeof(float);
}

int bf_qknorm_rope_bwd(const void* d_dq_out, const void* d_dk_out, const void* d_q, const void* d_k, const void* d_cos,
                       const void* d_sin, int cs_dtype, const void* d_gamma_q, const void* d_gamma_k, int param_dtype,
                       int weight_offset, float eps, void* d_dq, void* d_dk, float* d_dgamma_q, float* d_dgamma_k,
                       void* d_workspace, size_t workspace_bytes, int dtype, const bf_rope_t* shape, void* stream) {
    if (!shape) BF_FAIL("bf_qknorm_rope_bwd: shape is NULL");
    const bf_rope_t& s = *shape;
    if (s.head_dim != 64 && s.head_dim != 128 && s.head_dim != 256)
        BF_FAIL("bf_qknorm_rope_bwd: head_dim=%d must be 64, 128 or 256", s.head_dim);
    if (s.B < 0 || s.T < 1 || s.H < 1 || s.Hkv < 1)
        BF_FAIL("bf_qknorm_rope_bwd: bad shape B=%d T=%d H=%d Hkv=%d", s.B, s.T, s.H, s.Hkv);
    if (s.cos_batch != 1 && s.cos_batch != s.B) BF_FAIL("bf_qknorm_rope_bwd: cos_batch=%d must be 1 or B=%d", s.cos_batch, s.B);
    if (!d_dq_out || !d_dk_out || !d_cos || !d_sin || !d_dq || !d_dk) BF_FAIL("bf_qknorm_rope_bwd: null pointer");
    if ((d_gamma_q && (!d_q || !d_dgamma_q)) || (d_gamma_k && (!d_k || !d_dgamma_k)))
        BF_FAIL("bf_qknorm_rope_bwd: a gamma needs the forward's input and a parameter gradient");
    const uintptr_t al = (uintptr_t)d_dq_out | (uintptr_t)d_dk_out | (uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_cos |
                         (uintptr_t)d_sin | (uintptr_t)d_gamma_q | (uintptr_t)d_gamma_k | (uintptr_t)d_dq | (uintptr_t)d_dk |
                         (uintptr_t)d_dgamma_q | (uintptr_t)d_dgamma_k | (uintptr_t)d_workspace;
    if (al & 15) BF_FAIL("bf_qknorm_rope_bwd: pointers must be 16-byte aligned");
    if (!strides_ok(s.q_stride) || !strides_ok(s.k_stride))
        BF_FAIL("bf_qknorm_rope_bwd: strides must be non-negative multiples of 8 elements");
    if (weight_offset != 0 && weight_offset != 1) BF_FAIL("bf_qknorm_rope_bwd: weight_offset=%d must be 0 or 1", weight_offset);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_qknorm_rope_bwd: unknown dtype %d", dtype);
    if (cs_dtype != BF_DT_F32 && cs_dtype != dtype)
        BF_FAIL("bf_qknorm_rope_bwd: cos / sin must be fp32 or have the activation dtype");
    const bool norm = d_gamma_q || d_gamma_k;
    if (norm && param_dtype != BF_DT_F32 && param_dtype != dtype)
        BF_FAIL("bf_qknorm_rope_bwd: the gammas must be fp32 or have the activation dtype");
    const long long total = (long long)s.B * s.T * (s.H + s.Hkv) * (s.head_dim / 16);
    if (total > 0x7fffffffLL) BF_FAIL("bf_qknorm_rope_bwd: B * T * (H + Hkv) * head_dim / 16 = %lld exceeds 2^31 - 1", total);
    hipStream_t st = (hipStream_t)stream;
    if (total == 0) {
        if (d_gamma_q) BF_HIP_CHECK(hipMemsetAsync(d_dgamma_q, 0, (size_t)s.head_dim * sizeof(float), st));
        if (d_gamma_k) BF_HIP_CHECK(hipMemsetAsync(d_dgamma_k, 0, (size_t)s.head_dim * sizeof(float), st));
        return 0;
    }
    const size_t need = bf_qknorm_rope_bwd_workspace_bytes(shape, norm);
    if (norm && (!d_workspace || workspace_bytes < need))
        BF_FAIL("bf_qknorm_rope_bwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    qkrope_bwd_args_t a;
    a.T = s.T, a.H = s.H, a.Hkv = s.Hkv, a.cos_batch = s.cos_batch, a.total = (unsigned)total;
    a.woff = (float)weight_offset, a.eps = eps;
    for (int i = 0; i < 3; ++i) a.q[i] = s.q_stride[i], a.k[i] = s.k_stride[i];
    qkrope_bwd_ptrs_t p;
    p.dqo = d_dq_out, p.dko = d_dk_out, p.xq = d_q, p.xk = d_k, p.c = d_cos, p.s = d_sin, p.gq = d_gamma_q, p.gk = d_gamma_k;
    p.dq = d_dq, p.dk = d_dk, p.partial = reinterpret_cast<float*>(d_workspace);
    p.dgq = d_gamma_q ? d_dgamma_q : nullptr, p.dgk = d_gamma_k ? d_dgamma_k : nullptr;
    switch (dtype) {
        case BF_DT_BF16: return launch_qkrope_bwd_ct<__bf16>(p, cs_dtype, param_dtype, s.head_dim, a, st);
        case BF_DT_F16: return launch_qkrope_bwd_ct<_Float16>(p, cs_dtype, param_dtype, s.head_dim, a, st);
        default: return launch_qkrope_bwd_ct<float>(p, cs_dtype, param_dtype, s.head_dim, a, st);
    }
}

int bf_geglu_bwd(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, const void* d_dy,
                 int64_t dy_row_stride, void* d_dgate, int64_t dgate_row_stride, void* d_dup, int64_t dup_row_stride, int dtype,
                 int64_t rows, int N, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("bf_geglu_bwd: bad shape rows=%lld N=%d", (long long)rows, N);
    if (N % 8) BF_FAIL("bf_geglu_bwd: N=%d must be a multiple of 8", N);
    if (!d_gate || !d_up || !d_dy || !d_dgate || !d_dup) BF_FAIL("bf_geglu_bwd: null pointer");
    if (((uintptr_t)d_gate | (uintptr_t)d_up | (uintptr_t)d_dy | (uintptr_t)d_dgate | (uintptr_t)d_dup) & 15)
        BF_FAIL("bf_geglu_bwd: pointers must be 16-byte aligned");
    const int64_t strides[5] = {gate_row_stride, up_row_stride, dy_row_stride, dgate_row_stride, dup_row_stride};
    for (int i = 0; i < 5; ++i)
        if (strides[i] < N || (strides[i] & 7))
            BF_FAIL("bf_geglu_bwd: row strides (%lld, %lld, %lld, %lld, %lld) must be multiples of 8 and at least N=%d",
                    (long long)strides[0], (long long)strides[1], (long long)strides[2], (long long)strides[3],
                    (long long)strides[4], N);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_geglu_bwd: unknown dtype %d", dtype);
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define BF_GGB_ARGS d_gate, gate_row_stride, d_up, up_row_stride, d_dy, dy_row_stride, d_dgate, dgate_row_stride, d_dup, dup_row_stride, rows, N, st
    switch (dtype) {
        case BF_DT_BF16: return launch_geglu_bwd<__bf16>(BF_GGB_ARGS);
        case BF_DT_F16: return launch_geglu_bwd<_Float16>(BF_GGB_ARGS);
        default: return launch_geglu_bwd<float>(BF_GGB_ARGS);
    }
#undef BF_GGB_ARGS
}
