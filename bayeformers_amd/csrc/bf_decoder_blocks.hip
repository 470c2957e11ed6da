// bf_decoder_blocks.hip — the three memory-bound ops of a Llama-family decoder layer that sit between the Bayesian linear
// layers and the attention kernels: residual add + RMSNorm, rotary position embedding of q and k, SiLU(gate) * up.  Not
// reference functions: they are the wrapped model's own ops around /root/reference/bayeformers/nn/layers/linear.py:83-104's
// forward (HF LlamaRMSNorm.forward, apply_rotary_pos_emb, LlamaMLP's act_fn(gate) * up), each of which the framework runs
// as a chain of elementwise kernels with a full pass over the activations per link.
//
// HBM-bound streaming kernels in the manner of bf_norm.hip: 16-byte loads and stores, fp32 arithmetic in registers, one
// rounding into the output dtype.  No allocation, no host synchronisation (capturable), no trigonometry: cos and sin are
// the tables the model's rotary module returns.
#include "bf_common.h"
#include "bf_device.h"
#include "bf_vec8.h"

namespace {

constexpr int kRowsPerBlock = 4;  // one wave per row

// 8 floats rounded once to T (what the output tensor holds) and read back: the values the next op of the unfused model sees
template <typename T>
__device__ __forceinline__ void round8(float (&v)[8]) {
    if constexpr (!__is_same(T, float)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)(T)v[i];
    }
}

// z = x + residual (rounded to T once: bitwise torch's `residual + x`), y = z * rsqrt(mean(z^2) + eps) * gamma with the
// statistics taken from the rounded z.  One wave per row, the row lives in registers between the load and the stores.
// VPL = 8-element vectors per lane: a row has N/8 <= 64*VPL of them.  Algorithmic bytes per row: N * (2 reads + 2 writes)
// * sizeof(T) with a residual and a sum output.
template <typename T, typename GT, int VPL>
__global__ __launch_bounds__(64 * kRowsPerBlock) void add_rmsnorm_kernel(const T* x, const T* res, const GT* __restrict__ gamma,
                                                                         T* sum_out, T* out, long long rows, int N, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nvec = N >> 3;
    const T* xr = x + row * N;
    const T* rr = res ? res + row * N : nullptr;
    float v[VPL][8];
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < VPL; ++c) {
        const int vi = lane + 64 * c;
        if (vi < nvec) {
            load8(xr + vi * 8, v[c]);
            if (rr) {
                float r[8];
                load8(rr + vi * 8, r);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[c][i] += r[i];
                round8<T>(v[c]);
            }
            if (sum_out) store8(sum_out + row * N + vi * 8, v[c]);
#pragma unroll
            for (int i = 0; i < 8; ++i) sq = fmaf(v[c][i], v[c][i], sq);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) * (1.0f / (float)N) + eps);
    T* orow = out + row * N;
#pragma unroll
    for (int c = 0; c < VPL; ++c) {
        const int vi = lane + 64 * c;
        if (vi < nvec) {
            float g[8], o[8];
            load8(gamma + vi * 8, g);
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = (v[c][i] * rstd) * g[i];
            store8(orow + vi * 8, o);
        }
    }
}

// Rows of 32 V vectors (N = 256 V: 256 .. 1024): half a wave per row, two rows per wave, every lane busy
// (add_layernorm_half_kernel's layout).
template <typename T, typename GT, int V>
__global__ __launch_bounds__(64 * kRowsPerBlock) void add_rmsnorm_half_kernel(const T* x, const T* res, const GT* __restrict__ gamma,
                                                                              T* sum_out, T* out, long long rows, int N, float eps) {
    const int lane = threadIdx.x & 63, hl = lane & 31;
    const long long row_raw = ((long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6)) * 2 + (lane >> 5);
    if (row_raw - (lane >> 5) >= rows) return;           // the whole wave is past the end
    const bool live = row_raw < rows;
    const long long row = live ? row_raw : rows - 1;      // the idle half of the last wave reads a valid row, writes nothing
    const T* xr = x + row * N;
    const T* rr = res ? res + row * N : nullptr;
    float v[V][8];
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const int vi = hl + 32 * c;
        load8(xr + vi * 8, v[c]);
        if (rr) {
            float r[8];
            load8(rr + vi * 8, r);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[c][i] += r[i];
            round8<T>(v[c]);
        }
        if (sum_out && live) store8(sum_out + row * N + vi * 8, v[c]);
#pragma unroll
        for (int i = 0; i < 8; ++i) sq = fmaf(v[c][i], v[c][i], sq);
    }
    const float rstd = 1.0f / sqrtf(half_sum(sq, lane) * (1.0f / (float)N) + eps);
    if (!live) return;
    T* orow = out + row * N;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const int vi = hl + 32 * c;
        float g[8], o[8];
        load8(gamma + vi * 8, g);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (v[c][i] * rstd) * g[i];
        store8(orow + vi * 8, o);
    }
}

template <typename T, typename GT>
int launch_rmsnorm(const void* x, const void* res, const void* gamma, void* sum_out, void* out, long long rows, int N, float eps,
                   hipStream_t stream) {
    const int nvec = N >> 3;
    const dim3 block(64 * kRowsPerBlock);
#define BF_RMS_ARGS (const T*)x, (const T*)res, (const GT*)gamma, (T*)sum_out, (T*)out, rows, N, eps
    if (nvec % 32 == 0 && nvec <= 128) {
        const dim3 grid((unsigned)((rows + 2 * kRowsPerBlock - 1) / (2 * kRowsPerBlock)));
        switch (nvec / 32) {
            case 1: hipLaunchKernelGGL((add_rmsnorm_half_kernel<T, GT, 1>), grid, block, 0, stream, BF_RMS_ARGS); break;
            case 2: hipLaunchKernelGGL((add_rmsnorm_half_kernel<T, GT, 2>), grid, block, 0, stream, BF_RMS_ARGS); break;
            case 3: hipLaunchKernelGGL((add_rmsnorm_half_kernel<T, GT, 3>), grid, block, 0, stream, BF_RMS_ARGS); break;
            default: hipLaunchKernelGGL((add_rmsnorm_half_kernel<T, GT, 4>), grid, block, 0, stream, BF_RMS_ARGS); break;
        }
    } else {
        const dim3 grid((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock));
        if (nvec <= 64) hipLaunchKernelGGL((add_rmsnorm_kernel<T, GT, 1>), grid, block, 0, stream, BF_RMS_ARGS);
        else if (nvec <= 128) hipLaunchKernelGGL((add_rmsnorm_kernel<T, GT, 2>), grid, block, 0, stream, BF_RMS_ARGS);
        else if (nvec <= 256) hipLaunchKernelGGL((add_rmsnorm_kernel<T, GT, 4>), grid, block, 0, stream, BF_RMS_ARGS);
        else if (nvec <= 512) hipLaunchKernelGGL((add_rmsnorm_kernel<T, GT, 8>), grid, block, 0, stream, BF_RMS_ARGS);
        else hipLaunchKernelGGL((add_rmsnorm_kernel<T, GT, 16>), grid, block, 0, stream, BF_RMS_ARGS);
    }
#undef BF_RMS_ARGS
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int launch_rmsnorm_gt(const void* x, const void* res, const void* gamma, int param_dtype, int dtype, void* sum_out, void* out,
                      long long rows, int N, float eps, hipStream_t stream) {
    if (param_dtype == BF_DT_F32) return launch_rmsnorm<T, float>(x, res, gamma, sum_out, out, rows, N, eps, stream);
    if (param_dtype == dtype) return launch_rmsnorm<T, T>(x, res, gamma, sum_out, out, rows, N, eps, stream);
    BF_FAIL("bf_add_rmsnorm: gamma must be fp32 or have the activation dtype");
}

// ---- rotary position embedding of q and k --------------------------------------------------------------------------------
// out = x * cos + rotate_half(x) * sin with rotate_half(x) = [-x2, x1] over the two halves of a head (HF's convention).
// One lane owns 8 elements of the first half and their 8 partners of the second: it loads both, then stores both, which
// is what makes the in-place form safe.  Lanes run over (token row, head of q then of k, vector) with the heads fastest,
// so the projections' [B, T, H*D] layout is read in address order.
struct rope_args_t {
    int T, H, Hkv, cos_batch;
    unsigned total;  // lanes of work: B * T * (H + Hkv) * D / 16
    long long q[3], k[3], qo[3], ko[3];
};

// BWD: the transpose, dx1 = dy1 c1 + dy2 s2, dx2 = dy2 c2 - dy1 s1 (x is then the gradient of the rotated tensor): the
// adjoint for tables whose two halves differ as well, which "the forward with sin negated" is not.
template <typename T, typename CT, int D, bool BWD>
__global__ __launch_bounds__(256) void rope_qk_kernel(const T* q, const T* k, const CT* __restrict__ cosp,
                                                      const CT* __restrict__ sinp, T* q_out, T* k_out, const rope_args_t a) {
    constexpr int kVec = D / 16;  // lanes per head
    const unsigned per_row = (unsigned)(a.H + a.Hkv) * kVec;
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
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (BWD) {
                o1[i] = fmaf(x1[i], c1[i], x2[i] * s2[i]);
                o2[i] = fmaf(x2[i], c2[i], -(x1[i] * s1[i]));
            } else {
                o1[i] = fmaf(x1[i], c1[i], -(x2[i] * s1[i]));
                o2[i] = fmaf(x2[i], c2[i], x1[i] * s2[i]);
            }
        }
        store8(dst, o1);
        store8(dst + D / 2, o2);
    }
}

template <typename T, typename CT, bool BWD>
int launch_rope(const void* q, const void* k, const void* c, const void* s, void* qo, void* ko, int D, const rope_args_t& a,
                hipStream_t stream) {
    const unsigned blocks = (a.total + 255u) / 256u;
    const dim3 grid(blocks < 4096u ? blocks : 4096u), block(256);
    if (D == 64)
        hipLaunchKernelGGL((rope_qk_kernel<T, CT, 64, BWD>), grid, block, 0, stream, (const T*)q, (const T*)k, (const CT*)c,
                           (const CT*)s, (T*)qo, (T*)ko, a);
    else
        hipLaunchKernelGGL((rope_qk_kernel<T, CT, 128, BWD>), grid, block, 0, stream, (const T*)q, (const T*)k, (const CT*)c,
                           (const CT*)s, (T*)qo, (T*)ko, a);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int launch_rope_ct(const void* q, const void* k, const void* c, const void* s, int cs_dtype, void* qo, void* ko, int D,
                   const rope_args_t& a, bool bwd, hipStream_t stream) {
    if (cs_dtype == BF_DT_F32)
        return bwd ? launch_rope<T, float, true>(q, k, c, s, qo, ko, D, a, stream)
                   : launch_rope<T, float, false>(q, k, c, s, qo, ko, D, a, stream);
    return bwd ? launch_rope<T, T, true>(q, k, c, s, qo, ko, D, a, stream) : launch_rope<T, T, false>(q, k, c, s, qo, ko, D, a, stream);
}

// ---- SiLU(gate) * up -------------------------------------------------------------------------------------------------------
// y = gate / (1 + exp(-gate)) * up.  exp overflows to +inf for gate < -88.7 (the quotient is then -0, the limit) and
// underflows to 0 for large gates (the quotient is gate): finite for every finite input.
// blockIdx.x: 256 vectors of a row, blockIdx.y: rows blockIdx.y, + gridDim.y, ...
template <typename T>
__global__ __launch_bounds__(256) void swiglu_kernel(const T* gate, long long gate_stride, const T* up, long long up_stride,
                                                     T* out, long long out_stride, long long rows, int nvec) {
    const int vi = blockIdx.x * 256 + threadIdx.x;
    if (vi >= nvec) return;
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        float g[8], u[8], o[8];
        load8(gate + row * gate_stride + vi * 8, g);
        load8(up + row * up_stride + vi * 8, u);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = g[i] / (1.0f + expf(-g[i])) * u[i];
        store8(out + row * out_stride + vi * 8, o);
    }
}

template <typename T>
int launch_swiglu(const void* gate, long long gs, const void* up, long long us, void* out, long long os, long long rows, int N,
                  hipStream_t stream) {
    const int nvec = N >> 3;
    const unsigned gx = (unsigned)((nvec + 255) / 256);
    const long long want = 8192 / gx > 0 ? 8192 / gx : 1;  // about 8192 workgroups at most, the rest by the row loop
    const unsigned gy = (unsigned)(rows < want ? rows : want);
    hipLaunchKernelGGL((swiglu_kernel<T>), dim3(gx, gy), dim3(256), 0, stream, (const T*)gate, gs, (const T*)up, us, (T*)out, os,
                       rows, nvec);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

bool strides_ok(const int64_t* s) { return s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && !((s[0] | s[1] | s[2]) & 7); }

}  // namespace

int bf_add_rmsnorm(const void* d_x, const void* d_residual, const void* d_gamma, int param_dtype, void* d_sum_out, void* d_out,
                   int dtype, int64_t rows, int N, float eps, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("bf_add_rmsnorm: bad shape rows=%lld N=%d", (long long)rows, N);
    if (N % 8 || N > 8192) BF_FAIL("bf_add_rmsnorm: N=%d must be a multiple of 8 and at most 8192", N);
    if (!d_x || !d_gamma || !d_out) BF_FAIL("bf_add_rmsnorm: null pointer");
    if (rows > 0x7fffffffLL * kRowsPerBlock) BF_FAIL("bf_add_rmsnorm: too many rows");
    const uintptr_t al = (uintptr_t)d_x | (uintptr_t)d_residual | (uintptr_t)d_gamma | (uintptr_t)d_sum_out | (uintptr_t)d_out;
    if (al & 15) BF_FAIL("bf_add_rmsnorm: pointers must be 16-byte aligned");
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_add_rmsnorm: unknown dtype %d", dtype);
    if (param_dtype != BF_DT_F32 && param_dtype != dtype) BF_FAIL("bf_add_rmsnorm: gamma must be fp32 or have the activation dtype");
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case BF_DT_BF16: return launch_rmsnorm_gt<__bf16>(d_x, d_residual, d_gamma, param_dtype, dtype, d_sum_out, d_out, rows, N, eps, st);
        case BF_DT_F16: return launch_rmsnorm_gt<_Float16>(d_x, d_residual, d_gamma, param_dtype, dtype, d_sum_out, d_out, rows, N, eps, st);
        default: return launch_rmsnorm_gt<float>(d_x, d_residual, d_gamma, param_dtype, dtype, d_sum_out, d_out, rows, N, eps, st);
    }
}

// bf_rope_qk and bf_rope_qk_bwd: one set of checks, `who` names the entry in the messages
static int rope_entry(const char* who, bool bwd, const void* d_q, const void* d_k, const void* d_cos, const void* d_sin,
                      int cs_dtype, void* d_q_out, void* d_k_out, int dtype, const bf_rope_t* shape, void* stream) {
    if (!shape) BF_FAIL("%s: shape is NULL", who);
    const bf_rope_t& s = *shape;
    if (s.head_dim != 64 && s.head_dim != 128) BF_FAIL("%s: head_dim=%d must be 64 or 128", who, s.head_dim);
    if (s.B < 0 || s.T < 1 || s.H < 1 || s.Hkv < 1)
        BF_FAIL("%s: bad shape B=%d T=%d H=%d Hkv=%d", who, s.B, s.T, s.H, s.Hkv);
    if (s.cos_batch != 1 && s.cos_batch != s.B) BF_FAIL("%s: cos_batch=%d must be 1 or B=%d", who, s.cos_batch, s.B);
    if (!d_q || !d_k || !d_cos || !d_sin || !d_q_out || !d_k_out) BF_FAIL("%s: null pointer", who);
    const uintptr_t al = (uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_cos | (uintptr_t)d_sin | (uintptr_t)d_q_out | (uintptr_t)d_k_out;
    if (al & 15) BF_FAIL("%s: pointers must be 16-byte aligned", who);
    if (!strides_ok(s.q_stride) || !strides_ok(s.k_stride) || !strides_ok(s.q_out_stride) || !strides_ok(s.k_out_stride))
        BF_FAIL("%s: strides must be non-negative multiples of 8 elements", who);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("%s: unknown dtype %d", who, dtype);
    if (cs_dtype != BF_DT_F32 && cs_dtype != dtype) BF_FAIL("%s: cos / sin must be fp32 or have the activation dtype", who);
    const long long total = (long long)s.B * s.T * (s.H + s.Hkv) * (s.head_dim / 16);
    if (total > 0x7fffffffLL) BF_FAIL("%s: B * T * (H + Hkv) * head_dim / 16 = %lld exceeds 2^31 - 1", who, total);
    if (total == 0) return 0;
    rope_args_t a;
    a.T = s.T, a.H = s.H, a.Hkv = s.Hkv, a.cos_batch = s.cos_batch, a.total = (unsigned)total;
    for (int i = 0; i < 3; ++i)
        a.q[i] = s.q_stride[i], a.k[i] = s.k_stride[i], a.qo[i] = s.q_out_stride[i], a.ko[i] = s.k_out_stride[i];
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case BF_DT_BF16: return launch_rope_ct<__bf16>(d_q, d_k, d_cos, d_sin, cs_dtype, d_q_out, d_k_out, s.head_dim, a, bwd, st);
        case BF_DT_F16: return launch_rope_ct<_Float16>(d_q, d_k, d_cos, d_sin, cs_dtype, d_q_out, d_k_out, s.head_dim, a, bwd, st);
        default: return launch_rope_ct<float>(d_q, d_k, d_cos, d_sin, cs_dtype, d_q_out, d_k_out, s.head_dim, a, bwd, st);
    }
}

int bf_rope_qk(const void* d_q, const void* d_k, const void* d_cos, const void* d_sin, int cs_dtype, void* d_q_out,
               void* d_k_out, int dtype, const bf_rope_t* shape, void* stream) {
    return rope_entry("bf_rope_qk", false, d_q, d_k, d_cos, d_sin, cs_dtype, d_q_out, d_k_out, dtype, shape, stream);
}

int bf_rope_qk_bwd(const void* d_dq, const void* d_dk, const void* d_cos, const void* d_sin, int cs_dtype, void* d_dq_out,
                   void* d_dk_out, int dtype, const bf_rope_t* shape, void* stream) {
    return rope_entry("bf_rope_qk_bwd", true, d_dq, d_dk, d_cos, d_sin, cs_dtype, d_dq_out, d_dk_out, dtype, shape, stream);
}

int bf_swiglu(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, void* d_out,
              int64_t out_row_stride, int dtype, int64_t rows, int N, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("bf_swiglu: bad shape rows=%lld N=%d", (long long)rows, N);
    if (N % 8) BF_FAIL("bf_swiglu: N=%d must be a multiple of 8", N);
    if (!d_gate || !d_up || !d_out) BF_FAIL("bf_swiglu: null pointer");
    if (((uintptr_t)d_gate | (uintptr_t)d_up | (uintptr_t)d_out) & 15) BF_FAIL("bf_swiglu: pointers must be 16-byte aligned");
    if (gate_row_stride < N || up_row_stride < N || out_row_stride < N || ((gate_row_stride | up_row_stride | out_row_stride) & 7))
        BF_FAIL("bf_swiglu: row strides (%lld, %lld, %lld) must be multiples of 8 and at least N=%d", (long long)gate_row_stride,
                (long long)up_row_stride, (long long)out_row_stride, N);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_swiglu: unknown dtype %d", dtype);
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case BF_DT_BF16: return launch_swiglu<__bf16>(d_gate, gate_row_stride, d_up, up_row_stride, d_out, out_row_stride, rows, N, st);
        case BF_DT_F16: return launch_swiglu<_Float16>(d_gate, gate_row_stride, d_up, up_row_stride, d_out, out_row_stride, rows, N, st);
        default: return launch_swiglu<float>(d_gate, gate_row_stride, d_up, up_row_stride, d_out, out_row_stride, rows, N, st);
    }
}

// ==== the backward of the three ops ===========================================================================================
namespace {

// ---- residual add + RMSNorm -------------------------------------------------------------------------------------------------
// With z the forward's sum output, r = rsqrt(mean(z^2) + eps) recomputed from it and a = gamma o dy:
//     dz = r a - z r^3 mean_row(z o a) + dz_in,      dgamma = sum_rows dy o z r.
// Both row sums (z^2 and z o a) come out of the one pass that loads the row, so a row costs one reduction step; the row, dy
// and gamma stay in registers.  Algorithmic bytes per row: N * (2 reads + 1 write [+ 1 read with dz_in]) * sizeof(T).
// G lanes own a row, V 8-element vectors per lane: the forward's layouts (G = 32: half a wave per row for N = 256 .. 1024,
// G = 64: a wave per row up to N = 2048) and, beyond them, the whole workgroup on one row (G = 256, N <= 8192: a wave would
// need 4 x 128 registers for z, dy, gamma and the dgamma sums of such a row).  A workgroup walks rows blockIdx, + gridDim,
// ...; every lane keeps the dgamma partial sums of its own columns in registers, the workgroup's 256 / G rows are combined
// through LDS in a fixed order and leave one [N] fp32 row per workgroup, summed by rmsnorm_dgamma_kernel: deterministic.
// The sum of squares is taken in fp64 (exact products), and so is each dgamma term dy z r before it is added to the fp32
// partial sum: a term costs one fp32 rounding, the sum's, so dgamma meets the order-independent bound rows 2^-24 sum |dy z r|
// down to a single row, where three fp32 roundings (r, z r, the product) would not.  The price is about 7 fp64-rate
// instructions per element against 6 .. 8 bytes of traffic; the achieved bytes/s are in profiles/decoder_blocks_train.md.
constexpr int kBwdBlocks = 1024;      // workgroups at most (each leaves one [N] partial row)
constexpr int kBwdBlocksWide = 512;   // ... of the one-row-per-workgroup form (N > 2048)

template <int G>
__device__ __forceinline__ double group_sum_f64(double v) {
#pragma unroll
    for (int m = (G < 64 ? G : 64) / 2; m; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <typename T, typename GT, int G, int V>
__global__ __launch_bounds__(256) void add_rmsnorm_bwd_kernel(const T* z, const GT* __restrict__ gamma, const T* dy,
                                                              const T* dz_in, T* dz, float* __restrict__ partial,
                                                              long long rows, int N, float eps) {
    constexpr int kGroups = 256 / G;  // rows in flight per workgroup
    extern __shared__ float sh[];     // [N] (kGroups > 1)
    __shared__ double red_sq[4];
    __shared__ float red_s[4];
    const int lane = threadIdx.x & 63, gl = threadIdx.x % G, sub = threadIdx.x / G;
    const int nvec = N >> 3;
    float gm[V][8], dgam[V][8];
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const int vi = gl + G * c;
#pragma unroll
        for (int i = 0; i < 8; ++i) gm[c][i] = dgam[c][i] = 0.f;
        if (vi < nvec) load8(gamma + vi * 8, gm[c]);
    }
    const float inv_n = 1.0f / (float)N;
    for (long long base = (long long)blockIdx.x * kGroups; base < rows; base += (long long)gridDim.x * kGroups) {
        const bool live = base + sub < rows;
        const long long row = live ? base + sub : rows - 1;  // an idle group of the last round reads a valid row, writes nothing
        float v[V][8], g[V][8];
        double sq = 0.0;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const int vi = gl + G * c;
            if (vi < nvec) {
                load8(z + row * N + vi * 8, v[c]);
                load8(dy + row * N + vi * 8, g[c]);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    sq = fma((double)v[c][i], (double)v[c][i], sq);
                    s = fmaf(g[c][i] * gm[c][i], v[c][i], s);
                }
            }
        }
        sq = group_sum_f64<G>(sq);
        if constexpr (G == 32) s = half_sum(s, lane);
        else s = wave_sum(s);
        if constexpr (G == 256) {
            if (lane == 0) red_sq[threadIdx.x >> 6] = sq, red_s[threadIdx.x >> 6] = s;
            __syncthreads();
            sq = ((red_sq[0] + red_sq[1]) + red_sq[2]) + red_sq[3];
            s = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
            __syncthreads();
        }
        const double rd = 1.0 / sqrt(sq / (double)N + (double)eps);
        const float r = (float)rd;
        const float k = r * r * r * (s * inv_n);
        if (live) {
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const int vi = gl + G * c;
                if (vi < nvec) {
                    float o[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        o[i] = fmaf(-v[c][i], k, r * (g[c][i] * gm[c][i]));
                        // dy z is exact in fp64, r unrounded: the one rounding of a step is the sum's, back to fp32
                        dgam[c][i] = (float)fma((double)g[c][i] * (double)v[c][i], rd, (double)dgam[c][i]);
                    }
                    if (dz_in) {  // the sum had a second consumer: its gradient is added here, in fp32, not by a pass of its own
                        float h[8];
                        load8(dz_in + row * N + vi * 8, h);
#pragma unroll
                        for (int i = 0; i < 8; ++i) o[i] += h[i];
                    }
                    store8(dz + row * N + vi * 8, o);
                }
            }
        }
    }
    float* prow = partial + (long long)blockIdx.x * N;
    if constexpr (kGroups == 1) {
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const int vi = gl + G * c;
            if (vi < nvec)
#pragma unroll
                for (int i = 0; i < 8; ++i) prow[vi * 8 + i] = dgam[c][i];
        }
    } else {
        for (int grp = 0; grp < kGroups; ++grp) {  // group 0 stores, 1 .. kGroups - 1 add in turn: one fixed order
            if (sub == grp) {
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    const int vi = gl + G * c;
                    if (vi < nvec)
#pragma unroll
                        for (int i = 0; i < 8; ++i) sh[vi * 8 + i] = grp ? sh[vi * 8 + i] + dgam[c][i] : dgam[c][i];
                }
            }
            __syncthreads();
        }
        for (int n = threadIdx.x; n < N; n += 256) prow[n] = sh[n];
    }
}

// dgamma[n] = sum over the workgroups' partial rows, 16 columns x 64 lanes over the workgroup axis per block
// (layernorm_param_grad_kernel's shape); fixed order
__global__ __launch_bounds__(1024) void rmsnorm_dgamma_kernel(const float* __restrict__ partial, int nblocks, int N,
                                                              float* __restrict__ dgamma) {
    __shared__ float sh[64][16];
    const int c = threadIdx.x & 15, n = blockIdx.x * 16 + c, cl = threadIdx.x >> 4;
    float acc = 0.f;
    if (n < N)
        for (int b = cl; b < nblocks; b += 64) acc += partial[(long long)b * N + n];
    sh[cl][c] = acc;
    __syncthreads();
    if (cl == 0 && n < N) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 64; ++i) t += sh[i][c];
        dgamma[n] = t;
    }
}

// (lanes per row, workgroups) of a shape: what the launch and the workspace size both follow
void rmsnorm_bwd_layout(long long rows, int N, int* G, int* nblocks) {
    const int nvec = N >> 3;
    *G = (nvec % 32 == 0 && nvec <= 128) ? 32 : nvec <= 256 ? 64 : 256;
    const int groups = 256 / *G, cap = *G == 256 ? kBwdBlocksWide : kBwdBlocks;
    const long long need = (rows + groups - 1) / groups;
    *nblocks = (int)(need < cap ? (need < 1 ? 1 : need) : cap);
}

template <typename T, typename GT>
int launch_rmsnorm_bwd(const void* z, const void* gamma, const void* dy, const void* dz_in, void* dz, float* partial,
                       float* dgamma, long long rows, int N, float eps, hipStream_t stream) {
    int G, nb;
    rmsnorm_bwd_layout(rows, N, &G, &nb);
    const int nvec = N >> 3;
    const dim3 grid((unsigned)nb), block(256);
    const size_t lds = G == 256 ? 0 : (size_t)N * sizeof(float);
#define BF_RMSB_LAUNCH(G_, V_)                                                                                             \
    hipLaunchKernelGGL((add_rmsnorm_bwd_kernel<T, GT, G_, V_>), grid, block, lds, stream, (const T*)z, (const GT*)gamma,   \
                       (const T*)dy, (const T*)dz_in, (T*)dz, partial, rows, N, eps)
    if (G == 32) {
        switch (nvec / 32) {
            case 1: BF_RMSB_LAUNCH(32, 1); break;
            case 2: BF_RMSB_LAUNCH(32, 2); break;
            case 3: BF_RMSB_LAUNCH(32, 3); break;
            default: BF_RMSB_LAUNCH(32, 4); break;
        }
    } else if (G == 64) {
        if (nvec <= 64) BF_RMSB_LAUNCH(64, 1);
        else if (nvec <= 128) BF_RMSB_LAUNCH(64, 2);
        else BF_RMSB_LAUNCH(64, 4);
    } else {
        if (nvec <= 512) BF_RMSB_LAUNCH(256, 2);
        else BF_RMSB_LAUNCH(256, 4);
    }
#undef BF_RMSB_LAUNCH
    BF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(rmsnorm_dgamma_kernel, dim3((N + 15) / 16), dim3(1024), 0, stream, partial, nb, N, dgamma);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int launch_rmsnorm_bwd_gt(const void* z, const void* gamma, int param_dtype, const void* dy, const void* dz_in, void* dz,
                          float* partial, float* dgamma, long long rows, int N, float eps, hipStream_t stream) {
    if (param_dtype == BF_DT_F32) return launch_rmsnorm_bwd<T, float>(z, gamma, dy, dz_in, dz, partial, dgamma, rows, N, eps, stream);
    return launch_rmsnorm_bwd<T, T>(z, gamma, dy, dz_in, dz, partial, dgamma, rows, N, eps, stream);
}

// ---- SiLU(gate) * up --------------------------------------------------------------------------------------------------------
// With s = 1 / (1 + exp(-g)):  dgate = dy u s (1 + g (1 - s)),  dup = dy g s.  s and 1 - s are both taken from e = exp(-|g|)
// in (0, 1] — 1 / (1 + e) and e / (1 + e), whichever way round the sign of g says — so nothing overflows, 1 - s keeps its
// relative precision where s rounds to 1, and the limits come out by themselves: g -> -inf gives s = 0 and (0, 0),
// g -> +inf gives 1 - s = 0 and (dy u, dy g).  The bounded factors are multiplied first, dy last.
// The forward's grid: blockIdx.x: 256 vectors of a row, blockIdx.y: rows blockIdx.y, + gridDim.y, ...
template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* gate, long long gate_stride, const T* up, long long up_stride,
                                                         const T* dy, long long dy_stride, T* dgate, long long dgate_stride,
                                                         T* dup, long long dup_stride, long long rows, int nvec) {
    const int vi = blockIdx.x * 256 + threadIdx.x;
    if (vi >= nvec) return;
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        float g[8], u[8], d[8], og[8], ou[8];
        load8(gate + row * gate_stride + vi * 8, g);
        load8(up + row * up_stride + vi * 8, u);
        load8(dy + row * dy_stride + vi * 8, d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float e = expf(-fabsf(g[i]));
            const float big = 1.0f / (1.0f + e), small = e * big;
            const float s = g[i] >= 0.f ? big : small, ms = g[i] >= 0.f ? small : big;
            og[i] = d[i] * (u[i] * (s * fmaf(g[i], ms, 1.0f)));
            ou[i] = d[i] * (g[i] * s);
        }
        store8(dgate + row * dgate_stride + vi * 8, og);
        store8(dup + row * dup_stride + vi * 8, ou);
    }
}

template <typename T>
int launch_swiglu_bwd(const void* gate, long long gs, const void* up, long long us, const void* dy, long long ds, void* dgate,
                      long long dgs, void* dup, long long dus, long long rows, int N, hipStream_t stream) {
    const int nvec = N >> 3;
    const unsigned gx = (unsigned)((nvec + 255) / 256);
    const long long want = 8192 / gx > 0 ? 8192 / gx : 1;
    const unsigned gy = (unsigned)(rows < want ? rows : want);
    hipLaunchKernelGGL((swiglu_bwd_kernel<T>), dim3(gx, gy), dim3(256), 0, stream, (const T*)gate, gs, (const T*)up, us,
                       (const T*)dy, ds, (T*)dgate, dgs, (T*)dup, dus, rows, nvec);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

size_t bf_add_rmsnorm_bwd_workspace_bytes(int64_t rows, int N) {
    if (rows < 1 || N < 1) return 0;
    int G, nb;
    rmsnorm_bwd_layout(rows, N, &G, &nb);
    return (size_t)nb * N * sizeof(float);
}

int bf_add_rmsnorm_bwd(const void* d_z, const void* d_gamma, int param_dtype, const void* d_dy, const void* d_dz_in,
                       void* d_dz, float* d_dgamma, void* d_workspace, size_t workspace_bytes, int dtype, int64_t rows, int N,
                       float eps, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("bf_add_rmsnorm_bwd: bad shape rows=%lld N=%d", (long long)rows, N);
    if (N % 8 || N > 8192) BF_FAIL("bf_add_rmsnorm_bwd: N=%d must be a multiple of 8 and at most 8192", N);
    if (!d_dgamma) BF_FAIL("bf_add_rmsnorm_bwd: null parameter gradient");
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_add_rmsnorm_bwd: unknown dtype %d", dtype);
    if (param_dtype != BF_DT_F32 && param_dtype != dtype)
        BF_FAIL("bf_add_rmsnorm_bwd: gamma must be fp32 or have the activation dtype");
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        BF_HIP_CHECK(hipMemsetAsync(d_dgamma, 0, (size_t)N * sizeof(float), st));
        return 0;
    }
    if (!d_z || !d_gamma || !d_dy || !d_dz) BF_FAIL("bf_add_rmsnorm_bwd: null pointer");
    const uintptr_t al = (uintptr_t)d_z | (uintptr_t)d_gamma | (uintptr_t)d_dy | (uintptr_t)d_dz_in | (uintptr_t)d_dz |
                         (uintptr_t)d_dgamma | (uintptr_t)d_workspace;
    if (al & 15) BF_FAIL("bf_add_rmsnorm_bwd: pointers must be 16-byte aligned");
    const size_t need = bf_add_rmsnorm_bwd_workspace_bytes(rows, N);
    if (!d_workspace || workspace_bytes < need)
        BF_FAIL("bf_add_rmsnorm_bwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    float* partial = reinterpret_cast<float*>(d_workspace);
    switch (dtype) {
        case BF_DT_BF16: return launch_rmsnorm_bwd_gt<__bf16>(d_z, d_gamma, param_dtype, d_dy, d_dz_in, d_dz, partial, d_dgamma, rows, N, eps, st);
        case BF_DT_F16: return launch_rmsnorm_bwd_gt<_Float16>(d_z, d_gamma, param_dtype, d_dy, d_dz_in, d_dz, partial, d_dgamma, rows, N, eps, st);
        default: return launch_rmsnorm_bwd_gt<float>(d_z, d_gamma, param_dtype, d_dy, d_dz_in, d_dz, partial, d_dgamma, rows, N, eps, st);
    }
}

int bf_swiglu_bwd(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, const void* d_dy,
                  int64_t dy_row_stride, void* d_dgate, int64_t dgate_row_stride, void* d_dup, int64_t dup_row_stride,
                  int dtype, int64_t rows, int N, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("bf_swiglu_bwd: bad shape rows=%lld N=%d", (long long)rows, N);
    if (N % 8) BF_FAIL("bf_swiglu_bwd: N=%d must be a multiple of 8", N);
    if (!d_gate || !d_up || !d_dy || !d_dgate || !d_dup) BF_FAIL("bf_swiglu_bwd: null pointer");
    if (((uintptr_t)d_gate | (uintptr_t)d_up | (uintptr_t)d_dy | (uintptr_t)d_dgate | (uintptr_t)d_dup) & 15)
        BF_FAIL("bf_swiglu_bwd: pointers must be 16-byte aligned");
    const int64_t strides[5] = {gate_row_stride, up_row_stride, dy_row_stride, dgate_row_stride, dup_row_stride};
    for (int i = 0; i < 5; ++i)
        if (strides[i] < N || (strides[i] & 7))
            BF_FAIL("bf_swiglu_bwd: row strides (%lld, %lld, %lld, %lld, %lld) must be multiples of 8 and at least N=%d",
                    (long long)strides[0], (long long)strides[1], (long long)strides[2], (long long)strides[3],
                    (long long)strides[4], N);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_swiglu_bwd: unknown dtype %d", dtype);
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define BF_SWB_ARGS d_gate, gate_row_stride, d_up, up_row_stride, d_dy, dy_row_stride, d_dgate, dgate_row_stride, d_dup, dup_row_stride, rows, N, st
    switch (dtype) {
        case BF_DT_BF16: return launch_swiglu_bwd<__bf16>(BF_SWB_ARGS);
        case BF_DT_F16: return launch_swiglu_bwd<_Float16>(BF_SWB_ARGS);
        default: return launch_swiglu_bwd<float>(BF_SWB_ARGS);
    }
#undef BF_SWB_ARGS
}
