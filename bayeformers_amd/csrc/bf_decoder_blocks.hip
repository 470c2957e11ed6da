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

template <typename T, typename CT, int D>
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
            o1[i] = fmaf(x1[i], c1[i], -(x2[i] * s1[i]));
            o2[i] = fmaf(x2[i], c2[i], x1[i] * s2[i]);
        }
        store8(dst, o1);
        store8(dst + D / 2, o2);
    }
}

template <typename T, typename CT>
int launch_rope(const void* q, const void* k, const void* c, const void* s, void* qo, void* ko, int D, const rope_args_t& a,
                hipStream_t stream) {
    const unsigned blocks = (a.total + 255u) / 256u;
    const dim3 grid(blocks < 4096u ? blocks : 4096u), block(256);
    if (D == 64)
        hipLaunchKernelGGL((rope_qk_kernel<T, CT, 64>), grid, block, 0, stream, (const T*)q, (const T*)k, (const CT*)c,
                           (const CT*)s, (T*)qo, (T*)ko, a);
    else
        hipLaunchKernelGGL((rope_qk_kernel<T, CT, 128>), grid, block, 0, stream, (const T*)q, (const T*)k, (const CT*)c,
                           (const CT*)s, (T*)qo, (T*)ko, a);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int launch_rope_ct(const void* q, const void* k, const void* c, const void* s, int cs_dtype, int dtype, void* qo, void* ko,
                   int D, const rope_args_t& a, hipStream_t stream) {
    if (cs_dtype == BF_DT_F32) return launch_rope<T, float>(q, k, c, s, qo, ko, D, a, stream);
    if (cs_dtype == dtype) return launch_rope<T, T>(q, k, c, s, qo, ko, D, a, stream);
    BF_FAIL("bf_rope_qk: cos / sin must be fp32 or have the activation dtype");
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

int bf_rope_qk(const void* d_q, const void* d_k, const void* d_cos, const void* d_sin, int cs_dtype, void* d_q_out,
               void* d_k_out, int dtype, const bf_rope_t* shape, void* stream) {
    if (!shape) BF_FAIL("bf_rope_qk: shape is NULL");
    const bf_rope_t& s = *shape;
    if (s.head_dim != 64 && s.head_dim != 128) BF_FAIL("bf_rope_qk: head_dim=%d must be 64 or 128", s.head_dim);
    if (s.B < 0 || s.T < 1 || s.H < 1 || s.Hkv < 1)
        BF_FAIL("bf_rope_qk: bad shape B=%d T=%d H=%d Hkv=%d", s.B, s.T, s.H, s.Hkv);
    if (s.cos_batch != 1 && s.cos_batch != s.B) BF_FAIL("bf_rope_qk: cos_batch=%d must be 1 or B=%d", s.cos_batch, s.B);
    if (!d_q || !d_k || !d_cos || !d_sin || !d_q_out || !d_k_out) BF_FAIL("bf_rope_qk: null pointer");
    const uintptr_t al = (uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_cos | (uintptr_t)d_sin | (uintptr_t)d_q_out | (uintptr_t)d_k_out;
    if (al & 15) BF_FAIL("bf_rope_qk: pointers must be 16-byte aligned");
    if (!strides_ok(s.q_stride) || !strides_ok(s.k_stride) || !strides_ok(s.q_out_stride) || !strides_ok(s.k_out_stride))
        BF_FAIL("bf_rope_qk: strides must be non-negative multiples of 8 elements");
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16 && dtype != BF_DT_F32) BF_FAIL("bf_rope_qk: unknown dtype %d", dtype);
    if (cs_dtype != BF_DT_F32 && cs_dtype != dtype) BF_FAIL("bf_rope_qk: cos / sin must be fp32 or have the activation dtype");
    const long long total = (long long)s.B * s.T * (s.H + s.Hkv) * (s.head_dim / 16);
    if (total > 0x7fffffffLL) BF_FAIL("bf_rope_qk: B * T * (H + Hkv) * head_dim / 16 = %lld exceeds 2^31 - 1", total);
    if (total == 0) return 0;
    rope_args_t a;
    a.T = s.T, a.H = s.H, a.Hkv = s.Hkv, a.cos_batch = s.cos_batch, a.total = (unsigned)total;
    for (int i = 0; i < 3; ++i)
        a.q[i] = s.q_stride[i], a.k[i] = s.k_stride[i], a.qo[i] = s.q_out_stride[i], a.ko[i] = s.k_out_stride[i];
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case BF_DT_BF16: return launch_rope_ct<__bf16>(d_q, d_k, d_cos, d_sin, cs_dtype, dtype, d_q_out, d_k_out, s.head_dim, a, st);
        case BF_DT_F16: return launch_rope_ct<_Float16>(d_q, d_k, d_cos, d_sin, cs_dtype, dtype, d_q_out, d_k_out, s.head_dim, a, st);
        default: return launch_rope_ct<float>(d_q, d_k, d_cos, d_sin, cs_dtype, dtype, d_q_out, d_k_out, s.head_dim, a, st);
    }
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
