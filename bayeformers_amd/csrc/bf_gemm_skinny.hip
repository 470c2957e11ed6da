// bf_gemm_skinny.hip — batched NT GEMM for a few rows per sample on weights that already sit in HBM:
//   y[s] = act(x[s] W_s^T + b_s),  x [S][M][K] (sample stride x_sstride), W_s [S][N][K] 16-bit, b_s [S][N] fp32, M <= 64.
// What a decode step of a generation runs on the weights Model.pinned_samples(keep_weights=True) drew once
// (F.linear, /root/reference/bayeformers/nn/layers/linear.py:104).  At M <= 64 every W_s element is used by at most four
// MFMAs, so the launch is a stream over the weights:
//   * the MFMA orientation of bf_fused_small: 16 output features are the A operand of v_mfma_f32_16x16x32, a lane holds 8
//     consecutive k of one feature row (one 16-byte load), the K-contiguous activation fragment (L2-resident) is B;
//   * a workgroup = 4 waves owns 2 feature blocks (32 features) of one sample and one K range; its waves take chunks of U
//     32-deep slices in turn, each chunk issued as NB * U 16-byte loads per lane before its MFMAs (16 KiB of weights in
//     flight per wave at M <= 32);
//   * feature rows past N re-read row N - 1 (never stored), so no load is predicated;
//   * the four waves' partial sums meet in LDS in a fixed order; when the grid of (feature blocks x samples) is too small
//     to fill the chip at large K, K is split over `splits` workgroups whose fp32 partials (caller workspace) a second
//     launch sums in split order, then adds the bias and the activation.  No atomics: bitwise reproducible.
// No host synchronisation or allocation: capturable.
#include "bf_common.h"
#include "bf_device.h"

namespace {

constexpr int NW = 4;       // waves per workgroup
constexpr int NB = 2;       // 16-feature blocks per workgroup
constexpr int kMaxRows = 64;

struct SkinnyParams {
    const void* x;
    long long x_sstride;
    long long x_rstride;  // elements between consecutive rows of x (K for rows back to back)
    const void* w;
    const float* bias;
    void* y;
    float* partials;  // [splits][S][M][N] fp32 when splits > 1, else NULL
    int S, M, N, K, act, splits;
};

template <typename T>
struct Mfma;
template <>
struct Mfma<__bf16> {
    using frag = bf16x8_t;
    using vec4 = bf16x4_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <>
struct Mfma<_Float16> {
    using frag = f16x8_t;
    using vec4 = f16x4_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

__device__ __forceinline__ f32x4_t apply_act(f32x4_t v, int act) {
    if (act == BF_ACT_GELU) {
        const f32x2_t lo = bf_gelu2(f32x2_t{v[0], v[1]}), hi = bf_gelu2(f32x2_t{v[2], v[3]});
        v = f32x4_t{lo[0], lo[1], hi[0], hi[1]};
    }
    return v;
}

// four consecutive outputs n .. n + 3 of one row; the tail of N element by element
template <typename YT>
__device__ __forceinline__ void store4(YT* o, f32x4_t v, int n, int N) {
    if (n + 3 < N && (N & 3) == 0) {
        if constexpr (sizeof(YT) == 4) *reinterpret_cast<f32x4_t*>(o) = v;
        else *reinterpret_cast<typename Mfma<YT>::vec4*>(o) = __builtin_convertvector(v, typename Mfma<YT>::vec4);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n + j < N) o[j] = (YT)v[j];
    }
}

template <typename T, int MB, int U>
__global__ __launch_bounds__(NW * 64) void gemm_skinny_kernel(const SkinnyParams p) {
    using frag = typename Mfma<T>::frag;
    __shared__ f32x4_t red[NW][NB * MB][64];

    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = blockIdx.y, split = blockIdx.z;
    const int M = p.M, N = p.N, K = p.K;
    const int n0 = blockIdx.x * (16 * NB);
    const int nkb = K / 32;
    const int kb0 = (int)((long long)nkb * split / p.splits);
    const int kb1 = (int)((long long)nkb * (split + 1) / p.splits);
    const int kq = (lane >> 4) * 8;

    const T* wrow[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row = min(n0 + nb * 16 + (lane & 15), N - 1);
        wrow[nb] = reinterpret_cast<const T*>(p.w) + ((long long)s * N + row) * K + kq;
    }
    const T* xrow[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int m = min(mb * 16 + (lane & 15), M - 1);
        xrow[mb] = reinterpret_cast<const T*>(p.x) + (long long)s * p.x_sstride + (long long)m * p.x_rstride + kq;
    }

    f32x4_t acc[NB][MB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // whole chunks of U slices, wave-interleaved: all loads of a chunk are issued before its first MFMA
    const int nchunks = (kb1 - kb0) / U;
    for (int c = wid; c < nchunks; c += NW) {
        const int k = (kb0 + c * U) * 32;
        frag wf[U][NB], xf[U][MB];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) wf[u][nb] = *reinterpret_cast<const frag*>(wrow[nb] + k + u * 32);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) xf[u][mb] = *reinterpret_cast<const frag*>(xrow[mb] + k + u * 32);
        __builtin_amdgcn_sched_barrier(0);  // keep the whole chunk in flight: no MFMA is hoisted between the loads
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = Mfma<T>::run(wf[u][nb], xf[u][mb], acc[nb][mb]);
    }
    // the slices left over, one at a time
    for (int kb = kb0 + nchunks * U + wid; kb < kb1; kb += NW) {
        const int k = kb * 32;
        frag wf[NB], xf[MB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) wf[nb] = *reinterpret_cast<const frag*>(wrow[nb] + k);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) xf[mb] = *reinterpret_cast<const frag*>(xrow[mb] + k);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = Mfma<T>::run(wf[nb], xf[mb], acc[nb][mb]);
    }

#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) red[wid][nb * MB + mb][lane] = acc[nb][mb];
    __syncthreads();

    // D of block (nb, mb): lane holds features n0 + nb*16 + (lane>>4)*4 + j of row mb*16 + (lane&15)
    for (int i = wid; i < NB * MB; i += NW) {
        f32x4_t v = red[0][i][lane];
#pragma unroll
        for (int w = 1; w < NW; ++w) v += red[w][i][lane];
        const int nb = i / MB, mb = i % MB;
        const int m = mb * 16 + (lane & 15);
        const int n = n0 + nb * 16 + (lane >> 4) * 4;
        if (m >= M || n >= N) continue;
        if (p.partials) {
            store4<float>(p.partials + (((long long)split * p.S + s) * M + m) * N + n, v, n, N);
            continue;
        }
        if (p.bias) {
            const float* b = p.bias + (long long)s * N + n;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < N) v[j] += b[j];
        }
        store4<T>(reinterpret_cast<T*>(p.y) + ((long long)s * M + m) * N + n, apply_act(v, p.act), n, N);
    }
}

// y = act(sum over the splits in split order + bias): 4 consecutive outputs per thread
template <typename T>
__global__ __launch_bounds__(256) void gemm_skinny_reduce_kernel(const SkinnyParams p) {
    const int N = p.N;
    const int nq = (N + 3) / 4;
    const long long rows = (long long)p.S * p.M;
    const long long total = rows * nq;
    const long long plane = rows * N;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / nq;
        const int n = (int)(i - r * nq) * 4;
        const int s = (int)(r / p.M);
        f32x4_t v = {0.f, 0.f, 0.f, 0.f};
        for (int sp = 0; sp < p.splits; ++sp) {
            const float* q = p.partials + sp * plane + r * N + n;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < N) v[j] += q[j];
        }
        if (p.bias) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < N) v[j] += p.bias[(long long)s * N + n + j];
        }
        store4<T>(reinterpret_cast<T*>(p.y) + r * N + n, apply_act(v, p.act), n, N);
    }
}

// workgroups along N for one sample
int feature_tiles(int N) { return (N + 16 * NB - 1) / (16 * NB); }

// K is split only while (feature tiles x samples) leaves the chip short of two workgroups per CU, and never below one
// chunk of 8 slices per wave per split: a function of the shape alone
int skinny_splits(int S, int N, int K) {
    const long long wgs = (long long)feature_tiles(N) * S;
    const int nkb = K / 32;
    const long long want = (512 + wgs - 1) / wgs;
    const int most = nkb / (NW * 8);
    int sp = (int)(want < most ? want : most);
    if (sp > 16) sp = 16;
    return sp < 1 ? 1 : sp;
}

template <typename T, int MB>
void launch_mb(const SkinnyParams& p, dim3 grid, hipStream_t stream) {
    constexpr int U = MB <= 2 ? 8 : 4;  // 16 / 8 KiB of weights per wave per chunk: the registers of the x fragments bound U
    hipLaunchKernelGGL((gemm_skinny_kernel<T, MB, U>), grid, dim3(NW * 64), 0, stream, p);
}

template <typename T>
int launch(SkinnyParams p, hipStream_t stream) {
    const int MB = (p.M + 15) / 16;
    const dim3 grid((uint32_t)feature_tiles(p.N), (uint32_t)p.S, (uint32_t)p.splits);
    switch (MB) {
        case 1: launch_mb<T, 1>(p, grid, stream); break;
        case 2: launch_mb<T, 2>(p, grid, stream); break;
        case 3: launch_mb<T, 3>(p, grid, stream); break;
        default: launch_mb<T, 4>(p, grid, stream); break;
    }
    BF_HIP_CHECK(hipGetLastError());
    if (p.splits > 1) {
        const long long work = (long long)p.S * p.M * ((p.N + 3) / 4);
        const long long blocks = (work + 255) / 256;
        hipLaunchKernelGGL(gemm_skinny_reduce_kernel<T>, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, p);
        BF_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace

int bf_gemm_nt_skinny_max_rows(void) { return kMaxRows; }

size_t bf_gemm_nt_skinny_workspace_bytes(int S, int M, int N, int K) {
    if (S < 1 || M < 1 || N < 1 || K < 32) return 0;
    const int sp = skinny_splits(S, N, K);
    return sp > 1 ? (size_t)sp * S * M * N * sizeof(float) : 0;
}

const char* bf_gemm_skinny_refuses(int x_dtype, int w_dtype, int y_dtype, int S, int M, int N, int K,
                                   int64_t x_sample_stride, int64_t x_row_stride, const void* d_x, const void* d_w) {
    if (w_dtype != BF_DT_BF16 && w_dtype != BF_DT_F16) return "weights must be bf16 or fp16";
    if (x_dtype != w_dtype || y_dtype != x_dtype) return "x and y must have the weights' dtype";
    if (S < 1 || S > 65535 || M < 1 || M > kMaxRows || N < 1 || K < 32 || K % 32 != 0)
        return "unsupported shape (1 <= S <= 65535, 1 <= M <= 64, K % 32 == 0)";
    if (((uintptr_t)d_x | (uintptr_t)d_w | (uintptr_t)(x_sample_stride * 2) | (uintptr_t)(x_row_stride * 2)) & 15)
        return "x, w and the x sample and row strides must be 16-byte aligned";
    return nullptr;
}

int bf_launch_gemm_skinny(const void* d_x, int x_dtype, int64_t x_sample_stride, const void* d_w, int w_dtype,
                          const float* d_bias, void* d_y, int y_dtype, int S, int M, int N, int K, int act,
                          void* d_workspace, size_t workspace_bytes, hipStream_t stream, int64_t x_row_stride) {
    if (!d_x || !d_w || !d_y) BF_FAIL("bf_gemm_nt_skinny: NULL operand");
    if (act != BF_ACT_NONE && act != BF_ACT_GELU) BF_FAIL("bf_gemm_nt_skinny: unknown activation %d", act);
    if (!x_row_stride) x_row_stride = K;
    if (const char* why = bf_gemm_skinny_refuses(x_dtype, w_dtype, y_dtype, S, M, N, K, x_sample_stride, x_row_stride, d_x, d_w))
        BF_FAIL("bf_gemm_nt_skinny: %s (S=%d M=%d N=%d K=%d, x sample stride %lld, row stride %lld)", why, S, M, N, K,
                (long long)x_sample_stride, (long long)x_row_stride);
    if (x_row_stride < K) BF_FAIL("bf_gemm_nt_skinny: x row stride %lld < K", (long long)x_row_stride);
    if (x_sample_stride < (int64_t)(M - 1) * x_row_stride + K)
        BF_FAIL("bf_gemm_nt_skinny: x sample stride %lld < the rows of a sample", (long long)x_sample_stride);
    if ((uintptr_t)d_y & 7) BF_FAIL("bf_gemm_nt_skinny: y must be 8-byte aligned");
    SkinnyParams p{};
    p.x = d_x;
    p.x_sstride = x_sample_stride;
    p.x_rstride = x_row_stride;
    p.w = d_w;
    p.bias = d_bias;
    p.y = d_y;
    p.S = S; p.M = M; p.N = N; p.K = K; p.act = act;
    p.splits = skinny_splits(S, N, K);
    if (p.splits > 1) {
        const size_t need = (size_t)p.splits * S * M * N * sizeof(float);
        if (!d_workspace || workspace_bytes < need)
            BF_FAIL("bf_gemm_nt_skinny: needs %zu workspace bytes (got %zu)", need, d_workspace ? workspace_bytes : (size_t)0);
        if ((uintptr_t)d_workspace & 15) BF_FAIL("bf_gemm_nt_skinny: workspace must be 16-byte aligned");
        p.partials = static_cast<float*>(d_workspace);
    }
    if (w_dtype == BF_DT_BF16) return launch<__bf16>(p, stream);
    return launch<_Float16>(p, stream);
}

int bf_gemm_nt_skinny(const void* d_x, int x_dtype, int64_t x_sample_stride, const void* d_w, int w_dtype,
                      const float* d_bias, void* d_y, int y_dtype, int S, int M, int N, int K, int act, void* d_workspace,
                      size_t workspace_bytes, void* stream) {
    if ((uintptr_t)d_y & 7) BF_FAIL("bf_gemm_nt_skinny: y must be 8-byte aligned");
    return bf_launch_gemm_skinny(d_x, x_dtype, x_sample_stride, d_w, w_dtype, d_bias, d_y, y_dtype, S, M, N, K, act,
                                 d_workspace, workspace_bytes, (hipStream_t)stream);
}
