// bf_gemm_skinny_fp8.hip — the kept weights of Model.pinned_samples(keep_weights="fp8") (include/bayeformers_amd_fp8.h):
//   * bf_fp8_rows_quantize: W16 [S][N][K] bf16 draws and their centre C16 [N][K] -> q [S][N][K] e4m3fn of the deviation
//     W16 - C16 with one power-of-two scale per row (s, n);
//   * bf_fp8_rows_dequantize: W^ = bf16(fp32(q * scale + C16)) written out, for the GEMMs that want 16-bit weights;
//   * bf_gemm_nt_skinny_fp8: bf_gemm_skinny.hip's weight stream on q and C16, W^ formed in registers (bitwise the
//     dequantise kernel's: both call fp8_rows_weight below).
// The GEMM keeps the structure of bf_gemm_skinny.hip: 16 output features are the A operand of v_mfma_f32_16x16x32_bf16,
// feature rows past N re-read row N - 1, a workgroup = 4 waves owns 32 features of one sample and one K range, the waves'
// partial sums meet in LDS in a fixed order, split-K by the same rule with a second reduce launch, no atomics.  What
// differs is the k a lane owns: 16 consecutive k of a 64-deep slice (one 16-byte load of q, two of C16, two of x per row),
// feeding two MFMAs — the contraction only needs A and B to agree on which k sits where.  An odd 32-deep slice at the end
// of a K range is taken in bf_gemm_skinny.hip's layout (8 k per lane).
// No host synchronisation or allocation: capturable.
#include "bf_common.h"
#include "bf_device.h"
#include "bf_fp8.h"

namespace {

constexpr int NW = 4;       // waves per workgroup
constexpr int NB = 2;       // 16-feature blocks per workgroup
constexpr int kMaxRows = 64;
// W^ of 8 consecutive k: bf16(fp32(q * scale + c)).  q * scale is exact (a power of two, no underflow at |e| <= 64), so
// the fma rounds once to fp32, then once to bf16.
__device__ __forceinline__ bf16x8_t fp8_rows_weight(u32x2_t q, bf16x8_t c, float scale) {
    float f[8];
    fp8_rows_decode(q, f);
    bf16x8_t w;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (__bf16)fmaf(f[i], scale, (float)c[i]);
    return w;
}

// ---------------------------------------------------------------------------------------------- quantise / dequantise
constexpr int QT = 256;  // threads of a quantise workgroup: one row (s, n)
constexpr int QHOLD = 4;  // 8-element pieces a thread keeps in registers (rows up to QT * QHOLD * 8 = 8192 read once)

// elements k .. k + 7 of a row of K (k % 8 == 0): one 16-byte load when the rows are 16-byte aligned (VEC), else element
// by element with the tail past K read as 0
template <bool VEC>
__device__ __forceinline__ bf16x8_t load8(const __bf16* row, int k, int K) {
    if constexpr (VEC) return *reinterpret_cast<const bf16x8_t*>(row + k);
    bf16x8_t v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = k + i < K ? row[k + i] : (__bf16)0.f;
    return v;
}

template <bool VEC>
__device__ __forceinline__ void deviation8(const __bf16* w, const __bf16* c, int k, int K, float (&d)[8]) {
    const bf16x8_t wv = load8<VEC>(w, k, K), cv = load8<VEC>(c, k, K);
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = (float)wv[i] - (float)cv[i];
}

template <bool VEC>
__global__ __launch_bounds__(QT) void fp8_rows_quantize_kernel(const __bf16* __restrict__ w, const __bf16* __restrict__ center,
                                                               uint8_t* __restrict__ q, float* __restrict__ scale, int N,
                                                               int K) {
    __shared__ float wave_max[QT / 64];
    const long long row = blockIdx.x;  // s * N + n
    const __bf16* wr = w + row * K;
    const __bf16* cr = center + (row % N) * K;
    uint8_t* qr = q + row * K;
    const int pieces = (K + 7) / 8;

    float held[QHOLD][8];
    float amax = 0.f;
#pragma unroll
    for (int h = 0; h < QHOLD; ++h) {
        const int p = threadIdx.x + h * QT;
        if (p < pieces) {
            deviation8<VEC>(wr, cr, p * 8, K, held[h]);
#pragma unroll
            for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(held[h][i]));
        }
    }
    for (int p = threadIdx.x + QHOLD * QT; p < pieces; p += QT) {
        float d[8];
        deviation8<VEC>(wr, cr, p * 8, K, d);
#pragma unroll
        for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(d[i]));
    }
    // the maximum over the workgroup (a maximum does not depend on the order)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = wave_max[0];
#pragma unroll
    for (int i = 1; i < QT / 64; ++i) amax = fmaxf(amax, wave_max[i]);

    const int e = fp8_row_exponent(amax);
    const float inv = pow2f(-e);
    if (threadIdx.x == 0) scale[row] = pow2f(e);

    auto put = [&](int p, const float(&d)[8]) {
        const u32x2_t v = fp8_rows_encode(d, inv);
        if constexpr (VEC) {
            *reinterpret_cast<u32x2_t*>(qr + p * 8) = v;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (p * 8 + i < K) qr[p * 8 + i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
        }
    };
#pragma unroll
    for (int h = 0; h < QHOLD; ++h) {
        const int p = threadIdx.x + h * QT;
        if (p < pieces) put(p, held[h]);
    }
    for (int p = threadIdx.x + QHOLD * QT; p < pieces; p += QT) {  // longer rows: their tail is read again (from L2)
        float d[8];
        deviation8<VEC>(wr, cr, p * 8, K, d);
        put(p, d);
    }
}

// one 8-element piece per thread and step; a row of K is ceil(K / 8) pieces
template <bool VEC>
__global__ __launch_bounds__(256) void fp8_rows_dequantize_kernel(const uint8_t* __restrict__ q, const float* __restrict__ scale,
                                                                  const __bf16* __restrict__ center, __bf16* __restrict__ out,
                                                                  long long rows, int N, int K) {
    const int pieces = (K + 7) / 8;
    const long long total = rows * pieces;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / pieces;
        const int k = (int)(i - row * pieces) * 8;
        const uint8_t* qr = q + row * K;
        const bf16x8_t c = load8<VEC>(center + (row % N) * K, k, K);
        u32x2_t qv;
        if constexpr (VEC) {
            qv = *reinterpret_cast<const u32x2_t*>(qr + k);
        } else {
            qv = u32x2_t{0u, 0u};
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k + j < K) qv[j >> 2] |= (uint32_t)qr[k + j] << (8 * (j & 3));
        }
        const bf16x8_t w = fp8_rows_weight(qv, c, scale[row]);
        __bf16* o = out + row * K + k;
        if constexpr (VEC) {
            *reinterpret_cast<bf16x8_t*>(o) = w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k + j < K) o[j] = w[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------- the skinny GEMM
struct SkinnyFp8Params {
    const __bf16* x;
    long long x_sstride;
    const uint8_t* q;
    const float* scale;
    const __bf16* center;
    const float* bias;
    __bf16* y;
    float* partials;  // [splits][S][M][N] fp32 when splits > 1, else NULL
    int S, M, N, K, act, splits;
};

__device__ __forceinline__ f32x4_t mfma(bf16x8_t a, bf16x8_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

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
        else *reinterpret_cast<bf16x4_t*>(o) = __builtin_convertvector(v, bf16x4_t);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n + j < N) o[j] = (YT)v[j];
    }
}

// U: 64-deep slices per chunk
template <int MB, int U>
__global__ __launch_bounds__(NW * 64) void gemm_skinny_fp8_kernel(const SkinnyFp8Params p) {
    __shared__ f32x4_t red[NW][NB * MB][64];

    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = blockIdx.y, split = blockIdx.z;
    const int M = p.M, N = p.N, K = p.K;
    const int n0 = blockIdx.x * (16 * NB);
    const int nkb = K / 32;
    const int kb0 = (int)((long long)nkb * split / p.splits);
    const int kb1 = (int)((long long)nkb * (split + 1) / p.splits);
    const int g = lane >> 4;  // the lane's k group: k 16 g .. 16 g + 15 of a 64-deep slice, 8 g .. 8 g + 7 of a 32-deep one

    // row starts, without the lane's k offset
    const uint8_t* qrow[NB];
    const __bf16* crow[NB];
    float sc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row = min(n0 + nb * 16 + (lane & 15), N - 1);
        qrow[nb] = p.q + ((long long)s * N + row) * K;
        crow[nb] = p.center + (long long)row * K;
        sc[nb] = p.scale[(long long)s * N + row];
    }
    const __bf16* xrow[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int m = min(mb * 16 + (lane & 15), M - 1);
        xrow[mb] = p.x + (long long)s * p.x_sstride + (long long)m * K;
    }

    f32x4_t acc[NB][MB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int k_begin = kb0 * 32;
    const int npairs = (kb1 - kb0) / 2;  // whole 64-deep slices of this K range
    const int kl = g * 16;

    // whole chunks of U slices, wave-interleaved: all loads of a chunk are issued before its first MFMA
    const int nchunks = npairs / U;
    for (int c = wid; c < nchunks; c += NW) {
        const int k = k_begin + c * U * 64 + kl;
        u32x4_t qv[U][NB];
        bf16x8_t cv[U][NB][2], xf[U][MB][2];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) qv[u][nb] = *reinterpret_cast<const u32x4_t*>(qrow[nb] + k + u * 64);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int h = 0; h < 2; ++h) cv[u][nb][h] = *reinterpret_cast<const bf16x8_t*>(crow[nb] + k + u * 64 + h * 8);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int h = 0; h < 2; ++h) xf[u][mb][h] = *reinterpret_cast<const bf16x8_t*>(xrow[mb] + k + u * 64 + h * 8);
        __builtin_amdgcn_sched_barrier(0);  // keep the whole chunk in flight: no MFMA is hoisted between the loads
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bf16x8_t a = fp8_rows_weight(u32x2_t{qv[u][nb][2 * h], qv[u][nb][2 * h + 1]}, cv[u][nb][h], sc[nb]);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = mfma(a, xf[u][mb][h], acc[nb][mb]);
                }
    }
    // the 64-deep slices left over, one at a time
    for (int pr = nchunks * U + wid; pr < npairs; pr += NW) {
        const int k = k_begin + pr * 64 + kl;
        u32x4_t qv[NB];
        bf16x8_t cv[NB][2], xf[MB][2];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) qv[nb] = *reinterpret_cast<const u32x4_t*>(qrow[nb] + k);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int h = 0; h < 2; ++h) cv[nb][h] = *reinterpret_cast<const bf16x8_t*>(crow[nb] + k + h * 8);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int h = 0; h < 2; ++h) xf[mb][h] = *reinterpret_cast<const bf16x8_t*>(xrow[mb] + k + h * 8);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bf16x8_t a = fp8_rows_weight(u32x2_t{qv[nb][2 * h], qv[nb][2 * h + 1]}, cv[nb][h], sc[nb]);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = mfma(a, xf[mb][h], acc[nb][mb]);
            }
    }
    // an odd 32-deep slice at the end of the range: the wave whose turn it would be, 8 k per lane
    if (((kb1 - kb0) & 1) && wid == npairs % NW) {
        const int k = (kb1 - 1) * 32 + g * 8;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const u32x2_t qv = *reinterpret_cast<const u32x2_t*>(qrow[nb] + k);
            const bf16x8_t a = fp8_rows_weight(qv, *reinterpret_cast<const bf16x8_t*>(crow[nb] + k), sc[nb]);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
                acc[nb][mb] = mfma(a, *reinterpret_cast<const bf16x8_t*>(xrow[mb] + k), acc[nb][mb]);
        }
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
        store4<__bf16>(p.y + ((long long)s * M + m) * N + n, apply_act(v, p.act), n, N);
    }
}

// y = act(sum over the splits in split order + bias): 4 consecutive outputs per thread
__global__ __launch_bounds__(256) void gemm_skinny_fp8_reduce_kernel(const SkinnyFp8Params p) {
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
        store4<__bf16>(p.y + r * N + n, apply_act(v, p.act), n, N);
    }
}

int feature_tiles(int N) { return (N + 16 * NB - 1) / (16 * NB); }

// bf_gemm_skinny.hip's rule (skinny_splits there; tests/test_kept_fp8_cpu.py holds the two workspace sizes equal): K is
// split only while (feature tiles x samples) leaves the chip short of two workgroups per CU, never below 8 32-deep slices
// per wave per split
int skinny_splits(int S, int N, int K) {
    const long long wgs = (long long)feature_tiles(N) * S;
    const int nkb = K / 32;
    const long long want = (512 + wgs - 1) / wgs;
    const int most = nkb / (NW * 8);
    int sp = (int)(want < most ? want : most);
    if (sp > 16) sp = 16;
    return sp < 1 ? 1 : sp;
}

template <int MB>
void launch_mb(const SkinnyFp8Params& p, dim3 grid, hipStream_t stream) {
    constexpr int U = MB <= 2 ? 4 : 2;  // 12 / 6 KiB of q and C16 per wave per chunk: the x fragments' registers bound U
    hipLaunchKernelGGL((gemm_skinny_fp8_kernel<MB, U>), grid, dim3(NW * 64), 0, stream, p);
}

const char* rows_refuse(int w_dtype, int S, int N, int K) {
    if (w_dtype != BF_DT_BF16) return "the 16-bit weights must be bf16 (fp16 lacks the exponent range, fp32 is not kept)";
    if (S < 1 || N < 1 || K < 1) return "unsupported shape (S, N, K >= 1)";
    return nullptr;
}

}  // namespace

int bf_fp8_rows_quantize(const void* d_w, int w_dtype, const void* d_center, void* d_q, float* d_scale, int S, int N, int K,
                         void* stream) {
    if (!d_w || !d_center || !d_q || !d_scale) BF_FAIL("bf_fp8_rows_quantize: NULL operand");
    if (const char* why = rows_refuse(w_dtype, S, N, K)) BF_FAIL("bf_fp8_rows_quantize: %s (S=%d N=%d K=%d)", why, S, N, K);
    if ((long long)S * N > 0x7fffffffLL) BF_FAIL("bf_fp8_rows_quantize: S * N = %lld rows (at most 2^31 - 1)", (long long)S * N);
    if (((uintptr_t)d_w | (uintptr_t)d_center) & 1 || (uintptr_t)d_scale & 3)
        BF_FAIL("bf_fp8_rows_quantize: w and center must be 2-byte, scale 4-byte aligned");
    const bool vec = K % 8 == 0 && !(((uintptr_t)d_w | (uintptr_t)d_center) & 15) && !((uintptr_t)d_q & 7);
    const dim3 grid((uint32_t)((long long)S * N));
    auto w = static_cast<const __bf16*>(d_w), c = static_cast<const __bf16*>(d_center);
    if (vec) hipLaunchKernelGGL(fp8_rows_quantize_kernel<true>, grid, dim3(QT), 0, (hipStream_t)stream, w, c, static_cast<uint8_t*>(d_q), d_scale, N, K);
    else hipLaunchKernelGGL(fp8_rows_quantize_kernel<false>, grid, dim3(QT), 0, (hipStream_t)stream, w, c, static_cast<uint8_t*>(d_q), d_scale, N, K);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_fp8_rows_dequantize(const void* d_q, const float* d_scale, const void* d_center, void* d_w_out, int w_dtype, int S,
                           int N, int K, void* stream) {
    if (!d_q || !d_scale || !d_center || !d_w_out) BF_FAIL("bf_fp8_rows_dequantize: NULL operand");
    if (const char* why = rows_refuse(w_dtype, S, N, K)) BF_FAIL("bf_fp8_rows_dequantize: %s (S=%d N=%d K=%d)", why, S, N, K);
    if (((uintptr_t)d_w_out | (uintptr_t)d_center) & 1 || (uintptr_t)d_scale & 3)
        BF_FAIL("bf_fp8_rows_dequantize: w_out and center must be 2-byte, scale 4-byte aligned");
    const bool vec = K % 8 == 0 && !(((uintptr_t)d_w_out | (uintptr_t)d_center) & 15) && !((uintptr_t)d_q & 7);
    const long long rows = (long long)S * N;
    const long long work = rows * ((K + 7) / 8);
    const long long blocks = (work + 255) / 256;
    const dim3 grid((uint32_t)(blocks < 65536 ? blocks : 65536));
    auto q = static_cast<const uint8_t*>(d_q);
    auto c = static_cast<const __bf16*>(d_center);
    auto o = static_cast<__bf16*>(d_w_out);
    if (vec) hipLaunchKernelGGL(fp8_rows_dequantize_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, q, d_scale, c, o, rows, N, K);
    else hipLaunchKernelGGL(fp8_rows_dequantize_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, q, d_scale, c, o, rows, N, K);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

size_t bf_gemm_nt_skinny_fp8_workspace_bytes(int S, int M, int N, int K) {
    if (S < 1 || M < 1 || N < 1 || K < 32) return 0;
    const int sp = skinny_splits(S, N, K);
    return sp > 1 ? (size_t)sp * S * M * N * sizeof(float) : 0;
}

int bf_gemm_nt_skinny_fp8(const void* d_x, int x_dtype, int64_t x_sample_stride, const void* d_q, const float* d_scale,
                          const void* d_center, const float* d_bias, void* d_y, int y_dtype, int S, int M, int N, int K,
                          int act, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!d_x || !d_q || !d_scale || !d_center || !d_y) BF_FAIL("bf_gemm_nt_skinny_fp8: NULL operand");
    if (act != BF_ACT_NONE && act != BF_ACT_GELU) BF_FAIL("bf_gemm_nt_skinny_fp8: unknown activation %d", act);
    if (x_dtype != BF_DT_BF16 || y_dtype != BF_DT_BF16)
        BF_FAIL("bf_gemm_nt_skinny_fp8: x and y must be bf16 (the dequantised weights are exact in bf16 only)");
    if (S < 1 || S > 65535 || M < 1 || M > kMaxRows || N < 1 || K < 32 || K % 32 != 0)
        BF_FAIL("bf_gemm_nt_skinny_fp8: unsupported shape (1 <= S <= 65535, 1 <= M <= 64, K %% 32 == 0) (S=%d M=%d N=%d K=%d)", S,
                M, N, K);
    if (((uintptr_t)d_x | (uintptr_t)d_q | (uintptr_t)d_center | (uintptr_t)(x_sample_stride * 2)) & 15)
        BF_FAIL("bf_gemm_nt_skinny_fp8: x, q, center and the x sample stride must be 16-byte aligned");
    if ((uintptr_t)d_scale & 3) BF_FAIL("bf_gemm_nt_skinny_fp8: scale must be 4-byte aligned");
    if (x_sample_stride < (int64_t)M * K)
        BF_FAIL("bf_gemm_nt_skinny_fp8: x sample stride %lld < the rows of a sample", (long long)x_sample_stride);
    if ((uintptr_t)d_y & 7) BF_FAIL("bf_gemm_nt_skinny_fp8: y must be 8-byte aligned");
    SkinnyFp8Params p{};
    p.x = static_cast<const __bf16*>(d_x);
    p.x_sstride = x_sample_stride;
    p.q = static_cast<const uint8_t*>(d_q);
    p.scale = d_scale;
    p.center = static_cast<const __bf16*>(d_center);
    p.bias = d_bias;
    p.y = static_cast<__bf16*>(d_y);
    p.S = S; p.M = M; p.N = N; p.K = K; p.act = act;
    p.splits = skinny_splits(S, N, K);
    if (p.splits > 1) {
        const size_t need = (size_t)p.splits * S * M * N * sizeof(float);
        if (!d_workspace || workspace_bytes < need)
            BF_FAIL("bf_gemm_nt_skinny_fp8: needs %zu workspace bytes (got %zu)", need, d_workspace ? workspace_bytes : (size_t)0);
        if ((uintptr_t)d_workspace & 15) BF_FAIL("bf_gemm_nt_skinny_fp8: workspace must be 16-byte aligned");
        p.partials = static_cast<float*>(d_workspace);
    }
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((uint32_t)feature_tiles(N), (uint32_t)S, (uint32_t)p.splits);
    switch ((M + 15) / 16) {
        case 1: launch_mb<1>(p, grid, st); break;
        case 2: launch_mb<2>(p, grid, st); break;
        case 3: launch_mb<3>(p, grid, st); break;
        default: launch_mb<4>(p, grid, st); break;
    }
    BF_HIP_CHECK(hipGetLastError());
    if (p.splits > 1) {
        const long long work = (long long)S * M * ((N + 3) / 4);
        const long long blocks = (work + 255) / 256;
        hipLaunchKernelGGL(gemm_skinny_fp8_reduce_kernel, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, p);
        BF_HIP_CHECK(hipGetLastError());
    }
    return 0;
}
