// bf_lrt.hip — the local reparameterisation estimator of bnn.Linear (include/bayeformers_amd_lrt.h): the layer samples its
// pre-activations, y = act(m + sqrt(v) * zeta) with m = x mu^T + mu_b and v = x^2 (sigma^2)^T + sigma_b^2, instead of its
// weights.  The matrix products are the caller's (bf_gemm_nt_act, bf_gemm_nn, bf_gemm_tn); the kernels here are the
// memory- / VALU-bound passes around them.  bf16 only.
//
// Kernels in this file (a lane owns 8 consecutive elements of one row: 16 bytes of a 16-bit tensor)
//   lrt_operands_kernel<OT>  : fp32 masters (mu, rho) -> the pair [mu; softplus(rho)^2] in bf16 (weights) or fp32 (bias)
//   lrt_square_kernel        : x -> [x; x^2] (or x^2 alone), rows past R of the padded operand written as zeros
//   lrt_combine_kernel       : m, v (fp32) -> y = act(m + sqrt(v) zeta), optionally the pre-activation and sqrt(v) in bf16;
//                              zeta drawn in registers (two Philox groups per lane)
//   lrt_zeta_kernel          : zeta alone in fp32, any shape (what the framework composite and the tests read)
//   lrt_grad_prepare_kernel  : dy (, pre), sqrt(v), regenerated zeta -> [dm; dv] in bf16 and, per chunk of 256 rows, the
//                              column sums of their fp32 values; lrt_colsum_finish_kernel adds the chunks in order
//   lrt_dx_kernel            : dx = a + 2 x o b from the two slabs of the NN product
//   lrt_drho_kernel          : drho = dsigma2 * 2 sigma sigmoid(rho)
//   kl_gaussian_kernel / kl_gaussian_finish_kernel : the closed-form E_q log p and E_q log q of one tensor under a Gaussian
//                              prior, fp64, block partials added in block order
// No atomics anywhere: every output element is written by one thread and every sum has a fixed order.
#include "bf_common.h"
#include "bf_philox.h"

namespace {

constexpr int kChunkRows = 256;   // rows per column-sum chunk of lrt_grad_prepare_kernel
constexpr int kKlBlocks = 1024;   // most block partials of kl_gaussian_kernel

__device__ __forceinline__ float softplus_f(float rho) { return fmaxf(rho, 0.f) + log1pf(expf(-fabsf(rho))); }
__device__ __forceinline__ float sigmoid_f(float rho) {
    const float e = expf(-fabsf(rho));
    return (rho >= 0.f ? 1.f : e) / (1.f + e);
}
// erf-GELU through erfcf: relative accuracy in both tails (the GEMM epilogue's polynomial is absolute-accurate only)
__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * erfcf(-0.70710678118654752f * x); }

__device__ __forceinline__ void store_pair(__bf16* w, size_t off, const float (&a)[8]) {
    bf16x8_t r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (__bf16)a[i];
    *reinterpret_cast<bf16x8_t*>(w + off) = r;
}
__device__ __forceinline__ void store_pair(float* w, size_t off, const float (&a)[8]) {
    *reinterpret_cast<f32x4_t*>(w + off) = f32x4_t{a[0], a[1], a[2], a[3]};
    *reinterpret_cast<f32x4_t*>(w + off + 4) = f32x4_t{a[4], a[5], a[6], a[7]};
}

// out[0][e] = mu[e], out[1][e] = softplus(rho[e])^2, e < n (n % 8 == 0)
template <typename OT>
__global__ __launch_bounds__(256) void lrt_operands_kernel(const float* __restrict__ mu, const float* __restrict__ rho,
                                                           OT* __restrict__ out, unsigned long long n8, unsigned long long n) {
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n8; i += (unsigned long long)gridDim.x * 256ull) {
        const f32x4_t m0 = *reinterpret_cast<const f32x4_t*>(mu + i * 8), m1 = *reinterpret_cast<const f32x4_t*>(mu + i * 8 + 4);
        const f32x4_t r0 = *reinterpret_cast<const f32x4_t*>(rho + i * 8), r1 = *reinterpret_cast<const f32x4_t*>(rho + i * 8 + 4);
        float a[8], b[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = m0[j];
            a[4 + j] = m1[j];
            const float s0 = softplus_f(r0[j]), s1 = softplus_f(r1[j]);
            b[j] = s0 * s0;
            b[4 + j] = s1 * s1;
        }
        store_pair(out, i * 8, a);
        store_pair(out, n + i * 8, b);
    }
}

// xx[0][r][k] = x[r][k] (pair only), xx[1][r][k] = x[r][k]^2 for r < R, zeros for R <= r < R_pad.  slab = R_pad * K.
__global__ __launch_bounds__(256) void lrt_square_kernel(const __bf16* __restrict__ x, __bf16* __restrict__ xx,
                                                         unsigned long long n8, unsigned long long pad8,
                                                         unsigned long long slab, int pair) {
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < pad8; i += (unsigned long long)gridDim.x * 256ull) {
        bf16x8_t v = {}, q = {};
        if (i < n8) {
            v = *reinterpret_cast<const bf16x8_t*>(x + i * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float f = (float)v[j];
                q[j] = (__bf16)(f * f);
            }
        }
        if (pair) *reinterpret_cast<bf16x8_t*>(xx + i * 8) = v;
        *reinterpret_cast<bf16x8_t*>(xx + slab + i * 8) = q;
    }
}

struct ZetaParams {
    uint32_t k0, k1, sample_base, stream;
    const uint32_t* counter;
};

// the 8 normals of elements e0 .. e0 + 7 (e0 % 8 == 0) of global sample `sample`
__device__ __forceinline__ void zeta8(const ZetaParams& z, uint32_t sample, unsigned long long e0, float (&out)[8]) {
    const unsigned long long g = e0 >> 2;
    float a[4], b[4];
    bf_normal4_dev((uint32_t)g, (uint32_t)(g >> 32), sample, z.stream, z.k0, z.k1, a);
    bf_normal4_dev((uint32_t)(g + 1), (uint32_t)((g + 1) >> 32), sample, z.stream, z.k0, z.k1, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        out[j] = a[j];
        out[4 + j] = b[j];
    }
}

// y[row][n] = act(m + sqrt(v) zeta); row = s * M + i, element e = i * N + n of sample s.  G = N / 8 lanes per row.
__global__ __launch_bounds__(256) void lrt_combine_kernel(const float* __restrict__ m, const float* __restrict__ v,
                                                          __bf16* __restrict__ y, __bf16* __restrict__ pre,
                                                          __bf16* __restrict__ sd, unsigned long long total, int M, int N,
                                                          int G, int act, ZetaParams zp) {
    const uint32_t first = zp.sample_base + (zp.counter ? *zp.counter : 0u);
    for (unsigned long long idx = blockIdx.x * 256ull + threadIdx.x; idx < total; idx += (unsigned long long)gridDim.x * 256ull) {
        const unsigned long long row = idx / (unsigned)G;
        const int n0 = (int)(idx - row * (unsigned)G) * 8;
        const unsigned long long s = row / (unsigned)M, i = row - s * (unsigned)M;
        const size_t off = (size_t)row * N + n0;
        const f32x4_t m0 = *reinterpret_cast<const f32x4_t*>(m + off), m1 = *reinterpret_cast<const f32x4_t*>(m + off + 4);
        const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(v + off), v1 = *reinterpret_cast<const f32x4_t*>(v + off + 4);
        float z[8];
        zeta8(zp, first + (uint32_t)s, i * (unsigned long long)N + n0, z);
        bf16x8_t ry, rp, rs;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float mj = j < 4 ? m0[j] : m1[j - 4], vj = j < 4 ? v0[j] : v1[j - 4];
            const float sj = __builtin_sqrtf(fmaxf(vj, 0.f));
            const float p = fmaf(sj, z[j], mj);
            rp[j] = (__bf16)p;
            rs[j] = (__bf16)sj;
            ry[j] = (__bf16)(act == BF_ACT_GELU ? gelu_exact(p) : p);
        }
        *reinterpret_cast<bf16x8_t*>(y + off) = ry;
        if (pre) *reinterpret_cast<bf16x8_t*>(pre + off) = rp;
        if (sd) *reinterpret_cast<bf16x8_t*>(sd + off) = rs;
    }
}

// out[s][e] = zeta of element e of sample s, e < mn: one Philox group per lane, any M and N
__global__ __launch_bounds__(256) void lrt_zeta_kernel(float* __restrict__ out, unsigned long long total,
                                                       unsigned long long groups, unsigned long long mn, ZetaParams zp) {
    const uint32_t first = zp.sample_base + (zp.counter ? *zp.counter : 0u);
    for (unsigned long long idx = blockIdx.x * 256ull + threadIdx.x; idx < total; idx += (unsigned long long)gridDim.x * 256ull) {
        const unsigned long long s = idx / groups, g = idx - s * groups;
        float z[4];
        bf_normal4_dev((uint32_t)g, (uint32_t)(g >> 32), first + (uint32_t)s, zp.stream, zp.k0, zp.k1, z);
        float* o = out + s * mn + g * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (g * 4 + j < mn) o[j] = z[j];
    }
}

// g = dy (* gelu'(pre)); dm = g, dv = g zeta / (2 sqrt(v)) (0 where sqrt(v) == 0), both rounded to bf16 into the slabs of
// dmdv ([2][R_pad][N], rows R .. R_pad zero) and the column sums of the fp32 values (before that rounding: a column of large
// dv of both signs would otherwise keep the roundings of its terms) of this chunk of rows into partial[which][chunk][n].  Block = 64 column vectors (512 columns) x 4 row lanes, as the bias-gradient passes of
// bf_backward.hip.
__global__ __launch_bounds__(256) void lrt_grad_prepare_kernel(const __bf16* __restrict__ dy, const __bf16* __restrict__ pre,
                                                               const __bf16* __restrict__ sd, __bf16* __restrict__ dmdv,
                                                               float* __restrict__ partial, int R, int R_pad, int M, int N,
                                                               int chunks, ZetaParams zp) {
    __shared__ float sh[4][64][16];
    const int ch = blockIdx.y, cl = threadIdx.x & 63, cv = blockIdx.x * 64 + cl, rl = threadIdx.x >> 6;
    const uint32_t first = zp.sample_base + (zp.counter ? *zp.counter : 0u);
    const size_t slab = (size_t)R_pad * N;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    const int r1 = min(R_pad, (ch + 1) * kChunkRows);
    if (cv * 8 < N) {
        for (int row = ch * kChunkRows + rl; row < r1; row += 4) {
            const size_t off = (size_t)row * N + cv * 8;
            bf16x8_t rm = {}, rv = {};
            if (row < R) {
                const bf16x8_t g8 = __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(dy + off));
                const bf16x8_t s8 = __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(sd + off));
                bf16x8_t p8 = {};
                if (pre) p8 = __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(pre + off));
                const int s = row / M, i = row - s * M;
                float z[8];
                zeta8(zp, first + (uint32_t)s, (unsigned long long)i * N + cv * 8, z);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float g = (float)g8[j];
                    if (pre) g *= bf_gelu_grad((float)p8[j]);
                    const float sj = (float)s8[j];
                    const float dv = sj > 0.f ? g * z[j] / (2.f * sj) : 0.f;
                    rm[j] = (__bf16)g;
                    rv[j] = (__bf16)dv;
                    acc[j] += g;
                    acc[8 + j] += dv;
                }
            }
            *reinterpret_cast<bf16x8_t*>(dmdv + off) = rm;
            *reinterpret_cast<bf16x8_t*>(dmdv + slab + off) = rv;
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) sh[rl][cl][j] = acc[j];
    __syncthreads();
    if (rl == 0 && cv * 8 < N) {
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            float* o = partial + ((size_t)w * chunks + ch) * N + cv * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                o[j] = (sh[0][cl][w * 8 + j] + sh[1][cl][w * 8 + j]) + (sh[2][cl][w * 8 + j] + sh[3][cl][w * 8 + j]);
        }
    }
}

// out[w][n] = partial[w][0][n] + partial[w][1][n] + ..., the chunks in order
__global__ __launch_bounds__(256) void lrt_colsum_finish_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                                int N, int chunks) {
    const int n = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
    if (n >= N) return;
    const float* src = partial + (size_t)w * chunks * N + n;
    float sum = src[0];
    for (int c = 1; c < chunks; ++c) sum += src[(size_t)c * N];
    out[(size_t)w * N + n] = sum;
}

// dx[r][k] = a[r][k] + 2 x[r][k] b[r][k]; a = ab, b = ab + slab
__global__ __launch_bounds__(256) void lrt_dx_kernel(const __bf16* __restrict__ ab, unsigned long long slab,
                                                     const __bf16* __restrict__ x, __bf16* __restrict__ dx,
                                                     unsigned long long n8) {
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n8; i += (unsigned long long)gridDim.x * 256ull) {
        const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(ab + i * 8);
        const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(ab + slab + i * 8);
        const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(x + i * 8);
        bf16x8_t r;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = (__bf16)fmaf(2.f * (float)v[j], (float)b[j], (float)a[j]);
        *reinterpret_cast<bf16x8_t*>(dx + i * 8) = r;
    }
}

// drho[e] = dsig2[e] * 2 softplus(rho[e]) sigmoid(rho[e]), e < n (n % 4 == 0)
__global__ __launch_bounds__(256) void lrt_drho_kernel(const float* __restrict__ dsig2, const float* __restrict__ rho,
                                                       float* __restrict__ drho, unsigned long long n4) {
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n4; i += (unsigned long long)gridDim.x * 256ull) {
        const f32x4_t d = *reinterpret_cast<const f32x4_t*>(dsig2 + i * 4), r = *reinterpret_cast<const f32x4_t*>(rho + i * 4);
        f32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = d[j] * (2.f * softplus_f(r[j]) * sigmoid_f(r[j]));
        *reinterpret_cast<f32x4_t*>(drho + i * 4) = o;
    }
}

// E_q log p = -sum(log sp + c + (sigma^2 + (mu - mu_p)^2) / (2 sp^2)), E_q log q = -sum(log sigma + c + 1/2), c = log sqrt(2 pi):
// every thread adds its elements (a fixed set: the grid is a function of n alone) in index order, the block's 256 sums
// meet in a fixed tree, partial[block] = {E log p, E log q}.
__device__ __forceinline__ double softplus_d(double rho) { return fmax(rho, 0.0) + log1p(exp(-fabs(rho))); }
__global__ __launch_bounds__(256) void kl_gaussian_kernel(const float* __restrict__ mu, const float* __restrict__ rho,
                                                          const float* __restrict__ pmu, const float* __restrict__ prho,
                                                          unsigned long long n, double* __restrict__ partial) {
    __shared__ double sh[2][256];
    const double c = 0.91893853320467274178;
    double lp = 0.0, lq = 0.0;
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
        const double sg = softplus_d((double)rho[i]), sp = softplus_d((double)prho[i]);
        const double d = (double)mu[i] - (double)pmu[i];
        lp -= log(sp) + c + (sg * sg + d * d) / (2.0 * sp * sp);
        lq -= log(sg) + c + 0.5;
    }
    sh[0][threadIdx.x] = lp;
    sh[1][threadIdx.x] = lq;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = sh[0][0];
        partial[2 * blockIdx.x + 1] = sh[1][0];
    }
}
__global__ __launch_bounds__(64) void kl_gaussian_finish_kernel(const double* __restrict__ partial, int blocks,
                                                                double* __restrict__ out) {
    if (threadIdx.x < 2) {
        double sum = 0.0;
        for (int b = 0; b < blocks; ++b) sum += partial[2 * b + threadIdx.x];
        out[threadIdx.x] = sum;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned stream_grid(unsigned long long items) {
    const unsigned long long blocks = (items + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

int lrt_check(const char* what, int dtype, int S, int M, int N, int K) {
    if (dtype != BF_DT_BF16) BF_FAIL("%s: dtype %d: needs BF_DT_BF16 (fp16 squares overflow above |x| = 256)", what, dtype);
    if (S < 1 || M < 1 || N < 1 || K < 1) BF_FAIL("%s: bad shape S=%d M=%d N=%d K=%d", what, S, M, N, K);
    if (N % 8) BF_FAIL("%s: N=%d: needs N %% 8 == 0", what, N);
    if (K % 8) BF_FAIL("%s: K=%d: needs K %% 8 == 0", what, K);
    if ((long long)S * M > 0x7fffffffLL - 64) BF_FAIL("%s: S*M=%lld rows: needs S*M < 2^31 - 64", what, (long long)S * M);
    return 0;
}

ZetaParams zeta_params(uint64_t seed, uint32_t sample_base, uint32_t layer_id) {
    ZetaParams z;
    z.k0 = (uint32_t)seed;
    z.k1 = (uint32_t)(seed >> 32);
    z.sample_base = sample_base;
    z.stream = BF_LRT_STREAM | layer_id;
    z.counter = bf_sample_counter();
    return z;
}

int grad_chunks(int R_pad) { return (R_pad + kChunkRows - 1) / kChunkRows; }

int kl_blocks(uint64_t n) {
    const uint64_t b = (n + 1023) / 1024;
    return (int)(b < 1 ? 1 : (b > (uint64_t)kKlBlocks ? (uint64_t)kKlBlocks : b));
}

}  // namespace

extern "C" {

int bf_lrt_operands(const float* d_mu, const float* d_rho, const float* d_mu_b, const float* d_rho_b, void* d_w2, float* d_b2,
                    int dtype, int N, int K, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (lrt_check("bf_lrt_operands", dtype, 1, 1, N, K)) return 1;
    if (!d_mu || !d_rho || !d_w2) BF_FAIL("bf_lrt_operands: NULL argument (mu, rho and the weight pair are required)");
    if ((d_mu_b != nullptr) != (d_rho_b != nullptr) || (d_mu_b != nullptr) != (d_b2 != nullptr))
        BF_FAIL("bf_lrt_operands: the bias mean, rho and pair go together");
    if (!aligned16(d_mu) || !aligned16(d_rho) || !aligned16(d_mu_b) || !aligned16(d_rho_b) || !aligned16(d_w2) || !aligned16(d_b2))
        BF_FAIL("bf_lrt_operands: every operand must be 16-byte aligned");
    const unsigned long long n = (unsigned long long)N * K;
    hipLaunchKernelGGL((lrt_operands_kernel<__bf16>), dim3(stream_grid(n / 8)), dim3(256), 0, stream, d_mu, d_rho,
                       reinterpret_cast<__bf16*>(d_w2), n / 8, n);
    BF_HIP_CHECK(hipGetLastError());
    if (d_b2) {
        hipLaunchKernelGGL((lrt_operands_kernel<float>), dim3(stream_grid(N / 8)), dim3(256), 0, stream, d_mu_b, d_rho_b, d_b2,
                           (unsigned long long)(N / 8), (unsigned long long)N);
        BF_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int bf_lrt_square(const void* d_x, void* d_xx, int dtype, int R, int R_pad, int K, int pair, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (lrt_check("bf_lrt_square", dtype, 1, R, 8, K)) return 1;
    if (R_pad < R || (long long)R_pad > (long long)R + 64) BF_FAIL("bf_lrt_square: R_pad=%d: needs R <= R_pad <= R + 64 (R=%d)", R_pad, R);
    if (!d_x || !d_xx) BF_FAIL("bf_lrt_square: NULL argument");
    if (!aligned16(d_x) || !aligned16(d_xx)) BF_FAIL("bf_lrt_square: every operand must be 16-byte aligned");
    const unsigned long long n8 = (unsigned long long)R * K / 8, pad8 = (unsigned long long)R_pad * K / 8;
    hipLaunchKernelGGL(lrt_square_kernel, dim3(stream_grid(pad8)), dim3(256), 0, stream, reinterpret_cast<const __bf16*>(d_x),
                       reinterpret_cast<__bf16*>(d_xx), n8, pad8, pad8 * 8, pair);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_lrt_combine(const float* d_m, const float* d_v, void* d_y, void* d_pre, void* d_sd, int dtype, int S, int M, int N,
                   int act, uint64_t seed, uint32_t sample_base, uint32_t layer_id, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (lrt_check("bf_lrt_combine", dtype, S, M, N, 8)) return 1;
    if (act != BF_ACT_NONE && act != BF_ACT_GELU) BF_FAIL("bf_lrt_combine: unknown activation %d", act);
    if (layer_id >= BF_LRT_STREAM) BF_FAIL("bf_lrt_combine: layer_id %u does not fit below the stream bit", layer_id);
    if (!d_m || !d_v || !d_y) BF_FAIL("bf_lrt_combine: NULL argument (m, v and y are required)");
    if (!aligned16(d_m) || !aligned16(d_v) || !aligned16(d_y) || !aligned16(d_pre) || !aligned16(d_sd))
        BF_FAIL("bf_lrt_combine: every operand must be 16-byte aligned");
    const unsigned long long total = (unsigned long long)S * M * (N / 8);
    hipLaunchKernelGGL(lrt_combine_kernel, dim3(stream_grid(total)), dim3(256), 0, stream, d_m, d_v,
                       reinterpret_cast<__bf16*>(d_y), reinterpret_cast<__bf16*>(d_pre), reinterpret_cast<__bf16*>(d_sd), total, M,
                       N, N / 8, act, zeta_params(seed, sample_base, layer_id));
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_lrt_zeta(float* d_out, int S, int M, int N, uint64_t seed, uint32_t sample_base, uint32_t layer_id, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (S < 1 || M < 1 || N < 1) BF_FAIL("bf_lrt_zeta: bad shape S=%d M=%d N=%d", S, M, N);
    if (layer_id >= BF_LRT_STREAM) BF_FAIL("bf_lrt_zeta: layer_id %u does not fit below the stream bit", layer_id);
    if (!d_out) BF_FAIL("bf_lrt_zeta: d_out is NULL");
    const unsigned long long mn = (unsigned long long)M * N, groups = (mn + 3) / 4, total = groups * S;
    hipLaunchKernelGGL(lrt_zeta_kernel, dim3(stream_grid(total)), dim3(256), 0, stream, d_out, total, groups, mn,
                       zeta_params(seed, sample_base, layer_id));
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

size_t bf_lrt_grad_prepare_workspace_bytes(int R_pad, int N) {
    if (R_pad < 1 || N < 1) return 0;
    return bf_align_up((size_t)2 * grad_chunks(R_pad) * N * sizeof(float), 256);
}

int bf_lrt_grad_prepare(const void* d_dy, const void* d_pre, const void* d_sd, void* d_dmdv, float* d_colsum, int dtype, int S,
                        int M, int R_pad, int N, int act, uint64_t seed, uint32_t sample_base, uint32_t layer_id,
                        void* d_workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (lrt_check("bf_lrt_grad_prepare", dtype, S, M, N, 8)) return 1;
    const int R = S * M;
    if (R_pad < R || (long long)R_pad > (long long)R + 64)
        BF_FAIL("bf_lrt_grad_prepare: R_pad=%d: needs S*M <= R_pad <= S*M + 64 (S*M=%d)", R_pad, R);
    if (act != BF_ACT_NONE && act != BF_ACT_GELU) BF_FAIL("bf_lrt_grad_prepare: unknown activation %d", act);
    if ((act != BF_ACT_NONE) != (d_pre != nullptr))
        BF_FAIL("bf_lrt_grad_prepare: the pre-activation goes with a fused activation, and only with one");
    if (layer_id >= BF_LRT_STREAM) BF_FAIL("bf_lrt_grad_prepare: layer_id %u does not fit below the stream bit", layer_id);
    if (!d_dy || !d_sd || !d_dmdv || !d_colsum) BF_FAIL("bf_lrt_grad_prepare: NULL argument (dy, sqrt(v), [dm; dv] and the sums are required)");
    if (!aligned16(d_dy) || !aligned16(d_pre) || !aligned16(d_sd) || !aligned16(d_dmdv) || !aligned16(d_colsum) ||
        !aligned16(d_workspace))
        BF_FAIL("bf_lrt_grad_prepare: every operand and the workspace must be 16-byte aligned");
    const size_t need = bf_lrt_grad_prepare_workspace_bytes(R_pad, N);
    if (!d_workspace || workspace_bytes < need)
        BF_FAIL("bf_lrt_grad_prepare: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    const int chunks = grad_chunks(R_pad);
    float* partial = reinterpret_cast<float*>(d_workspace);
    hipLaunchKernelGGL(lrt_grad_prepare_kernel, dim3((N / 8 + 63) / 64, chunks), dim3(256), 0, stream,
                       reinterpret_cast<const __bf16*>(d_dy), reinterpret_cast<const __bf16*>(d_pre),
                       reinterpret_cast<const __bf16*>(d_sd), reinterpret_cast<__bf16*>(d_dmdv), partial, R, R_pad, M, N, chunks,
                       zeta_params(seed, sample_base, layer_id));
    BF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lrt_colsum_finish_kernel, dim3((N + 255) / 256, 2), dim3(256), 0, stream, partial, d_colsum, N, chunks);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_lrt_dx(const void* d_ab, int64_t slab, const void* d_x, void* d_dx, int dtype, int R, int K, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (lrt_check("bf_lrt_dx", dtype, 1, R, 8, K)) return 1;
    if (slab < (int64_t)R * K || slab % 8) BF_FAIL("bf_lrt_dx: slab=%lld: needs slab >= R*K and slab %% 8 == 0", (long long)slab);
    if (!d_ab || !d_x || !d_dx) BF_FAIL("bf_lrt_dx: NULL argument");
    if (!aligned16(d_ab) || !aligned16(d_x) || !aligned16(d_dx)) BF_FAIL("bf_lrt_dx: every operand must be 16-byte aligned");
    const unsigned long long n8 = (unsigned long long)R * K / 8;
    hipLaunchKernelGGL(lrt_dx_kernel, dim3(stream_grid(n8)), dim3(256), 0, stream, reinterpret_cast<const __bf16*>(d_ab),
                       (unsigned long long)slab, reinterpret_cast<const __bf16*>(d_x), reinterpret_cast<__bf16*>(d_dx), n8);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_lrt_drho(const float* d_dsig2, const float* d_rho, float* d_drho, uint64_t n, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_dsig2 || !d_rho || !d_drho) BF_FAIL("bf_lrt_drho: NULL argument");
    if (n < 4 || n % 4) BF_FAIL("bf_lrt_drho: n=%llu: needs n %% 4 == 0", (unsigned long long)n);
    if (!aligned16(d_dsig2) || !aligned16(d_rho) || !aligned16(d_drho)) BF_FAIL("bf_lrt_drho: every operand must be 16-byte aligned");
    hipLaunchKernelGGL(lrt_drho_kernel, dim3(stream_grid(n / 4)), dim3(256), 0, stream, d_dsig2, d_rho, d_drho,
                       (unsigned long long)(n / 4));
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_sample_logprob_like(const bf_tensor_t* tensors, int n_tensors, int S, uint64_t seed, uint32_t sample_base,
                           double* d_logprob_out, void* d_workspace, size_t workspace_bytes, int like_dtype, void* stream) {
    if (!tensors) BF_FAIL("bf_sample_logprob_like: tensors is NULL");
    if (like_dtype < BF_DT_F32 || like_dtype > BF_DT_F16) BF_FAIL("bf_sample_logprob_like: bad like_dtype %d", like_dtype);
    for (int t = 0; t < n_tensors && t < 2; ++t)
        if (tensors[t].d_sample_out) BF_FAIL("bf_sample_logprob_like: tensor %d has an output (this entry writes no samples)", t);
    return bf_launch_sample_logprob(tensors, n_tensors, S, seed, sample_base, d_logprob_out, d_workspace, workspace_bytes,
                                    (hipStream_t)stream, like_dtype);
}

size_t bf_kl_gaussian_workspace_bytes(void) { return (size_t)kKlBlocks * 2 * sizeof(double); }

int bf_kl_gaussian(const float* d_mu, const float* d_rho, const float* d_prior_mu, const float* d_prior_rho, uint64_t n,
                   double* d_out, void* d_workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_mu || !d_rho || !d_prior_mu || !d_prior_rho || !d_out) BF_FAIL("bf_kl_gaussian: NULL argument");
    if (n < 1) BF_FAIL("bf_kl_gaussian: empty tensor");
    if (!d_workspace || workspace_bytes < bf_kl_gaussian_workspace_bytes() || ((uintptr_t)d_workspace & 7))
        BF_FAIL("bf_kl_gaussian: workspace too small or misaligned (%zu < %zu bytes)", workspace_bytes,
                bf_kl_gaussian_workspace_bytes());
    const int blocks = kl_blocks(n);
    double* partial = reinterpret_cast<double*>(d_workspace);
    hipLaunchKernelGGL(kl_gaussian_kernel, dim3(blocks), dim3(256), 0, stream, d_mu, d_rho, d_prior_mu, d_prior_rho,
                       (unsigned long long)n, partial);
    BF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kl_gaussian_finish_kernel, dim3(1), dim3(64), 0, stream, partial, blocks, d_out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
