// bf_lora.hip — the rank-r terms of a Bayesian low-rank adapter on a frozen base projection (include/bayeformers_amd_lora.h:
// bf_lora_fwd, bf_lora_bwd, bf_lora_reduce_da).  The base products x W0^T and dy W0 are the caller's; these kernels add
//   y[s]  += scale * (x[s] A_s^T) B^T                 and          dx[s] += scale * (dy[s] B) A_s
// in place and form dA_s = scale * g[s]^T x[s], dB = scale * sum_s dy[s]^T h[s].
//
// Kernels in this file
//   lora_mid_kernel<T>       : mid[s] = in[s] P_s^T, the [M, r] intermediate, rounded once and stored.  Forward: in = x,
//                              P = A_s [r][K], mid = h.  Backward: in = dy, P = B^T [r][N], mid = g.
//   lora_apply_kernel<T, QT> : out[s] += scale * mid[s] Q_s^T in place.  Forward: Q = B [N][r] (fp32 master, rounded in
//                              registers), out = y.  Backward: Q = A_s^T [K][r], out = dx.
//                              Both run k-contiguous operands straight from global memory (16 bytes per lane; P, Q and mid
//                              are small and shared by many workgroups: L2) through v_mfma_f32_16x16x32; every element of
//                              `in` and `out` is touched by exactly one lane.
//   lora_tn_kernel<T>        : part[b][chunk] = p[b]^T q[b] over a chunk of rows (the TN contractions of the backward), fp32
//   lora_reduce_kernel       : out = scale * sum_chunk part, in chunk order (optionally transposed: dB is [N][r])
//   lora_transpose_kernel    : [R][C] -> [C][R] with a cast to the compute dtype (B^T and A_s^T of the backward)
// No atomics anywhere: every output element is written by one thread and every sum has a fixed order.
#include "bf_common.h"

namespace {

template <typename T>
struct Mma;
template <>
struct Mma<__bf16> {
    using frag = bf16x8_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <>
struct Mma<_Float16> {
    using frag = f16x8_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

constexpr int kRows = 64;    // rows of `out` per workgroup of the apply kernel: 16 per wave
constexpr int kMaxRank = 64;

// 8 consecutive elements of an operand as an MFMA fragment: 16-bit as they are, fp32 rounded (to nearest even) here
template <typename T>
__device__ __forceinline__ typename Mma<T>::frag load_frag(const T* p) {
    return *reinterpret_cast<const typename Mma<T>::frag*>(p);
}
template <typename T>
__device__ __forceinline__ typename Mma<T>::frag load_frag(const float* p) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p), b = *reinterpret_cast<const f32x4_t*>(p + 4);
    return __builtin_convertvector((f32x8_t{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}), typename Mma<T>::frag);
}

// mid[s] = in[s] p_s^T, rounded once.  in [S][M][K]; p [r][K] per sample (p_ss elements between samples, 0 = shared); mid
// [S][M][r].  grid = (ceil(M / 16), S): a workgroup owns 16 rows; the k-steps of 32 are dealt to its four waves in turn and
// the waves' fp32 partial products meet in LDS, added in wave order.  A operand: row li of `in`, 8 consecutive k of group
// lg; B operand: row 16 j + li of p, the same k.  D: rows 4 lg + reg, column li of block j.
template <typename T>
__global__ __launch_bounds__(256) void lora_mid_kernel(const T* __restrict__ in, const T* __restrict__ p, long long p_ss,
                                                       T* __restrict__ mid, int M, int K, int r) {
    using frag = typename Mma<T>::frag;
    __shared__ float part[4][16][kMaxRank + 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int s = blockIdx.y, m0 = blockIdx.x * 16;
    const int nb = (r + 15) >> 4;  // 16-column blocks of the intermediate
    const frag zero = {};
    p += (size_t)s * p_ss;
    const int row = m0 + li;
    const bool row_ok = row < M;
    const T* in_row = in + ((size_t)s * M + (row_ok ? row : 0)) * K;
    f32x4_t acc[4] = {};
    // four of the wave's k-steps per round, every load issued before the first MFMA (steps past K multiply zeros)
    for (int kb = wave * 32; kb < K; kb += 512) {
        frag xf[4], pf[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = kb + u * 128 + lg * 8;
            const bool k_ok = k < K;  // (K % 8 == 0: a lane's 8 elements are inside or outside together)
            xf[u] = row_ok && k_ok ? load_frag<T>(in_row + k) : zero;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nb) pf[u][j] = j * 16 + li < r && k_ok ? load_frag<T>(p + (size_t)(j * 16 + li) * K + k) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nb) acc[j] = Mma<T>::run(xf[u], pf[u][j], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < nb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) part[wave][lg * 4 + i][j * 16 + li] = acc[j][i];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < 16 * r; idx += 256) {
        const int rr = idx / r, c = idx - rr * r;
        if (m0 + rr < M)
            mid[((size_t)s * M + m0 + rr) * r + c] = (T)(((part[0][rr][c] + part[1][rr][c]) + part[2][rr][c]) + part[3][rr][c]);
    }
}

// out[s] += scale * mid[s] q_s^T in place, the sum in fp32 before the one rounding.  mid [S][M][r]; q [N][r] per sample (q_ss
// elements between samples, 0 = shared; fp32 masters are rounded in registers); out [S][M][N].  grid = (ceil(M / 64), S,
// column ranges of cols_per_z columns, a multiple of 32); a wave owns 16 rows.  Transposed so that a lane ends up with 8
// consecutive columns of ONE row: A operand = rows of q, B operand = the wave's rows of mid (column li = row li).  Row i of
// the A operand of block bq stands for column n0 + (i >> 2) * 8 + bq * 4 + (i & 3); D row 4 lg + reg of block bq is then
// column n0 + lg * 8 + bq * 4 + reg: blocks 0 and 1 give the lane columns n0 + lg * 8 + 0..7, 16 bytes of `out`.
template <typename T, typename QT>
__global__ __launch_bounds__(256) void lora_apply_kernel(const T* __restrict__ mid, const QT* __restrict__ q, long long q_ss,
                                                         T* __restrict__ out, float scale, int M, int N, int r,
                                                         int cols_per_z) {
    using frag = typename Mma<T>::frag;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int s = blockIdx.y;
    const int row = blockIdx.x * kRows + wave * 16 + li;
    const bool row_ok = row < M;
    const frag zero = {};
    q += (size_t)s * q_ss;
    frag hf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int kk = ks * 32 + lg * 8;
        hf[ks] = row_ok && kk < r ? load_frag<T>(mid + ((size_t)s * M + row) * r + kk) : zero;
    }
    const int nks = (r + 31) >> 5;
    const int col_lo = blockIdx.z * cols_per_z;
    const int col_hi = min(N, col_lo + cols_per_z);
    T* out_row = out + ((size_t)s * M + (row_ok ? row : 0)) * N;
    // two steps of 32 columns per round, every load issued before the first MFMA
    for (int nb0 = col_lo; nb0 < col_hi; nb0 += 64) {
        frag v[2], q0[2][2], q1[2][2];
        bool store[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int n0 = nb0 + u * 32;
            const int na = n0 + (li >> 2) * 8 + (li & 3);
            store[u] = row_ok && n0 + lg * 8 < col_hi;
            v[u] = store[u] ? *reinterpret_cast<const frag*>(out_row + n0 + lg * 8) : zero;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks < nks) {
                    const int kk = ks * 32 + lg * 8;
                    const bool ok = kk < r && na < col_hi;  // (col_hi % 8 == 0: na and na + 4 are inside or outside together)
                    q0[u][ks] = ok ? load_frag<T>(q + (size_t)na * r + kk) : zero;
                    q1[u][ks] = ok ? load_frag<T>(q + (size_t)(na + 4) * r + kk) : zero;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x4_t c0 = {}, c1 = {};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks < nks) {
                    c0 = Mma<T>::run(q0[u][ks], hf[ks], c0);
                    c1 = Mma<T>::run(q1[u][ks], hf[ks], c1);
                }
            }
            if (store[u]) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[u][i] = (T)fmaf(scale, c0[i], (float)v[u][i]);
                    v[u][4 + i] = (T)fmaf(scale, c1[i], (float)v[u][4 + i]);
                }
                *reinterpret_cast<frag*>(out_row + nb0 + u * 32 + lg * 8) = v[u];
            }
        }
    }
}

// part[b][chunk][j][c] = sum over the chunk's rows m of p[b][m][j] * q[b][m][c].  p [batch][rows][r], q [batch][rows][C].
// grid = (ceil(C / 64), chunks, batch); a wave owns 16 columns c.  Both operands are contraction-strided: a lane gathers
// its 8 rows element by element (the 16 lanes of a group read 32 consecutive bytes of a row).
template <typename T>
__global__ __launch_bounds__(256) void lora_tn_kernel(const T* __restrict__ p, const T* __restrict__ q,
                                                      float* __restrict__ part, int rows, int r, int C, int rows_per_chunk) {
    using frag = typename Mma<T>::frag;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int b = blockIdx.z, chunk = blockIdx.y;
    const int c = blockIdx.x * 64 + wave * 16 + li;
    const bool c_ok = c < C;
    const int nb = (r + 15) >> 4;
    p += (size_t)b * rows * r;
    q += (size_t)b * rows * C;
    const int m_lo = chunk * rows_per_chunk, m_hi = min(rows, m_lo + rows_per_chunk);
    f32x4_t acc[4] = {};
    for (int m0 = m_lo; m0 < m_hi; m0 += 32) {
        frag qf = {}, pf[4] = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + lg * 8 + i;
            if (m < m_hi) {
                if (c_ok) qf[i] = q[(size_t)m * C + c];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nb && j * 16 + li < r) pf[j][i] = p[(size_t)m * r + j * 16 + li];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nb) acc[j] = Mma<T>::run(pf[j], qf, acc[j]);
    }
    // D: row 16 j + 4 lg + reg of the [r][C] product, column c
    float* o = part + ((size_t)b * gridDim.y + chunk) * r * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = j * 16 + lg * 4 + i;
            if (j < nb && n < r && c_ok) o[(size_t)n * C + c] = acc[j][i];
        }
    }
}

// out[b][j][c] (or out[b][c][j]) = scale * (part[b][0][j][c] + part[b][1][j][c] + ...), the chunks in order
__global__ __launch_bounds__(256) void lora_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                          unsigned long long total, int chunks, int r, int C, float scale,
                                                          int transpose) {
    const unsigned long long idx = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const unsigned long long n = (unsigned long long)r * C, b = idx / n, e = idx - b * n;
    const float* src = part + b * chunks * n + e;
    float sum = src[0];
    for (int ch = 1; ch < chunks; ++ch) sum += src[(size_t)ch * n];
    const int j = (int)(e / C), c = (int)(e - (unsigned long long)j * C);
    out[transpose ? b * n + (size_t)c * r + j : idx] = scale * sum;
}

// out[b][c][rr] = (T) in[b][rr][c]
template <typename TI, typename T>
__global__ __launch_bounds__(256) void lora_transpose_kernel(const TI* __restrict__ in, T* __restrict__ out,
                                                             unsigned long long total, int R, int C) {
    const unsigned long long idx = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const unsigned long long n = (unsigned long long)R * C, b = idx / n, e = idx - b * n;
    const int c = (int)(e / R), rr = (int)(e - (unsigned long long)c * R);
    out[idx] = (T)in[b * n + (size_t)rr * C + c];
}

// What both entries refuse; `what` names the entry.
int lora_check(const char* what, int dtype, int S, int M, int N, int K, int r) {
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) BF_FAIL("%s: dtype %d: needs BF_DT_BF16 or BF_DT_F16 (16-bit compute)", what, dtype);
    if (S < 1 || M < 1 || N < 1 || K < 1) BF_FAIL("%s: bad shape S=%d M=%d N=%d K=%d", what, S, M, N, K);
    if (S > 65535) BF_FAIL("%s: S=%d: needs S <= 65535", what, S);
    if (K % 8) BF_FAIL("%s: K=%d: needs K %% 8 == 0", what, K);
    if (N % 8) BF_FAIL("%s: N=%d: needs N %% 8 == 0", what, N);
    if (r % 8) BF_FAIL("%s: r=%d: needs r %% 8 == 0", what, r);
    if (r < 8 || r > kMaxRank) BF_FAIL("%s: r=%d: needs 8 <= r <= %d", what, r, kMaxRank);
    if ((long long)S * M > 0x7fffffffLL) BF_FAIL("%s: S*M=%lld rows: needs S*M < 2^31", what, (long long)S * M);
    return 0;
}

bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

// Column ranges of the apply kernel: the columns of `out` are cut into ranges of at least 128 (a multiple of 32) until about
// four workgroups per CU exist — a decode step has one row tile per sample.
void apply_grid(int S, int M, int N, int* nz, int* cols_per_z) {
    const long long wg = (long long)S * ((M + kRows - 1) / kRows);
    long long z = (1024 + wg - 1) / wg;
    const long long z_max = (N + 127) / 128;
    z = z < 1 ? 1 : (z > z_max ? z_max : z);
    const int cols = (int)(((N + z - 1) / z + 31) / 32 * 32);
    *cols_per_z = cols;
    *nz = (N + cols - 1) / cols;
}

// mid = in p^T, then (out given) out += scale * mid q^T: two launches
template <typename T, typename QT>
int launch_pass(const void* in, const void* p, long long p_ss, const QT* q, long long q_ss, void* out, void* mid, float scale,
                int S, int M, int N, int K, int r, hipStream_t stream) {
    hipLaunchKernelGGL((lora_mid_kernel<T>), dim3((M + 15) / 16, S), dim3(256), 0, stream, reinterpret_cast<const T*>(in),
                       reinterpret_cast<const T*>(p), p_ss, reinterpret_cast<T*>(mid), M, K, r);
    BF_HIP_CHECK(hipGetLastError());
    if (!out) return 0;
    int nz = 1, cols = N;
    apply_grid(S, M, N, &nz, &cols);
    hipLaunchKernelGGL((lora_apply_kernel<T, QT>), dim3((M + kRows - 1) / kRows, S, nz), dim3(256), 0, stream,
                       reinterpret_cast<const T*>(mid), q, q_ss, reinterpret_cast<T*>(out), scale, M, N, r, cols);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// Row chunks of a TN contraction: at least 64 rows each, at most 256 chunks, until about two workgroups per CU exist.
void tn_chunks(int batch, int rows, int C, int* chunks, int* rows_per_chunk) {
    const long long wg = (long long)batch * ((C + 63) / 64);
    long long ch = (512 + wg - 1) / wg;
    long long ch_max = (rows + 63) / 64;
    if (ch_max > 256) ch_max = 256;
    ch = ch < 1 ? 1 : (ch > ch_max ? ch_max : ch);
    const int per = (int)(((rows + ch - 1) / ch + 31) / 32 * 32);
    *rows_per_chunk = per;
    *chunks = (rows + per - 1) / per;
}

struct BwdLayout {
    size_t bt, at, g, part_a, part_b, total;
    int chunks_a, per_a, chunks_b, per_b;
};

BwdLayout bwd_layout(int S, int M, int N, int K, int r, int dtype) {
    const size_t es = bf_dtype_size(dtype);
    BwdLayout L;
    tn_chunks(S, M, K, &L.chunks_a, &L.per_a);
    tn_chunks(1, S * M, N, &L.chunks_b, &L.per_b);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += bf_align_up(bytes, 256);
        return o;
    };
    L.bt = take((size_t)r * N * es);
    L.at = take((size_t)S * K * r * es);
    L.g = take((size_t)S * M * r * es);
    L.part_a = take((size_t)S * L.chunks_a * r * K * sizeof(float));
    L.part_b = take((size_t)L.chunks_b * r * N * sizeof(float));
    L.total = off;
    return L;
}

template <typename T>
int launch_tn(const void* p, const void* q, float* part, float* out, int batch, int rows, int r, int C, int chunks, int per,
              float scale, int transpose, hipStream_t stream) {
    hipLaunchKernelGGL((lora_tn_kernel<T>), dim3((C + 63) / 64, chunks, batch), dim3(256), 0, stream,
                       reinterpret_cast<const T*>(p), reinterpret_cast<const T*>(q), part, rows, r, C, per);
    BF_HIP_CHECK(hipGetLastError());
    const unsigned long long total = (unsigned long long)batch * r * C;
    hipLaunchKernelGGL(lora_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, part, out, total, chunks,
                       r, C, scale, transpose);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int bwd_typed(const void* d_x, const void* d_dy, const void* d_a_s, const float* d_b, const void* d_h, void* d_dx,
              float* d_da, float* d_db, float scale, int S, int M, int N, int K, int r, const BwdLayout& L, char* ws,
              hipStream_t stream) {
    int rc;
    T* bt = reinterpret_cast<T*>(ws + L.bt);
    T* at = reinterpret_cast<T*>(ws + L.at);
    // B^T [r][N] in the compute dtype (the rounding of the forward), and A_s^T [S][K][r] when dx is wanted
    unsigned long long total = (unsigned long long)N * r;
    hipLaunchKernelGGL((lora_transpose_kernel<float, T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, d_b, bt,
                       total, N, r);
    BF_HIP_CHECK(hipGetLastError());
    if (d_dx) {
        total = (unsigned long long)S * r * K;
        hipLaunchKernelGGL((lora_transpose_kernel<T, T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                           reinterpret_cast<const T*>(d_a_s), at, total, r, K);
        BF_HIP_CHECK(hipGetLastError());
    }
    // g = dy B (stored: dA reads it), dx += scale * g A_s
    if ((rc = launch_pass<T, T>(d_dy, bt, 0, at, (long long)K * r, d_dx, ws + L.g, scale, S, M, K, N, r, stream))) return rc;
    // dA_s = scale * g[s]^T x[s]
    if ((rc = launch_tn<T>(ws + L.g, d_x, reinterpret_cast<float*>(ws + L.part_a), d_da, S, M, r, K, L.chunks_a, L.per_a, scale, 0,
                           stream)))
        return rc;
    // dB = scale * (sum_s h[s]^T dy[s])^T
    if (d_db && (rc = launch_tn<T>(d_h, d_dy, reinterpret_cast<float*>(ws + L.part_b), d_db, 1, S * M, r, N, L.chunks_b, L.per_b,
                                   scale, 1, stream)))
        return rc;
    return 0;
}

}  // namespace

extern "C" {

size_t bf_lora_fwd_workspace_bytes(int, int, int, int, int, int) { return 0; }

int bf_lora_fwd(const void* d_x, const void* d_a_s, const float* d_b, void* d_y, void* d_h, float scale, int dtype, int S,
                int M, int N, int K, int r, void* /*d_workspace*/, size_t /*workspace_bytes*/, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (lora_check("bf_lora_fwd", dtype, S, M, N, K, r)) return 1;
    if (!d_x || !d_a_s || !d_b || !d_h) BF_FAIL("bf_lora_fwd: NULL argument (x, A_s, B and h are required)");
    if (!aligned16(d_x) || !aligned16(d_a_s) || !aligned16(d_b) || !aligned16(d_y) || !aligned16(d_h))
        BF_FAIL("bf_lora_fwd: every operand must be 16-byte aligned");
    if (dtype == BF_DT_BF16)
        return launch_pass<__bf16, float>(d_x, d_a_s, (long long)r * K, d_b, 0, d_y, d_h, scale, S, M, N, K, r, stream);
    return launch_pass<_Float16, float>(d_x, d_a_s, (long long)r * K, d_b, 0, d_y, d_h, scale, S, M, N, K, r, stream);
}

size_t bf_lora_bwd_workspace_bytes(int S, int M, int N, int K, int r, int dtype) {
    if (S < 1 || M < 1 || N < 1 || K < 1 || r < 1 || (long long)S * M > 0x7fffffffLL) return 0;
    return bwd_layout(S, M, N, K, r, dtype).total;
}

int bf_lora_bwd(const void* d_x, const void* d_dy, const void* d_a_s, const float* d_b, const void* d_h, void* d_dx,
                float* d_da, float* d_db, float scale, int dtype, int S, int M, int N, int K, int r, void* d_workspace,
                size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (lora_check("bf_lora_bwd", dtype, S, M, N, K, r)) return 1;
    if (!d_x || !d_dy || !d_a_s || !d_b || !d_da) BF_FAIL("bf_lora_bwd: NULL argument (x, dy, A_s, B and dA are required)");
    if (d_db && !d_h) BF_FAIL("bf_lora_bwd: dB needs the forward's h");
    if (!aligned16(d_x) || !aligned16(d_dy) || !aligned16(d_a_s) || !aligned16(d_b) || !aligned16(d_h) || !aligned16(d_dx) ||
        !aligned16(d_da) || !aligned16(d_db) || !aligned16(d_workspace))
        BF_FAIL("bf_lora_bwd: every operand and the workspace must be 16-byte aligned");
    const BwdLayout L = bwd_layout(S, M, N, K, r, dtype);
    if (!d_workspace || workspace_bytes < L.total)
        BF_FAIL("bf_lora_bwd: workspace too small (%zu < %zu bytes)", workspace_bytes, L.total);
    char* ws = reinterpret_cast<char*>(d_workspace);
    if (dtype == BF_DT_BF16)
        return bwd_typed<__bf16>(d_x, d_dy, d_a_s, d_b, d_h, d_dx, d_da, d_db, scale, S, M, N, K, r, L, ws, stream);
    return bwd_typed<_Float16>(d_x, d_dy, d_a_s, d_b, d_h, d_dx, d_da, d_db, scale, S, M, N, K, r, L, ws, stream);
}

int bf_lora_reduce_da(const float* d_da, const float* d_rho, uint64_t n, int S, uint64_t seed, uint32_t sample_base,
                      uint32_t stream_id, float* d_dmu, float* d_drho, void* stream) {
    if (!d_da || !d_rho || !d_drho) BF_FAIL("bf_lora_reduce_da: NULL argument (dA, rho and drho are required)");
    return bf_launch_param_grad(d_da, d_rho, n, S, 1, seed, sample_base, stream_id, d_dmu, d_drho, (hipStream_t)stream);
}

}  // extern "C"
