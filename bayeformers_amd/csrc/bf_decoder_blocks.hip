// bf_decoder_blocks.hip — the memory-bound ops of a decoder layer that sit between the Bayesian linear layers and the
// attention kernels, one kernel set for the Llama / Mistral / Qwen2 layer and for Gemma 1 / 2 / 3 and Qwen3:
//   * (norm ->) residual add -> RMSNorm in one pass, gamma or Gemma's (1 + gamma): bf_add_rmsnorm is bf_norm_add_rmsnorm
//     without the first norm and without an offset;
//   * (per-head RMSNorm of q and k ->) rotary position embedding at head size 64, 128 or 256: bf_rope_qk is bf_qknorm_rope
//     without gammas, held to 64 and 128;
//   * gate(g) * up with the gate SiLU (bf_swiglu) or tanh-GELU (bf_geglu);
// and the backward of each.  Not reference functions: they are the wrapped model's own ops around
// /root/reference/bayeformers/nn/layers/linear.py:83-104's forward (HF's *RMSNorm.forward, apply_rotary_pos_emb, the MLP's
// act_fn(gate) * up), each of which the framework runs as a chain of elementwise kernels with a full pass over the
// activations per link.
//
// HBM-bound streaming kernels in the manner of bf_norm.hip: 16-byte loads and stores (bf_vec8.h), fp32 arithmetic in
// registers, one rounding into the output dtype unless a comment names another.  No allocation, no host synchronisation
// (capturable), no trigonometry: cos and sin are the tables the model's rotary module returns.  No float atomics: every
// parameter gradient leaves a workgroup as one fp32 row of partial sums, and dgamma_rows_kernel adds the rows in a fixed order.
#include "bf_common.h"
#include "bf_device.h"
#include "bf_vec8.h"

namespace {

constexpr int kRowsPerBlock = 4;      // waves per workgroup of the forward norm
constexpr int kBwdBlocks = 1024;      // workgroups at most of a backward kernel that leaves a row of partial sums
constexpr int kBwdBlocksWide = 512;   // ... of the one-row-per-workgroup form of the norm (N > 2048)
constexpr unsigned kRopeBlocks = 4096;  // workgroups at most of a rotation without a reduction

// The weight offset of an entry that has none.  (woff + gamma) is what every norm multiplies by; -0.0f is the additive
// identity that also keeps a gamma of -0.0f (+0.0f would turn it into +0.0f and flip the sign of a zero output), so
// bf_add_rmsnorm[_bwd] multiply by gamma itself, bit for bit.  weight_offset = 0 of the family entries stays +0.0f.
constexpr float kNoOffset = -0.0f;

// 8 floats rounded once to T (what the output tensor holds) and read back: the values the next op of the unfused model sees
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

// the sum over the G lanes that own a row, as far as a wave reaches (G = 256: the four waves meet in LDS)
template <int G>
__device__ __forceinline__ double group_sum_f64(double v) {
#pragma unroll
    for (int m = (G < 64 ? G : 64) / 2; m; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <int G>
__device__ __forceinline__ float group_sum(float v, int lane) {
    if constexpr (G == 32) return half_sum(v, lane);
    else return wave_sum(v);
}

bool strides_ok(const int64_t* s) { return s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && !((s[0] | s[1] | s[2]) & 7); }

bool dtype_ok(int dtype) { return dtype == BF_DT_BF16 || dtype == BF_DT_F16 || dtype == BF_DT_F32; }

// out[n] = sum over the workgroups' partial rows [nblocks, W]; columns [0, N) go to out0, [N, W) to out1 (W = N or 2 N; a
// NULL output is skipped).  16 columns x 64 lanes over the workgroup axis per block (layernorm_param_grad_kernel's shape);
// fixed order.
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

// ---- (norm ->) residual add -> norm --------------------------------------------------------------------------------------
// u = PRE ? round_T(x * rstd(x) * (woff + gamma_pre)) : x,  z = res ? round_T(res + u) : u (bitwise torch's `residual + u`),
// y = round_T(z * rstd(z) * (woff + gamma_out)),  rstd(v) = rsqrt(mean(v^2) + eps), the statistics taken from the rounded z.
// G lanes own a row and V 8-element vectors each (N / 8 <= G * V): G = 64, one wave per row, or G = 32, half a wave per row
// and two rows per wave for N = 256 V (add_layernorm_half_kernel's layout, every lane busy).  The row is loaded once and
// stays in registers between the load and the stores; every lane reads its elements of x and the residual before it writes
// anything, and writes only where it read, which makes sum_out == res and out == x safe.  Algorithmic bytes per row:
// N * (2 reads + 2 writes) * sizeof(T) with a residual and a sum output.
template <typename T, typename GT, int G, int V, bool PRE>
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
    const T* xr = x + row * N;
    const T* rr = res ? res + row * N : nullptr;
    float v[V][8];
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const int vi = gl + G * c;
        if (vi < nvec) load8(xr + vi * 8, v[c]);
    }
    if constexpr (PRE) {
        // The first norm runs in fp64.  u is rounded to T and then feeds an add that is rounded again, so an fp32
        // evaluation error here (a few 2^-24) would carry about one u in 2^13 across a rounding boundary of a 16-bit T —
        // a whole spacing of u, where the framework's fp32 chain and a float64 restatement agree on the other side; in
        // fp64, rounded once (round_f64), u is the restatement's.  Some 6 fp64-rate instructions per element against 8
        // bytes of traffic.  A compile-time branch: the form without a first norm does not carry its registers.
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
    float sq = 0.f;
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
            if (sum_out && live) store8(sum_out + row * N + vi * 8, v[c]);
#pragma unroll
            for (int i = 0; i < 8; ++i) sq = fmaf(v[c][i], v[c][i], sq);
        }
    }
    const float rstd = 1.0f / sqrtf(group_sum<G>(sq, lane) * (1.0f / (float)N) + eps_out);
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

struct norm_args_t {
    const void *x, *gpre, *res, *gout;
    void *sum_out, *out;
    long long rows;
    int N;
    float woff, eps_pre, eps_out;
};

template <typename T, typename GT, bool PRE>
int launch_norm(const norm_args_t& a, hipStream_t stream) {
    const int nvec = a.N >> 3;
    const dim3 block(64 * kRowsPerBlock);
#define BF_NORM_LAUNCH(G_, V_)                                                                                                \
    hipLaunchKernelGGL((norm_add_rmsnorm_kernel<T, GT, G_, V_, PRE>), grid, block, 0, stream, (const T*)a.x, (const GT*)a.gpre, \
                       (const T*)a.res, (const GT*)a.gout, (T*)a.sum_out, (T*)a.out, a.rows, a.N, a.woff, a.eps_pre, a.eps_out)
    if (nvec % 32 == 0 && nvec <= 128) {
        const dim3 grid((unsigned)((a.rows + 2 * kRowsPerBlock - 1) / (2 * kRowsPerBlock)));
        switch (nvec / 32) {
            case 1: BF_NORM_LAUNCH(32, 1); break;
            case 2: BF_NORM_LAUNCH(32, 2); break;
            case 3: BF_NORM_LAUNCH(32, 3); break;
            default: BF_NORM_LAUNCH(32, 4); break;
        }
    } else {
        const dim3 grid((unsigned)((a.rows + kRowsPerBlock - 1) / kRowsPerBlock));
        if (nvec <= 64) BF_NORM_LAUNCH(64, 1);
        else if (nvec <= 128) BF_NORM_LAUNCH(64, 2);
        else if (nvec <= 256) BF_NORM_LAUNCH(64, 4);
        else if (nvec <= 512) BF_NORM_LAUNCH(64, 8);
        else BF_NORM_LAUNCH(64, 16);
    }
#undef BF_NORM_LAUNCH
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// The types a call names at run time, once for every op.  The macro reads the enclosing function's variables `dtype`
// (activations) and `param_dtype` (gammas) and RETURNS from that function with the result of LAUNCH<T, GT, FLAG>(args...),
// a function template over the two types and one compile-time switch: it is the last statement of an entry body.
#define BF_BY_TYPES(LAUNCH, FLAG, ...)                                                                           \
    do {                                                                                                         \
        const bool f32_ = param_dtype == BF_DT_F32;                                                              \
        switch (dtype) {                                                                                         \
            case BF_DT_BF16:                                                                                     \
                if (FLAG) return f32_ ? LAUNCH<__bf16, float, true>(__VA_ARGS__) : LAUNCH<__bf16, __bf16, true>(__VA_ARGS__);       \
                return f32_ ? LAUNCH<__bf16, float, false>(__VA_ARGS__) : LAUNCH<__bf16, __bf16, false>(__VA_ARGS__);               \
            case BF_DT_F16:                                                                                      \
                if (FLAG) return f32_ ? LAUNCH<_Float16, float, true>(__VA_ARGS__) : LAUNCH<_Float16, _Float16, true>(__VA_ARGS__); \
                return f32_ ? LAUNCH<_Float16, float, false>(__VA_ARGS__) : LAUNCH<_Float16, _Float16, false>(__VA_ARGS__);         \
            default:                                                                                             \
                return FLAG ? LAUNCH<float, float, true>(__VA_ARGS__) : LAUNCH<float, float, false>(__VA_ARGS__); \
        }                                                                                                        \
    } while (0)

// bf_add_rmsnorm and bf_norm_add_rmsnorm: one set of checks, `who` names the entry in the messages.  family: the entry has a
// weight offset (and speaks of "the gammas"); the other multiplies by gamma itself.
int norm_entry(const char* who, bool family, const void* d_x, const void* d_gamma_pre, const void* d_residual,
               const void* d_gamma_out, int param_dtype, int weight_offset, void* d_sum_out, void* d_out, int dtype,
               int64_t rows, int N, float eps_pre, float eps_out, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("%s: bad shape rows=%lld N=%d", who, (long long)rows, N);
    if (N % 8 || N > 8192) BF_FAIL("%s: N=%d must be a multiple of 8 and at most 8192", who, N);
    if (!d_x || !d_gamma_out || !d_out) BF_FAIL("%s: null pointer", who);
    if (rows > 0x7fffffffLL * kRowsPerBlock) BF_FAIL("%s: too many rows", who);
    const uintptr_t al = (uintptr_t)d_x | (uintptr_t)d_gamma_pre | (uintptr_t)d_residual | (uintptr_t)d_gamma_out |
                         (uintptr_t)d_sum_out | (uintptr_t)d_out;
    if (al & 15) BF_FAIL("%s: pointers must be 16-byte aligned", who);
    if (family && weight_offset != 0 && weight_offset != 1) BF_FAIL("%s: weight_offset=%d must be 0 or 1", who, weight_offset);
    if (!dtype_ok(dtype)) BF_FAIL("%s: unknown dtype %d", who, dtype);
    if (param_dtype != BF_DT_F32 && param_dtype != dtype)
        BF_FAIL("%s: %s must be fp32 or have the activation dtype", who, family ? "the gammas" : "gamma");
    if (rows == 0) return 0;
    const norm_args_t a = {d_x,  d_gamma_pre, d_residual, d_gamma_out, d_sum_out, d_out, rows, N,
                           family ? (float)weight_offset : kNoOffset, eps_pre, eps_out};
    BF_BY_TYPES(launch_norm, d_gamma_pre != nullptr, a, (hipStream_t)stream);
}

// ---- the backward of (norm ->) residual add -> norm ---------------------------------------------------------------------------
// Stage 2, the norm behind the add, from the stored z (the forward's sum output), with r_z = rsqrt(mean(z^2) + eps_out)
// recomputed from it and a = (woff + gamma_out) o dy:
//     dz = r_z a - z r_z^3 mean(z o a) + dz_in,      dgamma_out = sum_rows dy o z r_z
// (dy == NULL, only the sum was consumed: dz = dz_in, dgamma_out = 0).  dz is the gradient of the residual.
// Stage 1 (PRE), the norm in front of the add, with dz taken unrounded from the registers, b = (woff + gamma_pre) o dz:
//     dx = r_x b - x r_x^3 mean(x o b),              dgamma_pre = sum_rows dz o x r_x.
// Both row sums of a stage (z^2 and z o a) come out of the one pass that loads the row, so a stage costs one reduction step.
// G lanes own a row, V 8-element vectors per lane: the forward's layouts (G = 32: half a wave per row for N = 256 .. 1024 in
// steps of 256, G = 64: a wave per row up to N = 2048) and, beyond them, the whole workgroup on one row (G = 256, N <= 8192:
// a wave would need 4 x 128 registers for z, dy, gamma and the dgamma sums of such a row).  A workgroup walks rows blockIdx,
// + gridDim, ...; every lane keeps the dgamma partial sums of its own columns in registers, the workgroup's 256 / G rows
// are combined through LDS in a fixed order and leave one [W] fp32 row per workgroup, W = N or (PRE) 2 N with dgamma_pre in
// the second half, summed by dgamma_rows_kernel: deterministic.
// The sums of squares are taken in fp64 (exact products), and so is each dgamma term dy z r before it is added to the fp32
// partial sum: a term costs one fp32 rounding, the sum's, so dgamma meets the order-independent bound rows 2^-24 sum |dy z r|
// down to a single row, where three fp32 roundings (r, z r, the product) would not.  The price is about 7 fp64-rate
// instructions per element against 6 .. 8 bytes of traffic; the achieved bytes/s are in profiles/decoder_blocks_train.md.
// Registers: the row (z, dy and, PRE, x) and the dgamma partials.  Without PRE a fourth set holds (woff + gamma_out) across
// the rows, which measured faster than reading gamma again for every row at every shape (profiles/decoder_blocks_unified.md);
// PRE has five sets already and reads the gammas per row (from L2: [N] values that every workgroup reads).  Every lane
// reads all it needs of a row before it writes, and writes only where it read: dz may be dy or dz_in, dx may be dz.
// Algorithmic bytes per row: N * (2 reads + 1 write) * sizeof(T), + 1 read with dz_in, + 1 read and 1 write with gamma_pre.
template <typename T, typename GT, int G, int V, bool PRE>
__global__ __launch_bounds__(256) void norm_add_rmsnorm_bwd_kernel(const T* x, const T* z, const GT* __restrict__ gamma_pre,
                                                                   const GT* __restrict__ gamma_out, const T* dy,
                                                                   const T* dz_in, T* dz, T* dx, float* __restrict__ partial,
                                                                   long long rows, int N, float woff, float eps_pre,
                                                                   float eps_out) {
    constexpr int kGroups = 256 / G;  // rows in flight per workgroup
    constexpr bool kHeld = !PRE;      // (woff + gamma_out) lives in registers
    extern __shared__ float sh[];     // [W] (kGroups > 1)
    __shared__ double red_sq[2][4];
    __shared__ float red_s[2][4];
    const int lane = threadIdx.x & 63, gl = threadIdx.x % G, sub = threadIdx.x / G;
    const int nvec = N >> 3;
    const int W = PRE ? 2 * N : N;
    float dgo[V][8], dgp[PRE ? V : 1][8], held[kHeld ? V : 1][8];
#pragma unroll
    for (int c = 0; c < V; ++c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            dgo[c][i] = 0.f;
            if constexpr (PRE) dgp[c][i] = 0.f;
            if constexpr (kHeld) held[c][i] = 0.f;
        }
        if constexpr (kHeld) {
            if (gl + G * c < nvec) {
                load8(gamma_out + (gl + G * c) * 8, held[c]);
#pragma unroll
                for (int i = 0; i < 8; ++i) held[c][i] = woff + held[c][i];
            }
        }
    }
    // (woff + gamma_out) of vector c: the held registers, or read again
    auto gamma_of = [&](int c, float (&gm)[8]) {
        if constexpr (kHeld) {
#pragma unroll
            for (int i = 0; i < 8; ++i) gm[i] = held[c][i];
        } else {
            load8(gamma_out + (gl + G * c) * 8, gm);
#pragma unroll
            for (int i = 0; i < 8; ++i) gm[i] = woff + gm[i];
        }
    };
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
                // Without a first norm there is no branch on dy in here, so that a row's loads are all in flight together
                // (the Llama kernel's form): without dy the row of z is read in its place and what comes of it is dropped
                // below.  With a first norm the registers that would take are not there.
                if (!PRE || dy) {
                    float gm[8];
                    load8((dy ? dy : z) + row * N + vi * 8, g[c]);
                    gamma_of(c, gm);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        sq = fma((double)v[c][i], (double)v[c][i], sq);
                        s = fmaf(g[c][i] * gm[i], v[c][i], s);
                    }
                }
            }
        }
        double rd = 0.0;
        float r = 0.f, k = 0.f;
        if (dy) {
            sq = group_sum_f64<G>(sq);
            s = group_sum<G>(s, lane);
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
                    gamma_of(c, gm);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        // dy z is exact in fp64, r unrounded: the one rounding of a step is the sum's, back to fp32
                        if (live) dgo[c][i] = (float)fma((double)g[c][i] * (double)v[c][i], rd, (double)dgo[c][i]);
                        g[c][i] = fmaf(-v[c][i], k, r * (g[c][i] * gm[i]));
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
                } else if (live) {
                    store8(dz + row * N + vi * 8, g[c]);  // (no stage 1: dz leaves as soon as it is formed)
                }
            }
        }
        if constexpr (PRE) {
            sqx = group_sum_f64<G>(sqx);
            sx = group_sum<G>(sx, lane);
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

size_t norm_bwd_workspace_bytes(int64_t rows, int N, bool pre) {
    if (rows < 1 || N < 1) return 0;
    int G, nb;
    norm_bwd_layout(rows, N, &G, &nb);
    return (size_t)nb * N * (pre ? 2 : 1) * sizeof(float);
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
#define BF_NORMB_LAUNCH(G_, V_)                                                                                              \
    hipLaunchKernelGGL((norm_add_rmsnorm_bwd_kernel<T, GT, G_, V_, PRE>), grid, block, lds, stream, (const T*)a.x,            \
                       (const T*)a.z, (const GT*)a.gpre, (const GT*)a.gout, (const T*)a.dy, (const T*)a.dz_in, (T*)a.dz,      \
                       (T*)a.dx, a.partial, a.rows, a.N, a.woff, a.eps_pre, a.eps_out)
    if (G == 32) {
        switch (nvec / 32) {
            case 1: BF_NORMB_LAUNCH(32, 1); break;
            case 2: BF_NORMB_LAUNCH(32, 2); break;
            case 3: BF_NORMB_LAUNCH(32, 3); break;
            default: BF_NORMB_LAUNCH(32, 4); break;
        }
    } else if (G == 64) {
        if (nvec <= 64) BF_NORMB_LAUNCH(64, 1);
        else if (nvec <= 128) BF_NORMB_LAUNCH(64, 2);
        else BF_NORMB_LAUNCH(64, 4);
    } else {
        if (nvec <= 512) BF_NORMB_LAUNCH(256, 2);
        else BF_NORMB_LAUNCH(256, 4);
    }
#undef BF_NORMB_LAUNCH
    BF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dgamma_rows_kernel, dim3((W + 15) / 16), dim3(1024), 0, stream, a.partial, nb, W, a.N, a.dgout, a.dgpre);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// bf_add_rmsnorm_bwd's kernel: stage 2 above with gamma itself (no offset), dy always there, gamma held in registers across
// a workgroup's rows and dz stored in the loop that forms it; the same layouts, walk over the rows, precision and [N] row of
// partials per workgroup.  It is norm_add_rmsnorm_bwd_kernel<..., PRE = false> in arithmetic, bit for bit, and is kept
// beside it because that instantiation runs 7 - 11 % slower on the device at Llama's shapes (28.1 against 26.2 us at N 1024,
// 52.1 against 46.8 us at N 4096, 8192 rows of bf16) for a reason that was not found; folding the two is left open
// (profiles/decoder_blocks_unified.md).
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

template <typename T, typename GT>
int launch_rmsnorm_bwd(const void* z, const void* gamma, const void* dy, const void* dz_in, void* dz, float* partial,
                       float* dgamma, long long rows, int N, float eps, hipStream_t stream) {
    int G, nb;
    norm_bwd_layout(rows, N, &G, &nb);
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
    hipLaunchKernelGGL(dgamma_rows_kernel, dim3((N + 15) / 16), dim3(1024), 0, stream, partial, nb, N, N, dgamma, (float*)nullptr);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int launch_rmsnorm_bwd_gt(const void* z, const void* gamma, int param_dtype, const void* dy, const void* dz_in, void* dz,
                          float* partial, float* dgamma, long long rows, int N, float eps, hipStream_t stream) {
    if (param_dtype == BF_DT_F32) return launch_rmsnorm_bwd<T, float>(z, gamma, dy, dz_in, dz, partial, dgamma, rows, N, eps, stream);
    return launch_rmsnorm_bwd<T, T>(z, gamma, dy, dz_in, dz, partial, dgamma, rows, N, eps, stream);
}


// bf_add_rmsnorm_bwd and bf_norm_add_rmsnorm_bwd: one set of checks; `family` as norm_entry's (the other entry also needs dy)
int norm_bwd_entry(const char* who, bool family, const void* d_x, const void* d_z, const void* d_gamma_pre,
                   const void* d_gamma_out, int param_dtype, int weight_offset, const void* d_dy, const void* d_dz_in, void* d_dz,
                   void* d_dx, float* d_dgamma_pre, float* d_dgamma_out, void* d_workspace, size_t workspace_bytes, int dtype,
                   int64_t rows, int N, float eps_pre, float eps_out, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("%s: bad shape rows=%lld N=%d", who, (long long)rows, N);
    if (N % 8 || N > 8192) BF_FAIL("%s: N=%d must be a multiple of 8 and at most 8192", who, N);
    if (!d_dgamma_out || (d_gamma_pre && !d_dgamma_pre)) BF_FAIL("%s: null parameter gradient", who);
    if (family && weight_offset != 0 && weight_offset != 1) BF_FAIL("%s: weight_offset=%d must be 0 or 1", who, weight_offset);
    if (!dtype_ok(dtype)) BF_FAIL("%s: unknown dtype %d", who, dtype);
    if (param_dtype != BF_DT_F32 && param_dtype != dtype)
        BF_FAIL("%s: %s must be fp32 or have the activation dtype", who, family ? "the gammas" : "gamma");
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        BF_HIP_CHECK(hipMemsetAsync(d_dgamma_out, 0, (size_t)N * sizeof(float), st));
        if (d_gamma_pre) BF_HIP_CHECK(hipMemsetAsync(d_dgamma_pre, 0, (size_t)N * sizeof(float), st));
        return 0;
    }
    if (!d_z || !d_gamma_out || (family ? (!d_dy && !d_dz_in) : (!d_dy || !d_dz))) BF_FAIL("%s: null pointer", who);
    if (d_gamma_pre ? (!d_x || !d_dx) : !d_dz) BF_FAIL("%s: with gamma_pre x and dx are needed, without it dz", who);
    const uintptr_t al = (uintptr_t)d_x | (uintptr_t)d_z | (uintptr_t)d_gamma_pre | (uintptr_t)d_gamma_out | (uintptr_t)d_dy |
                         (uintptr_t)d_dz_in | (uintptr_t)d_dz | (uintptr_t)d_dx | (uintptr_t)d_dgamma_pre |
                         (uintptr_t)d_dgamma_out | (uintptr_t)d_workspace;
    if (al & 15) BF_FAIL("%s: pointers must be 16-byte aligned", who);
    const size_t need = norm_bwd_workspace_bytes(rows, N, d_gamma_pre != nullptr);
    if (!d_workspace || workspace_bytes < need) BF_FAIL("%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    const norm_bwd_args_t a = {d_x, d_z, d_gamma_pre, d_gamma_out, d_dy, d_dz_in, d_dz, d_gamma_pre ? d_dx : nullptr,
                               reinterpret_cast<float*>(d_workspace), d_gamma_pre ? d_dgamma_pre : nullptr, d_dgamma_out,
                               rows, N, family ? (float)weight_offset : kNoOffset, eps_pre, eps_out};
    if (!family) {
        float* partial = reinterpret_cast<float*>(d_workspace);
        switch (dtype) {
            case BF_DT_BF16: return launch_rmsnorm_bwd_gt<__bf16>(d_z, d_gamma_out, param_dtype, d_dy, d_dz_in, d_dz, partial, d_dgamma_out, rows, N, eps_out, st);
            case BF_DT_F16: return launch_rmsnorm_bwd_gt<_Float16>(d_z, d_gamma_out, param_dtype, d_dy, d_dz_in, d_dz, partial, d_dgamma_out, rows, N, eps_out, st);
            default: return launch_rmsnorm_bwd_gt<float>(d_z, d_gamma_out, param_dtype, d_dy, d_dz_in, d_dz, partial, d_dgamma_out, rows, N, eps_out, st);
        }
    }
    BF_BY_TYPES(launch_norm_bwd, d_gamma_pre != nullptr, a, st);
}

// ---- (per-head RMSNorm of q and k, then) the rotary embedding ----------------------------------------------------------------
// out = n * cos + rotate_half(n) * sin with rotate_half(n) = [-n2, n1] over the two halves of a head (HF's convention).
// One lane owns 8 elements of a head's first half and their 8 partners of the second: it loads both, then stores both,
// which is what makes the in-place form safe.  Lanes run over (token row, head of q then of k, vector) with the heads
// fastest, so the projections' [B, T, H*D] layout is read in address order.  NORM: the D / 16 lanes that own a head first
// normalise it, n = x * rsqrt(mean_D(x^2) + eps) * (woff + gamma), in fp32 and unrounded; the sum of squares crosses the
// lanes by xor shuffles.  Without NORM (and for a tensor whose gamma is NULL) n = x.
struct rope_args_t {
    int T, H, Hkv, cos_batch;
    unsigned total;  // lanes of work: B * T * (H + Hkv) * D / 16
    float woff, eps;
    long long q[3], k[3], qo[3], ko[3];
};

template <typename T, typename CT, typename GT, int D, bool NORM>
__global__ __launch_bounds__(256) void qknorm_rope_kernel(const T* q, const T* k, const CT* __restrict__ cosp,
                                                          const CT* __restrict__ sinp, const GT* __restrict__ gamma_q,
                                                          const GT* __restrict__ gamma_k, T* q_out, T* k_out,
                                                          const rope_args_t a) {
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

// The transpose, then the per-head norm's backward.  The forward's work split and loop.  A lane loads its 8 + 8 elements
// of the incoming gradient and rotates them back,
//     dn1 = do1 c1 + do2 s2,   dn2 = do2 c2 - do1 s1
// (the adjoint for tables whose two halves differ as well, which "the forward with sin negated" is not).  NORM, for a
// tensor that has a gamma: with x the forward's input, laid out as the output is, r = rsqrt(mean_D(x^2) + eps) recomputed
// across the head's D / 16 lanes (the sum of squares in fp64) and b = (woff + g) o dn,
//     dx = r b - x r^3 mean_D(x o b),   dgamma = sum_{b, t, heads} dn o x r.
// A lane's columns are the same in every round of the loop (the stride is a multiple of 256), so it keeps the fp32 dgamma
// partials of its 16 columns in registers, one set for q and one for k, each term formed in fp64.  The workgroup combines
// them through LDS in a fixed order into one [2, D] row, which dgamma_rows_kernel sums: the grid of a NORM launch fixes
// the order of that sum.  Algorithmic bytes per element: 1 read + 1 write (+ 1 read with a gamma) * sizeof(T), and the tables
// once per token.
template <typename T, typename CT, typename GT, int D, bool NORM>
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(const T* dqo, const T* dko, const T* xq, const T* xk,
                                                              const CT* __restrict__ cosp, const CT* __restrict__ sinp,
                                                              const GT* __restrict__ gamma_q, const GT* __restrict__ gamma_k,
                                                              T* dq, T* dk, float* __restrict__ partial, const rope_args_t a) {
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
        const long long* si = is_q ? a.q : a.k;
        const long long* so = is_q ? a.qo : a.ko;
        const T* src = (is_q ? dqo : dko) + b * si[0] + h * si[1] + t * si[2] + j * 8;
        const long long off = b * so[0] + h * so[1] + t * so[2] + j * 8;  // of the output and, NORM, of x
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

struct rope_ptrs_t {
    const void *q, *k, *c, *s, *gq, *gk;  // q / k: what is rotated (the backward's incoming gradients)
    const void *xq, *xk;                  // the backward's forward inputs
    void *qo, *ko;
    float *partial, *dgq, *dgk;
    int D, cs_dtype;
    unsigned blocks;  // the grid
    bool bwd;
};

template <typename T, typename CT, typename GT, bool NORM>
int launch_rope_types(const rope_ptrs_t& p, const rope_args_t& a, hipStream_t stream) {
    const dim3 grid(p.blocks), block(256);
#define BF_ROPE_LAUNCH(D_)                                                                                                      \
    if (p.bwd)                                                                                                                  \
        hipLaunchKernelGGL((qknorm_rope_bwd_kernel<T, CT, GT, D_, NORM>), grid, block, 0, stream, (const T*)p.q, (const T*)p.k,  \
                           (const T*)p.xq, (const T*)p.xk, (const CT*)p.c, (const CT*)p.s, (const GT*)p.gq, (const GT*)p.gk,     \
                           (T*)p.qo, (T*)p.ko, p.partial, a);                                                                   \
    else                                                                                                                        \
        hipLaunchKernelGGL((qknorm_rope_kernel<T, CT, GT, D_, NORM>), grid, block, 0, stream, (const T*)p.q, (const T*)p.k,      \
                           (const CT*)p.c, (const CT*)p.s, (const GT*)p.gq, (const GT*)p.gk, (T*)p.qo, (T*)p.ko, a)
    if (p.D == 64) BF_ROPE_LAUNCH(64);
    else if (p.D == 128) BF_ROPE_LAUNCH(128);
    else BF_ROPE_LAUNCH(256);
#undef BF_ROPE_LAUNCH
    BF_HIP_CHECK(hipGetLastError());
    if (NORM && p.bwd) {
        hipLaunchKernelGGL(dgamma_rows_kernel, dim3((2 * p.D + 15) / 16), dim3(1024), 0, stream, p.partial, (int)p.blocks,
                           2 * p.D, p.D, p.dgq, p.dgk);
        BF_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// (without gammas GT names nothing: one instantiation, on float)
template <typename T, typename GT, bool NORM>
int launch_rope(const rope_ptrs_t& p, const rope_args_t& a, hipStream_t stream) {
    using G = __type_pack_element<NORM ? 0 : 1, GT, float>;
    if (p.cs_dtype == BF_DT_F32) return launch_rope_types<T, float, G, NORM>(p, a, stream);
    return launch_rope_types<T, T, G, NORM>(p, a, stream);
}

long long rope_total(const bf_rope_t& s) { return (long long)s.B * s.T * (s.H + s.Hkv) * (s.head_dim / 16); }

unsigned rope_blocks(long long total, unsigned cap) {
    const long long blocks = (total + 255) / 256;
    return (unsigned)(blocks < cap ? blocks : cap);
}

// What tells the four rotary entries apart: the name in the messages, the direction, whether head size 256 is taken,
// whether the outputs follow the shape's strides (bf_qknorm_rope_bwd lays them out [B, T, heads, D] itself) and the grid's cap.
struct rope_entry_t {
    const char* who;
    bool bwd, d256, shape_out_strides;
    unsigned cap;
};
constexpr rope_entry_t kRopeQK = {"bf_rope_qk", false, false, true, kRopeBlocks};
constexpr rope_entry_t kRopeQKBwd = {"bf_rope_qk_bwd", true, false, true, kRopeBlocks};
constexpr rope_entry_t kQKNormRope = {"bf_qknorm_rope", false, true, true, kRopeBlocks};
constexpr rope_entry_t kQKNormRopeBwd = {"bf_qknorm_rope_bwd", true, true, false, kBwdBlocks};

// One set of checks for the four.  d_q / d_k: what is rotated (forward: q and k, backward: their outputs' gradients);
// d_xq / d_xk, d_dgamma_*, the workspace: the backward's, with gammas.
int rope_entry(const rope_entry_t& e, const void* d_q, const void* d_k, const void* d_xq, const void* d_xk, const void* d_cos,
               const void* d_sin, int cs_dtype, const void* d_gamma_q, const void* d_gamma_k, int param_dtype, int weight_offset,
               float eps, void* d_q_out, void* d_k_out, float* d_dgamma_q, float* d_dgamma_k, void* d_workspace,
               size_t workspace_bytes, int dtype, const bf_rope_t* shape, void* stream) {
    const char* who = e.who;
    if (!shape) BF_FAIL("%s: shape is NULL", who);
    const bf_rope_t& s = *shape;
    if (s.head_dim != 64 && s.head_dim != 128 && !(e.d256 && s.head_dim == 256))
        BF_FAIL("%s: head_dim=%d must be %s", who, s.head_dim, e.d256 ? "64, 128 or 256" : "64 or 128");
    if (s.B < 0 || s.T < 1 || s.H < 1 || s.Hkv < 1) BF_FAIL("%s: bad shape B=%d T=%d H=%d Hkv=%d", who, s.B, s.T, s.H, s.Hkv);
    if (s.cos_batch != 1 && s.cos_batch != s.B) BF_FAIL("%s: cos_batch=%d must be 1 or B=%d", who, s.cos_batch, s.B);
    if (!d_q || !d_k || !d_cos || !d_sin || !d_q_out || !d_k_out) BF_FAIL("%s: null pointer", who);
    if (e.bwd && ((d_gamma_q && (!d_xq || !d_dgamma_q)) || (d_gamma_k && (!d_xk || !d_dgamma_k))))
        BF_FAIL("%s: a gamma needs the forward's input and a parameter gradient", who);
    const uintptr_t al = (uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_xq | (uintptr_t)d_xk | (uintptr_t)d_cos |
                         (uintptr_t)d_sin | (uintptr_t)d_gamma_q | (uintptr_t)d_gamma_k | (uintptr_t)d_q_out |
                         (uintptr_t)d_k_out | (uintptr_t)d_dgamma_q | (uintptr_t)d_dgamma_k | (uintptr_t)d_workspace;
    if (al & 15) BF_FAIL("%s: pointers must be 16-byte aligned", who);
    if (!strides_ok(s.q_stride) || !strides_ok(s.k_stride) ||
        (e.shape_out_strides && (!strides_ok(s.q_out_stride) || !strides_ok(s.k_out_stride))))
        BF_FAIL("%s: strides must be non-negative multiples of 8 elements", who);
    if (weight_offset != 0 && weight_offset != 1) BF_FAIL("%s: weight_offset=%d must be 0 or 1", who, weight_offset);
    if (!dtype_ok(dtype)) BF_FAIL("%s: unknown dtype %d", who, dtype);
    if (cs_dtype != BF_DT_F32 && cs_dtype != dtype) BF_FAIL("%s: cos / sin must be fp32 or have the activation dtype", who);
    const bool norm = d_gamma_q || d_gamma_k;
    if (norm && param_dtype != BF_DT_F32 && param_dtype != dtype)
        BF_FAIL("%s: the gammas must be fp32 or have the activation dtype", who);
    const long long total = rope_total(s);
    if (total > 0x7fffffffLL) BF_FAIL("%s: B * T * (H + Hkv) * head_dim / 16 = %lld exceeds 2^31 - 1", who, total);
    hipStream_t st = (hipStream_t)stream;
    if (total == 0) {
        if (e.bwd && d_gamma_q) BF_HIP_CHECK(hipMemsetAsync(d_dgamma_q, 0, (size_t)s.head_dim * sizeof(float), st));
        if (e.bwd && d_gamma_k) BF_HIP_CHECK(hipMemsetAsync(d_dgamma_k, 0, (size_t)s.head_dim * sizeof(float), st));
        return 0;
    }
    const unsigned blocks = rope_blocks(total, e.cap);
    const size_t need = (size_t)blocks * 2 * s.head_dim * sizeof(float);
    if (e.bwd && norm && (!d_workspace || workspace_bytes < need))
        BF_FAIL("%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    rope_args_t a;
    a.T = s.T, a.H = s.H, a.Hkv = s.Hkv, a.cos_batch = s.cos_batch, a.total = (unsigned)total;
    a.woff = (float)weight_offset, a.eps = eps;
    const long long D = s.head_dim;
    const long long own_q[3] = {s.T * s.H * D, D, s.H * D}, own_k[3] = {s.T * s.Hkv * D, D, s.Hkv * D};  // [B, T, heads, D]
    for (int i = 0; i < 3; ++i) {
        a.q[i] = s.q_stride[i], a.k[i] = s.k_stride[i];
        a.qo[i] = e.shape_out_strides ? s.q_out_stride[i] : own_q[i];
        a.ko[i] = e.shape_out_strides ? s.k_out_stride[i] : own_k[i];
    }
    const rope_ptrs_t p = {d_q, d_k, d_cos, d_sin, d_gamma_q, d_gamma_k, d_xq, d_xk, d_q_out, d_k_out,
                           reinterpret_cast<float*>(d_workspace), d_gamma_q ? d_dgamma_q : nullptr,
                           d_gamma_k ? d_dgamma_k : nullptr, s.head_dim, cs_dtype, blocks, e.bwd};
    BF_BY_TYPES(launch_rope, norm, p, a, st);
}

// ---- gate(g) * up ------------------------------------------------------------------------------------------------------------
// A gate is a device functor: fwd(g) = g s(g), and bwd(g, &s, &f) with s = s(g) and f = d(g s)/dg, so that
//     y = fwd(g) u,      dup = dy (g s),      dgate = dy (u f)
// with the bounded factors multiplied first and dy last.  Both backwards take s and 1 - s from e = exp(-|.|) in (0, 1] —
// 1 / (1 + e) and e / (1 + e), whichever way round the sign says — so nothing overflows, 1 - s keeps its relative
// precision where s rounds to 1, and the limits come out by themselves: g -> -inf gives s = 0 and (0, 0), g -> +inf gives
// 1 - s = 0 and (dy u, dy g).

// SiLU: s = 1 / (1 + exp(-g)), f = s (1 + g (1 - s)).  The forward's exp overflows to +inf for g < -88.7 (the quotient is
// then -0, the limit) and underflows to 0 for large gates (the quotient is g): finite for every finite input.
struct silu_gate {
    static __device__ __forceinline__ float fwd(float g) { return g / (1.0f + expf(-g)); }
    static __device__ __forceinline__ void bwd(float g, float* s, float* f) {
        const float e = expf(-fabsf(g));
        const float big = 1.0f / (1.0f + e), small = e * big;
        const float ms = g >= 0.f ? small : big;
        *s = g >= 0.f ? big : small;
        *f = *s * fmaf(g, ms, 1.0f);
    }
};

// tanh-GELU: 0.5 g (1 + tanh k) = g / (1 + exp(-2 k)) with k = sqrt(2/pi) (g + 0.044715 g^3), so s = sigmoid(2k): the
// quotient form has no 1 + tanh k that cancels for negative gates.  The forward too goes through e = exp(-|2k|): for
// negative gates the result follows e down through the subnormals to -0 instead of dropping to 0 where exp(88.8) would be inf
// while g u / exp(88.8) is still a normal number, and g^2 beyond fp32's range gives e = 0 and the two limits (g u and -0):
// finite wherever gate * up is.  The argument 2k = g p, p = 2c + 2c 0.044715 g^2, is formed in fp64 and rounded to fp32
// once: where e dominates the result an absolute error of the argument is a relative error of y, and the argument passes
// 100 before e leaves the normal range — one rounding costs 100 * 2^-24, the four of an fp32 evaluation would cost most
// of the 2^-16 the result is held to.  Backward: d(2k)/dg = q = 2c + 3 * 2c 0.044715 g^2 and f = s (1 + g q (1 - s)); g q is
// formed in fp64: g^3 leaves fp32's range at |g| = 7e12, where 1 - s (or s) has long been 0, and the fp64 product is finite
// up to the largest gate of any dtype (1e116), so no inf * 0 appears.  f is bounded by 1.13 and rounded to fp32 once.
struct gelu_tanh_gate {
    static constexpr double k2c = 1.5957691216057308;  // 2 sqrt(2 / pi)
    static constexpr double k2ca = k2c * 0.044715;
    static __device__ __forceinline__ float fwd(float g) {
        const double gd = (double)g;
        const float arg = (float)(gd * fma(gd * gd, k2ca, k2c));  // 2k; +-inf beyond fp32's range
        const float e = expf(-fabsf(arg));
        const float s = (arg >= 0.f ? 1.0f : e) / (1.0f + e);
        return g * s;
    }
    static __device__ __forceinline__ void bwd(float g, float* s, float* f) {
        const double gd = (double)g, g2 = gd * gd;
        const float arg = (float)(gd * fma(g2, k2ca, k2c));
        const float e = expf(-fabsf(arg));
        const float big = 1.0f / (1.0f + e), small = e * big;
        const float ms = arg >= 0.f ? small : big;
        *s = arg >= 0.f ? big : small;
        *f = (float)((double)*s * fma(gd * fma(g2, 3.0 * k2ca, k2c), (double)ms, 1.0));
    }
};

// blockIdx.x: 256 vectors of a row, blockIdx.y: rows blockIdx.y, + gridDim.y, ...
// Algorithmic bytes per element: (2 reads + 1 write) * sizeof(T); backward (3 reads + 2 writes).
template <typename T, typename GATE>
__global__ __launch_bounds__(256) void glu_kernel(const T* gate, long long gate_stride, const T* up, long long up_stride, T* out,
                                                  long long out_stride, long long rows, int nvec) {
    const int vi = blockIdx.x * 256 + threadIdx.x;
    if (vi >= nvec) return;
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        float g[8], u[8], o[8];
        load8(gate + row * gate_stride + vi * 8, g);
        load8(up + row * up_stride + vi * 8, u);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = GATE::fwd(g[i]) * u[i];
        store8(out + row * out_stride + vi * 8, o);
    }
}

template <typename T, typename GATE>
__global__ __launch_bounds__(256) void glu_bwd_kernel(const T* gate, long long gate_stride, const T* up, long long up_stride,
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
            float s, f;
            GATE::bwd(g[i], &s, &f);
            og[i] = d[i] * (u[i] * f);
            ou[i] = d[i] * (g[i] * s);
        }
        store8(dgate + row * dgate_stride + vi * 8, og);
        store8(dup + row * dup_stride + vi * 8, ou);
    }
}

// gate, up, out — or gate, up, dy, dgate, dup — with their row strides
struct glu_args_t {
    const void* in[3];
    void* out[2];
    int64_t stride[5];
    int n;  // tensors: 3 forward, 5 backward
};

template <typename T, typename GATE>
int launch_glu(const glu_args_t& a, long long rows, int N, hipStream_t stream) {
    const int nvec = N >> 3;
    const unsigned gx = (unsigned)((nvec + 255) / 256);
    const long long want = 8192 / gx > 0 ? 8192 / gx : 1;  // about 8192 workgroups at most, the rest by the row loop
    const dim3 grid(gx, (unsigned)(rows < want ? rows : want)), block(256);
    if (a.n == 3)
        hipLaunchKernelGGL((glu_kernel<T, GATE>), grid, block, 0, stream, (const T*)a.in[0], a.stride[0], (const T*)a.in[1],
                           a.stride[1], (T*)a.out[0], a.stride[2], rows, nvec);
    else
        hipLaunchKernelGGL((glu_bwd_kernel<T, GATE>), grid, block, 0, stream, (const T*)a.in[0], a.stride[0], (const T*)a.in[1],
                           a.stride[1], (const T*)a.in[2], a.stride[2], (T*)a.out[0], a.stride[3], (T*)a.out[1], a.stride[4],
                           rows, nvec);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// bf_swiglu, bf_geglu and their backwards: one set of checks, `who` names the entry in the messages
int glu_entry(const char* who, bool gelu, const glu_args_t& a, int dtype, int64_t rows, int N, void* stream) {
    if (rows < 0 || N <= 0) BF_FAIL("%s: bad shape rows=%lld N=%d", who, (long long)rows, N);
    if (N % 8) BF_FAIL("%s: N=%d must be a multiple of 8", who, N);
    const void* ptr[5] = {a.in[0], a.in[1], a.n == 3 ? a.out[0] : a.in[2], a.out[0], a.out[1]};
    uintptr_t al = 0;
    bool null = false, bad_stride = false;
    for (int i = 0; i < a.n; ++i) {
        null |= !ptr[i], al |= (uintptr_t)ptr[i];
        bad_stride |= a.stride[i] < N || (a.stride[i] & 7);
    }
    if (null) BF_FAIL("%s: null pointer", who);
    if (al & 15) BF_FAIL("%s: pointers must be 16-byte aligned", who);
    const int64_t* st = a.stride;
    if (bad_stride && a.n == 3)
        BF_FAIL("%s: row strides (%lld, %lld, %lld) must be multiples of 8 and at least N=%d", who, (long long)st[0],
                (long long)st[1], (long long)st[2], N);
    if (bad_stride)
        BF_FAIL("%s: row strides (%lld, %lld, %lld, %lld, %lld) must be multiples of 8 and at least N=%d", who, (long long)st[0],
                (long long)st[1], (long long)st[2], (long long)st[3], (long long)st[4], N);
    if (!dtype_ok(dtype)) BF_FAIL("%s: unknown dtype %d", who, dtype);
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case BF_DT_BF16: return gelu ? launch_glu<__bf16, gelu_tanh_gate>(a, rows, N, s) : launch_glu<__bf16, silu_gate>(a, rows, N, s);
        case BF_DT_F16: return gelu ? launch_glu<_Float16, gelu_tanh_gate>(a, rows, N, s) : launch_glu<_Float16, silu_gate>(a, rows, N, s);
        default: return gelu ? launch_glu<float, gelu_tanh_gate>(a, rows, N, s) : launch_glu<float, silu_gate>(a, rows, N, s);
    }
}

}  // namespace

int bf_add_rmsnorm(const void* d_x, const void* d_residual, const void* d_gamma, int param_dtype, void* d_sum_out, void* d_out,
                   int dtype, int64_t rows, int N, float eps, void* stream) {
    return norm_entry("bf_add_rmsnorm", false, d_x, nullptr, d_residual, d_gamma, param_dtype, 0, d_sum_out, d_out, dtype, rows,
                      N, eps, eps, stream);
}

int bf_norm_add_rmsnorm(const void* d_x, const void* d_gamma_pre, const void* d_residual, const void* d_gamma_out,
                        int param_dtype, int weight_offset, void* d_sum_out, void* d_out, int dtype, int64_t rows, int N,
                        float eps_pre, float eps_out, void* stream) {
    return norm_entry("bf_norm_add_rmsnorm", true, d_x, d_gamma_pre, d_residual, d_gamma_out, param_dtype, weight_offset,
                      d_sum_out, d_out, dtype, rows, N, eps_pre, eps_out, stream);
}

size_t bf_add_rmsnorm_bwd_workspace_bytes(int64_t rows, int N) { return norm_bwd_workspace_bytes(rows, N, false); }

size_t bf_norm_add_rmsnorm_bwd_workspace_bytes(int64_t rows, int N, int has_gamma_pre) {
    return norm_bwd_workspace_bytes(rows, N, has_gamma_pre != 0);
}

int bf_add_rmsnorm_bwd(const void* d_z, const void* d_gamma, int param_dtype, const void* d_dy, const void* d_dz_in,
                       void* d_dz, float* d_dgamma, void* d_workspace, size_t workspace_bytes, int dtype, int64_t rows, int N,
                       float eps, void* stream) {
    return norm_bwd_entry("bf_add_rmsnorm_bwd", false, nullptr, d_z, nullptr, d_gamma, param_dtype, 0, d_dy, d_dz_in, d_dz,
                          nullptr, nullptr, d_dgamma, d_workspace, workspace_bytes, dtype, rows, N, eps, eps, stream);
}

int bf_norm_add_rmsnorm_bwd(const void* d_x, const void* d_z, const void* d_gamma_pre, const void* d_gamma_out, int param_dtype,
                            int weight_offset, const void* d_dy, const void* d_dz_in, void* d_dz, void* d_dx,
                            float* d_dgamma_pre, float* d_dgamma_out, void* d_workspace, size_t workspace_bytes, int dtype,
                            int64_t rows, int N, float eps_pre, float eps_out, void* stream) {
    return norm_bwd_entry("bf_norm_add_rmsnorm_bwd", true, d_x, d_z, d_gamma_pre, d_gamma_out, param_dtype, weight_offset, d_dy,
                          d_dz_in, d_dz, d_dx, d_dgamma_pre, d_dgamma_out, d_workspace, workspace_bytes, dtype, rows, N,
                          eps_pre, eps_out, stream);
}

int bf_rope_qk(const void* d_q, const void* d_k, const void* d_cos, const void* d_sin, int cs_dtype, void* d_q_out,
               void* d_k_out, int dtype, const bf_rope_t* shape, void* stream) {
    return rope_entry(kRopeQK, d_q, d_k, nullptr, nullptr, d_cos, d_sin, cs_dtype, nullptr, nullptr, BF_DT_F32, 0, 0.f, d_q_out,
                      d_k_out, nullptr, nullptr, nullptr, 0, dtype, shape, stream);
}

int bf_rope_qk_bwd(const void* d_dq, const void* d_dk, const void* d_cos, const void* d_sin, int cs_dtype, void* d_dq_out,
                   void* d_dk_out, int dtype, const bf_rope_t* shape, void* stream) {
    return rope_entry(kRopeQKBwd, d_dq, d_dk, nullptr, nullptr, d_cos, d_sin, cs_dtype, nullptr, nullptr, BF_DT_F32, 0, 0.f,
                      d_dq_out, d_dk_out, nullptr, nullptr, nullptr, 0, dtype, shape, stream);
}

int bf_qknorm_rope(const void* d_q, const void* d_k, const void* d_cos, const void* d_sin, int cs_dtype,
                   const void* d_gamma_q, const void* d_gamma_k, int param_dtype, int weight_offset, float eps,
                   void* d_q_out, void* d_k_out, int dtype, const bf_rope_t* shape, void* stream) {
    return rope_entry(kQKNormRope, d_q, d_k, nullptr, nullptr, d_cos, d_sin, cs_dtype, d_gamma_q, d_gamma_k, param_dtype,
                      weight_offset, eps, d_q_out, d_k_out, nullptr, nullptr, nullptr, 0, dtype, shape, stream);
}

size_t bf_qknorm_rope_bwd_workspace_bytes(const bf_rope_t* shape, int has_gamma) {
    if (!shape || !has_gamma) return 0;
    const long long total = rope_total(*shape);
    if (total < 1) return 0;
    return (size_t)rope_blocks(total, kQKNormRopeBwd.cap) * 2 * shape->head_dim * sizeof(float);
}

int bf_qknorm_rope_bwd(const void* d_dq_out, const void* d_dk_out, const void* d_q, const void* d_k, const void* d_cos,
                       const void* d_sin, int cs_dtype, const void* d_gamma_q, const void* d_gamma_k, int param_dtype,
                       int weight_offset, float eps, void* d_dq, void* d_dk, float* d_dgamma_q, float* d_dgamma_k,
                       void* d_workspace, size_t workspace_bytes, int dtype, const bf_rope_t* shape, void* stream) {
    return rope_entry(kQKNormRopeBwd, d_dq_out, d_dk_out, d_q, d_k, d_cos, d_sin, cs_dtype, d_gamma_q, d_gamma_k, param_dtype,
                      weight_offset, eps, d_dq, d_dk, d_dgamma_q, d_dgamma_k, d_workspace, workspace_bytes, dtype, shape, stream);
}

int bf_swiglu(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, void* d_out,
              int64_t out_row_stride, int dtype, int64_t rows, int N, void* stream) {
    return glu_entry("bf_swiglu", false, {{d_gate, d_up}, {d_out}, {gate_row_stride, up_row_stride, out_row_stride}, 3}, dtype,
                     rows, N, stream);
}

int bf_geglu(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, void* d_out,
             int64_t out_row_stride, int dtype, int64_t rows, int N, void* stream) {
    return glu_entry("bf_geglu", true, {{d_gate, d_up}, {d_out}, {gate_row_stride, up_row_stride, out_row_stride}, 3}, dtype,
                     rows, N, stream);
}

int bf_swiglu_bwd(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, const void* d_dy,
                  int64_t dy_row_stride, void* d_dgate, int64_t dgate_row_stride, void* d_dup, int64_t dup_row_stride,
                  int dtype, int64_t rows, int N, void* stream) {
    return glu_entry("bf_swiglu_bwd", false,
                     {{d_gate, d_up, d_dy}, {d_dgate, d_dup},
                      {gate_row_stride, up_row_stride, dy_row_stride, dgate_row_stride, dup_row_stride}, 5},
                     dtype, rows, N, stream);
}

int bf_geglu_bwd(const void* d_gate, int64_t gate_row_stride, const void* d_up, int64_t up_row_stride, const void* d_dy,
                 int64_t dy_row_stride, void* d_dgate, int64_t dgate_row_stride, void* d_dup, int64_t dup_row_stride, int dtype,
                 int64_t rows, int N, void* stream) {
    return glu_entry("bf_geglu_bwd", true,
                     {{d_gate, d_up, d_dy}, {d_dgate, d_dup},
                      {gate_row_stride, up_row_stride, dy_row_stride, dgate_row_stride, dup_row_stride}, 5},
                     dtype, rows, N, stream);
}
