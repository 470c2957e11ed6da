// bf_predictive.hip — Monte-Carlo predictive statistics of S per-sample logits (bf_mc_predictive_*).
//
// Replaces what a user of the reference computes by hand on the host after sample_bayesian: the per-sample accuracy
// spread (`acc_std`, the reference's examples/bert_glue.py:186, 237, 281; bert_squad.py:478-483) and the softmax
// statistics of the Bayesian model average (predictive entropy, expected entropy, mutual information).
//
// Two kernels, both one workgroup per row (grid-strided over rows, at most kMaxGrid workgroups):
//   partial  logits [S_local][R][C] -> mergeable sums over this rank's samples (layout: bf_mc_predictive_bytes);
//            pass 1 runs an online (max, sum e^d, sum e^d * d, argmax) over each sample's row, d = l - max, split
//            into (sample, segment) work items over the waves and merged per sample in a fixed order; pass 2 sums
//            p_s(c) = exp(l_s(c) - lse_s) over the samples.  When the row's S x C slice fits in kStageBytes of LDS,
//            pass 1 leaves it there (fp32) and pass 2 reads LDS: the logits are read from memory once.
//   finish   complete partials -> probs, entropies, prediction, log-likelihood; the scalars (acc_std, nll, the BMA
//            correct count, the invalid-label count) are reduced by the last workgroup to arrive.
// Cross-workgroup reductions (the per-sample correct counts in partial, the scalars in finish) write one slot per
// workgroup and hand off through an agent-scope release / ticket / acquire; the last arriver sums the slots in
// workgroup order (deterministic) and resets the ticket, so the workspace is zero-filled once by the caller and
// stays reusable by every later launch on the same stream.
#include <float.h>
#include <math.h>

#include "bf_common.h"
#include "bf_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGrid = 1024;
constexpr int kMaxSegs = 16;
constexpr int kSegMin = 1024;                       // elements per (sample, segment) work item, at least
constexpr size_t kStageBytes = 64 * 1024;           // LDS for the staged fp32 S x C slice of a row
constexpr int kMaxSLocal = 1024;
constexpr int kMaxItems = 1024;                     // (sample, segment) work items per row
constexpr size_t kMaxLds = 64 * 1024;
constexpr int kMaxSTotal = 1 << 20;
constexpr size_t kTicketBytes = 64;

struct Layout {
    size_t sum_p, sum_h, sum_py, sum_logpy, counts, end;
};

Layout layout_of(int64_t R, int64_t C, int S_total, int has_labels) {
    Layout L;
    L.sum_p = 0;
    L.sum_h = L.sum_p + sizeof(float) * (size_t)R * (size_t)C;
    L.sum_py = bf_align_up(L.sum_h + sizeof(float) * (size_t)R, 8);
    const size_t nl = has_labels ? (size_t)R : 0;
    L.sum_logpy = L.sum_py + sizeof(double) * nl;
    L.counts = L.sum_logpy + sizeof(double) * nl;
    L.end = L.counts + sizeof(double) * (has_labels ? (size_t)S_total : 0);
    return L;
}

int grid_for(int64_t R) { return (int)(R < kMaxGrid ? R : kMaxGrid); }

size_t slot_bytes(int S_total) {
    const size_t s = (size_t)(S_total < kMaxSLocal ? S_total : kMaxSLocal);  // per-sample slots hold S_local counts
    return bf_align_up(sizeof(uint32_t) * (size_t)kMaxGrid * s, 16);
}

size_t workspace_bytes(int S_total) {
    // [ticket partial | ticket finish] [partial slots: grid x S_local uint32] [finish slots: grid x 4 doubles]
    return kTicketBytes + slot_bytes(S_total) + sizeof(double) * 4 * kMaxGrid;
}

template <size_t A, typename P>
__device__ __forceinline__ unsigned char* align_dev(P* p) {
    return reinterpret_cast<unsigned char*>(((uintptr_t)p + (A - 1)) & ~(uintptr_t)(A - 1));
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__bf16 v) { return (float)v; }
__device__ __forceinline__ float to_f32(_Float16 v) { return (float)v; }

// 8 consecutive elements [c0, c0 + 8) of one (sample, row); past C they read as -inf.  `vec`: the row start is 16-byte
// aligned (the chunk is then too), so a full chunk is one 16-byte load (two for fp32).
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ p, int64_t c0, int64_t C, bool vec, float v[8]) {
    if (vec && c0 + 8 <= C) {
        if constexpr (sizeof(T) == 2) {
            const uint4 u = *reinterpret_cast<const uint4*>(p + c0);
            const T* h = reinterpret_cast<const T*>(&u);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = to_f32(h[j]);
        } else {
            const float4 a = *reinterpret_cast<const float4*>(p + c0);
            const float4 b = *reinterpret_cast<const float4*>(p + c0 + 4);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = c0 + j < C ? to_f32(p[c0 + j]) : -INFINITY;
    }
}

// online softmax state of a stretch of one row: m = max, s = sum e^(l - m), t = sum e^(l - m) (l - m), i = first argmax
struct Online {
    float m, s, t;
    int64_t i;
};

__device__ __forceinline__ float exp_neg(float d) { return exp_fast(fmaxf(d, -200.0f)); }  // e^d, d <= 0; -inf -> 0

__device__ __forceinline__ void online_chunk(Online& o, const float v[8], int64_t c0) {
    float cm = v[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) cm = fmaxf(cm, v[j]);
    if (cm > o.m) {
        int64_t first = c0 + 7;
#pragma unroll
        for (int j = 7; j >= 0; --j) first = v[j] == cm ? c0 + j : first;
        if (o.s > 0.0f) {
            const float dm = o.m - cm, a = exp_neg(dm);
            o.t = a * fmaf(dm, o.s, o.t);
            o.s *= a;
        }
        o.m = cm;
        o.i = first;
    }
    if (o.m == -INFINITY) return;  // nothing finite yet (a -inf or masked chunk)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float d = v[j] - o.m;
        const float e = v[j] == -INFINITY ? 0.0f : exp_neg(d);
        o.s += e;
        o.t = v[j] == -INFINITY ? o.t : fmaf(e, d, o.t);
    }
}

// merge b into a (a holds the lower element indices on a tie)
__device__ __forceinline__ Online online_merge(Online a, Online b) {
    const float M = fmaxf(a.m, b.m);
    Online r;
    r.m = M;
    r.i = a.m > b.m ? a.i : (b.m > a.m ? b.i : (a.i < b.i ? a.i : b.i));
    if (M == -INFINITY) {
        r.s = r.t = 0.0f;
        return r;
    }
    float s = 0.0f, t = 0.0f;
    if (a.s > 0.0f) {
        const float d = a.m - M, e = exp_neg(d);
        s += e * a.s;
        t += e * fmaf(d, a.s, a.t);
    }
    if (b.s > 0.0f) {
        const float d = b.m - M, e = exp_neg(d);
        s += e * b.s;
        t += e * fmaf(d, b.s, b.t);
    }
    r.s = s, r.t = t;
    return r;
}

__device__ __forceinline__ Online wave_merge(Online o) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        Online b;
        b.m = __shfl_xor(o.m, k);
        b.s = __shfl_xor(o.s, k);
        b.t = __shfl_xor(o.t, k);
        b.i = __shfl_xor(o.i, k);
        o = online_merge(o, b);  // (merge order is fixed per lane: results are run-to-run identical)
    }
    return o;
}

// Last-arriver hand-off (cdna_hip_programming.md, Guideline 16 counter form).  `flag` is a word of the dynamic LDS array.
__device__ bool arrive_last(uint32_t* ticket, uint32_t n_blocks, volatile uint32_t* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == n_blocks - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
        }
        *flag = last ? 1u : 0u;
    }
    __syncthreads();
    return *flag != 0u;
}

struct PartialArgs {
    const void* logits;
    int64_t sample_stride, row_stride, R, C;
    int S_local, S_total, sample_base;
    const int64_t* labels;
    int64_t ignore_index;
    float* sum_p;
    float* sum_h;
    double* sum_py;
    double* sum_logpy;
    double* counts;
    uint32_t* ticket;
    uint32_t* slots;  // [grid][S_local]
    int segs;         // segments per sample in pass 1
    int64_t seg_len;  // elements per segment, a multiple of 8
};

__device__ __forceinline__ bool label_ok(int64_t y, int64_t C, int64_t ignore_index) {
    return y != ignore_index && y >= 0 && y < C;
}

template <typename T, bool STAGE>
__global__ __launch_bounds__(kThreads) void predictive_partial_kernel(const PartialArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    // dynamic LDS: per work item (m, s, t, i) | per sample lse, H, logpy | per sample counts | flag | staged slice
    const int S = a.S_local, items = S * a.segs;
    float* w_m = reinterpret_cast<float*>(smem);
    float* w_s = w_m + items;
    float* w_t = w_s + items;
    int64_t* w_i = reinterpret_cast<int64_t*>(align_dev<8>(w_t + items));
    float* s_lse = reinterpret_cast<float*>(w_i + items);
    float* s_h = s_lse + S;
    float* s_logpy = s_h + S;
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_logpy + S);
    uint32_t* s_flag = s_cnt + S;
    float* stage = reinterpret_cast<float*>(align_dev<16>(s_flag + 4));

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t C = a.C;
    const T* base = static_cast<const T*>(a.logits);
    for (int s = tid; s < S; s += kThreads) s_cnt[s] = 0;

    for (int64_t r = blockIdx.x; r < a.R; r += gridDim.x) {
        // ---- pass 1: (sample, segment) items over the waves
        for (int it = wave; it < items; it += kWaves) {
            const int s = it / a.segs, g = it - s * a.segs;
            const T* p = base + (int64_t)s * a.sample_stride + r * a.row_stride;
            const bool vec = ((uintptr_t)p & 15) == 0;
            const int64_t c_begin = (int64_t)g * a.seg_len;
            const int64_t c_end = c_begin + a.seg_len < C ? c_begin + a.seg_len : C;
            Online o{-INFINITY, 0.0f, 0.0f, INT64_MAX};
            for (int64_t c0 = c_begin + 8 * lane; c0 < c_end; c0 += 8 * 64) {
                float v[8];
                load8(p, c0, c_end, vec, v);  // (segment bounds are multiples of 8: whole chunks until the row's tail)
                if (STAGE) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (c0 + j < c_end) stage[(int64_t)s * C + c0 + j] = v[j];
                }
                online_chunk(o, v, c0);
            }
            o = wave_merge(o);
            if (lane == 0) w_m[it] = o.m, w_s[it] = o.s, w_t[it] = o.t, w_i[it] = o.i;
        }
        __syncthreads();
        // ---- per sample: merge the segments in order; lse, H, argmax, and with labels log p(y) and the correct flag
        const int64_t y = a.labels ? a.labels[r] : 0;
        const bool valid = a.labels && label_ok(y, C, a.ignore_index);
        for (int s = tid; s < S; s += kThreads) {
            Online o{w_m[s * a.segs], w_s[s * a.segs], w_t[s * a.segs], w_i[s * a.segs]};
            for (int g = 1; g < a.segs; ++g) {
                const int it = s * a.segs + g;
                o = online_merge(o, Online{w_m[it], w_s[it], w_t[it], w_i[it]});
            }
            const bool any = o.s > 0.0f;  // a row of -inf only: p = 0 everywhere, H = 0, argmax 0 (torch.argmax)
            const float ls = any ? log_fast(o.s) : 0.0f;
            s_lse[s] = any ? o.m + ls : -INFINITY;
            s_h[s] = any ? fmaxf(ls - o.t / o.s, 0.0f) : 0.0f;
            const int64_t arg = o.i == INT64_MAX ? 0 : o.i;
            if (valid) {
                const float ly = STAGE ? stage[(int64_t)s * C + y]
                                       : to_f32(base[(int64_t)s * a.sample_stride + r * a.row_stride + y]);
                s_logpy[s] = any && ly != -INFINITY ? ly - s_lse[s] : -INFINITY;
                s_cnt[s] += arg == y ? 1u : 0u;
            }
        }
        __syncthreads();
        if (tid == 0) {
            float h = 0.0f;
            double py = 0.0, lpy = 0.0;
            for (int s = 0; s < S; ++s) {
                h += s_h[s];
                if (valid) {
                    py += exp((double)s_logpy[s]);
                    lpy += (double)s_logpy[s];
                }
            }
            a.sum_h[r] = h;
            if (a.labels) a.sum_py[r] = py, a.sum_logpy[r] = lpy;
        }
        // ---- pass 2: sum over the samples of p_s(c), from LDS or re-read
        float* out = a.sum_p + r * C;
        for (int64_t c0 = 8 * (int64_t)tid; c0 < C; c0 += 8 * kThreads) {
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < S; ++s) {
                const float lse = s_lse[s];
                if (lse == -INFINITY) continue;
                float v[8];
                if (STAGE) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = c0 + j < C ? stage[(int64_t)s * C + c0 + j] : -INFINITY;
                } else {
                    const T* p = base + (int64_t)s * a.sample_stride + r * a.row_stride;
                    load8(p, c0, C, ((uintptr_t)p & 15) == 0, v);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += exp_neg(v[j] - lse);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j < C) out[c0 + j] = acc[j];
        }
        __syncthreads();  // the LDS of this row is rewritten by the next one
    }
    if (!a.labels) return;
    // ---- per-sample correct counts: one slot per workgroup, summed by the last one in workgroup order
    uint32_t* mine = a.slots + (size_t)blockIdx.x * S;
    for (int s = tid; s < S; s += kThreads) mine[s] = s_cnt[s];
    if (!arrive_last(a.ticket, gridDim.x, s_flag)) return;
    for (int s = tid; s < S; s += kThreads) s_cnt[s] = 0;
    __syncthreads();
    // every thread adds a coalesced stretch of the [grid][S] slots (integer adds: the sum is the same in any order)
    const size_t n_slots = (size_t)gridDim.x * S;
    for (size_t k = tid; k < n_slots; k += kThreads) atomicAdd(&s_cnt[k % S], a.slots[k]);
    __syncthreads();
    for (int s = tid; s < a.S_total; s += kThreads) {
        const int ls = s - a.sample_base;
        // other ranks' samples stay 0: a SUM over the ranks gives all S_total counts
        a.counts[s] = ls >= 0 && ls < S ? (double)s_cnt[ls] : 0.0;
    }
}

// sum over the workgroup in a fixed order (butterfly in each wave, lane 0's value, waves in order): run-to-run identical
__device__ double block_sum(double v, double* red) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
    v = __shfl(v, 0);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t += red[w];
    __syncthreads();
    return t;
}

struct FinishArgs {
    const float* sum_p;
    const float* sum_h;
    const double* sum_py;
    const double* counts;
    int64_t R, C;
    int S_total;
    const int64_t* labels;
    int64_t ignore_index;
    bf_predictive_out_t out;
    uint32_t* ticket;
    double* slots;  // [grid][4]: bma correct, sum of -log-likelihood, valid rows, invalid labels
};

__global__ __launch_bounds__(kThreads) void predictive_finish_kernel(const FinishArgs a) {
    __shared__ float red_h[kWaves];
    __shared__ float red_q[kWaves];
    __shared__ int64_t red_i[kWaves];
    __shared__ uint32_t flag[4];
    __shared__ double red_d[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t C = a.C;
    const float inv_s = 1.0f / (float)a.S_total;
    double bma = 0.0, nll = 0.0, nvalid = 0.0, invalid = 0.0;  // (thread 0's)
    for (int64_t r = blockIdx.x; r < a.R; r += gridDim.x) {
        const float* sp = a.sum_p + r * C;
        float* probs = a.out.d_probs + r * C;
        float h = 0.0f, best = -1.0f;
        int64_t bi = INT64_MAX;
        for (int64_t c = tid; c < C; c += kThreads) {  // lane-contiguous fp32: coalesced loads and stores
            const float q = sp[c] * inv_s;
            probs[c] = q;
            // (v_log_f32 does not take subnormal inputs; a q below FLT_MIN adds less than 1e-36 to the sum)
            h -= q >= FLT_MIN ? q * log_fast(q) : 0.0f;
            if (q > best) best = q, bi = c;
        }
        h = wave_sum(h);
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const float ob = __shfl_xor(best, k);
            const int64_t oi = __shfl_xor(bi, k);
            if (ob > best || (ob == best && oi < bi)) best = ob, bi = oi;
        }
        if (lane == 0) red_h[wave] = h, red_q[wave] = best, red_i[wave] = bi;
        __syncthreads();
        if (tid == 0) {
            float H = 0.0f, q = red_q[0];
            int64_t idx = red_i[0];
            for (int w = 0; w < kWaves; ++w) {
                H += red_h[w];
                if (red_q[w] > q || (red_q[w] == q && red_i[w] < idx)) q = red_q[w], idx = red_i[w];
            }
            if (idx == INT64_MAX) idx = 0;
            const float ee = a.sum_h[r] * inv_s;
            a.out.d_predictive_entropy[r] = H;
            a.out.d_expected_entropy[r] = ee;
            a.out.d_mutual_information[r] = fmaxf(H - ee, 0.0f);
            a.out.d_prediction[r] = idx;
            if (a.labels) {
                const int64_t y = a.labels[r];
                const bool valid = label_ok(y, C, a.ignore_index);
                const double ll = valid ? log(a.sum_py[r] / (double)a.S_total) : (double)NAN;
                a.out.d_log_likelihood[r] = ll;
                if (valid) {
                    bma += idx == y ? 1.0 : 0.0;
                    nll -= ll;
                    nvalid += 1.0;
                } else if (y != a.ignore_index) {
                    invalid += 1.0;
                }
            }
        }
        __syncthreads();
    }
    if (!a.labels) return;
    if (tid == 0) {
        double* mine = a.slots + 4 * (size_t)blockIdx.x;
        mine[0] = bma, mine[1] = nll, mine[2] = nvalid, mine[3] = invalid;
    }
    if (!arrive_last(a.ticket, gridDim.x, flag)) return;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t b = tid; b < gridDim.x; b += kThreads)
        for (int k = 0; k < 4; ++k) t[k] += a.slots[4 * (size_t)b + k];
    for (int k = 0; k < 4; ++k) t[k] = block_sum(t[k], red_d);
    // acc_std: population std of the per-sample counts, np.std's two passes (bert_glue.py:237)
    double csum = 0.0;
    for (int s = tid; s < a.S_total; s += kThreads) {
        a.out.d_correct_per_sample[s] = (int64_t)a.counts[s];
        csum += a.counts[s];
    }
    const double mean = block_sum(csum, red_d) / (double)a.S_total;
    double dev = 0.0;
    for (int s = tid; s < a.S_total; s += kThreads) dev += (a.counts[s] - mean) * (a.counts[s] - mean);
    const double var = block_sum(dev, red_d) / (double)a.S_total;
    if (tid == 0) {
        a.out.d_scalars[0] = sqrt(var);
        a.out.d_scalars[1] = t[2] > 0.0 ? t[1] / t[2] : (double)NAN;
        a.out.d_counts[0] = (int64_t)t[0];
        a.out.d_counts[1] = (int64_t)t[3];
    }
}

template <typename T, bool STAGE>
void launch_partial(const PartialArgs& a, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL((predictive_partial_kernel<T, STAGE>), dim3(grid_for(a.R)), dim3(kThreads), lds, stream, a);
}

}  // namespace

extern "C" size_t bf_mc_predictive_bytes(int64_t R, int64_t C, int S_total, int has_labels, size_t* offsets) {
    if (R < 1 || C < 1 || S_total < 1) return 0;
    const Layout L = layout_of(R, C, S_total, has_labels);
    if (offsets) {
        offsets[0] = L.sum_p, offsets[1] = L.sum_h, offsets[2] = L.sum_py;
        offsets[3] = L.sum_logpy, offsets[4] = L.counts, offsets[5] = L.end;
    }
    return L.end;
}

extern "C" size_t bf_mc_predictive_workspace_bytes(int S_total) {
    return S_total < 1 ? 0 : workspace_bytes(S_total);
}

extern "C" int bf_mc_predictive_partial(const void* d_logits, int dtype, int64_t sample_stride, int64_t row_stride,
                                        int S_local, int64_t R, int64_t C, const int64_t* d_labels,
                                        int64_t ignore_index, int sample_base, int S_total, void* d_partial,
                                        void* d_workspace, size_t workspace_bytes_, void* stream) {
    if (!d_logits || !d_partial || !d_workspace) BF_FAIL("bf_mc_predictive_partial: NULL logits, partial or workspace");
    if (R < 1 || C < 1 || C > INT32_MAX) BF_FAIL("bf_mc_predictive_partial: bad R=%lld C=%lld", (long long)R, (long long)C);
    if (S_local < 1 || S_local > kMaxSLocal || S_total < 1 || S_total > kMaxSTotal || sample_base < 0 ||
        sample_base + S_local > S_total)
        BF_FAIL("bf_mc_predictive_partial: bad samples (S_local=%d, sample_base=%d, S_total=%d; S_local <= %d)", S_local,
                sample_base, S_total, kMaxSLocal);
    if (dtype != BF_DT_F32 && dtype != BF_DT_BF16 && dtype != BF_DT_F16)
        BF_FAIL("bf_mc_predictive_partial: unknown dtype %d", dtype);
    if (row_stride < C || sample_stride < 0) BF_FAIL("bf_mc_predictive_partial: rows overlap (row_stride < C)");
    if (workspace_bytes_ < workspace_bytes(S_total))
        BF_FAIL("bf_mc_predictive_partial: workspace too small (%zu < %zu bytes)", workspace_bytes_,
                workspace_bytes(S_total));
    const Layout L = layout_of(R, C, S_total, d_labels != nullptr);
    unsigned char* P = static_cast<unsigned char*>(d_partial);
    unsigned char* W = static_cast<unsigned char*>(d_workspace);
    PartialArgs a;
    a.logits = d_logits, a.sample_stride = sample_stride, a.row_stride = row_stride, a.R = R, a.C = C;
    a.S_local = S_local, a.S_total = S_total, a.sample_base = sample_base;
    a.labels = d_labels, a.ignore_index = ignore_index;
    a.sum_p = reinterpret_cast<float*>(P + L.sum_p);
    a.sum_h = reinterpret_cast<float*>(P + L.sum_h);
    a.sum_py = reinterpret_cast<double*>(P + L.sum_py);
    a.sum_logpy = reinterpret_cast<double*>(P + L.sum_logpy);
    a.counts = reinterpret_cast<double*>(P + L.counts);
    a.ticket = reinterpret_cast<uint32_t*>(W);
    a.slots = reinterpret_cast<uint32_t*>(W + kTicketBytes);
    const int64_t chunks = (C + 7) / 8;
    int segs = (int)((C + kSegMin - 1) / kSegMin);
    const int seg_cap = kMaxItems / S_local < kMaxSegs ? kMaxItems / S_local : kMaxSegs;
    segs = segs > seg_cap ? seg_cap : segs;
    segs = segs < 1 ? 1 : segs;
    a.seg_len = (chunks + segs - 1) / segs * 8;
    a.segs = (int)((C + a.seg_len - 1) / a.seg_len);
    const size_t items = (size_t)S_local * a.segs;
    // must match the carve-up at the top of predictive_partial_kernel
    size_t lds = bf_align_up(3 * sizeof(float) * items, 8) + sizeof(int64_t) * items + 3 * sizeof(float) * S_local +
                 sizeof(uint32_t) * (S_local + 4);
    lds = bf_align_up(lds, 16);
    const size_t stage = sizeof(float) * (size_t)S_local * (size_t)C;
    const bool staged = stage <= kStageBytes && lds + stage <= kMaxLds;
    if (staged) lds += stage;
    if (lds > kMaxLds) BF_FAIL("bf_mc_predictive_partial: %zu bytes of LDS needed (S_local=%d)", lds, S_local);
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == BF_DT_BF16)
        staged ? launch_partial<__bf16, true>(a, lds, st) : launch_partial<__bf16, false>(a, lds, st);
    else if (dtype == BF_DT_F16)
        staged ? launch_partial<_Float16, true>(a, lds, st) : launch_partial<_Float16, false>(a, lds, st);
    else
        staged ? launch_partial<float, true>(a, lds, st) : launch_partial<float, false>(a, lds, st);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int bf_mc_predictive_finish(const void* d_partial, int64_t R, int64_t C, int S_total, const int64_t* d_labels,
                                       int64_t ignore_index, const bf_predictive_out_t* out, void* d_workspace,
                                       size_t workspace_bytes_, void* stream) {
    if (!d_partial || !out || !d_workspace) BF_FAIL("bf_mc_predictive_finish: NULL partial, out or workspace");
    if (R < 1 || C < 1 || C > INT32_MAX || S_total < 1 || S_total > kMaxSTotal)
        BF_FAIL("bf_mc_predictive_finish: bad R=%lld C=%lld S_total=%d", (long long)R, (long long)C, S_total);
    if (!out->d_probs || !out->d_predictive_entropy || !out->d_expected_entropy || !out->d_mutual_information ||
        !out->d_prediction)
        BF_FAIL("bf_mc_predictive_finish: NULL output");
    if (d_labels && (!out->d_log_likelihood || !out->d_correct_per_sample || !out->d_scalars || !out->d_counts))
        BF_FAIL("bf_mc_predictive_finish: labels given but a label output is NULL");
    if (workspace_bytes_ < workspace_bytes(S_total))
        BF_FAIL("bf_mc_predictive_finish: workspace too small (%zu < %zu bytes)", workspace_bytes_,
                workspace_bytes(S_total));
    const Layout L = layout_of(R, C, S_total, d_labels != nullptr);
    const unsigned char* P = static_cast<const unsigned char*>(d_partial);
    unsigned char* W = static_cast<unsigned char*>(d_workspace);
    FinishArgs a;
    a.sum_p = reinterpret_cast<const float*>(P + L.sum_p);
    a.sum_h = reinterpret_cast<const float*>(P + L.sum_h);
    a.sum_py = reinterpret_cast<const double*>(P + L.sum_py);
    a.counts = reinterpret_cast<const double*>(P + L.counts);
    a.R = R, a.C = C, a.S_total = S_total, a.labels = d_labels, a.ignore_index = ignore_index;
    a.out = *out;
    a.ticket = reinterpret_cast<uint32_t*>(W) + 1;
    a.slots = reinterpret_cast<double*>(W + kTicketBytes + slot_bytes(S_total));
    hipLaunchKernelGGL(predictive_finish_kernel, dim3(grid_for(R)), dim3(kThreads), 0, (hipStream_t)stream, a);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
