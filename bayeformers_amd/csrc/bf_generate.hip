// bf_generate.hip — the epilogue of one sample_generate step in one capturable launch: token choice (lowest-index argmax
// of the model-average probabilities, or an inverse-CDF draw of one Philox uniform), the eos / pad / finished / lengths
// bookkeeping, the writes into the sequences and the statistics, the next step's input ids and positions, and the step
// counter.  One 256-thread workgroup per prompt row; the step index lives on the device (d_state[0]), so one captured
// launch serves every step of a graph-replayed generation.
//
// The draw sums the row in a fixed order, so it is deterministic: the row is cut into tiles of 1024 probabilities, thread
// t holding elements 4t .. 4t + 3 of a tile.  Tile totals are wave sums (a fixed xor tree) added in wave order; the running
// total carry_k adds them in tile order.  With x = u * total the token is in the first tile k with a positive total and
// carry_k + total_k >= x, at the first element j with p_j > 0 and carry_k + cum_j >= x (cum_j: the tile's exclusive scan
// over threads plus the thread's own prefix), else — a rounding gap — the tile's last positive element.  A zero
// probability is never chosen; a row whose total is not positive (all zero, NaN) takes the argmax.
#include "bf_common.h"
#include "bf_philox.h"

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64, PER = 4, TILE = THREADS * PER;
constexpr int MAX_TILES = 512;  // V <= 524288

struct GenParams {
    const float* probs;
    const float* stat_probs;  // the row the token's probability statistic is read from (probs when NULL)
    const float* pe;
    const float* ee;
    const float* mi;
    int64_t* state;  // {step, arrivals}
    int64_t* seq;
    float* stats;
    uint8_t* finished;
    int64_t* lengths;
    int64_t* next_ids;
    int64_t* positions;
    const uint64_t* seed;
    int64_t B, V, n, seq_stride, T0, eos, pad;
    int S, do_sample;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
    return v;
}

__global__ __launch_bounds__(THREADS) void generate_step_kernel(const GenParams p) {
    __shared__ float tile_wave[MAX_TILES][WAVES];
    __shared__ float red_q[WAVES];
    __shared__ int64_t red_i[WAVES];
    __shared__ int64_t s_tok;
    __shared__ int s_tile;
    __shared__ float s_carry, s_x;
    __shared__ float scan_wave[WAVES];
    __shared__ int64_t s_pick[WAVES], s_last[WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x, V = p.V;
    const int64_t step = *p.state;
    if (step >= p.n) return;  // past the last step: nothing to write (and the counter stays)
    const float* row = p.probs + b * V;
    const float* stat_row = p.stat_probs ? p.stat_probs + b * V : row;
    const int tiles = (int)((V + TILE - 1) / TILE);

    // pass 1: argmax (first index of the largest value; NaN never wins) and the per-tile wave sums
    float best = -1.0f;
    int64_t bi = INT64_MAX;
    for (int k = 0; k < tiles; ++k) {
        float s = 0.0f;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int64_t c = (int64_t)k * TILE + tid * PER + e;
            const float q = c < V ? row[c] : 0.0f;
            if (q > best) best = q, bi = c;
            s += q;
        }
        if (p.do_sample) {
            s = wave_sum(s);
            if (lane == 0) tile_wave[k][wave] = s;
        }
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const float ob = __shfl_xor(best, k);
        const int64_t oi = __shfl_xor(bi, k);
        if (ob > best || (ob == best && oi < bi)) best = ob, bi = oi;
    }
    if (lane == 0) red_q[wave] = best, red_i[wave] = bi;
    __syncthreads();
    if (tid == 0) {
        float q = red_q[0];
        int64_t idx = red_i[0];
        for (int w = 1; w < WAVES; ++w)
            if (red_q[w] > q || (red_q[w] == q && red_i[w] < idx)) q = red_q[w], idx = red_i[w];
        s_tok = idx == INT64_MAX ? 0 : idx;
        s_tile = -1;
        if (p.do_sample) {
            float total = 0.0f;
            for (int k = 0; k < tiles; ++k) {
                float t = 0.0f;
                for (int w = 0; w < WAVES; ++w) t += tile_wave[k][w];
                total += t;
            }
            if (total > 0.0f) {  // (false for NaN)
                const uint64_t seed = *p.seed;
                const bf_u32x4 r = bf_philox4x32((uint32_t)b, (uint32_t)step, BF_GENERATE_STREAM, (uint32_t)(b >> 32),
                                                 (uint32_t)seed, (uint32_t)(seed >> 32));
                const float x = bf_u32_to_unit(r.x) * total;
                float carry = 0.0f;
                for (int k = 0; k < tiles; ++k) {
                    float t = 0.0f;
                    for (int w = 0; w < WAVES; ++w) t += tile_wave[k][w];
                    if (t > 0.0f && carry + t >= x) {
                        s_tile = k;
                        break;
                    }
                    carry += t;
                }
                s_carry = carry;
                s_x = x;
            }
        }
    }
    __syncthreads();

    // pass 2 (a draw): the chosen tile again, scanned
    const int k = s_tile;
    if (k >= 0) {
        float q[PER], cum[PER], s = 0.0f;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int64_t c = (int64_t)k * TILE + tid * PER + e;
            q[e] = c < V ? row[c] : 0.0f;
            cum[e] = s += q[e];  // the thread's inclusive prefix
        }
        float incl = s;  // inclusive scan over the wave (Hillis-Steele: a fixed order)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) scan_wave[wave] = incl;
        __syncthreads();
        float before = 0.0f;
        for (int w = 0; w < wave; ++w) before += scan_wave[w];
        const float excl = before + (incl - s);
        const float carry = s_carry, x = s_x;
        int64_t pick = INT64_MAX, last = -1;
#pragma unroll
        for (int e = PER - 1; e >= 0; --e) {
            const int64_t c = (int64_t)k * TILE + tid * PER + e;
            if (q[e] > 0.0f) {
                if (carry + (excl + cum[e]) >= x) pick = c;
                if (last < 0) last = c;
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            pick = min(pick, (int64_t)__shfl_xor(pick, d));
            last = max(last, (int64_t)__shfl_xor(last, d));
        }
        if (lane == 0) s_pick[wave] = pick, s_last[wave] = last;
        __syncthreads();
        if (tid == 0) {
            int64_t pk = INT64_MAX, ls = -1;
            for (int w = 0; w < WAVES; ++w) pk = min(pk, s_pick[w]), ls = max(ls, s_last[w]);
            s_tok = pk != INT64_MAX ? pk : ls;
        }
        __syncthreads();
    }

    // the bookkeeping of the eager loop; the token's ids for every sample
    const bool done = p.eos >= 0 && p.finished[b];
    const int64_t tok = done ? p.pad : s_tok;
    if (tid == 0) {
        const int64_t B = p.B, n = p.n;
        const float st[4] = {p.pe[b], p.ee[b], p.mi[b], stat_row[s_tok]};
        for (int i = 0; i < 4; ++i) p.stats[(i * B + b) * n + step] = done ? 0.0f : st[i];
        p.seq[b * p.seq_stride + p.T0 + step] = tok;
        if (p.eos >= 0) {
            if (!done) p.lengths[b] += 1;
            p.finished[b] = done || tok == p.eos;
        } else {
            p.lengths[b] += 1;
        }
    }
    for (int s = tid; s < p.S; s += THREADS) {
        p.next_ids[s * p.B + b] = tok;
        if (p.positions) p.positions[s * p.B + b] += 1;
    }
    // the last workgroup to arrive advances the step (every workgroup has read it by then)
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(reinterpret_cast<unsigned long long*>(p.state + 1), 1ull) == (unsigned long long)(p.B - 1)) {
            p.state[1] = 0;
            p.state[0] = step + 1;
            __threadfence();
        }
    }
}

}  // namespace

// bf_generate_step and bf_generate_step_stat_probs (d_stat_probs NULL: the statistics read d_probs)
static int generate_step(const float* d_probs, const float* d_stat_probs, const float* d_predictive_entropy,
                         const float* d_expected_entropy, const float* d_mutual_information, int64_t B, int64_t V, int S,
                         int64_t* d_state, int64_t max_new_tokens, int64_t* d_sequences, int64_t seq_stride, int64_t T0,
                         float* d_stats, uint8_t* d_finished, int64_t* d_lengths, int64_t* d_next_ids, int64_t* d_positions,
                         int64_t eos_token_id, int64_t pad_token_id, int do_sample, const uint64_t* d_seed,
                         hipStream_t stream) {
    const char* what = "bf_generate_step";
    if (B < 1 || B > 0x7fffffff || V < 1 || S < 1 || max_new_tokens < 1)
        BF_FAIL("%s: B=%lld, V=%lld, S=%d, max_new_tokens=%lld must be positive", what, (long long)B, (long long)V, S,
                (long long)max_new_tokens);
    if (V > (int64_t)MAX_TILES * TILE) BF_FAIL("%s: V=%lld exceeds %d", what, (long long)V, MAX_TILES * TILE);
    if (T0 < 0 || seq_stride < T0 + max_new_tokens)
        BF_FAIL("%s: a sequence row of %lld tokens does not hold T0=%lld + %lld", what, (long long)seq_stride,
                (long long)T0, (long long)max_new_tokens);
    if (!d_probs || !d_predictive_entropy || !d_expected_entropy || !d_mutual_information || !d_state || !d_sequences ||
        !d_stats || !d_lengths || !d_next_ids)
        BF_FAIL("%s: NULL argument", what);
    if (eos_token_id >= 0 && !d_finished) BF_FAIL("%s: an eos token needs the finished flags", what);
    if (do_sample && !d_seed) BF_FAIL("%s: sampling needs a device seed", what);
    if (((uintptr_t)d_state | (uintptr_t)d_sequences | (uintptr_t)d_lengths | (uintptr_t)d_next_ids |
         (uintptr_t)d_positions | (uintptr_t)d_seed) & 7)
        BF_FAIL("%s: int64 arguments must be 8-byte aligned", what);
    GenParams p = {};
    p.probs = d_probs;
    p.stat_probs = d_stat_probs;
    p.pe = d_predictive_entropy;
    p.ee = d_expected_entropy;
    p.mi = d_mutual_information;
    p.state = d_state;
    p.seq = d_sequences;
    p.stats = d_stats;
    p.finished = d_finished;
    p.lengths = d_lengths;
    p.next_ids = d_next_ids;
    p.positions = d_positions;
    p.seed = d_seed;
    p.B = B;
    p.V = V;
    p.n = max_new_tokens;
    p.seq_stride = seq_stride;
    p.T0 = T0;
    p.eos = eos_token_id;
    p.pad = pad_token_id;
    p.S = S;
    p.do_sample = do_sample ? 1 : 0;
    generate_step_kernel<<<(unsigned)B, THREADS, 0, stream>>>(p);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_generate_step(const float* d_probs, const float* d_predictive_entropy, const float* d_expected_entropy,
                     const float* d_mutual_information, int64_t B, int64_t V, int S, int64_t* d_state,
                     int64_t max_new_tokens, int64_t* d_sequences, int64_t seq_stride, int64_t T0, float* d_stats,
                     uint8_t* d_finished, int64_t* d_lengths, int64_t* d_next_ids, int64_t* d_positions,
                     int64_t eos_token_id, int64_t pad_token_id, int do_sample, const uint64_t* d_seed, void* stream) {
    return generate_step(d_probs, nullptr, d_predictive_entropy, d_expected_entropy, d_mutual_information, B, V, S, d_state,
                         max_new_tokens, d_sequences, seq_stride, T0, d_stats, d_finished, d_lengths, d_next_ids, d_positions,
                         eos_token_id, pad_token_id, do_sample, d_seed, (hipStream_t)stream);
}

int bf_generate_step_stat_probs(const float* d_probs, const float* d_stat_probs, const float* d_predictive_entropy,
                                const float* d_expected_entropy, const float* d_mutual_information, int64_t B, int64_t V,
                                int S, int64_t* d_state, int64_t max_new_tokens, int64_t* d_sequences,
                                int64_t seq_stride, int64_t T0, float* d_stats, uint8_t* d_finished, int64_t* d_lengths,
                                int64_t* d_next_ids, int64_t* d_positions, int64_t eos_token_id, int64_t pad_token_id,
                                int do_sample, const uint64_t* d_seed, void* stream) {
    if (!d_stat_probs) BF_FAIL("bf_generate_step_stat_probs: NULL argument");
    return generate_step(d_probs, d_stat_probs, d_predictive_entropy, d_expected_entropy, d_mutual_information, B, V, S,
                         d_state, max_new_tokens, d_sequences, seq_stride, T0, d_stats, d_finished, d_lengths, d_next_ids,
                         d_positions, eos_token_id, pad_token_id, do_sample, d_seed, (hipStream_t)stream);
}

// ---- bf_probs_truncate: top-k / top-p / min-p on the model-average rows ---------------------------------------------
// One 1024-thread workgroup per row; no state between launches and no grid-wide synchronisation.  Every criterion is a
// threshold on the value, found by a radix select over the key of a probability: its fp32 bit pattern (which orders
// non-negative floats), 0 for p <= 0.  A select takes three digit passes over the row (key bits 30..20, 19..9, 8..0), each
// a histogram in LDS of the elements whose higher digits match the prefix chosen so far: counts (top-k) or the fixed-point
// mass q = floor(p * 2^(40 - E)) (top-p), all integer adds, so no sum depends on the order threads arrive in.  The first
// pass also takes the row's largest key and its non-finite check and counts the top-k's first digit; the last pass
// writes the row.  After the first, the row is re-read from L2.
namespace {

constexpr int TR_THREADS = 1024, TR_WAVES = TR_THREADS / 64, TR_BINS = 2048;
constexpr int TR_SHIFT[3] = {20, 9, 0}, TR_WIDTH[3] = {11, 11, 9};

struct TruncParams {
    const float* probs;
    float* out;
    int64_t V, top_k;
    float top_p, min_p;
};

__device__ __forceinline__ uint32_t prob_key(float p) {
    const uint32_t u = __float_as_uint(p);
    return (u >> 31) ? 0u : u;  // negative values and -0 are 0, like +0
}

// f(index, value, valid) for every element of the row; every thread runs the same number of iterations (the tail is
// `valid = false`), so whole waves reach the wave-wide votes inside f
template <bool VEC, typename F>
__device__ __forceinline__ void for_row(const float* row, int V, F&& f) {
    if constexpr (VEC) {
        const int n4 = V >> 2, iters = (n4 + TR_THREADS - 1) / TR_THREADS;
        for (int it = 0; it < iters; ++it) {
            const int i = it * TR_THREADS + (int)threadIdx.x;
            const bool ok = i < n4;
            const float4 v = ok ? reinterpret_cast<const float4*>(row)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            f(4 * i, v.x, ok);
            f(4 * i + 1, v.y, ok);
            f(4 * i + 2, v.z, ok);
            f(4 * i + 3, v.w, ok);
        }
    } else {
        const int iters = (V + TR_THREADS - 1) / TR_THREADS;
        for (int it = 0; it < iters; ++it) {
            const int i = it * TR_THREADS + (int)threadIdx.x;
            const bool ok = i < V;
            f(i, ok ? row[i] : 0.0f, ok);
        }
    }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
    return v;
}

// adds (1, or q) at bin (-1: nothing).  A wave whose lanes all hit one bin (flat or quantised rows) adds once.
template <bool MASS>
__device__ __forceinline__ void hist_add(int bin, unsigned long long q, uint32_t* cnt, unsigned long long* mass) {
    const int b0 = __builtin_amdgcn_readfirstlane(bin);
    if (__all(bin == b0)) {
        if (b0 < 0) return;
        if constexpr (MASS) {
            q = wave_sum_u64(q);
            if ((threadIdx.x & 63) == 0) atomicAdd(&mass[b0], q);
        } else {
            if ((threadIdx.x & 63) == 0) atomicAdd(&cnt[b0], 64u);
        }
    } else if (bin >= 0) {
        if constexpr (MASS) atomicAdd(&mass[bin], q);
        else atomicAdd(&cnt[bin], 1u);
    }
}

// The bin of `hist` [nbins] where the running sum from the top bin down first reaches need(total): *s_bin, and the sum of
// the bins above it *s_above (total = the sum of every bin).  Thread t holds bins 2t, 2t + 1; a suffix scan over threads.
template <typename T, typename Need>
__device__ __forceinline__ void find_bin(const T* hist, int nbins, Need need_of, T* s_wave, int* s_bin, T* s_above) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = min(2 * tid, nbins), hi = min(2 * tid + 2, nbins);
    T s = 0;
    for (int i = lo; i < hi; ++i) s += hist[i];
    T incl = s;  // sum over this wave's lanes >= lane (a fixed order)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_down(incl, d);
        if (lane + d < 64) incl += o;
    }
    if (lane == 0) s_wave[wave] = incl;
    __syncthreads();
    T above = incl - s, total = 0;
    for (int w = 0; w < TR_WAVES; ++w) {
        total += s_wave[w];
        if (w > wave) above += s_wave[w];
    }
    const T need = need_of(total);
    for (int i = hi - 1; i >= lo; --i) {
        if (above < need && above + hist[i] >= need) *s_bin = i, *s_above = above;
        above += hist[i];
    }
    __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(TR_THREADS) void probs_truncate_kernel(const TruncParams p) {
    __shared__ uint32_t cnt[TR_BINS];
    __shared__ unsigned long long mass[TR_BINS];
    __shared__ uint32_t s_wave_u[TR_WAVES];
    __shared__ unsigned long long s_wave_q[TR_WAVES];
    __shared__ uint32_t s_max[TR_WAVES], s_bad[TR_WAVES];
    __shared__ int s_bin;
    __shared__ uint32_t s_above_u;
    __shared__ unsigned long long s_above_q;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = (int)p.V;
    const float* row = p.probs + (int64_t)blockIdx.x * V;
    float* out = p.out + (int64_t)blockIdx.x * V;
    const bool topk = p.top_k > 0 && p.top_k < p.V, topp = p.top_p < 1.0f, minp = p.min_p > 0.0f;

    // pass 1: the largest key, a NaN / infinity anywhere, the top-k's first-digit counts
    if (topk)
        for (int i = tid; i < TR_BINS; i += TR_THREADS) cnt[i] = 0;
    __syncthreads();
    uint32_t kmax = 0, bad = 0;
    for_row<VEC>(row, V, [&](int, float v, bool ok) {
        const uint32_t u = __float_as_uint(v), key = prob_key(v);
        bad |= ok && (u & 0x7f800000u) == 0x7f800000u;
        kmax = max(kmax, key);
        if (topk) hist_add<false>(ok && key > 0 ? (int)(key >> TR_SHIFT[0]) : -1, 0, cnt, mass);
    });
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor(kmax, k)), bad |= (uint32_t)__shfl_xor(bad, k);
    if (lane == 0) s_max[wave] = kmax, s_bad[wave] = bad;
    __syncthreads();
    for (int w = 0; w < TR_WAVES; ++w) kmax = max(kmax, s_max[w]), bad |= s_bad[w];
    if (bad || kmax == 0) {  // copied through (the whole workgroup takes this branch)
        if (out != row)
            for_row<false>(row, V, [&](int i, float v, bool ok) {
                if (ok) out[i] = v;
            });
        return;
    }

    uint32_t thr = 1;  // keep key >= thr (p > 0)
    if (topk) {  // the top_k-th largest key: three digits of counts
        uint32_t prefix = 0, need = (uint32_t)p.top_k;
        bool all = false;
        for (int lvl = 0; lvl < 3 && !all; ++lvl) {
            if (lvl > 0) {
                for (int i = tid; i < TR_BINS; i += TR_THREADS) cnt[i] = 0;
                __syncthreads();
                const int up = TR_SHIFT[lvl] + TR_WIDTH[lvl], sh = TR_SHIFT[lvl], m = (1 << TR_WIDTH[lvl]) - 1;
                for_row<VEC>(row, V, [&](int, float v, bool ok) {
                    const uint32_t key = prob_key(v);
                    hist_add<false>(ok && key > 0 && (key >> up) == prefix ? (int)((key >> sh) & m) : -1, 0, cnt, mass);
                });
                __syncthreads();
            }
            uint32_t total0 = 0;
            find_bin(cnt, 1 << TR_WIDTH[lvl], [&](uint32_t total) {
                total0 = total;
                return min(need, total);
            }, s_wave_u, &s_bin, &s_above_u);
            if (lvl == 0 && need >= total0) all = true;  // k >= the positive entries: every one of them
            need -= s_above_u;
            prefix = (prefix << TR_WIDTH[lvl]) | (uint32_t)s_bin;
        }
        if (!all) thr = prefix;
    }
    if (topp) {  // the largest key t with mass(key >= t) >= top_p * mass(key >= thr): three digits of fixed-point mass
        int e2;
        const float fr = frexpf(__uint_as_float(kmax), &e2);
        const int sexp = 40 - (fr == 0.5f ? e2 - 1 : e2);  // max p * 2^sexp in (2^39, 2^40]
        const uint32_t lo = thr;
        uint32_t prefix = 0;
        unsigned long long need = 0;
        for (int lvl = 0; lvl < 3; ++lvl) {
            for (int i = tid; i < TR_BINS; i += TR_THREADS) mass[i] = 0;
            __syncthreads();
            const int up = TR_SHIFT[lvl] + TR_WIDTH[lvl], sh = TR_SHIFT[lvl], m = (1 << TR_WIDTH[lvl]) - 1;
            for_row<VEC>(row, V, [&](int, float v, bool ok) {
                const uint32_t key = prob_key(v);
                const bool in = ok && key >= lo && (key >> up) == prefix;
                hist_add<true>(in ? (int)((key >> sh) & m) : -1,
                               in ? (unsigned long long)ldexpf(v, sexp) : 0ull, cnt, mass);
            });
            __syncthreads();
            find_bin(mass, 1 << TR_WIDTH[lvl], [&](unsigned long long total) {
                if (lvl == 0) {
                    need = (unsigned long long)ceil((double)p.top_p * (double)total);
                    need = need < 1 ? 1 : (need > total ? total : need);
                }
                return need;
            }, s_wave_q, &s_bin, &s_above_q);
            need -= s_above_q;
            prefix = (prefix << TR_WIDTH[lvl]) | (uint32_t)s_bin;
        }
        thr = max(thr, prefix);
    }
    if (minp) thr = max(thr, prob_key(__fmul_rn(p.min_p, __uint_as_float(kmax))));
    thr = min(thr, kmax);  // the argmax always stays

    if constexpr (VEC) {
        const int n4 = V >> 2;
        for (int i = tid; i < n4; i += TR_THREADS) {
            float4 v = reinterpret_cast<const float4*>(row)[i];
            v.x = prob_key(v.x) >= thr ? v.x : 0.0f;
            v.y = prob_key(v.y) >= thr ? v.y : 0.0f;
            v.z = prob_key(v.z) >= thr ? v.z : 0.0f;
            v.w = prob_key(v.w) >= thr ? v.w : 0.0f;
            reinterpret_cast<float4*>(out)[i] = v;
        }
    } else {
        for (int i = tid; i < V; i += TR_THREADS) {
            const float v = row[i];
            out[i] = prob_key(v) >= thr ? v : 0.0f;
        }
    }
}

}  // namespace

int bf_probs_truncate(const float* d_probs, float* d_out, int64_t R, int64_t V, int64_t top_k, float top_p,
                      float min_p, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* what = "bf_probs_truncate";
    if (R < 1 || R > 65535 || V < 1 || V > (int64_t)MAX_TILES * TILE)
        BF_FAIL("%s: R=%lld must be in [1, 65535] and V=%lld in [1, %d]", what, (long long)R, (long long)V,
                MAX_TILES * TILE);
    if (!d_probs || !d_out) BF_FAIL("%s: NULL argument", what);
    if (!(top_p > 0.0f)) BF_FAIL("%s: top_p=%g must be positive (>= 1: off)", what, (double)top_p);
    if (!(min_p <= 1.0f)) BF_FAIL("%s: min_p=%g must be at most 1 (<= 0: off)", what, (double)min_p);
    const uintptr_t a = (uintptr_t)d_probs, b = (uintptr_t)d_out, n = (uintptr_t)(R * V) * sizeof(float);
    if (a != b && a < b + n && b < a + n) BF_FAIL("%s: d_out overlaps d_probs without being it", what);
    if ((a | b) & 3) BF_FAIL("%s: rows must be 4-byte aligned", what);
    TruncParams p = {d_probs, d_out, V, top_k, top_p, min_p};
    if (V % 4 == 0 && ((a | b) & 15) == 0)
        probs_truncate_kernel<true><<<(unsigned)R, TR_THREADS, 0, stream>>>(p);
    else
        probs_truncate_kernel<false><<<(unsigned)R, TR_THREADS, 0, stream>>>(p);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- bf_logits_process: repetition penalty, no-repeat n-grams, min_new_tokens, temperature --------------------------
// A grid of (2048-column chunk, batch row b).  Each workgroup first scans row b's L tokens (from L2) into two LDS bitmaps
// over its chunk: "seen" (the token occurs) and "banned" (the token completes a window whose first n - 1 tokens equal the
// row's last n - 1).  The bits are set with LDS atomicOr, which does not depend on the order threads arrive in.  Then it
// streams its chunk of the S sample rows of b (rows s * B + b): thread t owns columns 8t .. 8t + 7 of the chunk, read as
// one 16-byte load per bf16 / fp16 row (two for fp32) and written as two float4.
namespace {

constexpr int LP_THREADS = 256, LP_PER = 8, LP_CHUNK = LP_THREADS * LP_PER, LP_WORDS = LP_CHUNK / 32;
constexpr int LP_MAX_NGRAM = 64;
constexpr int64_t LP_MAX_V = 524288;

struct ProcParams {
    const void* logits;
    float* out;
    const int64_t* seq;
    const int64_t* d_step;
    int64_t row_stride, seq_stride, T0, step, eos, m;
    int V, B, S, n;
    float theta, T;
};

__device__ __forceinline__ float lp_f32(float v) { return v; }
__device__ __forceinline__ float lp_f32(__bf16 v) { return (float)v; }
__device__ __forceinline__ float lp_f32(_Float16 v) { return (float)v; }

template <typename T, bool VEC>
__global__ __launch_bounds__(LP_THREADS) void logits_process_kernel(const ProcParams p) {
    __shared__ uint32_t seen[LP_WORDS], banned[LP_WORDS];
    __shared__ int64_t prefix[LP_MAX_NGRAM];

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y, c0 = (int64_t)blockIdx.x * LP_CHUNK, V = p.V;
    const int64_t step = p.d_step ? *p.d_step : p.step;
    const int64_t L = min(max(p.T0 + step, (int64_t)0), p.seq_stride);  // the history: seq[0, L)
    const int64_t* seq = p.seq + b * p.seq_stride;
    const bool pen = p.theta != 1.0f;
    const int n = L >= p.n ? p.n : 0;  // no complete n-gram yet: nothing to ban
    if (tid < LP_WORDS) seen[tid] = 0u, banned[tid] = 0u;
    for (int j = tid; j < n - 1; j += LP_THREADS) prefix[j] = seq[L - n + 1 + j];
    __syncthreads();
    if (pen || n > 0) {
        for (int64_t i = tid; i < L; i += LP_THREADS) {
            const int64_t id = seq[i];
            if (id < c0 || id >= c0 + LP_CHUNK || id >= V) continue;  // c0 >= 0: ids < 0 are out too
            const int c = (int)(id - c0);
            const uint32_t bit = 1u << (c & 31);
            if (pen) atomicOr(&seen[c >> 5], bit);
            if (n > 0 && i >= n - 1) {  // the window seq[i - n + 1 .. i] ends with id: banned if it starts with the prefix
                bool match = true;
                for (int j = 0; j < n - 1 && match; ++j) match = seq[i - n + 1 + j] == prefix[j];
                if (match) atomicOr(&banned[c >> 5], bit);
            }
        }
    }
    __syncthreads();

    const int64_t col = c0 + LP_PER * tid;
    if (col >= V) return;
    const int sh = LP_PER * (tid & 3);
    const uint32_t sb = (seen[tid >> 2] >> sh) & 0xffu;
    uint32_t bb = (banned[tid >> 2] >> sh) & 0xffu;
    if (step < p.m && p.eos >= col && p.eos < col + LP_PER) bb |= 1u << (int)(p.eos - col);  // eos < V: host-checked
    const bool full = col + LP_PER <= V;
    for (int s = 0; s < p.S; ++s) {
        const int64_t r = (int64_t)s * p.B + b;
        const T* row = reinterpret_cast<const T*>(p.logits) + r * p.row_stride + col;
        float* out = p.out + r * V + col;
        float v[LP_PER];
        if (VEC && full) {
            if constexpr (sizeof(T) == 2) {
                const uint4 u = *reinterpret_cast<const uint4*>(row);
                const T* h = reinterpret_cast<const T*>(&u);
#pragma unroll
                for (int e = 0; e < LP_PER; ++e) v[e] = lp_f32(h[e]);
            } else {
                const float4 a = reinterpret_cast<const float4*>(row)[0], c = reinterpret_cast<const float4*>(row)[1];
                v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = c.x, v[5] = c.y, v[6] = c.z, v[7] = c.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < LP_PER; ++e) v[e] = col + e < V ? lp_f32(row[e]) : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < LP_PER; ++e) {
            float x = v[e];
            if ((sb >> e) & 1u) x = x < 0.0f ? __fmul_rn(x, p.theta) : __fdiv_rn(x, p.theta);
            if ((bb >> e) & 1u) x = -INFINITY;
            v[e] = p.T != 1.0f ? __fdiv_rn(x, p.T) : x;
        }
        if (VEC && full) {
            reinterpret_cast<float4*>(out)[0] = make_float4(v[0], v[1], v[2], v[3]);
            reinterpret_cast<float4*>(out)[1] = make_float4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
            for (int e = 0; e < LP_PER; ++e)
                if (col + e < V) out[e] = v[e];
        }
    }
}

template <typename T>
void launch_logits_process(const ProcParams& p, bool vec, dim3 grid, hipStream_t stream) {
    if (vec)
        logits_process_kernel<T, true><<<grid, LP_THREADS, 0, stream>>>(p);
    else
        logits_process_kernel<T, false><<<grid, LP_THREADS, 0, stream>>>(p);
}

}  // namespace

int bf_logits_process(const void* d_logits, int dtype, int64_t R, int64_t V, int64_t row_stride, float* d_out,
                      const int64_t* d_sequences, int64_t B, int64_t seq_stride, int64_t T0, const int64_t* d_step,
                      int64_t step, float repetition_penalty, int64_t no_repeat_ngram_size, int64_t min_new_tokens,
                      int64_t eos_token_id, float temperature, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* what = "bf_logits_process";
    if (dtype != BF_DT_F32 && dtype != BF_DT_BF16 && dtype != BF_DT_F16) BF_FAIL("%s: dtype=%d is not a BF_DT_*", what, dtype);
    if (B < 1 || B > 65535 || R < B || R % B != 0 || R / B > 0x7fffffff)
        BF_FAIL("%s: R=%lld must be a positive multiple of B=%lld (B in [1, 65535])", what, (long long)R, (long long)B);
    if (V < 1 || V > LP_MAX_V) BF_FAIL("%s: V=%lld must be in [1, %lld]", what, (long long)V, (long long)LP_MAX_V);
    if (row_stride < V) BF_FAIL("%s: row_stride=%lld is shorter than V=%lld", what, (long long)row_stride, (long long)V);
    if (T0 < 0 || seq_stride < 1 || (!d_step && (step < 0 || T0 + step > seq_stride)))
        BF_FAIL("%s: a sequence row of %lld tokens does not hold T0=%lld + step=%lld", what, (long long)seq_stride,
                (long long)T0, (long long)step);
    if (!d_logits || !d_out || !d_sequences) BF_FAIL("%s: NULL argument", what);
    if (!(repetition_penalty > 0.0f) || !isfinite(repetition_penalty))
        BF_FAIL("%s: repetition_penalty=%g must be finite and positive", what, (double)repetition_penalty);
    if (no_repeat_ngram_size < 0 || no_repeat_ngram_size > LP_MAX_NGRAM)
        BF_FAIL("%s: no_repeat_ngram_size=%lld must be in [0, %d]", what, (long long)no_repeat_ngram_size, LP_MAX_NGRAM);
    if (min_new_tokens < 0) BF_FAIL("%s: min_new_tokens=%lld must be non-negative", what, (long long)min_new_tokens);
    if (min_new_tokens > 0 && (eos_token_id < 0 || eos_token_id >= V))
        BF_FAIL("%s: min_new_tokens needs an eos_token_id in [0, V) (got %lld)", what, (long long)eos_token_id);
    if (!(temperature > 0.0f) || !isfinite(temperature))
        BF_FAIL("%s: temperature=%g must be finite and positive", what, (double)temperature);
    const size_t esz = bf_dtype_size(dtype);
    const uintptr_t a = (uintptr_t)d_logits, o = (uintptr_t)d_out;
    if ((a & (esz - 1)) || (o & 3)) BF_FAIL("%s: logits must be aligned to their element and d_out to 4 bytes", what);
    if (((uintptr_t)d_sequences | (uintptr_t)d_step) & 7) BF_FAIL("%s: int64 arguments must be 8-byte aligned", what);
    const uintptr_t in_end = a + (uintptr_t)((R - 1) * row_stride + V) * esz, out_end = o + (uintptr_t)(R * V) * 4;
    if (a < out_end && o < in_end) BF_FAIL("%s: d_out overlaps the logits", what);
    ProcParams p = {};
    p.logits = d_logits;
    p.out = d_out;
    p.seq = d_sequences;
    p.d_step = d_step;
    p.row_stride = row_stride;
    p.seq_stride = seq_stride;
    p.T0 = T0;
    p.step = step;
    p.eos = min_new_tokens > 0 ? eos_token_id : -1;
    p.m = min_new_tokens;
    p.V = (int)V;
    p.B = (int)B;
    p.S = (int)(R / B);
    p.n = (int)no_repeat_ngram_size;
    p.theta = repetition_penalty;
    p.T = temperature;
    const bool vec = (a & 15) == 0 && ((uintptr_t)row_stride * esz & 15) == 0 && (o & 15) == 0 && V % 4 == 0;
    const dim3 grid((unsigned)((V + LP_CHUNK - 1) / LP_CHUNK), (unsigned)B);
    if (dtype == BF_DT_F32)
        launch_logits_process<float>(p, vec, grid, stream);
    else if (dtype == BF_DT_BF16)
        launch_logits_process<__bf16>(p, vec, grid, stream);
    else
        launch_logits_process<_Float16>(p, vec, grid, stream);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- bf_spec_accept: the epilogue of one speculative iteration ------------------------------------------------------
// One workgroup.  Thread b < B counts row b's leading agreements and, once the common run length a is known, walks its
// a + 1 kept positions (the eos / pad / finished / lengths rules of generate_step_kernel, one gather per kept token);
// then every thread helps to write the next iteration's ids and to advance the positions.  B * (gamma + 1) <= 16 rows of
// scalars: nothing here is worth more than one workgroup, and with one there is no arrival count to keep.
namespace {

constexpr int SPEC_THREADS = 256, SPEC_MAX_ROWS = 16;

struct SpecParams {
    const int64_t* argmax;  // [B][G + 1]
    const int64_t* draft;   // [B][G]
    const float* probs;     // [B * (G + 1)][V]
    const float* pe;
    const float* ee;
    const float* mi;
    int64_t* state;  // {step, 0}
    int64_t* seq;
    float* stats;
    uint8_t* finished;
    int64_t* lengths;
    int64_t* verify_ids;  // [S * B][G + 1]: column 0
    int64_t* verify_pos;  // [S * B][G + 1]
    int64_t* draft_ids;   // [B][2]
    int64_t* draft_pos;   // [B][G + 1]
    int64_t* rewind;
    int64_t* speculation;  // {verify steps, drafts proposed, drafts accepted}
    int64_t B, G, V, n, seq_stride, T0, eos, pad;
    int S;
};

__global__ __launch_bounds__(SPEC_THREADS) void spec_accept_kernel(const SpecParams p) {
    __shared__ int s_run[SPEC_MAX_ROWS];
    __shared__ int64_t s_last[SPEC_MAX_ROWS];

    const int tid = threadIdx.x;
    const int64_t B = p.B, G = p.G, V = p.V, n = p.n;
    const int64_t step = *p.state;
    if (step >= n) {  // past the last token: the forwards of this iteration still moved both fills by G + 1
        if (tid == 0) *p.rewind = G + 1;
        return;
    }
    if (tid < B) {
        const int64_t b = tid;
        int run = (int)G;
        if (!(p.eos >= 0 && p.finished[b])) {
            run = 0;
            while (run < G && p.draft[b * G + run] == p.argmax[b * (G + 1) + run]) ++run;
        }
        s_run[tid] = run;
        s_last[tid] = p.verify_ids[b * (G + 1)];  // the token the verify forward was fed first (sample 0's row)
    }
    __syncthreads();
    int64_t room = n - step - 1;  // drafts that still fit in front of the iteration's own token
    room = room < G ? room : G;
    int64_t a = room;
    for (int b = 0; b < B; ++b) a = s_run[b] < a ? s_run[b] : a;
    __syncthreads();

    if (tid < B) {
        const int64_t b = tid;
        bool done = p.eos >= 0 && p.finished[b];
        int64_t len = p.lengths[b], tok = s_last[tid], before = tok;
        for (int64_t j = 0; j <= a; ++j) {
            const int64_t r = b * (G + 1) + j;
            before = tok;
            tok = done ? p.pad : (j < a ? p.draft[b * G + j] : p.argmax[r]);
            const bool in = tok >= 0 && tok < V;
            const float st[4] = {p.pe[r], p.ee[r], p.mi[r], in ? p.probs[r * V + tok] : 0.0f};
            for (int i = 0; i < 4; ++i) p.stats[(i * B + b) * n + step + j] = done ? 0.0f : st[i];
            p.seq[b * p.seq_stride + p.T0 + step + j] = tok;
            if (!done) len += 1;
            if (p.eos >= 0) done = done || tok == p.eos;
        }
        p.lengths[b] = len;
        if (p.eos >= 0) p.finished[b] = done;
        p.draft_ids[2 * b] = before;
        p.draft_ids[2 * b + 1] = tok;
        s_last[tid] = tok;
    }
    __syncthreads();
    const int64_t rows = (int64_t)p.S * B;
    for (int64_t i = tid; i < rows; i += SPEC_THREADS) p.verify_ids[i * (G + 1)] = s_last[i % B];
    if (p.verify_pos)
        for (int64_t i = tid; i < rows * (G + 1); i += SPEC_THREADS) p.verify_pos[i] += a + 1;
    if (p.draft_pos)
        for (int64_t i = tid; i < B * (G + 1); i += SPEC_THREADS) p.draft_pos[i] += a + 1;
    if (tid == 0) {
        p.state[0] = step + a + 1;
        *p.rewind = G - a;
        p.speculation[0] += 1;
        p.speculation[1] += room;
        p.speculation[2] += a;
    }
}

}  // namespace

int bf_spec_accept(const int64_t* d_argmax, const int64_t* d_draft, const float* d_probs,
                   const float* d_predictive_entropy, const float* d_expected_entropy, const float* d_mutual_information,
                   int64_t B, int64_t gamma, int64_t V, int S, int64_t* d_state, int64_t max_new_tokens,
                   int64_t* d_sequences, int64_t seq_stride, int64_t T0, float* d_stats, uint8_t* d_finished,
                   int64_t* d_lengths, int64_t* d_verify_ids, int64_t* d_verify_positions, int64_t* d_draft_ids,
                   int64_t* d_draft_positions, int64_t* d_rewind, int64_t* d_speculation, int64_t eos_token_id,
                   int64_t pad_token_id, void* stream) {
    const char* what = "bf_spec_accept";
    if (B < 1 || gamma < 1 || B * (gamma + 1) > SPEC_MAX_ROWS)
        BF_FAIL("%s: B=%lld rows of gamma=%lld + 1 positions must be at least 1 x 2 and at most %d in all", what,
                (long long)B, (long long)gamma, SPEC_MAX_ROWS);
    if (V < 1 || S < 1 || max_new_tokens < 1)
        BF_FAIL("%s: V=%lld, S=%d, max_new_tokens=%lld must be positive", what, (long long)V, S, (long long)max_new_tokens);
    if (T0 < 0 || seq_stride < T0 + max_new_tokens)
        BF_FAIL("%s: a sequence row of %lld tokens does not hold T0=%lld + %lld", what, (long long)seq_stride,
                (long long)T0, (long long)max_new_tokens);
    if (!d_argmax || !d_draft || !d_probs || !d_predictive_entropy || !d_expected_entropy || !d_mutual_information ||
        !d_state || !d_sequences || !d_stats || !d_lengths || !d_verify_ids || !d_draft_ids || !d_rewind || !d_speculation)
        BF_FAIL("%s: NULL argument", what);
    if (eos_token_id >= 0 && !d_finished) BF_FAIL("%s: an eos token needs the finished flags", what);
    if (((uintptr_t)d_argmax | (uintptr_t)d_draft | (uintptr_t)d_state | (uintptr_t)d_sequences | (uintptr_t)d_lengths |
         (uintptr_t)d_verify_ids | (uintptr_t)d_verify_positions | (uintptr_t)d_draft_ids | (uintptr_t)d_draft_positions |
         (uintptr_t)d_rewind | (uintptr_t)d_speculation) & 7)
        BF_FAIL("%s: int64 arguments must be 8-byte aligned", what);
    SpecParams p = {};
    p.argmax = d_argmax;
    p.draft = d_draft;
    p.probs = d_probs;
    p.pe = d_predictive_entropy;
    p.ee = d_expected_entropy;
    p.mi = d_mutual_information;
    p.state = d_state;
    p.seq = d_sequences;
    p.stats = d_stats;
    p.finished = d_finished;
    p.lengths = d_lengths;
    p.verify_ids = d_verify_ids;
    p.verify_pos = d_verify_positions;
    p.draft_ids = d_draft_ids;
    p.draft_pos = d_draft_positions;
    p.rewind = d_rewind;
    p.speculation = d_speculation;
    p.B = B;
    p.G = gamma;
    p.V = V;
    p.n = max_new_tokens;
    p.seq_stride = seq_stride;
    p.T0 = T0;
    p.eos = eos_token_id;
    p.pad = pad_token_id;
    p.S = S;
    spec_accept_kernel<<<1, SPEC_THREADS, 0, (hipStream_t)stream>>>(p);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
