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
        const float st[4] = {p.pe[b], p.ee[b], p.mi[b], row[s_tok]};
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

int bf_launch_generate_step(const float* d_probs, const float* d_predictive_entropy, const float* d_expected_entropy,
                            const float* d_mutual_information, int64_t B, int64_t V, int S, int64_t* d_state,
                            int64_t max_new_tokens, int64_t* d_sequences, int64_t seq_stride, int64_t T0, float* d_stats,
                            uint8_t* d_finished, int64_t* d_lengths, int64_t* d_next_ids, int64_t* d_positions,
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
