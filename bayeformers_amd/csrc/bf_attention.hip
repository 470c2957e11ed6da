// bf_attention.hip — softmax(Q K^T * scale + mask) V for the attention block that sits between the Bayesian
// query/key/value projections and the Bayesian output projection of the transformers the reference converts
// (HF BertSelfAttention around bnn.Linear.forward; the reference itself runs whatever the wrapped model runs).
//
// Shape of the kernel (head size 64, keys/queries in tiles of 128, bf16 or fp16; fragment layouts and LDS images:
// bf_attention_tiles.h):
//   * one 256-thread workgroup per (128 queries, head, sequence); each of its 4 waves owns 32 queries;
//   * a 128-key tile of K (swizzled image) and of V (padded image) is staged in LDS with 16-byte accesses;
//   * S^T = K Q^T with K as the row operand, the softmax statistics of a query in-lane + two cross-lane steps, the
//     probabilities of two neighbouring key blocks the column operand of O^T = V^T P^T, V^T through the LDS transpose read;
//   * O^T accumulates in fp32; longer sequences walk the key tiles with the usual running max / sum rescale;
//   * a lane owns 4 consecutive features of one query at the end: 8-byte stores into the [B, T, H, 64] output.
// Algorithmic HBM bytes: (3 reads + 1 write) * B*T*H*64 * 2 B.
#include "bf_attention_tiles.h"
#include "bf_philox.h"
#include "../../include/bayeformers_amd_encoder_any.h"

namespace {

// The attention output rows (the x of the attention-out GEMM that runs next) leave through plain stores: nontemporal, sc1 and
// sc0 sc1 (write-through) stores were measured in the BERT-base step, one box, interleaved runs
// (profiles/r5e_gemm_variants_in_step_ab.txt): no policy beats plain stores.
template <typename V>
__device__ __forceinline__ void attn_st8(V* p, V v) { *p = v; }

constexpr int HD = 64;          // head size
constexpr int TQ = 128;         // queries per workgroup
constexpr int TKEY = 128;       // keys per tile
constexpr int K_BYTES = TKEY * Rows<HD>::SWZ;  // 16 KiB
constexpr int V_BYTES = TKEY * Rows<HD>::PAD;  // 20 KiB

struct AttnParams {
    const void* q;
    const void* k;
    const void* v;
    const float* mask;  // [B][T] additive, nullable
    const unsigned char* mask_off;  // nullable device flag: non-zero = the mask is all zeros, skip it
    void* out;
    float* lse;  // nullable: [B][H][T] log2-sum-exp2 of the scaled, masked scores (for the backward kernels)
    long long tok_stride;  // elements between consecutive tokens of q / k / v (H * 64 for packed heads)
    int B, T, H;
    float scale_log2e;  // scaling * log2(e)
    // DROP instantiation (training, HF attention_probs_dropout): the probabilities are dropped AFTER the softmax
    // normalisation (the row sums keep every term) with the Philox keep-mask of bf_philox.h.  A dropout group is the 8
    // probabilities of one P^T fragment: query q, keys tile * 128 + (2c + e) * 16 + 4 lg + j (e = 0, 1; j = 0..3) ->
    //   group index g = (((b * H + h) * T + q) * (T / 32) + tile * 4 + c) * 4 + lg,   field = e * 4 + j.
    // keep_bits (nullable): the decisions as one 32-bit word per (b, h, q, tile, lg), bit c * 8 + e * 4 + j — 1 bit per
    // probability, 3 % of the layer's q/k/v/o traffic — for the backward kernel, whose lanes own 4 QUERIES of one key and
    // would have to evaluate eight Philox blocks per group of eight to regenerate them.
    // TAIL instantiation (any T >= 1, the bf_attention_fwd_any entries): with Tp = 128 * ceil(T / 128) the key tiles are
    // those of a sequence of Tp keys, so
    //   group index g = (((b * H + h) * T + q) * (Tp / 32) + tile * 4 + c) * 4 + lg,   keep_bits [B][H][T][Tp / 32]
    // — at T % 128 == 0 the contract above, bit for bit.  Bits drawn for keys >= T are meaningless and unread; a query
    // >= T stores no word.
    bf_dropout_t drop;
    uint32_t* keep_bits;  // [B][H][T][T / 32] (TAIL: [B][H][T][Tp / 32])
    // ROWS instantiation: only queries 0 .. q_rows - 1 (<= 16) of each (sequence, head) are computed, against all T keys;
    // out is the compact [B][q_rows][H][64]
    int q_rows;
};

// 3 workgroups per CU, for the DROP instantiation too: at 3 it spills 12 registers (168 VGPRs + 48 B of scratch), at 2 it does
// not (178 VGPRs); measured back to back, same box: 69.9 vs 72.0 us at the BERT-base shape, 278 vs 304 us at 160 x 16 heads x
// 384 tokens — the third workgroup is worth more than the spills cost.
// ROWS: the first q_rows <= 16 queries only — the block (wave 0, qi 0) of the full kernel that owns them, run as it is (the
// lanes past q_rows repeat the last row and store nothing), so those rows come out bit for bit as the full kernel's; the other
// three waves only stage the key / value tiles, which is what the launch costs.
// TAIL: any T >= 1 on the same tiles.  Rows of q / k / v past T - 1 re-read row T - 1 (never what lies around the tensor);
// a key >= T scores -inf through the tile's mask row in LDS — into which the mask, when there is one, goes by bounded 4-byte
// reads (its row b * T is 16-byte aligned only when T % 4 == 0) — so its probability is exactly 0 and the rows < T come
// out bit for bit as the plain kernel's on a sequence padded to Tp with -inf on the pad keys; a query >= T stores nothing.
template <typename T, bool DROP = false, bool ROWS = false, bool TAIL = false>
__global__ __launch_bounds__(256, 3) void attention_fwd_kernel(const AttnParams p) {
    static_assert(!(DROP && ROWS), "the query-subset form is an inference kernel");
    using frag = typename Mfma<T>::frag;
    using half4 = typename Mfma<T>::half4;
    __shared__ __attribute__((aligned(16))) char smem[K_BYTES + V_BYTES + TKEY * 4];
    char* const ks = smem;
    char* const vs = smem + K_BYTES;
    float* const ms = reinterpret_cast<float*>(smem + K_BYTES + V_BYTES);  // this tile's key mask, in log2 units
    // the caller may not know on the host whether its padding mask hides anything: a device flag says so (uniform)
    const float* const mask = (p.mask && !(p.mask_off && *p.mask_off)) ? p.mask : nullptr;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int q0 = blockIdx.x * TQ + wid * 32, h = blockIdx.y, b = blockIdx.z;
    const T* qb = reinterpret_cast<const T*>(p.q) + (long long)b * p.T * p.tok_stride + (long long)h * HD;
    const T* kb = reinterpret_cast<const T*>(p.k) + (long long)b * p.T * p.tok_stride + (long long)h * HD;
    const T* vb = reinterpret_cast<const T*>(p.v) + (long long)b * p.T * p.tok_stride + (long long)h * HD;

    // Q^T column operand: lane (query = li, k group = lg) holds 8 consecutive features of its query
    frag qf[2][2];
#pragma unroll
    for (int qb_i = 0; qb_i < 2; ++qb_i)
#pragma unroll
        for (int dh = 0; dh < 2; ++dh)
            qf[qb_i][dh] = *reinterpret_cast<const frag*>(
                qb + (long long)(ROWS ? min(li, p.q_rows - 1) : (TAIL ? min(q0 + qb_i * 16 + li, p.T - 1) : q0 + qb_i * 16 + li)) *
                         p.tok_stride + dh * 32 + lg * 8);

    f32x4_t o[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float run_max[2] = {-INFINITY, -INFINITY}, run_sum[2] = {0.f, 0.f};

    for (int key0 = 0; key0 < p.T; key0 += TKEY) {
        if (key0) __syncthreads();  // the previous tile's fragment reads are done
        // stage K (swizzled) and V (padded), 16 bytes per lane; not two stage<> calls: the assembly of those is longer
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i, row = c >> 3, c8 = c & 7;
            const int krow = TAIL ? min(key0 + row, p.T - 1) : key0 + row;
            const f32x4_t kv = *reinterpret_cast<const f32x4_t*>(kb + (long long)krow * p.tok_stride + c8 * 8);
            *reinterpret_cast<f32x4_t*>(ks + row * Rows<HD>::SWZ + ((c8 ^ (row & 7)) << 4)) = kv;
            const f32x4_t vv = *reinterpret_cast<const f32x4_t*>(vb + (long long)krow * p.tok_stride + c8 * 8);
            *reinterpret_cast<f32x4_t*>(vs + row * Rows<HD>::PAD + (c8 << 4)) = vv;
        }
        // (uniform) TAIL: the last tile always has a mask row, -inf on the keys >= T
        const bool masked = TAIL ? mask || key0 + TKEY > p.T : mask != nullptr;
        if constexpr (TAIL) {
            if (masked && tid < TKEY) {
                const int key = key0 + tid;
                ms[tid] = key < p.T ? (mask ? mask[(long long)b * p.T + key] * LOG2E : 0.f) : -INFINITY;
            }
        } else if (mask && tid < TKEY / 4)
            *reinterpret_cast<f32x4_t*>(ms + tid * 4) =
                *reinterpret_cast<const f32x4_t*>(mask + (long long)b * p.T + key0 + tid * 4) * LOG2E;
        __syncthreads();

        // One block of 16 queries at a time (keeps the live scores at 32 registers, 4 waves per SIMD fit).
#pragma unroll
        for (int qi = 0; qi < 2; ++qi) {
            if (ROWS && (qi || wid)) continue;  // (wave-uniform)
            // S^T[key][query]: lane (query li, group lg) holds keys kb*16 + 4*lg + 0..3 of each 16-key block
            f32x4_t s[8];
#pragma unroll
            for (int kbk = 0; kbk < 8; ++kbk) {
                s[kbk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dh = 0; dh < 2; ++dh) s[kbk] = Mfma<T>::run(row_frag<T, HD>(ks, kbk, dh, li, lg), qf[qi][dh], s[kbk]);
            }
            // scale (+ additive key mask: a lane's 4 keys of a block are one 16-byte LDS read), in log2 units
            float mx = -INFINITY;
#pragma unroll
            for (int kbk = 0; kbk < 8; ++kbk) {
                f32x4_t mk = {0.f, 0.f, 0.f, 0.f};
                if (TAIL ? masked : mask != nullptr) mk = *reinterpret_cast<const f32x4_t*>(ms + kbk * 16 + lg * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s[kbk][j] = fmaf(s[kbk][j], p.scale_log2e, mk[j]);
                    mx = fmaxf(mx, s[kbk][j]);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float new_max = fmaxf(run_max[qi], mx);
            // a fully masked row so far keeps max = -inf: use 0 as the reference point (all terms become 0)
            const float ref = new_max == -INFINITY ? 0.f : new_max;
            const float corr = __builtin_amdgcn_exp2f(run_max[qi] - ref);  // exp2(-inf) = 0 on the first tile
            float sum = 0.f;
#pragma unroll
            for (int kbk = 0; kbk < 8; ++kbk)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s[kbk][j] = __builtin_amdgcn_exp2f(s[kbk][j] - ref);
                    sum += s[kbk][j];
                }
            sum += __shfl_xor(sum, 16);
            sum += __shfl_xor(sum, 32);
            run_sum[qi] = run_sum[qi] * corr + sum;
            run_max[qi] = new_max;
            if constexpr (DROP) {
                // drop probabilities (the sum above saw all of them); the 1 / (1 - p) factor joins the final normalisation
                const unsigned long long qrow = ((unsigned long long)b * p.H + h) * p.T + (q0 + qi * 16 + li);
                const unsigned tiles = TAIL ? (unsigned)(p.T + TKEY - 1) >> 7 : (unsigned)(p.T >> 7);  // Tp / 128
                const unsigned long long g0 = (qrow * (TAIL ? tiles * 4u : (unsigned)(p.T >> 5)) + (unsigned)(key0 >> 7) * 4u) * 4u + lg +
                                              (((unsigned long long)p.drop.g0_hi << 32) | p.drop.g0_lo);
                uint32_t word = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const unsigned long long g = g0 + 4ull * c;
                    const uint32_t keep = bf_dropout_keep8((uint32_t)g, (uint32_t)(g >> 32), bf_dropout_call(p.drop), p.drop.site,
                                                           p.drop.k0, p.drop.k1, p.drop.thresh);
                    word |= keep << (8 * c);
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (!((keep >> (e * 4 + j)) & 1u)) s[2 * c + e][j] = 0.f;
                }
                if (p.keep_bits && (!TAIL || q0 + qi * 16 + li < p.T))
                    p.keep_bits[(qrow * tiles + (unsigned)(key0 >> 7)) * 4u + lg] = word;
            }
#pragma unroll
            for (int db = 0; db < 4; ++db) o[qi][db] *= corr;
            // O^T[d][query] += V^T[d][k] P^T[k][query], k walking 32 keys at a time in the order pack2 / tr_frag share
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const frag pf = pack2<T>(s[2 * c], s[2 * c + 1]);
#pragma unroll
                for (int db = 0; db < 4; ++db) o[qi][db] = Mfma<T>::run(tr_frag<T, HD>(vs, c, db, li, lg), pf, o[qi][db]);
            }
            // (TAIL: keeps the two query blocks' scores from being live at once)
            if constexpr (TAIL) __builtin_amdgcn_sched_barrier(0);
        }
    }

    // lane (query li, group lg) holds features db*16 + 4*lg + 0..3 of its query: 8-byte stores
    if constexpr (ROWS) {
        if (wid || li >= p.q_rows) return;
        T* orow = reinterpret_cast<T*>(p.out) + (((long long)b * p.q_rows + li) * p.H + h) * HD;
        const float inv = run_sum[0] > 0.f ? 1.0f / run_sum[0] : 0.f;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const f32x4_t r = o[0][db] * inv;
            attn_st8(reinterpret_cast<half4*>(orow + db * 16 + lg * 4), __builtin_convertvector(r, half4));
        }
        return;
    }
    T* ob = reinterpret_cast<T*>(p.out) + ((long long)b * p.T * p.H + h) * HD;
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        if (TAIL && q0 + qi * 16 + li >= p.T) continue;
        const float inv = run_sum[qi] > 0.f ? (DROP ? p.drop.inv_keep : 1.0f) / run_sum[qi] : 0.f;
        // a fully masked query has no probabilities: +inf makes exp2(score - lse) = 0 in the backward kernels
        if (p.lse && lg == 0)
            p.lse[((long long)b * p.H + h) * p.T + q0 + qi * 16 + li] =
                run_sum[qi] > 0.f ? run_max[qi] + __builtin_amdgcn_logf(run_sum[qi]) : INFINITY;
        T* orow = ob + (long long)(q0 + qi * 16 + li) * p.H * HD;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const f32x4_t r = o[qi][db] * inv;
            attn_st8(reinterpret_cast<half4*>(orow + db * 16 + lg * 4), __builtin_convertvector(r, half4));
        }
    }
}

// ROWS: one workgroup per (sequence, head)
template <typename T, bool DROP, bool ROWS, bool TAIL = false>
void launch(const AttnParams& p, hipStream_t stream) {
    hipLaunchKernelGGL((attention_fwd_kernel<T, DROP, ROWS, TAIL>), dim3(ROWS ? 1 : (p.T + TQ - 1) / TQ, p.H, p.B), dim3(256), 0,
                       stream, p);
}

}  // namespace

// the three entries' shared worker: drop / d_keep_bits for the dropout entry, q_rows for the rows entry
static int attention_fwd(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                         void* d_out, float* d_lse, int dtype, int B, int T, int H, int head_dim, long long token_stride,
                         float scaling, hipStream_t stream, const bf_dropout_t* drop = nullptr, uint32_t* d_keep_bits = nullptr,
                         int q_rows = 0) {
    if (!d_q || !d_k || !d_v || !d_out) BF_FAIL("bf_attention_fwd: NULL argument");
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) BF_FAIL("bf_attention_fwd: dtype must be bf16 or fp16");
    if (head_dim != HD) BF_FAIL("bf_attention_fwd: head size %d (only %d)", head_dim, HD);
    if (B < 1 || H < 1 || T < TKEY || T % TKEY) BF_FAIL("bf_attention_fwd: T=%d must be a positive multiple of %d", T, TKEY);
    if (B > 65535 || H > 65535) BF_FAIL("bf_attention_fwd: B or H exceeds the grid");
    if (token_stride < (long long)H * HD || token_stride % 8) BF_FAIL("bf_attention_fwd: bad token stride %lld", token_stride);
    if (((uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out) & 15) BF_FAIL("bf_attention_fwd: pointers must be 16-byte aligned");
    if (d_mask && ((uintptr_t)d_mask & 15)) BF_FAIL("bf_attention_fwd: mask must be 16-byte aligned");  // read 16 bytes at a time
    AttnParams p;
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.mask = d_mask;
    p.mask_off = d_mask_off;
    p.out = d_out;
    p.lse = d_lse;
    p.tok_stride = token_stride;
    p.B = B;
    p.T = T;
    p.H = H;
    p.scale_log2e = scaling * LOG2E;
    p.keep_bits = nullptr;
    p.drop = bf_dropout_t{0, 0, 0, 0, 0, 1.0f, 0, 0, nullptr};
    p.q_rows = q_rows;
    const bool bf16 = dtype == BF_DT_BF16;
    if (q_rows) {
        if (q_rows < 1 || q_rows > 16) BF_FAIL("bf_attention_fwd_rows: q_rows=%d (1 .. 16)", q_rows);
        if (d_lse || (drop && drop->thresh)) BF_FAIL("bf_attention_fwd_rows: inference only (no log-sum-exp rows, no dropout)");
        if (bf16) launch<__bf16, false, true>(p, stream);
        else launch<_Float16, false, true>(p, stream);
    } else if (drop && drop->thresh) {
        if (d_keep_bits && ((uintptr_t)d_keep_bits & 3)) BF_FAIL("bf_attention_fwd: keep bits must be 4-byte aligned");
        p.drop = *drop;
        p.keep_bits = d_keep_bits;
        if (bf16) launch<__bf16, true, false>(p, stream);
        else launch<_Float16, true, false>(p, stream);
    } else {
        if (bf16) launch<__bf16, false, false>(p, stream);
        else launch<_Float16, false, false>(p, stream);
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_attention_fwd(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                     void* d_out, float* d_lse, int dtype, int B, int T, int H, int head_dim, int64_t token_stride,
                     float scaling, void* stream) {
    return attention_fwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_lse, dtype, B, T, H, head_dim, token_stride, scaling,
                         (hipStream_t)stream);
}

int bf_attention_fwd_rows(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                          void* d_out, int dtype, int B, int T, int H, int head_dim, int64_t token_stride, int q_rows,
                          float scaling, void* stream) {
    if (q_rows < 1 || q_rows > 16) BF_FAIL("bf_attention_fwd_rows: q_rows=%d (1 .. 16)", q_rows);
    return attention_fwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, nullptr, dtype, B, T, H, head_dim, token_stride, scaling,
                         (hipStream_t)stream, nullptr, nullptr, q_rows);
}

int bf_attention_fwd_dropout(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                             void* d_out, float* d_lse, int dtype, int B, int T, int H, int head_dim, int64_t token_stride,
                             float scaling, float p_drop, uint64_t seed, uint32_t call, uint32_t site, uint64_t first_group,
                             uint32_t* d_keep_bits, const uint32_t* d_call, void* stream) {
    if (!(p_drop >= 0.f) || !(p_drop < 1.f)) BF_FAIL("bf_attention_fwd_dropout: p must be in [0, 1) (got %g)", p_drop);
    const bf_dropout_t d = bf_make_dropout(p_drop, seed, call, site, first_group, d_call);
    return attention_fwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_lse, dtype, B, T, H, head_dim, token_stride, scaling,
                         (hipStream_t)stream, &d, d_keep_bits);
}

// ------------------------------------------------------------------------------- any T >= 1 (bayeformers_amd_encoder_any.h)
// T % 128 == 0: the sibling's own worker, kernel and bits.  Otherwise the TAIL instantiations; their mask reads are 4 bytes
// wide, so the mask needs no more than its type's alignment.
static int attention_fwd_any(const char* what, const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                             const uint8_t* d_mask_off, void* d_out, float* d_lse, int dtype, int B, int T, int H, int head_dim,
                             long long token_stride, float scaling, hipStream_t stream, const bf_dropout_t* drop = nullptr,
                             uint32_t* d_keep_bits = nullptr, int q_rows = 0) {
    if (T >= TKEY && T % TKEY == 0)
        return attention_fwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_lse, dtype, B, T, H, head_dim, token_stride, scaling,
                             stream, drop, d_keep_bits, q_rows);
    if (!d_q || !d_k || !d_v || !d_out) BF_FAIL("%s: NULL argument", what);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) BF_FAIL("%s: dtype must be bf16 or fp16", what);
    if (head_dim != HD) BF_FAIL("%s: head size %d (only %d)", what, head_dim, HD);
    if (B < 1 || H < 1 || T < 1) BF_FAIL("%s: B=%d, H=%d, T=%d must be positive", what, B, H, T);
    if (T > 0x7fffff00) BF_FAIL("%s: T=%d exceeds the key index", what, T);
    if (B > 65535 || H > 65535) BF_FAIL("%s: B or H exceeds the grid", what);
    if (token_stride < (long long)H * HD || token_stride % 8) BF_FAIL("%s: bad token stride %lld", what, token_stride);
    if (((uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out) & 15) BF_FAIL("%s: pointers must be 16-byte aligned", what);
    if (d_mask && ((uintptr_t)d_mask & 3)) BF_FAIL("%s: mask must be 4-byte aligned", what);
    if (d_lse && ((uintptr_t)d_lse & 3)) BF_FAIL("%s: lse must be 4-byte aligned", what);
    AttnParams p;
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.mask = d_mask;
    p.mask_off = d_mask_off;
    p.out = d_out;
    p.lse = d_lse;
    p.tok_stride = token_stride;
    p.B = B;
    p.T = T;
    p.H = H;
    p.scale_log2e = scaling * LOG2E;
    p.keep_bits = nullptr;
    p.drop = bf_dropout_t{0, 0, 0, 0, 0, 1.0f, 0, 0, nullptr};
    p.q_rows = q_rows;
    const bool bf16 = dtype == BF_DT_BF16;
    if (q_rows) {
        if (q_rows > T) BF_FAIL("%s: q_rows=%d exceeds T=%d", what, q_rows, T);
        if (bf16) launch<__bf16, false, true, true>(p, stream);
        else launch<_Float16, false, true, true>(p, stream);
    } else if (drop && drop->thresh) {
        if (d_keep_bits && ((uintptr_t)d_keep_bits & 3)) BF_FAIL("%s: keep bits must be 4-byte aligned", what);
        p.drop = *drop;
        p.keep_bits = d_keep_bits;
        if (bf16) launch<__bf16, true, false, true>(p, stream);
        else launch<_Float16, true, false, true>(p, stream);
    } else {
        if (bf16) launch<__bf16, false, false, true>(p, stream);
        else launch<_Float16, false, false, true>(p, stream);
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_attention_fwd_any(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                         void* d_out, float* d_lse, int dtype, int B, int T, int H, int head_dim, int64_t token_stride,
                         float scaling, void* stream) {
    return attention_fwd_any("bf_attention_fwd_any", d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_lse, dtype, B, T, H, head_dim,
                             token_stride, scaling, (hipStream_t)stream);
}

int bf_attention_fwd_any_rows(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                              void* d_out, int dtype, int B, int T, int H, int head_dim, int64_t token_stride, int q_rows,
                              float scaling, void* stream) {
    if (q_rows < 1 || q_rows > 16) BF_FAIL("bf_attention_fwd_any_rows: q_rows=%d (1 .. 16)", q_rows);
    return attention_fwd_any("bf_attention_fwd_any_rows", d_q, d_k, d_v, d_mask, d_mask_off, d_out, nullptr, dtype, B, T, H,
                             head_dim, token_stride, scaling, (hipStream_t)stream, nullptr, nullptr, q_rows);
}

int bf_attention_fwd_any_dropout(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                 const uint8_t* d_mask_off, void* d_out, float* d_lse, int dtype, int B, int T, int H,
                                 int head_dim, int64_t token_stride, float scaling, float p_drop, uint64_t seed, uint32_t call,
                                 uint32_t site, uint64_t first_group, uint32_t* d_keep_bits, const uint32_t* d_call,
                                 void* stream) {
    if (!(p_drop >= 0.f) || !(p_drop < 1.f)) BF_FAIL("bf_attention_fwd_any_dropout: p must be in [0, 1) (got %g)", p_drop);
    const bf_dropout_t d = bf_make_dropout(p_drop, seed, call, site, first_group, d_call);
    return attention_fwd_any("bf_attention_fwd_any_dropout", d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_lse, dtype, B, T, H,
                             head_dim, token_stride, scaling, (hipStream_t)stream, &d, d_keep_bits);
}
