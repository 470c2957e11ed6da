// bf_attention_bwd.hip — backward of bf_attention_fwd (bf_attention.hip): autograd through the attention block between the
// Bayesian query/key/value projections and the Bayesian output projection in the reference's training loop
// (examples/bert_glue.py, `loss.backward()` through HF BertSelfAttention).
//
// With P = softmax(scale Q K^T + mask) (recomputed from Q, K and the log-sum-exp rows the forward saved),
// delta_q = sum_d dO[q][d] O[q][d] and dS = P o (dO V^T - delta):
//     dV = P^T dO,   dK = scale dS^T Q,   dQ = scale dS K.
// Two kernels, no atomics (deterministic), head size 64, queries / keys in tiles of 128, bf16 or fp16; the fragment layouts
// and LDS images are the forward's (bf_attention_tiles.h):
//   * dq kernel — one workgroup per (128 queries, head, sequence), 4 waves x 32 queries, walking the key tiles in the
//     forward's orientation: S^T = K Q^T and dP^T = V dO^T with the keys as rows, dS^T the column operand of
//     dQ^T = K^T dS^T, K^T through the transpose read.  Also leaves delta for the second kernel.
//   * dk/dv kernel — one workgroup per (128 keys, head, sequence), 8 waves x 16 keys, walking the query tiles with the roles
//     swapped: S = Q K^T and dP = dO V^T with the QUERIES as rows; P and dS are the column operands of dV^T = dO^T P and
//     dK^T = Q^T dS, dO^T / Q^T through the transpose read.
// Algorithmic HBM bytes: dq kernel 5 reads (Q, K, V, O, dO) + 1 write; dk/dv kernel 4 reads + 2 writes, x B*T*H*64*2 B.
#include "bf_attention_tiles.h"
#include "bf_device.h"
#include "bf_philox.h"
#include "../../include/bayeformers_amd_encoder_any.h"

namespace {

constexpr int HD = 64;
constexpr int TT = 128;                      // queries / keys per tile
constexpr int S_BYTES = TT * Rows<HD>::SWZ;  // 16 KiB: a swizzled tile
constexpr int P_BYTES = TT * Rows<HD>::PAD;  // 20 KiB: a padded tile

struct BwdParams {
    const void* q;
    const void* k;
    const void* v;
    const float* mask;              // [B][T] additive over the keys, nullable
    const unsigned char* mask_off;  // nullable device flag: non-zero = skip the mask
    const void* o;                  // [B][T][H][64]
    const void* dout;               // [B][T][H][64]
    const float* lse;               // [B][H][T], log2 units
    float* delta;                   // [B][H][T]
    void* dq;                       // [B][T][H][64]
    void* dk;
    void* dv;
    long long tok_stride;           // elements between consecutive tokens of q / k / v
    int B, T, H;
    float scale, scale_log2e;
    // attention_probs_dropout (the forward's DROP instantiation): the keep decisions the forward stored, one bit per
    // probability in AttnParams' layout (bf_attention.hip), and the 1 / (1 - p) factor.  NULL: no dropout.
    // With P~ = P o keep / (1 - p):  dV = P~^T dO,  dS = P o (keep / (1 - p) o dP~ - delta).
    const uint32_t* keep_bits;
    float inv_keep;
    // one-tile kernel only (round 5): per (sequence, head) the sums over the 128 tokens of dq, dk, dv AS STORED —
    // [B][H][3][64] fp32 — from which attention_colsum_finish_kernel makes the per-sample column sums that the Bayesian
    // query / key / value layers take as their bias gradient (bf_linear_bwd: d_dy_colsum).  NULL: not wanted.
    float* cs_partial;
};

// ---------------------------------------------------------------------------------------------------- dQ (+ delta)
// TAIL (both kernels; any T >= 1, the bf_attention_bwd_any entries; Tp = 128 * ceil(T / 128)): rows of q / k / v / o / dO
// past T - 1 re-read row T - 1, never what lies around the tensor.  A key >= T scores -inf through the mask row in LDS (dq
// kernel) and stores no dk / dv row (dk/dv kernel); a query >= T has lse = +inf — its probabilities are exactly 0, so it
// adds exactly 0 to dk and dv — and stores no delta and no dq row.  The mask, lse and delta rows start at b * T or
// (b * H + h) * T floats, 16-byte aligned only when T % 4 == 0: bounded 4-byte reads.  The keep words are the TAIL
// forward's, [B][H][T][Tp / 32].
template <typename T, bool DROP = false, bool TAIL = false>
__global__ __launch_bounds__(256, 2) void attention_bwd_dq_kernel(const BwdParams p) {
    using frag = typename Mfma<T>::frag;
    using half4 = typename Mfma<T>::half4;
    __shared__ __attribute__((aligned(16))) char smem[2 * S_BYTES + P_BYTES + TT * 4];
    char* const ks = smem;                     // K, swizzled: row operand of S^T
    char* const vs = smem + S_BYTES;           // V, swizzled: row operand of dP^T
    char* const kp = smem + 2 * S_BYTES;       // K, padded: K^T through the transpose read
    float* const ms = reinterpret_cast<float*>(smem + 2 * S_BYTES + P_BYTES);
    const float* const mask = (p.mask && !(p.mask_off && *p.mask_off)) ? p.mask : nullptr;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int q0 = blockIdx.x * TT + wid * 32, h = blockIdx.y, b = blockIdx.z;
    const long long hoff = (long long)h * HD;
    const T* qb = reinterpret_cast<const T*>(p.q) + (long long)b * p.T * p.tok_stride + hoff;
    const T* kb = reinterpret_cast<const T*>(p.k) + (long long)b * p.T * p.tok_stride + hoff;
    const T* vb = reinterpret_cast<const T*>(p.v) + (long long)b * p.T * p.tok_stride + hoff;
    const long long ostride = (long long)p.H * HD;
    const T* ob = reinterpret_cast<const T*>(p.o) + (long long)b * p.T * ostride + hoff;
    const T* dob = reinterpret_cast<const T*>(p.dout) + (long long)b * p.T * ostride + hoff;

    // column operands: lane (query li, k group lg) holds 8 consecutive features of its query, per 32-feature half
    frag qf[2][2], dof[2][2];
    float delta[2], lse[2];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        const bool live = !TAIL || q0 + qi * 16 + li < p.T;  // (TAIL: a query >= T repeats row T - 1 and stores nothing)
        const long long q = TAIL ? min(q0 + qi * 16 + li, p.T - 1) : q0 + qi * 16 + li;
        float part = 0.f;
#pragma unroll
        for (int dh = 0; dh < 2; ++dh) {
            qf[qi][dh] = *reinterpret_cast<const frag*>(qb + q * p.tok_stride + dh * 32 + lg * 8);
            dof[qi][dh] = *reinterpret_cast<const frag*>(dob + q * ostride + dh * 32 + lg * 8);
            const frag of = *reinterpret_cast<const frag*>(ob + q * ostride + dh * 32 + lg * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) part = fmaf((float)dof[qi][dh][e], (float)of[e], part);
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        delta[qi] = part;
        lse[qi] = live ? p.lse[((long long)b * p.H + h) * p.T + q] : INFINITY;
        if (lg == 0 && live) p.delta[((long long)b * p.H + h) * p.T + q] = part;
    }

    f32x4_t dq[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) dq[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int key0 = 0; key0 < p.T; key0 += TT) {
        if (key0) __syncthreads();
        // (uniform) TAIL: the last tile always has a mask row, -inf on the keys >= T
        const bool masked = TAIL ? mask || key0 + TT > p.T : mask != nullptr;
        if constexpr (TAIL) {
            stage_clamped<T, HD, TT, 256>(kb, p.tok_stride, key0, 0, p.T - 1, ks, kp, tid);
            stage_clamped<T, HD, TT, 256>(vb, p.tok_stride, key0, 0, p.T - 1, vs, nullptr, tid);
            if (masked && tid < TT) {
                const int key = key0 + tid;
                ms[tid] = key < p.T ? (mask ? mask[(long long)b * p.T + key] * LOG2E : 0.f) : -INFINITY;
            }
        } else {
            stage<T, HD, TT, 256>(kb, p.tok_stride, key0, ks, kp, tid);
            stage<T, HD, TT, 256>(vb, p.tok_stride, key0, vs, nullptr, tid);
            if (mask && tid < TT / 4)
                *reinterpret_cast<f32x4_t*>(ms + tid * 4) =
                    *reinterpret_cast<const f32x4_t*>(mask + (long long)b * p.T + key0 + tid * 4) * LOG2E;
        }
        __syncthreads();
#pragma unroll
        for (int qi = 0; qi < 2; ++qi) {
            // DROP: the lane's 32 probabilities of this (query, key tile) are the 32 bits of ONE keep word, in the
            // forward's own layout (word (query, key tile, lg), bit 4 kbk + j) — loaded ahead of the products
            uint32_t kw = 0;
            if constexpr (DROP && TAIL)
                kw = p.keep_bits[((((long long)b * p.H + h) * p.T + min(q0 + qi * 16 + li, p.T - 1)) * ((p.T + TT - 1) / TT) +
                                  key0 / TT) * 4 + lg];
            else if constexpr (DROP)
                kw = p.keep_bits[((((long long)b * p.H + h) * p.T + (q0 + qi * 16 + li)) * (p.T / TT) + key0 / TT) * 4 + lg];
            // S^T and dP^T [key][query]: lane (query li, group lg) holds keys kbk*16 + 4 lg + 0..3 of each block
            f32x4_t s[8], dp[8];
#pragma unroll
            for (int kbk = 0; kbk < 8; ++kbk) {
                s[kbk] = dp[kbk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dh = 0; dh < 2; ++dh) {
                    s[kbk] = Mfma<T>::run(row_frag<T, HD>(ks, kbk, dh, li, lg), qf[qi][dh], s[kbk]);
                    dp[kbk] = Mfma<T>::run(row_frag<T, HD>(vs, kbk, dh, li, lg), dof[qi][dh], dp[kbk]);
                }
            }
#pragma unroll
            for (int kbk = 0; kbk < 8; ++kbk) {
                f32x4_t mk = {0.f, 0.f, 0.f, 0.f};
                if (TAIL ? masked : mask != nullptr) mk = *reinterpret_cast<const f32x4_t*>(ms + kbk * 16 + lg * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float pr = __builtin_amdgcn_exp2f(fmaf(s[kbk][j], p.scale_log2e, mk[j]) - lse[qi]);
                    if constexpr (DROP) {
                        const float m = ((kw >> (kbk * 4 + j)) & 1u) ? p.inv_keep : 0.f;
                        s[kbk][j] = pr * (dp[kbk][j] * m - delta[qi]);  // dS^T = P o (keep / (1 - p) o dP~ - delta)
                    } else {
                        s[kbk][j] = pr * (dp[kbk][j] - delta[qi]);  // dS^T
                    }
                }
            }
            // dQ^T[d][query] += K^T[d][k] dS^T[k][query], k walking 32 keys at a time in the order the blocks give
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const frag dsf = pack2<T>(s[2 * c], s[2 * c + 1]);
#pragma unroll
                for (int db = 0; db < 4; ++db) dq[qi][db] = Mfma<T>::run(tr_frag<T, HD>(kp, c, db, li, lg), dsf, dq[qi][db]);
            }
        }
    }
    // lane (query li, group lg) holds features db*16 + 4 lg + 0..3 of its query
    T* dqb = reinterpret_cast<T*>(p.dq) + (long long)b * p.T * ostride + hoff;
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        if (TAIL && q0 + qi * 16 + li >= p.T) continue;
        T* row = dqb + (long long)(q0 + qi * 16 + li) * ostride;
#pragma unroll
        for (int db = 0; db < 4; ++db)
            *reinterpret_cast<half4*>(row + db * 16 + lg * 4) = __builtin_convertvector(dq[qi][db] * p.scale, half4);
    }
}

// ---------------------------------------------------------------------------------------------------- dK, dV
// 8 waves, each owning 16 keys of the workgroup's 128 (32 keys per wave need 117 spilled registers).
template <typename T, bool DROP = false, bool TAIL = false>
__global__ __launch_bounds__(512, 2) void attention_bwd_dkv_kernel(const BwdParams p) {
    using frag = typename Mfma<T>::frag;
    using half4 = typename Mfma<T>::half4;
    __shared__ __attribute__((aligned(16))) char smem[2 * S_BYTES + 2 * P_BYTES + 2 * TT * 4 + (DROP ? TT * 16 : 0)];
    char* const qs = smem;                               // Q, swizzled: row operand of S
    char* const dos = smem + S_BYTES;                    // dO, swizzled: row operand of dP
    char* const qp = smem + 2 * S_BYTES;                 // Q, padded: Q^T through the transpose read
    char* const dop = smem + 2 * S_BYTES + P_BYTES;      // dO, padded: dO^T through the transpose read
    float* const lse_s = reinterpret_cast<float*>(smem + 2 * S_BYTES + 2 * P_BYTES);
    float* const del_s = lse_s + TT;
    uint32_t* const keep_s = reinterpret_cast<uint32_t*>(del_s + TT);  // DROP: [128 queries][4 lg] keep words of this (query tile, key tile)
    const float* const mask = (p.mask && !(p.mask_off && *p.mask_off)) ? p.mask : nullptr;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z;
    const long long key = blockIdx.x * TT + wid * 16 + li;
    // DROP: this lane's key sits in word (query, key tile, lg_f) at one fixed bit (the forward's layout)
    const int key_i = wid * 16 + li;
    const int keep_word = (key_i >> 2) & 3, keep_bit = ((key_i >> 5) << 3) | (((key_i >> 4) & 1) << 2) | (key_i & 3);
    const long long hoff = (long long)h * HD;
    const T* qb = reinterpret_cast<const T*>(p.q) + (long long)b * p.T * p.tok_stride + hoff;
    const T* kb = reinterpret_cast<const T*>(p.k) + (long long)b * p.T * p.tok_stride + hoff;
    const T* vb = reinterpret_cast<const T*>(p.v) + (long long)b * p.T * p.tok_stride + hoff;
    const long long ostride = (long long)p.H * HD;
    const T* dob = reinterpret_cast<const T*>(p.dout) + (long long)b * p.T * ostride + hoff;
    const float* lse_g = p.lse + ((long long)b * p.H + h) * p.T;
    const float* del_g = p.delta + ((long long)b * p.H + h) * p.T;

    // column operands: lane (key li, k group lg) holds 8 consecutive features of its key
    const long long key_r = TAIL ? (key < p.T ? key : p.T - 1) : key;  // (TAIL: a key >= T repeats row T - 1 and stores nothing)
    frag kf[2], vf[2];
#pragma unroll
    for (int dh = 0; dh < 2; ++dh) {
        kf[dh] = *reinterpret_cast<const frag*>(kb + key_r * p.tok_stride + dh * 32 + lg * 8);
        vf[dh] = *reinterpret_cast<const frag*>(vb + key_r * p.tok_stride + dh * 32 + lg * 8);
    }
    const float mk = mask ? mask[(long long)b * p.T + key_r] * LOG2E : 0.f;
    f32x4_t dk[4], dv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) dk[j] = dv[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int q0 = 0; q0 < p.T; q0 += TT) {
        if (q0) __syncthreads();
        if constexpr (TAIL) {
            stage_clamped<T, HD, TT, 512>(qb, p.tok_stride, q0, 0, p.T - 1, qs, qp, tid);
            stage_clamped<T, HD, TT, 512>(dob, ostride, q0, 0, p.T - 1, dos, dop, tid);
            if (tid < TT) {  // a query >= T: lse = +inf, every probability exactly 0
                const bool live = q0 + tid < p.T;
                lse_s[tid] = live ? lse_g[q0 + tid] : INFINITY;
                del_s[tid] = live ? del_g[q0 + tid] : 0.f;
            }
            if constexpr (DROP)
                keep_s[tid] = p.keep_bits[((((long long)b * p.H + h) * p.T + min(q0 + (tid >> 2), p.T - 1)) * ((p.T + TT - 1) / TT) +
                                           blockIdx.x) * 4 + (tid & 3)];
        } else {
            stage<T, HD, TT, 512>(qb, p.tok_stride, q0, qs, qp, tid);
            stage<T, HD, TT, 512>(dob, ostride, q0, dos, dop, tid);
            if (tid < TT / 4) {
                *reinterpret_cast<f32x4_t*>(lse_s + tid * 4) = *reinterpret_cast<const f32x4_t*>(lse_g + q0 + tid * 4);
                *reinterpret_cast<f32x4_t*>(del_s + tid * 4) = *reinterpret_cast<const f32x4_t*>(del_g + q0 + tid * 4);
            }
            if constexpr (DROP)  // 512 words = 128 queries x 4 groups of this tile pair
                keep_s[tid] = p.keep_bits[((((long long)b * p.H + h) * p.T + q0 + (tid >> 2)) * (p.T / TT) + blockIdx.x) * 4 + (tid & 3)];
        }
        __syncthreads();
        // S and dP [query][key]: lane (key li, group lg) holds queries qbk*16 + 4 lg + 0..3 of each block
        f32x4_t s[8], dp[8];
#pragma unroll
        for (int qbk = 0; qbk < 8; ++qbk) {
            s[qbk] = dp[qbk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) {
                s[qbk] = Mfma<T>::run(row_frag<T, HD>(qs, qbk, dh, li, lg), kf[dh], s[qbk]);
                dp[qbk] = Mfma<T>::run(row_frag<T, HD>(dos, qbk, dh, li, lg), vf[dh], dp[qbk]);
            }
        }
#pragma unroll
        for (int qbk = 0; qbk < 8; ++qbk) {
            const f32x4_t l4 = *reinterpret_cast<const f32x4_t*>(lse_s + qbk * 16 + lg * 4);
            const f32x4_t d4 = *reinterpret_cast<const f32x4_t*>(del_s + qbk * 16 + lg * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float pr = __builtin_amdgcn_exp2f(fmaf(s[qbk][j], p.scale_log2e, mk) - l4[j]);
                if constexpr (DROP) {
                    const uint32_t wrd = keep_s[(qbk * 16 + lg * 4 + j) * 4 + keep_word];
                    const float m = ((wrd >> keep_bit) & 1u) ? p.inv_keep : 0.f;
                    s[qbk][j] = pr * m;                          // P~ = P o keep / (1 - p)
                    dp[qbk][j] = pr * (dp[qbk][j] * m - d4[j]);  // dS
                } else {
                    s[qbk][j] = pr;                          // P
                    dp[qbk][j] = pr * (dp[qbk][j] - d4[j]);  // dS
                }
            }
        }
        // dV^T[d][key] += dO^T[d][q] P[q][key];  dK^T[d][key] += Q^T[d][q] dS[q][key]
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const frag pf = pack2<T>(s[2 * c], s[2 * c + 1]);
            const frag dsf = pack2<T>(dp[2 * c], dp[2 * c + 1]);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                dv[db] = Mfma<T>::run(tr_frag<T, HD>(dop, c, db, li, lg), pf, dv[db]);
                dk[db] = Mfma<T>::run(tr_frag<T, HD>(qp, c, db, li, lg), dsf, dk[db]);
            }
        }
    }
    T* dkb = reinterpret_cast<T*>(p.dk) + (long long)b * p.T * ostride + hoff;
    T* dvb = reinterpret_cast<T*>(p.dv) + (long long)b * p.T * ostride + hoff;
    if (TAIL && key >= p.T) return;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        *reinterpret_cast<half4*>(dkb + key * ostride + db * 16 + lg * 4) = __builtin_convertvector(dk[db] * p.scale, half4);
        *reinterpret_cast<half4*>(dvb + key * ostride + db * 16 + lg * 4) = __builtin_convertvector(dv[db], half4);
    }
}


// ---------------------------------------------------------------------------------------------------- T = 128: all three
// One key tile = one query tile: dQ, dK and dV of a (sequence, head) in ONE workgroup, P and dS computed once.
// The first part is the dK / dV kernel (8 waves x 16 keys; S = Q K^T, dP = dO V^T with the queries as rows), with delta
// computed here (wave w: queries 16 w .. 16 w + 15).  Every wave leaves its 16 K rows (still in registers as the column
// operand) as rows of a padded K image once S and dP are done, and the dS of its 16 keys — a lane holds 4 consecutive
// queries of one key: 8-byte writes — as rows of a padded dS^T[key][query] image, over the Q / dO images that are dead by then;
// wave w takes queries 16 w .. 16 w + 15 of dQ^T = K^T dS^T with BOTH operands through the LDS transpose read (the
// same contraction order on either side: keys (2c) 16 + 4 lg + 0..3, (2c + 1) 16 + 4 lg + 0..3).  Deterministic: no
// atomics, a fixed summation order.  HBM: 5 reads (Q, K, V, O, dO) + 3 writes, against 9 + 3 of the two-kernel path.
constexpr int DS_ROW = TT * 2 + 32;  // 288 B: a row of dS^T (128 queries) + the transpose read's padding

template <typename T, bool DROP = false>
__global__ __launch_bounds__(512, 4) void attention_bwd_tile_kernel(const BwdParams p) {
    using frag = typename Mfma<T>::frag;
    using half4 = typename Mfma<T>::half4;
    __shared__ __attribute__((aligned(16))) char smem[2 * S_BYTES + 2 * P_BYTES + 2 * TT * 4 + (DROP ? TT * 16 : 0)];
    char* const qs = smem;                               // Q, swizzled: row operand of S
    char* const dos = smem + S_BYTES;                    // dO, swizzled: row operand of dP
    char* const qp = smem + 2 * S_BYTES;                 // Q, padded: Q^T through the transpose read
    char* const dop = smem + 2 * S_BYTES + P_BYTES;      // dO, padded: dO^T through the transpose read
    float* const lse_s = reinterpret_cast<float*>(smem + 2 * S_BYTES + 2 * P_BYTES);
    float* const del_s = lse_s + TT;
    uint32_t* const keep_s = reinterpret_cast<uint32_t*>(del_s + TT);  // DROP: [128 queries][4 lg] keep words of this (b, h)
    char* const kp = smem;                               // K, padded, over qs | dos once S and dP are done (K is still in registers)
    char* const dst = smem + 2 * S_BYTES;                // dS^T [128 keys][DS_ROW] over qp | dop once dK and dV are done
    static_assert(P_BYTES <= 2 * S_BYTES && TT * DS_ROW <= 2 * P_BYTES, "the K and dS^T images alias dead tiles only");
    const float* const mask = (p.mask && !(p.mask_off && *p.mask_off)) ? p.mask : nullptr;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z;
    const long long row = wid * 16 + li;                 // this lane's key in the first part, its query in the second
    const long long hoff = (long long)h * HD;
    const T* qb = reinterpret_cast<const T*>(p.q) + (long long)b * p.T * p.tok_stride + hoff;
    const T* kb = reinterpret_cast<const T*>(p.k) + (long long)b * p.T * p.tok_stride + hoff;
    const T* vb = reinterpret_cast<const T*>(p.v) + (long long)b * p.T * p.tok_stride + hoff;
    const long long ostride = (long long)p.H * HD;
    const T* ob = reinterpret_cast<const T*>(p.o) + (long long)b * p.T * ostride + hoff;
    const T* dob = reinterpret_cast<const T*>(p.dout) + (long long)b * p.T * ostride + hoff;
    const float* lse_g = p.lse + ((long long)b * p.H + h) * p.T;

    frag kf[2], vf[2], of[2];
#pragma unroll
    for (int dh = 0; dh < 2; ++dh) {
        kf[dh] = *reinterpret_cast<const frag*>(kb + row * p.tok_stride + dh * 32 + lg * 8);
        vf[dh] = *reinterpret_cast<const frag*>(vb + row * p.tok_stride + dh * 32 + lg * 8);
        of[dh] = *reinterpret_cast<const frag*>(ob + row * ostride + dh * 32 + lg * 8);
    }
    const float mk = mask ? mask[(long long)b * p.T + row] * LOG2E : 0.f;

    stage<T, HD, TT, 512>(qb, p.tok_stride, 0, qs, qp, tid);
    stage<T, HD, TT, 512>(dob, ostride, 0, dos, dop, tid);
    if (tid < TT / 4)
        *reinterpret_cast<f32x4_t*>(lse_s + tid * 4) = *reinterpret_cast<const f32x4_t*>(lse_g + tid * 4);
    if constexpr (DROP) keep_s[tid] = p.keep_bits[(((long long)b * p.H + h) * p.T) * 4 + tid];  // 512 words = 128 x 4
    __syncthreads();
    {   // delta of query `row` = <dO, O>: the dO row comes out of the staged tile (a row fragment of block wid is the
        // lane's 8 features of that row); it is first read behind the barrier that follows the S / dP products
        float part = 0.f;
#pragma unroll
        for (int dh = 0; dh < 2; ++dh) {
            const frag df = row_frag<T, HD>(dos, wid, dh, li, lg);
#pragma unroll
            for (int e = 0; e < 8; ++e) part = fmaf((float)df[e], (float)of[dh][e], part);
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (lg == 0) {
            del_s[row] = part;
            p.delta[((long long)b * p.H + h) * p.T + row] = part;
        }
    }
    // S and dP [query][key]: lane (key li, group lg) holds queries qbk*16 + 4 lg + 0..3 of each block
    f32x4_t s[8], dp[8];
#pragma unroll
    for (int qbk = 0; qbk < 8; ++qbk) {
        s[qbk] = dp[qbk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dh = 0; dh < 2; ++dh) {
            s[qbk] = Mfma<T>::run(row_frag<T, HD>(qs, qbk, dh, li, lg), kf[dh], s[qbk]);
            dp[qbk] = Mfma<T>::run(row_frag<T, HD>(dos, qbk, dh, li, lg), vf[dh], dp[qbk]);
        }
        if (qbk & 1) __builtin_amdgcn_sched_barrier(0);  // (keeps the fragment reads of later blocks from piling up in registers)
    }
    __syncthreads();  // delta of all 128 queries is in LDS; the swizzled Q and dO images are dead
#pragma unroll
    for (int dh = 0; dh < 2; ++dh) *reinterpret_cast<frag*>(kp + row * Rows<HD>::PAD + (dh * 32 + lg * 8) * 2) = kf[dh];
    // P and dS leave the fp32 accumulators as 16-bit column operands right away (half the registers through the dV /
    // dK products: no spills at 128 VGPRs); pf[c] / dsf[c] = query blocks 2c, 2c + 1
    frag pf[4], dsf[4];
    // DROP: this lane's key sits in word (query, lg_f) at one fixed bit
    const int key_i = (int)row;
    const int keep_word = (key_i >> 2) & 3, keep_bit = ((key_i >> 5) << 3) | (((key_i >> 4) & 1) << 2) | (key_i & 3);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int qbk = 2 * c + e;
            const f32x4_t l4 = *reinterpret_cast<const f32x4_t*>(lse_s + qbk * 16 + lg * 4);
            const f32x4_t d4 = *reinterpret_cast<const f32x4_t*>(del_s + qbk * 16 + lg * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float pr = __builtin_amdgcn_exp2f(fmaf(s[qbk][j], p.scale_log2e, mk) - l4[j]);
                if constexpr (DROP) {
                    const uint32_t wrd = keep_s[(qbk * 16 + lg * 4 + j) * 4 + keep_word];
                    const float m = ((wrd >> keep_bit) & 1u) ? p.inv_keep : 0.f;
                    s[qbk][j] = pr * m;                          // P~ = P o keep / (1 - p)
                    dp[qbk][j] = pr * (dp[qbk][j] * m - d4[j]);  // dS
                } else {
                    s[qbk][j] = pr;                          // P
                    dp[qbk][j] = pr * (dp[qbk][j] - d4[j]);  // dS
                }
            }
        }
        pf[c] = pack2<T>(s[2 * c], s[2 * c + 1]);
        dsf[c] = pack2<T>(dp[2 * c], dp[2 * c + 1]);
    }
    f32x4_t dk[4], dv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) dk[j] = dv[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            dv[db] = Mfma<T>::run(tr_frag<T, HD>(dop, c, db, li, lg), pf[c], dv[db]);
            dk[db] = Mfma<T>::run(tr_frag<T, HD>(qp, c, db, li, lg), dsf[c], dk[db]);
        }
    }
    T* dkb = reinterpret_cast<T*>(p.dk) + (long long)b * p.T * ostride + hoff;
    T* dvb = reinterpret_cast<T*>(p.dv) + (long long)b * p.T * ostride + hoff;
    // column sums of this tile's dq / dk / dv: [8 waves][3][64] floats in the 12 KiB between the K image (kp, 20 KiB over
    // qs | dos) and the padded images — dead since S and dP were formed
    float* const cs = reinterpret_cast<float*>(smem + P_BYTES);
    auto colsum_rows = [&](const half4 (&v)[4], int t) {  // the wave's 16 rows of one tensor, as stored
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            f32x4_t r;
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = row_sum((float)v[db][j]);
            if (li == 15) *reinterpret_cast<f32x4_t*>(cs + (wid * 3 + t) * HD + db * 16 + lg * 4) = r;
        }
    };
    {
        half4 hk[4], hv[4];
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            hk[db] = __builtin_convertvector(dk[db] * p.scale, half4);
            hv[db] = __builtin_convertvector(dv[db], half4);
            *reinterpret_cast<half4*>(dkb + row * ostride + db * 16 + lg * 4) = hk[db];
            *reinterpret_cast<half4*>(dvb + row * ostride + db * 16 + lg * 4) = hv[db];
        }
        if (p.cs_partial) {
            colsum_rows(hk, 1);
            colsum_rows(hv, 2);
        }
    }

    __syncthreads();  // every wave has read the last of Q, dO and their transposes
#pragma unroll
    for (int c = 0; c < 4; ++c) {  // elements 0..3 / 4..7 of dsf[c]: queries (2c) 16 + 4 lg + 0..3 / (2c + 1) 16 + 4 lg + 0..3
        const half4 lo = {dsf[c][0], dsf[c][1], dsf[c][2], dsf[c][3]}, hi = {dsf[c][4], dsf[c][5], dsf[c][6], dsf[c][7]};
        *reinterpret_cast<half4*>(dst + row * DS_ROW + ((2 * c) * 16 + lg * 4) * 2) = lo;
        *reinterpret_cast<half4*>(dst + row * DS_ROW + ((2 * c + 1) * 16 + lg * 4) * 2) = hi;
    }
    __syncthreads();
    // dQ^T[d][query] = sum_k K^T[d][k] dS^T[k][query] for the wave's query block `wid`
    f32x4_t dq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) dq[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const frag dsf = tr_frag_row<T, DS_ROW>(dst, c, wid, li, lg);
#pragma unroll
        for (int db = 0; db < 4; ++db) dq[db] = Mfma<T>::run(tr_frag<T, HD>(kp, c, db, li, lg), dsf, dq[db]);
    }
    T* dqb = reinterpret_cast<T*>(p.dq) + (long long)b * p.T * ostride + hoff;
    half4 hq[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        hq[db] = __builtin_convertvector(dq[db] * p.scale, half4);
        *reinterpret_cast<half4*>(dqb + row * ostride + db * 16 + lg * 4) = hq[db];
    }
    if (p.cs_partial) {
        colsum_rows(hq, 0);
        __syncthreads();
        if (tid < 3 * HD) {  // fixed order over the 8 waves: deterministic
            float acc = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) acc += cs[w * 3 * HD + tid];
            p.cs_partial[((long long)b * p.H + h) * 3 * HD + tid] = acc;
        }
    }
}

// out[t][s][h * 64 + d] = sum over the sequences of sample s of partial[b][h][t][d]; grid = (3 H, S), 64 threads
__global__ __launch_bounds__(64) void attention_colsum_finish_kernel(const float* __restrict__ partial, int seq_per_sample, int H,
                                                                     int S, float* __restrict__ out) {
    const int t = blockIdx.x / H, h = blockIdx.x % H, s = blockIdx.y, d = threadIdx.x;
    float acc = 0.f;
    for (int i = 0; i < seq_per_sample; ++i)
        acc += partial[(((long long)s * seq_per_sample + i) * H + h) * 3 * HD + t * HD + d];
    out[((long long)t * S + s) * H * HD + h * HD + d] = acc;
}

// one tile (T = 128): dQ, dK, dV in one launch; else the dq kernel, then the dk/dv kernel that reads its delta
template <typename T, bool DROP>
void launch(const BwdParams& p, bool one_tile, hipStream_t stream) {
    const dim3 grid(p.T / TT, p.H, p.B);
    if (one_tile) {
        hipLaunchKernelGGL((attention_bwd_tile_kernel<T, DROP>), grid, dim3(512), 0, stream, p);
    } else {
        hipLaunchKernelGGL((attention_bwd_dq_kernel<T, DROP>), grid, dim3(256), 0, stream, p);
        hipLaunchKernelGGL((attention_bwd_dkv_kernel<T, DROP>), grid, dim3(512), 0, stream, p);
    }
}

// T % 128 != 0: the TAIL forms of the dq kernel and of the dk/dv kernel that reads its delta, over ceil(T / 128) tiles
template <typename T, bool DROP>
void launch_tail(const BwdParams& p, hipStream_t stream) {
    const dim3 grid((p.T + TT - 1) / TT, p.H, p.B);
    hipLaunchKernelGGL((attention_bwd_dq_kernel<T, DROP, true>), grid, dim3(256), 0, stream, p);
    hipLaunchKernelGGL((attention_bwd_dkv_kernel<T, DROP, true>), grid, dim3(512), 0, stream, p);
}

}  // namespace

// the three entries' shared worker: d_keep_bits / inv_keep for the dropout entries, the rest for the column sums
static int attention_bwd(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                         const void* d_out, const void* d_dout, const float* d_lse, float* d_delta, void* d_dq, void* d_dk,
                         void* d_dv, int dtype, int B, int T, int H, int head_dim, long long token_stride, float scaling,
                         hipStream_t stream, const uint32_t* d_keep_bits = nullptr, float inv_keep = 1.0f, int samples = 0,
                         float* d_cs_partial = nullptr, float* d_colsum = nullptr) {
    if (!d_q || !d_k || !d_v || !d_out || !d_dout || !d_lse || !d_delta || !d_dq || !d_dk || !d_dv)
        BF_FAIL("bf_attention_bwd: NULL argument");
    if (d_colsum && (T != TT || !d_cs_partial || samples < 1 || B % samples || samples > 65535))
        BF_FAIL("bf_attention_bwd: column sums need one-tile sequences (T = %d), a partial buffer and B %% samples == 0", TT);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) BF_FAIL("bf_attention_bwd: dtype must be bf16 or fp16");
    if (head_dim != HD) BF_FAIL("bf_attention_bwd: head size %d (only %d)", head_dim, HD);
    if (B < 1 || H < 1 || T < TT || T % TT) BF_FAIL("bf_attention_bwd: T=%d must be a positive multiple of %d", T, TT);
    if (B > 65535 || H > 65535) BF_FAIL("bf_attention_bwd: B or H exceeds the grid");
    if (token_stride < (long long)H * HD || token_stride % 8) BF_FAIL("bf_attention_bwd: bad token stride %lld", token_stride);
    const uintptr_t al = (uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out | (uintptr_t)d_dout |
                         (uintptr_t)d_dq | (uintptr_t)d_dk | (uintptr_t)d_dv | (uintptr_t)d_lse | (uintptr_t)d_delta;
    if (al & 15) BF_FAIL("bf_attention_bwd: pointers must be 16-byte aligned");
    if (d_mask && ((uintptr_t)d_mask & 15)) BF_FAIL("bf_attention_bwd: mask must be 16-byte aligned");
    BwdParams p;
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.mask = d_mask;
    p.mask_off = d_mask_off;
    p.o = d_out;
    p.dout = d_dout;
    p.lse = d_lse;
    p.delta = d_delta;
    p.dq = d_dq;
    p.dk = d_dk;
    p.dv = d_dv;
    p.tok_stride = token_stride;
    p.B = B;
    p.T = T;
    p.H = H;
    p.scale = scaling;
    p.scale_log2e = scaling * LOG2E;
    p.keep_bits = d_keep_bits;
    p.inv_keep = inv_keep;
    p.cs_partial = d_colsum ? d_cs_partial : nullptr;
    if (d_keep_bits && ((uintptr_t)d_keep_bits & 3)) BF_FAIL("bf_attention_bwd: keep bits must be 4-byte aligned");
    if (dtype == BF_DT_BF16) {
        if (d_keep_bits) launch<__bf16, true>(p, T == TT, stream);
        else launch<__bf16, false>(p, T == TT, stream);
    } else {
        if (d_keep_bits) launch<_Float16, true>(p, T == TT, stream);
        else launch<_Float16, false>(p, T == TT, stream);
    }
    if (d_colsum)
        hipLaunchKernelGGL(attention_colsum_finish_kernel, dim3(3 * H, samples), dim3(64), 0, stream, d_cs_partial, B / samples,
                           H, samples, d_colsum);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_attention_bwd(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                     const void* d_out, const void* d_dout, const float* d_lse, float* d_delta, void* d_dq, void* d_dk,
                     void* d_dv, int dtype, int B, int T, int H, int head_dim, int64_t token_stride, float scaling,
                     void* stream) {
    return attention_bwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta, d_dq, d_dk, d_dv, dtype, B, T, H,
                         head_dim, token_stride, scaling, (hipStream_t)stream);
}

int bf_attention_bwd_dropout(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                             const void* d_out, const void* d_dout, const float* d_lse, float* d_delta, void* d_dq, void* d_dk,
                             void* d_dv, int dtype, int B, int T, int H, int head_dim, int64_t token_stride, float scaling,
                             float p_drop, const uint32_t* d_keep_bits, void* stream) {
    if (!(p_drop >= 0.f) || !(p_drop < 1.f)) BF_FAIL("bf_attention_bwd_dropout: p must be in [0, 1) (got %g)", p_drop);
    const bf_dropout_t d = bf_make_dropout(p_drop, 0, 0, 0);
    if (d.thresh && !d_keep_bits) BF_FAIL("bf_attention_bwd_dropout: the forward's keep bits are needed");
    return attention_bwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta, d_dq, d_dk, d_dv, dtype, B, T, H,
                         head_dim, token_stride, scaling, (hipStream_t)stream, d.thresh ? d_keep_bits : nullptr, d.inv_keep);
}

int bf_attention_bwd_colsum(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                            const void* d_out, const void* d_dout, const float* d_lse, float* d_delta, void* d_dq, void* d_dk,
                            void* d_dv, int dtype, int B, int T, int H, int head_dim, int64_t token_stride, float scaling,
                            float p_drop, const uint32_t* d_keep_bits, int samples, float* d_partial, float* d_colsum,
                            void* stream) {
    if (!(p_drop >= 0.f) || !(p_drop < 1.f)) BF_FAIL("bf_attention_bwd_colsum: p must be in [0, 1) (got %g)", p_drop);
    if (!d_partial || !d_colsum) BF_FAIL("bf_attention_bwd_colsum: needs d_partial ([B][H][3][64] fp32) and d_colsum ([3][samples][H*64] fp32)");
    const bf_dropout_t d = bf_make_dropout(p_drop, 0, 0, 0);
    if (d.thresh && !d_keep_bits) BF_FAIL("bf_attention_bwd_colsum: the forward's keep bits are needed");
    return attention_bwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta, d_dq, d_dk, d_dv, dtype, B, T, H,
                         head_dim, token_stride, scaling, (hipStream_t)stream, d.thresh ? d_keep_bits : nullptr, d.inv_keep,
                         samples, d_partial, d_colsum);
}

// ------------------------------------------------------------------------------- any T >= 1 (bayeformers_amd_encoder_any.h)
// T % 128 == 0: the sibling's own worker, kernels and bits (T = 128: the one-tile kernel).  Otherwise the TAIL forms of the
// dq and dk/dv kernels; their mask, lse and delta accesses are 4 bytes wide.
static int attention_bwd_any(const char* what, const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                             const uint8_t* d_mask_off, const void* d_out, const void* d_dout, const float* d_lse,
                             float* d_delta, void* d_dq, void* d_dk, void* d_dv, int dtype, int B, int T, int H, int head_dim,
                             long long token_stride, float scaling, hipStream_t stream, const uint32_t* d_keep_bits = nullptr,
                             float inv_keep = 1.0f) {
    if (T >= TT && T % TT == 0)
        return attention_bwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta, d_dq, d_dk, d_dv, dtype, B, T, H,
                             head_dim, token_stride, scaling, stream, d_keep_bits, inv_keep);
    if (!d_q || !d_k || !d_v || !d_out || !d_dout || !d_lse || !d_delta || !d_dq || !d_dk || !d_dv)
        BF_FAIL("%s: NULL argument", what);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) BF_FAIL("%s: dtype must be bf16 or fp16", what);
    if (head_dim != HD) BF_FAIL("%s: head size %d (only %d)", what, head_dim, HD);
    if (B < 1 || H < 1 || T < 1) BF_FAIL("%s: B=%d, H=%d, T=%d must be positive", what, B, H, T);
    if (T > 0x7fffff00) BF_FAIL("%s: T=%d exceeds the key index", what, T);
    if (B > 65535 || H > 65535) BF_FAIL("%s: B or H exceeds the grid", what);
    if (token_stride < (long long)H * HD || token_stride % 8) BF_FAIL("%s: bad token stride %lld", what, token_stride);
    const uintptr_t al = (uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out | (uintptr_t)d_dout |
                         (uintptr_t)d_dq | (uintptr_t)d_dk | (uintptr_t)d_dv;
    if (al & 15) BF_FAIL("%s: pointers must be 16-byte aligned", what);
    if (((uintptr_t)d_lse | (uintptr_t)d_delta) & 3) BF_FAIL("%s: lse and delta must be 4-byte aligned", what);
    if (d_mask && ((uintptr_t)d_mask & 3)) BF_FAIL("%s: mask must be 4-byte aligned", what);
    if (d_keep_bits && ((uintptr_t)d_keep_bits & 3)) BF_FAIL("%s: keep bits must be 4-byte aligned", what);
    BwdParams p;
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.mask = d_mask;
    p.mask_off = d_mask_off;
    p.o = d_out;
    p.dout = d_dout;
    p.lse = d_lse;
    p.delta = d_delta;
    p.dq = d_dq;
    p.dk = d_dk;
    p.dv = d_dv;
    p.tok_stride = token_stride;
    p.B = B;
    p.T = T;
    p.H = H;
    p.scale = scaling;
    p.scale_log2e = scaling * LOG2E;
    p.keep_bits = d_keep_bits;
    p.inv_keep = inv_keep;
    p.cs_partial = nullptr;
    if (dtype == BF_DT_BF16) {
        if (d_keep_bits) launch_tail<__bf16, true>(p, stream);
        else launch_tail<__bf16, false>(p, stream);
    } else {
        if (d_keep_bits) launch_tail<_Float16, true>(p, stream);
        else launch_tail<_Float16, false>(p, stream);
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_attention_bwd_any(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                         const void* d_out, const void* d_dout, const float* d_lse, float* d_delta, void* d_dq, void* d_dk,
                         void* d_dv, int dtype, int B, int T, int H, int head_dim, int64_t token_stride, float scaling,
                         void* stream) {
    return attention_bwd_any("bf_attention_bwd_any", d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta, d_dq,
                             d_dk, d_dv, dtype, B, T, H, head_dim, token_stride, scaling, (hipStream_t)stream);
}

int bf_attention_bwd_any_dropout(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                 const uint8_t* d_mask_off, const void* d_out, const void* d_dout, const float* d_lse,
                                 float* d_delta, void* d_dq, void* d_dk, void* d_dv, int dtype, int B, int T, int H,
                                 int head_dim, int64_t token_stride, float scaling, float p_drop, const uint32_t* d_keep_bits,
                                 void* stream) {
    if (!(p_drop >= 0.f) || !(p_drop < 1.f)) BF_FAIL("bf_attention_bwd_any_dropout: p must be in [0, 1) (got %g)", p_drop);
    const bf_dropout_t d = bf_make_dropout(p_drop, 0, 0, 0);
    if (d.thresh && !d_keep_bits) BF_FAIL("bf_attention_bwd_any_dropout: the forward's keep bits are needed");
    return attention_bwd_any("bf_attention_bwd_any_dropout", d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta,
                             d_dq, d_dk, d_dv, dtype, B, T, H, head_dim, token_stride, scaling, (hipStream_t)stream,
                             d.thresh ? d_keep_bits : nullptr, d.inv_keep);
}
