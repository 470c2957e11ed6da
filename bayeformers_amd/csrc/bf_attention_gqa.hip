// bf_attention_gqa.hip — causal and grouped-query attention, forward and backward, for the decoder-only transformers
// the reference converts (to_bayesian turns every nn.Linear of e.g. HF LlamaForCausalLM into a Bayesian layer:
// /root/reference/bayeformers/convert.py; the attention between q/k/v_proj and o_proj is the wrapped model's own).
//
//   out[b,t,h,:] = sum_{j <= t (causal), key j visible in b} softmax_j(scale q[b,t,h] . k[b,j,g] + mask[b,j]) v[b,j,g,:],
//   g = h / (H / Hkv).
//
// Siblings of bf_attention.hip / bf_attention_bwd.hip (same online softmax; layouts and LDS images: bf_attention_tiles.h), made
// generic over the head size (64, 128, 256), the key / query tile of the inner loop, causality and the K/V head group, and
// reading q, k and v through their own (batch, head, token) strides.  The BERT entries keep their own kernels: the new
// entry hands the case they cover (non-causal, one K/V head per query head, head size 64, packed heads) to them.
//   * forward — one 256-thread workgroup per (128 queries, head, sequence), 4 waves x 32 queries, walking key tiles of KT.
//     Causal: query tile i visits key tiles up to the diagonal only, the tiles that cross it are masked element-wise, and
//     a wave skips the 16-query blocks a tile lies wholly above.  The grid runs the query tiles in reverse on its slowest
//     dimension: the heaviest workgroups are dispatched first, spread over the XCDs.
//   * dq kernel — as the forward (plus delta = <dO, O> per query), key tiles of KT.
//   * dk/dv kernel — one 512-thread workgroup per (128 keys, K/V head, sequence), 8 waves x 16 keys, walking the query
//     tiles (QT) of every query head of the group in turn: the group sum stays in registers, no atomics, deterministic.
//     Causal: key tile j visits query tiles from j on; the low key tiles (heavy) come first in the grid.
//     Head size 256 (Gemma, Qwen3-Next): 256 threads per 64 keys, and so twice the key tiles in the grid (Shape).
// Rows with no visible key (left padding under a causal mask) output 0 and store lse = +inf, so the backward recomputes
// P = 0 for them and their gradients are 0.
#include "bf_attention_tiles.h"

#include <type_traits>

namespace {

constexpr int TQ = 128;   // queries per forward / dq workgroup, keys per dk/dv workgroup (head size 256: Shape)

// Tile shapes.  Head size 64: the BERT kernels' (128-key tiles; dk/dv over 128-query tiles, 72 KiB of LDS, 2 workgroups per
// CU).  Head size 128: 128-key tiles in the forward (68 KiB of LDS: 2 workgroups per CU), 64-key tiles in the dq kernel and
// 64-query tiles in the dk/dv kernel (50 / 68 KiB), whose 128-row variants would hold one workgroup per CU by LDS alone.
// Head size 256 keeps a wave's 32 queries of q, dO and dq (dq kernel), or its 16 keys of k, v, dk and dv (dk/dv kernel), in
// more than the 256 registers that two waves per SIMD leave each lane, so every kernel holds one wave per SIMD, each lane with
// the whole 512-register file (accumulators in the AGPR half), no scratch: the forward over 64-key tiles (66 KiB of LDS), the
// dq kernel at one workgroup per CU (DQ_MINB) over 32-key tiles (49 KiB; with 64 its causal form spills 8 - 20 bytes a lane),
// the dk/dv kernel with 4 waves over 64 keys (DKV_KEYS: 16 keys a wave) and 64-query tiles (133 KiB of the CU's 160).
template <int HD>
struct Shape;
template <>
struct Shape<64> {
    static constexpr int FWD_KT = FwdShape<64>::KT, FWD_MINB = FwdShape<64>::MINB, DQ_KT = 128, DKV_QT = 128, DKV_MINB = 2;
    static constexpr int DQ_MINB = 2, DKV_KEYS = TQ;
};
// (the head-128 alternatives were measured: profiles/causal_attention.md)
template <>
struct Shape<128> {
    static constexpr int FWD_KT = FwdShape<128>::KT, FWD_MINB = FwdShape<128>::MINB, DQ_KT = 64, DKV_QT = 64, DKV_MINB = 1;
    static constexpr int DQ_MINB = 2, DKV_KEYS = TQ;
};
// (measured against the framework's attention: profiles/head256_attention.md)
template <>
struct Shape<256> {
    static constexpr int FWD_KT = FwdShape<256>::KT, FWD_MINB = FwdShape<256>::MINB, DQ_KT = 32, DKV_QT = 64, DKV_MINB = 1;
    static constexpr int DQ_MINB = 1, DKV_KEYS = 64;
};

struct GqaParams {
    const void* q;
    const void* k;
    const void* v;
    const float* mask;              // [B][T] additive over the keys, nullable
    const unsigned char* mask_off;  // nullable device flag: non-zero = skip the mask
    const void* o;                  // backward: the forward's output, [B][T][H][D]
    const void* dout;               // backward: its gradient, [B][T][H][D]
    void* out;                      // forward: [B][T][H][D]
    float* lse;                     // [B][H][T], log2 units
    float* delta;                   // [B][H][T]
    void* dq;                       // [B][T][H][D]
    void* dk;                       // [B][T][Hkv][D]
    void* dv;
    long long qs[3], ks[3], vs[3];  // (batch, head, token) element strides
    int B, T, H, Hkv, group;
    int window;                     // LOCAL: query i sees keys i - window + 1 .. i (1 <= window <= T)
    float scale, scale_log2e;
};

// The CAP instantiations soft-cap the logits (Gemma 2): the score is softcap * tanh(scale q.k / softcap) in place of
// scale q.k, in log2 units th * cap_log2e with th = tanh(s * cap_x); the mask and the -inf of the diagonal, the window
// edge, the tail and the unseen keys come after the cap, and the online softmax is the same.  The backward recomputes th
// with P and multiplies dS by d tanh = 1 - th^2 (the dk/dv kernel's P for dv goes without).  A compile-time flag with a
// parameter block of its own (SoftCap: bf_attention_tiles.h); `if constexpr (CAP)` stands where the score is formed and
// where that factor is applied, nowhere else.
struct GqaCapParams : GqaParams, SoftCap {};
// The BAND instantiations run banded causal attention (packed sequences: include/bayeformers_amd_packed.h): query i sees
// key j iff lo[b][i] <= j <= i, and key j is seen by the queries j .. hi[b][j]; both bounds are non-decreasing along T, so
// a block's first row holds its least bound and its last row its greatest.  The forward and the dq kernel read lo, the
// dk/dv kernel hi: LOCAL with a bound that varies per row, and like it a compile-time flag with a parameter block and
// branches of its own (no key mask, no cap).  Rows >= T of a TAIL launch read the bound of row T - 1.
struct GqaBandParams : GqaParams {
    const int* lo;  // [B][T]
    const int* hi;  // [B][T], backward only
};
template <bool CAP, bool BAND = false>
using ParamsOf = std::conditional_t<BAND, GqaBandParams, std::conditional_t<CAP, GqaCapParams, GqaParams>>;

// The TAIL instantiations run a sequence whose length is no multiple of TQ (any T >= 1): the last tile's missing rows are
// never read or written.  A load of row >= T re-reads row T - 1 (finite values of the caller's, no branch), keys >= T get
// a score of -inf (P = 0), queries >= T contribute P = dS = 0 and nothing of theirs is stored: rows < T see the arithmetic
// of a launch zero-padded to the next multiple of TQ.  The T % TQ == 0 launches keep the instantiations without the flag.
template <bool TAIL>
__device__ __forceinline__ int tail_row(int row, int T) {
    return TAIL ? min(row, T - 1) : row;
}

template <bool TAIL, typename T, int HD, int NR, int NT>
__device__ __forceinline__ void stage_rows(const T* base, long long stride, int row0, int rows, char* swz, char* pad, int tid) {
    if (TAIL) stage_clamped<T, HD, NR, NT>(base, stride, row0, 0, rows - 1, swz, pad, tid);
    else stage<T, HD, NR, NT>(base, stride, row0, swz, pad, tid);
}

// A wave's bounds over its NB blocks of 16 rows (queries with lo, keys with hi): each lane's own row's (rows >= T of a TAIL
// launch: row T - 1's), wave-uniform copies of each block's first and last row's — the least and the greatest, the bounds
// being monotone — and whether the tile in hand crosses some row's bound.  The kernels touch it behind `BAND &&` or
// `if constexpr (BAND)` alone: in their other instantiations it is an object nobody reads or writes.
template <int NB>
struct Band {
    int row[NB], first[NB], last[NB];
    bool edge;
    template <bool TAIL>
    __device__ __forceinline__ void load(const int* bound, int r0, int li, int T) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            row[i] = bound[tail_row<TAIL>(r0 + i * 16 + li, T)];
            first[i] = __builtin_amdgcn_readlane(row[i], 0);
            last[i] = __builtin_amdgcn_readlane(row[i], 15);
        }
    }
};
// the first key tile of query tile qt: its first row's bound (clamped: the range stays inside the sequence)
template <int KT, typename P>
__device__ __forceinline__ int band_first_key(const P& p, int b, int qt) {
    if constexpr (std::is_same_v<P, GqaBandParams>)
        return max(0, __builtin_amdgcn_readfirstlane(p.lo[(long long)b * p.T + qt * TQ])) / KT * KT;
    else return 0;
}
// the end of the query tiles of a key tile whose last key is `key`: after the tile of the last query that sees it
template <int QT, typename P>
__device__ __forceinline__ int band_query_end(const P& p, int b, int key) {
    if constexpr (std::is_same_v<P, GqaBandParams>) {
        const int last = min(p.T - 1, __builtin_amdgcn_readfirstlane(p.hi[(long long)b * p.T + min(key, p.T - 1)]));
        return min(p.T, last / QT * QT + QT);
    } else return 0;
}

// ---------------------------------------------------------------------------------------------------- forward
template <typename T, int HD, int KT, bool CAUSAL, bool LOCAL, bool TAIL, bool CAP, int MINB, bool BAND = false>
__global__ __launch_bounds__(256, MINB) void gqa_fwd_kernel(const ParamsOf<CAP, BAND> p) {
    using frag = typename Mfma<T>::frag;
    using half4 = typename Mfma<T>::half4;
    constexpr int NDH = HD / 32, NDB = HD / 16, NKB = KT / 16;
    constexpr int K_BYTES = KT * Rows<HD>::SWZ, V_BYTES = KT * Rows<HD>::PAD;
    __shared__ __attribute__((aligned(16))) char smem[K_BYTES + V_BYTES + KT * 4];
    char* const ks = smem;
    char* const vs = smem + K_BYTES;
    float* const ms = reinterpret_cast<float*>(smem + K_BYTES + V_BYTES);  // this tile's key mask, log2 units
    const float* const mask = (p.mask && !(p.mask_off && *p.mask_off)) ? p.mask : nullptr;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int qt = (int)gridDim.z - 1 - (int)blockIdx.z;  // heavy query tiles first (see launch_fwd)
    const int q0 = qt * TQ + wid * 32, h = blockIdx.x, b = blockIdx.y, g = h / p.group;
    const T* qb = reinterpret_cast<const T*>(p.q) + b * p.qs[0] + h * p.qs[1];
    const T* kb = reinterpret_cast<const T*>(p.k) + b * p.ks[0] + g * p.ks[1];
    const T* vb = reinterpret_cast<const T*>(p.v) + b * p.vs[0] + g * p.vs[1];

    frag qf[2][NDH];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi)
#pragma unroll
        for (int dh = 0; dh < NDH; ++dh)
            qf[qi][dh] = *reinterpret_cast<const frag*>(qb + (long long)tail_row<TAIL>(q0 + qi * 16 + li, p.T) * p.qs[2] +
                                                        dh * 32 + lg * 8);

    f32x4_t o[2][NDB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NDB; ++j) o[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    SoftmaxRow run[2];

    const int kend = CAUSAL ? (TAIL ? min((qt + 1) * TQ, p.T) : (qt + 1) * TQ) : p.T;
    Band<2> lo;  // BAND: the lower bounds of the wave's queries
    if constexpr (BAND) lo.template load<TAIL>(p.lo + (long long)b * p.T, q0, li, p.T);
    // the tile of the tile's first window key (BAND: of its first visible key)
    const int kbeg = BAND ? band_first_key<KT>(p, b, qt) : LOCAL ? max(0, qt * TQ - p.window + 1) / KT * KT : 0;
    for (int key0 = kbeg; key0 < kend; key0 += KT) {
        if (key0 != kbeg) __syncthreads();
        stage_rows<TAIL, T, HD, KT, 256>(kb, p.ks[2], key0, p.T, ks, nullptr, tid);
        stage_rows<TAIL, T, HD, KT, 256>(vb, p.vs[2], key0, p.T, nullptr, vs, tid);
        if (TAIL) {  // the dense [B][T] rows are not 16-byte aligned: element-wise, with a bound
            if (mask && tid < KT) ms[tid] = key0 + tid < p.T ? mask[(long long)b * p.T + key0 + tid] * LOG2E : 0.f;
        } else if (mask && tid < KT / 4)
            *reinterpret_cast<f32x4_t*>(ms + tid * 4) =
                *reinterpret_cast<const f32x4_t*>(mask + (long long)b * p.T + key0 + tid * 4) * LOG2E;
        __syncthreads();

#pragma unroll
        for (int qi = 0; qi < 2; ++qi) {
            const int qr0 = q0 + qi * 16;  // the block's first query
            if (TAIL && qr0 >= p.T) continue;  // no query of the block exists (after the barriers: every wave stages)
            if (CAUSAL && key0 > qr0 + 15) continue;  // the tile lies wholly above the diagonal for these 16 queries
            if (LOCAL && key0 + KT - 1 < qr0 - p.window + 1) continue;  // ... or wholly before their windows
            if (BAND && key0 + KT - 1 < lo.first[qi]) continue;         // ... or wholly before their bounds
            f32x4_t s[NKB];
#pragma unroll
            for (int kbk = 0; kbk < NKB; ++kbk) {
                s[kbk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dh = 0; dh < NDH; ++dh) s[kbk] = Mfma<T>::run(row_frag<T, HD>(ks, kbk, dh, li, lg), qf[qi][dh], s[kbk]);
            }
            const bool diag = CAUSAL && key0 + KT - 1 > qr0;
            const bool edge = LOCAL && key0 < qr0 + 16 - p.window;  // the tile crosses a window's lower edge
            if constexpr (BAND) lo.edge = key0 < lo.last[qi];       // ... or some row's lower bound
            const bool past = TAIL && key0 + KT > p.T;              // the tile crosses the sequence's end
            float mx = -INFINITY;
#pragma unroll
            for (int kbk = 0; kbk < NKB; ++kbk) {
                f32x4_t mk = {0.f, 0.f, 0.f, 0.f};
                if (mask) mk = *reinterpret_cast<const f32x4_t*>(ms + kbk * 16 + lg * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (CAP) s[kbk][j] = fmaf(softcap_tanh(s[kbk][j] * p.cap_x), p.cap_log2e, mk[j]);
                    else s[kbk][j] = fmaf(s[kbk][j], p.scale_log2e, mk[j]);
                    if (diag && key0 + kbk * 16 + lg * 4 + j > qr0 + li) s[kbk][j] = -INFINITY;
                    if (edge && qr0 + li - (key0 + kbk * 16 + lg * 4 + j) >= p.window) s[kbk][j] = -INFINITY;
                    if (BAND && lo.edge && key0 + kbk * 16 + lg * 4 + j < lo.row[qi]) s[kbk][j] = -INFINITY;
                    if (past && key0 + kbk * 16 + lg * 4 + j >= p.T) s[kbk][j] = -INFINITY;
                    mx = fmaxf(mx, s[kbk][j]);
                }
            }
            softmax_pv_step<T, HD, KT>(s, mx, run[qi], o[qi], (lds_image)vs, li, lg);
        }
    }

    T* ob = reinterpret_cast<T*>(p.out) + ((long long)b * p.T * p.H + h) * HD;
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        const float inv = run[qi].sum > 0.f ? 1.0f / run[qi].sum : 0.f;
        if (TAIL && q0 + qi * 16 + li >= p.T) continue;  // rows >= T are never written
        if (p.lse && lg == 0)
            p.lse[((long long)b * p.H + h) * p.T + q0 + qi * 16 + li] =
                run[qi].sum > 0.f ? run[qi].max + __builtin_amdgcn_logf(run[qi].sum) : INFINITY;
        T* orow = ob + (long long)(q0 + qi * 16 + li) * p.H * HD;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
            *reinterpret_cast<half4*>(orow + db * 16 + lg * 4) = __builtin_convertvector(o[qi][db] * inv, half4);
    }
}

// ---------------------------------------------------------------------------------------------------- dQ (+ delta)
template <typename T, int HD, int KT, bool CAUSAL, bool LOCAL, bool TAIL, bool CAP, bool BAND = false>
__global__ __launch_bounds__(256, Shape<HD>::DQ_MINB) void gqa_bwd_dq_kernel(const ParamsOf<CAP, BAND> p) {
    using frag = typename Mfma<T>::frag;
    using half4 = typename Mfma<T>::half4;
    constexpr int NDH = HD / 32, NDB = HD / 16, NKB = KT / 16;
    constexpr int S_BYTES = KT * Rows<HD>::SWZ, P_BYTES = KT * Rows<HD>::PAD;
    __shared__ __attribute__((aligned(16))) char smem[2 * S_BYTES + P_BYTES + KT * 4];
    char* const ks = smem;                // K, swizzled: row operand of S^T
    char* const vs = smem + S_BYTES;      // V, swizzled: row operand of dP^T
    char* const kp = smem + 2 * S_BYTES;  // K, padded: K^T through the transpose read
    float* const ms = reinterpret_cast<float*>(smem + 2 * S_BYTES + P_BYTES);
    const float* const mask = (p.mask && !(p.mask_off && *p.mask_off)) ? p.mask : nullptr;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int qt = (int)gridDim.z - 1 - (int)blockIdx.z;  // heavy query tiles first (see launch_fwd)
    const int q0 = qt * TQ + wid * 32, h = blockIdx.x, b = blockIdx.y, g = h / p.group;
    const T* qb = reinterpret_cast<const T*>(p.q) + b * p.qs[0] + h * p.qs[1];
    const T* kb = reinterpret_cast<const T*>(p.k) + b * p.ks[0] + g * p.ks[1];
    const T* vb = reinterpret_cast<const T*>(p.v) + b * p.vs[0] + g * p.vs[1];
    const long long ostride = (long long)p.H * HD;
    const long long ooff = (long long)b * p.T * ostride + (long long)h * HD;
    const T* ob = reinterpret_cast<const T*>(p.o) + ooff;
    const T* dob = reinterpret_cast<const T*>(p.dout) + ooff;

    frag qf[2][NDH], dof[2][NDH];
    float delta[2], lse[2];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        const long long q = tail_row<TAIL>(q0 + qi * 16 + li, p.T);  // TAIL: a missing row re-reads the last one
        float part = 0.f;
#pragma unroll
        for (int dh = 0; dh < NDH; ++dh) {
            qf[qi][dh] = *reinterpret_cast<const frag*>(qb + q * p.qs[2] + dh * 32 + lg * 8);
            dof[qi][dh] = *reinterpret_cast<const frag*>(dob + q * ostride + dh * 32 + lg * 8);
            const frag of = *reinterpret_cast<const frag*>(ob + q * ostride + dh * 32 + lg * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) part = fmaf((float)dof[qi][dh][e], (float)of[e], part);
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        delta[qi] = part;
        lse[qi] = p.lse[((long long)b * p.H + h) * p.T + q];
        if (lg == 0 && (!TAIL || q0 + qi * 16 + li < p.T)) p.delta[((long long)b * p.H + h) * p.T + q] = part;
    }

    f32x4_t dq[2][NDB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NDB; ++j) dq[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int kend = CAUSAL ? (TAIL ? min((qt + 1) * TQ, p.T) : (qt + 1) * TQ) : p.T;
    Band<2> lo;  // BAND: as in the forward
    if constexpr (BAND) lo.template load<TAIL>(p.lo + (long long)b * p.T, q0, li, p.T);
    const int kbeg = BAND ? band_first_key<KT>(p, b, qt) : LOCAL ? max(0, qt * TQ - p.window + 1) / KT * KT : 0;
    for (int key0 = kbeg; key0 < kend; key0 += KT) {
        if (key0 != kbeg) __syncthreads();
        stage_rows<TAIL, T, HD, KT, 256>(kb, p.ks[2], key0, p.T, ks, kp, tid);
        stage_rows<TAIL, T, HD, KT, 256>(vb, p.vs[2], key0, p.T, vs, nullptr, tid);
        if (TAIL) {  // the dense [B][T] rows are not 16-byte aligned: element-wise, with a bound
            if (mask && tid < KT) ms[tid] = key0 + tid < p.T ? mask[(long long)b * p.T + key0 + tid] * LOG2E : 0.f;
        } else if (mask && tid < KT / 4)
            *reinterpret_cast<f32x4_t*>(ms + tid * 4) =
                *reinterpret_cast<const f32x4_t*>(mask + (long long)b * p.T + key0 + tid * 4) * LOG2E;
        __syncthreads();
#pragma unroll
        for (int qi = 0; qi < 2; ++qi) {
            const int qr0 = q0 + qi * 16;
            if (TAIL && qr0 >= p.T) continue;
            if (CAUSAL && key0 > qr0 + 15) continue;
            if (LOCAL && key0 + KT - 1 < qr0 - p.window + 1) continue;
            if (BAND && key0 + KT - 1 < lo.first[qi]) continue;
            f32x4_t s[NKB], dp[NKB];
#pragma unroll
            for (int kbk = 0; kbk < NKB; ++kbk) {
                s[kbk] = dp[kbk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dh = 0; dh < NDH; ++dh) {
                    s[kbk] = Mfma<T>::run(row_frag<T, HD>(ks, kbk, dh, li, lg), qf[qi][dh], s[kbk]);
                    dp[kbk] = Mfma<T>::run(row_frag<T, HD>(vs, kbk, dh, li, lg), dof[qi][dh], dp[kbk]);
                }
            }
            const bool diag = CAUSAL && key0 + KT - 1 > qr0;
            const bool edge = LOCAL && key0 < qr0 + 16 - p.window;
            if constexpr (BAND) lo.edge = key0 < lo.last[qi];
            const bool past = TAIL && key0 + KT > p.T;
#pragma unroll
            for (int kbk = 0; kbk < NKB; ++kbk) {
                f32x4_t mk = {0.f, 0.f, 0.f, 0.f};
                if (mask) mk = *reinterpret_cast<const f32x4_t*>(ms + kbk * 16 + lg * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    [[maybe_unused]] float th = 0.f;  // CAP: tanh(scale q.k / softcap)
                    float pr;
                    if constexpr (CAP) {
                        th = softcap_tanh(s[kbk][j] * p.cap_x);
                        pr = __builtin_amdgcn_exp2f(fmaf(th, p.cap_log2e, mk[j]) - lse[qi]);
                    } else pr = __builtin_amdgcn_exp2f(fmaf(s[kbk][j], p.scale_log2e, mk[j]) - lse[qi]);
                    if (diag && key0 + kbk * 16 + lg * 4 + j > qr0 + li) pr = 0.f;
                    if (edge && qr0 + li - (key0 + kbk * 16 + lg * 4 + j) >= p.window) pr = 0.f;
                    if (BAND && lo.edge && key0 + kbk * 16 + lg * 4 + j < lo.row[qi]) pr = 0.f;
                    if (past && key0 + kbk * 16 + lg * 4 + j >= p.T) pr = 0.f;
                    s[kbk][j] = pr * (dp[kbk][j] - delta[qi]);  // dS^T
                    if constexpr (CAP) s[kbk][j] *= fmaf(-th, th, 1.0f);  // ... through the cap
                }
            }
#pragma unroll
            for (int c = 0; c < KT / 32; ++c) {
                const frag dsf = pack2<T>(s[2 * c], s[2 * c + 1]);
#pragma unroll
                for (int db = 0; db < NDB; ++db) dq[qi][db] = Mfma<T>::run(tr_frag<T, HD>(kp, c, db, li, lg), dsf, dq[qi][db]);
            }
        }
    }
    T* dqb = reinterpret_cast<T*>(p.dq) + ooff;
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        if (TAIL && q0 + qi * 16 + li >= p.T) continue;
        T* row = dqb + (long long)(q0 + qi * 16 + li) * ostride;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
            *reinterpret_cast<half4*>(row + db * 16 + lg * 4) = __builtin_convertvector(dq[qi][db] * p.scale, half4);
    }
}

// ---------------------------------------------------------------------------------------------------- dK, dV
template <typename T, int HD, int QT, bool CAUSAL, bool LOCAL, bool TAIL, bool CAP, int MINB, bool BAND = false>
__global__ __launch_bounds__(Shape<HD>::DKV_KEYS * 4, MINB) void gqa_bwd_dkv_kernel(const ParamsOf<CAP, BAND> p) {
    using frag = typename Mfma<T>::frag;
    using half4 = typename Mfma<T>::half4;
    constexpr int NDH = HD / 32, NDB = HD / 16, NQB = QT / 16;
    constexpr int KEYS = Shape<HD>::DKV_KEYS, NT = KEYS * 4;  // keys per workgroup: 16 a wave
    constexpr int S_BYTES = QT * Rows<HD>::SWZ, P_BYTES = QT * Rows<HD>::PAD;
    __shared__ __attribute__((aligned(16))) char smem[2 * S_BYTES + 2 * P_BYTES + 2 * QT * 4];
    char* const qs = smem;                           // Q, swizzled: row operand of S
    char* const dos = smem + S_BYTES;                // dO, swizzled: row operand of dP
    char* const qp = smem + 2 * S_BYTES;             // Q, padded: Q^T through the transpose read
    char* const dop = smem + 2 * S_BYTES + P_BYTES;  // dO, padded: dO^T through the transpose read
    float* const lse_s = reinterpret_cast<float*>(smem + 2 * S_BYTES + 2 * P_BYTES);
    float* const del_s = lse_s + QT;
    const float* const mask = (p.mask && !(p.mask_off && *p.mask_off)) ? p.mask : nullptr;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int kt = blockIdx.z, g = blockIdx.x, b = blockIdx.y;  // causal: the low key tiles are the heavy ones
    const int wkey0 = kt * KEYS + wid * 16;                      // the wave's first key
    const long long key = wkey0 + li;
    const long long krow = tail_row<TAIL>(wkey0 + li, p.T);  // TAIL: a missing key re-reads the last one and is not stored
    const T* kb = reinterpret_cast<const T*>(p.k) + b * p.ks[0] + g * p.ks[1];
    const T* vb = reinterpret_cast<const T*>(p.v) + b * p.vs[0] + g * p.vs[1];
    const long long ostride = (long long)p.H * HD;

    frag kf[NDH], vf[NDH];
#pragma unroll
    for (int dh = 0; dh < NDH; ++dh) {
        kf[dh] = *reinterpret_cast<const frag*>(kb + krow * p.ks[2] + dh * 32 + lg * 8);
        vf[dh] = *reinterpret_cast<const frag*>(vb + krow * p.vs[2] + dh * 32 + lg * 8);
    }
    const float mk = mask ? mask[(long long)b * p.T + krow] * LOG2E : 0.f;
    f32x4_t dk[NDB], dv[NDB];
#pragma unroll
    for (int j = 0; j < NDB; ++j) dk[j] = dv[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int qbeg = CAUSAL ? kt * KEYS : 0;
    Band<1> hi;  // BAND: the upper bounds of the wave's keys
    if constexpr (BAND) hi.template load<TAIL>(p.hi + (long long)b * p.T, wkey0, li, p.T);
    // LOCAL, BAND: up to the query tile of the last query that sees the tile's last key
    const int qend = BAND    ? band_query_end<QT>(p, b, kt * KEYS + KEYS - 1)
                     : LOCAL ? min(p.T, (kt * KEYS + KEYS - 1 + p.window - 1) / QT * QT + QT)
                             : p.T;
    bool first = true;
    for (int h = g * p.group; h < (g + 1) * p.group; ++h) {  // the group's query heads, in order: a fixed summation order
        const T* qb = reinterpret_cast<const T*>(p.q) + b * p.qs[0] + h * p.qs[1];
        const T* dob = reinterpret_cast<const T*>(p.dout) + (long long)b * p.T * ostride + (long long)h * HD;
        const float* lse_g = p.lse + ((long long)b * p.H + h) * p.T;
        const float* del_g = p.delta + ((long long)b * p.H + h) * p.T;
        for (int q0 = qbeg; q0 < qend; q0 += QT) {
            if (!first) __syncthreads();
            first = false;
            stage_rows<TAIL, T, HD, QT, NT>(qb, p.qs[2], q0, p.T, qs, qp, tid);
            stage_rows<TAIL, T, HD, QT, NT>(dob, ostride, q0, p.T, dos, dop, tid);
            if (TAIL) {  // dense ragged rows are not 16-byte aligned; a missing query gets lse = +inf, delta = 0: P = dS = 0
                if (tid < QT) {
                    const bool in = q0 + tid < p.T;
                    lse_s[tid] = in ? lse_g[q0 + tid] : INFINITY;
                    del_s[tid] = in ? del_g[q0 + tid] : 0.f;
                }
            } else if (tid < QT / 4) {
                *reinterpret_cast<f32x4_t*>(lse_s + tid * 4) = *reinterpret_cast<const f32x4_t*>(lse_g + q0 + tid * 4);
                *reinterpret_cast<f32x4_t*>(del_s + tid * 4) = *reinterpret_cast<const f32x4_t*>(del_g + q0 + tid * 4);
            }
            __syncthreads();
            if (TAIL && wkey0 >= p.T) continue;  // no key of the wave exists (after the barriers: every wave stages)
            if (CAUSAL && q0 + QT - 1 < wkey0) continue;  // every query of the tile precedes the wave's keys
            if (LOCAL && q0 > wkey0 + 15 + p.window - 1) continue;  // ... or lies past all their windows
            if (BAND && q0 > hi.last[0]) continue;                    // ... or past all their bounds
            f32x4_t s[NQB], dp[NQB];
#pragma unroll
            for (int qbk = 0; qbk < NQB; ++qbk) {
                s[qbk] = dp[qbk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dh = 0; dh < NDH; ++dh) {
                    s[qbk] = Mfma<T>::run(row_frag<T, HD>(qs, qbk, dh, li, lg), kf[dh], s[qbk]);
                    dp[qbk] = Mfma<T>::run(row_frag<T, HD>(dos, qbk, dh, li, lg), vf[dh], dp[qbk]);
                }
            }
            const bool diag = CAUSAL && q0 < wkey0 + 15;
            const bool edge = LOCAL && q0 + QT - 1 > wkey0 + p.window - 1;  // some query lies past a key's window
            if constexpr (BAND) hi.edge = q0 + QT - 1 > hi.first[0];        // ... or past a key's bound
            const bool past = TAIL && q0 + QT > p.T;                        // the tile crosses the sequence's end
#pragma unroll
            for (int qbk = 0; qbk < NQB; ++qbk) {
                const f32x4_t l4 = *reinterpret_cast<const f32x4_t*>(lse_s + qbk * 16 + lg * 4);
                const f32x4_t d4 = *reinterpret_cast<const f32x4_t*>(del_s + qbk * 16 + lg * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    [[maybe_unused]] float th = 0.f;  // CAP: tanh(scale q.k / softcap)
                    float pr;
                    if constexpr (CAP) {
                        th = softcap_tanh(s[qbk][j] * p.cap_x);
                        pr = __builtin_amdgcn_exp2f(fmaf(th, p.cap_log2e, mk) - l4[j]);
                    } else pr = __builtin_amdgcn_exp2f(fmaf(s[qbk][j], p.scale_log2e, mk) - l4[j]);
                    if (diag && q0 + qbk * 16 + lg * 4 + j < key) pr = 0.f;
                    if (edge && q0 + qbk * 16 + lg * 4 + j - key >= p.window) pr = 0.f;
                    if (BAND && hi.edge && q0 + qbk * 16 + lg * 4 + j > hi.row[0]) pr = 0.f;
                    if (past && q0 + qbk * 16 + lg * 4 + j >= p.T) pr = 0.f;
                    s[qbk][j] = pr;                          // P (CAP: for dv, without the factor)
                    dp[qbk][j] = pr * (dp[qbk][j] - d4[j]);  // dS
                    if constexpr (CAP) dp[qbk][j] *= fmaf(-th, th, 1.0f);  // ... through the cap
                }
            }
#pragma unroll
            for (int c = 0; c < QT / 32; ++c) {
                const frag pf = pack2<T>(s[2 * c], s[2 * c + 1]);
                const frag dsf = pack2<T>(dp[2 * c], dp[2 * c + 1]);
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    dv[db] = Mfma<T>::run(tr_frag<T, HD>(dop, c, db, li, lg), pf, dv[db]);
                    dk[db] = Mfma<T>::run(tr_frag<T, HD>(qp, c, db, li, lg), dsf, dk[db]);
                }
            }
        }
    }
    const long long kvstride = (long long)p.Hkv * HD;
    T* dkb = reinterpret_cast<T*>(p.dk) + ((long long)b * p.T * p.Hkv + g) * HD;
    T* dvb = reinterpret_cast<T*>(p.dv) + ((long long)b * p.T * p.Hkv + g) * HD;
    if (TAIL && key >= p.T) return;  // keys >= T are never written (no barrier follows)
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
        *reinterpret_cast<half4*>(dkb + key * kvstride + db * 16 + lg * 4) = __builtin_convertvector(dk[db] * p.scale, half4);
        *reinterpret_cast<half4*>(dvb + key * kvstride + db * 16 + lg * 4) = __builtin_convertvector(dv[db], half4);
    }
}

// The tile index is the grid's SLOWEST dimension: the hardware hands consecutive workgroups to the 8 XCDs in turn, so with
// the tiles fastest (as the BERT kernels order them) every XCD would get the tiles of one position — under a causal mask one
// XCD all the heaviest — while tiles-slowest issues the heavy tiles of every (head, sequence) first, spread over all XCDs.
// TAIL (T % TQ != 0): one more tile, whose rows >= T the kernels neither read nor write.
template <typename T, int HD, bool CAUSAL, bool LOCAL, bool TAIL, bool CAP, bool BAND = false>
void launch_fwd(const ParamsOf<CAP, BAND>& p, hipStream_t stream) {
    const dim3 grid(p.H, p.B, (p.T + TQ - 1) / TQ);
    hipLaunchKernelGGL((gqa_fwd_kernel<T, HD, Shape<HD>::FWD_KT, CAUSAL, LOCAL, TAIL, CAP, Shape<HD>::FWD_MINB, BAND>), grid,
                       dim3(256), 0, stream, p);
}

template <typename T, int HD, bool CAUSAL, bool LOCAL, bool TAIL, bool CAP, bool BAND = false>
void launch_bwd(const ParamsOf<CAP, BAND>& p, hipStream_t stream) {
    constexpr int KEYS = Shape<HD>::DKV_KEYS;  // keys per dk/dv workgroup: its own tile count
    hipLaunchKernelGGL((gqa_bwd_dq_kernel<T, HD, Shape<HD>::DQ_KT, CAUSAL, LOCAL, TAIL, CAP, BAND>),
                       dim3(p.H, p.B, (p.T + TQ - 1) / TQ), dim3(256), 0, stream, p);
    hipLaunchKernelGGL((gqa_bwd_dkv_kernel<T, HD, Shape<HD>::DKV_QT, CAUSAL, LOCAL, TAIL, CAP, Shape<HD>::DKV_MINB, BAND>),
                       dim3(p.Hkv, p.B, (p.T + KEYS - 1) / KEYS), dim3(KEYS * 4), 0, stream, p);
}

// The instantiations, by the parameter block: the plain one runs non-causal, causal and (local) sliding-window causal
// kernels, the soft-cap one causal kernels with or without a window, the band one causal kernels alone; each with and
// without a tail, at every dtype and head size.
template <typename P>
void launch(const P& p, int dtype, int D, bool causal, bool local, bool bwd, hipStream_t stream) {
    constexpr bool CAP = std::is_same_v<P, GqaCapParams>, BAND = std::is_same_v<P, GqaBandParams>;
    with_dtype(dtype, [&](auto tag) {
        with_head_size(D, [&](auto hd) {
            with_flag(p.T % TQ != 0, [&](auto tail) {
                auto run = [&](auto is_causal, auto is_local) {
                    using T = typename decltype(tag)::type;
                    constexpr int HD = decltype(hd)::value;
                    constexpr bool CAUSAL = decltype(is_causal)::value, LOCAL = decltype(is_local)::value;
                    constexpr bool TAIL = decltype(tail)::value;
                    if (bwd) launch_bwd<T, HD, CAUSAL, LOCAL, TAIL, CAP, BAND>(p, stream);
                    else launch_fwd<T, HD, CAUSAL, LOCAL, TAIL, CAP, BAND>(p, stream);
                };
                if constexpr (BAND) run(std::true_type{}, std::false_type{});
                else if (local) run(std::true_type{}, std::true_type{});
                else if (CAP || causal) run(std::true_type{}, std::false_type{});
                else if constexpr (!CAP) run(std::false_type{}, std::false_type{});
            });
        });
    });
}

// Validates the shape and fills the parameters' shape part; returns 0 or the BF_FAIL status
int fill_shape(const char* what, GqaParams& p, const bf_attn_gqa_t* s, int dtype, float scaling) {
    if (!s) BF_FAIL("%s: shape is NULL", what);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) BF_FAIL("%s: dtype must be bf16 or fp16", what);
    if (s->head_dim != 64 && s->head_dim != 128 && s->head_dim != 256)
        BF_FAIL("%s: head size %d (64, 128 or 256)", what, s->head_dim);
    if (s->B < 1 || s->H < 1 || s->Hkv < 1 || s->T < 1)
        BF_FAIL("%s: T=%d, B=%d, H=%d and Hkv=%d must be at least 1", what, s->T, s->B, s->H, s->Hkv);
    if (s->H % s->Hkv) BF_FAIL("%s: %d query heads do not divide into %d K/V head groups", what, s->H, s->Hkv);
    if (s->B > 65535 || s->H > 65535) BF_FAIL("%s: B or H exceeds the grid", what);
    if (s->causal != 0 && s->causal != 1) BF_FAIL("%s: causal must be 0 or 1", what);
    for (int i = 0; i < 3; ++i) {
        const int64_t st[3] = {s->q_stride[i], s->k_stride[i], s->v_stride[i]};
        for (int t = 0; t < 3; ++t)
            if (st[t] < 0 || st[t] % 8) BF_FAIL("%s: strides must be non-negative multiples of 8 elements", what);
    }
    p.B = s->B;
    p.T = s->T;
    p.H = s->H;
    p.Hkv = s->Hkv;
    p.group = s->H / s->Hkv;
    for (int i = 0; i < 3; ++i) {
        p.qs[i] = s->q_stride[i];
        p.ks[i] = s->k_stride[i];
        p.vs[i] = s->v_stride[i];
    }
    p.scale = scaling;
    p.scale_log2e = scaling * LOG2E;
    return 0;
}

// the case bf_attention_fwd / bf_attention_bwd take: non-causal, one K/V head per query head, head size 64, T a multiple of
// 128 (their own limit: a ragged T runs the generic kernels here), q / k / v element (b, t, h, d) at
// (b T + t) token_stride + 64 h + d with one token stride
bool bert_case(const bf_attn_gqa_t* s, long long* token_stride) {
    const long long ts = s->q_stride[2];
    const int64_t want[3] = {(int64_t)s->T * ts, 64, ts};
    for (int i = 0; i < 3; ++i)
        if (s->q_stride[i] != want[i] || s->k_stride[i] != want[i] || s->v_stride[i] != want[i]) return false;
    *token_stride = ts;
    return !s->causal && s->H == s->Hkv && s->head_dim == 64 && s->T % TQ == 0 && ts >= (long long)s->H * 64;
}

// The window entries' extra arguments: causal shapes only, window >= 1 (clamped to T: a wider window hides nothing)
int fill_window(const char* what, GqaParams& p, const bf_attn_gqa_t* s, int window) {
    if (window < 1) BF_FAIL("%s: window=%d must be at least 1", what, window);
    if (s->causal != 1) BF_FAIL("%s: a sliding window needs a causal shape (causal=%d)", what, s->causal);
    p.window = window < p.T ? window : p.T;
    return 0;
}

// The soft-cap entries' extra argument (finite and > 0: the entries checked it): causal shapes only
int fill_softcap(const char* what, GqaCapParams& p, const bf_attn_gqa_t* s, float softcap, float scaling) {
    if (s->causal != 1) BF_FAIL("%s: the soft-cap kernels need a causal shape (causal=%d)", what, s->causal);
    return p.fill(what, softcap, scaling);
}

// window 0: the plain entries; >= 1: the sliding-window ones.  softcap 0: no cap
int fwd_gqa(const char* what, const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
            const unsigned char* d_mask_off, void* d_out, float* d_lse, int dtype, const bf_attn_gqa_t* shape, int window,
            float softcap, float scaling, hipStream_t stream) {
    if (!d_q || !d_k || !d_v || !d_out) BF_FAIL("%s: NULL argument", what);
    GqaCapParams p = {};
    if (fill_shape(what, p, shape, dtype, scaling)) return 1;
    if (softcap != 0.f && fill_softcap(what, p, shape, softcap, scaling)) return 1;
    if (window && fill_window(what, p, shape, window)) return 1;
    long long ts;
    if (!window && bert_case(shape, &ts))
        return bf_attention_fwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_lse, dtype, shape->B, shape->T, shape->H, 64, ts,
                                scaling, stream);
    if (((uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out) & 15) BF_FAIL("%s: pointers must be 16-byte aligned", what);
    if ((d_mask && ((uintptr_t)d_mask & 15)) || (d_lse && ((uintptr_t)d_lse & 15))) BF_FAIL("%s: mask / lse must be 16-byte aligned", what);
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.mask = d_mask;
    p.mask_off = d_mask_off;
    p.out = d_out;
    p.lse = d_lse;
    if (softcap != 0.f) launch(p, dtype, shape->head_dim, true, window > 0, false, stream);
    else launch<GqaParams>(p, dtype, shape->head_dim, shape->causal, window > 0, false, stream);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bwd_gqa(const char* what, const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
            const unsigned char* d_mask_off, const void* d_out, const void* d_dout, const float* d_lse, float* d_delta,
            void* d_dq, void* d_dk, void* d_dv, int dtype, const bf_attn_gqa_t* shape, int window, float softcap,
            float scaling, hipStream_t stream) {
    if (!d_q || !d_k || !d_v || !d_out || !d_dout || !d_lse || !d_delta || !d_dq || !d_dk || !d_dv)
        BF_FAIL("%s: NULL argument", what);
    GqaCapParams p = {};
    if (fill_shape(what, p, shape, dtype, scaling)) return 1;
    if (softcap != 0.f && fill_softcap(what, p, shape, softcap, scaling)) return 1;
    if (window && fill_window(what, p, shape, window)) return 1;
    long long ts;
    if (!window && bert_case(shape, &ts))
        return bf_attention_bwd(d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta, d_dq, d_dk, d_dv, dtype,
                                shape->B, shape->T, shape->H, 64, ts, scaling, stream);
    const uintptr_t al = (uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out | (uintptr_t)d_dout |
                         (uintptr_t)d_dq | (uintptr_t)d_dk | (uintptr_t)d_dv | (uintptr_t)d_lse | (uintptr_t)d_delta;
    if (al & 15) BF_FAIL("%s: pointers must be 16-byte aligned", what);
    if (d_mask && ((uintptr_t)d_mask & 15)) BF_FAIL("%s: mask must be 16-byte aligned", what);
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.mask = d_mask;
    p.mask_off = d_mask_off;
    p.o = d_out;
    p.dout = d_dout;
    p.lse = const_cast<float*>(d_lse);
    p.delta = d_delta;
    p.dq = d_dq;
    p.dk = d_dk;
    p.dv = d_dv;
    if (softcap != 0.f) launch(p, dtype, shape->head_dim, true, window > 0, true, stream);
    else launch<GqaParams>(p, dtype, shape->head_dim, shape->causal, window > 0, true, stream);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// The band entries' shape: what fill_shape takes, causal only (the bounds sit under the diagonal)
int fill_band(const char* what, GqaBandParams& p, const bf_attn_gqa_t* s, int dtype, float scaling) {
    if (fill_shape(what, p, s, dtype, scaling)) return 1;
    if (s->causal != 1) BF_FAIL("%s: the band kernels need a causal shape (causal=%d)", what, s->causal);
    return 0;
}

}  // namespace

int bf_attention_fwd_gqa_band(const void* d_q, const void* d_k, const void* d_v, const int32_t* d_lo, void* d_out, float* d_lse,
                              int dtype, const bf_attn_gqa_t* shape, float scaling, void* stream) {
    const char* what = "bf_attention_fwd_gqa_band";
    if (!d_lo) BF_FAIL("%s: d_lo is NULL", what);
    if (!d_q || !d_k || !d_v || !d_out) BF_FAIL("%s: NULL argument", what);
    GqaBandParams p = {};
    if (fill_band(what, p, shape, dtype, scaling)) return 1;
    if (((uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out) & 15) BF_FAIL("%s: pointers must be 16-byte aligned", what);
    if (d_lse && ((uintptr_t)d_lse & 15)) BF_FAIL("%s: lse must be 16-byte aligned", what);
    if ((uintptr_t)d_lo & 3) BF_FAIL("%s: d_lo must be 4-byte aligned", what);
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.out = d_out;
    p.lse = d_lse;
    p.lo = d_lo;
    launch(p, dtype, shape->head_dim, true, false, false, (hipStream_t)stream);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_attention_bwd_gqa_band(const void* d_q, const void* d_k, const void* d_v, const int32_t* d_lo, const int32_t* d_hi,
                              const void* d_out, const void* d_dout, const float* d_lse, float* d_delta, void* d_dq, void* d_dk,
                              void* d_dv, int dtype, const bf_attn_gqa_t* shape, float scaling, void* stream) {
    const char* what = "bf_attention_bwd_gqa_band";
    if (!d_lo) BF_FAIL("%s: d_lo is NULL", what);
    if (!d_hi) BF_FAIL("%s: d_hi is NULL", what);
    if (!d_q || !d_k || !d_v || !d_out || !d_dout || !d_lse || !d_delta || !d_dq || !d_dk || !d_dv)
        BF_FAIL("%s: NULL argument", what);
    GqaBandParams p = {};
    if (fill_band(what, p, shape, dtype, scaling)) return 1;
    const uintptr_t al = (uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out | (uintptr_t)d_dout |
                         (uintptr_t)d_dq | (uintptr_t)d_dk | (uintptr_t)d_dv | (uintptr_t)d_lse | (uintptr_t)d_delta;
    if (al & 15) BF_FAIL("%s: pointers must be 16-byte aligned", what);
    if (((uintptr_t)d_lo | (uintptr_t)d_hi) & 3) BF_FAIL("%s: d_lo / d_hi must be 4-byte aligned", what);
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.o = d_out;
    p.dout = d_dout;
    p.lse = const_cast<float*>(d_lse);
    p.delta = d_delta;
    p.dq = d_dq;
    p.dk = d_dk;
    p.dv = d_dv;
    p.lo = d_lo;
    p.hi = d_hi;
    launch(p, dtype, shape->head_dim, true, false, true, (hipStream_t)stream);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_attention_fwd_gqa(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                         void* d_out, float* d_lse, int dtype, const bf_attn_gqa_t* shape, float scaling, void* stream) {
    return fwd_gqa("bf_attention_fwd_gqa", d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_lse, dtype, shape, 0, 0.f, scaling,
                   (hipStream_t)stream);
}

int bf_attention_fwd_gqa_window(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                const uint8_t* d_mask_off, void* d_out, float* d_lse, int dtype, const bf_attn_gqa_t* shape,
                                int32_t window, float scaling, void* stream) {
    const char* what = "bf_attention_fwd_gqa_window";
    if (window < 1) BF_FAIL("%s: window=%d must be at least 1", what, window);
    return fwd_gqa(what, d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_lse, dtype, shape, window, 0.f, scaling,
                   (hipStream_t)stream);
}

int bf_attention_bwd_gqa(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                         const void* d_out, const void* d_dout, const float* d_lse, float* d_delta, void* d_dq, void* d_dk,
                         void* d_dv, int dtype, const bf_attn_gqa_t* shape, float scaling, void* stream) {
    return bwd_gqa("bf_attention_bwd_gqa", d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta, d_dq, d_dk, d_dv,
                   dtype, shape, 0, 0.f, scaling, (hipStream_t)stream);
}

int bf_attention_bwd_gqa_window(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                const uint8_t* d_mask_off, const void* d_out, const void* d_dout, const float* d_lse,
                                float* d_delta, void* d_dq, void* d_dk, void* d_dv, int dtype, const bf_attn_gqa_t* shape,
                                int32_t window, float scaling, void* stream) {
    const char* what = "bf_attention_bwd_gqa_window";
    if (window < 1) BF_FAIL("%s: window=%d must be at least 1", what, window);
    return bwd_gqa(what, d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta, d_dq, d_dk, d_dv, dtype, shape,
                   window, 0.f, scaling, (hipStream_t)stream);
}

int bf_attention_fwd_gqa_softcap(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                 const uint8_t* d_mask_off, void* d_out, float* d_lse, int dtype, const bf_attn_gqa_t* shape,
                                 int32_t window, float softcap, float scaling, void* stream) {
    const char* what = "bf_attention_fwd_gqa_softcap";
    if (!(softcap > 0.f) || !(softcap < INFINITY)) BF_FAIL("%s: softcap=%g must be finite and positive", what, (double)softcap);
    if (window < 0) BF_FAIL("%s: window=%d must be at least 0 (0: no window)", what, window);
    return fwd_gqa(what, d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_lse, dtype, shape, window, softcap, scaling,
                   (hipStream_t)stream);
}

int bf_attention_bwd_gqa_softcap(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                 const uint8_t* d_mask_off, const void* d_out, const void* d_dout, const float* d_lse,
                                 float* d_delta, void* d_dq, void* d_dk, void* d_dv, int dtype, const bf_attn_gqa_t* shape,
                                 int32_t window, float softcap, float scaling, void* stream) {
    const char* what = "bf_attention_bwd_gqa_softcap";
    if (!(softcap > 0.f) || !(softcap < INFINITY)) BF_FAIL("%s: softcap=%g must be finite and positive", what, (double)softcap);
    if (window < 0) BF_FAIL("%s: window=%d must be at least 0 (0: no window)", what, window);
    return bwd_gqa(what, d_q, d_k, d_v, d_mask, d_mask_off, d_out, d_dout, d_lse, d_delta, d_dq, d_dk, d_dv, dtype, shape,
                   window, softcap, scaling, (hipStream_t)stream);
}
