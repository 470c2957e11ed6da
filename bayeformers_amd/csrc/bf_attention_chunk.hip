// bf_attention_chunk.hip — causal grouped-query attention of a CHUNK of new queries against a KV cache (inference only):
// Tq new queries per sequence (any Tq >= 1; the routing sends it the chunks of more than 16 queries the decode kernels do
// not take) against Tk cached keys, bottom-right aligned — the chunked prefill of sample_generate(prefill_chunk=...).
//
//   L = *kv_len clamped to [0, Tk] (the cache's fill after this call's append), or Tk without a kv_len; off = L - Tq;
//   query i has position p_i = off + i and sees the keys max(0, p_i - W + 1) .. p_i the key mask leaves visible:
//   out[n,i,h,:] = sum_j softmax_j(scale q[n,h,i] . k[n,g,j] + mask[n,j]) v[n,g,j,:],  g = h / (H / Hkv).
//   Keys at or past L are never read; a query with p_i < 0, or with every key hidden, gives 0.
//
// Shares with bf_attention_gqa.hip's forward the tiles, LDS images, fragment layouts, staging and the online-softmax step
// (bf_attention_tiles.h: FwdShape, stage_clamped, softmax_pv_step), and has its work split: one 256-thread workgroup per
// (128 queries, head, sequence), 4 waves x 32 queries, walking key tiles of KT; the heaviest query tiles first on the
// grid's slowest dimension.  Its own is what a query sees:
//   * the diagonal sits at key = off + query, which is aligned to no tile: every comparison carries off;
//   * the query tail (Tq % 128) and the key end (L, any value, a device scalar) are independent bounds.  A load of query
//     row >= Tq re-reads row Tq - 1, a load of key row >= L re-reads row L - 1 (finite values of the caller's, no branch);
//     such keys score -inf and nothing is stored for such queries;
//   * query tile t walks the keys [max(0, off + 128 t - W + 1) / KT * KT, min(L, off + q_last + 1));
//   * key_origin: the index in its sequence of the cache's key 0 (a sliding-window cache that kept the last W - 1 keys
//     only; 0 otherwise).  It changes no result in exact arithmetic: the key tiles are laid at multiples of KT of the
//     SEQUENCE's keys (tile index = (key + key_origin % KT) / KT), as the cache-free forward lays them, so a query's online
//     softmax runs over the same tiles in a chunk as in the whole-prompt forward and rounds the same way.  The slots of
//     the first tile before key 0 re-read row 0 and score -inf.
// CAP: the soft-capped logits of the CAP forward there (softcap * tanh(scale q.k / softcap), then the mask and the -inf's).
// KV8: k and v are the e4m3 rows of an FP8 cache (include/bayeformers_amd_kv8.h) with one fp32 scale per row.  Only the
// staging differs — 16 bytes are 16 features, dequantised in registers (bf_fp8.h: exact in bf16) into the same two LDS
// images by the write it shares with bf_attention_decode.hip's kv8 kernel (write_fp8) — so everything behind it is the
// bf16 kernel's and the result is bitwise that kernel's on the dequantised cache.
// Head size 256 keeps one wave per SIMD and 64-key tiles, as the forward there (its header gives the reasons).
#include "bf_attention_tiles.h"

#include "../../include/bayeformers_amd_chunk.h"

#include <type_traits>

namespace {

constexpr int TQ = 128;  // queries per workgroup

// key tile and workgroups per CU: the causal forward's (FwdShape, bf_attention_tiles.h), shared with bf_attention_gqa.hip
template <int HD>
using Shape = FwdShape<HD>;

struct ChunkParams {
    const void* q;
    const void* k;
    const void* v;
    const float* mask;              // [N][Tk] additive over the keys, nullable
    const unsigned char* mask_off;  // nullable device flag: non-zero = skip the mask
    const int64_t* kv_len;          // nullable device scalar: the filled keys L (Tk is then the capacity)
    void* out;                      // [N][Tq][H][D]
    long long qs[3], ks[3], vs[3];  // (batch, head, token) strides: elements (KV8: k and v in bytes, which are elements)
    int N, Tq, Tk, H, Hkv, group;
    int window;                     // LOCAL: query i sees keys p_i - window + 1 .. p_i
    int origin;                     // key 0's index in its sequence (tile alignment only)
    float scale_log2e;
};
struct ChunkCapParams : ChunkParams, SoftCap {};
struct ChunkKv8Params : ChunkCapParams {
    const float* k_scale;  // [N][Hkv][Tk]
    const float* v_scale;
};
template <bool CAP, bool KV8>
using ParamsOf = std::conditional_t<KV8, ChunkKv8Params, std::conditional_t<CAP, ChunkCapParams, ChunkParams>>;

// rows row0 .. row0 + NR - 1 of an FP8 cache head (rows of HD bytes, `stride` bytes apart, scales scale[row]) into the
// swizzled and / or the padded bf16 image; a row before 0 re-reads row 0, a row past `last` row `last`
template <int HD, int NR, int NT>
__device__ __forceinline__ void stage_kv8(const uint8_t* base, long long stride, const float* scale, int row0, int last,
                                          char* swz, char* pad, int tid) {
    constexpr int CPR = HD / 16;  // 16-byte chunks per row of bytes
    static_assert((NR * CPR) % NT == 0, "whole passes");
#pragma unroll
    for (int i = 0; i < NR * CPR / NT; ++i) {
        const int c = tid + NT * i, row = c / CPR, c16 = c % CPR, src = max(0, min(row0 + row, last));
        write_fp8<HD>(*reinterpret_cast<const u32x4_t*>(base + (long long)src * stride + c16 * 16), scale[src], row, c16, swz,
                      pad);
    }
}

template <typename T, int HD, int KT, bool LOCAL, bool CAP, bool KV8, int MINB>
__global__ __launch_bounds__(256, MINB) void chunk_fwd_kernel(const ParamsOf<CAP, KV8> p) {
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
    const int qt = (int)gridDim.z - 1 - (int)blockIdx.z;  // heavy query tiles first
    const int q0 = qt * TQ + wid * 32, h = blockIdx.x, n = blockIdx.y, g = h / p.group;
    const int L = filled_keys(p.kv_len, p.Tk);
    // Everything below counts keys and positions from `shift` slots before the cache's key 0, where a tile of the sequence
    // begins: key j is slot j + shift, the cache holds the slots [shift, end)
    const int shift = p.origin % KT, end = L + shift;
    const int off = end - p.Tq;  // the slot of query 0's position (below shift: the first queries see nothing)
    const T* qb = reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1];

    frag qf[2][NDH];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi)
#pragma unroll
        for (int dh = 0; dh < NDH; ++dh)
            qf[qi][dh] = *reinterpret_cast<const frag*>(qb + (long long)min(q0 + qi * 16 + li, p.Tq - 1) * p.qs[2] +
                                                        dh * 32 + lg * 8);

    f32x4_t o[2][NDB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NDB; ++j) o[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    SoftmaxRow run[2];

    // the tile's keys: up to its last query's position (and the fill), from the tile of its first query's first window key
    const int kend = min(end, off + min((qt + 1) * TQ, p.Tq));
    const int kbeg = LOCAL ? max(0, off + qt * TQ - p.window + 1) / KT * KT : 0;
    for (int key0 = kbeg; key0 < kend && L > 0; key0 += KT) {  // (L >= 1 in here: row L - 1 exists)
        if (key0 != kbeg) __syncthreads();
        if constexpr (KV8) {
            const long long srow = ((long long)n * p.Hkv + g) * p.Tk;
            stage_kv8<HD, KT, 256>(reinterpret_cast<const uint8_t*>(p.k) + n * p.ks[0] + g * p.ks[1], p.ks[2],
                                   p.k_scale + srow, key0 - shift, L - 1, ks, nullptr, tid);
            stage_kv8<HD, KT, 256>(reinterpret_cast<const uint8_t*>(p.v) + n * p.vs[0] + g * p.vs[1], p.vs[2],
                                   p.v_scale + srow, key0 - shift, L - 1, nullptr, vs, tid);
        } else {
            stage_clamped<T, HD, KT, 256>(reinterpret_cast<const T*>(p.k) + n * p.ks[0] + g * p.ks[1], p.ks[2], key0 - shift,
                                          0, L - 1, ks, nullptr, tid);
            stage_clamped<T, HD, KT, 256>(reinterpret_cast<const T*>(p.v) + n * p.vs[0] + g * p.vs[1], p.vs[2], key0 - shift,
                                          0, L - 1, nullptr, vs, tid);
        }
        // the dense [N][Tk] rows are not 16-byte aligned: element-wise, with a bound
        if (mask && tid < KT) {
            const int j = key0 - shift + tid;
            ms[tid] = j >= 0 && j < L ? mask[(long long)n * p.Tk + j] * LOG2E : 0.f;
        }
        __syncthreads();

#pragma unroll
        for (int qi = 0; qi < 2; ++qi) {
            const int qr0 = q0 + qi * 16;  // the block's first query
            const int pr0 = off + qr0;     // ... and its position
            if (qr0 >= p.Tq) continue;     // no query of the block exists (after the barriers: every wave stages)
            if (key0 > pr0 + 15) continue;  // the tile lies wholly above the diagonal for these 16 queries
            if (LOCAL && key0 + KT - 1 < pr0 - p.window + 1) continue;  // ... or wholly before their windows
            f32x4_t s[NKB];
#pragma unroll
            for (int kbk = 0; kbk < NKB; ++kbk) {
                s[kbk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dh = 0; dh < NDH; ++dh) s[kbk] = Mfma<T>::run(row_frag<T, HD>(ks, kbk, dh, li, lg), qf[qi][dh], s[kbk]);
            }
            const bool diag = key0 + KT - 1 > pr0;                   // the tile crosses the diagonal
            const bool edge = LOCAL && key0 < pr0 + 16 - p.window;   // ... or a window's lower edge
            const bool past = key0 + KT > end || key0 < shift;       // ... or the fill, or lies before key 0
            float mx = -INFINITY;
#pragma unroll
            for (int kbk = 0; kbk < NKB; ++kbk) {
                f32x4_t mk = {0.f, 0.f, 0.f, 0.f};
                if (mask) mk = *reinterpret_cast<const f32x4_t*>(ms + kbk * 16 + lg * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int key = key0 + kbk * 16 + lg * 4 + j;
                    if constexpr (CAP) s[kbk][j] = fmaf(softcap_tanh(s[kbk][j] * p.cap_x), p.cap_log2e, mk[j]);
                    else s[kbk][j] = fmaf(s[kbk][j], p.scale_log2e, mk[j]);
                    if (diag && key > pr0 + li) s[kbk][j] = -INFINITY;
                    if (edge && pr0 + li - key >= p.window) s[kbk][j] = -INFINITY;
                    if (past && (key >= end || key < shift)) s[kbk][j] = -INFINITY;
                    mx = fmaxf(mx, s[kbk][j]);
                }
            }
            softmax_pv_step<T, HD, KT>(s, mx, run[qi], o[qi], (lds_image)vs, li, lg);
        }
    }

    T* ob = reinterpret_cast<T*>(p.out) + ((long long)n * p.Tq * p.H + h) * HD;
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        const float inv = run[qi].sum > 0.f ? 1.0f / run[qi].sum : 0.f;
        if (q0 + qi * 16 + li >= p.Tq) continue;  // rows >= Tq are never written
        T* orow = ob + (long long)(q0 + qi * 16 + li) * p.H * HD;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
            *reinterpret_cast<half4*>(orow + db * 16 + lg * 4) = __builtin_convertvector(o[qi][db] * inv, half4);
    }
}

// The query tiles are the grid's SLOWEST dimension, last tile first: the heavy tiles of every (head, sequence) are
// dispatched first, spread over the XCDs (bf_attention_gqa.hip: launch_fwd)
// kv8: the FP8 instantiations (bf16 compute); each dtype and head size with and without a window and a cap
void launch(const ChunkKv8Params& p, int dtype, int D, bool cap, bool kv8, hipStream_t stream) {
    const dim3 grid(p.H, p.N, (p.Tq + TQ - 1) / TQ);
    with_head_size(D, [&](auto hd) {
        with_flag(p.window != 0, [&](auto local) {
            with_flag(cap, [&](auto capped) {
                auto run = [&](auto tag, auto fp8) {
                    using T = typename decltype(tag)::type;
                    constexpr int HD = decltype(hd)::value;
                    constexpr bool LOCAL = decltype(local)::value, CAP = decltype(capped)::value, KV8 = decltype(fp8)::value;
                    const ParamsOf<CAP, KV8>& kp = p;
                    hipLaunchKernelGGL((chunk_fwd_kernel<T, HD, Shape<HD>::KT, LOCAL, CAP, KV8, Shape<HD>::MINB>), grid,
                                       dim3(256), 0, stream, kp);
                };
                if (kv8) run(TypeTag<__bf16>{}, std::true_type{});
                else with_dtype(dtype, [&](auto tag) { run(tag, std::false_type{}); });
            });
        });
    });
}

// Validates the shape; returns 0 or the BF_FAIL status
int check_shape(const char* what, const bf_attn_decode_t* s, int dtype, bool kv8) {
    if (check_decode_dims(what, s, dtype, 0, kv8 ? 16 : 8)) return 1;
    if (s->N > 65535 || s->H > 65535 || (s->Tq + TQ - 1) / TQ > 65535) BF_FAIL("%s: N, H or Tq / 128 exceeds the grid", what);
    return check_decode_strides(what, s, kv8 ? 16 : 8);
}

// window 0: none.  softcap 0: no cap.  kv8: d_k / d_v are e4m3fn rows with the scales d_k_scale / d_v_scale (bf16 compute)
int chunk(const char* what, const void* d_q, const void* d_k, const void* d_v, const float* d_k_scale, const float* d_v_scale,
          const float* d_mask, const unsigned char* d_mask_off, const int64_t* d_kv_len, void* d_out, int dtype,
          const bf_attn_decode_t* shape, int window, int key_origin, float softcap, float scaling, hipStream_t stream,
          bool kv8) {
    if (!(softcap >= 0.f) || !(softcap < INFINITY))
        BF_FAIL("%s: softcap=%g must be finite and at least 0 (0: no cap)", what, (double)softcap);
    if (window < 0) BF_FAIL("%s: window=%d must be at least 0 (0: no window)", what, window);
    if (key_origin < 0) BF_FAIL("%s: key_origin=%d must be at least 0", what, key_origin);
    if (check_shape(what, shape, dtype, kv8)) return 1;
    if (!d_q || !d_k || !d_v || !d_out) BF_FAIL("%s: NULL argument", what);
    if (kv8) {
        if (!d_k_scale || !d_v_scale) BF_FAIL("%s: NULL scale", what);
        if (((uintptr_t)d_k_scale | (uintptr_t)d_v_scale) & 3) BF_FAIL("%s: the scales must be 4-byte aligned", what);
    }
    if (((uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out) & 15) BF_FAIL("%s: pointers must be 16-byte aligned", what);
    if (d_mask && ((uintptr_t)d_mask & 3)) BF_FAIL("%s: mask must be 4-byte aligned", what);
    if (d_kv_len && ((uintptr_t)d_kv_len & 7)) BF_FAIL("%s: kv_len must be an 8-byte aligned device int64", what);
    ChunkKv8Params p = {};
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.mask = d_mask;
    p.mask_off = d_mask_off;
    p.kv_len = d_kv_len;
    p.out = d_out;
    p.N = shape->N;
    p.Tq = shape->Tq;
    p.Tk = shape->Tk;
    p.H = shape->H;
    p.Hkv = shape->Hkv;
    p.group = shape->H / shape->Hkv;
    p.window = window < shape->Tk ? window : shape->Tk;  // (a wider window hides nothing)
    p.origin = key_origin;
    for (int i = 0; i < 3; ++i) {
        p.qs[i] = shape->q_stride[i];
        p.ks[i] = shape->k_stride[i];
        p.vs[i] = shape->v_stride[i];
    }
    p.scale_log2e = scaling * LOG2E;
    if (softcap != 0.f && p.fill(what, softcap, scaling)) return 1;
    p.k_scale = d_k_scale;
    p.v_scale = d_v_scale;
    launch(p, dtype, shape->head_dim, softcap != 0.f, kv8, stream);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int bf_attention_chunk_gqa(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                           const int64_t* d_kv_len, void* d_out, int dtype, const bf_attn_decode_t* shape, int32_t window,
                           int32_t key_origin, float softcap, float scaling, void* stream) {
    return chunk("bf_attention_chunk_gqa", d_q, d_k, d_v, nullptr, nullptr, d_mask, d_mask_off, d_kv_len, d_out, dtype, shape,
                 window, key_origin, softcap, scaling, (hipStream_t)stream, false);
}

int bf_attention_chunk_gqa_kv8(const void* d_q, const void* d_kq, const void* d_vq, const float* d_k_scale,
                               const float* d_v_scale, const float* d_mask, const uint8_t* d_mask_off,
                               const int64_t* d_kv_len, void* d_out, int dtype, const bf_attn_decode_t* shape,
                               int32_t window, int32_t key_origin, float softcap, float scaling, void* stream) {
    return chunk("bf_attention_chunk_gqa_kv8", d_q, d_kq, d_vq, d_k_scale, d_v_scale, d_mask, d_mask_off, d_kv_len, d_out,
                 dtype, shape, window, key_origin, softcap, scaling, (hipStream_t)stream, true);
}
