// bf_attention_tiles.h — MFMA fragment layouts and LDS images shared by the attention kernels of bf_attention.hip,
// bf_attention_bwd.hip, bf_attention_gqa.hip, bf_attention_chunk.hip and bf_attention_decode.hip (bf16 / fp16 operands,
// mfma_f32_16x16x32, head size 64, 128 or 256).  The contract all of them lean on:
//   * lane (li, lg) = (lane & 15, lane >> 4).  As an operand it holds 8 consecutive features (k group lg) of row / column li.
//     S^T = K Q^T with the keys as rows leaves it 4 consecutive keys, blk*16 + 4 lg + 0..3, of ONE query li per 16-key block:
//     a query's softmax statistics are in-lane values + two cross-lane steps (the dk/dv kernels swap the roles);
//   * two neighbouring blocks are then the 8-element column operand of the next product as they stand (pack2), its k index
//     a fixed permutation of the keys: (2c)*16 + 4 lg + 0..3, then (2c + 1)*16 + 4 lg + 0..3.  tr_frag(c) applies the same
//     order to the other operand, straight out of a row-major image through gfx950's LDS transpose read (ds_read_b64_tr_b16);
//   * the dropout keep-bit layout (AttnParams, bf_attention.hip: bit c*8 + e*4 + j of word lg) is that order written
//     down, and the backward kernels read the bits by it.  Changing the order changes all of these at once.
// The contract is code as well: the causal forward (bf_attention_gqa.hip), the chunk and the decode kernels share one online-
// softmax-and-PV step (softmax_pv_step), one clamped and one FP8 staging write, the cache's fill length, the soft-cap
// parameters and, on the host, the dispatch helpers and the bf_attn_decode_t checks below.  What a key is visible to stays
// in each kernel: they differ there on purpose.
#pragma once
#include "bf_common.h"
#include "bf_fp8.h"

#include <type_traits>

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// tanh for the soft-capped logits (gfx950 has no tanh instruction): 1 - 2 / (1 + e^2x) from the exp2 and rcp units.  e^2x
// overflows to +inf (rcp gives 0: th = 1) and underflows to 0 (th = -1): saturation, never NaN, at both ends.  Near 0 that
// form cancels — its error is an ulp of 1, which is all of a tiny x — so the result is held between x and x - x^3 / 3, which
// bracket tanh(x) for either sign (one median instruction, no branch): the error is the smaller of the two, and a cap far
// above the logits gives the uncapped scores to rounding.  (An overflowing x^3 leaves -inf / +inf as the far bound.)
__device__ __forceinline__ float softcap_tanh(float x) {
    const float e = __builtin_amdgcn_exp2f(x * (2.0f * LOG2E));
    const float th = fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);
    return __builtin_amdgcn_fmed3f(th, x, fmaf(x * x * x, -1.0f / 3.0f, x));
}

typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;

template <typename T>
struct Mfma;
template <>
struct Mfma<__bf16> {
    using frag = bf16x8_t;
    using half4 = bf16x4_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <>
struct Mfma<_Float16> {
    using frag = f16x8_t;
    using half4 = f16x4_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

// Row stride of the LDS images: swizzled (16-byte chunk ^= row & 7, for direct row-operand reads) and padded (+32 B, for
// the transpose reads: the 8 rows a 32-lane half of one touches tile one bank row)
template <int HD>
struct Rows {
    static constexpr int SWZ = HD * 2;
    static constexpr int PAD = HD * 2 + 32;
};

// Key tile and workgroups per CU of the causal forward kernels, per head size: bf_attention_gqa.hip's forward (its Shape gives
// the reasons) and bf_attention_chunk.hip's, whose rows are bitwise that forward's only while both walk the same key tiles.
template <int HD>
struct FwdShape;
template <>
struct FwdShape<64> {
    static constexpr int KT = 128, MINB = 3;
};
template <>
struct FwdShape<128> {
    static constexpr int KT = 128, MINB = 2;
};
template <>
struct FwdShape<256> {
    static constexpr int KT = 64, MINB = 1;
};

// stage rows row0 .. row0 + NR - 1 of a [tokens][stride] tensor into the swizzled and / or the padded image
template <typename T, int HD, int NR, int NT>
__device__ __forceinline__ void stage(const T* base, long long stride, int row0, char* swz, char* pad, int tid) {
    constexpr int CPR = HD / 8;  // 16-byte chunks per row
    static_assert((NR * CPR) % NT == 0, "whole passes");
#pragma unroll
    for (int i = 0; i < NR * CPR / NT; ++i) {
        const int c = tid + NT * i, row = c / CPR, c8 = c % CPR;
        const f32x4_t x = *reinterpret_cast<const f32x4_t*>(base + (long long)(row0 + row) * stride + c8 * 8);
        if (swz) *reinterpret_cast<f32x4_t*>(swz + row * Rows<HD>::SWZ + ((c8 ^ (row & 7)) << 4)) = x;
        if (pad) *reinterpret_cast<f32x4_t*>(pad + row * Rows<HD>::PAD + (c8 << 4)) = x;
    }
}

// ... of a tensor whose rows first .. last exist: a row outside re-reads the nearer of the two (a finite value of the
// caller's, never what lies around the tensor; no branch).  The caller gives such rows no weight and stores nothing for them.
template <typename T, int HD, int NR, int NT>
__device__ __forceinline__ void stage_clamped(const T* base, long long stride, int row0, int first, int last, char* swz,
                                              char* pad, int tid) {
    constexpr int CPR = HD / 8;
    static_assert((NR * CPR) % NT == 0, "whole passes");
#pragma unroll
    for (int i = 0; i < NR * CPR / NT; ++i) {
        const int c = tid + NT * i, row = c / CPR, c8 = c % CPR;
        const f32x4_t x =
            *reinterpret_cast<const f32x4_t*>(base + (long long)max(first, min(row0 + row, last)) * stride + c8 * 8);
        if (swz) *reinterpret_cast<f32x4_t*>(swz + row * Rows<HD>::SWZ + ((c8 ^ (row & 7)) << 4)) = x;
        if (pad) *reinterpret_cast<f32x4_t*>(pad + row * Rows<HD>::PAD + (c8 << 4)) = x;
    }
}

// 16 bytes of an FP8 cache row (include/bayeformers_amd_kv8.h) are the features 16 c16 .. 16 c16 + 15 of image row `row`:
// dequantised with the row's scale (bf_fp8.h: exact in bf16) into two 16-byte chunks of the swizzled and / or padded image
template <int HD>
__device__ __forceinline__ void write_fp8(u32x4_t x, float scale, int row, int c16, char* swz, char* pad) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int d8 = 2 * c16 + h;
        const bf16x8_t w = fp8_rows_value(u32x2_t{x[2 * h], x[2 * h + 1]}, scale);
        if (swz) *reinterpret_cast<bf16x8_t*>(swz + row * Rows<HD>::SWZ + ((d8 ^ (row & 7)) << 4)) = w;
        if (pad) *reinterpret_cast<bf16x8_t*>(pad + row * Rows<HD>::PAD + (d8 << 4)) = w;
    }
}

// row-operand fragment (16 rows x 32 features, half dh) of block `blk` of a swizzled image: lane (row li, k group lg)
template <typename T, int HD>
__device__ __forceinline__ typename Mfma<T>::frag row_frag(const char* swz, int blk, int dh, int li, int lg) {
    const int row = blk * 16 + li;
    return *reinterpret_cast<const typename Mfma<T>::frag*>(swz + row * Rows<HD>::SWZ + (((dh * 4 + lg) ^ (row & 7)) << 4));
}

// transposed fragment of a row-major image with rows of ROW bytes: rows = features db*16 + li, k = the 32 image rows
// {(2c)*16 + 4 lg + 0..3, (2c+1)*16 + 4 lg + 0..3}, by two LDS transpose reads (the 16 lanes of a group point at a
// [4 rows][16 features] block: lane -> row li >> 2, features 4 * (li & 3) .., each gets its column = 4 rows of feature li)
template <typename T, int ROW>
__device__ __forceinline__ typename Mfma<T>::frag tr_frag_row(const char* pad, int c, int db, int li, int lg) {
    const char* blk = pad + (lg * 4 + (li >> 2)) * ROW + (db * 16 + (li & 3) * 4) * 2;
    const s16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(blk + (2 * c) * 16 * ROW));
    const s16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(blk + (2 * c + 1) * 16 * ROW));
    const s16x8_t ab = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(typename Mfma<T>::frag, ab);
}

// ... of a padded image of head size HD
template <typename T, int HD>
__device__ __forceinline__ typename Mfma<T>::frag tr_frag(const char* pad, int c, int db, int li, int lg) {
    return tr_frag_row<T, Rows<HD>::PAD>(pad, c, db, li, lg);
}

template <typename T>
__device__ __forceinline__ typename Mfma<T>::frag pack2(const f32x4_t a, const f32x4_t b) {
    const f32x8_t v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_convertvector(v, typename Mfma<T>::frag);
}

// One online-softmax step of the causal forward, the chunk and the decode kernels, and its P V product: s holds the scores
// of KT keys for the lane's query (log2 units, the mask added, -inf where the kernel's own visibility rule hides a key), mx
// the lane's maximum over them, v_image the padded V image of the tile.  Rescales the query's running max, sum and output block
// o and adds the tile's; s is left holding the probabilities.  The operation order is the kernels' result, bit for bit.
// The code is the kernels' own as well (profiles/attention_tile_step.md) as long as the compiler sees what it saw there:
// the image as an LDS pointer (it folds the blocks' offsets into the transpose reads' immediates for that address space
// alone) and a query's two statistics as one object (two float arrays by reference come out as vector phis).
struct SoftmaxRow {
    float max = -INFINITY, sum = 0.f;  // log2 units; no key seen yet
};
typedef const __attribute__((address_space(3))) char* lds_image;
template <typename T, int HD, int KT>
__device__ __forceinline__ void softmax_pv_step(f32x4_t (&s)[KT / 16], float mx, SoftmaxRow& run, f32x4_t (&o)[HD / 16],
                                                lds_image v_image, int li, int lg) {
    const char* vs = (const char*)v_image;
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float new_max = fmaxf(run.max, mx);
    const float ref = new_max == -INFINITY ? 0.f : new_max;  // nothing visible yet: every term is 0
    const float corr = __builtin_amdgcn_exp2f(run.max - ref);
    float sum = 0.f;
#pragma unroll
    for (int kbk = 0; kbk < KT / 16; ++kbk)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[kbk][j] = __builtin_amdgcn_exp2f(s[kbk][j] - ref);
            sum += s[kbk][j];
        }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    run.sum = run.sum * corr + sum;
    run.max = new_max;
#pragma unroll
    for (int db = 0; db < HD / 16; ++db) o[db] *= corr;
#pragma unroll
    for (int c = 0; c < KT / 32; ++c) {
        const typename Mfma<T>::frag pf = pack2<T>(s[2 * c], s[2 * c + 1]);
#pragma unroll
        for (int db = 0; db < HD / 16; ++db) o[db] = Mfma<T>::run(tr_frag<T, HD>(vs, c, db, li, lg), pf, o[db]);
    }
}

// the filled keys of a cache of Tk rows: *kv_len clamped to [0, Tk] (a fixed-capacity cache), or Tk without a kv_len
__device__ __forceinline__ int filled_keys(const int64_t* kv_len, int Tk) {
    if (!kv_len) return Tk;
    const int64_t len = *kv_len;
    return len < 0 ? 0 : (len > Tk ? Tk : (int)len);
}

// The soft-cap (CAP) instantiations' two parameters: the score is softcap * tanh(scale q.k / softcap), in log2 units
// softcap_tanh(s * cap_x) * cap_log2e.  A base of the CAP parameter blocks of every attention file.
struct SoftCap {
    float cap_x, cap_log2e;  // scale / softcap and softcap * log2(e)
    // softcap: finite and > 0 (the entries checked it); returns 0 or the BF_FAIL status
    int fill(const char* what, float softcap, float scaling) {
        cap_x = scaling / softcap;
        cap_log2e = softcap * LOG2E;
        if (!(cap_log2e < INFINITY) || !(fabsf(cap_x) < INFINITY))
            BF_FAIL("%s: softcap=%g: scaling / softcap or softcap * log2(e) is not finite", what, (double)softcap);
        return 0;
    }
};

// Host dispatch, one helper per axis: each hands the run-time value to a generic lambda as a compile-time one
// (decltype(tag)::type, decltype(hd)::value, decltype(flag)::value), so a file's launch nests them instead of spelling
// an if-ladder per combination.
template <typename T>
struct TypeTag {
    using type = T;
};
template <typename F>
void with_dtype(int dtype, F&& f) {  // BF_DT_BF16 or BF_DT_F16 (the shape checks saw to it)
    if (dtype == BF_DT_BF16) f(TypeTag<__bf16>{});
    else f(TypeTag<_Float16>{});
}
template <typename F>
void with_head_size(int D, F&& f) {  // 64, 128 or 256
    if (D == 64) f(std::integral_constant<int, 64>{});
    else if (D == 128) f(std::integral_constant<int, 128>{});
    else f(std::integral_constant<int, 256>{});
}
template <typename F>
void with_flag(bool on, F&& f) {
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

// The checks of a bf_attn_decode_t that the decode and the chunk entries share, before and after their own grid limits:
// tq_max 0 = any Tq >= 1 (the chunk kernel, whose key index then needs a tile of headroom); kv_unit = what the K / V
// strides are multiples of, 8 (elements) or 16 (the bytes of an FP8 cache, which only bf16 reads).  0 or the BF_FAIL status.
int check_decode_dims(const char* what, const bf_attn_decode_t* s, int dtype, int tq_max, int kv_unit) {
    if (!s) BF_FAIL("%s: shape is NULL", what);
    if (kv_unit == 16 && dtype != BF_DT_BF16)
        BF_FAIL("%s: dtype must be bf16 (bfloat16: the dequantised rows are exact in it alone)", what);
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) BF_FAIL("%s: dtype must be bf16 or fp16", what);
    if (s->head_dim != 64 && s->head_dim != 128 && s->head_dim != 256)
        BF_FAIL("%s: head size %d (64, 128 or 256)", what, s->head_dim);
    if (tq_max && (s->Tq < 1 || s->Tq > tq_max)) BF_FAIL("%s: Tq=%d new queries (1 .. %d)", what, s->Tq, tq_max);
    if (s->Tq < 1) BF_FAIL("%s: Tq=%d new queries (at least 1)", what, s->Tq);
    if (s->Tk < s->Tq) BF_FAIL("%s: Tk=%d cached keys, fewer than Tq=%d", what, s->Tk, s->Tq);
    if (!tq_max && s->Tk > 0x7fffff00) BF_FAIL("%s: Tk=%d cached keys exceeds the key index", what, s->Tk);
    if (s->N < 1 || s->H < 1 || s->Hkv < 1) BF_FAIL("%s: N=%d, H=%d, Hkv=%d must be positive", what, s->N, s->H, s->Hkv);
    if (s->H % s->Hkv) BF_FAIL("%s: %d query heads do not divide into %d K/V head groups", what, s->H, s->Hkv);
    return 0;
}
int check_decode_strides(const char* what, const bf_attn_decode_t* s, int kv_unit) {
    for (int i = 0; i < 3; ++i) {
        if (s->q_stride[i] < 0 || s->q_stride[i] % 8) BF_FAIL("%s: strides must be non-negative multiples of 8 elements", what);
        const int64_t st[2] = {s->k_stride[i], s->v_stride[i]};
        for (int t = 0; t < 2; ++t) {
            if (kv_unit == 16 && (st[t] < 0 || st[t] % 16))
                BF_FAIL("%s: the K / V strides (bytes) must be non-negative multiples of 16", what);
            if (st[t] < 0 || st[t] % 8) BF_FAIL("%s: strides must be non-negative multiples of 8 elements", what);
        }
    }
    return 0;
}

}  // namespace
