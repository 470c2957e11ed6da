// bf_attention_decode.hip — causal grouped-query attention of a decode step against a KV cache (inference only): Tq new
// queries per sequence (1 <= Tq <= 16) against Tk cached keys (Tq <= Tk, any Tk >= 1), for the decoder-only transformers
// the reference converts (/root/reference/bayeformers/convert.py) when they generate with `past_key_values`.
//
//   out[n,i,h,:] = sum_{j <= Tk - Tq + i, key j visible in n} softmax_j(scale q[n,h,i] . k[n,g,j] + mask[n,j]) v[n,g,j,:],
//   g = h / (H / Hkv).
//
// Decode is bound by the read of the cache, so one workgroup reads a K/V head ONCE for the whole head group: the
// G = H / Hkv query heads x Tq queries of one (sequence, kv head) are the rows of the MFMA tiles (row r = head-in-group *
// Tq + query), 16 per wave, 64 per 256-thread workgroup (more rows: the grid's z dimension, each chunk reading the head
// again).  The keys are split so that the grid fills the chip: the split count and boundaries are a function of the
// shape only (decode_split), and with more than one split a second launch merges the partial (max, sum, output) rows in
// split order — bitwise the same result on every run, no atomics, no host synchronisation, no allocation (the partials
// live in the caller's workspace: bf_attention_decode_workspace_bytes).
// It shares the fragment layouts, LDS images and the online-softmax step with bf_attention_gqa.hip's forward
// (bf_attention_tiles.h: softmax_pv_step, one 64-key block per wave and tile): S^T = K Q^T, then O^T = V^T P^T with P^T
// straight from the accumulators.  The next key tile is fetched into registers while the current
// one is computed.  A query with no visible key returns 0.
//
// bf_attention_decode_gqa_len runs the same kernels over a fixed-capacity cache (a static cache that one captured graph
// serves at every step): Tk is the capacity, the filled length L comes from a device scalar.  The grid and the workspace
// follow the capacity; the split boundaries follow the keys-per-split rule applied to L, computed in the kernel (splits
// past L write an empty partial the merge skips), so at L == Tk the launch is bitwise bf_attention_decode_gqa's.
//
// bf_attention_decode_gqa_kv8 (include/bayeformers_amd_kv8.h) runs them over an FP8 cache: K and V rows of D e4m3fn bytes
// with one fp32 power-of-two scale each (bf_kv8.hip writes them).  Only the fetch differs: a key row is HD / 16 16-byte
// chunks plus its scale, and the dequantised bf16 values — exact — are written into the same LDS images (write_fp8, shared
// with bf_attention_chunk.hip), so everything behind the fetch is the bf16 kernel's and the result is bitwise that kernel's on the dequantised cache.
//
// bf_attention_decode_gqa_ring / _ring_kv8 (include/bayeformers_amd_ring.h) run the window form over a ring buffer: the
// cache holds C = ring_slots rows and the key with sequence index j lives in row j % C.  The tile grid, the splits, the mask
// and the visibility test stay over sequence indices (Tk is the logical capacity); again only the fetch differs, which
// reads row key % C — the slot of a tile's first key once per tile, then a conditional subtract per row (the keys a launch
// reads span at most window + Tq - 1 <= C indices, so one subtract wraps them).  A compile-time form (RING) instantiated
// with LOCAL alone: the result is bitwise the window entry's on the same keys laid out in sequence order.
#include "bf_attention_tiles.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int KT = 64;             // keys per tile
constexpr int ROWS = 64;           // query rows per workgroup: 4 waves x 16
constexpr int MIN_SPLIT_KEYS = 128;  // a split walks at least two key tiles
constexpr long long TARGET_WGS = 1024;  // 256 CUs x 4 resident workgroups

struct DecodeParams {
    const void* q;
    const void* k;
    const void* v;
    const float* mask;              // [N][Tk] additive over the keys, nullable
    const unsigned char* mask_off;  // nullable device flag: non-zero = skip the mask
    void* out;                      // [N][Tq][H][D]
    float* part_o;                  // [nsplit][N * Hkv][R][D] unnormalised partial outputs (nsplit > 1)
    float* part_ml;                 // [nsplit][N * Hkv][R][2] their running max (log2 units) and sum
    long long qs[3], ks[3], vs[3];  // (batch, head, token) element strides
    const int64_t* kv_len;          // nullable device scalar: the filled keys L (Tk is then the capacity)
    int N, Tq, Tk, H, Hkv, group, R, nsplit, split_keys;
    int window;                     // LOCAL: query i (index L - Tq + i) sees keys L - Tq + i - window + 1 .. L - Tq + i
    long long want;                 // the split count the grid asks for (decode_split), the kernel's rule for L
    float scale_log2e;
};

// CAP: the soft-capped logits of bf_attention_gqa.hip's CAP forward (softcap * tanh(scale q.k / softcap), then the mask): a
// compile-time flag with a parameter block of its own (SoftCap: bf_attention_tiles.h)
struct DecodeCapParams : DecodeParams, SoftCap {};
// KV8: k and v are e4m3fn rows (ks / vs in bytes), with one scale per (sequence, K/V head, key); again a compile-time flag
// with a parameter block of its own
struct DecodeKv8Params : DecodeCapParams {
    const float* k_scale;  // [N][Hkv][Tk]
    const float* v_scale;
};
// RING: k, v and the kv8 scales hold `ring` rows, key j in row j % ring; a compile-time flag with a parameter block of its
// own once more (one block for every RING instantiation)
struct DecodeRingParams : DecodeKv8Params {
    int ring;
};
template <bool CAP, bool KV8, bool RING = false>
using ParamsOf = std::conditional_t<RING, DecodeRingParams,
                                    std::conditional_t<KV8, DecodeKv8Params, std::conditional_t<CAP, DecodeCapParams, DecodeParams>>>;

struct Split {
    int n, keys;  // splits, keys per split (a multiple of KT; the last split ends at Tk)
};

long long split_want(const bf_attn_decode_t* s) {
    const int R = s->H / s->Hkv * s->Tq;
    const long long base = (long long)s->N * s->Hkv * ((R + ROWS - 1) / ROWS);
    return std::max(1LL, (TARGET_WGS + base - 1) / base);
}

// key tiles per split for `keys` keys when the grid asks for `want` splits (at least two tiles a split)
__host__ __device__ inline int split_tiles(int keys, long long want) {
    const int tiles = (keys + KT - 1) / KT;
    const int most = (keys + MIN_SPLIT_KEYS - 1) / MIN_SPLIT_KEYS;
    const int n0 = (int)(want < most ? want : (most > 1 ? most : 1));
    return (tiles + n0 - 1) / n0;
}

Split decode_split(const bf_attn_decode_t* s) {
    const int tiles = (s->Tk + KT - 1) / KT;
    const int per = split_tiles(s->Tk, split_want(s));
    return Split{(tiles + per - 1) / per, per * KT};
}

template <typename T, int HD, bool LOCAL, bool CAP, bool KV8 = false, bool RING = false>
__global__ __launch_bounds__(256) void decode_kernel(const ParamsOf<CAP, KV8, RING> p) {
    static_assert(LOCAL || !RING, "a ring cache is read through a window");
    using frag = typename Mfma<T>::frag;
    using half4 = typename Mfma<T>::half4;
    using KV = std::conditional_t<KV8, uint8_t, T>;          // what the cache holds
    using chunk = std::conditional_t<KV8, u32x4_t, f32x4_t>;  // 16 bytes of it in flight
    constexpr int NDH = HD / 32, NDB = HD / 16, NKB = KT / 16;
    constexpr int CPR = HD * (int)sizeof(KV) / 16, NLD = KT * CPR / 256;  // 16-byte chunks per key row; per thread and tile
    constexpr int K_BYTES = KT * Rows<HD>::SWZ, V_BYTES = KT * Rows<HD>::PAD;
    __shared__ __attribute__((aligned(16))) char smem[K_BYTES + V_BYTES + KT * 4];
    char* const ks = smem;
    char* const vs = smem + K_BYTES;
    float* const ms = reinterpret_cast<float*>(smem + K_BYTES + V_BYTES);  // this tile's key mask, log2 units
    const float* const mask = (p.mask && !(p.mask_off && *p.mask_off)) ? p.mask : nullptr;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int split = blockIdx.x, nk = blockIdx.y, n = nk / p.Hkv, g = nk % p.Hkv;
    const int L = filled_keys(p.kv_len, p.Tk);
    int split_keys = p.split_keys;
    // LOCAL: the keys some query sees start at lo (the first query's window); the splits are laid over [lo, L)
    const int lo = LOCAL ? max(0, L - p.Tq - p.window + 1) : 0;
    if (p.kv_len) {  // the range's own split rule, within the grid's nsplit splits
        const int tiles = (L - lo + KT - 1) / KT;
        split_keys = max(max(split_tiles(L - lo, p.want), (tiles + p.nsplit - 1) / p.nsplit), 1) * KT;
    }
    const int k_lo = lo + split * split_keys, k_hi = min(L, k_lo + split_keys);
    const int r = blockIdx.z * ROWS + wid * 16 + li;  // this lane's query row (its column of S^T and O^T)
    const bool wave_live = (int)blockIdx.z * ROWS + wid * 16 < p.R, row_ok = r < p.R;
    const int qi = row_ok ? r % p.Tq : 0, h = g * p.group + (row_ok ? r / p.Tq : 0);
    const int lim = L - p.Tq + qi;  // the last key query qi sees
    const KV* kb = reinterpret_cast<const KV*>(p.k) + n * p.ks[0] + g * p.ks[1];
    const KV* vb = reinterpret_cast<const KV*>(p.v) + n * p.vs[0] + g * p.vs[1];

    frag qf[NDH];
    const T* qrow = reinterpret_cast<const T*>(p.q) + n * p.qs[0] + h * p.qs[1] + qi * p.qs[2];
#pragma unroll
    for (int dh = 0; dh < NDH; ++dh) {
        qf[dh] = frag{};
        if (row_ok) qf[dh] = *reinterpret_cast<const frag*>(qrow + dh * 32 + lg * 8);
    }

    f32x4_t o[NDB];
#pragma unroll
    for (int j = 0; j < NDB; ++j) o[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    SoftmaxRow run;

    // the next tile travels in registers while the current one is computed; keys past the split read as 0
    // (KV8: with the rows' scales; a key past the split has scale 0 too)
    chunk kr[NLD], vr[NLD];
    float ksc[KV8 ? NLD : 1], vsc[KV8 ? NLD : 1];
    float mr = 0.f;
    auto fetch = [&](int key0) {
        // RING: the tile's keys are consecutive sequence indices, so its rows are consecutive slots from key0 % ring on; a
        // key this launch reads lies fewer than ring indices past key0 (k_hi - k_lo <= window + Tq - 1 <= ring)
        int slot0 = 0;
        if constexpr (RING) slot0 = key0 % p.ring;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int c = tid + 256 * i, key = key0 + c / CPR, c8 = c % CPR;
            kr[i] = vr[i] = chunk{};
            if constexpr (KV8) ksc[i] = vsc[i] = 0.f;
            if (key < k_hi) {
                int row = key, rows = p.Tk;  // the cache row of the key, of the rows the cache holds
                if constexpr (RING) {
                    row = slot0 + c / CPR;
                    rows = p.ring;
                    if (row >= rows) row -= rows;
                }
                kr[i] = *reinterpret_cast<const chunk*>(kb + (long long)row * p.ks[2] + c8 * (16 / (int)sizeof(KV)));
                vr[i] = *reinterpret_cast<const chunk*>(vb + (long long)row * p.vs[2] + c8 * (16 / (int)sizeof(KV)));
                if constexpr (KV8) {
                    const long long srow = ((long long)n * p.Hkv + g) * rows + row;
                    ksc[i] = p.k_scale[srow];
                    vsc[i] = p.v_scale[srow];
                }
            }
        }
        if (mask && tid < KT && key0 + tid < k_hi) mr = mask[(long long)n * p.Tk + key0 + tid] * LOG2E;
    };
    fetch(k_lo);
    for (int key0 = k_lo; key0 < k_hi; key0 += KT) {
        if (key0 != k_lo) __syncthreads();  // every wave is done with the previous tile
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int c = tid + 256 * i, row = c / CPR, c8 = c % CPR;
            if constexpr (KV8) {  // 16 bytes are 16 features: two 16-byte chunks of the bf16 images
                write_fp8<HD>(kr[i], ksc[i], row, c8, ks, nullptr);
                write_fp8<HD>(vr[i], vsc[i], row, c8, nullptr, vs);
            } else {
                *reinterpret_cast<f32x4_t*>(ks + row * Rows<HD>::SWZ + ((c8 ^ (row & 7)) << 4)) = kr[i];
                *reinterpret_cast<f32x4_t*>(vs + row * Rows<HD>::PAD + (c8 << 4)) = vr[i];
            }
        }
        if (mask && tid < KT) ms[tid] = mr;
        __syncthreads();
        if (key0 + KT < k_hi) fetch(key0 + KT);
        if (!wave_live) continue;

        f32x4_t s[NKB];
#pragma unroll
        for (int kbk = 0; kbk < NKB; ++kbk) {
            s[kbk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dh = 0; dh < NDH; ++dh) s[kbk] = Mfma<T>::run(row_frag<T, HD>(ks, kbk, dh, li, lg), qf[dh], s[kbk]);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kbk = 0; kbk < NKB; ++kbk) {
            f32x4_t mk = {0.f, 0.f, 0.f, 0.f};
            if (mask) mk = *reinterpret_cast<const f32x4_t*>(ms + kbk * 16 + lg * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int key = key0 + kbk * 16 + lg * 4 + j;
                const bool seen = key < k_hi && key <= lim && (!LOCAL || key > lim - p.window);
                if constexpr (CAP) s[kbk][j] = seen ? fmaf(softcap_tanh(s[kbk][j] * p.cap_x), p.cap_log2e, mk[j]) : -INFINITY;
                else s[kbk][j] = seen ? fmaf(s[kbk][j], p.scale_log2e, mk[j]) : -INFINITY;
                mx = fmaxf(mx, s[kbk][j]);
            }
        }
        softmax_pv_step<T, HD, KT>(s, mx, run, o, (lds_image)vs, li, lg);
    }
    if (!row_ok) return;

    if (p.nsplit == 1) {  // one split: the final rows
        const float inv = run.sum > 0.f ? 1.0f / run.sum : 0.f;
        T* orow = reinterpret_cast<T*>(p.out) + (((long long)n * p.Tq + qi) * p.H + h) * HD;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
            *reinterpret_cast<half4*>(orow + db * 16 + lg * 4) = __builtin_convertvector(o[db] * inv, half4);
        return;
    }
    const long long prow = ((long long)split * p.N * p.Hkv + nk) * p.R + r;
#pragma unroll
    for (int db = 0; db < NDB; ++db) *reinterpret_cast<f32x4_t*>(p.part_o + prow * HD + db * 16 + lg * 4) = o[db];
    if (lg == 0) {
        p.part_ml[2 * prow] = run.max;
        p.part_ml[2 * prow + 1] = run.sum;
    }
}

// one thread per 4 features of an output row [n][i][h]: the splits' partial rows merged in split order
template <typename T, int HD>
__global__ __launch_bounds__(256) void decode_merge_kernel(const DecodeParams p) {
    using half4 = typename Mfma<T>::half4;
    constexpr int TPR = HD / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, row = t / TPR;
    const int c4 = (int)(t % TPR);
    if (row >= (long long)p.N * p.Tq * p.H) return;
    const int h = (int)(row % p.H), qi = (int)(row / p.H % p.Tq), n = (int)(row / ((long long)p.H * p.Tq));
    const int r = (h % p.group) * p.Tq + qi, nk = n * p.Hkv + h / p.group;
    const long long stride = (long long)p.N * p.Hkv * p.R;  // partial rows per split
    const long long r0 = (long long)nk * p.R + r;
    float m = -INFINITY;
    for (int s = 0; s < p.nsplit; ++s) m = fmaxf(m, p.part_ml[2 * (s * stride + r0)]);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    if (m != -INFINITY) {
        for (int s = 0; s < p.nsplit; ++s) {
            const long long pr = s * stride + r0;
            const float ms = p.part_ml[2 * pr];
            if (ms == -INFINITY) continue;  // nothing visible in this split
            const float w = __builtin_amdgcn_exp2f(ms - m);
            l = fmaf(w, p.part_ml[2 * pr + 1], l);
            acc += w * *reinterpret_cast<const f32x4_t*>(p.part_o + pr * HD + c4 * 4);
        }
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    *reinterpret_cast<half4*>(reinterpret_cast<T*>(p.out) + row * HD + c4 * 4) = __builtin_convertvector(acc * inv, half4);
}

// kv8: the FP8 instantiations (bf16 compute); each dtype and head size with and without a window and a cap
// ring (p.ring != 0): the RING instantiations, which exist beside the LOCAL ones alone (the entries require a window)
void launch(const DecodeRingParams& p, int dtype, int D, bool cap, bool kv8, hipStream_t stream) {
    const dim3 grid(p.nsplit, p.N * p.Hkv, (p.R + ROWS - 1) / ROWS);
    with_head_size(D, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        with_flag(p.window != 0, [&](auto local) {
            with_flag(cap, [&](auto capped) {
                auto run = [&](auto tag, auto fp8) {
                    using T = typename decltype(tag)::type;
                    constexpr bool LOCAL = decltype(local)::value, CAP = decltype(capped)::value, KV8 = decltype(fp8)::value;
                    if constexpr (LOCAL) {
                        if (p.ring) {
                            decode_kernel<T, HD, true, CAP, KV8, true><<<grid, 256, 0, stream>>>(p);
                            return;
                        }
                    }
                    const ParamsOf<CAP, KV8>& kp = p;
                    decode_kernel<T, HD, LOCAL, CAP, KV8><<<grid, 256, 0, stream>>>(kp);
                };
                if (kv8) run(TypeTag<__bf16>{}, std::true_type{});
                else with_dtype(dtype, [&](auto tag) { run(tag, std::false_type{}); });
            });
        });
        if (p.nsplit > 1) {
            const long long threads = (long long)p.N * p.Tq * p.H * (HD / 4);
            with_dtype(dtype, [&](auto tag) {
                decode_merge_kernel<typename decltype(tag)::type, HD><<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(p);
            });
        }
    });
}

// Validates the shape; returns 0 or the BF_FAIL status
int check_shape(const char* what, const bf_attn_decode_t* s, int dtype) {
    if (check_decode_dims(what, s, dtype, 16, 8)) return 1;
    const long long rows = (long long)(s->H / s->Hkv) * s->Tq;
    if ((long long)s->N * s->Hkv > 65535 || (rows + ROWS - 1) / ROWS > 65535) BF_FAIL("%s: N * Hkv or H / Hkv * Tq exceeds the grid", what);
    return check_decode_strides(what, s, 8);
}

int64_t workspace_bytes(const bf_attn_decode_t* s) {
    const Split sp = decode_split(s);
    if (sp.n == 1) return 0;
    const long long rows = (long long)sp.n * s->N * s->Hkv * (s->H / s->Hkv) * s->Tq;
    return rows * (s->head_dim + 2) * (int64_t)sizeof(float);
}

}  // namespace

int64_t bf_attention_decode_workspace_bytes(const bf_attn_decode_t* shape) {
    if (check_shape("bf_attention_decode_workspace_bytes", shape, BF_DT_BF16)) return -1;
    return workspace_bytes(shape);
}

namespace {

// window 0: the plain entries; >= 1: the sliding-window ones.  softcap 0: no cap.  kv8: d_k / d_v are e4m3fn rows with the
// scales d_k_scale / d_v_scale (bf16 compute).  ring 0: k / v hold Tk rows in sequence order; >= 1: that many rows, key j
// in row j % ring (the ring entries checked the window against it)
int decode(const char* what, const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
           const unsigned char* d_mask_off, const int64_t* d_kv_len, void* d_out, void* d_workspace, int dtype,
           const bf_attn_decode_t* shape, int window, float softcap, float scaling, hipStream_t stream, bool kv8 = false,
           const float* d_k_scale = nullptr, const float* d_v_scale = nullptr, int ring = 0) {
    if (window < 0) BF_FAIL("%s: window=%d must be at least 1", what, window);
    if (kv8 && dtype != BF_DT_BF16)
        BF_FAIL("%s: dtype must be bf16 (bfloat16: the dequantised rows are exact in it alone)", what);
    if (check_shape(what, shape, dtype)) return 1;
    if (!d_q || !d_k || !d_v || !d_out) BF_FAIL("%s: NULL argument", what);
    if (kv8) {
        if (!d_k_scale || !d_v_scale) BF_FAIL("%s: NULL scale", what);
        if (((uintptr_t)d_k_scale | (uintptr_t)d_v_scale) & 3) BF_FAIL("%s: the scales must be 4-byte aligned", what);
        for (int i = 0; i < 3; ++i)
            if (shape->k_stride[i] % 16 || shape->v_stride[i] % 16)
                BF_FAIL("%s: the K / V strides (bytes) must be multiples of 16", what);
    }
    if (((uintptr_t)d_q | (uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_out | (uintptr_t)d_workspace) & 15)
        BF_FAIL("%s: pointers must be 16-byte aligned", what);
    if (d_mask && ((uintptr_t)d_mask & 3)) BF_FAIL("%s: mask must be 4-byte aligned", what);
    const Split sp = decode_split(shape);
    if (sp.n > 1 && !d_workspace) BF_FAIL("%s: %d key splits need a workspace of %lld bytes", what, sp.n,
                                          (long long)workspace_bytes(shape));
    DecodeRingParams p = {};
    p.ring = ring;
    p.q = d_q;
    p.k = d_k;
    p.v = d_v;
    p.mask = d_mask;
    p.mask_off = d_mask_off;
    p.out = d_out;
    p.N = shape->N;
    p.Tq = shape->Tq;
    p.Tk = shape->Tk;
    p.H = shape->H;
    p.Hkv = shape->Hkv;
    p.group = shape->H / shape->Hkv;
    p.R = p.group * shape->Tq;
    p.nsplit = sp.n;
    p.split_keys = sp.keys;
    p.kv_len = d_kv_len;
    p.want = split_want(shape);
    p.window = window < shape->Tk ? window : shape->Tk;  // (a wider window hides nothing)
    if (window && !d_kv_len) {
        // the keys [lo, Tk) some query sees, split by the shape's rule within the workspace's sp.n splits (the kernel's
        // rule for a fixed-capacity cache at L = Tk); at lo == 0 these are the plain entry's splits
        const int lo = std::max(0, shape->Tk - shape->Tq - p.window + 1), keys = shape->Tk - lo;
        const int tiles = (keys + KT - 1) / KT;
        const int per = std::max(std::max(split_tiles(keys, p.want), (tiles + sp.n - 1) / sp.n), 1);
        p.nsplit = (tiles + per - 1) / per;
        p.split_keys = per * KT;
    }
    if (sp.n > 1) {
        p.part_o = reinterpret_cast<float*>(d_workspace);
        p.part_ml = p.part_o + (long long)sp.n * p.N * p.Hkv * p.R * shape->head_dim;
    }
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

int bf_attention_decode_gqa(const void* d_q, const void* d_k, const void* d_v, const float* d_mask, const uint8_t* d_mask_off,
                            void* d_out, void* d_workspace, int dtype, const bf_attn_decode_t* shape, float scaling,
                            void* stream) {
    return decode("bf_attention_decode_gqa", d_q, d_k, d_v, d_mask, d_mask_off, nullptr, d_out, d_workspace, dtype, shape, 0,
                  0.f, scaling, (hipStream_t)stream);
}

int bf_attention_decode_gqa_window(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                   const uint8_t* d_mask_off, void* d_out, void* d_workspace, int dtype,
                                   const bf_attn_decode_t* shape, int32_t window, float scaling, void* stream) {
    const char* what = "bf_attention_decode_gqa_window";
    if (window < 1) BF_FAIL("%s: window=%d must be at least 1", what, window);
    return decode(what, d_q, d_k, d_v, d_mask, d_mask_off, nullptr, d_out, d_workspace, dtype, shape, window, 0.f, scaling,
                  (hipStream_t)stream);
}

int bf_attention_decode_gqa_len(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                const uint8_t* d_mask_off, const int64_t* d_kv_len, void* d_out, void* d_workspace,
                                int dtype, const bf_attn_decode_t* shape, float scaling, void* stream) {
    const char* what = "bf_attention_decode_gqa_len";
    if (!d_kv_len || ((uintptr_t)d_kv_len & 7)) BF_FAIL("%s: kv_len must be an 8-byte aligned device int64", what);
    return decode(what, d_q, d_k, d_v, d_mask, d_mask_off, d_kv_len, d_out, d_workspace, dtype, shape, 0, 0.f, scaling,
                  (hipStream_t)stream);
}

int bf_attention_decode_gqa_len_window(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                       const uint8_t* d_mask_off, const int64_t* d_kv_len, void* d_out, void* d_workspace,
                                       int dtype, const bf_attn_decode_t* shape, int32_t window, float scaling,
                                       void* stream) {
    const char* what = "bf_attention_decode_gqa_len_window";
    if (window < 1) BF_FAIL("%s: window=%d must be at least 1", what, window);
    if (!d_kv_len || ((uintptr_t)d_kv_len & 7)) BF_FAIL("%s: kv_len must be an 8-byte aligned device int64", what);
    return decode(what, d_q, d_k, d_v, d_mask, d_mask_off, d_kv_len, d_out, d_workspace, dtype, shape, window, 0.f, scaling,
                  (hipStream_t)stream);
}

int bf_attention_decode_gqa_softcap(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                    const uint8_t* d_mask_off, const int64_t* d_kv_len, void* d_out, void* d_workspace,
                                    int dtype, const bf_attn_decode_t* shape, int32_t window, float softcap, float scaling,
                                    void* stream) {
    const char* what = "bf_attention_decode_gqa_softcap";
    if (!(softcap > 0.f) || !(softcap < INFINITY)) BF_FAIL("%s: softcap=%g must be finite and positive", what, (double)softcap);
    if (window < 0) BF_FAIL("%s: window=%d must be at least 0 (0: no window)", what, window);
    if (d_kv_len && ((uintptr_t)d_kv_len & 7)) BF_FAIL("%s: kv_len must be an 8-byte aligned device int64", what);
    return decode(what, d_q, d_k, d_v, d_mask, d_mask_off, d_kv_len, d_out, d_workspace, dtype, shape, window, softcap, scaling,
                  (hipStream_t)stream);
}

int bf_attention_decode_gqa_kv8(const void* d_q, const void* d_kq, const void* d_vq, const float* d_k_scale,
                                const float* d_v_scale, const float* d_mask, const uint8_t* d_mask_off,
                                const int64_t* d_kv_len, void* d_out, void* d_workspace, int dtype,
                                const bf_attn_decode_t* shape, int32_t window, float softcap, float scaling, void* stream) {
    const char* what = "bf_attention_decode_gqa_kv8";
    if (!(softcap >= 0.f) || !(softcap < INFINITY)) BF_FAIL("%s: softcap=%g must be finite and at least 0 (0: no cap)", what, (double)softcap);
    if (window < 0) BF_FAIL("%s: window=%d must be at least 0 (0: no window)", what, window);
    if (d_kv_len && ((uintptr_t)d_kv_len & 7)) BF_FAIL("%s: kv_len must be an 8-byte aligned device int64", what);
    return decode(what, d_q, d_kq, d_vq, d_mask, d_mask_off, d_kv_len, d_out, d_workspace, dtype, shape, window, softcap,
                  scaling, (hipStream_t)stream, true, d_k_scale, d_v_scale);
}

namespace {

// the checks the two ring entries share; 0 or the BF_FAIL status
int check_ring(const char* what, const int64_t* d_kv_len, const bf_attn_decode_t* shape, int ring_slots, int window,
               float softcap) {
    if (!shape) BF_FAIL("%s: shape is NULL", what);
    if (!(softcap >= 0.f) || !(softcap < INFINITY)) BF_FAIL("%s: softcap=%g must be finite and at least 0 (0: no cap)", what, (double)softcap);
    if (!d_kv_len || ((uintptr_t)d_kv_len & 7)) BF_FAIL("%s: kv_len must be an 8-byte aligned device int64", what);
    if (ring_slots < 1) BF_FAIL("%s: ring_slots=%d must be at least 1", what, ring_slots);
    if (window < 1) BF_FAIL("%s: window=%d must be at least 1", what, window);
    if ((long long)window + shape->Tq - 1 > ring_slots)
        BF_FAIL("%s: window=%d and Tq=%d need %lld ring slots (ring_slots=%d): a step's keys would overwrite each other", what,
                window, shape->Tq, (long long)window + shape->Tq - 1, ring_slots);
    return 0;
}

}  // namespace

int bf_attention_decode_gqa_ring(const void* d_q, const void* d_k, const void* d_v, const float* d_mask,
                                 const uint8_t* d_mask_off, const int64_t* d_kv_len, void* d_out, void* d_workspace, int dtype,
                                 const bf_attn_decode_t* shape, int32_t ring_slots, int32_t window, float softcap,
                                 float scaling, void* stream) {
    const char* what = "bf_attention_decode_gqa_ring";
    if (check_ring(what, d_kv_len, shape, ring_slots, window, softcap)) return 1;
    return decode(what, d_q, d_k, d_v, d_mask, d_mask_off, d_kv_len, d_out, d_workspace, dtype, shape, window, softcap, scaling,
                  (hipStream_t)stream, false, nullptr, nullptr, ring_slots);
}

int bf_attention_decode_gqa_ring_kv8(const void* d_q, const void* d_kq, const void* d_vq, const float* d_k_scale,
                                     const float* d_v_scale, const float* d_mask, const uint8_t* d_mask_off,
                                     const int64_t* d_kv_len, void* d_out, void* d_workspace, int dtype,
                                     const bf_attn_decode_t* shape, int32_t ring_slots, int32_t window, float softcap,
                                     float scaling, void* stream) {
    const char* what = "bf_attention_decode_gqa_ring_kv8";
    if (check_ring(what, d_kv_len, shape, ring_slots, window, softcap)) return 1;
    return decode(what, d_q, d_kq, d_vq, d_mask, d_mask_off, d_kv_len, d_out, d_workspace, dtype, shape, window, softcap,
                  scaling, (hipStream_t)stream, true, d_k_scale, d_v_scale, ring_slots);
}
