// bf_kv_ring.hip — the appends of the ring-buffer KV cache of sample_generate(sliding_cache="ring")
// (include/bayeformers_amd_ring.h): a sliding-window layer keeps C = ring_slots rows per (sequence, K/V head) and the key
// with sequence index j lives in row j % C.
//   * bf_kv_ring_append: the new K and V rows [N][Hkv][T][D] (bf16 or fp16, each tensor with its own strides) of a forward
//     -> rows (pos + i) % C of the two cache buffers, one launch for both;
//   * bf_kv8_ring_append: the same into an FP8 ring, on bf_kv8_append's quantisation (bf_kv8_rows.h), scales included.
// pos is a device int64 (the layer's fill, which counts every appended row and never wraps), so one captured launch serves
// every step.  Of T > C rows (the prompt's hand-over) only the last C are written: no slot is written twice in a launch.
// Every row index is a remainder by C, so nothing outside the buffers is written whatever *pos holds (a negative fill
// writes nothing).  No host synchronisation or allocation: capturable.
// The decode kernel that reads the rows is bf_attention_decode.hip's RING form.
#include "bf_kv8_rows.h"

namespace {

struct RingCopyParams {
    const uint16_t* k;
    const uint16_t* v;
    uint16_t* kc;
    uint16_t* vc;
    const int64_t* pos;
    long long ks[3], vs[3];  // (batch, head, token) element strides of k and v
    int N, Hkv, T, first, ring;  // T rows are written, row i of them being row first + i of k / v
};

// one thread per 16 bytes (8 elements) of a row; CPR = D / 8 of them per row
template <int CPR>
__global__ __launch_bounds__(256) void kv_ring_append_kernel(const RingCopyParams p) {
    constexpr int D = 8 * CPR;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per = (long long)p.N * p.Hkv * p.T;  // rows of K; V's follow
    const long long row = t / CPR;
    const int part = (int)(t % CPR);
    if (row >= 2 * per) return;
    const bool is_v = row >= per;
    const long long r = is_v ? row - per : row;
    const int i = (int)(r % p.T), g = (int)(r / p.T % p.Hkv);
    const long long n = r / ((long long)p.T * p.Hkv);
    const int64_t index = *p.pos + p.first + i;  // the row's sequence index
    if (*p.pos < 0) return;
    const int slot = (int)(index % p.ring);  // in [0, ring): inside the two buffers
    const long long* st = is_v ? p.vs : p.ks;
    const uint16_t* src = (is_v ? p.v : p.k) + n * st[0] + g * st[1] + (long long)(p.first + i) * st[2] + part * 8;
    uint16_t* dst = (is_v ? p.vc : p.kc) + ((n * p.Hkv + g) * p.ring + slot) * D + part * 8;
    *reinterpret_cast<u32x4_t*>(dst) = *reinterpret_cast<const u32x4_t*>(src);
}

// the checks the two entries share; 0 or the BF_FAIL status
int check_append(const char* what, const void* d_k, const void* d_v, const int64_t* k_stride, const int64_t* v_stride,
                 const void* d_kc, const void* d_vc, const int64_t* d_pos, int N, int Hkv, int T, int D, int ring_slots) {
    if (D != 64 && D != 128 && D != 256) BF_FAIL("%s: head size %d (64, 128 or 256)", what, D);
    if (!d_k || !d_v || !d_kc || !d_vc || !k_stride || !v_stride) BF_FAIL("%s: NULL argument", what);
    if (N < 1 || Hkv < 1 || T < 1 || ring_slots < 1)
        BF_FAIL("%s: N=%d, Hkv=%d, T=%d, ring_slots=%d must be positive", what, N, Hkv, T, ring_slots);
    if (((uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_kc | (uintptr_t)d_vc) & 15)
        BF_FAIL("%s: k, v and the cache buffers must be 16-byte aligned", what);
    if (!d_pos || ((uintptr_t)d_pos & 7)) BF_FAIL("%s: pos must be an 8-byte aligned device int64", what);
    for (int i = 0; i < 3; ++i)
        if (k_stride[i] < 0 || k_stride[i] % 8 || v_stride[i] < 0 || v_stride[i] % 8)
            BF_FAIL("%s: strides must be non-negative multiples of 8 elements", what);
    return 0;
}

}  // namespace

int bf_kv_ring_append(const void* d_k, const void* d_v, int dtype, const int64_t* k_stride, const int64_t* v_stride,
                      void* d_kc, void* d_vc, const int64_t* d_pos, int N, int Hkv, int T, int D, int ring_slots,
                      void* stream) {
    const char* what = "bf_kv_ring_append";
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) BF_FAIL("%s: dtype must be bf16 or fp16", what);
    if (check_append(what, d_k, d_v, k_stride, v_stride, d_kc, d_vc, d_pos, N, Hkv, T, D, ring_slots)) return 1;
    RingCopyParams p = {};
    p.k = static_cast<const uint16_t*>(d_k);
    p.v = static_cast<const uint16_t*>(d_v);
    p.kc = static_cast<uint16_t*>(d_kc);
    p.vc = static_cast<uint16_t*>(d_vc);
    p.pos = d_pos;
    for (int i = 0; i < 3; ++i) {
        p.ks[i] = k_stride[i];
        p.vs[i] = v_stride[i];
    }
    p.N = N;
    p.Hkv = Hkv;
    p.T = T < ring_slots ? T : ring_slots;  // the last rows: an earlier one's slot is overwritten within this call
    p.first = T - p.T;
    p.ring = ring_slots;
    const long long threads = 2LL * N * Hkv * p.T * (D / 8);
    const long long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) BF_FAIL("%s: N * Hkv * T = %lld rows exceed the grid", what, (long long)N * Hkv * p.T);
    const dim3 grid((uint32_t)blocks);
    const hipStream_t st = (hipStream_t)stream;
    if (D == 64) hipLaunchKernelGGL(kv_ring_append_kernel<8>, grid, dim3(256), 0, st, p);
    else if (D == 128) hipLaunchKernelGGL(kv_ring_append_kernel<16>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(kv_ring_append_kernel<32>, grid, dim3(256), 0, st, p);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_kv8_ring_append(const void* d_k, const void* d_v, int dtype, const int64_t* k_stride, const int64_t* v_stride,
                       void* d_kq, void* d_vq, float* d_k_scale, float* d_v_scale, const int64_t* d_pos, int N, int Hkv,
                       int T, int D, int ring_slots, void* stream) {
    const char* what = "bf_kv8_ring_append";
    if (dtype != BF_DT_BF16) BF_FAIL("%s: k and v must be bf16 (bfloat16: the dequantised rows are exact in it alone)", what);
    if (check_append(what, d_k, d_v, k_stride, v_stride, d_kq, d_vq, d_pos, N, Hkv, T, D, ring_slots)) return 1;
    if (!d_k_scale || !d_v_scale) BF_FAIL("%s: NULL scale", what);
    if (((uintptr_t)d_k_scale | (uintptr_t)d_v_scale) & 3) BF_FAIL("%s: the scales must be 4-byte aligned", what);
    RingAppendParams p = {};
    p.k = static_cast<const __bf16*>(d_k);
    p.v = static_cast<const __bf16*>(d_v);
    p.kq = static_cast<uint8_t*>(d_kq);
    p.vq = static_cast<uint8_t*>(d_vq);
    p.k_scale = d_k_scale;
    p.v_scale = d_v_scale;
    p.pos = d_pos;
    for (int i = 0; i < 3; ++i) {
        p.ks[i] = k_stride[i];
        p.vs[i] = v_stride[i];
    }
    p.N = N;
    p.Hkv = Hkv;
    p.Tq = T < ring_slots ? T : ring_slots;
    p.first = T - p.Tq;
    p.capacity = ring_slots;
    const long long threads = 2LL * N * Hkv * p.Tq * (D / 16);
    const long long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) BF_FAIL("%s: N * Hkv * T = %lld rows exceed the grid", what, (long long)N * Hkv * p.Tq);
    const dim3 grid((uint32_t)blocks);
    const hipStream_t st = (hipStream_t)stream;
    if (D == 64) hipLaunchKernelGGL((kv8_append_kernel<4, true>), grid, dim3(256), 0, st, p);
    else if (D == 128) hipLaunchKernelGGL((kv8_append_kernel<8, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((kv8_append_kernel<16, true>), grid, dim3(256), 0, st, p);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
