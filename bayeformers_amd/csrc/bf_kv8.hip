// bf_kv8.hip — the FP8 KV cache of sample_generate(kv_cache="fp8") (include/bayeformers_amd_kv8.h): each cached K and V row
// is D e4m3fn bytes over one fp32 power-of-two scale (bf_fp8.h's row format with centre zero).
//   * bf_kv8_append: the new K and V rows [N][Hkv][Tq][D] bf16 of a forward -> bytes and scales at cache slots
//     pos .. pos + Tq - 1, pos a device int64 (the layer's fill), so one captured launch serves every step;
//   * bf_kv8_dequantize: bytes and scales -> bf16 rows, for the callers that read a 16-bit cache.
// The decode kernel that reads the rows directly is bf_attention_decode.hip's KV8 form.
// A row is owned by D / 16 neighbouring lanes, 16 features each: two 16-byte loads, the row's amax by shuffles among those
// lanes, one 16-byte store.  No host synchronisation or allocation: capturable.
#include "bf_kv8_rows.h"

namespace {

// 16 features per thread and step
__global__ __launch_bounds__(256) void kv8_dequantize_kernel(const uint8_t* __restrict__ q, const float* __restrict__ scale,
                                                             __bf16* __restrict__ out, long long rows, int D) {
    const int pieces = D / 16;
    const long long total = rows * pieces;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / pieces;
        const u32x4_t b = *reinterpret_cast<const u32x4_t*>(q + i * 16);
        const float s = scale[row];
        *reinterpret_cast<bf16x8_t*>(out + i * 16) = fp8_rows_value(u32x2_t{b[0], b[1]}, s);
        *reinterpret_cast<bf16x8_t*>(out + i * 16 + 8) = fp8_rows_value(u32x2_t{b[2], b[3]}, s);
    }
}

}  // namespace

int bf_kv8_append(const void* d_k, const void* d_v, int dtype, const int64_t* k_stride, const int64_t* v_stride, void* d_kq,
                  void* d_vq, float* d_k_scale, float* d_v_scale, const int64_t* d_pos, int N, int Hkv, int Tq, int D,
                  int capacity, void* stream) {
    const char* what = "bf_kv8_append";
    if (dtype != BF_DT_BF16) BF_FAIL("%s: k and v must be bf16 (bfloat16: the dequantised rows are exact in it alone)", what);
    if (D != 64 && D != 128 && D != 256) BF_FAIL("%s: head size %d (64, 128 or 256)", what, D);
    if (!d_k || !d_v || !d_kq || !d_vq || !k_stride || !v_stride) BF_FAIL("%s: NULL argument", what);
    if (!d_k_scale || !d_v_scale) BF_FAIL("%s: NULL scale", what);
    if (N < 1 || Hkv < 1 || Tq < 1 || capacity < 1)
        BF_FAIL("%s: N=%d, Hkv=%d, Tq=%d, capacity=%d must be positive", what, N, Hkv, Tq, capacity);
    if (((uintptr_t)d_k | (uintptr_t)d_v | (uintptr_t)d_kq | (uintptr_t)d_vq) & 15)
        BF_FAIL("%s: k, v, kq and vq must be 16-byte aligned", what);
    if (((uintptr_t)d_k_scale | (uintptr_t)d_v_scale) & 3) BF_FAIL("%s: the scales must be 4-byte aligned", what);
    if (!d_pos || ((uintptr_t)d_pos & 7)) BF_FAIL("%s: pos must be an 8-byte aligned device int64", what);
    for (int i = 0; i < 3; ++i)
        if (k_stride[i] < 0 || k_stride[i] % 8 || v_stride[i] < 0 || v_stride[i] % 8)
            BF_FAIL("%s: strides must be non-negative multiples of 8 elements", what);
    const int lpr = D / 16;
    const long long threads = 2LL * N * Hkv * Tq * lpr;
    const long long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) BF_FAIL("%s: N * Hkv * Tq = %lld rows exceed the grid", what, (long long)N * Hkv * Tq);
    AppendParams p = {};
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
    p.Tq = Tq;
    p.capacity = capacity;
    const dim3 grid((uint32_t)blocks);
    const hipStream_t st = (hipStream_t)stream;
    if (D == 64) hipLaunchKernelGGL(kv8_append_kernel<4>, grid, dim3(256), 0, st, p);
    else if (D == 128) hipLaunchKernelGGL(kv8_append_kernel<8>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(kv8_append_kernel<16>, grid, dim3(256), 0, st, p);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

int bf_kv8_dequantize(const void* d_q, const float* d_scale, void* d_out, int dtype, int64_t rows, int D, void* stream) {
    const char* what = "bf_kv8_dequantize";
    if (dtype != BF_DT_BF16) BF_FAIL("%s: out must be bf16 (bfloat16: the dequantised rows are exact in it alone)", what);
    if (D < 16 || D % 16) BF_FAIL("%s: D=%d must be a positive multiple of 16", what, D);
    if (rows < 1) BF_FAIL("%s: rows=%lld must be positive", what, (long long)rows);
    if (!d_q || !d_out) BF_FAIL("%s: NULL argument", what);
    if (!d_scale) BF_FAIL("%s: NULL scale", what);
    if (((uintptr_t)d_q | (uintptr_t)d_out) & 15) BF_FAIL("%s: q and out must be 16-byte aligned", what);
    if ((uintptr_t)d_scale & 3) BF_FAIL("%s: scale must be 4-byte aligned", what);
    const long long work = (long long)rows * (D / 16);
    const long long blocks = (work + 255) / 256;
    const dim3 grid((uint32_t)(blocks < 65536 ? blocks : 65536));
    hipLaunchKernelGGL(kv8_dequantize_kernel, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const uint8_t*>(d_q), d_scale,
                       static_cast<__bf16*>(d_out), (long long)rows, D);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
