// bf_kv8_rows.h — the quantising append of the FP8 KV cache (include/bayeformers_amd_kv8.h's row format), shared by
// bf_kv8.hip (bf_kv8_append: slots in sequence order) and bf_kv_ring.hip (bf_kv8_ring_append: slot = index % ring_slots).
// One kernel with a compile-time RING form and a parameter block of its own for it: the plain instantiations are what they
// were when the kernel lived in bf_kv8.hip.
#pragma once
#include "bf_common.h"
#include "bf_fp8.h"

#include <type_traits>

namespace {

struct AppendParams {
    const __bf16* k;
    const __bf16* v;
    uint8_t* kq;
    uint8_t* vq;
    float* k_scale;
    float* v_scale;
    const int64_t* pos;
    long long ks[3], vs[3];  // (batch, head, token) element strides of k and v
    int N, Hkv, Tq, capacity;
};
// RING: `capacity` is the ring's slot count and row i of the launch is row first + i of k / v, bound for slot
// (*pos + first + i) % capacity (Tq <= capacity rows a launch: no slot is written twice)
struct RingAppendParams : AppendParams {
    int first;
};

// LPR lanes per row, 16 features each (D = 16 LPR)
template <int LPR, bool RING = false>
__global__ __launch_bounds__(256) void kv8_append_kernel(const std::conditional_t<RING, RingAppendParams, AppendParams> p) {
    constexpr int D = 16 * LPR;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per = (long long)p.N * p.Hkv * p.Tq;  // rows of K; V's follow
    const long long row = t / LPR;
    const int part = (int)(t % LPR);
    const bool is_v = row >= per;
    const long long r = is_v ? row - per : row;
    const int i = (int)(r % p.Tq), g = (int)(r / p.Tq % p.Hkv);
    const long long n = r / ((long long)p.Tq * p.Hkv);
    int64_t slot = *p.pos + i;
    int in = i;  // the row of k / v
    if constexpr (RING) {
        in = p.first + i;
        slot = *p.pos < 0 ? -1 : (slot + p.first) % p.capacity;  // (a negative fill: nothing is written)
    }
    // (the lanes of a row agree on `live`; a dead row still takes part in the shuffles below, on zeros)
    const bool live = row < 2 * per && slot >= 0 && slot < p.capacity;

    float x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = 0.f;
    if (live) {
        const long long* st = is_v ? p.vs : p.ks;
        const __bf16* src = (is_v ? p.v : p.k) + n * st[0] + g * st[1] + in * st[2] + part * 16;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bf16x8_t w = *reinterpret_cast<const bf16x8_t*>(src + h * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) x[h * 8 + j] = (float)w[j];
        }
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) amax = fmaxf(amax, fabsf(x[j]));
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    if (!live) return;

    const int e = fp8_row_exponent(amax);
    const float inv = pow2f(-e);
    const long long orow = (n * p.Hkv + g) * p.capacity + slot;  // < N * Hkv * capacity: inside the four buffers
    u32x4_t out;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = x[h * 8 + j];
        const u32x2_t b = fp8_rows_encode(d, inv);
        out[2 * h] = b[0];
        out[2 * h + 1] = b[1];
    }
    *reinterpret_cast<u32x4_t*>((is_v ? p.vq : p.kq) + orow * D + part * 16) = out;
    if (part == 0) (is_v ? p.v_scale : p.k_scale)[orow] = pow2f(e);
}

}  // namespace
