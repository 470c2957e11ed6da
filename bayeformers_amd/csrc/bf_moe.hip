// bf_moe.hip — Bayesian mixture-of-experts layers (include/bayeformers_amd_moe.h: bf_moe_route, bf_moe_gate_up, bf_moe_down,
// bf_moe_combine).  Every (sample, expert) pair has a weight matrix of its own, so the products are a grouped GEMM over
// S * E groups whose sizes the router decides; the route entry lays the groups out on the device and the GEMMs run a fixed
// grid over a tile table.
//
// Kernels in this file
//   moe_scatter_kernel<FILL> : a wave per (sample, expert) walks the sample's slots 64 at a time (ballot): FILL = false
//                              counts its slots, FILL = true writes their numbers from the group's offset on, in slot order
//   moe_scan_kernel          : one workgroup: exclusive scan of the counts -> offsets, tiles per group -> the tile table
//   moe_tile_kernel<T, GATED>: a 16-row tile of one group times 64 features of its weight matrix on v_mfma_f32_16x16x32,
//                              operands k-contiguous straight from global memory (16 bytes per lane).  GATED: rows of x
//                              gathered by slot / k, gate and up accumulators, h = silu(gate) * up rounded once.
//                              Otherwise rows of h by slot, one accumulator, fp32 y at the slot's own row.
//   moe_combine_kernel<T, WT>: out[r] = sum_j w[r][j] * y[r][j] in j order, dropped slots skipped, rounded once
// No atomics anywhere: every output element is written by one thread and every sum has a fixed order.
#include "bf_common.h"

namespace {

template <typename T>
struct Mma;
template <>
struct Mma<__bf16> {
    using frag = bf16x8_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <>
struct Mma<_Float16> {
    using frag = f16x8_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

constexpr int kBM = BF_MOE_TILE_ROWS;
constexpr int kScanThreads = 256;
constexpr int kScanChunk = BF_MOE_MAX_GROUPS / kScanThreads;  // groups per thread of the scan, at the cap
static_assert(kBM == 16, "a tile is one 16-row MFMA block");
static_assert(kScanChunk * kScanThreads == BF_MOE_MAX_GROUPS, "the scan covers the cap exactly");

// grid = (ceil(E / 4), S), 256 threads: wave w of block b owns expert e = 4 b + w of sample blockIdx.y.  The sample's slots are
// the contiguous range [s * Mk, (s + 1) * Mk) of top [R * k]; an index that is no expert (E, the dropped sentinel) matches
// no wave.  FILL: slots[offsets[g] + i] = number of the group's i-th slot in slot order; else counts[g] = its slot count.
template <bool FILL>
__global__ __launch_bounds__(256) void moe_scatter_kernel(const long long* __restrict__ top, const int* __restrict__ offsets,
                                                          int* __restrict__ out, int E, int Mk) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + wave, s = blockIdx.y;
    if (e >= E) return;
    const int g = s * E + e;
    const long long base = (long long)s * Mk;
    int n = FILL ? offsets[g] : 0;
    for (int i0 = 0; i0 < Mk; i0 += 64) {
        const int i = i0 + lane;
        const bool hit = i < Mk && top[base + i] == (long long)e;
        const unsigned long long m = __ballot(hit);
        if (FILL && hit) out[n + __popcll(m & ((1ull << lane) - 1ull))] = (int)(base + i);
        n += __popcll(m);
    }
    if (!FILL && lane == 0) out[g] = n;
}

// One workgroup of 256 threads; thread t owns groups [t * chunk, (t + 1) * chunk), chunk = ceil(G / 256) <= kScanChunk.
// offsets[g] = slots before group g, offsets[G] = live slots; tiles[t] = {g, first position, live rows} for the tiles of
// every group in group order, {0, 0, 0} for tiles [total, max_tiles).
__global__ __launch_bounds__(kScanThreads) void moe_scan_kernel(const int* __restrict__ counts, int* __restrict__ offsets,
                                                                int* __restrict__ tiles, int G, int max_tiles) {
    __shared__ int s_slots[kScanThreads], s_tiles[kScanThreads];
    const int t = threadIdx.x;
    const int chunk = (G + kScanThreads - 1) / kScanThreads;
    const int g_lo = min(G, t * chunk), g_hi = min(G, g_lo + chunk);
    int n_slots = 0, n_tiles = 0;
    for (int g = g_lo; g < g_hi; ++g) {
        const int c = counts[g];
        n_slots += c;
        n_tiles += (c + kBM - 1) / kBM;
    }
    s_slots[t] = n_slots;
    s_tiles[t] = n_tiles;
    __syncthreads();
    // inclusive scan over the 256 thread totals (integers: any order gives the same sums)
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int a = t >= d ? s_slots[t - d] : 0, b = t >= d ? s_tiles[t - d] : 0;
        __syncthreads();
        s_slots[t] += a;
        s_tiles[t] += b;
        __syncthreads();
    }
    int pos = s_slots[t] - n_slots, tile = s_tiles[t] - n_tiles;
    const int total = s_tiles[kScanThreads - 1];
    for (int g = g_lo; g < g_hi; ++g) {
        const int c = counts[g];
        offsets[g] = pos;
        for (int r0 = 0; r0 < c; r0 += kBM, ++tile) {
            if (tile < max_tiles) {  // (always: max_tiles bounds the sum; the guard keeps a wrong bound from writing outside)
                tiles[3 * tile] = g;
                tiles[3 * tile + 1] = pos + r0;
                tiles[3 * tile + 2] = min(kBM, c - r0);
            }
        }
        pos += c;
    }
    if (t == kScanThreads - 1) offsets[G] = s_slots[t];
    for (int i = total + t; i < max_tiles; i += kScanThreads) tiles[3 * i] = tiles[3 * i + 1] = tiles[3 * i + 2] = 0;
}

template <typename T>
__device__ __forceinline__ typename Mma<T>::frag load_frag(const T* p) {
    return *reinterpret_cast<const typename Mma<T>::frag*>(p);
}

__device__ __forceinline__ float silu(float v) { return v / (1.0f + __expf(-v)); }

// out rows of one tile times features [n0, n0 + 64) of its group's matrix.  a: GATED ? x [R][K] : h [R*k][K]; w: [G][NW][K]
// with NW = GATED ? 2 N : N output features per group; slots / tiles: bf_moe_route's.  grid = (max_tiles, ceil(N / 64)); a
// wave owns 16 features.  A operand: row li of the tile (gathered), 8 consecutive k of group lg; B operand: feature
// n0 + 16 wave + li, the same k; D: tile rows 4 lg + reg, feature li of the wave's 16.  Rows past the tile's live count and
// features past N are zero operands and are not stored; k-steps past K multiply zeros (K % 8 == 0: a lane's 8 elements are
// inside or outside together).
template <typename T, bool GATED>
__global__ __launch_bounds__(256) void moe_tile_kernel(const T* __restrict__ a, const T* __restrict__ w,
                                                       const int* __restrict__ slots, const int* __restrict__ tiles,
                                                       void* __restrict__ out, int k_top, int N, int K) {
    using frag = typename Mma<T>::frag;
    const int live = tiles[3 * blockIdx.x + 2];
    if (live == 0) return;  // a surplus tile
    const int g = tiles[3 * blockIdx.x], first = tiles[3 * blockIdx.x + 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int nw0 = blockIdx.y * 64 + wave * 16;
    if (nw0 >= N) return;  // (the whole wave: no barrier follows)
    const int n = nw0 + li;
    const bool n_ok = n < N, row_ok = li < live;
    const int slot = row_ok ? slots[first + li] : 0;
    const T* a_row = a + (size_t)(GATED ? slot / k_top : slot) * K;
    const size_t NW = GATED ? 2 * (size_t)N : (size_t)N;
    const T* w_row = w + ((size_t)g * NW + (n_ok ? n : 0)) * K;
    const T* w_up = w_row + (size_t)N * K;  // (GATED only: the `up` half of gate_up)
    const frag zero = {};
    f32x4_t acc0 = {}, acc1 = {};
    // four k-steps of 32 per round, every load issued before the first MFMA
    for (int kb = 0; kb < K; kb += 128) {
        frag af[4], wf[4], uf[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kk = kb + u * 32 + lg * 8;
            const bool k_ok = kk < K;
            af[u] = row_ok && k_ok ? load_frag<T>(a_row + kk) : zero;
            wf[u] = n_ok && k_ok ? load_frag<T>(w_row + kk) : zero;
            if (GATED) uf[u] = n_ok && k_ok ? load_frag<T>(w_up + kk) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc0 = Mma<T>::run(af[u], wf[u], acc0);
            if (GATED) acc1 = Mma<T>::run(af[u], uf[u], acc1);
        }
    }
    if (!n_ok) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = lg * 4 + i;
        if (row < live) {
            const size_t o = (size_t)slots[first + row] * N + n;
            if (GATED)
                reinterpret_cast<T*>(out)[o] = (T)(silu(acc0[i]) * acc1[i]);
            else
                reinterpret_cast<float*>(out)[o] = acc0[i];
        }
    }
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__bf16 v) { return (float)v; }
__device__ __forceinline__ float to_f32(_Float16 v) { return (float)v; }

// A thread owns 4 consecutive columns of one row (H % 8 == 0).  y [R][k][H] fp32; dropped slots (index outside 0 .. E-1) are
// skipped: their y rows were never written.
template <typename T, typename WT>
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ y, const long long* __restrict__ top,
                                                          const WT* __restrict__ wts, T* __restrict__ out, int E, int k_top,
                                                          int H, unsigned long long total) {
    const unsigned long long idx = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int h4 = H >> 2;
    const unsigned long long r = idx / h4;
    const int c = (int)(idx - r * h4) * 4;
    f32x4_t acc = {};
    for (int j = 0; j < k_top; ++j) {
        const long long e = top[r * k_top + j];
        if (e < 0 || e >= E) continue;
        const float wj = to_f32(wts[r * k_top + j]);
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(y + (r * k_top + j) * H + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += wj * v[i];
    }
    T* o = out + r * H + c;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (T)acc[i];
}

bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

// What every entry refuses about the routing problem; `what` names the entry.
int moe_check_route(const char* what, int S, int E, int R, int k) {
    if (S < 1 || E < 1 || R < 1 || k < 1) BF_FAIL("%s: bad shape S=%d E=%d R=%d k=%d", what, S, E, R, k);
    if (k > BF_MOE_MAX_TOPK) BF_FAIL("%s: k=%d: needs k <= %d", what, k, BF_MOE_MAX_TOPK);
    if ((long long)S * E > BF_MOE_MAX_GROUPS)
        BF_FAIL("%s: S*E=%lld groups: needs S*E <= %d", what, (long long)S * E, BF_MOE_MAX_GROUPS);
    if (S > 65535) BF_FAIL("%s: S=%d: needs S <= 65535", what, S);
    if (R % S) BF_FAIL("%s: R=%d rows: needs R %% S == 0 (S=%d)", what, R, S);
    if ((long long)R * k > 0x7fffffffLL) BF_FAIL("%s: R*k=%lld slots: needs R*k < 2^31", what, (long long)R * k);
    return 0;
}

// ... and about the products
int moe_check_gemm(const char* what, int dtype, int S, int E, int R, int k, int H, int I) {
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16)
        BF_FAIL("%s: dtype %d: needs BF_DT_BF16 or BF_DT_F16 (16-bit compute)", what, dtype);
    if (moe_check_route(what, S, E, R, k)) return 1;
    if (H < 1 || I < 1) BF_FAIL("%s: bad shape H=%d I=%d", what, H, I);
    if (H % 8) BF_FAIL("%s: H=%d: needs H %% 8 == 0", what, H);
    if (I % 8) BF_FAIL("%s: I=%d: needs I %% 8 == 0", what, I);
    return 0;
}

size_t max_tiles(int S, int E, int R, int k) {
    const long long slots = (long long)R * k, G = (long long)S * E;
    return (size_t)(slots / kBM + (G < slots ? G : slots));
}

template <typename T, bool GATED>
int launch_tiles(const void* a, const void* w, const int* slots, const int* tiles, void* out, int S, int E, int R, int k,
                 int N, int K, hipStream_t stream) {
    const size_t nt = max_tiles(S, E, R, k);
    if (nt > 0x7fffffffULL) BF_FAIL("bf_moe: %zu tiles: needs fewer than 2^31", nt);
    hipLaunchKernelGGL((moe_tile_kernel<T, GATED>), dim3((unsigned)nt, (N + 63) / 64), dim3(256), 0, stream,
                       reinterpret_cast<const T*>(a), reinterpret_cast<const T*>(w), slots, tiles, out, k, N, K);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T, typename WT>
int launch_combine(const float* y, const long long* top, const void* wts, void* out, int E, int R, int k, int H,
                   hipStream_t stream) {
    const unsigned long long total = (unsigned long long)R * (H / 4);
    hipLaunchKernelGGL((moe_combine_kernel<T, WT>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, y, top,
                       reinterpret_cast<const WT*>(wts), reinterpret_cast<T*>(out), E, k, H, total);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

size_t bf_moe_max_tiles(int S, int E, int R, int k) {
    if (S < 1 || E < 1 || R < 1 || k < 1) return 0;
    return max_tiles(S, E, R, k);
}

size_t bf_moe_route_workspace_bytes(int S, int E, int, int) {
    if (S < 1 || E < 1) return 0;
    return bf_align_up((size_t)S * E * sizeof(int), 256);
}

int bf_moe_route(const long long* d_top_k_index, int* d_offsets, int* d_slots, int* d_tiles, int S, int E, int R, int k,
                 void* d_workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (moe_check_route("bf_moe_route", S, E, R, k)) return 1;
    if (!d_top_k_index || !d_offsets || !d_slots || !d_tiles)
        BF_FAIL("bf_moe_route: NULL argument (top_k_index, offsets, slots and tiles are required)");
    const size_t need = bf_moe_route_workspace_bytes(S, E, R, k);
    if (!d_workspace || workspace_bytes < need)
        BF_FAIL("bf_moe_route: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    if (!aligned16(d_workspace)) BF_FAIL("bf_moe_route: the workspace must be 16-byte aligned");
    const size_t nt = max_tiles(S, E, R, k);
    if (nt > 0x7fffffffULL / 3) BF_FAIL("bf_moe_route: %zu tiles: needs 3 * tiles < 2^31", nt);
    int* counts = reinterpret_cast<int*>(d_workspace);
    const int G = S * E, Mk = R / S * k;
    const dim3 grid((E + 3) / 4, S);
    hipLaunchKernelGGL((moe_scatter_kernel<false>), grid, dim3(256), 0, stream, d_top_k_index, (const int*)nullptr, counts, E,
                       Mk);
    BF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, counts, d_offsets, d_tiles, G, (int)nt);
    BF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((moe_scatter_kernel<true>), grid, dim3(256), 0, stream, d_top_k_index, d_offsets, d_slots, E, Mk);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

size_t bf_moe_gate_up_workspace_bytes(int, int, int, int, int, int, int) { return 0; }

int bf_moe_gate_up(const void* d_x, const void* d_w_gu, const int* d_slots, const int* d_tiles, void* d_h, int dtype, int S,
                   int E, int R, int k, int H, int I, void* /*d_workspace*/, size_t /*workspace_bytes*/, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (moe_check_gemm("bf_moe_gate_up", dtype, S, E, R, k, H, I)) return 1;
    if (!d_x || !d_w_gu || !d_slots || !d_tiles || !d_h)
        BF_FAIL("bf_moe_gate_up: NULL argument (x, w_gu, slots, tiles and h are required)");
    if (!aligned16(d_x) || !aligned16(d_w_gu) || !aligned16(d_h))
        BF_FAIL("bf_moe_gate_up: every operand must be 16-byte aligned");
    if (dtype == BF_DT_BF16) return launch_tiles<__bf16, true>(d_x, d_w_gu, d_slots, d_tiles, d_h, S, E, R, k, I, H, stream);
    return launch_tiles<_Float16, true>(d_x, d_w_gu, d_slots, d_tiles, d_h, S, E, R, k, I, H, stream);
}

size_t bf_moe_down_workspace_bytes(int, int, int, int, int, int, int) { return 0; }

int bf_moe_down(const void* d_h, const void* d_w_d, const int* d_slots, const int* d_tiles, float* d_y, int dtype, int S, int E,
                int R, int k, int H, int I, void* /*d_workspace*/, size_t /*workspace_bytes*/, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (moe_check_gemm("bf_moe_down", dtype, S, E, R, k, H, I)) return 1;
    if (!d_h || !d_w_d || !d_slots || !d_tiles || !d_y)
        BF_FAIL("bf_moe_down: NULL argument (h, w_d, slots, tiles and y are required)");
    if (!aligned16(d_h) || !aligned16(d_w_d) || !aligned16(d_y)) BF_FAIL("bf_moe_down: every operand must be 16-byte aligned");
    if (dtype == BF_DT_BF16) return launch_tiles<__bf16, false>(d_h, d_w_d, d_slots, d_tiles, d_y, S, E, R, k, H, I, stream);
    return launch_tiles<_Float16, false>(d_h, d_w_d, d_slots, d_tiles, d_y, S, E, R, k, H, I, stream);
}

size_t bf_moe_combine_workspace_bytes(int, int, int) { return 0; }

int bf_moe_combine(const float* d_y, const long long* d_top_k_index, const void* d_top_k_weights, int weights_dtype,
                   void* d_out, int dtype, int E, int R, int k, int H, void* /*d_workspace*/, size_t /*workspace_bytes*/,
                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16)
        BF_FAIL("bf_moe_combine: dtype %d: needs BF_DT_BF16 or BF_DT_F16 (16-bit compute)", dtype);
    if (weights_dtype != BF_DT_F32 && weights_dtype != dtype)
        BF_FAIL("bf_moe_combine: weights dtype %d: needs BF_DT_F32 or the compute dtype %d", weights_dtype, dtype);
    if (E < 1 || R < 1 || k < 1 || H < 1) BF_FAIL("bf_moe_combine: bad shape E=%d R=%d k=%d H=%d", E, R, k, H);
    if (k > BF_MOE_MAX_TOPK) BF_FAIL("bf_moe_combine: k=%d: needs k <= %d", k, BF_MOE_MAX_TOPK);
    if (H % 8) BF_FAIL("bf_moe_combine: H=%d: needs H %% 8 == 0", H);
    if ((long long)R * k > 0x7fffffffLL) BF_FAIL("bf_moe_combine: R*k=%lld slots: needs R*k < 2^31", (long long)R * k);
    if (!d_y || !d_top_k_index || !d_top_k_weights || !d_out)
        BF_FAIL("bf_moe_combine: NULL argument (y, top_k_index, top_k_weights and out are required)");
    if (!aligned16(d_y) || !aligned16(d_out)) BF_FAIL("bf_moe_combine: y and out must be 16-byte aligned");
    if (dtype == BF_DT_BF16) {
        if (weights_dtype == BF_DT_F32)
            return launch_combine<__bf16, float>(d_y, d_top_k_index, d_top_k_weights, d_out, E, R, k, H, stream);
        return launch_combine<__bf16, __bf16>(d_y, d_top_k_index, d_top_k_weights, d_out, E, R, k, H, stream);
    }
    if (weights_dtype == BF_DT_F32)
        return launch_combine<_Float16, float>(d_y, d_top_k_index, d_top_k_weights, d_out, E, R, k, H, stream);
    return launch_combine<_Float16, _Float16>(d_y, d_top_k_index, d_top_k_weights, d_out, E, R, k, H, stream);
}

}  // extern "C"
