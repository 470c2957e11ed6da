// bf_gemm256_dev.h — device helpers and the tile-schedule interface shared by the translation units of the 256-wide
// sampled-weight GEMM (bf_gemm256.hip: burst / unit-ring forms; bf_gemm256_r5.hip: the five-slot ring of the forward;
// bf_gemm_schedule.hip: the host-built tile schedule).
// Everything here is internal (anonymous namespace per translation unit); the C-ABI is include/bayeformers_amd.h.
#pragma once
#include <type_traits>

#include "bf_common.h"
#include "bf_gemm_params.h"

// schedule policy bits (build_schedule): 1 = odd workgroups run their tiles in reverse order, 2 = fixed full-height
// tiles (no balancing), 4 = XCD-chunked dealing, 8 = every XCD walks a contiguous share of each height class, bits 4-7 =
// tallest tile (0 = 8 units), bits 8-11 = columns per group of the locality order (0 = 4), 0x1000 = the columns that get one
// tile more are the first ones (columns of a sample share their row cuts), 0x2000 = the column-group size is chosen per shape
// by the modelled fabric fetch.  0x300C since round 6 (12 before: same times, 9 % more fabric reads per BERT-base step:
// profiles/r6b_sched_l2_model.md)
#ifndef BF_SCHED_POLICY
#define BF_SCHED_POLICY 0x300C
#endif

// The tile schedule of a shape (built on the host once per device, kept in device memory): bf_gemm_schedule.hip.
struct Gemm256Sched {
    int4* d_table;
    int rounds, grid;
};
int bf_gemm256_get_schedule(int S, int layers, int tiles_n, int M, int policy, hipStream_t stream, Gemm256Sched& out);

// the five-slot-ring forward kernel (bf_gemm256_r5.hip)
bool bf_gemm256_r5_supported(const GemmParams& p, int w_dtype, int y_dtype);
int bf_launch_gemm256_r5(const GemmParams& p, int w_dtype, hipStream_t stream, int grid);
int bf_launch_gemm256_r5_nn(const GemmParams& p, int dtype, hipStream_t stream, int grid);

namespace {

constexpr int TN = 256, TK = 64;
constexpr int UNIT = 32;                          // rows per schedule unit (one 16-row block per wave group)
constexpr int HMAX = 8;                           // tallest tile: 256 rows = 128 fp32 accumulators per lane (9 and 10
                                                  // were measured: they spill and run 6-8 % slower per flop)
constexpr int HMIN = 4;                           // shortest tile the k-loop is instantiated for
constexpr int TM = HMAX * UNIT;                   // rows of x a stage holds
constexpr int XPIECES = TM / 64;                  // 1 KiB DMA pieces per wave for the x rows of a stage: 4
constexpr int ROW_BYTES = TK * 2;                 // 128
constexpr int X_BYTES = TM * ROW_BYTES;           // 32 KiB
constexpr int STAGE_BYTES = (TM + TN) * ROW_BYTES;  // 64 KiB

// The launch preamble of every 256-wide launcher: normalises p.layers, fills the tile counts, fetches the shape's schedule
// (built and uploaded on its first use) and points p at it.  Returns the launch grid, 0 after a failure (bf_last_error).
inline int gemm256_plan(GemmParams& p, hipStream_t stream) {
    if (p.layers < 1) p.layers = 1;
    p.tiles_m = (p.M + TM - 1) / TM;
    p.tiles_n = (p.N + TN - 1) / TN;
    Gemm256Sched sc;
    if (bf_gemm256_get_schedule(p.S, p.layers, p.tiles_n, p.M, BF_SCHED_POLICY, stream, sc)) return 0;
    p.sched = sc.d_table;
    p.sched_rounds = sc.rounds;
    return sc.grid;
}

template <typename T>
struct Mfma16;
template <>
struct Mfma16<__bf16> {
    using frag = bf16x8_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <>
struct Mfma16<_Float16> {
    using frag = f16x8_t;
    static __device__ __forceinline__ f32x4_t run(frag a, frag b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

template <>
struct Mfma16<float> {  // a 16-byte fragment = 4 consecutive k of fp32: four 16x16x4 MFMAs, ordered by bf_gemm256_r5.hip itself
    using frag = f32x4_t;
};

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
    // 64 lanes x 16 B: lane i lands at lds_wave_base + 16*i (wave-uniform base)
    __builtin_amdgcn_global_load_lds((glb_void*)g, (lds_void*)lds_wave_base, 16, 0, 0);
}

// Segmented contraction (NN form): k-step kt lies in segment kt / nks, nks = k-steps per segment (at most 4 segments);
// kt becomes the k-step inside the segment.  All wave-uniform arithmetic.
__device__ __forceinline__ int segment_of(int& kt, int nks) {
    const int seg = (kt >= nks ? 1 : 0) + (kt >= 2 * nks ? 1 : 0) + (kt >= 3 * nks ? 1 : 0);
    kt -= seg * nks;
    return seg;
}

// Fragment of a contraction-major tile (512-byte rows, 32-byte granules XOR-swizzled by the row) through the LDS transpose
// read: two ds_read_b64_tr_b16 give a lane the 8 contraction values of its row that a ds_read_b128 of a K-contiguous
// operand delivers.  a0 = the lane's address in the wave's first block, blk = block (one XOR away), half = integral_constant
// 0 / 1 (the 32-row half: an immediate offset).
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
template <typename frag, typename Half>
__device__ __forceinline__ frag tr_read(unsigned a0, int blk, Half) {
    const unsigned a = a0 ^ (unsigned)(blk << 5);
    constexpr int off = Half::value * 32 * 512;
    s16x4_t lo, hi;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(a), "n"(off));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(a), "n"(off + 4 * 512));
    const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(frag, v);
}

// acc[nb][mb][j] starts at bias[n] (n = the lane's 4 consecutive features of fragment nb): the bias add costs no
// epilogue work and its loads overlap the first DMA wait of the tile.
template <int H>
__device__ __forceinline__ void init_acc(f32x4_t (&acc)[4][H], const float* bias, int n0, int N, int wn, int lane) {
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        f32x4_t b = {0.f, 0.f, 0.f, 0.f};
        if (bias) {
            const int n = n0 + wn * 64 + nb * 16 + (lane >> 4) * 4;
            if (n + 3 < N) {
                b = *reinterpret_cast<const f32x4_t*>(bias + n);  // [S][N] fp32 rows, N % 4 == 0 checked on the host
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n + j < N) b[j] = bias[n + j];
            }
        }
#pragma unroll
        for (int mb = 0; mb < H; ++mb) acc[nb][mb] = b;
    }
}

// compile-time loop (immediate offsets for the inline-asm LDS reads)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// output stores are nontemporal (plain and sc1 / sc0 sc1 write-through stores were measured: profiles/r3t_gemm_output_store_policy.txt)
__device__ __forceinline__ void gemm_st16(f32x4_t* p, f32x4_t v) { __builtin_nontemporal_store(v, p); }


// act() of a 16-byte chunk of YT outputs (8 x 16-bit or 4 x fp32), computed in fp32
template <typename YT>
__device__ __forceinline__ f32x4_t act_chunk(f32x4_t c, int act) {
    if constexpr (sizeof(YT) == 4) {
        return bf_apply_act(c, act);
    } else {
        typedef __attribute__((ext_vector_type(8))) YT yt8;
        typedef __attribute__((ext_vector_type(4))) YT yt4;
        const yt8 h = __builtin_bit_cast(yt8, c);
        const f32x4_t lo = bf_apply_act<true>(f32x4_t{(float)h[0], (float)h[1], (float)h[2], (float)h[3]}, act);
        const f32x4_t hi = bf_apply_act<true>(f32x4_t{(float)h[4], (float)h[5], (float)h[6], (float)h[7]}, act);
        const yt4 a = __builtin_convertvector(lo, yt4), b = __builtin_convertvector(hi, yt4);
        const yt8 r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        return __builtin_bit_cast(f32x4_t, r);
    }
}

// Wave-private epilogue: a wave's part of the tile is 16 h rows x 64 features — for every
// 16-row block a full 128-byte line (256 bytes of fp32) per row.  The block goes through a 2 / 4 KiB slice of LDS that
// only this wave touches (XOR-swizzled like the operand rows: conflict-free ds_write_b64 / ds_read_b128) and leaves as
// 16-byte stores of whole lines, 8 (4) rows per instruction.  Nothing is exchanged between waves, so the epilogue has
// no barrier at all: wave group 0 starts it a slot before group 1, and every wave runs it at its own pace.
// `scratch` = this wave's 8 KiB of the stage buffer the k-loop consumed last (every fragment read of it is complete
// when a wave gets here, see the kernel).
template <typename YT, int H, int SLICES = 2>
__device__ __forceinline__ void epilogue_wave(char* scratch, const f32x4_t (&acc)[4][H], YT* y, YT* y2, int m0,
                                              int m_end, int n0, int N, int wm, int wn, int lane, int act,
                                              const YT* gpre = nullptr) {  // gpre: the stored rows are multiplied by act'(gpre)
    constexpr int ROWB = 64 * (int)sizeof(YT);   // 128 or 256
    constexpr int BLK = 16 * ROWB;               // 2 or 4 KiB
    constexpr int CH = ROWB / 16;                // 16-byte chunks per row: 8 or 16
    constexpr int RPI = 64 / CH;                 // rows per store instruction: 8 or 4
    constexpr int NI = 16 / RPI;                 // store instructions per block: 2 or 4
    constexpr int EPC = 16 / (int)sizeof(YT);
    asm volatile("" : "+v"(lane));               // offsets recomputed per tile, not hoisted into the k-loop's registers
    const bool vec_ok = (N % EPC) == 0 && ((uintptr_t)y % 16) == 0 && (!y2 || ((uintptr_t)y2 % 16) == 0);
    const int m_l = lane & 15, q = lane >> 4;
    // write side: lane holds 4 consecutive features 16 nb + 4 q of row m_l
    const int wsw = sizeof(YT) == 2 ? (m_l >> 1) & 7 : m_l;
    int wr_off[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int c = sizeof(YT) == 2 ? nb * 2 + (q >> 1) : nb * 4 + q;
        wr_off[nb] = m_l * ROWB + ((c ^ wsw) << 4) + (sizeof(YT) == 2 ? (q & 1) * 8 : 0);
    }
    // read side: instruction it covers rows it * RPI + lane / CH, chunk lane % CH
    const int rr = lane / CH, rc = lane % CH;
    const int n = n0 + wn * 64 + rc * EPC;
    const bool n_ok = n < N, n_full = vec_ok && n + EPC <= N;
    auto write_block = [&](int mb) {
        char* R = scratch + (SLICES == 2 ? (mb & 1) * BLK : 0);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const f32x4_t v = (y2 || gpre) ? acc[nb][mb] : bf_apply_act<sizeof(YT) == 2>(acc[nb][mb], act);
            char* dst = R + wr_off[nb];
            if constexpr (sizeof(YT) == 4)
                *reinterpret_cast<f32x4_t*>(dst) = v;
            else if constexpr (__is_same(YT, __bf16))
                *reinterpret_cast<bf16x4_t*>(dst) = __builtin_convertvector(v, bf16x4_t);
            else
                *reinterpret_cast<f16x4_t*>(dst) = __builtin_convertvector(v, f16x4_t);
        }
    };
    // software pipeline over the blocks: block mb + 1 is converted and written (other slice) behind the row reads of
    // block mb — one LDS round trip per block instead of two
    // gpre: the 16-byte chunks of the pre-activation that belong to the rows of block mb are fetched TWO blocks ahead (they come
    // from HBM: written by the forward pass long ago) into registers the accumulators of the blocks already written out gave up
    constexpr int PF = 2;
    f32x4_t gp[PF + 1][NI];
    auto fetch_gpre = [&](int mb) {
        if constexpr (sizeof(YT) == 2) {
#pragma unroll
            for (int it = 0; it < NI; ++it) {
                const int m = m0 + (2 * mb + wm) * 16 + it * RPI + rr;
                gp[mb % (PF + 1)][it] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                if (m < m_end && n_full) gp[mb % (PF + 1)][it] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(gpre + (unsigned)(m * N + n)));
            }
        }
    };
    write_block(0);
    if (gpre) {
#pragma unroll
        for (int b = 0; b < PF && b < H; ++b) fetch_gpre(b);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int mb = 0; mb < H; ++mb) {
        const char* R = scratch + (SLICES == 2 ? (mb & 1) * BLK : 0);
        f32x4_t rows[NI];
        if (gpre && mb + PF < H) fetch_gpre(mb + PF);
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            const int r = it * RPI + rr;
            const int rsw = sizeof(YT) == 2 ? (r >> 1) & 7 : r;
            rows[it] = *reinterpret_cast<const f32x4_t*>(R + r * ROWB + ((rc ^ rsw) << 4));
        }
        if (SLICES == 2 && mb + 1 < H) write_block(mb + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (SLICES == 1 && mb + 1 < H) {  // one slice: the next block goes in once this one's rows are in registers
            write_block(mb + 1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            const int m = m0 + (2 * mb + wm) * 16 + it * RPI + rr;
            if (m < m_end && n_ok) {
                f32x4_t v = rows[it];
                if (y2) {
                    YT* o2 = y2 + (unsigned)(m * N + n);
                    if (n_full) {
                        gemm_st16(reinterpret_cast<f32x4_t*>(o2), v);
                    } else {
                        const YT* e = reinterpret_cast<const YT*>(&v);
                        for (int j = 0; j < EPC; ++j)
                            if (n + j < N) o2[j] = e[j];
                    }
                    v = act_chunk<YT>(v, act);
                }
                YT* o = y + (unsigned)(m * N + n);
                if constexpr (sizeof(YT) == 2) {
                    if (gpre && n_full) {  // (whole 16-byte chunks only: the host requires N % 8 == 0 for this form)
                        typedef __attribute__((ext_vector_type(8))) YT yt8;
                        const yt8 g = __builtin_bit_cast(yt8, v);
                        const yt8 x = __builtin_bit_cast(yt8, gp[mb % (PF + 1)][it]);
                        yt8 r;
#pragma unroll
                        for (int j = 0; j < 8; ++j) r[j] = (YT)((float)g[j] * bf_gelu_grad((float)x[j]));
                        v = __builtin_bit_cast(f32x4_t, r);
                    }
                }
                if (n_full) {
                    gemm_st16(reinterpret_cast<f32x4_t*>(o), v);
                } else {
                    const YT* e = reinterpret_cast<const YT*>(&v);
                    for (int j = 0; j < EPC; ++j)
                        if (n + j < N) o[j] = e[j];
                }
            }
        }
    }
}

// The LDS image of a 16-row block in epilogue_wave_full: 128-byte rows, the 16-byte chunks of a row XOR-swizzled by
// (row >> 1) & 7 — the formulas of epilogue_wave's 16-bit case.  (Each epilogue writes and reads its own image, so the two need
// not agree; epilogue_wave keeps its inline arithmetic because routing it through these helpers reorders instructions in every
// kernel that uses it.)  Write side: lane (row m_l = lane & 15, q = lane >> 4) holds the 4 consecutive features 16 nb + 4 q of
// its row; read side: chunk rc of row r.  Byte offsets inside the block.
__device__ __forceinline__ int epi16_wr_off(int m_l, int q, int nb) {
    return m_l * 128 + (((nb * 2 + (q >> 1)) ^ ((m_l >> 1) & 7)) << 4) + (q & 1) * 8;
}
__device__ __forceinline__ int epi16_rd_off(int r, int rc) { return r * 128 + ((rc ^ ((r >> 1) & 7)) << 4); }

// The epilogue of a FULL tile of 16-bit outputs (every row of the tile's template height inside M, all 256 columns inside
// N, whole aligned 16-byte chunks, no second output): the same values on the same route as epilogue_wave — act() on the
// fp32 accumulators, rounded once, through the wave's two 2 KiB slices, out as nontemporal 16-byte stores of whole lines —
// with nothing per lane left to decide and two blocks in flight.
//  - No predicate, no EXEC change, one wave-uniform choice of the activation per tile instead of one per fragment.
//  - Stores go through a buffer descriptor whose base is this wave's part of the tile (`yw` = its first element: row 16 wm of
//    the tile at column 64 wn): ONE per-lane byte offset per tile ((lane / 8) rows + 16 (lane % 8) bytes), and store `it` of
//    block mb adds (32 mb + 8 it) rows as the SCALAR offset, so the element written is row m0 + 16 wm + 32 mb + 8 it + lane / 8,
//    column n0 + 64 wn + 8 (lane % 8) — epilogue_wave's mapping.  The descriptor is there for the addressing form (no 64-bit
//    vector arithmetic), NOT as a guard: the range check of a raw buffer covers the per-lane offset only, never the scalar
//    offset that carries the row multiple, so nothing clamps a wrong row.  The stores are in range by arithmetic: the caller
//    takes this path only for a tile whose 32 H rows and 256 columns lie inside the matrix.  All byte offsets are 32-bit: the
//    caller also requires N <= 2^22, which keeps the largest one, (32 H - 17) rows + 128 bytes at H = 8, below 2^31.
//  - A wave's LDS operations execute in issue order, so the only waits are the counted ones before a block's rows are stored:
//        W(0) W(1) R(0) | R(1) W(2) [R(0) landed] S(0) | R(2) W(3) [R(1) landed] S(1) | ...
//    R(mb + 1) is issued before the stores of block mb and reads what W(mb + 1) wrote a block earlier; W(mb + 2) goes into
//    the slice of block mb behind R(mb).  The waits are the compiler's own (all these are plain LDS accesses it counts; no
//    scalar load is outstanding here: the next schedule entry was consumed by the last k-steps): lgkmcnt(11) and (10) in
//    the steady state — the second read of the block, W(mb + 1), R(mb + 1) and W(mb + 2) are younger than the row being stored —
//    instead of a full drain, and the read latency of a block is covered by the conversion of the block after next.
//    The rows of one more block live in registers that the accumulators already written out gave up.
template <typename YT, int H, bool GELU>
__device__ __forceinline__ void epilogue_wave_full(char* scratch, const f32x4_t (&acc)[4][H], YT* yw, int N, int lane) {
    static_assert(sizeof(YT) == 2, "16-bit outputs");
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
    constexpr int BLK = 16 * 128;                // one slice: 16 rows of 128 bytes
    asm volatile("" : "+v"(lane));               // offsets recomputed per tile, not hoisted into the k-loop's registers
    int wr_off[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) wr_off[nb] = epi16_wr_off(lane & 15, lane >> 4, nb);
    // read side: instruction it covers rows 8 it + lane / 8, chunk lane % 8
    const int rr = lane >> 3, rc = lane & 7;
    int rd_off[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) rd_off[it] = epi16_rd_off(it * 8 + rr, rc);
    const unsigned row_bytes = (unsigned)N * 2u;
    const unsigned voff = (unsigned)rr * row_bytes + (unsigned)rc * 16u;
    const __amdgpu_buffer_rsrc_t dsc =
        __builtin_amdgcn_make_buffer_rsrc(yw, 0, (int)((unsigned)(32 * H - 17) * row_bytes + 128u), 0x00020000);
    auto write_block = [&](int mb) {
        char* R = scratch + (mb & 1) * BLK;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const f32x4_t v = GELU ? bf_apply_act<true>(acc[nb][mb], BF_ACT_GELU) : acc[nb][mb];
            if constexpr (__is_same(YT, __bf16))
                *reinterpret_cast<bf16x4_t*>(R + wr_off[nb]) = __builtin_convertvector(v, bf16x4_t);
            else
                *reinterpret_cast<f16x4_t*>(R + wr_off[nb]) = __builtin_convertvector(v, f16x4_t);
        }
    };
    u32x4_t rows[2][2];
    auto read_block = [&](int mb) {
        const char* R = scratch + (mb & 1) * BLK;
#pragma unroll
        for (int it = 0; it < 2; ++it) rows[mb & 1][it] = *reinterpret_cast<const u32x4_t*>(R + rd_off[it]);
    };
    static_assert(H >= 2, "two blocks in flight");
    write_block(0);
    write_block(1);
    read_block(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mb = 0; mb < H; ++mb) {
        if (mb + 1 < H) read_block(mb + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (mb + 2 < H) write_block(mb + 2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int it = 0; it < 2; ++it)  // rows (2 mb + wm) 16 + 8 it + rr: nontemporal, 8 whole lines per instruction
            __builtin_amdgcn_raw_buffer_store_b128(rows[mb & 1][it], dsc, (int)voff, (int)((unsigned)(4 * mb + it) * 8u * row_bytes), 2);
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace
