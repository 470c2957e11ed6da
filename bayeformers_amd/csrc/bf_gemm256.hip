// bf_gemm256.hip — the fast path of the sampled-weight GEMM on gfx950: y[s] = x[s] W_s^T + b_s
// (F.linear at /root/reference/bayeformers/nn/layers/linear.py:104, all S samples in one launch).
//
// Shape of the kernel (MI355X: 256 CUs, 160 KiB LDS/CU, wave64, v_mfma_f32_16x16x32_{bf16,f16}):
//   * one (32 h)(m) x 256(n) output tile per 512-thread workgroup, h = 4..8 (128..256 rows), 8 waves = 2(m) x 4(n);
//     the two wave groups take the 16-row blocks of the tile alternately (group g owns blocks g, g+2, ...), so a wave
//     holds 16 h x 64 outputs = 16 h fp32 accumulator registers per lane; K walked in steps of 64;
//   * both operands are K-contiguous ([M][K] activations, [N][K] sampled weights) and are DMA'd straight into LDS
//     with global_load_lds_dwordx4 (no VGPR round trip), double-buffered: 2 x (256+256) rows x 128 B = 128 KiB;
//   * LDS rows are 128 B; the 16-byte chunk c of row r is stored at chunk position c ^ ((r >> 1) & 7).  The DMA
//     destination is lane-linear, so the swizzle is applied to the per-lane SOURCE address and again on the
//     fragment read, which makes every ds_read_b128 of an MFMA fragment bank-conflict-free;
//   * the MFMA runs with swapped operands (D rows = n, cols = m) so each lane owns 4 consecutive output features
//     of one row of y; the epilogue moves a wave's 16 h x 64 part through a private LDS slice and stores whole
//     128-byte lines (epilogue_wave below);
//   * WHICH tiles a workgroup runs is decided on the host (build_schedule, bf_gemm_schedule.hip): the output is cut into columns
//     (sample, layer, n-tile) of ceil(M/32) units of 32 rows, every column into tiles of near-equal height, and the
//     tiles are dealt to the 256 persistent workgroups so that all of them carry the same number of units.  With
//     fixed 256-row tiles BERT-base's launches have 480 k tiles = 1.875 k rounds of 256 CUs — 1/16 of the CU-time is
//     a partial last round; with heights {8, 7} every CU gets exactly 15 k units.  Every XCD walks a contiguous
//     share of each height class in (sample, column group, m-band, column) order, so the W_s n-panels and the x
//     m-bands its 32 CUs re-read stay in its private 4 MiB L2 from one round to the next.
// Requirements: K % 64 == 0, 16-byte aligned operands; M and N are arbitrary (edge rows are clamped on load and
// masked on store).  Everything else goes to the generic kernel in bf_gemm.hip.
// Since round 3 the forward with 16-bit outputs and the NN input-gradient form run bf_gemm256_r5.hip (the same tile, waves,
// schedule and epilogue with the operands streamed through a five-slot LDS ring, K >= 128); this file keeps the
// fp32-output forward, K = 64, operands past 2^30 elements, and the TN weight-gradient form with its unit ring.
#include "bf_gemm256_dev.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// The kernel: persistent ping-pong over a host-built tile schedule.
// The two waves that share a SIMD belong to different wave groups (G0 = waves 0-3 = even 16-row blocks of the tile,
// G1 = waves 4-7 = odd blocks) and run the same slot sequence one slot apart:
//
//      slot:   4t        4t+1      4t+2      4t+3      4t+4
//      G0:     L0(t)     M0(t)     L1(t)     M1(t)     L0(t+1) ...
//      G1:     M1(t-1)   L0(t)     M0(t)     L1(t)     M1(t)   ...
//
// L = 4 + h ds_read_b128 (the fragments of one 32-deep half of the k-tile) + lgkmcnt(0); M = 4 h MFMAs on registers.
// Every slot ends in one workgroup barrier, so a SIMD always has one wave on the matrix pipe while its partner is
// on the LDS pipe.  The LDS DMA of k-step t+1 is issued by each wave at the start of its own L0(t) and is only
// waited for at the last barrier before slot 4(t+1), i.e. it has 3-4 slots (>= 1500 cycles) to land.
//   * the LDS DMA issued in the LAST k-step of a tile fetches k-step 0 of the workgroup's NEXT tile into the buffer
//     that would otherwise idle, and is retired by the k-loop's existing waits — the next tile starts without a
//     cold-start load;
//   * the epilogue is wave-private (epilogue_wave): no barrier between a tile's last k-step and the next tile's
//     first slot barrier; the next tile's first DMA (into the buffer whose slices were epilogue scratch) waits for
//     that barrier (`defer` in kstep).
// Schedule entry (int4): x = (layer, sample) pair index into w / bias / y, y = sample index into x,
// z = n-tile | height << 24 (height in 32-row units; 0 = no tile), w = first row.
// TRX / TRW = the operand is contraction-major.  Both: the TN form used by the weight-gradient GEMM of the backward pass,
// dW[n][k] = sum_m dy[m][n] x[m][k]: both operands are CONTRACTION-major in memory — p.x is [batch][K][M] (dy: rows = contraction index m, M = output rows n),
// p.w is [batch][K][N] (x) — so no transposed copies of dy and x are ever made.  A stage then holds two [64][256]
// tiles (64 contraction rows of 512 B); their 32-byte granules are XOR-swizzled by the row (again on the DMA source
// address) and the MFMA fragments come out through the LDS transpose read ds_read_b64_tr_b16: two reads give a lane
// the 8 contraction values 8 lg + 0..7 of its row, the same ones a ds_read_b128 of a K-contiguous operand delivers, so
// the two operand forms mix:
//   TRX TRW
//    0   0   NT   y = x W^T          (forward; x [M][K], W [N][K])
//    1   1   TN   dW = dy^T x        (weight gradient; dy [m][N], x [m][K], contraction over the batch rows m)
//    0   1   NN   dx = dy W          (input gradient; dy [M][N], W [N][K] read as it was sampled: no transposed copy)
//
// RING (TN form only, >= 2 k-steps): the DMA of a k-step is not issued in one burst of 8 pieces per wave at L0 but as
// four UNITS of [32 contraction rows][256] (16 KiB: X0, W0 = the halves read in L0, X1, W1 = the halves read in L1),
// one unit per wave group per L slot, each into the half-buffer whose last read is one barrier behind:
//      G0:  L0(t): X1(t+1)    L1(t): X0(t+2)          G1:  L0(t): W1(t+1)    L1(t): W0(t+2)
// so a wave has at most 12 pieces in flight and never more than 4 are issued into one slot; the waits are counted
// (vmcnt(8) = "everything but the two youngest units"): G0 at the end of its M slots, G1 at the end of its L slots.
// The units of the next tile's first two k-steps are issued by the last two k-steps of a tile; the epilogue scratch
// is a separate 32 KiB region, so nothing of the next tile has to wait for the epilogue.
// Measured (dW GEMMs of the BERT-base step, one box): 940-958 -> 1067-1117 TFLOP/s.  A row-major unit ring was 3-7 %
// slower than the burst form at every K and is gone (LABBOOK.md section 4.2).
template <typename T, typename YT, bool TRX = false, bool TRW = false, bool SEG = false, bool RING = false>
__global__ __launch_bounds__(512, 2) void gemm256_sched_kernel(const GemmParams p) {
    static_assert(!RING || (TRX && TRW && !SEG), "the unit ring: TN form only");
    using frag = typename Mfma16<T>::frag;

    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_BYTES + (RING ? 32768 : 0)];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 2, wn = wid & 3;
    const int M = p.M, N = p.N, K = p.K;

    // One tile's DMA sources: wave-uniform sample bases (SGPRs) + eight 32-bit per-lane element offsets.
    struct Src {
        const T* xb;
        const T* wb;
        const T* ob;  // RING: the base of the operand this wave's group fetches (x: group 0, w: group 1)
        unsigned xo[XPIECES], wo[4];
    };
    auto tile_setup = [&](const int4 d, Src& t, int& s, int& m0, int& n0, int& h) {
        // the lane's place in a DMA piece, recomputed per tile from an opaque copy of the lane id: as kernel-lifetime
        // values the two would sit in VGPRs through every k-loop (the fp32-output instantiations spilled two registers)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int prow = ln >> 3;
        const int kc8 = ((ln & 7) ^ ((((wid & 1) << 2) + (ln >> 4)) & 7)) * 8;
        // the entry is the same for every lane: say so, so that everything derived from it lives in SGPRs
        s = __builtin_amdgcn_readfirstlane(d.x);
        const int z = __builtin_amdgcn_readfirstlane(d.z);
        h = z >> 24;
        m0 = __builtin_amdgcn_readfirstlane(d.w);
        n0 = (z & 0xFFFFFF) * TN;
        const T* xb = reinterpret_cast<const T*>(p.x) + (long long)__builtin_amdgcn_readfirstlane(d.y) * p.x_sstride;
        const T* wb = reinterpret_cast<const T*>(p.w) + (long long)s * N * K;
        t.xb = xb;
        t.wb = wb;
        t.ob = wm == 0 ? xb : wb;
        if constexpr (RING) {
            // Group 0 only ever fetches x units, group 1 w units: each wave keeps its own operand's offsets in xo[].
            // A unit = 16 pieces of 2 rows; wave wn of the group fetches pieces i * 4 + wn = rows i * 8 + rb (+ lane >> 5
            // inside rb).  key(row) = (rb & 3) | (i & 1) << 2: xo[] is indexed by the piece number i.
            auto offsets = [&](int rows, int c0) {
                const int rb = wn * 2 + (lane >> 5);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = (lane & 31) ^ (((rb & 3) | ((e & 1) << 2)) << 1);
                    t.xo[e] = (unsigned)rb * (unsigned)rows + (unsigned)min(c0 + c * 8, rows - 8);
                }
            };
            if (wm == 0) offsets(M, m0);
            else offsets(N, n0);
            return;
        }
        // contraction-major operand: piece q = i * 8 + wid = contraction rows 2 q, 2 q + 1 of the k-step; lane -> (row,
        // 16-byte position); the position holds source chunk c = position ^ (key(row) << 1), key = row bits {0, 1, 3};
        // columns past the edge are clamped (they only feed output rows / columns that are masked on store).  The key
        // does not depend on i, so one offset per operand serves all four pieces (piece i = + 16 i rows, added to the
        // wave-uniform base)
        const int tr_r = wid * 2 + (lane >> 5);
        const int tr_c = (lane & 31) ^ (((tr_r & 3) | ((tr_r >> 1) & 4)) << 1);
        if constexpr (TRX) {
            t.xo[0] = (unsigned)tr_r * (unsigned)M + (unsigned)min(m0 + tr_c * 8, M - 8);
        } else {
#pragma unroll
            for (int i = 0; i < XPIECES; ++i)
                t.xo[i] = (unsigned)min(m0 + (i * 8 + wid) * 8 + prow, M - 1) * (unsigned)K + kc8;
        }
        if constexpr (TRW) {
            t.wo[0] = (unsigned)tr_r * (unsigned)N + (unsigned)min(n0 + tr_c * 8, N - 8);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                t.wo[i] = (unsigned)min(n0 + (i * 8 + wid) * 8 + prow, N - 1) * (unsigned)K + kc8;
        }
    };
    // piece q = i * 8 + wid covers rows 8 q .. 8 q + 7 of the stage; only the 4 h pieces of a tile's rows are fetched
    // (inside a tile's k-loop h is the compile-time height, so a full-height tile issues its pieces without branches)
    auto stage = [&](const Src& t, int kt, int buf, auto h) {
        char* base = smem + buf * STAGE_BYTES;
        const T* xk = t.xb;
        const T* wk = t.wb;
        if constexpr (SEG) {
            // segmented contraction (NN form): k-step kt lies in segment kt / (K / TK), all wave-uniform arithmetic
            const int nks = K / TK;
            const int seg = (kt >= nks ? 1 : 0) + (kt >= 2 * nks ? 1 : 0) + (kt >= 3 * nks ? 1 : 0);
            kt -= seg * nks;
            xk += (long long)seg * p.x_seg_stride;
            wk += (long long)seg * p.w_seg_stride;
        }
        xk += TRX ? (long long)kt * TK * M : (long long)kt * TK;
        wk += TRW ? (long long)kt * TK * N : (long long)kt * TK;
        if constexpr (TRX) {
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16(xk + (long long)i * 16 * M + t.xo[0], base + (i * 8 + wid) * 1024);
        } else {
#pragma unroll
            for (int i = 0; i < XPIECES; ++i)
                if (i * 8 + 7 < 4 * h || i * 8 + wid < 4 * h) glds16(xk + t.xo[i], base + (i * 8 + wid) * 1024);
        }
        if constexpr (TRW) {
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16(wk + (long long)i * 16 * N + t.wo[0], base + X_BYTES + (i * 8 + wid) * 1024);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16(wk + t.wo[i], base + X_BYTES + (i * 8 + wid) * 1024);
        }
    };

    // RING: this wave's four pieces of its group's unit `half` (0 / 1) of k-step kt of tile t, into buffer buf, through a
    // buffer descriptor over the sample's operand — 32-bit per-lane byte offset + a scalar row offset, no 64-bit vector
    // address arithmetic per piece (what the forward ring kernel gained 3-5 % from at K = 768, bf_gemm256_r5.hip).  A
    // sample's operand is < 2^31 bytes (host check).
    auto issue_unit = [&](const Src& t, int kt, int buf, int half) {
        char* dst = smem + buf * STAGE_BYTES + (wm == 0 ? 0 : X_BYTES) + half * 16384 + wn * 1024;
        auto go = [&](long long ld) {
            const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(t.ob), 0, 0x7FFFFFFF, 0x00020000);
            const int row0 = kt * TK + half * 32;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)(dst + i * 4096), 16, (int)(t.xo[i] * 2u),
                                                         (int)((row0 + i * 8) * ld) * 2, 0, 0);
        };
        if (wm == 0) go(M);
        else go(N);
    };
    // RING waits (wave-uniform): all but this wave's two / one / no most recent units (of 4 pieces) have landed
    auto wait_units = [&](bool two, bool one) {
        if (two) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (one) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };

    const int fsw = (lane >> 1) & 7;
    const int foff0 = (lane & 15) * ROW_BYTES + ((((lane >> 4)) ^ fsw) << 4);
    const int foff1 = (lane & 15) * ROW_BYTES + (((4 + (lane >> 4)) ^ fsw) << 4);
    const int xfrag_base = wm * 16 * ROW_BYTES;  // + j * 32 rows: wave group wm owns blocks wm, wm + 2, ...
    const int wfrag_base = X_BYTES + wn * 64 * ROW_BYTES;
    // contraction-major tiles: the 16 lanes of a group point at a [4 contraction rows][16 columns] block: lane -> row
    // 8 lg + (li >> 2) of the 32-row half (the second read takes the 4 rows below: + 2 KiB, same key), 8 bytes (li & 3)
    // of the block's 32-byte granule; granule' = granule ^ key(row)
    const int tr_rl = ((lane & 15) >> 2) | (((lane >> 4) & 1) << 2);
    const int tr_lane = ((lane >> 4) * 8 + ((lane & 15) >> 2)) * 512 + (lane & 3) * 8;
    // LDS byte addresses of the wave's first w block (wn * 4) and first x block (wm) in buffer 0; the other blocks are
    // one XOR with a constant away (smem is 1 KiB aligned, the granule index sits alone in address bits 5..8), so the
    // k-loop holds two address registers instead of twelve
    // The reads are inline asm: after an LDS DMA hipcc waits vmcnt(0) before any LDS load it can see through the
    // builtin, which would expose the whole DMA latency in every k-step; the k-loop's own s_waitcnt lgkmcnt(0) /
    // vmcnt(0) statements order these reads against the DMA and the MFMAs.
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned tr_w0 = lds0 + X_BYTES + tr_lane + (((wn * 4) ^ tr_rl) << 5);
    const unsigned tr_x0 = lds0 + tr_lane + ((wm ^ tr_rl) << 5);

    const int nk = SEG ? p.segs * (K / TK) : K / TK;
    const int4* __restrict__ sched = p.sched + blockIdx.x;
    const unsigned G = gridDim.x;
    int4 d = sched[0];
    if ((d.z >> 24) == 0) return;
    Src cur;
    int s, m0, n0, h;
    tile_setup(d, cur, s, m0, n0, h);
    int g = 0;  // running k-step counter: step g lives in LDS buffer g & 1
    if constexpr (RING) {
        issue_unit(cur, 0, 0, 0);
        issue_unit(cur, 0, 0, 1);
        issue_unit(cur, 1, 1, 0);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
        stage(cur, 0, 0, h);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();

    int round = 0;
    for (;;) {
        int4 dn = {0, 0, 0, 0};
        if (round + 1 < p.sched_rounds) dn = sched[(unsigned)(round + 1) * G];
        const bool has_next = (dn.z >> 24) != 0;

        auto body = [&](auto hc) {
            constexpr int H = decltype(hc)::value;
            f32x4_t acc[4][H];
            frag wf[4], xf[H];
            // the four slots of one k-step; `dma()` issues this step's LDS DMA at the top of L0
            // `defer`: the first k-step of a tile that follows another one.  There is no barrier between the tiles: the
            // DMA of this step lands in the buffer whose slices the waves used as epilogue scratch, so group 0 issues
            // it only after the step's first barrier (every wave of both groups reaches that barrier — group 1 as
            // its start-of-tile barrier — after its epilogue); group 1's own issue point already lies behind it.
            auto kstep = [&](auto&& dma, auto last, bool defer) {
                const char* sb = smem + (g & 1) * STAGE_BYTES;
                if (!(defer && wm == 0)) dma();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (TRW) wf[i] = tr_read<frag>(tr_w0 + (g & 1) * STAGE_BYTES, i, std::integral_constant<int, 0>{});
                    else wf[i] = *reinterpret_cast<const frag*>(sb + wfrag_base + i * 16 * ROW_BYTES + foff0);
                }
#pragma unroll
                for (int j = 0; j < H; ++j) {
                    if constexpr (TRX) xf[j] = tr_read<frag>(tr_x0 + (g & 1) * STAGE_BYTES, 2 * j, std::integral_constant<int, 0>{});
                    else xf[j] = *reinterpret_cast<const frag*>(sb + xfrag_base + j * 32 * ROW_BYTES + foff0);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                if (defer && wm == 0) dma();
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < H; ++j) acc[i][j] = Mfma16<T>::run(wf[i], xf[j], acc[i][j]);
                __builtin_amdgcn_s_setprio(0);
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (TRW) wf[i] = tr_read<frag>(tr_w0 + (g & 1) * STAGE_BYTES, i, std::integral_constant<int, 1>{});
                    else wf[i] = *reinterpret_cast<const frag*>(sb + wfrag_base + i * 16 * ROW_BYTES + foff1);
                }
#pragma unroll
                for (int j = 0; j < H; ++j) {
                    if constexpr (TRX) xf[j] = tr_read<frag>(tr_x0 + (g & 1) * STAGE_BYTES, 2 * j, std::integral_constant<int, 1>{});
                    else xf[j] = *reinterpret_cast<const frag*>(sb + xfrag_base + j * 32 * ROW_BYTES + foff1);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (wm == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < H; ++j) acc[i][j] = Mfma16<T>::run(wf[i], xf[j], acc[i][j]);
                __builtin_amdgcn_s_setprio(0);
                if (wm == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                // (with the wave-private epilogue group 1 does not meet group 0 again before the tile-end barrier: its
                // last slot ends without one, which also keeps the two groups' barrier counts equal)
                if (!(decltype(last)::value && wm == 1)) __builtin_amdgcn_s_barrier();
                ++g;
            };

            // the RING k-step: same slots and barriers; one unit issued per L slot, counted waits (wait_units).
            // `steady`: kt + 2 < nk — every unit issued is this tile's own, no conditions in the loop body
            auto read_frags = [&](unsigned sboff, auto half) {
                static_for<0, 4>([&](auto ic) { wf[decltype(ic)::value] = tr_read<frag>(tr_w0 + sboff, decltype(ic)::value, half); });
                static_for<0, H>([&](auto jc) { xf[decltype(jc)::value] = tr_read<frag>(tr_x0 + sboff, 2 * decltype(jc)::value, half); });
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            };
            Src nxt = cur;  // the next tile's sources, set up before the last two k-steps
            auto kstep_ring = [&](int kt, auto last, auto steady) {
                constexpr bool ST = decltype(steady)::value;
                const bool e1 = ST || kt + 1 < nk || has_next, e2 = ST || kt + 2 < nk || has_next;
                const unsigned sboff = (g & 1) * STAGE_BYTES;
                if (e1) {
                    if (ST || kt + 1 < nk) issue_unit(cur, kt + 1, (g & 1) ^ 1, 1);
                    else issue_unit(nxt, 0, (g & 1) ^ 1, 1);
                }
                read_frags(sboff, std::integral_constant<int, 0>{});
                if (wm == 1) wait_units(e1, false);  // W1(kt)
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < H; ++j) acc[i][j] = Mfma16<T>::run(wf[i], xf[j], acc[i][j]);
                __builtin_amdgcn_s_setprio(0);
                if (wm == 0) wait_units(e1, false);  // X1(kt)
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                if (e2) {
                    if (ST || kt + 2 < nk) issue_unit(cur, kt + 2, g & 1, 0);
                    else issue_unit(nxt, kt + 2 - nk, g & 1, 0);
                }
                read_frags(sboff, std::integral_constant<int, 1>{});
                if (wm == 1) wait_units(e2, e1);  // W0(kt + 1)
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < H; ++j) acc[i][j] = Mfma16<T>::run(wf[i], xf[j], acc[i][j]);
                __builtin_amdgcn_s_setprio(0);
                if (wm == 0) wait_units(e2, e1);  // X0(kt + 1)
                __builtin_amdgcn_sched_barrier(0);
                if (!(decltype(last)::value && wm == 1)) __builtin_amdgcn_s_barrier();
                ++g;
            };

            if (wm == 1) __builtin_amdgcn_s_barrier();  // G1 runs one slot behind G0
            init_acc<H>(acc, p.bias ? p.bias + (long long)s * N : nullptr, n0, N, wn, lane);

            if constexpr (RING) {
                for (int kt = 0; kt + 2 < nk; ++kt) kstep_ring(kt, std::false_type{}, std::true_type{});
                if (has_next) {
                    int s2, m2, n2, h2;
                    tile_setup(dn, nxt, s2, m2, n2, h2);
                }
                kstep_ring(nk - 2, std::false_type{}, std::false_type{});
                kstep_ring(nk - 1, std::true_type{}, std::false_type{});
            } else {
            for (int kt = 0; kt + 1 < nk; ++kt)
                kstep([&] { stage(cur, kt + 1, (g & 1) ^ 1, hc); }, std::false_type{}, round > 0 && kt == 0);
            // last k-step: its DMA slot fetches k-step 0 of this workgroup's next tile
            kstep([&] {
                if (has_next) {
                    Src nxt;
                    int s2, m2, n2, h2;
                    tile_setup(dn, nxt, s2, m2, n2, h2);
                    stage(nxt, 0, (g & 1) ^ 1, h2);
                }
            }, std::true_type{}, round > 0 && nk == 1);
            }
            // the last consumed buffer is (g-1)&1; buffer g&1 already holds k-step 0 of the next tile.  Group 0 is one
            // slot ahead here and stays ahead through its epilogue
            YT* y = reinterpret_cast<YT*>(p.y) + (long long)s * M * N;
            const int m_end = min(M, m0 + h * UNIT);
            YT* y2 = p.y2 ? reinterpret_cast<YT*>(p.y2) + (long long)s * M * N : nullptr;
            // every fragment read of buffer (g - 1) & 1 is complete: group 0 passed its last barrier together with the
            // end of group 1's last LDS slot, group 1 comes from its last MFMA slot
            if constexpr (RING)
                epilogue_wave<YT, H, sizeof(YT) == 2 ? 2 : 1>(smem + 2 * STAGE_BYTES + wid * 4096, acc, y, y2, m0, m_end, n0, N, wm, wn, lane,
                                        p.act);
            else
                epilogue_wave<YT, H>(smem + ((g - 1) & 1) * STAGE_BYTES + wid * 8192, acc, y, y2, m0, m_end, n0, N, wm,
                                     wn, lane, p.act);
        };
        switch (h) {
            case 8: body(std::integral_constant<int, 8>{}); break;
            case 7: body(std::integral_constant<int, 7>{}); break;
            case 6: body(std::integral_constant<int, 6>{}); break;
            case 5: body(std::integral_constant<int, 5>{}); break;
            default: body(std::integral_constant<int, 4>{}); break;  // h <= 4: rows past 32 h are masked on store
        }
        if (!has_next) break;
        d = dn;
        ++round;
        tile_setup(d, cur, s, m0, n0, h);
        // (no barrier between tiles: see `defer` in kstep)
    }
}

template <typename T>
int launch256_tn(const GemmParams& p, hipStream_t stream, int grid) {
    // the unit ring needs two k-steps to wrap around (the contraction here is over the S * B * L batch rows: always)
    if (p.K >= 2 * TK)
        hipLaunchKernelGGL((gemm256_sched_kernel<T, float, true, true, false, true>), dim3(grid), dim3(512), 0, stream, p);
    else
        hipLaunchKernelGGL((gemm256_sched_kernel<T, float, true, true>), dim3(grid), dim3(512), 0, stream, p);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int launch256_nn(const GemmParams& p, hipStream_t stream, int grid) {
    // (the unit ring of the TN form was measured slower than the burst form for row-major operands: LABBOOK.md section 4.2)
    if (p.segs > 1) hipLaunchKernelGGL((gemm256_sched_kernel<T, T, false, true, true>), dim3(grid), dim3(512), 0, stream, p);
    else hipLaunchKernelGGL((gemm256_sched_kernel<T, T, false, true>), dim3(grid), dim3(512), 0, stream, p);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int launch256(const GemmParams& p, int y_dtype, hipStream_t stream, int grid) {
    if (y_dtype == BF_DT_F32)
        hipLaunchKernelGGL((gemm256_sched_kernel<T, float>), dim3(grid), dim3(512), 0, stream, p);
    else
        hipLaunchKernelGGL((gemm256_sched_kernel<T, T>), dim3(grid), dim3(512), 0, stream, p);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

bool bf_gemm256_supported(int x_dtype, int w_dtype, int y_dtype, int S, int M, int N, int K, const void* d_x,
                          const void* d_w, int64_t x_sample_stride) {
    if (w_dtype != BF_DT_BF16 && w_dtype != BF_DT_F16) return false;
    if (x_dtype != w_dtype) return false;
    if (y_dtype != w_dtype && y_dtype != BF_DT_F32) return false;
    if (K % TK != 0 || K < TK) return false;
    if (N % 4 != 0) return false;  // 16-byte bias rows / output chunks
    if (((uintptr_t)d_x | (uintptr_t)d_w) & 15) return false;
    if (((size_t)x_sample_stride * 2) % 16 != 0) return false;
    if ((long long)M * K >= (1ll << 32) || (long long)N * K >= (1ll << 32) || (long long)M * N >= (1ll << 31)) return false;
    if (M >= (1 << 24) || (N + TN - 1) / TN >= (1 << 24)) return false;  // schedule entry packing
    const long long tiles = (long long)((M + UNIT * HMIN - 1) / (UNIT * HMIN)) * ((N + TN - 1) / TN) * S;  // S counts (layer, sample) pairs
    if (tiles > 0x3FFFFFll) return false;  // the host-built schedule stays small
    return true;
}

int bf_launch_gemm256(const GemmParams& p0, int w_dtype, int y_dtype, hipStream_t stream) {
    GemmParams p = p0;
    const int grid = gemm256_plan(p, stream);
    if (!grid) return 1;
    // forward form: the five-slot ring (bf_gemm256_r5.hip) where it applies, the burst kernel for the other shapes
    if (bf_gemm256_r5_supported(p, w_dtype, y_dtype)) return bf_launch_gemm256_r5(p, w_dtype, stream, grid);
    if (w_dtype == BF_DT_BF16) return launch256<__bf16>(p, y_dtype, stream, grid);
    return launch256<_Float16>(p, y_dtype, stream, grid);
}

// out[b][n][k] = sum_m a[b][m][n] * bmat[b][m][k]  (fp32 out): the weight-gradient GEMM dW = dy^T x of the backward pass
// without transposed copies of its operands (kernel form TR).  a: [batch][Mc][Nl], bmat: [batch][Mc][Kl], 16-bit.
bool bf_gemm256_tn_supported(int dtype, int batch, int Mc, int Nl, int Kl, const void* d_a, const void* d_b,
                             const void* d_out) {
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) return false;
    if (batch < 1 || batch > 65535 || Mc < TK || Mc % TK || Nl < 8 || Nl % 8 || Kl < 8 || Kl % 8) return false;
    if (((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_out) & 15) return false;
    // (a sample's operand is addressed by 32-bit byte offsets through a buffer descriptor: < 2^30 elements)
    if ((long long)Mc * Nl >= (1ll << 30) || (long long)Mc * Kl >= (1ll << 30) || (long long)Nl * Kl >= (1ll << 31)) return false;
    if (Nl >= (1 << 24) || (Kl + TN - 1) / TN >= (1 << 24)) return false;
    return true;
}

int bf_launch_gemm256_tn(const void* d_a, const void* d_b, float* d_out, int dtype, int batch, int Mc, int Nl, int Kl,
                         hipStream_t stream) {
    GemmParams p{};
    p.x = d_a;
    p.w = d_b;
    p.bias = nullptr;
    p.y = d_out;
    p.x_sstride = (long long)Mc * Nl;
    p.S = batch;
    p.M = Nl;
    p.N = Kl;
    p.K = Mc;
    p.act = BF_ACT_NONE;
    const int grid = gemm256_plan(p, stream);
    if (!grid) return 1;
    // the two-buffer unit ring of this file: the TN form on the five-slot ring measured bit-identical and 0-1.4 % per
    // launch in round 6, nothing in the training step
    if (dtype == BF_DT_BF16) return launch256_tn<__bf16>(p, stream, grid);
    return launch256_tn<_Float16>(p, stream, grid);
}

// y[s][m][k] = sum_n x[s][m][n] * w[s][n][k]  (16-bit in and out): the input-gradient GEMM dx = dy W of the backward pass
// with W_s [Nl][Kl] read as the sampling kernel wrote it (kernel form NN).  x: [S][M][Nl], w: [S][Nl][Kl], y: [S][M][Kl].
bool bf_gemm256_nn_supported(int dtype, int S, int M, int Nl, int Kl, const void* d_x, const void* d_w, const void* d_y) {
    if (dtype != BF_DT_BF16 && dtype != BF_DT_F16) return false;
    if (S < 1 || S > 65535 || M < 1 || Nl < TK || Nl % TK || Kl < 8 || Kl % 8) return false;
    if (((uintptr_t)d_x | (uintptr_t)d_w | (uintptr_t)d_y) & 15) return false;
    if ((long long)M * Nl >= (1ll << 32) || (long long)Nl * Kl >= (1ll << 32) || (long long)M * Kl >= (1ll << 31)) return false;
    if (M >= (1 << 24) || (Kl + TN - 1) / TN >= (1 << 24)) return false;
    return (long long)M * Kl >= 128 * 128;
}

static bool nn_actgrad_supported(int dtype, int S, int M, int Nl, int Kl, const void* d_x, const void* d_w, const void* d_y,
                                 const void* d_gpre) {
    if (!bf_gemm256_nn_supported(dtype, S, M, Nl, Kl, d_x, d_w, d_y) || !d_gpre || ((uintptr_t)d_gpre & 15)) return false;
    GemmParams p{};
    p.M = M, p.N = Kl, p.K = Nl;
    return bf_gemm256_r5_supported(p, dtype, dtype);  // the fused derivative lives in the ring kernel's epilogue only
}

int bf_launch_gemm256_nn(const void* d_x, const void* d_w, void* d_y, int dtype, int S, int M, int Nl, int Kl,
                         hipStream_t stream, int segs, const void* d_gpre, int act) {
    if (segs < 1 || segs > 4) BF_FAIL("bf_gemm_nn: 1 to 4 layers (got %d)", segs);
    if (d_gpre && (segs != 1 || act != BF_ACT_GELU || !nn_actgrad_supported(dtype, S, M, Nl, Kl, d_x, d_w, d_y, d_gpre)))
        BF_FAIL("bf_gemm_nn_actgrad: needs the ring form of the NN GEMM (16-bit, K %% 8 == 0, contraction >= 128), the GELU and one layer");
    GemmParams p{};
    p.x = d_x;
    p.w = d_w;
    p.bias = nullptr;
    p.y = d_y;
    p.y2 = nullptr;
    p.gpre = d_gpre;
    p.x_sstride = (long long)M * Nl;
    p.S = S;
    p.M = M;
    p.N = Kl;
    p.K = Nl;
    p.segs = segs;
    p.x_seg_stride = (long long)S * M * Nl;
    p.w_seg_stride = (long long)S * Nl * Kl;
    p.act = BF_ACT_NONE;
    const int grid = gemm256_plan(p, stream);
    if (!grid) return 1;
    // the five-slot ring (bf_gemm256_r5.hip) where it applies, the burst kernel for the other shapes
    if (bf_gemm256_r5_supported(p, dtype, dtype)) return bf_launch_gemm256_r5_nn(p, dtype, stream, grid);
    if (dtype == BF_DT_BF16) return launch256_nn<__bf16>(p, stream, grid);
    return launch256_nn<_Float16>(p, stream, grid);
}

int bf_gemm_tn(const void* d_a, const void* d_bm, float* d_out, int dtype, int batch, int Mc, int N, int K, void* stream) {
    if (!d_a || !d_bm || !d_out) BF_FAIL("bf_gemm_tn: null pointer");
    if (!bf_gemm256_tn_supported(dtype, batch, Mc, N, K, d_a, d_bm, d_out))
        BF_FAIL("bf_gemm_tn: needs a 16-bit dtype, Mc %% 64 == 0, N %% 8 == 0, K %% 8 == 0 and 16-byte aligned pointers");
    return bf_launch_gemm256_tn(d_a, d_bm, d_out, dtype, batch, Mc, N, K, (hipStream_t)stream);
}

int bf_gemm_nn(const void* d_x, const void* d_w, void* d_y, int dtype, int S, int M, int N, int K, void* stream) {
    if (!d_x || !d_w || !d_y) BF_FAIL("bf_gemm_nn: null pointer");
    if (!bf_gemm256_nn_supported(dtype, S, M, N, K, d_x, d_w, d_y))
        BF_FAIL("bf_gemm_nn: needs a 16-bit dtype, N %% 64 == 0, K %% 8 == 0, M * K >= 16384 and 16-byte aligned pointers");
    return bf_launch_gemm256_nn(d_x, d_w, d_y, dtype, S, M, N, K, (hipStream_t)stream);
}

int bf_gemm_nn_actgrad_supported(const void* d_x, const void* d_w, const void* d_y, const void* d_pre, int dtype, int S, int M,
                                 int N, int K) {
    return nn_actgrad_supported(dtype, S, M, N, K, d_x, d_w, d_y, d_pre) ? 1 : 0;
}

int bf_gemm_nn_actgrad(const void* d_x, const void* d_w, void* d_y, const void* d_pre, int dtype, int S, int M, int N, int K,
                       int act, void* stream) {
    if (!d_x || !d_w || !d_y || !d_pre) BF_FAIL("bf_gemm_nn_actgrad: null pointer");
    if (act != BF_ACT_GELU) BF_FAIL("bf_gemm_nn_actgrad: unknown activation %d", act);
    return bf_launch_gemm256_nn(d_x, d_w, d_y, dtype, S, M, N, K, (hipStream_t)stream, 1, d_pre, act);
}

int bf_gemm_nn_layers(const void* d_x, const void* d_w, void* d_y, int dtype, int L, int S, int M, int N, int K,
                      void* stream) {
    if (!d_x || !d_w || !d_y) BF_FAIL("bf_gemm_nn_layers: null pointer");
    if (L < 1 || L > 4) BF_FAIL("bf_gemm_nn_layers: L must be 1..4 (got %d)", L);
    if (!bf_gemm256_nn_supported(dtype, S, M, N, K, d_x, d_w, d_y) || (long long)L * S * M * N >= (1ll << 40))
        BF_FAIL("bf_gemm_nn_layers: needs a 16-bit dtype, N %% 64 == 0, K %% 8 == 0, M * K >= 16384 and 16-byte aligned pointers");
    return bf_launch_gemm256_nn(d_x, d_w, d_y, dtype, S, M, N, K, (hipStream_t)stream, L);
}
