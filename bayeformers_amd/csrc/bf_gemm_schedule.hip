// bf_gemm_schedule.hip — the host side of the 256-wide sampled-weight GEMM: WHICH tiles each persistent workgroup of
// bf_gemm256.hip / bf_gemm256_r5.hip runs.  Host code only (the HIP runtime is needed for the table upload): the builder
// (build_schedule), its fabric-fetch model (schedule_fetch_rows), the per-device cache of uploaded tables (get_schedule),
// and the C-ABI entries bf_gemm_prepare / bf_gemm_schedule*.  The launchers reach the cache through gemm256_plan
// (bf_gemm256_dev.h).
// The tile constants (TN, UNIT, HMIN, HMAX) and the default policy are those of bf_gemm256_dev.h.
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "bf_gemm256_dev.h"

namespace {

struct Tile {
    int pair, xs, tn, m0, h;
    long long key;  // locality order inside a height class
};

// XCD-aware bijective map of a block id to its position in the logical workgroup order (block b runs on XCD b % 8,
// observed; speed only): XCD x owns a contiguous run of logical positions.
unsigned xcd_remap(unsigned b, unsigned nwg) {
    const unsigned xcd = b & 7u, q = nwg >> 3, r = nwg & 7u;
    const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (b >> 3);
}

// Modelled fabric fetch of a schedule, in rows of K elements: every XCD's workgroups (block b runs on XCD b % 8, observed)
// run their j-th tiles together and in k-lockstep, so a panel shared by several of them is fetched into the XCD's L2 once
// per round — and nothing survives to the next round: the k-slices a round touches (a + b panels for a x b tiles, 12 x
// 393 KB at K = 768) exceed the 4 MiB L2 under LRU.  Validated against TCC_EA0_RDREQ on the four BERT-base launches
// (308 / 107 / 386 / 427 MB modelled, 308 / 108 / 384 / 428 MB counted: profiles/r6b_sched_l2_model.md), independent of
// the modelled L2 size between 2 and 4 MiB.  tools/sched_l2_sim.py is the same model with an explicit LRU.
long long schedule_fetch_rows(const std::vector<int4>& table, int rounds, int grid) {
    long long rows = 0;
    std::vector<long long> seen;
    for (int xcd = 0; xcd < 8; ++xcd)
        for (int j = 0; j < rounds; ++j) {
            seen.clear();
            for (int b = xcd; b < grid; b += 8) {
                const int4 d = table[(size_t)j * grid + b];
                const int h = d.z >> 24;
                if (!h) continue;
                seen.push_back(((long long)d.x << 32) | (unsigned)(d.z & 0xFFFFFF) | (1ll << 62));  // W panel (pair, n-tile)
                for (int u = 0; u < h; ++u) seen.push_back(((long long)d.y << 32) | (unsigned)(d.w / UNIT + u));  // x unit
            }
            std::sort(seen.begin(), seen.end());
            seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
            for (long long v : seen) rows += (v >> 62) ? TN : UNIT;
        }
    return rows;
}

// Cut S * layers * tiles_n columns of ceil(M / 32) units into tiles of 1..8 units and deal them to at most n_cu
// workgroups.  Returns the table ([rounds][grid] int4) and the launch grid.
// policy bit 0: workgroups at odd logical positions run their tiles in reverse order (short tiles first), which
// spreads the workgroups' epilogue store bursts over time instead of all of them ending a tile in the same
// microsecond.
// policy bit 12 (round 6): the columns that get one tile more than the others (the Bresenham remainder of the target tile
// count) are the FIRST columns instead of being spread evenly: columns of one sample then share their row cuts, so the
// tiles of a band of x rows that run together on an XCD fetch the same units (modelled fetch of the BERT-base FFN-up
// launch 3.50 -> 2.90 x its operands, BERT-large Q/K/V 4.07 -> 3.33).
// `cg` = columns per group of the locality order (policy bit 3).
void build_schedule_cg(int S, int layers, int tiles_n, int M, int n_cu, int policy, int cg, std::vector<int4>& table,
                       int& rounds, int& grid) {
    const int hmax = ((policy >> 4) & 15) ? std::min(HMAX, std::max(HMIN, (policy >> 4) & 15)) : HMAX;
    const int C = S * layers * tiles_n;
    const int Hc = (M + UNIT - 1) / UNIT;
    const long long U = (long long)C * Hc;
    const int n_min = (Hc + hmax - 1) / hmax;
    const int n_max = std::max(n_min, Hc / HMIN);
    long long T = std::max<long long>(1, (U + (long long)hmax * n_cu - 1) / ((long long)hmax * n_cu));  // tiles per CU
    std::vector<Tile> tiles;
    for (int iter = 0; iter < 4; ++iter) {
        const long long target = T * n_cu;
        tiles.clear();
        for (int c = 0; c < C; ++c) {
            // spread of the target tile count over the columns: Bresenham, or (bit 12) the remainder on the first columns
            long long n = (target * (c + 1)) / C - (target * c) / C;
            if (policy & 0x1000) n = target / C + (c < target % C ? 1 : 0);
            n = std::min<long long>(std::max<long long>(n, n_min), n_max);
            if (policy & 2) n = n_min;  // fixed full-height tiles (the round-1 decomposition)
            const int q = Hc / (int)n, r = Hc % (int)n;
            const int xs = c / (tiles_n * layers), cn = c % (tiles_n * layers);
            const int layer = cn / tiles_n, tn = cn % tiles_n;
            int u = 0;
            for (int i = 0; i < (int)n; ++i) {
                const int hh = q + (i < r ? 1 : 0);
                Tile t;
                t.pair = layer * S + xs;
                t.xs = xs;
                t.tn = tn;
                t.m0 = u * UNIT;
                t.h = hh;
                // (sample, band of 1024 rows, column, row): the 32 concurrent tiles of an XCD share few panels
                t.key = (((long long)xs * 4096 + t.m0 / 1024) * 4096 + cn) * 65536 + (t.m0 / UNIT);
                // policy bit 3: (sample, group of cg columns, 256-row band, column) — an XCD that walks this order keeps
                // cg W panels in its L2 while the x bands stream past them (groups of 3 / 4 / 6 / 9 / 12 columns measured
                // in the BERT-base step on one box, round 3: GEMM 7.13 / 7.10 / 7.20 / 7.29 / 7.22 ms, L2 fills 302 / 307 /
                // 299 / 310 / 318 MB per launch)
                if (policy & 8) t.key = ((((long long)xs * 4096 + cn / cg) * 65536 + t.m0 / 256) * 4096 + cn) * 8 + (t.m0 / UNIT) % 8;
                tiles.push_back(t);
                u += hh;
            }
        }
        if ((long long)tiles.size() <= target) break;
        T = ((long long)tiles.size() + n_cu - 1) / n_cu;  // the height cap forced more tiles than T rounds hold
    }
    const int total = (int)tiles.size();
    grid = std::min(total, n_cu);
    std::vector<std::vector<int>> lists(grid);  // per logical workgroup: indices into `tiles`, in running order
    // class-by-class dealing: tiles sorted tallest first (locality order inside a height class); round r takes the next
    // `grid` tiles.  Odd rounds are dealt backwards so that a workgroup that drew a tall tile in one round draws a
    // short one in the next — either over all workgroups, or (policy bit 4, the default) only among the 32 workgroups of
    // each XCD, which keeps an XCD on the same range of every height class (measured in the BERT-base step: 7.18 vs
    // 7.25 ms of GEMM time).
    std::stable_sort(tiles.begin(), tiles.end(), [](const Tile& a, const Tile& b) {
        return a.h != b.h ? a.h > b.h : a.key < b.key;
    });
    const bool per_xcd = (policy & 4) && grid % 8 == 0 && total >= grid;
    // (only when every height class fills whole rounds: then a workgroup that takes every 32nd tile of its XCD's list
    // gets the same number of tiles of every class; otherwise the span dealing below, which balances odd classes)
    bool whole_classes = (policy & 8) && grid % 8 == 0 && total >= grid;
    for (int a = 0; a < total && whole_classes;) {
        int b = a;
        while (b < total && tiles[b].h == tiles[a].h) ++b;
        if ((b - a) % grid) whole_classes = false;
        a = b;
    }
    if (whole_classes) {
        // Every XCD takes a CONTIGUOUS share of each height class (shares rotate so that the XCDs' tile counts stay
        // within one of each other) and its 32 workgroups walk that share 32 tiles at a time: consecutive rounds of an
        // XCD are neighbours in the locality order.  A workgroup draws every 32nd tile of its XCD's list, i.e. the same
        // number of tiles of every class: the unit balance of the class-by-class dealing is kept.
        const int span = grid / 8;
        std::vector<std::vector<int>> share(8);
        int carry = 0;
        for (int a = 0; a < total;) {
            int b = a;
            while (b < total && tiles[b].h == tiles[a].h) ++b;
            const int n = b - a;
            int start = a;
            for (int i = 0; i < 8; ++i) {
                const int x = (i + carry) % 8;
                const int cnt = (int)(((long long)n * (i + 1)) / 8 - ((long long)n * i) / 8);
                for (int k = start; k < start + cnt; ++k) share[x].push_back(k);
                start += cnt;
            }
            carry = (carry + n % 8) % 8;
            a = b;
        }
        for (int x = 0; x < 8; ++x)
            for (size_t j = 0; j < share[x].size(); ++j) {
                const int r = (int)(j / span), in = (int)(j % span);
                lists[x * span + ((r & 1) ? span - 1 - in : in)].push_back(share[x][j]);
            }
    } else if (!per_xcd) {
        for (int k = 0; k < total; ++k) {
            const int r = k / grid, pos = k % grid;
            lists[(r & 1) ? grid - 1 - pos : pos].push_back(k);
        }
    } else {
        // round r = tiles [r grid, (r+1) grid) cut into 8 spans of grid/8; XCD x takes span x of every round unless
        // swapping two XCDs' spans of some round evens out their totals (only where a height class ends inside a round)
        const int span = grid / 8, nr = (total + grid - 1) / grid;
        std::vector<std::vector<long long>> sum(nr, std::vector<long long>(8, 0));
        for (int k = 0; k < total; ++k) sum[k / grid][(k % grid) / span] += tiles[k].h;
        std::vector<std::vector<int>> perm(nr, std::vector<int>(8));
        for (int r = 0; r < nr; ++r)
            for (int x = 0; x < 8; ++x) perm[r][x] = x;
        auto tot = [&](int x) {
            long long t = 0;
            for (int r = 0; r < nr; ++r) t += sum[r][perm[r][x]];
            return t;
        };
        for (int it = 0; it < 64; ++it) {
            int hi = 0, lo = 0;
            for (int x = 1; x < 8; ++x) {
                if (tot(x) > tot(hi)) hi = x;
                if (tot(x) < tot(lo)) lo = x;
            }
            const long long th = tot(hi), tl = tot(lo);
            int best_r = -1;
            long long best = th;
            for (int r = 0; r < nr; ++r) {
                const long long d = sum[r][perm[r][hi]] - sum[r][perm[r][lo]];
                const long long m = std::max(th - d, tl + d);
                if (d > 0 && m < best) best = m, best_r = r;
            }
            if (best_r < 0) break;
            std::swap(perm[best_r][hi], perm[best_r][lo]);
        }
        for (int r = 0; r < nr; ++r)
            for (int x = 0; x < 8; ++x)
                for (int in = 0; in < span; ++in) {
                    const int k = r * grid + perm[r][x] * span + in;
                    if (k < total) lists[x * span + ((r & 1) ? span - 1 - in : in)].push_back(k);
                }
    }
    if (policy & 1)
        for (int li = 1; li < grid; li += 2) std::reverse(lists[li].begin(), lists[li].end());
    rounds = 0;
    for (const auto& l : lists) rounds = std::max(rounds, (int)l.size());
    table.assign((size_t)rounds * grid, int4{0, 0, 0, 0});
    for (int b = 0; b < grid; ++b) {
        const std::vector<int>& l = lists[xcd_remap((unsigned)b, (unsigned)grid)];
        for (size_t j = 0; j < l.size(); ++j) {
            const Tile& t = tiles[l[j]];
            table[j * grid + b] = int4{t.pair, t.xs, t.tn | (t.h << 24), t.m0};
        }
    }
}

// policy bits 8-11: columns per group of the locality order (0 = 4).  policy bit 13 (round 6): the group size is CHOSEN per
// shape — among 3, 4, 6, 8 and all columns of a sample — by the modelled fabric fetch of the resulting schedule
// (schedule_fetch_rows); the tiles, their heights and every workgroup's unit count are the same for every candidate.
void build_schedule(int S, int layers, int tiles_n, int M, int n_cu, int policy, std::vector<int4>& table, int& rounds,
                    int& grid) {
    const int cg0 = ((policy >> 8) & 15) ? (policy >> 8) & 15 : 4;
    if (!(policy & 0x2000) || !(policy & 8)) return build_schedule_cg(S, layers, tiles_n, M, n_cu, policy, cg0, table, rounds, grid);
    const int cols = tiles_n * layers;
    long long best = -1;
    for (int cg : {4, 3, 6, 8, cols}) {  // (the first candidate wins a tie: 4 is the round-3 default)
        if (cg > cols && cg != 4) continue;
        std::vector<int4> t;
        int r = 0, g = 0;
        build_schedule_cg(S, layers, tiles_n, M, n_cu, policy, cg, t, r, g);
        const long long f = schedule_fetch_rows(t, r, g);
        if (best < 0 || f < best) best = f, table.swap(t), rounds = r, grid = g;
    }
}

typedef Gemm256Sched Sched;
typedef std::tuple<int, int, int, int, int, int, int> SchedKey;  // device, S, layers, tiles_n, M, n_cu, policy
std::mutex g_sched_mu;
std::map<SchedKey, Sched> g_sched;

// The schedule of a shape is built once per device and kept in device memory for the life of the process (a few KB
// per shape).  The first launch of a shape therefore allocates: it cannot happen inside a stream capture.
int get_schedule(int S, int layers, int tiles_n, int M, int policy, hipStream_t stream, Sched& out) {
    int dev = 0;
    BF_HIP_CHECK(hipGetDevice(&dev));
    static std::map<int, int> cu_of;
    std::lock_guard<std::mutex> lk(g_sched_mu);
    int n_cu = cu_of[dev];
    if (!n_cu) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) n_cu = 256;
        else n_cu = prop.multiProcessorCount / 8 * 8;
        if (n_cu < 8) n_cu = 8;
        cu_of[dev] = n_cu;
    }
    const SchedKey key(dev, S, layers, tiles_n, M, n_cu, policy);
    auto it = g_sched.find(key);
    if (it != g_sched.end()) {
        out = it->second;
        return 0;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        BF_FAIL("bf_gemm_nt: the first launch of a shape (S=%d M=%d) builds its tile schedule and allocates device "
                "memory; call bf_gemm_prepare() for it, or run the step once, before capturing it into a graph", S, M);
    // Tables are NEVER freed or rewritten: a captured HIP graph keeps the raw d_table pointer in its kernel arguments
    // (bf_gemm_prepare / bench --graph), so a table must stay valid for the life of the process.  Variable-length batches
    // make every new M a new shape; a table is a few KB to a few hundred KB, so the cache is bounded by BYTES per device
    // (default 1 GiB, BF_GEMM_SCHED_CACHE_BYTES) and a shape past the bound is refused loudly instead of evicting.
    static std::map<int, size_t> bytes_of;
    static const size_t cap = [] {
        const char* e = getenv("BF_GEMM_SCHED_CACHE_BYTES");
        const long long v = e ? atoll(e) : 0;
        return v > 0 ? (size_t)v : ((size_t)1 << 30);
    }();
    std::vector<int4> table;
    Sched sc;
    build_schedule(S, layers, tiles_n, M, n_cu, policy, table, sc.rounds, sc.grid);
    if (bytes_of[dev] + table.size() * sizeof(int4) > cap)
        BF_FAIL("bf_gemm_nt: the tile schedules of this device already hold %zu bytes (%zu shapes in the process); raise "
                "BF_GEMM_SCHED_CACHE_BYTES (now %zu) or bucket the batch sizes", bytes_of[dev], g_sched.size(), cap);
    bytes_of[dev] += table.size() * sizeof(int4);
    BF_HIP_CHECK(hipMalloc((void**)&sc.d_table, table.size() * sizeof(int4)));
    BF_HIP_CHECK(hipMemcpy(sc.d_table, table.data(), table.size() * sizeof(int4), hipMemcpyHostToDevice));
    g_sched[key] = sc;
    out = sc;
    return 0;
}

}  // namespace

int bf_gemm256_get_schedule(int S, int layers, int tiles_n, int M, int policy, hipStream_t stream, Gemm256Sched& out) {
    return get_schedule(S, layers, tiles_n, M, policy, stream, out);
}

extern "C" int bf_gemm_prepare(int S, int L, int M, int N, void* stream) {
    if (S < 1 || L < 1 || M < 1 || N < 1) BF_FAIL("bf_gemm_prepare: bad shape S=%d L=%d M=%d N=%d", S, L, M, N);
    Sched sc;
    return get_schedule(S, L, (N + TN - 1) / TN, M, BF_SCHED_POLICY, (hipStream_t)stream, sc);
}

extern "C" size_t bf_gemm_schedule(int S, int L, int M, int N, int n_cu, int32_t* out, size_t cap_values, int* rounds,
                                   int* grid) {
    return bf_gemm_schedule_policy(S, L, M, N, n_cu, -1, out, cap_values, rounds, grid);
}

extern "C" int64_t bf_gemm_schedule_fetch_rows(const int32_t* table, int rounds, int grid) {
    if (!table || rounds < 1 || grid < 1) return -1;
    std::vector<int4> t((size_t)rounds * grid);
    for (size_t i = 0; i < t.size(); ++i) t[i] = int4{table[4 * i], table[4 * i + 1], table[4 * i + 2], table[4 * i + 3]};
    return schedule_fetch_rows(t, rounds, grid);
}

extern "C" size_t bf_gemm_schedule_policy(int S, int L, int M, int N, int n_cu, int policy, int32_t* out, size_t cap_values,
                                          int* rounds, int* grid) {
    if (S < 1 || L < 1 || M < 1 || N < 1 || n_cu < 1) return 0;
    std::vector<int4> table;
    int r = 0, g = 0;
    build_schedule(S, L, (N + TN - 1) / TN, M, n_cu, policy < 0 ? BF_SCHED_POLICY : policy, table, r, g);
    if (rounds) *rounds = r;
    if (grid) *grid = g;
    const size_t n = table.size() * 4;
    if (out && cap_values >= n)
        for (size_t i = 0; i < table.size(); ++i) {
            out[4 * i] = table[i].x;
            out[4 * i + 1] = table[i].y;
            out[4 * i + 2] = table[i].z;
            out[4 * i + 3] = table[i].w;
        }
    return n;
}
