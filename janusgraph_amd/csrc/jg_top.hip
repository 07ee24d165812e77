// jg_top.hip — the k highest-ranked vertices of a PageRank session (jg_pagerank_top): a radix select over
// the rank vector the session leaves on the device, so that k records cross to the host instead of two
// n-element arrays ("PageRank top-k on the device").
//
// Order (total): rank descending by numeric value, ties by caller-order index ascending; -0.0 orders as
// +0.0, a NaN orders below every number and ties with other NaNs.  top_key_of maps a rank to a 64-bit
// unsigned key with that order (larger key = earlier); the composite a select works on is (key, inv) with
// inv = inv_max - index (inv_max = n - 1, so a smaller index is a larger inv), 64 + bits(n - 1) bits, every
// composite distinct.  Values are only ordered, never altered: the listed rank is the stored bit pattern.
//
// Per shard, over rank = Shard::pr_rank[rows], dense = Shard::dense_rows[rows], Shard::out_degree[rows]
// (all three only read here), with want = min(k, rows):
//   seed       writes state[0] (nothing determined, want records wanted).
//   histogram  pass p, MSB first: digits of 11, 11, 11, 11, 10, 10 key bits, then up to 3 digits of the inv
//              bits.  One grid-stride read of the rows; a row whose composite matches the prefix in state[p]
//              adds 1 to its digit's bin in the block's LDS histogram (a wave whose matching lanes share
//              one digit adds once); the block then adds its non-zero bins to hist[p].  Reads state[p],
//              adds to hist[p] (zeroed by one memset before the first pass).
//   threshold  pass p, one block: walks hist[p] from the top bin to the one where the running count crosses
//              the records still wanted, and writes state[p + 1]: the prefix extended by that digit, the
//              records wanted from inside that bin, and done when the bin holds exactly that many (the rows
//              at or above the prefix are then the winners and every later pass returns at once; the last
//              pass always ends so, its bins holding one row at most).  Reads hist[p] and state[p].
//   filter     one pass over the rows: a winner has key > the threshold key, or key == it and inv >= the
//              threshold inv.  Winners are stored as (index, row) records at slots reserved with a block
//              scan and one atomic per block; a slot at or past `want` is never stored to.  Reads
//              state[last]; writes rec_key, rec_row, adds to ctr.
//   order      prim::radix_sort of the records on the index bits; the rekey kernel then overwrites rec_key[j]
//              with ~top_key_of(rank[rec_row[j]]) (it reads rec_row and rank only), and a second, stable sort
//              on those 64 bits leaves rank descending, index ascending.  At most kTopSmall records are
//              instead placed by one launch that counts, for each record, the records ordered before it,
//              and emits it there (reads rec_key, rec_row and the shard's arrays; writes the outputs).
//   emit       gathers index, rank and out-degree of each record's row into the shard's output arrays.
// want == rows skips the select: every row is a record.  No kernel reads a value that it or a concurrent
// launch writes (the slot counter's atomic reservation aside): every launch is on the shard's stream, each
// pass reads the state slot and histogram the launches before it completed and writes the next.
// Every buffer is a DevBuf written or cleared before it is read (JG_DEV_POISON).
//
// The shards' records (at most P * k) are merged on the host under the same order and held there
// (Graph::top_*): the list owns its storage, so later steps, sessions and programs do not touch it.
#include <cstring>

#include "jg_internal.h"
#include "jg_prim.h"

namespace jg {
namespace {

constexpr int kTopBins = 2048;                // bins of one digit (11 bits)
constexpr int kTopKeyPasses = 6;              // 11 + 11 + 11 + 11 + 10 + 10 key bits
constexpr int kTopMaxPasses = kTopKeyPasses + 3;
constexpr int kTopSmall = 4096;               // records ordered by counting, all staged in LDS (48 KB)

// rank -> order key: fold the zeros, flip for the monotone integer view, NaN lowest.  (An int64 key would
// flip the sign bit only.)
__host__ __device__ __forceinline__ uint64_t top_key_of(double r) {
    const double v = r + 0.0;  // -0.0 + 0.0 == +0.0
    if (v != v) return 0;      // below -inf's key (0x000f...f)
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// Select state after p passes: the composite's determined high bits (the rest zero), the records still
// wanted from the rows that match them, and bookkeeping for the byte model.
struct TopState {
    unsigned long long key, inv, remaining;
    unsigned long long done;    // 1: the rows at or above (key, inv) are exactly the winners; 2: counts inconsistent
    unsigned long long passes;  // histogram passes that read the rows
    unsigned long long tie;     // rows whose key equals the threshold key (set by the first inv pass)
};

__global__ void top_seed_kernel(TopState* __restrict__ st, unsigned long long want) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *st = TopState{0, 0, want, 0, 0, 0};
}

template <bool kInv>
__global__ __launch_bounds__(kBlock) void top_hist_kernel(const double* __restrict__ rank, const int32_t* __restrict__ dense,
                                                          int64_t rows, const TopState* __restrict__ st,
                                                          uint32_t* __restrict__ hist, int shift, int width,
                                                          uint32_t inv_max) {
    __shared__ uint32_t bins[kTopBins];
    const TopState s = *st;
    if (s.done) return;  // block-uniform
    for (int i = threadIdx.x; i < kTopBins; i += kBlock) bins[i] = 0;
    __syncthreads();
    const int hs = shift + width;  // the bits from hs up are the prefix
    const uint32_t mask = (1u << width) - 1u;
    constexpr int R = 4;  // rows per thread and trip, their loads issued together
    const int64_t span = (int64_t)kBlock * R;
    for (int64_t x0 = (int64_t)blockIdx.x * span; x0 < rows; x0 += (int64_t)gridDim.x * span) {  // block-uniform
        double r[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int64_t l = x0 + (int64_t)k * kBlock + threadIdx.x;
            r[k] = l < rows ? rank[l] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int64_t l = x0 + (int64_t)k * kBlock + threadIdx.x;
            const uint64_t key = top_key_of(r[k]);
            bool m = l < rows;
            uint32_t d;
            if (!kInv) {
                m = m && (hs >= 64 || (key >> hs) == (s.key >> hs));
                d = (uint32_t)(key >> shift) & mask;
            } else {
                m = m && key == s.key;
                uint64_t inv = 0;
                if (m) {
                    inv = (uint64_t)(inv_max - (uint32_t)dense[l]);
                    m = (inv >> hs) == (s.inv >> hs);
                }
                d = (uint32_t)(inv >> shift) & mask;
            }
            const uint64_t act = __ballot(m);
            if (act == 0) continue;  // wave-uniform
            const int lead = __ffsll((unsigned long long)act) - 1;
            const uint32_t first = __shfl(d, lead, kWave);
            if (__ballot(m && d == first) == act) {  // one digit in the wave (a tie class): one add
                if (lane_id() == lead) atomicAdd(&bins[first], (uint32_t)__popcll(act));
            } else if (m) {
                atomicAdd(&bins[d], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTopBins; i += kBlock) {
        const uint32_t c = bins[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// One block.  Thread t holds bins kTopBins - 1 - 8t downwards, so a block scan gives the count above each.
__global__ __launch_bounds__(kBlock) void top_threshold_kernel(const uint32_t* __restrict__ hist,
                                                               const TopState* __restrict__ in, TopState* __restrict__ out,
                                                               int shift, int inv_pass, int first_inv, int last) {
    __shared__ long long scratch[kBlock / kWave];
    const TopState s = *in;
    if (s.done) {  // block-uniform
        if (threadIdx.x == 0) *out = s;
        return;
    }
    constexpr int kPer = kTopBins / kBlock;
    uint32_t c[kPer];
    long long mine = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        c[j] = hist[kTopBins - 1 - ((int)threadIdx.x * kPer + j)];
        mine += c[j];
    }
    long long total;
    long long run = block_exclusive_scan_add(mine, scratch, &total);
    const long long want = (long long)s.remaining;
    if (total < want || want < 1) {  // never, while the counts add up: the host fails the call on done == 2
        if (threadIdx.x == 0) {
            TopState o = s;
            o.done = 2;
            *out = o;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        if (run < want && run + (long long)c[j] >= want) {  // exactly one bin of the block
            const unsigned long long bin = (unsigned long long)(kTopBins - 1 - ((int)threadIdx.x * kPer + j));
            TopState o = s;
            if (inv_pass) o.inv |= bin << shift;
            else o.key |= bin << shift;
            o.remaining = (unsigned long long)(want - run);
            o.done = (run + (long long)c[j] == want || last) ? 1 : 0;
            o.passes = s.passes + 1;
            if (first_inv) o.tie = (unsigned long long)total;
            *out = o;
        }
        run += c[j];
    }
}

__global__ __launch_bounds__(kBlock) void top_filter_kernel(const double* __restrict__ rank, const int32_t* __restrict__ dense,
                                                            int64_t rows, const TopState* __restrict__ fin, uint32_t inv_max,
                                                            int64_t want, unsigned long long* __restrict__ ctr,
                                                            uint64_t* __restrict__ rec_key, uint32_t* __restrict__ rec_row) {
    __shared__ int32_t scratch[kBlock / kWave];
    __shared__ unsigned long long base;
    const TopState s = *fin;
    for (int64_t x0 = (int64_t)blockIdx.x * kBlock; x0 < rows; x0 += (int64_t)gridDim.x * kBlock) {  // block-uniform
        const int64_t l = x0 + threadIdx.x;
        bool win = false;
        uint32_t idx = 0;
        if (l < rows) {
            const uint64_t key = top_key_of(rank[l]);
            if (key >= s.key) {
                idx = (uint32_t)dense[l];
                win = key > s.key || (uint64_t)(inv_max - idx) >= s.inv;
            }
        }
        int32_t total;
        const int32_t off = block_exclusive_scan_add(win ? 1 : 0, scratch, &total);
        if (total == 0) continue;  // block-uniform
        if (threadIdx.x == 0) base = atomicAdd(ctr, (unsigned long long)total);
        __syncthreads();
        const unsigned long long pos = base + (unsigned long long)off;
        if (win && pos < (unsigned long long)want) {
            rec_key[pos] = idx;
            rec_row[pos] = (uint32_t)l;
        }
        __syncthreads();  // base is rewritten on the next trip
    }
}

// want == rows: every row is a record
__global__ void top_all_kernel(const int32_t* __restrict__ dense, int64_t rows, uint64_t* __restrict__ rec_key,
                               uint32_t* __restrict__ rec_row) {
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < rows; l += (int64_t)gridDim.x * blockDim.x) {
        rec_key[l] = (uint32_t)dense[l];
        rec_row[l] = (uint32_t)l;
    }
}

__global__ void top_rekey_kernel(const double* __restrict__ rank, const uint32_t* __restrict__ rec_row, int64_t want,
                                 uint64_t* __restrict__ rec_key) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < want; j += (int64_t)gridDim.x * blockDim.x)
        rec_key[j] = ~top_key_of(rank[rec_row[j]]);
}

__global__ void top_emit_kernel(const uint32_t* __restrict__ rec_row, int64_t want, const double* __restrict__ rank,
                                const int32_t* __restrict__ dense, const int32_t* __restrict__ outdeg,
                                int32_t* __restrict__ index_out, double* __restrict__ rank_out, int32_t* __restrict__ deg_out) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < want; j += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t row = rec_row[j];
        index_out[j] = dense[row];
        rank_out[j] = rank[row];
        deg_out[j] = outdeg[row];
    }
}

// want <= kTopSmall records (index in rec_key, row in rec_row, any order): record j's place is the number of
// records ordered before it (the order is total, so the places are a permutation); order and emit in one
// launch.  Every block stages all the records in LDS and places kWave of them: lane l of each wave holds
// record blockIdx.x * kWave + l, the block's waves each count over a quarter of the records (one LDS
// broadcast per record and wave).
__global__ __launch_bounds__(kBlock) void top_small_kernel(const uint64_t* __restrict__ rec_key,
                                                           const uint32_t* __restrict__ rec_row, int want,
                                                           const double* __restrict__ rank, const int32_t* __restrict__ outdeg,
                                                           int32_t* __restrict__ index_out, double* __restrict__ rank_out,
                                                           int32_t* __restrict__ deg_out) {
    __shared__ uint64_t key[kTopSmall];
    __shared__ uint32_t idx[kTopSmall];
    __shared__ int place[kWave];
    for (int i = threadIdx.x; i < want; i += kBlock) {
        key[i] = top_key_of(rank[rec_row[i]]);
        idx[i] = (uint32_t)rec_key[i];
    }
    if (threadIdx.x < kWave) place[threadIdx.x] = 0;
    __syncthreads();
    const int j = (int)blockIdx.x * kWave + lane_id();
    const bool valid = j < want;
    const uint64_t kj = valid ? key[j] : 0;
    const uint32_t ij = valid ? idx[j] : 0;
    const int part = (want + kBlock / kWave - 1) / (kBlock / kWave);
    const int lo = wave_id() * part, hi = min(want, lo + part);
    int before = 0;
#pragma unroll 8
    for (int i = lo; i < hi; ++i) before += (key[i] > kj || (key[i] == kj && idx[i] < ij)) ? 1 : 0;
    if (valid && before) atomicAdd(&place[lane_id()], before);
    __syncthreads();
    if (threadIdx.x < kWave && valid) {
        const int at = place[threadIdx.x];
        const uint32_t row = rec_row[j];
        index_out[at] = (int32_t)ij;
        rank_out[at] = rank[row];
        deg_out[at] = outdeg[row];
    }
}

struct TopRun {
    int64_t listed = 0;
    float ms = 0;
    int64_t launches = 0;
    double bytes = 0;
    std::vector<int32_t> index, degree;
    std::vector<double> rank;
};

// One shard's min(k, rows) first rows under the order, on the shard's stream, read back in order.
TopRun top_of_shard(const Graph& g, Shard& sh, int64_t k) {
    TopRun r;
    const int64_t rows = sh.rows;
    if (rows == 0) return r;
    DeviceGuard dg(sh);
    hipStream_t st = sh.stream;
    const int64_t want = std::min(k, rows);
    const double* rank = sh.pr_rank.get();
    const int32_t* dense = sh.dense_rows.get();
    const uint32_t inv_max = (uint32_t)(g.n - 1);
    const int ibits = bits_for((uint64_t)(g.n - 1));
    Event c0, c1;
    JG_HIP(hipEventRecord(c0, st));
    DevBuf<uint64_t> rec_key((size_t)want);
    DevBuf<uint32_t> rec_row((size_t)want);
    DevBuf<int32_t> index_out((size_t)want), deg_out((size_t)want);
    DevBuf<double> rank_out((size_t)want);
    TopState fin{};
    if (want == rows) {
        top_all_kernel<<<grid_for(rows), kBlock, 0, st>>>(dense, rows, rec_key.get(), rec_row.get());
        JG_LAUNCH_CHECK();
        ++r.launches;
    } else {
        // ---- select ----
        struct Pass {
            int shift, width;
            bool inv;
        };
        Pass pass[kTopMaxPasses];
        int np = 0;
        for (int hi = 64, p = 0; p < kTopKeyPasses; ++p) {
            const int w = p < 4 ? 11 : 10;
            pass[np++] = Pass{hi - w, w, false};
            hi -= w;
        }
        for (int hi = ibits; hi > 0;) {
            const int w = std::min(hi, 11);
            pass[np++] = Pass{hi - w, w, true};
            hi -= w;
        }
        DevBuf<TopState> state((size_t)np + 1);
        DevBuf<uint32_t> hist((size_t)np * kTopBins);
        DevBuf<unsigned long long> ctr(1);
        JG_HIP(hipMemsetAsync(hist.get(), 0, hist.bytes(), st));
        JG_HIP(hipMemsetAsync(ctr.get(), 0, ctr.bytes(), st));
        top_seed_kernel<<<1, 1, 0, st>>>(state.get(), (unsigned long long)want);
        JG_LAUNCH_CHECK();
        ++r.launches;
        const unsigned grid = grid_for((rows + 3) / 4, kBlock, 2048);
        for (int p = 0; p < np; ++p) {
            uint32_t* h = hist.get() + (size_t)p * kTopBins;
            if (pass[p].inv)
                top_hist_kernel<true><<<grid, kBlock, 0, st>>>(rank, dense, rows, state.get() + p, h, pass[p].shift,
                                                                pass[p].width, inv_max);
            else
                top_hist_kernel<false><<<grid, kBlock, 0, st>>>(rank, dense, rows, state.get() + p, h, pass[p].shift,
                                                                 pass[p].width, inv_max);
            JG_LAUNCH_CHECK();
            top_threshold_kernel<<<1, kBlock, 0, st>>>(h, state.get() + p, state.get() + p + 1, pass[p].shift,
                                                       pass[p].inv ? 1 : 0, p == kTopKeyPasses ? 1 : 0, p == np - 1 ? 1 : 0);
            JG_LAUNCH_CHECK();
            r.launches += 2;
        }
        // ---- filter ----
        top_filter_kernel<<<grid_for(rows, kBlock, 2048), kBlock, 0, st>>>(rank, dense, rows, state.get() + np, inv_max, want,
                                                                          ctr.get(), rec_key.get(), rec_row.get());
        JG_LAUNCH_CHECK();
        ++r.launches;
        unsigned long long stored = 0;
        copy_d2h(&fin, state.get() + np, sizeof fin, st);
        copy_d2h(&stored, ctr.get(), sizeof stored, st);
        if (fin.done != 1 || stored != (unsigned long long)want)
            fail(JG_ERR_STATE, "jg_pagerank_top: the select's counts do not add up");
    }
    // ---- order, emit ----
    int sort_passes = 0;
    if (want <= kTopSmall) {
        top_small_kernel<<<(unsigned)((want + kWave - 1) / kWave), kBlock, 0, st>>>(rec_key.get(), rec_row.get(), (int)want, rank, sh.out_degree.get(),
                                               index_out.get(), rank_out.get(), deg_out.get());
        JG_LAUNCH_CHECK();
        ++r.launches;
    } else {
        prim::radix_sort(rec_key.get(), rec_row.get(), want, ibits, st);
        top_rekey_kernel<<<grid_for(want), kBlock, 0, st>>>(rank, rec_row.get(), want, rec_key.get());
        JG_LAUNCH_CHECK();
        prim::radix_sort(rec_key.get(), rec_row.get(), want, 64, st);
        top_emit_kernel<<<grid_for(want), kBlock, 0, st>>>(rec_row.get(), want, rank, dense, sh.out_degree.get(),
                                                           index_out.get(), rank_out.get(), deg_out.get());
        JG_LAUNCH_CHECK();
        sort_passes = (ibits + 7) / 8 + 8;
        // a sort pass: upsweep, the scan's reduce and apply, downsweep (a scan of several tiles launches
        // more; those are not counted)
        r.launches += 2 + 4 * (int64_t)sort_passes;
    }
    JG_HIP(hipEventRecord(c1, st));
    r.index.resize((size_t)want);
    r.degree.resize((size_t)want);
    r.rank.resize((size_t)want);
    copy_d2h(r.index.data(), index_out.get(), (size_t)want * sizeof(int32_t), st);
    copy_d2h(r.degree.data(), deg_out.get(), (size_t)want * sizeof(int32_t), st);
    copy_d2h(r.rank.data(), rank_out.get(), (size_t)want * sizeof(double), st);
    JG_HIP(hipEventSynchronize(c1));
    JG_HIP(hipEventElapsedTime(&r.ms, c0, c1));
    r.listed = want;
    // Byte model.  A histogram pass reads every row's rank (8 B per row: all rows are read, whether they
    // match the prefix or not); an inv pass also reads the index of the rows whose key is the threshold key
    // (4 B each).  Filter: rank and index (8 + 4 B per row; the index is only loaded for rows at or above
    // the threshold key, the model counts it for all) and a record stored (12 B).  want == rows: index read,
    // record stored (16 B per row).  Order: per 8-bit sort pass a record is read twice and written once
    // (8 + 12 + 12 B), the rekey reads a row, gathers a rank and stores a key (4 + 8 + 8 B); the counting
    // order reads a record and gathers its rank (12 + 8 B, counted once: the blocks' repeats hit the cache).
    // Emit: a row read, index, rank and degree gathered and stored (4 + 16 + 16 B).
    const double w = (double)want, n = (double)rows;
    if (want == rows) {
        r.bytes = 16.0 * n;
    } else {
        const double inv_passes = fin.passes > (unsigned long long)kTopKeyPasses ? (double)(fin.passes - kTopKeyPasses) : 0.0;
        r.bytes = 8.0 * n * (double)fin.passes + 4.0 * (double)fin.tie * inv_passes + 12.0 * n + 12.0 * w;
    }
    r.bytes += want <= kTopSmall ? 20.0 * w : 32.0 * w * (double)sort_passes + 20.0 * w;
    r.bytes += 36.0 * w;
    return r;
}

}  // namespace

void pagerank_top_drop(Graph& g) {
    g.top_listed = -1;
    std::vector<int64_t>().swap(g.top_index);
    std::vector<double>().swap(g.top_rank);
    std::vector<double>().swap(g.top_edges);
}

void pagerank_top(Graph& g, int64_t k, int64_t* listed_out, double* select_ms_out) {
    pagerank_top_drop(g);  // a failed call leaves nothing held
    if (k < 1) fail(JG_ERR_ARG, "jg_pagerank_top: k must be at least 1");
    if (g.ctx->nranks > 1 || g.P != (int)g.shards.size())
        fail(JG_ERR_UNSUPPORTED, "jg_pagerank_top runs on the shards of one process (rank mode: jg_pagerank_end)");
    if (!g.pr_begun) fail(JG_ERR_STATE, "jg_pagerank_top before jg_pagerank_begin");
    g.ctx->last = jg_stats{};
    struct Rec {
        uint64_t key;
        int32_t index, degree;
        double rank;
    };
    std::vector<TopRun> runs;
    float ms = 0;
    int64_t launches = 0, listed = 0;
    double bytes = 0;
    for (auto& sp : g.shards) {
        runs.push_back(top_of_shard(g, *sp, k));
        launches += runs.back().launches;
        bytes += runs.back().bytes;
    }
    ms = runs[0].ms;
    if (runs.size() == 1) {  // one shard's records are the list
        TopRun& r = runs[0];
        listed = r.listed;
        g.top_index.assign(r.index.begin(), r.index.end());
        g.top_edges.assign(r.degree.begin(), r.degree.end());
        g.top_rank = std::move(r.rank);
    } else {
        std::vector<Rec> recs;
        for (const TopRun& r : runs)
            for (size_t j = 0; j < (size_t)r.listed; ++j)
                recs.push_back(Rec{top_key_of(r.rank[j]), r.index[j], r.degree[j], r.rank[j]});
        std::sort(recs.begin(), recs.end(),
                  [](const Rec& a, const Rec& b) { return a.key != b.key ? a.key > b.key : a.index < b.index; });
        listed = std::min<int64_t>(k, (int64_t)recs.size());
        g.top_index.resize((size_t)listed);
        g.top_rank.resize((size_t)listed);
        g.top_edges.resize((size_t)listed);
        for (size_t j = 0; j < (size_t)listed; ++j) {
            g.top_index[j] = recs[j].index;
            g.top_rank[j] = recs[j].rank;
            g.top_edges[j] = (double)recs[j].degree;
        }
    }
    g.top_listed = listed;
    g.ctx->last.compute_ms = ms;
    g.ctx->last.kernel_launches = launches;
    g.ctx->last.algorithmic_bytes = bytes;
    if (listed_out) *listed_out = listed;
    if (select_ms_out) *select_ms_out = (double)ms;
}

void pagerank_top_read(const Graph& g, int64_t first, int64_t count, int64_t* vid_out, int64_t* index_out, double* rank_out,
                       double* edge_count_out) {
    if (g.top_listed < 0) fail(JG_ERR_STATE, "no PageRank top list is held (jg_pagerank_top)");
    if (first < 0 || count < 0 || first > g.top_listed || count > g.top_listed - first)
        fail(JG_ERR_ARG, "range outside the listed vertices");
    for (int64_t j = 0; j < count; ++j) {
        const size_t s = (size_t)(first + j);
        if (vid_out) vid_out[j] = g.vid_of(g.top_index[s]);
        if (index_out) index_out[j] = g.top_index[s];
    }
    if (rank_out && count) std::memcpy(rank_out, g.top_rank.data() + first, (size_t)count * sizeof(double));
    if (edge_count_out && count) std::memcpy(edge_count_out, g.top_edges.data() + first, (size_t)count * sizeof(double));
}

}  // namespace jg
