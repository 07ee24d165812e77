// jg_pathdag.hip — the shortest-path predecessor DAG of one kept depth row (jg_bfs_kept_dag), built on
// the device so that only the DAG crosses to the host ("Predecessor DAG on the device").
//
// One shard (column ids are local rows).  `dep` is the kept depth plane, `c` the adjacency the
// predecessors are read from (the reverse of the kept traversal's direction), rows sorted so that equal
// columns are adjacent (jg_build.hip).
//   seed    on[l] = row l is a reached target; deepest = their largest depth.  The targets, compacted in
//           row order and stably sorted by depth (descending), are the per-depth buckets.
//   sweep   d = deepest + 1 .. 1, one launch each (dag_step_kernel), no host read in between: the frontier
//           of level d (a queue with edge offsets, jg_frontier.h) is walked edge-parallel; an entry u with
//           dep[u] == d - 1 whose `on` byte the walker is first to set joins level d - 1's queue; the
//           targets at depth d - 1 join it from their bucket.  Level d's size is read by level d's launch
//           from the counter level d + 1's launch filled.  Work: the DAG rows' entries + deepest launches.
//   emit    the DAG vertices are the rows with `on` set: compacted in row order, stably sorted by depth
//           (descending) — an order that does not depend on the queues' atomic append order.  One count
//           pass and one fill pass over the edge space of all DAG rows (source excluded) then apply the
//           same predicate to the same inputs: entry u of v counts if dep[u] == dep[v] - 1 and u differs
//           from the entry before it in the row.  Nothing either pass reads is written by either.
// The count and fill passes cut the edge space into ranges of kDagRange entries, one wave each, 64
// consecutive entries per step: a row's rank inside a step is a ballot popcount over the row's lanes,
// across steps a wave-uniform carry, across ranges the sum of the per-range partial counts of the row
// (dag_count_kernel leaves them; a 10^5-entry row spans ~100 ranges).  So a hub row is walked by many
// lanes and waves and still emitted in row order.
#include "jg_frontier.h"
#include "jg_internal.h"

namespace jg {
namespace {

constexpr int kDagRange = 1024;  // entries per wave of the count / fill passes (16 steps of 64)

// on[l] (bytes of `on`) = row l is a reached target; *deepest = the largest depth of one (-1: none)
__global__ __launch_bounds__(kBlock) void dag_seed_kernel(const int32_t* __restrict__ dep,
                                                          const int32_t* __restrict__ dense,
                                                          const uint8_t* __restrict__ target, int64_t rows,
                                                          uint8_t* __restrict__ on, int32_t* __restrict__ deepest) {
    __shared__ int32_t red[kBlock / kWave];
    int32_t m = -1;
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < rows; l += (int64_t)gridDim.x * blockDim.x) {
        const int32_t d = dep[l];
        const bool t = d >= 0 && (!target || target[dense[l]] != 0);
        on[l] = t ? 1 : 0;
        if (t && d > m) m = d;
    }
    m = wave_reduce_max(m);
    if (lane_id() == 0) red[wave_id()] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; ++w) m = red[w] > m ? red[w] : m;
        if (m >= 0) atomicMax(deepest, m);
    }
}

// key[j] = deepest - dep[idx[j]] (ascending keys = descending depth), val[j] = the row
__global__ void dag_keys_kernel(const int64_t* __restrict__ idx, int64_t k, const int32_t* __restrict__ dep,
                                int32_t deepest, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < k; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = idx[j];
        key[j] = (uint64_t)(deepest - dep[l]);
        val[j] = (uint32_t)l;
    }
}

struct DagStep {
    const int64_t* rp;
    const int32_t* col;
    const int32_t* dep;
    uint32_t* on;  // the `on` bytes as words (a byte is set with an atomic OR on its word)
    int32_t* vq;   // the level queues, concatenated deepest level first ([rows])
    int64_t* qo;   // each entry's first edge number inside its level
    unsigned long long* packed;  // [deepest + 2] per level: (vertices << kPackShift) | entries
    int64_t* lbase;              // [deepest + 2] first queue slot of each level
    const uint64_t* tkey;        // the targets' keys (deepest - depth), ascending
    const uint32_t* tval;        // their rows
    int64_t nt;
    int32_t d, deepest;
};

// first j in [0, n) with key[j] >= k (n if none)
__device__ __forceinline__ int64_t lower_bound_key(const uint64_t* __restrict__ key, int64_t n, uint64_t k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Level a.d: walks its frontier's entries and fills level a.d - 1's queue (marked rows + that depth's targets).
__global__ __launch_bounds__(kBlock) void dag_step_kernel(DagStep a) {
    __shared__ WaveStage ws;
    __shared__ int64_t s_t[2];
    WaveApp app{ws};
    const unsigned long long pk = a.packed[a.d];
    const int64_t nq = (int64_t)(pk >> kPackShift), mf = (int64_t)(pk & kEdgeMask);
    const int64_t base = a.lbase[a.d], nbase = base + nq;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.lbase[a.d - 1] = nbase;
    if (threadIdx.x == 0) {
        const uint64_t k = (uint64_t)(a.deepest - (a.d - 1));
        s_t[0] = lower_bound_key(a.tkey, a.nt, k);
        s_t[1] = lower_bound_key(a.tkey, a.nt, k + 1);
    }
    __syncthreads();
    const int32_t* queue = a.vq + base;
    const int64_t* qoff = a.qo + base;
    int32_t* qout = a.vq + nbase;
    int64_t* qoout = a.qo + nbase;
    unsigned long long* pout = a.packed + (a.d - 1);
    const int32_t want = a.d - 1;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_tile = nthreads * 4;
    const int64_t tiles = (mf + per_tile - 1) / per_tile;
    for (int64_t t = 0; t < tiles; ++t) {
        if ((t * nthreads + (int64_t)blockIdx.x * blockDim.x) * 4 >= mf) break;  // block-uniform
        const int64_t e0 = (t * nthreads + tid) * 4;
        EdgeCursor cur{qoff, nq, mf};
        if (e0 < mf) cur.seek(e0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t e = e0 + k;
            bool take = false;
            int32_t u = 0;
            int64_t deg = 0;
            if (e < mf) {
                cur.advance(e);
                const int32_t v = queue[cur.i];
                u = a.col[a.rp[v] + cur.row_offset(e)];
                if (a.dep[u] == want) {
                    const uint32_t bit = 1u << ((u & 3) * 8);
                    if (!(a.on[u >> 2] & bit)) take = !(atomicOr(&a.on[u >> 2], bit) & bit);
                    if (take) deg = a.rp[u + 1] - a.rp[u];
                }
            }
            app.append(take, u, deg, qout, qoout, pout);
        }
    }
    // the targets at depth d - 1: their `on` byte was set by the seed, so the walk above never takes them
    const int64_t t0 = s_t[0], t1 = s_t[1];
    for (int64_t j0 = t0 + (int64_t)blockIdx.x * blockDim.x; j0 < t1; j0 += nthreads) {  // block-uniform
        const int64_t j = j0 + threadIdx.x;
        const bool take = j < t1;
        int32_t u = 0;
        int64_t deg = 0;
        if (take) {
            u = (int32_t)a.tval[j];
            deg = a.rp[u + 1] - a.rp[u];
        }
        app.append(take, u, deg, qout, qoout, pout);
    }
    app.final(qout, qoout, pout);
}

// The sorted DAG rows: local row, caller-order vertex, depth, and the row length the passes walk (0 for
// the source: its predecessor range is empty).
__global__ void dag_unpack_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t nv,
                                  int32_t deepest, const int64_t* __restrict__ rp, const int32_t* __restrict__ dense,
                                  int32_t* __restrict__ local, int32_t* __restrict__ vertex,
                                  int32_t* __restrict__ depth, int64_t* __restrict__ len) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nv; j += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = (int32_t)val[j];
        const int32_t d = deepest - (int32_t)key[j];
        local[j] = l;
        vertex[j] = dense[l];
        depth[j] = d;
        len[j] = d > 0 ? rp[l + 1] - rp[l] : 0;
    }
}

struct DagWalk {
    const int32_t* local;   // [nv] DAG rows
    const int32_t* depth;   // [nv]
    const int64_t* qoff;    // [nv + 1] first edge number of each DAG row (exclusive scan of the lengths)
    int64_t nv, mf, nranges;
    const int64_t* rp;
    const int32_t* col;
    const int32_t* dep;
    const int32_t* dense;
    int32_t* cnt;           // [nv] distinct predecessors per DAG row (zeroed before the count pass)
    // per range: the DAG rows of its first and last entry, and the counted entries of each inside the range
    int32_t *r_fi, *r_li, *r_ca, *r_cl;
    const int64_t* off;     // [nv + 1] exclusive scan of cnt (fill)
    int32_t* pred;          // [off[nv]] (fill)
};

// One step of a range: lane l looks at edge sb + l.  Returns whether the lane's entry counts; i = its DAG
// row, mask = the lanes of this step on that row, x = the entry.
struct DagLane {
    bool valid, counts;
    int32_t i, x;
    uint64_t mask;
    int lo;  // the row's first lane in this step
};
__device__ __forceinline__ DagLane dag_lane(const DagWalk& a, EdgeCursor& cur, int64_t sb, int64_t end) {
    DagLane r{false, false, 0, 0, 0ull, 0};
    const int64_t e = sb + lane_id();
    r.valid = e < end;
    if (r.valid) {
        cur.advance(e);
        r.i = (int32_t)cur.i;
        const int64_t q0 = a.qoff[cur.i];
        const int64_t p = a.rp[a.local[cur.i]] + (e - q0);
        r.x = a.col[p];
        r.counts = a.dep[r.x] == a.depth[cur.i] - 1 && (e == q0 || a.col[p - 1] != r.x);
        const int64_t lo = q0 > sb ? q0 - sb : 0;
        const int64_t hi = cur.next_bound - sb < kWave ? cur.next_bound - sb : kWave;
        r.lo = (int)lo;
        const uint64_t upto = hi >= kWave ? ~0ull : ((1ull << hi) - 1ull);
        r.mask = upto & ~((1ull << lo) - 1ull);
    }
    return r;
}

__global__ __launch_bounds__(kBlock) void dag_count_kernel(DagWalk a) {
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / kWave);
    for (int64_t w = (int64_t)blockIdx.x * (kBlock / kWave) + wave_id(); w < a.nranges; w += nwaves) {
        const int64_t base = w * kDagRange;
        const int64_t end = base + kDagRange < a.mf ? base + kDagRange : a.mf;
        EdgeCursor cur{a.qoff, a.nv, a.mf}, last{a.qoff, a.nv, a.mf};
        const int64_t e0 = base + lane_id();
        cur.seek(e0 < end ? e0 : end - 1);
        last.seek(end - 1);
        const int32_t fi = __shfl((int32_t)cur.i, 0, kWave), li = (int32_t)last.i;
        int32_t ca = 0, cl = 0;
        for (int64_t sb = base; sb < end; sb += kWave) {
            const DagLane r = dag_lane(a, cur, sb, end);
            const uint64_t b = __ballot(r.counts);
            ca += __popcll(__ballot(r.counts && r.i == fi));
            cl += __popcll(__ballot(r.counts && r.i == li));
            if (r.valid && lane_id() == r.lo) {  // the row's first lane of this step
                const int32_t c = __popcll(b & r.mask);
                const bool contained = a.qoff[r.i] >= sb && cur.next_bound <= sb + kWave;
                if (contained) a.cnt[r.i] = c;
                else if (c) atomicAdd(&a.cnt[r.i], c);
            }
        }
        if (lane_id() == 0) {
            a.r_fi[w] = fi;
            a.r_li[w] = li;
            a.r_ca[w] = ca;
            a.r_cl[w] = cl;
        }
    }
}

__global__ __launch_bounds__(kBlock) void dag_fill_kernel(DagWalk a) {
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / kWave);
    for (int64_t w = (int64_t)blockIdx.x * (kBlock / kWave) + wave_id(); w < a.nranges; w += nwaves) {
        const int64_t base = w * kDagRange;
        const int64_t end = base + kDagRange < a.mf ? base + kDagRange : a.mf;
        EdgeCursor cur{a.qoff, a.nv, a.mf};
        const int64_t e0 = base + lane_id();
        cur.seek(e0 < end ? e0 : end - 1);
        // the row open at the range's start, and its counted entries in the ranges before (wave-uniform)
        int32_t open_row = __shfl((int32_t)cur.i, 0, kWave);
        int32_t open_carry = 0;
        const int64_t row_begin = a.qoff[open_row];
        for (int64_t p = w - 1; p >= 0 && row_begin < (p + 1) * kDagRange; --p) {
            const bool whole = a.r_fi[p] == open_row;  // range p lies inside the row (or starts with it)
            open_carry += whole ? a.r_ca[p] : a.r_cl[p];
            if (!whole) break;
        }
        for (int64_t sb = base; sb < end; sb += kWave) {
            const DagLane r = dag_lane(a, cur, sb, end);
            const uint64_t b = __ballot(r.counts);
            const int32_t before = r.valid && r.i == open_row ? open_carry : 0;
            if (r.counts) a.pred[a.off[r.i] + before + __popcll(b & r.mask & lanemask_lt())] = a.dense[r.x];
            // the step's last row stays open
            const int nvalid = end - sb < kWave ? (int)(end - sb) : kWave;
            const int32_t tot = before + __popcll(b & r.mask);
            open_carry = __shfl(tot, nvalid - 1, kWave);
            open_row = __shfl(r.i, nvalid - 1, kWave);
        }
    }
}

const Csr& reverse_csr(const Shard& sh, int dir) {
    return dir == JG_DIR_BOTH ? sh.both : dir == JG_DIR_OUT ? sh.in : sh.out;
}

}  // namespace

void bfs_kept_dag_drop(Graph& g) {
    for (auto& sp : g.shards) {
        DeviceGuard dg(*sp);
        sp->dag_vertex.reset();
        sp->dag_depth.reset();
        sp->dag_pred.reset();
        sp->dag_off.reset();
    }
    g.dag_nv = -1;
    g.dag_ne = 0;
}

void bfs_kept_dag(Graph& g, int s, const uint8_t* target, int64_t* nv_out, int64_t* ne_out, int32_t* deepest_out) {
    if (g.P != 1 || g.shards.size() != 1)
        fail(JG_ERR_UNSUPPORTED, "jg_bfs_kept_dag runs on one shard (sharded graphs: walk back on the host)");
    if (s < 0 || s >= g.kept_nsrc) fail(JG_ERR_ARG, "no kept depth row with that index (jg_bfs_keep)");
    Shard& sh = *g.shards[0];
    const Csr& c = reverse_csr(sh, g.kept_dir);
    if (!c.present())
        fail(JG_ERR_UNSUPPORTED, "jg_bfs_kept_dag reads the reverse of the kept traversal's adjacency: not built");
    if (sh.rows != g.n || sh.dense_rows.size() < (size_t)std::max<int64_t>(sh.rows, 1))
        fail(JG_ERR_UNSUPPORTED, "jg_bfs_kept_dag: the shard does not hold every vertex");
    if (sh.rows >> (64 - kPackShift)) fail(JG_ERR_UNSUPPORTED, "jg_bfs_kept_dag: too many rows for the level counters");
    bfs_kept_dag_drop(g);
    Ctx& ctx = *g.ctx;
    ctx.last = jg_stats{};
    DeviceGuard dg(sh);
    hipStream_t st = sh.stream;
    const int64_t rows = sh.rows;
    const int32_t* dep = sh.kept_depth.get() + (int64_t)s * rows;
    const auto finish = [&](int64_t nv, int64_t ne, int32_t deepest) {
        g.dag_nv = nv;
        g.dag_ne = ne;
        if (nv_out) *nv_out = nv;
        if (ne_out) *ne_out = ne;
        if (deepest_out) *deepest_out = deepest;
        ctx.last.levels = deepest;
        ctx.last.supersteps = deepest < 0 ? 0 : deepest;
    };
    if (rows == 0) return finish(0, 0, -1);

    DevBuf<uint8_t> dtarget;
    if (target) {  // the mask travels before the timed region
        dtarget.alloc((size_t)g.n);
        copy_h2d(dtarget.get(), target, (size_t)g.n, st);
    }
    Event t0, t1;
    JG_HIP(hipEventRecord(t0, st));

    // ---- seed ----
    const int64_t on_words = (rows + 3) / 4;
    DevBuf<uint32_t> on((size_t)on_words);
    DevBuf<int32_t> d_deepest(1);
    JG_HIP(hipMemsetAsync(on.get(), 0, on.bytes(), st));
    JG_HIP(hipMemsetAsync(d_deepest.get(), 0xff, sizeof(int32_t), st));
    uint8_t* on8 = reinterpret_cast<uint8_t*>(on.get());
    dag_seed_kernel<<<grid_for(rows, kBlock, 2048), kBlock, 0, st>>>(dep, sh.dense_rows.get(), dtarget.get(), rows, on8,
                                                                    d_deepest.get());
    JG_LAUNCH_CHECK();
    DevBuf<int64_t> idx((size_t)rows), cpos, cscan;
    const int64_t nt = prim::compact_indices(on8, rows, idx.get(), cpos, cscan, st);
    if (nt == 0) {
        JG_HIP(hipEventRecord(t1, st));
        JG_HIP(hipEventSynchronize(t1));
        float ms = 0;
        JG_HIP(hipEventElapsedTime(&ms, t0, t1));
        finish(0, 0, -1);
        ctx.last.compute_ms = ms;
        ctx.last.algorithmic_bytes = 10.0 * (double)rows;
        return;
    }
    int32_t deepest = -1;
    copy_d2h(&deepest, d_deepest.get(), sizeof(int32_t), st);
    const int dbits = std::max(bits_for((uint64_t)deepest), 1);
    DevBuf<uint64_t> tkey((size_t)nt);
    DevBuf<uint32_t> tval((size_t)nt);
    dag_keys_kernel<<<grid_for(nt), kBlock, 0, st>>>(idx.get(), nt, dep, deepest, tkey.get(), tval.get());
    JG_LAUNCH_CHECK();
    prim::radix_sort(tkey.get(), tval.get(), nt, dbits, st);

    // ---- backward sweep: levels deepest + 1 (no frontier: it seeds the deepest level's queue) .. 1 ----
    DevBuf<int32_t> vq((size_t)rows);
    DevBuf<int64_t> qo((size_t)rows);
    DevBuf<unsigned long long> packed((size_t)deepest + 2);
    DevBuf<int64_t> lbase((size_t)deepest + 2);
    JG_HIP(hipMemsetAsync(packed.get(), 0, packed.bytes(), st));
    JG_HIP(hipMemsetAsync(lbase.get(), 0, lbase.bytes(), st));
    DagStep sp{c.row_ptr.get(), c.col.get(), dep, on.get(), vq.get(), qo.get(), packed.get(), lbase.get(),
               tkey.get(), tval.get(), nt, 0, deepest};
    const unsigned step_grid = grid_for(std::max<int64_t>(c.nnz / 4, rows), kBlock, 1024);
    for (int32_t d = deepest + 1; d >= 1; --d) {
        sp.d = d;
        dag_step_kernel<<<step_grid, kBlock, 0, st>>>(sp);
        JG_LAUNCH_CHECK();
    }
    int64_t launches = (int64_t)deepest + 1;

    // ---- emit ----
    const int64_t nv = prim::compact_indices(on8, rows, idx.get(), cpos, cscan, st);
    DevBuf<uint64_t> vkey((size_t)nv);
    DevBuf<uint32_t> vval((size_t)nv);
    dag_keys_kernel<<<grid_for(nv), kBlock, 0, st>>>(idx.get(), nv, dep, deepest, vkey.get(), vval.get());
    JG_LAUNCH_CHECK();
    prim::radix_sort(vkey.get(), vval.get(), nv, dbits, st);
    DevBuf<int32_t> local((size_t)nv);
    DevBuf<int64_t> len((size_t)nv), qoff((size_t)nv + 1);
    sh.dag_vertex.alloc((size_t)nv);
    sh.dag_depth.alloc((size_t)nv);
    sh.dag_off.alloc((size_t)nv + 1);
    dag_unpack_kernel<<<grid_for(nv), kBlock, 0, st>>>(vkey.get(), vval.get(), nv, deepest, c.row_ptr.get(),
                                                       sh.dense_rows.get(), local.get(), sh.dag_vertex.get(),
                                                       sh.dag_depth.get(), len.get());
    JG_LAUNCH_CHECK();
    prim::exclusive_scan(len.get(), qoff.get(), nv, st);
    int64_t mf = 0;
    copy_d2h(&mf, qoff.get() + nv, sizeof(int64_t), st);
    DevBuf<int32_t> cnt((size_t)nv);
    JG_HIP(hipMemsetAsync(cnt.get(), 0, cnt.bytes(), st));
    const int64_t nranges = (mf + kDagRange - 1) / kDagRange;
    DevBuf<int32_t> rfi((size_t)std::max<int64_t>(nranges, 1)), rli((size_t)std::max<int64_t>(nranges, 1)),
        rca((size_t)std::max<int64_t>(nranges, 1)), rcl((size_t)std::max<int64_t>(nranges, 1));
    DagWalk wk{local.get(), sh.dag_depth.get(), qoff.get(), nv, mf, nranges, c.row_ptr.get(), c.col.get(), dep,
               sh.dense_rows.get(), cnt.get(), rfi.get(), rli.get(), rca.get(), rcl.get(), nullptr, nullptr};
    const unsigned walk_grid = grid_for(nranges, kBlock / kWave, 16384);
    if (mf > 0) {
        dag_count_kernel<<<walk_grid, kBlock, 0, st>>>(wk);
        JG_LAUNCH_CHECK();
        ++launches;
    }
    prim::exclusive_scan(cnt.get(), sh.dag_off.get(), nv, st);
    int64_t ne = 0;
    copy_d2h(&ne, sh.dag_off.get() + nv, sizeof(int64_t), st);
    sh.dag_pred.alloc((size_t)std::max<int64_t>(ne, 1));
    if (mf > 0) {
        wk.off = sh.dag_off.get();
        wk.pred = sh.dag_pred.get();
        dag_fill_kernel<<<walk_grid, kBlock, 0, st>>>(wk);
        JG_LAUNCH_CHECK();
        ++launches;
    }
    JG_HIP(hipEventRecord(t1, st));
    JG_HIP(hipEventSynchronize(t1));
    float ms = 0;
    JG_HIP(hipEventElapsedTime(&ms, t0, t1));
    finish(nv, ne, deepest);
    ctx.last.compute_ms = ms;
    ctx.last.kernel_launches = launches;
    ctx.last.edges_traversed = (double)mf;
    // Byte model.  Seed and the two compactions: 10 B per row (depth, dense index, mask and `on` byte), 9 B
    // per row per compaction (flag + position).  Each of the three walks (sweep, count, fill) reads a
    // DAG-row entry's column and probes its depth: 3 x 8 B per entry.  A DAG vertex costs ~64 B (two
    // sort records of 12 B read and written, queue entry, row_ptr pair, count, offset, outputs), an
    // emitted predecessor 8 B (dense probe + store).
    ctx.last.algorithmic_bytes = 28.0 * (double)rows + 24.0 * (double)mf + 64.0 * (double)nv + 8.0 * (double)ne;
}

void bfs_kept_dag_read(Graph& g, int64_t first, int64_t count, int32_t* vertex_out, int32_t* depth_out,
                       int64_t* off_out, int32_t* pred_out) {
    if (g.dag_nv < 0) fail(JG_ERR_STATE, "no predecessor DAG is held (jg_bfs_kept_dag)");
    if (first < 0 || count < 0 || first > g.dag_nv || count > g.dag_nv - first)
        fail(JG_ERR_ARG, "range outside the DAG's vertices");
    if (g.dag_nv == 0) {
        if (off_out) off_out[0] = 0;
        return;
    }
    Shard& sh = *g.shards[0];
    DeviceGuard dg(sh);
    hipStream_t st = sh.stream;
    if (vertex_out) copy_d2h(vertex_out, sh.dag_vertex.get() + first, (size_t)count * sizeof(int32_t), st);
    if (depth_out) copy_d2h(depth_out, sh.dag_depth.get() + first, (size_t)count * sizeof(int32_t), st);
    if (off_out) copy_d2h(off_out, sh.dag_off.get() + first, (size_t)(count + 1) * sizeof(int64_t), st);
    if (pred_out) {
        int64_t b = 0, e = 0;
        copy_d2h(&b, sh.dag_off.get() + first, sizeof(int64_t), st);
        copy_d2h(&e, sh.dag_off.get() + first + count, sizeof(int64_t), st);
        copy_d2h(pred_out, sh.dag_pred.get() + b, (size_t)(e - b) * sizeof(int32_t), st);
    }
}

}  // namespace jg
