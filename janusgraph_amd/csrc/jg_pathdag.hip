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
//
// The weighted DAG of a kept distance plane (jg_sssp_kept_dag; DESIGN.md, "Weighted predecessor DAG on the
// device") shares the emit: the count and fill passes are templates over the DAG's flavour (HopDag: depth
// planes and "one level up"; TightDag: distance planes and "a tight edge"), which names the per-vertex value
// and decides whether an entry counts.  Its sweep runs by rounds instead of levels (wdag_round_kernel).
// On the host the two drivers (bfs_kept_dag_t, sssp_kept_dag_t) hold what differs: their checks, seed, sweep,
// what their stats mean and their byte model.  The rest is one copy: the common checks, the target upload and
// the timed region (dag_only_shard, DagRun), the emit (dag_emit<T>, into the shard's HeldDag of the family), the
// readers (dag_read, dag_read_edges) and the drop (drop_held).
//
// The edge-listing DAGs (jg_bfs_kept_dag_edges, jg_sssp_kept_dag_edges; DESIGN.md, "Edge-listing predecessor
// DAG") are the same sweeps with two more flavours (HopEdgeDag, TightEdgeDag): the predicate without the
// de-duplication, so every qualifying entry of a run of parallel edges is listed, and the fill pass stores the
// entry's edge ordinal (Csr::eidx, JG_ADJ_EDGE_INDEX) beside its predecessor.
#include <climits>
#include <cstring>
#include <type_traits>

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

// key[j] = deepest - dep[idx[j]] (ascending keys = descending depth), val[j] = the row (V: int32 depths, or
// int64 distances with `deepest` the farthest one)
template <class V>
__global__ void dag_keys_kernel(const int64_t* __restrict__ idx, int64_t k, const V* __restrict__ dep,
                                V deepest, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
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
template <class V>
__global__ void dag_unpack_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t nv,
                                  V deepest, const int64_t* __restrict__ rp, const int32_t* __restrict__ dense,
                                  int32_t* __restrict__ local, int32_t* __restrict__ vertex,
                                  V* __restrict__ depth, int64_t* __restrict__ len) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nv; j += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = (int32_t)val[j];
        const V d = deepest - (V)key[j];
        local[j] = l;
        vertex[j] = dense[l];
        depth[j] = d;
        len[j] = d > 0 ? rp[l + 1] - rp[l] : 0;
    }
}

// The two flavours of the emit passes.  Val: the per-vertex value (of the plane `dep` and of the sorted DAG
// rows `depth`); Extra: what the predicate reads besides; counts(a, i, x, p, k): whether entry p of the
// adjacency (column x, the k-th of its row) is listed as a predecessor of DAG row i.
struct HopDag {  // jg_bfs_kept_dag: one level up, the first entry of its equal-column run
    using Val = int32_t;
    static constexpr bool kEdges = false;
    struct Extra {};
    template <class W>
    static __device__ __forceinline__ bool counts(const W& a, int64_t i, int32_t x, int64_t p, int64_t k) {
        return a.dep[x] == a.depth[i] - 1 && (k == 0 || a.col[p - 1] != x);
    }
};
struct HopEdgeDag {  // jg_bfs_kept_dag_edges: one level up, every entry (a self-loop is never one level up)
    using Val = int32_t;
    static constexpr bool kEdges = true;
    struct Extra {};
    template <class W>
    static __device__ __forceinline__ bool counts(const W& a, int64_t i, int32_t x, int64_t, int64_t) {
        return a.dep[x] == a.depth[i] - 1;
    }
};
struct TightInt {  // the arithmetic of TightDag / TightEdgeDag, for the sweep
    using W = int32_t;
    static constexpr long long kAbsent = LLONG_MIN;
    static __device__ __forceinline__ bool tight(long long du, int32_t w, long long dv) {
        return w != INT32_MIN && du != LLONG_MIN && du + (long long)w == dv;
    }
    static const int32_t* weights(const Csr& c) { return c.weight.get(); }
    static size_t weight_count(const Csr& c) { return c.weight.size(); }
};
struct TightDag {  // jg_sssp_kept_dag: a tight edge, the first of its weight in its equal-column run
    using Val = long long;
    using Arith = TightInt;
    static constexpr bool kEdges = false;
    struct Extra {
        const int32_t* wt;
    };
    // All tight entries of one (v, u) run carry the run's smallest weight (a lighter one would have given v a
    // smaller distance), so "the first tight entry of the run" is "tight, and no earlier entry of the run has
    // this weight": a backward scan over the run's entries before p (parallel edges: a handful).
    template <class W>
    static __device__ __forceinline__ bool counts(const W& a, int64_t i, int32_t x, int64_t p, int64_t k) {
        const int32_t w = a.wt[p];
        const long long du = a.dep[x];
        if (w == INT32_MIN || du == LLONG_MIN || du + (long long)w != a.depth[i]) return false;
        for (int64_t q = p - 1; q >= p - k && a.col[q] == x; --q)
            if (a.wt[q] == w) return false;
        return true;
    }
};
struct TightEdgeDag {  // jg_sssp_kept_dag_edges: every tight entry (weights are positive: a self-loop is never tight)
    using Val = long long;
    using Arith = TightInt;
    static constexpr bool kEdges = true;
    using Extra = TightDag::Extra;
    template <class W>
    static __device__ __forceinline__ bool counts(const W& a, int64_t i, int32_t x, int64_t p, int64_t) {
        const int32_t w = a.wt[p];
        const long long du = a.dep[x];
        return w != INT32_MIN && du != LLONG_MIN && du + (long long)w == a.depth[i];
    }
};

// The f64 flavours (jg_sssp_kept_dag_f64, jg_sssp_kept_dag_edges_f64): the plane holds the bit patterns of
// doubles >= 0 (+Inf's: absent), whose integer order is the distance order, so Val stays long long and seed, sweep,
// sort and emit move the same 64-bit values; only the tight-edge predicate adds, in double.  u -> v with weight w
// is tight iff dist[u] is present, dist[u] < dist[v] and fl(dist[u] + w) == dist[v], with no epsilon.
constexpr long long kF64Absent = 0x7FF0000000000000ll;  // +Inf
struct TightF64 {
    using W = double;
    static constexpr long long kAbsent = kF64Absent;
    static __device__ __forceinline__ bool tight(long long du, double w, long long dv) {
        // (patterns of non-negative doubles: equal patterns are equal doubles, and du < dv orders the doubles)
        return du != kF64Absent && du < dv && __double_as_longlong(__longlong_as_double(du) + w) == dv;
    }
    static const double* weights(const Csr& c) { return c.wf.get(); }
    static size_t weight_count(const Csr& c) { return c.wf.size(); }
};
struct TightDagF64 {  // a tight edge, the first tight entry of its equal-column run
    using Val = long long;
    using Arith = TightF64;
    static constexpr bool kEdges = false;
    struct Extra {
        const double* wt;
    };
    // Two entries of one (v, u) run may both be tight with different weights (their sums round to the same
    // double), so "the first of its weight" could list u twice: here an entry counts when no earlier entry of the
    // run is tight (in integers the two rules agree).
    template <class Wk>
    static __device__ __forceinline__ bool counts(const Wk& a, int64_t i, int32_t x, int64_t p, int64_t k) {
        const long long du = a.dep[x], dv = a.depth[i];
        if (!TightF64::tight(du, a.wt[p], dv)) return false;
        for (int64_t q = p - 1; q >= p - k && a.col[q] == x; --q)
            if (TightF64::tight(du, a.wt[q], dv)) return false;
        return true;
    }
};
struct TightEdgeDagF64 {  // every tight entry (a self-loop has dist[u] == dist[v]: never tight)
    using Val = long long;
    using Arith = TightF64;
    static constexpr bool kEdges = true;
    using Extra = TightDagF64::Extra;
    template <class Wk>
    static __device__ __forceinline__ bool counts(const Wk& a, int64_t i, int32_t x, int64_t p, int64_t) {
        return TightF64::tight(a.dep[x], a.wt[p], a.depth[i]);
    }
};

template <class T>
struct DagWalk : T::Extra {
    const int32_t* local;   // [nv] DAG rows
    const typename T::Val* depth;  // [nv]
    const int64_t* qoff;    // [nv + 1] first edge number of each DAG row (exclusive scan of the lengths)
    int64_t nv, mf, nranges;
    const int64_t* rp;
    const int32_t* col;
    const typename T::Val* dep;
    const int32_t* dense;
    int32_t* cnt;           // [nv] distinct predecessors per DAG row (zeroed before the count pass)
    // per range: the DAG rows of its first and last entry, and the counted entries of each inside the range
    int32_t *r_fi, *r_li, *r_ca, *r_cl;
    const int64_t* off;     // [nv + 1] exclusive scan of cnt (fill)
    int32_t* pred;          // [off[nv]] (fill)
    const uint32_t* eidx;   // the adjacency's edge ordinals (edge flavours; else null)
    uint32_t* edge;         // [off[nv]] each listed entry's ordinal, parallel to pred (edge flavours, fill)
};

// One step of a range: lane l looks at edge sb + l.  Returns whether the lane's entry counts; i = its DAG
// row, mask = the lanes of this step on that row, x = the entry.
struct DagLane {
    bool valid, counts;
    int32_t i, x;
    uint64_t mask;
    int lo;  // the row's first lane in this step
    int64_t p;  // the entry's position in the adjacency
};
template <class T>
__device__ __forceinline__ DagLane dag_lane(const DagWalk<T>& a, EdgeCursor& cur, int64_t sb, int64_t end) {
    DagLane r{false, false, 0, 0, 0ull, 0, 0};
    const int64_t e = sb + lane_id();
    r.valid = e < end;
    if (r.valid) {
        cur.advance(e);
        r.i = (int32_t)cur.i;
        const int64_t q0 = a.qoff[cur.i];
        const int64_t p = a.rp[a.local[cur.i]] + (e - q0);
        r.p = p;
        r.x = a.col[p];
        r.counts = T::counts(a, cur.i, r.x, p, e - q0);
        const int64_t lo = q0 > sb ? q0 - sb : 0;
        const int64_t hi = cur.next_bound - sb < kWave ? cur.next_bound - sb : kWave;
        r.lo = (int)lo;
        const uint64_t upto = hi >= kWave ? ~0ull : ((1ull << hi) - 1ull);
        r.mask = upto & ~((1ull << lo) - 1ull);
    }
    return r;
}

template <class T>
__global__ __launch_bounds__(kBlock) void dag_count_kernel(DagWalk<T> a) {
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

template <class T>
__global__ __launch_bounds__(kBlock) void dag_fill_kernel(DagWalk<T> a) {
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
            if (r.counts) {
                const int64_t slot = a.off[r.i] + before + __popcll(b & r.mask & lanemask_lt());
                a.pred[slot] = a.dense[r.x];
                if constexpr (T::kEdges) a.edge[slot] = a.eidx[r.p];
            }
            // the step's last row stays open
            const int nvalid = end - sb < kWave ? (int)(end - sb) : kWave;
            const int32_t tot = before + __popcll(b & r.mask);
            open_carry = __shfl(tot, nvalid - 1, kWave);
            open_row = __shfl(r.i, nvalid - 1, kWave);
        }
    }
}

// ---------------- the weighted DAG: seed and backward sweep by rounds ----------------

// on[l] = row l is a target: a present distance, <= max_distance when that is >= 0, and its flag set;
// *farthest = the largest distance of one (-1: none).  kAbsent: the plane's "unreached" (an f64 plane's values,
// its max_distance and farthest are bit patterns: the same compares)
template <long long kAbsent>
__global__ __launch_bounds__(kBlock) void wdag_seed_kernel(const long long* __restrict__ dist,
                                                           const int32_t* __restrict__ dense,
                                                           const uint8_t* __restrict__ target, int64_t rows,
                                                           long long max_distance, uint8_t* __restrict__ on,
                                                           long long* __restrict__ farthest) {
    __shared__ long long red[kBlock / kWave];
    long long m = -1;
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < rows; l += (int64_t)gridDim.x * blockDim.x) {
        const long long d = dist[l];
        const bool t = d != kAbsent && (max_distance < 0 || d <= max_distance) && (!target || target[dense[l]] != 0);
        on[l] = t ? 1 : 0;
        if (t && d > m) m = d;
    }
    m = wave_reduce_max(m);
    if (lane_id() == 0) red[wave_id()] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; ++w) m = red[w] > m ? red[w] : m;
        if (m >= 0) atomicMax(farthest, m);
    }
}

// Distances are not dense, so there are no levels to sweep: round 0's queue is every target, and round r
// walks its queue's entries edge-parallel (as dag_step_kernel) and lists for round r + 1 each tight entry u
// whose `on` byte it is first to set.  A row enters a queue once (a target's byte is set by the seed), so the
// rounds' queues lie one after the other in one [rows] array and the work is the DAG rows' entries.  How many
// rounds there are is not known up front: the host enqueues them in batches (SdBatches) and reads the ring
// once per batch; a round whose queue has no entries returns at once, and so does every round after it.
constexpr int kWdRing = 4;
template <class A>  // TightInt or TightF64
struct WdagRound {
    const int64_t* rp;
    const int32_t* col;
    const typename A::W* wt;
    const long long* dist;
    uint32_t* on;  // the `on` bytes as words (a byte is set with an atomic OR on its word)
    int32_t* vq;   // [rows] the rounds' queues, concatenated
    int64_t* qo;   // [rows + 1] each entry's first edge number inside its round
    unsigned long long* packed;  // [kWdRing] round r's queue: (rows << kPackShift) | entries, slot r % kWdRing
    int64_t* lbase;              // [kWdRing] its first queue slot
    unsigned long long* rounds;  // rounds whose queue had rows
    int32_t r;
};

// round 0's queue: the targets in row order, with their row lengths (scanned into qo by the host)
__global__ void wdag_queue0_kernel(const int64_t* __restrict__ idx, int64_t nt, const int64_t* __restrict__ rp,
                                   int32_t* __restrict__ vq, int64_t* __restrict__ len) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nt; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = idx[j];
        vq[j] = (int32_t)l;
        len[j] = rp[l + 1] - rp[l];
    }
}
template <class A>
__global__ void wdag_ring0_kernel(WdagRound<A> a, int64_t nt) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int k = 0; k < kWdRing; ++k) a.packed[k] = 0ull, a.lbase[k] = 0;
        a.packed[0] = ((unsigned long long)nt << kPackShift) | (unsigned long long)a.qo[nt];
        a.rounds[0] = 0ull;
    }
}

template <class A>
__global__ __launch_bounds__(kBlock) void wdag_round_kernel(WdagRound<A> a) {
    __shared__ WaveStage ws;
    const int cs = a.r % kWdRing, ns = (a.r + 1) % kWdRing;
    const unsigned long long pk = a.packed[cs];
    const int64_t nq = (int64_t)(pk >> kPackShift), mf = (int64_t)(pk & kEdgeMask);
    const int64_t base = a.lbase[cs], nbase = base + nq;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.lbase[ns] = nbase;
        a.packed[(a.r + 2) % kWdRing] = 0ull;  // round r + 1's output starts empty (no round reads or fills it now)
        if (nq > 0) a.rounds[0] += 1;
    }
    if (mf == 0) return;  // (grid-uniform) nothing left to walk: this round and every later one
    WaveApp app{ws};
    const int32_t* queue = a.vq + base;
    const int64_t* qoff = a.qo + base;
    int32_t* qout = a.vq + nbase;
    int64_t* qoout = a.qo + nbase;
    unsigned long long* pout = a.packed + ns;
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
                const int64_t j = a.rp[v] + cur.row_offset(e);
                u = a.col[j];
                if (A::tight(a.dist[u], a.wt[j], a.dist[v])) {
                    const uint32_t bit = 1u << ((u & 3) * 8);
                    if (!(a.on[u >> 2] & bit)) take = !(atomicOr(&a.on[u >> 2], bit) & bit);
                    if (take) deg = a.rp[u + 1] - a.rp[u];
                }
            }
            app.append(take, u, deg, qout, qoout, pout);
        }
    }
    app.final(qout, qoout, pout);
}

const Csr& reverse_csr(const Shard& sh, int dir) {
    return dir == JG_DIR_BOTH ? sh.both : dir == JG_DIR_OUT ? sh.in : sh.out;
}

template <class V>
void drop_held(Graph& g, HeldDag<V> Shard::*held) {
    for (auto& sp : g.shards) {
        DeviceGuard dg(*sp);
        (*sp).*held = HeldDag<V>{};
    }
}

// The checks every flavour makes before its family's own (`name`: the entry point, for the messages)
Shard& dag_only_shard(Graph& g, const std::string& name, bool edges, const char* sharded_hint = "") {
    if (edges && !(g.flags & JG_ADJ_EDGE_INDEX))
        fail(JG_ERR_UNSUPPORTED, name + "_edges: the graph was built without JG_ADJ_EDGE_INDEX");
    if (g.P != 1 || g.shards.size() != 1) fail(JG_ERR_UNSUPPORTED, name + " runs on one shard" + sharded_hint);
    return *g.shards[0];
}

// One run of either driver, begun after the family's checks: the remaining checks (`counters`: what the rows must
// fit, for the message), then the family's held DAG goes (`drop`) and the call's stats start empty.  start() and
// stop() bound the timed region: the target mask travels before it, stop() leaves its length in compute_ms.
// `on`: one byte per row, zeroed by start(), set by the seed (the targets) and the sweep (the DAG's other rows);
// compact() lists the rows whose byte is set, in row order, in idx, and returns their number.
struct DagRun {
    Shard& sh;
    jg_stats& last;
    DeviceGuard dg;
    hipStream_t st;
    int64_t rows;
    DevBuf<uint8_t> dtarget;
    Event t0, t1;
    DevBuf<uint32_t> on;  // the bytes as words (the sweeps set a byte with an atomic OR on its word)
    DevBuf<int64_t> idx, cpos, cscan;
    DagRun(Graph& g, Shard& shard, const std::string& name, const char* counters, void (*drop)(Graph&))
        : sh(shard), last(g.ctx->last), dg(sh), st(sh.stream), rows(sh.rows) {
        if (sh.rows != g.n || sh.dense_rows.size() < (size_t)std::max<int64_t>(sh.rows, 1))
            fail(JG_ERR_UNSUPPORTED, name + ": the shard does not hold every vertex");
        if (sh.rows >> (64 - kPackShift))
            fail(JG_ERR_UNSUPPORTED, name + ": too many rows for the " + counters + " counters");
        drop(g);
        last = jg_stats{};
    }
    void start(const uint8_t* target) {
        if (target) {  // one flag per vertex: the shard holds them all
            dtarget.alloc((size_t)rows);
            copy_h2d(dtarget.get(), target, (size_t)rows, st);
        }
        JG_HIP(hipEventRecord(t0, st));
        on.alloc((size_t)((rows + 3) / 4));
        JG_HIP(hipMemsetAsync(on.get(), 0, on.bytes(), st));
    }
    uint8_t* on8() const { return reinterpret_cast<uint8_t*>(on.get()); }
    int64_t compact() {
        if (!idx.size()) idx.alloc((size_t)rows);
        return prim::compact_indices(on8(), rows, idx.get(), cpos, cscan, st);
    }
    void stop() {
        JG_HIP(hipEventRecord(t1, st));
        JG_HIP(hipEventSynchronize(t1));
        float ms = 0;
        JG_HIP(hipEventElapsedTime(&ms, t0, t1));
        last.compute_ms = ms;
    }
};

// The emit of every flavour T, after the sweep left the DAG rows' `on` bytes set: the held DAG's buffers, from the
// plane `dep` whose largest value among the targets is `top` (dbits: its width).  nv, ne: the DAG's vertices and
// listed entries; mf: the entries its rows hold.
struct DagEmitted {
    int64_t nv, ne, mf, launches;
};
template <class T>
DagEmitted dag_emit(DagRun& run, const Csr& c, const typename T::Val* dep, typename T::Val top, int dbits,
                    typename T::Extra extra, HeldDag<typename T::Val>& held) {
    using V = typename T::Val;
    const Shard& sh = run.sh;
    hipStream_t st = run.st;
    int64_t launches = 0;
    const int64_t nv = run.compact();
    const DevBuf<int64_t>& idx = run.idx;
    DevBuf<uint64_t> vkey((size_t)nv);
    DevBuf<uint32_t> vval((size_t)nv);
    dag_keys_kernel<V><<<grid_for(nv), kBlock, 0, st>>>(idx.get(), nv, dep, top, vkey.get(), vval.get());
    JG_LAUNCH_CHECK();
    prim::radix_sort(vkey.get(), vval.get(), nv, dbits, st);
    DevBuf<int32_t> local((size_t)nv);
    DevBuf<int64_t> len((size_t)nv), qoff((size_t)nv + 1);
    held.vertex.alloc((size_t)nv);
    held.value.alloc((size_t)nv);
    held.off.alloc((size_t)nv + 1);
    dag_unpack_kernel<V><<<grid_for(nv), kBlock, 0, st>>>(vkey.get(), vval.get(), nv, top, c.row_ptr.get(),
                                                          sh.dense_rows.get(), local.get(), held.vertex.get(),
                                                          held.value.get(), len.get());
    JG_LAUNCH_CHECK();
    prim::exclusive_scan(len.get(), qoff.get(), nv, st);
    int64_t mf = 0;
    copy_d2h(&mf, qoff.get() + nv, sizeof(int64_t), st);
    DevBuf<int32_t> cnt((size_t)nv);
    JG_HIP(hipMemsetAsync(cnt.get(), 0, cnt.bytes(), st));
    const int64_t nranges = (mf + kDagRange - 1) / kDagRange;
    const size_t nr = (size_t)std::max<int64_t>(nranges, 1);
    DevBuf<int32_t> rfi(nr), rli(nr), rca(nr), rcl(nr);
    DagWalk<T> wk{extra, local.get(), held.value.get(), qoff.get(), nv, mf, nranges, c.row_ptr.get(), c.col.get(), dep,
                  sh.dense_rows.get(), cnt.get(), rfi.get(), rli.get(), rca.get(), rcl.get(), nullptr, nullptr,
                  T::kEdges ? c.eidx.get() : nullptr, nullptr};
    const unsigned walk_grid = grid_for(nranges, kBlock / kWave, 16384);
    if (mf > 0) {
        dag_count_kernel<T><<<walk_grid, kBlock, 0, st>>>(wk);
        JG_LAUNCH_CHECK();
        ++launches;
    }
    prim::exclusive_scan(cnt.get(), held.off.get(), nv, st);
    int64_t ne = 0;
    copy_d2h(&ne, held.off.get() + nv, sizeof(int64_t), st);
    held.pred.alloc((size_t)std::max<int64_t>(ne, 1));
    if (T::kEdges) held.edge.alloc((size_t)std::max<int64_t>(ne, 1));
    if (mf > 0) {
        wk.off = held.off.get();
        wk.pred = held.pred.get();
        wk.edge = held.edge.get();
        dag_fill_kernel<T><<<walk_grid, kBlock, 0, st>>>(wk);
        JG_LAUNCH_CHECK();
        ++launches;
    }
    return {nv, ne, mf, launches};
}

}  // namespace

void bfs_kept_dag_drop(Graph& g) { drop_held(g, &Shard::dag); }

// T: HopDag (jg_bfs_kept_dag) or HopEdgeDag (jg_bfs_kept_dag_edges).  Seed, sweep and the DAG's vertices do not
// depend on T; the count and fill passes do.
template <class T>
static void bfs_kept_dag_t(Graph& g, int s, const uint8_t* target, int64_t* nv_out, int64_t* ne_out,
                           int32_t* deepest_out) {
    Shard& sh = dag_only_shard(g, "jg_bfs_kept_dag", T::kEdges, " (sharded graphs: walk back on the host)");
    if (s < 0 || s >= g.kept_nsrc) fail(JG_ERR_ARG, "no kept depth row with that index (jg_bfs_keep)");
    const Csr& c = reverse_csr(sh, g.kept_dir);
    if (!c.present())
        fail(JG_ERR_UNSUPPORTED, "jg_bfs_kept_dag reads the reverse of the kept traversal's adjacency: not built");
    DagRun run(g, sh, "jg_bfs_kept_dag", "level", bfs_kept_dag_drop);
    hipStream_t st = run.st;
    const int64_t rows = run.rows;
    const int32_t* dep = sh.kept_depth.get() + (int64_t)s * rows;
    const auto finish = [&](int64_t nv, int64_t ne, int32_t deepest) {
        sh.dag.nv = nv;
        sh.dag.ne = ne;
        sh.dag.edges = T::kEdges;
        if (nv_out) *nv_out = nv;
        if (ne_out) *ne_out = ne;
        if (deepest_out) *deepest_out = deepest;
        run.last.levels = deepest;
        run.last.supersteps = deepest < 0 ? 0 : deepest;
    };
    if (rows == 0) return finish(0, 0, -1);
    run.start(target);

    // ---- seed ----
    DevBuf<int32_t> d_deepest(1);
    JG_HIP(hipMemsetAsync(d_deepest.get(), 0xff, sizeof(int32_t), st));
    dag_seed_kernel<<<grid_for(rows, kBlock, 2048), kBlock, 0, st>>>(dep, sh.dense_rows.get(), run.dtarget.get(), rows,
                                                                    run.on8(), d_deepest.get());
    JG_LAUNCH_CHECK();
    const int64_t nt = run.compact();
    if (nt == 0) {
        run.stop();
        finish(0, 0, -1);
        run.last.algorithmic_bytes = 10.0 * (double)rows;
        return;
    }
    int32_t deepest = -1;
    copy_d2h(&deepest, d_deepest.get(), sizeof(int32_t), st);
    const int dbits = std::max(bits_for((uint64_t)deepest), 1);
    DevBuf<uint64_t> tkey((size_t)nt);
    DevBuf<uint32_t> tval((size_t)nt);
    dag_keys_kernel<int32_t><<<grid_for(nt), kBlock, 0, st>>>(run.idx.get(), nt, dep, deepest, tkey.get(), tval.get());
    JG_LAUNCH_CHECK();
    prim::radix_sort(tkey.get(), tval.get(), nt, dbits, st);

    // ---- backward sweep: levels deepest + 1 (no frontier: it seeds the deepest level's queue) .. 1 ----
    DevBuf<int32_t> vq((size_t)rows);
    DevBuf<int64_t> qo((size_t)rows);
    DevBuf<unsigned long long> packed((size_t)deepest + 2);
    DevBuf<int64_t> lbase((size_t)deepest + 2);
    JG_HIP(hipMemsetAsync(packed.get(), 0, packed.bytes(), st));
    JG_HIP(hipMemsetAsync(lbase.get(), 0, lbase.bytes(), st));
    DagStep sp{c.row_ptr.get(), c.col.get(), dep, run.on.get(), vq.get(), qo.get(), packed.get(), lbase.get(),
               tkey.get(), tval.get(), nt, 0, deepest};
    const unsigned step_grid = grid_for(std::max<int64_t>(c.nnz / 4, rows), kBlock, 1024);
    for (int32_t d = deepest + 1; d >= 1; --d) {
        sp.d = d;
        dag_step_kernel<<<step_grid, kBlock, 0, st>>>(sp);
        JG_LAUNCH_CHECK();
    }

    const auto [nv, ne, mf, emit_launches] = dag_emit<T>(run, c, dep, deepest, dbits, {}, sh.dag);
    run.stop();
    finish(nv, ne, deepest);
    run.last.kernel_launches = (int64_t)deepest + 1 + emit_launches;
    run.last.edges_traversed = (double)mf;
    // Byte model.  Seed and the two compactions: 10 B per row (depth, dense index, mask and `on` byte), 9 B
    // per row per compaction (flag + position).  Each of the three walks (sweep, count, fill) reads a
    // DAG-row entry's column and probes its depth: 3 x 8 B per entry.  A DAG vertex costs ~64 B (two
    // sort records of 12 B read and written, queue entry, row_ptr pair, count, offset, outputs), an
    // emitted predecessor 8 B (dense probe + store).  The edge-listing DAG adds the ordinal: 4 B per walked
    // entry in the fill pass (the listed entries' ordinals, fetched by the line) and 4 B per emitted entry (its
    // store); the count pass reads no ordinal.
    run.last.algorithmic_bytes = 28.0 * (double)rows + 24.0 * (double)mf + 64.0 * (double)nv + 8.0 * (double)ne +
                                 (T::kEdges ? 4.0 * (double)mf + 4.0 * (double)ne : 0.0);
}

void bfs_kept_dag(Graph& g, int s, const uint8_t* target, int64_t* nv_out, int64_t* ne_out, int32_t* deepest_out,
                  bool edges) {
    if (edges) bfs_kept_dag_t<HopEdgeDag>(g, s, target, nv_out, ne_out, deepest_out);
    else bfs_kept_dag_t<HopDag>(g, s, target, nv_out, ne_out, deepest_out);
}

// The two readers of a held DAG `h` of shard sh; the exported names check first that the right one is held.
// Entries [off[first], off[first + count]) of `entries` (pred or edge):
template <class E>
static void dag_read_entries(const Shard& sh, const DevBuf<int64_t>& off, const DevBuf<E>& entries, int64_t first,
                             int64_t count, E* out) {
    int64_t b = 0, e = 0;
    copy_d2h(&b, off.get() + first, sizeof(int64_t), sh.stream);
    copy_d2h(&e, off.get() + first + count, sizeof(int64_t), sh.stream);
    copy_d2h(out, entries.get() + b, (size_t)(e - b) * sizeof(E), sh.stream);
}
// vertices [first, first + count): value_out takes the values as the DAG holds them, sizeof(V) bytes each
template <class V>
static void dag_read(const Shard& sh, const HeldDag<V>& h, int64_t first, int64_t count, int32_t* vertex_out,
                     void* value_out, int64_t* off_out, int32_t* pred_out) {
    if (first < 0 || count < 0 || first > h.nv || count > h.nv - first)
        fail(JG_ERR_ARG, "range outside the DAG's vertices");
    if (h.nv == 0) {
        if (off_out) off_out[0] = 0;
        return;
    }
    DeviceGuard dg(sh);
    hipStream_t st = sh.stream;
    if (vertex_out) copy_d2h(vertex_out, h.vertex.get() + first, (size_t)count * sizeof(int32_t), st);
    if (value_out) copy_d2h(value_out, h.value.get() + first, (size_t)count * sizeof(V), st);
    if (off_out) copy_d2h(off_out, h.off.get() + first, (size_t)(count + 1) * sizeof(int64_t), st);
    if (pred_out) dag_read_entries(sh, h.off, h.pred, first, count, pred_out);
}
// name: the entry point; built_by: the call that would have built an edge-listing DAG of this family
template <class V>
static void dag_read_edges(const Graph& g, const HeldDag<V>& h, const std::string& name, const std::string& built_by,
                           int64_t first, int64_t count, uint32_t* edge_out) {
    if (!(g.flags & JG_ADJ_EDGE_INDEX))
        fail(JG_ERR_UNSUPPORTED, name + ": the graph was built without JG_ADJ_EDGE_INDEX");
    if (h.nv < 0 || !h.edges) fail(JG_ERR_STATE, "no edge-listing " + built_by);
    if (first < 0 || count < 0 || first > h.nv || count > h.nv - first)
        fail(JG_ERR_ARG, "range outside the DAG's vertices");
    if (h.nv == 0 || count == 0 || !edge_out) return;
    const Shard& sh = *g.shards[0];
    DeviceGuard dg(sh);
    dag_read_entries(sh, h.off, h.edge, first, count, edge_out);
}
// The same entries as relation ids: Graph::edge_rel gathered through the held ordinals on the device, so only the
// ids cross to the host (parallel to pred_out, as the ordinals are)
template <class V>
static void dag_read_relations(const Graph& g, const HeldDag<V>& h, const std::string& name, const std::string& built_by,
                               int64_t first, int64_t count, int64_t* rel_out) {
    if (!g.has_edge_rel)
        fail(JG_ERR_UNSUPPORTED, name + ": the graph holds no relation ids (jg_builder_keep_relations)");
    if (h.nv < 0 || !h.edges) fail(JG_ERR_STATE, "no edge-listing " + built_by);
    if (first < 0 || count < 0 || first > h.nv || count > h.nv - first)
        fail(JG_ERR_ARG, "range outside the DAG's vertices");
    if (h.nv == 0 || count == 0 || !rel_out) return;
    const Shard& sh = *g.shards[0];
    DeviceGuard dg(sh);
    int64_t b = 0, e = 0;
    copy_d2h(&b, h.off.get() + first, sizeof(int64_t), sh.stream);
    copy_d2h(&e, h.off.get() + first + count, sizeof(int64_t), sh.stream);
    gather_edge_relations(g, h.edge.get() + b, e - b, rel_out);
}

void bfs_kept_dag_read(Graph& g, int64_t first, int64_t count, int32_t* vertex_out, int32_t* depth_out,
                       int64_t* off_out, int32_t* pred_out) {
    const Shard& sh = *g.shards[0];
    if (sh.dag.nv < 0) fail(JG_ERR_STATE, "no predecessor DAG is held (jg_bfs_kept_dag)");
    dag_read(sh, sh.dag, first, count, vertex_out, depth_out, off_out, pred_out);
}

void bfs_kept_dag_read_edges(Graph& g, int64_t first, int64_t count, uint32_t* edge_out) {
    dag_read_edges(g, g.shards[0]->dag, "jg_bfs_kept_dag_read_edges", "predecessor DAG is held (jg_bfs_kept_dag_edges)",
                   first, count, edge_out);
}

void bfs_kept_dag_read_relations(Graph& g, int64_t first, int64_t count, int64_t* rel_out) {
    dag_read_relations(g, g.shards[0]->dag, "jg_bfs_kept_dag_read_relations",
                       "predecessor DAG is held (jg_bfs_kept_dag_edges)", first, count, rel_out);
}

void sssp_kept_dag_drop(Graph& g) {
    drop_held(g, &Shard::wdag);
    g.wdag_f64 = false;
}

// T: TightDag (jg_sssp_kept_dag) or TightEdgeDag (jg_sssp_kept_dag_edges), as bfs_kept_dag_t; TightDagF64 /
// TightEdgeDagF64 over a plane of jg_sssp_keep_f64, where max_distance and farthest are the doubles' bit patterns
// (max_distance < 0: none; farthest -1: no target)
template <class T>
static void sssp_kept_dag_t(Graph& g, const uint8_t* target, int64_t max_distance, int64_t* nv_out, int64_t* ne_out,
                            int64_t* farthest_out) {
    using A = typename T::Arith;
    constexpr bool kF64 = std::is_same<A, TightF64>::value;
    Shard& sh = dag_only_shard(g, "jg_sssp_kept_dag", T::kEdges);
    if (!g.sssp_kept) fail(JG_ERR_STATE, "no distance plane is kept (jg_sssp_keep)");
    if (g.sssp_f64 != kF64)
        fail(JG_ERR_STATE, kF64 ? "the kept plane holds integers (jg_sssp_keep): use jg_sssp_kept_dag"
                                : "the kept plane holds doubles (jg_sssp_keep_f64): use jg_sssp_kept_dag_f64");
    const Csr& c = reverse_csr(sh, g.sssp_dir);
    if (!c.present() || A::weight_count(c) == 0)
        fail(JG_ERR_UNSUPPORTED,
             "jg_sssp_kept_dag reads the reverse of the kept direction's adjacency: not built, or built without weights");
    DagRun run(g, sh, "jg_sssp_kept_dag", "round", sssp_kept_dag_drop);
    hipStream_t st = run.st;
    const int64_t rows = run.rows;
    const long long* dist = sh.sssp_dist.get();
    const auto finish = [&](int64_t nv, int64_t ne, int64_t farthest, int64_t rounds) {
        sh.wdag.nv = nv;
        sh.wdag.ne = ne;
        sh.wdag.edges = T::kEdges;
        g.wdag_f64 = kF64;
        if (nv_out) *nv_out = nv;
        if (ne_out) *ne_out = ne;
        if (farthest_out) *farthest_out = farthest;
        run.last.levels = (int32_t)std::min<int64_t>(rounds, INT32_MAX);
        run.last.supersteps = run.last.levels;
    };
    if (rows == 0) return finish(0, 0, -1, 0);
    run.start(target);

    // ---- seed ----
    DevBuf<long long> d_far(1);
    JG_HIP(hipMemsetAsync(d_far.get(), 0xff, sizeof(long long), st));
    wdag_seed_kernel<A::kAbsent><<<grid_for(rows, kBlock, 2048), kBlock, 0, st>>>(
        dist, sh.dense_rows.get(), run.dtarget.get(), rows, (long long)max_distance, run.on8(), d_far.get());
    JG_LAUNCH_CHECK();
    const int64_t nt = run.compact();
    if (nt == 0) {
        run.stop();
        finish(0, 0, -1, 0);
        run.last.algorithmic_bytes = 14.0 * (double)rows;
        return;
    }
    long long farthest = -1;
    copy_d2h(&farthest, d_far.get(), sizeof(long long), st);
    const int dbits = std::max(bits_for((uint64_t)farthest), 1);

    // ---- backward sweep by rounds ----
    DevBuf<int32_t> vq((size_t)rows);
    DevBuf<int64_t> qo((size_t)rows + 1), len((size_t)rows);
    DevBuf<unsigned long long> ring((size_t)kWdRing + 1);
    DevBuf<int64_t> lbase((size_t)kWdRing);
    WdagRound<A> rd{c.row_ptr.get(), c.col.get(), A::weights(c), dist, run.on.get(), vq.get(), qo.get(), ring.get(),
                 lbase.get(), ring.get() + kWdRing, 0};
    wdag_queue0_kernel<<<grid_for(nt), kBlock, 0, st>>>(run.idx.get(), nt, c.row_ptr.get(), vq.get(), len.get());
    JG_LAUNCH_CHECK();
    prim::exclusive_scan(len.get(), qo.get(), nt, st);
    wdag_ring0_kernel<A><<<1, kWave, 0, st>>>(rd, nt);
    JG_LAUNCH_CHECK();
    const unsigned round_grid = grid_for(std::max<int64_t>(c.nnz / 4, rows), kBlock, 1024);
    int32_t r = 0;
    unsigned long long pk = 0;  // round r's queue (the first not yet enqueued): no entries = nothing left
    for (SdBatches b{16};;) {
        if (r > (1 << 30)) fail(JG_ERR_STATE, "the weighted DAG's round control did not terminate");
        for (int k = 0, batch = b.take(); k < batch; ++k, ++r) {
            rd.r = r;
            wdag_round_kernel<A><<<round_grid, kBlock, 0, st>>>(rd);
            JG_LAUNCH_CHECK();
        }
        copy_d2h(&pk, ring.get() + r % kWdRing, sizeof pk, st);
        if ((pk & kEdgeMask) == 0) break;
    }
    unsigned long long rounds = 0;  // rounds whose queue had rows: the launched ones', and a last edgeless queue
    copy_d2h(&rounds, ring.get() + kWdRing, sizeof rounds, st);
    if ((pk >> kPackShift) > 0) ++rounds;

    const auto [nv, ne, mf, emit_launches] = dag_emit<T>(run, c, dist, farthest, dbits, {A::weights(c)}, sh.wdag);
    run.stop();
    finish(nv, ne, farthest, (int64_t)rounds);
    run.last.kernel_launches = (int64_t)r + emit_launches;
    run.last.edges_traversed = (double)mf;
    // Byte model, as the hop DAG's with 8-byte distances and the weights.  Seed and the two compactions: 14 B
    // per row (distance, dense index, mask and `on` byte), 9 B per row per compaction (flag + position).  Each
    // of the three walks (sweep, count, fill) reads a DAG-row entry's column (4 B) and weight (4 B) and probes
    // its distance (8 B): 3 x 16 B per entry (the sweep also walks the source's row when it is a target, the
    // backward scan over a run of parallel edges re-reads cached lines: neither is counted).  A DAG vertex costs
    // ~72 B (two sort records of 12 B read and written, queue entry, row_ptr pair, count, offset, the 8-byte
    // distance and the other outputs), an emitted predecessor 8 B (dense probe + store).  The edge-listing DAG
    // adds the ordinal as the hop DAG's does: 4 B per walked entry in the fill pass, 4 B per emitted entry.
    // The f64 flavours read an 8-byte weight: 3 x 20 B per entry.
    run.last.algorithmic_bytes = 32.0 * (double)rows + (kF64 ? 60.0 : 48.0) * (double)mf + 72.0 * (double)nv +
                                 8.0 * (double)ne + (T::kEdges ? 4.0 * (double)mf + 4.0 * (double)ne : 0.0);
}

void sssp_kept_dag(Graph& g, const uint8_t* target, int64_t max_distance, int64_t* nv_out, int64_t* ne_out,
                   int64_t* farthest_out, bool edges) {
    if (edges) sssp_kept_dag_t<TightEdgeDag>(g, target, max_distance, nv_out, ne_out, farthest_out);
    else sssp_kept_dag_t<TightDag>(g, target, max_distance, nv_out, ne_out, farthest_out);
}

static int64_t f64_bits(double x) {
    int64_t b;
    std::memcpy(&b, &x, sizeof b);
    return b;
}

void sssp_kept_dag_f64(Graph& g, const uint8_t* target, double max_distance, int64_t* nv_out, int64_t* ne_out,
                       double* farthest_out, bool edges) {
    // inclusive on the sum; < 0 or NaN: none (0 is +0.0's pattern, whichever zero came in)
    const int64_t md = !(max_distance >= 0.0) ? -1 : max_distance == 0.0 ? 0 : f64_bits(max_distance);
    int64_t far = -1;
    if (edges) sssp_kept_dag_t<TightEdgeDagF64>(g, target, md, nv_out, ne_out, &far);
    else sssp_kept_dag_t<TightDagF64>(g, target, md, nv_out, ne_out, &far);
    if (farthest_out) {
        double f = -1.0;
        if (far >= 0) std::memcpy(&f, &far, sizeof f);
        *farthest_out = f;
    }
}

void sssp_kept_dag_read(Graph& g, int64_t first, int64_t count, int32_t* vertex_out, int64_t* dist_out,
                        int64_t* off_out, int32_t* pred_out) {
    const Shard& sh = *g.shards[0];
    if (sh.wdag.nv < 0) fail(JG_ERR_STATE, "no weighted predecessor DAG is held (jg_sssp_kept_dag)");
    if (g.wdag_f64) fail(JG_ERR_STATE, "the held weighted DAG has double distances: read it with jg_sssp_kept_dag_read_f64");
    dag_read(sh, sh.wdag, first, count, vertex_out, dist_out, off_out, pred_out);
}

void sssp_kept_dag_read_f64(Graph& g, int64_t first, int64_t count, int32_t* vertex_out, double* dist_out,
                            int64_t* off_out, int32_t* pred_out) {
    const Shard& sh = *g.shards[0];
    if (sh.wdag.nv < 0) fail(JG_ERR_STATE, "no weighted predecessor DAG is held (jg_sssp_kept_dag_f64)");
    if (!g.wdag_f64) fail(JG_ERR_STATE, "the held weighted DAG has integer distances: read it with jg_sssp_kept_dag_read");
    dag_read(sh, sh.wdag, first, count, vertex_out, dist_out, off_out, pred_out);
}

void sssp_kept_dag_read_edges(Graph& g, int64_t first, int64_t count, uint32_t* edge_out) {
    dag_read_edges(g, g.shards[0]->wdag, "jg_sssp_kept_dag_read_edges",
                   "weighted predecessor DAG is held (jg_sssp_kept_dag_edges)", first, count, edge_out);
}

void sssp_kept_dag_read_relations(Graph& g, int64_t first, int64_t count, int64_t* rel_out) {
    dag_read_relations(g, g.shards[0]->wdag, "jg_sssp_kept_dag_read_relations",
                       "weighted predecessor DAG is held (jg_sssp_kept_dag_edges)", first, count, rel_out);
}

}  // namespace jg
