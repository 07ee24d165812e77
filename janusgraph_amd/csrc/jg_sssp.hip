// jg_sssp.hip — hop-bounded weighted shortest distance (ShortestDistanceVertexProgram).
//
// Reference semantics:
//   ShortestDistanceVertexProgram (janusgraph-backend-testutils/.../olap/
//   ShortestDistanceVertexProgram.java:112-146, combiner ShortestDistanceMessageCombiner.java:29-31):
//   v pulls over its OUT edges the targets' previous-superstep messages + edge weight, keeps the
//   minimum, forwards on improvement; supersteps 0..maxDepth => min over paths of <= maxDepth hops.
//
// Engines (shortest_distance_run chooses): frontier Bellman-Ford supersteps with exact snapshot semantics
//   (messages of superstep t-1 only: push over the in-CSR with 64-bit atomicMin into a scratch array, then
//   apply), on one shard or sharded over the IN halo plan; delta-stepping when the hop bound cannot bind
//   and no weight is negative; unit weights on one shard: the DO-BFS of jg_traverse.hip (bfs_in_depths).
// jg_sssp_keep (sssp_keep, at the end): the delta-stepping engine over the adjacency of a direction, its
//   distances left on the device for the weighted predecessor DAG of jg_pathdag.hip (ShortestPathVertexProgram
//   with a distanceProperty).
// jg_graph_set_weights_f64 / jg_sssp_keep_f64 (after it): the same engine over double weights, a third flavour of
//   its templates (SdF64): distances as the bit patterns of non-negative doubles, the same integer atomicMin.
#include <cfloat>
#include <climits>
#include <cmath>

#include "jg_frontier.h"
#include "jg_internal.h"
#include "jg_scatter.h"

namespace jg {

namespace {

// ---------------- weighted shortest distance (frontier Bellman-Ford) ----------------
// An edge without the weight property carries kWeightAbsent: a message crossing it is an error, as
// in Fulgora; distances may be negative, so an absent DISTANCE is reported as INT64_MIN.
constexpr int32_t kWeightAbsent = INT32_MIN;

// The relax walk of the three edge-parallel kernels: the edges of a queue's rows (EdgeCursor: nq rows,
// their first edge numbers qoff, mf edges in all), tile by tile over the grid, kTdEdgesPerThread
// consecutive edges per thread after one binary search; a workgroup whose slice of a tile is past the end
// leaves.  A slot with an edge w -> u whose weight wk is present gets take = relax(w, u, wk), in its lane
// alone; then every slot calls append(u, take) wave-uniformly (the appends inside it are wave-uniform
// calls).  A slot past mf, or an edge without the weight (which sets *err), comes there with "no edge":
// a value-initialised take (nothing to append).
// bdim (here and in the helpers below) is blockDim.x as the kernel reads it: there the compiler folds it to
// the launch's uniform group size, in an inlined helper it stays a compare, a select and a load per wave.
// W: the weights' type, int32 (kWeightAbsent: the edge lacks the property) or double (jg_sssp_keep_f64: the
// weights of jg_graph_set_weights_f64, never absent).
template <class W>
struct SdWalkT {
    const int64_t* rp;
    const int32_t* col;
    const W* wt;  // null: unit weights
    const int32_t* queue;
    const int64_t* qoff;
    int64_t nq, mf;
    int32_t* err;
};
using SdWalk = SdWalkT<int32_t>;
__device__ __forceinline__ bool sd_weight_absent(int32_t w) { return w == kWeightAbsent; }
__device__ __forceinline__ bool sd_weight_absent(double) { return false; }
template <class W, class Relax, class Append>
__device__ __forceinline__ void sd_relax_walk(const SdWalkT<W>& q, unsigned bdim, Relax&& relax, Append&& append) {
    const int64_t nthreads = (int64_t)gridDim.x * bdim;
    const int64_t tid = (int64_t)blockIdx.x * bdim + threadIdx.x;
    const int64_t per_tile = nthreads * kTdEdgesPerThread;
    const int64_t tiles = (q.mf + per_tile - 1) / per_tile;
    for (int64_t t = 0; t < tiles; ++t) {
        if ((t * nthreads + (int64_t)blockIdx.x * bdim) * kTdEdgesPerThread >= q.mf) break;  // block-uniform
        const int64_t e0 = (t * nthreads + tid) * kTdEdgesPerThread;
        EdgeCursor cur{q.qoff, q.nq, q.mf};
        if (e0 < q.mf) cur.seek(e0);
#pragma unroll
        for (int k = 0; k < kTdEdgesPerThread; ++k) {
            const int64_t e = e0 + k;
            decltype(relax(0, 0, W(0))) take{};
            int32_t u = 0;
            if (e < q.mf) {
                cur.advance(e);
                const int32_t w = q.queue[cur.i];
                const int64_t j = q.rp[w] + cur.row_offset(e);
                u = q.col[j];
                const W wk = q.wt ? q.wt[j] : W(1);
                // the edge function would throw (ShortestDistanceVertexProgram.java:69)
                if (sd_weight_absent(wk)) *q.err = 1;
                else take = relax(w, u, wk);
            }
            append(u, take);
        }
    }
}

// A superstep's relax, one shard or many: a candidate that beats the best so far takes the atomicMin, and
// the lane that finds the row untouched lists it.  kOwnOnly (sharded): targets are compact positions, and
// only own rows (position >> tbits == 0) are listed; a peer's row keeps its candidate in its halo slot.
template <bool kOwnOnly>
__device__ __forceinline__ void sd_push_relax(const SdWalk& q, unsigned bdim, const long long* msg, long long* best, int tbits,
                                              int32_t* touched, unsigned long long* tsize) {
    sd_relax_walk(q, bdim,
        [=](int32_t w, int32_t u, int32_t wk) {
            const long long cand = msg[w] + (long long)wk;
            // a read first (past L1, as in sd_near_kernel): a candidate no better than the best so far
            // takes no atomic
            if (cand >= __hip_atomic_load(&best[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
            const bool first = atomicMin(&best[u], cand) == LLONG_MAX;
            return kOwnOnly ? first && (u >> tbits) == 0 : first;
        },
        [=](int32_t u, bool first) { wave_append(first, u, touched, tsize); });
}

// A superstep's apply: touched rows whose candidate beats their distance take it and form the next
// frontier, with its first edge numbers (for the next push)
__device__ __forceinline__ void sd_apply_rows(WaveStage& ws, unsigned bdim, const int32_t* __restrict__ touched, int64_t tsize,
                                              long long* __restrict__ best, long long* __restrict__ dist,
                                              long long* __restrict__ msg, const int64_t* __restrict__ rp,
                                              int32_t* next_frontier, int64_t* next_qoff, unsigned long long* packed) {
    WaveApp app{ws};
    const int64_t stride = (int64_t)gridDim.x * bdim;
    for (int64_t x0 = (int64_t)blockIdx.x * bdim; x0 < tsize; x0 += stride) {  // block-uniform trips
        const int64_t i = x0 + threadIdx.x;
        bool improved = false;
        int32_t u = 0;
        int64_t du = 0;
        if (i < tsize) {
            u = touched[i];
            const long long b = best[u];
            best[u] = LLONG_MAX;
            if (dist[u] == LLONG_MIN || dist[u] > b) {
                dist[u] = b;
                msg[u] = b;
                improved = true;
                du = rp[u + 1] - rp[u];
            }
        }
        app.append(improved, u, du, next_frontier, next_qoff, packed);
    }
    app.final(next_frontier, next_qoff, packed);
}

// A superstep edge-balanced: the frontier carries each row's first edge number
// (qoff), and each thread takes kTdEdgesPerThread consecutive edges of the whole frontier after one
// binary search, so a hub row's 10^5 in-entries are spread over the grid instead of holding one lane
// group for the superstep (RMAT-20, weights 1..255, unbounded: 15.8 ms with the lane groups).
//
// The supersteps are controlled on the device (round 6, as the delta-stepping steps): superstep t's push
// and apply take the frontier count from a ring the previous apply filled, and its state (done, the
// superstep count) from the push's decision; the host enqueues supersteps in batches and reads the state
// once per batch instead of twice per superstep.
constexpr int kSdRing = 4;  // decision / counter rings of the device-controlled SD loops
struct SdSuper {      // superstep t's decision, ring slot t % kSdRing
    int32_t done;     // no superstep from t on
    int32_t levels;   // the supersteps counted so far (as the host loop counted them)
};
struct SdPush {
    const int64_t* rp;
    const int32_t* col;
    const int32_t* wt;
    int32_t* frontier[2];         // superstep t reads frontier[t & 1] (+ qoff), its apply writes [(t + 1) & 1]
    int64_t* qoff[2];
    unsigned long long* fr;       // [kSdRing] superstep t's frontier, packed (rows << kPackShift) | edges
    unsigned long long* tsz;      // [kSdRing] rows superstep t touched
    SdSuper* st;                  // [kSdRing]
    long long* msg;
    long long* best;
    long long* dist;
    int32_t* touched;
    int32_t* err;
    int32_t t;
};
__device__ __forceinline__ SdSuper sd_super_decide(const SdPush& a, int64_t* nq, int64_t* mf) {
    const SdSuper p = a.st[(a.t + kSdRing - 1) % kSdRing];
    const unsigned long long h = a.fr[a.t % kSdRing];
    *nq = (int64_t)(h >> kPackShift);
    *mf = (int64_t)(h & kEdgeMask);
    SdSuper c = p;
    if (p.done) return c;
    if (*nq == 0) {
        c.done = 1;
    } else if (*mf == 0) {  // the frontier's rows have no entries: the superstep sends nothing, the run ends
        c.done = 1;
        c.levels = a.t;
    } else {
        c.levels = a.t;
    }
    return c;
}
__global__ __launch_bounds__(kBlock) void sd_push_q_kernel(SdPush a) {
    __shared__ SdSuper s_c;
    __shared__ int64_t s_nq, s_mf;
    if (threadIdx.x == 0) {
        int64_t nq, mf;
        s_c = sd_super_decide(a, &nq, &mf);
        s_nq = nq;
        s_mf = mf;
        if (blockIdx.x == 0) {
            a.st[a.t % kSdRing] = s_c;
            if (!s_c.done) {  // the apply's next frontier and the next push's touched count start at zero
                a.fr[(a.t + 1) % kSdRing] = 0ull;
                a.tsz[(a.t + 1) % kSdRing] = 0ull;
            }
        }
    }
    __syncthreads();
    if (s_c.done) return;
    const SdWalk q{a.rp, a.col, a.wt, a.frontier[a.t & 1], a.qoff[a.t & 1], s_nq, s_mf, a.err};
    sd_push_relax<false>(q, blockDim.x, a.msg, a.best, 0, a.touched, a.tsz + a.t % kSdRing);
}

// The apply of a superstep (sd_apply_rows), the superstep's state and counts from the rings
__global__ __launch_bounds__(kBlock) void sd_apply_q_kernel(SdPush a) {
    __shared__ WaveStage ws;
    if (a.st[a.t % kSdRing].done) return;
    sd_apply_rows(ws, blockDim.x, a.touched, (int64_t)a.tsz[a.t % kSdRing], a.best, a.dist, a.msg, a.rp, a.frontier[(a.t + 1) & 1],
                  a.qoff[(a.t + 1) & 1], a.fr + (a.t + 1) % kSdRing);
}

// ---------------- weighted shortest distance, unbounded hops (near-far delta-stepping) ----------------
// When the hop bound cannot bind (maxDepth >= rows - 1) and no weight is negative, the hop-bounded
// minimum is the plain shortest distance (a shortest path can be taken simple: <= rows - 1 hops), so
// the supersteps can be replaced by delta-stepping (Meyer & Sanders; the GPU
// near-far pile of Davidson et al.): the rows below the threshold T are relaxed pass by pass (the near
// queue), the rest wait in a far pile, and T rises by delta once the near queue is empty.  The frontier
// Bellman-Ford above re-relaxes a row every time a longer-hop path improves it; here a row is relaxed
// only while its distance is below T, so most rows are relaxed once.  The reported distances are the
// Bellman-Ford ones bit for bit (integers, a min); an absent weight on an edge out of a reached row
// fails the run as there (every reached row is relaxed at least once, at its final distance).
// Queues hold each row at most once: near entries by a pass stamp, far entries by a flag.
//
// The passes are controlled on the device (round 6): a step is sd_split_kernel (which moves the far pile
// when the near queue came out empty) and sd_near_kernel (one near pass); both take the step's decision
// from the state ring and the previous step's counters, as the DO-BFS levels do, and the host enqueues
// steps in batches and reads the state once per batch.  (A host read per pass cost ~50 us of every pass:
// RMAT-22, 10 passes, 0.5 of 3.0 ms.)
struct SdState {     // a step's decision, ring slot = step % kSdRing
    long long T;     // the threshold: the near pass relaxes rows below it
    int32_t fc;      // the far pile rows join (far[fc], its size fsz[fc])
    int32_t split;   // this step moved the far pile before its near pass
    int32_t done;
    int32_t end_step;  // done: the step that found nothing left
};

// Distances are 64-bit, or 32-bit when every distance the run can store fits (sd_delta_stepping: a row's
// first distance is a path of at most rows - 1 entries, later ones only fall): half the bytes per
// random distance read and atomicMin, so twice the rows per cached line.
template <class D> struct DistTraits;
template <> struct DistTraits<long long> { static constexpr long long kNone = LLONG_MAX; };
template <> struct DistTraits<unsigned int> { static constexpr unsigned int kNone = UINT_MAX; };

// The arithmetic of a run.  SdInt: integer distances and weights.  SdF64 (jg_sssp_keep_f64): the distances are
// doubles >= 0 held as their bit patterns in a long long plane: such patterns order, as signed integers, exactly
// as the doubles do, so the prefilter load, the atomicMin, the far-pile minimum and every threshold compare are
// the integer ones and only the add (and the threshold's arithmetic) goes through double.  A threshold
// (SdState::T) is held the same way.  No float atomic: nothing depends on the order candidates arrive in.
struct SdInt {
    using W = int32_t;
    using Delta = long long;
    template <class D> static constexpr __host__ __device__ D none() { return DistTraits<D>::kNone; }
    static constexpr long long kPlaneAbsent = LLONG_MIN;
    static constexpr bool kSync = false;  // a near pass relaxes a row from its distance as the lane finds it
    static __device__ __forceinline__ long long add(long long d, int32_t w) { return d + (long long)w; }
    static __host__ __device__ __forceinline__ long long first_threshold(long long delta) { return delta; }
    // past the previous threshold by delta, or to the bucket of the smallest far distance m when that lies
    // further (has_m: a far distance was seen)
    static __device__ __forceinline__ long long next_threshold(long long T, bool, bool has_m, unsigned long long m,
                                                               long long delta) {
        long long t2 = T + delta;
        if (has_m) {
            const long long jump = ((long long)m / delta + 1) * delta;
            t2 = jump > t2 ? jump : t2;
        }
        return t2;
    }
    static const int32_t* weights(const Csr& c) { return c.weight.get(); }
};
constexpr long long kF64InfBits = 0x7FF0000000000000ll;  // +Inf: unreached
struct SdF64 {
    using W = double;
    using Delta = double;
    // +Inf's pattern: above every finite distance, and an infinite candidate never replaces it
    template <class D> static constexpr __host__ __device__ D none() { return (D)kF64InfBits; }
    static constexpr long long kPlaneAbsent = kF64InfBits;
    // The same distances come out of any interleaving, but how many near passes it takes does not: a lane that
    // reads dist[w] while another lane lowers it relaxes from either value, and the far minimum the near passes
    // collect holds whatever candidates happened to win.  This route promises the same stats.levels on every run,
    // so its passes are synchronous: a pass relaxes its queue's rows from their distances as they stood before the
    // pass (sd_snap_kernel copies them out first), which makes the distances after every pass, the next queue as
    // a set and the rows of the far pile at or above the threshold functions of the input alone; and the
    // threshold moves by the far pile's exact minimum only (below).
    static constexpr bool kSync = true;
    static __device__ __forceinline__ long long add(long long d, double w) {
        return __double_as_longlong(__longlong_as_double(d) + w);
    }
    static __host__ __device__ __forceinline__ long long first_threshold(double delta) {
        long long b;
        __builtin_memcpy(&b, &delta, sizeof b);
        return b;
    }
    // As SdInt's, in double: (floor(m / delta) + 1) * delta.  Rounding may leave that at or below m, or T + delta
    // at T; the threshold must pass m (so that the split moves the row at m) and strictly rise, so it is
    // lifted to the next double after m, or after T, where it does not.
    // m is used only when the step before was itself a split (prev_split): then m is the smallest distance of
    // the rows that split kept, read while no kernel changes a distance, the pile's exact minimum.  (What the
    // near passes see on the way holds candidates that won an atomicMin and were beaten later: which of them
    // do depends on timing, so SdF64's near pass does not collect them.)  A threshold change thus first tries
    // T + delta and, when that bucket holds no row with entries, jumps with the next step.
    static __device__ __forceinline__ long long next_threshold(long long T, bool prev_split, bool has_m,
                                                               unsigned long long m, double delta) {
        const double t = __longlong_as_double(T);
        double t2 = t + delta;
        long long b2 = __double_as_longlong(t2);
        if (prev_split && has_m) {
            const double dm = __longlong_as_double((long long)m);
            const double jump = (floor(dm / delta) + 1.0) * delta;
            t2 = jump > t2 ? jump : t2;
            b2 = __double_as_longlong(t2);
            if (b2 <= (long long)m) b2 = (long long)m + 1;  // the next double after m (m is finite)
        }
        if (b2 <= T) b2 = T + 1;
        return b2 > kF64InfBits ? kF64InfBits : b2;
    }
    static const double* weights(const Csr& c) { return c.wf.get(); }
};

template <class D, class A = SdInt>
struct SdStep {
    const int64_t* rp;
    const int32_t* col;
    const typename A::W* wt;
    D* dist;                    // A::none<D>(): unreached
    D* snap;                    // A::kSync: the near queue's rows' distances before the pass (by row); else null
    int32_t* nq[2];             // near queues: step s relaxes nq[s & 1] (and its first-edge offsets qo),
    int64_t* qo[2];             // its near pass appends to nq[(s + 1) & 1]
    unsigned long long* nctr;   // [kSdRing] step s's near queue as the near pass before it left it, packed
                                //   (rows << kPackShift) | edges
    unsigned long long* sctr;   // [kSdRing] the near queue step s's split filled instead (same packing)
    int32_t* far[2];            // far piles and their sizes
    unsigned long long* fsz;    // [2]
    int32_t* far_flag;
    int32_t* stamp;             // near-queue stamps (pass = step + 1)
    unsigned long long* fmin;   // [kSdRing] smallest distance seen in the far pile up to step s
    SdState* st;                // [kSdRing]
    unsigned long long* passes; // near passes run (a near queue with rows)
    int32_t* err;
    typename A::Delta delta;
    int32_t step;
};

// Step s's decision: relax the near queue when it has entries; else stop when the far pile is empty; else
// move the far pile, with the threshold past the previous one by delta, or to the bucket of the smallest far
// distance seen when that lies further (the host version's two split attempts; any threshold sequence gives
// the same distances, the bucket only decides how much is relaxed again).
// Invariant: the decision reads only what no kernel of step s writes, so every workgroup of
// sd_split_kernel computes the same one however late it starts: st[s - 1] and fmin[s - 1] (step s - 1's),
// nctr[s] (appended to by step s - 1's near pass alone; step s's split appends to sctr[s], which is not read
// here), and fsz[p.fc] (step s's split appends to fsz[p.fc ^ 1]; its near pass runs after every split
// workgroup has decided).  A split that appended to nctr[s] let a late workgroup see entries, decide
// "no split" and leave its part of the far pile where it was.
template <class D, class A>
__device__ SdState sd_decide(const SdStep<D, A>& a) {
    const int ps = (a.step + kSdRing - 1) % kSdRing;
    const SdState p = a.st[ps];
    SdState c = p;
    c.split = 0;
    if (p.done) return c;
    if ((a.nctr[a.step % kSdRing] & kEdgeMask) > 0) return c;
    if (a.fsz[p.fc] == 0) {
        c.done = 1;
        c.end_step = a.step;
        return c;
    }
    const unsigned long long m = a.fmin[ps];
    c.T = A::next_threshold(p.T, p.split != 0, m != ULLONG_MAX, m, a.delta);
    c.fc = p.fc ^ 1;
    c.split = 1;
    return c;
}

// The far pile at a threshold change: rows now below T join the step's near queue, rows below the previous
// threshold were relaxed at their final distance already (dropped), the others stay (their smallest
// distance goes to fmin[step]).
template <class D, class A>
__global__ __launch_bounds__(kBlock) void sd_split_kernel(SdStep<D, A> a) {
    __shared__ SdState s_st;
    __shared__ long long s_tprev;
    __shared__ WaveStage ws;
    if (threadIdx.x == 0) {
        s_st = sd_decide(a);
        s_tprev = a.st[(a.step + kSdRing - 1) % kSdRing].T;
        if (blockIdx.x == 0) a.st[a.step % kSdRing] = s_st;
    }
    __syncthreads();
    if (!s_st.split) return;
    WaveApp app{ws};
    const int from = s_st.fc ^ 1;
    const int64_t fsize = (int64_t)a.fsz[from];
    const int32_t* __restrict__ far = a.far[from];
    const long long T = s_st.T, t_prev = s_tprev;
    int32_t* nq = a.nq[a.step & 1];
    int64_t* qo = a.qo[a.step & 1];
    unsigned long long* packed = a.sctr + a.step % kSdRing;  // not nctr: sd_decide reads that one
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long mk = ULLONG_MAX;
    for (int64_t x0 = (int64_t)blockIdx.x * blockDim.x; x0 < fsize; x0 += stride) {  // block-uniform trips
        const int64_t i = x0 + threadIdx.x;
        bool to_near = false, keep = false;
        int32_t u = 0;
        int64_t du = 0;
        if (i < fsize) {
            u = far[i];
            const long long d = (long long)a.dist[u];
            keep = d >= T;
            to_near = !keep && d >= t_prev;
            if (keep) mk = (unsigned long long)d < mk ? (unsigned long long)d : mk;
            else a.far_flag[u] = 0;
            if (to_near) du = a.rp[u + 1] - a.rp[u];
        }
        app.append(to_near, u, du, nq, qo, packed);
        wave_append(keep, u, a.far[s_st.fc], a.fsz + s_st.fc);
    }
    app.final(nq, qo, packed);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(mk, o, kWave);
        mk = t < mk ? t : mk;
    }
    if (lane_id() == 0 && mk != ULLONG_MAX) atomicMin(a.fmin + a.step % kSdRing, mk);
}

// One near pass, edge-balanced over the step's near queue (first-edge numbers, one binary search per 4
// edges per thread): after a split the queue the split filled (sctr; the rows the pass before left in nctr
// have no entries, or the step would not have split, so the split wrote over them from slot 0 and only their
// count is kept, for `passes`).  Block 0 also keeps the rings: the next step's output counters and far
// minimum start empty, the far minimum carries over a step without a split, and after a split the emptied
// pile's size is reset.
template <class D, class A>
__global__ __launch_bounds__(kBlock) void sd_near_kernel(SdStep<D, A> a) {
    __shared__ SdState s_st;
    __shared__ long long s_nq, s_mf;
    __shared__ WaveStage ws;
    const int cs = a.step % kSdRing;
    if (threadIdx.x == 0) {
        s_st = a.st[cs];
        const unsigned long long h = s_st.split ? a.sctr[cs] : a.nctr[cs];
        s_nq = (long long)(h >> kPackShift);
        s_mf = (long long)(h & kEdgeMask);
        const long long left = s_st.split ? (long long)(a.nctr[cs] >> kPackShift) : 0;  // edgeless rows
        if (blockIdx.x == 0 && !s_st.done) {
            a.nctr[(a.step + 2) % kSdRing] = 0ull;
            a.sctr[(a.step + 2) % kSdRing] = 0ull;
            a.fmin[(a.step + 2) % kSdRing] = ULLONG_MAX;
            if (s_st.split) a.fsz[s_st.fc ^ 1] = 0ull;
            else if (!A::kSync) atomicMin(a.fmin + cs, a.fmin[(a.step + kSdRing - 1) % kSdRing]);
            if (s_nq + left > 0) a.passes[0] += 1;  // (as the host-driven passes counted: a queue with rows)
        }
    }
    __syncthreads();
    if (s_st.done || s_mf == 0) return;
    WaveApp app{ws};
    const int64_t nq = s_nq, mf = s_mf;
    const long long T = s_st.T;
    const int32_t pass = a.step + 1;
    const int32_t* __restrict__ near = a.nq[a.step & 1];
    const int64_t* __restrict__ qoff = a.qo[a.step & 1];
    int32_t* near_next = a.nq[(a.step + 1) & 1];
    int64_t* qoff_next = a.qo[(a.step + 1) & 1];
    unsigned long long* packed = a.nctr + (a.step + 1) % kSdRing;
    int32_t* far = a.far[s_st.fc];
    unsigned long long* far_size = a.fsz + s_st.fc;
    unsigned long long fm = ULLONG_MAX;  // this lane's smallest distance that stays in the far pile
    struct Take { bool to_near, to_far; int64_t du; };  // where a relaxed row goes (du: its push degree)
    sd_relax_walk(
        SdWalkT<typename A::W>{a.rp, a.col, a.wt, near, qoff, nq, mf, a.err}, blockDim.x,
        [&](int32_t w, int32_t u, typename A::W wk) {
            Take r{};
            // dist[w] now: it only fell since w was queued
            const long long nd = A::add((long long)(A::kSync ? a.snap[w] : a.dist[w]), wk);
            // the prefilter reads past L1 (agent scope): a hub row's entry is hit from every XCD at
            // once, and a stale L1 copy would send each of those lanes to the atomic
            if (nd < (long long)__hip_atomic_load(&a.dist[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &&
                nd < (long long)atomicMin(&a.dist[u], (D)nd)) {
                if (nd < T) {
                    r.to_near = atomicExch(&a.stamp[u], pass) != pass;
                    if (r.to_near) r.du = a.rp[u + 1] - a.rp[u];
                } else {
                    r.to_far = atomicExch(&a.far_flag[u], 1) == 0;
                    fm = (unsigned long long)nd < fm ? (unsigned long long)nd : fm;
                }
            }
            return r;
        },
        [&](int32_t u, const Take& r) {
            app.append(r.to_near, u, r.du, near_next, qoff_next, packed);
            wave_append(r.to_far, u, far, far_size);
        });
    app.final(near_next, qoff_next, packed);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_xor(fm, o, kWave);
        fm = x < fm ? x : fm;
    }
    if (!A::kSync && lane_id() == 0 && fm != ULLONG_MAX) atomicMin(a.fmin + cs, fm);
}

// A::kSync: the distances of the step's near queue's rows as they stand before its near pass (between the step's
// split and near kernels; the queue and its size as sd_near_kernel finds them)
template <class D, class A>
__global__ __launch_bounds__(kBlock) void sd_snap_kernel(SdStep<D, A> a) {
    const int cs = a.step % kSdRing;
    const SdState st = a.st[cs];
    if (st.done) return;
    const unsigned long long h = st.split ? a.sctr[cs] : a.nctr[cs];
    const int64_t nq = (int64_t)(h >> kPackShift);
    const int32_t* __restrict__ near = a.nq[a.step & 1];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t w = near[i];
        a.snap[w] = a.dist[w];
    }
}

// The superstep start: distances absent, best empty, the seed at 0 as superstep 1's frontier.
__global__ void sd_super_init_kernel(SdPush a, int64_t rows, int32_t seed) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        a.dist[i] = i == seed ? 0ll : LLONG_MIN;
        a.best[i] = LLONG_MAX;
        if (i == seed) a.msg[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.frontier[1][0] = seed;
        a.qoff[1][0] = 0;
        for (int k = 0; k < kSdRing; ++k) {
            a.fr[k] = 0ull;
            a.tsz[k] = 0ull;
        }
        a.fr[1 % kSdRing] = (1ull << kPackShift) | (unsigned long long)(a.rp[seed + 1] - a.rp[seed]);
        a.st[0] = SdSuper{0, 0};
        *a.err = 0;
    }
}

// The start: every row unreached, no stamps or far flags, the seed at 0 as step 0's near queue, the ring
// empty, the state before step 0: threshold delta, far pile 0.
template <class D, class A>
__global__ void sd_init_kernel(SdStep<D, A> a, int64_t rows, int32_t seed) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        a.dist[i] = i == seed ? (D)0 : A::template none<D>();
        a.stamp[i] = 0;
        a.far_flag[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.nq[0][0] = seed;
        a.qo[0][0] = 0;
        a.nctr[0] = (1ull << kPackShift) | (unsigned long long)(a.rp[seed + 1] - a.rp[seed]);
        for (int k = 1; k < kSdRing; ++k) a.nctr[k] = 0ull;
        for (int k = 0; k < kSdRing; ++k) a.sctr[k] = 0ull;
        for (int k = 0; k < kSdRing; ++k) a.fmin[k] = ULLONG_MAX;
        a.fsz[0] = a.fsz[1] = 0ull;
        a.passes[0] = 0ull;
        *a.err = 0;
        SdState s0{};
        s0.T = A::first_threshold(a.delta);
        a.st[kSdRing - 1] = s0;
    }
}

// Weight statistics of a CSR for the delta-stepping gate and its automatic delta: [0] the smallest
// weight, [1] the sum, [2] the count, [3] the largest (absent weights excluded).
__global__ void sd_weight_stats_kernel(const int32_t* __restrict__ wt, int64_t nnz, long long* __restrict__ out) {
    long long mn = LLONG_MAX, mx = LLONG_MIN, sum = 0, cnt = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * blockDim.x) {
        const int32_t w = wt[j];
        if (w == kWeightAbsent) continue;
        mn = w < mn ? w : mn;
        mx = w > mx ? w : mx;
        sum += w;
        ++cnt;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const long long a = __shfl_xor(mn, o, kWave), b = __shfl_xor(mx, o, kWave);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        sum += __shfl_xor(sum, o, kWave);
        cnt += __shfl_xor(cnt, o, kWave);
    }
    if (lane_id() == 0) {
        atomicMin(&out[0], mn);
        atomicMax(&out[3], mx);
        atomicAdd((unsigned long long*)&out[1], (unsigned long long)sum);
        atomicAdd((unsigned long long*)&out[2], (unsigned long long)cnt);
    }
}


// Sharded supersteps, edge-balanced as sd_push_q_kernel (round 6; the 16-lane row groups of
// ssd_push_kernel held a hub row's group for the superstep): the frontier carries each row's first edge
// number, targets are compact positions, a candidate for a peer's row stays in its halo slot of best
// (the reverse exchange takes it to the owner), only own rows are listed as touched.
__global__ __launch_bounds__(kBlock) void ssd_push_q_kernel(SdWalk q, const long long* msg, long long* best, int tbits,
                                                            int32_t* touched, unsigned long long* tsize) {
    sd_push_relax<true>(q, blockDim.x, msg, best, tbits, touched, tsize);
}

// The halo slots of every peer's run back to "no candidate" once sent, one launch per shard (a fill per
// peer was 7 launches per superstep and shard at P = 8: 0.20 of 2.89 ms per shard at RMAT-22)
struct SlotRuns {
    long long* p[64];
    int64_t n[64];
};
__global__ __launch_bounds__(kBlock) void ssd_reset_slots_kernel(SlotRuns r) {
    long long* __restrict__ p = r.p[blockIdx.y];
    const int64_t n = r.n[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = LLONG_MAX;
}

// sd_apply_q_kernel's apply with the counts from the host (for ssd_push_q_kernel)
__global__ __launch_bounds__(kBlock) void ssd_apply_q_kernel(const int32_t* __restrict__ touched, int64_t tsize,
                                                             long long* __restrict__ best, long long* __restrict__ dist,
                                                             long long* __restrict__ msg, const int64_t* __restrict__ rp,
                                                             int32_t* next_frontier, int64_t* next_qoff,
                                                             unsigned long long* packed) {
    __shared__ WaveStage ws;
    sd_apply_rows(ws, blockDim.x, touched, tsize, best, dist, msg, rp, next_frontier, next_qoff, packed);
}

// The peers' candidates for own rows, received at the send-list positions (send_src[k] = own row)
__global__ void ssd_recv_kernel(const long long* __restrict__ rbuf, const int32_t* __restrict__ send_src, int64_t nrecv,
                                long long* __restrict__ best, int32_t* __restrict__ touched,
                                unsigned long long* __restrict__ tsize) {
    const int64_t iters = (nrecv + (int64_t)gridDim.x * blockDim.x - 1) / ((int64_t)gridDim.x * blockDim.x);
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + it * (int64_t)gridDim.x * blockDim.x;
        bool first = false;
        int32_t u = 0;
        if (k < nrecv) {
            const long long v = rbuf[k];
            if (v != LLONG_MAX) {
                u = send_src[k];
                first = atomicMin(&best[u], v) == LLONG_MAX;
            }
        }
        wave_append(first, u, touched, tsize);
    }
}

__global__ void fill_ll_kernel(long long* p, int64_t n, long long v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

const char* const kMissingWeight =
    "a message crossed an edge without the weight property (ShortestDistanceVertexProgram.java:69 "
    "edge.value(weightProperty) throws)";

// The buffers of the supersteps, one shard's: rows = the shard's rows, nbest = the positions candidates are
// sent to (the rows, or the compact positions of the IN halo plan)
struct SdSuperBufs {
    DevBuf<long long> dist, msg, best;
    DevBuf<int32_t> frontier[2], touched, err;
    DevBuf<int64_t> qoff[2];  // the frontiers' first edge numbers
    void alloc(int64_t rows, int64_t nbest) {
        const int64_t cap = std::max<int64_t>(rows, 1);
        dist.alloc(cap);
        msg.alloc(cap);
        best.alloc(std::max<int64_t>(nbest, 1));
        for (int k = 0; k < 2; ++k) frontier[k].alloc(cap), qoff[k].alloc(cap);
        touched.alloc(cap);
        err.alloc(1);
    }
};

// Sharded ShortestDistanceVertexProgram (weighted or unit): the same exact supersteps as the single
// shard (push from the rows whose distance fell last superstep, min into `best`, apply), over the IN
// adjacency's halo plan.  Candidates for remote vertices collect in their halo slots and go to the
// owners by the reverse halo exchange (the transpose of the PageRank/CC exchange), which take their
// min; frontier sizes are summed over shards and ranks every superstep.
void shortest_distance_sharded(Graph& g, int64_t seed_vid, int max_depth, int64_t* dist_out) {
    Ctx& ctx = *g.ctx;
    const size_t ns = g.shards.size();
    for (auto& sp : g.shards)
        if (!sp->halo_in.on)
            fail(JG_ERR_UNSUPPORTED, "sharded shortest distance needs the halo plan (tune \"halo\" = 1 at build)");
    int seed_shard = -1;
    const int64_t seed_local = local_of_vid(g, seed_vid, &seed_shard);
    struct St : SdSuperBufs {  // superstep lv reads frontier[0] / qoff[0], its apply writes [1]; then they swap
        DevBuf<long long> rbuf;
        DevBuf<unsigned long long> sizes;
        int64_t fsize = 0, fedges = 0;
    };
    std::vector<St> st(ns);
    std::vector<void*> bv, rv;
    for (size_t i = 0; i < ns; ++i) {
        Shard& sh = *g.shards[i];
        DeviceGuard dg(sh);
        const Halo& h = sh.halo_in;
        St& t = st[i];
        t.alloc(sh.rows, h.C);
        t.rbuf.alloc(std::max<int64_t>(h.send_off[g.P], 1));
        t.sizes.alloc(2);
        JG_HIP(hipMemsetAsync(t.err.get(), 0, sizeof(int32_t), sh.stream));
        fill_ll_kernel<<<grid_for(h.C), kBlock, 0, sh.stream>>>(t.best.get(), h.C, LLONG_MAX);
        fill_ll_kernel<<<grid_for(sh.rows), kBlock, 0, sh.stream>>>(t.dist.get(), sh.rows, LLONG_MIN);  // absent
        JG_LAUNCH_CHECK();
        if (seed_local >= 0 && sh.index == seed_shard) {
            const long long zero = 0;
            const int32_t seed32 = (int32_t)seed_local;
            copy_h2d(t.dist.get() + seed_local, &zero, sizeof zero, sh.stream);
            copy_h2d(t.msg.get() + seed_local, &zero, sizeof zero, sh.stream);
            copy_h2d(t.frontier[0].get(), &seed32, sizeof seed32, sh.stream);
            const int64_t zero64 = 0;
            copy_h2d(t.qoff[0].get(), &zero64, sizeof zero64, sh.stream);
            int64_t srp[2];
            copy_d2h(srp, sh.in.row_ptr.get() + seed_local, sizeof srp, sh.stream);
            t.fsize = 1;
            t.fedges = srp[1] - srp[0];
        }
        bv.push_back(t.best.peer());
        rv.push_back(t.rbuf.peer());
    }
    int64_t total = seed_local >= 0 ? 1 : 0;
    allreduce_sum_i64(g, &total, 1);
    Shard& sh0 = *g.shards[0];
    Event t0(sh0.device), t1(sh0.device);
    {
        DeviceGuard dg(sh0.device);
        region_mark(sh0.stream, true);
        JG_HIP(hipEventRecord(t0, sh0.stream));
    }
    int levels = 0;
    for (int lv = 1; lv <= max_depth && total > 0; ++lv) {
        for (size_t i = 0; i < ns; ++i) {
            Shard& sh = *g.shards[i];
            DeviceGuard dg(sh);
            St& t = st[i];
            JG_HIP(hipMemsetAsync(t.sizes.get(), 0, 2 * sizeof(unsigned long long), sh.stream));
            if (t.fsize > 0 && t.fedges > 0) {
                const SdWalk q{sh.in.row_ptr.get(), sh.in.col.get(), g.has_weights ? sh.in.weight.get() : nullptr,
                               t.frontier[0].get(), t.qoff[0].get(), t.fsize, t.fedges, t.err.get()};
                const unsigned grid = (unsigned)std::min<int64_t>(
                    std::max<int64_t>((t.fedges + (int64_t)kBlock * kTdEdgesPerThread - 1) / ((int64_t)kBlock * kTdEdgesPerThread), 1),
                    8192);
                ssd_push_q_kernel<<<grid, kBlock, 0, sh.stream>>>(q, t.msg.get(), t.best.get(), sh.halo_in.tbits,
                                                                   t.touched.get(), t.sizes.get());
                JG_LAUNCH_CHECK();
            }
        }
        exchange_halo_reverse(g, JG_ADJ_IN, bv, rv, sizeof(long long), ncclInt64);
        int64_t next = 0;
        for (size_t i = 0; i < ns; ++i) {
            Shard& sh = *g.shards[i];
            DeviceGuard dg(sh);
            St& t = st[i];
            const Halo& h = sh.halo_in;
            const int64_t nrecv = h.send_off[g.P];
            if (nrecv > 0) {
                ssd_recv_kernel<<<grid_for(nrecv, kBlock, 256 * 8), kBlock, 0, sh.stream>>>(
                    t.rbuf.get(), h.send_src.get(), nrecv, t.best.get(), t.touched.get(), t.sizes.get());
                JG_LAUNCH_CHECK();
            }
            {  // the halo slots are sent: back to "no candidate"
                SlotRuns r{};
                int nr_runs = 0;
                int64_t nmax = 0;
                for (int q = 0; q < g.P; ++q) {
                    const int64_t nr = h.recv_off[q + 1] - h.recv_off[q];
                    if (q == sh.index || nr == 0) continue;
                    if (nr_runs == 64) {  // (more than 65 shards: the runs so far in one launch, then on)
                        ssd_reset_slots_kernel<<<dim3(grid_for(nmax, kBlock, 1024), 64u), kBlock, 0, sh.stream>>>(r);
                        JG_LAUNCH_CHECK();
                        nr_runs = 0;
                        nmax = 0;
                    }
                    r.p[nr_runs] = t.best.get() + ((int64_t)h.seg_of(q, sh.index) << h.tbits);
                    r.n[nr_runs++] = nr;
                    nmax = std::max(nmax, nr);
                }
                if (nr_runs > 0) {
                    ssd_reset_slots_kernel<<<dim3(grid_for(nmax, kBlock, 1024), (unsigned)nr_runs), kBlock, 0, sh.stream>>>(r);
                    JG_LAUNCH_CHECK();
                }
            }
            unsigned long long ts = 0;
            copy_d2h(&ts, t.sizes.get(), sizeof ts, sh.stream);
            if (ts > 0) {
                ssd_apply_q_kernel<<<grid_for((int64_t)ts, kBlock, 256 * 8), kBlock, 0, sh.stream>>>(
                    t.touched.get(), (int64_t)ts, t.best.get(), t.dist.get(), t.msg.get(), sh.in.row_ptr.get(), t.frontier[1].get(),
                    t.qoff[1].get(), t.sizes.get() + 1);
                JG_LAUNCH_CHECK();
            }
            unsigned long long nn = 0;
            copy_d2h(&nn, t.sizes.get() + 1, sizeof nn, sh.stream);
            t.fsize = (int64_t)(nn >> kPackShift);
            t.fedges = (int64_t)(nn & kEdgeMask);
            t.frontier[0].swap(t.frontier[1]);
            t.qoff[0].swap(t.qoff[1]);
            next += t.fsize;
        }
        allreduce_sum_i64(g, &next, 1);
        total = next;
        levels = lv;
    }
    float ms = 0;
    {
        DeviceGuard dg(sh0.device);
        JG_HIP(hipEventRecord(t1, sh0.stream));
        region_mark(sh0.stream, false);
        JG_HIP(hipEventSynchronize(t1));
        JG_HIP(hipEventElapsedTime(&ms, t0, t1));
    }
    int missing = 0;
    for (size_t i = 0; i < ns; ++i) {
        Shard& sh = *g.shards[i];
        DeviceGuard dg(sh);
        int32_t e = 0;
        copy_d2h(&e, st[i].err.get(), sizeof e, sh.stream);
        missing |= e;
        rows_to_dense(g, sh, st[i].dist.get(), reinterpret_cast<long long*>(dist_out));  // LLONG_MIN: absent
    }
    if (allreduce_or(g, missing)) fail(JG_ERR_ARG, kMissingWeight);
    ctx.last.compute_ms = ms;
    ctx.last.levels = levels;
    ctx.last.supersteps = max_depth;
}

// The weight statistics of c (sd_weight_stats_kernel), cached on the CSR.
const long long* sd_weight_stats(Shard& sh, const Csr& c) {
    if (!c.wstat_ok) {
        hipStream_t s = sh.stream;
        DevBuf<long long> out(4);
        const long long init[4] = {LLONG_MAX, 0, 0, LLONG_MIN};
        copy_h2d(out.get(), init, sizeof init, s);
        if (c.nnz > 0 && c.weight.get()) {
            sd_weight_stats_kernel<<<grid_for(c.nnz), kBlock, 0, s>>>(c.weight.get(), c.nnz, out.get());
            JG_LAUNCH_CHECK();
        }
        copy_d2h(c.wstat, out.get(), sizeof c.wstat, s);
        c.wstat_ok = true;
    }
    return c.wstat;
}

// delta: Tune::sd_delta when set, else kSdDeltaScale x the mean weight / the mean in-degree, at least 1
// (the near-far rule of thumb, delta ~ c w / d; RMAT-20 / 22 with weights 1..255 and c = 32, 128: 1.50 /
// 3.40 and 1.23 / 3.05 ms, c = 512 equal to 128: profiles/r05/sssp/)
constexpr double kSdDeltaScale = 128.0;
long long sd_auto_delta(const long long* ws, int64_t nnz, int64_t rows) {
    if (tune().sd_delta > 0) return tune().sd_delta;
    const double mean_w = ws[2] > 0 ? (double)ws[1] / (double)ws[2] : 1.0;
    const double mean_deg = std::max(1.0, (double)nnz / (double)std::max<int64_t>(rows, 1));
    return std::max<long long>(1, (long long)std::llround(kSdDeltaScale * mean_w / mean_deg));
}

// The kept plane of a run (jg_sssp_keep): int64 in local row order, LLONG_MIN where the run's own plane has
// "unreached"
template <class D, class A>
__global__ void sd_widen_kernel(const D* __restrict__ dist, int64_t rows, long long* __restrict__ plane) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        const D d = dist[i];
        plane[i] = d == A::template none<D>() ? A::kPlaneAbsent : (long long)d;
    }
}

// Near-far delta-stepping from `seed` over the rows of c (an adjacency of sh: a row's entries are the rows
// it relaxes; see sd_near_kernel).  host[] (nullable) gets the distances (INT64_MIN: absent), plane
// (nullable, on the device, [rows]) the same in local row order, written before end_ev; end_ev is recorded
// once the distances are final, before they are copied out.  Returns the near passes run.
template <class D, class A = SdInt>
int sd_delta_stepping_t(Shard& sh, const Csr& c, int64_t seed, typename A::Delta delta, int64_t* host, long long* plane,
                        hipEvent_t end_ev) {
    hipStream_t s = sh.stream;
    const int64_t rows = sh.rows, cap = std::max<int64_t>(rows, 1);
    DevBuf<D> dist(cap);
    DevBuf<int32_t> nq[2] = {DevBuf<int32_t>(cap), DevBuf<int32_t>(cap)};
    DevBuf<int64_t> qo[2] = {DevBuf<int64_t>(cap), DevBuf<int64_t>(cap)};
    DevBuf<int32_t> far[2] = {DevBuf<int32_t>(cap), DevBuf<int32_t>(cap)};
    DevBuf<int32_t> stamp(cap), far_flag(cap), err(1);
    DevBuf<unsigned long long> ring(3 * kSdRing + 3);  // nctr[kSdRing], fmin[kSdRing], fsz[2], passes, sctr[kSdRing]
    DevBuf<SdState> st(kSdRing);
    SdStep<D, A> a{};
    a.rp = c.row_ptr.get();
    a.col = c.col.get();
    a.wt = A::weights(c);
    a.dist = dist.get();
    DevBuf<D> snap(A::kSync ? cap : 0);
    a.snap = snap.get();
    for (int k = 0; k < 2; ++k) {
        a.nq[k] = nq[k].get();
        a.qo[k] = qo[k].get();
        a.far[k] = far[k].get();
    }
    a.nctr = ring.get();
    a.fmin = ring.get() + kSdRing;
    a.fsz = ring.get() + 2 * kSdRing;
    a.passes = ring.get() + 2 * kSdRing + 2;
    a.sctr = ring.get() + 2 * kSdRing + 3;
    a.far_flag = far_flag.get();
    a.stamp = stamp.get();
    a.st = st.get();
    a.err = err.get();
    a.delta = delta;
    sd_init_kernel<D, A><<<grid_for(rows), kBlock, 0, s>>>(a, rows, (int32_t)seed);
    JG_LAUNCH_CHECK();
    // Fixed grids (the host does not know a pass's size): the near pass grid-strides over its edges, a
    // workgroup whose slice of a tile is past the end leaves at once.  tools/sd_bench.py, weights 1..255,
    // median ms at a cap of 4096 / 8192 / 16384 / 32768 / 65536 near workgroups: RMAT-24 10.25 / 9.94 / 9.68 /
    // 9.95 / 10.41, RMAT-22 2.84 / 2.74 / 2.72 (its entries / 4096 = 16384); split 1024 -> 256: equal
    // (profiles/r06/sssp_ctl/)
    const unsigned near_grid = (unsigned)std::min<int64_t>(std::max<int64_t>(c.nnz / ((int64_t)kBlock * kTdEdgesPerThread * 4), 64), 16384);
    const unsigned split_grid = (unsigned)std::min<int64_t>(std::max<int64_t>(rows / ((int64_t)kBlock * 8), 16), 256);
    // Steps in batches, the state read once per batch: the first sized from the last calls' step counts
    int step = 0, predicted = 0;
    for (int k = 0; k < std::min(sh.sd_hist_n, 4); ++k) predicted = std::max(predicted, sh.sd_hist[k]);
    SdState hs{};
    for (SdBatches b{predicted > 0 ? predicted + 1 : 16};;) {
        if (step > (1 << 26)) fail(JG_ERR_STATE, "delta-stepping control did not terminate");
        for (int k = 0, batch = b.take(); k < batch; ++k, ++step) {
            a.step = step;
            sd_split_kernel<D, A><<<split_grid, kBlock, 0, s>>>(a);
            JG_LAUNCH_CHECK();
            if (A::kSync) {
                sd_snap_kernel<D, A><<<split_grid, kBlock, 0, s>>>(a);
                JG_LAUNCH_CHECK();
            }
            sd_near_kernel<D, A><<<near_grid, kBlock, 0, s>>>(a);
            JG_LAUNCH_CHECK();
        }
        copy_d2h(&hs, st.get() + (step - 1) % kSdRing, sizeof hs, s);
        if (hs.done) break;
    }
    if (plane && rows) {
        sd_widen_kernel<D, A><<<grid_for(rows), kBlock, 0, s>>>(dist.get(), rows, plane);
        JG_LAUNCH_CHECK();
    }
    JG_HIP(hipEventRecord(end_ev, s));  // the distances are final: their copy-out is the caller's
    region_mark(s, false);
    unsigned long long passes = 0;
    copy_d2h(&passes, a.passes, sizeof passes, s);
    // the steps this call needed: up to the one that found nothing left (the next call's first batch)
    for (int k = 3; k > 0; --k) sh.sd_hist[k] = sh.sd_hist[k - 1];
    sh.sd_hist[0] = hs.end_step + 1;
    sh.sd_hist_n = std::min(sh.sd_hist_n + 1, 4);
    if (host) {
        std::vector<D> hd(rows);
        if (rows) copy_d2h(hd.data(), dist.get(), rows * sizeof(D), s);
        for (int64_t l = 0; l < rows; ++l) host[l] = hd[l] == A::template none<D>() ? LLONG_MIN : (int64_t)hd[l];
    }
    int32_t e = 0;
    copy_d2h(&e, err.get(), sizeof e, s);
    if (e) fail(JG_ERR_ARG, kMissingWeight);
    return (int)passes;
}

// 32-bit distances when no stored distance can reach UINT_MAX: a row's first distance is the length of a
// path of at most rows - 1 entries (the first-touch tree has no cycle), every later one is smaller, and a
// candidate adds one more weight (ws: sd_weight_stats).  Tune::sd_dist32: 0 keeps 64 bits, 2 takes 32 when
// safe, 1 (default) when safe and rows >= 2^23: weights 1..255, tools/sd_bench.py, median ms 64 / 32 bits,
// RMAT-20 1.197 / 1.249, RMAT-22 3.036 / 3.130, RMAT-24 10.715 / 10.228 (fabric reads -18% at RMAT-22, but
// the near pass is bound by its random round trips and atomics more than by the lines they move;
// profiles/r06/sssp32/)
int sd_delta_stepping(Shard& sh, const Csr& c, int64_t seed, long long delta, int64_t* host, long long* plane,
                      hipEvent_t end_ev, const long long* ws) {
    const unsigned long long wmax = ws[3] > 0 ? (unsigned long long)ws[3] : 0ull;
    const unsigned long long bound = (unsigned long long)std::max<int64_t>(sh.rows, 1) * wmax;  // rows * wmax
    const bool want32 = tune().sd_dist32 == 2 || (tune().sd_dist32 == 1 && sh.rows >= (1ll << 23));
    if (want32 && wmax < (1ull << 31) && (uint64_t)sh.rows < (1ull << 32) && bound < (unsigned long long)UINT_MAX)
        return sd_delta_stepping_t<unsigned int>(sh, c, seed, delta, host, plane, end_ev);
    return sd_delta_stepping_t<long long>(sh, c, seed, delta, host, plane, end_ev);
}

// The hop-bounded supersteps from `seed` over sh.in (sd_push_q_kernel + sd_apply_q_kernel per superstep);
// host[] gets the distances (INT64_MIN: absent); end_ev is recorded once the distances are final, before
// they are copied out.  Returns the supersteps counted.
int sd_supersteps(Shard& sh, int64_t seed, int max_depth, int64_t* host, hipEvent_t end_ev) {
    hipStream_t s = sh.stream;
    const int64_t rows = sh.rows;
    SdSuperBufs b;
    b.alloc(rows, rows);
    DevBuf<unsigned long long> ring(2 * kSdRing);  // frontier counts, touched counts
    DevBuf<SdSuper> sst(kSdRing);
    SdPush a{sh.in.row_ptr.get(), sh.in.col.get(), sh.in.weight.get(), {b.frontier[0].get(), b.frontier[1].get()},
             {b.qoff[0].get(), b.qoff[1].get()}, ring.get(), ring.get() + kSdRing, sst.get(), b.msg.get(),
             b.best.get(), b.dist.get(), b.touched.get(), b.err.get(), 0};
    sd_super_init_kernel<<<grid_for(rows), kBlock, 0, s>>>(a, rows, (int32_t)seed);
    JG_LAUNCH_CHECK();
    // fixed grids (the host does not know a superstep's size): the push grid-strides over its edges
    const unsigned push_grid = (unsigned)std::min<int64_t>(
        std::max<int64_t>(sh.in.nnz / ((int64_t)kBlock * kTdEdgesPerThread * 4), 64), 16384);
    const unsigned apply_grid = grid_for(rows, kBlock, 4096);
    SdSuper hs{};
    int t = 1;
    for (SdBatches bt{std::min(max_depth, 16)}; t <= max_depth;) {
        for (int k = 0, batch = std::min(bt.take(), max_depth - t + 1); k < batch; ++k, ++t) {
            a.t = t;
            sd_push_q_kernel<<<push_grid, kBlock, 0, s>>>(a);
            JG_LAUNCH_CHECK();
            sd_apply_q_kernel<<<apply_grid, kBlock, 0, s>>>(a);
            JG_LAUNCH_CHECK();
        }
        copy_d2h(&hs, sst.get() + (t - 1) % kSdRing, sizeof hs, s);
        if (hs.done) break;
    }
    JG_HIP(hipEventRecord(end_ev, s));  // the distances are final: the copy-out is outside the timed region
    region_mark(s, false);
    if (rows) copy_d2h(host, b.dist.get(), rows * sizeof(int64_t), s);  // (LLONG_MIN: absent, as host[] has it)
    int32_t e = 0;
    copy_d2h(&e, b.err.get(), sizeof e, s);
    if (e) fail(JG_ERR_ARG, kMissingWeight);
    return hs.levels;
}

}  // namespace

void shortest_distance_run(Graph& g, int64_t seed_vid, int max_depth, int64_t* dist_out) {
    Ctx& ctx = *g.ctx;
    ctx.last = jg_stats{};
    prof_discard_exchanges(g);  // exchange pairs of this call only
    if (!(g.flags & JG_ADJ_IN)) fail(JG_ERR_UNSUPPORTED, "shortest distance needs a graph built with JG_ADJ_IN");
    if (g.P != 1) {
        shortest_distance_sharded(g, seed_vid, max_depth, dist_out);
        return;
    }
    Shard& sh = *g.shards[0];
    DeviceGuard dg(sh);
    hipStream_t s = sh.stream;
    const int64_t rows = sh.rows;
    int shard = 0;
    const int64_t seed = local_of_vid(g, seed_vid, &shard);
    std::vector<int64_t> host(rows, LLONG_MIN);  // absent
    Event t0, t1;
    if (seed >= 0 && !g.has_weights) {
        bfs_buffers(sh);
        if (sh.out.present()) bfs_first_col(sh, sh.out);  // the traversal's pull adjacency
    }
    // weighted with an unbounded hop count and no negative weight: delta-stepping (the weight
    // statistics are taken once per graph, outside the timed region)
    long long delta = 0;
    if (seed >= 0 && g.has_weights && tune().sd_delta != 0 && (int64_t)max_depth >= rows - 1) {
        const long long* ws = sd_weight_stats(sh, sh.in);
        if (ws[0] >= 0) delta = sd_auto_delta(ws, sh.in.nnz, rows);
    }
    region_mark(s, true);
    JG_HIP(hipEventRecord(t0, s));
    // every engine records t1 once its distances are final, before its output copy
    int levels = 0;
    if (seed < 0) {  // not a vertex: every distance absent, nothing runs
        JG_HIP(hipEventRecord(t1, s));
        region_mark(s, false);
    } else if (!g.has_weights) {
        // unit weights: min over <= maxDepth-hop paths == BFS depth along IN edges, capped
        DevBuf<int32_t> depth(std::max<int64_t>(rows, 1));
        levels = bfs_in_depths(ctx, sh, seed, max_depth, depth.get(), t1);
        std::vector<int32_t> h(rows);
        if (rows) copy_d2h(h.data(), depth.get(), rows * sizeof(int32_t), s);
        for (int64_t l = 0; l < rows; ++l) host[l] = h[l] >= 0 ? h[l] : LLONG_MIN;
    } else if (delta > 0) {
        levels = sd_delta_stepping(sh, sh.in, seed, delta, host.data(), nullptr, t1, sd_weight_stats(sh, sh.in));
    } else {
        levels = sd_supersteps(sh, seed, max_depth, host.data(), t1);
    }
    JG_HIP(hipEventSynchronize(t1));
    float ms = 0;
    JG_HIP(hipEventElapsedTime(&ms, t0, t1));
    ctx.last.compute_ms = ms;
    ctx.last.levels = levels;
    ctx.last.supersteps = max_depth;  // Fulgora always runs supersteps 0..maxDepth
    for (int64_t l = 0; l < rows; ++l) dist_out[sh.dense_of_local()[l]] = host[l];
    prof_collect(ctx, g);
}

// ---------------- jg_sssp_keep: the distances stay on the device ----------------

void sssp_kept_release(Graph& g) {
    sssp_kept_dag_drop(g);
    for (auto& sp : g.shards) {
        DeviceGuard dg(*sp);
        sp->sssp_dist.reset();
    }
    g.sssp_kept = false;
    g.sssp_f64 = false;
}

// Shortest summed weights from one source along `direction`, by the delta-stepping of jg_shortest_distance
// over the adjacency whose rows hold the edges followed (OUT: sh.out, IN: sh.in, BOTH: the weighted sh.both);
// the int64 plane stays in Shard::sssp_dist for jg_sssp_kept_row and jg_sssp_kept_dag.
void sssp_keep(Graph& g, int64_t source_vid, int direction) {
    if (direction < JG_DIR_OUT || direction > JG_DIR_BOTH) fail(JG_ERR_ARG, "bad direction");
    if (g.P != 1 || g.shards.size() != 1) fail(JG_ERR_UNSUPPORTED, "jg_sssp_keep runs on one shard");
    sssp_kept_release(g);
    Ctx& ctx = *g.ctx;
    ctx.last = jg_stats{};
    Shard& sh = *g.shards[0];
    const Csr& c = direction == JG_DIR_BOTH ? sh.both : direction == JG_DIR_OUT ? sh.out : sh.in;
    if (!g.has_weights) fail(JG_ERR_UNSUPPORTED, "jg_sssp_keep needs a graph built with edge weights");
    if (!c.present() || c.weight.size() == 0)
        fail(JG_ERR_UNSUPPORTED, direction == JG_DIR_BOTH
                                     ? "jg_sssp_keep over JG_DIR_BOTH needs JG_ADJ_BOTH | JG_ADJ_WEIGHT_BOTH at build time"
                                     : "jg_sssp_keep: the adjacency of that direction was not built with weights");
    DeviceGuard dg(sh);
    hipStream_t s = sh.stream;
    const int64_t rows = sh.rows;
    // the weight statistics are taken once per adjacency, outside the timed region
    const long long* ws = sd_weight_stats(sh, c);
    if (ws[2] > 0 && ws[0] < 1)
        fail(JG_ERR_ARG, "jg_sssp_keep needs weights >= 1 (a zero-weight edge makes the tight-edge graph cyclic)");
    int shard = 0;
    const int64_t seed = local_of_vid(g, source_vid, &shard);
    DevBuf<long long> plane((size_t)std::max<int64_t>(rows, 1));
    Event t0, t1;
    region_mark(s, true);
    JG_HIP(hipEventRecord(t0, s));
    int levels = 0;
    if (seed < 0) {  // not a vertex: every distance absent
        if (rows) {
            fill_ll_kernel<<<grid_for(rows), kBlock, 0, s>>>(plane.get(), rows, LLONG_MIN);
            JG_LAUNCH_CHECK();
        }
        JG_HIP(hipEventRecord(t1, s));
        region_mark(s, false);
    } else {
        levels = sd_delta_stepping(sh, c, seed, sd_auto_delta(ws, c.nnz, rows), nullptr, plane.get(), t1, ws);
    }
    JG_HIP(hipEventSynchronize(t1));
    float ms = 0;
    JG_HIP(hipEventElapsedTime(&ms, t0, t1));
    ctx.last.compute_ms = ms;
    ctx.last.levels = levels;
    sh.sssp_dist.swap(plane);
    g.sssp_kept = true;
    g.sssp_dir = direction;
}

void sssp_kept_row(Graph& g, int64_t* dist_out) {
    if (!g.sssp_kept) fail(JG_ERR_STATE, "no distance plane is kept (jg_sssp_keep)");
    if (g.sssp_f64) fail(JG_ERR_STATE, "the kept plane holds doubles (jg_sssp_keep_f64): read it with jg_sssp_kept_row_f64");
    Shard& sh = *g.shards[0];
    rows_to_dense(g, sh, sh.sssp_dist.get(), reinterpret_cast<long long*>(dist_out));
}

// ---------------- double weights: jg_graph_set_weights_f64, jg_sssp_keep_f64 ----------------

namespace {

// The weights' statistics, one partial per workgroup: the smallest, largest and summed value of the workgroup's
// share (a fixed grid-stride assignment, reduced in a fixed order: lanes by a butterfly, waves in wave order) and
// how many values are not finite and > 0.  The host sums the partials in workgroup order, so the statistics, the
// automatic delta and with it stats.levels are the same on every run.  No atomic.
struct WfPart {
    double mn, mx, sum;
    unsigned long long bad;
};
constexpr int kWfGrid = 1024;
__global__ __launch_bounds__(kBlock) void wf_stats_kernel(const double* __restrict__ w, int64_t m, WfPart* __restrict__ part) {
    __shared__ WfPart red[kBlock / kWave];
    double mn = __builtin_huge_val(), mx = 0.0, sum = 0.0;
    unsigned long long bad = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
        const double x = w[j];
        if (!(x > 0.0) || !(x < __builtin_huge_val())) {  // zero, negative, NaN, +Inf
            ++bad;
            continue;
        }
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
        sum += x;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const double a = __shfl_xor(mn, o, kWave), b = __shfl_xor(mx, o, kWave);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        sum += __shfl_xor(sum, o, kWave);
        bad += __shfl_xor(bad, o, kWave);
    }
    if (lane_id() == 0) red[wave_id()] = WfPart{mn, mx, sum, bad};
    __syncthreads();
    if (threadIdx.x == 0) {
        WfPart r = red[0];
        for (int k = 1; k < kBlock / kWave; ++k) {
            r.mn = red[k].mn < r.mn ? red[k].mn : r.mn;
            r.mx = red[k].mx > r.mx ? red[k].mx : r.mx;
            r.sum += red[k].sum;
            r.bad += red[k].bad;
        }
        part[blockIdx.x] = r;
    }
}

// wf[j] = weight[eidx[j]]: each entry's double, through its edge ordinal (as csr_finish gathers the int32 weights)
__global__ void wf_gather_kernel(const double* __restrict__ w, const uint32_t* __restrict__ eidx, int64_t nnz,
                                 double* __restrict__ wf) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * blockDim.x)
        wf[j] = w[eidx[j]];
}

}  // namespace

// The gate: with n = the vertex count, wmin >= n * wmax * 2^-52, wmin >= DBL_MIN and n * wmax finite.
// Why no relaxation is absorbed under it.  A row's first stored distance is the left-to-right sum of the weights
// along the first-touch tree's path to it: at most n - 1 weights (the tree has no cycle), each at most wmax, each
// add rounding up by at most a factor 1 + 2^-53; every later stored distance of the row is smaller (the atomicMin
// only lets a distance fall, and fl(a + w) is monotone in a).  So a stored distance d is below
// n * wmax * (1 + 2^-53)^n < n * wmax * (1 + 2^-21) for n < 2^31.  d is 0 (the source: fl(0 + w) = w > 0) or at
// least wmin >= DBL_MIN, hence normal, and the gap from a normal d to the next double is at most d * 2^-52.  The
// gate's product is rounded once (by at most 1 - 2^-53), so half that gap, d * 2^-53, is below
// n * wmax * (1 + 2^-21) * 2^-53 < fl(n * wmax) * 2^-52 <= wmin <= w: d + w lies past the midpoint to the next
// double and fl(d + w) > d.  Every relaxed edge therefore strictly increases the distance: a tight edge u -> v has
// dist[u] < dist[v], and the tight-edge graph has no cycle.
// No stored distance is infinite: unreached is +Inf's own pattern, so a candidate that overflowed to +Inf is
// never below what a row holds and the atomicMin never sees it (with n * wmax finite none arises but in the
// last binade).
void graph_set_weights_f64(Graph& g, const double* weight, int64_t m) {
    if (!(g.flags & JG_ADJ_EDGE_INDEX) || g.edge_list_m < 0)
        fail(JG_ERR_UNSUPPORTED,
             "jg_graph_set_weights_f64 needs a graph built with JG_ADJ_EDGE_INDEX (its entries' edge ordinals)");
    if (g.P != 1 || g.shards.size() != 1) fail(JG_ERR_UNSUPPORTED, "jg_graph_set_weights_f64: graphs of one shard only");
    if (m != g.edge_list_m) fail(JG_ERR_ARG, "jg_graph_set_weights_f64: m is not the length of the edge list the graph was built from");
    if (m > 0 && !weight) fail(JG_ERR_ARG, "weight is null");
    Shard& sh = *g.shards[0];
    DeviceGuard dg(sh);
    DevBuf<double> dw((size_t)std::max<int64_t>(m, 1));
    if (m > 0) copy_h2d(dw.get(), weight, (size_t)m * sizeof(double), sh.stream);
    graph_set_weights_f64_device(g, dw.get(), m, "jg_graph_set_weights_f64");
}

// The device half: dw[0, m) = one double per listed edge on the shard's device (uploaded above, or decoded from
// the rows by a builder with jg_builder_set_weight_key_f64, whose finish calls this).
void graph_set_weights_f64_device(Graph& g, const double* dw, int64_t m, const char* who) {
    const std::string name(who);
    if (!(g.flags & JG_ADJ_EDGE_INDEX) || m != g.edge_list_m || g.P != 1 || g.shards.size() != 1)
        fail(JG_ERR_STATE, name + ": the weights are not those of the graph's edge list");
    Shard& sh = *g.shards[0];
    DeviceGuard dg(sh);
    hipStream_t s = sh.stream;
    double wmin = 0, wmax = 0, mean = 0;
    if (m > 0) {
        const unsigned grid = grid_for(m, kBlock, kWfGrid);
        DevBuf<WfPart> part(grid);
        wf_stats_kernel<<<grid, kBlock, 0, s>>>(dw, m, part.get());
        JG_LAUNCH_CHECK();
        std::vector<WfPart> hp(grid);
        copy_d2h(hp.data(), part.get(), grid * sizeof(WfPart), s);
        WfPart r = hp[0];
        for (unsigned k = 1; k < grid; ++k) {  // workgroup order
            r.mn = hp[k].mn < r.mn ? hp[k].mn : r.mn;
            r.mx = hp[k].mx > r.mx ? hp[k].mx : r.mx;
            r.sum += hp[k].sum;
            r.bad += hp[k].bad;
        }
        if (r.bad) fail(JG_ERR_ARG, name + ": every weight must be finite and > 0");
        wmin = r.mn;
        wmax = r.mx;
        mean = std::isfinite(r.sum) ? r.sum / (double)m : wmax;  // (a sum past DBL_MAX: any delta is correct)
        const double span = (double)std::max<int64_t>(g.n, 1) * wmax;
        if (!std::isfinite(span) || wmin < DBL_MIN || wmin < span * 0x1p-52)
            fail(JG_ERR_UNSUPPORTED,
                 name + ": the weights' range lets a relaxation be absorbed (needs wmin >= rows * wmax * 2^-52, "
                        "wmin >= DBL_MIN, rows * wmax finite)");
    }
    // gathered beside every built adjacency, into buffers of their own: a failure up to here left the graph as it was
    Csr* cs[3] = {&sh.out, &sh.in, &sh.both};
    DevBuf<double> nw[3];
    for (int k = 0; k < 3; ++k) {
        const Csr& c = *cs[k];
        if (!c.present()) continue;
        if (c.eidx.size() < (size_t)c.nnz) fail(JG_ERR_STATE, name + ": an adjacency holds no edge ordinals");
        nw[k].alloc((size_t)std::max<int64_t>(c.nnz, 1));
        if (c.nnz > 0) {
            wf_gather_kernel<<<grid_for(c.nnz), kBlock, 0, s>>>(dw, c.eidx.get(), c.nnz, nw[k].get());
            JG_LAUNCH_CHECK();
        }
    }
    JG_HIP(hipStreamSynchronize(s));
    if (g.sssp_kept && g.sssp_f64) sssp_kept_release(g);  // distances of the weights that leave
    int64_t before = 0, after = 0;
    for (int k = 0; k < 3; ++k) {
        before += (int64_t)cs[k]->wf.bytes();
        cs[k]->wf.swap(nw[k]);
        after += (int64_t)cs[k]->wf.bytes();
    }
    g.info.device_bytes += after - before;
    g.has_wf = true;
    g.wf_min = wmin;
    g.wf_max = wmax;
    g.wf_mean = mean;
}

// jg_sssp_keep over the double weights: the same engine with SdF64's arithmetic, the plane (bit patterns, +Inf:
// unreached) in jg_sssp_keep's slot.  delta: Tune::sd_delta when set, else kSdDeltaScale x the mean weight / the
// mean degree in double, at least wmin.
void sssp_keep_f64(Graph& g, int64_t source_vid, int direction) {
    if (direction < JG_DIR_OUT || direction > JG_DIR_BOTH) fail(JG_ERR_ARG, "bad direction");
    if (g.P != 1 || g.shards.size() != 1) fail(JG_ERR_UNSUPPORTED, "jg_sssp_keep_f64 runs on one shard");
    sssp_kept_release(g);
    Ctx& ctx = *g.ctx;
    ctx.last = jg_stats{};
    Shard& sh = *g.shards[0];
    const Csr& c = direction == JG_DIR_BOTH ? sh.both : direction == JG_DIR_OUT ? sh.out : sh.in;
    if (!g.has_wf) fail(JG_ERR_UNSUPPORTED, "jg_sssp_keep_f64 needs jg_graph_set_weights_f64 first");
    if (!c.present() || c.wf.size() == 0)
        fail(JG_ERR_UNSUPPORTED, "jg_sssp_keep_f64: the adjacency of that direction was not built");
    DeviceGuard dg(sh);
    hipStream_t s = sh.stream;
    const int64_t rows = sh.rows;
    double delta = 1.0;
    if (tune().sd_delta > 0) {
        delta = (double)tune().sd_delta;
    } else if (c.nnz > 0 && g.wf_mean > 0) {
        const double mean_deg = std::max(1.0, (double)c.nnz / (double)std::max<int64_t>(rows, 1));
        delta = std::max(g.wf_min, kSdDeltaScale * g.wf_mean / mean_deg);
        if (!std::isfinite(delta)) delta = g.wf_max;
    }
    int shard = 0;
    const int64_t seed = local_of_vid(g, source_vid, &shard);
    DevBuf<long long> plane((size_t)std::max<int64_t>(rows, 1));
    Event t0, t1;
    region_mark(s, true);
    JG_HIP(hipEventRecord(t0, s));
    int levels = 0;
    if (seed < 0) {  // not a vertex: every distance absent
        if (rows) {
            fill_ll_kernel<<<grid_for(rows), kBlock, 0, s>>>(plane.get(), rows, kF64InfBits);
            JG_LAUNCH_CHECK();
        }
        JG_HIP(hipEventRecord(t1, s));
        region_mark(s, false);
    } else {
        levels = sd_delta_stepping_t<long long, SdF64>(sh, c, seed, delta, nullptr, plane.get(), t1);
    }
    JG_HIP(hipEventSynchronize(t1));
    float ms = 0;
    JG_HIP(hipEventElapsedTime(&ms, t0, t1));
    ctx.last.compute_ms = ms;
    ctx.last.levels = levels;
    sh.sssp_dist.swap(plane);
    g.sssp_kept = true;
    g.sssp_f64 = true;
    g.sssp_dir = direction;
}

void sssp_kept_row_f64(Graph& g, double* dist_out) {
    if (!g.sssp_kept) fail(JG_ERR_STATE, "no distance plane is kept (jg_sssp_keep_f64)");
    if (!g.sssp_f64) fail(JG_ERR_STATE, "the kept plane holds integers (jg_sssp_keep): read it with jg_sssp_kept_row");
    Shard& sh = *g.shards[0];
    rows_to_dense(g, sh, sh.sssp_dist.get(), reinterpret_cast<long long*>(dist_out));
}

}  // namespace jg
