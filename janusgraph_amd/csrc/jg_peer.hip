// jg_peer.hip — PeerPressureVertexProgram (jg_peer_pressure): every vertex takes the weighted MODE of the
// cluster labels its neighbours vote, superstep after superstep, until no label changes ("Peer
// pressure on the device").  The mode is no semiring fold, so this unit does not go through jg_pull.h: a
// row's (label, strength) votes are sorted by label, equal labels are summed, and the largest sum wins.
//
// One shard.  Labels are int32 RANKS of the vertex ids in numeric (signed int64) order, made once per call
// by a radix sort of (vid, row): the smallest id among tied clusters is the smallest label.  (Shard::cc_rank0
// is the String order and is not used here.)  Two label vectors, indexed by local row as the CSR's columns
// are, ping-pong: a vote kernel reads `in` and writes `out`, never the same buffer.  Rows without entries
// keep their own label in both vectors and are never visited.
//
// Row classes, by the row's own entry count e = degree + 1 (the own vote enters like one more entry); the
// rows of a class are listed once per call (a row need not sit where the degree order would put it):
//   e <= 4, <= 16, <= 64   a group of 4 / 16 / 64 lanes per row, one entry per lane: bitonic sort of the lanes
//           by label, segmented scan of the strengths over equal labels, argmax (sum desc, label asc) across
//           the group.  Everything stays in registers.
//   e > 64  the sort path, whatever the distinct-label count (in the first superstep every entry of a row
//           carries another label): each entry becomes a key (row slot << label bits | label), the keys of
//           all long rows are radix sorted together (stable, so the additions of a run have a fixed order),
//           every run end finds its run's start by a galloping search and sums it (a lane for short runs, the
//           whole wave in a fixed lane-strided order for long ones), and the row slots take the maximum of the
//           run sums (atomicMax on the sum's ordered bits: order-independent) and then the smallest label
//           among the runs that reach it (atomicMin).
// Unit strength counts in uint32 (no strength gather, no fp); distributed strength sums fp64 gathered from
// strength[u] = 1 / (entries u sends on), +Inf for a vertex that sends on none.
// Halting: `changed` is zeroed before a superstep's kernels, a wave adds its changed rows once, the host reads
// it once per superstep.
//
// Byte model of one vote superstep (unit strength; [+ x] = more with distributed strength).  An entry is an
// adjacency entry or a row's own vote.
//   every non-empty row   4 B list + 16 B row_ptr + 4 B own label + 4 B label store = 28 B [+ 8 B own strength]
//   group-class entry     4 B column + 4 B gathered label = 8 B [+ 8 B gathered strength]
//   sort-path entry       the same 8 B, the key stored (8 B [+ 4 B sender]), per 8-bit sort pass the key read
//                         twice and moved once (24 B [+ 8 B sender read and written]), the fold and the pick
//                         each read the key (16 B), the run sum written and read (16 B) [+ 4 B sender + 8 B
//                         gathered strength]
#include "jg_internal.h"
#include "jg_prim.h"

namespace jg {
namespace {

constexpr int kPeerLong = 64;          // most entries (degree + 1) of a row the lane groups take
constexpr int kPeerLaneRun = 32;       // longest run a single lane sums in the sort path's fold
constexpr int32_t kNoLabel = INT32_MAX;

template <bool DIST>
struct Vote;
template <>
struct Vote<false> {
    using W = uint32_t;
    __device__ static __forceinline__ W of(const double*, int32_t) { return 1u; }
    __device__ static __forceinline__ unsigned long long order(W w) { return w; }
};
template <>
struct Vote<true> {
    using W = double;
    __device__ static __forceinline__ W of(const double* __restrict__ strength, int32_t c) { return strength[c]; }
    // sums are positive (or +Inf): their bit patterns order as the values do
    __device__ static __forceinline__ unsigned long long order(W w) { return (unsigned long long)__double_as_longlong(w); }
};

// ---- per call: ranks, strengths, row classes ----
__global__ void peer_vid_key_kernel(const int64_t* __restrict__ vid, const int32_t* __restrict__ dense, int64_t rows,
                                    int64_t vmin, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < rows; l += (int64_t)gridDim.x * blockDim.x) {
        key[l] = (uint64_t)vid[dense[l]] - (uint64_t)vmin;
        val[l] = (uint32_t)l;
    }
}

// sorted position p = the rank of row val[p]; vor[p] = the id of rank p
__global__ void peer_rank_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t rows,
                                 int64_t vmin, int32_t* __restrict__ lab0, int32_t* __restrict__ lab1,
                                 int64_t* __restrict__ vor) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < rows; p += (int64_t)gridDim.x * blockDim.x) {
        lab0[val[p]] = (int32_t)p;
        lab1[val[p]] = (int32_t)p;
        vor[p] = (int64_t)(key[p] + (uint64_t)vmin);
    }
}

// ids equal to the caller's indices (generated graphs): the rank of a row is its caller index
__global__ void peer_rank_dense_kernel(const int32_t* __restrict__ dense, int64_t rows, int32_t* __restrict__ lab0,
                                       int32_t* __restrict__ lab1) {
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < rows; l += (int64_t)gridDim.x * blockDim.x)
        lab0[l] = lab1[l] = dense[l];
}

// strength[l] = 1 / (entries in which row l is the sender): its out-degree (cnt) or its own row's length
__global__ void peer_strength_kernel(const int32_t* __restrict__ cnt, const int64_t* __restrict__ row_ptr, int64_t rows,
                                     double* __restrict__ strength) {
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < rows; l += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = cnt ? (int64_t)cnt[l] : row_ptr[l + 1] - row_ptr[l];
        strength[l] = c > 0 ? 1.0 / (double)c : __longlong_as_double(0x7FF0000000000000ll);
    }
}

// flag[k][l] = row l belongs to class k (0..2: lane groups of 4, 16, 64; 3: the sort path); empty rows to none
__global__ void peer_class_kernel(const int64_t* __restrict__ row_ptr, int64_t rows, uint8_t* __restrict__ flag) {
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < rows; l += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = row_ptr[l + 1] - row_ptr[l] + 1;
        const int k = e == 1 ? -1 : e <= 4 ? 0 : e <= 16 ? 1 : e <= kPeerLong ? 2 : 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) flag[(int64_t)j * rows + l] = j == k;
    }
}

// the class's row list as int32, and (entries, nullable) each listed row's entry count e
__global__ void peer_list_kernel(const int64_t* __restrict__ idx, int64_t count, const int64_t* __restrict__ row_ptr,
                                 int32_t* __restrict__ list, int64_t* __restrict__ entries) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = idx[i];
        list[i] = (int32_t)l;
        if (entries) entries[i] = row_ptr[l + 1] - row_ptr[l] + 1;
    }
}

// ---- vote superstep: rows of at most G entries, G lanes per row ----
template <int G, bool DIST>
__global__ __launch_bounds__(kBlock) void peer_group_kernel(const int32_t* __restrict__ list, int64_t count,
                                                            const int64_t* __restrict__ row_ptr,
                                                            const int32_t* __restrict__ col,
                                                            const int32_t* __restrict__ lab_in,
                                                            const double* __restrict__ strength,
                                                            int32_t* __restrict__ lab_out, uint32_t* __restrict__ changed) {
    using V = Vote<DIST>;
    using W = typename V::W;
    const int64_t grp = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    const bool valid = grp < count;
    int32_t row = 0;
    int64_t b = 0;
    int d = 0;
    if (valid) {
        row = list[grp];
        b = row_ptr[row];
        d = (int)(row_ptr[row + 1] - b);
        d = d < G ? d : G - 1;  // always (peer_class_kernel): a bound, not a case
    }
    int32_t lab = kNoLabel;
    W w = 0;
    if (valid && sub <= d) {
        const int32_t c = sub < d ? col[b + sub] : row;  // lane d: the own vote
        lab = lab_in[c];
        w = V::of(strength, c);
    }
    const int32_t own = __shfl(lab, d, G);
    // bitonic sort of the group's lanes by label, the strength riding along
#pragma unroll
    for (int k = 2; k <= G; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int32_t pl = __shfl_xor(lab, j, G);
            const W pw = __shfl_xor(w, j, G);
            const bool up = (sub & k) == 0, lower = (sub & j) == 0;
            const bool take = (lower == up) ? pl < lab : pl > lab;
            if (take) {
                lab = pl;
                w = pw;
            }
        }
    }
    // inclusive scan of the strengths inside each run of equal labels
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        const int32_t pl = __shfl_up(lab, o, G);
        const W pw = __shfl_up(w, o, G);
        if (sub >= o && pl == lab) w += pw;
    }
    const int32_t next = __shfl_down(lab, 1, G);
    const bool cand = lab != kNoLabel && (sub == G - 1 || next != lab);  // the run's last lane holds its sum
    unsigned long long ord = cand ? V::order(w) : 0ull;
    int32_t best = cand ? lab : kNoLabel;
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) {
        const unsigned long long po = __shfl_xor(ord, o, G);
        const int32_t pl = __shfl_xor(best, o, G);
        if (po > ord || (po == ord && pl < best)) {
            ord = po;
            best = pl;
        }
    }
    const bool head = valid && sub == 0;
    if (head) lab_out[row] = best;
    const uint64_t ch = __ballot(head && best != own);
    if (ch && lane_id() == 0) atomicAdd(changed, (uint32_t)__popcll(ch));
}

// ---- vote superstep: the sort path ----
// slot s = long row list[s], its e entries at key[off[s], off[s] + e): (s << lbits | label); val = the sender
template <bool DIST>
__global__ __launch_bounds__(kBlock) void peer_fill_kernel(const int32_t* __restrict__ list, int64_t slots,
                                                           const int64_t* __restrict__ off,
                                                           const int64_t* __restrict__ row_ptr,
                                                           const int32_t* __restrict__ col,
                                                           const int32_t* __restrict__ lab_in, int lbits,
                                                           uint64_t* __restrict__ key, uint32_t* __restrict__ val,
                                                           unsigned long long* __restrict__ best_sum,
                                                           int32_t* __restrict__ best_lab) {
    const int64_t nw = (int64_t)gridDim.x * (kBlock / kWave);
    for (int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave_id(); s < slots; s += nw) {
        const int32_t row = list[s];
        const int64_t b = row_ptr[row], d = row_ptr[row + 1] - b, o = off[s];
        for (int64_t j = lane_id(); j <= d; j += kWave) {
            const int32_t c = j < d ? col[b + j] : row;
            key[o + j] = ((uint64_t)s << lbits) | (uint64_t)(uint32_t)lab_in[c];
            if (DIST) val[o + j] = (uint32_t)c;
        }
        if (lane_id() == 0) {
            best_sum[s] = 0ull;
            best_lab[s] = kNoLabel;
        }
    }
}

// Over the sorted keys: sum[p] = the ordered bits of the sum of the run that ends at p (0 elsewhere), and
// best_sum[slot] = the largest of them.
template <bool DIST>
__global__ __launch_bounds__(kBlock) void peer_fold_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                           int64_t n, int lbits, const double* __restrict__ strength,
                                                           unsigned long long* __restrict__ sum,
                                                           unsigned long long* __restrict__ best_sum) {
    using V = Vote<DIST>;
    using W = typename V::W;
    for (int64_t p0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1)); p0 < n; p0 += (int64_t)gridDim.x * kBlock) {
        const int64_t p = p0 + lane_id();
        const bool in = p < n;
        const uint64_t k = in ? key[p] : ~0ull;
        const bool end = in && (p == n - 1 || key[p + 1] != k);
        int64_t lb = p;  // first entry of the run
        if (end && p > 0 && key[p - 1] == k) {
            int64_t hi = p - 1, lo, step = 2;  // key[hi] == k; key[lo] != k or lo == -1
            for (;;) {
                lo = p - step;
                if (lo < 0) {
                    lo = -1;
                    break;
                }
                if (key[lo] != k) break;
                hi = lo;
                step <<= 1;
            }
            while (hi - lo > 1) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (key[mid] == k) hi = mid;
                else lo = mid;
            }
            lb = hi;
        }
        W total = 0;
        if (DIST) {
            const bool wide = end && p - lb >= kPeerLaneRun;
            if (end && !wide)
                for (int64_t q = lb; q <= p; ++q) total += V::of(strength, (int32_t)val[q]);
            // a long run: the wave sums it, lane-strided, then across the lanes (the same order on every run)
            for (uint64_t pend = __ballot(wide); pend; pend &= pend - 1) {  // wave-uniform
                const int f = __ffsll((unsigned long long)pend) - 1;
                const int64_t flb = __shfl((long long)lb, f, kWave), fp = p0 + f;
                W acc = 0;
                for (int64_t q = flb + lane_id(); q <= fp; q += kWave) acc += V::of(strength, (int32_t)val[q]);
                acc = wave_reduce_add(acc);
                if (lane_id() == f) total = acc;
            }
        } else {
            total = (W)(p - lb + 1);
        }
        const unsigned long long ord = end ? V::order(total) : 0ull;
        if (in) sum[p] = ord;
        // a wave inside one row: a single atomic
        const uint64_t slot = k >> lbits, first = __shfl((unsigned long long)slot, 0, kWave);
        if (__ballot(in && slot != first) == 0) {
            const unsigned long long m = wave_reduce_max(ord);
            if (m && lane_id() == 0) atomicMax(&best_sum[first], m);
        } else if (end) {
            atomicMax(&best_sum[slot], ord);
        }
    }
}

// best_lab[slot] = the smallest label among the runs whose sum is best_sum[slot]
__global__ __launch_bounds__(kBlock) void peer_pick_kernel(const uint64_t* __restrict__ key,
                                                           const unsigned long long* __restrict__ sum, int64_t n, int lbits,
                                                           const unsigned long long* __restrict__ best_sum,
                                                           int32_t* __restrict__ best_lab) {
    const uint64_t lmask = (1ull << lbits) - 1ull;
    for (int64_t p0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1)); p0 < n; p0 += (int64_t)gridDim.x * kBlock) {
        const int64_t p = p0 + lane_id();
        const bool in = p < n;
        const uint64_t k = in ? key[p] : ~0ull;
        const unsigned long long ord = in ? sum[p] : 0ull;
        const uint64_t slot = k >> lbits, first = __shfl((unsigned long long)slot, 0, kWave);
        const bool same = __ballot(in && slot != first) == 0;  // wave-uniform
        const unsigned long long top = same ? best_sum[first] : (ord ? best_sum[slot] : 0ull);
        const int32_t lab = ord && ord == top ? (int32_t)(k & lmask) : kNoLabel;
        if (same) {
            const int32_t m = wave_reduce_min(lab);
            if (m != kNoLabel && lane_id() == 0) atomicMin(&best_lab[first], m);
        } else if (lab != kNoLabel) {
            atomicMin(&best_lab[slot], lab);
        }
    }
}

__global__ __launch_bounds__(kBlock) void peer_apply_kernel(const int32_t* __restrict__ list, int64_t slots,
                                                            const int32_t* __restrict__ best_lab,
                                                            const int32_t* __restrict__ lab_in,
                                                            int32_t* __restrict__ lab_out, uint32_t* __restrict__ changed) {
    for (int64_t s0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1)); s0 < slots; s0 += (int64_t)gridDim.x * kBlock) {
        const int64_t s = s0 + lane_id();
        bool moved = false;
        if (s < slots) {
            const int32_t row = list[s], nl = best_lab[s];
            lab_out[row] = nl;
            moved = nl != lab_in[row];
        }
        const uint64_t ch = __ballot(moved);
        if (ch && lane_id() == 0) atomicAdd(changed, (uint32_t)__popcll(ch));
    }
}

// out[dense[l]] = the id of row l's cluster
__global__ void peer_out_kernel(const int32_t* __restrict__ lab, const int64_t* __restrict__ vor,
                                const int32_t* __restrict__ dense, int64_t rows, int64_t* __restrict__ out) {
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < rows; l += (int64_t)gridDim.x * blockDim.x)
        out[dense[l]] = vor ? vor[lab[l]] : (int64_t)lab[l];
}

struct PeerLists {
    DevBuf<int32_t> list[4];
    int64_t count[4] = {0, 0, 0, 0};
    DevBuf<int64_t> off;     // [count[3] + 1] first key of each long row
    int64_t long_entries = 0;
    int64_t group_entries = 0;  // entries (own votes included) of the lane-group rows
};

template <bool DIST>
int64_t vote_superstep(const Csr& c, const PeerLists& pl, const int32_t* in, int32_t* out, const double* strength, int lbits,
                       int kbits, uint64_t* key, uint32_t* val, unsigned long long* sum, unsigned long long* best_sum,
                       int32_t* best_lab, uint32_t* changed, hipStream_t st) {
    int64_t launches = 0;
    const int64_t* rp = c.row_ptr.get();
    const int32_t* col = c.col.get();
    if (pl.count[0]) {
        peer_group_kernel<4, DIST><<<(unsigned)((pl.count[0] * 4 + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            pl.list[0].get(), pl.count[0], rp, col, in, strength, out, changed);
        JG_LAUNCH_CHECK();
        ++launches;
    }
    if (pl.count[1]) {
        peer_group_kernel<16, DIST><<<(unsigned)((pl.count[1] * 16 + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            pl.list[1].get(), pl.count[1], rp, col, in, strength, out, changed);
        JG_LAUNCH_CHECK();
        ++launches;
    }
    if (pl.count[2]) {
        peer_group_kernel<64, DIST><<<(unsigned)((pl.count[2] * 64 + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            pl.list[2].get(), pl.count[2], rp, col, in, strength, out, changed);
        JG_LAUNCH_CHECK();
        ++launches;
    }
    if (pl.count[3]) {
        const int64_t slots = pl.count[3], n = pl.long_entries;
        peer_fill_kernel<DIST><<<grid_for(slots, kBlock / kWave), kBlock, 0, st>>>(pl.list[3].get(), slots, pl.off.get(), rp, col, in,
                                                                                  lbits, key, val, best_sum, best_lab);
        JG_LAUNCH_CHECK();
        prim::radix_sort(key, DIST ? val : nullptr, n, kbits, st);
        peer_fold_kernel<DIST><<<grid_for(n), kBlock, 0, st>>>(key, val, n, lbits, strength, sum, best_sum);
        JG_LAUNCH_CHECK();
        peer_pick_kernel<<<grid_for(n), kBlock, 0, st>>>(key, sum, n, lbits, best_sum, best_lab);
        JG_LAUNCH_CHECK();
        peer_apply_kernel<<<grid_for(slots), kBlock, 0, st>>>(pl.list[3].get(), slots, best_lab, in, out, changed);
        JG_LAUNCH_CHECK();
        launches += 4 + 2 * ((kbits + 7) / 8);
    }
    return launches;
}

}  // namespace

void peer_pressure_run(Graph& g, int direction, int distribute, int max_iterations, int64_t* cluster_out,
                       int32_t* iterations_out) {
    if (direction == JG_DIR_IN)
        fail(JG_ERR_UNSUPPORTED, "jg_peer_pressure: JG_DIR_IN (votes along in-edges) is not run: its vote strength divides by a "
                                 "degree that neither adjacency flag guarantees");
    if (direction != JG_DIR_OUT && direction != JG_DIR_BOTH) fail(JG_ERR_ARG, "direction must be JG_DIR_OUT or JG_DIR_BOTH");
    if (max_iterations < 0) fail(JG_ERR_ARG, "jg_peer_pressure: negative max_iterations");
    const uint32_t adj = direction == JG_DIR_OUT ? JG_ADJ_IN : JG_ADJ_BOTH;
    if (!(g.flags & adj))
        fail(JG_ERR_UNSUPPORTED, std::string("jg_peer_pressure: graph was built without the ") +
                                     (adj == JG_ADJ_IN ? "IN" : "BOTH") + " adjacency");
    if (g.P != 1 || g.shards.size() != 1)
        fail(JG_ERR_UNSUPPORTED, "jg_peer_pressure runs on one shard");
    Shard& sh = *g.shards[0];
    if (sh.rows != g.n || sh.dense_rows.size() < (size_t)std::max<int64_t>(sh.rows, 1))
        fail(JG_ERR_UNSUPPORTED, "jg_peer_pressure: the shard does not hold every vertex");
    Ctx& ctx = *g.ctx;
    DeviceGuard dg(sh);
    hipStream_t st = sh.stream;
    const Csr& c = adj == JG_ADJ_IN ? sh.in : sh.both;
    const int64_t n = sh.rows;
    const bool dist = distribute != 0;
    int votes = 0;
    float ms = 0, vote_ms = 0;
    int64_t launches = 0;
    PeerLists pl;
    int sort_passes = 0;
    if (n > 0) {
        Event t0, t1, v0, v1;
        region_mark(st, true);
        JG_HIP(hipEventRecord(t0, st));
        // ---- ranks of the ids ----
        DevBuf<int32_t> lab[2];
        lab[0].alloc((size_t)n);
        lab[1].alloc((size_t)n);
        DevBuf<int64_t> vor;
        if (g.vid.empty()) {
            peer_rank_dense_kernel<<<grid_for(n), kBlock, 0, st>>>(sh.dense_rows.get(), n, lab[0].get(), lab[1].get());
            JG_LAUNCH_CHECK();
        } else {
            int64_t vmin = g.vid[0], vmax = g.vid[0];
            for (int64_t v : g.vid) {
                vmin = std::min(vmin, v);
                vmax = std::max(vmax, v);
            }
            DevBuf<int64_t> dvid((size_t)n);
            DevBuf<uint64_t> rkey((size_t)n);
            DevBuf<uint32_t> rval((size_t)n);
            vor.alloc((size_t)n);
            copy_h2d(dvid.get(), g.vid.data(), (size_t)n * sizeof(int64_t), st);
            peer_vid_key_kernel<<<grid_for(n), kBlock, 0, st>>>(dvid.get(), sh.dense_rows.get(), n, vmin, rkey.get(), rval.get());
            JG_LAUNCH_CHECK();
            prim::radix_sort(rkey.get(), rval.get(), n, std::max(bits_for((uint64_t)vmax - (uint64_t)vmin), 1), st);
            peer_rank_kernel<<<grid_for(n), kBlock, 0, st>>>(rkey.get(), rval.get(), n, vmin, lab[0].get(), lab[1].get(), vor.get());
            JG_LAUNCH_CHECK();
        }
        // ---- strengths (the counting superstep of distributeVote) ----
        DevBuf<double> strength;
        if (dist) {
            strength.alloc((size_t)n);
            peer_strength_kernel<<<grid_for(n), kBlock, 0, st>>>(adj == JG_ADJ_IN ? sh.out_degree.get() : nullptr, c.row_ptr.get(), n,
                                                                 strength.get());
            JG_LAUNCH_CHECK();
        }
        // ---- row classes ----
        {
            DevBuf<uint8_t> flag((size_t)(4 * n));
            DevBuf<int64_t> idx((size_t)n);
            peer_class_kernel<<<grid_for(n), kBlock, 0, st>>>(c.row_ptr.get(), n, flag.get());
            JG_LAUNCH_CHECK();
            for (int k = 0; k < 4; ++k) {
                pl.count[k] = prim::compact_indices(flag.get() + (int64_t)k * n, n, idx.get(), st);
                pl.list[k].alloc((size_t)std::max<int64_t>(pl.count[k], 1));
                if (!pl.count[k]) continue;
                DevBuf<int64_t> entries((size_t)(k == 3 ? pl.count[k] : 0));
                peer_list_kernel<<<grid_for(pl.count[k]), kBlock, 0, st>>>(idx.get(), pl.count[k], c.row_ptr.get(), pl.list[k].get(),
                                                                         entries.get());
                JG_LAUNCH_CHECK();
                if (k < 3) continue;
                pl.off.alloc((size_t)pl.count[k] + 1);
                prim::exclusive_scan(entries.get(), pl.off.get(), pl.count[k], st);
                copy_d2h(&pl.long_entries, pl.off.get() + pl.count[k], sizeof(int64_t), st);
            }
            // every entry and every own vote of a non-empty row belongs to one class
            pl.group_entries = c.nnz + pl.count[0] + pl.count[1] + pl.count[2] + pl.count[3] - pl.long_entries;
        }
        const int lbits = std::max(bits_for((uint64_t)(n - 1)), 1);
        const int kbits = lbits + (pl.count[3] > 1 ? bits_for((uint64_t)(pl.count[3] - 1)) : 0);
        sort_passes = pl.count[3] ? (kbits + 7) / 8 : 0;
        DevBuf<uint64_t> key((size_t)std::max<int64_t>(pl.long_entries, 1));
        DevBuf<uint32_t> val((size_t)(dist ? std::max<int64_t>(pl.long_entries, 1) : 1));
        DevBuf<unsigned long long> sum((size_t)std::max<int64_t>(pl.long_entries, 1));
        DevBuf<unsigned long long> best_sum((size_t)std::max<int64_t>(pl.count[3], 1));
        DevBuf<int32_t> best_lab((size_t)std::max<int64_t>(pl.count[3], 1));
        DevBuf<uint32_t> changed(1);
        // ---- vote supersteps ----
        int cur = 0;
        while (votes < max_iterations) {
            JG_HIP(hipEventRecord(v0, st));
            JG_HIP(hipMemsetAsync(changed.get(), 0, sizeof(uint32_t), st));
            launches += dist ? vote_superstep<true>(c, pl, lab[cur].get(), lab[cur ^ 1].get(), strength.get(), lbits, kbits, key.get(),
                                                    val.get(), sum.get(), best_sum.get(), best_lab.get(), changed.get(), st)
                             : vote_superstep<false>(c, pl, lab[cur].get(), lab[cur ^ 1].get(), nullptr, lbits, kbits, key.get(),
                                                     val.get(), sum.get(), best_sum.get(), best_lab.get(), changed.get(), st);
            JG_HIP(hipEventRecord(v1, st));
            uint32_t moved = 0;
            copy_d2h(&moved, changed.get(), sizeof moved, st);
            float t = 0;
            JG_HIP(hipEventElapsedTime(&t, v0, v1));
            vote_ms += t;
            if (pl.count[3]) dev_cache_sync();  // the sort's temporaries of this superstep serve the next
            cur ^= 1;
            ++votes;
            if (!moved) break;
        }
        // ---- cluster ids in caller order ----
        DevBuf<int64_t> out;
        if (cluster_out) {
            out.alloc((size_t)n);
            peer_out_kernel<<<grid_for(n), kBlock, 0, st>>>(lab[cur].get(), vor.get(), sh.dense_rows.get(), n, out.get());
            JG_LAUNCH_CHECK();
        }
        JG_HIP(hipEventRecord(t1, st));
        region_mark(st, false);
        JG_HIP(hipEventSynchronize(t1));
        JG_HIP(hipEventElapsedTime(&ms, t0, t1));
        if (cluster_out) copy_d2h(cluster_out, out.get(), (size_t)n * sizeof(int64_t), st);
    } else if (max_iterations > 0) {
        votes = 1;  // a superstep over no vertex changes none
    }
    const int iterations = votes + 1 + (dist ? 1 : 0);
    if (iterations_out) *iterations_out = iterations;
    ctx.last = jg_stats{};
    ctx.last.supersteps = iterations;
    ctx.last.levels = votes;
    ctx.last.compute_ms = ms;
    ctx.last.kernel_ms_total = vote_ms;
    ctx.last.kernel_launches = launches;
    ctx.last.edges_traversed = (double)votes * (double)c.nnz;
    // the byte model at the top of this file
    const double w = dist ? 8.0 : 0.0;
    const double group_rows = (double)(pl.count[0] + pl.count[1] + pl.count[2]);
    const double per_vote = group_rows * (28.0 + w) + (double)pl.group_entries * (8.0 + w) +
                            (double)pl.count[3] * (28.0 + w) +
                            (double)pl.long_entries * (8.0 + w + 8.0 + (dist ? 4.0 : 0.0) + sort_passes * (24.0 + (dist ? 8.0 : 0.0)) +
                                                       32.0 + (dist ? 4.0 + w : 0.0));
    ctx.last.algorithmic_bytes = per_vote * (double)votes;
}

}  // namespace jg
