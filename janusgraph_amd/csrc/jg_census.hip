// jg_census.hip — the component census of a ConnectedComponentVertexProgram run (jg_cc_census): one
// (component id, population) pair per component, largest first, made on the device from the labels the
// program leaves there, so that no per-vertex array crosses to the host ("Component census on
// the device").
//
// One shard.  The labels are String-order ranks (jg_cc.hip): `label[0, lrows)` for the rows the program
// labelled, `rank0[lrows, rows)` for the union-find's edgeless suffix, whose rows are their own components.
//   count   cnt[r] = vertices labelled r, one pass over the rows.  Rows of row 0's component (the
//           highest-degree row: the giant component of a power-law graph) are counted from ballot
//           popcounts, summed per wave and per block: one atomic per block.  The other lanes of a wave
//           that carry the same label merge into one add (peer masks over the label's bits, as the radix
//           sort's match_digit does for a digit): one atomic per distinct label per wave.  A row of the
//           edgeless suffix stores its own counter plainly.  Nothing depends on row 0's component being the
//           largest: it is only the label whose adds are merged across a block instead of across a wave.
//   select  the counters >= min_population, compacted in rank order: a pass over tiles of kCensusTile
//           counters leaves each tile's listed count (and adds up the components and the largest
//           population), a scan of the tile counts gives each tile's first slot, a second pass applies the
//           same predicate to the same counters and stores (largest - population, rank) records.
//   order   a stable radix sort of the records by largest - population on bits(largest) bits: population
//           descending, rank order (the labels' String order) surviving inside ties.  The emit pass turns
//           each rank into its vertex id (Graph::cc_vor) and stores the held (id, population) arrays.
// No kernel reads a value that it or a concurrent launch writes: the count pass only adds to / stores cnt
// (a suffix rank is never the label of a row with edges, so the plain stores and the atomics never share a
// counter), the select passes only read it.
#include "jg_internal.h"
#include "jg_prim.h"

namespace jg {
namespace {

constexpr int kCensusItems = 8;                        // consecutive counters per thread of the select passes
constexpr int kCensusTile = kBlock * kCensusItems;     // 2048

// Lanes of the calling wave whose label equals this lane's (only lanes with `valid`): match_digit
// (jg_prim.hip) over the `bits` bits a label can have.
__device__ __forceinline__ uint64_t match_label(uint32_t label, bool valid, int bits) {
    uint64_t peers = __ballot(valid);
    for (int b = 0; b < bits; ++b) {
        const bool bit = (label >> b) & 1u;
        const uint64_t ball = __ballot(bit);
        peers &= bit ? ball : ~ball;
    }
    return peers;
}

// cnt[label[l]] += 1 for l in [0, lrows) (lrows > 0; cnt[0, n) zeroed before).  A label outside [0, n) is
// never used as an index: it is counted in *bad, and the call fails.
__global__ __launch_bounds__(kBlock) void census_count_kernel(const int32_t* __restrict__ label, int64_t lrows,
                                                              uint32_t* __restrict__ cnt, uint32_t n, int bits,
                                                              unsigned long long* __restrict__ bad) {
    __shared__ uint32_t red[kBlock / kWave];
    const int32_t gl = label[0];
    uint32_t giant = 0;  // wave-uniform: this wave's rows of row 0's component
    constexpr int R = 4;  // 64-row groups per wave and trip, their label loads issued together
    const int64_t span = (int64_t)blockDim.x * R;
    for (int64_t x0 = (int64_t)blockIdx.x * span; x0 < lrows; x0 += (int64_t)gridDim.x * span) {  // block-uniform
        int32_t labs[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int64_t l = x0 + (int64_t)k * blockDim.x + threadIdx.x;
            labs[k] = l < lrows ? __builtin_nontemporal_load(&label[l]) : gl;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int64_t l = x0 + (int64_t)k * blockDim.x + threadIdx.x;
            const bool valid = l < lrows;
            const int32_t lab = labs[k];
            giant += (uint32_t)__popcll(__ballot(valid && lab == gl));
            bool other = valid && lab != gl;
            if (other && (uint32_t)lab >= n) {
                atomicAdd(bad, 1ull);
                other = false;
            }
            const uint64_t rest = __ballot(other);
            if (rest == 0) continue;  // wave-uniform
            // a wave inside one other component: a single add, without the bit loop
            const int32_t first = __shfl(lab, __ffsll((unsigned long long)rest) - 1, kWave);
            uint64_t peers = __ballot(other && lab == first);
            if (peers != rest) peers = match_label((uint32_t)lab, other, bits);
            if (other && (peers & lanemask_lt()) == 0) atomicAdd(&cnt[lab], (uint32_t)__popcll(peers));
        }
    }
    if (lane_id() == 0) red[wave_id()] = giant;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kBlock / kWave; ++w) t += red[w];
        if ((uint32_t)gl >= n) atomicAdd(bad, 1ull);
        else if (t) atomicAdd(&cnt[gl], t);
    }
}

// the edgeless suffix: row l in [lrows, rows) is the only vertex labelled rank0[l]
__global__ void census_suffix_kernel(const int32_t* __restrict__ rank0, int64_t lrows, int64_t rows,
                                     uint32_t* __restrict__ cnt) {
    for (int64_t l = lrows + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < rows; l += (int64_t)gridDim.x * blockDim.x)
        if ((uint64_t)rank0[l] < (uint64_t)rows) cnt[rank0[l]] = 1u;  // always (cc_prepare_ranks): a bound, not a case
}

// Tile b = counters [b * kCensusTile, ...): tile_listed[b] = those >= min_population; tot[0] += the
// non-zero ones (the components), tot[1] = max(the largest population).
__global__ __launch_bounds__(kBlock) void census_tile_kernel(const uint32_t* __restrict__ cnt, int64_t n,
                                                             int64_t min_population, uint32_t* __restrict__ tile_listed,
                                                             unsigned long long* __restrict__ tot) {
    __shared__ uint32_t red[3][kBlock / kWave];
    const int64_t base = (int64_t)blockIdx.x * kCensusTile + (int64_t)threadIdx.x * kCensusItems;
    uint32_t listed = 0, comps = 0, mx = 0;
#pragma unroll
    for (int k = 0; k < kCensusItems; ++k) {
        const int64_t i = base + k;
        const uint32_t c = i < n ? cnt[i] : 0u;
        listed += (int64_t)c >= min_population ? 1u : 0u;
        comps += c ? 1u : 0u;
        mx = c > mx ? c : mx;
    }
    listed = wave_reduce_add(listed);
    comps = wave_reduce_add(comps);
    mx = wave_reduce_max(mx);
    if (lane_id() == 0) {
        red[0][wave_id()] = listed;
        red[1][wave_id()] = comps;
        red[2][wave_id()] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        listed = comps = mx = 0;
        for (int w = 0; w < kBlock / kWave; ++w) {
            listed += red[0][w];
            comps += red[1][w];
            mx = red[2][w] > mx ? red[2][w] : mx;
        }
        tile_listed[blockIdx.x] = listed;
        if (comps) {
            atomicAdd(&tot[0], (unsigned long long)comps);
            atomicMax(&tot[1], (unsigned long long)mx);
        }
    }
}

// The listed counters of tile b, in rank order, from slot tile_off[b] on: key = largest - population, val = rank.
__global__ __launch_bounds__(kBlock) void census_scatter_kernel(const uint32_t* __restrict__ cnt, int64_t n,
                                                                int64_t min_population,
                                                                const int64_t* __restrict__ tile_off, uint32_t largest,
                                                                uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    __shared__ int32_t scratch[kBlock / kWave];
    const int64_t off = tile_off[blockIdx.x];
    if (tile_off[blockIdx.x + 1] == off) return;  // block-uniform: nothing listed in this tile
    const int64_t base = (int64_t)blockIdx.x * kCensusTile + (int64_t)threadIdx.x * kCensusItems;
    uint32_t c[kCensusItems];
    int32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kCensusItems; ++k) {
        const int64_t i = base + k;
        c[k] = i < n ? cnt[i] : 0u;
        mine += (int64_t)c[k] >= min_population ? 1 : 0;
    }
    int32_t total;
    int64_t pos = off + block_exclusive_scan_add(mine, scratch, &total);
#pragma unroll
    for (int k = 0; k < kCensusItems; ++k) {
        if ((int64_t)c[k] >= min_population) {
            key[pos] = (uint64_t)(largest - c[k]);
            val[pos] = (uint32_t)(base + k);
            ++pos;
        }
    }
}

__global__ void census_emit_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t listed,
                                   uint32_t largest, const int64_t* __restrict__ vor, int64_t* __restrict__ vid_out,
                                   int64_t* __restrict__ pop_out) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < listed; j += (int64_t)gridDim.x * blockDim.x) {
        vid_out[j] = vor[val[j]];
        pop_out[j] = (int64_t)largest - (int64_t)key[j];
    }
}

struct CensusRun {
    int64_t components = 0, listed = 0, largest = 0;
    float ms = 0;
    double bytes = 0;
};

// The census of label[0, lrows) + rank0[lrows, rows) on the shard's stream; the held arrays land in
// sh.census_vid / census_pop.  Every other buffer is a temporary of this function.
CensusRun census_of_labels(Graph& g, Shard& sh, const int32_t* label, int64_t lrows, int64_t min_population) {
    CensusRun r;
    DeviceGuard dg(sh);
    hipStream_t st = sh.stream;
    const int64_t n = sh.rows;
    if (n == 0) {
        sh.census_vid.alloc(1);
        sh.census_pop.alloc(1);
        return r;
    }
    Event c0, c1;
    JG_HIP(hipEventRecord(c0, st));
    const int bits = std::max(bits_for((uint64_t)(n - 1)), 1);
    const int64_t tiles = (n + kCensusTile - 1) / kCensusTile;
    DevBuf<uint32_t> cnt((size_t)n), tile_listed((size_t)tiles);
    DevBuf<int64_t> tile_off((size_t)tiles + 1);
    DevBuf<unsigned long long> tot(3);  // components, largest population, labels out of range
    JG_HIP(hipMemsetAsync(cnt.get(), 0, cnt.bytes(), st));
    JG_HIP(hipMemsetAsync(tot.get(), 0, tot.bytes(), st));
    // ---- count ----
    if (lrows > 0) {
        census_count_kernel<<<grid_for((lrows + 3) / 4, kBlock, 2048), kBlock, 0, st>>>(label, lrows, cnt.get(), (uint32_t)n, bits,
                                                                                         tot.get() + 2);
        JG_LAUNCH_CHECK();
    }
    // a suffix row is a component of population 1: with min_population > 1 none is listed, and they are
    // counted below without their counters (34 M scattered stores at RMAT-26)
    const bool suffix_counters = min_population == 1;
    if (lrows < n && suffix_counters) {
        census_suffix_kernel<<<grid_for(n - lrows), kBlock, 0, st>>>(sh.cc_rank0.get(), lrows, n, cnt.get());
        JG_LAUNCH_CHECK();
    }
    // ---- select ----
    census_tile_kernel<<<(unsigned)tiles, kBlock, 0, st>>>(cnt.get(), n, min_population, tile_listed.get(), tot.get());
    JG_LAUNCH_CHECK();
    prim::exclusive_scan(tile_listed.get(), tile_off.get(), tiles, st);
    unsigned long long htot[3] = {0, 0, 0};
    copy_d2h(htot, tot.get(), sizeof htot, st);
    if (htot[2]) fail(JG_ERR_STATE, "jg_cc_census: a component label lies outside the vertex ranks");
    int64_t listed = 0;
    copy_d2h(&listed, tile_off.get() + tiles, sizeof(int64_t), st);
    if (lrows < n && !suffix_counters) {
        htot[0] += (unsigned long long)(n - lrows);
        if (htot[1] < 1) htot[1] = 1;
    }
    r.components = (int64_t)htot[0];
    r.largest = (int64_t)htot[1];
    r.listed = listed;
    const uint32_t largest = (uint32_t)htot[1];
    const int kbits = std::max(bits_for((uint64_t)largest), 1);
    sh.census_vid.alloc((size_t)std::max<int64_t>(listed, 1));
    sh.census_pop.alloc((size_t)std::max<int64_t>(listed, 1));
    if (listed > 0) {
        DevBuf<uint64_t> key((size_t)listed);
        DevBuf<uint32_t> val((size_t)listed);
        census_scatter_kernel<<<(unsigned)tiles, kBlock, 0, st>>>(cnt.get(), n, min_population, tile_off.get(), largest,
                                                                 key.get(), val.get());
        JG_LAUNCH_CHECK();
        // ---- order ----
        prim::radix_sort(key.get(), val.get(), listed, kbits, st);
        census_emit_kernel<<<grid_for(listed), kBlock, 0, st>>>(key.get(), val.get(), listed, largest, g.cc_vor.get(),
                                                               sh.census_vid.get(), sh.census_pop.get());
        JG_LAUNCH_CHECK();
    }
    JG_HIP(hipEventRecord(c1, st));
    JG_HIP(hipEventSynchronize(c1));
    JG_HIP(hipEventElapsedTime(&r.ms, c0, c1));
    // Byte model.  Counters: zeroed (4 B per vertex), read by both select passes (8 B).  Count: a label read
    // per labelled row (4 B; the merged adds are not counted), a rank read and a counter store per suffix row
    // (8 B; min_population 1 only).  A listed component: its sort record stored (12 B), per 8-bit sort pass read twice and written
    // once (8 + 12 + 12 B), then read, its id gathered and the pair stored (12 + 8 + 16 B).
    const int passes = (kbits + 7) / 8;
    r.bytes = 12.0 * (double)n + 4.0 * (double)lrows + (suffix_counters ? 8.0 * (double)(n - lrows) : 0.0) +
              (double)listed * (48.0 + 32.0 * (double)passes);
    return r;
}

}  // namespace

void cc_census_drop(Graph& g) {
    for (auto& sp : g.shards) {
        DeviceGuard dg(*sp);
        sp->census_vid.reset();
        sp->census_pop.reset();
    }
    g.census_listed = -1;
}

void cc_census(Graph& g, int64_t min_population, int32_t* iterations_out, int64_t* components_out, int64_t* listed_out,
               int64_t* largest_out, double* census_ms_out) {
    cc_census_drop(g);  // a failed call leaves no census held
    if (min_population < 1) fail(JG_ERR_ARG, "jg_cc_census: min_population must be at least 1");
    if (g.P != 1 || g.shards.size() != 1)
        fail(JG_ERR_UNSUPPORTED,
             "jg_cc_census runs on one shard (sharded graphs: jg_connected_components, grouped on the host)");
    Shard& sh = *g.shards[0];
    if (sh.rows != g.n) fail(JG_ERR_UNSUPPORTED, "jg_cc_census: the shard does not hold every vertex");
    CensusRun r;
    const CcLabelHook hook = [&](const int32_t* label, int64_t lrows) {
        r = census_of_labels(g, sh, label, lrows, min_population);
    };
    try {
        cc_run(g, nullptr, iterations_out, &hook);
    } catch (...) {
        cc_census_drop(g);
        throw;
    }
    g.census_listed = r.listed;
    g.ctx->last.algorithmic_bytes += r.bytes;
    if (components_out) *components_out = r.components;
    if (listed_out) *listed_out = r.listed;
    if (largest_out) *largest_out = r.largest;
    if (census_ms_out) *census_ms_out = (double)r.ms;
}

void cc_census_read(Graph& g, int64_t first, int64_t count, int64_t* vid_out, int64_t* pop_out) {
    if (g.census_listed < 0) fail(JG_ERR_STATE, "no component census is held (jg_cc_census)");
    if (first < 0 || count < 0 || first > g.census_listed || count > g.census_listed - first)
        fail(JG_ERR_ARG, "range outside the listed components");
    if (count == 0) return;
    Shard& sh = *g.shards[0];
    DeviceGuard dg(sh);
    hipStream_t st = sh.stream;
    if (vid_out) copy_d2h(vid_out, sh.census_vid.get() + first, (size_t)count * sizeof(int64_t), st);
    if (pop_out) copy_d2h(pop_out, sh.census_pop.get() + first, (size_t)count * sizeof(int64_t), st);
}

}  // namespace jg
