// jg_scope.hip — the label scope select behind jg_builder_finish_labels: a stable stream compaction of
// the builder's accumulated (src, dst[, w]) by membership of each edge's label in the scope's label set.
//
// Three stream-ordered steps, no workgroup ever waiting on another (no look-back, no spin):
//   1. scope_count_kernel:   kept edges per tile of kScopeTile edges
//   2. prim::exclusive_scan_async over the tile counts -> every tile's first output position
//   3. scope_scatter_kernel: membership evaluated again, src / dst / w of the kept edges written in one pass
// The label set (sorted, distinct, <= kScopeMaxLabels) is staged in LDS; membership is a binary search
// there.  A wave takes kScopeEpt runs of 64 consecutive edges of its tile (coalesced, all label loads in
// flight together), so the order of the kept edges is wave-major, then run, then lane: the rank inside a
// run is popcount(ballot & lanemask_lt), the runs of a wave add up in registers (the ballots are
// wave-uniform), and the waves of a block are ranked by block_exclusive_scan_add.  64-bit indices.
// A numbered scope (jg_builder_keep_scope_ordinals) takes up to three 8-byte columns along in the same scatter:
// each kept edge's position in the accumulated list, its relation id and its decoded double (ScopeCols).
#include "jg_internal.h"
#include "jg_labelset.h"
#include "jg_prim.h"

namespace jg {

namespace {

constexpr int64_t kScopeWaveSpan = (int64_t)kScopeEpt * kWave;  // consecutive edges one wave owns in a tile
static_assert(kScopeTile == kScopeWaveSpan * (kBlock / kWave), "a tile is split evenly over the block's waves");

// the sorted label set into LDS (nset <= kScopeMaxLabels); the caller synchronises
__device__ __forceinline__ void stage_label_set(const int64_t* __restrict__ set, int nset, int64_t* lds_set) {
    for (int i = threadIdx.x; i < nset; i += kBlock) lds_set[i] = set[i];
}

__device__ __forceinline__ bool in_label_set(const int64_t* lds_set, int nset, int64_t x) {
    int lo = 0, hi = nset;  // first position with lds_set[pos] >= x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lds_set[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < nset && lds_set[lo] == x;
}

// The tiles [t0, t1) of block b when ntiles tiles are dealt out in contiguous ranges.
__device__ __forceinline__ void block_tiles(int64_t ntiles, int64_t& t0, int64_t& t1) {
    const int64_t per = (ntiles + gridDim.x - 1) / gridDim.x;
    t0 = (int64_t)blockIdx.x * per;
    t1 = t0 + per < ntiles ? t0 + per : ntiles;
}

__global__ __launch_bounds__(kBlock) void scope_count_kernel(const int64_t* __restrict__ lab, int64_t m,
                                                              const int64_t* __restrict__ set, int nset,
                                                              int64_t ntiles, uint32_t* __restrict__ tile_count) {
    __shared__ int64_t lds_set[kScopeMaxLabels];
    __shared__ uint32_t wave_count[kBlock / kWave];
    stage_label_set(set, nset, lds_set);
    __syncthreads();
    int64_t t0, t1;
    block_tiles(ntiles, t0, t1);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t base = t * kScopeTile + (int64_t)wave_id() * kScopeWaveSpan + lane_id();
        int64_t l[kScopeEpt];
#pragma unroll
        for (int j = 0; j < kScopeEpt; ++j) {
            const int64_t e = base + (int64_t)j * kWave;
            l[j] = e < m ? lab[e] : 0;
        }
        uint32_t cnt = 0;
#pragma unroll
        for (int j = 0; j < kScopeEpt; ++j) {
            const int64_t e = base + (int64_t)j * kWave;
            const bool f = e < m && in_label_set(lds_set, nset, l[j]);
            cnt += (uint32_t)__popcll(__ballot(f));
        }
        if (lane_id() == 0) wave_count[wave_id()] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t sum = 0;
#pragma unroll
            for (int w = 0; w < kBlock / kWave; ++w) sum += wave_count[w];
            tile_count[t] = sum;
        }
        __syncthreads();
    }
}

// kCols: the numbered scope's flavour.  Its columns are each optional (a null output: not asked for; the checks
// are kernel arguments, so wave-uniform).  A column is loaded and stored in a phase of its own behind src / dst /
// w, reusing the flags and ranks.  The compiler hoists the later phases' loads above the earlier stores, so the
// flavour does hold more live values than the plain one: 114 / 122 VGPRs against 67 / 75 (no scratch; 4 waves per
// SIMD against 7 / 6).  The plain flavours' code is what it was.
template <bool kWeights, bool kCols>
__global__ __launch_bounds__(kBlock) void scope_scatter_kernel(const int64_t* __restrict__ lab,
                                                                const int64_t* __restrict__ src,
                                                                const int64_t* __restrict__ dst,
                                                                const int32_t* __restrict__ w, int64_t m,
                                                                const int64_t* __restrict__ set, int nset,
                                                                int64_t ntiles, const int64_t* __restrict__ tile_off,
                                                                int64_t kept, int64_t* __restrict__ osrc,
                                                                int64_t* __restrict__ odst, int32_t* __restrict__ ow,
                                                                const int64_t* __restrict__ rel,
                                                                const double* __restrict__ wf,
                                                                int64_t* __restrict__ opos,
                                                                int64_t* __restrict__ orel,
                                                                double* __restrict__ owf) {
    __shared__ int64_t lds_set[kScopeMaxLabels];
    __shared__ uint32_t scan_scratch[kBlock / kWave];
    stage_label_set(set, nset, lds_set);
    __syncthreads();
    int64_t t0, t1;
    block_tiles(ntiles, t0, t1);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t base = t * kScopeTile + (int64_t)wave_id() * kScopeWaveSpan + lane_id();
        int64_t l[kScopeEpt];
#pragma unroll
        for (int j = 0; j < kScopeEpt; ++j) {
            const int64_t e = base + (int64_t)j * kWave;
            l[j] = e < m ? lab[e] : 0;
        }
        bool f[kScopeEpt];
        uint32_t rank[kScopeEpt];  // position among the wave's kept edges of this tile
        uint32_t wave_total = 0;
        const uint64_t below = lanemask_lt();
#pragma unroll
        for (int j = 0; j < kScopeEpt; ++j) {
            const int64_t e = base + (int64_t)j * kWave;
            f[j] = e < m && in_label_set(lds_set, nset, l[j]);
            const uint64_t b = __ballot(f[j]);
            rank[j] = wave_total + (uint32_t)__popcll(b & below);
            wave_total += (uint32_t)__popcll(b);
        }
        // the wave's total sits on its last lane, so every lane's exclusive prefix is the sum of the waves before it
        uint32_t tile_total;
        const uint32_t wave_off =
            block_exclusive_scan_add<uint32_t>(lane_id() == kWave - 1 ? wave_total : 0u, scan_scratch, &tile_total);
        const int64_t out0 = tile_off[t] + wave_off;
        int64_t a[kScopeEpt], b[kScopeEpt];
        int32_t c[kScopeEpt];
#pragma unroll
        for (int j = 0; j < kScopeEpt; ++j) {
            const int64_t e = base + (int64_t)j * kWave;
            if (f[j]) {
                a[j] = src[e];
                b[j] = dst[e];
                if (kWeights) c[j] = w[e];
            }
        }
#pragma unroll
        for (int j = 0; j < kScopeEpt; ++j) {
            const int64_t o = out0 + rank[j];
            if (f[j] && o < kept) {  // o < kept always holds (the counts come from the same predicate)
                osrc[o] = a[j];
                odst[o] = b[j];
                if (kWeights) ow[o] = c[j];
            }
        }
        if (kCols) {
            if (opos) {
#pragma unroll
                for (int j = 0; j < kScopeEpt; ++j) {
                    const int64_t o = out0 + rank[j];
                    if (f[j] && o < kept) opos[o] = base + (int64_t)j * kWave;
                }
            }
            if (orel) {
                int64_t r[kScopeEpt];
#pragma unroll
                for (int j = 0; j < kScopeEpt; ++j)
                    if (f[j]) r[j] = rel[base + (int64_t)j * kWave];
#pragma unroll
                for (int j = 0; j < kScopeEpt; ++j) {
                    const int64_t o = out0 + rank[j];
                    if (f[j] && o < kept) orel[o] = r[j];
                }
            }
            if (owf) {
                double d[kScopeEpt];
#pragma unroll
                for (int j = 0; j < kScopeEpt; ++j)
                    if (f[j]) d[j] = wf[base + (int64_t)j * kWave];
#pragma unroll
                for (int j = 0; j < kScopeEpt; ++j) {
                    const int64_t o = out0 + rank[j];
                    if (f[j] && o < kept) owf[o] = d[j];
                }
            }
        }
    }
}

}  // namespace

ScopeSelect scope_select(const int64_t* lab, const int64_t* src, const int64_t* dst, const int32_t* w, int64_t m,
                         const std::vector<int64_t>& set, DevBuf<int64_t>& osrc, DevBuf<int64_t>& odst,
                         DevBuf<int32_t>& ow, hipStream_t s, ScopeCols* cols) {
    if (set.empty() || (int64_t)set.size() > kScopeMaxLabels) fail(JG_ERR_ARG, "label set outside [1, JG_MAX_SCOPE_LABELS]");
    ScopeSelect r;
    if (m > 0) {
        const int nset = (int)set.size();
        const int64_t ntiles = (m + kScopeTile - 1) / kScopeTile;
        DevBuf<int64_t> d_set((size_t)nset), tile_off((size_t)ntiles + 1), scratch((size_t)prim::scan_scratch_size(ntiles));
        DevBuf<uint32_t> tile_count((size_t)ntiles);
        copy_h2d(d_set.get(), set.data(), (size_t)nset * sizeof(int64_t), s);
        // a few tiles per block once the device is full (<= 4 blocks of 256 threads on each of the 256 CUs)
        const unsigned grid = (unsigned)std::min<int64_t>(ntiles, 256 * 16);
        // two timed regions, so that the host's read of the kept count between them is not counted
        Event t0, t1, t2, t3;
        JG_HIP(hipEventRecord(t0, s));
        scope_count_kernel<<<grid, kBlock, 0, s>>>(lab, m, d_set.get(), nset, ntiles, tile_count.get());
        JG_LAUNCH_CHECK();
        prim::exclusive_scan_async(tile_count.get(), tile_off.get(), ntiles, scratch.get(), s);
        JG_HIP(hipEventRecord(t1, s));
        int64_t kept = 0;
        copy_d2h(&kept, tile_off.get() + ntiles, sizeof kept, s);
        if (kept < 0 || kept > m) fail(JG_ERR_HIP, "label scope select: kept count out of range");
        r.kept = kept;
        r.launches = 1;  // the select's own kernels: the count, then the scatter (the scan's are the primitive's)
        JG_HIP(hipEventElapsedTime(&r.ms, t0, t1));
        if (kept > 0) {
            osrc.alloc((size_t)kept);
            odst.alloc((size_t)kept);
            if (w) ow.alloc((size_t)kept);
            if (cols) {
                cols->opos.alloc((size_t)kept);
                if (cols->rel) cols->orel.alloc((size_t)kept);
                if (cols->wf) cols->owf.alloc((size_t)kept);
            }
            JG_HIP(hipEventRecord(t2, s));
            const auto launch = [&](auto kernel) {
                kernel<<<grid, kBlock, 0, s>>>(lab, src, dst, w, m, d_set.get(), nset, ntiles, tile_off.get(), kept,
                                               osrc.get(), odst.get(), w ? ow.get() : nullptr, cols ? cols->rel : nullptr,
                                               cols ? cols->wf : nullptr, cols ? cols->opos.get() : nullptr,
                                               cols && cols->rel ? cols->orel.get() : nullptr,
                                               cols && cols->wf ? cols->owf.get() : nullptr);
            };
            if (cols) {
                if (w) launch(scope_scatter_kernel<true, true>);
                else launch(scope_scatter_kernel<false, true>);
            } else {
                if (w) launch(scope_scatter_kernel<true, false>);
                else launch(scope_scatter_kernel<false, false>);
            }
            JG_LAUNCH_CHECK();
            r.launches = 2;
            JG_HIP(hipEventRecord(t3, s));
            JG_HIP(hipEventSynchronize(t3));
            float ms2 = 0;
            JG_HIP(hipEventElapsedTime(&ms2, t2, t3));
            r.ms += ms2;
        }
        const double payload = w ? 20.0 : 16.0;
        r.bytes = 16.0 * (double)m + 2.0 * payload * (double)kept;
        // a numbered scope: positions are written only (8 B), a relation id or a double is read and written (16 B)
        if (cols) r.bytes += (8.0 + (cols->rel ? 16.0 : 0.0) + (cols->wf ? 16.0 : 0.0)) * (double)kept;
    }
    if (cols) {
        if (cols->opos.size() == 0) cols->opos.alloc(1);
        if (cols->rel && cols->orel.size() == 0) cols->orel.alloc(1);
        if (cols->wf && cols->owf.size() == 0) cols->owf.alloc(1);
    }
    if (osrc.size() == 0) osrc.alloc(1);
    if (odst.size() == 0) odst.alloc(1);
    if (w && ow.size() == 0) ow.alloc(1);
    return r;
}

}  // namespace jg
