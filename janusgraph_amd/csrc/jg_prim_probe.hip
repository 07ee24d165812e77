// jg_prim_probe.hip — jg_tune_set("prim_probe", op | pattern << 4 | bits << 8 | n << 16) (tests): one primitive of
// jg_prim.hip on one generated input, compared element for element with plain host code.
//
// jg::prim is not on the C ABI, and the programs reach it at sizes their graphs happen to give.  The probe runs
// one primitive at a size the caller picks, so a test can sit on the tile structure: kScanTile = 2048 (two scan
// levels above it, three above 2048^2), kRadixTile = 4096 keys (1024 per wave in 16 rounds of 64; the count table's
// scan goes to two levels from 9 tiles on), the copy-back after an odd number of 8-bit passes, and the scratch
// layout of the asynchronous scans.  The input comes from a fixed splitmix64 stream of the element index, the
// primitive runs on a non-blocking stream of the probe's own on the calling thread's current device, and what is
// expected comes from jg_prim_probe_host.h (std::stable_sort, a running int64_t sum, a loop over the flags): never
// from a second device run.  A difference is JG_ERR_STATE with the op, n, bits, the first differing index and
// what was got and wanted; a bad argument is JG_ERR_ARG before the device is touched.  Nothing is kept.
#include "jg_prim.h"
#include "jg_prim_probe_host.h"
#include "janusgpu.h"

namespace jg {
namespace prim {

namespace {

using namespace probe;

constexpr int64_t kGuard = 64;                                    // canary elements behind every checked buffer
constexpr int64_t kCanary = (int64_t)0xA5C3A5C3A5C3A5C3ull;       // no scan total, index or offset here equals it

struct ProbeStream {
    hipStream_t s = nullptr;
    ProbeStream() { JG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~ProbeStream() {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
};

[[noreturn]] void mismatch(const Spec& sp, const std::string& what) { fail(JG_ERR_STATE, describe(sp) + ": " + what); }

template <typename T>
std::string got_wanted(const char* name, int64_t i, T got, T want) {
    return std::string(name) + "[" + std::to_string(i) + "] is " + std::to_string(got) + ", not " + std::to_string(want);
}

template <typename T>
void upload(DevBuf<T>& d, const std::vector<T>& h, hipStream_t s) {
    d.alloc(h.size());
    copy_h2d(d.get(), h.data(), h.size() * sizeof(T), s);
}

template <typename T>
std::vector<T> download(const DevBuf<T>& d, hipStream_t s) {
    std::vector<T> h(d.size());
    copy_d2h(h.data(), d.get(), h.size() * sizeof(T), s);
    return h;
}

// `count` checked elements followed by kGuard canaries, the whole buffer canary-filled at first
DevBuf<int64_t> guarded(int64_t count, hipStream_t s) {
    DevBuf<int64_t> d;
    upload(d, std::vector<int64_t>((size_t)(count + kGuard), kCanary), s);
    return d;
}

void check_guard(const Spec& sp, const char* name, const std::vector<int64_t>& h, int64_t count) {
    for (int64_t i = count; i < (int64_t)h.size(); ++i)
        if (h[(size_t)i] != kCanary)
            mismatch(sp, std::string(name) + " was written " + std::to_string(i - count) + " elements past its " +
                             std::to_string(count) + " (" + std::to_string(h[(size_t)i]) + ")");
}

template <typename T>
void probe_scan(const Spec& sp, bool async, hipStream_t s) {
    const int64_t n = sp.n;
    const std::vector<T> in = scan_input<T>(sp.pattern, n);
    const std::vector<int64_t> want = scan_reference(in);
    DevBuf<T> din;
    upload(din, in, s);
    DevBuf<int64_t> out = guarded(n + 1, s);
    if constexpr (std::is_same_v<T, uint8_t> || std::is_same_v<T, uint32_t>) {
        if (async) {
            const int64_t need = scan_scratch_size(n);
            DevBuf<int64_t> scratch = guarded(need, s);
            exclusive_scan_async(din.get(), out.get(), n, scratch.get(), s);
            JG_HIP(hipStreamSynchronize(s));
            check_guard(sp, "the scan scratch", download(scratch, s), need);
        }
    }
    if constexpr (!std::is_same_v<T, uint8_t>) {
        if (!async) exclusive_scan(din.get(), out.get(), n, s);
    }
    const std::vector<int64_t> got = download(out, s);
    const int64_t i = first_difference(got.data(), want.data(), n + 1);
    if (i >= 0) mismatch(sp, got_wanted("out", i, got[(size_t)i], want[(size_t)i]) + (i == n ? " (the total)" : ""));
    check_guard(sp, "out", got, n + 1);
}

void probe_sort(const Spec& sp, hipStream_t s) {
    const int64_t n = sp.n;
    const bool pairs = sp.op == kSortPairs;
    const std::vector<uint64_t> keys = sort_keys(sp.pattern, sp.bits, n);
    const std::vector<uint32_t> perm = sort_reference(keys);
    DevBuf<uint64_t> dk;
    DevBuf<uint32_t> dv;
    upload(dk, keys, s);
    if (pairs) {
        std::vector<uint32_t> vals((size_t)n);
        for (int64_t i = 0; i < n; ++i) vals[(size_t)i] = (uint32_t)i;
        upload(dv, vals, s);
    }
    radix_sort(dk.get(), pairs ? dv.get() : nullptr, n, sp.bits, s);
    const std::vector<uint64_t> gk = download(dk, s);
    for (int64_t j = 0; j < n; ++j)
        if (gk[(size_t)j] != keys[perm[(size_t)j]]) mismatch(sp, got_wanted("keys", j, gk[(size_t)j], keys[perm[(size_t)j]]));
    if (pairs) {
        const std::vector<uint32_t> gv = download(dv, s);
        const int64_t j = first_difference(gv.data(), perm.data(), n);
        if (j >= 0) mismatch(sp, got_wanted("vals", j, gv[(size_t)j], perm[(size_t)j]));
    }
}

void check_compaction(const Spec& sp, const char* call, int64_t count, const std::vector<int64_t>& got,
                      const std::vector<int64_t>& want) {
    if (count != (int64_t)want.size())
        mismatch(sp, std::string(call) + " returned " + std::to_string(count) + ", not " + std::to_string(want.size()));
    const int64_t i = first_difference(got.data(), want.data(), count);
    if (i >= 0) mismatch(sp, std::string(call) + ": " + got_wanted("idx_out", i, got[(size_t)i], want[(size_t)i]));
    check_guard(sp, "idx_out", got, count);  // nothing behind the count either
}

void probe_compact(const Spec& sp, hipStream_t s) {
    const int64_t n = sp.n;
    const bool scratch = sp.op == kCompactScratch;
    const std::vector<uint8_t> flags = flag_input(sp.pattern, n, !scratch);
    DevBuf<uint8_t> df;
    upload(df, flags, s);
    if (!scratch) {
        DevBuf<int64_t> idx = guarded(n, s);
        const int64_t count = compact_indices(df.get(), n, idx.get(), s);
        check_compaction(sp, "compact_indices(n)", count, download(idx, s), compact_reference(flags, n));
        return;
    }
    DevBuf<int64_t> pos, scan;  // grown by the first call, reused (or grown again) by the second
    for (const int64_t k : {n / 2, n}) {
        DevBuf<int64_t> idx = guarded(k, s);
        const int64_t count = compact_indices(df.get(), k, idx.get(), pos, scan, s);
        check_compaction(sp, k == n ? "compact_indices(n)" : "compact_indices(n / 2)", count, download(idx, s),
                         compact_reference(flags, k));
    }
}

}  // namespace

void prim_probe(int64_t value) {
    Spec sp;
    const std::string bad = unpack(value, &sp);
    if (!bad.empty()) fail(JG_ERR_ARG, "prim_probe: " + bad);
    ProbeStream ps;  // destroyed after every buffer below
    switch (sp.op) {
        case kScanI32: probe_scan<int32_t>(sp, false, ps.s); break;
        case kScanI64: probe_scan<int64_t>(sp, false, ps.s); break;
        case kScanU32: probe_scan<uint32_t>(sp, false, ps.s); break;
        case kScanAsyncU8: probe_scan<uint8_t>(sp, true, ps.s); break;
        case kScanAsyncU32: probe_scan<uint32_t>(sp, true, ps.s); break;
        case kSortKeys:
        case kSortPairs: probe_sort(sp, ps.s); break;
        default: probe_compact(sp, ps.s); break;
    }
}

}  // namespace prim
}  // namespace jg
