// prim_probe_host.cpp — the host half of the primitive probe (janusgraph_amd/csrc/jg_prim_probe_host.h) as a
// stand-alone CPU program, for the sanitizers: the generators and the three reference routines the device results
// are compared with are code that can be wrong too.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I janusgraph_amd/csrc
//       tools/micro/prim_probe_host.cpp -o prim_probe_host   (one line), then run ./prim_probe_host
//
// Every generator is run at a handful of sizes around the tiles and checked for what the probe promises of it
// (keys below 2^bits, the ramps monotone, pattern 4 constant below its top digit, flag counts), and every
// reference against a second, slower statement of the same thing (differences of the scan, an insertion sort,
// a membership test).  Prints "ok" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>

#include "jg_prim_probe_host.h"

using namespace jg::prim::probe;

static int failures = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            std::fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                     \
            std::fprintf(stderr, "\n");   \
            ++failures;                   \
        }                                 \
    } while (0)

template <typename T>
static void check_scans(int64_t n) {
    for (int p = 0; p < kScanPatterns; ++p) {
        const std::vector<T> in = scan_input<T>(p, n);
        EXPECT((int64_t)in.size() == n, "pattern %d n %lld", p, (long long)n);
        const std::vector<int64_t> out = scan_reference(in);
        EXPECT((int64_t)out.size() == n + 1 && out[0] == 0, "pattern %d n %lld", p, (long long)n);
        // in wide arithmetic: no partial sum leaves int64_t, and out is its running value
        __int128 run = 0;
        bool same = true, fits = true;
        for (int64_t i = 0; i < n; ++i) {
            same = same && (__int128)out[(size_t)i] == run;
            run += (__int128)in[(size_t)i];
            fits = fits && run <= (__int128)std::numeric_limits<int64_t>::max() &&
                   run >= (__int128)std::numeric_limits<int64_t>::min();
        }
        same = same && (__int128)out[(size_t)n] == run;
        EXPECT(same && fits, "pattern %d n %lld sizeof %zu", p, (long long)n, sizeof(T));
        if (p == 1) EXPECT(out[(size_t)n] == 0, "zeros n %lld", (long long)n);
        if (p == 2 && n > 0) EXPECT(in[0] == scan_max<T>(n) && in[(size_t)n - 1] == in[0], "max n %lld", (long long)n);
        if (p == 3 && n > 0) {
            EXPECT(in[(size_t)n - 1] == std::numeric_limits<T>::max(), "last n %lld", (long long)n);
            EXPECT(out[(size_t)n - 1] == 0 && out[(size_t)n] == (int64_t)std::numeric_limits<T>::max(), "last n %lld",
                   (long long)n);
        }
    }
    if (n >= 4097) {  // the random pattern reaches both halves of the type's range
        const std::vector<T> in = scan_input<T>(0, n);
        const T lo = *std::min_element(in.begin(), in.end()), hi = *std::max_element(in.begin(), in.end());
        if constexpr (!std::is_same_v<T, int64_t>) {
            EXPECT(hi > std::numeric_limits<T>::max() / 2 + std::numeric_limits<T>::max() / 4, "range n %lld", (long long)n);
            if (std::is_signed_v<T>) EXPECT(lo < std::numeric_limits<T>::min() / 2, "range n %lld", (long long)n);
        } else {
            EXPECT(hi > i64_cap(n) / 2 && lo < -(i64_cap(n) / 2) && hi <= i64_cap(n) && lo >= -i64_cap(n), "range n %lld",
                   (long long)n);
        }
    }
}

static void check_flags(int64_t n) {
    for (int any = 0; any < 2; ++any)
        for (int p = 0; p < kFlagPatterns; ++p) {
            const std::vector<uint8_t> f = flag_input(p, n, any != 0);
            const std::vector<int64_t> idx = compact_reference(f, n);
            int64_t set = 0;
            for (uint8_t b : f) {
                set += b != 0;
                if (!any) EXPECT(b <= 1, "pattern %d n %lld", p, (long long)n);
            }
            EXPECT((int64_t)idx.size() == set, "pattern %d n %lld", p, (long long)n);
            std::vector<uint8_t> member((size_t)n, 0);
            for (size_t j = 0; j < idx.size(); ++j) {
                EXPECT(idx[j] >= 0 && idx[j] < n && f[(size_t)idx[j]] != 0, "pattern %d n %lld", p, (long long)n);
                EXPECT(j == 0 || idx[j] > idx[j - 1], "pattern %d n %lld", p, (long long)n);
                member[(size_t)idx[j]] = 1;
            }
            for (int64_t i = 0; i < n; ++i) EXPECT(member[(size_t)i] == (f[(size_t)i] != 0), "pattern %d n %lld", p, (long long)n);
            const int64_t want = p == 1 ? 0 : p == 2 ? n : p >= 3 ? (n > 0) : -1;
            if (want >= 0) EXPECT(set == want, "pattern %d n %lld set %lld", p, (long long)n, (long long)set);
            if (p == 0 && n >= 2047) EXPECT(set > n / 2 - n / 8 && set < n / 2 + n / 8, "half set n %lld", (long long)n);
            if (p == 3 && n > 0) EXPECT(idx[0] == 0, "n %lld", (long long)n);
            if (p == 4 && n > 0) EXPECT(idx[0] == n - 1, "n %lld", (long long)n);
            // the leading half, as op 8 asks first
            const std::vector<int64_t> half = compact_reference(f, n / 2);
            for (size_t j = 0; j < half.size(); ++j) EXPECT(half[j] == idx[j] && half[j] < n / 2, "half n %lld", (long long)n);
        }
}

static void check_sorts(int64_t n, int bits) {
    const uint64_t mask = low_mask(bits);
    for (int p = 0; p < kSortPatterns; ++p) {
        const std::vector<uint64_t> k = sort_keys(p, bits, n);
        EXPECT((int64_t)k.size() == n, "pattern %d", p);
        for (int64_t i = 0; i < n; ++i) EXPECT((k[(size_t)i] & ~mask) == 0, "pattern %d bits %d key %lld", p, bits, (long long)i);
        for (int64_t i = 1; i < n; ++i) {
            if (p == 1) EXPECT(k[(size_t)i] == k[0], "equal");
            if (p == 2) EXPECT(k[(size_t)i] >= k[(size_t)i - 1], "ascending bits %d n %lld", bits, (long long)n);
            if (p == 3) EXPECT(k[(size_t)i] <= k[(size_t)i - 1], "descending bits %d n %lld", bits, (long long)n);
            if (p == 4) EXPECT(((k[(size_t)i] ^ k[0]) & low_mask(8 * ((bits - 1) / 8))) == 0, "top digit only, bits %d", bits);
            if (p == 5) EXPECT((k[(size_t)i] == k[0]) == (((i >> 6) & 1) == 0), "runs of 64, bits %d", bits);
        }
        if (p == 4 && n >= 1024) {
            bool varies = false;
            for (int64_t i = 1; i < n; ++i) varies = varies || k[(size_t)i] != k[0];
            EXPECT(varies, "top digit varies, bits %d", bits);
        }
        if ((p == 2 || p == 3) && n > 1 && bits >= 20) EXPECT(k[0] != k[(size_t)n - 1], "ramp spans, bits %d", bits);
        const std::vector<uint32_t> perm = sort_reference(k);
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int64_t j = 0; j < n; ++j) {
            EXPECT(perm[(size_t)j] < (uint64_t)n && !seen[perm[(size_t)j]], "perm pattern %d", p);
            if (perm[(size_t)j] < (uint64_t)n) seen[perm[(size_t)j]] = 1;
            if (j > 0) {
                const uint64_t a = k[perm[(size_t)j - 1]], b = k[perm[(size_t)j]];
                EXPECT(a < b || (a == b && perm[(size_t)j - 1] < perm[(size_t)j]), "stable order pattern %d bits %d at %lld", p, bits,
                       (long long)j);
            }
        }
        if (n <= 1025) {  // an insertion sort is stable by construction
            std::vector<uint32_t> ins;
            for (int64_t i = 0; i < n; ++i) {
                size_t at = ins.size();
                while (at > 0 && k[ins[at - 1]] > k[(size_t)i]) --at;
                ins.insert(ins.begin() + (std::ptrdiff_t)at, (uint32_t)i);
            }
            EXPECT(ins == perm, "insertion sort pattern %d bits %d n %lld", p, bits, (long long)n);
        }
    }
}

static void check_unpack() {
    Spec s;
    auto pack = [](int64_t op, int64_t pattern, int64_t bits, int64_t n) { return op | pattern << 4 | bits << 8 | n * 65536; };
    EXPECT(unpack(pack(6, 5, 64, kMaxN), &s).empty() && s.op == 6 && s.pattern == 5 && s.bits == 64 && s.n == kMaxN, "max");
    EXPECT(unpack(pack(0, 0, 1, 0), &s).empty() && s.n == 0 && s.bits == 1, "min");
    EXPECT(!unpack(pack(9, 0, 8, 10), &s).empty() && !unpack(pack(15, 0, 8, 10), &s).empty(), "op");
    EXPECT(!unpack(pack(0, 4, 8, 10), &s).empty() && !unpack(pack(7, 5, 8, 10), &s).empty() && !unpack(pack(5, 6, 8, 10), &s).empty(),
           "pattern");
    EXPECT(unpack(pack(0, 3, 8, 10), &s).empty() && unpack(pack(8, 4, 8, 10), &s).empty(), "pattern ok");
    EXPECT(!unpack(pack(0, 0, 0, 10), &s).empty() && !unpack(pack(5, 0, 65, 10), &s).empty() && !unpack(pack(5, 0, 255, 10), &s).empty(),
           "bits");
    EXPECT(!unpack(pack(0, 0, 8, -1), &s).empty() && !unpack(pack(0, 0, 8, kMaxN + 1), &s).empty(), "n");
    EXPECT(!unpack(std::numeric_limits<int64_t>::min(), &s).empty() && !unpack(std::numeric_limits<int64_t>::max(), &s).empty(), "ends");
}

int main() {
    check_unpack();
    for (int64_t n : {0, 1, 7, 9, 257, 2047, 2048, 2049, 4097, 100003}) {
        check_scans<int32_t>(n);
        check_scans<int64_t>(n);
        check_scans<uint32_t>(n);
        check_scans<uint8_t>(n);
        check_flags(n);
    }
    check_scans<int64_t>(2048 * 2048 + 2049);
    check_scans<uint32_t>(2048 * 2048 + 2049);
    check_scans<uint8_t>(kMaxN);
    check_flags(2048 * 2048 + 1);
    for (int bits : {1, 5, 8, 9, 16, 33, 40, 63, 64})
        for (int64_t n : {0, 1, 2, 63, 64, 65, 1025, 4097, 32769}) check_sorts(n, bits);
    check_sorts(100003, 33);
    for (int bits : {1, 5, 8, 9, 16, 33, 40, 64}) {  // kSortSalt: two random keys are out of order at every width
        const std::vector<uint64_t> k = sort_keys(0, bits, 2);
        EXPECT(k[0] > k[1], "bits %d", bits);
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
