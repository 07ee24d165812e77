// jg_prim_probe_host.h — the host half of jg_tune_set("prim_probe", ...): argument unpacking, the input
// generators and the three reference routines the device results are compared with.  Plain C++17, no HIP:
// jg_prim_probe.hip includes it, and tools/micro/prim_probe_host.cpp compiles it alone for the sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <limits>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

namespace jg {
namespace prim {
namespace probe {

enum Op {
    kScanI32 = 0,       // exclusive_scan(int32_t)
    kScanI64 = 1,       // exclusive_scan(int64_t)
    kScanU32 = 2,       // exclusive_scan(uint32_t)
    kScanAsyncU8 = 3,   // exclusive_scan_async(uint8_t)
    kScanAsyncU32 = 4,  // exclusive_scan_async(uint32_t)
    kSortKeys = 5,      // radix_sort, keys only
    kSortPairs = 6,     // radix_sort with vals[i] = i
    kCompactAlloc = 7,  // compact_indices, allocating overload
    kCompactScratch = 8,  // compact_indices, scratch overload: n / 2 flags, then n, same two buffers
    kNumOps = 9
};
constexpr int64_t kMaxN = int64_t(1) << 25;
constexpr int kScanPatterns = 4, kFlagPatterns = 5, kSortPatterns = 6;

struct Spec {
    int op = 0, pattern = 0, bits = 0;
    int64_t n = 0;
};

inline bool is_scan(int op) { return op >= kScanI32 && op <= kScanAsyncU32; }
inline bool is_sort(int op) { return op == kSortKeys || op == kSortPairs; }
inline int patterns_of(int op) { return is_scan(op) ? kScanPatterns : is_sort(op) ? kSortPatterns : kFlagPatterns; }

inline const char* op_name(int op) {
    static const char* const names[kNumOps] = {
        "exclusive_scan<int32>",       "exclusive_scan<int64>", "exclusive_scan<uint32>",
        "exclusive_scan_async<uint8>", "exclusive_scan_async<uint32>", "radix_sort keys",
        "radix_sort pairs",            "compact_indices",       "compact_indices scratch"};
    return op >= 0 && op < kNumOps ? names[op] : "?";
}

// value = op | pattern << 4 | bits << 8 | n << 16.  Returns "" and fills *s, or says what is wrong.
inline std::string unpack(int64_t value, Spec* s) {
    if (value < 0) return "n must not be negative";
    s->op = (int)(value & 15);
    s->pattern = (int)((value >> 4) & 15);
    s->bits = (int)((value >> 8) & 255);
    s->n = value >> 16;
    if (s->op >= kNumOps) return "op must be in [0, 8]";
    if (s->pattern >= patterns_of(s->op))
        return "pattern must be in [0, " + std::to_string(patterns_of(s->op) - 1) + "] for op " + std::to_string(s->op);
    if (s->bits < 1 || s->bits > 64) return "bits must be in [1, 64]";
    if (s->n > kMaxN) return "n must be at most 2^25";
    return "";
}

inline std::string describe(const Spec& s) {
    return std::string("prim_probe: op ") + std::to_string(s.op) + " (" + op_name(s.op) + ") pattern " +
           std::to_string(s.pattern) + " n " + std::to_string(s.n) + " bits " + std::to_string(s.bits);
}

// The fixed stream: element i of stream `salt` is splitmix64's output number i + 1 from seed `salt`.
inline uint64_t mix(uint64_t i, uint64_t salt = 0) {
    uint64_t z = salt + (i + 1) * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// ---- scan inputs ----
// The largest magnitude an int64_t element may have so that every partial sum of n of them is representable
// (the scan's contract: the total fits its int64_t output).
inline int64_t i64_cap(int64_t n) { return std::numeric_limits<int64_t>::max() / std::max<int64_t>(n, 1); }

template <typename T>
T scan_random(uint64_t r, int64_t n) {
    if constexpr (std::is_same_v<T, int64_t>) {
        const int64_t cap = i64_cap(n);  // uniform in [-cap, cap]
        const uint64_t x = r % (2 * (uint64_t)cap + 1);
        return x >= (uint64_t)cap ? (int64_t)(x - (uint64_t)cap) : -(int64_t)((uint64_t)cap - x);
    } else if constexpr (std::is_same_v<T, int32_t>) {
        const uint32_t u = (uint32_t)r;  // the whole range, negatives included
        return u <= 0x7fffffffu ? (int32_t)u : (int32_t)(int64_t(u) - (int64_t(1) << 32));
    } else {
        return (T)r;  // uint32_t up to 2^32 - 1, uint8_t up to 255
    }
}

template <typename T>
T scan_max(int64_t n) {
    if constexpr (std::is_same_v<T, int64_t>) return i64_cap(n);
    else return std::numeric_limits<T>::max();
}

// 0 random over the type's range, 1 all zero, 2 all at the maximum, 3 a single nonzero at the last index
template <typename T>
std::vector<T> scan_input(int pattern, int64_t n) {
    std::vector<T> v((size_t)std::max<int64_t>(n, 0), T(0));
    for (int64_t i = 0; i < n; ++i) {
        if (pattern == 0) v[(size_t)i] = scan_random<T>(mix((uint64_t)i, 1), n);
        else if (pattern == 2) v[(size_t)i] = scan_max<T>(n);
    }
    if (pattern == 3 && n > 0) v[(size_t)n - 1] = std::numeric_limits<T>::max();
    return v;
}

// ---- flags ----
// 0 random (half set), 1 none, 2 all, 3 only index 0, 4 only index n - 1.  any_nonzero: a set flag holds a value in
// 1..255 (the allocating overload's contract is "nonzero"); otherwise 1 (the scratch overload's is "0 or 1").
inline std::vector<uint8_t> flag_input(int pattern, int64_t n, bool any_nonzero) {
    std::vector<uint8_t> f((size_t)std::max<int64_t>(n, 0), 0);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t r = mix((uint64_t)i, 2);
        const bool on = pattern == 0 ? (r & 1) : pattern == 2 ? true : pattern == 3 ? i == 0 : pattern == 4 ? i == n - 1 : false;
        f[(size_t)i] = on ? (any_nonzero ? (uint8_t)(1 + (r >> 8) % 255) : 1) : 0;
    }
    return f;
}

// ---- sort keys, all below 2^bits ----
inline uint64_t low_mask(int bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1ull); }
// The random keys' stream: the first salt at which key 0 exceeds key 1 under every width the tests use (1, 5, 8, 9,
// 16, 33, 40, 64), so that even two keys come out of order and a sort that did nothing shows at n = 2.
constexpr uint64_t kSortSalt = 110;

// 0 random, 1 all equal, 2 ascending, 3 descending, 4 only the top 8-bit digit of `bits` varies, 5 two values
// alternating in runs of 64 (so the 64 keys one wave ranks together share their digit in every pass, and
// consecutive rounds of the wave take turns on two digits).
inline std::vector<uint64_t> sort_keys(int pattern, int bits, int64_t n) {
    const uint64_t mask = low_mask(bits);
    const int top_shift = 8 * ((bits - 1) / 8);  // the last pass reads bits [top_shift, bits)
    const uint64_t low = mix(7, 3) & low_mask(top_shift) & mask;
    const uint64_t a = mix(8, 3) & mask, b = ~a & mask;
    std::vector<uint64_t> k((size_t)std::max<int64_t>(n, 0));
    // ascending: floor(i * 2^bits / n), a non-decreasing map of [0, n) onto [0, 2^bits)
    auto ramp = [&](int64_t i) {
        const unsigned __int128 range = (unsigned __int128)mask + 1;
        return (uint64_t)(((unsigned __int128)(uint64_t)i * range) / (unsigned __int128)(uint64_t)n);
    };
    for (int64_t i = 0; i < n; ++i) {
        uint64_t v = 0;
        switch (pattern) {
            case 0: v = mix((uint64_t)i, kSortSalt) & mask; break;
            case 1: v = a; break;
            case 2: v = ramp(i); break;
            case 3: v = ramp(n - 1 - i); break;
            case 4: v = (((mix((uint64_t)i, 5) << top_shift) & mask) & ~low_mask(top_shift)) | low; break;
            default: v = ((i >> 6) & 1) ? b : a; break;
        }
        k[(size_t)i] = v;
    }
    return k;
}

// ---- references ----
// out[0..n]: out[i] = in[0] + ... + in[i - 1] as a running int64_t sum, out[n] the total.
template <typename T>
std::vector<int64_t> scan_reference(const std::vector<T>& in) {
    std::vector<int64_t> out(in.size() + 1);
    int64_t run = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        out[i] = run;
        run += (int64_t)in[i];
    }
    out[in.size()] = run;
    return out;
}

// The stable order of keys: perm[j] = the input index that lands at j (std::stable_sort on the whole key: the
// keys are below 2^bits, so that is the order of their low `bits` bits).
inline std::vector<uint32_t> sort_reference(const std::vector<uint64_t>& keys) {
    std::vector<uint32_t> perm(keys.size());
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
    return perm;
}

// The indices of the nonzero flags among the first n, ascending.
inline std::vector<int64_t> compact_reference(const std::vector<uint8_t>& flags, int64_t n) {
    std::vector<int64_t> idx;
    for (int64_t i = 0; i < n; ++i)
        if (flags[(size_t)i]) idx.push_back(i);
    return idx;
}

// First index at which got[i] != want[i] over [0, count), or -1.
template <typename T>
int64_t first_difference(const T* got, const T* want, int64_t count) {
    for (int64_t i = 0; i < count; ++i)
        if (got[i] != want[i]) return i;
    return -1;
}

}  // namespace probe
}  // namespace prim
}  // namespace jg
