// Stand-alone check of the label-set preparation behind jg_builder_finish_labels (csrc/jg_labelset.h:
// sort, dedup, cap) for AddressSanitizer + UBSan builds on the CPU (tests/test_label_scope_host.py).
// Prints "<checks> checks, <bad> bad"; exit status 1 if any check failed.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "jg_labelset.h"

static int checks = 0, bad = 0;

static void expect(bool ok, const char* what) {
    ++checks;
    if (!ok) {
        ++bad;
        std::printf("FAILED: %s\n", what);
    }
}

int main() {
    using namespace jg;
    std::vector<int64_t> out{1, 2, 3};
    expect(label_set_prepare(nullptr, 3, out) == kLabelSetBadArg && out.empty(), "null labels");
    const int64_t one[] = {42};
    expect(label_set_prepare(one, 0, out) == kLabelSetBadArg, "nlabels = 0");
    expect(label_set_prepare(one, -5, out) == kLabelSetBadArg, "nlabels < 0");
    expect(label_set_prepare(one, 1, out) == kLabelSetOk && out == std::vector<int64_t>{42}, "one label");
    const int64_t lo = std::numeric_limits<int64_t>::min(), hi = std::numeric_limits<int64_t>::max();
    const int64_t ext[] = {hi, 0, lo, hi, -1, lo, 0};
    expect(label_set_prepare(ext, 7, out) == kLabelSetOk && out == std::vector<int64_t>({lo, -1, 0, hi}),
           "extreme values, duplicates");
    // exactly the cap (with every label repeated), then one more
    std::vector<int64_t> in;
    for (int r = 0; r < 3; ++r)
        for (int64_t i = kScopeMaxLabels; i-- > 0;) in.push_back(i * 7 - 100);
    expect(label_set_prepare(in.data(), (int32_t)in.size(), out) == kLabelSetOk && (int)out.size() == kScopeMaxLabels,
           "the cap, repeated");
    for (size_t i = 1; i < out.size(); ++i) expect(out[i - 1] < out[i], "strictly ascending");
    in.push_back(hi);
    expect(label_set_prepare(in.data(), (int32_t)in.size(), out) == kLabelSetTooMany && out.empty(), "one past the cap");
    // random sets against std::set
    std::mt19937_64 rng(7);
    for (int round = 0; round < 200; ++round) {
        const int n = 1 + (int)(rng() % 3000);
        const uint64_t span = 1 + rng() % 2000;
        std::vector<int64_t> v((size_t)n);
        for (auto& x : v) x = (int64_t)(rng() % span) - (int64_t)(span / 2);
        const std::set<int64_t> want(v.begin(), v.end());
        const LabelSetStatus st = label_set_prepare(v.data(), n, out);
        if ((int)want.size() > kScopeMaxLabels)
            expect(st == kLabelSetTooMany && out.empty(), "random: too many");
        else
            expect(st == kLabelSetOk && out == std::vector<int64_t>(want.begin(), want.end()), "random: the sorted set");
    }
    std::printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
