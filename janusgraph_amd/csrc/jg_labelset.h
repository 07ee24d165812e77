// jg_labelset.h — host-side preparation of a label scope (jg_builder_finish_labels): plain C++, no HIP,
// so that it also compiles into a stand-alone program (tests/san/label_set_main.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace jg {

// Labels the scope select stages in LDS (8 KB of the 160 KB a CU has; JG_MAX_SCOPE_LABELS).
constexpr int kScopeMaxLabels = 1024;

enum LabelSetStatus { kLabelSetOk = 0, kLabelSetBadArg = 1, kLabelSetTooMany = 2 };

// out = labels[0, nlabels) sorted ascending without duplicates.  kLabelSetBadArg: null labels or
// nlabels < 1; kLabelSetTooMany: more than kScopeMaxLabels distinct labels (out is left empty).
inline LabelSetStatus label_set_prepare(const int64_t* labels, int32_t nlabels, std::vector<int64_t>& out) {
    out.clear();
    if (!labels || nlabels < 1) return kLabelSetBadArg;
    out.assign(labels, labels + nlabels);
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    if ((int64_t)out.size() > kScopeMaxLabels) {
        out.clear();
        return kLabelSetTooMany;
    }
    return kLabelSetOk;
}

}  // namespace jg
