// lm_mask_plan.h — what the index builder (lm_builder.hip) asks of a mask set before any kernel sees it, and the table the
// kernels find the masks of a p-base prefix in.  One rule for every front end: a set generated here, a caller's set
// (lm_index_builder_new_masks) and the masks of a resident index that is extended, joined or taken as a model.  Host-only and
// free of HIP, so that it is tested without a device (tests/mask_plan_host.cpp).
//   k in [10, 32] (index.go: the reference's range); 4 .. 65535 masks (a seed names its mask in 16 bits); strictly ascending
//   and below 4^k (what lm_format.cpp asks of a masks.bin); p = max(floor(log4 n), 1) (lib-index-search.go:467-469); every
//   p-base prefix has a mask (the reference's behaviour for a prefix without one cannot be determined from its tree) and none
//   has more than 32 (the width of the bit set desert_capturing_mask sweeps a window with).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace lm {

enum { MASK_PLAN_MIN_K = 10, MASK_PLAN_MAX_K = 32, MASK_PLAN_MIN_MASKS = 4, MASK_PLAN_MAX_MASKS = 65535, MASK_PLAN_MAX_PER_PREFIX = 32 };

struct MaskPlan {
    int p = 0;                      // bases of the mask prefix
    std::vector<int32_t> pfx_first; // [4^p + 1] CSR: the masks of prefix f are [pfx_first[f], pfx_first[f + 1])
    int max_per_prefix = 0;         // the fullest prefix
    bool once_or_twice = false;     // every prefix has one mask or two: the shape of a generated set (k_capture_g<LDS, false>)
};

// floor(log4 n), at least 1, in integers (n >= 1)
static inline int mask_plan_prefix(size_t n) {
    int p = 0;
    while (p < 31 && ((size_t)1 << (2 * (p + 1))) <= n) p++;
    return p < 1 ? 1 : p;
}

// true: `out` is filled.  false: `err` says what is wrong and names the first offending mask (0-based), the first prefix
// without a mask, or the first prefix with too many.
static inline bool plan_masks(int k, const uint64_t *masks, size_t n, MaskPlan &out, std::string &err) {
    out = MaskPlan();
    if (k < MASK_PLAN_MIN_K || k > MASK_PLAN_MAX_K) {
        err = "k = " + std::to_string(k) + " is outside [" + std::to_string((int)MASK_PLAN_MIN_K) + ", " + std::to_string((int)MASK_PLAN_MAX_K) + "]";
        return false;
    }
    if (n < (size_t)MASK_PLAN_MIN_MASKS || n > (size_t)MASK_PLAN_MAX_MASKS || !masks) {
        err = std::to_string(n) + " masks: the number of masks must be in [" + std::to_string((int)MASK_PLAN_MIN_MASKS) + ", " +
              std::to_string((int)MASK_PLAN_MAX_MASKS) + "]";
        return false;
    }
    for (size_t i = 0; i < n; i++) {
        if (k < 32 && (masks[i] >> (2 * k)) != 0) {
            err = "mask " + std::to_string(i) + " is not below 4^k (k = " + std::to_string(k) + ")";
            return false;
        }
        if (i > 0 && masks[i] <= masks[i - 1]) {
            err = "mask " + std::to_string(i) + (masks[i] == masks[i - 1] ? " equals mask " : " is smaller than mask ") + std::to_string(i - 1) +
                  ": the masks must be strictly ascending";
            return false;
        }
    }
    const int p = mask_plan_prefix(n);
    const size_t npfx = (size_t)1 << (2 * p);
    const int shift = (k - p) << 1; // 6 .. 62: p <= 7 for at most 65535 masks, k >= 10
    out.p = p;
    out.pfx_first.assign(npfx + 1, 0);
    for (size_t i = 0; i < n; i++) out.pfx_first[(size_t)(masks[i] >> shift) + 1]++;
    out.once_or_twice = true;
    for (size_t f = 0; f < npfx; f++) {
        const int c = out.pfx_first[f + 1];
        if (c < 1) {
            err = "prefix " + std::to_string(f) + " (of " + std::to_string(npfx) + " prefixes of " + std::to_string(p) + " bases) has no mask";
            return false;
        }
        if (c > (int)MASK_PLAN_MAX_PER_PREFIX) {
            err = "prefix " + std::to_string(f) + " has " + std::to_string(c) + " masks: at most " + std::to_string((int)MASK_PLAN_MAX_PER_PREFIX) + " masks may share a " +
                  std::to_string(p) + "-base prefix";
            return false;
        }
        if (c > out.max_per_prefix) out.max_per_prefix = c;
        if (c > 2) out.once_or_twice = false;
        out.pfx_first[f + 1] += out.pfx_first[f];
    }
    return true;
}

} // namespace lm
