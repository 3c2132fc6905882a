// Host arithmetic that the context-tree translation units share: the dense layout of a (k, D) tree (ctree.hip, ctseq.hip),
// the reference's price of a full subtree (ctree.hip, ctsp.hip) and the split of a sample into workgroup ranges (ctree.hip,
// ctsp.hip).  Host only; the kernel headers do not include it.
#pragma once
#include "../../include/ctree.h"
#include "entry.h"

#include <cmath>
#include <cstdint>

namespace ctree_shape {

// Sizes of a (k, D) tree; pw[d] = k^d, off[d] = first entry of level d in an all-levels table.
struct Shape {
    int64_t pw[26], off[27];
    int64_t bins, nodes, upper;       // k^(D+1); entries of all levels; entries of levels 0..D-1
};

// entry::kOk, or kInvalid / kUnsupported (the value of every family's *_EINVAL / *_EUNSUPPORTED); no message is set: each
// family words its own.
inline int shape_of(int k, int D, Shape* sh) {
    if (k < 1 || D < 1) return entry::kInvalid;
    if (k > CTREE_MAX_K || D > 24) return entry::kUnsupported;
    int64_t p = 1;
    sh->off[0] = 0;
    for (int d = 0; d <= D; ++d) {
        sh->pw[d] = p;
        sh->off[d + 1] = sh->off[d] + p;
        p *= k;
        if (p > CTREE_MAX_SLOTS) return entry::kUnsupported;
    }
    sh->bins = p;
    sh->nodes = sh->off[D + 1];
    sh->upper = sh->off[D];
    return entry::kOk;
}

// hn_g^((k^(D-depth) - 1)/(k - 1) - 1), the reference's price of a full subtree under a missing child of a node at `depth`
// (:757), in the host's binary64 pow as there; k = 1 takes the limit D - depth of the geometric sum.  k^(D-depth) is
// accumulated in binary64, which the sparse engine needs (it overflows int64 there).  Wherever the dense engine runs,
// k^(D+1) <= 2^24: every partial product, p - 1 and k - 1 are integers below 2^53 and so exact, and the one rounding of the
// quotient is the one that the division of the two integers has.
inline double subtree_pow(double hn_g, int k, int D, int depth) {
    double m = (double)(D - depth);
    if (k > 1) {
        double p = 1.0;
        for (int j = 0; j < D - depth; ++j) p *= (double)k;
        m = (p - 1.0) / (double)(k - 1);
    }
    return std::pow(hn_g, m - 1.0);
}

// A count pass over n samples: at most max_slabs workgroups, each given `*span` >= min_span consecutive samples.  Returns
// the number of workgroups.
inline int slab_span(int64_t n, int max_slabs, int64_t min_span, int64_t* span) {
    *span = (n + max_slabs - 1) / max_slabs;
    if (*span < min_span) *span = min_span;
    return (int)((n + *span - 1) / *span);
}

}  // namespace ctree_shape
