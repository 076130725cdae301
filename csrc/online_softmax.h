// Online softmax statistics: a running (max, sum of exp(x - max)) pair, pushed one logit at a time and merged across
// lanes, waves and workgroups.  Shared by the token-NLL kernel (csrc/perplexity.hip) and InfoLM (csrc/infolm.hip).
#pragma once

#include "device_common.h"

namespace tmx {

template <typename A>
struct MaxSum {
  A m, s;
};

template <typename A>
__device__ __forceinline__ void ms_push(MaxSum<A>& a, A x) {
  if (x > a.m) {
    a.s = a.s * exp(a.m - x) + A(1);
    a.m = x;
  } else {
    // A value equal to the maximum adds 1 without forming x - m: a second +inf stays +inf (inf - inf would be NaN).
    // A masked (-inf) logit adds exp(-inf) = 0 under a finite maximum.  While the side is still empty (m = -inf) it
    // counts as 1, which nothing can see: the first real logit scales s by exp(-inf - x) = 0, a merge scales an empty
    // side by exp(-inf) = 0, and a row of nothing else ends as -inf + log s = -inf (NaN after the target's -inf).
    // No separate test for -inf in the loop.  A NaN logit makes s NaN for good, whatever the maximum is.
    a.s += x == a.m ? A(1) : exp(x - a.m);
  }
}

template <typename A>
__device__ __forceinline__ MaxSum<A> ms_merge(MaxSum<A> a, MaxSum<A> b) {
  // The side that holds the maximum keeps its sum unscaled; equal maxima add their sums, so inf - inf never forms:
  // two empty sides (m = -inf) stay empty, an empty side adds s * exp(-inf) = 0, two +inf maxima stay +inf.  A NaN
  // logit sits in its side's sum (never in m) and survives every scaling, 0 included.
  if (a.m >= b.m) return {a.m, a.s + (b.m == a.m ? b.s : b.s * exp(b.m - a.m))};
  return {b.m, b.s + a.s * exp(a.m - b.m)};
}

}  // namespace tmx
