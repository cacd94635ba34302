// The pairs (i, j), i < j, of F fields in itertools.combinations order, as fibinet.hip and pnn.hip number them:
// pair p = i (2 F - i - 1) / 2 + j - i - 1, P = F (F - 1) / 2.
#pragma once
#include "common.h"

namespace satrans {
namespace {

__device__ __forceinline__ int pair_index(int i, int j, int F) { return i * (2 * F - i - 1) / 2 + j - i - 1; }

__device__ __forceinline__ void pair_fields(int p, int F, int& i, int& j) {
    i = 0;
    while (p >= F - 1 - i) {
        p -= F - 1 - i;
        ++i;
    }
    j = i + 1 + p;
}

}  // namespace
}  // namespace satrans
