// Walking a scenario-bucketed batch without reading anything back to the host (pnorm.hip, star.hip).
//
// Layout.  The rows of a batch stay in the caller's order; `order` [B] / `seg` [S+1] (satrans_bucket_scenarios) give every
// scenario's run: scenario s owns positions [seg[s], seg[s+1]) of `order`.  A run is cut into units of `rows` positions counted
// from the start of the run (a chunk, a row tile: the caller's word), so a unit never straddles two scenarios and only the last
// unit of a run is short; a scenario without rows has no unit.
//
// Slots.  How many units a batch has depends on seg, which lives on the device.  The grid is therefore sized for the most a
// batch of B rows over S scenarios can have,
//     sum_s ceil(n_s / rows)  <=  sum_s (n_s / rows + 1)  <=  ceil(B / rows) + S        (seg_slots, below)
// and a workgroup finds (scenario, unit) of its slot - the units of scenario 0 in order, then those of scenario 1, ... - by
// walking seg (find_slot).  A slot past the last unit gets s < 0 and its workgroup returns at once: it reads no row and writes
// nothing, and nobody reads its partials, because the ordered walk (scenario_units) visits exactly the slots find_slot hands out.
// Partials are merged in unit order, then scenario order: no floating-point atomics, equal inputs give equal bits.
//
// Safety.  Every read of seg goes through seg_range, which clips the run into [0, B] so that a damaged seg cannot send a read
// outside `order`; every read of `order` goes through row_at, which turns a row outside [0, B) into "no row".  A workgroup's
// slot is below the grid's seg_slots, so what it writes per slot stays inside buffers sized by seg_slots.  The bound itself
// holds for a seg as satrans_bucket_scenarios writes it (non-decreasing: the runs are disjoint pieces of [0, B)).
//
// Two other partitions of work are deliberately NOT expressed through this header: work_range / tiles_of in
// layer_fused_common.h (a persistent grid split into equal ranges, on the hot path - a different scheme), and attn_stats.hip
// (a prefix plan stored in memory and searched by bisection).
#pragma once
#include "common.h"

namespace satrans {

// positions [a, b) of scenario s, clipped into [0, B]
__device__ __forceinline__ void seg_range(const int32_t* __restrict__ seg, int s, int B, int& a, int& b) {
    a = min(max(seg[s], 0), B);
    b = min(max(seg[s + 1], a), B);
}

// units of a run of n positions
__device__ __forceinline__ int units_of(int n, int rows) { return n > 0 ? (n + rows - 1) / rows : 0; }

struct SegSlot {
    int s, r0, r1;      // scenario, positions [r0, r1) of `order`;  s < 0: no such unit
};
struct SegSlotN {
    int s, r0, r1, n;      // the same, and the rows of the whole scenario
};

// Slot = SegSlot or SegSlotN; `rows` is a compile-time constant at every call site
template <class Slot>
__device__ __forceinline__ Slot find_slot(const int32_t* __restrict__ seg, int S, int B, int slot, int rows) {
    int cum = 0;
    for (int s = 0; s < S; ++s) {
        int a, b;
        seg_range(seg, s, B, a, b);
        const int nu = units_of(b - a, rows);
        if (slot < cum + nu) {
            const int r0 = a + (slot - cum) * rows;
            if constexpr (sizeof(Slot) == sizeof(SegSlotN))
                return Slot{s, r0, min(r0 + rows, b), b - a};
            else
                return Slot{s, r0, min(r0 + rows, b)};
        }
        cum += nu;
    }
    return Slot{-1, 0, 0};
}

// row at position p of `order` (p < r1), or -1
__device__ __forceinline__ int row_at(const int32_t* __restrict__ order, int p, int r1, int B) {
    if (p >= r1) return -1;
    const int row = order[p];
    return (unsigned)row < (unsigned)B ? row : -1;
}

// The ordered walk: scenario s owns slots [k0, k0 + scenario_units(s)), k0 = first_slot(s); a loop over all scenarios keeps
// k0 by adding each scenario's units after its body.
__device__ __forceinline__ int scenario_units(const int32_t* __restrict__ seg, int s, int B, int rows) {
    int a, b;
    seg_range(seg, s, B, a, b);
    return units_of(b - a, rows);
}

__device__ __forceinline__ int first_slot(const int32_t* __restrict__ seg, int s, int B, int rows) {
    int k0 = 0;
    for (int t = 0; t < s; ++t) k0 += scenario_units(seg, t, B, rows);
    return k0;
}

// host: slots of a batch of B rows over S scenarios (the bound above)
inline int64_t seg_slots(int64_t B, int64_t S, int64_t rows) { return ceil_div(B, rows) + S; }

}  // namespace satrans
