// The field table of the pooled gather (pool.hip) and of the order-1 term (linear.hip): the by-value kernel argument and the
// host-side check that every row, slot and X column the table can produce lies inside its buffer.
#pragma once
#include <cstring>

#include "common.h"

namespace satrans {

struct PoolFields {
    satrans_pool_field f[SATRANS_POOL_MAX_FIELDS];
};

inline PoolFields pool_fields_of(const satrans_pool_field* fields, int F) {
    PoolFields pf;
    memset(&pf, 0, sizeof(pf));
    if (F > 0) memcpy(pf.f, fields, sizeof(satrans_pool_field) * F);
    return pf;
}

// Host-side check of the field table (it travels by value as a kernel argument: every row index it can produce is checked here)
static int check_fields(const satrans_pool_field* fields, int F, int R, int Fv, int64_t x_stride, int64_t arena_rows,
                        const char* who) {
    SATRANS_REQUIRE(fields && F > 0 && F <= SATRANS_POOL_MAX_FIELDS, SATRANS_E_BADARG, "%s: F = %d (1..%d fields)", who, F,
                    SATRANS_POOL_MAX_FIELDS);
    int slot = 0, nv = 0;
    for (int f = 0; f < F; ++f) {
        const satrans_pool_field& d = fields[f];
        const bool var = d.combiner != SATRANS_POOL_COPY;
        SATRANS_REQUIRE(d.combiner >= SATRANS_POOL_COPY && d.combiner <= SATRANS_POOL_MAX, SATRANS_E_BADARG,
                        "%s: field %d: combiner %d", who, f, d.combiner);
        SATRANS_REQUIRE(var ? (d.maxlen >= 1 && d.maxlen <= SATRANS_POOL_MAX_LEN) : d.maxlen == 1, SATRANS_E_UNSUPPORTED,
                        "%s: field %d: maxlen %d (1..%d)", who, f, d.maxlen, SATRANS_POOL_MAX_LEN);
        SATRANS_REQUIRE(d.slot == slot, SATRANS_E_BADARG, "%s: field %d: first slot %d, expected %d", who, f, d.slot, slot);
        SATRANS_REQUIRE(var ? d.varlen == nv : d.varlen == -1, SATRANS_E_BADARG, "%s: field %d: varlen index %d", who, f, d.varlen);
        SATRANS_REQUIRE(d.col >= 0 && (int64_t)d.col + d.maxlen <= x_stride && d.len_col < x_stride &&
                            (var || d.len_col == -1) && d.len_col >= -1, SATRANS_E_BADARG,
                        "%s: field %d: X columns [%d, %d) / length column %d outside a row of %lld", who, f, d.col,
                        d.col + d.maxlen, d.len_col, (long long)x_stride);
        SATRANS_REQUIRE(d.lo >= 0 && d.lo < d.hi && d.hi <= arena_rows, SATRANS_E_BADARG,
                        "%s: field %d: table rows [%lld, %lld) outside the arena of %lld", who, f, (long long)d.lo,
                        (long long)d.hi, (long long)arena_rows);
        slot += d.maxlen;
        nv += var ? 1 : 0;
    }
    SATRANS_REQUIRE(slot == R && nv == Fv, SATRANS_E_BADARG, "%s: R = %d, Fv = %d; the fields give %d slots, %d varlen", who, R,
                    Fv, slot, nv);
    return SATRANS_OK;
}

}  // namespace satrans
