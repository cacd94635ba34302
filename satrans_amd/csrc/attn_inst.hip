// Instance-level attention search (reference models/meta_basemodel.py:440-445, 460-499: predict's `inst_attn_dict` and `instattn`
// branches): find the (sample, head) pairs of a batch whose attention map of one layer satisfies a rule - a conjunction of
// clauses, a clause a disjunction of atoms att[h, b, q, k] > thr - append one record per (pair, rule) to a device list, and copy
// the maps, probabilities and input rows of listed records out of the batch's buffers.  Only the matches leave the device.
//
// Order: sample index, then head, then rule - the list of a pass over a data set does not depend on how the pass was cut into
// batches.  (Deliberate deviation: the reference walks head-major inside every batch, so its file order changes with batch_size.)
//
// Deterministic by construction, no atomics: pair p = b * H + h is lane p of a flat launch.  The count kernel evaluates the rules
// of its pair (reading only the atoms they name, short-circuiting), keeps the pair's rule bits and writes one count per wave; one
// workgroup scans the wave counts, takes the list's total as the base and advances it - beyond the capacity too, so truncation
// is visible; the write kernel puts every pair's records at base + its wave's offset + its lanes' prefix while that is below the
// capacity.
//
// Traffic of the search: one dword per evaluated atom and pair, each in a cache line of its own (a pair's map is F*F*4 bytes away
// from the next sample's); of the gather: F*F dwords per record, read and written as dwords (F*F*4 is not 16-byte aligned for odd F).
#include <math.h>

#include "common.h"

namespace satrans {

constexpr int kInstThreads = 256;
constexpr int kInstAlign = 256;
constexpr int kInstGatherGroups = 2048;     // most workgroups of a gather launch (they stride over the records)

struct InstRules {                           // the rules by value, a kernel argument (3.3 KB of the 4 KB a launch carries)
    int32_t n;
    satrans_attn_rule r[SATRANS_ATTN_MAX_RULES];
};

struct InstLayout {
    size_t bits, wave, base, total;
    int64_t waves;
};

static size_t inst_align(size_t v) { return (v + kInstAlign - 1) / kInstAlign * kInstAlign; }

static InstLayout inst_layout(int B, int H) {
    InstLayout L;
    const int64_t P = (int64_t)B * H;
    L.waves = ceil_div(P, kWave);
    size_t at = 0;
    L.bits = at;  at = inst_align(at + (size_t)P);
    L.wave = at;  at = inst_align(at + (size_t)L.waves * 4);
    L.base = at;  at = inst_align(at + 8);
    L.total = at;
    return L;
}

// The rule bits of pair (b, h): bit r set when rule r holds on att[h, b].  `map` = that pair's F x F map.
__device__ __forceinline__ uint32_t inst_rule_bits(const float* __restrict__ map, int F, const InstRules& R, uint32_t allowed) {
    uint32_t bits = 0;
    for (int r = 0; r < R.n; ++r) {
        if (!((allowed >> r) & 1u)) continue;
        const satrans_attn_rule& rule = R.r[r];
        bool all = true;
        for (int c = 0; c < rule.n_clauses && all; ++c) {
            bool any = false;
            for (int a = 0; a < rule.n_atoms[c] && !any; ++a) {
                const satrans_attn_atom& t = rule.atoms[c][a];
                any = map[t.q * F + t.k] > t.thr;               // (strict, fp32; false for a NaN)
            }
            all = any;
        }
        if (all) bits |= 1u << r;
    }
    return bits;
}

// lane = pair p = b * H + h: bits[p] = its rule bits, wave_count[p / 64] = the records of the wave's pairs.
__global__ __launch_bounds__(kInstThreads) void inst_count_kernel(const float* __restrict__ att, const uint8_t* __restrict__ eligible,
                                                                 int B, int H, int F, InstRules R, uint8_t* __restrict__ bits,
                                                                 int32_t* __restrict__ wave_count) {
    const int64_t p = (int64_t)blockIdx.x * kInstThreads + threadIdx.x;
    const int64_t P = (int64_t)B * H;
    uint32_t mine = 0;
    if (p < P) {
        const int b = (int)(p / H), h = (int)(p - (int64_t)b * H);
        const uint32_t allowed = eligible ? eligible[b] : 0xffu;
        if (allowed) mine = inst_rule_bits(att + ((size_t)h * B + b) * F * F, F, R, allowed);
        bits[p] = (uint8_t)mine;
    }
    int32_t n = __popc(mine);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && p < P) wave_count[p / kWave] = n;
}

// wave_count -> its exclusive prefix in place; base[0] = total[0] before the call, total[0] += the records of the batch;
// range (optional) = the list positions this call fills, clamped to the capacity.  One workgroup.
__global__ __launch_bounds__(kInstThreads) void inst_scan_kernel(int32_t* __restrict__ wave_count, int64_t waves, int64_t capacity,
                                                                int64_t* __restrict__ total, int64_t* __restrict__ base,
                                                                int64_t* __restrict__ range) {
    __shared__ int32_t s_wave[kInstThreads / kWave];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
    int64_t carry = 0;
    for (int64_t i0 = 0; i0 < waves; i0 += kInstThreads) {
        const int64_t i = i0 + t;
        const int32_t n = i < waves ? wave_count[i] : 0;
        int32_t incl = n;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int32_t up = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += up;
        }
        if (lane == kWave - 1) s_wave[w] = incl;
        __syncthreads();
        int64_t before = carry;
        for (int ww = 0; ww < w; ++ww) before += s_wave[ww];
        // (the prefix of one batch fits 32 bits: B * H * 8 < 2^31 is checked on the host)
        if (i < waves) wave_count[i] = (int32_t)(before + incl - n);
        for (int ww = 0; ww < kInstThreads / kWave; ++ww) carry += s_wave[ww];
        __syncthreads();
    }
    if (t == 0) {
        const int64_t old = total[0];
        base[0] = old;
        total[0] = old + carry;
        if (range) {
            range[0] = old < capacity ? old : capacity;
            range[1] = old + carry < capacity ? old + carry : capacity;
        }
    }
}

// lane = pair: its records, one per set rule bit in rule order, at base + wave offset + the prefix of the lanes before it.
__global__ __launch_bounds__(kInstThreads) void inst_write_kernel(const uint8_t* __restrict__ bits, const int32_t* __restrict__ wave_off,
                                                                 const int64_t* __restrict__ base, int B, int H, int64_t first_index,
                                                                 int64_t capacity, satrans_attn_match* __restrict__ records) {
    const int64_t p = (int64_t)blockIdx.x * kInstThreads + threadIdx.x;
    const int64_t P = (int64_t)B * H;
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t mine = p < P ? bits[p] : 0u;
    const int32_t n = __popc(mine);
    int32_t incl = n;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int32_t up = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += up;
    }
    if (!mine) return;
    int64_t at = base[0] + wave_off[p / kWave] + (incl - n);
    const int b = (int)(p / H), h = (int)(p - (int64_t)b * H);
    while (mine && at < capacity) {
        const int r = __ffs(mine) - 1;
        mine &= mine - 1;
        satrans_attn_match rec;
        rec.index = first_index + b;
        rec.head = h;
        rec.rule = r;
        records[at++] = rec;
    }
}

// One workgroup per record at a time: maps[m] = att[head, b], pred[m] = prob[b], x_rows[m] = the dwords of row b of X, b = index -
// first_index.  A record that names no pair of this batch (another batch's, a bad head) is skipped.
__global__ __launch_bounds__(kInstThreads) void inst_gather_kernel(const float* __restrict__ att, int B, int H, int E,
                                                                  const satrans_attn_match* __restrict__ records, int64_t m0, int64_t m1,
                                                                  const int64_t* __restrict__ range, int64_t first_index,
                                                                  float* __restrict__ maps, const float* __restrict__ prob,
                                                                  float* __restrict__ pred, const uint32_t* __restrict__ x,
                                                                  int64_t x_stride, int row_dwords, uint32_t* __restrict__ x_rows) {
    if (range) {
        m0 = max(m0, range[0]);
        m1 = min(m1, range[1]);
    }
    for (int64_t m = m0 + blockIdx.x; m < m1; m += gridDim.x) {
        const satrans_attn_match rec = records[m];
        const int64_t b = rec.index - first_index;
        if (b < 0 || b >= B || rec.head < 0 || rec.head >= H) continue;         // (uniform over the workgroup)
        if (maps) {
            const uint32_t* src = (const uint32_t*)att + ((size_t)rec.head * B + (size_t)b) * E;
            uint32_t* dst = (uint32_t*)maps + (size_t)m * E;
            for (int e = threadIdx.x; e < E; e += kInstThreads) dst[e] = src[e];
        }
        if (x_rows) {
            const uint32_t* src = x + (size_t)b * x_stride;
            uint32_t* dst = x_rows + (size_t)m * row_dwords;
            for (int e = threadIdx.x; e < row_dwords; e += kInstThreads) dst[e] = src[e];
        }
        if (pred && threadIdx.x == 0) pred[m] = prob[b];
    }
}

static int inst_check_rules(const satrans_attn_rule* rules, int n_rules, int F, const char* who) {
    SATRANS_REQUIRE(rules, SATRANS_E_BADARG, "%s: null pointer", who);
    SATRANS_REQUIRE(n_rules >= 1 && n_rules <= SATRANS_ATTN_MAX_RULES, SATRANS_E_BADARG, "%s: %d rules (1..%d)", who, n_rules,
                    SATRANS_ATTN_MAX_RULES);
    for (int r = 0; r < n_rules; ++r) {
        const satrans_attn_rule& rule = rules[r];
        SATRANS_REQUIRE(rule.n_clauses >= 1 && rule.n_clauses <= SATRANS_ATTN_MAX_CLAUSES, SATRANS_E_BADARG,
                        "%s: rule %d has %d clauses (1..%d)", who, r, rule.n_clauses, SATRANS_ATTN_MAX_CLAUSES);
        for (int c = 0; c < rule.n_clauses; ++c) {
            SATRANS_REQUIRE(rule.n_atoms[c] >= 1 && rule.n_atoms[c] <= SATRANS_ATTN_MAX_ATOMS, SATRANS_E_BADARG,
                            "%s: rule %d clause %d has %d atoms (1..%d)", who, r, c, rule.n_atoms[c], SATRANS_ATTN_MAX_ATOMS);
            for (int a = 0; a < rule.n_atoms[c]; ++a) {
                const satrans_attn_atom& t = rule.atoms[c][a];
                SATRANS_REQUIRE(t.q >= 0 && t.q < F && t.k >= 0 && t.k < F, SATRANS_E_BADARG,
                                "%s: rule %d clause %d atom %d names field (%d, %d) outside [0, %d)", who, r, c, a, t.q, t.k, F);
                SATRANS_REQUIRE(isfinite(t.thr), SATRANS_E_BADARG, "%s: rule %d clause %d atom %d has a non-finite threshold", who, r,
                                c, a);
            }
        }
    }
    return SATRANS_OK;
}

static bool inst_sizes_ok(int B, int H, int F) {
    return B > 0 && H >= 1 && H <= SATRANS_ATTN_MAX_HEADS && F > 0 && F <= 4096 &&
           (int64_t)B * H * SATRANS_ATTN_MAX_RULES < ((int64_t)1 << 31);
}

}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_attn_inst_workspace_bytes(int B, int H, int F) {
    SATRANS_REQUIRE(inst_sizes_ok(B, H, F), SATRANS_E_BADARG, "attn_inst_workspace_bytes: bad sizes B=%d H=%d F=%d", B, H, F);
    return (int64_t)inst_layout(B, H).total;
}

extern "C" int satrans_attn_inst_check_rules(const satrans_attn_rule* rules, int n_rules, int F) {
    SATRANS_REQUIRE(F > 0, SATRANS_E_BADARG, "attn_inst_check_rules: bad size F=%d", F);
    return inst_check_rules(rules, n_rules, F, "attn_inst_check_rules");
}

extern "C" int satrans_attn_inst_match(const float* att, int B, int H, int F, const satrans_attn_rule* rules, int n_rules,
                                       const uint8_t* eligible, int64_t first_index, satrans_attn_match* records, int64_t capacity,
                                       int64_t* total, int64_t* range, void* workspace, int64_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SATRANS_REQUIRE(att && rules && total && workspace, SATRANS_E_BADARG, "attn_inst_match: null pointer");
    SATRANS_REQUIRE(inst_sizes_ok(B, H, F), SATRANS_E_BADARG, "attn_inst_match: bad sizes B=%d H=%d F=%d", B, H, F);
    SATRANS_REQUIRE(capacity >= 0 && (records || capacity == 0), SATRANS_E_BADARG, "attn_inst_match: bad capacity %lld",
                    (long long)capacity);
    const int rc = inst_check_rules(rules, n_rules, F, "attn_inst_match");
    if (rc != SATRANS_OK) return rc;
    const InstLayout L = inst_layout(B, H);
    SATRANS_REQUIRE((int64_t)L.total <= workspace_bytes, SATRANS_E_WORKSPACE, "attn_inst_match: workspace %lld < %lld bytes",
                    (long long)workspace_bytes, (long long)L.total);
    InstRules R;
    R.n = n_rules;
    for (int r = 0; r < SATRANS_ATTN_MAX_RULES; ++r) R.r[r] = rules[r < n_rules ? r : 0];
    char* ws = (char*)workspace;
    uint8_t* bits = (uint8_t*)(ws + L.bits);
    int32_t* wave = (int32_t*)(ws + L.wave);
    int64_t* base = (int64_t*)(ws + L.base);
    const unsigned groups = (unsigned)ceil_div((int64_t)B * H, kInstThreads);
    inst_count_kernel<<<groups, kInstThreads, 0, stream>>>(att, eligible, B, H, F, R, bits, wave);
    SATRANS_CHECK_LAUNCH("inst_count_kernel");
    inst_scan_kernel<<<1, kInstThreads, 0, stream>>>(wave, L.waves, capacity, total, base, range);
    SATRANS_CHECK_LAUNCH("inst_scan_kernel");
    if (capacity > 0) {
        inst_write_kernel<<<groups, kInstThreads, 0, stream>>>(bits, wave, base, B, H, first_index, capacity, records);
        SATRANS_CHECK_LAUNCH("inst_write_kernel");
    }
    return SATRANS_OK;
}

extern "C" int satrans_attn_inst_gather(const float* att, int B, int H, int F, const satrans_attn_match* records, int64_t m0,
                                        int64_t m1, const int64_t* range, int64_t first_index, float* maps, const float* prob,
                                        float* pred, const void* x, int64_t x_stride_dwords, int row_dwords, void* x_rows,
                                        void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SATRANS_REQUIRE(records, SATRANS_E_BADARG, "attn_inst_gather: null pointer");
    SATRANS_REQUIRE(!maps || att, SATRANS_E_BADARG, "attn_inst_gather: null pointer (maps without att)");
    SATRANS_REQUIRE(!pred || prob, SATRANS_E_BADARG, "attn_inst_gather: null pointer (pred without prob)");
    SATRANS_REQUIRE(!x_rows || x, SATRANS_E_BADARG, "attn_inst_gather: null pointer (x_rows without x)");
    SATRANS_REQUIRE(inst_sizes_ok(B, H, F), SATRANS_E_BADARG, "attn_inst_gather: bad sizes B=%d H=%d F=%d", B, H, F);
    SATRANS_REQUIRE(m0 >= 0 && m1 >= m0, SATRANS_E_BADARG, "attn_inst_gather: bad record range [%lld, %lld)", (long long)m0,
                    (long long)m1);
    SATRANS_REQUIRE(!x_rows || (row_dwords > 0 && x_stride_dwords >= row_dwords), SATRANS_E_BADARG,
                    "attn_inst_gather: bad row size %d (stride %lld)", row_dwords, (long long)x_stride_dwords);
    if (m1 == m0) return SATRANS_OK;
    const unsigned groups = (unsigned)(m1 - m0 < kInstGatherGroups ? m1 - m0 : kInstGatherGroups);
    inst_gather_kernel<<<groups, kInstThreads, 0, stream>>>(att, B, H, F * F, records, m0, m1, range, first_index, maps, prob, pred,
                                                           (const uint32_t*)x, x_stride_dwords, row_dwords, (uint32_t*)x_rows);
    SATRANS_CHECK_LAUNCH("inst_gather_kernel");
    return SATRANS_OK;
}
