// Pooled embedding gather for VarLenSparseFeat fields, and its backward.
//
// Forward: deepctr-torch's varlen_embedding_lookup + get_varlen_pooling_list (SequencePoolingLayer) behind the SparseFeat lookups,
// concatenated as BaseModel.input_from_feature_columns does (reference models/meta_basemodel.py:519-545): ONE launch writes the
// layer input [B, F, D] (F = sparse fields, then varlen fields) and the arena row of every SLOT [B, R] (R = sparse fields + the
// sum of maxlen), which the existing sort / segment-sum / Adam chain consumes as it consumes the one-row-per-field gather's rows.
// Backward: layer 0's dx [B, F, D] -> the gradient of every slot's row [B*R, D], written once per slot (no atomics: the bits
// of a row's gradient do not depend on scheduling).
//
// HBM-bound like gather.hip: 128-byte random rows at D = 32, D/4 lanes x one 16-byte load per row.  A thread owns kPoolItems
// (sample, field) items at a time and requests kPoolSlotStep slots of every one of them before it uses any, so up to
// kPoolItems x kPoolSlotStep = 8 independent rows are in flight per lane against the ~900-cycle miss latency
// (MI355X_MICROARCH.md).  (sample, field) is advanced incrementally - no integer division per item or per slot.
#include <cstring>

#include "common.h"
#include "pool_fields.h"

namespace satrans {

constexpr int kPoolBlock = SATRANS_POOL_BLOCK;
constexpr int kPoolItems = SATRANS_POOL_ITEMS;
constexpr int kPoolSlotStep = 2;
constexpr int kPoolMaxBlocks = SATRANS_POOL_MAX_BLOCKS;      // 8 blocks per CU (256 CUs)
static_assert(kPoolBlock == 256 && kPoolItems == 4 && kPoolMaxBlocks == 256 * 8, "the launch shape the kernels were tuned at");

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// one element of `max` pooling: w = E - (1 - mask) * 1e9 (both factors exact in fp32), strict > keeps the first maximal slot
__device__ __forceinline__ void max_step(float& acc, uint32_t& am, float v, bool valid, int s, int byte) {
    const float w = valid ? v : v - 1e9f;
    if (s == 0 || w > acc) {
        acc = w;
        am = (am & ~(0xFFu << byte)) | ((uint32_t)s << byte);
    }
}

template <int LPR>  // lanes per row = D/4
__global__ __launch_bounds__(kPoolBlock) void pool_gather_kernel(
    const float4* __restrict__ arena, const float4* __restrict__ src, const int32_t* __restrict__ src_rows, const PoolFields pf,
    int F, int R, int Fv, const void* __restrict__ X, int id_dtype, int64_t x_stride, int64_t n_items, float4* __restrict__ out,
    int32_t* __restrict__ rows_out, uint32_t* __restrict__ mask_out, uint32_t* __restrict__ argmax_out,
    int32_t* __restrict__ status) {
    const int64_t tid = (int64_t)blockIdx.x * kPoolBlock + threadIdx.x;
    const int64_t item0 = tid / LPR;
    const int q = (int)(tid % LPR);
    const int64_t stride = (int64_t)gridDim.x * kPoolBlock / LPR;
    const int sb = (int)stride / F;          // (n_items = B * F < 2^31: checked by the caller)
    const int sf = (int)stride - sb * F;
    int b0 = (int)min(item0, n_items) / F;
    int f0 = (int)min(item0, n_items) - b0 * F;
    bool bad_any = false;
    for (int64_t base = item0; base < n_items; base += stride * kPoolItems) {
        int bb[kPoolItems], ff[kPoolItems], n[kPoolItems];
        int64_t len[kPoolItems];
        float4 acc[kPoolItems];
        uint32_t mask[kPoolItems], am[kPoolItems];
        int nmax = 0;
#pragma unroll
        for (int k = 0; k < kPoolItems; ++k) {
            const int64_t item = base + k * stride;
            bb[k] = b0;
            ff[k] = f0;
            n[k] = item < n_items ? pf.f[f0].maxlen : 0;
            len[k] = 0;
            if (n[k] > 0 && pf.f[f0].len_col >= 0) len[k] = load_id(X, id_dtype, x_stride, b0, pf.f[f0].len_col);
            nmax = max(nmax, n[k]);
            acc[k] = f4_zero();
            mask[k] = 0;
            am[k] = 0;
            b0 += sb;
            f0 += sf;
            if (f0 >= F) { f0 -= F; ++b0; }
        }
        for (int s0 = 0; s0 < nmax; s0 += kPoolSlotStep) {
            int64_t row[kPoolItems][kPoolSlotStep];
            bool valid[kPoolItems][kPoolSlotStep];
            float4 val[kPoolItems][kPoolSlotStep];
#pragma unroll
            for (int k = 0; k < kPoolItems; ++k) {
#pragma unroll
                for (int u = 0; u < kPoolSlotStep; ++u) {
                    const int s = s0 + u;
                    row[k][u] = -1;
                    valid[k][u] = false;
                    if (s < n[k]) {
                        const satrans_pool_field& fd = pf.f[ff[k]];
                        const int64_t id = load_id(X, id_dtype, x_stride, bb[k], fd.col + s);
                        // out of range (padding slots included, as nn.Embedding): flagged, zeros, the table's first row recorded
                        const bool bad = id < 0 || id >= fd.hi - fd.lo;
                        bad_any |= bad;
                        row[k][u] = bad ? fd.lo : fd.lo + id;
                        valid[k][u] = fd.len_col >= 0 ? (int64_t)s < len[k] : id != 0;
                        if (valid[k][u]) mask[k] |= 1u << s;
                        if (q == 0 && rows_out) rows_out[(int64_t)bb[k] * R + fd.slot + s] = (int32_t)row[k][u];
                        if (bad) row[k][u] = -2;
                    }
                }
            }
            if (!out) continue;
#pragma unroll
            for (int k = 0; k < kPoolItems; ++k) {
#pragma unroll
                for (int u = 0; u < kPoolSlotStep; ++u) {
                    val[k][u] = f4_zero();
                    if (row[k][u] >= 0) {
                        val[k][u] = src_rows ? src[(int64_t)src_rows[(int64_t)bb[k] * R + pf.f[ff[k]].slot + s0 + u] * LPR + q]
                                             : arena[row[k][u] * LPR + q];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kPoolItems; ++k) {
                const int comb = pf.f[ff[k]].combiner;
#pragma unroll
                for (int u = 0; u < kPoolSlotStep; ++u) {
                    const int s = s0 + u;
                    if (s >= n[k]) continue;
                    const float4 v = val[k][u];
                    const bool ok = valid[k][u];
                    if (comb == SATRANS_POOL_COPY) {
                        acc[k] = v;
                    } else if (comb == SATRANS_POOL_MAX) {
                        max_step(acc[k].x, am[k], v.x, ok, s, 0);
                        max_step(acc[k].y, am[k], v.y, ok, s, 8);
                        max_step(acc[k].z, am[k], v.z, ok, s, 16);
                        max_step(acc[k].w, am[k], v.w, ok, s, 24);
                    } else if (ok) {          // sum / mean: slot order; a padding slot adds E * 0, which changes no bit
                        acc[k].x += v.x;
                        acc[k].y += v.y;
                        acc[k].z += v.z;
                        acc[k].w += v.w;
                    }
                }
            }
        }
        if (!out && !mask_out) continue;
#pragma unroll
        for (int k = 0; k < kPoolItems; ++k) {
            if (n[k] == 0) continue;
            const satrans_pool_field& fd = pf.f[ff[k]];
            float4 r = acc[k];
            if (fd.combiner == SATRANS_POOL_MEAN) {
                const float c = (float)__popc(mask[k]) + 1e-8f;       // a true division, as torch.div
                r = make_float4(r.x / c, r.y / c, r.z / c, r.w / c);
            }
            if (out) out[((int64_t)bb[k] * F + ff[k]) * LPR + q] = r;
            if (fd.varlen >= 0) {
                const int64_t at = (int64_t)bb[k] * Fv + fd.varlen;
                if (q == 0 && mask_out) mask_out[at] = mask[k];
                if (out && argmax_out && fd.combiner == SATRANS_POOL_MAX) argmax_out[at * LPR + q] = am[k];
            }
        }
    }
    if (bad_any) atomicOr(status, 1);
}

template <int LPR>
__global__ __launch_bounds__(kPoolBlock) void pool_bwd_kernel(const float4* __restrict__ dx, const PoolFields pf, int F, int R,
                                                             int Fv, int64_t n_items, const uint32_t* __restrict__ mask,
                                                             const uint32_t* __restrict__ argmax, float4* __restrict__ gemb) {
    const int64_t tid = (int64_t)blockIdx.x * kPoolBlock + threadIdx.x;
    const int64_t item0 = tid / LPR;
    const int q = (int)(tid % LPR);
    const int64_t stride = (int64_t)gridDim.x * kPoolBlock / LPR;
    const int sb = (int)stride / F;
    const int sf = (int)stride - sb * F;
    int b = (int)min(item0, n_items) / F;
    int f = (int)min(item0, n_items) - b * F;
    for (int64_t item = item0; item < n_items; item += stride) {
        const satrans_pool_field& fd = pf.f[f];
        float4 g = dx[item * LPR + q];
        float4* o = gemb + ((int64_t)b * R + fd.slot) * LPR + q;
        if (fd.varlen < 0) {
            o[0] = g;
        } else {
            const int64_t at = (int64_t)b * Fv + fd.varlen;
            const uint32_t m = mask[at];
            if (fd.combiner == SATRANS_POOL_MAX) {
                // the whole gradient to the (first) maximal slot of every element - a padding slot too when it is the maximum
                const uint32_t a = argmax[at * LPR + q];
                for (int s = 0; s < fd.maxlen; ++s) {
                    float4 r;
                    r.x = (int)(a & 0xFF) == s ? g.x : 0.f;
                    r.y = (int)((a >> 8) & 0xFF) == s ? g.y : 0.f;
                    r.z = (int)((a >> 16) & 0xFF) == s ? g.z : 0.f;
                    r.w = (int)(a >> 24) == s ? g.w : 0.f;
                    o[(int64_t)s * LPR] = r;
                }
            } else {
                if (fd.combiner == SATRANS_POOL_MEAN) {
                    const float c = (float)__popc(m) + 1e-8f;
                    g = make_float4(g.x / c, g.y / c, g.z / c, g.w / c);
                }
                for (int s = 0; s < fd.maxlen; ++s) o[(int64_t)s * LPR] = (m >> s) & 1u ? g : f4_zero();
            }
        }
        b += sb;
        f += sf;
        if (f >= F) { f -= F; ++b; }
    }
}

static int64_t pool_blocks(int64_t n_items, int lpr, int per_thread) {
    int64_t blocks = ceil_div(ceil_div(n_items, per_thread) * lpr, kPoolBlock);
    if (blocks > kPoolMaxBlocks) blocks = kPoolMaxBlocks;      // 8 blocks per CU, grid-strided beyond that
    return blocks < 1 ? 1 : blocks;
}

}  // namespace satrans

extern "C" int64_t satrans_pool_argmax_bytes(int B, int Fv, int D) { return (int64_t)B * Fv * D; }

extern "C" int satrans_pool_gather_fwd(const float* arena, int64_t arena_rows, const float* src, const int32_t* src_rows,
                                       const satrans_pool_field* fields, int F, int R, int Fv, const void* X, int id_dtype,
                                       int64_t x_stride, int B, int D, float* out, int32_t* rows_out, uint32_t* mask_out,
                                       uint8_t* argmax_out, int32_t* status, void* stream_) {
    using namespace satrans;
    hipStream_t stream = (hipStream_t)stream_;
    SATRANS_REQUIRE(arena && X && status && (out || rows_out || mask_out), SATRANS_E_BADARG, "pool_gather_fwd: null pointer");
    SATRANS_REQUIRE(!src_rows || src, SATRANS_E_BADARG, "pool_gather_fwd: src_rows without src");
    SATRANS_REQUIRE(!out || Fv == 0 || (mask_out && argmax_out), SATRANS_E_BADARG,
                    "pool_gather_fwd: a pooled output needs mask_out and argmax_out");
    SATRANS_REQUIRE(B > 0, SATRANS_E_BADARG, "pool_gather_fwd: B = %d", B);
    SATRANS_REQUIRE(id_dtype >= 0 && id_dtype <= 2, SATRANS_E_BADARG, "pool_gather_fwd: id_dtype %d", id_dtype);
    SATRANS_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128, SATRANS_E_UNSUPPORTED,
                    "pool_gather_fwd: embedding_dim %d not in {16,32,64,128}", D);
    int rc = check_fields(fields, F, R, Fv, x_stride, arena_rows, "pool_gather_fwd");
    if (rc != SATRANS_OK) return rc;
    SATRANS_REQUIRE((int64_t)B * R < ((int64_t)1 << 31), SATRANS_E_BADARG, "pool_gather_fwd: B * R = %lld does not fit 31 bits",
                    (long long)B * R);
    PoolFields pf;
    memset(&pf, 0, sizeof(pf));
    memcpy(pf.f, fields, sizeof(satrans_pool_field) * F);
    const int lpr = D / 4;
    const int64_t n_items = (int64_t)B * F;
    const int64_t blocks = pool_blocks(n_items, lpr, kPoolItems);
#define LAUNCH(LPR)                                                                                                          \
    pool_gather_kernel<LPR><<<(unsigned)blocks, kPoolBlock, 0, stream>>>(                                                    \
        (const float4*)arena, (const float4*)src, src_rows, pf, F, R, Fv, X, id_dtype, x_stride, n_items, (float4*)out,        \
        rows_out, mask_out, (uint32_t*)argmax_out, status)
    switch (lpr) {
        case 4: LAUNCH(4); break;
        case 8: LAUNCH(8); break;
        case 16: LAUNCH(16); break;
        default: LAUNCH(32); break;
    }
#undef LAUNCH
    SATRANS_CHECK_LAUNCH("pool_gather_kernel");
    return SATRANS_OK;
}

extern "C" int satrans_pool_bwd(const float* dx, const satrans_pool_field* fields, int F, int R, int Fv, int B, int D,
                                const uint32_t* mask, const uint8_t* argmax, float* gemb, void* stream_) {
    using namespace satrans;
    hipStream_t stream = (hipStream_t)stream_;
    SATRANS_REQUIRE(dx && gemb && (Fv == 0 || (mask && argmax)), SATRANS_E_BADARG, "pool_bwd: null pointer");
    SATRANS_REQUIRE(B > 0, SATRANS_E_BADARG, "pool_bwd: B = %d", B);
    SATRANS_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128, SATRANS_E_UNSUPPORTED,
                    "pool_bwd: embedding_dim %d not in {16,32,64,128}", D);
    // (the backward reads no id and no arena row: columns and table rows are not its concern)
    int rc = check_fields(fields, F, R, Fv, INT64_MAX, INT64_MAX, "pool_bwd");
    if (rc != SATRANS_OK) return rc;
    SATRANS_REQUIRE((int64_t)B * R < ((int64_t)1 << 31), SATRANS_E_BADARG, "pool_bwd: B * R = %lld does not fit 31 bits",
                    (long long)B * R);
    PoolFields pf;
    memset(&pf, 0, sizeof(pf));
    memcpy(pf.f, fields, sizeof(satrans_pool_field) * F);
    const int lpr = D / 4;
    const int64_t n_items = (int64_t)B * F;
    const int64_t blocks = pool_blocks(n_items, lpr, 1);
#define LAUNCH(LPR)                                                                                                          \
    pool_bwd_kernel<LPR><<<(unsigned)blocks, kPoolBlock, 0, stream>>>((const float4*)dx, pf, F, R, Fv, n_items, mask,         \
                                                                      (const uint32_t*)argmax, (float4*)gemb)
    switch (lpr) {
        case 4: LAUNCH(4); break;
        case 8: LAUNCH(8); break;
        case 16: LAUNCH(16); break;
        default: LAUNCH(32); break;
    }
#undef LAUNCH
    SATRANS_CHECK_LAUNCH("pool_bwd_kernel");
    return SATRANS_OK;
}
