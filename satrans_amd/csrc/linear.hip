// The order-1 ("linear") term of deepctr's models and its backward: Linear.forward of reference models/meta_basemodel.py:63-92,
// the sum over the sparse and pooled varlen fields of their 1-wide embeddings plus dense @ weight.
//
// Forward, one launch.  A row of a 1-wide table is 4 bytes: every read is a dependent pair (the id from X, then the value),
// nothing is there to vectorise, and a lane per sample would put B lanes of F dependent reads each on the card.  The (sample,
// field) items of kLinSamples samples are spread over the 256 lanes of a workgroup instead (adjacent lanes take adjacent fields
// of one sample: its X row is read contiguously), four slots of a varlen list requested before any is used; the pooled values
// meet in LDS, and one lane per sample adds them in field order and then the dense products in column order.  That order is
// the contract (satrans_hip.h): a sample's logit depends on nothing but its own row of X.
//
// Backward.  No float atomics.  (1) every slot's contribution is stored once, [B R] floats; (2) the sorted (row, position)
// list of the caller's sort is cut into chunks of kSegChunk positions, a lane per chunk: a run of equal rows that lies inside
// its chunk is summed in position order and stored; a run that crosses a chunk bound leaves one partial sum per chunk; (3) a
// lane per crossing run adds its partials in chunk order.  A row that every sample gathers (cdna_hip_programming.md Appendix B,
// 'Scatter / gather / embedding': the pass that gives a destination to one lane runs as long as its longest list) thus costs
// n / kSegChunk lanes of kSegChunk reads and one lane of n / kSegChunk reads of consecutive floats whose count is known up
// front (a binary search for the run's end), not one lane of n dependent gathers.  The chunk bounds are multiples of kSegChunk
// in the sorted list: the order of the additions, and with it the bits, depend on the list alone, not on the grid.
// (4) dweight: per kDwRows rows a partial per dense column (fmaf in row order), then the heads' ordered reduce.
#include "common.h"
#include "grouped_gemm.h"
#include "pool_fields.h"

namespace satrans {
namespace {

constexpr int kLinBlock = 256;
constexpr int kLinSamples = SATRANS_LINEAR_SAMPLES;
constexpr int kLinMaxBlocks = SATRANS_LINEAR_MAX_BLOCKS;      // 2 workgroups per CU (256 CUs), grid-strided beyond
constexpr int kLinSlotStep = 4;                               // slots of a list in flight per lane
constexpr int kSegChunk = SATRANS_LINEAR_SEG_CHUNK;
constexpr int kDwRows = SATRANS_LINEAR_DW_ROW_CHUNK;
static_assert(kLinSamples * SATRANS_POOL_MAX_FIELDS * sizeof(float) <= 16 * 1024, "the pooled values of a trip in LDS");

__global__ __launch_bounds__(kLinBlock) void linear_fwd_kernel(
    const float* __restrict__ arena, const PoolFields pf, int F, int R, int Fv, const void* __restrict__ X, int id_dtype,
    int64_t x_stride, int B, const float* __restrict__ dense, int64_t dense_stride, const int32_t* __restrict__ dense_cols,
    const float* __restrict__ weight, int n_dense, float* __restrict__ logit, int32_t* __restrict__ rows_out,
    uint32_t* __restrict__ mask_out, uint8_t* __restrict__ argmax_out, int32_t* __restrict__ status) {
    __shared__ float pooled[kLinSamples][SATRANS_POOL_MAX_FIELDS + 1];
    const int tiles = (B + kLinSamples - 1) / kLinSamples;
    int flags = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int b0 = tile * kLinSamples;
        const int ns = min(kLinSamples, B - b0);
        for (int i = threadIdx.x; i < ns * F; i += kLinBlock) {
            const int sl = i / F, f = i - sl * F;
            const int64_t b = b0 + sl;
            const satrans_pool_field fd = pf.f[f];
            const int n = fd.maxlen;
            const int64_t len = fd.len_col >= 0 ? load_id(X, id_dtype, x_stride, b, fd.len_col) : 0;
            float acc = 0.f;
            uint32_t mask = 0;
            int am = 0;
            for (int s0 = 0; s0 < n; s0 += kLinSlotStep) {
                float v[kLinSlotStep];
                bool ok[kLinSlotStep];
#pragma unroll
                for (int u = 0; u < kLinSlotStep; ++u) {
                    const int s = s0 + u;
                    v[u] = 0.f;
                    ok[u] = false;
                    if (s < n) {
                        const int64_t id = load_id(X, id_dtype, x_stride, b, fd.col + s);
                        // out of range (padding slots included, as nn.Embedding): flagged, zero, the table's first row recorded
                        const bool bad = id < 0 || id >= fd.hi - fd.lo;
                        const int64_t row = bad ? fd.lo : fd.lo + id;
                        ok[u] = fd.len_col >= 0 ? (int64_t)s < len : id != 0;
                        rows_out[b * R + fd.slot + s] = (int32_t)row;
                        if (bad) flags |= 1; else v[u] = arena[row];
                    }
                }
#pragma unroll
                for (int u = 0; u < kLinSlotStep; ++u) {
                    const int s = s0 + u;
                    if (s >= n) continue;
                    if (ok[u]) mask |= 1u << s;
                    if (fd.combiner == SATRANS_POOL_COPY) {
                        acc = v[u];
                    } else if (fd.combiner == SATRANS_POOL_MAX) {      // w - (1 - mask) * 1e9, strict >: the first maximal slot
                        const float w = ok[u] ? v[u] : v[u] - 1e9f;
                        if (s == 0 || w > acc) { acc = w; am = s; }
                    } else if (ok[u]) {                                // sum / mean: slot order
                        acc += v[u];
                    }
                }
            }
            if (fd.combiner == SATRANS_POOL_MEAN) acc = acc / ((float)__popc(mask) + 1e-8f);      // a true division, as torch.div
            pooled[sl][f] = acc;
            if (fd.varlen >= 0) {
                mask_out[b * Fv + fd.varlen] = mask;
                argmax_out[b * Fv + fd.varlen] = (uint8_t)am;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < ns) {
            const int64_t b = b0 + threadIdx.x;
            float sum = 0.f;
            for (int f = 0; f < F; ++f) sum += pooled[threadIdx.x][f];
            for (int k = 0; k < n_dense; ++k) {
                const int c = dense_cols[k];
                const bool in = c >= 0 && c < dense_stride;
                if (!in) flags |= 2;
                sum = fmaf(in ? dense[b * dense_stride + c] : 0.f, weight[k], sum);
            }
            logit[b] = sum;
        }
        __syncthreads();
    }
    if (flags) atomicOr(status, flags);
}

// the contribution of every slot position b R + r to its row: dlogit[b] times the derivative of the pooling
__global__ __launch_bounds__(kLinBlock) void linear_contrib_kernel(const float* __restrict__ dlogit, const PoolFields pf, int F,
                                                                  int R, int Fv, int64_t n_items,
                                                                  const uint32_t* __restrict__ mask,
                                                                  const uint8_t* __restrict__ argmax, float* __restrict__ contrib) {
    const int64_t stride = (int64_t)gridDim.x * kLinBlock;
    for (int64_t item = (int64_t)blockIdx.x * kLinBlock + threadIdx.x; item < n_items; item += stride) {
        const int64_t b = item / F;
        const int f = (int)(item - b * F);
        const satrans_pool_field fd = pf.f[f];
        float g = dlogit[b];
        float* o = contrib + b * R + fd.slot;
        if (fd.varlen < 0) {
            o[0] = g;
            continue;
        }
        const int64_t at = b * Fv + fd.varlen;
        const uint32_t m = mask[at];
        if (fd.combiner == SATRANS_POOL_MAX) {      // everything to the (first) maximal slot - a padding slot too when it is the maximum
            const int a = argmax[at];
            for (int s = 0; s < fd.maxlen; ++s) o[s] = s == a ? g : 0.f;
        } else {
            if (fd.combiner == SATRANS_POOL_MEAN) g = g / ((float)__popc(m) + 1e-8f);
            for (int s = 0; s < fd.maxlen; ++s) o[s] = (m >> s) & 1u ? g : 0.f;
        }
    }
}

// A lane per chunk of kSegChunk sorted positions.  Runs inside the chunk: summed in position order and stored.  The chunk's
// first run when it began in an earlier chunk: head_part[chunk].  Its last run when it began here and goes on: tail_part[chunk].
__global__ __launch_bounds__(kLinBlock) void linear_seg_chunk_kernel(const int32_t* __restrict__ sorted_rows,
                                                                    const int32_t* __restrict__ src, int64_t n, int64_t arena_rows,
                                                                    const float* __restrict__ contrib, float* __restrict__ head_part,
                                                                    float* __restrict__ tail_part, float* __restrict__ g_arena) {
    const int64_t c = (int64_t)blockIdx.x * kLinBlock + threadIdx.x;
    const int64_t j0 = c * kSegChunk;
    if (j0 >= n) return;
    const int64_t j1 = min(n, j0 + kSegChunk);
    int32_t row = sorted_rows[j0];
    const bool from_before = j0 > 0 && sorted_rows[j0 - 1] == row;
    bool first = true;
    float acc = 0.f;
    for (int64_t j = j0; j < j1; ++j) {
        const int32_t r = sorted_rows[j];
        if (r != row) {
            if (first && from_before) head_part[c] = acc;
            else if (row >= 0 && row < arena_rows) g_arena[row] = acc;
            first = false;
            row = r;
            acc = 0.f;
        }
        const int32_t p = src[j];
        acc += p >= 0 && p < n ? contrib[p] : 0.f;
    }
    const bool goes_on = j1 < n && sorted_rows[j1] == row;
    if (first && from_before) head_part[c] = acc;
    else if (goes_on) tail_part[c] = acc;
    else if (row >= 0 && row < arena_rows) g_arena[row] = acc;
}

// A lane per chunk whose last run began there and goes on: its partial, then those of the following chunks in chunk order.
__global__ __launch_bounds__(kLinBlock) void linear_seg_join_kernel(const int32_t* __restrict__ sorted_rows, int64_t n,
                                                                   int64_t arena_rows, const float* __restrict__ head_part,
                                                                   const float* __restrict__ tail_part, float* __restrict__ g_arena) {
    const int64_t c = (int64_t)blockIdx.x * kLinBlock + threadIdx.x;
    const int64_t j0 = c * kSegChunk, j1 = j0 + kSegChunk;
    if (j1 >= n) return;
    const int32_t row = sorted_rows[j1 - 1];
    if (sorted_rows[j1] != row) return;                                              // the last run ends with the chunk
    if (sorted_rows[j0] == row && j0 > 0 && sorted_rows[j0 - 1] == row) return;      // it began earlier: that chunk's lane adds it
    int64_t lo = j1, hi = n;                                                         // the run's end: first position > row
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted_rows[mid] <= row) lo = mid + 1; else hi = mid;
    }
    const int64_t last = (lo - 1) / kSegChunk;
    float sum = tail_part[c];
#pragma unroll 8
    for (int64_t k = c + 1; k <= last; ++k) sum += head_part[k];
    if (row >= 0 && row < arena_rows) g_arena[row] = sum;
}

// part[chunk, k] = sum over the chunk's rows, ascending, of dense[b, dense_cols[k]] * dlogit[b]
__global__ __launch_bounds__(kLinBlock) void linear_dw_kernel(const float* __restrict__ dense, int64_t dense_stride,
                                                             const int32_t* __restrict__ dense_cols, int n_dense,
                                                             const float* __restrict__ dlogit, int B, int chunks,
                                                             float* __restrict__ part) {
    const int64_t e = (int64_t)blockIdx.x * kLinBlock + threadIdx.x;
    if (e >= (int64_t)chunks * n_dense) return;
    const int chunk = (int)(e / n_dense), k = (int)(e - (int64_t)chunk * n_dense);
    const int c = dense_cols[k];
    float acc = 0.f;
    if (c >= 0 && c < dense_stride) {
        const int b1 = min(B, (chunk + 1) * kDwRows);
        for (int64_t b = (int64_t)chunk * kDwRows; b < b1; ++b) acc = fmaf(dense[b * dense_stride + c], dlogit[b], acc);
    }
    part[e] = acc;
}

struct LinearLayout {
    int64_t n, seg_chunks, dw_chunks;            // slot positions, chunks of the sorted list, row chunks of dweight
    int64_t contrib, head, tail, dw, total;      // byte offsets into the workspace
};

int linear_validate(const satrans_linear_desc* d, const char* who, LinearLayout& L) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->F >= 0 && d->n_dense >= 0 && d->arena_rows >= 0 && d->x_stride >= 0 && d->dense_stride >= 0,
                    SATRANS_E_BADARG, "%s: bad sizes B=%d F=%d n_dense=%d arena_rows=%lld x_stride=%lld dense_stride=%lld", who, d->B,
                    d->F, d->n_dense, (long long)d->arena_rows, (long long)d->x_stride, (long long)d->dense_stride);
    SATRANS_REQUIRE(d->F > 0 || d->n_dense > 0, SATRANS_E_BADARG, "%s: neither fields nor dense columns", who);
    if (d->F > 0) {
        SATRANS_REQUIRE(d->id_dtype >= 0 && d->id_dtype <= 2, SATRANS_E_BADARG, "%s: id_dtype %d", who, d->id_dtype);
        SATRANS_REQUIRE(d->arena_rows < ((int64_t)1 << 31), SATRANS_E_BADARG, "%s: arena_rows = %lld does not fit 31 bits", who,
                        (long long)d->arena_rows);
        if (int rc = check_fields(d->fields, d->F, d->R, d->Fv, d->x_stride, d->arena_rows, who)) return rc;
        SATRANS_REQUIRE((int64_t)d->B * d->R < ((int64_t)1 << 31), SATRANS_E_BADARG, "%s: B * R = %lld does not fit 31 bits", who,
                        (long long)d->B * d->R);
    } else {
        SATRANS_REQUIRE(d->R == 0 && d->Fv == 0, SATRANS_E_BADARG, "%s: R = %d, Fv = %d without fields", who, d->R, d->Fv);
    }
    auto align = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
    L.n = (int64_t)d->B * d->R;
    L.seg_chunks = ceil_div(L.n, kSegChunk);
    L.dw_chunks = ceil_div(d->B, kDwRows);
    L.contrib = 0;
    L.head = align(L.contrib + 4 * L.n);
    L.tail = align(L.head + 4 * L.seg_chunks);
    L.dw = align(L.tail + 4 * L.seg_chunks);
    L.total = align(L.dw + 4 * L.dw_chunks * d->n_dense);
    return SATRANS_OK;
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_linear_workspace_bytes(const satrans_linear_desc* d) {
    LinearLayout L;
    const int rc = linear_validate(d, "linear_workspace_bytes", L);
    return rc ? rc : L.total;
}

extern "C" int satrans_linear_fwd(const satrans_linear_desc* d, float* logit, int32_t* rows_out, uint32_t* mask_out,
                                  uint8_t* argmax_out, int32_t* status, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    LinearLayout L;
    if (int rc = linear_validate(d, "linear_fwd", L)) return rc;
    SATRANS_REQUIRE(logit && status, SATRANS_E_BADARG, "linear_fwd: null pointer");
    SATRANS_REQUIRE(d->F == 0 || (d->arena && d->X && rows_out && (d->Fv == 0 || (mask_out && argmax_out))), SATRANS_E_BADARG,
                    "linear_fwd: null pointer (arena, X, rows_out; mask_out and argmax_out with varlen fields)");
    SATRANS_REQUIRE(d->n_dense == 0 || (d->dense && d->dense_cols && d->weight && d->dense_stride > 0), SATRANS_E_BADARG,
                    "linear_fwd: null pointer (dense, dense_cols, weight) or dense_stride = 0");
    const PoolFields pf = pool_fields_of(d->fields, d->F);
    const int64_t blocks = std::min<int64_t>(ceil_div(d->B, kLinSamples), kLinMaxBlocks);
    linear_fwd_kernel<<<(unsigned)blocks, kLinBlock, 0, st>>>(d->arena, pf, d->F, d->R, d->Fv, d->X, d->id_dtype, d->x_stride, d->B,
                                                             d->dense, d->dense_stride, d->dense_cols, d->weight, d->n_dense, logit,
                                                             rows_out, mask_out, argmax_out, status);
    SATRANS_CHECK_LAUNCH("linear_fwd_kernel");
    return SATRANS_OK;
}

extern "C" int satrans_linear_bwd(const satrans_linear_desc* d, const float* dlogit, const int32_t* rows, const uint32_t* mask,
                                  const uint8_t* argmax, const int32_t* sorted_rows, const int32_t* src, float* g_arena,
                                  float* dweight, void* workspace, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    LinearLayout L;
    if (int rc = linear_validate(d, "linear_bwd", L)) return rc;
    (void)rows;      // the forward's rows_out: sorted_rows carries the same rows, nothing else reads them here
    SATRANS_REQUIRE(dlogit && workspace, SATRANS_E_BADARG, "linear_bwd: null pointer");
    SATRANS_REQUIRE(d->F == 0 || (sorted_rows && src && g_arena && (d->Fv == 0 || (mask && argmax))), SATRANS_E_BADARG,
                    "linear_bwd: null pointer (sorted_rows, src, g_arena; mask and argmax with varlen fields)");
    SATRANS_REQUIRE(d->n_dense == 0 || (d->dense && d->dense_cols && dweight && d->dense_stride > 0), SATRANS_E_BADARG,
                    "linear_bwd: null pointer (dense, dense_cols, dweight) or dense_stride = 0");
    char* ws = (char*)workspace;
    if (d->F > 0) {
        float* contrib = (float*)(ws + L.contrib);
        float* head = (float*)(ws + L.head);
        float* tail = (float*)(ws + L.tail);
        const PoolFields pf = pool_fields_of(d->fields, d->F);
        const int64_t n_items = (int64_t)d->B * d->F;
        const int64_t blocks = std::min<int64_t>(ceil_div(n_items, kLinBlock), kLinMaxBlocks);      // grid-strided beyond
        linear_contrib_kernel<<<(unsigned)blocks, kLinBlock, 0, st>>>(dlogit, pf, d->F, d->R, d->Fv, n_items, mask, argmax, contrib);
        SATRANS_CHECK_LAUNCH("linear_contrib_kernel");
        const unsigned seg_blocks = (unsigned)ceil_div(L.seg_chunks, kLinBlock);
        linear_seg_chunk_kernel<<<seg_blocks, kLinBlock, 0, st>>>(sorted_rows, src, L.n, d->arena_rows, contrib, head, tail, g_arena);
        SATRANS_CHECK_LAUNCH("linear_seg_chunk_kernel");
        linear_seg_join_kernel<<<seg_blocks, kLinBlock, 0, st>>>(sorted_rows, L.n, d->arena_rows, head, tail, g_arena);
        SATRANS_CHECK_LAUNCH("linear_seg_join_kernel");
    }
    if (d->n_dense > 0) {
        float* part = (float*)(ws + L.dw);
        const int64_t e = L.dw_chunks * d->n_dense;
        linear_dw_kernel<<<(unsigned)ceil_div(e, kLinBlock), kLinBlock, 0, st>>>(d->dense, d->dense_stride, d->dense_cols, d->n_dense,
                                                                               dlogit, d->B, (int)L.dw_chunks, part);
        SATRANS_CHECK_LAUNCH("linear_dw_kernel");
        mmoe_reduce_kernel<false><<<(unsigned)ceil_div(d->n_dense, kThreads), kThreads, 0, st>>>(
            part, nullptr, nullptr, d->B, (int64_t)d->n_dense, 1, 0, 1, 1, (int)L.dw_chunks, dweight, nullptr);
        SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel");
    }
    return SATRANS_OK;
}
