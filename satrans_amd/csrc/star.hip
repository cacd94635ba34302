// STAR's star-topology towers (reference models/star.py:156-170) for a mixed batch: every scenario's FC tower in one set of
// launches.  Layer l of scenario s multiplies by W_eff[s,l] = W_dom[s,l] * W_sh[l] (elementwise) and adds b_dom[s,l] + b_sh[l].
//
// Layout.  x [B,C], the hidden rows, the dz rows and dx all stay in the caller's row order; a scenario's run is cut into row
// tiles of kTM rows (products) or chunks of kDwChunk rows (weight gradients) and the grids are sized in slots, as seg_walk.h
// describes.  A workgroup owns (one row tile) x (one tile of kTN output columns) and streams the contraction in steps of kTK.
//
// Products.  Exact f32-input MFMA (v_mfma_f32_32x32x2_f32): a result element is a k-ordered fmaf chain, so it does not depend on
// the tile a row falls into.  The four waves of a workgroup take the 2 x 2 quadrants of its 64 x 64 tile, one 32 x 32
// accumulator each.  Both operands go through LDS ([64][kTK + 1] floats, conflict-free for the fragment reads); the next step's
// global loads are issued before the current step's MFMAs.  W_eff is never materialised: the weight tile is W_dom * W_sh,
// multiplied on its way into LDS (both L2-resident; at S = 32 a materialised W_eff would be another 24 MB written and read).
//
//   forward   h_l = relu(h_{l-1} W_eff^T + b_eff), every layer one launch of star_gemm_kernel<false>; the last layer (width 1) is
//             the same kernel with one valid column.  h_1 .. h_{L-1} are SAVED (row order) for the backward.
//   backward  per layer, last to first:
//             star_dw_kernel      part[chunk] = dz_l^T h_{l-1} over a chunk of kDwChunk rows counted from the start of the
//                                 scenario's run, and the chunk's column sums of dz_l (the bias gradient)
//             star_reduce_kernel  the chunks of a scenario in chunk order, the scenarios in scenario order (fp64 sums of the fp32
//                                 partials) -> g_W_dom, g_b_dom, g_W_sh, g_b_sh, all WRITTEN; a scenario without rows gets zeros
//             star_gemm_kernel<true>   dh_{l-1} = dz_l W_eff, masked by h_{l-1} > 0 into dz_{l-1}, or written as dx for l = 1
// No floating-point atomics anywhere: equal inputs give equal bits, and a scenario's rows give the same bits alone as in a mix.
#include <algorithm>

#include "seg_walk.h"

namespace satrans {
namespace {

constexpr int kTM = SATRANS_STAR_ROW_TILE;
constexpr int kTN = 64;
constexpr int kTK = 32;
constexpr int kLd = kTK + 1;
constexpr int kThreads = 256;
constexpr int kDwChunk = SATRANS_STAR_DW_ROW_CHUNK;
constexpr int kPer = kTM * kTK / kThreads;      // elements of an operand tile per thread
static_assert(kTM == 64 && kTN == 64, "four waves take the 2 x 2 quadrants of 32 x 32");
static_assert(kDwChunk % kTK == 0 && kPer == 8, "tile loaders");

typedef float f32x16 __attribute__((ext_vector_type(16)));

// one contraction step of the workgroup's 64 x 64 tile: wave quadrant (wm, wn), A[i][k] = As[i][k], B[k][j] = Bs[j][k]
__device__ __forceinline__ void mma_step(const float (*As)[kLd], const float (*Bs)[kLd], int lane, int wm, int wn, f32x16& acc) {
    const int r = lane & 31, h = lane >> 5;
    const float* a = &As[wm * 32 + r][h];
    const float* b = &Bs[wn * 32 + r][h];
#pragma unroll
    for (int kk = 0; kk < kTK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], acc, 0, 0, 0);
}

// Thread mappings of a [64][kTK] operand tile, element e = 0..kPer-1 of thread t:
//   "k fast"  (the contraction index is contiguous in memory):  i = (t >> 5) + 8 e,  k = t & 31
//   "i fast"  (the tile's row index is contiguous in memory):   i = t & 63,          k = (t >> 6) + 4 e

// ---- forward layers and the input gradients -------------------------------------------------------------------------------------

// out[row, n] = epilogue(sum_k in[row, k] * Weff[s][n, k])                     WT = false   (W [N, K] per scenario)
// out[row, n] = epilogue(sum_k in[row, k] * Weff[s][k, n])                     WT = true    (W [K, N] per scenario)
// epilogue: + b_dom[s][n] + b_sh[n] (when b_dom), relu (when relu), * (mask[row, n] > 0) (when mask)
template <bool WT>
__global__ __launch_bounds__(kThreads) void star_gemm_kernel(const float* __restrict__ in, const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ seg, int B, int K, int N, int S, int ntiles,
                                                             const float* __restrict__ w_dom, const float* __restrict__ w_sh,
                                                             const float* __restrict__ b_dom, const float* __restrict__ b_sh,
                                                             int relu, const float* __restrict__ mask, float* __restrict__ out) {
    __shared__ float As[kTM][kLd];
    __shared__ float Bs[kTN][kLd];
    __shared__ int rows_sh[kTM];
    const int slot = blockIdx.x / ntiles, n0 = (blockIdx.x % ntiles) * kTN;
    const SegSlot tl = find_slot<SegSlot>(seg, S, B, slot, kTM);
    if (tl.s < 0) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w & 1, wn = w >> 1;
    if (t < kTM) rows_sh[t] = row_at(order, tl.r0 + t, tl.r1, B);
    const float* wd = w_dom + (size_t)tl.s * N * K;
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    const int jf = t & 63, kf0 = t >> 6;      // "i fast"
    int my_rows[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) my_rows[e] = row_at(order, tl.r0 + if0 + 8 * e, tl.r1, B);
    float ra[kPer], rb[kPer];
    auto load = [&](int k0) {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int k = k0 + kf;
            ra[e] = (my_rows[e] >= 0 && k < K) ? in[(size_t)my_rows[e] * K + k] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            size_t at;
            bool ok;
            if (WT) {
                const int n = n0 + jf, k = k0 + kf0 + 4 * e;
                ok = n < N && k < K;
                at = (size_t)k * N + n;
            } else {
                const int n = n0 + if0 + 8 * e, k = k0 + kf;
                ok = n < N && k < K;
                at = (size_t)n * K + k;
            }
            rb[e] = ok ? wd[at] * w_sh[at] : 0.f;
        }
    };
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    load(0);
    for (int k0 = 0; k0 < K; k0 += kTK) {
        __syncthreads();      // the previous step's fragment reads are done
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            As[if0 + 8 * e][kf] = ra[e];
            if (WT)
                Bs[jf][kf0 + 4 * e] = rb[e];
            else
                Bs[if0 + 8 * e][kf] = rb[e];
        }
        __syncthreads();
        if (k0 + kTK < K) load(k0 + kTK);
        mma_step(As, Bs, lane, wm, wn, acc);
    }
    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= N) return;
    const float bias = b_dom ? b_dom[(size_t)tl.s * N + n] + b_sh[n] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = rows_sh[wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)];
        if (row < 0) continue;
        float v = acc[q] + bias;
        if (relu) v = fmaxf(v, 0.f);
        const size_t at = (size_t)row * N + n;
        if (mask) v = mask[at] > 0.f ? v : 0.f;
        out[at] = v;
    }
}

// ---- weight gradients -----------------------------------------------------------------------------------------------------------

// part_w[chunk][n, k] = sum over the chunk's rows of dz[row, n] * h[row, k];  part_b[chunk][n] = sum of dz[row, n]
// grid: chunk slots x n tiles x k tiles
__global__ __launch_bounds__(kThreads) void star_dw_kernel(const float* __restrict__ dz, const float* __restrict__ h,
                                                           const int32_t* __restrict__ order, const int32_t* __restrict__ seg, int B,
                                                           int K, int N, int S, int ntiles, int ktiles, float* __restrict__ part_w,
                                                           float* __restrict__ part_b) {
    __shared__ float As[kTM][kLd];      // [n][row of the step]
    __shared__ float Bs[kTN][kLd];      // [k][row of the step]
    const int per_slot = ntiles * ktiles;
    const int slot = blockIdx.x / per_slot, rem = blockIdx.x % per_slot;
    const int n0 = (rem / ktiles) * kTM, c0 = (rem % ktiles) * kTN;
    const SegSlot tl = find_slot<SegSlot>(seg, S, B, slot, kDwChunk);
    if (tl.s < 0) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w & 1, wn = w >> 1;
    const int jf = t & 63, kf0 = t >> 6;
    float ra[kPer], rb[kPer];
    auto load = [&](int p0) {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int row = row_at(order, p0 + kf0 + 4 * e, tl.r1, B);
            const int n = n0 + jf, c = c0 + jf;
            ra[e] = (row >= 0 && n < N) ? dz[(size_t)row * N + n] : 0.f;
            rb[e] = (row >= 0 && c < K) ? h[(size_t)row * K + c] : 0.f;
        }
    };
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    load(tl.r0);
    for (int p0 = tl.r0; p0 < tl.r1; p0 += kTK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            As[jf][kf0 + 4 * e] = ra[e];
            Bs[jf][kf0 + 4 * e] = rb[e];
        }
        __syncthreads();
        if (p0 + kTK < tl.r1) load(p0 + kTK);
        if (c0 == 0 && t < kTM) {      // the bias gradient: rows of the chunk in order (rows past its end hold zeros)
#pragma unroll
            for (int kk = 0; kk < kTK; ++kk) bsum += As[t][kk];
        }
        mma_step(As, Bs, lane, wm, wn, acc);
    }
    if (c0 == 0 && t < kTM && n0 + t < N) part_b[(size_t)slot * N + n0 + t] = bsum;
    const int c = c0 + wn * 32 + (lane & 31);
    if (c >= K) return;
    float* out = part_w + (size_t)slot * N * K;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int n = n0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (n < N) out[(size_t)n * K + c] = acc[q];
    }
}

// One thread per element of [N*K weights | N biases]: the chunks of a scenario in chunk order, the scenarios in scenario order.
__global__ __launch_bounds__(kThreads) void star_reduce_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                               const int32_t* __restrict__ seg, int B, int64_t NK, int N, int S,
                                                               const float* __restrict__ w_dom, const float* __restrict__ w_sh,
                                                               float* __restrict__ g_w_dom, float* __restrict__ g_b_dom,
                                                               float* __restrict__ g_w_sh, float* __restrict__ g_b_sh) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= NK + N) return;
    const bool is_w = e < NK;
    const int64_t at = is_w ? e : e - NK, width = is_w ? NK : N;
    const float* part = is_w ? part_w : part_b;
    const float sh = is_w ? w_sh[at] : 0.f;
    double total = 0.0;
    int k0 = 0;
    for (int s = 0; s < S; ++s) {
        const int nch = scenario_units(seg, s, B, kDwChunk);
        double sum = 0.0;
        for (int k = k0; k < k0 + nch; ++k) sum += part[(size_t)k * width + at];
        k0 += nch;
        const float g = (float)sum;
        if (is_w) {
            g_w_dom[(size_t)s * NK + at] = g * sh;
            total += (double)g * w_dom[(size_t)s * NK + at];
        } else {
            g_b_dom[(size_t)s * N + at] = g;
            total += g;
        }
    }
    (is_w ? g_w_sh : g_b_sh)[at] = (float)total;
}

struct StarLayout {
    int64_t slots, dw_slots, hidden, max_w, dz, part, total;
};

StarLayout star_layout(const satrans_star_desc* d) {
    StarLayout L;
    L.slots = seg_slots(d->B, d->S, kTM);
    L.dw_slots = seg_slots(d->B, d->S, kDwChunk);
    L.hidden = 0;
    L.max_w = 0;
    int64_t prev = d->C, per_chunk = 0;
    for (int l = 0; l < d->L; ++l) {
        const int64_t n = d->width[l];
        if (l < d->L - 1) {
            L.hidden += n;
            L.max_w = std::max(L.max_w, n);
        }
        per_chunk = std::max(per_chunk, n * (prev + 1));
        prev = n;
    }
    L.dz = 0;                                  // two buffers [B, max_w], used in turn
    L.part = 2 * (int64_t)d->B * L.max_w;      // [dw_slots][n * k] then [dw_slots][n], of the layer in hand
    L.total = L.part + L.dw_slots * per_chunk;
    return L;
}

// checks the descriptor and hands out its layout
int star_validate(const satrans_star_desc* d, const char* who, StarLayout& L) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->C > 0 && d->S > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d C=%d S=%d", who, d->B, d->C, d->S);
    SATRANS_REQUIRE(d->L >= 2 && d->L <= SATRANS_STAR_MAX_LAYERS, SATRANS_E_BADARG,
                    "%s: bad sizes L=%d (1 to %d hidden layers and the logit layer)", who, d->L, SATRANS_STAR_MAX_LAYERS - 1);
    for (int l = 0; l < d->L; ++l)
        SATRANS_REQUIRE(d->width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes width[%d]=%d", who, l, d->width[l]);
    SATRANS_REQUIRE(d->width[d->L - 1] == 1, SATRANS_E_BADARG, "%s: bad sizes: the last layer has width 1, got %d", who,
                    d->width[d->L - 1]);
    SATRANS_REQUIRE(d->S <= 65535, SATRANS_E_UNSUPPORTED, "%s: S=%d scenarios (65535 at most)", who, d->S);
    L = star_layout(d);
    int64_t prev = d->C;
    for (int l = 0; l < d->L; ++l) {
        const int64_t n = d->width[l];
        SATRANS_REQUIRE(n * prev <= 0x7fffffffLL && L.slots * ceil_div(std::max(n, prev), kTN) <= 0x7fffffffLL &&
                            L.dw_slots * ceil_div(n, kTM) * ceil_div(prev, kTN) <= 0x7fffffffLL,
                        SATRANS_E_UNSUPPORTED, "%s: layer %d (%lld x %lld) at B=%d needs more than 2^31 workgroups", who, l,
                        (long long)n, (long long)prev, d->B);
        prev = n;
    }
    return SATRANS_OK;
}

bool star_has_operands(const satrans_star_desc* d) {
    if (!d->x || !d->order || !d->seg) return false;
    for (int l = 0; l < d->L; ++l)
        if (!d->w_dom[l] || !d->b_dom[l] || !d->w_sh[l] || !d->b_sh[l]) return false;
    return true;
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_star_saved_floats(const satrans_star_desc* d) {
    StarLayout L;
    const int rc = star_validate(d, "star_saved_floats", L);
    return rc ? rc : (int64_t)d->B * L.hidden;
}

extern "C" int64_t satrans_star_workspace_floats(const satrans_star_desc* d) {
    StarLayout L;
    const int rc = star_validate(d, "star_workspace_floats", L);
    return rc ? rc : L.total;
}

extern "C" int satrans_star_fwd(const satrans_star_desc* d, float* logit, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    StarLayout L;
    const int rc = star_validate(d, "star_fwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(star_has_operands(d) && logit && saved, SATRANS_E_BADARG, "star_fwd: null pointer");
    const int B = d->B, S = d->S;
    const float* in = d->x;
    float* h = saved;
    int K = d->C;
    for (int l = 0; l < d->L; ++l) {
        const int N = d->width[l], ntiles = (int)ceil_div(N, kTN);
        const bool last = l == d->L - 1;
        float* out = last ? logit : h;
        star_gemm_kernel<false><<<(unsigned)(L.slots * ntiles), kThreads, 0, st>>>(in, d->order, d->seg, B, K, N, S, ntiles, d->w_dom[l],
                                                                                   d->w_sh[l], d->b_dom[l], d->b_sh[l], last ? 0 : 1,
                                                                                   nullptr, out);
        SATRANS_CHECK_LAUNCH("star_gemm_kernel (forward)");
        in = out;
        h += (size_t)B * N;
        K = N;
    }
    return SATRANS_OK;
}

extern "C" int satrans_star_bwd(const satrans_star_desc* d, const float* dlogit, float* dx, const float* saved, float* workspace,
                                float* const* g_w_dom, float* const* g_b_dom, float* const* g_w_sh, float* const* g_b_sh,
                                void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    StarLayout L;
    const int rc = star_validate(d, "star_bwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(star_has_operands(d) && dlogit && dx && saved && workspace && g_w_dom && g_b_dom && g_w_sh && g_b_sh,
                    SATRANS_E_BADARG, "star_bwd: null pointer");
    for (int l = 0; l < d->L; ++l)
        SATRANS_REQUIRE(g_w_dom[l] && g_b_dom[l] && g_w_sh[l] && g_b_sh[l], SATRANS_E_BADARG, "star_bwd: null pointer (layer %d)", l);
    const int B = d->B, S = d->S;
    // h_{l-1} of layer l: x for l = 0, else the saved rows of layer l - 1
    const float* hin[SATRANS_STAR_MAX_LAYERS];
    int kin[SATRANS_STAR_MAX_LAYERS];
    {
        const float* h = saved;
        hin[0] = d->x;
        kin[0] = d->C;
        for (int l = 1; l < d->L; ++l) {
            hin[l] = h;
            kin[l] = d->width[l - 1];
            h += (size_t)B * d->width[l - 1];
        }
    }
    float* dzbuf[2] = {workspace + L.dz, workspace + L.dz + (size_t)B * L.max_w};
    const float* dz = dlogit;
    for (int l = d->L - 1; l >= 0; --l) {
        const int N = d->width[l], K = kin[l];
        const int64_t NK = (int64_t)N * K;
        const int ntiles = (int)ceil_div(N, kTM), ktiles = (int)ceil_div(K, kTN);
        float* part_w = workspace + L.part;
        float* part_b = part_w + L.dw_slots * NK;
        star_dw_kernel<<<(unsigned)(L.dw_slots * ntiles * ktiles), kThreads, 0, st>>>(dz, hin[l], d->order, d->seg, B, K, N, S, ntiles,
                                                                                      ktiles, part_w, part_b);
        SATRANS_CHECK_LAUNCH("star_dw_kernel");
        star_reduce_kernel<<<(unsigned)ceil_div(NK + N, kThreads), kThreads, 0, st>>>(part_w, part_b, d->seg, B, NK, N, S, d->w_dom[l],
                                                                                      d->w_sh[l], g_w_dom[l], g_b_dom[l], g_w_sh[l],
                                                                                      g_b_sh[l]);
        SATRANS_CHECK_LAUNCH("star_reduce_kernel");
        // dh_{l-1} = dz_l W_eff: contraction over this layer's N outputs, K columns out
        float* out = l == 0 ? dx : dzbuf[l & 1];
        const int otiles = (int)ceil_div(K, kTN);
        star_gemm_kernel<true><<<(unsigned)(L.slots * otiles), kThreads, 0, st>>>(dz, d->order, d->seg, B, N, K, S, otiles, d->w_dom[l],
                                                                                  d->w_sh[l], nullptr, nullptr, 0,
                                                                                  l == 0 ? nullptr : hin[l], out);
        SATRANS_CHECK_LAUNCH("star_gemm_kernel (backward)");
        dz = out;
    }
    return SATRANS_OK;
}
