// STAR's star-topology towers (reference models/star.py:156-170) for a mixed batch: every scenario's FC tower in one set of
// launches.  Layer l of scenario s multiplies by W_eff[s,l] = W_dom[s,l] * W_sh[l] (elementwise) and adds b_dom[s,l] + b_sh[l].
//
// Layout.  x [B,C], the hidden rows, the dz rows and dx all stay in the caller's row order; a scenario's run is cut into row
// tiles of kTM rows (products) or chunks of kDwChunk rows (weight gradients) and the grids are sized in slots, as seg_walk.h
// describes.  A workgroup owns (one row tile) x (one tile of kTN output columns) and streams the contraction in steps of kTK.
//
// Products.  The tile product and the weight-gradient body are those of grouped_gemm.h, shared with the scenario heads: exact
// f32-input MFMA, a result element is a k-ordered fmaf chain, so it does not depend on the tile a row falls into.  This file
// holds the reduction (which folds in W_sh and the sum over scenarios), the layout, the validation and the launches.  W_eff is
// never materialised: the weight tile is W_dom * W_sh, multiplied on its way into LDS (the SHARED form of the tile body; both
// L2-resident; at S = 32 a materialised W_eff would be another 24 MB written and read).
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

#include "grouped_gemm.h"

namespace satrans {
namespace {

static_assert(SATRANS_STAR_ROW_TILE == SATRANS_MMOE_ROW_TILE && SATRANS_STAR_DW_ROW_CHUNK == SATRANS_MMOE_DW_ROW_CHUNK,
              "STAR's row tile and weight-gradient chunk are those of grouped_gemm.h");

// out[row, n] = epilogue(sum_k in[row, k] * Weff[s][n, k])                     WT = false   (W [N, K] per scenario)
// out[row, n] = epilogue(sum_k in[row, k] * Weff[s][k, n])                     WT = true    (W [K, N] per scenario)
// epilogue: + b_dom[s][n] + b_sh[n] (when b_dom), relu (when relu), * (mask[row, n] > 0) (when mask)
// grid: row-tile slots x n tiles
template <bool WT>
__global__ __launch_bounds__(kThreads) void star_gemm_kernel(const float* __restrict__ in, const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ seg, int B, int K, int N, int S, int ntiles,
                                                             const float* __restrict__ w_dom, const float* __restrict__ w_sh,
                                                             const float* __restrict__ b_dom, const float* __restrict__ b_sh,
                                                             int relu, const float* __restrict__ mask, float* __restrict__ out) {
    gemm_tile<WT, /*ROUTED=*/true, /*SHARED=*/true>(in, K, 0, order, seg, B, K, N, S, 1, ntiles, w_dom, w_sh, b_dom, b_sh, relu, mask, 0,
                                                    out, N, 0);
}

// part_w[chunk][n, k] = sum over the chunk's rows of dz[row, n] * h[row, k];  part_b[chunk][n] = sum of dz[row, n]
// grid: chunk slots x n tiles x k tiles.  The routed body of mmoe_dw_kernel with G = 1 and whole rows as constants: a workgroup
// runs only eight steps, so the two divisions by a runtime G in front of them would show (1 % of forward + backward at S = 32).
__global__ __launch_bounds__(kThreads) void star_dw_kernel(const float* __restrict__ dz, const float* __restrict__ h,
                                                           const int32_t* __restrict__ order, const int32_t* __restrict__ seg, int B,
                                                           int K, int N, int S, int ntiles, int ktiles, float* __restrict__ part_w,
                                                           float* __restrict__ part_b) {
    dw_tile<true>(dz, N, 0, h, K, 0, order, seg, B, K, N, S, 1, ntiles, ktiles, part_w, part_b);
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
