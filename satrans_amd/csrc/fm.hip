// The pairwise-interaction family of deepctr-torch 0.2.9, which the reference's models/deepfm.py, nfm.py and afm.py import, and the
// halves of DeepFM.forward (deepfm.py:87-113), NFM.forward (nfm.py:73-83) and AFM.forward (afm.py:66-73) behind the lookup.
// e [B, F, D], S = sum_f e_f:
//     FM                     out[b]   = 0.5 sum_d (S_d^2 - sum_f e_fd^2)        de_f  = dout (S - e_f)
//     BiInteractionPooling   out[b,d] = 0.5 (S_d^2 - sum_f e_fd^2)              de_fd = dout_d (S_d - e_fd)
//     AFM, over the pairs p = (i, j), i < j, in pair_index.h's order, P = F (F - 1) / 2:
//         x_p = e_i * e_j   z_p = x_p W + b   t_p = relu(z_p)   a = softmax_p(t_p h)   ao = sum_p a_p x_p   out = ao . pp
//         do = dout pp   da_p = do . x_p   ds_p = a_p (da_p - sum_q a_q da_q)   dt_p = ds_p h [z_p > 0]
//         dx_p = a_p do + W dt_p   de_i += dx_p e_j   de_j += dx_p e_i
//         dW = sum x_p^T dt_p   db = sum dt_p   dh = sum ds_p t_p   dpp = sum_b dout ao
//
// fm_rows_fwd_kernel / fm_rows_bwd_kernel   a wave per row, a lane per d (d, d + 64): one pass over the row's F D floats each way.
//                        Forward: S_d and the squares f ascending; the FM term over d by a fixed butterfly, with linear_logit and
//                        out.bias into the logit; or the pooled row into the DNN input; flatten(e) and the dense columns copied
//                        into the DNN input on the way.  Backward: S_d again, then de written once: the DNN input gradient's
//                        embedding block plus the FM or pooling term; ddense beside it.
// afm_fwd_kernel         a workgroup owns whole samples, `n` of them a pass: their rows once into LDS (odd stride); a thread per
//                        (sample, pair) forms x_p[d] from two LDS reads as the operand of the [pairs, D] x [D, A] product, eight
//                        columns of A at a time in registers (those columns of W through LDS), relu, times h: the score stays in LDS;
//                        the softmax a wave per sample (fixed butterflies); ao a thread per (sample, d), p ascending, from
//                        regenerated products; out a wave per sample.  Written: out, a [B, P], ao [B, D].
// afm_bwd_kernel         the same staging; a thread per (sample, pair) recomputes z_p (its sign bits into LDS, one word of 64 per
//                        pair: the relu mask is not stored between the passes) and da_p; a wave per sample turns da into ds in
//                        place; a thread per (sample, f, d) is the only writer of its de element, partners ascending, dx_p[d]
//                        regenerated from ds_p, the mask and W h; the parameter sums G[d, a] = sum mask_pa ds_p x_p[d] (row D:
//                        x = 1, which is db / h) by threads (d, eight columns of A, item group), groups merged in order through
//                        LDS into the workgroup's partial.  At the end the workgroup forms dh = sum_d W G + b G_D from its own
//                        G, scales G by h, and leaves [dW | db | dh | dpp] = D A + 2 A + D floats.
// afm_reduce_kernel      the workgroups' partials in a fixed order (fp64: kReduceGroups contiguous shares, then the shares), and
//                        sum_b dout for out.bias in a fixed tree.
// VALU, not the matrix pipe: see DESIGN.md 3.16.  The DNN of the two heads is head_layers.h's dense launcher.
// No floating-point atomics; every sum has a fixed order; a sample's results do not depend on its place in a pass.  fp32 only.
#include "head_layers.h"
#include "pair_index.h"

namespace satrans {
namespace {

constexpr int kFmF = SATRANS_FM_MAX_FIELDS;
constexpr int kFmD = SATRANS_FM_MAX_DIM;
constexpr int kAfmA = SATRANS_AFM_MAX_FACTOR;
constexpr int kAfmWg = SATRANS_AFM_MAX_WORKGROUPS;
constexpr int kAfmRow = kFmF * (kFmD | 1);          // floats of the staged rows: one sample at the limits, rows of odd stride
constexpr int kAfmPairs = kFmF * (kFmF - 1) / 2;    // scores of a pass: one sample at the limits
constexpr int kAfmGroup = 16;                       // samples of a pass at most
constexpr int kAfmCols = 8;                         // columns of A a thread holds at a time
constexpr int kFmRows = kThreads / kWave;           // rows of a workgroup of the row kernels: a wave each
static_assert(kAfmRow * sizeof(float) <= 33 * 1024 && kAfmPairs * sizeof(float) <= 8 * 1024, "a sample's rows and scores in LDS");
static_assert(kFmF <= 256 && kAfmA <= 64, "a pair packs into 16 bits, a pair's relu mask into 64");
static_assert(kFmD <= kThreads && kAfmA <= kThreads, "a thread per d and per a in the epilogues");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- FM and BiInteractionPooling ------------------------------------------------------------------------------------------------

// grid: ceil(B / 4).  With t_d = 0.5 (S_d^2 - sum_f e_fd^2):
//   copy_e: x[row, f D + d] = e;   pool: x[row, d] = t_d;   dense_dim: x[row, ld - dense_dim + c] = dense[row, c];
//   logit (when not null): logit[row] = (fm ? sum_d t_d : 0) + lin[row] + bias[0]   (lin, bias: when not null)
__global__ __launch_bounds__(kThreads) void fm_rows_fwd_kernel(const float* __restrict__ e, int B, int F, int D, int copy_e, int pool, int fm,
                                                               const float* __restrict__ dense, int dense_dim,
                                                               const float* __restrict__ lin, const float* __restrict__ bias,
                                                               float* __restrict__ x, int ld, float* __restrict__ logit) {
    const int64_t row = (int64_t)blockIdx.x * kFmRows + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    const float* er = e + (size_t)row * F * D;
    float* xr = x ? x + (size_t)row * ld : nullptr;
    float term = 0.f;
    for (int d = lane; d < D; d += kWave) {
        float s = 0.f, q = 0.f;
        for (int f = 0; f < F; ++f) {
            const float v = er[f * D + d];
            s += v;
            q = fmaf(v, v, q);
            if (copy_e) xr[f * D + d] = v;
        }
        const float td = 0.5f * (s * s - q);
        if (pool) xr[d] = td;
        term += td;
    }
    for (int c = lane; c < dense_dim; c += kWave) xr[ld - dense_dim + c] = dense[(size_t)row * dense_dim + c];
    if (!logit) return;
    float v = fm ? wave_sum(term) : 0.f;
    if (lin) v += lin[row];
    if (bias) v += bias[0];
    if (lane == 0) logit[row] = v;
}

// grid: ceil(B / 4).  de[row, f, d] = (lin_block ? dx[row, f D + d] : 0) + (pool ? dx[row, d] (S_d - e_fd) : 0)
//                                     + (gfm ? gfm[row] (S_d - e_fd) : 0);   ddense[row, c] = dx[row, ld - dense_dim + c]
__global__ __launch_bounds__(kThreads) void fm_rows_bwd_kernel(const float* __restrict__ e, int B, int F, int D, const float* __restrict__ dx,
                                                               int ld, int lin_block, int pool, const float* __restrict__ gfm,
                                                               float* __restrict__ de, float* __restrict__ ddense, int dense_dim) {
    const int64_t row = (int64_t)blockIdx.x * kFmRows + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    const float* er = e + (size_t)row * F * D;
    const float* gr = dx ? dx + (size_t)row * ld : nullptr;
    float* dr = de + (size_t)row * F * D;
    const float g = gfm ? gfm[row] : 0.f;
    for (int d = lane; d < D; d += kWave) {
        float s = 0.f;
        for (int f = 0; f < F; ++f) s += er[f * D + d];
        const float c = (pool ? gr[d] : 0.f) + g;
        for (int f = 0; f < F; ++f) {
            const float v = c * (s - er[f * D + d]);
            dr[f * D + d] = lin_block ? gr[f * D + d] + v : v;
        }
    }
    for (int c = lane; c < dense_dim; c += kWave) ddense[(size_t)row * dense_dim + c] = gr[ld - dense_dim + c];
}

// the sum of v[0 .. n) in a fixed order: a thread's strided share in index order (fp64), then a fixed tree over the threads
__device__ float block_sum_ordered(const float* __restrict__ v, int64_t n, double* sh) {
    const int t = threadIdx.x;
    double s = 0.0;
    for (int64_t i = t; i < n; i += kThreads) s += v[i];
    sh[t] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    return (float)sh[0];
}

// grid: 1.  out[0] = sum_b v[b]
__global__ __launch_bounds__(kThreads) void fm_sum_kernel(const float* __restrict__ v, int64_t n, float* __restrict__ out) {
    __shared__ double sh[kThreads];
    const float s = block_sum_ordered(v, n, sh);
    if (threadIdx.x == 0) out[0] = s;
}

// ---- AFM ------------------------------------------------------------------------------------------------------------------------

// the rows of the pass's m samples into LDS (rows of stride Dp)
__device__ __forceinline__ void afm_stage(const float* __restrict__ e, int64_t b0, int m, int F, int D, int Dp, float* se) {
    const int FD = F * D;
    const float* src = e + (size_t)b0 * FD;
    for (int idx = threadIdx.x; idx < m * FD; idx += kThreads) {
        const int s = idx / FD, r = idx - s * FD, f = r / D;
        se[(s * F + f) * Dp + (r - f * D)] = src[idx];
    }
}

__device__ __forceinline__ void afm_pairs(int F, int P, uint16_t* spair) {
    for (int p = threadIdx.x; p < P; p += kThreads) {
        int i, j;
        pair_fields(p, F, i, j);
        spair[p] = (uint16_t)(i | (j << 8));
    }
}

// grid: workgroups; workgroup w owns the passes [w ppw, (w + 1) ppw) of n samples each.
__global__ __launch_bounds__(kThreads) void afm_fwd_kernel(const float* __restrict__ e, const float* __restrict__ W,
                                                           const float* __restrict__ bA, const float* __restrict__ h,
                                                           const float* __restrict__ pp, const float* __restrict__ lin,
                                                           const float* __restrict__ bias, int B, int F, int D, int A, int P, int n,
                                                           int ppw, float* __restrict__ out, float* __restrict__ att,
                                                           float* __restrict__ ao) {
    __shared__ float se[kAfmRow];
    __shared__ float sc[kAfmPairs];
    __shared__ float sao[kAfmGroup * kFmD];
    __shared__ __attribute__((aligned(16))) float sW[kFmD * kAfmCols];
    __shared__ uint16_t spair[kAfmPairs];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, Dp = D | 1, FDp = F * Dp;
    afm_pairs(F, P, spair);
    const int64_t passes = ((int64_t)B + n - 1) / n;
    const int64_t pass0 = (int64_t)blockIdx.x * ppw, pass1 = pass0 + ppw < passes ? pass0 + ppw : passes;
    for (int64_t pass = pass0; pass < pass1; ++pass) {
        const int64_t b0 = pass * n;
        const int m = b0 + n <= B ? n : (int)(B - b0);
        __syncthreads();      // the previous pass's reads are done (the first time: spair is written)
        afm_stage(e, b0, m, F, D, Dp, se);
        __syncthreads();
        for (int a0 = 0; a0 < A; a0 += kAfmCols) {      // eight columns of W at a time through LDS, zero beyond A
            if (a0) __syncthreads();                    // the previous columns' reads are done
            for (int idx = t; idx < D * kAfmCols; idx += kThreads) {
                const int a = a0 + (idx & (kAfmCols - 1));
                sW[idx] = a < A ? W[(idx / kAfmCols) * A + a] : 0.f;
            }
            __syncthreads();
            for (int it = t; it < m * P; it += kThreads) {
                const int s = it / P, pr = spair[it - s * P];
                const float* ei = se + s * FDp + (pr & 255) * Dp;
                const float* ej = se + s * FDp + (pr >> 8) * Dp;
                float z[kAfmCols];
#pragma unroll
                for (int u = 0; u < kAfmCols; ++u) z[u] = 0.f;
#pragma unroll 4
                for (int d = 0; d < D; ++d) {
                    const float xv = ei[d] * ej[d];
                    const float* w = sW + d * kAfmCols;
#pragma unroll
                    for (int u = 0; u < kAfmCols; ++u) z[u] = fmaf(xv, w[u], z[u]);
                }
                float score = a0 ? sc[it] : 0.f;      // (one chain over all of A, in order)
#pragma unroll
                for (int u = 0; u < kAfmCols; ++u)
                    if (a0 + u < A) score = fmaf(fmaxf(z[u] + bA[a0 + u], 0.f), h[a0 + u], score);
                sc[it] = score;
            }
        }
        __syncthreads();
        for (int s = wv; s < m; s += kFmRows) {
            float* r = sc + s * P;
            float mx = -INFINITY, sum = 0.f;
            for (int p = lane; p < P; p += kWave) mx = fmaxf(mx, r[p]);
            mx = wave_max(mx);
            for (int p = lane; p < P; p += kWave) {
                const float v = expf(r[p] - mx);
                r[p] = v;
                sum += v;
            }
            sum = wave_sum(sum);
            for (int p = lane; p < P; p += kWave) {
                const float v = r[p] / sum;
                r[p] = v;
                att[(size_t)(b0 + s) * P + p] = v;
            }
        }
        __syncthreads();
        for (int idx = t; idx < m * D; idx += kThreads) {
            const int s = idx / D, d = idx - s * D;
            const float* er = se + s * FDp + d;
            const float* r = sc + s * P;
            float acc = 0.f;
            for (int p = 0; p < P; ++p) {
                const int pr = spair[p];
                acc = fmaf(r[p], er[(pr & 255) * Dp] * er[(pr >> 8) * Dp], acc);
            }
            sao[idx] = acc;
            ao[(size_t)b0 * D + idx] = acc;
        }
        __syncthreads();
        for (int s = wv; s < m; s += kFmRows) {
            float v = 0.f;
            for (int d = lane; d < D; d += kWave) v = fmaf(sao[s * D + d], pp[d], v);
            v = wave_sum(v);
            if (lin) v += lin[b0 + s];
            if (bias) v += bias[0];
            if (lane == 0) out[b0 + s] = v;
        }
    }
}

// grid: as the forward's.  part: per workgroup [G (D + 1 rows of A; at the end dW and db) | dh (A) | dpp (D)].
__global__ __launch_bounds__(kThreads) void afm_bwd_kernel(const float* __restrict__ e, const float* __restrict__ W,
                                                           const float* __restrict__ bA, const float* __restrict__ h,
                                                           const float* __restrict__ pp, const float* __restrict__ dout,
                                                           const float* __restrict__ att, const float* __restrict__ ao, int B, int F,
                                                           int D, int A, int P, int n, int ppw, float* __restrict__ de, float* part) {
    __shared__ float se[kAfmRow];
    __shared__ float sa[kAfmPairs];
    __shared__ float sds[kAfmPairs];
    __shared__ unsigned long long smask[kAfmPairs];
    __shared__ float red[kThreads * kAfmCols];
    __shared__ uint16_t spair[kAfmPairs];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, Dp = D | 1, FDp = F * Dp, FD = F * D;
    const int nch = (A + kAfmCols - 1) / kAfmCols, ncombo = (D + 1) * nch;      // (row of G, eight of its columns)
    const int cpt = ncombo < kThreads ? ncombo : kThreads;                    // combos of a tile
    const int groups = kThreads / cpt;                                        // item groups of a tile
    const int width = D * A + 2 * A + D;
    float* G = part + (size_t)blockIdx.x * width;
    float* gdh = G + (D + 1) * A;
    float* gdp = gdh + A;
    for (int idx = t; idx < (D + 1) * A; idx += kThreads) G[idx] = 0.f;
    float dp_acc = 0.f;
    afm_pairs(F, P, spair);
    const int64_t passes = ((int64_t)B + n - 1) / n;
    const int64_t pass0 = (int64_t)blockIdx.x * ppw, pass1 = pass0 + ppw < passes ? pass0 + ppw : passes;
    for (int64_t pass = pass0; pass < pass1; ++pass) {
        const int64_t b0 = pass * n;
        const int m = b0 + n <= B ? n : (int)(B - b0);
        const int items = m * P;
        __syncthreads();      // the previous pass's reads are done (the first time: spair and G's zeros are written)
        afm_stage(e, b0, m, F, D, Dp, se);
        for (int it = t; it < items; it += kThreads) sa[it] = att[(size_t)b0 * P + it];
        __syncthreads();
        // z_p again: its sign bits and da_p = dout (pp . x_p)
        for (int it = t; it < items; it += kThreads) {
            const int s = it / P, pr = spair[it - s * P];
            const float* ei = se + s * FDp + (pr & 255) * Dp;
            const float* ej = se + s * FDp + (pr >> 8) * Dp;
            unsigned long long mask = 0;
            float da = 0.f;
            for (int a0 = 0; a0 < A; a0 += kAfmCols) {
                float z[kAfmCols];
#pragma unroll
                for (int u = 0; u < kAfmCols; ++u) z[u] = 0.f;
#pragma unroll 4
                for (int d = 0; d < D; ++d) {
                    const float xv = ei[d] * ej[d];
                    const float* w = W + d * A + a0;
                    if (a0 == 0) da = fmaf(pp[d], xv, da);
#pragma unroll
                    for (int u = 0; u < kAfmCols; ++u)
                        if (a0 + u < A) z[u] = fmaf(xv, w[u], z[u]);
                }
#pragma unroll
                for (int u = 0; u < kAfmCols; ++u)
                    if (a0 + u < A && z[u] + bA[a0 + u] > 0.f) mask |= 1ull << (a0 + u);
            }
            smask[it] = mask;
            sds[it] = dout[b0 + s] * da;
        }
        __syncthreads();
        // ds_p = a_p (da_p - sum_q a_q da_q), in place
        for (int s = wv; s < m; s += kFmRows) {
            const float* a = sa + s * P;
            float* r = sds + s * P;
            float dot = 0.f;
            for (int p = lane; p < P; p += kWave) dot = fmaf(a[p], r[p], dot);
            dot = wave_sum(dot);
            for (int p = lane; p < P; p += kWave) r[p] = a[p] * (r[p] - dot);
        }
        __syncthreads();
        // de: the owner of (sample, f, d), partners ascending
        for (int idx = t; idx < m * FD; idx += kThreads) {
            const int s = idx / FD, r = idx - s * FD, f = r / D, d = r - f * D;
            const float* er = se + s * FDp + d;
            const float dod = dout[b0 + s] * pp[d];
            float acc = 0.f;
            for (int a0 = 0; a0 < A; a0 += kAfmCols) {
                float wh[kAfmCols];
#pragma unroll
                for (int u = 0; u < kAfmCols; ++u) wh[u] = a0 + u < A ? W[d * A + a0 + u] * h[a0 + u] : 0.f;
                for (int o = 0; o < F; ++o) {
                    if (o == f) continue;
                    const int it = s * P + (o < f ? pair_index(o, f, F) : pair_index(f, o, F));
                    const unsigned mk = (unsigned)(smask[it] >> a0);
                    float sum = 0.f;
#pragma unroll
                    for (int u = 0; u < kAfmCols; ++u) sum += (mk >> u) & 1u ? wh[u] : 0.f;
                    float dxv = sds[it] * sum;
                    if (a0 == 0) dxv = fmaf(sa[it], dod, dxv);
                    acc = fmaf(dxv, er[o * Dp], acc);
                }
            }
            de[(size_t)b0 * FD + idx] = acc;
        }
        // G[d, a] += sum over the pass's items of mask_pa ds_p x_p[d]  (row D: x = 1)
        for (int c0 = 0; c0 < ncombo; c0 += cpt) {
            const int cl = t % cpt, gi = t / cpt, combo = c0 + cl;
            float acc[kAfmCols];
#pragma unroll
            for (int u = 0; u < kAfmCols; ++u) acc[u] = 0.f;
            if (gi < groups && combo < ncombo) {
                const int d = combo % (D + 1), a0 = (combo / (D + 1)) * kAfmCols;
                int s = gi / P, p = gi - s * P;
                for (int it = gi; it < items; it += groups) {
                    const int pr = spair[p];
                    const float* er = se + s * FDp;
                    const float xv = d < D ? er[(pr & 255) * Dp + d] * er[(pr >> 8) * Dp + d] : 1.f;
                    const float v = xv * sds[it];
                    const unsigned mk = (unsigned)(smask[it] >> a0);
#pragma unroll
                    for (int u = 0; u < kAfmCols; ++u) acc[u] += (mk >> u) & 1u ? v : 0.f;
                    p += groups;
                    while (p >= P) {
                        p -= P;
                        ++s;
                    }
                }
            }
            __syncthreads();      // the previous tile's merge has read red
#pragma unroll
            for (int u = 0; u < kAfmCols; ++u) red[(gi * cpt + cl) * kAfmCols + u] = acc[u];
            __syncthreads();
            for (int k = t; k < cpt * kAfmCols; k += kThreads) {
                const int c = k / kAfmCols, u = k - c * kAfmCols, cb = c0 + c;
                if (cb >= ncombo) continue;
                const int d = cb % (D + 1), a = (cb / (D + 1)) * kAfmCols + u;
                if (a >= A) continue;
                float sum = 0.f;
                for (int g = 0; g < groups; ++g) sum += red[(g * cpt + c) * kAfmCols + u];
                G[d * A + a] += sum;      // (this thread alone, every pass)
            }
        }
        if (t < D)
            for (int s = 0; s < m; ++s) dp_acc = fmaf(dout[b0 + s], ao[(size_t)(b0 + s) * D + t], dp_acc);
    }
    __threadfence_block();
    __syncthreads();
    if (t < A) {
        float sum = 0.f;
        for (int d = 0; d < D; ++d) sum = fmaf(W[d * A + t], G[d * A + t], sum);
        gdh[t] = fmaf(bA[t], G[D * A + t], sum);
    }
    if (t < D) gdp[t] = dp_acc;
    __threadfence_block();
    __syncthreads();
    for (int idx = t; idx < (D + 1) * A; idx += kThreads) G[idx] *= h[idx % A];
}

// grid: ceil(width / 16) (+ 1 with g_bias: that workgroup sums dout).  The partials [nwg][width]: a workgroup is 16 elements x
// kReduceGroups groups, every group adds its contiguous share of the workgroups in index order (fp64), the group sums are combined
// in group order.
__global__ __launch_bounds__(kThreads) void afm_reduce_kernel(const float* __restrict__ part, int nwg, int width, int DA, int A,
                                                              float* __restrict__ gW, float* __restrict__ gb, float* __restrict__ gh,
                                                              float* __restrict__ gp, const float* __restrict__ dout, int B,
                                                              float* __restrict__ g_bias) {
    __shared__ double sh[kThreads];
    constexpr int kEls = kThreads / kReduceGroups;
    const int nblk = (width + kEls - 1) / kEls;
    if ((int)blockIdx.x >= nblk) {
        const float s = block_sum_ordered(dout, B, sh);
        if (threadIdx.x == 0) g_bias[0] = s;
        return;
    }
    const int t = threadIdx.x, el = blockIdx.x * kEls + t % kEls, grp = t / kEls;
    const int share = (nwg + kReduceGroups - 1) / kReduceGroups;
    const int w0 = grp * share, w1 = w0 + share < nwg ? w0 + share : nwg;
    double sum = 0.0;
    if (el < width) {
#pragma unroll 4
        for (int w = w0; w < w1; ++w) sum += part[(size_t)w * width + el];
    }
    sh[t] = sum;
    __syncthreads();
    if (grp != 0 || el >= width) return;
    for (int g = 1; g < kReduceGroups; ++g) sum += sh[g * kEls + t];
    const float v = (float)sum;
    if (el < DA)
        gW[el] = v;
    else if (el < DA + A)
        gb[el - DA] = v;
    else if (el < DA + 2 * A)
        gh[el - DA - A] = v;
    else
        gp[el - DA - 2 * A] = v;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

int fm_shape(int B, int F, int D, const char* who) {
    SATRANS_REQUIRE(B > 0 && F >= 2 && D > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d F=%d D=%d", who, B, F, D);
    SATRANS_REQUIRE(F <= kFmF && D <= kFmD, SATRANS_E_UNSUPPORTED, "%s: F=%d fields, D=%d (at most %d, %d)", who, F, D, kFmF, kFmD);
    return SATRANS_OK;
}

int fm_validate(const satrans_fm_desc* d, const char* who) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    return fm_shape(d->B, d->F, d->D, who);
}

unsigned fm_grid(int B) { return (unsigned)ceil_div(B, kFmRows); }

// the shapes of an AFM call and its launches
struct Afm {
    int B, F, D, A, P, n, ppw, nwg, width;
};

int afm_validate(const satrans_afm_desc* d, const char* who, Afm& s) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    if (int rc = fm_shape(d->B, d->F, d->D, who)) return rc;
    SATRANS_REQUIRE(d->A > 0, SATRANS_E_BADARG, "%s: bad attention factor A=%d", who, d->A);
    SATRANS_REQUIRE(d->A <= kAfmA, SATRANS_E_UNSUPPORTED, "%s: attention factor A=%d (at most %d)", who, d->A, kAfmA);
    s.B = d->B, s.F = d->F, s.D = d->D, s.A = d->A;
    s.P = s.F * (s.F - 1) / 2;
    s.n = std::min({kAfmGroup, kAfmRow / (s.F * (s.D | 1)), kAfmPairs / s.P});
    const int64_t passes = ceil_div(s.B, s.n);
    s.ppw = (int)ceil_div(passes, kAfmWg);
    s.nwg = (int)ceil_div(passes, s.ppw);
    s.width = s.D * s.A + 2 * s.A + s.D;
    return SATRANS_OK;
}

// the two heads
struct FmHead {
    int B, F, D, kind, use_fm, dense, ld, n_dnn;
    bool has_dnn;
    Rows rows;
    Chain dnn;
    int64_t saved;
    int64_t w_dx, w_buf[2], w_part, total;
};

int fmhead_validate(const satrans_fmhead_desc* d, const char* who, FmHead& Y) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->kind == SATRANS_FMHEAD_DEEPFM || d->kind == SATRANS_FMHEAD_NFM, SATRANS_E_BADARG, "%s: kind=%d", who, d->kind);
    SATRANS_REQUIRE(d->dense_dim >= 0 && d->n_dnn >= 0, SATRANS_E_BADARG, "%s: bad sizes dense_dim=%d n_dnn=%d", who, d->dense_dim, d->n_dnn);
    SATRANS_REQUIRE(d->n_dnn <= kMaxH, SATRANS_E_UNSUPPORTED, "%s: %d hidden layers (at most %d)", who, d->n_dnn, kMaxH);
    for (int l = 0; l < d->n_dnn; ++l) SATRANS_REQUIRE(d->width[l] > 0, SATRANS_E_BADARG, "%s: width[%d]=%d", who, l, d->width[l]);
    if (int rc = fm_shape(d->B, d->F, d->D, who)) return rc;
    const bool nfm = d->kind == SATRANS_FMHEAD_NFM;
    SATRANS_REQUIRE(nfm ? d->n_dnn > 0 : (d->n_dnn > 0 || d->use_fm), SATRANS_E_BADARG,
                    "%s: %s", who, nfm ? "NFM needs hidden layers" : "neither the FM term nor a DNN");
    Y.B = d->B, Y.F = d->F, Y.D = d->D, Y.kind = d->kind, Y.use_fm = !nfm && d->use_fm, Y.dense = d->dense_dim, Y.n_dnn = d->n_dnn;
    Y.has_dnn = d->n_dnn > 0;
    const int64_t ld = (nfm ? (int64_t)d->D : (int64_t)d->F * d->D) + d->dense_dim;
    SATRANS_REQUIRE(ld <= 0x7fffffffLL, SATRANS_E_UNSUPPORTED, "%s: %lld DNN input columns", who, (long long)ld);
    Y.ld = (int)ld;
    Y.saved = Y.total = 0;
    if (!Y.has_dnn) return SATRANS_OK;
    Y.rows = rows_of(d->B, 0, nullptr, nullptr);
    // (out.bias is the final layer's bias)
    chain_dnn(Y.dnn, false, d->n_dnn, d->width, Y.ld, 1, d->dnn_w, d->dnn_b, d->dnn_linear_w, d->out_bias);
    int64_t part = 0;
    if (int rc = chain_fits(Y.rows, Y.dnn, who, "dnn", part)) return rc;
    const int64_t B = d->B;
    int64_t at = B * ld, wide = 1;
    for (int l = 0; l < d->n_dnn; ++l) {
        Y.dnn.s[l] = at;
        at += B * d->width[l];
        wide = std::max<int64_t>(wide, d->width[l]);
    }
    Y.saved = at;
    Y.w_dx = 0, Y.w_buf[0] = B * ld, Y.w_buf[1] = Y.w_buf[0] + B * wide, Y.w_part = Y.w_buf[1] + B * wide;
    Y.total = Y.w_part + part;
    return SATRANS_OK;
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int satrans_fm_fwd(const satrans_fm_desc* d, float* out, void* stream_) {
    if (int rc = fm_validate(d, "fm_fwd")) return rc;
    SATRANS_REQUIRE(d->e && out, SATRANS_E_BADARG, "fm_fwd: null pointer");
    fm_rows_fwd_kernel<<<fm_grid(d->B), kThreads, 0, (hipStream_t)stream_>>>(d->e, d->B, d->F, d->D, 0, 0, 1, nullptr, 0, nullptr, nullptr,
                                                                            nullptr, 0, out);
    SATRANS_CHECK_LAUNCH("fm_rows_fwd_kernel");
    return SATRANS_OK;
}

extern "C" int satrans_fm_bwd(const satrans_fm_desc* d, const float* dout, float* de, void* stream_) {
    if (int rc = fm_validate(d, "fm_bwd")) return rc;
    SATRANS_REQUIRE(d->e && dout && de, SATRANS_E_BADARG, "fm_bwd: null pointer");
    fm_rows_bwd_kernel<<<fm_grid(d->B), kThreads, 0, (hipStream_t)stream_>>>(d->e, d->B, d->F, d->D, nullptr, 0, 0, 0, dout, de, nullptr, 0);
    SATRANS_CHECK_LAUNCH("fm_rows_bwd_kernel");
    return SATRANS_OK;
}

extern "C" int satrans_bipool_fwd(const satrans_fm_desc* d, float* out, void* stream_) {
    if (int rc = fm_validate(d, "bipool_fwd")) return rc;
    SATRANS_REQUIRE(d->e && out, SATRANS_E_BADARG, "bipool_fwd: null pointer");
    fm_rows_fwd_kernel<<<fm_grid(d->B), kThreads, 0, (hipStream_t)stream_>>>(d->e, d->B, d->F, d->D, 0, 1, 0, nullptr, 0, nullptr, nullptr, out,
                                                                            d->D, nullptr);
    SATRANS_CHECK_LAUNCH("fm_rows_fwd_kernel");
    return SATRANS_OK;
}

extern "C" int satrans_bipool_bwd(const satrans_fm_desc* d, const float* dout, float* de, void* stream_) {
    if (int rc = fm_validate(d, "bipool_bwd")) return rc;
    SATRANS_REQUIRE(d->e && dout && de, SATRANS_E_BADARG, "bipool_bwd: null pointer");
    fm_rows_bwd_kernel<<<fm_grid(d->B), kThreads, 0, (hipStream_t)stream_>>>(d->e, d->B, d->F, d->D, dout, d->D, 0, 1, nullptr, de, nullptr, 0);
    SATRANS_CHECK_LAUNCH("fm_rows_bwd_kernel");
    return SATRANS_OK;
}

extern "C" int64_t satrans_afm_saved_floats(const satrans_afm_desc* d) {
    Afm s;
    const int rc = afm_validate(d, "afm_saved_floats", s);
    return rc ? rc : (int64_t)s.B * (s.P + s.D);
}

extern "C" int64_t satrans_afm_workspace_floats(const satrans_afm_desc* d) {
    Afm s;
    const int rc = afm_validate(d, "afm_workspace_floats", s);
    return rc ? rc : (int64_t)s.nwg * s.width;
}

extern "C" int satrans_afm_fwd(const satrans_afm_desc* d, float* out, float* saved, void* stream_) {
    Afm s;
    if (int rc = afm_validate(d, "afm_fwd", s)) return rc;
    SATRANS_REQUIRE(d->e && d->attention_W && d->attention_b && d->projection_h && d->projection_p && out && saved, SATRANS_E_BADARG,
                    "afm_fwd: null pointer");
    afm_fwd_kernel<<<(unsigned)s.nwg, kThreads, 0, (hipStream_t)stream_>>>(d->e, d->attention_W, d->attention_b, d->projection_h,
                                                                          d->projection_p, d->linear_logit, d->out_bias, s.B, s.F, s.D, s.A,
                                                                          s.P, s.n, s.ppw, out, saved, saved + (size_t)s.B * s.P);
    SATRANS_CHECK_LAUNCH("afm_fwd_kernel");
    return SATRANS_OK;
}

extern "C" int satrans_afm_bwd(const satrans_afm_desc* d, const float* dout, float* de, const float* saved, float* workspace,
                               const satrans_afm_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    Afm s;
    if (int rc = afm_validate(d, "afm_bwd", s)) return rc;
    SATRANS_REQUIRE(d->e && d->attention_W && d->attention_b && d->projection_h && d->projection_p && dout && de && saved && workspace &&
                        g && g->attention_W && g->attention_b && g->projection_h && g->projection_p && (g->out_bias || !d->out_bias),
                    SATRANS_E_BADARG, "afm_bwd: null pointer");
    afm_bwd_kernel<<<(unsigned)s.nwg, kThreads, 0, st>>>(d->e, d->attention_W, d->attention_b, d->projection_h, d->projection_p, dout, saved,
                                                        saved + (size_t)s.B * s.P, s.B, s.F, s.D, s.A, s.P, s.n, s.ppw, de, workspace);
    SATRANS_CHECK_LAUNCH("afm_bwd_kernel");
    const unsigned blocks = (unsigned)ceil_div(s.width, kThreads / kReduceGroups) + (g->out_bias ? 1 : 0);
    afm_reduce_kernel<<<blocks, kThreads, 0, st>>>(workspace, s.nwg, s.width, s.D * s.A, s.A, g->attention_W, g->attention_b,
                                                  g->projection_h, g->projection_p, dout, s.B, g->out_bias);
    SATRANS_CHECK_LAUNCH("afm_reduce_kernel");
    return SATRANS_OK;
}

extern "C" int64_t satrans_fmhead_saved_floats(const satrans_fmhead_desc* d) {
    FmHead Y;
    const int rc = fmhead_validate(d, "fmhead_saved_floats", Y);
    return rc ? rc : Y.saved;
}

extern "C" int64_t satrans_fmhead_workspace_floats(const satrans_fmhead_desc* d) {
    FmHead Y;
    const int rc = fmhead_validate(d, "fmhead_workspace_floats", Y);
    return rc ? rc : Y.total;
}

extern "C" int satrans_fmhead_fwd(const satrans_fmhead_desc* d, float* logit, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    FmHead Y;
    if (int rc = fmhead_validate(d, "fmhead_fwd", Y)) return rc;
    SATRANS_REQUIRE(d->emb && (d->dense || !Y.dense || !Y.has_dnn) && d->out_bias && logit && (saved || !Y.has_dnn) &&
                        (!Y.has_dnn || chain_has(Y.dnn, d->dnn_w, d->dnn_b, d->dnn_linear_w, false)),
                    SATRANS_E_BADARG, "fmhead_fwd: null pointer");
    const bool nfm = Y.kind == SATRANS_FMHEAD_NFM;
    // the FM term and linear_logit go straight into the logit (without a DNN: out.bias too, which is the DNN's final bias
    // otherwise); the pooled row, flatten(e) and the dense columns straight into the DNN input
    fm_rows_fwd_kernel<<<fm_grid(Y.B), kThreads, 0, st>>>(d->emb, Y.B, Y.F, Y.D, Y.has_dnn && !nfm, nfm, Y.use_fm, d->dense,
                                                         Y.has_dnn ? Y.dense : 0, d->linear_logit, Y.has_dnn ? nullptr : d->out_bias,
                                                         Y.has_dnn ? saved : nullptr, Y.ld, logit);
    SATRANS_CHECK_LAUNCH("fm_rows_fwd_kernel");
    if (!Y.has_dnn) return SATRANS_OK;
    return dnn_fwd<false>(Y.rows, Y.dnn, saved, saved, logit, st, 1);
}

extern "C" int satrans_fmhead_bwd(const satrans_fmhead_desc* d, const float* dlogit, float* demb, float* ddense, const float* saved,
                                  float* workspace, const satrans_fmhead_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    FmHead Y;
    if (int rc = fmhead_validate(d, "fmhead_bwd", Y)) return rc;
    SATRANS_REQUIRE(d->emb && d->out_bias && dlogit && demb && g && g->out_bias, SATRANS_E_BADARG, "fmhead_bwd: null pointer");
    if (!Y.has_dnn) {
        fm_sum_kernel<<<1, kThreads, 0, st>>>(dlogit, Y.B, g->out_bias);
        SATRANS_CHECK_LAUNCH("fm_sum_kernel");
        fm_rows_bwd_kernel<<<fm_grid(Y.B), kThreads, 0, st>>>(d->emb, Y.B, Y.F, Y.D, nullptr, 0, 0, 0, dlogit, demb, nullptr, 0);
        SATRANS_CHECK_LAUNCH("fm_rows_bwd_kernel");
        return SATRANS_OK;
    }
    SATRANS_REQUIRE((ddense || !Y.dense) && saved && workspace && chain_has(Y.dnn, d->dnn_w, d->dnn_b, d->dnn_linear_w, false) &&
                        chain_has(Y.dnn, g->dnn_w, g->dnn_b, g->dnn_linear_w, false),
                    SATRANS_E_BADARG, "fmhead_bwd: null pointer");
    set_grads(Y.dnn, g->dnn_w, g->dnn_b, g->dnn_linear_w, g->out_bias, false);
    float* dx = workspace + Y.w_dx;
    float* buf[2] = {workspace + Y.w_buf[0], workspace + Y.w_buf[1]};
    int cur = 0;
    if (int rc = dnn_bwd<false>(Y.rows, Y.dnn, dlogit, saved, saved, 0, dx, buf, cur, workspace + Y.w_part, st)) return rc;
    const bool nfm = Y.kind == SATRANS_FMHEAD_NFM;
    fm_rows_bwd_kernel<<<fm_grid(Y.B), kThreads, 0, st>>>(d->emb, Y.B, Y.F, Y.D, dx, Y.ld, !nfm, nfm, Y.use_fm ? dlogit : nullptr, demb, ddense,
                                                         Y.dense);
    SATRANS_CHECK_LAUNCH("fm_rows_bwd_kernel");
    return SATRANS_OK;
}
