// deepctr-torch 0.2.9's InteractingLayer, which the reference's models/autoint.py builds (autoint.py:13,75-76), and the half of
// AutoInt.forward behind the lookup (autoint.py:93-121).  x [B, F, D], H heads of dh = D / H columns:
//     [q | k | v | r] = x [W_Query | W_key | W_Value | W_Res]         s_ij = q_i . k_j (/ sqrt(dh) with scaling), per (sample, head)
//     p = softmax_j(s)      o_i = sum_j p_ij v_j                      y = relu(o + r)            (no r without use_res)
//     dt = dy [y > 0]       dp_ij = dt_i . v_j    delta_i = sum_j p_ij dp_ij    ds_ij = p_ij (dp_ij - delta_i) (/ sqrt(dh))
//     dq_i = sum_j ds_ij k_j      dk_j = sum_i ds_ij q_i      dv_j = sum_i p_ij dt_i
//     dx = [dq | dk | dv | dt] [W_Query | W_key | W_Value | W_Res]^T      dW = x^T [dq | dk | dv | dt]
//
// int_fwd_kernel     a workgroup owns whole samples, `n` of them a pass (the host picks n from F and D: the backward's LDS
//                    budget): their rows once into LDS (odd stride), the one product x [Wq | Wk | Wv | Wr] on the f32 MFMA (32 x 32
//                    tiles, the weight fragments straight from global memory: 16 KB at D = 32, cache resident) into LDS; a thread
//                    per (sample, head, query) runs the scores, the softmax and the sum over v in registers (two walks over the
//                    keys: the row maximum, then exp, the row sum and o), leaves o where its q stood and writes the row's
//                    (max, sum): the only thing saved; y = relu(o + r) written once, coalesced.  With `att`: the normalised
//                    scores [H, B, F, F].
// int_bwd_kernel     the same ownership.  x, dt = dy [y > 0] and the statistics staged; q, k, v again by the same product; a
//                    thread per (sample, head, query) forms delta_i and dq_i, then a thread per (sample, head, key) dk_j and
//                    dv_j, p regenerated from the saved (max, sum) both times; dx = G W^T on the MFMA straight from LDS into
//                    global memory (plus the head's DNN-input gradient on the first layer), written once; x^T G accumulated in
//                    MFMA accumulators over all the workgroup's passes and left as one [blocks, D, D] partial per workgroup.
// int_reduce_kernel  the workgroups' partials in a fixed order (fp64: kReduceGroups contiguous shares, then the shares).
// The head's DNN and dnn_linear run on head_layers.h's dense launcher.
// No atomics; every sum has a fixed order; a sample's results do not depend on its place in a pass (an MFMA result element is
// a k-ordered fmaf chain whatever its tile).  fp32 only.
#include "head_layers.h"

namespace satrans {
namespace {

constexpr int kIntWg = SATRANS_INTERACTING_MAX_WORKGROUPS;
constexpr int kIntLayers = SATRANS_AUTOINT_MAX_LAYERS;
constexpr int kIntGroup = 16;                 // samples of a pass at most
constexpr int kIntRows = 128;                 // rows of a pass at most (one sample always fits: F <= 64)
constexpr int kIntLds = 80 * 1024;            // the backward's LDS a workgroup aims at: two workgroups a CU
constexpr int kIntLdsMax = 160 * 1024;        // what a CU has
constexpr int kIntMaxF = 64;

__device__ __forceinline__ const float* int_block(int blk, const float* wq, const float* wk, const float* wv, const float* wr) {
    return blk == 0 ? wq : blk == 1 ? wk : blk == 2 ? wv : wr;
}

__device__ __forceinline__ f32x16 int_zero() {
    f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    return z;
}

// a (registers) . b (LDS, 16-byte aligned): four chains, d = c, c + 4, .. each, then (0 + 1) + (2 + 3)
template <int DH>
__device__ __forceinline__ float int_dot(const float* a, const float* b) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        const float4 v = *reinterpret_cast<const float4*>(b + d);
        acc[0] = fmaf(a[d], v.x, acc[0]);
        acc[1] = fmaf(a[d + 1], v.y, acc[1]);
        acc[2] = fmaf(a[d + 2], v.z, acc[2]);
        acc[3] = fmaf(a[d + 3], v.w, acc[3]);
    }
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// dst[d] = fmaf(c, src[d], dst[d]) over a row of LDS (16-byte aligned)
template <int DH>
__device__ __forceinline__ void int_axpy(float c, const float* src, float* dst) {
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        const float4 v = *reinterpret_cast<const float4*>(src + d);
        dst[d] = fmaf(c, v.x, dst[d]);
        dst[d + 1] = fmaf(c, v.y, dst[d + 1]);
        dst[d + 2] = fmaf(c, v.z, dst[d + 2]);
        dst[d + 3] = fmaf(c, v.w, dst[d + 3]);
    }
}

// sq[row, c] = sum_k sx[row, k] W_(c / D)[k, c % D] for row < M, c < NC: (row tile, column tile) pairs in column-major order, a
// wave a contiguous share of them, so that it keeps a column tile's weight fragments in registers over its row tiles
template <int D>
__device__ __forceinline__ void int_project(const float* sx, int Mp, int M, const float* __restrict__ wq, const float* __restrict__ wk,
                                            const float* __restrict__ wv, const float* __restrict__ wr, int NC, float* sq, int ldq) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int mt = Mp >> 5, nt = (NC + 31) >> 5, P = mt * nt;
    const int p0 = wave * P / 4, p1 = (wave + 1) * P / 4;
    int have = -1;
    float bf[D / 2];
    for (int p = p0; p < p1; ++p) {
        const int ct = p / mt, rt = p - ct * mt, c = ct * 32 + r;
        if (ct != have) {
            have = ct;
            const float* w = c < NC ? int_block(c / D, wq, wk, wv, wr) + c % D : nullptr;
#pragma unroll
            for (int i = 0; i < D / 2; ++i) bf[i] = w ? w[(2 * i + h) * D] : 0.f;
        }
        f32x16 acc = int_zero();
        const float* a = sx + (rt * 32 + r) * (D + 1) + h;
#pragma unroll
        for (int i = 0; i < D / 2; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * i], bf[i], acc, 0, 0, 0);
        if (c < NC) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = rt * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (row < M) sq[row * ldq + c] = acc[q];
            }
        }
    }
}

// grid: workgroups; workgroup w owns the passes [w ppw, (w + 1) ppw) of n samples each.  LDS: sx [Mp][D + 1], sq [n F][4 D + 4]
template <int D, int DH>
__global__ __launch_bounds__(kThreads) void int_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wq,
                                                           const float* __restrict__ wk, const float* __restrict__ wv,
                                                           const float* __restrict__ wr, int B, int F, int n, int ppw, float scale,
                                                           float* __restrict__ y, float* __restrict__ stats, float* __restrict__ att) {
    extern __shared__ __align__(16) float int_lds[];
    constexpr int H = D / DH, ldx = D + 1, ldq = 4 * D + 4;      // (rows of sq 16-byte aligned: the attention reads float4)
    const int NC = wr ? 4 * D : 3 * D;
    const int Mp = (n * F + 31) & ~31;
    float* sx = int_lds;
    float* sq = sx + Mp * ldx;
    const int t = threadIdx.x;
    const int64_t passes = ((int64_t)B + n - 1) / n;
    const int64_t pass0 = (int64_t)blockIdx.x * ppw, pass1 = pass0 + ppw < passes ? pass0 + ppw : passes;
    for (int64_t pass = pass0; pass < pass1; ++pass) {
        const int64_t b0 = pass * n;
        const int m = b0 + n <= B ? n : (int)(B - b0), M = m * F;
        const float* xs = x + (size_t)b0 * F * D;
        for (int idx = t; idx < Mp * D; idx += kThreads) {      // (the previous pass's product has read sx: the sync before its attention)
            const int row = idx / D, d = idx - row * D;
            sx[row * ldx + d] = row < M ? xs[idx] : 0.f;
        }
        __syncthreads();      // and the previous pass's epilogue has read sq
        int_project<D>(sx, Mp, M, wq, wk, wv, wr, NC, sq, ldq);
        __syncthreads();
        for (int it = t; it < m * H * F; it += kThreads) {
            const int i = it % F, sh = it / F, hd = sh % H, s = sh / H;
            float* qi = sq + (s * F + i) * ldq + hd * DH;
            const float* kb = sq + s * F * ldq + D + hd * DH;
            const float* vb = kb + D;
            float q[DH], o[DH];
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                q[d] = qi[d];
                o[d] = 0.f;
            }
            float mx = -INFINITY, sum = 0.f;
            for (int j = 0; j < F; ++j) mx = fmaxf(mx, int_dot<DH>(q, kb + j * ldq) * scale);
            for (int j = 0; j < F; ++j) {
                const float e = expf(int_dot<DH>(q, kb + j * ldq) * scale - mx);
                sum += e;
                int_axpy<DH>(e, vb + j * ldq, o);
            }
#pragma unroll
            for (int d = 0; d < DH; ++d) qi[d] = o[d] / sum;      // (this thread alone reads q_i)
            float* st = stats + ((size_t)b0 * H * F + it) * 2;
            st[0] = mx;
            st[1] = sum;
            if (att) {
                float* ar = att + (((size_t)hd * B + b0 + s) * F + i) * F;
                for (int j = 0; j < F; ++j) ar[j] = expf(int_dot<DH>(q, kb + j * ldq) * scale - mx) / sum;
            }
        }
        __syncthreads();
        float* ys = y + (size_t)b0 * F * D;
        for (int idx = t; idx < M * D; idx += kThreads) {
            const int row = idx / D, d = idx - row * D;
            const float v = sq[row * ldq + d] + (wr ? sq[row * ldq + 3 * D + d] : 0.f);
            ys[idx] = fmaxf(v, 0.f);
        }
    }
}

// grid: as the forward's.  LDS: sx [Mp][D + 1], sg [Mp][4 D + 4] = [dq | dk | dv | dt], sq [n F][3 D + 4] = [q | k | v],
// the rows' (max, sum) [n H F][2], delta [n H F].  part: per workgroup [blocks][D][D].  dx_add (or null): rows of ld_add floats,
// whose first F D columns are added to dx.
template <int D, int DH>
__global__ __launch_bounds__(kThreads) void int_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ dy, const float* __restrict__ wq,
                                                           const float* __restrict__ wk, const float* __restrict__ wv,
                                                           const float* __restrict__ wr, const float* __restrict__ stats, int B, int F,
                                                           int n, int ppw, float scale, const float* __restrict__ dx_add, int ld_add,
                                                           float* __restrict__ dx, float* __restrict__ part) {
    extern __shared__ __align__(16) float int_lds[];
    constexpr int H = D / DH, ldx = D + 1, ldq = 3 * D + 4, ldg = 4 * D + 4;      // (rows of sq and sg 16-byte aligned)
    constexpr int kDt = (D + 31) / 32;                            // tiles of 32 over D
    constexpr int kSlots = (kDt * ((4 * D + 31) / 32) + 3) / 4;   // tiles of x^T G a wave holds at most
    const int nblk = wr ? 4 : 3, NC = nblk * D, nt = (NC + 31) >> 5;
    const int Mp = (n * F + 31) & ~31;
    float* sx = int_lds;
    float* sg = sx + Mp * ldx;
    float* sq = sg + Mp * ldg;
    float* sst = sq + n * F * ldq;
    float* sdl = sst + 2 * n * H * F;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    f32x16 accw[kSlots];
#pragma unroll
    for (int u = 0; u < kSlots; ++u) accw[u] = int_zero();
    const int64_t passes = ((int64_t)B + n - 1) / n;
    const int64_t pass0 = (int64_t)blockIdx.x * ppw, pass1 = pass0 + ppw < passes ? pass0 + ppw : passes;
    for (int64_t pass = pass0; pass < pass1; ++pass) {
        const int64_t b0 = pass * n;
        const int m = b0 + n <= B ? n : (int)(B - b0), M = m * F, items = m * H * F;
        const size_t g0 = (size_t)b0 * F * D;
        __syncthreads();      // the previous pass's products have read sx and sg
        for (int idx = t; idx < Mp * D; idx += kThreads) {
            const int row = idx / D, d = idx - row * D;
            const bool live = row < M;
            sx[row * ldx + d] = live ? x[g0 + idx] : 0.f;
            sg[row * ldg + 3 * D + d] = live && y[g0 + idx] > 0.f ? dy[g0 + idx] : 0.f;
            if (!live) sg[row * ldg + d] = sg[row * ldg + D + d] = sg[row * ldg + 2 * D + d] = 0.f;      // (the rows beyond M of x^T G)
        }
        for (int it = t; it < 2 * items; it += kThreads) sst[it] = stats[(size_t)b0 * H * F * 2 + it];
        __syncthreads();
        int_project<D>(sx, Mp, M, wq, wk, wv, nullptr, 3 * D, sq, ldq);
        __syncthreads();
        // a thread per query: delta_i, dq_i
        for (int it = t; it < items; it += kThreads) {
            const int i = it % F, sh = it / F, hd = sh % H, s = sh / H, row = s * F + i;
            const float* kb = sq + s * F * ldq + D + hd * DH;
            const float* vb = kb + D;
            float q[DH], g[DH], dq[DH];
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                q[d] = sq[row * ldq + hd * DH + d];
                g[d] = sg[row * ldg + 3 * D + hd * DH + d];
                dq[d] = 0.f;
            }
            const float mx = sst[2 * it], sum = sst[2 * it + 1];
            float delta = 0.f;
            for (int j = 0; j < F; ++j) {
                const float p = expf(int_dot<DH>(q, kb + j * ldq) * scale - mx) / sum;
                delta = fmaf(p, int_dot<DH>(g, vb + j * ldq), delta);
            }
            for (int j = 0; j < F; ++j) {
                const float* k = kb + j * ldq;
                const float p = expf(int_dot<DH>(q, k) * scale - mx) / sum;
                const float ds = p * (int_dot<DH>(g, vb + j * ldq) - delta) * scale;
                int_axpy<DH>(ds, k, dq);
            }
            sdl[it] = delta;
#pragma unroll
            for (int d = 0; d < DH; ++d) sg[row * ldg + hd * DH + d] = dq[d];
        }
        __syncthreads();
        // a thread per key: dk_j, dv_j
        for (int it = t; it < items; it += kThreads) {
            const int j = it % F, sh = it / F, hd = sh % H, s = sh / H, row = s * F + j;
            float k[DH], v[DH], dk[DH], dv[DH];
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                k[d] = sq[row * ldq + D + hd * DH + d];
                v[d] = sq[row * ldq + 2 * D + hd * DH + d];
                dk[d] = dv[d] = 0.f;
            }
            for (int i = 0; i < F; ++i) {
                const float* qi = sq + (s * F + i) * ldq + hd * DH;
                const float* gi = sg + (s * F + i) * ldg + 3 * D + hd * DH;
                const int at = sh * F + i;
                const float p = expf(int_dot<DH>(k, qi) * scale - sst[2 * at]) / sst[2 * at + 1];
                const float ds = p * (int_dot<DH>(v, gi) - sdl[at]) * scale;
                int_axpy<DH>(ds, qi, dk);
                int_axpy<DH>(p, gi, dv);
            }
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                sg[row * ldg + D + hd * DH + d] = dk[d];
                sg[row * ldg + 2 * D + hd * DH + d] = dv[d];
            }
        }
        __syncthreads();
        // dx[row, d] = sum_c G[row, c] W_(c / D)[d, c % D], blocks in order
        const int mtl = (M + 31) >> 5;
        for (int p = wave; p < mtl * kDt; p += 4) {
            const int rt = p / kDt, ct = p - rt * kDt, dc = ct * 32 + r;
            f32x16 acc = int_zero();
            const float* a = sg + (rt * 32 + r) * ldg + h;
            for (int blk = 0; blk < nblk; ++blk) {
                const float* w = dc < D ? int_block(blk, wq, wk, wv, wr) + dc * D + h : nullptr;
                float bf[D / 2];
#pragma unroll
                for (int i = 0; i < D / 2; ++i) bf[i] = w ? w[2 * i] : 0.f;
#pragma unroll
                for (int i = 0; i < D / 2; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[blk * D + 2 * i], bf[i], acc, 0, 0, 0);
            }
            if (dc < D) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = rt * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                    if (row >= M) continue;
                    float v = acc[q];
                    if (dx_add) {
                        const int s = row / F;
                        v += dx_add[(size_t)(b0 + s) * ld_add + (row - s * F) * D + dc];
                    }
                    dx[g0 + (size_t)row * D + dc] = v;
                }
            }
        }
        // (x^T G)[d, c] += sum over the pass's rows (those beyond M hold zeros)
        const int Me = (M + 1) & ~1;
#pragma unroll
        for (int u = 0; u < kSlots; ++u) {
            const int tile = wave + 4 * u;
            if (tile < kDt * nt) {
                const int dt = tile % kDt, ct = tile / kDt, di = dt * 32 + r, c = ct * 32 + r;
                const float* a = sx + h * ldx + (di < D ? di : 0);
                const float* b = sg + h * ldg + c;
                const bool on = di < D;
                for (int kk = 0; kk < Me; kk += 2)
                    accw[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(on ? a[kk * ldx] : 0.f, b[kk * ldg], accw[u], 0, 0, 0);
            }
        }
    }
    float* mine = part + (size_t)blockIdx.x * nblk * D * D;
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
        const int tile = wave + 4 * u;
        if (tile < kDt * nt) {
            const int dt = tile % kDt, ct = tile / kDt, c = ct * 32 + r;
            if (c < NC) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int di = dt * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                    if (di < D) mine[((c / D) * D + di) * D + c % D] = accw[u][q];
                }
            }
        }
    }
}

// grid: ceil(width / 16).  The workgroups' partials [nwg][width] -> out [width]: a workgroup is 16 elements x kReduceGroups
// groups, every group adds its contiguous share of the partials in index order (fp64), the group sums are combined in group
// order.  (grouped_gemm.h's mmoe_reduce_kernel fits in form - a thread per element walks all the partials - and took 108 us for
// 512 partials of 4096 floats: its callers have a few chunks, not hundreds.)
__global__ __launch_bounds__(kThreads) void int_reduce_kernel(const float* __restrict__ part, int nwg, int width, float* __restrict__ out) {
    __shared__ double sh[kThreads];
    constexpr int kEls = kThreads / kReduceGroups;
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
    out[el] = (float)sum;
}

// x[row] = [emb[row] (FD) | dense[row] (dense_dim)], rows of ld floats
__global__ __launch_bounds__(kThreads) void autoint_concat_kernel(const float* __restrict__ emb, const float* __restrict__ dense, int64_t B,
                                                                  int FD, int dense_dim, float* __restrict__ x) {
    const int ld = FD + dense_dim;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= B * ld) return;
    const int64_t row = idx / ld;
    const int c = (int)(idx - row * ld);
    x[idx] = c < FD ? emb[row * FD + c] : dense[row * dense_dim + c - FD];
}

// ddense[row] = dx[row, FD : FD + dense_dim]
__global__ __launch_bounds__(kThreads) void autoint_dense_grad_kernel(const float* __restrict__ dx, int64_t B, int FD, int dense_dim,
                                                                      float* __restrict__ ddense) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= B * dense_dim) return;
    const int64_t row = idx / dense_dim;
    ddense[idx] = dx[row * (FD + dense_dim) + FD + (idx - row * dense_dim)];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

// the shapes of a layer call and its launches
struct IntPlan {
    int B, F, D, H, dh, nblk, n, ppw, nwg;
    float scale;
    size_t lds_fwd, lds_bwd;
};

size_t int_lds_bwd(int n, int F, int D, int H) {
    const size_t M = (size_t)n * F, Mp = (M + 31) & ~(size_t)31;
    return sizeof(float) * (Mp * (D + 1) + Mp * (4 * D + 4) + M * (3 * D + 4) + 3 * M * H);
}

int int_plan(int B, int F, int D, int H, uint32_t flags, const char* who, IntPlan& p) {
    SATRANS_REQUIRE(B > 0 && F > 0 && D > 0 && H > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d F=%d D=%d H=%d", who, B, F, D, H);
    SATRANS_REQUIRE(!(flags & ~(uint32_t)(SATRANS_NO_RES | SATRANS_NO_SCALING)), SATRANS_E_BADARG, "%s: unknown flags %u", who, flags);
    const int dh = D % H ? 0 : D / H;
    SATRANS_REQUIRE((D == 16 || D == 32 || D == 64) && (dh == 8 || dh == 16 || dh == 32) && F >= 2 && F <= kIntMaxF,
                    SATRANS_E_UNSUPPORTED, "%s: D=%d in {16, 32, 64}, D / H=%d in {8, 16, 32}, F=%d in [2, %d]", who, D, dh, F, kIntMaxF);
    p.B = B, p.F = F, p.D = D, p.H = H, p.dh = dh, p.nblk = flags & SATRANS_NO_RES ? 3 : 4;
    p.scale = flags & SATRANS_NO_SCALING ? 1.f : 1.f / sqrtf((float)dh);
    int n = 1;
    while (n < kIntGroup && (n + 1) * F <= kIntRows && int_lds_bwd(n + 1, F, D, H) <= (size_t)kIntLds) ++n;
    p.n = n;
    const size_t M = (size_t)n * F, Mp = (M + 31) & ~(size_t)31;
    p.lds_fwd = sizeof(float) * (Mp * (D + 1) + M * (4 * D + 4));
    p.lds_bwd = int_lds_bwd(n, F, D, H);
    SATRANS_REQUIRE(p.lds_bwd <= (size_t)kIntLdsMax, SATRANS_E_UNSUPPORTED, "%s: F=%d D=%d H=%d needs %zu bytes of LDS", who, F, D, H,
                    p.lds_bwd);
    const int64_t passes = ceil_div(B, n);
    p.ppw = (int)ceil_div(passes, kIntWg);
    p.nwg = (int)ceil_div(passes, p.ppw);
    return SATRANS_OK;
}

#define INT_DISPATCH(P, CALL)                                  \
    do {                                                       \
        if ((P).D == 16 && (P).dh == 8) CALL(16, 8);           \
        else if ((P).D == 16 && (P).dh == 16) CALL(16, 16);    \
        else if ((P).D == 32 && (P).dh == 8) CALL(32, 8);      \
        else if ((P).D == 32 && (P).dh == 16) CALL(32, 16);    \
        else if ((P).D == 32 && (P).dh == 32) CALL(32, 32);    \
        else if ((P).D == 64 && (P).dh == 8) CALL(64, 8);      \
        else if ((P).D == 64 && (P).dh == 16) CALL(64, 16);    \
        else CALL(64, 32);                                     \
    } while (0)

int int_launch_fwd(const IntPlan& p, const float* x, const float* wq, const float* wk, const float* wv, const float* wr, float* y,
                   float* stats, float* att, hipStream_t st) {
#define INT_FWD(D_, DH_)                                                                                                           \
    do {                                                                                                                           \
        hipError_t e = hipFuncSetAttribute((const void*)int_fwd_kernel<D_, DH_>, hipFuncAttributeMaxDynamicSharedMemorySize,       \
                                           (int)p.lds_fwd);                                                                        \
        SATRANS_REQUIRE(e == hipSuccess, SATRANS_E_LAUNCH, "interacting_fwd: LDS attribute: %s", hipGetErrorString(e));            \
        int_fwd_kernel<D_, DH_><<<(unsigned)p.nwg, kThreads, p.lds_fwd, st>>>(x, wq, wk, wv, wr, p.B, p.F, p.n, p.ppw, p.scale, y, \
                                                                              stats, att);                                         \
    } while (0)
    INT_DISPATCH(p, INT_FWD);
#undef INT_FWD
    SATRANS_CHECK_LAUNCH("int_fwd_kernel");
    return SATRANS_OK;
}

// one layer's backward: dx written (plus dx_add's embedding block), its weight gradients [blocks, D, D] into g_w
int int_launch_bwd(const IntPlan& p, const float* x, const float* y, const float* dy, const float* wq, const float* wk, const float* wv,
                   const float* wr, const float* stats, const float* dx_add, int ld_add, float* dx, float* part, float* g_w,
                   hipStream_t st) {
#define INT_BWD(D_, DH_)                                                                                                              \
    do {                                                                                                                              \
        hipError_t e = hipFuncSetAttribute((const void*)int_bwd_kernel<D_, DH_>, hipFuncAttributeMaxDynamicSharedMemorySize,          \
                                           (int)p.lds_bwd);                                                                           \
        SATRANS_REQUIRE(e == hipSuccess, SATRANS_E_LAUNCH, "interacting_bwd: LDS attribute: %s", hipGetErrorString(e));               \
        int_bwd_kernel<D_, DH_><<<(unsigned)p.nwg, kThreads, p.lds_bwd, st>>>(x, y, dy, wq, wk, wv, wr, stats, p.B, p.F, p.n, p.ppw,  \
                                                                              p.scale, dx_add, ld_add, dx, part);                     \
    } while (0)
    INT_DISPATCH(p, INT_BWD);
#undef INT_BWD
    SATRANS_CHECK_LAUNCH("int_bwd_kernel");
    const int width = p.nblk * p.D * p.D;
    int_reduce_kernel<<<(unsigned)ceil_div(width, kThreads / kReduceGroups), kThreads, 0, st>>>(part, p.nwg, width, g_w);
    SATRANS_CHECK_LAUNCH("int_reduce_kernel");
    return SATRANS_OK;
}

int64_t int_stats(const IntPlan& p) { return 2 * (int64_t)p.B * p.H * p.F; }
int64_t int_part(const IntPlan& p) { return (int64_t)p.nwg * p.nblk * p.D * p.D; }

int int_validate(const satrans_interacting_desc* d, const char* who, IntPlan& p) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    return int_plan(d->B, d->F, d->D, d->H, d->flags, who, p);
}

// the head
struct AutoInt {
    IntPlan p;
    int L, dense, ld, FD, n_dnn;
    bool has_dnn;
    Rows rows;
    Lyr att;          // dnn_linear's columns over att_output, with out.bias
    Chain dnn;        // the DNN and dnn_linear's columns over deep_out
    int64_t s_y, s_stats, s_in, saved;
    int64_t w_g[2], w_dx, w_buf[2], w_part, total;
};

int autoint_validate(const satrans_autoint_desc* d, const char* who, AutoInt& Y) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->n_layers >= 1 && d->dense_dim >= 0 && d->n_dnn >= 0, SATRANS_E_BADARG,
                    "%s: bad sizes n_layers=%d dense_dim=%d n_dnn=%d", who, d->n_layers, d->dense_dim, d->n_dnn);
    SATRANS_REQUIRE(d->n_layers <= kIntLayers && d->n_dnn <= kMaxH, SATRANS_E_UNSUPPORTED,
                    "%s: %d interacting layers (at most %d), %d hidden layers (at most %d)", who, d->n_layers, kIntLayers, d->n_dnn, kMaxH);
    for (int l = 0; l < d->n_dnn; ++l) SATRANS_REQUIRE(d->width[l] > 0, SATRANS_E_BADARG, "%s: width[%d]=%d", who, l, d->width[l]);
    if (int rc = int_plan(d->B, d->F, d->D, d->H, d->flags, who, Y.p)) return rc;
    Y.L = d->n_layers, Y.dense = d->dense_dim, Y.n_dnn = d->n_dnn, Y.has_dnn = d->n_dnn > 0;
    Y.FD = d->F * d->D;
    const int64_t ld = (int64_t)Y.FD + d->dense_dim;
    SATRANS_REQUIRE(ld <= 0x7fffffffLL, SATRANS_E_UNSUPPORTED, "%s: %lld DNN input columns", who, (long long)ld);
    Y.ld = (int)ld;
    Y.rows = rows_of(d->B, 0, nullptr, nullptr);
    Y.att = Lyr{Y.FD, 1, 1, d->dnn_linear_w, d->out_bias, nullptr, nullptr};
    int64_t part = layer_part(Y.rows, false, Y.att, who, "dnn_linear", 0);
    if (part < 0) return (int)part;
    const int64_t B = d->B, BFD = B * Y.FD;
    Y.s_y = 0, Y.s_stats = Y.L * BFD, Y.s_in = Y.s_stats + Y.L * int_stats(Y.p);
    int64_t at = Y.s_in, wide = 1;
    if (Y.has_dnn) {
        chain_dnn(Y.dnn, false, d->n_dnn, d->width, Y.ld, 1, d->dnn_w, d->dnn_b, d->dnn_linear_w ? d->dnn_linear_w + Y.FD : nullptr,
                  nullptr);
        if (int rc = chain_fits(Y.rows, Y.dnn, who, "dnn", part)) return rc;
        at += B * ld;
        for (int l = 0; l < d->n_dnn; ++l) {
            Y.dnn.s[l] = at;
            at += B * d->width[l];
            wide = std::max<int64_t>(wide, d->width[l]);
        }
    }
    Y.saved = at;
    part = std::max(part, int_part(Y.p));
    Y.w_g[0] = 0, Y.w_g[1] = BFD;
    Y.w_dx = 2 * BFD;
    Y.w_buf[0] = Y.w_dx + (Y.has_dnn ? B * ld : 0);
    Y.w_buf[1] = Y.w_buf[0] + (Y.has_dnn ? B * wide : 0);
    Y.w_part = Y.w_buf[1] + (Y.has_dnn ? B * wide : 0);
    Y.total = Y.w_part + part;
    return SATRANS_OK;
}

bool autoint_has(const satrans_autoint_desc* d, const AutoInt& Y) {
    for (int l = 0; l < Y.L; ++l)
        if (!d->w_query[l] || !d->w_key[l] || !d->w_value[l] || (!(d->flags & SATRANS_NO_RES) && !d->w_res[l])) return false;
    return d->emb && d->dnn_linear_w && d->out_bias && (d->dense || !Y.dense || !Y.has_dnn) &&
           (!Y.has_dnn || chain_has(Y.dnn, d->dnn_w, d->dnn_b, d->dnn_linear_w, false));
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_interacting_saved_floats(const satrans_interacting_desc* d) {
    IntPlan p;
    return int_validate(d, "interacting_saved_floats", p) ? -1 : int_stats(p);
}

extern "C" int64_t satrans_interacting_scratch_floats(const satrans_interacting_desc* d) {
    IntPlan p;
    return int_validate(d, "interacting_scratch_floats", p) ? -1 : int_part(p);
}

extern "C" int satrans_interacting_fwd(const satrans_interacting_desc* d, float* y, float* att, float* saved, void* stream_) {
    IntPlan p;
    if (int rc = int_validate(d, "interacting_fwd", p)) return rc;
    SATRANS_REQUIRE(d->x && d->w_query && d->w_key && d->w_value && (d->w_res || p.nblk == 3) && y && saved, SATRANS_E_BADARG,
                    "interacting_fwd: null pointer");
    return int_launch_fwd(p, d->x, d->w_query, d->w_key, d->w_value, p.nblk == 4 ? d->w_res : nullptr, y, saved, att,
                          (hipStream_t)stream_);
}

extern "C" int satrans_interacting_bwd(const satrans_interacting_desc* d, const float* y, const float* dy, float* dx, const float* saved,
                                       float* scratch, float* g_w, void* stream_) {
    IntPlan p;
    if (int rc = int_validate(d, "interacting_bwd", p)) return rc;
    SATRANS_REQUIRE(d->x && d->w_query && d->w_key && d->w_value && (d->w_res || p.nblk == 3) && y && dy && dx && saved && scratch && g_w,
                    SATRANS_E_BADARG, "interacting_bwd: null pointer");
    return int_launch_bwd(p, d->x, y, dy, d->w_query, d->w_key, d->w_value, p.nblk == 4 ? d->w_res : nullptr, saved, nullptr, 0, dx,
                          scratch, g_w, (hipStream_t)stream_);
}

extern "C" int64_t satrans_autoint_saved_floats(const satrans_autoint_desc* d) {
    AutoInt Y;
    const int rc = autoint_validate(d, "autoint_saved_floats", Y);
    return rc ? -1 : Y.saved;
}

extern "C" int64_t satrans_autoint_workspace_floats(const satrans_autoint_desc* d) {
    AutoInt Y;
    const int rc = autoint_validate(d, "autoint_workspace_floats", Y);
    return rc ? -1 : Y.total;
}

extern "C" int satrans_autoint_fwd(const satrans_autoint_desc* d, float* logit, float* const* att, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    AutoInt Y;
    if (int rc = autoint_validate(d, "autoint_fwd", Y)) return rc;
    SATRANS_REQUIRE(autoint_has(d, Y) && logit && saved, SATRANS_E_BADARG, "autoint_fwd: null pointer");
    const bool res = !(d->flags & SATRANS_NO_RES);
    const int64_t BFD = (int64_t)Y.p.B * Y.FD;
    const float* x = d->emb;
    for (int l = 0; l < Y.L; ++l) {
        float* y = saved + Y.s_y + l * BFD;
        if (int rc = int_launch_fwd(Y.p, x, d->w_query[l], d->w_key[l], d->w_value[l], res ? d->w_res[l] : nullptr, y,
                                    saved + Y.s_stats + l * int_stats(Y.p), att ? att[l] : nullptr, st))
            return rc;
        x = y;
    }
    // logit = att_output . dnn_linear[: F D] + out.bias, then + deep_out . dnn_linear[F D :]
    if (int rc = launch_fwd<false>(Y.rows, Y.att, x, Y.FD, 0, 0, logit, 1, 0, st)) return rc;
    if (!Y.has_dnn) return SATRANS_OK;
    float* in = saved + Y.s_in;
    autoint_concat_kernel<<<(unsigned)ceil_div((int64_t)Y.p.B * Y.ld, kThreads), kThreads, 0, st>>>(d->emb, d->dense, Y.p.B, Y.FD, Y.dense,
                                                                                                   in);
    SATRANS_CHECK_LAUNCH("autoint_concat_kernel");
    return dnn_fwd<false>(Y.rows, Y.dnn, in, saved, logit, st, 1);
}

extern "C" int satrans_autoint_bwd(const satrans_autoint_desc* d, const float* dlogit, float* demb, float* ddense, const float* saved,
                                   float* workspace, const satrans_autoint_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    AutoInt Y;
    if (int rc = autoint_validate(d, "autoint_bwd", Y)) return rc;
    SATRANS_REQUIRE(autoint_has(d, Y) && dlogit && demb && saved && workspace && g && g->dnn_linear_w && g->out_bias &&
                        (ddense || !Y.dense || !Y.has_dnn) && (!Y.has_dnn || chain_has(Y.dnn, g->dnn_w, g->dnn_b, g->dnn_linear_w, false)),
                    SATRANS_E_BADARG, "autoint_bwd: null pointer");
    for (int l = 0; l < Y.L; ++l) SATRANS_REQUIRE(g->int_w[l], SATRANS_E_BADARG, "autoint_bwd: null gradient of layer %d", l);
    const bool res = !(d->flags & SATRANS_NO_RES);
    const int64_t BFD = (int64_t)Y.p.B * Y.FD;
    float* part = workspace + Y.w_part;
    float* gbuf[2] = {workspace + Y.w_g[0], workspace + Y.w_g[1]};
    // dnn_linear's att_output columns and out.bias; the gradient of att_output
    Y.att.gw = g->dnn_linear_w, Y.att.gb = g->out_bias;
    if (int rc = launch_bwd<false>(Y.rows, Y.att, dlogit, 1, saved + Y.s_y + (Y.L - 1) * BFD, Y.FD, 0, false, 0, gbuf[0], part, st)) return rc;
    float* dxd = nullptr;
    if (Y.has_dnn) {
        set_grads(Y.dnn, g->dnn_w, g->dnn_b, g->dnn_linear_w + Y.FD, nullptr, false);
        dxd = workspace + Y.w_dx;
        float* buf[2] = {workspace + Y.w_buf[0], workspace + Y.w_buf[1]};
        int cur = 0;
        if (int rc = dnn_bwd<false>(Y.rows, Y.dnn, dlogit, saved + Y.s_in, saved, 0, dxd, buf, cur, part, st)) return rc;
        if (Y.dense) {
            autoint_dense_grad_kernel<<<(unsigned)ceil_div((int64_t)Y.p.B * Y.dense, kThreads), kThreads, 0, st>>>(dxd, Y.p.B, Y.FD, Y.dense,
                                                                                                                  ddense);
            SATRANS_CHECK_LAUNCH("autoint_dense_grad_kernel");
        }
    }
    int cur = 0;
    for (int l = Y.L - 1; l >= 0; --l) {
        const float* x = l ? saved + Y.s_y + (l - 1) * BFD : d->emb;
        float* dx = l ? gbuf[cur ^ 1] : demb;
        if (int rc = int_launch_bwd(Y.p, x, saved + Y.s_y + l * BFD, gbuf[cur], d->w_query[l], d->w_key[l], d->w_value[l],
                                    res ? d->w_res[l] : nullptr, saved + Y.s_stats + l * int_stats(Y.p), l ? nullptr : dxd, Y.ld, dx, part,
                                    g->int_w[l], st))
            return rc;
        cur ^= 1;
    }
    return SATRANS_OK;
}
