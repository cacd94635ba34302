// The grouped 64 x 64 tile product of the scenario heads (mmoe.hip, ple.hip, sharedbottom.hip, adasparse.hip), of the dense
// DNNs of the single-task heads (fibinet.hip, pnn.hip, fm.hip, autoint.hip, esmm.hip) and of STAR's towers (star.hip), its weight-gradient and reduce kernels, and the softmax mixture over up to 8 experts.  Every kernel sits
// in an unnamed namespace: each file that includes this header gets its own copies, under the names mmoe.hip gave them.
// star.hip wraps the same tile body with the shared factor switched on (SHARED: W_dom * W_sh on operand load, b_dom + b_sh)
// and the weight-gradient body with G = 1 as a constant; esmm.hip switches on the dropout option of the dense form (DROP,
// mmoe_gemm_drop_kernel).  This header is device code only; the host code that launches it for
// the four heads (a layer, a batch, launch_fwd / launch_bwd, the grid check, the walks over a DNN) is head_layers.h.
//
// Layout.  Rows, hidden rows, dz and dx stay in the caller's row order.  The hidden rows of G blocks of a layer sit side by
// side: [B, G * n_l], block g in columns [g n_l, (g + 1) n_l).  A workgroup owns (one row tile of kTM rows) x (one tile of kTN
// output columns) of one group and streams the contraction in steps of kTK.  Three forms of a group:
//   dense             group = block g of the grid; the row tiles are cut in the caller's row order
//   routed            group = task; the row tiles are cut from the start of the task's run (seg_walk.h); whole rows
//   routed, grouped   group = (task, block j of G): block j of the row's task reads its own column block and writes its own;
//                     the weights are [T, G, N, K]                                        (routed with G = 1 is the plain form)
//
// Products.  Exact f32-input MFMA (v_mfma_f32_32x32x2_f32): a result element is a k-ordered fmaf chain and does not depend on
// the tile its row falls into.  Both operands go through LDS ([64][kTK + 1] floats, conflict-free for the fragment reads); the
// next step's global loads are issued before the current step's MFMAs.
#pragma once
#include "seg_walk.h"
// (after seg_walk.h, which brings in the HIP runtime)
#include "rng.h"

namespace satrans {
namespace {

constexpr int kTM = SATRANS_MMOE_ROW_TILE;
constexpr int kTN = 64;
constexpr int kTK = 32;
constexpr int kLd = kTK + 1;
constexpr int kThreads = 256;
constexpr int kDwChunk = SATRANS_MMOE_DW_ROW_CHUNK;
constexpr int kPer = kTM * kTK / kThreads;      // elements of an operand tile per thread
constexpr int kMaxE = SATRANS_MMOE_MAX_EXPERTS;
constexpr int kMaxH = SATRANS_MMOE_MAX_HIDDEN;
constexpr int kMixRows = kThreads / 64;         // rows of a workgroup of the mixture kernels: a wave each
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

// the unit of rows a workgroup takes and the group whose parameters it uses.  ROUTED: a unit of a task's run (seg_walk.h),
// group = task.  Dense: unit `slot` of the caller's row order, group `g` from the grid.
template <bool ROUTED>
__device__ __forceinline__ SegSlot unit_of(const int32_t* __restrict__ seg, int S, int B, int slot, int rows, int g) {
    if (ROUTED) return find_slot<SegSlot>(seg, S, B, slot, rows);
    const int r0 = slot * rows;
    return r0 < B ? SegSlot{g, r0, min(r0 + rows, B)} : SegSlot{-1, 0, 0};
}

template <bool ROUTED>
__device__ __forceinline__ int unit_row(const int32_t* __restrict__ order, int p, int r1, int B) {
    if (ROUTED) return row_at(order, p, r1, B);
    return p < r1 ? p : -1;
}

// Thread mappings of a [64][kTK] operand tile, element e = 0..kPer-1 of thread t:
//   "k fast"  (the contraction index is contiguous in memory):  i = (t >> 5) + 8 e,  k = t & 31
//   "i fast"  (the tile's row index is contiguous in memory):   i = t & 63,          k = (t >> 6) + 4 e

// ---- forward layers and the input gradients -------------------------------------------------------------------------------------

// The dropout option of a hidden layer (DROP; off by default, and then nothing of it is compiled in).  The keep bit is rng.h's
// counter-based function of (seed, step, layer, site, row + row_offset, column), so it depends neither on the tiling nor on what
// else is in the batch; oracle.satrans_oracle.dropout_keep restates it.  A layer whose output stacks several sites side by
// side (a first layer shared by two towers) gives `per`, the columns of one site: column n of block g belongs to site
// site + g + n / per and is element n % per of it.  Forward: h = keep ? relu(z) * scale : 0.  Backward: nothing is regenerated -
// h > 0 already means "kept and past the relu" - and the masked input gradient becomes mask > 0 ? v * scale : 0.
struct DropArgs {
    uint32_t seed, step;
    int layer, site, per;      // per = 0: the whole block is one site
    uint32_t thresh;           // drop_threshold(p)
    float scale;               // 1 / (1 - p), formed on the host
    uint32_t row_offset;       // of the caller's row 0 in the global batch
};

// the site key and the element index of output column n of block blk
__device__ __forceinline__ uint32_t drop_column(const DropArgs& dr, int blk, int n, uint32_t& elem) {
    const int s = dr.per > 0 ? n / dr.per : 0;
    elem = (uint32_t)(dr.per > 0 ? n - s * dr.per : n);
    return drop_site_key(dr.seed, dr.step, dr.layer, dr.site + blk + s);
}

// group of the workgroup: block g of G (dense) or block g of G of the rows' task t (ROUTED; G = 1: the task's whole rows).
// W = w + g N K (dense) or w + (t G + g) N K (ROUTED), times w_sh [N, K] elementwise when SHARED; row strides ldin / ldout:
//   out[row, g ogo + n] = epilogue(sum_k in[row, g igo + k] * W[n, k])            WT = false   (W [N, K])
//   out[row, g ogo + n] = epilogue(sum_k in[row, g igo + k] * W[k, n])            WT = true    (W [K, N])
// epilogue: + bias[group N + n] (+ b_sh[n] when SHARED) (when bias), relu (when relu), * (mask[same place as out] > 0) (when
// mask), + out (when add).  DROP: the forward epilogue (WT = false) drops after the relu, the masked one (WT = true) scales.
template <bool WT, bool ROUTED, bool SHARED, bool DROP = false>
__device__ __forceinline__ void gemm_tile(const float* __restrict__ in, int ldin, int igo, const int32_t* __restrict__ order,
                                          const int32_t* __restrict__ seg, int B, int K, int N, int S, int G, int ntiles,
                                          const float* __restrict__ w, const float* __restrict__ w_sh,
                                          const float* __restrict__ bias, const float* __restrict__ b_sh, int relu,
                                          const float* __restrict__ mask, int add, float* out, int ldout, int ogo,
                                          const DropArgs& dr = DropArgs{}) {
    __shared__ float As[kTM][kLd];
    __shared__ float Bs[kTN][kLd];
    __shared__ int rows_sh[kTM];
    const int n0 = (blockIdx.x % ntiles) * kTN;
    const int unit = blockIdx.x / ntiles;
    const int blk = unit % G;
    const SegSlot tl = unit_of<ROUTED>(seg, S, B, unit / G, kTM, blk);
    if (tl.s < 0) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    if (t < kTM) rows_sh[t] = unit_row<ROUTED>(order, tl.r0 + t, tl.r1, B);
    const size_t grp = ROUTED ? (size_t)tl.s * G + blk : (size_t)blk;      // whose parameters
    const float* wd = w + grp * N * K;
    const int ic = blk * igo, oc = blk * ogo;      // G = 1: whole rows
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    const int jf = t & 63, kf0 = t >> 6;      // "i fast"
    int my_rows[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) my_rows[e] = unit_row<ROUTED>(order, tl.r0 + if0 + 8 * e, tl.r1, B);
    float ra[kPer], rb[kPer];
    auto load = [&](int k0) {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int k = k0 + kf;
            ra[e] = (my_rows[e] >= 0 && k < K) ? in[(size_t)my_rows[e] * ldin + ic + k] : 0.f;
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
            if (SHARED)
                rb[e] = ok ? wd[at] * w_sh[at] : 0.f;
            else
                rb[e] = ok ? wd[at] : 0.f;
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
    const float bv = bias ? (SHARED ? bias[grp * N + n] + b_sh[n] : bias[grp * N + n]) : 0.f;
    uint32_t site_key = 0, elem = 0;
    if (DROP && !WT) site_key = drop_column(dr, blk, n, elem);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = rows_sh[wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)];
        if (row < 0) continue;
        float v = acc[q] + bv;
        if (relu) v = fmaxf(v, 0.f);
        if (DROP && !WT) v = drop_keep(drop_sample_key(site_key, (uint32_t)row + dr.row_offset), elem, dr.thresh) ? v * dr.scale : 0.f;
        const size_t at = (size_t)row * ldout + oc + n;
        if (DROP && WT) {
            if (mask) v = mask[at] > 0.f ? v * dr.scale : 0.f;
        } else if (mask) v = mask[at] > 0.f ? v : 0.f;
        if (add) v = out[at] + v;
        out[at] = v;
    }
}

// grid: ROUTED  row-tile slots x G x n tiles;  dense  row tiles x G x n tiles
template <bool WT, bool ROUTED>
__global__ __launch_bounds__(kThreads) void mmoe_gemm_kernel(const float* __restrict__ in, int ldin, int igo,
                                                             const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                             int B, int K, int N, int S, int G, int ntiles,
                                                             const float* __restrict__ w, const float* __restrict__ bias, int relu,
                                                             const float* __restrict__ mask, int add, float* out, int ldout,
                                                             int ogo) {
    gemm_tile<WT, ROUTED, false>(in, ldin, igo, order, seg, B, K, N, S, G, ntiles, w, nullptr, bias, nullptr, relu, mask, add, out,
                                 ldout, ogo);
}

// the same launch with the dropout option on; dense only (the routed heads refuse dropout)
template <bool WT>
__global__ __launch_bounds__(kThreads) void mmoe_gemm_drop_kernel(const float* __restrict__ in, int ldin, int igo, int B, int K, int N,
                                                                  int G, int ntiles, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, int relu,
                                                                  const float* __restrict__ mask, int add, float* out, int ldout,
                                                                  int ogo, DropArgs dr) {
    gemm_tile<WT, false, false, true>(in, ldin, igo, nullptr, nullptr, B, K, N, 0, G, ntiles, w, nullptr, bias, nullptr, relu, mask,
                                      add, out, ldout, ogo, dr);
}

// ---- softmax and mixture --------------------------------------------------------------------------------------------------------

// a wave per row: g = softmax(scores[row, :E]), m[row, j] = sum_e g[e] * eo[row, e n + j] (e ascending)
__global__ __launch_bounds__(kThreads) void mmoe_mix_fwd_kernel(const float* __restrict__ scores, const float* __restrict__ eo, int B,
                                                                int E, int n, float* __restrict__ gates, float* __restrict__ m) {
    const int row = blockIdx.x * kMixRows + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float g[kMaxE];
    float mx = -INFINITY, sum = 0.f;
#pragma unroll
    for (int e = 0; e < kMaxE; ++e) {
        g[e] = e < E ? scores[(size_t)row * E + e] : -INFINITY;
        mx = fmaxf(mx, g[e]);
    }
#pragma unroll
    for (int e = 0; e < kMaxE; ++e) {
        g[e] = e < E ? expf(g[e] - mx) : 0.f;
        sum += g[e];
    }
#pragma unroll
    for (int e = 0; e < kMaxE; ++e) {
        g[e] = g[e] / sum;
        if (lane == e && e < E) gates[(size_t)row * E + e] = g[e];
    }
    const float* er = eo + (size_t)row * E * n;
    for (int j = lane; j < n; j += 64) {
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < kMaxE; ++e)
            if (e < E) acc = fmaf(g[e], er[(size_t)e * n + j], acc);
        m[(size_t)row * n + j] = acc;
    }
}

// a wave per row: dz[row, e n + j] = g[e] dm[row, j] (eo > 0);  dg[e] = sum_j dm[row, j] eo[row, e n + j] (a lane's j ascending,
// then the 64 lanes by a fixed butterfly);  dscores[row, e] = g[e] (dg[e] - sum_e' g[e'] dg[e'])
__global__ __launch_bounds__(kThreads) void mmoe_mix_bwd_kernel(const float* __restrict__ dm, const float* __restrict__ gates,
                                                                const float* __restrict__ eo, int B, int E, int n,
                                                                float* __restrict__ dz, float* __restrict__ dscores) {
    const int row = blockIdx.x * kMixRows + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float g[kMaxE], dg[kMaxE];
#pragma unroll
    for (int e = 0; e < kMaxE; ++e) {
        g[e] = e < E ? gates[(size_t)row * E + e] : 0.f;
        dg[e] = 0.f;
    }
    const float* er = eo + (size_t)row * E * n;
    float* zr = dz + (size_t)row * E * n;
    for (int j = lane; j < n; j += 64) {
        const float d = dm[(size_t)row * n + j];
#pragma unroll
        for (int e = 0; e < kMaxE; ++e)
            if (e < E) {
                const float v = er[(size_t)e * n + j];
                dg[e] = fmaf(d, v, dg[e]);
                zr[(size_t)e * n + j] = v > 0.f ? g[e] * d : 0.f;
            }
    }
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < kMaxE; ++e) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dg[e] += __shfl_xor(dg[e], off, 64);
        dot = fmaf(g[e], dg[e], dot);
    }
#pragma unroll
    for (int e = 0; e < kMaxE; ++e)
        if (lane == e && e < E) dscores[(size_t)row * E + e] = g[e] * (dg[e] - dot);
}

// ---- weight gradients -----------------------------------------------------------------------------------------------------------

// unit u = a chunk of kDwChunk rows of block g of G:  part_w[u][n, k] = sum over the chunk's rows of dz[row, g zgo + n] * h[row, g hgo + k],
// part_b[u][n] = sum of dz[row, g zgo + n] (when part_b).  ROUTED: u = chunk slot * G + g (the slot names the task).
// Dense: u = chunk * G + g.   grid: units x n tiles x k tiles
template <bool ROUTED>
__device__ __forceinline__ void dw_tile(const float* __restrict__ dz, int ldz, int zgo, const float* __restrict__ h, int ldh, int hgo,
                                        const int32_t* __restrict__ order, const int32_t* __restrict__ seg, int B, int K, int N, int S,
                                        int G, int ntiles, int ktiles, float* __restrict__ part_w, float* __restrict__ part_b) {
    __shared__ float As[kTM][kLd];      // [n][row of the step]
    __shared__ float Bs[kTN][kLd];      // [k][row of the step]
    const int per_unit = ntiles * ktiles;
    const int unit = blockIdx.x / per_unit, rem = blockIdx.x % per_unit;
    const int n0 = (rem / ktiles) * kTM, c0 = (rem % ktiles) * kTN;
    const int blk = unit % G;
    const SegSlot tl = unit_of<ROUTED>(seg, S, B, unit / G, kDwChunk, blk);
    if (tl.s < 0) return;
    const int zc = blk * zgo, hc = blk * hgo;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int jf = t & 63, kf0 = t >> 6;
    float ra[kPer], rb[kPer];
    auto load = [&](int p0) {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int row = unit_row<ROUTED>(order, p0 + kf0 + 4 * e, tl.r1, B);
            const int n = n0 + jf, c = c0 + jf;
            ra[e] = (row >= 0 && n < N) ? dz[(size_t)row * ldz + zc + n] : 0.f;
            rb[e] = (row >= 0 && c < K) ? h[(size_t)row * ldh + hc + c] : 0.f;
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
        if (part_b && c0 == 0 && t < kTM) {      // the bias gradient: rows of the chunk in order (rows past its end hold zeros)
#pragma unroll
            for (int kk = 0; kk < kTK; ++kk) bsum += As[t][kk];
        }
        mma_step(As, Bs, lane, wm, wn, acc);
    }
    if (part_b && c0 == 0 && t < kTM && n0 + t < N) part_b[(size_t)unit * N + n0 + t] = bsum;
    const int c = c0 + wn * 32 + (lane & 31);
    if (c >= K) return;
    float* out = part_w + (size_t)unit * N * K;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int n = n0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (n < N) out[(size_t)n * K + c] = acc[q];
    }
}

template <bool ROUTED>
__global__ __launch_bounds__(kThreads) void mmoe_dw_kernel(const float* __restrict__ dz, int ldz, int zgo, const float* __restrict__ h,
                                                           int ldh, int hgo, const int32_t* __restrict__ order,
                                                           const int32_t* __restrict__ seg, int B, int K, int N, int S, int G,
                                                           int ntiles, int ktiles, float* __restrict__ part_w,
                                                           float* __restrict__ part_b) {
    dw_tile<ROUTED>(dz, ldz, zgo, h, ldh, hgo, order, seg, B, K, N, S, G, ntiles, ktiles, part_w, part_b);
}

// One thread per element of a group's [N*K weights | N biases] (the biases only when part_b): the group's chunks in chunk
// order.  G groups; ROUTED: group = (task, block j of J), G = T J, its chunks are the units k J + j of the task's slots k in
// [first_slot, + scenario_units).  Dense: chunk c of group g is unit c G + g.
template <bool ROUTED>
__global__ __launch_bounds__(kThreads) void mmoe_reduce_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                               const int32_t* __restrict__ seg, int B, int64_t NK, int N, int S, int G,
                                                               int J, int nchunks, float* __restrict__ g_w, float* __restrict__ g_b) {
    const int64_t per = NK + (part_b ? N : 0);
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= per * G) return;
    const int g = (int)(e / per);
    const int64_t r = e % per;
    const bool is_w = r < NK;
    const int64_t at = is_w ? r : r - NK, width = is_w ? NK : N;
    const float* part = is_w ? part_w : part_b;
    double sum = 0.0;
    if (ROUTED) {
        const int task = g / J, j = g % J;
        const int k0 = first_slot(seg, task, B, kDwChunk), nch = scenario_units(seg, task, B, kDwChunk);
        for (int k = k0; k < k0 + nch; ++k) sum += part[((size_t)k * J + j) * width + at];
    } else {
        for (int k = 0; k < nchunks; ++k) sum += part[((size_t)k * G + g) * width + at];
    }
    (is_w ? g_w : g_b)[(size_t)g * width + at] = (float)sum;
}

}  // namespace
}  // namespace satrans
