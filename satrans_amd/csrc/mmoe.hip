// Scenario-routed MMoE head (reference models/mmoe.py:142-171 with the loss of mtl_basemodel.py:268-269) for a mixed batch.
// The reference runs every task's gate and tower over every row and then keeps the column of the row's own scenario; here the
// experts run over all rows (dense products) and a row goes through its OWN task's gate, mixture, tower and logit only
// (scenario-grouped products over order / seg, walked as seg_walk.h describes).
//
// Layout.  x [B,C], every hidden row, the gates, the mixture, every dz and dx stay in the caller's row order.  The E experts'
// hidden rows of a layer sit side by side: [B, E * n_l], expert e in columns [e n_l, (e + 1) n_l).  A workgroup owns (one row
// tile of kTM rows) x (one tile of kTN output columns) of one group and streams the contraction in steps of kTK.  A group is an
// expert (dense: the row tiles are cut in the caller's row order) or a task (routed: the row tiles are cut from the start of
// the task's run).
//
// Products.  Exact f32-input MFMA (v_mfma_f32_32x32x2_f32), the tile product of star.hip restated: a result element is a
// k-ordered fmaf chain and does not depend on the tile its row falls into.  Both operands go through LDS ([64][kTK + 1]
// floats, conflict-free for the fragment reads); the next step's global loads are issued before the current step's MFMAs.
//
//   forward   mmoe_gemm_kernel<false, false>   experts: layer 1 is one product with N = E n_1 over x, layer l >= 2 has E groups
//             mmoe_gemm_kernel<false, true>    gate DNN and gate_dnn_final_layer of the row's task -> scores [B,E]
//             mmoe_mix_fwd_kernel              g = softmax(scores), m = sum_e g[e] expert_out[e]; a wave per row, E in registers
//             mmoe_gemm_kernel<false, true>    tower DNN, tower_dnn_final_layer and out[t].bias of the row's task -> logit
//   backward  tower (routed), last layer to first, the last product writes dm;
//             mmoe_mix_bwd_kernel              dz of the experts' last layer = g[e] dm (expert_out > 0), dscores
//             experts (dense), last layer to first, the last product WRITES dx;
//             gate (routed), last layer to first, the last product ADDS its dx to the experts' (one add per element);
//             per layer: mmoe_dw_kernel (partials over chunks of kDwChunk rows: routed chunks are counted from the start of a
//             task's run, the experts' chunks in the caller's row order) and mmoe_reduce_kernel (chunks in chunk order, fp64
//             sums of the fp32 partials; a task without rows gets zeros), then mmoe_gemm_kernel<true, .> for the input gradient.
// No floating-point atomics anywhere: equal inputs give equal bits, and a task's rows give the same bits alone as in a mix
// (logits, dx rows, that task's gate / tower / out-bias gradients; the experts' gradients sum over all rows).
#include <algorithm>

#include "seg_walk.h"

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

// group g of the workgroup (a task when ROUTED, else an expert), W = w + g N K, row strides ldin / ldout:
//   out[row, g ogo + n] = epilogue(sum_k in[row, g igo + k] * W[n, k])            WT = false   (W [N, K])
//   out[row, g ogo + n] = epilogue(sum_k in[row, g igo + k] * W[k, n])            WT = true    (W [K, N])
// epilogue: + bias[g N + n] (when bias), relu (when relu), * (mask[same place as out] > 0) (when mask), + out (when add)
// grid: ROUTED  row-tile slots x n tiles;  dense  row tiles x G x n tiles
template <bool WT, bool ROUTED>
__global__ __launch_bounds__(kThreads) void mmoe_gemm_kernel(const float* __restrict__ in, int ldin, int igo,
                                                             const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                             int B, int K, int N, int S, int G, int ntiles,
                                                             const float* __restrict__ w, const float* __restrict__ bias, int relu,
                                                             const float* __restrict__ mask, int add, float* out, int ldout,
                                                             int ogo) {
    __shared__ float As[kTM][kLd];
    __shared__ float Bs[kTN][kLd];
    __shared__ int rows_sh[kTM];
    const int n0 = (blockIdx.x % ntiles) * kTN;
    const int unit = blockIdx.x / ntiles;
    const SegSlot tl = unit_of<ROUTED>(seg, S, B, ROUTED ? unit : unit / G, kTM, ROUTED ? 0 : unit % G);
    if (tl.s < 0) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    if (t < kTM) rows_sh[t] = unit_row<ROUTED>(order, tl.r0 + t, tl.r1, B);
    const float* wd = w + (size_t)tl.s * N * K;
    const int ic = ROUTED ? 0 : tl.s * igo, oc = ROUTED ? 0 : tl.s * ogo;      // a task's rows are whole rows
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
    const float bv = bias ? bias[(size_t)tl.s * N + n] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = rows_sh[wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)];
        if (row < 0) continue;
        float v = acc[q] + bv;
        if (relu) v = fmaxf(v, 0.f);
        const size_t at = (size_t)row * ldout + oc + n;
        if (mask) v = mask[at] > 0.f ? v : 0.f;
        if (add) v = out[at] + v;
        out[at] = v;
    }
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

// unit u = a chunk of kDwChunk rows of group g:  part_w[u][n, k] = sum over the chunk's rows of dz[row, g zgo + n] * h[row, g hgo + k],
// part_b[u][n] = sum of dz[row, g zgo + n] (when part_b).  ROUTED: u = chunk slot, g = its task, zgo = hgo = 0.
// Dense: u = chunk * G + g.   grid: units x n tiles x k tiles
template <bool ROUTED>
__global__ __launch_bounds__(kThreads) void mmoe_dw_kernel(const float* __restrict__ dz, int ldz, int zgo, const float* __restrict__ h,
                                                           int ldh, int hgo, const int32_t* __restrict__ order,
                                                           const int32_t* __restrict__ seg, int B, int K, int N, int S, int G,
                                                           int ntiles, int ktiles, float* __restrict__ part_w,
                                                           float* __restrict__ part_b) {
    __shared__ float As[kTM][kLd];      // [n][row of the step]
    __shared__ float Bs[kTN][kLd];      // [k][row of the step]
    const int per_unit = ntiles * ktiles;
    const int unit = blockIdx.x / per_unit, rem = blockIdx.x % per_unit;
    const int n0 = (rem / ktiles) * kTM, c0 = (rem % ktiles) * kTN;
    const SegSlot tl = unit_of<ROUTED>(seg, S, B, ROUTED ? unit : unit / G, kDwChunk, ROUTED ? 0 : unit % G);
    if (tl.s < 0) return;
    const int zc = ROUTED ? 0 : tl.s * zgo, hc = ROUTED ? 0 : tl.s * hgo;
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

// One thread per element of a group's [N*K weights | N biases] (the biases only when part_b): the group's chunks in chunk
// order.  ROUTED: group = task, its chunks are the slots [first_slot, + scenario_units).  Dense: chunk c of group g is unit c G + g.
template <bool ROUTED>
__global__ __launch_bounds__(kThreads) void mmoe_reduce_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                               const int32_t* __restrict__ seg, int B, int64_t NK, int N, int S, int G,
                                                               int nchunks, float* __restrict__ g_w, float* __restrict__ g_b) {
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
        const int k0 = first_slot(seg, g, B, kDwChunk), nch = scenario_units(seg, g, B, kDwChunk);
        for (int k = k0; k < k0 + nch; ++k) sum += part[(size_t)k * width + at];
    } else {
        for (int k = 0; k < nchunks; ++k) sum += part[((size_t)k * G + g) * width + at];
    }
    (is_w ? g_w : g_b)[(size_t)g * width + at] = (float)sum;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

// a layer of one of the three DNNs as the launches see it: G groups of [N, K] weights (G = 1 for routed layers and for the
// experts' first layer, whose E blocks share x and so form one product of N = E n_1)
struct Lyr {
    int K, N, G;
    const float *w, *b;
    float *gw, *gb;
};

struct MmoeLayout {
    int nx, ng, nt;                                   // layers of the three chains (gate and tower: hidden + final)
    Lyr x[kMaxH], g[kMaxH + 1], t[kMaxH + 1];
    int64_t slots, dw_slots, tiles, chunks;
    int64_t n_last;                                   // width of an expert's output
    // saved (floats from its start): gates [B,E], mixture [B,n_last], scores [B,E], then the hidden rows
    int64_t s_gates, s_mix, s_scores, s_x[kMaxH], s_g[kMaxH], s_t[kMaxH], saved;
    // workspace: two dz buffers [B, max_w], dscores [B,E], the partials of the layer in hand
    int64_t max_w, w_dz, w_dscores, w_part, total;
};

int mmoe_validate(const satrans_mmoe_desc* d, const char* who, MmoeLayout& L) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->C > 0 && d->T > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d C=%d T=%d", who, d->B, d->C, d->T);
    SATRANS_REQUIRE(d->E >= 2 && d->E <= kMaxE, SATRANS_E_BADARG, "%s: bad sizes E=%d (2 to %d experts)", who, d->E, kMaxE);
    SATRANS_REQUIRE(d->n_expert >= 1 && d->n_expert <= kMaxH && d->n_gate >= 0 && d->n_gate <= kMaxH && d->n_tower >= 0 &&
                        d->n_tower <= kMaxH,
                    SATRANS_E_BADARG, "%s: bad sizes: %d expert, %d gate, %d tower hidden layers (1 to %d, 0 to %d, 0 to %d)", who,
                    d->n_expert, d->n_gate, d->n_tower, kMaxH, kMaxH, kMaxH);
    for (int l = 0; l < d->n_expert; ++l)
        SATRANS_REQUIRE(d->expert_width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes expert_width[%d]=%d", who, l, d->expert_width[l]);
    for (int l = 0; l < d->n_gate; ++l)
        SATRANS_REQUIRE(d->gate_width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes gate_width[%d]=%d", who, l, d->gate_width[l]);
    for (int l = 0; l < d->n_tower; ++l)
        SATRANS_REQUIRE(d->tower_width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes tower_width[%d]=%d", who, l, d->tower_width[l]);
    SATRANS_REQUIRE(d->T <= 65535, SATRANS_E_UNSUPPORTED, "%s: T=%d tasks (65535 at most)", who, d->T);
    const int64_t B = d->B, E = d->E;
    L.nx = d->n_expert, L.ng = d->n_gate + 1, L.nt = d->n_tower + 1;
    int prev = d->C;
    for (int l = 0; l < L.nx; ++l) {
        const int n = d->expert_width[l];
        SATRANS_REQUIRE(E * n <= 0x7fffffffLL / 4, SATRANS_E_UNSUPPORTED, "%s: E * expert_width[%d] = %lld", who, l, (long long)(E * n));
        L.x[l] = l == 0 ? Lyr{prev, (int)(E * n), 1, d->expert_w[l], d->expert_b[l], nullptr, nullptr}
                        : Lyr{prev, n, (int)E, d->expert_w[l], d->expert_b[l], nullptr, nullptr};
        prev = n;
    }
    L.n_last = prev;
    prev = d->C;
    for (int l = 0; l < L.ng; ++l) {
        const bool fin = l == L.ng - 1;
        L.g[l] = Lyr{prev, fin ? (int)E : d->gate_width[l], 1, fin ? d->gate_final_w : d->gate_w[l], fin ? nullptr : d->gate_b[l],
                     nullptr, nullptr};
        prev = L.g[l].N;
    }
    prev = (int)L.n_last;
    for (int l = 0; l < L.nt; ++l) {
        const bool fin = l == L.nt - 1;
        L.t[l] = Lyr{prev, fin ? 1 : d->tower_width[l], 1, fin ? d->tower_final_w : d->tower_w[l], fin ? d->out_bias : d->tower_b[l],
                     nullptr, nullptr};
        prev = L.t[l].N;
    }
    L.slots = seg_slots(B, d->T, kTM);
    L.dw_slots = seg_slots(B, d->T, kDwChunk);
    L.tiles = ceil_div(B, kTM);
    L.chunks = ceil_div(B, kDwChunk);
    int64_t at = 0, per_part = 0;
    L.max_w = std::max<int64_t>(L.n_last, E);
    auto take = [&](int64_t n) {
        const int64_t a = at;
        at += B * n;
        return a;
    };
    L.s_gates = take(E);
    L.s_mix = take(L.n_last);
    L.s_scores = take(E);
    for (int l = 0; l < L.nx; ++l) {
        const Lyr& y = L.x[l];
        const int64_t wide = (int64_t)y.N * y.G;
        L.s_x[l] = take(wide);
        L.max_w = std::max(L.max_w, wide);
        per_part = std::max(per_part, L.chunks * y.G * y.N * ((int64_t)y.K + 1));
        SATRANS_REQUIRE((int64_t)y.N * y.K <= 0x7fffffffLL && L.tiles * y.G * ceil_div(std::max(y.N, y.K), kTN) <= 0x7fffffffLL &&
                            L.chunks * y.G * ceil_div(y.N, kTM) * ceil_div(y.K, kTN) <= 0x7fffffffLL,
                        SATRANS_E_UNSUPPORTED, "%s: expert layer %d (%d x %d) at B=%d needs more than 2^31 workgroups", who, l, y.N,
                        y.K, d->B);
    }
    for (int c = 0; c < 2; ++c) {
        const int nl = c ? L.nt : L.ng;
        for (int l = 0; l < nl; ++l) {
            const Lyr& y = c ? L.t[l] : L.g[l];
            if (l < nl - 1) {
                (c ? L.s_t : L.s_g)[l] = take(y.N);
                L.max_w = std::max<int64_t>(L.max_w, y.N);
            }
            per_part = std::max(per_part, L.dw_slots * y.N * ((int64_t)y.K + 1));
            SATRANS_REQUIRE((int64_t)y.N * y.K <= 0x7fffffffLL && L.slots * ceil_div(std::max(y.N, y.K), kTN) <= 0x7fffffffLL &&
                                L.dw_slots * ceil_div(y.N, kTM) * ceil_div(y.K, kTN) <= 0x7fffffffLL,
                            SATRANS_E_UNSUPPORTED, "%s: %s layer %d (%d x %d) at B=%d needs more than 2^31 workgroups", who,
                            c ? "tower" : "gate", l, y.N, y.K, d->B);
        }
    }
    L.saved = at;
    L.w_dz = 0;
    L.w_dscores = 2 * B * L.max_w;
    L.w_part = L.w_dscores + B * E;
    L.total = L.w_part + per_part;
    return SATRANS_OK;
}

bool mmoe_has_operands(const satrans_mmoe_desc* d) {
    if (!d->x || !d->order || !d->seg || !d->gate_final_w || !d->tower_final_w || !d->out_bias) return false;
    for (int l = 0; l < d->n_expert; ++l)
        if (!d->expert_w[l] || !d->expert_b[l]) return false;
    for (int l = 0; l < d->n_gate; ++l)
        if (!d->gate_w[l] || !d->gate_b[l]) return false;
    for (int l = 0; l < d->n_tower; ++l)
        if (!d->tower_w[l] || !d->tower_b[l]) return false;
    return true;
}

bool mmoe_has_grads(const satrans_mmoe_desc* d, const satrans_mmoe_grads* g) {
    if (!g || !g->gate_final_w || !g->tower_final_w || !g->out_bias) return false;
    for (int l = 0; l < d->n_expert; ++l)
        if (!g->expert_w[l] || !g->expert_b[l]) return false;
    for (int l = 0; l < d->n_gate; ++l)
        if (!g->gate_w[l] || !g->gate_b[l]) return false;
    for (int l = 0; l < d->n_tower; ++l)
        if (!g->tower_w[l] || !g->tower_b[l]) return false;
    return true;
}

// out = epilogue(in W^T) of one layer;  in [B, ldin] with group column offset igo, out [B, G N]
template <bool ROUTED>
int launch_fwd(const satrans_mmoe_desc* d, const MmoeLayout& L, const Lyr& y, const float* in, int ldin, int igo, int relu, float* out,
               hipStream_t st) {
    const int ntiles = (int)ceil_div(y.N, kTN);
    const int64_t units = ROUTED ? L.slots : L.tiles * y.G;
    mmoe_gemm_kernel<false, ROUTED><<<(unsigned)(units * ntiles), kThreads, 0, st>>>(in, ldin, igo, d->order, d->seg, d->B, y.K, y.N, d->T,
                                                                                     y.G, ntiles, y.w, y.b, relu, nullptr, 0, out,
                                                                                     y.N * y.G, y.N);
    SATRANS_CHECK_LAUNCH("mmoe_gemm_kernel (forward)");
    return SATRANS_OK;
}

// the backward of one layer: its parameter gradients from (dz, hin), then din = dz W, masked by hin > 0 (when masked), added
// to what din holds (when add).  dz [B, G N], hin / din [B, ldh] with group column offset hgo.
template <bool ROUTED>
int launch_bwd(const satrans_mmoe_desc* d, const MmoeLayout& L, const Lyr& y, const float* dz, const float* hin, int ldh, int hgo,
               bool masked, int add, float* din, float* workspace, hipStream_t st) {
    const int64_t NK = (int64_t)y.N * y.K;
    const int ntiles = (int)ceil_div(y.N, kTM), ktiles = (int)ceil_div(y.K, kTN);
    const int64_t units = ROUTED ? L.dw_slots : L.chunks * y.G;
    const int groups = ROUTED ? d->T : y.G;
    float* part_w = workspace + L.w_part;
    float* part_b = y.b ? part_w + units * NK : nullptr;
    mmoe_dw_kernel<ROUTED><<<(unsigned)(units * ntiles * ktiles), kThreads, 0, st>>>(dz, y.N * y.G, y.N, hin, ldh, hgo, d->order, d->seg,
                                                                                    d->B, y.K, y.N, d->T, y.G, ntiles, ktiles, part_w,
                                                                                    part_b);
    SATRANS_CHECK_LAUNCH("mmoe_dw_kernel");
    const int64_t elems = (NK + (y.b ? y.N : 0)) * groups;
    mmoe_reduce_kernel<ROUTED><<<(unsigned)ceil_div(elems, kThreads), kThreads, 0, st>>>(part_w, part_b, d->seg, d->B, NK, y.N, d->T,
                                                                                        groups, (int)L.chunks, y.gw, y.gb);
    SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel");
    // contraction over this layer's N outputs, K columns out
    const int otiles = (int)ceil_div(y.K, kTN);
    const int64_t gunits = ROUTED ? L.slots : L.tiles * y.G;
    mmoe_gemm_kernel<true, ROUTED><<<(unsigned)(gunits * otiles), kThreads, 0, st>>>(dz, y.N * y.G, y.N, d->order, d->seg, d->B, y.N, y.K,
                                                                                    d->T, y.G, otiles, y.w, nullptr, 0,
                                                                                    masked ? hin : nullptr, add, din, ldh, hgo);
    SATRANS_CHECK_LAUNCH("mmoe_gemm_kernel (backward)");
    return SATRANS_OK;
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_mmoe_saved_floats(const satrans_mmoe_desc* d) {
    MmoeLayout L;
    const int rc = mmoe_validate(d, "mmoe_saved_floats", L);
    return rc ? rc : L.saved;
}

extern "C" int64_t satrans_mmoe_workspace_floats(const satrans_mmoe_desc* d) {
    MmoeLayout L;
    const int rc = mmoe_validate(d, "mmoe_workspace_floats", L);
    return rc ? rc : L.total;
}

extern "C" int satrans_mmoe_fwd(const satrans_mmoe_desc* d, float* logit, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MmoeLayout L;
    int rc = mmoe_validate(d, "mmoe_fwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(mmoe_has_operands(d) && logit && saved, SATRANS_E_BADARG, "mmoe_fwd: null pointer");
    const int B = d->B, E = d->E, n_last = (int)L.n_last;
    // experts: layer 1 over x, then block-diagonal
    const float* in = d->x;
    int ldin = d->C;
    for (int l = 0; l < L.nx; ++l) {
        float* out = saved + L.s_x[l];
        if ((rc = launch_fwd<false>(d, L, L.x[l], in, ldin, l == 0 ? 0 : L.x[l].K, 1, out, st))) return rc;
        in = out;
        ldin = L.x[l].N * L.x[l].G;
    }
    const float* eo = in;
    // the row's own gate
    in = d->x;
    for (int l = 0; l < L.ng; ++l) {
        const bool fin = l == L.ng - 1;
        float* out = saved + (fin ? L.s_scores : L.s_g[l]);
        if ((rc = launch_fwd<true>(d, L, L.g[l], in, L.g[l].K, 0, fin ? 0 : 1, out, st))) return rc;
        in = out;
    }
    mmoe_mix_fwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(saved + L.s_scores, eo, B, E, n_last, saved + L.s_gates,
                                                                             saved + L.s_mix);
    SATRANS_CHECK_LAUNCH("mmoe_mix_fwd_kernel");
    // the row's own tower, final layer and out bias
    in = saved + L.s_mix;
    for (int l = 0; l < L.nt; ++l) {
        const bool fin = l == L.nt - 1;
        float* out = fin ? logit : saved + L.s_t[l];
        if ((rc = launch_fwd<true>(d, L, L.t[l], in, L.t[l].K, 0, fin ? 0 : 1, out, st))) return rc;
        in = out;
    }
    return SATRANS_OK;
}

extern "C" int satrans_mmoe_bwd(const satrans_mmoe_desc* d, const float* dlogit, float* dx, const float* saved, float* workspace,
                                const satrans_mmoe_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MmoeLayout L;
    int rc = mmoe_validate(d, "mmoe_bwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(mmoe_has_operands(d) && dlogit && dx && saved && workspace && mmoe_has_grads(d, g), SATRANS_E_BADARG,
                    "mmoe_bwd: null pointer");
    for (int l = 0; l < L.nx; ++l) L.x[l].gw = g->expert_w[l], L.x[l].gb = g->expert_b[l];
    for (int l = 0; l < L.ng; ++l) {
        const bool fin = l == L.ng - 1;
        L.g[l].gw = fin ? g->gate_final_w : g->gate_w[l];
        L.g[l].gb = fin ? nullptr : g->gate_b[l];
    }
    for (int l = 0; l < L.nt; ++l) {
        const bool fin = l == L.nt - 1;
        L.t[l].gw = fin ? g->tower_final_w : g->tower_w[l];
        L.t[l].gb = fin ? g->out_bias : g->tower_b[l];
    }
    const int B = d->B, E = d->E, n_last = (int)L.n_last;
    float* buf[2] = {workspace + L.w_dz, workspace + L.w_dz + (size_t)B * L.max_w};
    float* dscores = workspace + L.w_dscores;
    int cur = 0;      // the buffer the next product writes
    // tower: dlogit -> dm
    const float* dz = dlogit;
    for (int l = L.nt - 1; l >= 0; --l) {
        const float* hin = saved + (l == 0 ? L.s_mix : L.s_t[l - 1]);
        if ((rc = launch_bwd<true>(d, L, L.t[l], dz, hin, L.t[l].K, 0, l > 0, 0, buf[cur], workspace, st))) return rc;
        dz = buf[cur];
        cur ^= 1;
    }
    // mixture and softmax: dm -> dz of the experts' last layer, dscores
    const float* eo = saved + L.s_x[L.nx - 1];
    mmoe_mix_bwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(dz, saved + L.s_gates, eo, B, E, n_last, buf[cur], dscores);
    SATRANS_CHECK_LAUNCH("mmoe_mix_bwd_kernel");
    dz = buf[cur];
    cur ^= 1;
    // experts (dense): the last product writes dx
    for (int l = L.nx - 1; l >= 0; --l) {
        const Lyr& y = L.x[l];
        if (l == 0) {
            if ((rc = launch_bwd<false>(d, L, y, dz, d->x, d->C, 0, false, 0, dx, workspace, st))) return rc;
        } else {
            if ((rc = launch_bwd<false>(d, L, y, dz, saved + L.s_x[l - 1], y.K * y.G, y.K, true, 0, buf[cur], workspace, st))) return rc;
            dz = buf[cur];
            cur ^= 1;
        }
    }
    // gate (routed): the last product adds its dx to the experts'
    dz = dscores;
    for (int l = L.ng - 1; l >= 0; --l) {
        const Lyr& y = L.g[l];
        if (l == 0) {
            if ((rc = launch_bwd<true>(d, L, y, dz, d->x, d->C, 0, false, 1, dx, workspace, st))) return rc;
        } else {
            if ((rc = launch_bwd<true>(d, L, y, dz, saved + L.s_g[l - 1], y.K, 0, true, 0, buf[cur], workspace, st))) return rc;
            dz = buf[cur];
            cur ^= 1;
        }
    }
    return SATRANS_OK;
}
