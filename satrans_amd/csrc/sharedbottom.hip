// Scenario-routed SharedBottom head (reference models/sharedbottom.py:120-133 with the loss of mtl_basemodel.py:268-269) for a
// mixed batch.  The reference runs every task's tower over every row and then keeps the column of the row's own scenario;
// here the bottom DNN runs over all rows (dense products) and a row goes through its OWN task's tower, final layer and
// out bias only (scenario-grouped products over order / seg, walked as seg_walk.h describes).
//
// Layout, the tile product and the weight-gradient kernels are in grouped_gemm.h; the launches of a layer, the backward walk over
// a DNN and the per-layer grid check are in head_layers.h, shared with the other heads.  This file holds the tower tail, the
// layout of the saved rows and the workspace, the validation and the order of the launches.
//
//   forward   mmoe_gemm_kernel<false, false>   the bottom DNN, G = 1
//             mmoe_gemm_kernel<false, true>    the tower's hidden layers except the last, group = task
//             sb_tail_fwd_kernel               the tail, one launch: a workgroup takes one row tile of a task's run and walks the
//                                              64-column tiles of the last tower layer; per tile h = relu(acc + b[t]) goes to
//                                              saved and, through LDS, to the thread that owns the row, which continues
//                                              logit = fmaf(h[n], wf[t][n], logit), n ascending; logit + out_bias[t] at the end.
//                                              Without a tower layer the tiles are read from the bottom's last rows instead.
//             (composed, satrans_sharedbottom_set_forward(1): the last tower layer and the final layer as two launches of
//             mmoe_gemm_kernel<false, true>, the second with N = 1 - the same chains, so the same bits)
//   backward  sb_tail_bwd_kernel               dz[row, n] = dlogit[row] wf[t][n] (h[row, n] > 0) and, in the same pass, the chunk
//                                              partials of d wf[t][n] = sum dlogit h and d out_bias[t] = sum dlogit; merged in
//                                              chunk order by mmoe_reduce_kernel<true>
//             tower (routed) and bottom (dense), last layer to first: mmoe_dw_kernel, mmoe_reduce_kernel, then
//             mmoe_gemm_kernel<true, .> for the input gradient; the bottom's first layer WRITES dx.
// No floating-point atomics anywhere: equal inputs give equal bits, and a task's rows give the same bits alone as in a mix
// (logits, dx rows, that task's tower / final-layer / out-bias gradients; the bottom's gradients sum over all rows).
#include "head_layers.h"

namespace satrans {
namespace {

int g_sb_composed = 0;

constexpr int kHLd = kTN + 1;      // a row of the staged h tile: the owner of row i reads Hs[i][0 .. 63], conflict-free
constexpr int kTailRows = kDwChunk / (kThreads / 64);      // rows of a chunk under one wave of sb_tail_bwd_kernel
static_assert(kTailRows * (kThreads / 64) == kDwChunk, "the waves of sb_tail_bwd_kernel split a chunk evenly");

// The tower tail.  A workgroup = one row tile (kTM rows) of a task's run; slot = blockIdx.x.
//   LAYER   h[row, n] = relu(sum_k in[row, k] w[t][n, k] + b[t][n]) -> hout [B,N]   (in [B,K]; the chain of mmoe_gemm_kernel)
//   !LAYER  h = in [B,N]
//   logit[row] = (fmaf chain over n = 0 .. N-1 of h[row, n] wf[t][n], from 0.f) + out_bias[t]
template <bool LAYER>
__global__ __launch_bounds__(kThreads) void sb_tail_fwd_kernel(const float* __restrict__ in, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ seg, int B, int K, int N, int S,
                                                               const float* __restrict__ w, const float* __restrict__ b,
                                                               const float* __restrict__ wf, const float* __restrict__ out_bias,
                                                               float* __restrict__ hout, float* __restrict__ logit) {
    __shared__ float As[LAYER ? kTM : 1][kLd];
    __shared__ float Bs[LAYER ? kTN : 1][kLd];
    __shared__ float Hs[kTM][kHLd];
    __shared__ int rows_sh[kTM];
    const SegSlot tl = find_slot<SegSlot>(seg, S, B, blockIdx.x, kTM);
    if (tl.s < 0) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    if (t < kTM) rows_sh[t] = row_at(order, tl.r0 + t, tl.r1, B);
    __syncthreads();
    const float* wfd = wf + (size_t)tl.s * N;
    float lg = 0.f;
    if constexpr (LAYER) {
        const float* wd = w + (size_t)tl.s * N * K;
        const float* bd = b + (size_t)tl.s * N;
        const int kf = t & 31, if0 = t >> 5;      // "k fast"
        int my_rows[kPer];
#pragma unroll
        for (int e = 0; e < kPer; ++e) my_rows[e] = rows_sh[if0 + 8 * e];
        for (int n0 = 0; n0 < N; n0 += kTN) {
            float ra[kPer], rb[kPer];
            auto load = [&](int k0) {
                const int k = k0 + kf;
#pragma unroll
                for (int e = 0; e < kPer; ++e) ra[e] = (my_rows[e] >= 0 && k < K) ? in[(size_t)my_rows[e] * K + k] : 0.f;
#pragma unroll
                for (int e = 0; e < kPer; ++e) {
                    const int n = n0 + if0 + 8 * e;
                    rb[e] = (n < N && k < K) ? wd[(size_t)n * K + k] : 0.f;
                }
            };
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            load(0);
            for (int k0 = 0; k0 < K; k0 += kTK) {
                __syncthreads();      // the previous step's fragment reads are done
#pragma unroll
                for (int e = 0; e < kPer; ++e) {
                    As[if0 + 8 * e][kf] = ra[e];
                    Bs[if0 + 8 * e][kf] = rb[e];
                }
                __syncthreads();
                if (k0 + kTK < K) load(k0 + kTK);
                mma_step(As, Bs, lane, wm, wn, acc);
            }
            const int j = wn * 32 + (lane & 31), n = n0 + j;
            const float bv = n < N ? bd[n] : 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                const float v = fmaxf(acc[q] + bv, 0.f);
                Hs[i][j] = v;
                const int row = rows_sh[i];
                if (row >= 0 && n < N) hout[(size_t)row * N + n] = v;
            }
            __syncthreads();
            if (t < kTM) {
                const int jn = min(kTN, N - n0);
                for (int c = 0; c < jn; ++c) lg = fmaf(Hs[t][c], wfd[n0 + c], lg);
            }
            // the next tile's first barrier (before As / Bs are written) also orders these reads of Hs before its epilogue
        }
    } else {
        for (int n0 = 0; n0 < N; n0 += kTN) {
            __syncthreads();      // the previous tile's chain has read Hs
            const int j = t & 63, n = n0 + j;
#pragma unroll
            for (int e = 0; e < kTM / 4; ++e) {
                const int i = (t >> 6) + 4 * e, row = rows_sh[i];
                Hs[i][j] = (row >= 0 && n < N) ? in[(size_t)row * N + n] : 0.f;
            }
            __syncthreads();
            if (t < kTM) {
                const int jn = min(kTN, N - n0);
                for (int c = 0; c < jn; ++c) lg = fmaf(Hs[t][c], wfd[n0 + c], lg);
            }
        }
    }
    if (t < kTM && rows_sh[t] >= 0) logit[rows_sh[t]] = lg + out_bias[tl.s];
}

// The tail's backward.  A workgroup = (one chunk of kDwChunk rows of a task's run) x (one tile of 64 columns); unit =
// blockIdx.x / ntiles names the chunk slot.  Wave v takes rows [v kTailRows, (v + 1) kTailRows) of the chunk in order, lane =
// column n:
//   dz[row, n] = h[row, n] > 0 ? dlogit[row] wf[t][n] : 0
//   part_w[unit][n] = sum over the chunk's rows of dlogit[row] h[row, n]      (a wave's rows in order, then the waves in order)
//   part_b[unit]    = sum over the chunk's rows of dlogit[row]                (likewise; written by the first column tile)
__global__ __launch_bounds__(kThreads) void sb_tail_bwd_kernel(const float* __restrict__ dlogit, const float* __restrict__ h,
                                                               const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                               int B, int N, int S, int ntiles, const float* __restrict__ wf,
                                                               float* __restrict__ dz, float* __restrict__ part_w,
                                                               float* __restrict__ part_b) {
    __shared__ float red_w[kThreads / 64][64];
    __shared__ float red_b[kThreads / 64];
    const int unit = blockIdx.x / ntiles, n = (blockIdx.x % ntiles) * 64 + (threadIdx.x & 63);
    const SegSlot tl = find_slot<SegSlot>(seg, S, B, unit, kDwChunk);
    if (tl.s < 0) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool live = n < N;
    const float wv_n = live ? wf[(size_t)tl.s * N + n] : 0.f;
    float pw = 0.f, pb = 0.f;
    const int p0 = tl.r0 + wv * kTailRows, p1 = min(p0 + kTailRows, tl.r1);
    for (int p = p0; p < p1; ++p) {
        const int row = row_at(order, p, tl.r1, B);
        if (row < 0) continue;
        const float d = dlogit[row];
        pb += d;
        if (live) {
            const float hv = h[(size_t)row * N + n];
            dz[(size_t)row * N + n] = hv > 0.f ? d * wv_n : 0.f;
            pw = fmaf(d, hv, pw);
        }
    }
    red_w[wv][lane] = pw;
    if (lane == 0) red_b[wv] = pb;
    __syncthreads();
    if (wv == 0) {
        float sw = red_w[0][lane], sb = red_b[0];
#pragma unroll
        for (int v = 1; v < kThreads / 64; ++v) {
            sw += red_w[v][lane];
            sb += red_b[v];
        }
        if (live) part_w[(size_t)unit * N + n] = sw;
        if (blockIdx.x % ntiles == 0 && lane == 0) part_b[unit] = sb;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

struct SbLayout {
    Chain b, t;                // the bottom (dense) and the towers' hidden layers (routed), no final layer: every layer's rows are saved
    int n_bottom, n_tail;      // width of the bottom's last rows; width under the final layer
    Rows rows;
    int64_t saved;                              // saved: the hidden rows, floats from its start
    int64_t max_w, w_dz, w_part, total;         // workspace: two dz buffers [B, max_w], the partials of the layer in hand
};

int sb_validate(const satrans_sharedbottom_desc* d, const char* who, SbLayout& L) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->C > 0 && d->T > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d C=%d T=%d", who, d->B, d->C, d->T);
    SATRANS_REQUIRE(d->n_bottom >= 1 && d->n_bottom <= kMaxH && d->n_tower >= 0 && d->n_tower <= kMaxH, SATRANS_E_BADARG,
                    "%s: bad sizes: %d bottom, %d tower hidden layers (1 to %d, 0 to %d)", who, d->n_bottom, d->n_tower, kMaxH, kMaxH);
    for (int l = 0; l < d->n_bottom; ++l)
        SATRANS_REQUIRE(d->bottom_width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes bottom_width[%d]=%d", who, l, d->bottom_width[l]);
    for (int l = 0; l < d->n_tower; ++l)
        SATRANS_REQUIRE(d->tower_width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes tower_width[%d]=%d", who, l, d->tower_width[l]);
    SATRANS_REQUIRE(d->T <= 65535, SATRANS_E_UNSUPPORTED, "%s: T=%d tasks (65535 at most)", who, d->T);
    const int64_t B = d->B;
    L.n_bottom = d->bottom_width[d->n_bottom - 1];
    L.n_tail = d->n_tower ? d->tower_width[d->n_tower - 1] : L.n_bottom;
    chain_dnn(L.b, false, d->n_bottom, d->bottom_width, d->C, 0, d->bottom_w, d->bottom_b, nullptr, nullptr);
    chain_dnn(L.t, true, d->n_tower, d->tower_width, L.n_bottom, 0, d->tower_w, d->tower_b, nullptr, nullptr);
    L.rows = rows_of(d->B, d->T, d->order, d->seg);
    int64_t at = 0, per_part = 0;
    L.max_w = 0;
    for (Chain* c : {&L.b, &L.t})
        for (int l = 0; l < c->n; ++l) {
            c->s[l] = at;
            at += B * c->y[l].N;
            L.max_w = std::max<int64_t>(L.max_w, c->y[l].N);
        }
    int rc;
    if ((rc = chain_fits(L.rows, L.b, who, "bottom", per_part)) || (rc = chain_fits(L.rows, L.t, who, "tower", per_part))) return rc;
    per_part = std::max(per_part, L.rows.dw_slots * ((int64_t)L.n_tail + 1));
    SATRANS_REQUIRE(L.rows.dw_slots * ceil_div(L.n_tail, 64) <= 0x7fffffffLL, SATRANS_E_UNSUPPORTED,
                    "%s: the final layer (%d wide) at B=%d needs more than 2^31 workgroups", who, L.n_tail, d->B);
    L.saved = at;
    L.w_dz = 0;
    L.w_part = 2 * B * L.max_w;
    L.total = L.w_part + per_part;
    return SATRANS_OK;
}

// every pointer of a satrans_sharedbottom_desc (P = const float) or a satrans_sharedbottom_grads (P = float) that the head
// reads or writes
template <class P, class S>
bool sb_has(const SbLayout& L, const S* g) {
    return g && g->tower_final_w && g->out_bias && chain_has<P>(L.b, g->bottom_w, g->bottom_b, nullptr, true) &&
           chain_has<P>(L.t, g->tower_w, g->tower_b, nullptr, true);
}

// the hidden layers [0, n) of a chain, forward: in -> the last of them, every layer's rows into saved
template <bool ROUTED>
int hidden_fwd(const Rows& r, const Chain& c, int n, const float*& in, float* saved, hipStream_t st) {
    for (int l = 0; l < n; ++l) {
        const Lyr& y = c.y[l];
        if (int rc = launch_fwd<ROUTED>(r, y, in, y.K, 0, 1, saved + c.s[l], y.N, 0, st)) return rc;
        in = saved + c.s[l];
    }
    return SATRANS_OK;
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int satrans_sharedbottom_set_forward(int composed) {
    SATRANS_REQUIRE(composed == 0 || composed == 1, SATRANS_E_BADARG, "sharedbottom_set_forward: mode %d (0 fused, 1 composed)",
                    composed);
    const int was = g_sb_composed;
    g_sb_composed = composed;
    return was;
}

extern "C" int64_t satrans_sharedbottom_saved_floats(const satrans_sharedbottom_desc* d) {
    SbLayout L;
    const int rc = sb_validate(d, "sharedbottom_saved_floats", L);
    return rc ? rc : L.saved;
}

extern "C" int64_t satrans_sharedbottom_workspace_floats(const satrans_sharedbottom_desc* d) {
    SbLayout L;
    const int rc = sb_validate(d, "sharedbottom_workspace_floats", L);
    return rc ? rc : L.total;
}

extern "C" int satrans_sharedbottom_fwd(const satrans_sharedbottom_desc* d, float* logit, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    SbLayout L;
    int rc = sb_validate(d, "sharedbottom_fwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x && d->order && d->seg && sb_has<const float>(L, d) && logit && saved, SATRANS_E_BADARG,
                    "sharedbottom_fwd: null pointer");
    const Rows& R = L.rows;
    const int nt = L.t.n;
    const float* in = d->x;
    if ((rc = hidden_fwd<false>(R, L.b, L.b.n, in, saved, st))) return rc;
    if ((rc = hidden_fwd<true>(R, L.t, g_sb_composed ? nt : nt - 1, in, saved, st))) return rc;
    if (g_sb_composed) {
        const Lyr fin{L.n_tail, 1, 1, d->tower_final_w, d->out_bias, nullptr, nullptr};
        return launch_fwd<true>(R, fin, in, L.n_tail, 0, 0, logit, 1, 0, st);
    }
    if (nt > 0) {
        const Lyr& y = L.t.y[nt - 1];
        sb_tail_fwd_kernel<true><<<(unsigned)R.slots, kThreads, 0, st>>>(in, d->order, d->seg, d->B, y.K, y.N, d->T, y.w, y.b,
                                                                         d->tower_final_w, d->out_bias, saved + L.t.s[nt - 1], logit);
    } else {
        sb_tail_fwd_kernel<false><<<(unsigned)R.slots, kThreads, 0, st>>>(in, d->order, d->seg, d->B, 0, L.n_tail, d->T, nullptr, nullptr,
                                                                          d->tower_final_w, d->out_bias, nullptr, logit);
    }
    SATRANS_CHECK_LAUNCH("sb_tail_fwd_kernel");
    return SATRANS_OK;
}

extern "C" int satrans_sharedbottom_bwd(const satrans_sharedbottom_desc* d, const float* dlogit, float* dx, const float* saved,
                                        float* workspace, const satrans_sharedbottom_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    SbLayout L;
    int rc = sb_validate(d, "sharedbottom_bwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x && d->order && d->seg && sb_has<const float>(L, d) && dlogit && dx && saved && workspace && sb_has<float>(L, g),
                    SATRANS_E_BADARG, "sharedbottom_bwd: null pointer");
    set_grads(L.b, g->bottom_w, g->bottom_b, nullptr, nullptr, true);
    set_grads(L.t, g->tower_w, g->tower_b, nullptr, nullptr, true);
    const Rows& R = L.rows;
    const int B = d->B, nt = L.t.n;
    float* buf[2] = {workspace + L.w_dz, workspace + L.w_dz + (size_t)B * L.max_w};
    float* part = workspace + L.w_part;
    int cur = 0;      // the buffer the next product writes
    // the tail: dlogit -> dz of the last tower layer (of the bottom's last layer without one), d tower_final_w, d out_bias
    const float* h_bottom = saved + L.b.s[L.b.n - 1];
    {
        const float* h = nt > 0 ? saved + L.t.s[nt - 1] : h_bottom;
        const int n = L.n_tail, ntiles = (int)ceil_div(n, 64);
        float* part_b = part + R.dw_slots * n;
        sb_tail_bwd_kernel<<<(unsigned)(R.dw_slots * ntiles), kThreads, 0, st>>>(dlogit, h, d->order, d->seg, B, n, d->T, ntiles,
                                                                                 d->tower_final_w, buf[cur], part, part_b);
        SATRANS_CHECK_LAUNCH("sb_tail_bwd_kernel");
        mmoe_reduce_kernel<true><<<(unsigned)ceil_div((int64_t)(n + 1) * d->T, kThreads), kThreads, 0, st>>>(
            part, part_b, d->seg, B, n, 1, d->T, d->T, 1, (int)R.chunks, g->tower_final_w, g->out_bias);
        SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel");
    }
    const float* dz = buf[cur];
    cur ^= 1;
    // towers (routed): the first layer's input gradient goes under the bottom's relu mask
    for (int l = nt - 1; l >= 0; --l) {
        const Lyr& y = L.t.y[l];
        const float* hin = l == 0 ? h_bottom : saved + L.t.s[l - 1];
        if ((rc = launch_bwd<true>(R, y, dz, y.N, hin, y.K, 0, true, 0, buf[cur], part, st))) return rc;
        dz = buf[cur];
        cur ^= 1;
    }
    // bottom (dense): the last product writes dx
    return dnn_bwd<false>(R, L.b, dz, d->x, saved, 0, dx, buf, cur, part, st);
}
