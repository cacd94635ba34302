// ESMM's two towers (reference models/esmm.py:84-96) and WDL's DNN-only head (models/wdl.py:75-79) with dropout inside the
// DNNs.  Nothing is routed: `towers` DNNs of equal widths run over all rows of x, each ends in a bias-free final layer, and
//   towers = 2 (ESMM)   p_t = sigmoid(logit_t + out_bias),  out[row] = (p_0, p_0 p_1)      (ctr, ctcvr; p_1 is the pCVR)
//   towers = 1 (WDL)    out[row] = logit_0 + out_bias                                      (a logit; the caller keeps the sigmoid)
//
// Layout, the tile product and the weight-gradient kernels are in grouped_gemm.h; the launches of a layer, the dense
// block-diagonal stack and the dropout option (DropArgs) are in head_layers.h.  The towers are that stack with blocks = towers:
// layer 1 is ONE product of N = towers * n_1 over x, a later layer is block-diagonal with G = towers; tower t's hidden rows
// sit in columns [t n_l, (t + 1) n_l) of [B, towers * n_l].  This file holds the two tail kernels, the pointwise end, the layout
// of the saved rows and the workspace, the validation and the order of the launches.
//
//   forward   mmoe_gemm_kernel<false, false>   the hidden layers (mmoe_gemm_drop_kernel<false> in training with p > 0), then
//                                              the final layer as one more launch of the tile product with N = 1, G = towers
//             esmm_point_kernel                towers = 2: the sigmoids and the product          (the composed form, the default)
//             (fused, satrans_esmm_set_forward(0): esmm_tail_fwd_kernel, one launch for the last hidden layer and everything after
//             it: a workgroup takes a row tile and walks the 64-column tiles of the last hidden layer of tower 0, then of tower
//             1; per tile h = relu(acc + b), with dropout in training, goes to saved and, through LDS, to the thread that owns the
//             row, which continues logit_t = fmaf(h[n], wf[t][n], logit_t), n ascending; then the pointwise end.  With one hidden
//             layer that launch is the whole head.  The same chains, so the same bits.  Measured at B = 8192, C = 608, (256, 128)
//             it is up to 6 % slower - 128 workgroups walk four tiles each where the composed form spreads 512 - so it is not
//             the default: profiles/esmm_time.txt)
//   backward  esmm_tail_bwd_kernel             dlogit_t from dout and the saved p_t; dz_t[row, n] = dlogit_t wf[t][n] (* scale)
//                                              where h_t[row, n] > 0, and in the same pass the chunk partials of d wf[t][n] =
//                                              sum dlogit_t h_t and d out_bias = sum (dlogit_0 + dlogit_1); merged in chunk order
//                                              by mmoe_reduce_kernel<false>
//             the stack, last layer to first: mmoe_dw_kernel, mmoe_reduce_kernel, then the input gradient (mmoe_gemm_kernel<true,
//             false>, or mmoe_gemm_drop_kernel<true> where the mask went through dropout); the first layer WRITES dx.
// Dropout: the keep bit of (hidden layer l, tower t, row, column n of that tower's layer) is rng.h's function of (seed, step, l, t,
// row + row_offset, n); only the dropped-out h is saved and the backward regenerates nothing - h > 0 is "kept and past the relu".
// No floating-point atomics anywhere: equal inputs give equal bits, and a sample alone gives the bits it gives inside a batch
// (its out row and its dx row; with dropout when row_offset places it where it sat).
#include "head_layers.h"

namespace satrans {
namespace {

int g_esmm_composed = 1;      // the default: the fused tail did not beat it (profiles/esmm_time.txt)

constexpr int kHLd = kTN + 1;      // a row of the staged h tile: the owner of row i reads Hs[i][0 .. 63], conflict-free
constexpr int kTailRows = kDwChunk / (kThreads / 64);      // rows of a chunk under one wave of esmm_tail_bwd_kernel
static_assert(kTailRows * (kThreads / 64) == kDwChunk, "the waves of esmm_tail_bwd_kernel split a chunk evenly");

__device__ __forceinline__ float esmm_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// the pointwise end of a row from its towers' logits (without out_bias)
template <int TOWERS>
__device__ __forceinline__ void esmm_point(float lg0, float lg1, float ob, int row, float* __restrict__ probs, float* __restrict__ out) {
    if constexpr (TOWERS == 1) {
        out[row] = lg0 + ob;
    } else {
        const float p0 = esmm_sigmoid(lg0 + ob), p1 = esmm_sigmoid(lg1 + ob);
        probs[2 * (size_t)row] = p0;
        probs[2 * (size_t)row + 1] = p1;
        out[2 * (size_t)row] = p0;
        out[2 * (size_t)row + 1] = p0 * p1;
    }
}

// The tail.  A workgroup = one row tile (kTM rows) of the caller's row order; tower t reads columns [t igo, t igo + K) of
// in [B, ldin] (igo = 0: the towers share their input) and the parameters w [TOWERS, N, K], b [TOWERS, N], wf [TOWERS, N]:
//   h_t[row, n] = drop(relu(sum_k in[row, t igo + k] w[t][n, k] + b[t][n])) -> hout [B, TOWERS N]   (the chain of mmoe_gemm_kernel)
//   logit_t[row] = fmaf chain over n = 0 .. N-1 of h_t[row, n] wf[t][n], from 0.f;  then esmm_point
template <int TOWERS, bool DROP>
__global__ __launch_bounds__(kThreads) void esmm_tail_fwd_kernel(const float* __restrict__ in, int ldin, int igo, int B, int K, int N,
                                                                 const float* __restrict__ w, const float* __restrict__ b,
                                                                 const float* __restrict__ wf, const float* __restrict__ out_bias,
                                                                 float* __restrict__ hout, float* __restrict__ probs,
                                                                 float* __restrict__ out, DropArgs dr) {
    __shared__ float As[kTM][kLd];
    __shared__ float Bs[kTN][kLd];
    __shared__ float Hs[kTM][kHLd];
    const int r0 = blockIdx.x * kTM;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    int my_rows[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) my_rows[e] = r0 + if0 + 8 * e < B ? r0 + if0 + 8 * e : -1;
    const int ldh = TOWERS * N;
    float lgs[2] = {0.f, 0.f};
#pragma unroll
    for (int tw = 0; tw < TOWERS; ++tw) {
        const float* wd = w + (size_t)tw * N * K;
        const float* bd = b + (size_t)tw * N;
        const float* wfd = wf + (size_t)tw * N;
        const int ic = tw * igo;
        float lg = 0.f;
        for (int n0 = 0; n0 < N; n0 += kTN) {
            float ra[kPer], rb[kPer];
            auto load = [&](int k0) {
                const int k = k0 + kf;
#pragma unroll
                for (int e = 0; e < kPer; ++e) ra[e] = (my_rows[e] >= 0 && k < K) ? in[(size_t)my_rows[e] * ldin + ic + k] : 0.f;
#pragma unroll
                for (int e = 0; e < kPer; ++e) {
                    const int n = n0 + if0 + 8 * e;
                    rb[e] = (n < N && k < K) ? wd[(size_t)n * K + k] : 0.f;
                }
            };
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            load(0);
            for (int k0 = 0; k0 < K; k0 += kTK) {
                __syncthreads();      // the previous step's fragment reads (and the previous tile's reads of Hs) are done
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
            uint32_t site_key = 0;
            if (DROP) site_key = drop_site_key(dr.seed, dr.step, dr.layer, dr.site + tw);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                const int row = r0 + i;
                float v = fmaxf(acc[q] + bv, 0.f);
                if (DROP) v = drop_keep(drop_sample_key(site_key, (uint32_t)row + dr.row_offset), (uint32_t)n, dr.thresh) ? v * dr.scale : 0.f;
                Hs[i][j] = v;
                if (row < B && n < N) hout[(size_t)row * ldh + tw * N + n] = v;
            }
            __syncthreads();
            if (t < kTM) {
                const int jn = min(kTN, N - n0);
                for (int c = 0; c < jn; ++c) lg = fmaf(Hs[t][c], wfd[n0 + c], lg);
            }
            // the next tile's first barrier (before As / Bs are written) also orders these reads of Hs before its epilogue
        }
        lgs[tw] = lg;
    }
    if (t < kTM && r0 + t < B) esmm_point<TOWERS>(lgs[0], lgs[1], out_bias[0], r0 + t, probs, out);
}

// the pointwise end of the composed form, towers = 2: probs [B, 2] holds the two logits on entry and (p_0, p_1) on return
__global__ __launch_bounds__(kThreads) void esmm_point_kernel(float* __restrict__ probs, const float* __restrict__ out_bias, int B,
                                                              float* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (row >= B) return;
    const float lg0 = probs[2 * row], lg1 = probs[2 * row + 1];
    esmm_point<2>(lg0, lg1, out_bias[0], (int)row, probs, out);
}

// The tail's backward.  A workgroup = (one chunk of kDwChunk rows) x (one tower) x (one tile of 64 of its columns); unit =
// blockIdx.x / (TOWERS ntiles) names the chunk.  Wave v takes rows [v kTailRows, (v + 1) kTailRows) of the chunk in order, lane
// = column n of tower t:
//   TOWERS = 2   dp_0 = dout_0 + dout_1 p_1,  dp_1 = dout_1 p_0,  dlogit_t = dp_t p_t (1 - p_t);      TOWERS = 1   dlogit_0 = dout
//   dz[row, t N + n] = h[row, t N + n] > 0 ? dlogit_t wf[t][n] (* scale when DROP) : 0
//   part_w[unit][t N + n] = sum over the chunk's rows of dlogit_t h[row, t N + n]   (a wave's rows in order, then the waves in order)
//   part_b[unit]          = sum over the chunk's rows of (dlogit_0 + dlogit_1)      (likewise; written by the chunk's first workgroup)
template <int TOWERS, bool DROP>
__global__ __launch_bounds__(kThreads) void esmm_tail_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ probs,
                                                                 const float* __restrict__ h, int B, int N, int ntiles,
                                                                 const float* __restrict__ wf, float scale, float* __restrict__ dz,
                                                                 float* __restrict__ part_w, float* __restrict__ part_b) {
    __shared__ float red_w[kThreads / 64][64];
    __shared__ float red_b[kThreads / 64];
    const int per_unit = TOWERS * ntiles;
    const int unit = blockIdx.x / per_unit, rem = blockIdx.x % per_unit;
    const int tw = rem / ntiles;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = (rem % ntiles) * 64 + lane;
    const bool live = n < N;
    const int ldh = TOWERS * N, col = tw * N + n;
    const float wv_n = live ? wf[col] : 0.f;
    float pw = 0.f, pb = 0.f;
    const int64_t p0 = (int64_t)unit * kDwChunk + wv * kTailRows, p1 = p0 + kTailRows < B ? p0 + kTailRows : B;
    for (int64_t row = p0; row < p1; ++row) {
        float d;
        if constexpr (TOWERS == 1) {
            d = dout[row];
            pb += d;
        } else {
            const float d0 = dout[2 * row], d1 = dout[2 * row + 1], q0 = probs[2 * row], q1 = probs[2 * row + 1];
            const float dl0 = (fmaf(d1, q1, d0) * q0) * (1.f - q0);
            const float dl1 = ((d1 * q0) * q1) * (1.f - q1);
            pb += dl0 + dl1;
            d = tw == 0 ? dl0 : dl1;
        }
        if (live) {
            const float hv = h[(size_t)row * ldh + col];
            const float g = DROP ? (d * wv_n) * scale : d * wv_n;
            dz[(size_t)row * ldh + col] = hv > 0.f ? g : 0.f;
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
        if (live) part_w[(size_t)unit * ldh + col] = sw;
        if (rem == 0 && lane == 0) part_b[unit] = sb;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

struct EsmmLayout {
    Chain c;                   // the towers' hidden layers as one dense block-diagonal stack, no final layer
    int towers, n_tail;        // width of one tower under the final layer
    bool drop;
    DropArgs dr;
    Rows rows;
    int64_t probs, saved;                    // saved: the hidden rows, then (towers = 2) p [B, 2]; floats from its start
    int64_t max_w, w_part, total;            // workspace: two dz buffers [B, max_w], the partials of the layer in hand
};

int esmm_validate(const satrans_esmm_desc* d, const char* who, EsmmLayout& L) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->C > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d C=%d", who, d->B, d->C);
    SATRANS_REQUIRE(d->towers == 1 || d->towers == 2, SATRANS_E_BADARG, "%s: towers=%d (1 = WDL, 2 = ESMM)", who, d->towers);
    SATRANS_REQUIRE(d->n_dnn >= 1 && d->n_dnn <= kMaxH, SATRANS_E_BADARG, "%s: bad sizes: %d hidden layers (1 to %d)", who, d->n_dnn,
                    kMaxH);
    for (int l = 0; l < d->n_dnn; ++l)
        SATRANS_REQUIRE(d->width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes width[%d]=%d", who, l, d->width[l]);
    SATRANS_REQUIRE((d->flags & ~(uint32_t)SATRANS_TRAIN) == 0, SATRANS_E_BADARG, "%s: flags %u (SATRANS_TRAIN only)", who, d->flags);
    SATRANS_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, SATRANS_E_BADARG, "%s: drop_p=%g (0 <= p < 1)", who, (double)d->drop_p);
    for (int l = 0; l < d->n_dnn; ++l)
        SATRANS_REQUIRE((int64_t)d->towers * d->width[l] <= 0x7fffffffLL, SATRANS_E_UNSUPPORTED, "%s: width[%d]=%d times %d towers", who,
                        l, d->width[l], d->towers);
    const int64_t B = d->B;
    L.towers = d->towers;
    L.n_tail = d->width[d->n_dnn - 1];
    L.drop = (d->flags & SATRANS_TRAIN) && d->drop_p > 0.f;
    L.dr = DropArgs{d->seed, d->step, 0, 0, 0, drop_threshold(d->drop_p), 1.0f / (1.0f - d->drop_p), d->row_offset};
    chain_experts(L.c, false, d->towers, d->n_dnn, d->width, d->C, d->dnn_w, d->dnn_b);
    L.rows = rows_of(d->B, 0, nullptr, nullptr);
    int64_t at = 0, per_part = 0;
    L.max_w = 0;
    for (int l = 0; l < L.c.n; ++l) {
        L.c.s[l] = at;
        at += B * L.c.y[l].N * L.c.y[l].G;
        L.max_w = std::max<int64_t>(L.max_w, (int64_t)L.c.y[l].N * L.c.y[l].G);
    }
    L.probs = at;
    L.saved = at + (d->towers == 2 ? 2 * B : 0);
    if (int rc = chain_fits(L.rows, L.c, who, "tower", per_part)) return rc;
    const Lyr fin{L.n_tail, 1, d->towers, nullptr, nullptr, nullptr, nullptr};      // the composed form's final layer
    if (layer_part(L.rows, false, fin, who, "final", d->n_dnn) < 0) return SATRANS_E_UNSUPPORTED;
    SATRANS_REQUIRE(L.rows.chunks * d->towers * ceil_div(L.n_tail, 64) <= 0x7fffffffLL, SATRANS_E_UNSUPPORTED,
                    "%s: the final layer (%d wide) at B=%d needs more than 2^31 workgroups", who, L.n_tail, d->B);
    per_part = std::max(per_part, L.rows.chunks * ((int64_t)d->towers * L.n_tail + 1));
    L.w_part = 2 * B * L.max_w;
    L.total = L.w_part + per_part;
    return SATRANS_OK;
}

// every pointer of a satrans_esmm_desc (P = const float) or a satrans_esmm_grads (P = float) that the head reads or writes
template <class P, class S>
bool esmm_has(const EsmmLayout& L, const S* g) {
    return g && g->final_w && g->out_bias && chain_has<P>(L.c, g->dnn_w, g->dnn_b, nullptr, true);
}

template <int TOWERS, bool DROP>
int esmm_fwd_run(const satrans_esmm_desc* d, const EsmmLayout& L, float* out, float* saved, hipStream_t st) {
    const Rows& R = L.rows;
    const int nl = L.c.n, N = L.n_tail;
    float* probs = saved + L.probs;
    if (g_esmm_composed) {
        if (int rc = experts_fwd<DROP>(R, L.c, d->x, d->C, saved, st, -1, TOWERS, L.dr)) return rc;
        const float* h = saved + L.c.s[nl - 1];
        if (TOWERS == 1) {
            const Lyr fin{N, 1, 1, d->final_w, d->out_bias, nullptr, nullptr};
            return launch_fwd<false>(R, fin, h, N, 0, 0, out, 1, 0, st);
        }
        const Lyr fin{N, 1, TOWERS, d->final_w, nullptr, nullptr, nullptr};
        if (int rc = launch_fwd<false>(R, fin, h, TOWERS * N, N, 0, probs, TOWERS, 1, st)) return rc;
        esmm_point_kernel<<<(unsigned)ceil_div(d->B, kThreads), kThreads, 0, st>>>(probs, d->out_bias, d->B, out);
        SATRANS_CHECK_LAUNCH("esmm_point_kernel");
        return SATRANS_OK;
    }
    if (int rc = experts_fwd<DROP>(R, L.c, d->x, d->C, saved, st, nl - 1, TOWERS, L.dr)) return rc;
    const bool first = nl == 1;      // the tail is the whole head: the towers share x
    const int K = first ? d->C : d->width[nl - 2];
    DropArgs dr = L.dr;
    dr.layer = nl - 1;
    esmm_tail_fwd_kernel<TOWERS, DROP><<<(unsigned)R.tiles, kThreads, 0, st>>>(
        first ? d->x : saved + L.c.s[nl - 2], first ? d->C : TOWERS * K, first ? 0 : K, d->B, K, N, d->dnn_w[nl - 1], d->dnn_b[nl - 1],
        d->final_w, d->out_bias, saved + L.c.s[nl - 1], probs, out, dr);
    SATRANS_CHECK_LAUNCH("esmm_tail_fwd_kernel");
    return SATRANS_OK;
}

template <int TOWERS, bool DROP>
int esmm_bwd_run(const satrans_esmm_desc* d, EsmmLayout& L, const float* dout, float* dx, const float* saved, float* workspace,
                 const satrans_esmm_grads* g, hipStream_t st) {
    const Rows& R = L.rows;
    const int B = d->B, nl = L.c.n, N = L.n_tail, ntiles = (int)ceil_div(N, 64);
    float* buf[2] = {workspace, workspace + (size_t)B * L.max_w};
    float* part = workspace + L.w_part;
    int cur = 0;      // the buffer the next product writes
    float* part_b = part + R.chunks * TOWERS * N;
    esmm_tail_bwd_kernel<TOWERS, DROP><<<(unsigned)(R.chunks * TOWERS * ntiles), kThreads, 0, st>>>(
        dout, saved + L.probs, saved + L.c.s[nl - 1], B, N, ntiles, d->final_w, L.dr.scale, buf[cur], part, part_b);
    SATRANS_CHECK_LAUNCH("esmm_tail_bwd_kernel");
    mmoe_reduce_kernel<false><<<(unsigned)ceil_div((int64_t)TOWERS * N + 1, kThreads), kThreads, 0, st>>>(
        part, part_b, nullptr, B, (int64_t)TOWERS * N, 1, 0, 1, 1, (int)R.chunks, g->final_w, g->out_bias);
    SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel");
    const float* dz = buf[cur];
    cur ^= 1;
    return experts_bwd<DROP>(R, L.c, dz, d->x, d->C, saved, dx, buf, cur, part, st, L.dr);
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int satrans_esmm_set_forward(int composed) {
    SATRANS_REQUIRE(composed == 0 || composed == 1, SATRANS_E_BADARG, "esmm_set_forward: mode %d (0 fused, 1 composed)", composed);
    const int was = g_esmm_composed;
    g_esmm_composed = composed;
    return was;
}

extern "C" int64_t satrans_esmm_saved_floats(const satrans_esmm_desc* d) {
    EsmmLayout L;
    const int rc = esmm_validate(d, "esmm_saved_floats", L);
    return rc ? rc : L.saved;
}

extern "C" int64_t satrans_esmm_workspace_floats(const satrans_esmm_desc* d) {
    EsmmLayout L;
    const int rc = esmm_validate(d, "esmm_workspace_floats", L);
    return rc ? rc : L.total;
}

extern "C" int satrans_esmm_fwd(const satrans_esmm_desc* d, float* out, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EsmmLayout L;
    int rc = esmm_validate(d, "esmm_fwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x && esmm_has<const float>(L, d) && out && saved, SATRANS_E_BADARG, "esmm_fwd: null pointer");
    if (L.towers == 2) return L.drop ? esmm_fwd_run<2, true>(d, L, out, saved, st) : esmm_fwd_run<2, false>(d, L, out, saved, st);
    return L.drop ? esmm_fwd_run<1, true>(d, L, out, saved, st) : esmm_fwd_run<1, false>(d, L, out, saved, st);
}

extern "C" int satrans_esmm_bwd(const satrans_esmm_desc* d, const float* dout, float* dx, const float* saved, float* workspace,
                                const satrans_esmm_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EsmmLayout L;
    int rc = esmm_validate(d, "esmm_bwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x && esmm_has<const float>(L, d) && dout && dx && saved && workspace && esmm_has<float>(L, g), SATRANS_E_BADARG,
                    "esmm_bwd: null pointer");
    set_grads(L.c, g->dnn_w, g->dnn_b, nullptr, nullptr, true);
    if (L.towers == 2)
        return L.drop ? esmm_bwd_run<2, true>(d, L, dout, dx, saved, workspace, g, st)
                      : esmm_bwd_run<2, false>(d, L, dout, dx, saved, workspace, g, st);
    return L.drop ? esmm_bwd_run<1, true>(d, L, dout, dx, saved, workspace, g, st)
                  : esmm_bwd_run<1, false>(d, L, dout, dx, saved, workspace, g, st);
}
