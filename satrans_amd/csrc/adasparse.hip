// AdaSparse's scenario-pruned DNN (reference models/adasparse.py:88-106, use_bn = False, relu, no dropout) and the bias-free logit
// layer behind it (adasparse.py:185-189).  Nothing is routed: every row uses the same weights and the scenario enters through the
// row's scenario embedding only, so there is no walker here.  A layer is a PAIR of products over one row operand,
//     fc = h W^T + b            W [N, K]
//     z  = [h | e] P^T + c      P [N, K + E]          (the concatenation is never materialised)
// followed by a discontinuous epilogue: pi = beta sigmoid(alpha z), pi = 0 where |pi| - epsilon <= 0, h' = relu(fc pi).
//
//   forward   ada_fwd_kernel                  one launch per layer: the row tile (from h for k < K, from e past it) is staged
//                                             through LDS once per contraction step and feeds two weight tiles and two MFMA
//                                             accumulators; whole steps past K skip the fc product; the epilogue writes pi,
//                                             dzf = d(fc pi)/dz and h' into `saved`
//             mmoe_gemm_kernel<false, false>  logit = h_L w^T + out_bias (head_layers.h's launch_fwd<false>, a layer with N = 1)
//   backward  the logit layer as the other heads do it (head_layers.h's launch_bwd<false>: mmoe_dw_kernel, mmoe_reduce_kernel,
//             mmoe_gemm_kernel<true, false> with the relu mask of h_L), then per layer, last to first:
//             ada_dd_kernel                   [dfc | dz] = [g pi | g dzf] [B, 2N] from the masked output gradient g
//             ada_dw_kernel                   partials of dW = dfc^T h and dP = dz^T [h | e] over chunks of kDwChunk rows: the
//                                             [h | e] tile is staged once and feeds both; the column blocks past K come from e and
//                                             skip dW; the two bias gradients ride along
//             mmoe_reduce_kernel<false>       chunks in chunk order (twice: W and b, P and c)
//             ada_din_kernel                  one launch: [dfc | dz] [W ; P] over 2N; columns [0, K) -> dh of the layer below under
//                                             its relu mask, columns [K, K + E) -> demb (written by the last layer, added to by the
//                                             layers below it, in that order)
// Every product is the k-ordered fmaf chain of grouped_gemm.h's mma_step: an element does not depend on the tile its row falls
// into.  No floating-point atomics; equal inputs give equal bits.
//
// satrans_adasparse_set_forward(1) swaps the fused forward layer for the composed form it was measured against: the fc product,
// a concatenating copy, the z product over the copy, and a pointwise epilogue (tools/adasparse_time.py).
#include "head_layers.h"

namespace satrans {
namespace {

int g_composed = 0;

__device__ __forceinline__ f32x16 zero16() {
    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    return z;
}

// The epilogue of one unit from its two pre-activations: the pruned factor pi, and dzf = d(fc pi)/dz = fc alpha pi (1 - pi / beta),
// exactly 0 where pruned.  1 - pi / beta = sigmoid(-alpha z) is taken from z: formed from the rounded pi it would lose every digit
// where nothing is pruned (pi close to beta), which is where that gradient is small but not zero.
__device__ __forceinline__ float pruned_factor(float fc, float z, float alpha, float beta, float eps, float& dzf) {
    const float az = alpha * z;
    const float pi = beta / (1.f + expf(-az));
    const bool cut = fabsf(pi) - eps <= 0.f;
    dzf = cut ? 0.f : fc * alpha * pi / (1.f + expf(az));
    return cut ? 0.f : pi;
}

// ---- forward --------------------------------------------------------------------------------------------------------------------

// grid: row tiles x n tiles.  h [B, K], e [B, E], w [N, K], p [N, K + E]; pi, dzf, out [B, N]
__global__ __launch_bounds__(kThreads) void ada_fwd_kernel(const float* __restrict__ h, const float* __restrict__ e, int B, int K, int E,
                                                           int N, int ntiles, const float* __restrict__ w, const float* __restrict__ wb,
                                                           const float* __restrict__ p, const float* __restrict__ pb, float alpha,
                                                           float beta, float eps, float* __restrict__ pi_out, float* __restrict__ dzf_out,
                                                           float* __restrict__ out) {
    __shared__ float As[kTM][kLd];
    __shared__ float Ws[kTN][kLd];
    __shared__ float Ps[kTN][kLd];
    const int n0 = (blockIdx.x % ntiles) * kTN;
    const int r0 = (blockIdx.x / ntiles) * kTM;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    const int KE = K + E;
    float ra[kPer], rw[kPer], rp[kPer];
    auto load = [&](int k0) {
        const int k = k0 + kf;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int row = r0 + if0 + 8 * q;
            float v = 0.f;
            if (row < B) {
                if (k < K)
                    v = h[(size_t)row * K + k];
                else if (k < KE)
                    v = e[(size_t)row * E + (k - K)];
            }
            ra[q] = v;
        }
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int n = n0 + if0 + 8 * q;
            rw[q] = (n < N && k < K) ? w[(size_t)n * K + k] : 0.f;
            rp[q] = (n < N && k < KE) ? p[(size_t)n * KE + k] : 0.f;
        }
    };
    f32x16 accw = zero16(), accp = zero16();
    load(0);
    for (int k0 = 0; k0 < KE; k0 += kTK) {
        __syncthreads();      // the previous step's fragment reads are done
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            As[if0 + 8 * q][kf] = ra[q];
            Ws[if0 + 8 * q][kf] = rw[q];
            Ps[if0 + 8 * q][kf] = rp[q];
        }
        __syncthreads();
        if (k0 + kTK < KE) load(k0 + kTK);
        if (k0 < K) mma_step(As, Ws, lane, wm, wn, accw);      // a whole step past K holds zeros of W only
        mma_step(As, Ps, lane, wm, wn, accp);
    }
    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= N) return;
    const float bw = wb[n], bp = pb[n];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = r0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (row >= B) continue;
        const float fc = accw[q] + bw;
        float dzf;
        const float pi = pruned_factor(fc, accp[q] + bp, alpha, beta, eps, dzf);
        const size_t at = (size_t)row * N + n;
        pi_out[at] = pi;
        dzf_out[at] = dzf;
        out[at] = fmaxf(fc * pi, 0.f);
    }
}

// the composed form's two pointwise kernels: cat = [h | e], and the epilogue over (fc, z) with z in pi's place and fc in dzf's
__global__ __launch_bounds__(kThreads) void ada_cat_kernel(const float* __restrict__ h, const float* __restrict__ e, int64_t total, int K,
                                                           int E, float* __restrict__ cat) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t row = i / (K + E);
    const int k = (int)(i % (K + E));
    cat[i] = k < K ? h[row * K + k] : e[row * E + (k - K)];
}

__global__ __launch_bounds__(kThreads) void ada_epilogue_kernel(float* __restrict__ fc, float* __restrict__ pi, int64_t total,
                                                                float alpha, float beta, float eps, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const float v = fc[i];
    float dzf;
    const float f = pruned_factor(v, pi[i], alpha, beta, eps, dzf);
    pi[i] = f;
    fc[i] = dzf;
    out[i] = fmaxf(v * f, 0.f);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------

// dd [B, 2N]: columns [0, N) dfc = g pi, columns [N, 2N) dz = g dzf (dzf = fc alpha pi (1 - pi / beta), exactly 0 where pruned).
// g is the output gradient already under the relu mask (fc pi > 0), or (when hmask) put under it here: hmask = the layer's output.
__global__ __launch_bounds__(kThreads) void ada_dd_kernel(const float* __restrict__ g, const float* __restrict__ hmask,
                                                          const float* __restrict__ pi,
                                                          const float* __restrict__ dzf, int64_t total, int N, float* __restrict__ dd) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t row = i / N;
    const int n = (int)(i % N);
    const float gv = (!hmask || hmask[i] > 0.f) ? g[i] : 0.f, pv = pi[i];
    float* o = dd + row * 2 * N + n;
    o[0] = gv * pv;
    o[N] = pv != 0.f ? gv * dzf[i] : 0.f;
}

// unit = a chunk of kDwChunk rows; part_w[u][n, c] (c < K) = sum over the chunk's rows of dfc[row, n] h[row, c];
// part_p[u][n, c] (c < K + E) = sum of dz[row, n] [h | e][row, c]; part_b[u][n], part_c[u][n] the sums of dfc and dz.
// grid: chunks x n tiles x column tiles of K + E
__global__ __launch_bounds__(kThreads) void ada_dw_kernel(const float* __restrict__ dd, const float* __restrict__ h,
                                                          const float* __restrict__ e, int B, int K, int E, int N, int ntiles, int ktiles,
                                                          float* __restrict__ part_w, float* __restrict__ part_b,
                                                          float* __restrict__ part_p, float* __restrict__ part_c) {
    __shared__ float Fs[kTM][kLd];      // dfc [n][row of the step]
    __shared__ float Zs[kTM][kLd];      // dz  [n][row of the step]
    __shared__ float Bs[kTN][kLd];      // [h | e] [c][row of the step]
    const int per_unit = ntiles * ktiles;
    const int unit = blockIdx.x / per_unit, rem = blockIdx.x % per_unit;
    const int n0 = (rem / ktiles) * kTM, c0 = (rem % ktiles) * kTN;
    const int r0 = unit * kDwChunk, r1 = min(r0 + kDwChunk, B);
    const int KE = K + E, ldd = 2 * N;
    const bool with_w = c0 < K;      // a column block of e only has no part of dW
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int jf = t & 63, kf0 = t >> 6;      // "i fast"
    float rf[kPer], rz[kPer], rb[kPer];
    auto load = [&](int p0) {
        const int n = n0 + jf, c = c0 + jf;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int row = p0 + kf0 + 4 * q;
            const bool ok = row < r1;
            rf[q] = (ok && n < N && with_w) ? dd[(size_t)row * ldd + n] : 0.f;
            rz[q] = (ok && n < N) ? dd[(size_t)row * ldd + N + n] : 0.f;
            float v = 0.f;
            if (ok) {
                if (c < K)
                    v = h[(size_t)row * K + c];
                else if (c < KE)
                    v = e[(size_t)row * E + (c - K)];
            }
            rb[q] = v;
        }
    };
    f32x16 accw = zero16(), accp = zero16();
    float bsum = 0.f;
    load(r0);
    for (int p0 = r0; p0 < r1; p0 += kTK) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            Fs[jf][kf0 + 4 * q] = rf[q];
            Zs[jf][kf0 + 4 * q] = rz[q];
            Bs[jf][kf0 + 4 * q] = rb[q];
        }
        __syncthreads();
        if (p0 + kTK < r1) load(p0 + kTK);
        if (c0 == 0 && t < 2 * kTM) {      // the bias gradients: rows of the chunk in order (rows past its end hold zeros)
            const float* src = t < kTM ? Fs[t] : Zs[t - kTM];
#pragma unroll
            for (int kk = 0; kk < kTK; ++kk) bsum += src[kk];
        }
        if (with_w) mma_step(Fs, Bs, lane, wm, wn, accw);
        mma_step(Zs, Bs, lane, wm, wn, accp);
    }
    if (c0 == 0 && t < 2 * kTM) {
        const int n = n0 + (t & (kTM - 1));
        if (n < N) (t < kTM ? part_b : part_c)[(size_t)unit * N + n] = bsum;
    }
    const int c = c0 + wn * 32 + (lane & 31);
    if (c >= KE) return;
    float* ow = part_w + (size_t)unit * N * K;
    float* op = part_p + (size_t)unit * N * KE;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int n = n0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (n >= N) continue;
        if (c < K) ow[(size_t)n * K + c] = accw[q];
        op[(size_t)n * KE + c] = accp[q];
    }
}

// out[row, c] = sum_{j < N} dfc[row, j] W[j, c] (c < K) + sum_{j < N} dz[row, j] P[j, c], one chain over 2N in that order.
// c < K: din[row, c], times (mask[row, c] > 0) when mask;  K <= c < K + E: de[row, c - K], added to what it holds when add.
// grid: row tiles x column tiles of K + E
__global__ __launch_bounds__(kThreads) void ada_din_kernel(const float* __restrict__ dd, int B, int K, int E, int N, int ctiles,
                                                           const float* __restrict__ w, const float* __restrict__ p,
                                                           const float* __restrict__ mask, int add, float* __restrict__ din,
                                                           float* de) {
    __shared__ float As[kTM][kLd];
    __shared__ float Bs[kTN][kLd];
    const int c0 = (blockIdx.x % ctiles) * kTN;
    const int r0 = (blockIdx.x / ctiles) * kTM;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int kf = t & 31, if0 = t >> 5;      // "k fast": the row operand
    const int jf = t & 63, kf0 = t >> 6;      // "i fast": the weights, [j][c] with c contiguous
    const int KE = K + E, N2 = 2 * N;
    float ra[kPer], rb[kPer];
    auto load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int row = r0 + if0 + 8 * q, k = k0 + kf;
            ra[q] = (row < B && k < N2) ? dd[(size_t)row * N2 + k] : 0.f;
        }
        const int c = c0 + jf;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int k = k0 + kf0 + 4 * q;
            float v = 0.f;
            if (k < N) {
                if (c < K) v = w[(size_t)k * K + c];
            } else if (k < N2 && c < KE) {
                v = p[(size_t)(k - N) * KE + c];
            }
            rb[q] = v;
        }
    };
    f32x16 acc = zero16();
    // a tile of demb columns only: W contributes exact zeros there, so the whole steps inside [0, N) are left out
    const int kbegin = c0 >= K ? (N / kTK) * kTK : 0;
    load(kbegin);
    for (int k0 = kbegin; k0 < N2; k0 += kTK) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            As[if0 + 8 * q][kf] = ra[q];
            Bs[jf][kf0 + 4 * q] = rb[q];
        }
        __syncthreads();
        if (k0 + kTK < N2) load(k0 + kTK);
        mma_step(As, Bs, lane, wm, wn, acc);
    }
    const int c = c0 + wn * 32 + (lane & 31);
    if (c >= KE) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = r0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (row >= B) continue;
        float v = acc[q];
        if (c < K) {
            const size_t at = (size_t)row * K + c;
            if (mask) v = mask[at] > 0.f ? v : 0.f;
            din[at] = v;
        } else {
            const size_t at = (size_t)row * E + (c - K);
            de[at] = add ? de[at] + v : v;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

struct AdaLayout {
    int nl;
    int K[kMaxH], N[kMaxH];
    Rows rows;      // nothing is routed: T = 0, no order, no seg
    int64_t s_pi[kMaxH], s_fc[kMaxH], s_h[kMaxH], s_cat, saved;      // floats from the start of saved (s_fc: dzf)
    int64_t max_w, w_g, w_dd, w_part, total;                         // workspace
};

int ada_validate(const satrans_adasparse_desc* d, const char* who, AdaLayout& L) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->C > 0 && d->E > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d C=%d E=%d", who, d->B, d->C, d->E);
    SATRANS_REQUIRE(d->n_layers >= 1 && d->n_layers <= kMaxH, SATRANS_E_BADARG, "%s: bad sizes: %d layers (1 to %d)", who, d->n_layers,
                    kMaxH);
    for (int l = 0; l < d->n_layers; ++l)
        SATRANS_REQUIRE(d->width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes width[%d]=%d", who, l, d->width[l]);
    SATRANS_REQUIRE(d->beta > 0.f && d->epsilon >= 0.f && d->alpha == d->alpha, SATRANS_E_BADARG,
                    "%s: bad constants alpha=%g beta=%g epsilon=%g (beta > 0, epsilon >= 0)", who, (double)d->alpha, (double)d->beta,
                    (double)d->epsilon);
    const int64_t B = d->B, E = d->E;
    L.nl = d->n_layers;
    L.rows = rows_of(d->B, 0, nullptr, nullptr);
    int64_t at = 0, per_part = 0, max_ke = 0;
    L.max_w = 1;
    int prev = d->C;
    for (int l = 0; l < L.nl; ++l) {
        const int64_t K = prev, N = d->width[l], KE = K + E;
        SATRANS_REQUIRE(KE <= 0x7fffffffLL / 4 && N <= 0x7fffffffLL / 8 && N * KE <= 0x7fffffffLL &&
                            L.rows.tiles * ceil_div(std::max(N, KE), kTN) <= 0x7fffffffLL &&
                            L.rows.chunks * ceil_div(N, kTM) * ceil_div(KE, kTN) <= 0x7fffffffLL,
                        SATRANS_E_UNSUPPORTED, "%s: layer %d (%lld x %lld) at B=%d needs more than 2^31 workgroups", who, l, (long long)N,
                        (long long)KE, d->B);
        L.K[l] = (int)K, L.N[l] = (int)N;
        L.s_pi[l] = at, L.s_fc[l] = at + B * N, L.s_h[l] = at + 2 * B * N;
        at += 3 * B * N;
        L.max_w = std::max(L.max_w, N);
        max_ke = std::max(max_ke, KE);
        per_part = std::max(per_part, L.rows.chunks * (N * (K + 1) + N * (KE + 1)));
        prev = (int)N;
    }
    per_part = std::max(per_part, L.rows.chunks * ((int64_t)prev + 1));      // the logit layer
    L.s_cat = at;
    if (g_composed) at += B * max_ke;
    L.saved = at;
    L.w_g = 0;
    L.w_dd = 2 * B * L.max_w;
    L.w_part = L.w_dd + 2 * B * L.max_w;
    L.total = L.w_part + per_part;
    return SATRANS_OK;
}

bool ada_has_operands(const satrans_adasparse_desc* d) {
    if (!d->x || !d->emb || !d->final_w != !d->out_bias) return false;      // neither final_w nor out_bias: the DNN alone
    for (int l = 0; l < d->n_layers; ++l)
        if (!d->lin_w[l] || !d->lin_b[l] || !d->prn_w[l] || !d->prn_b[l]) return false;
    return true;
}

bool ada_has_grads(const satrans_adasparse_desc* d, const satrans_adasparse_grads* g) {
    if (!g || (d->final_w && (!g->final_w || !g->out_bias))) return false;
    for (int l = 0; l < d->n_layers; ++l)
        if (!g->lin_w[l] || !g->lin_b[l] || !g->prn_w[l] || !g->prn_b[l]) return false;
    return true;
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int satrans_adasparse_set_forward(int composed) {
    SATRANS_REQUIRE(composed == 0 || composed == 1, SATRANS_E_BADARG, "adasparse_set_forward: mode %d (0 fused, 1 composed)", composed);
    const int was = g_composed;
    g_composed = composed;
    return was;
}

extern "C" int64_t satrans_adasparse_saved_floats(const satrans_adasparse_desc* d) {
    AdaLayout L;
    const int rc = ada_validate(d, "adasparse_saved_floats", L);
    return rc ? rc : L.saved;
}

extern "C" int64_t satrans_adasparse_workspace_floats(const satrans_adasparse_desc* d) {
    AdaLayout L;
    const int rc = ada_validate(d, "adasparse_workspace_floats", L);
    return rc ? rc : L.total;
}

extern "C" int satrans_adasparse_fwd(const satrans_adasparse_desc* d, float* logit, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    AdaLayout L;
    int rc = ada_validate(d, "adasparse_fwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(ada_has_operands(d) && (logit || !d->final_w) && saved, SATRANS_E_BADARG, "adasparse_fwd: null pointer");
    const int B = d->B, E = d->E;
    const float* in = d->x;
    for (int l = 0; l < L.nl; ++l) {
        const int K = L.K[l], N = L.N[l];
        float *pi = saved + L.s_pi[l], *fc = saved + L.s_fc[l], *out = saved + L.s_h[l];
        if (g_composed) {
            float* cat = saved + L.s_cat;
            const int64_t nc = (int64_t)B * (K + E), no = (int64_t)B * N;
            const Lyr lin{K, N, 1, d->lin_w[l], d->lin_b[l], nullptr, nullptr};
            const Lyr prn{K + E, N, 1, d->prn_w[l], d->prn_b[l], nullptr, nullptr};
            if ((rc = launch_fwd<false>(L.rows, lin, in, K, 0, 0, fc, N, 0, st))) return rc;
            ada_cat_kernel<<<(unsigned)ceil_div(nc, kThreads), kThreads, 0, st>>>(in, d->emb, nc, K, E, cat);
            SATRANS_CHECK_LAUNCH("ada_cat_kernel");
            if ((rc = launch_fwd<false>(L.rows, prn, cat, K + E, 0, 0, pi, N, 0, st))) return rc;
            ada_epilogue_kernel<<<(unsigned)ceil_div(no, kThreads), kThreads, 0, st>>>(fc, pi, no, d->alpha, d->beta, d->epsilon, out);
            SATRANS_CHECK_LAUNCH("ada_epilogue_kernel");
        } else {
            const int ntiles = (int)ceil_div(N, kTN);
            ada_fwd_kernel<<<(unsigned)(L.rows.tiles * ntiles), kThreads, 0, st>>>(in, d->emb, B, K, E, N, ntiles, d->lin_w[l],
                                                                                  d->lin_b[l], d->prn_w[l], d->prn_b[l], d->alpha, d->beta,
                                                                                  d->epsilon, pi, fc, out);
            SATRANS_CHECK_LAUNCH("ada_fwd_kernel");
        }
        in = out;
    }
    if (!d->final_w) return SATRANS_OK;      // the DNN alone: h_L is the last block of saved
    const Lyr fin{L.N[L.nl - 1], 1, 1, d->final_w, d->out_bias, nullptr, nullptr};
    return launch_fwd<false>(L.rows, fin, in, fin.K, 0, 0, logit, 1, 0, st);
}

extern "C" int satrans_adasparse_bwd(const satrans_adasparse_desc* d, const float* dlogit, float* dx, float* demb, const float* saved,
                                     float* workspace, const satrans_adasparse_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    AdaLayout L;
    int rc = ada_validate(d, "adasparse_bwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(ada_has_operands(d) && dlogit && dx && demb && saved && workspace && ada_has_grads(d, g), SATRANS_E_BADARG,
                    "adasparse_bwd: null pointer");
    const int B = d->B, E = d->E, chunks = (int)L.rows.chunks;
    float* gbuf[2] = {workspace + L.w_g, workspace + L.w_g + (size_t)B * L.max_w};
    float* dd = workspace + L.w_dd;
    float* part = workspace + L.w_part;
    int cur = 0;
    const float* gin = dlogit;      // the DNN alone: dlogit is dh_L [B, n_L], put under h_L's relu mask by the first ada_dd_kernel
    if (d->final_w) {   // the logit layer: d final_w = dlogit^T h_L, d out_bias = sum dlogit, g_L = dlogit final_w under the relu mask of h_L
        const Lyr fin{L.N[L.nl - 1], 1, 1, d->final_w, d->out_bias, g->final_w, g->out_bias};
        if ((rc = launch_bwd<false>(L.rows, fin, dlogit, 1, saved + L.s_h[L.nl - 1], fin.K, 0, true, 0, gbuf[cur], part, st))) return rc;
        gin = gbuf[cur];
    }
    for (int l = L.nl - 1; l >= 0; --l) {
        const int K = L.K[l], N = L.N[l], KE = K + E;
        const float* hin = l > 0 ? saved + L.s_h[l - 1] : d->x;
        const int64_t no = (int64_t)B * N;
        ada_dd_kernel<<<(unsigned)ceil_div(no, kThreads), kThreads, 0, st>>>(gin, gin == dlogit ? saved + L.s_h[l] : nullptr, saved + L.s_pi[l],
                                                                            saved + L.s_fc[l], no, N, dd);
        SATRANS_CHECK_LAUNCH("ada_dd_kernel");
        const int ntiles = (int)ceil_div(N, kTM), ktiles = (int)ceil_div(KE, kTN);
        float* part_w = part;
        float* part_b = part_w + (size_t)chunks * N * K;
        float* part_p = part_b + (size_t)chunks * N;
        float* part_c = part_p + (size_t)chunks * N * KE;
        ada_dw_kernel<<<(unsigned)(chunks * ntiles * ktiles), kThreads, 0, st>>>(dd, hin, d->emb, B, K, E, N, ntiles, ktiles, part_w, part_b,
                                                                                part_p, part_c);
        SATRANS_CHECK_LAUNCH("ada_dw_kernel");
        const int64_t NK = (int64_t)N * K, NKE = (int64_t)N * KE;
        mmoe_reduce_kernel<false><<<(unsigned)ceil_div(NK + N, kThreads), kThreads, 0, st>>>(part_w, part_b, nullptr, B, NK, N, 0, 1, 1, chunks,
                                                                                            g->lin_w[l], g->lin_b[l]);
        SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel (adasparse linears)");
        mmoe_reduce_kernel<false><<<(unsigned)ceil_div(NKE + N, kThreads), kThreads, 0, st>>>(part_p, part_c, nullptr, B, NKE, N, 0, 1, 1,
                                                                                             chunks, g->prn_w[l], g->prn_b[l]);
        SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel (adasparse pruners)");
        float* din = l > 0 ? gbuf[cur ^ 1] : dx;
        ada_din_kernel<<<(unsigned)(L.rows.tiles * ktiles), kThreads, 0, st>>>(dd, B, K, E, N, ktiles, d->lin_w[l], d->prn_w[l],
                                                                         l > 0 ? hin : nullptr, l < L.nl - 1, din, demb);
        SATRANS_CHECK_LAUNCH("ada_din_kernel");
        cur ^= 1;
        gin = gbuf[cur];
    }
    return SATRANS_OK;
}
