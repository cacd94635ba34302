// PNN (deepctr-torch 0.2.9's InnerProductLayer and OutterProductLayer, which the reference's models/pnn.py:14,61,65 calls, and the
// half of PNN.forward behind the lookup, pnn.py:91-114).  e [B, F, D]; pairs (i, j), i < j, in itertools.combinations order, pair
// p = i (2 F - i - 1) / 2 + j - i - 1, P = F (F - 1) / 2; K_p = kernel[:, p, :] of the 'mat' kernel [D, P, D], row n at
// kernel + (n P + p) D, read in place.
//     inner        ip[b,p] = <e_i, e_j>
//     outer 'mat'  op[b,p] = <K_p e_i, e_j>          'vec'  op[b,p] = sum_d e_i[d] e_j[d] kernel[p,d]          'num'  kernel[p] <e_i, e_j>
//     head         x = [ flatten(e) | ip | op | dense ]    the DNN, dnn_linear, out.bias       logit [B, 1]
// Backward, g_p[b] the gradient of one product column:
//     pointwise    de_i += g_p c_p * e_j    de_j += g_p c_p * e_i    c_p = 1 (inner), kernel[p] ('num'), kernel[p,:] ('vec')
//     'mat'        de_j += K_p (g_p e_i)    de_i += K_p^T (g_p e_j)   dkernel[n,p,k] = sum_b g_p e_j[n] e_i[k]
//
// pnn_point_fwd_kernel     workgroup = one row: its F D floats once into LDS (rows of odd stride), copied into the linear block of x;
//                          then a thread per pair, d ascending: ip and the 'vec' / 'num' op from the same read, straight into x.
// pnn_mat_fwd_kernel       workgroup = (64 rows) x (field i): e_i staged ONCE, all of its k steps; partners j > i ascending stream
//                          K_p through grouped_gemm.h's tile product (mma_step, v_mfma_f32_32x32x2_f32, steps of 32 over D).  The
//                          epilogue stays in the accumulators: times e_j, a fixed butterfly over the 32 columns of the wave's
//                          quadrant, the quadrants' sums (both column tiles at D > 64) through LDS in a fixed order, one float per
//                          row and pair into x.  At D <= 32 a pass takes TWO partners, the second in the tile's columns 32..,
//                          which would multiply zeros otherwise.  The result is 1 / D of fibinet_bil_fwd_kernel's.
// pnn_mat_dx_kernel        workgroup = (64 rows) x (field f) x (64 columns of D), the only writer of its de tile.  g_p is a scalar
//                          per row, so it is folded into the row operand on load and BOTH directions go into one set of MFMA
//                          accumulators: partners i < f ascending acc += (g_p e_i) K_p^T, then partners j > f ascending
//                          acc += (g_p e_j) K_p.  The pointwise gradients (inner) and the gradient of x's linear block are summed by
//                          the same owner in the operand loader's registers (e_o is there already) and join the accumulators
//                          through LDS: demb is written once.  The three 'mat' kernels fetch the next step's operands before
//                          the current step's MFMAs.
// pnn_point_dx_kernel      without 'mat': a thread per de element, partners ascending.
// pnn_mat_dk_kernel        workgroup = (chunk of SATRANS_PNN_DW_ROW_CHUNK rows) x (pair p) x (64 x 64 tile of [D, D]); partials in
//                          the [D, P, D] layout per chunk, merged in chunk order by mmoe_reduce_kernel<false>.
// pnn_point_dk_kernel      'vec' / 'num': a thread per (p, d) sums the chunk's rows in order; 'vec' partials [chunk][P D]; 'num'
//                          partials [chunk][d][P], so that the same ordered merge also sums over d.
// The DNN is head_layers.h's dense launcher (dnn_fwd<false> / dnn_bwd<false>) with dnn_linear as the one-column final layer and
// out.bias as that layer's bias.
// No floating-point atomics; every sum has a fixed order; a row's results do not depend on its place in a tile.  fp32 only.
#include "head_layers.h"
#include "pair_index.h"

namespace satrans {
namespace {

constexpr int kPnnF = SATRANS_PNN_MAX_FIELDS;
constexpr int kPnnD = SATRANS_PNN_MAX_DIM;
constexpr int kPnnChunk = SATRANS_PNN_DW_ROW_CHUNK;
constexpr int kPnnSteps = (kPnnD + kTK - 1) / kTK;      // k steps of a staged e_i
constexpr int kPnnTiles = (kPnnD + kTN - 1) / kTN;      // column tiles of K_p
constexpr int kPnnRow = kPnnF * (kPnnD | 1);            // floats of a row in LDS, rows of odd stride
static_assert(kPnnChunk % kTK == 0, "row steps");
static_assert(kPnnRow * sizeof(float) <= 48 * 1024, "a row in LDS");

// row of the wave's accumulator q (the 32 x 32 quadrant wm of the tile)
__device__ __forceinline__ int acc_row(int q, int lane, int wm) { return wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5); }

// ---- pointwise ------------------------------------------------------------------------------------------------------------------

// grid: B.  x rows of ld floats: flatten(e) at column eofs, ip at iofs, the 'vec' / 'num' op at oofs (each when >= 0).
__global__ __launch_bounds__(kThreads) void pnn_point_fwd_kernel(const float* __restrict__ e, const float* __restrict__ kern, int F, int D,
                                                                 int P, int ktype, float* __restrict__ x, int ld, int eofs, int iofs,
                                                                 int oofs) {
    __shared__ float sh[kPnnRow];
    const size_t row = blockIdx.x;
    const int t = threadIdx.x, FD = F * D, Dp = D | 1;
    const float* er = e + row * FD;
    float* xr = x + row * ld;
    for (int idx = t; idx < FD; idx += kThreads) {
        const float v = er[idx];
        sh[(idx / D) * Dp + idx % D] = v;
        if (eofs >= 0) xr[eofs + idx] = v;
    }
    if (iofs < 0 && oofs < 0) return;
    __syncthreads();
    for (int p = t; p < P; p += kThreads) {
        int i, j;
        pair_fields(p, F, i, j);
        const float* ei = sh + i * Dp;
        const float* ej = sh + j * Dp;
        float ip = 0.f, op = 0.f;
        if (oofs >= 0 && ktype == SATRANS_PNN_KERNEL_VEC) {
            const float* kp = kern + (size_t)p * D;
            for (int d = 0; d < D; ++d) {
                const float pq = ei[d] * ej[d];
                ip += pq;
                op = fmaf(pq, kp[d], op);
            }
        } else {
            for (int d = 0; d < D; ++d) ip = fmaf(ei[d], ej[d], ip);
            if (oofs >= 0) op = kern[p] * ip;
        }
        if (iofs >= 0) xr[iofs + p] = ip;
        if (oofs >= 0) xr[oofs + p] = op;
    }
}

// de[row, f, d] of the pointwise products and of x's linear block: dx rows of ld floats in the forward's layout (a block at a
// negative column is absent); partners o != f ascending.
__device__ __forceinline__ float point_grad(const float* __restrict__ e, const float* __restrict__ kern, const float* __restrict__ dx,
                                            size_t row, int F, int D, int ktype, int ld, int eofs, int iofs, int oofs, int f, int d) {
    const float* g = dx + row * ld;
    const float* er = e + row * F * D + d;
    float s = eofs >= 0 ? g[eofs + f * D + d] : 0.f;
    if (iofs < 0 && oofs < 0) return s;
    for (int o = 0; o < F; ++o) {
        if (o == f) continue;
        const int p = o < f ? pair_index(o, f, F) : pair_index(f, o, F);
        float c = iofs >= 0 ? g[iofs + p] : 0.f;
        if (oofs >= 0) c = fmaf(g[oofs + p], ktype == SATRANS_PNN_KERNEL_VEC ? kern[(size_t)p * D + d] : kern[p], c);
        s = fmaf(c, er[(size_t)o * D], s);
    }
    return s;
}

// grid: ceil(B F D / 256).  de [B, F, D] written.
__global__ __launch_bounds__(kThreads) void pnn_point_dx_kernel(const float* __restrict__ e, const float* __restrict__ kern,
                                                                const float* __restrict__ dx, int64_t total, int F, int D, int ktype,
                                                                int ld, int eofs, int iofs, int oofs, float* __restrict__ de) {
    const int64_t el = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (el >= total) return;
    const int d = (int)(el % D), f = (int)(el / D % F);
    de[el] = point_grad(e, kern, dx, (size_t)(el / D / F), F, D, ktype, ld, eofs, iofs, oofs, f, d);
}

// grid: chunks x ceil(P D / 256).  'vec': part[chunk][p D + d];  'num': part[chunk D + d][p]  =  the chunk's rows in order of
// g_p e_i[d] e_j[d].  g_p = dx[row, oofs + p].
__global__ __launch_bounds__(kThreads) void pnn_point_dk_kernel(const float* __restrict__ e, const float* __restrict__ dx, int B, int F,
                                                                int D, int P, int ktype, int ld, int oofs, int per_chunk,
                                                                float* __restrict__ part) {
    const int chunk = blockIdx.x / per_chunk;
    const int el = (blockIdx.x % per_chunk) * kThreads + threadIdx.x;
    if (el >= P * D) return;
    const int p = el / D, d = el % D;
    int i, j;
    pair_fields(p, F, i, j);
    const int64_t r0 = (int64_t)chunk * kPnnChunk;
    const int64_t r1 = r0 + kPnnChunk < B ? r0 + kPnnChunk : B;
    float sum = 0.f;
    for (int64_t row = r0; row < r1; ++row) {
        const float* er = e + (size_t)row * F * D + d;
        sum = fmaf(dx[(size_t)row * ld + oofs + p], er[(size_t)i * D] * er[(size_t)j * D], sum);
    }
    if (ktype == SATRANS_PNN_KERNEL_VEC)
        part[(size_t)chunk * P * D + el] = sum;
    else
        part[((size_t)chunk * D + d) * P + p] = sum;
}

// ---- 'mat' ----------------------------------------------------------------------------------------------------------------------

// grid: row tiles x (F - 1).  x[row, oofs + p] = <K_p e_i, e_j> for the partners j of field i = blockIdx.x % (F - 1).
__global__ __launch_bounds__(kThreads) void pnn_mat_fwd_kernel(const float* __restrict__ e, const float* __restrict__ kern, int B, int F,
                                                               int D, int P, float* __restrict__ x, int ld, int oofs) {
    __shared__ float As[kPnnSteps][kTM][kLd];      // e_i, every k step
    __shared__ float Bs[kTN][kLd];
    __shared__ float red[2 * kPnnTiles][kTM];      // [column tile, wave column][row]: the quadrants' sums of a pair
    const int i = blockIdx.x % (F - 1);
    const int64_t r0 = (int64_t)(blockIdx.x / (F - 1)) * kTM;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    const int steps = (D + kTK - 1) / kTK, ntiles = (D + kTN - 1) / kTN;
    for (int s = 0; s < steps; ++s) {
        const int k = s * kTK + kf;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int64_t row = r0 + if0 + 8 * q;
            As[s][if0 + 8 * q][kf] = (row < B && k < D) ? e[((size_t)row * F + i) * D + k] : 0.f;
        }
    }
    // D <= 32 (one k step, half a column tile): the tile's columns 32.. take the NEXT partner, whose pair index is the next
    // one, so that no wave multiplies zeros; every pair then has one quadrant sum per row.
    const bool narrow = D <= kTK;
    const int jstep = narrow ? 2 : 1;
    // the next step's K_p tile is fetched before the current step's MFMAs
    float rb[kPer];
    auto fetch = [&](int j, int tile, int s) {
        const int k = s * kTK + kf;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int r = if0 + 8 * q;
            const int jj = narrow ? j + (r >> 5) : j, n = narrow ? r & 31 : tile * kTN + r;
            rb[q] = (jj < F && n < D && k < D) ? kern[((size_t)n * P + pair_index(i, jj, F)) * D + k] : 0.f;
        }
    };
    fetch(i + 1, 0, 0);
    for (int j = i + 1; j < F; j += jstep) {
        const int p = pair_index(i, j, F);
        for (int tile = 0; tile < ntiles; ++tile) {
            const int jj = narrow ? j + wn : j;
            const int col = narrow ? lane & 31 : tile * kTN + wn * 32 + (lane & 31);
            float ej[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t row = r0 + acc_row(q, lane, wm);
                ej[q] = (row < B && col < D && jj < F) ? e[((size_t)row * F + jj) * D + col] : 0.f;
            }
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < steps; ++s) {
                __syncthreads();      // the previous step's fragment reads (and the first time, e_i's staging) are done
#pragma unroll
                for (int q = 0; q < kPer; ++q) Bs[if0 + 8 * q][kf] = rb[q];
                __syncthreads();
                if (s + 1 < steps)
                    fetch(j, tile, s + 1);
                else if (tile + 1 < ntiles)
                    fetch(j, tile + 1, 0);
                else if (j + jstep < F)
                    fetch(j + jstep, 0, 0);
                mma_step(As[s], Bs, lane, wm, wn, acc);
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {      // over the quadrant's 32 columns: the same tree in every lane
                float v = acc[q] * ej[q];
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
                if ((lane & 31) == 0) red[2 * tile + wn][acc_row(q, lane, wm)] = v;
            }
        }
        __syncthreads();
        if (t < kTM && r0 + t < B) {
            float* out = x + (size_t)(r0 + t) * ld + oofs + p;
            if (narrow) {
                out[0] = red[0][t];
                if (j + 1 < F) out[1] = red[1][t];
            } else {
                float sum = 0.f;
                for (int u = 0; u < 2 * ntiles; ++u) sum += red[u][t];
                out[0] = sum;
            }
        }
        // (the next pass writes red only behind the barriers of its k steps)
    }
}

// grid: row tiles x F x ntiles.  de [B, F, D] written.  dx rows of ld floats in the forward's layout: g_p = dx[row, oofs + p]; the
// inner products' gradient at iofs and the linear block's at eofs (each when >= 0).  The partners o != f ascending, each over its
// k steps; the next step's operands are fetched before the current step's MFMAs.  The loader that fetches e_o[row, k] for the
// row operand also owns the pointwise sum of (row, column k) when k lies in the workgroup's columns - ps, started from the
// linear block's gradient - so the inner products cost one more fmaf on a value already in a register.
__global__ __launch_bounds__(kThreads) void pnn_mat_dx_kernel(const float* __restrict__ e, const float* __restrict__ kern,
                                                              const float* __restrict__ dx, int B, int F, int D, int P, int ntiles,
                                                              int ld, int eofs, int iofs, int oofs, float* __restrict__ de) {
    __shared__ float As[kTM][kLd];
    __shared__ float Bs[kTN][kLd];
    __shared__ float Cs[kTM][kTN + 1];      // ps on its way to the accumulators' layout
    const int n0 = (blockIdx.x % ntiles) * kTN;
    const int f = (blockIdx.x / ntiles) % F;
    const int64_t r0 = (int64_t)(blockIdx.x / ntiles / F) * kTM;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    const int jf = t & 63, kf0 = t >> 6;      // "i fast"
    float ra[kPer], rb[kPer], ps[2][kPer];    // ps[h][q]: row if0 + 8 q, column n0 + 32 h + kf
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int64_t row = r0 + if0 + 8 * q;
            const int col = n0 + kTK * h + kf;
            ps[h][q] = (eofs >= 0 && row < B && col < D) ? dx[(size_t)row * ld + eofs + f * D + col] : 0.f;
        }
    // o < f: f is the pair's second field, de_f[n] += sum_k K_p[n, k] (g_p e_o[k]);  o > f: its first, de_f[k] += sum_n (g_p e_o[n]) K_p[n, k]
    auto fetch = [&](int o, int k0) {
        const bool second = o < f;
        const int p = second ? pair_index(o, f, F) : pair_index(f, o, F);
        const int k = k0 + kf;
        const bool mine = k0 >= n0 && k0 < n0 + kTN, upper = k0 > n0;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int64_t row = r0 + if0 + 8 * q;
            float ev = 0.f, g = 0.f, gi = 0.f;
            if (row < B && k < D) {
                ev = e[((size_t)row * F + o) * D + k];
                g = dx[(size_t)row * ld + oofs + p];
                if (iofs >= 0) gi = dx[(size_t)row * ld + iofs + p];
            }
            ra[q] = g * ev;
            if (mine) {
                if (upper)
                    ps[1][q] = fmaf(gi, ev, ps[1][q]);
                else
                    ps[0][q] = fmaf(gi, ev, ps[0][q]);
            }
            if (second) {
                const int nn = n0 + if0 + 8 * q;
                rb[q] = (nn < D && k < D) ? kern[((size_t)nn * P + p) * D + k] : 0.f;
            } else {
                const int nn = n0 + jf, kk = k0 + kf0 + 4 * q;
                rb[q] = (nn < D && kk < D) ? kern[((size_t)kk * P + p) * D + nn] : 0.f;
            }
        }
    };
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int o = f == 0 ? 1 : 0, k0 = 0;
    fetch(o, k0);
    while (true) {
        __syncthreads();      // the previous step's fragment reads are done
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            As[if0 + 8 * q][kf] = ra[q];
            if (o < f)
                Bs[if0 + 8 * q][kf] = rb[q];
            else
                Bs[jf][kf0 + 4 * q] = rb[q];
        }
        __syncthreads();
        int no = o, nk = k0 + kTK;
        if (nk >= D) {
            nk = 0;
            no = o + 1 == f ? o + 2 : o + 1;
        }
        if (no < F) fetch(no, nk);
        mma_step(As, Bs, lane, wm, wn, acc);
        if (no >= F) break;
        o = no, k0 = nk;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < kPer; ++q) Cs[if0 + 8 * q][kTK * h + kf] = ps[h][q];
    __syncthreads();
    const int cl = wn * 32 + (lane & 31);
    if (n0 + cl >= D) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int rl = acc_row(q, lane, wm);
        if (r0 + rl < B) de[((size_t)(r0 + rl) * F + f) * D + n0 + cl] = acc[q] + Cs[rl][cl];
    }
}

// grid: chunks x P x (ntiles x ntiles).  part [chunks][D, P, D]:  part[c][n, p, k] = sum over the chunk's rows of
// (g_p e_j)[row, n] e_i[row, k].
__global__ __launch_bounds__(kThreads) void pnn_mat_dk_kernel(const float* __restrict__ e, const float* __restrict__ dx, int B, int F,
                                                              int D, int P, int ntiles, int ld, int oofs, float* __restrict__ part) {
    __shared__ float As[kTM][kLd];      // [n][row of the step]
    __shared__ float Bs[kTN][kLd];      // [k][row of the step]
    const int per_unit = ntiles * ntiles;
    const int unit = blockIdx.x / per_unit, rem = blockIdx.x % per_unit;
    const int n0 = (rem / ntiles) * kTM, c0 = (rem % ntiles) * kTN;
    const int p = unit % P;
    const int64_t r0 = (int64_t)(unit / P) * kPnnChunk;
    const int64_t r1 = r0 + kPnnChunk < B ? r0 + kPnnChunk : B;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    // operand loaders as fibinet_bil_dw_kernel's: column jf of the rows kf0, kf0 + rs, .. of a step; at D <= 32 32 columns x 8 row
    // groups, so that no lane idles - the same LDS contents either way.  The next step's rows are fetched before the MFMAs.
    const bool narrow = D <= kTK;
    const int jf = narrow ? t & 31 : t & 63, kf0 = narrow ? t >> 5 : t >> 6, rs = narrow ? 8 : 4, cnt = narrow ? kPer / 2 : kPer;
    if (narrow)
        for (int idx = t; idx < kTM * kLd; idx += kThreads) (&As[0][0])[idx] = (&Bs[0][0])[idx] = 0.f;      // rows 32.. stay zero
    int i, j;
    pair_fields(p, F, i, j);
    float ra[kPer], rb[kPer];
    auto fetch = [&](int64_t p0) {
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int64_t row = p0 + kf0 + rs * q;
            const int n = n0 + jf, c = c0 + jf;
            const bool ok = q < cnt && row < r1;
            ra[q] = (ok && n < D) ? dx[(size_t)row * ld + oofs + p] * e[((size_t)row * F + j) * D + n] : 0.f;
            rb[q] = (ok && c < D) ? e[((size_t)row * F + i) * D + c] : 0.f;
        }
    };
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    fetch(r0);
    for (int64_t p0 = r0; p0 < r1; p0 += kTK) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q)
            if (q < cnt) {
                As[jf][kf0 + rs * q] = ra[q];
                Bs[jf][kf0 + rs * q] = rb[q];
            }
        __syncthreads();
        if (p0 + kTK < r1) fetch(p0 + kTK);
        mma_step(As, Bs, lane, wm, wn, acc);
    }
    const int c = c0 + wn * 32 + (lane & 31);
    if (c >= D) return;
    float* out = part + (size_t)(unit / P) * D * P * D;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int n = n0 + acc_row(q, lane, wm);
        if (n < D) out[((size_t)n * P + p) * D + c] = acc[q];
    }
}

// dst[row, dofs + c] = src[row, sofs + c], c < n: the dense columns into the DNN input, their gradient out of it
__global__ __launch_bounds__(kThreads) void pnn_cols_kernel(const float* __restrict__ src, int lds, int sofs, float* __restrict__ dst,
                                                            int ldd, int dofs, int64_t total, int n) {
    const int64_t el = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (el >= total) return;
    const int64_t row = el / n;
    const int c = (int)(el % n);
    dst[(size_t)row * ldd + dofs + c] = src[(size_t)row * lds + sofs + c];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

// the shapes of a call and what its launches need
struct Pnn {
    int B, F, D, P, ktype, ntiles;
    int64_t tiles, chunks;
    int64_t kernel_floats, part;      // the kernel of ktype; the partials of its gradient
};

int pnn_shape(Pnn& s, int B, int F, int D, int ktype, const char* who) {
    SATRANS_REQUIRE(B > 0 && F >= 2 && D > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d F=%d D=%d", who, B, F, D);
    SATRANS_REQUIRE(ktype >= SATRANS_PNN_KERNEL_MAT && ktype <= SATRANS_PNN_KERNEL_NUM, SATRANS_E_BADARG, "%s: kernel_type=%d", who, ktype);
    SATRANS_REQUIRE(F <= kPnnF && D <= kPnnD, SATRANS_E_UNSUPPORTED, "%s: F=%d fields, D=%d (at most %d, %d)", who, F, D, kPnnF, kPnnD);
    s.B = B, s.F = F, s.D = D, s.ktype = ktype;
    s.P = F * (F - 1) / 2;
    s.ntiles = (int)ceil_div(D, kTN);
    s.tiles = ceil_div(B, kTM), s.chunks = ceil_div(B, kPnnChunk);
    const int64_t PD = (int64_t)s.P * D;
    s.kernel_floats = ktype == SATRANS_PNN_KERNEL_MAT ? PD * D : ktype == SATRANS_PNN_KERNEL_VEC ? PD : s.P;
    s.part = s.chunks * PD * (ktype == SATRANS_PNN_KERNEL_MAT ? D : 1);
    SATRANS_REQUIRE(s.tiles * F * s.ntiles <= 0x7fffffffLL && s.chunks * s.P * s.ntiles * s.ntiles <= 0x7fffffffLL &&
                        s.chunks * ceil_div(PD, kThreads) <= 0x7fffffffLL && s.chunks * D <= 0x7fffffffLL &&
                        ceil_div((int64_t)B * F * D, kThreads) <= 0x7fffffffLL,
                    SATRANS_E_UNSUPPORTED, "%s: B=%d F=%d D=%d needs more than 2^31 workgroups", who, B, F, D);
    return SATRANS_OK;
}

// x rows of ld floats: flatten(e) at eofs, ip at iofs, op at oofs (each when >= 0)
int pnn_products_fwd(const Pnn& s, const float* e, const float* kern, float* x, int ld, int eofs, int iofs, int oofs, hipStream_t st) {
    const bool mat = oofs >= 0 && s.ktype == SATRANS_PNN_KERNEL_MAT;
    if (eofs >= 0 || iofs >= 0 || (oofs >= 0 && !mat)) {
        pnn_point_fwd_kernel<<<(unsigned)s.B, kThreads, 0, st>>>(e, kern, s.F, s.D, s.P, s.ktype, x, ld, eofs, iofs, mat ? -1 : oofs);
        SATRANS_CHECK_LAUNCH("pnn_point_fwd_kernel");
    }
    if (mat) {
        pnn_mat_fwd_kernel<<<(unsigned)(s.tiles * (s.F - 1)), kThreads, 0, st>>>(e, kern, s.B, s.F, s.D, s.P, x, ld, oofs);
        SATRANS_CHECK_LAUNCH("pnn_mat_fwd_kernel");
    }
    return SATRANS_OK;
}

// de written; dkernel written (with an outer block).  dx rows of ld floats in the forward's layout.  part: s.part floats
int pnn_products_bwd(const Pnn& s, const float* e, const float* kern, const float* dx, int ld, int eofs, int iofs, int oofs, float* de,
                     float* part, float* dkernel, hipStream_t st) {
    const bool mat = oofs >= 0 && s.ktype == SATRANS_PNN_KERNEL_MAT;
    if (mat) {
        pnn_mat_dk_kernel<<<(unsigned)(s.chunks * s.P * s.ntiles * s.ntiles), kThreads, 0, st>>>(e, dx, s.B, s.F, s.D, s.P, s.ntiles, ld, oofs,
                                                                                               part);
        SATRANS_CHECK_LAUNCH("pnn_mat_dk_kernel");
        mmoe_reduce_kernel<false><<<(unsigned)ceil_div(s.kernel_floats, kThreads), kThreads, 0, st>>>(
            part, nullptr, nullptr, s.B, s.kernel_floats, s.D, 0, 1, 1, (int)s.chunks, dkernel, nullptr);
        SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel (pnn mat)");
        pnn_mat_dx_kernel<<<(unsigned)(s.tiles * s.F * s.ntiles), kThreads, 0, st>>>(e, kern, dx, s.B, s.F, s.D, s.P, s.ntiles, ld, eofs, iofs,
                                                                                    oofs, de);
        SATRANS_CHECK_LAUNCH("pnn_mat_dx_kernel");
        return SATRANS_OK;
    }
    if (oofs >= 0) {
        const int per_chunk = (int)ceil_div((int64_t)s.P * s.D, kThreads);
        pnn_point_dk_kernel<<<(unsigned)(s.chunks * per_chunk), kThreads, 0, st>>>(e, dx, s.B, s.F, s.D, s.P, s.ktype, ld, oofs, per_chunk,
                                                                                  part);
        SATRANS_CHECK_LAUNCH("pnn_point_dk_kernel");
        // ('num': the chunk's D partials of a pair count as chunks of their own)
        const int nparts = (int)(s.ktype == SATRANS_PNN_KERNEL_VEC ? s.chunks : s.chunks * s.D);
        mmoe_reduce_kernel<false><<<(unsigned)ceil_div(s.kernel_floats, kThreads), kThreads, 0, st>>>(
            part, nullptr, nullptr, s.B, s.kernel_floats, s.D, 0, 1, 1, nparts, dkernel, nullptr);
        SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel (pnn vec / num)");
    }
    const int64_t total = (int64_t)s.B * s.F * s.D;
    pnn_point_dx_kernel<<<(unsigned)ceil_div(total, kThreads), kThreads, 0, st>>>(e, kern, dx, total, s.F, s.D, s.ktype, ld, eofs, iofs, oofs,
                                                                                 de);
    SATRANS_CHECK_LAUNCH("pnn_point_dx_kernel");
    return SATRANS_OK;
}

// the whole head
struct PnnLayout {
    Pnn s;
    int ld, dense, iofs, oofs;      // columns of the DNN input, the dense ones among them; where ip and op start (-1: absent)
    Rows rows;
    Chain dnn;
    int64_t saved;                                  // saved: x, the hidden rows (dnn.s)
    int64_t w_dx, w_buf[2], w_part, total;          // workspace
};

int pnn_validate(const satrans_pnn_desc* d, const char* who, PnnLayout& Y) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->dense_dim >= 0 && d->n_dnn >= 0, SATRANS_E_BADARG, "%s: bad sizes dense_dim=%d n_dnn=%d", who, d->dense_dim, d->n_dnn);
    SATRANS_REQUIRE(d->n_dnn <= kMaxH, SATRANS_E_UNSUPPORTED, "%s: %d hidden layers (at most %d)", who, d->n_dnn, kMaxH);
    for (int l = 0; l < d->n_dnn; ++l) SATRANS_REQUIRE(d->width[l] > 0, SATRANS_E_BADARG, "%s: width[%d]=%d", who, l, d->width[l]);
    if (int rc = pnn_shape(Y.s, d->B, d->F, d->D, d->use_outer ? d->kernel_type : SATRANS_PNN_KERNEL_MAT, who)) return rc;
    const int FD = d->F * d->D, P = Y.s.P;
    Y.iofs = d->use_inner ? FD : -1;
    Y.oofs = d->use_outer ? FD + (d->use_inner ? P : 0) : -1;
    const int64_t ld = (int64_t)FD + (d->use_inner ? P : 0) + (d->use_outer ? P : 0) + d->dense_dim;
    SATRANS_REQUIRE(ld <= 0x7fffffffLL && ceil_div((int64_t)d->B * std::max(d->dense_dim, 1), kThreads) <= 0x7fffffffLL,
                    SATRANS_E_UNSUPPORTED, "%s: B=%d with %lld DNN input columns needs more than 2^31 workgroups", who, d->B, (long long)ld);
    Y.ld = (int)ld, Y.dense = d->dense_dim;
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
    Y.total = Y.w_part + std::max(part, d->use_outer ? Y.s.part : 0);
    return SATRANS_OK;
}

int inner_validate(const satrans_inner_product_desc* d, const char* who, Pnn& s) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    return pnn_shape(s, d->B, d->F, d->D, SATRANS_PNN_KERNEL_MAT, who);
}

int outer_validate(const satrans_outer_product_desc* d, const char* who, Pnn& s) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    return pnn_shape(s, d->B, d->F, d->D, d->kernel_type, who);
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int satrans_inner_product_fwd(const satrans_inner_product_desc* d, float* out, void* stream_) {
    Pnn s;
    if (int rc = inner_validate(d, "inner_product_fwd", s)) return rc;
    SATRANS_REQUIRE(d->e && out, SATRANS_E_BADARG, "inner_product_fwd: null pointer");
    return pnn_products_fwd(s, d->e, nullptr, out, s.P, -1, 0, -1, (hipStream_t)stream_);
}

extern "C" int satrans_inner_product_bwd(const satrans_inner_product_desc* d, const float* dout, float* de, void* stream_) {
    Pnn s;
    if (int rc = inner_validate(d, "inner_product_bwd", s)) return rc;
    SATRANS_REQUIRE(d->e && dout && de, SATRANS_E_BADARG, "inner_product_bwd: null pointer");
    return pnn_products_bwd(s, d->e, nullptr, dout, s.P, -1, 0, -1, de, nullptr, nullptr, (hipStream_t)stream_);
}

extern "C" int64_t satrans_outer_product_workspace_floats(const satrans_outer_product_desc* d) {
    Pnn s;
    const int rc = outer_validate(d, "outer_product_workspace_floats", s);
    return rc ? rc : s.part;
}

extern "C" int satrans_outer_product_fwd(const satrans_outer_product_desc* d, float* out, void* stream_) {
    Pnn s;
    if (int rc = outer_validate(d, "outer_product_fwd", s)) return rc;
    SATRANS_REQUIRE(d->e && d->kernel && out, SATRANS_E_BADARG, "outer_product_fwd: null pointer");
    return pnn_products_fwd(s, d->e, d->kernel, out, s.P, -1, -1, 0, (hipStream_t)stream_);
}

extern "C" int satrans_outer_product_bwd(const satrans_outer_product_desc* d, const float* dout, float* de, float* workspace,
                                         float* dkernel, void* stream_) {
    Pnn s;
    if (int rc = outer_validate(d, "outer_product_bwd", s)) return rc;
    SATRANS_REQUIRE(d->e && d->kernel && dout && de && workspace && dkernel, SATRANS_E_BADARG, "outer_product_bwd: null pointer");
    return pnn_products_bwd(s, d->e, d->kernel, dout, s.P, -1, -1, 0, de, workspace, dkernel, (hipStream_t)stream_);
}

extern "C" int64_t satrans_pnn_saved_floats(const satrans_pnn_desc* d) {
    PnnLayout Y;
    const int rc = pnn_validate(d, "pnn_saved_floats", Y);
    return rc ? rc : Y.saved;
}

extern "C" int64_t satrans_pnn_workspace_floats(const satrans_pnn_desc* d) {
    PnnLayout Y;
    const int rc = pnn_validate(d, "pnn_workspace_floats", Y);
    return rc ? rc : Y.total;
}

extern "C" int satrans_pnn_fwd(const satrans_pnn_desc* d, float* logit, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    PnnLayout Y;
    if (int rc = pnn_validate(d, "pnn_fwd", Y)) return rc;
    SATRANS_REQUIRE(d->emb && (d->dense || !Y.dense) && (d->kernel || !d->use_outer) && d->out_bias && logit && saved &&
                        chain_has(Y.dnn, d->dnn_w, d->dnn_b, d->dnn_linear_w, false),
                    SATRANS_E_BADARG, "pnn_fwd: null pointer");
    float* x = saved;
    if (int rc = pnn_products_fwd(Y.s, d->emb, d->kernel, x, Y.ld, 0, Y.iofs, Y.oofs, st)) return rc;
    if (Y.dense) {
        const int64_t total = (int64_t)d->B * Y.dense;
        pnn_cols_kernel<<<(unsigned)ceil_div(total, kThreads), kThreads, 0, st>>>(d->dense, Y.dense, 0, x, Y.ld, Y.ld - Y.dense, total, Y.dense);
        SATRANS_CHECK_LAUNCH("pnn_cols_kernel");
    }
    return dnn_fwd<false>(Y.rows, Y.dnn, x, saved, logit, st);
}

extern "C" int satrans_pnn_bwd(const satrans_pnn_desc* d, const float* dlogit, float* demb, float* ddense, const float* saved,
                               float* workspace, const satrans_pnn_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    PnnLayout Y;
    if (int rc = pnn_validate(d, "pnn_bwd", Y)) return rc;
    SATRANS_REQUIRE(d->emb && (d->kernel || !d->use_outer) && d->out_bias && dlogit && demb && (ddense || !Y.dense) && saved && workspace &&
                        g && (g->kernel || !d->use_outer) && g->out_bias && chain_has(Y.dnn, d->dnn_w, d->dnn_b, d->dnn_linear_w, false) &&
                        chain_has(Y.dnn, g->dnn_w, g->dnn_b, g->dnn_linear_w, false),
                    SATRANS_E_BADARG, "pnn_bwd: null pointer");
    set_grads(Y.dnn, g->dnn_w, g->dnn_b, g->dnn_linear_w, g->out_bias, false);
    const float* x = saved;
    float* dx = workspace + Y.w_dx;
    float* buf[2] = {workspace + Y.w_buf[0], workspace + Y.w_buf[1]};
    float* part = workspace + Y.w_part;
    int cur = 0;
    if (int rc = dnn_bwd<false>(Y.rows, Y.dnn, dlogit, x, saved, 0, dx, buf, cur, part, st)) return rc;
    if (Y.dense) {
        const int64_t total = (int64_t)d->B * Y.dense;
        pnn_cols_kernel<<<(unsigned)ceil_div(total, kThreads), kThreads, 0, st>>>(dx, Y.ld, Y.ld - Y.dense, ddense, Y.dense, 0, total, Y.dense);
        SATRANS_CHECK_LAUNCH("pnn_cols_kernel");
    }
    return pnn_products_bwd(Y.s, d->emb, d->kernel, dx, Y.ld, 0, Y.iofs, Y.oofs, demb, part, g->kernel, st);
}
