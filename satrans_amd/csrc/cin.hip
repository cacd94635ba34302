// Compressed interaction network (xDeepFM's CIN: deepctr-torch 0.2.9's `CIN`, which the reference's models/xdeepfm.py:73,96-98
// calls) with the outer product as a GENERATED operand.  With X0 = inputs [B, M, D], H_0 = M, layer i of O_i channels:
//     z_i[b,o,d] = b_i[o] + sum_{h < H_i, m < M} W_i[o, h M + m] X_i[b,h,d] X0[b,m,d]          a_i = relu(z_i)
// which is a product whose rows are the (sample, d) pairs r = b D + d, whose contraction index is k = h M + m and whose operand
//     A[r, k] = X_i[b,h,d] * X0[b,m,d]
// is one multiply of two values the workgroup holds - the [B, H M, D] tensor of the torch form never exists in memory.
//
// The tile product is grouped_gemm.h's: exact f32-input MFMA (v_mfma_f32_32x32x2_f32), 64 x 64 tile, contraction steps of 32,
// four waves on the 2 x 2 quadrants; a result element is a k-ordered fmaf chain and does not depend on the tile its row is in.
//
//   forward   cin_fwd_kernel   one launch per layer.  A workgroup = (64 rows r) x (128 channels o), two accumulators per wave.
//                              X0's rows of the tile [M][64] stay in LDS; X_i's go through LDS in blocks of 64 h ([64][64]; 64 M
//                              is a multiple of the step, so a step never straddles two blocks); W_i streams through LDS
//                              ([128][33]).  The tile is computed TRANSPOSED - W is the MFMA's A operand, the generated values
//                              its B operand, formed as fragments Xs[h][r] * X0s[m][r] straight from LDS and shared by the
//                              wave's two accumulators - so a lane holds one r and 32 channels and the stores of a_i [B, O, D]
//                              run along d.  Epilogue: + bias, relu.
//             cin_sum_kernel   result[b, c] = sum over d (ascending) of the direct channel behind column c
//   backward  per layer, last to first:
//             cin_dz_kernel    dz = (dresult of the direct channels, broadcast over d, + dX_{i+1} of the hidden ones) (a_i > 0)
//             cin_dw_kernel    chunk partials of dW_i = dz^T A and db_i = sum dz over chunks of kCinChunk rows r, the operand
//                              generated again; merged in chunk order by mmoe_reduce_kernel<false>
//             cin_dx_kernel    a workgroup owns 64 rows r and walks the 64-wide tiles of k in order: dA = dz W_i as a tile
//                              product over o, through LDS, then folded  dX_i[b,h,d] += dA X0[b,m,d]  (a register chain per h,
//                              carried over tile edges by the wave that owns h) and  dX0[b,m,d] += dA X_i[b,h,d]  (LDS
//                              accumulators [M][64], the wave that owns m).  dA is never stored.  Layer 0 has X_0 = X0: the
//                              chain of h is added to the accumulator of m = h when it closes.
// No floating-point atomics; every sum has a fixed order, so equal inputs give equal bits, and a sample's result row and dX0 rows
// are the same bits alone as inside a batch (dW and db sum over all rows).
#include <algorithm>

#include "grouped_gemm.h"

namespace satrans {
namespace {

constexpr int kCinL = SATRANS_CIN_MAX_LAYERS;
constexpr int kCinM = SATRANS_CIN_MAX_FIELDS;
constexpr int kCinW = SATRANS_CIN_MAX_WIDTH;
constexpr int kCinChunk = SATRANS_CIN_DW_ROW_CHUNK;
constexpr int kHB = 64;      // h rows of X_i in LDS at a time
constexpr int kFO = 128;     // channels under a workgroup of the forward
static_assert(SATRANS_CIN_ROW_TILE == kTM && kTM == 64 && kTN == 64, "the CIN kernels are written for the 64 x 64 tile");
static_assert(kCinChunk % kTK == 0 && kHB % kTK == 0, "whole steps per chunk and per block of h");

// X rows: X[b,h,d] = x[b ldx + h D + d] (X0 itself, or the leading channels of the previous layer's a with ldx = O_prev D).
// A workgroup = kFO = 128 channels x 64 rows r: wave (wm, wn) holds the channel blocks wm 32 and 64 + wm 32 of the row block
// wn 32 in two accumulators, which share every generated fragment.  (h, m) of the step's even k is kept in scalar registers;
// a lane adds its own half (k odd for lanes 32 - 63).
__global__ __launch_bounds__(kThreads) void cin_fwd_kernel(const float* __restrict__ x, int64_t ldx, int H,
                                                           const float* __restrict__ x0, int M, int D, int64_t rows,
                                                           const float* __restrict__ w, const float* __restrict__ bias, int O,
                                                           int ntiles, float* __restrict__ a) {
    __shared__ float Ws[kFO][kLd];        // [o][k of the step]
    __shared__ float Xs[kHB][kTN];        // [h of the block][r]
    __shared__ float X0s[kCinM][kTN];     // [m][r]
    const int n0 = (blockIdx.x % ntiles) * kFO;
    const int64_t r0 = (int64_t)(blockIdx.x / ntiles) * kTN;
    const int K = H * M;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    // staging: column lane = row r0 + lane of the tile, LDS rows wv, wv + 4, ..
    const int64_t rj = r0 + lane;
    const bool livej = rj < rows;
    const int64_t bj = livej ? rj / D : 0;
    const int dj = livej ? (int)(rj % D) : 0;
    const float* xj = x + bj * ldx + dj;
    const float* x0j = x0 + bj * (int64_t)M * D + dj;
    for (int m = wv; m < M; m += 4) X0s[m][lane] = livej ? x0j[(size_t)m * D] : 0.f;
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    constexpr int kPerW = kFO * kTK / kThreads;
    float rw[kPerW];
    auto load = [&](int k0) {
        const int k = k0 + kf;
#pragma unroll
        for (int e = 0; e < kPerW; ++e) {
            const int o = n0 + if0 + 8 * e;
            rw[e] = (o < O && k < K) ? w[(size_t)o * K + k] : 0.f;
        }
    };
    f32x16 acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 acc1 = acc0;
    load(0);
    const int r = lane & 31, hh = lane >> 5, col = wn * 32 + r;
    const int kblock = kHB * M;
    for (int k0 = 0; k0 < K; k0 += kTK) {
        __syncthreads();      // the previous step's fragment reads are done
#pragma unroll
        for (int e = 0; e < kPerW; ++e) Ws[if0 + 8 * e][kf] = rw[e];
        const int hb = (k0 / kblock) * kHB;
        if (k0 % kblock == 0) {
            for (int hl = wv; hl < kHB; hl += 4) Xs[hl][lane] = (livej && hb + hl < H) ? xj[(size_t)(hb + hl) * D] : 0.f;
        }
        __syncthreads();
        if (k0 + kTK < K) load(k0 + kTK);
        // even k = k0 + kk -> (he, me), the same for all lanes; the lane's k = even k + hh.  h stays inside the block: the
        // block's last k is a multiple of the step minus one.
        int he = k0 / M, me = k0 - he * M;
        he -= hb;
        const float* aw0 = &Ws[wm * 32 + r][hh];
        const float* aw1 = &Ws[64 + wm * 32 + r][hh];
        const float* xc = &Xs[0][col];
        const float* x0c = &X0s[0][col];
#pragma unroll
        for (int kk = 0; kk < kTK; kk += 2) {
            const bool wrap = me + hh >= M;      // (M = 1: the odd k is the next h)
            const int h = wrap ? he + 1 : he, m = wrap ? me + hh - M : me + hh;
            const float bv = xc[h * kTN] * x0c[m * kTN];      // rows h >= H hold zeros, and so do Ws's columns k >= K
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw0[kk], bv, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw1[kk], bv, acc1, 0, 0, 0);
            me += 2;
            if (me >= M) me -= M, ++he;
            if (me >= M) me -= M, ++he;      // M = 1
        }
    }
    const int64_t rr = r0 + col;
    if (rr >= rows) return;
    const int64_t bb = rr / D;
    const int dd = (int)(rr % D);
    float* ar = a + (size_t)bb * O * D + dd;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int o = n0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (o < O) ar[(size_t)o * D] = fmaxf(acc0[q] + bias[o], 0.f);
        if (o + 64 < O) ar[(size_t)(o + 64) * D] = fmaxf(acc1[q] + bias[o + 64], 0.f);
    }
}

struct CinSum {
    const float* a[kCinL];
    int O[kCinL], d0[kCinL], off[kCinL + 1];
};

// one thread per result element: column c of layer i (off[i] <= c < off[i + 1]) is channel d0[i] + c - off[i], summed over d
__global__ __launch_bounds__(kThreads) void cin_sum_kernel(CinSum p, int L, int64_t total, int D, int F, float* __restrict__ result) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const int64_t b = e / F;
    const int c = (int)(e % F);
    int i = 0;
    while (i + 1 < L && c >= p.off[i + 1]) ++i;
    const float* src = p.a[i] + ((size_t)b * p.O[i] + p.d0[i] + c - p.off[i]) * D;
    float s = 0.f;
    for (int d = 0; d < D; ++d) s += src[d];
    result[e] = s;
}

// dz[b,o,d] = a[b,o,d] > 0 ? (o >= d0: dres[b, off + o - d0]) + (dxn and o < hn: dxn[b,o,d]) : 0
__global__ __launch_bounds__(kThreads) void cin_dz_kernel(const float* __restrict__ a, const float* __restrict__ dres, int F, int off,
                                                          int d0, const float* __restrict__ dxn, int hn, int O, int D, int64_t total,
                                                          float* __restrict__ dz) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const int d = (int)(e % D);
    const int64_t bo = e / D;
    const int o = (int)(bo % O);
    const int64_t b = bo / O;
    float up = 0.f;
    if (o >= d0) up = dres[(size_t)b * F + off + o - d0];
    if (dxn && o < hn) up += dxn[((size_t)b * hn + o) * D + d];
    dz[e] = a[e] > 0.f ? up : 0.f;
}

// unit u = rows [u kCinChunk, (u + 1) kCinChunk) of r:  part_w[u][o, k] = sum over the chunk's rows (ascending) of dz[r, o] A[r, k],
// part_b[u][o] = sum of dz[r, o].   grid: units x o tiles x k tiles
__global__ __launch_bounds__(kThreads) void cin_dw_kernel(const float* __restrict__ dz, int O, const float* __restrict__ x,
                                                          int64_t ldx, int H, const float* __restrict__ x0, int M, int D,
                                                          int64_t rows, int ntiles, int ktiles, float* __restrict__ part_w,
                                                          float* __restrict__ part_b) {
    __shared__ float As[kTM][kLd];      // [o][row of the step]
    __shared__ float Bs[kTN][kLd];      // [k][row of the step]
    const int per_unit = ntiles * ktiles;
    const int unit = blockIdx.x / per_unit, rem = blockIdx.x % per_unit;
    const int n0 = (rem / ktiles) * kTM, c0 = (rem % ktiles) * kTN;
    const int K = H * M;
    const int64_t p_begin = (int64_t)unit * kCinChunk, p_end = p_begin + kCinChunk < rows ? p_begin + kCinChunk : rows;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int pf = t & 31, if0 = t >> 5;      // the step's row index is the one contiguous in memory (d runs fastest)
    int xo[kPer], x0o[kPer];                  // offsets of this thread's k's: h D and m D; -1: k >= K
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const int k = c0 + if0 + 8 * e, h = k / M;
        xo[e] = k < K ? h * D : -1;
        x0o[e] = (k - h * M) * D;
    }
    float ra[kPer], rb[kPer];
    auto load = [&](int64_t p0) {
        const int64_t p = p0 + pf;
        const bool live = p < p_end;
        const unsigned pu = live ? (unsigned)p : 0u;      // rows < 2^31
        const int64_t b = pu / (unsigned)D;
        const int d = (int)(pu % (unsigned)D);
        const float* zr = dz + (size_t)b * O * D + d;
        const float* xr = x + b * ldx + d;
        const float* x0r = x0 + b * (int64_t)M * D + d;
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int o = n0 + if0 + 8 * e;
            ra[e] = (live && o < O) ? zr[(size_t)o * D] : 0.f;
            rb[e] = (live && xo[e] >= 0) ? xr[xo[e]] * x0r[x0o[e]] : 0.f;
        }
    };
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    load(p_begin);
    for (int64_t p0 = p_begin; p0 < p_end; p0 += kTK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            As[if0 + 8 * e][pf] = ra[e];
            Bs[if0 + 8 * e][pf] = rb[e];
        }
        __syncthreads();
        if (p0 + kTK < p_end) load(p0 + kTK);
        if (c0 == 0 && t < kTM) {      // the bias gradient: rows of the chunk in order (rows past its end hold zeros)
#pragma unroll
            for (int kk = 0; kk < kTK; ++kk) bsum += As[t][kk];
        }
        mma_step(As, Bs, lane, wm, wn, acc);
    }
    if (c0 == 0 && t < kTM && n0 + t < O) part_b[(size_t)unit * O + n0 + t] = bsum;
    const int c = c0 + wn * 32 + (lane & 31);
    if (c >= K) return;
    float* out = part_w + (size_t)unit * O * K;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int n = n0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (n < O) out[(size_t)n * K + c] = acc[q];
    }
}

// A workgroup = 64 rows r; lane = its row in the staging and in the fold, wave v owns the h and the m with index % 4 == v.
//   same = 0   dx [B,H,D] is WRITTEN (every h closes exactly once); dx0 gets the accumulators
//   same = 1   X = X0 (layer 0): the chain of h goes into the accumulator of m = h; dx is not touched
//   dx0 [B,M,D]: written (add = 0) or added to (add = 1; by the thread that owns the element in every launch)
__global__ __launch_bounds__(kThreads) void cin_dx_kernel(const float* __restrict__ dz, int O, const float* __restrict__ w,
                                                          const float* __restrict__ x, int64_t ldx, int H,
                                                          const float* __restrict__ x0, int M, int D, int64_t rows, int same, int add,
                                                          float* __restrict__ dx, float* dx0) {
    __shared__ float tiles[2 * kTM * kLd];      // the two operand tiles; after a tile's product, dA [k][r]
    __shared__ float X0s[kCinM][kTN];
    __shared__ float acc0[kCinM][kTN];
    static_assert(kTN * kTM <= 2 * kTM * kLd, "dA fits over the operand tiles");
    float(*Wt)[kLd] = reinterpret_cast<float(*)[kLd]>(tiles);                  // [k][o of the step]
    float(*Zs)[kLd] = reinterpret_cast<float(*)[kLd]>(tiles + kTM * kLd);      // [r][o of the step]
    float(*T)[kTN] = reinterpret_cast<float(*)[kTN]>(tiles);
    const int64_t r0 = (int64_t)blockIdx.x * kTN;
    const int K = H * M;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int64_t rj = r0 + lane;
    const bool live = rj < rows;
    const int64_t bj = live ? rj / D : 0;
    const int dj = live ? (int)(rj % D) : 0;
    const float* zj = dz + (size_t)bj * O * D + dj;
    const float* xr = x + bj * ldx + dj;
    const float* x0r = x0 + bj * (int64_t)M * D + dj;
    for (int m = wv; m < M; m += 4) {
        X0s[m][lane] = live ? x0r[(size_t)m * D] : 0.f;
        acc0[m][lane] = 0.f;
    }
    float cx = 0.f;      // the open chain of dX[h] of this wave's h
    for (int c0 = 0; c0 < K; c0 += kTM) {
        float rw[kPer], rz[kPer];
        auto load = [&](int o0) {
            const int k = c0 + lane;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                const int o = o0 + wv + 4 * e;
                rw[e] = (o < O && k < K) ? w[(size_t)o * K + k] : 0.f;
                rz[e] = (live && o < O) ? zj[(size_t)o * D] : 0.f;
            }
        };
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        load(0);
        for (int o0 = 0; o0 < O; o0 += kTK) {
            __syncthreads();      // the previous step's fragment reads, or the previous tile's fold, are done
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                Wt[lane][wv + 4 * e] = rw[e];
                Zs[lane][wv + 4 * e] = rz[e];
            }
            __syncthreads();
            if (o0 + kTK < O) load(o0 + kTK);
            mma_step(Wt, Zs, lane, wm, wn, acc);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) T[wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)][wn * 32 + (lane & 31)] = acc[q];
        __syncthreads();
        // the fold over this tile's k, ascending
        const int kend = min(kTM, K - c0);
        int h = c0 / M, m = c0 - h * M, hx = -1;
        float xh = 0.f;
        for (int kl = 0; kl < kend; ++kl) {
            const float tv = T[kl][lane];
            if ((m & 3) == wv) {
                if (hx != h) {
                    xh = live ? xr[(size_t)h * D] : 0.f;
                    hx = h;
                }
                acc0[m][lane] = fmaf(tv, xh, acc0[m][lane]);
            }
            if ((h & 3) == wv) cx = fmaf(tv, X0s[m][lane], cx);
            if (++m == M) {
                if ((h & 3) == wv) {
                    if (same)
                        acc0[h][lane] += cx;
                    else if (live)
                        dx[((size_t)bj * H + h) * D + dj] = cx;
                    cx = 0.f;
                }
                m = 0;
                ++h;
            }
        }
    }
    if (live)
        for (int m = wv; m < M; m += 4) {
            const size_t at = ((size_t)bj * M + m) * D + dj;
            dx0[at] = add ? dx0[at] + acc0[m][lane] : acc0[m][lane];
        }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

struct CinLayout {
    int L, F;                     // layers, result columns
    int O[kCinL], H[kCinL];       // channels out and in
    int d0[kCinL], off[kCinL + 1], hn[kCinL];      // first direct channel, its result column, channels handed to the next layer
    int64_t s[kCinL];             // saved: a_i [B, O_i, D], floats from its start
    int64_t rows, tiles, chunks;
    int64_t saved, w_dz, w_dx, w_part, total;      // workspace: dz, dX of the layer above, the partials
};

int cin_validate(const satrans_cin_desc* d, const char* who, CinLayout& Y) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->M > 0 && d->D > 0 && d->L > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d M=%d D=%d L=%d", who, d->B, d->M,
                    d->D, d->L);
    SATRANS_REQUIRE(d->split_half == 0 || d->split_half == 1, SATRANS_E_BADARG, "%s: split_half=%d", who, d->split_half);
    SATRANS_REQUIRE(d->L <= kCinL && d->M <= kCinM, SATRANS_E_UNSUPPORTED, "%s: L=%d layers, M=%d fields (at most %d, %d)", who, d->L,
                    d->M, kCinL, kCinM);
    Y.L = d->L;
    Y.rows = (int64_t)d->B * d->D;
    SATRANS_REQUIRE(Y.rows <= 0x7fffffffLL - kCinChunk, SATRANS_E_UNSUPPORTED, "%s: B D = %lld rows (2^31 at most)", who,
                    (long long)Y.rows);
    Y.tiles = ceil_div(Y.rows, kTM);
    Y.chunks = ceil_div(Y.rows, kCinChunk);
    int h = d->M, col = 0;
    int64_t at = 0, max_o = 0, max_h = 0, per_part = 0;
    for (int i = 0; i < d->L; ++i) {
        const int o = d->width[i];
        const bool last = i == d->L - 1, split = d->split_half && !last;
        SATRANS_REQUIRE(o > 0, SATRANS_E_BADARG, "%s: bad sizes width[%d]=%d", who, i, o);
        SATRANS_REQUIRE(o <= kCinW, SATRANS_E_UNSUPPORTED, "%s: width[%d]=%d (at most %d)", who, i, o, kCinW);
        SATRANS_REQUIRE(!split || o % 2 == 0, SATRANS_E_BADARG, "%s: width[%d]=%d must be even under split_half", who, i, o);
        Y.O[i] = o, Y.H[i] = h;
        Y.d0[i] = split ? o / 2 : 0;
        Y.off[i] = col;
        col += o - Y.d0[i];
        Y.hn[i] = last ? 0 : (split ? o / 2 : o);
        Y.s[i] = at;
        at += Y.rows * o;
        const int64_t K = (int64_t)h * d->M;
        SATRANS_REQUIRE(Y.tiles * ceil_div(o, kTM) <= 0x7fffffffLL && Y.chunks * ceil_div(o, kTM) * ceil_div(K, kTN) <= 0x7fffffffLL &&
                            ceil_div(Y.rows * o, kThreads) <= 0x7fffffffLL,
                        SATRANS_E_UNSUPPORTED, "%s: layer %d (%d x %lld) at B=%d D=%d needs more than 2^31 workgroups", who, i, o,
                        (long long)K, d->B, d->D);
        per_part = std::max(per_part, Y.chunks * o * (K + 1));
        max_o = std::max<int64_t>(max_o, o);
        if (i > 0) max_h = std::max<int64_t>(max_h, h);
        h = Y.hn[i];
    }
    Y.off[d->L] = Y.F = col;
    Y.saved = at;
    Y.w_dz = 0;
    Y.w_dx = Y.rows * max_o;
    Y.w_part = Y.w_dx + Y.rows * max_h;
    Y.total = Y.w_part + per_part;
    return SATRANS_OK;
}

template <class S>
bool cin_has(const CinLayout& Y, const S* g) {
    if (!g) return false;
    for (int i = 0; i < Y.L; ++i)
        if (!g->w[i] || !g->b[i]) return false;
    return true;
}

// the input of layer i: X0, or the leading channels of a_{i-1}
inline const float* cin_x(const satrans_cin_desc* d, const CinLayout& Y, const float* saved, int i, int64_t& ldx) {
    ldx = i == 0 ? (int64_t)d->M * d->D : (int64_t)Y.O[i - 1] * d->D;
    return i == 0 ? d->x0 : saved + Y.s[i - 1];
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_cin_saved_floats(const satrans_cin_desc* d) {
    CinLayout Y;
    const int rc = cin_validate(d, "cin_saved_floats", Y);
    return rc ? rc : Y.saved;
}

extern "C" int64_t satrans_cin_workspace_floats(const satrans_cin_desc* d) {
    CinLayout Y;
    const int rc = cin_validate(d, "cin_workspace_floats", Y);
    return rc ? rc : Y.total;
}

extern "C" int satrans_cin_fwd(const satrans_cin_desc* d, float* result, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    CinLayout Y;
    const int rc = cin_validate(d, "cin_fwd", Y);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x0 && cin_has(Y, d) && result && saved, SATRANS_E_BADARG, "cin_fwd: null pointer");
    CinSum sum;
    for (int i = 0; i < Y.L; ++i) {
        int64_t ldx;
        const float* x = cin_x(d, Y, saved, i, ldx);
        const int ntiles = (int)ceil_div(Y.O[i], kFO);
        cin_fwd_kernel<<<(unsigned)(Y.tiles * ntiles), kThreads, 0, st>>>(x, ldx, Y.H[i], d->x0, d->M, d->D, Y.rows, d->w[i], d->b[i],
                                                                          Y.O[i], ntiles, saved + Y.s[i]);
        SATRANS_CHECK_LAUNCH("cin_fwd_kernel");
        sum.a[i] = saved + Y.s[i], sum.O[i] = Y.O[i], sum.d0[i] = Y.d0[i], sum.off[i] = Y.off[i];
    }
    for (int i = Y.L; i <= kCinL; ++i) sum.off[i] = Y.F;
    for (int i = Y.L; i < kCinL; ++i) sum.a[i] = nullptr, sum.O[i] = sum.d0[i] = 0;
    const int64_t total = (int64_t)d->B * Y.F;
    cin_sum_kernel<<<(unsigned)ceil_div(total, kThreads), kThreads, 0, st>>>(sum, Y.L, total, d->D, Y.F, result);
    SATRANS_CHECK_LAUNCH("cin_sum_kernel");
    return SATRANS_OK;
}

extern "C" int satrans_cin_bwd(const satrans_cin_desc* d, const float* dresult, float* dx0, const float* saved, float* workspace,
                               const satrans_cin_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    CinLayout Y;
    const int rc = cin_validate(d, "cin_bwd", Y);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x0 && cin_has(Y, d) && dresult && dx0 && saved && workspace && cin_has(Y, g), SATRANS_E_BADARG,
                    "cin_bwd: null pointer");
    float* dz = workspace + Y.w_dz;
    float* dxb = workspace + Y.w_dx;      // dX_{i+1}: read by layer i's dz launch before layer i's fold writes dX_i over it
    float* part = workspace + Y.w_part;
    const float* dxn = nullptr;      // dX_{i+1}, from the layer above
    for (int i = Y.L - 1; i >= 0; --i) {
        const int O = Y.O[i], H = Y.H[i];
        const int64_t K = (int64_t)H * d->M, total = Y.rows * O;
        int64_t ldx;
        const float* x = cin_x(d, Y, saved, i, ldx);
        cin_dz_kernel<<<(unsigned)ceil_div(total, kThreads), kThreads, 0, st>>>(saved + Y.s[i], dresult, Y.F, Y.off[i], Y.d0[i], dxn,
                                                                               Y.hn[i], O, d->D, total, dz);
        SATRANS_CHECK_LAUNCH("cin_dz_kernel");
        const int ntiles = (int)ceil_div(O, kTM), ktiles = (int)ceil_div(K, kTN);
        float* part_b = part + Y.chunks * O * K;
        cin_dw_kernel<<<(unsigned)(Y.chunks * ntiles * ktiles), kThreads, 0, st>>>(dz, O, x, ldx, H, d->x0, d->M, d->D, Y.rows, ntiles,
                                                                                  ktiles, part, part_b);
        SATRANS_CHECK_LAUNCH("cin_dw_kernel");
        mmoe_reduce_kernel<false><<<(unsigned)ceil_div((int64_t)O * K + O, kThreads), kThreads, 0, st>>>(
            part, part_b, nullptr, d->B, (int64_t)O * K, O, 0, 1, 1, (int)Y.chunks, g->w[i], g->b[i]);
        SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel");
        float* dxi = i > 0 ? dxb : nullptr;
        cin_dx_kernel<<<(unsigned)Y.tiles, kThreads, 0, st>>>(dz, O, d->w[i], x, ldx, H, d->x0, d->M, d->D, Y.rows, i == 0 ? 1 : 0,
                                                              i == Y.L - 1 ? 0 : 1, dxi, dx0);
        SATRANS_CHECK_LAUNCH("cin_dx_kernel");
        dxn = dxi;
    }
    return SATRANS_OK;
}
