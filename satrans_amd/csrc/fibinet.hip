// FiBiNET (deepctr-torch 0.2.9's SENETLayer and BilinearInteraction, which the reference's models/fibinet.py:51-52,93-95 calls,
// and the half of FiBiNET.forward behind the lookup).  e [B, F, D]; pairs (i, j), i < j, in itertools.combinations order,
// pair p = i (2 F - i - 1) / 2 + j - i - 1, P = F (F - 1) / 2; W_w(p) the weight of pair p: w = 0 (all), i (each), p (interaction).
//     SENet      z = mean_d e    hid = relu(z w1^T)    a = relu(hid w2^T)                         v = e * a
//     bilinear   q_p = W_w(p) e_i    r_p = q_p * e_j                                              (the raw block)
//                s_p = a_i a_j r_p = (W_w(p) v_i) * v_j                                           (the SENet block)
//     head       x = [ s | r | dense ]  [B, 2 P D + dense]    the DNN, dnn_linear, out.bias       logit [B, 1]
// One D x D product per pair serves both blocks, forward and backward.  Backward, with dS_p, dR_p the two blocks of dx:
//     g_p = dR_p + a_i a_j dS_p        t_p[b] = sum_d dS_p r_p      da_i += a_j t_p      da_j += a_i t_p
//     dq_p = g_p * e_j                 de_j += g_p * q_p            de_i += W_w(p)^T dq_p
//     dW_w(p) += sum_b dq_p e_i^T      then da through the excitation, and de[b,f,:] += dz[b,f] / D
//
// fibinet_se_fwd_kernel    a wave per row: lane f sums its field (d ascending), lanes r < R the hidden units (f ascending), lanes
//                          f the gates (r ascending); a, hid saved; v written when asked for.
// fibinet_bil_fwd_kernel   workgroup = (64 rows) x (pair p) x (64 columns of D): grouped_gemm.h's tile product (mma_step,
//                          v_mfma_f32_32x32x2_f32, steps of 32 over D - one step at D = 32), the tile staged through LDS so that a
//                          thread stores four consecutive d: r = q * e_j into the raw block and a_i a_j r into the SENet block of
//                          the DNN input, 16-byte stores when D % 4 == 0 and the rows allow.  ONE kernel for the three types:
//                          the kernel is bound by its stores (2 P D floats out per sample against 2 P D^2 FLOP), so the
//                          repeated products of 'all' / 'each' cost nothing that matters.
// fibinet_bil_da_kernel    a wave per row: pairs ascending, t_p by the lanes over d and a fixed butterfly; lane f holds da_f.
//                          r_p is read back from the raw block.
// fibinet_bil_dx_kernel    workgroup = (64 rows) x (field f) x (64 columns of D), the only writer of its de tile.  Partners
//                          i < f ascending: q_p = W e_i by the same product as the forward (not saved a second time), then
//                          sum += g_p * q_p elementwise; partners j > f ascending: dq_p = g_p * e_j formed on operand load,
//                          acc += dq_p W over all of them in the MFMA accumulators.  de = acc + sum.
// fibinet_bil_dw_kernel    workgroup = (chunk of SATRANS_FIBINET_DW_ROW_CHUNK rows) x (weight w) x (64 x 64 tile of [D, D]): the
//                          pairs that share w in ascending pair order, each over the chunk's rows in steps of 32; one partial
//                          per (chunk, w), merged in chunk order by mmoe_reduce_kernel<false>.
// fibinet_se_bwd_kernel    workgroup = chunk of SATRANS_FIBINET_SENET_ROW_CHUNK rows, a wave per row: z again, the two masks from
//                          the saved a and hid, de += dz / D (+ dv * a); the row's four vectors into LDS, then a thread per
//                          element of dw1 / dw2 sums the chunk's rows in order; partials merged in chunk order.
// The DNN is head_layers.h's dense launcher (dnn_fwd<false> / dnn_bwd<false>) with dnn_linear as the one-column final layer and
// out.bias as that layer's bias, so d out.bias falls out of the same launches.
// No floating-point atomics; every sum has a fixed order; a row's results do not depend on its place in a tile.  fp32 only.
#include "head_layers.h"
#include "pair_index.h"

namespace satrans {
namespace {

constexpr int kFibF = SATRANS_FIBINET_MAX_FIELDS;
constexpr int kFibD = SATRANS_FIBINET_MAX_DIM;
constexpr int kFibChunk = SATRANS_FIBINET_DW_ROW_CHUNK;
constexpr int kSeChunk = SATRANS_FIBINET_SENET_ROW_CHUNK;
constexpr int kFibWaves = kThreads / 64;
static_assert(kFibF <= 64, "a lane per field");
static_assert(kFibChunk % kTK == 0 && kSeChunk % kFibWaves == 0, "row steps");

__device__ __forceinline__ float fib_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int weight_of(int type, int i, int p) {
    return type == SATRANS_BILINEAR_ALL ? 0 : type == SATRANS_BILINEAR_EACH ? i : p;
}

// g_p[row, col] = dR_p + a_i a_j dS_p (with a), dR_p (without).  dx rows of ld floats, the raw block at column rofs.
__device__ __forceinline__ float g_of(const float* __restrict__ dx, const float* __restrict__ a, size_t row, int ld, int rofs, int F,
                                      int D, int p, int i, int j, int col) {
    const float* xr = dx + row * ld + (size_t)p * D + col;
    const float dr = xr[rofs];
    if (!a) return dr;
    return fmaf(a[row * F + i] * a[row * F + j], xr[0], dr);
}

// ---- SENet ----------------------------------------------------------------------------------------------------------------------

// z of the wave's row: lane f < F the mean of its field, d ascending
__device__ __forceinline__ float se_mean(const float* __restrict__ er, int F, int D, int lane) {
    float z = 0.f;
    if (lane < F) {
        const float* p = er + (size_t)lane * D;
        for (int d = 0; d < D; ++d) z += p[d];
        z = z / (float)D;
    }
    return z;
}

// grid: ceil(B / 4)
__global__ __launch_bounds__(kThreads) void fibinet_se_fwd_kernel(const float* __restrict__ e, const float* __restrict__ w1,
                                                                  const float* __restrict__ w2, int B, int F, int D, int R,
                                                                  float* __restrict__ a_out, float* __restrict__ h_out,
                                                                  float* __restrict__ v) {
    const int64_t row = (int64_t)blockIdx.x * kFibWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    const float* er = e + (size_t)row * F * D;
    const float z = se_mean(er, F, D, lane);
    float h = 0.f;
    for (int f = 0; f < F; ++f) {
        const float zf = __shfl(z, f, 64);
        if (lane < R) h = fmaf(w1[(size_t)lane * F + f], zf, h);
    }
    h = fmaxf(h, 0.f);
    float av = 0.f;
    for (int r = 0; r < R; ++r) {
        const float hr = __shfl(h, r, 64);
        if (lane < F) av = fmaf(w2[(size_t)lane * R + r], hr, av);
    }
    av = fmaxf(av, 0.f);
    if (lane < F) a_out[(size_t)row * F + lane] = av;
    if (lane < R) h_out[(size_t)row * R + lane] = h;
    if (!v) return;
    const int FD = F * D;
    float* vr = v + (size_t)row * FD;
    for (int base = 0; base < FD; base += 64) {      // (every lane takes part in the shuffle)
        const int idx = base + lane;
        const float af = __shfl(av, min(idx, FD - 1) / D, 64);
        if (idx < FD) vr[idx] = er[idx] * af;
    }
}

// grid: ceil(B / kSeChunk).  part1 [chunks][R F], part2 [chunks][F R].  de (+)= the input gradient.
__global__ __launch_bounds__(kThreads) void fibinet_se_bwd_kernel(const float* __restrict__ e, const float* __restrict__ w1,
                                                                  const float* __restrict__ w2, const float* __restrict__ a_s,
                                                                  const float* __restrict__ h_s, const float* __restrict__ da,
                                                                  const float* __restrict__ dv, int B, int F, int D, int R,
                                                                  float* __restrict__ de, float* __restrict__ part1,
                                                                  float* __restrict__ part2) {
    __shared__ float sh[kSeChunk][4][kFibF];      // per row: dpre2 [F], hid [R], dpre1 [R], z [F]
    const int64_t r0 = (int64_t)blockIdx.x * kSeChunk;
    const int nr = (int)(B - r0 < kSeChunk ? B - r0 : kSeChunk);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int FD = F * D;
    for (int r = wv; r < nr; r += kFibWaves) {
        const size_t row = (size_t)(r0 + r);
        const float* er = e + row * FD;
        const float* dvr = dv ? dv + row * FD : nullptr;
        float* der = de + row * FD;
        const float z = se_mean(er, F, D, lane);
        const float av = lane < F ? a_s[row * F + lane] : 0.f;
        const float hv = lane < R ? h_s[row * R + lane] : 0.f;
        float dA = (da && lane < F) ? da[row * F + lane] : 0.f;
        if (dvr && lane < F)
            for (int d = 0; d < D; ++d) dA = fmaf(dvr[(size_t)lane * D + d], er[(size_t)lane * D + d], dA);
        const float dp2 = av > 0.f ? dA : 0.f;
        float dh = 0.f;
        for (int f = 0; f < F; ++f) {
            const float g = __shfl(dp2, f, 64);
            if (lane < R) dh = fmaf(w2[(size_t)f * R + lane], g, dh);
        }
        const float dp1 = hv > 0.f ? dh : 0.f;
        float dz = 0.f;
        for (int q = 0; q < R; ++q) {
            const float g = __shfl(dp1, q, 64);
            if (lane < F) dz = fmaf(w1[(size_t)q * F + lane], g, dz);
        }
        dz = dz / (float)D;
        for (int base = 0; base < FD; base += 64) {
            const int idx = base + lane, f = min(idx, FD - 1) / D;
            const float dzf = __shfl(dz, f, 64), af = __shfl(av, f, 64);
            if (idx < FD) der[idx] += dvr ? fmaf(dvr[idx], af, dzf) : dzf;
        }
        sh[r][0][lane] = dp2;
        sh[r][1][lane] = hv;
        sh[r][2][lane] = dp1;
        sh[r][3][lane] = z;
    }
    __syncthreads();
    const int FR = F * R;
    for (int el = t; el < 2 * FR; el += kThreads) {
        float sum = 0.f;
        if (el < FR) {      // dw1[q, f] = sum_b dpre1[b, q] z[b, f]
            const int q = el / F, f = el % F;
            for (int r = 0; r < nr; ++r) sum = fmaf(sh[r][2][q], sh[r][3][f], sum);
            part1[(size_t)blockIdx.x * FR + el] = sum;
        } else {            // dw2[f, q] = sum_b dpre2[b, f] hid[b, q]
            const int f = (el - FR) / R, q = (el - FR) % R;
            for (int r = 0; r < nr; ++r) sum = fmaf(sh[r][0][f], sh[r][1][q], sum);
            part2[(size_t)blockIdx.x * FR + (el - FR)] = sum;
        }
    }
}

// ---- bilinear -------------------------------------------------------------------------------------------------------------------

// grid: row tiles x P x ntiles (ntiles = ceil(D / 64)).  x rows of ld floats: the SENet block at column 0 (with a), the raw block
// at column rofs.
__global__ __launch_bounds__(kThreads) void fibinet_bil_fwd_kernel(const float* __restrict__ e, const float* __restrict__ w,
                                                                   const float* __restrict__ a, int B, int F, int D, int type, int P,
                                                                   int ntiles, float* __restrict__ x, int ld, int rofs, int vec) {
    __shared__ float As[kTM][kLd];
    __shared__ float Bs[kTN][kLd];
    __shared__ float Cs[kTM][kTN + 1];
    const int n0 = (blockIdx.x % ntiles) * kTN;
    const int p = (blockIdx.x / ntiles) % P;
    const int64_t r0 = (int64_t)(blockIdx.x / ntiles / P) * kTM;
    int i, j;
    pair_fields(p, F, i, j);
    const float* wp = w + (size_t)weight_of(type, i, p) * D * D;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += kTK) {
        __syncthreads();      // the previous step's fragment reads are done
        const int k = k0 + kf;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int64_t row = r0 + if0 + 8 * q;
            const int n = n0 + if0 + 8 * q;
            As[if0 + 8 * q][kf] = (row < B && k < D) ? e[((size_t)row * F + i) * D + k] : 0.f;
            Bs[if0 + 8 * q][kf] = (n < D && k < D) ? wp[(size_t)n * D + k] : 0.f;
        }
        __syncthreads();
        mma_step(As, Bs, lane, wm, wn, acc);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) Cs[wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)][wn * 32 + (lane & 31)] = acc[q];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kTM * kTN / 4 / kThreads; ++s) {      // a thread: four consecutive columns of a row
        const int slot = t + kThreads * s, rl = slot >> 4, c4 = (slot & 15) * 4;
        const int64_t row = r0 + rl;
        const int n = n0 + c4;
        if (row >= B || n >= D) continue;
        const float* ej = e + ((size_t)row * F + j) * D + n;
        float* xs = x + (size_t)row * ld + (size_t)p * D + n;
        float* xr = xs + rofs;
        const float aa = a ? a[(size_t)row * F + i] * a[(size_t)row * F + j] : 0.f;
        if (vec) {      // D % 4 == 0: the quad is inside the row
            const float4 ev = *reinterpret_cast<const float4*>(ej);
            const float4 r = make_float4(Cs[rl][c4] * ev.x, Cs[rl][c4 + 1] * ev.y, Cs[rl][c4 + 2] * ev.z, Cs[rl][c4 + 3] * ev.w);
            *reinterpret_cast<float4*>(xr) = r;
            if (a) *reinterpret_cast<float4*>(xs) = make_float4(aa * r.x, aa * r.y, aa * r.z, aa * r.w);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (n + c < D) {
                    const float r = Cs[rl][c4 + c] * ej[c];
                    xr[c] = r;
                    if (a) xs[c] = aa * r;
                }
        }
    }
}

// grid: ceil(B / 4).  da [B, F].  dx: the SENet block's gradient at column 0; x: the raw block at column rofs.
__global__ __launch_bounds__(kThreads) void fibinet_bil_da_kernel(const float* __restrict__ a, const float* __restrict__ dx,
                                                                  const float* __restrict__ x, int B, int F, int D, int ld, int rofs,
                                                                  float* __restrict__ da) {
    const int64_t row = (int64_t)blockIdx.x * kFibWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    const float av = lane < F ? a[(size_t)row * F + lane] : 0.f;
    const float* ds = dx + (size_t)row * ld;
    const float* rr = x + (size_t)row * ld + rofs;
    float dav = 0.f;
    int p = 0;
    for (int i = 0; i < F - 1; ++i) {
        const float ai = __shfl(av, i, 64);
        for (int j = i + 1; j < F; ++j, ++p) {
            float tp = 0.f;
            for (int d = lane; d < D; d += 64) tp = fmaf(ds[(size_t)p * D + d], rr[(size_t)p * D + d], tp);
            tp = fib_wave_sum(tp);
            const float aj = __shfl(av, j, 64);
            if (lane == i) dav = fmaf(aj, tp, dav);
            if (lane == j) dav = fmaf(ai, tp, dav);
        }
    }
    if (lane < F) da[(size_t)row * F + lane] = dav;
}

// grid: row tiles x F x ntiles.  de [B, F, D] written.  The i < f partners' elementwise sums are held per (row, four
// consecutive columns) - the product tile goes through LDS, as in the forward - so g_p is read 16 bytes at a time (vec).
__global__ __launch_bounds__(kThreads) void fibinet_bil_dx_kernel(const float* __restrict__ e, const float* __restrict__ w,
                                                                  const float* __restrict__ a, const float* __restrict__ dx, int B,
                                                                  int F, int D, int type, int ntiles, int ld, int rofs, int vec,
                                                                  float* __restrict__ de) {
    __shared__ float As[kTM][kLd];
    __shared__ float Bs[kTN][kLd];
    __shared__ float Cs[kTM][kTN + 1];
    constexpr int kSlots = kTM * kTN / 4 / kThreads;      // a thread: four consecutive columns of kSlots rows
    const int n0 = (blockIdx.x % ntiles) * kTN;
    const int f = (blockIdx.x / ntiles) % F;
    const int64_t r0 = (int64_t)(blockIdx.x / ntiles / F) * kTM;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    const int jf = t & 63, kf0 = t >> 6;      // "i fast"
    const int c4 = (t & 15) * 4, n4 = n0 + c4;
    float sum[kSlots][4], af[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int64_t row = r0 + ((t + kThreads * s) >> 4);
        af[s] = (a && row < B) ? a[(size_t)row * F + f] : 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) sum[s][c] = 0.f;
    }
    auto stage = [&](const f32x16& v) {
#pragma unroll
        for (int q = 0; q < 16; ++q) Cs[wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)][wn * 32 + (lane & 31)] = v[q];
    };
    // f is the pair's second field: de_f += g_p * (W e_i)
    for (int i = 0; i < f; ++i) {
        const int p = pair_index(i, f, F);
        const float* wp = w + (size_t)weight_of(type, i, p) * D * D;
        f32x16 qa = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < D; k0 += kTK) {
            __syncthreads();      // the previous step's fragment reads and the previous partner's tile reads are done
            const int k = k0 + kf;
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                const int64_t row = r0 + if0 + 8 * q;
                const int nn = n0 + if0 + 8 * q;
                As[if0 + 8 * q][kf] = (row < B && k < D) ? e[((size_t)row * F + i) * D + k] : 0.f;
                Bs[if0 + 8 * q][kf] = (nn < D && k < D) ? wp[(size_t)nn * D + k] : 0.f;
            }
            __syncthreads();
            mma_step(As, Bs, lane, wm, wn, qa);
        }
        stage(qa);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const int rl = (t + kThreads * s) >> 4;
            const int64_t row = r0 + rl;
            if (row >= B || n4 >= D) continue;
            const float* xs = dx + (size_t)row * ld + (size_t)p * D + n4;
            const float aa = a ? a[(size_t)row * F + i] * af[s] : 0.f;
            if (vec) {      // D % 4 == 0: the quad is inside the row
                const float4 dr = *reinterpret_cast<const float4*>(xs + rofs);
                float4 g = dr;
                if (a) {
                    const float4 ds = *reinterpret_cast<const float4*>(xs);
                    g = make_float4(fmaf(aa, ds.x, dr.x), fmaf(aa, ds.y, dr.y), fmaf(aa, ds.z, dr.z), fmaf(aa, ds.w, dr.w));
                }
                sum[s][0] = fmaf(g.x, Cs[rl][c4], sum[s][0]);
                sum[s][1] = fmaf(g.y, Cs[rl][c4 + 1], sum[s][1]);
                sum[s][2] = fmaf(g.z, Cs[rl][c4 + 2], sum[s][2]);
                sum[s][3] = fmaf(g.w, Cs[rl][c4 + 3], sum[s][3]);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (n4 + c < D) {
                        const float g = a ? fmaf(aa, xs[c], xs[rofs + c]) : xs[rofs + c];
                        sum[s][c] = fmaf(g, Cs[rl][c4 + c], sum[s][c]);
                    }
            }
        }
    }
    // f is the pair's first field: de_f += (g_p * e_j) W
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = f + 1; j < F; ++j) {
        const int p = pair_index(f, j, F);
        const float* wp = w + (size_t)weight_of(type, f, p) * D * D;
        for (int k0 = 0; k0 < D; k0 += kTK) {
            __syncthreads();
            const int k = k0 + kf;
#pragma unroll 2
            for (int q = 0; q < kPer; ++q) {
                const int64_t row = r0 + if0 + 8 * q;
                As[if0 + 8 * q][kf] = (row < B && k < D)
                                          ? g_of(dx, a, (size_t)row, ld, rofs, F, D, p, f, j, k) * e[((size_t)row * F + j) * D + k]
                                          : 0.f;
                const int nn = n0 + jf, kk = k0 + kf0 + 4 * q;
                Bs[jf][kf0 + 4 * q] = (nn < D && kk < D) ? wp[(size_t)kk * D + nn] : 0.f;
            }
            __syncthreads();
            mma_step(As, Bs, lane, wm, wn, acc);
        }
    }
    __syncthreads();      // the last partner's tile reads are done
    stage(acc);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int rl = (t + kThreads * s) >> 4;
        const int64_t row = r0 + rl;
        if (row >= B || n4 >= D) continue;
        float* out = de + ((size_t)row * F + f) * D + n4;
        if (vec) {
            *reinterpret_cast<float4*>(out) = make_float4(Cs[rl][c4] + sum[s][0], Cs[rl][c4 + 1] + sum[s][1], Cs[rl][c4 + 2] + sum[s][2],
                                                          Cs[rl][c4 + 3] + sum[s][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (n4 + c < D) out[c] = Cs[rl][c4 + c] + sum[s][c];
        }
    }
}

// grid: chunks x nW x (ntiles x ntiles).  part [chunks][nW][D, D]:  part[c][w][n, k] = sum over the pairs p of w (ascending), then
// over the chunk's rows, of (g_p * e_j)[row, n] e_i[row, k].  A weight without pairs leaves zeros.
__global__ __launch_bounds__(kThreads) void fibinet_bil_dw_kernel(const float* __restrict__ e, const float* __restrict__ a,
                                                                  const float* __restrict__ dx, int B, int F, int D, int type, int nW,
                                                                  int ntiles, int ld, int rofs, float* __restrict__ part) {
    __shared__ float As[kTM][kLd];      // [n][row of the step]
    __shared__ float Bs[kTN][kLd];      // [k][row of the step]
    const int per_unit = ntiles * ntiles;
    const int unit = blockIdx.x / per_unit, rem = blockIdx.x % per_unit;
    const int n0 = (rem / ntiles) * kTM, c0 = (rem % ntiles) * kTN;
    const int wi = unit % nW;
    const int64_t r0 = (int64_t)(unit / nW) * kFibChunk;
    const int64_t r1 = r0 + kFibChunk < B ? r0 + kFibChunk : B;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
    // operand loaders: a thread takes column jf of the rows kf0, kf0 + rs, .. of a step.  64 columns x 4 row groups; at D <= 32
    // (one tile, half of it used) 32 columns x 8 row groups, so that no lane idles - the same LDS contents either way.
    const bool narrow = D <= kTK;
    const int jf = narrow ? t & 31 : t & 63, kf0 = narrow ? t >> 5 : t >> 6, rs = narrow ? 8 : 4, cnt = narrow ? kPer / 2 : kPer;
    if (narrow)
        for (int idx = t; idx < kTM * kLd; idx += kThreads) (&As[0][0])[idx] = (&Bs[0][0])[idx] = 0.f;      // rows 32.. stay zero
    // the pairs of weight wi: fields i in [i_lo, i_hi), partners j in [j_lo(i), j_hi(i))
    int i_lo = 0, i_hi = F - 1, j_one = -1;
    if (type == SATRANS_BILINEAR_EACH) i_lo = wi, i_hi = min(wi + 1, F - 1);
    if (type == SATRANS_BILINEAR_INTERACTION) {
        pair_fields(wi, F, i_lo, j_one);
        i_hi = i_lo + 1;
    }
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = i_lo; i < i_hi; ++i) {
        const int j_lo = j_one >= 0 ? j_one : i + 1, j_hi = j_one >= 0 ? j_one + 1 : F;
        for (int j = j_lo; j < j_hi; ++j) {
            const int p = pair_index(i, j, F);
            for (int64_t p0 = r0; p0 < r1; p0 += kTK) {
                __syncthreads();
#pragma unroll 2
                for (int q = 0; q < kPer; ++q) {
                    if (q >= cnt) break;
                    const int64_t row = p0 + kf0 + rs * q;
                    const int n = n0 + jf, c = c0 + jf;
                    As[jf][kf0 + rs * q] = (row < r1 && n < D)
                                               ? g_of(dx, a, (size_t)row, ld, rofs, F, D, p, i, j, n) * e[((size_t)row * F + j) * D + n]
                                               : 0.f;
                    Bs[jf][kf0 + rs * q] = (row < r1 && c < D) ? e[((size_t)row * F + i) * D + c] : 0.f;
                }
                __syncthreads();
                mma_step(As, Bs, lane, wm, wn, acc);
            }
        }
    }
    const int c = c0 + wn * 32 + (lane & 31);
    if (c >= D) return;
    float* out = part + (size_t)unit * D * D;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int n = n0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (n < D) out[(size_t)n * D + c] = acc[q];
    }
}

// dst[row, dofs + c] = src[row, sofs + c], c < n: the dense columns into the DNN input, their gradient out of it
__global__ __launch_bounds__(kThreads) void fibinet_cols_kernel(const float* __restrict__ src, int lds, int sofs, float* __restrict__ dst,
                                                                int ldd, int dofs, int64_t total, int n) {
    const int64_t el = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (el >= total) return;
    const int64_t row = el / n;
    const int c = (int)(el % n);
    dst[(size_t)row * ldd + dofs + c] = src[(size_t)row * lds + sofs + c];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the shapes of a call and what its launches need
struct Fib {
    int B, F, D, R, type, P, nW, ntiles;
    int64_t se_chunks, dw_chunks, tiles;
    int64_t se_part, bil_part;      // floats of the partials of the two backward reductions
};

int fib_shape(Fib& s, int B, int F, int D, int R, int type, const char* who) {
    SATRANS_REQUIRE(B > 0 && F >= 2 && D > 0 && R > 0 && R <= F, SATRANS_E_BADARG, "%s: bad sizes B=%d F=%d D=%d R=%d", who, B, F, D, R);
    SATRANS_REQUIRE(type >= SATRANS_BILINEAR_ALL && type <= SATRANS_BILINEAR_INTERACTION, SATRANS_E_BADARG, "%s: type=%d", who, type);
    SATRANS_REQUIRE(F <= kFibF && D <= kFibD, SATRANS_E_UNSUPPORTED, "%s: F=%d fields, D=%d (at most %d, %d)", who, F, D, kFibF, kFibD);
    s.B = B, s.F = F, s.D = D, s.R = R, s.type = type;
    s.P = F * (F - 1) / 2;
    s.nW = type == SATRANS_BILINEAR_ALL ? 1 : type == SATRANS_BILINEAR_EACH ? F : s.P;
    s.ntiles = (int)ceil_div(D, kTN);
    s.se_chunks = ceil_div(B, kSeChunk), s.dw_chunks = ceil_div(B, kFibChunk), s.tiles = ceil_div(B, kTM);
    s.se_part = 2 * s.se_chunks * F * R;
    s.bil_part = s.dw_chunks * s.nW * D * D;
    SATRANS_REQUIRE(s.tiles * s.P * s.ntiles <= 0x7fffffffLL && s.dw_chunks * s.nW * s.ntiles * s.ntiles <= 0x7fffffffLL &&
                        ceil_div(B, kFibWaves) <= 0x7fffffffLL,
                    SATRANS_E_UNSUPPORTED, "%s: B=%d F=%d D=%d needs more than 2^31 workgroups", who, B, F, D);
    return SATRANS_OK;
}

int se_fwd(const Fib& s, const float* e, const float* w1, const float* w2, float* a, float* hid, float* v, hipStream_t st) {
    fibinet_se_fwd_kernel<<<(unsigned)ceil_div(s.B, kFibWaves), kThreads, 0, st>>>(e, w1, w2, s.B, s.F, s.D, s.R, a, hid, v);
    SATRANS_CHECK_LAUNCH("fibinet_se_fwd_kernel");
    return SATRANS_OK;
}

// de += ; dw1, dw2 written.  part: s.se_part floats
int se_bwd(const Fib& s, const float* e, const float* w1, const float* w2, const float* a, const float* hid, const float* da,
           const float* dv, float* de, float* part, float* dw1, float* dw2, hipStream_t st) {
    const int FR = s.F * s.R;
    float* part2 = part + s.se_chunks * FR;
    fibinet_se_bwd_kernel<<<(unsigned)s.se_chunks, kThreads, 0, st>>>(e, w1, w2, a, hid, da, dv, s.B, s.F, s.D, s.R, de, part, part2);
    SATRANS_CHECK_LAUNCH("fibinet_se_bwd_kernel");
    for (int h = 0; h < 2; ++h) {
        mmoe_reduce_kernel<false><<<(unsigned)ceil_div(FR, kThreads), kThreads, 0, st>>>(h ? part2 : part, nullptr, nullptr, s.B, FR, s.F, 0, 1,
                                                                                        1, (int)s.se_chunks, h ? dw2 : dw1, nullptr);
        SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel (senet)");
    }
    return SATRANS_OK;
}

// x rows of ld floats: [ s | r ] from column 0 (with a), r from column 0 (without)
int bil_fwd(const Fib& s, const float* e, const float* w, const float* a, float* x, int ld, hipStream_t st) {
    const int rofs = a ? s.P * s.D : 0;
    const int vec = s.D % 4 == 0 && ld % 4 == 0 && aligned16(e) && aligned16(x);
    fibinet_bil_fwd_kernel<<<(unsigned)(s.tiles * s.P * s.ntiles), kThreads, 0, st>>>(e, w, a, s.B, s.F, s.D, s.type, s.P, s.ntiles, x, ld,
                                                                                     rofs, vec);
    SATRANS_CHECK_LAUNCH("fibinet_bil_fwd_kernel");
    return SATRANS_OK;
}

// de, dw written; da written (with a).  dx, x rows of ld floats in bil_fwd's layout.  part: s.bil_part floats
int bil_bwd(const Fib& s, const float* e, const float* w, const float* a, const float* dx, const float* x, int ld, float* de, float* da,
            float* part, float* dw, hipStream_t st) {
    const int rofs = a ? s.P * s.D : 0, DD = s.D * s.D;
    fibinet_bil_dw_kernel<<<(unsigned)(s.dw_chunks * s.nW * s.ntiles * s.ntiles), kThreads, 0, st>>>(e, a, dx, s.B, s.F, s.D, s.type, s.nW,
                                                                                                    s.ntiles, ld, rofs, part);
    SATRANS_CHECK_LAUNCH("fibinet_bil_dw_kernel");
    mmoe_reduce_kernel<false><<<(unsigned)ceil_div((int64_t)DD * s.nW, kThreads), kThreads, 0, st>>>(part, nullptr, nullptr, s.B, DD, s.D, 0,
                                                                                                    s.nW, 1, (int)s.dw_chunks, dw, nullptr);
    SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel (bilinear)");
    if (a) {
        fibinet_bil_da_kernel<<<(unsigned)ceil_div(s.B, kFibWaves), kThreads, 0, st>>>(a, dx, x, s.B, s.F, s.D, ld, rofs, da);
        SATRANS_CHECK_LAUNCH("fibinet_bil_da_kernel");
    }
    const int vec = s.D % 4 == 0 && ld % 4 == 0 && aligned16(dx) && aligned16(de);
    fibinet_bil_dx_kernel<<<(unsigned)(s.tiles * s.F * s.ntiles), kThreads, 0, st>>>(e, w, a, dx, s.B, s.F, s.D, s.type, s.ntiles, ld, rofs,
                                                                                    vec, de);
    SATRANS_CHECK_LAUNCH("fibinet_bil_dx_kernel");
    return SATRANS_OK;
}

// the whole head
struct HeadLayout {
    Fib s;
    int ld, dense;              // columns of the DNN input, the dense ones among them
    Rows rows;
    Chain dnn;
    int64_t sv_a, sv_hid, sv_x, saved;                     // saved: a, hid, (up to a multiple of 4 floats,) x, the hidden rows (dnn.s)
    int64_t w_dx, w_buf[2], w_da, w_part, total;           // workspace
};

int head_validate(const satrans_fibinet_desc* d, const char* who, HeadLayout& Y) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->dense_dim >= 0 && d->n_dnn >= 0, SATRANS_E_BADARG, "%s: bad sizes dense_dim=%d n_dnn=%d", who, d->dense_dim, d->n_dnn);
    SATRANS_REQUIRE(d->n_dnn <= kMaxH, SATRANS_E_UNSUPPORTED, "%s: %d hidden layers (at most %d)", who, d->n_dnn, kMaxH);
    for (int l = 0; l < d->n_dnn; ++l) SATRANS_REQUIRE(d->width[l] > 0, SATRANS_E_BADARG, "%s: width[%d]=%d", who, l, d->width[l]);
    if (int rc = fib_shape(Y.s, d->B, d->F, d->D, d->R, d->type, who)) return rc;
    const int64_t ld = 2 * (int64_t)Y.s.P * d->D + d->dense_dim;
    SATRANS_REQUIRE(ld <= 0x7fffffffLL && ceil_div((int64_t)d->B * std::max(d->dense_dim, 1), kThreads) <= 0x7fffffffLL,
                    SATRANS_E_UNSUPPORTED, "%s: B=%d with %lld DNN input columns needs more than 2^31 workgroups", who, d->B, (long long)ld);
    Y.ld = (int)ld, Y.dense = d->dense_dim;
    Y.rows = rows_of(d->B, 0, nullptr, nullptr);
    // (out.bias is the final layer's bias)
    chain_dnn(Y.dnn, false, d->n_dnn, d->width, Y.ld, 1, d->dnn_w, d->dnn_b, d->dnn_linear_w, d->out_bias);
    int64_t part = 0;
    if (int rc = chain_fits(Y.rows, Y.dnn, who, "dnn", part)) return rc;
    const int64_t B = d->B;
    Y.sv_a = 0, Y.sv_hid = B * d->F, Y.sv_x = ceil_div(Y.sv_hid + B * d->R, 4) * 4;      // (x 16-byte aligned in an aligned buffer)
    int64_t at = Y.sv_x + B * ld, wide = 1;
    for (int l = 0; l < d->n_dnn; ++l) {
        Y.dnn.s[l] = at;
        at += B * d->width[l];
        wide = std::max<int64_t>(wide, d->width[l]);
    }
    Y.saved = at;
    Y.w_dx = 0, Y.w_buf[0] = B * ld, Y.w_buf[1] = Y.w_buf[0] + B * wide, Y.w_da = Y.w_buf[1] + B * wide;
    Y.w_part = Y.w_da + B * d->F;
    Y.total = Y.w_part + std::max(part, std::max(Y.s.se_part, Y.s.bil_part));
    return SATRANS_OK;
}

int senet_validate(const satrans_senet_desc* d, const char* who, Fib& s) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    return fib_shape(s, d->B, d->F, d->D, d->R, SATRANS_BILINEAR_ALL, who);
}

int bilinear_validate(const satrans_bilinear_desc* d, const char* who, Fib& s) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    return fib_shape(s, d->B, d->F, d->D, 1, d->type, who);
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_senet_saved_floats(const satrans_senet_desc* d) {
    Fib s;
    const int rc = senet_validate(d, "senet_saved_floats", s);
    return rc ? rc : (int64_t)s.B * (s.F + s.R);
}

extern "C" int64_t satrans_senet_workspace_floats(const satrans_senet_desc* d) {
    Fib s;
    const int rc = senet_validate(d, "senet_workspace_floats", s);
    return rc ? rc : s.se_part;
}

extern "C" int satrans_senet_fwd(const satrans_senet_desc* d, float* v, float* saved, void* stream_) {
    Fib s;
    if (int rc = senet_validate(d, "senet_fwd", s)) return rc;
    SATRANS_REQUIRE(d->e && d->w1 && d->w2 && saved, SATRANS_E_BADARG, "senet_fwd: null pointer");
    return se_fwd(s, d->e, d->w1, d->w2, saved, saved + (int64_t)s.B * s.F, v, (hipStream_t)stream_);
}

extern "C" int satrans_senet_bwd(const satrans_senet_desc* d, const float* da, const float* dv, const float* saved, float* de,
                                 float* workspace, const satrans_senet_grads* g, void* stream_) {
    Fib s;
    if (int rc = senet_validate(d, "senet_bwd", s)) return rc;
    SATRANS_REQUIRE(d->e && d->w1 && d->w2 && (da || dv) && saved && de && workspace && g && g->w1 && g->w2, SATRANS_E_BADARG,
                    "senet_bwd: null pointer");
    return se_bwd(s, d->e, d->w1, d->w2, saved, saved + (int64_t)s.B * s.F, da, dv, de, workspace, g->w1, g->w2, (hipStream_t)stream_);
}

extern "C" int64_t satrans_bilinear_workspace_floats(const satrans_bilinear_desc* d) {
    Fib s;
    const int rc = bilinear_validate(d, "bilinear_workspace_floats", s);
    return rc ? rc : s.bil_part;
}

extern "C" int satrans_bilinear_fwd(const satrans_bilinear_desc* d, float* out, void* stream_) {
    Fib s;
    if (int rc = bilinear_validate(d, "bilinear_fwd", s)) return rc;
    SATRANS_REQUIRE(d->e && d->w && out, SATRANS_E_BADARG, "bilinear_fwd: null pointer");
    return bil_fwd(s, d->e, d->w, d->a, out, (d->a ? 2 : 1) * s.P * s.D, (hipStream_t)stream_);
}

extern "C" int satrans_bilinear_bwd(const satrans_bilinear_desc* d, const float* dout, const float* out, float* de, float* da,
                                    float* workspace, float* dw, void* stream_) {
    Fib s;
    if (int rc = bilinear_validate(d, "bilinear_bwd", s)) return rc;
    SATRANS_REQUIRE(d->e && d->w && dout && out && de && (da || !d->a) && workspace && dw, SATRANS_E_BADARG, "bilinear_bwd: null pointer");
    return bil_bwd(s, d->e, d->w, d->a, dout, out, (d->a ? 2 : 1) * s.P * s.D, de, da, workspace, dw, (hipStream_t)stream_);
}

extern "C" int64_t satrans_fibinet_saved_floats(const satrans_fibinet_desc* d) {
    HeadLayout Y;
    const int rc = head_validate(d, "fibinet_saved_floats", Y);
    return rc ? rc : Y.saved;
}

extern "C" int64_t satrans_fibinet_workspace_floats(const satrans_fibinet_desc* d) {
    HeadLayout Y;
    const int rc = head_validate(d, "fibinet_workspace_floats", Y);
    return rc ? rc : Y.total;
}

extern "C" int satrans_fibinet_fwd(const satrans_fibinet_desc* d, float* logit, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    HeadLayout Y;
    if (int rc = head_validate(d, "fibinet_fwd", Y)) return rc;
    SATRANS_REQUIRE(d->emb && (d->dense || !Y.dense) && d->se_w1 && d->se_w2 && d->bilinear_w && d->out_bias && logit && saved &&
                        chain_has(Y.dnn, d->dnn_w, d->dnn_b, d->dnn_linear_w, false),
                    SATRANS_E_BADARG, "fibinet_fwd: null pointer");
    float* a = saved + Y.sv_a;
    float* x = saved + Y.sv_x;
    // (the up to three floats between hid and the aligned x belong to nobody: zero, so that equal inputs give an equal buffer)
    const int64_t pad0 = Y.sv_hid + (int64_t)d->B * d->R;
    if (Y.sv_x > pad0 && hipMemsetAsync(saved + pad0, 0, (size_t)(Y.sv_x - pad0) * sizeof(float), st) != hipSuccess) {
        set_error("fibinet_fwd: hipMemsetAsync failed");
        return SATRANS_E_LAUNCH;
    }
    if (int rc = se_fwd(Y.s, d->emb, d->se_w1, d->se_w2, a, saved + Y.sv_hid, nullptr, st)) return rc;
    if (int rc = bil_fwd(Y.s, d->emb, d->bilinear_w, a, x, Y.ld, st)) return rc;
    if (Y.dense) {
        const int64_t total = (int64_t)d->B * Y.dense;
        fibinet_cols_kernel<<<(unsigned)ceil_div(total, kThreads), kThreads, 0, st>>>(d->dense, Y.dense, 0, x, Y.ld, Y.ld - Y.dense, total,
                                                                                     Y.dense);
        SATRANS_CHECK_LAUNCH("fibinet_cols_kernel");
    }
    return dnn_fwd<false>(Y.rows, Y.dnn, x, saved, logit, st);
}

extern "C" int satrans_fibinet_bwd(const satrans_fibinet_desc* d, const float* dlogit, float* demb, float* ddense, const float* saved,
                                   float* workspace, const satrans_fibinet_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    HeadLayout Y;
    if (int rc = head_validate(d, "fibinet_bwd", Y)) return rc;
    SATRANS_REQUIRE(d->emb && d->se_w1 && d->se_w2 && d->bilinear_w && d->out_bias && dlogit && demb && (ddense || !Y.dense) && saved &&
                        workspace && g && g->se_w1 && g->se_w2 && g->bilinear_w && g->out_bias &&
                        chain_has(Y.dnn, d->dnn_w, d->dnn_b, d->dnn_linear_w, false) &&
                        chain_has(Y.dnn, g->dnn_w, g->dnn_b, g->dnn_linear_w, false),
                    SATRANS_E_BADARG, "fibinet_bwd: null pointer");
    set_grads(Y.dnn, g->dnn_w, g->dnn_b, g->dnn_linear_w, g->out_bias, false);
    const float* a = saved + Y.sv_a;
    const float* x = saved + Y.sv_x;
    float* dx = workspace + Y.w_dx;
    float* buf[2] = {workspace + Y.w_buf[0], workspace + Y.w_buf[1]};
    float* da = workspace + Y.w_da;
    float* part = workspace + Y.w_part;
    int cur = 0;
    if (int rc = dnn_bwd<false>(Y.rows, Y.dnn, dlogit, x, saved, 0, dx, buf, cur, part, st)) return rc;
    if (Y.dense) {
        const int64_t total = (int64_t)d->B * Y.dense;
        fibinet_cols_kernel<<<(unsigned)ceil_div(total, kThreads), kThreads, 0, st>>>(dx, Y.ld, Y.ld - Y.dense, ddense, Y.dense, 0, total,
                                                                                     Y.dense);
        SATRANS_CHECK_LAUNCH("fibinet_cols_kernel");
    }
    if (int rc = bil_bwd(Y.s, d->emb, d->bilinear_w, a, dx, x, Y.ld, demb, da, part, g->bilinear_w, st)) return rc;
    return se_bwd(Y.s, d->emb, d->se_w1, d->se_w2, a, saved + Y.sv_hid, da, nullptr, demb, part, g->se_w1, g->se_w2, st);
}
