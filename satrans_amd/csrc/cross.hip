// DCN's cross network (deepctr-torch 0.2.9's `CrossNet`, which the reference's models/dcn.py:70,101 calls), vector and matrix
// forms.  With x0 = inputs [B, N], x_0 = x0, kernels w [L, N] (vector) or W [L, N, N] (matrix, W_l [n_out, n_in]), bias [L, N]:
//     vector   s_l[b]   = sum_n x_l[b,n] w_l[n]            x_{l+1} = x0 s_l[b] + b_l + x_l
//     matrix   u_l[b,:] = W_l x_l[b,:] + b_l               x_{l+1} = x0 * u_l + x_l                      result = x_L
// and backward, g_L = dresult, l = L-1 .. 0:
//     vector   ds_l[b] = sum_n g_{l+1}[b,n] x0[b,n]        dx0 += g_{l+1} s_l[b]       g_l = g_{l+1} + w_l ds_l[b]
//              dw_l[n] = sum_b ds_l[b] x_l[b,n]            db_l[n] = sum_b g_{l+1}[b,n]
//     matrix   du_l = g_{l+1} * x0                         dx0 += g_{l+1} * u_l        g_l = g_{l+1} + du_l W_l
//              dW_l[o,k] = sum_b du_l[b,o] x_l[b,k]        db_l[o] = sum_b du_l[b,o]
//     finally  dx0 += g_0
//
// VECTOR form: 3 N FLOP per sample and layer - memory traffic and launches, so the whole stack is one launch each way.
//   cross_vec_fwd_kernel<Q>   a wave per row, the row in registers over all L layers: lane i holds the quads (4 consecutive
//                             columns) i, 64 + i, .. of Q quads, loaded with 16-byte loads when N % 4 == 0 and the pointers allow
//                             and with four scalar loads otherwise - the SAME lane owns the same columns either way, so the bits
//                             do not depend on alignment.  s_l = the lane's columns ascending (an fmaf chain), then the 64 lanes by
//                             a fixed xor butterfly.  x0 is read once, x_L written once; saved = s [B, L] and nothing else.
//   cross_vec_bwd_kernel<Q>   a workgroup (8 waves, 4 from Q = 12) owns a chunk of kVecChunk rows.  Phase 1, a wave per row, layers in reverse, g and dx0
//                             in registers: ds_l, dx0 (written).  Since x_l = A_l x0 + c_l with A_l[b] = 1 + sum_{j<l} s_j[b] and
//                             c_l[n] = sum_{j<l} b_j[n], and g_{l+1} = g_L + sum_{j>l} w_j ds_j, the column sums of the chunk are
//                                 dw_l[n] = sum_b (ds_l A_l)[b] x0[b,n] + c_l[n] sum_b ds_l[b]
//                                 db_l[n] = sum_b g_L[b,n] + sum_{j>l} w_j[n] sum_b ds_j[b]
//                             so a row leaves 2 L scalars in LDS (ds_l A_l, ds_l).  Phase 2, a thread per column (columns t,
//                             t + threads, ..): the chunk's rows in order, L + 1 running sums (not 2 L N / 64 per lane), x0 and dy of
//                             the chunk read a second time while they are still in cache; the chunk's partials [L N | L N].
//   cross_vec_reduce_kernel   the ordered reduce of the partials: eight contiguous shares of the chunks, each in chunk order,
//                             added in share order.
// MATRIX form: a [B,N] x [N,N] product per layer.
//   cross_mat_fwd_kernel      one launch per layer: grouped_gemm.h's 64 x 64 tile product (mma_step, steps of 32, four waves) with
//                             the epilogue u = acc + b_l[n] (stored), x_{l+1} = x0 u + x_l read at the output's own place.
//   cross_mat_du_kernel       per layer of the backward, a thread per element (the same thread in every launch):
//                             du = g * x0, dx0 (+)= g * u_l; the first launch also copies dresult into the g buffer.
//   head_layers.h's launch_bwd<false>   dW_l, db_l from (du, x_l) through chunk partials and the ordered reduce, and
//                             g += du W_l into the g buffer.
//   cross_mat_fin_kernel      dx0 += g_0
// saved (matrix) = u_0 .. u_{L-1}, then x_1 .. x_{L-1}: (2 L - 1) B N floats.
// No floating-point atomics; every sum has a fixed order, so equal inputs give equal bits, and a sample's result row and dx0 row
// are the same bits alone as inside a batch (the parameter gradients sum over all rows).  fp32 only.
#include "head_layers.h"

namespace satrans {
namespace {

constexpr int kCrossL = SATRANS_CROSS_MAX_LAYERS;
constexpr int kCrossN = SATRANS_CROSS_MAX_FEATURES;
constexpr int kVecChunk = SATRANS_CROSS_VEC_ROW_CHUNK;
constexpr int kWaves = kThreads / 64;      // rows of a workgroup of the vector forward: a wave each
static_assert(kCrossN % 256 == 0 && kCrossN / 256 <= 16, "a lane holds at most 16 quads");
static_assert(kCrossL <= 64 && kVecChunk % 8 == 0, "the saved scalars of a row sit in one wave's lanes");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// quad q of the lane = columns 4 (64 q + lane) .. + 3 of a row of N floats; columns >= N read as zero and are not stored
template <int Q>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int N, int lane, int vec, float (&v)[Q][4]) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int n = 4 * (64 * q + lane);
        if (vec) {      // N % 4 == 0: a quad is inside the row or outside it
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < N) f = *reinterpret_cast<const float4*>(p + n);
            v[q][0] = f.x, v[q][1] = f.y, v[q][2] = f.z, v[q][3] = f.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[q][j] = n + j < N ? p[n + j] : 0.f;
        }
    }
}

template <int Q>
__device__ __forceinline__ void store_row(float* __restrict__ p, int N, int lane, int vec, const float (&v)[Q][4]) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int n = 4 * (64 * q + lane);
        if (vec) {
            if (n < N) *reinterpret_cast<float4*>(p + n) = make_float4(v[q][0], v[q][1], v[q][2], v[q][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < N) p[n + j] = v[q][j];
        }
    }
}

// grid: ceil(B / kWaves).  256 Q >= N.
template <int Q>
__global__ __launch_bounds__(kThreads) void cross_vec_fwd_kernel(const float* __restrict__ x0, int B, int N, int L, int vec,
                                                                 const float* __restrict__ w, const float* __restrict__ bias,
                                                                 float* __restrict__ result, float* __restrict__ s_out) {
    const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    float a[Q][4], x[Q][4];
    load_row<Q>(x0 + (size_t)row * N, N, lane, vec, a);
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) x[q][j] = a[q][j];
    for (int l = 0; l < L; ++l) {
        float p[Q][4];
        load_row<Q>(w + (size_t)l * N, N, lane, vec, p);
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) s = fmaf(x[q][j], p[q][j], s);
        s = wave_sum(s);
        if (lane == 0) s_out[(size_t)row * L + l] = s;
        load_row<Q>(bias + (size_t)l * N, N, lane, vec, p);
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) x[q][j] = fmaf(a[q][j], s, p[q][j]) + x[q][j];
    }
    store_row<Q>(result + (size_t)row * N, N, lane, vec, x);
}

// grid: ceil(B / kVecChunk), TPB threads (8 waves while a row's registers allow two waves per SIMD, else 4).
// part_w, part_b [chunks][L, N].
template <int Q, int TPB>
__global__ __launch_bounds__(TPB) void cross_vec_bwd_kernel(const float* __restrict__ x0, const float* __restrict__ dy, int B, int N,
                                                                 int L, int vec, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, const float* __restrict__ s_saved,
                                                                 float* __restrict__ dx0, float* __restrict__ part_w,
                                                                 float* __restrict__ part_b) {
    __shared__ float al[kVecChunk][kCrossL];       // ds_l A_l of the chunk's rows
    __shared__ float dsl[kVecChunk][kCrossL];      // ds_l
    __shared__ float beta[kCrossL];                // sum of ds_l over the chunk's rows
    const int64_t r0 = (int64_t)blockIdx.x * kVecChunk;
    const int nr = (int)(B - r0 < kVecChunk ? B - r0 : kVecChunk);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int r = wv; r < nr; r += TPB / 64) {
        const size_t at = (size_t)(r0 + r) * N;
        float a[Q][4], g[Q][4], dx[Q][4];
        load_row<Q>(x0 + at, N, lane, vec, a);
        load_row<Q>(dy + at, N, lane, vec, g);
        // lane l holds s_l and A_l = 1 + s_0 + .. + s_{l-1}
        const float sv = lane < L ? s_saved[(size_t)(r0 + r) * L + lane] : 0.f;
        float Av = 1.f, run = 1.f;
        for (int j = 0; j < L; ++j) {
            if (lane == j) Av = run;
            run += __shfl(sv, j, 64);
        }
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) dx[q][j] = 0.f;
        for (int l = L - 1; l >= 0; --l) {
            float p[Q][4];
            load_row<Q>(w + (size_t)l * N, N, lane, vec, p);
            const float s = __shfl(sv, l, 64), A = __shfl(Av, l, 64);
            float ds = 0.f;
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) ds = fmaf(g[q][j], a[q][j], ds);
            ds = wave_sum(ds);
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    dx[q][j] = fmaf(g[q][j], s, dx[q][j]);
                    g[q][j] = fmaf(p[q][j], ds, g[q][j]);
                }
            if (lane == 0) {
                al[r][l] = ds * A;
                dsl[r][l] = ds;
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) dx[q][j] += g[q][j];
        store_row<Q>(dx0 + at, N, lane, vec, dx);
    }
    __syncthreads();
    if (t < L) {
        float b = 0.f;
        for (int r = 0; r < nr; ++r) b += dsl[r][t];
        beta[t] = b;
    }
    __syncthreads();
    float* pw = part_w + (size_t)blockIdx.x * L * N;
    float* pb = part_b + (size_t)blockIdx.x * L * N;
    for (int c = t; c < N; c += TPB) {
        const float* xc = x0 + (size_t)r0 * N + c;
        const float* gc = dy + (size_t)r0 * N + c;
        float G = 0.f, P[kCrossL];
#pragma unroll
        for (int l = 0; l < kCrossL; ++l) P[l] = 0.f;
        for (int rb = 0; rb < nr; rb += 8) {      // eight rows' loads in flight; the sums stay in row order
            float xv[8], gv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool ok = rb + i < nr;
                xv[i] = ok ? xc[(size_t)(rb + i) * N] : 0.f;
                gv[i] = ok ? gc[(size_t)(rb + i) * N] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (rb + i < nr) {      // (al of a row past the chunk's end is not written)
                    G += gv[i];
#pragma unroll
                    for (int l = 0; l < kCrossL; ++l)
                        if (l < L) P[l] = fmaf(al[rb + i][l], xv[i], P[l]);
                }
            }
        }
        float cl = 0.f;      // c_l[c]
#pragma unroll
        for (int l = 0; l < kCrossL; ++l)
            if (l < L) {
                pw[(size_t)l * N + c] = fmaf(cl, beta[l], P[l]);
                cl += bias[(size_t)l * N + c];
            }
        float tail = 0.f;      // sum over j > l of w_j[c] beta_j
        for (int l = L - 1; l >= 0; --l) {
            pb[(size_t)l * N + c] = G + tail;
            tail = fmaf(w[(size_t)l * N + c], beta[l], tail);
        }
    }
}

// The ordered reduce of the vector form's partials part [chunks][E] into out [E] (E = L N, kernels then bias: two reduces
// in one, part_b / out_b behind part_w / out_w).  A workgroup = 32 elements x 8 groups: group q adds its contiguous
// share of the chunks in chunk order (in double), the eight group sums are added in group order.
__global__ __launch_bounds__(kThreads) void cross_vec_reduce_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                                    int E, int nchunks, float* __restrict__ out_w,
                                                                    float* __restrict__ out_b) {
    __shared__ double sums[8][32];
    const int j = threadIdx.x & 31, q = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + j;      // over [0, 2 E)
    const bool live = e < 2 * E;
    const float* part = e < E ? part_w + e : part_b + (e - E);
    const int per = (nchunks + 7) / 8, k0 = q * per, k1 = min(k0 + per, nchunks);
    double sum = 0.0;
    if (live)
        for (int k = k0; k < k1; ++k) sum += part[(size_t)k * E];
    sums[q][j] = sum;
    __syncthreads();
    if (q == 0 && live) {
        double total = sums[0][j];
#pragma unroll
        for (int i = 1; i < 8; ++i) total += sums[i][j];
        (e < E ? out_w + e : out_b + (e - E))[0] = (float)total;
    }
}

// workgroup = (row tile of 64) x (tile of 64 output columns) of layer l:  u[row, n] = sum_k xl[row, k] W[n, k] + bias[n],
// xn[row, n] = x0[row, n] u[row, n] + xl[row, n].  xn is not xl.   grid: row tiles x n tiles
__global__ __launch_bounds__(kThreads) void cross_mat_fwd_kernel(const float* __restrict__ x0, const float* __restrict__ xl, int B, int N,
                                                                 int ntiles, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, float* __restrict__ u,
                                                                 float* __restrict__ xn) {
    __shared__ float As[kTM][kLd];
    __shared__ float Bs[kTN][kLd];
    const int n0 = (blockIdx.x % ntiles) * kTN;
    const int64_t r0 = (int64_t)(blockIdx.x / ntiles) * kTM;
    const int t = threadIdx.x, lane = t & 63, wvv = t >> 6, wm = wvv & 1, wn = wvv >> 1;
    const int kf = t & 31, if0 = t >> 5;      // "k fast"
    float ra[kPer], rb[kPer];
    auto load = [&](int k0) {
        const int k = k0 + kf;
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int64_t row = r0 + if0 + 8 * e;
            const int n = n0 + if0 + 8 * e;
            ra[e] = (row < B && k < N) ? xl[(size_t)row * N + k] : 0.f;
            rb[e] = (n < N && k < N) ? w[(size_t)n * N + k] : 0.f;
        }
    };
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    load(0);
    for (int k0 = 0; k0 < N; k0 += kTK) {
        __syncthreads();      // the previous step's fragment reads are done
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            As[if0 + 8 * e][kf] = ra[e];
            Bs[if0 + 8 * e][kf] = rb[e];
        }
        __syncthreads();
        if (k0 + kTK < N) load(k0 + kTK);
        mma_step(As, Bs, lane, wm, wn, acc);
    }
    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= N) return;
    const float bv = bias[n];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int64_t row = r0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (row >= B) continue;
        const size_t at = (size_t)row * N + n;
        const float uv = acc[q] + bv;
        u[at] = uv;
        xn[at] = fmaf(x0[at], uv, xl[at]);
    }
}

// du = g * x0;  dx0 = g * u (first) or dx0 + g * u;  first: gbuf = g (g is dresult then, gbuf afterwards)
__global__ __launch_bounds__(kThreads) void cross_mat_du_kernel(const float* __restrict__ g, const float* __restrict__ x0,
                                                                const float* __restrict__ u, int64_t total, int first,
                                                                float* __restrict__ du, float* __restrict__ dx0, float* gbuf) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const float gv = g[e];
    du[e] = gv * x0[e];
    dx0[e] = first ? gv * u[e] : fmaf(gv, u[e], dx0[e]);
    if (first) gbuf[e] = gv;
}

__global__ __launch_bounds__(kThreads) void cross_mat_fin_kernel(const float* __restrict__ g, int64_t total, float* __restrict__ dx0) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < total) dx0[e] += g[e];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

struct CrossLayout {
    int64_t BN, chunks;                        // B N; row chunks of the vector backward
    int64_t saved;                             // vector: s [B, L];  matrix: u_l [L][B, N], then x_1 .. x_{L-1}
    int64_t w_du, w_g, w_part, total;          // matrix workspace: du, g, partials;  vector: part_w at w_part, part_b behind it
    Rows rows;
};

int cross_validate(const satrans_cross_desc* d, const char* who, CrossLayout& Y) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->N > 0 && d->L > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d N=%d L=%d", who, d->B, d->N, d->L);
    SATRANS_REQUIRE(d->matrix == 0 || d->matrix == 1, SATRANS_E_BADARG, "%s: matrix=%d", who, d->matrix);
    SATRANS_REQUIRE(d->L <= kCrossL && d->N <= kCrossN, SATRANS_E_UNSUPPORTED, "%s: L=%d layers, N=%d features (at most %d, %d)", who,
                    d->L, d->N, kCrossL, kCrossN);
    Y.BN = (int64_t)d->B * d->N;
    Y.chunks = ceil_div(d->B, kVecChunk);
    Y.rows = rows_of(d->B, 0, nullptr, nullptr);
    if (!d->matrix) {
        Y.saved = (int64_t)d->B * d->L;
        Y.w_du = Y.w_g = Y.w_part = 0;
        Y.total = 2 * Y.chunks * d->L * d->N;
        return SATRANS_OK;
    }
    SATRANS_REQUIRE(ceil_div(Y.BN, kThreads) <= 0x7fffffffLL, SATRANS_E_UNSUPPORTED, "%s: B=%d N=%d needs more than 2^31 workgroups", who,
                    d->B, d->N);
    const int64_t part = layer_part(Y.rows, false, Lyr{d->N, d->N, 1, nullptr, nullptr, nullptr, nullptr}, who, "cross", 0);
    if (part < 0) return (int)part;
    Y.saved = (2 * (int64_t)d->L - 1) * Y.BN;
    Y.w_du = 0, Y.w_g = Y.BN, Y.w_part = 2 * Y.BN;
    Y.total = Y.w_part + part;
    return SATRANS_OK;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the smallest built Q with 256 Q >= N
#define CROSS_DISPATCH_Q(N, CALL)        \
    do {                                 \
        const int q__ = ((N) + 255) / 256; \
        if (q__ <= 1) { CALL(1); }       \
        else if (q__ <= 2) { CALL(2); }  \
        else if (q__ <= 3) { CALL(3); }  \
        else if (q__ <= 4) { CALL(4); }  \
        else if (q__ <= 6) { CALL(6); }  \
        else if (q__ <= 8) { CALL(8); }  \
        else if (q__ <= 12) { CALL(12); } \
        else { CALL(16); }               \
    } while (0)

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_cross_saved_floats(const satrans_cross_desc* d) {
    CrossLayout Y;
    const int rc = cross_validate(d, "cross_saved_floats", Y);
    return rc ? rc : Y.saved;
}

extern "C" int64_t satrans_cross_workspace_floats(const satrans_cross_desc* d) {
    CrossLayout Y;
    const int rc = cross_validate(d, "cross_workspace_floats", Y);
    return rc ? rc : Y.total;
}

extern "C" int satrans_cross_fwd(const satrans_cross_desc* d, float* result, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    CrossLayout Y;
    const int rc = cross_validate(d, "cross_fwd", Y);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x0 && d->kernels && d->bias && result && saved, SATRANS_E_BADARG, "cross_fwd: null pointer");
    const int B = d->B, N = d->N, L = d->L;
    if (!d->matrix) {
        const int vec = N % 4 == 0 && aligned16(d->x0) && aligned16(d->kernels) && aligned16(d->bias) && aligned16(result);
#define CROSS_FWD(Q) \
    cross_vec_fwd_kernel<Q><<<(unsigned)ceil_div(B, kWaves), kThreads, 0, st>>>(d->x0, B, N, L, vec, d->kernels, d->bias, result, saved)
        CROSS_DISPATCH_Q(N, CROSS_FWD);
#undef CROSS_FWD
        SATRANS_CHECK_LAUNCH("cross_vec_fwd_kernel");
        return SATRANS_OK;
    }
    const int ntiles = (int)ceil_div(N, kTN);
    for (int l = 0; l < L; ++l) {
        const float* xl = l == 0 ? d->x0 : saved + (L + l - 1) * Y.BN;
        float* xn = l == L - 1 ? result : saved + (L + l) * Y.BN;
        cross_mat_fwd_kernel<<<(unsigned)(Y.rows.tiles * ntiles), kThreads, 0, st>>>(d->x0, xl, B, N, ntiles, d->kernels + (size_t)l * N * N,
                                                                                    d->bias + (size_t)l * N, saved + l * Y.BN, xn);
        SATRANS_CHECK_LAUNCH("cross_mat_fwd_kernel");
    }
    return SATRANS_OK;
}

extern "C" int satrans_cross_bwd(const satrans_cross_desc* d, const float* dresult, float* dx0, const float* saved, float* workspace,
                                 const satrans_cross_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    CrossLayout Y;
    const int rc = cross_validate(d, "cross_bwd", Y);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x0 && d->kernels && d->bias && dresult && dx0 && saved && workspace && g && g->kernels && g->bias,
                    SATRANS_E_BADARG, "cross_bwd: null pointer");
    const int B = d->B, N = d->N, L = d->L;
    if (!d->matrix) {
        const int vec = N % 4 == 0 && aligned16(d->x0) && aligned16(d->kernels) && aligned16(dresult) && aligned16(dx0);
        float* part_w = workspace + Y.w_part;
        float* part_b = part_w + Y.chunks * L * N;
#define CROSS_BWD(Q)                                                                                                              \
    cross_vec_bwd_kernel<Q, (Q <= 8 ? 512 : 256)><<<(unsigned)Y.chunks, (Q <= 8 ? 512 : 256), 0, st>>>(                             \
        d->x0, dresult, B, N, L, vec, d->kernels, d->bias, saved, dx0, part_w, part_b)
        CROSS_DISPATCH_Q(N, CROSS_BWD);
#undef CROSS_BWD
        SATRANS_CHECK_LAUNCH("cross_vec_bwd_kernel");
        const int LN = L * N;
        cross_vec_reduce_kernel<<<(unsigned)ceil_div(2 * LN, 32), kThreads, 0, st>>>(part_w, part_b, LN, (int)Y.chunks, g->kernels,
                                                                                     g->bias);
        SATRANS_CHECK_LAUNCH("cross_vec_reduce_kernel");
        return SATRANS_OK;
    }
    float* du = workspace + Y.w_du;
    float* gb = workspace + Y.w_g;
    float* part = workspace + Y.w_part;
    const unsigned egrid = (unsigned)ceil_div(Y.BN, kThreads);
    for (int l = L - 1; l >= 0; --l) {
        const int first = l == L - 1;
        cross_mat_du_kernel<<<egrid, kThreads, 0, st>>>(first ? dresult : gb, d->x0, saved + l * Y.BN, Y.BN, first, du, dx0, gb);
        SATRANS_CHECK_LAUNCH("cross_mat_du_kernel");
        const float* xl = l == 0 ? d->x0 : saved + (L + l - 1) * Y.BN;
        const Lyr y{N, N, 1, d->kernels + (size_t)l * N * N, d->bias + (size_t)l * N, g->kernels + (size_t)l * N * N, g->bias + (size_t)l * N};
        if (int rc2 = launch_bwd<false>(Y.rows, y, du, N, xl, N, 0, false, 1, gb, part, st)) return rc2;
    }
    cross_mat_fin_kernel<<<egrid, kThreads, 0, st>>>(gb, Y.BN, dx0);
    SATRANS_CHECK_LAUNCH("cross_mat_fin_kernel");
    return SATRANS_OK;
}
