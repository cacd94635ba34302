// Partitioned normalisation: one batch-norm per scenario (the reference's MDR_BatchNorm, models/submodules.py:107-175, as
// star.py:147-154 loops over it), every scenario of a batch in one pass.
//
// Layout.  x [B,C] stays in the caller's row order; a scenario's run is cut into chunks of kRowChunk rows and the grid is sized
// in slots, as seg_walk.h describes.  A workgroup owns (one chunk) x (one tile of kChanTile adjacent channels).  Its 64 lanes
// run along the channels, so a wave reads 256 contiguous bytes of a row; its kWaves waves take the chunk's rows round-robin
// (wave w: rows w, w + kWaves, ...), kRowsPerThread rows per lane, all loaded before the first use.
//
// Reduction order (fixed; no floating-point atomics, so equal inputs give equal bits):
//   lane     its <= kRowsPerThread rows around a pivot (its first row): d = x - pivot is exact for values of one magnitude,
//            mean = pivot + sum(d) / n, M2 = sum((d - sum(d)/n)^2).  Never E[x^2] - E[x]^2.
//   block    the kWaves lane results of a channel, Chan's merge in wave order      -> one (count, mean, M2) per (chunk, channel)
//   finalise the chunks of a (scenario, channel): kGroups groups merge contiguous shares in chunk order, then the group
//            results in group order.  The merges run in fp64 (a handful per channel); the stored partials are fp32.
// The backward's two sums (dy, dy * xhat) go the same way with plain additions.
#include "seg_walk.h"

namespace satrans {
namespace {

constexpr int kChanTile = 64;
constexpr int kRowChunk = SATRANS_PNORM_ROW_CHUNK;
constexpr int kWaves = 4;
constexpr int kGroups = 4;
constexpr int kThreads = kChanTile * kWaves;
constexpr int kRowsPerThread = kRowChunk / kWaves;
static_assert(kChanTile == kWave, "lanes run along the channels of a tile");
static_assert(kRowChunk % kWaves == 0 && kRowsPerThread <= 32, "row mask is 32 bits");
static_assert(kGroups == kWaves, "the finalise kernels reuse the block shape");

// row j of wave w in the chunk, or -1
__device__ __forceinline__ int chunk_row(const int32_t* __restrict__ order, const SegSlotN& sl, int w, int j, int B) {
    return row_at(order, sl.r0 + w + j * kWaves, sl.r1, B);
}

struct Moments {
    double n, mean, m2;
};

// Chan et al.: the moments of the union of two sets
__device__ __forceinline__ void merge(Moments& a, double nb, double mb, double m2b) {
    if (nb == 0.0) return;
    if (a.n == 0.0) {
        a = Moments{nb, mb, m2b};
        return;
    }
    const double n = a.n + nb, delta = mb - a.mean;
    a.mean += delta * (nb / n);
    a.m2 += m2b + delta * delta * (a.n * nb / n);
    a.n = n;
}

// ---- forward --------------------------------------------------------------------------------------------------------------

// part [slots][3][C]: count, mean, M2 of (chunk, channel)
__global__ __launch_bounds__(kThreads) void pnorm_stats_kernel(const float* __restrict__ x, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ seg, int B, int C, int S, int ctiles,
                                                               float* __restrict__ part) {
    __shared__ float sh[3][kWaves][kChanTile];
    const int slot = blockIdx.x / ctiles, ct = blockIdx.x % ctiles;
    const SegSlotN sl = find_slot<SegSlotN>(seg, S, B, slot, kRowChunk);
    if (sl.s < 0) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = ct * kChanTile + lane;
    float cnt = 0.f, mean = 0.f, m2 = 0.f;
    if (c < C) {
        float v[kRowsPerThread];
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < kRowsPerThread; ++j) {
            const int row = chunk_row(order, sl, w, j, B);
            v[j] = 0.f;
            if (row >= 0) {
                v[j] = x[(size_t)row * C + c];
                ok |= 1u << j;
            }
        }
        if (ok) {
            float pivot = 0.f, dsum = 0.f;
#pragma unroll
            for (int j = kRowsPerThread - 1; j >= 0; --j)
                if (ok >> j & 1) pivot = v[j];      // (the first of its rows; selects, no indexed register read)
#pragma unroll
            for (int j = 0; j < kRowsPerThread; ++j) {
                v[j] -= pivot;
                if (ok >> j & 1) dsum += v[j];
            }
            cnt = (float)__popc(ok);
            const float dmean = dsum / cnt;
#pragma unroll
            for (int j = 0; j < kRowsPerThread; ++j) {
                const float e = v[j] - dmean;
                if (ok >> j & 1) m2 = fmaf(e, e, m2);
            }
            mean = pivot + dmean;
        }
    }
    sh[0][w][lane] = cnt;
    sh[1][w][lane] = mean;
    sh[2][w][lane] = m2;
    __syncthreads();
    if (w == 0 && c < C) {
        Moments m{0.0, 0.0, 0.0};
#pragma unroll
        for (int g = 0; g < kWaves; ++g) merge(m, sh[0][g][lane], sh[1][g][lane], sh[2][g][lane]);
        float* out = part + (size_t)slot * 3 * C + c;
        out[0] = (float)m.n;
        out[(size_t)C] = (float)m.mean;
        out[(size_t)2 * C] = (float)m.m2;
    }
}

// grid (ctiles, S): merges the chunks of (scenario, channel), writes saved = [mean | invstd], updates the running statistics
__global__ __launch_bounds__(kThreads) void pnorm_finalize_kernel(const float* __restrict__ part, const int32_t* __restrict__ seg,
                                                                  int B, int C, int S, float eps, float factor,
                                                                  float* __restrict__ saved, float* __restrict__ running_mean,
                                                                  float* __restrict__ running_var) {
    __shared__ double sh[3][kGroups][kChanTile];
    const int s = blockIdx.y, lane = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.x * kChanTile + lane;
    const int k0 = first_slot(seg, s, B, kRowChunk), nch = scenario_units(seg, s, B, kRowChunk);
    const int per = (nch + kGroups - 1) / kGroups;
    Moments m{0.0, 0.0, 0.0};
    if (c < C) {
        for (int k = k0 + g * per; k < min(k0 + nch, k0 + (g + 1) * per); ++k) {
            const float* in = part + (size_t)k * 3 * C + c;
            merge(m, in[0], in[(size_t)C], in[(size_t)2 * C]);
        }
    }
    sh[0][g][lane] = m.n;
    sh[1][g][lane] = m.mean;
    sh[2][g][lane] = m.m2;
    __syncthreads();
    if (g != 0 || c >= C) return;
    Moments t{0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < kGroups; ++q) merge(t, sh[0][q][lane], sh[1][q][lane], sh[2][q][lane]);
    const size_t at = (size_t)s * C + c, SC = (size_t)S * C;
    if (t.n == 0.0) {      // no rows: nothing to normalise, running statistics untouched
        saved[at] = 0.f;
        saved[SC + at] = 0.f;
        return;
    }
    const double var = t.m2 / t.n;
    saved[at] = (float)t.mean;
    saved[SC + at] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean && running_var && t.n > 1.0) {
        const float unbiased = (float)(t.m2 / (t.n - 1.0));
        running_mean[at] = (1.f - factor) * running_mean[at] + factor * (float)t.mean;
        running_var[at] = (1.f - factor) * running_var[at] + factor * unbiased;
    }
}

// evaluation: saved = [running_mean | 1 / sqrt(running_var + eps)]
__global__ __launch_bounds__(256) void pnorm_running_kernel(const float* __restrict__ running_mean,
                                                            const float* __restrict__ running_var, int64_t SC, float eps,
                                                            float* __restrict__ saved) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= SC) return;
    saved[i] = running_mean[i];
    saved[SC + i] = (float)(1.0 / sqrt((double)running_var[i] + (double)eps));
}

__global__ __launch_bounds__(kThreads) void pnorm_apply_kernel(const float* __restrict__ x, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ seg, int B, int C, int S, int ctiles,
                                                               const float* __restrict__ saved, const float* __restrict__ weight,
                                                               const float* __restrict__ bias, const float* __restrict__ shared_w,
                                                               const float* __restrict__ shared_b, float* __restrict__ y) {
    const int slot = blockIdx.x / ctiles, ct = blockIdx.x % ctiles;
    const SegSlotN sl = find_slot<SegSlotN>(seg, S, B, slot, kRowChunk);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = ct * kChanTile + lane;
    if (sl.s < 0 || c >= C) return;
    const size_t at = (size_t)sl.s * C + c;
    const float mean = saved[at], a = saved[(size_t)S * C + at] * (weight[at] * shared_w[c]), b = bias[at] + shared_b[c];
#pragma unroll 8
    for (int j = 0; j < kRowsPerThread; ++j) {
        const int row = chunk_row(order, sl, w, j, B);
        if (row >= 0) y[(size_t)row * C + c] = fmaf(x[(size_t)row * C + c] - mean, a, b);
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------

// part [slots][2][C]: sum(dy), sum(dy * xhat) of (chunk, channel)
__global__ __launch_bounds__(kThreads) void pnorm_bwd_stats_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                   const int32_t* __restrict__ order,
                                                                   const int32_t* __restrict__ seg, int B, int C, int S,
                                                                   int ctiles, const float* __restrict__ saved,
                                                                   float* __restrict__ part) {
    __shared__ float sh[2][kWaves][kChanTile];
    const int slot = blockIdx.x / ctiles, ct = blockIdx.x % ctiles;
    const SegSlotN sl = find_slot<SegSlotN>(seg, S, B, slot, kRowChunk);
    if (sl.s < 0) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = ct * kChanTile + lane;
    float s_dy = 0.f, s_dyx = 0.f;
    if (c < C) {
        const size_t at = (size_t)sl.s * C + c;
        const float mean = saved[at], invstd = saved[(size_t)S * C + at];
#pragma unroll 8
        for (int j = 0; j < kRowsPerThread; ++j) {
            const int row = chunk_row(order, sl, w, j, B);
            if (row >= 0) {
                const float g = dy[(size_t)row * C + c], xh = (x[(size_t)row * C + c] - mean) * invstd;
                s_dy += g;
                s_dyx = fmaf(g, xh, s_dyx);
            }
        }
    }
    sh[0][w][lane] = s_dy;
    sh[1][w][lane] = s_dyx;
    __syncthreads();
    if (w == 0 && c < C) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int g = 0; g < kWaves; ++g) {
            a += sh[0][g][lane];
            b += sh[1][g][lane];
        }
        float* out = part + (size_t)slot * 2 * C + c;
        out[0] = (float)a;
        out[(size_t)C] = (float)b;
    }
}

// grid (ctiles): walks the scenarios in order; sums [2][S][C] = sum(dy), sum(dy * xhat) per (scenario, channel) for the
// elementwise pass, and every parameter gradient
__global__ __launch_bounds__(kThreads) void pnorm_bwd_finalize_kernel(const float* __restrict__ part, const int32_t* __restrict__ seg,
                                                                      int B, int C, int S, const float* __restrict__ weight,
                                                                      const float* __restrict__ shared_w, float* __restrict__ sums,
                                                                      float* __restrict__ g_weight, float* __restrict__ g_bias,
                                                                      float* __restrict__ g_shared_w,
                                                                      float* __restrict__ g_shared_b) {
    __shared__ double sh[2][kGroups][kChanTile];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.x * kChanTile + lane;
    const size_t SC = (size_t)S * C;
    double gsw = 0.0, gsb = 0.0;
    int k0 = 0;
    for (int s = 0; s < S; ++s) {
        const int nch = scenario_units(seg, s, B, kRowChunk), per = (nch + kGroups - 1) / kGroups;
        double t_dy = 0.0, t_dyx = 0.0;
        if (c < C) {
            for (int k = k0 + g * per; k < min(k0 + nch, k0 + (g + 1) * per); ++k) {
                const float* in = part + (size_t)k * 2 * C + c;
                t_dy += in[0];
                t_dyx += in[(size_t)C];
            }
        }
        sh[0][g][lane] = t_dy;
        sh[1][g][lane] = t_dyx;
        __syncthreads();
        if (g == 0 && c < C) {
            double u = 0.0, v = 0.0;
#pragma unroll
            for (int q = 0; q < kGroups; ++q) {
                u += sh[0][q][lane];
                v += sh[1][q][lane];
            }
            const size_t at = (size_t)s * C + c;
            sums[at] = (float)u;
            sums[SC + at] = (float)v;
            g_bias[at] = (float)u;
            g_weight[at] = (float)((double)shared_w[c] * v);
            gsb += u;
            gsw += (double)weight[at] * v;
        }
        __syncthreads();
        k0 += nch;
    }
    if (g == 0 && c < C) {
        g_shared_w[c] = (float)gsw;
        g_shared_b[c] = (float)gsb;
    }
}

__global__ __launch_bounds__(kThreads) void pnorm_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                   const int32_t* __restrict__ order,
                                                                   const int32_t* __restrict__ seg, int B, int C, int S,
                                                                   int ctiles, int batch_stats, const float* __restrict__ saved,
                                                                   const float* __restrict__ sums, const float* __restrict__ weight,
                                                                   const float* __restrict__ shared_w, float* __restrict__ dx) {
    const int slot = blockIdx.x / ctiles, ct = blockIdx.x % ctiles;
    const SegSlotN sl = find_slot<SegSlotN>(seg, S, B, slot, kRowChunk);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = ct * kChanTile + lane;
    if (sl.s < 0 || c >= C) return;
    const size_t at = (size_t)sl.s * C + c, SC = (size_t)S * C;
    const float mean = saved[at], invstd = saved[SC + at], k = weight[at] * shared_w[c] * invstd;
    if (!batch_stats) {
#pragma unroll 8
        for (int j = 0; j < kRowsPerThread; ++j) {
            const int row = chunk_row(order, sl, w, j, B);
            if (row >= 0) dx[(size_t)row * C + c] = dy[(size_t)row * C + c] * k;
        }
        return;
    }
    const float n = (float)sl.n, kn = k / n, s_dy = sums[at], s_dyx = sums[SC + at];
#pragma unroll 8
    for (int j = 0; j < kRowsPerThread; ++j) {
        const int row = chunk_row(order, sl, w, j, B);
        if (row >= 0) {
            const float xh = (x[(size_t)row * C + c] - mean) * invstd;
            dx[(size_t)row * C + c] = kn * (fmaf(n, dy[(size_t)row * C + c], -s_dy) - xh * s_dyx);
        }
    }
}

struct PnLayout {
    int64_t slots, ctiles, blocks, part, sums, total;
};

PnLayout pnorm_layout(const satrans_pnorm_desc* d) {
    PnLayout L;
    L.slots = seg_slots(d->B, d->S, kRowChunk);
    L.ctiles = ceil_div(d->C, kChanTile);
    L.blocks = L.slots * L.ctiles;
    L.part = 0;
    L.sums = L.part + L.slots * 3 * d->C;
    L.total = L.sums + 2 * (int64_t)d->S * d->C;
    return L;
}

// checks the descriptor and hands out its layout
int pnorm_validate(const satrans_pnorm_desc* d, const char* who, PnLayout& L) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->C > 0 && d->S > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d C=%d S=%d", who, d->B, d->C, d->S);
    SATRANS_REQUIRE(!(d->flags & ~SATRANS_TRAIN), SATRANS_E_BADARG, "%s: flags %d (SATRANS_TRAIN is the only one)", who, d->flags);
    SATRANS_REQUIRE(d->eps >= 0.f && d->factor >= 0.f && d->factor <= 1.f, SATRANS_E_BADARG, "%s: eps %g, factor %g", who,
                    (double)d->eps, (double)d->factor);
    SATRANS_REQUIRE(d->S <= 65535, SATRANS_E_UNSUPPORTED, "%s: S=%d scenarios (65535 at most)", who, d->S);
    L = pnorm_layout(d);
    SATRANS_REQUIRE(L.blocks <= 0x7fffffffLL, SATRANS_E_UNSUPPORTED, "%s: B=%d x C=%d needs more than 2^31 workgroups", who, d->B,
                    d->C);
    return SATRANS_OK;
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_pnorm_saved_floats(const satrans_pnorm_desc* d) {
    PnLayout L;
    const int rc = pnorm_validate(d, "pnorm_saved_floats", L);
    return rc ? rc : 2 * (int64_t)d->S * d->C;
}

extern "C" int64_t satrans_pnorm_workspace_floats(const satrans_pnorm_desc* d) {
    PnLayout L;
    const int rc = pnorm_validate(d, "pnorm_workspace_floats", L);
    return rc ? rc : L.total;
}

extern "C" int satrans_pnorm_fwd(const satrans_pnorm_desc* d, float* y, float* saved, float* workspace, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    PnLayout L;
    int rc = pnorm_validate(d, "pnorm_fwd", L);
    if (rc) return rc;
    const bool batch_stats = d->flags & SATRANS_TRAIN;
    SATRANS_REQUIRE(d->x && d->order && d->seg && d->weight && d->bias && d->shared_w && d->shared_b && y && saved && workspace,
                    SATRANS_E_BADARG, "pnorm_fwd: null pointer");
    SATRANS_REQUIRE(!d->running_mean == !d->running_var, SATRANS_E_BADARG, "pnorm_fwd: running_mean without running_var (or the reverse)");
    SATRANS_REQUIRE(batch_stats || d->running_mean, SATRANS_E_BADARG, "pnorm_fwd: without SATRANS_TRAIN the running statistics normalise");
    const int B = d->B, C = d->C, S = d->S, ctiles = (int)L.ctiles;
    if (batch_stats) {
        pnorm_stats_kernel<<<(unsigned)L.blocks, kThreads, 0, st>>>(d->x, d->order, d->seg, B, C, S, ctiles, workspace + L.part);
        SATRANS_CHECK_LAUNCH("pnorm_stats_kernel");
        pnorm_finalize_kernel<<<dim3((unsigned)ctiles, (unsigned)S), kThreads, 0, st>>>(workspace + L.part, d->seg, B, C, S, d->eps,
                                                                                        d->factor, saved, d->running_mean,
                                                                                        d->running_var);
        SATRANS_CHECK_LAUNCH("pnorm_finalize_kernel");
    } else {
        const int64_t SC = (int64_t)S * C;
        pnorm_running_kernel<<<(unsigned)ceil_div(SC, 256), 256, 0, st>>>(d->running_mean, d->running_var, SC, d->eps, saved);
        SATRANS_CHECK_LAUNCH("pnorm_running_kernel");
    }
    pnorm_apply_kernel<<<(unsigned)L.blocks, kThreads, 0, st>>>(d->x, d->order, d->seg, B, C, S, ctiles, saved, d->weight, d->bias,
                                                                d->shared_w, d->shared_b, y);
    SATRANS_CHECK_LAUNCH("pnorm_apply_kernel");
    return SATRANS_OK;
}

extern "C" int satrans_pnorm_bwd(const satrans_pnorm_desc* d, const float* dy, float* dx, const float* saved, float* workspace,
                                 float* g_weight, float* g_bias, float* g_shared_w, float* g_shared_b, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    PnLayout L;
    int rc = pnorm_validate(d, "pnorm_bwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x && d->order && d->seg && d->weight && d->shared_w && dy && dx && saved && workspace && g_weight && g_bias &&
                        g_shared_w && g_shared_b,
                    SATRANS_E_BADARG, "pnorm_bwd: null pointer");
    const int B = d->B, C = d->C, S = d->S, ctiles = (int)L.ctiles;
    pnorm_bwd_stats_kernel<<<(unsigned)L.blocks, kThreads, 0, st>>>(d->x, dy, d->order, d->seg, B, C, S, ctiles, saved,
                                                                    workspace + L.part);
    SATRANS_CHECK_LAUNCH("pnorm_bwd_stats_kernel");
    pnorm_bwd_finalize_kernel<<<(unsigned)ctiles, kThreads, 0, st>>>(workspace + L.part, d->seg, B, C, S, d->weight, d->shared_w,
                                                                     workspace + L.sums, g_weight, g_bias, g_shared_w, g_shared_b);
    SATRANS_CHECK_LAUNCH("pnorm_bwd_finalize_kernel");
    pnorm_bwd_apply_kernel<<<(unsigned)L.blocks, kThreads, 0, st>>>(d->x, dy, d->order, d->seg, B, C, S, ctiles,
                                                                    (d->flags & SATRANS_TRAIN) ? 1 : 0, saved, workspace + L.sums,
                                                                    d->weight, d->shared_w, dx);
    SATRANS_CHECK_LAUNCH("pnorm_bwd_apply_kernel");
    return SATRANS_OK;
}
