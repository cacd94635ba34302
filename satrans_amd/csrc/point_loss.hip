// Prediction + loss(reduction='sum') + d(loss sum)/dlogit for a column of logits: what the sibling models' fit runs after their
// head (reference models/basemodel.py: `y_pred = model(x).squeeze()`, `loss_func(y_pred, y, reduction='sum')`, and the backward of
// both), in one launch plus one small fixed-order reduction.
//
// The per-sample arithmetic restates head_kernel's (head.hip) expression for expression, so that `pred` and `dz` carry the bits
// satrans_head_loss gives for the same logit: none of these expressions has a multiply feeding an add, so the compiler has
// nothing to contract differently here.  One sample per lane.  The fp32 loss of a sample is widened to double and summed lane ->
// wave -> block; the block sums are added in index order by a second launch (a single block adds its sum itself).
#include "common.h"

namespace satrans {

constexpr int kPointBlock = 256;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kPointBlock) void point_loss_kernel(const float* __restrict__ z, int64_t z_stride,
                                                                 const float* __restrict__ y, int B, int pred_kind, int loss_kind,
                                                                 float* __restrict__ pred, float* __restrict__ dz,
                                                                 double* __restrict__ loss_sum, double* __restrict__ partial) {
    __shared__ double s_wave[kPointBlock / kWave];
    const int b = blockIdx.x * kPointBlock + threadIdx.x;
    float loss = 0.f;
    if (b < B) {
        const float zb = z[(int64_t)b * z_stride];
        const bool sigmoid = pred_kind == SATRANS_PRED_SIGMOID;
        const float p = sigmoid ? 1.0f / (1.0f + expf(-zb)) : zb;
        pred[b] = p;
        if (y) {
            const float t = y[b];
            const float pq = (1.0f - p) * p;
            const float dp = sigmoid ? pq : 1.0f;       // d pred / d logit
            float g;
            if (loss_kind == SATRANS_LOSS_MSE) {            // F.mse_loss(reduction='sum'): (p - t)^2, d/dp = 2 (p - t)
                loss = (p - t) * (p - t);
                g = 2.0f * (p - t) * dp;
            } else if (loss_kind == SATRANS_LOSS_MAE) {     // F.l1_loss(reduction='sum'): |p - t|, d/dp = sign(p - t)
                loss = fabsf(p - t);
                g = (p > t ? 1.0f : (p < t ? -1.0f : 0.0f)) * dp;
            } else {
                // torch.nn.functional.binary_cross_entropy clamps both logs at -100
                const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.0f - p), -100.f);
                loss = -(t * lp + (1.0f - t) * lq);
                // BCE backward (grad * (p - t) / max(p(1-p), 1e-12)) chained with the prediction's backward
                g = (p - t) / fmaxf(pq, 1e-12f) * dp;
            }
            if (dz) dz[b] = g;
        }
    }
    if (!y) return;
    const double w = wave_sum_f64((double)loss);
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < kPointBlock / kWave; ++k) total += s_wave[k];
        if (gridDim.x == 1) loss_sum[0] += total;
        else partial[blockIdx.x] = total;
    }
}

// one wave: lane l adds its contiguous share of the block sums in index order, lane 0 adds the lanes' sums in lane order
__global__ __launch_bounds__(kWave) void point_loss_reduce_kernel(const double* __restrict__ partial, int nblk,
                                                                  double* __restrict__ loss_sum) {
    __shared__ double s_lane[kWave];
    const int share = (nblk + kWave - 1) / kWave;
    const int lo = min(nblk, (int)threadIdx.x * share), hi = min(nblk, lo + share);
    double acc = 0.0;
    for (int k = lo; k < hi; ++k) acc += partial[k];
    s_lane[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int k = 0; k < kWave; ++k) total += s_lane[k];
    loss_sum[0] += total;
}

// The routed form: z [B, T], row b takes column task[b] (the multi-task models' masked per-task loss sum and predict assembly,
// reference models/mtl_basemodel.py:268-269, :376-378).  The per-sample expressions are point_loss_kernel's, restated rather
// than shared so that kernel stays as it was compiled.  A row whose task lies outside [0, T) belongs to no mask: pred 0, no
// loss, a zero dz row.  Every dz entry is written here.  The sum is point_loss_kernel's, and so is the second launch.
__global__ __launch_bounds__(kPointBlock) void point_loss_routed_kernel(const float* __restrict__ z, int64_t z_stride,
                                                                        const int32_t* __restrict__ task,
                                                                        const float* __restrict__ y, int B, int T, int pred_kind,
                                                                        int loss_kind, float* __restrict__ pred,
                                                                        float* __restrict__ dz, double* __restrict__ loss_sum,
                                                                        double* __restrict__ partial) {
    __shared__ double s_wave[kPointBlock / kWave];
    const int b = blockIdx.x * kPointBlock + threadIdx.x;
    float loss = 0.f;
    if (b < B) {
        const int col = task[b];
        const bool routed = col >= 0 && col < T;
        float p = 0.f, g = 0.f;
        if (routed) {
            const float zb = z[(int64_t)b * z_stride + col];
            const bool sigmoid = pred_kind == SATRANS_PRED_SIGMOID;
            p = sigmoid ? 1.0f / (1.0f + expf(-zb)) : zb;
            if (y) {
                const float t = y[b];
                const float pq = (1.0f - p) * p;
                const float dp = sigmoid ? pq : 1.0f;
                if (loss_kind == SATRANS_LOSS_MSE) {
                    loss = (p - t) * (p - t);
                    g = 2.0f * (p - t) * dp;
                } else if (loss_kind == SATRANS_LOSS_MAE) {
                    loss = fabsf(p - t);
                    g = (p > t ? 1.0f : (p < t ? -1.0f : 0.0f)) * dp;
                } else {
                    const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.0f - p), -100.f);
                    loss = -(t * lp + (1.0f - t) * lq);
                    g = (p - t) / fmaxf(pq, 1e-12f) * dp;
                }
            }
        }
        pred[b] = p;
        if (y && dz) {
            float* row = dz + (int64_t)b * T;
            for (int k = 0; k < T; ++k) row[k] = k == col ? g : 0.f;
        }
    }
    if (!y) return;
    const double w = wave_sum_f64((double)loss);
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < kPointBlock / kWave; ++k) total += s_wave[k];
        if (gridDim.x == 1) loss_sum[0] += total;
        else partial[blockIdx.x] = total;
    }
}

}  // namespace satrans

using namespace satrans;

extern "C" int satrans_point_loss_routed(const float* z, int64_t z_stride, const int32_t* task, const float* y, int B, int T,
                                         int pred_kind, int loss_kind, float* pred, float* dz, double* loss_sum, double* partial,
                                         void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SATRANS_REQUIRE(z && task && pred, SATRANS_E_BADARG, "point_loss_routed: null pointer");
    SATRANS_REQUIRE(B >= 1 && T >= 1 && z_stride >= T, SATRANS_E_BADARG, "point_loss_routed: bad sizes B=%d T=%d z_stride=%lld", B, T,
                    (long long)z_stride);
    SATRANS_REQUIRE(pred_kind == SATRANS_PRED_SIGMOID || pred_kind == SATRANS_PRED_LINEAR, SATRANS_E_BADARG,
                    "point_loss_routed: prediction kind %d", pred_kind);
    SATRANS_REQUIRE(loss_kind >= SATRANS_LOSS_BCE && loss_kind <= SATRANS_LOSS_MAE, SATRANS_E_BADARG,
                    "point_loss_routed: loss kind %d", loss_kind);
    if (y) SATRANS_REQUIRE(loss_sum, SATRANS_E_BADARG, "point_loss_routed: labels without a loss sum");
    const int nblk = (int)ceil_div(B, kPointBlock);
    if (y && nblk > 1) SATRANS_REQUIRE(partial, SATRANS_E_BADARG, "point_loss_routed: labels without the partial sums' scratch");
    point_loss_routed_kernel<<<nblk, kPointBlock, 0, stream>>>(z, z_stride, task, y, B, T, pred_kind, loss_kind, pred, dz, loss_sum,
                                                               partial);
    SATRANS_CHECK_LAUNCH("point_loss_routed_kernel");
    if (y && nblk > 1) {
        point_loss_reduce_kernel<<<1, kWave, 0, stream>>>(partial, nblk, loss_sum);
        SATRANS_CHECK_LAUNCH("point_loss_reduce_kernel");
    }
    return SATRANS_OK;
}

extern "C" int64_t satrans_point_loss_partials(int B) { return B > 0 ? ceil_div(B, kPointBlock) : 0; }

extern "C" int satrans_point_loss(const float* z, int64_t z_stride, const float* y, int B, int pred_kind, int loss_kind, float* pred,
                                  float* dz, double* loss_sum, double* partial, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SATRANS_REQUIRE(z && pred, SATRANS_E_BADARG, "point_loss: null pointer");
    SATRANS_REQUIRE(B >= 1 && z_stride >= 1, SATRANS_E_BADARG, "point_loss: bad sizes B=%d z_stride=%lld", B, (long long)z_stride);
    SATRANS_REQUIRE(pred_kind == SATRANS_PRED_SIGMOID || pred_kind == SATRANS_PRED_LINEAR, SATRANS_E_BADARG,
                    "point_loss: prediction kind %d", pred_kind);
    SATRANS_REQUIRE(loss_kind >= SATRANS_LOSS_BCE && loss_kind <= SATRANS_LOSS_MAE, SATRANS_E_BADARG, "point_loss: loss kind %d",
                    loss_kind);
    if (y) SATRANS_REQUIRE(loss_sum, SATRANS_E_BADARG, "point_loss: labels without a loss sum");
    const int nblk = (int)ceil_div(B, kPointBlock);
    if (y && nblk > 1) SATRANS_REQUIRE(partial, SATRANS_E_BADARG, "point_loss: labels without the partial sums' scratch");
    point_loss_kernel<<<nblk, kPointBlock, 0, stream>>>(z, z_stride, y, B, pred_kind, loss_kind, pred, dz, loss_sum, partial);
    SATRANS_CHECK_LAUNCH("point_loss_kernel");
    if (y && nblk > 1) {
        point_loss_reduce_kernel<<<1, kWave, 0, stream>>>(partial, nblk, loss_sum);
        SATRANS_CHECK_LAUNCH("point_loss_reduce_kernel");
    }
    return SATRANS_OK;
}
