// Scenario-specific attention maps (reference models/meta_basemodel.py:421-426, 439-458, 506-514: predict's `showattn` branch):
// per (scenario, label class) sums of one layer's `normalized_att_scores` [H, B, F, F] over the samples of a batch, added into an
// fp64 accumulator [K = 3 S, H, F*F] that the caller keeps across batches.
//
// Deterministic by construction, no float atomics: the samples are stably grouped by scenario (satrans_bucket_scenarios on
// key / 3 + 1, group 0 holding the samples that count nowhere: S + 1 groups, so the one- or two-launch bucketing serves the usual
// handful of scenarios), every scenario's run of sample positions is cut into blocks of kStatsBlock positions, one workgroup sums
// one block for one head and one chunk of map elements in fp64 - the three label classes in three registers, every sample adding
// to its own class's one - and writes the block's sums, and the fold adds every scenario's block sums in a fixed order (16 strided
// partial sums over the blocks, combined in wave order) into the accumulator.  The partition depends on B, the scenario counts and
// the shape only.
//
// Traffic: the attention is read once (H*B*F*F*4 bytes; one sample's map of one head is F*F contiguous floats, read as dwords:
// F*F*4 bytes is not 16-byte aligned for odd F), the block sums are (B/kStatsBlock + S)*3*H*F*F*8 bytes written and read back.
#include "common.h"

namespace satrans {

constexpr int kStatsBlock = 128;     // sample positions per block
constexpr int kStatsAhead = 16;      // loads in flight per thread
constexpr int kStatsThreads = 256;   // widest element chunk
constexpr int kStatsAlign = 256;

struct StatsLayout {
    size_t key1, cls, sid, order, seg, status, blk, bucket, partial, total;
    int64_t cap;                     // blocks the partial sums have room for
};

static size_t stats_align(size_t v) { return (v + kStatsAlign - 1) / kStatsAlign * kStatsAlign; }

static StatsLayout stats_layout(int B, int H, int F, int K) {
    StatsLayout L;
    const int64_t E = (int64_t)F * F;
    const int S = K / 3;
    // sum over scenarios of ceil(n_s / kStatsBlock) <= B / kStatsBlock + S
    L.cap = ceil_div(B, kStatsBlock) + S;
    size_t at = 0;
    L.key1 = at;    at = stats_align(at + (size_t)B * 4);
    L.cls = at;     at = stats_align(at + (size_t)B * 4);
    L.sid = at;     at = stats_align(at + (size_t)B * 4);
    L.order = at;   at = stats_align(at + (size_t)B * 4);
    L.seg = at;     at = stats_align(at + (size_t)(S + 2) * 4);
    L.status = at;  at = stats_align(at + 4);
    L.blk = at;     at = stats_align(at + (size_t)(S + 1) * 4);
    L.bucket = at;  at = stats_align(at + (size_t)satrans_bucket_workspace_bytes(B, S + 1));
    L.partial = at; at = stats_align(at + (size_t)L.cap * 3 * H * E * sizeof(double));
    L.total = at;
    return L;
}

// grp[b] = scenario + 1 of key[b] (0 = counts nowhere; a key outside [-1, K) counts nowhere either), cls[b] = its class.
__global__ void stats_split_keys_kernel(const int32_t* __restrict__ key, int B, int K, int32_t* __restrict__ grp,
                                        int32_t* __restrict__ cls) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int32_t k = key[b];
    const bool ok = k >= 0 && k < K;
    grp[b] = ok ? k / 3 + 1 : 0;
    cls[b] = ok ? k % 3 : 0;
}

// blk[k] = first block of scenario k (exclusive prefix of ceil(n_k / kStatsBlock)), blk[K] = blocks in all.  One workgroup.
__global__ __launch_bounds__(256) void stats_plan_kernel(const int32_t* __restrict__ seg, int K, int32_t* __restrict__ blk) {
    __shared__ int32_t s_wave[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int32_t carry = 0;
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + t;
        const int32_t n = k < K ? (seg[k + 2] - seg[k + 1] + kStatsBlock - 1) / kStatsBlock : 0;
        int32_t incl = n;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_wave[w] = incl;
        __syncthreads();
        int32_t before = carry;
        for (int ww = 0; ww < w; ++ww) before += s_wave[ww];
        if (k < K) blk[k] = before + incl - n;
        carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (t == 0) blk[K] = carry;
}

// One block of one scenario, one head, one chunk of map elements: the fp64 sums over the block's samples in position order, one per
// label class (a sample adds to its class's sum only).  grid (cap, H, chunks), block = chunk width (a multiple of 64);
// partial [cap][3][H][E].
__global__ __launch_bounds__(kStatsThreads) void stats_block_kernel(const float* __restrict__ att, const int32_t* __restrict__ order,
                                                                    const int32_t* __restrict__ cls, const int32_t* __restrict__ seg,
                                                                    const int32_t* __restrict__ blk, int B, int E, int S, int64_t cap,
                                                                    double* __restrict__ partial) {
    const int j = blockIdx.x;
    const int total = blk[S];
    if (j >= total || j >= cap) return;                     // (uniform: the grid is sized for the largest possible count)
    int lo = 0, hi = S;                                     // the scenario whose blocks hold j: blk[lo] <= j < blk[lo + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk[mid] <= j) lo = mid; else hi = mid;
    }
    const int p0 = seg[lo + 1] + (j - blk[lo]) * kStatsBlock;
    const int p1 = min(p0 + kStatsBlock, seg[lo + 2]);
    const int h = blockIdx.y;
    const int e = blockIdx.z * blockDim.x + threadIdx.x;
    const int H = gridDim.y;
    if (e >= E) return;
    const float* base = att + (size_t)h * B * E + e;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int p = p0;
    for (; p + kStatsAhead <= p1; p += kStatsAhead) {
        float v[kStatsAhead];
        int c[kStatsAhead];
#pragma unroll
        for (int u = 0; u < kStatsAhead; ++u) {
            const int b = order[p + u];
            v[u] = base[(size_t)b * E];
            c[u] = cls[b];
        }
#pragma unroll
        for (int u = 0; u < kStatsAhead; ++u) {
            const double x = (double)v[u];
            if (c[u] == 0) s0 += x; else if (c[u] == 1) s1 += x; else s2 += x;     // (uniform branch)
        }
    }
    for (; p < p1; ++p) {
        const int b = order[p];
        const double x = (double)base[(size_t)b * E];
        const int c = cls[b];
        if (c == 0) s0 += x; else if (c == 1) s1 += x; else s2 += x;
    }
    const size_t HE = (size_t)H * E, at = (size_t)j * 3 * HE + (size_t)h * E + e;
    partial[at] = s0;
    partial[at + HE] = s1;
    partial[at + 2 * HE] = s2;
}

// acc[3 g + c][he] += the block sums of scenario g and class c.  grid (ceil(HE / 64), S), kFoldWaves waves: lane = element of the
// chunk, wave w sums the blocks blk[g] + w, + w + kFoldWaves, ... in that order, the wave sums are added in wave order.
constexpr int kFoldWaves = 16;
__global__ __launch_bounds__(kFoldWaves * 64) void stats_fold_kernel(const double* __restrict__ partial,
                                                                     const int32_t* __restrict__ blk, int64_t HE, int64_t cap,
                                                                     double* __restrict__ acc) {
    __shared__ double s_part[kFoldWaves][3][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = blockIdx.y;
    const int64_t he = (int64_t)blockIdx.x * 64 + lane;
    const int end = (int)min((int64_t)blk[g + 1], cap);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (he < HE) {
        for (int j = blk[g] + w; j < end; j += kFoldWaves) {
            const double* q = partial + (size_t)j * 3 * HE + he;
            s0 += q[0];
            s1 += q[HE];
            s2 += q[2 * HE];
        }
    }
    s_part[w][0][lane] = s0;
    s_part[w][1][lane] = s1;
    s_part[w][2][lane] = s2;
    __syncthreads();
    if (w < 3 && he < HE) {
        double t = 0.0;
        for (int ww = 0; ww < kFoldWaves; ++ww) t += s_part[ww][w][lane];
        acc[(size_t)(3 * g + w) * HE + he] += t;
    }
}

}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_attn_stats_workspace_bytes(int B, int H, int F, int K) {
    SATRANS_REQUIRE(B > 0 && H > 0 && F > 0 && K > 0 && K % 3 == 0, SATRANS_E_BADARG,
                    "attn_stats_workspace_bytes: bad sizes B=%d H=%d F=%d K=%d", B, H, F, K);
    return (int64_t)stats_layout(B, H, F, K).total;
}

extern "C" int satrans_attn_stats_accumulate(const float* att, const int32_t* key, int B, int H, int F, int K, double* acc,
                                             void* workspace, int64_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SATRANS_REQUIRE(att && key && acc && workspace, SATRANS_E_BADARG, "attn_stats_accumulate: null pointer");
    SATRANS_REQUIRE(B > 0 && H > 0 && F > 0 && K > 0 && K % 3 == 0, SATRANS_E_BADARG,
                    "attn_stats_accumulate: bad sizes B=%d H=%d F=%d K=%d", B, H, F, K);
    SATRANS_REQUIRE(H <= 65535, SATRANS_E_UNSUPPORTED, "attn_stats_accumulate: %d heads", H);
    const StatsLayout L = stats_layout(B, H, F, K);
    SATRANS_REQUIRE((int64_t)L.total <= workspace_bytes, SATRANS_E_WORKSPACE, "attn_stats_accumulate: workspace %lld < %lld bytes",
                    (long long)workspace_bytes, (long long)L.total);
    char* ws = (char*)workspace;
    int32_t* key1 = (int32_t*)(ws + L.key1);
    int32_t* cls = (int32_t*)(ws + L.cls);
    int32_t* seg = (int32_t*)(ws + L.seg);
    int32_t* order = (int32_t*)(ws + L.order);
    int32_t* blk = (int32_t*)(ws + L.blk);
    double* partial = (double*)(ws + L.partial);
    const int S = K / 3;
    stats_split_keys_kernel<<<(unsigned)ceil_div(B, 256), 256, 0, stream>>>(key, B, K, key1, cls);
    SATRANS_CHECK_LAUNCH("stats_split_keys_kernel");
    const int rc = satrans_bucket_scenarios(key1, SATRANS_ID_I32, 1, 0, B, S + 1, (int32_t*)(ws + L.sid), order, seg,
                                            (int32_t*)(ws + L.status), ws + L.bucket, (int64_t)(L.partial - L.bucket), stream);
    if (rc != SATRANS_OK) return rc;
    stats_plan_kernel<<<1, 256, 0, stream>>>(seg, S, blk);
    SATRANS_CHECK_LAUNCH("stats_plan_kernel");
    const int E = F * F;
    const int chunks = (int)ceil_div(E, kStatsThreads);
    const int width = (int)ceil_div(ceil_div(E, chunks), kWave) * kWave;
    stats_block_kernel<<<dim3((unsigned)L.cap, (unsigned)H, (unsigned)chunks), width, 0, stream>>>(att, order, cls, seg, blk, B, E, S,
                                                                                                   L.cap, partial);
    SATRANS_CHECK_LAUNCH("stats_block_kernel");
    const int64_t HE = (int64_t)H * E;
    stats_fold_kernel<<<dim3((unsigned)ceil_div(HE, 64), (unsigned)S), kFoldWaves * 64, 0, stream>>>(partial, blk, HE, L.cap, acc);
    SATRANS_CHECK_LAUNCH("stats_fold_kernel");
    return SATRANS_OK;
}
