// Scenario-routed PLE head (reference models/ple.py:161-248 with the loss of mtl_basemodel.py:268-269) for a mixed batch, one
// or two CGC levels.  The reference runs every task's experts, gates and towers over every row at every level and then keeps
// the column of the row's own scenario.  With two levels a row of task t sends gradient only through: all level-0 experts
// (the shared mixture needs every one of them) and the level-0 shared gate - dense over all rows; task t's level-0 gate, task
// t's last-level experts, gate and tower - routed; the last level's shared experts over the shared mixture - dense; the last
// level's shared gate - not at all.  That is what runs here (include/satrans_hip.h states the arithmetic).
//
// Every product, weight gradient and reduce is grouped_gemm.h's, launched and walked by head_layers.h; the last level's mixture
// and its backward are mmoe_mix_fwd_kernel / mmoe_mix_bwd_kernel with E = ns + nsh over [B, (ns + nsh) n]: the task's routed
// specific experts, then the dense shared ones.  New here: the level-0 CGC mixture, a wave per row.
//
//   forward   level 0 (two levels only): experts dense (layer 1 one product with N = E0 n_1, then E0 groups), own gate
//             routed, shared gate dense, ple_cgc_fwd_kernel -> both softmaxes, own and shared mixture;
//             last level: specific experts routed (layer 1 one product with N = ns n_1, then routed AND grouped), shared
//             experts dense, gate routed, mmoe_mix_fwd_kernel, tower routed -> logit
//   backward  tower; mmoe_mix_bwd_kernel; per expert layer the specific then the shared experts, the first layer's products
//             WRITE d own mixture / d shared mixture; the gate ADDS its dx to d own mixture; ple_cgc_bwd_kernel; level-0
//             experts WRITE dx; own gate ADDS; shared gate ADDS.  (One level: specific experts WRITE dx, shared experts ADD,
//             gate ADDS.)
// No floating-point atomics anywhere, no scratch: equal inputs give equal bits, and a task's rows give the same bits alone as
// in a mix (logits, dx rows, the task's gates on both levels, last-level experts, tower, out bias); the dense gradients sum
// over all rows in the caller's order.
#include "head_layers.h"

namespace satrans {
namespace {

constexpr int kMaxShared = SATRANS_PLE_MAX_SHARED_SCORES;
static_assert(SATRANS_PLE_ROW_TILE == kTM && SATRANS_PLE_DW_ROW_CHUNK == kDwChunk && SATRANS_PLE_MAX_OWN == kMaxE &&
                  SATRANS_PLE_MAX_HIDDEN == kMaxH && kMaxShared == 64,
              "the PLE head runs on the MMoE head's kernels; a lane per shared score");

// fixed butterflies over the 64 lanes: every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- level-0 CGC mixture ------------------------------------------------------------------------------------------------------------

// a wave per row of task t = task[row].  eo [B, E0 n], E0 = T ns + nsh blocks: task 0's ns experts, task 1's, ..., the shared.
//   g_own = softmax(s_own[row, :ns + nsh]) in registers;  m_own[j] = sum_u g_own[u] eo[block(u), j], block(u) = t ns + u for
//           u < ns, else T ns + u - ns  (u ascending)
//   g_sh  = softmax(s_sh[row, :E0]), a lane per score, max and sum by the fixed butterfly;  m_sh[j] = sum_e g_sh[e] eo[e, j]
//           (e ascending)
// A row whose task lies outside [0, T) (the module raises before it comes to that) gets zeros in g_own and m_own.
__global__ __launch_bounds__(kThreads) void ple_cgc_fwd_kernel(const int32_t* __restrict__ task, const float* __restrict__ s_own,
                                                               const float* __restrict__ s_sh, const float* __restrict__ eo, int B,
                                                               int T, int ns, int nsh, int n, float* __restrict__ g_own,
                                                               float* __restrict__ g_sh, float* __restrict__ m_own,
                                                               float* __restrict__ m_sh) {
    const int row = blockIdx.x * kMixRows + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const int Eo = ns + nsh, E0 = T * ns + nsh;
    const int t = task[row];
    const bool has = (unsigned)t < (unsigned)T;
    float g[kMaxE];
    float mx = -INFINITY, sum = 0.f;
#pragma unroll
    for (int u = 0; u < kMaxE; ++u) {
        g[u] = u < Eo ? s_own[(size_t)row * Eo + u] : -INFINITY;
        mx = fmaxf(mx, g[u]);
    }
#pragma unroll
    for (int u = 0; u < kMaxE; ++u) {
        g[u] = u < Eo ? expf(g[u] - mx) : 0.f;
        sum += g[u];
    }
#pragma unroll
    for (int u = 0; u < kMaxE; ++u) {
        g[u] = has ? g[u] / sum : 0.f;
        if (lane == u && u < Eo) g_own[(size_t)row * Eo + u] = g[u];
    }
    const float sc = lane < E0 ? s_sh[(size_t)row * E0 + lane] : -INFINITY;
    const float smx = wave_max(sc);
    const float ex = lane < E0 ? expf(sc - smx) : 0.f;
    const float gs = ex / wave_sum(ex);
    if (lane < E0) g_sh[(size_t)row * E0 + lane] = gs;
    const float* er = eo + (size_t)row * E0 * n;
    const int tb = has ? t * ns : 0;
    for (int j0 = 0; j0 < n; j0 += 64) {      // uniform trip count: the shuffles below need every lane
        const int j = j0 + lane;
        const bool ok = j < n;
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < kMaxE; ++u)
            if (u < Eo && ok) acc = fmaf(g[u], er[(size_t)(u < ns ? tb + u : T * ns + u - ns) * n + j], acc);
        float acs = 0.f;
        for (int e = 0; e < E0; ++e) {
            const float ge = __shfl(gs, e, 64);
            if (ok) acs = fmaf(ge, er[(size_t)e * n + j], acs);
        }
        if (ok) {
            m_own[(size_t)row * n + j] = acc;
            m_sh[(size_t)row * n + j] = acs;
        }
    }
}

// a wave per row, block e of eo ascending; u = e's place in the row's own set (or none):
//   dz[row, e n + j] = (eo > 0) (g_sh[e] dm_sh[j] + g_own[u] dm_own[j])        the shared term first, one add
//   dg_sh[e] = sum_j dm_sh[j] eo[e, j],  dg_own[u] = sum_j dm_own[j] eo[e, j]    a lane's j ascending, then the fixed butterfly
//   ds_own[u] = g_own[u] (dg_own[u] - sum_u' g_own[u'] dg_own[u'])  (u' ascending);  ds_sh likewise, its dot by the butterfly
__global__ __launch_bounds__(kThreads) void ple_cgc_bwd_kernel(const int32_t* __restrict__ task, const float* __restrict__ dm_own,
                                                               const float* __restrict__ dm_sh, const float* __restrict__ g_own,
                                                               const float* __restrict__ g_sh, const float* __restrict__ eo, int B,
                                                               int T, int ns, int nsh, int n, float* __restrict__ dz,
                                                               float* __restrict__ ds_own, float* __restrict__ ds_sh) {
    const int row = blockIdx.x * kMixRows + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const int Eo = ns + nsh, E0 = T * ns + nsh;
    const int t = task[row];
    const bool has = (unsigned)t < (unsigned)T;
    float g[kMaxE], dgo[kMaxE];
#pragma unroll
    for (int u = 0; u < kMaxE; ++u) {
        g[u] = u < Eo ? g_own[(size_t)row * Eo + u] : 0.f;
        dgo[u] = 0.f;
    }
    const float gs = lane < E0 ? g_sh[(size_t)row * E0 + lane] : 0.f;
    float dgs = 0.f;      // lane e keeps dg_sh[e]
    const float* er = eo + (size_t)row * E0 * n;
    const float* dor = dm_own + (size_t)row * n;
    const float* dsr = dm_sh + (size_t)row * n;
    float* zr = dz + (size_t)row * E0 * n;
    for (int e = 0; e < E0; ++e) {      // everything that branches below is uniform over the wave
        int u = -1;
        if (e >= T * ns)
            u = ns + e - T * ns;
        else if (has && e / ns == t)
            u = e - t * ns;
        float go = 0.f;
#pragma unroll
        for (int q = 0; q < kMaxE; ++q) go = q == u ? g[q] : go;
        const float ge = __shfl(gs, e, 64);
        float ps = 0.f, po = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float v = er[(size_t)e * n + j], ds = dsr[j];
            ps = fmaf(ds, v, ps);
            float z = __fmul_rn(ge, ds);
            if (u >= 0) {
                const float dn = dor[j];
                po = fmaf(dn, v, po);
                z = __fadd_rn(z, __fmul_rn(go, dn));
            }
            zr[(size_t)e * n + j] = v > 0.f ? z : 0.f;
        }
        ps = wave_sum(ps);
        if (lane == e) dgs = ps;
        if (u >= 0) {
            po = wave_sum(po);
#pragma unroll
            for (int q = 0; q < kMaxE; ++q) dgo[q] = q == u ? po : dgo[q];
        }
    }
    float dot = 0.f;
#pragma unroll
    for (int u = 0; u < kMaxE; ++u) dot = fmaf(g[u], dgo[u], dot);
#pragma unroll
    for (int u = 0; u < kMaxE; ++u)
        if (lane == u && u < Eo) ds_own[(size_t)row * Eo + u] = g[u] * (dgo[u] - dot);
    const float sdot = wave_sum(gs * dgs);
    if (lane < E0) ds_sh[(size_t)row * E0 + lane] = gs * (dgs - sdot);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

struct PleLayout {
    int two;                                          // levels == 2
    int Eo, E0, n_last, kin;                          // own and all blocks, an expert's output width, the last level's input width
    Chain e0, g0, sg0, spec, shr, gate, tower;
    Rows rows;
    // saved: the last level first (gates, mixture, scores as the MMoE head saves them), then level 0
    int64_t s_gates, s_mix, s_scores, s_g_own, s_g_sh, s_m_own, s_m_sh, s_sc_own, s_sc_sh, saved;
    // workspace: two dz buffers [B, max_w], d mixture, the three dscores, d own mixture, d shared mixture, the partials of the layer in hand
    int64_t max_w, w_dm, w_ds1, w_ds_own, w_ds_sh, w_dm_own, w_dm_sh, w_part, total;
};

int ple_validate(const satrans_ple_desc* d, const char* who, PleLayout& L) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->C > 0 && d->T > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d C=%d T=%d", who, d->B, d->C, d->T);
    SATRANS_REQUIRE(d->levels == 1 || d->levels == 2, SATRANS_E_BADARG, "%s: bad sizes levels=%d (1 or 2)", who, d->levels);
    SATRANS_REQUIRE(d->ns >= 1 && d->nsh >= 1 && d->ns <= kMaxE && d->nsh <= kMaxE && d->ns + d->nsh <= kMaxE, SATRANS_E_BADARG,
                    "%s: bad sizes ns=%d nsh=%d (each at least 1, ns + nsh at most %d)", who, d->ns, d->nsh, kMaxE);
    SATRANS_REQUIRE(d->T <= 65535, SATRANS_E_UNSUPPORTED, "%s: T=%d tasks (65535 at most)", who, d->T);
    SATRANS_REQUIRE(d->levels == 1 || (int64_t)d->T * d->ns + d->nsh <= kMaxShared, SATRANS_E_BADARG,
                    "%s: bad sizes T * ns + nsh = %lld (%d scores of the level-0 shared gate at most)", who,
                    (long long)d->T * d->ns + d->nsh, kMaxShared);
    SATRANS_REQUIRE(d->n_expert >= 1 && d->n_expert <= kMaxH && d->n_gate >= 0 && d->n_gate <= kMaxH && d->n_tower >= 0 &&
                        d->n_tower <= kMaxH,
                    SATRANS_E_BADARG, "%s: bad sizes: %d expert, %d gate, %d tower hidden layers (1 to %d, 0 to %d, 0 to %d)", who,
                    d->n_expert, d->n_gate, d->n_tower, kMaxH, kMaxH, kMaxH);
    for (int l = 0; l < d->n_expert; ++l)
        SATRANS_REQUIRE(d->expert_width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes expert_width[%d]=%d", who, l, d->expert_width[l]);
    for (int l = 0; l < d->n_gate; ++l)
        SATRANS_REQUIRE(d->gate_width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes gate_width[%d]=%d", who, l, d->gate_width[l]);
    for (int l = 0; l < d->n_tower; ++l)
        SATRANS_REQUIRE(d->tower_width[l] > 0, SATRANS_E_BADARG, "%s: bad sizes tower_width[%d]=%d", who, l, d->tower_width[l]);
    const int64_t B = d->B;
    const int nx = d->n_expert;
    L.two = d->levels == 2;
    L.Eo = d->ns + d->nsh;
    L.E0 = d->T * d->ns + d->nsh;
    L.n_last = d->expert_width[nx - 1];
    L.kin = L.two ? L.n_last : d->C;
    for (int l = 0; l < nx; ++l)
        SATRANS_REQUIRE((int64_t)std::max(L.two ? L.E0 : 0, L.Eo) * d->expert_width[l] <= 0x7fffffffLL / 4, SATRANS_E_UNSUPPORTED,
                        "%s: blocks * expert_width[%d] = %lld", who, l, (long long)std::max(L.two ? L.E0 : 0, L.Eo) * d->expert_width[l]);
    chain_experts(L.e0, false, L.E0, nx, d->expert_width, d->C, d->e0_w, d->e0_b);
    chain_dnn(L.g0, true, d->n_gate, d->gate_width, d->C, L.Eo, d->g0_w, d->g0_b, d->g0_final_w, nullptr);
    chain_dnn(L.sg0, false, d->n_gate, d->gate_width, d->C, L.E0, d->sg0_w, d->sg0_b, d->sg0_final_w, nullptr);
    chain_experts(L.spec, true, d->ns, nx, d->expert_width, L.kin, d->spec_w, d->spec_b);
    chain_experts(L.shr, false, d->nsh, nx, d->expert_width, L.kin, d->shared_w, d->shared_b);
    chain_dnn(L.gate, true, d->n_gate, d->gate_width, L.kin, L.Eo, d->gate_w, d->gate_b, d->gate_final_w, nullptr);
    chain_dnn(L.tower, true, d->n_tower, d->tower_width, L.n_last, 1, d->tower_w, d->tower_b, d->tower_final_w, d->out_bias);
    L.rows = rows_of(d->B, d->T, d->order, d->seg);
    int64_t at = 0, per_part = 0;
    L.max_w = std::max<int64_t>(L.n_last, L.two ? L.E0 : L.Eo);
    auto take = [&](int64_t n) {
        const int64_t a = at;
        at += B * n;
        L.max_w = std::max(L.max_w, n);
        return a;
    };
    auto fits = [&](const Chain& c, const char* name) { return chain_fits(L.rows, c, who, name, per_part); };
    int rc;
    L.s_gates = take(L.Eo);
    L.s_mix = take(L.n_last);
    L.s_scores = take(L.Eo);
    for (int l = 0; l < nx; ++l) L.spec.s[l] = L.shr.s[l] = take((int64_t)L.Eo * d->expert_width[l]);      // one row: specific, then shared
    for (int l = 0; l < L.gate.n - 1; ++l) L.gate.s[l] = take(L.gate.y[l].N);
    for (int l = 0; l < L.tower.n - 1; ++l) L.tower.s[l] = take(L.tower.y[l].N);
    if ((rc = fits(L.spec, "specific expert")) || (rc = fits(L.shr, "shared expert")) || (rc = fits(L.gate, "gate")) ||
        (rc = fits(L.tower, "tower")))
        return rc;
    if (L.two) {
        L.s_g_own = take(L.Eo);
        L.s_g_sh = take(L.E0);
        L.s_m_own = take(L.n_last);
        L.s_m_sh = take(L.n_last);
        L.s_sc_own = take(L.Eo);
        L.s_sc_sh = take(L.E0);
        for (int l = 0; l < nx; ++l) L.e0.s[l] = take((int64_t)L.E0 * d->expert_width[l]);
        for (int l = 0; l < L.g0.n - 1; ++l) L.g0.s[l] = take(L.g0.y[l].N);
        for (int l = 0; l < L.sg0.n - 1; ++l) L.sg0.s[l] = take(L.sg0.y[l].N);
        if ((rc = fits(L.e0, "level-0 expert")) || (rc = fits(L.g0, "level-0 gate")) || (rc = fits(L.sg0, "level-0 shared gate")))
            return rc;
    }
    L.saved = at;
    at = 2 * B * L.max_w;
    auto work = [&](int64_t n) {
        const int64_t a = at;
        at += B * n;
        return a;
    };
    L.w_dm = work(L.n_last);
    L.w_ds1 = work(L.Eo);
    L.w_ds_own = work(L.two ? L.Eo : 0);
    L.w_ds_sh = work(L.two ? L.E0 : 0);
    L.w_dm_own = work(L.two ? L.n_last : 0);
    L.w_dm_sh = work(L.two ? L.n_last : 0);
    L.w_part = at;
    L.total = L.w_part + per_part;
    return SATRANS_OK;
}

// every pointer of a satrans_ple_desc (P = const float) or a satrans_ple_grads (P = float) that the head reads or writes
template <class P, class S>
bool ple_has(const PleLayout& L, const S* g) {
    if (!g || !g->out_bias) return false;
    if (L.two && !(chain_has<P>(L.e0, g->e0_w, g->e0_b, nullptr, true) && chain_has<P>(L.g0, g->g0_w, g->g0_b, g->g0_final_w, false) &&
                   chain_has<P>(L.sg0, g->sg0_w, g->sg0_b, g->sg0_final_w, false)))
        return false;
    return chain_has<P>(L.spec, g->spec_w, g->spec_b, nullptr, true) && chain_has<P>(L.shr, g->shared_w, g->shared_b, nullptr, true) &&
           chain_has<P>(L.gate, g->gate_w, g->gate_b, g->gate_final_w, false) &&
           chain_has<P>(L.tower, g->tower_w, g->tower_b, g->tower_final_w, false);
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_ple_saved_floats(const satrans_ple_desc* d) {
    PleLayout L;
    const int rc = ple_validate(d, "ple_saved_floats", L);
    return rc ? rc : L.saved;
}

extern "C" int64_t satrans_ple_workspace_floats(const satrans_ple_desc* d) {
    PleLayout L;
    const int rc = ple_validate(d, "ple_workspace_floats", L);
    return rc ? rc : L.total;
}

extern "C" int satrans_ple_fwd(const satrans_ple_desc* d, float* logit, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    PleLayout L;
    int rc = ple_validate(d, "ple_fwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x && d->order && d->seg && (!L.two || d->task) && ple_has<const float>(L, d) && logit && saved, SATRANS_E_BADARG,
                    "ple_fwd: null pointer");
    const int B = d->B, ns = d->ns, n = L.n_last, nx = d->n_expert;
    const float *in_own = d->x, *in_sh = d->x;      // what the last level's specific experts and gate / shared experts read
    if (L.two) {
        // level 0: every expert over x
        if ((rc = experts_fwd(L.rows, L.e0, d->x, d->C, saved, st))) return rc;
        if ((rc = dnn_fwd<true>(L.rows, L.g0, d->x, saved, saved + L.s_sc_own, st))) return rc;
        if ((rc = dnn_fwd<false>(L.rows, L.sg0, d->x, saved, saved + L.s_sc_sh, st))) return rc;
        ple_cgc_fwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(d->task, saved + L.s_sc_own, saved + L.s_sc_sh,
                                                                                saved + L.e0.s[nx - 1], B, d->T, ns, d->nsh, n,
                                                                                saved + L.s_g_own, saved + L.s_g_sh, saved + L.s_m_own,
                                                                                saved + L.s_m_sh);
        SATRANS_CHECK_LAUNCH("ple_cgc_fwd_kernel");
        in_own = saved + L.s_m_own;
        in_sh = saved + L.s_m_sh;
    }
    // the last level's experts: one hidden row [B, (ns + nsh) n_l], the task's specific experts, then the shared ones
    const float *hs = in_own, *hh = in_sh;
    int ldin = L.kin;
    for (int l = 0; l < nx; ++l) {
        const Lyr &ys = L.spec.y[l], &yh = L.shr.y[l];
        const int w = d->expert_width[l], ld = L.Eo * w;
        float* out = saved + L.spec.s[l];
        if ((rc = launch_fwd<true>(L.rows, ys, hs, ldin, l == 0 ? 0 : ys.K, 1, out, ld, w, st))) return rc;
        if ((rc = launch_fwd<false>(L.rows, yh, hh, ldin, l == 0 ? 0 : yh.K, 1, out + ns * w, ld, w, st))) return rc;
        hs = out;
        hh = out + ns * w;
        ldin = ld;
    }
    if ((rc = dnn_fwd<true>(L.rows, L.gate, in_own, saved, saved + L.s_scores, st))) return rc;
    mmoe_mix_fwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(saved + L.s_scores, hs, B, L.Eo, n, saved + L.s_gates,
                                                                             saved + L.s_mix);
    SATRANS_CHECK_LAUNCH("mmoe_mix_fwd_kernel (ple)");
    return dnn_fwd<true>(L.rows, L.tower, saved + L.s_mix, saved, logit, st);
}

extern "C" int satrans_ple_bwd(const satrans_ple_desc* d, const float* dlogit, float* dx, const float* saved, float* workspace,
                               const satrans_ple_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    PleLayout L;
    int rc = ple_validate(d, "ple_bwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x && d->order && d->seg && (!L.two || d->task) && ple_has<const float>(L, d) && dlogit && dx && saved &&
                        workspace && ple_has<float>(L, g),
                    SATRANS_E_BADARG, "ple_bwd: null pointer");
    if (L.two) {
        set_grads(L.e0, g->e0_w, g->e0_b, nullptr, nullptr, true);
        set_grads(L.g0, g->g0_w, g->g0_b, g->g0_final_w, nullptr, false);
        set_grads(L.sg0, g->sg0_w, g->sg0_b, g->sg0_final_w, nullptr, false);
    }
    set_grads(L.spec, g->spec_w, g->spec_b, nullptr, nullptr, true);
    set_grads(L.shr, g->shared_w, g->shared_b, nullptr, nullptr, true);
    set_grads(L.gate, g->gate_w, g->gate_b, g->gate_final_w, nullptr, false);
    set_grads(L.tower, g->tower_w, g->tower_b, g->tower_final_w, g->out_bias, false);
    const int B = d->B, ns = d->ns, n = L.n_last, nx = d->n_expert;
    float* buf[2] = {workspace, workspace + (size_t)B * L.max_w};
    float* ds1 = workspace + L.w_ds1;
    float* part = workspace + L.w_part;
    int cur = 0;      // the buffer the next product writes
    // what the last level read, and where the gradient of that goes
    const float* in_own = L.two ? saved + L.s_m_own : d->x;
    const float* in_sh = L.two ? saved + L.s_m_sh : d->x;
    float* d_own = L.two ? workspace + L.w_dm_own : dx;
    float* d_sh = L.two ? workspace + L.w_dm_sh : dx;
    // tower: dlogit -> d mixture
    float* dm = workspace + L.w_dm;
    if ((rc = dnn_bwd<true>(L.rows, L.tower, dlogit, saved + L.s_mix, saved, 0, dm, buf, cur, part, st))) return rc;
    // mixture and softmax: d mixture -> dz of the experts' last layer, dscores
    mmoe_mix_bwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(dm, saved + L.s_gates, saved + L.spec.s[nx - 1], B, L.Eo, n,
                                                                             buf[cur], ds1);
    SATRANS_CHECK_LAUNCH("mmoe_mix_bwd_kernel (ple)");
    const float* dz = buf[cur];
    cur ^= 1;
    // the last level's experts, per layer the specific (routed) then the shared (dense) ones
    for (int l = nx - 1; l >= 0; --l) {
        const Lyr &ys = L.spec.y[l], &yh = L.shr.y[l];
        const int w = d->expert_width[l], ldz = L.Eo * w;
        if (l == 0) {
            if ((rc = launch_bwd<true>(L.rows, ys, dz, ldz, in_own, L.kin, 0, false, 0, d_own, part, st))) return rc;
            if ((rc = launch_bwd<false>(L.rows, yh, dz + ns * w, ldz, in_sh, L.kin, 0, false, L.two ? 0 : 1, d_sh, part, st))) return rc;
        } else {
            const int wp = d->expert_width[l - 1], ldh = L.Eo * wp;
            const float* hin = saved + L.spec.s[l - 1];
            if ((rc = launch_bwd<true>(L.rows, ys, dz, ldz, hin, ldh, wp, true, 0, buf[cur], part, st))) return rc;
            if ((rc = launch_bwd<false>(L.rows, yh, dz + ns * w, ldz, hin + ns * wp, ldh, wp, true, 0, buf[cur] + ns * wp, part, st)))
                return rc;
            dz = buf[cur];
            cur ^= 1;
        }
    }
    // the last level's gate: its dx is added to the specific experts'
    if ((rc = dnn_bwd<true>(L.rows, L.gate, ds1, in_own, saved, 1, d_own, buf, cur, part, st))) return rc;
    if (!L.two) return SATRANS_OK;
    // level 0: both mixtures -> dz of every expert's last layer and both dscores
    float* ds_own = workspace + L.w_ds_own;
    float* ds_sh = workspace + L.w_ds_sh;
    ple_cgc_bwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(d->task, d_own, d_sh, saved + L.s_g_own, saved + L.s_g_sh,
                                                                            saved + L.e0.s[nx - 1], B, d->T, ns, d->nsh, n, buf[cur],
                                                                            ds_own, ds_sh);
    SATRANS_CHECK_LAUNCH("ple_cgc_bwd_kernel");
    dz = buf[cur];
    cur ^= 1;
    if ((rc = experts_bwd(L.rows, L.e0, dz, d->x, d->C, saved, dx, buf, cur, part, st))) return rc;
    if ((rc = dnn_bwd<true>(L.rows, L.g0, ds_own, d->x, saved, 1, dx, buf, cur, part, st))) return rc;
    return dnn_bwd<false>(L.rows, L.sg0, ds_sh, d->x, saved, 1, dx, buf, cur, part, st);
}
