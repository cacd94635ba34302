// Scenario-routed MMoE head (reference models/mmoe.py:142-171 with the loss of mtl_basemodel.py:268-269) for a mixed batch.
// The reference runs every task's gate and tower over every row and then keeps the column of the row's own scenario; here the
// experts run over all rows (dense products) and a row goes through its OWN task's gate, mixture, tower and logit only
// (scenario-grouped products over order / seg, walked as seg_walk.h describes).
//
// Layout, the tile product and the kernels themselves are in grouped_gemm.h; the launches of a layer, the walks over a DNN and
// over the expert stack and the per-layer grid check are in head_layers.h, shared with the other heads.  This file holds the
// layout of the saved rows and the workspace, the validation and the order of the launches.
//
//   forward   mmoe_gemm_kernel<false, false>   experts: layer 1 is one product with N = E n_1 over x, layer l >= 2 has E groups
//             mmoe_gemm_kernel<false, true>    gate DNN and gate_dnn_final_layer of the row's task -> scores [B,E]
//             mmoe_mix_fwd_kernel              g = softmax(scores), m = sum_e g[e] expert_out[e]; a wave per row, E in registers
//             mmoe_gemm_kernel<false, true>    tower DNN, tower_dnn_final_layer and out[t].bias of the row's task -> logit
//   backward  tower (routed), last layer to first, the last product writes dm;
//             mmoe_mix_bwd_kernel              dz of the experts' last layer = g[e] dm (expert_out > 0), dscores
//             experts (dense), last layer to first, the last product WRITES dx;
//             gate (routed), last layer to first, the last product ADDS its dx to the experts' (one add per element);
//             per layer: mmoe_dw_kernel (partials over chunks of kDwChunk rows: routed chunks are counted from the start of a
//             task's run, the experts' chunks in the caller's row order) and mmoe_reduce_kernel (chunks in chunk order, fp64
//             sums of the fp32 partials; a task without rows gets zeros), then mmoe_gemm_kernel<true, .> for the input gradient.
// No floating-point atomics anywhere: equal inputs give equal bits, and a task's rows give the same bits alone as in a mix
// (logits, dx rows, that task's gate / tower / out-bias gradients; the experts' gradients sum over all rows).
#include "head_layers.h"

namespace satrans {
namespace {

// ---- host -----------------------------------------------------------------------------------------------------------------------

struct MmoeLayout {
    Chain x, g, t;      // experts (dense), gate and tower (routed; hidden + final)
    Rows rows;
    int64_t n_last;                                   // width of an expert's output
    // saved (floats from its start): gates [B,E], mixture [B,n_last], scores [B,E], then the hidden rows
    int64_t s_gates, s_mix, s_scores, saved;
    // workspace: two dz buffers [B, max_w], dscores [B,E], the partials of the layer in hand
    int64_t max_w, w_dz, w_dscores, w_part, total;
};

int mmoe_validate(const satrans_mmoe_desc* d, const char* who, MmoeLayout& L) {
    SATRANS_REQUIRE(d, SATRANS_E_BADARG, "%s: null descriptor", who);
    SATRANS_REQUIRE(d->B > 0 && d->C > 0 && d->T > 0, SATRANS_E_BADARG, "%s: bad sizes B=%d C=%d T=%d", who, d->B, d->C, d->T);
    SATRANS_REQUIRE(d->E >= 2 && d->E <= kMaxE, SATRANS_E_BADARG, "%s: bad sizes E=%d (2 to %d experts)", who, d->E, kMaxE);
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
    SATRANS_REQUIRE(d->T <= 65535, SATRANS_E_UNSUPPORTED, "%s: T=%d tasks (65535 at most)", who, d->T);
    const int64_t B = d->B, E = d->E;
    for (int l = 0; l < d->n_expert; ++l)
        SATRANS_REQUIRE(E * d->expert_width[l] <= 0x7fffffffLL / 4, SATRANS_E_UNSUPPORTED, "%s: E * expert_width[%d] = %lld", who, l,
                        (long long)(E * d->expert_width[l]));
    L.n_last = d->expert_width[d->n_expert - 1];
    chain_experts(L.x, false, d->E, d->n_expert, d->expert_width, d->C, d->expert_w, d->expert_b);
    chain_dnn(L.g, true, d->n_gate, d->gate_width, d->C, d->E, d->gate_w, d->gate_b, d->gate_final_w, nullptr);
    chain_dnn(L.t, true, d->n_tower, d->tower_width, (int)L.n_last, 1, d->tower_w, d->tower_b, d->tower_final_w, d->out_bias);
    L.rows = rows_of(d->B, d->T, d->order, d->seg);
    int64_t at = 0, per_part = 0;
    L.max_w = 0;
    auto take = [&](int64_t n) {
        const int64_t a = at;
        at += B * n;
        L.max_w = std::max(L.max_w, n);
        return a;
    };
    L.s_gates = take(E);
    L.s_mix = take(L.n_last);
    L.s_scores = take(E);
    for (int l = 0; l < L.x.n; ++l) L.x.s[l] = take((int64_t)L.x.y[l].N * L.x.y[l].G);
    int rc;
    if ((rc = chain_fits(L.rows, L.x, who, "expert", per_part))) return rc;
    for (int l = 0; l < L.g.n - 1; ++l) L.g.s[l] = take(L.g.y[l].N);
    if ((rc = chain_fits(L.rows, L.g, who, "gate", per_part))) return rc;
    for (int l = 0; l < L.t.n - 1; ++l) L.t.s[l] = take(L.t.y[l].N);
    if ((rc = chain_fits(L.rows, L.t, who, "tower", per_part))) return rc;
    L.saved = at;
    L.w_dz = 0;
    L.w_dscores = 2 * B * L.max_w;
    L.w_part = L.w_dscores + B * E;
    L.total = L.w_part + per_part;
    return SATRANS_OK;
}

// every pointer of a satrans_mmoe_desc (P = const float) or a satrans_mmoe_grads (P = float) that the head reads or writes
template <class P, class S>
bool mmoe_has(const MmoeLayout& L, const S* g) {
    return g && g->out_bias && chain_has<P>(L.x, g->expert_w, g->expert_b, nullptr, true) &&
           chain_has<P>(L.g, g->gate_w, g->gate_b, g->gate_final_w, false) &&
           chain_has<P>(L.t, g->tower_w, g->tower_b, g->tower_final_w, false);
}

}  // namespace
}  // namespace satrans

using namespace satrans;

extern "C" int64_t satrans_mmoe_saved_floats(const satrans_mmoe_desc* d) {
    MmoeLayout L;
    const int rc = mmoe_validate(d, "mmoe_saved_floats", L);
    return rc ? rc : L.saved;
}

extern "C" int64_t satrans_mmoe_workspace_floats(const satrans_mmoe_desc* d) {
    MmoeLayout L;
    const int rc = mmoe_validate(d, "mmoe_workspace_floats", L);
    return rc ? rc : L.total;
}

extern "C" int satrans_mmoe_fwd(const satrans_mmoe_desc* d, float* logit, float* saved, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MmoeLayout L;
    int rc = mmoe_validate(d, "mmoe_fwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x && d->order && d->seg && mmoe_has<const float>(L, d) && logit && saved, SATRANS_E_BADARG,
                    "mmoe_fwd: null pointer");
    const int B = d->B, E = d->E, n_last = (int)L.n_last;
    // experts over x, then the row's own gate
    if ((rc = experts_fwd(L.rows, L.x, d->x, d->C, saved, st))) return rc;
    if ((rc = dnn_fwd<true>(L.rows, L.g, d->x, saved, saved + L.s_scores, st))) return rc;
    mmoe_mix_fwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(saved + L.s_scores, saved + L.x.s[L.x.n - 1], B, E, n_last,
                                                                             saved + L.s_gates, saved + L.s_mix);
    SATRANS_CHECK_LAUNCH("mmoe_mix_fwd_kernel");
    // the row's own tower, final layer and out bias
    return dnn_fwd<true>(L.rows, L.t, saved + L.s_mix, saved, logit, st);
}

extern "C" int satrans_mmoe_bwd(const satrans_mmoe_desc* d, const float* dlogit, float* dx, const float* saved, float* workspace,
                                const satrans_mmoe_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MmoeLayout L;
    int rc = mmoe_validate(d, "mmoe_bwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(d->x && d->order && d->seg && mmoe_has<const float>(L, d) && dlogit && dx && saved && workspace &&
                        mmoe_has<float>(L, g),
                    SATRANS_E_BADARG, "mmoe_bwd: null pointer");
    set_grads(L.x, g->expert_w, g->expert_b, nullptr, nullptr, true);
    set_grads(L.g, g->gate_w, g->gate_b, g->gate_final_w, nullptr, false);
    set_grads(L.t, g->tower_w, g->tower_b, g->tower_final_w, g->out_bias, false);
    const int B = d->B, E = d->E, n_last = (int)L.n_last;
    float* buf[2] = {workspace + L.w_dz, workspace + L.w_dz + (size_t)B * L.max_w};
    float* dscores = workspace + L.w_dscores;
    float* part = workspace + L.w_part;
    int cur = 0;      // the buffer the next product writes
    // tower: dlogit -> dm, in the buffer before `cur`
    if ((rc = dnn_bwd<true>(L.rows, L.t, dlogit, saved + L.s_mix, saved, 0, nullptr, buf, cur, part, st))) return rc;
    // mixture and softmax: dm -> dz of the experts' last layer, dscores
    const float* eo = saved + L.x.s[L.x.n - 1];
    mmoe_mix_bwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(buf[cur ^ 1], saved + L.s_gates, eo, B, E, n_last, buf[cur],
                                                                             dscores);
    SATRANS_CHECK_LAUNCH("mmoe_mix_bwd_kernel");
    const float* dz = buf[cur];
    cur ^= 1;
    // experts (dense): the last product WRITES dx;  gate (routed): the last product ADDS its dx to the experts'
    if ((rc = experts_bwd(L.rows, L.x, dz, d->x, d->C, saved, dx, buf, cur, part, st))) return rc;
    return dnn_bwd<true>(L.rows, L.g, dscores, d->x, saved, 1, dx, buf, cur, part, st);
}
