// Scenario-routed MMoE head (reference models/mmoe.py:142-171 with the loss of mtl_basemodel.py:268-269) for a mixed batch.
// The reference runs every task's gate and tower over every row and then keeps the column of the row's own scenario; here the
// experts run over all rows (dense products) and a row goes through its OWN task's gate, mixture, tower and logit only
// (scenario-grouped products over order / seg, walked as seg_walk.h describes).
//
// Layout, the tile product and the kernels themselves are in grouped_gemm.h, shared with ple.hip; this file holds the layout
// of the saved rows and the workspace, the validation and the launches.
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
#include <algorithm>

#include "grouped_gemm.h"

namespace satrans {
namespace {

// ---- host -----------------------------------------------------------------------------------------------------------------------

// a layer of one of the three DNNs as the launches see it: G groups of [N, K] weights (G = 1 for routed layers and for the
// experts' first layer, whose E blocks share x and so form one product of N = E n_1)
struct Lyr {
    int K, N, G;
    const float *w, *b;
    float *gw, *gb;
};

struct MmoeLayout {
    int nx, ng, nt;                                   // layers of the three chains (gate and tower: hidden + final)
    Lyr x[kMaxH], g[kMaxH + 1], t[kMaxH + 1];
    int64_t slots, dw_slots, tiles, chunks;
    int64_t n_last;                                   // width of an expert's output
    // saved (floats from its start): gates [B,E], mixture [B,n_last], scores [B,E], then the hidden rows
    int64_t s_gates, s_mix, s_scores, s_x[kMaxH], s_g[kMaxH], s_t[kMaxH], saved;
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
    L.nx = d->n_expert, L.ng = d->n_gate + 1, L.nt = d->n_tower + 1;
    int prev = d->C;
    for (int l = 0; l < L.nx; ++l) {
        const int n = d->expert_width[l];
        SATRANS_REQUIRE(E * n <= 0x7fffffffLL / 4, SATRANS_E_UNSUPPORTED, "%s: E * expert_width[%d] = %lld", who, l, (long long)(E * n));
        L.x[l] = l == 0 ? Lyr{prev, (int)(E * n), 1, d->expert_w[l], d->expert_b[l], nullptr, nullptr}
                        : Lyr{prev, n, (int)E, d->expert_w[l], d->expert_b[l], nullptr, nullptr};
        prev = n;
    }
    L.n_last = prev;
    prev = d->C;
    for (int l = 0; l < L.ng; ++l) {
        const bool fin = l == L.ng - 1;
        L.g[l] = Lyr{prev, fin ? (int)E : d->gate_width[l], 1, fin ? d->gate_final_w : d->gate_w[l], fin ? nullptr : d->gate_b[l],
                     nullptr, nullptr};
        prev = L.g[l].N;
    }
    prev = (int)L.n_last;
    for (int l = 0; l < L.nt; ++l) {
        const bool fin = l == L.nt - 1;
        L.t[l] = Lyr{prev, fin ? 1 : d->tower_width[l], 1, fin ? d->tower_final_w : d->tower_w[l], fin ? d->out_bias : d->tower_b[l],
                     nullptr, nullptr};
        prev = L.t[l].N;
    }
    L.slots = seg_slots(B, d->T, kTM);
    L.dw_slots = seg_slots(B, d->T, kDwChunk);
    L.tiles = ceil_div(B, kTM);
    L.chunks = ceil_div(B, kDwChunk);
    int64_t at = 0, per_part = 0;
    L.max_w = std::max<int64_t>(L.n_last, E);
    auto take = [&](int64_t n) {
        const int64_t a = at;
        at += B * n;
        return a;
    };
    L.s_gates = take(E);
    L.s_mix = take(L.n_last);
    L.s_scores = take(E);
    for (int l = 0; l < L.nx; ++l) {
        const Lyr& y = L.x[l];
        const int64_t wide = (int64_t)y.N * y.G;
        L.s_x[l] = take(wide);
        L.max_w = std::max(L.max_w, wide);
        per_part = std::max(per_part, L.chunks * y.G * y.N * ((int64_t)y.K + 1));
        SATRANS_REQUIRE((int64_t)y.N * y.K <= 0x7fffffffLL && L.tiles * y.G * ceil_div(std::max(y.N, y.K), kTN) <= 0x7fffffffLL &&
                            L.chunks * y.G * ceil_div(y.N, kTM) * ceil_div(y.K, kTN) <= 0x7fffffffLL,
                        SATRANS_E_UNSUPPORTED, "%s: expert layer %d (%d x %d) at B=%d needs more than 2^31 workgroups", who, l, y.N,
                        y.K, d->B);
    }
    for (int c = 0; c < 2; ++c) {
        const int nl = c ? L.nt : L.ng;
        for (int l = 0; l < nl; ++l) {
            const Lyr& y = c ? L.t[l] : L.g[l];
            if (l < nl - 1) {
                (c ? L.s_t : L.s_g)[l] = take(y.N);
                L.max_w = std::max<int64_t>(L.max_w, y.N);
            }
            per_part = std::max(per_part, L.dw_slots * y.N * ((int64_t)y.K + 1));
            SATRANS_REQUIRE((int64_t)y.N * y.K <= 0x7fffffffLL && L.slots * ceil_div(std::max(y.N, y.K), kTN) <= 0x7fffffffLL &&
                                L.dw_slots * ceil_div(y.N, kTM) * ceil_div(y.K, kTN) <= 0x7fffffffLL,
                            SATRANS_E_UNSUPPORTED, "%s: %s layer %d (%d x %d) at B=%d needs more than 2^31 workgroups", who,
                            c ? "tower" : "gate", l, y.N, y.K, d->B);
        }
    }
    L.saved = at;
    L.w_dz = 0;
    L.w_dscores = 2 * B * L.max_w;
    L.w_part = L.w_dscores + B * E;
    L.total = L.w_part + per_part;
    return SATRANS_OK;
}

bool mmoe_has_operands(const satrans_mmoe_desc* d) {
    if (!d->x || !d->order || !d->seg || !d->gate_final_w || !d->tower_final_w || !d->out_bias) return false;
    for (int l = 0; l < d->n_expert; ++l)
        if (!d->expert_w[l] || !d->expert_b[l]) return false;
    for (int l = 0; l < d->n_gate; ++l)
        if (!d->gate_w[l] || !d->gate_b[l]) return false;
    for (int l = 0; l < d->n_tower; ++l)
        if (!d->tower_w[l] || !d->tower_b[l]) return false;
    return true;
}

bool mmoe_has_grads(const satrans_mmoe_desc* d, const satrans_mmoe_grads* g) {
    if (!g || !g->gate_final_w || !g->tower_final_w || !g->out_bias) return false;
    for (int l = 0; l < d->n_expert; ++l)
        if (!g->expert_w[l] || !g->expert_b[l]) return false;
    for (int l = 0; l < d->n_gate; ++l)
        if (!g->gate_w[l] || !g->gate_b[l]) return false;
    for (int l = 0; l < d->n_tower; ++l)
        if (!g->tower_w[l] || !g->tower_b[l]) return false;
    return true;
}

// out = epilogue(in W^T) of one layer;  in [B, ldin] with group column offset igo, out [B, G N]
template <bool ROUTED>
int launch_fwd(const satrans_mmoe_desc* d, const MmoeLayout& L, const Lyr& y, const float* in, int ldin, int igo, int relu, float* out,
               hipStream_t st) {
    const int ntiles = (int)ceil_div(y.N, kTN);
    const int64_t units = ROUTED ? L.slots : L.tiles * y.G;
    mmoe_gemm_kernel<false, ROUTED><<<(unsigned)(units * ntiles), kThreads, 0, st>>>(in, ldin, igo, d->order, d->seg, d->B, y.K, y.N, d->T,
                                                                                     y.G, ntiles, y.w, y.b, relu, nullptr, 0, out,
                                                                                     y.N * y.G, y.N);
    SATRANS_CHECK_LAUNCH("mmoe_gemm_kernel (forward)");
    return SATRANS_OK;
}

// the backward of one layer: its parameter gradients from (dz, hin), then din = dz W, masked by hin > 0 (when masked), added
// to what din holds (when add).  dz [B, G N], hin / din [B, ldh] with group column offset hgo.
template <bool ROUTED>
int launch_bwd(const satrans_mmoe_desc* d, const MmoeLayout& L, const Lyr& y, const float* dz, const float* hin, int ldh, int hgo,
               bool masked, int add, float* din, float* workspace, hipStream_t st) {
    const int64_t NK = (int64_t)y.N * y.K;
    const int ntiles = (int)ceil_div(y.N, kTM), ktiles = (int)ceil_div(y.K, kTN);
    const int64_t units = ROUTED ? L.dw_slots : L.chunks * y.G;
    const int groups = ROUTED ? d->T : y.G;
    float* part_w = workspace + L.w_part;
    float* part_b = y.b ? part_w + units * NK : nullptr;
    mmoe_dw_kernel<ROUTED><<<(unsigned)(units * ntiles * ktiles), kThreads, 0, st>>>(dz, y.N * y.G, y.N, hin, ldh, hgo, d->order, d->seg,
                                                                                    d->B, y.K, y.N, d->T, y.G, ntiles, ktiles, part_w,
                                                                                    part_b);
    SATRANS_CHECK_LAUNCH("mmoe_dw_kernel");
    const int64_t elems = (NK + (y.b ? y.N : 0)) * groups;
    mmoe_reduce_kernel<ROUTED><<<(unsigned)ceil_div(elems, kThreads), kThreads, 0, st>>>(part_w, part_b, d->seg, d->B, NK, y.N, d->T,
                                                                                        groups, 1, (int)L.chunks, y.gw, y.gb);
    SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel");
    // contraction over this layer's N outputs, K columns out
    const int otiles = (int)ceil_div(y.K, kTN);
    const int64_t gunits = ROUTED ? L.slots : L.tiles * y.G;
    mmoe_gemm_kernel<true, ROUTED><<<(unsigned)(gunits * otiles), kThreads, 0, st>>>(dz, y.N * y.G, y.N, d->order, d->seg, d->B, y.N, y.K,
                                                                                    d->T, y.G, otiles, y.w, nullptr, 0,
                                                                                    masked ? hin : nullptr, add, din, ldh, hgo);
    SATRANS_CHECK_LAUNCH("mmoe_gemm_kernel (backward)");
    return SATRANS_OK;
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
    SATRANS_REQUIRE(mmoe_has_operands(d) && logit && saved, SATRANS_E_BADARG, "mmoe_fwd: null pointer");
    const int B = d->B, E = d->E, n_last = (int)L.n_last;
    // experts: layer 1 over x, then block-diagonal
    const float* in = d->x;
    int ldin = d->C;
    for (int l = 0; l < L.nx; ++l) {
        float* out = saved + L.s_x[l];
        if ((rc = launch_fwd<false>(d, L, L.x[l], in, ldin, l == 0 ? 0 : L.x[l].K, 1, out, st))) return rc;
        in = out;
        ldin = L.x[l].N * L.x[l].G;
    }
    const float* eo = in;
    // the row's own gate
    in = d->x;
    for (int l = 0; l < L.ng; ++l) {
        const bool fin = l == L.ng - 1;
        float* out = saved + (fin ? L.s_scores : L.s_g[l]);
        if ((rc = launch_fwd<true>(d, L, L.g[l], in, L.g[l].K, 0, fin ? 0 : 1, out, st))) return rc;
        in = out;
    }
    mmoe_mix_fwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(saved + L.s_scores, eo, B, E, n_last, saved + L.s_gates,
                                                                             saved + L.s_mix);
    SATRANS_CHECK_LAUNCH("mmoe_mix_fwd_kernel");
    // the row's own tower, final layer and out bias
    in = saved + L.s_mix;
    for (int l = 0; l < L.nt; ++l) {
        const bool fin = l == L.nt - 1;
        float* out = fin ? logit : saved + L.s_t[l];
        if ((rc = launch_fwd<true>(d, L, L.t[l], in, L.t[l].K, 0, fin ? 0 : 1, out, st))) return rc;
        in = out;
    }
    return SATRANS_OK;
}

extern "C" int satrans_mmoe_bwd(const satrans_mmoe_desc* d, const float* dlogit, float* dx, const float* saved, float* workspace,
                                const satrans_mmoe_grads* g, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MmoeLayout L;
    int rc = mmoe_validate(d, "mmoe_bwd", L);
    if (rc) return rc;
    SATRANS_REQUIRE(mmoe_has_operands(d) && dlogit && dx && saved && workspace && mmoe_has_grads(d, g), SATRANS_E_BADARG,
                    "mmoe_bwd: null pointer");
    for (int l = 0; l < L.nx; ++l) L.x[l].gw = g->expert_w[l], L.x[l].gb = g->expert_b[l];
    for (int l = 0; l < L.ng; ++l) {
        const bool fin = l == L.ng - 1;
        L.g[l].gw = fin ? g->gate_final_w : g->gate_w[l];
        L.g[l].gb = fin ? nullptr : g->gate_b[l];
    }
    for (int l = 0; l < L.nt; ++l) {
        const bool fin = l == L.nt - 1;
        L.t[l].gw = fin ? g->tower_final_w : g->tower_w[l];
        L.t[l].gb = fin ? g->out_bias : g->tower_b[l];
    }
    const int B = d->B, E = d->E, n_last = (int)L.n_last;
    float* buf[2] = {workspace + L.w_dz, workspace + L.w_dz + (size_t)B * L.max_w};
    float* dscores = workspace + L.w_dscores;
    int cur = 0;      // the buffer the next product writes
    // tower: dlogit -> dm
    const float* dz = dlogit;
    for (int l = L.nt - 1; l >= 0; --l) {
        const float* hin = saved + (l == 0 ? L.s_mix : L.s_t[l - 1]);
        if ((rc = launch_bwd<true>(d, L, L.t[l], dz, hin, L.t[l].K, 0, l > 0, 0, buf[cur], workspace, st))) return rc;
        dz = buf[cur];
        cur ^= 1;
    }
    // mixture and softmax: dm -> dz of the experts' last layer, dscores
    const float* eo = saved + L.s_x[L.nx - 1];
    mmoe_mix_bwd_kernel<<<(unsigned)ceil_div(B, kMixRows), kThreads, 0, st>>>(dz, saved + L.s_gates, eo, B, E, n_last, buf[cur], dscores);
    SATRANS_CHECK_LAUNCH("mmoe_mix_bwd_kernel");
    dz = buf[cur];
    cur ^= 1;
    // experts (dense): the last product writes dx
    for (int l = L.nx - 1; l >= 0; --l) {
        const Lyr& y = L.x[l];
        if (l == 0) {
            if ((rc = launch_bwd<false>(d, L, y, dz, d->x, d->C, 0, false, 0, dx, workspace, st))) return rc;
        } else {
            if ((rc = launch_bwd<false>(d, L, y, dz, saved + L.s_x[l - 1], y.K * y.G, y.K, true, 0, buf[cur], workspace, st))) return rc;
            dz = buf[cur];
            cur ^= 1;
        }
    }
    // gate (routed): the last product adds its dx to the experts'
    dz = dscores;
    for (int l = L.ng - 1; l >= 0; --l) {
        const Lyr& y = L.g[l];
        if (l == 0) {
            if ((rc = launch_bwd<true>(d, L, y, dz, d->x, d->C, 0, false, 1, dx, workspace, st))) return rc;
        } else {
            if ((rc = launch_bwd<true>(d, L, y, dz, saved + L.s_g[l - 1], y.K, 0, true, 0, buf[cur], workspace, st))) return rc;
            dz = buf[cur];
            cur ^= 1;
        }
    }
    return SATRANS_OK;
}
