// The host side of grouped_gemm.h for the scenario heads (mmoe.hip, ple.hip, sharedbottom.hip, adasparse.hip): what a layer and
// a batch look like to a launch, the three launches of a layer's forward and backward, the per-layer grid check, and the walks
// over a DNN and over the dense block-diagonal expert stack, each with the dropout option of the dense launches as a template
// argument that defaults off (esmm.hip is its one user so far).  It sits in the same unnamed namespace as the kernels, so every
// file still launches its own kernel copies.  star.hip keeps its own launches (the SHARED wrappers, a reduce of its own) and
// does not include this header.
#pragma once
#include <algorithm>

#include "grouped_gemm.h"

namespace satrans {
namespace {

// a layer as the launches see it: G blocks of [N, K] weights per group of parameters (dense: G blocks in all; routed: G blocks
// of every task).  G = 1 for gates, towers, bottoms and for a first expert layer, whose blocks share their input and so form
// one product of N = blocks * n_1.
struct Lyr {
    int K, N, G;
    const float *w, *b;
    float *gw, *gb;
};

// what a launch needs from the batch.  T = 0, order = seg = nullptr: nothing is routed (dense launches only).
struct Rows {
    int B, T;
    const int32_t *order, *seg;
    int64_t slots, dw_slots, tiles, chunks;      // routed row tiles and chunks (seg_walk.h's bound), dense row tiles and chunks
};

inline Rows rows_of(int B, int T, const int32_t* order, const int32_t* seg) {
    return Rows{B, T, order, seg, seg_slots(B, T, kTM), seg_slots(B, T, kDwChunk), ceil_div(B, kTM), ceil_div(B, kDwChunk)};
}

// The floats of a layer's partials (weights, then biases: the layer in hand owns the whole partials region), or
// SATRANS_E_UNSUPPORTED when one of its launches would not fit: the tile products, the weight gradient, the ordered reduce.
inline int64_t layer_part(const Rows& r, bool routed, const Lyr& y, const char* who, const char* name, int l) {
    const int64_t rows = (routed ? r.slots : r.tiles) * y.G, units = (routed ? r.dw_slots : r.chunks) * y.G;
    SATRANS_REQUIRE((int64_t)y.N * y.K <= 0x7fffffffLL && rows * ceil_div(std::max(y.N, y.K), kTN) <= 0x7fffffffLL &&
                        units * ceil_div(y.N, kTM) * ceil_div(y.K, kTN) <= 0x7fffffffLL &&
                        ((int64_t)y.N * y.K + y.N) * y.G * (routed ? r.T : 1) <= 0x7fffffffLL * (int64_t)kThreads,
                    SATRANS_E_UNSUPPORTED, "%s: %s layer %d (%d x %d) at B=%d needs more than 2^31 workgroups", who, name, l, y.N, y.K,
                    r.B);
    return units * y.N * ((int64_t)y.K + 1);
}

// out[:, block * ogo + n] = epilogue(in[:, block * igo + k] W^T) of one layer; in / out are rows of ldin / ldout floats; `add`:
// added to what out holds.  DROP (dense layers only; grouped_gemm.h's DropArgs, with layer, site and per set for this layer): the
// hidden layer's dropout in its epilogue.
template <bool ROUTED, bool DROP = false>
int launch_fwd(const Rows& r, const Lyr& y, const float* in, int ldin, int igo, int relu, float* out, int ldout, int ogo,
               hipStream_t st, int add = 0, const DropArgs& dr = DropArgs{}) {
    static_assert(!(ROUTED && DROP), "dropout is built for the dense launches");
    const int ntiles = (int)ceil_div(y.N, kTN);
    const int64_t units = (ROUTED ? r.slots : r.tiles) * y.G;
    if constexpr (DROP) {
        mmoe_gemm_drop_kernel<false><<<(unsigned)(units * ntiles), kThreads, 0, st>>>(in, ldin, igo, r.B, y.K, y.N, y.G, ntiles, y.w, y.b,
                                                                                      relu, nullptr, add, out, ldout, ogo, dr);
        SATRANS_CHECK_LAUNCH("mmoe_gemm_drop_kernel (forward)");
        return SATRANS_OK;
    }
    mmoe_gemm_kernel<false, ROUTED><<<(unsigned)(units * ntiles), kThreads, 0, st>>>(in, ldin, igo, r.order, r.seg, r.B, y.K, y.N, r.T, y.G,
                                                                                     ntiles, y.w, y.b, relu, nullptr, add, out, ldout, ogo);
    SATRANS_CHECK_LAUNCH("mmoe_gemm_kernel (forward)");
    return SATRANS_OK;
}

// the backward of one layer: its parameter gradients from (dz, hin) through `part`, the start of the partials region, then
// din = dz W, masked by hin > 0 (when masked), added to what din holds (when add).  dz rows of ldz floats with block offset
// y.N; hin / din rows of ldh floats with block offset hgo.  DROP: hin went through dropout, so the masked din is also scaled
// (dr.scale; nothing else of dr is read).
template <bool ROUTED, bool DROP = false>
int launch_bwd(const Rows& r, const Lyr& y, const float* dz, int ldz, const float* hin, int ldh, int hgo, bool masked, int add,
               float* din, float* part, hipStream_t st, const DropArgs& dr = DropArgs{}) {
    static_assert(!(ROUTED && DROP), "dropout is built for the dense launches");
    const int64_t NK = (int64_t)y.N * y.K;
    const int ntiles = (int)ceil_div(y.N, kTM), ktiles = (int)ceil_div(y.K, kTN);
    const int64_t units = (ROUTED ? r.dw_slots : r.chunks) * y.G;
    const int groups = (ROUTED ? r.T : 1) * y.G;
    float* part_w = part;
    float* part_b = y.b ? part_w + units * NK : nullptr;
    mmoe_dw_kernel<ROUTED><<<(unsigned)(units * ntiles * ktiles), kThreads, 0, st>>>(dz, ldz, y.N, hin, ldh, hgo, r.order, r.seg, r.B, y.K,
                                                                                    y.N, r.T, y.G, ntiles, ktiles, part_w, part_b);
    SATRANS_CHECK_LAUNCH("mmoe_dw_kernel");
    const int64_t elems = (NK + (y.b ? y.N : 0)) * groups;
    mmoe_reduce_kernel<ROUTED><<<(unsigned)ceil_div(elems, kThreads), kThreads, 0, st>>>(part_w, part_b, r.seg, r.B, NK, y.N, r.T, groups,
                                                                                        y.G, (int)r.chunks, y.gw, y.gb);
    SATRANS_CHECK_LAUNCH("mmoe_reduce_kernel");
    const int otiles = (int)ceil_div(y.K, kTN);      // contraction over this layer's N outputs, K columns out
    const int64_t gunits = (ROUTED ? r.slots : r.tiles) * y.G;
    if constexpr (DROP) {
        mmoe_gemm_drop_kernel<true><<<(unsigned)(gunits * otiles), kThreads, 0, st>>>(dz, ldz, y.N, r.B, y.N, y.K, y.G, otiles, y.w, nullptr, 0,
                                                                                      masked ? hin : nullptr, add, din, ldh, hgo, dr);
        SATRANS_CHECK_LAUNCH("mmoe_gemm_drop_kernel (backward)");
        return SATRANS_OK;
    }
    mmoe_gemm_kernel<true, ROUTED><<<(unsigned)(gunits * otiles), kThreads, 0, st>>>(dz, ldz, y.N, r.order, r.seg, r.B, y.N, y.K, r.T, y.G,
                                                                                    otiles, y.w, nullptr, 0, masked ? hin : nullptr, add,
                                                                                    din, ldh, hgo);
    SATRANS_CHECK_LAUNCH("mmoe_gemm_kernel (backward)");
    return SATRANS_OK;
}

// ---- chains of layers -----------------------------------------------------------------------------------------------------------

// a DNN (and, for gates and towers, its final layer) and where its hidden rows are saved
struct Chain {
    int n;
    bool routed;
    Lyr y[kMaxH + 1];
    int64_t s[kMaxH + 1];
};

// an expert DNN of `blocks` blocks over `in` columns: layer 1 one product, then block-diagonal
inline void chain_experts(Chain& c, bool routed, int blocks, int layers, const int32_t* width, int in, const float* const* w,
                          const float* const* b) {
    c.n = layers, c.routed = routed;
    for (int l = 0; l < layers; ++l) {
        c.y[l] = l == 0 ? Lyr{in, blocks * width[l], 1, w[l], b[l], nullptr, nullptr}
                        : Lyr{in, width[l], blocks, w[l], b[l], nullptr, nullptr};
        in = width[l];
    }
}

// a gate, tower or bottom DNN of `hidden` layers over `in` columns and its final layer of `fin` outputs (fin = 0: none)
inline void chain_dnn(Chain& c, bool routed, int hidden, const int32_t* width, int in, int fin, const float* const* w,
                      const float* const* b, const float* final_w, const float* final_b) {
    c.n = hidden + (fin > 0), c.routed = routed;
    for (int l = 0; l < c.n; ++l) {
        const bool last = l == hidden;
        c.y[l] = Lyr{in, last ? fin : width[l], 1, last ? final_w : w[l], last ? final_b : b[l], nullptr, nullptr};
        in = c.y[l].N;
    }
}

// the grids of a chain's layers; per_part grows to the largest partials region among them
inline int chain_fits(const Rows& r, const Chain& c, const char* who, const char* name, int64_t& per_part) {
    for (int l = 0; l < c.n; ++l) {
        const int64_t part = layer_part(r, c.routed, c.y[l], who, name, l);
        if (part < 0) return (int)part;
        per_part = std::max(per_part, part);
    }
    return SATRANS_OK;
}

// every pointer of a chain in a descriptor (P = const float) or in its gradients (P = float); experts: no final layer
template <class P>
bool chain_has(const Chain& c, P* const* w, P* const* b, P* final_w, bool experts) {
    const int hidden = experts ? c.n : c.n - 1;
    for (int l = 0; l < hidden; ++l)
        if (!w[l] || !b[l]) return false;
    return experts || final_w;
}

inline void set_grads(Chain& c, float* const* w, float* const* b, float* final_w, float* final_b, bool experts) {
    for (int l = 0; l < c.n; ++l) {
        const bool fin = !experts && l == c.n - 1;
        c.y[l].gw = fin ? final_w : w[l];
        c.y[l].gb = fin ? final_b : b[l];
    }
}

// a gate or tower DNN and its final layer, forward: hidden rows into saved, the final layer's output into `out` (`add`: added
// to what `out` holds).  DROP: every hidden layer l drops with (dr.seed, dr.step, layer l, dr.site); the final layer does not.
template <bool ROUTED, bool DROP = false>
int dnn_fwd(const Rows& r, const Chain& c, const float* in, float* saved, float* out, hipStream_t st, int add = 0,
            DropArgs dr = DropArgs{}) {
    for (int l = 0; l < c.n; ++l) {
        const bool fin = l == c.n - 1;
        float* o = fin ? out : saved + c.s[l];
        dr.layer = l, dr.per = 0;
        const int rc = DROP && !fin ? launch_fwd<ROUTED, DROP>(r, c.y[l], in, c.y[l].K, 0, 1, o, c.y[l].N, 0, st, 0, dr)
                                    : launch_fwd<ROUTED>(r, c.y[l], in, c.y[l].K, 0, fin ? 0 : 1, o, c.y[l].N, 0, st, fin ? add : 0);
        if (rc) return rc;
        in = o;
    }
    return SATRANS_OK;
}

// the backward of a DNN from dz of its last layer, alternating the two dz buffers (cur: the one the next product writes).  The
// first layer's input gradient goes to din (written, or added when add); a null din: to buf[cur], which then counts as written.
// DROP: the saved hidden rows went through dropout (dr.scale).
template <bool ROUTED, bool DROP = false>
int dnn_bwd(const Rows& r, const Chain& c, const float* dz, const float* in, const float* saved, int add, float* din, float* buf[2],
            int& cur, float* part, hipStream_t st, const DropArgs& dr = DropArgs{}) {
    for (int l = c.n - 1; l >= 0; --l) {
        const Lyr& y = c.y[l];
        const bool first = l == 0;
        float* o = first && din ? din : buf[cur];
        if (int rc = launch_bwd<ROUTED, DROP>(r, y, dz, y.N, first ? in : saved + c.s[l - 1], y.K, 0, !first, first ? add : 0, o, part, st, dr))
            return rc;
        if (o != din) cur ^= 1;
        dz = o;
    }
    return SATRANS_OK;
}

// the dense block-diagonal expert stack over in [B, ldin]: hidden rows [B, G N] into saved, the last of them the experts' output.
// The layers [0, n) of the chain (n < 0: all).  DROP: block g is site dr.site + g; `blocks` cuts the first layer's one product.
template <bool DROP = false>
int experts_fwd(const Rows& r, const Chain& c, const float* in, int ldin, float* saved, hipStream_t st, int n = -1, int blocks = 1,
                DropArgs dr = DropArgs{}) {
    for (int l = 0; l < (n < 0 ? c.n : n); ++l) {
        const Lyr& y = c.y[l];
        float* out = saved + c.s[l];
        dr.layer = l, dr.per = l == 0 ? y.N / blocks : 0;
        if (int rc = launch_fwd<false, DROP>(r, y, in, ldin, l == 0 ? 0 : y.K, 1, out, y.N * y.G, y.N, st, 0, dr)) return rc;
        in = out;
        ldin = y.N * y.G;
    }
    return SATRANS_OK;
}

// its backward from dz of the last layer; the first layer WRITES din [B, ldin].  DROP: the saved rows went through dropout.
template <bool DROP = false>
int experts_bwd(const Rows& r, const Chain& c, const float* dz, const float* in, int ldin, const float* saved, float* din,
                float* buf[2], int& cur, float* part, hipStream_t st, const DropArgs& dr = DropArgs{}) {
    for (int l = c.n - 1; l > 0; --l) {
        const Lyr& y = c.y[l];
        if (int rc = launch_bwd<false, DROP>(r, y, dz, y.N * y.G, saved + c.s[l - 1], y.K * y.G, y.K, true, 0, buf[cur], part, st, dr))
            return rc;
        dz = buf[cur];
        cur ^= 1;
    }
    return launch_bwd<false>(r, c.y[0], dz, c.y[0].N, in, ldin, 0, false, 0, din, part, st);
}

}  // namespace
}  // namespace satrans
