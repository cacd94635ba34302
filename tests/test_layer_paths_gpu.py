"""The layer kernels on the shapes whose route through satrans_layer_fwd / satrans_layer_bwd (csrc/capi.hip) no other module
takes: the fused forward's F > 32 arm, the fused forward paired with the LDS-resident backward, and the shapes that only the
LDS-resident kernels (csrc/layer_lds.hip) serve, with MFMA products or - a MetaNet width that is no multiple of 16 - with scalar
FMA loops.  Every case first asks the library which kernels serve its shape (the descriptor the engine builds), then compares
logits, BCE and every gradient with the CPU oracle, in evaluation mode and in training mode with the kernels' dropout masks
replayed.  Run on an MI355X:  python -m pytest tests/test_layer_paths_gpu.py -m gpu

Measured on the MI355X over the sweep (bounds: logit 2e-5 max(1, |logit|), BCE rel 1e-5, gradient 2e-4 max|g|, attention map
2e-6), largest logit error / largest BCE relative error / worst gradient tensor as a fraction of its max|g|:
  fused forward + LDS backward (F > 32, and D = 64)   3.0e-8 / 1.3e-7 / 4.4e-6 (layer 1 MetaNet LayerNorm bias, F = 38, evaluation)
  LDS only, MFMA arm, no general path                 1.5e-8 / 1.6e-7 / 2.0e-6 (layer 1 LayerNorm bias, head dimension 32, training)
  LDS, MFMA arm, general path possible                1.9e-8 / 4.7e-8 / 1.2e-6 (layer 1 MetaNet LayerNorm weight, training)
  LDS, scalar arm                                     3.0e-8 / 1.7e-7 / 1.2e-6 (layer 0 MetaNet LayerNorm bias, (16, 1, 10, 5), training)
  general path at F = 39 / F = 65                     1.9e-8 / 1.5e-7 / 6.7e-6
  several tiles per workgroup (B = 400)               6.6e-8 / 2.2e-8 / 7.4e-7;  empty scenarios: 6.1e-8 / 9.0e-8 / 2.0e-6
  attention maps: 2.7e-7 (fused F > 32 arm, training), 3.5e-7 (LDS forward, training);  the fused-forward + LDS-backward step
  against the same step on the LDS kernels both ways: layer outputs 8.9e-8, worst gradient tensor 1.5e-6 of its max|g|.
No case needed a bound of its own or the ReLU-kink allowance, and no kernel defect was found: every figure is 25 times or more
inside its bound.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import DEV, note_worst, softmax_side_floor, synthetic_shape_against_oracle

pytestmark = pytest.mark.gpu

# route -> (fused forward, general path supports the shape, scalar-FMA arm); no shape here has a fused backward
FUSED_LDS, LDS_ONLY, LDS_CHOSEN, LDS_SCALAR = "fused fwd + LDS bwd", "LDS only", "LDS, general path possible", "LDS scalar arm"
EXPECT = {FUSED_LDS: (True, True, False), LDS_ONLY: (False, False, False), LDS_CHOSEN: (False, True, False),
          LDS_SCALAR: (False, False, True)}
# (route, D, H, U, F, B, oracle in fp64, samples per backward tile).  fp64 oracle where the contraction is long: D = 64, head
# dimension 32.  B: 21 or 50, whichever leaves a scenario with a full tile followed by a partial one (asserted per case).
CASES = [
    # fused forward, F > 32 arm (its own score loop, __expf, per-element keep flags) + LDS backward; 39 / 65 fields: general path
    (FUSED_LDS, 32, 4, 64, 33, 21, False, 1), (FUSED_LDS, 32, 4, 64, 38, 50, False, 1),
    (FUSED_LDS, 16, 2, 32, 33, 21, False, 2), (FUSED_LDS, 16, 2, 32, 47, 21, False, 1), (FUSED_LDS, 16, 2, 32, 64, 50, False, 1),
    # fused forward, F <= 32 arm at D = 64 (forward-only instantiation) + LDS backward
    (FUSED_LDS, 64, 4, 16, 13, 21, True, 1), (FUSED_LDS, 64, 4, 16, 20, 50, True, 1),
    # LDS kernels both ways, MFMA arm; no general path: head dimension 32, 4, 32, 4
    (LDS_ONLY, 32, 1, 64, 19, 21, True, 2), (LDS_ONLY, 16, 4, 32, 9, 50, False, 8), (LDS_ONLY, 64, 2, 32, 5, 21, True, 5),
    (LDS_ONLY, 16, 4, 16, 33, 21, False, 2),
    # LDS kernels both ways, MFMA arm; the general path supports the shape but is not chosen
    (LDS_CHOSEN, 32, 2, 48, 13, 21, False, 4), (LDS_CHOSEN, 64, 8, 32, 10, 21, True, 2),
    # LDS kernels both ways, scalar arm because U % 16 != 0; the last one with F > 32
    (LDS_SCALAR, 16, 2, 20, 6, 50, False, 8), (LDS_SCALAR, 32, 4, 40, 11, 21, False, 2), (LDS_SCALAR, 16, 1, 10, 5, 50, False, 8),
    (LDS_SCALAR, 64, 4, 24, 9, 21, True, 2), (LDS_SCALAR, 16, 2, 24, 37, 50, False, 1),
]
S = 4                                                      # rows of the scenario table: ids 1..3 and the unused id 0


def _lib():
    """The library with the two size queries that are exported but not part of the public binding (native.SIGNATURES)."""
    from satrans_amd import native as N
    lib = N.lib()
    lib.satrans_layer_bwd_fused_supported.restype, lib.satrans_layer_bwd_fused_supported.argtypes = C.c_int, [C.POINTER(N.LayerDesc)]
    lib.satrans_layer_bwd_slab_floats_lds.restype, lib.satrans_layer_bwd_slab_floats_lds.argtypes = C.c_int64, [C.POINTER(N.LayerDesc)]
    return lib


def _slab_floats(D, U):
    """Floats of one workgroup's gradient slab (csrc/layer_lds.hip, slab_offsets)."""
    return 4 * D * D + 4 * D * U + 6 * D


def _lds_bwd_grid(eng, B):
    """Workgroups per scenario of the LDS backward at batch size B, read back from the slab size the library asks for:
    (S gx + S kReduceSplit) slabs, kReduceSplit = 16."""
    ws = eng.workspace(B)
    d = eng._layer_desc(ws, 0, B, None, None, True)
    n = int(_lib().satrans_layer_bwd_slab_floats_lds(C.byref(d)))
    assert n > 0 and n % (eng.S * _slab_floats(eng.D, eng.U)) == 0, n
    return n // (eng.S * _slab_floats(eng.D, eng.U)) - 16


def _lds_bwd_tile(eng, B):
    """Samples per tile of the LDS backward (plan_bwd: 1..8): a batch of b <= T samples is one tile, so one workgroup."""
    ws = eng.workspace(B)
    T = 0
    for b in range(1, 9):
        d = eng._layer_desc(ws, 0, b, None, None, True)
        n = int(_lib().satrans_layer_bwd_slab_floats_lds(C.byref(d)))
        if n // (eng.S * _slab_floats(eng.D, eng.U)) - 16 == 1:
            T = b
    return T


def _lds_fwd_tile(F, D, H, U):
    """Samples per tile of the LDS forward: plan_fwd / fwd_lds_floats of csrc/layer_lds.hip restated (the library exports no
    query for it); it only guards that a case keeps a partial forward tile."""
    mfma = D % 16 == 0 and U % 16 == 0
    pad, wp = (4, 4) if mfma else (1, 0)
    r4 = lambda n: (n + 3) & ~3

    def floats(T):
        tok = T * F
        hp = max(tok * (U + pad), tok * (D + pad), T * H * F * (F + 1))
        return 4 * r4(tok * (D + pad)) + r4(hp) + max(D * (3 * D + wp), D * (U + wp), U * (D + wp)) + 64

    return max([t for t in range(1, 17) if floats(t) * 4 <= 78 * 1024] or [1])


def _scenario_ids(B, seed):
    return np.random.RandomState(seed).randint(1, S, size=B)


def _full_then_partial(ids, T):
    """Some scenario holds a full tile of T samples followed by a partial one (T = 1: more than one tile)."""
    counts = np.bincount(np.asarray(ids, dtype=np.int64), minlength=S)
    return any(c > T and (c % T != 0 or T == 1) for c in counts)


def _route_check(route, D, H, U, F, ids=None, bwd_tile=None):
    fused, general, scalar = EXPECT[route]

    def check(eng, B):
        lib = _lib()
        assert eng.S == S and lib.satrans_layer_impl() == 0      # (automatic choice: nothing forces a kernel family)
        ws = eng.workspace(B)
        d = eng._layer_desc(ws, 0, B, None, None, True)
        assert not ws["generic"], "the general path took the shape"
        assert bool(lib.satrans_layer_fused_supported(C.byref(d))) == fused
        assert not lib.satrans_layer_bwd_fused_supported(C.byref(d)), "the fused backward took the shape"
        assert bool(lib.satrans_layer_generic_supported(C.byref(d))) == general
        assert (U % 16 != 0) == scalar
        T = _lds_bwd_tile(eng, B)
        if bwd_tile is not None:
            assert T == bwd_tile, (T, bwd_tile)
        if ids is not None:                                       # the batch is no multiple of a tile, and some scenario is not either
            assert (T == 1 or B % T) and _full_then_partial(ids, T), ("no partial backward tile", T, np.bincount(ids))
            if not fused:
                Tf = _lds_fwd_tile(F, D, H, U)
                assert (Tf == 1 or B % Tf) and _full_then_partial(ids, Tf), ("no partial forward tile", Tf, np.bincount(ids))
    return check


def _case_id(c):
    return f"{c[1]}-{c[2]}-{c[3]}-F{c[4]}-B{c[5]}"


@pytest.mark.parametrize("route,D,H,U,F,B,ref64,bwd_tile", CASES, ids=[_case_id(c) for c in CASES])
def test_route_is_asserted_and_matches_the_oracle(route, D, H, U, F, B, ref64, bwd_tile):
    """Every row of the route table at two layers, `SATRANS_GENERIC` unset: the library's own answer about the shape (general
    path not chosen, fused forward / fused backward / general path supported or not, MFMA or scalar arm, samples per backward
    tile) is asserted before any kernel runs; then logits, BCE and every gradient against the oracle in evaluation and in
    training mode (four dropout sites, p = 0.1, masks replayed), on a batch in which a scenario has a full tile followed by a
    partial one."""
    ids = _scenario_ids(B, F)
    synthetic_shape_against_oracle(D, H, U, F, generic=False, B=B, L=2, ref64=ref64, scen_ids=ids,
                                   route_check=_route_check(route, D, H, U, F, ids, bwd_tile), tag=route)


@pytest.mark.parametrize("D,H,U,F", [(32, 4, 64, 39), (16, 2, 32, 65)])
def test_one_field_more_goes_to_the_general_path(monkeypatch, D, H, U, F):
    """The other side of the hand-over: at 39 fields (D = 32) one sample of the LDS backward no longer fits LDS, at 65 fields
    (D = 16) the fused forward is not built either - the general path picks itself, with SATRANS_GENERIC unset, and matches the
    oracle.  (F - 1 fields stay on the fused forward + LDS backward: test_route_is_asserted_and_matches_the_oracle.)"""
    monkeypatch.delenv("SATRANS_GENERIC", raising=False)

    def check(eng, B):
        lib = _lib()
        ws = eng.workspace(B)
        d = eng._layer_desc(ws, 0, B, None, None, True)
        assert ws["generic"], "the general path was not selected"
        assert int(lib.satrans_layer_bwd_slab_floats_lds(C.byref(d))) < 0, "the LDS backward still fits"
        assert bool(lib.satrans_layer_fused_supported(C.byref(d))) == (F <= 64)
        assert lib.satrans_layer_generic_supported(C.byref(d))

    synthetic_shape_against_oracle(D, H, U, F, generic=True, B=21, L=2, route_check=check, tag="general path at the boundary")


@pytest.mark.parametrize("route,D,H,U,F", [(FUSED_LDS, 16, 2, 32, 47), (LDS_ONLY, 32, 1, 64, 19)])
def test_attention_maps_of_the_private_arms(route, D, H, U, F):
    """normalized_att_scores of both layers against the oracle's (atol 2e-6, the general-path test's bound), evaluation and
    training mode with the same replayed masks: the fused forward's F > 32 arm recomputes the map in a third loop of its own -
    wrong keep flags or a missing 1 / (1 - p) there show nowhere else - and the LDS forward writes it from its P image."""
    ids = _scenario_ids(21, F)
    synthetic_shape_against_oracle(D, H, U, F, generic=False, B=21, L=2, ref64=(route == LDS_ONLY), scen_ids=ids,
                                   check_attention=True, route_check=_route_check(route, D, H, U, F), tag="attention maps")


def _fresh_model(D, H, U, F, L=2):
    """The model synthetic_shape_against_oracle builds for this shape (same generators, same seeds), and its id ranges."""
    from satrans_amd import SATrans, SparseFeat
    rng = np.random.RandomState(D + F)
    fields = [f"f{i}" for i in range(F)]
    vocab = [int(rng.randint(5, 60)) for _ in fields]
    vocab[0] = 4
    cols = [SparseFeat(f, vocabulary_size=v + 1, embedding_dim=D) for f, v in zip(fields, vocab)]
    torch.manual_seed(3)                                   # (also the seed of the engine's dropout counters)
    model = SATrans(cols, cols, [fields[0]], [3], att_layer_num=0, domain_att_layer_num=L, att_head_num=H, use_linear=False,
                    use_dnn=False, meta_mode='QK', meta_dnn_hidden_units=(U, D), seed='1021', device='cpu', flag='sota')
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "embedding" in k:
                p.mul_(300.0)
    model.to(DEV); model.device = DEV
    model.compile("adam", "binary_crossentropy")
    return model, vocab


def _batch(vocab, ids, seed):
    rng = np.random.RandomState(seed)
    B = len(ids)
    X = np.stack([rng.randint(0, v, size=B) for v in vocab], axis=1).astype(np.float32)
    X[:, 0] = ids
    y = (rng.rand(B) < 0.4).astype(np.float32)
    return torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)


def test_forward_and_backward_masks_agree_across_files():
    """(32, 4, 64, 36) in training mode, the same model twice with the same dropout counters: as routed - the masks of the
    forward come from layer_fused.hip's F > 32 arm, the backward regenerates them in layer_lds.hip - and with the LDS kernels
    forced both ways (satrans_set_layer_impl(2)), where one file makes both.  Layer outputs within 2e-5, BCE and gradients within
    the route tests' bounds; and the evaluation-mode outputs differ from the training-mode ones, so dropout was on."""
    from satrans_amd import native as N
    D, H, U, F, B = 32, 4, 64, 36, 21
    ids = _scenario_ids(B, F)
    runs = []
    try:
        for impl in (0, 2):
            N.check(N.lib().satrans_set_layer_impl(impl), "set_layer_impl")
            model, vocab = _fresh_model(D, H, U, F)
            X, y = _batch(vocab, ids, 7)
            eng = model._require_engine()
            if impl == 0:
                _route_check(FUSED_LDS, D, H, U, F, ids, 1)(eng, B)
            else:
                assert not eng.workspace(B)["generic"]
            model.train(True)
            bce, reg, grads = eng.loss_and_grads(X, y)
            outs = [a.cpu() for a in eng.layer_outputs(B)]
            counters = (eng.drop_seed, eng.drop_step)
            model.train(False)
            model(X)
            outs_eval = [a.cpu() for a in eng.layer_outputs(B)]
            runs.append((bce, {k: g.cpu() for k, g in grads.items()}, outs, counters, outs_eval))
    finally:
        N.check(N.lib().satrans_set_layer_impl(0), "set_layer_impl")
    (bce0, g0, o0, c0, e0), (bce2, g2, o2, c2, e2) = runs
    assert c0 == c2, "the two runs did not use the same dropout counters"
    assert torch.equal(o0[0], o2[0])
    for l in (1, 2):
        note_worst("masks across files", "layer output abs err", float((o0[l] - o2[l]).abs().max()), f"layer {l - 1}")
        np.testing.assert_allclose(o0[l].numpy(), o2[l].numpy(), rtol=0, atol=2e-5, err_msg=f"output of layer {l - 1}")
        np.testing.assert_allclose(e0[l].numpy(), e2[l].numpy(), rtol=0, atol=2e-5, err_msg=f"evaluation output of layer {l - 1}")
        # (ten times the bound the two training runs agree to; measured 8e-3 - the residual dominates these rows)
        assert float((o0[l] - e0[l]).abs().max()) > 10 * 2e-5, "training-mode output equals the evaluation-mode one: no dropout"
    assert bce0 == pytest.approx(bce2, rel=1e-5)
    assert set(g0) == set(g2)
    for k in g0:
        scale = max(1e-6, float(g2[k].abs().max()))
        note_worst("masks across files", "gradient err / max|g|", float((g0[k] - g2[k]).abs().max()) / scale, k)
        np.testing.assert_allclose(g0[k].numpy(), g2[k].numpy(), rtol=0, atol=2e-4 * scale + softmax_side_floor(k, g2, 1e-8),
                                   err_msg=k)


@pytest.mark.parametrize("route,D,H,U,F", [(FUSED_LDS, 16, 2, 32, 47), (FUSED_LDS, 64, 4, 16, 13), (LDS_ONLY, 16, 4, 32, 9),
                                           (LDS_CHOSEN, 32, 2, 48, 13), (LDS_SCALAR, 32, 4, 40, 11)])
def test_a_sample_alone_equals_the_sample_in_the_batch(route, D, H, U, F):
    """Evaluation-mode logit of a sample computed at B = 1 against the same sample inside a batch of 21: BIT equality on every
    route.  Read from the kernels: no forward here sums over samples, and the tile a sample falls into decides only WHICH lane
    or work item computes its tokens, not the order of any sum - a token's products are k-ordered fmaf chains, in
    v_mfma_f32_16x16x4_f32 (tokens are columns of the B operand; a column of D depends on its own column of B alone: fused
    `chain`, gemm_tokens_mfma) as in the scalar loops (gemm_tokens: one accumulator per (token, column)); scores, softmax and
    P V run per (sample, head, query row) over j = 0..F-1 in both forwards, LayerNorm per token row, the head per sample."""
    B = 21
    ids = _scenario_ids(B, F)
    model, vocab = _fresh_model(D, H, U, F)
    X, _ = _batch(vocab, ids, 11)
    eng = model._require_engine()
    _route_check(route, D, H, U, F)(eng, B)
    model.eval()
    model(X)
    batch_logit = eng.last_logit().reshape(-1).clone()
    for b in (0, 8, B - 1):
        model(X[b:b + 1].contiguous())
        assert not eng._ws[1]["generic"]
        assert torch.equal(eng.last_logit().reshape(-1), batch_logit[b:b + 1]), (b, float(eng.last_logit()), float(batch_logit[b]))


# ---- tiles, slabs and empty scenarios of the LDS backward: all on (32, 4, 64, 36), one sample per backward tile ----------------
SLAB_SHAPE = (32, 4, 64, 36)
MULTI_B = 400


def _multi_tile_ids():
    """400 samples, 360 of them in scenario 2: with one sample per tile that scenario has 360 tiles for the ceil(256 / S) = 64
    workgroups of its grid row, so each of them walks five or six tiles."""
    ids = np.array([2] * 360 + [1] * 25 + [3] * 15)
    return ids[np.random.RandomState(5).permutation(MULTI_B)]


def _multi_tile_route(eng, B):
    D, H, U, F = SLAB_SHAPE
    ids = _multi_tile_ids()
    _route_check(FUSED_LDS, D, H, U, F, ids, 1)(eng, B)
    gx, T = _lds_bwd_grid(eng, B), _lds_bwd_tile(eng, B)
    tiles = -(-int(np.bincount(ids).max()) // T)
    assert tiles > 2 * gx, ("no workgroup walks several tiles", tiles, gx)


def test_a_workgroup_of_the_lds_backward_walks_several_tiles():
    """layer_bwd_kernel accumulates the weight gradients of all tiles a workgroup walks into its slab (`first`, then +=): a
    scenario with more tiles than the grid has workgroups per scenario (asserted from the slab size the library reports), every
    gradient against the oracle."""
    D, H, U, F = SLAB_SHAPE
    synthetic_shape_against_oracle(D, H, U, F, generic=False, B=MULTI_B, L=2, scen_ids=_multi_tile_ids(),
                                   route_check=_multi_tile_route, tag="LDS backward, several tiles per workgroup")


def test_empty_and_single_sample_scenarios_after_a_full_batch():
    """One scenario without a sample and one with a single sample, on an engine whose previous step (same batch size, so the
    same `slabs` workspace, which is torch.empty) populated every scenario: the slabs of workgroups that find no tile must read
    as zeros, not as what the previous step left.  Gradients of the second batch against the oracle."""
    D, H, U, F = SLAB_SHAPE
    B = 50
    ids = np.full(B, 3)
    ids[17] = 2                                            # scenario 1: nobody; scenario 2: one sample; scenario 3: the rest
    first = np.arange(B) % S                               # every row of the scenario table, the unused id 0 included
    assert np.bincount(ids, minlength=S).tolist() == [0, 0, 1, 49] and np.bincount(first, minlength=S).min() > 0
    synthetic_shape_against_oracle(D, H, U, F, generic=False, B=B, L=2, scen_ids=ids, first_scen_ids=first,
                                   route_check=_route_check(FUSED_LDS, D, H, U, F, None, 1), tag="LDS backward, empty scenarios")


def test_two_runs_of_the_multi_tile_batch_leave_the_same_bits():
    """The slab accumulation (fixed order over a workgroup's tiles) and the two-level slab reduction (index order) promise
    bitwise reproducible gradients (csrc/layer_lds.hip, file header): two fresh models, training mode, same counters."""
    D, H, U, F = SLAB_SHAPE
    ids = _multi_tile_ids()
    res = []
    for _ in range(2):
        model, vocab = _fresh_model(D, H, U, F)
        X, y = _batch(vocab, ids, 13)
        eng = model._require_engine()
        _multi_tile_route(eng, MULTI_B)
        model.train(True)
        bce, reg, grads = eng.loss_and_grads(X, y)
        res.append((bce, {k: g.clone() for k, g in grads.items()}))
        del model, eng
    assert res[0][0] == res[1][0]
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), f"run-to-run difference in {k}"
