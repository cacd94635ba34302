"""GPU parity: the HIP path (through the C ABI) against golden vectors recorded from the reference and against
the CPU oracle on the same seeded inputs.  Run on an MI355X:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest
import torch

from oracle import satrans_oracle as O
from tests.helpers import (NATIVE_ADAM_CASES, NATIVE_CASES, NATIVE_TRAIN_CASES, Case, assert_grad_close_but_for_kinks, build_model,
                           oracle_grads_probing_kinks, softmax_side_floor)
from tests.helpers import synthetic_shape_against_oracle as _synthetic_shape_against_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# fp32 tolerance on logits: SURVEY.md §6 measured 2.3e-7 between fp32 and fp64 forwards; 1e-5 is the stated bar
LOGIT_ATOL = 1e-5


def assert_close_but_for_kinks(got, want, rtol, atol, err_msg, frac=5e-4, slack=20.0, kinks=None):
    """assert_allclose, except that a fraction `frac` of the elements may sit up to `slack` x outside it - only when the ORACLE saw
    MetaNet hidden units within fp32 rounding of the ReLU's kink on these very inputs (`kinks` > 0: the count of O.KINK_PROBE; at B = 8,192 a step evaluates 6e7 hidden units and a few of them always are).
    A ReLU whose pre-activation is within the products' error of zero takes the other branch than the oracle's: the gradient
    of the one sample involved then changes by O(1) of that sample's share, which an element-wise bound at 1e-4 of the
    largest entry sees in the table rows that sample touched.  With fp32 products (error ~1e-7) 8,192 samples x 2 x 64 hidden
    units x 19 fields almost never hold such a unit."""
    if not kinks:
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=err_msg)
        return
    err = np.abs(got - want)
    tol = atol + rtol * np.abs(want)
    bad = err > tol
    assert float(bad.mean()) <= frac, (err_msg, float(bad.mean()))
    assert bool((err <= slack * tol).all()), (err_msg, float((err / tol).max()))


def sd_to_cpu(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def sd_aliased(model, dtype=None):
    """state_dict on the CPU with the reference's ALIASING kept: keys that share storage in the model (K_/V_meta_mlp and
    domain_map_dnn_K/V are the Q objects without 'pos', satrans.py:46) share ONE tensor, so the oracle sees one leaf and its
    gradient is the sum over the roles - as in the reference."""
    out, by_ptr = {}, {}
    for k, v in model.state_dict().items():
        key = (v.data_ptr(), tuple(v.shape))
        if key not in by_ptr:
            t = v.detach().cpu()
            by_ptr[key] = t.to(dtype) if dtype is not None else t
        out[k] = by_ptr[key]
    return out


@pytest.mark.parametrize("name", NATIVE_CASES)
def test_forward_matches_reference_golden(name):
    c = Case(name)
    model = build_model(c, DEV)
    model.eval()
    model.capture_attention = True
    prob = model(c.X.to(DEV))
    eng = model._engine
    want = c.arrays("out")
    acts = eng.layer_outputs(c.X.shape[0])
    assert np.array_equal(acts[0].cpu().numpy(), want["att_input"]), "gather must be bit-exact"
    for l in range(c.meta["L"]):
        np.testing.assert_allclose(acts[l + 1].cpu().numpy(), want[f"layer{l}"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(model.domain_int_layers[l].normalized_att_scores.cpu().numpy(), want[f"att{l}"],
                                   rtol=0, atol=2e-6)
    np.testing.assert_allclose(eng.last_logit().cpu().numpy(), want["logit"], rtol=0, atol=LOGIT_ATOL)
    np.testing.assert_allclose(prob.cpu().numpy(), want["prob"], rtol=0, atol=2e-6)
    assert prob.shape == (c.X.shape[0], 1) and prob.dtype == torch.float32


@pytest.mark.parametrize("name", NATIVE_TRAIN_CASES)
def test_gradients_match_reference_golden(name):
    c = Case(name)
    model = build_model(c, DEV)
    model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
    model.eval()                                   # no dropout: the golden step was recorded with p = 0
    eng = model._require_engine()
    bce, reg, grads = eng.loss_and_grads(c.X.to(DEV), c.y.to(DEV))
    assert bce == pytest.approx(float(c.z["train/bce"]), rel=2e-6)
    assert reg == pytest.approx(float(c.z["train/reg"]), rel=1e-5)
    want = c.arrays("grad")
    assert set(grads) == set(want)
    # 40 fields x 64 dims: longer fp32 sums and projection gradients of ~1e-5 that are differences of nearly equal softmax
    # terms carry ~5e-9 of cancellation noise in any fp32 evaluation (same floor as the ragged-batch test)
    rel, floor = (1e-4, 5e-9) if name == "small_d64_u128" else (5e-5, 1e-9)
    for k, g in want.items():
        scale = max(1e-6, float(np.abs(g).max()))
        np.testing.assert_allclose(grads[k].cpu().numpy(), g, rtol=0, atol=rel * scale + floor, err_msg=k)


def test_gradients_are_the_same_bits_run_to_run():
    """Same inputs, same weights: the same bits (no float atomics anywhere on the path; every reduction in a fixed order)."""
    c = Case("aliccp_sota")
    outs = []
    for _ in range(2):
        model = build_model(c, DEV)
        model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
        model.eval()
        _, _, grads = model._require_engine().loss_and_grads(c.X.to(DEV), c.y.to(DEV))
        outs.append({k: g.cpu() for k, g in grads.items()})
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])


def test_fp32_products_against_the_fp64_oracle():
    """The kernels' products are v_mfma_f32_16x16x4_f32 (bit for bit an fmaf chain): logits and every gradient of the
    AliCCP-shaped golden case against the SAME graph evaluated in fp64 by the oracle.  Recorded on an MI355X: logits 1.4e-8 on
    values of ~0.1; worst gradient 1.8e-5 of the tensor's largest entry (the cancellation-dominated W_Query / W_Key gradients)."""
    c = Case("aliccp_sota")
    spec = c.spec()
    P64 = c.tensors("param", torch.float64)
    _, logit64 = O.forward(P64, c.X, spec)
    _, _, ref = O.loss_and_grads(P64, c.X, c.y, spec)             # BCE(sum) + regulariser, as loss_and_grads of the engine
    model = build_model(c, DEV)
    model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
    model.eval()
    eng = model._require_engine()
    model(c.X.to(DEV))
    logit_err = float((eng.last_logit().cpu().double().reshape(-1) - logit64.detach().reshape(-1)).abs().max())
    _, _, grads = eng.loss_and_grads(c.X.to(DEV), c.y.to(DEV))
    worst = 0.0
    for k, g in grads.items():
        if k in ref and float(ref[k].abs().max()) > 1e-7:
            worst = max(worst, float((g.cpu().double() - ref[k]).abs().max() / ref[k].abs().max()))
    print(f"fp32 products against fp64: logit {logit_err:.2e} gradient {worst:.2e}")
    assert logit_err <= 2e-7 and worst <= 3e-5, (logit_err, worst)


def _trained_aliccp_model(steps=120, B=8192, rows_cap=20000, seed=5):
    """An AliCCP-shaped model (19 fields, D = 32, 3 layers, 4 heads, QK; tables capped at `rows_cap` rows per field so that the
    oracle's dense step stays cheap) after `steps` training steps at the baseline batch on labels that can be learnt: logits of
    order 1, MetaNet pre-activations and LayerNorm statistics of a trained network - the regime the near-init golden cases
    (|logit| ~ 0.1) do not reach."""
    from satrans_amd import SATrans, SparseFeat
    import bench
    rng = np.random.RandomState(seed)
    vocab = {f: min(bench.ALICCP_MAX[f], rows_cap) + 2 for f in bench.ALICCP_FIELDS}
    cols = [SparseFeat(f, vocabulary_size=vocab[f], embedding_dim=32) for f in bench.ALICCP_FIELDS]
    N = (steps + 1) * B
    X = np.stack([rng.randint(1 if f == '301' else 0, vocab[f] - 1, size=N) for f in bench.ALICCP_FIELDS], axis=1)
    y = ((X[:, 1] % 2 == 0) & (rng.rand(N) < 0.6) | (rng.rand(N) < 0.05)).astype(np.float32)
    X = X.astype(np.float32)
    model = SATrans(cols, cols, ['301'], [3], att_layer_num=0, domain_att_layer_num=3, att_head_num=4,
                    use_linear=False, use_dnn=False, meta_mode='QK', seed='1021', device=DEV, flag='sota')
    model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy")
    model.train()
    eng = model._require_engine()
    Xd, yd = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    for i in range(steps):
        eng.train_step(Xd[i * B:(i + 1) * B], yd[i * B:(i + 1) * B])
    spec = O.PathSpec(sparse=[(f, i) for i, f in enumerate(bench.ALICCP_FIELDS)], dense=[], domain_cols=[18],
                      embedding_dim=32, head_num=4, layer_num=3, flag='sota', meta_mode='QK', meta_units=[32, 64, 32])
    return model, spec, X[steps * B:], y[steps * B:]


# measured on an MI355X (printed by the test; bounds = ~2x the measurement): logit 1.6e-6, worst gradient 4.2e-6 of the tensor's
# largest entry
TRAINED_BOUNDS = (1e-5, 5e-5)


def test_trained_weights_regime_against_the_oracle():
    """After 120 training steps at B = 8,192 (trained weights, |logit| of order 1):
      (a) the TRAINING forward (the kernels of the training step, dropouts switched off) on 2,048 fresh samples against the CPU
          oracle on the same weights: within the 1e-5 bar of SURVEY 8c;
      (b) one training-mode step's gradients (dropout on, masks replayed through the oracle in fp64) at B = 1,024: every
          tensor within the stated fraction of its largest entry, element by element."""
    model, spec, X, y = _trained_aliccp_model()
    eng = model._require_engine()
    sd = sd_to_cpu(model)
    nb = 2048
    Xt = torch.from_numpy(X[:nb])
    _, logit_ref = O.forward(sd, Xt, spec)
    model.eval()
    model(Xt.to(DEV))
    err_eval = float((eng.last_logit().cpu() - logit_ref).abs().max())
    model.train()
    keep_p, eng.drop_p = eng.drop_p, 0.0
    try:
        model(Xt.to(DEV))
        err_train = float((eng.last_logit().cpu() - logit_ref).abs().max())
    finally:
        eng.drop_p = keep_p
    scale_logit = float(logit_ref.abs().max())
    assert scale_logit > 1.0, f"the model did not train (max |logit| {scale_logit})"
    assert err_eval <= 1e-5, ("evaluation forward", err_eval)
    # (b) gradients of a training-mode step, masks replayed
    B = 1024
    Xb, yb = torch.from_numpy(X[:B]), torch.from_numpy(y[:B])
    bce, reg, grads = eng.loss_and_grads(Xb.to(DEV), yb.to(DEV))
    masks = O.dropout_masks(eng.drop_seed, eng.drop_step, B, 19, 32, 4, 3, 0.1)
    sd64 = sd_aliased(model, torch.float64)
    (bce_ref, reg_ref, g_ref), kinks = oracle_grads_probing_kinks(sd64, Xb, yb, spec, O.Dropper("masks", 0.1, masks))
    worst, worst_key = 0.0, None
    for k, g in g_ref.items():
        if k in grads and float(g.abs().max()) > 1e-7:
            e = float((grads[k].cpu().double() - g).abs().max() / g.abs().max())
            if e > worst:
                worst, worst_key = e, k
    print(f"trained weights: max |logit| {scale_logit:.2f}; logit err eval {err_eval:.2e} train {err_train:.2e}; "
          f"worst gradient {worst:.2e} of the tensor's largest entry ({worst_key})")
    lb, gb = TRAINED_BOUNDS
    assert err_train <= lb, err_train
    assert bce == pytest.approx(bce_ref, rel=1e-5)
    for k, g in g_ref.items():
        if k in grads:
            sc = max(1e-6, float(g.abs().max()))
            assert_grad_close_but_for_kinks(grads[k].cpu().numpy(), g.numpy(), gb * sc + softmax_side_floor(k, g_ref, 1e-8),
                                            f"{k} (trained weights)", kinks=kinks)


def test_gate_layer_with_a_metanet_width_that_is_not_2d():
    """a `gate` layer ignores meta_dnn_hidden_units' hidden width, but the fused kernels lay LDS and their
    generated-row records out with the width they are INSTANTIATED for (2 D); sizing either from the descriptor's U (here 48
    at D = 32, and 16 at D = 16) left the softmax caches outside the allocation.  Logits and every gradient against the oracle."""
    from satrans_amd import SATrans, SparseFeat
    for D, H, U in ((32, 4, 48), (16, 2, 16), (32, 4, 32)):
        for flag in ("sota-gate", "sota-bilinear"):
            rng = np.random.RandomState(D + U)
            F, B = 19, 45
            fields = [f"f{i}" for i in range(F)]
            vocab = {f: int(rng.randint(5, 60)) for f in fields}
            vocab[fields[0]] = 4
            cols = [SparseFeat(f, vocabulary_size=vocab[f] + 1, embedding_dim=D) for f in fields]
            model = SATrans(cols, cols, [fields[0]], [3], att_layer_num=0, domain_att_layer_num=2, att_head_num=H, use_linear=False,
                            use_dnn=False, meta_mode='QK', meta_dnn_hidden_units=(U, D), seed='1021', device='cpu', flag=flag)
            with torch.no_grad():
                for k, p in model.named_parameters():
                    if "embedding" in k:
                        p.mul_(300.0)
            state, by_ptr = {}, {}
            for k, v in model.state_dict().items():
                state[k] = by_ptr.setdefault(v.data_ptr(), v.detach().clone())
            X = np.stack([rng.randint(1 if f == fields[0] else 0, vocab[f], size=B) for f in fields], axis=1).astype(np.float32)
            y = (rng.rand(B) < 0.4).astype(np.float32)
            spec = O.PathSpec(sparse=[(f, i) for i, f in enumerate(fields)], dense=[], domain_cols=[0], embedding_dim=D, head_num=H,
                              layer_num=2, flag=flag, meta_mode='QK', meta_units=[D, U, D])
            Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
            model.to(DEV); model.device = DEV
            model.compile("adam", "binary_crossentropy")
            model.eval()
            eng = model._require_engine()
            bce, reg, grads = eng.loss_and_grads(Xt.to(DEV), yt.to(DEV))
            assert not eng._ws[B]["generic"], "the fused kernels were expected to take this shape"
            bce_ref, reg_ref, g_ref = O.loss_and_grads(state, Xt, yt, spec)
            model(Xt.to(DEV))
            _, logit_ref = O.forward(state, Xt, spec)
            np.testing.assert_allclose(eng.last_logit().cpu().numpy().reshape(-1), logit_ref.numpy().reshape(-1), rtol=0,
                                       atol=2e-5 * max(1.0, float(logit_ref.abs().max())))
            assert bce == pytest.approx(bce_ref, rel=1e-5)
            for k, g in g_ref.items():
                if k in grads:
                    sc = max(1e-6, float(g.abs().max()))
                    np.testing.assert_allclose(grads[k].cpu().numpy(), g.numpy(), rtol=0, atol=2e-4 * sc + 1e-8,
                                               err_msg=f"{k} D={D} U={U} {flag}")


@pytest.mark.parametrize("name", NATIVE_ADAM_CASES)
def test_adam_steps_match_reference_golden(name):
    c = Case(name)
    model = build_model(c, DEV)
    model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
    model.eval()
    eng = model._require_engine()
    X, y = c.X.to(DEV), c.y.to(DEV)
    for _ in range(c.meta["adam_steps"]):
        eng.train_step(X, y)
    got, want, grads = sd_to_cpu(model), c.tensors("adam"), c.arrays("grad")
    lr, steps = c.meta["lr"], c.meta["adam_steps"]
    init = c.tensors("param")
    for k, w in want.items():
        # Adam's update lr*m_hat/(sqrt(v_hat)+eps) is ill-conditioned wherever |g| is not >> eps = 1e-8 (sensitivity
        # lr/(|g|+eps)), and after the first step every weight has moved by ~lr = 50x its init scale, so individual
        # elements whose later gradients pass near zero differ by a few % of a step between ANY two correct fp32
        # implementations.  The element-wise bound is therefore loose (10 % of the possible movement) and the tight
        # bound is on the tensor as a whole: relative L2 error of the applied update.  The optimizer arithmetic is
        # pinned exactly by test_optimizer_kernels_exact, the trajectory by the loss history of the fit test.
        err = (got[k] - w).abs().flatten().double()
        if k in grads and float(np.abs(grads[k]).max()) >= 1e-7 and float((w - init[k]).abs().max()) > 0:
            # (a sign flip of one near-zero gradient moves that element by 2*lr, so no max / L2 bound is meaningful)
            assert float(err.median()) <= 2e-3 * lr * steps, (k, float(err.median()))
            assert float(torch.quantile(err, 0.95)) <= 2e-2 * lr * steps, (k, float(torch.quantile(err, 0.95)))
        assert float(err.max()) <= 2.0 * lr * steps + 1e-6, (k, float(err.max()))
    # The moments ARE well-conditioned (exp_avg linear, exp_avg_sq quadratic in the gradients of the steps), so they pin the
    # trajectory tightly: torch.optim.Adam's own state after the same steps of the reference, element by element.
    opt = model.optimizer_state_dict()
    assert opt["step"] == steps
    checked = 0
    # Free-running, the steps after the first see parameters that already differ in their ill-conditioned elements (an
    # embedding element whose gradient is ~eps moves by up to lr = 50x its init scale whichever way the rounding falls), and
    # that feeds back into the LATER gradients at the 1e-3..1e-2 level (measured: 7e-3 of the largest moment on W_Query
    # after three steps).  So against the reference's own end state the moments are only held to 2e-2 of their largest
    # element; the TIGHT pin of the trajectory is test_adam_trajectory_step_by_step_against_the_oracle below, where every
    # step starts from identical state.
    for kind, tol in (("exp_avg", 2e-2), ("exp_avg_sq", 2e-2)):
        for k, w in c.arrays(f"opt/{kind}").items():
            assert k in opt["state"], k
            checked += 1
            if k in grads and float(np.abs(grads[k]).max()) < 1e-7:
                continue                                   # mathematically-zero gradient: its moments are rounding noise
            g = opt["state"][k][kind].numpy()
            scale = float(np.abs(w).max())
            np.testing.assert_allclose(g, w, rtol=1e-5, atol=tol * scale + 1e-30, err_msg=f"{kind}/{k}")
    assert checked >= 2 * len(grads)


@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos", "small_qkv"])
def test_adam_trajectory_step_by_step_against_the_oracle(name):
    """The optimizer on the reference's trajectory, without the chaos: before every step the CPU oracle (torch.optim.Adam on
    the reference's arithmetic, pinned to the reference's own moments at 2e-5 in tests/test_oracle_golden.py) is given the
    GPU's current parameters and moments bit for bit; both then take ONE step on the same batch.  Moments after the step must
    agree element by element at single-gradient accuracy, parameters wherever the update is well-conditioned."""
    c = Case(name)
    model = build_model(c, DEV)
    lr = c.meta["lr"]
    model.compile(torch.optim.Adam(model.parameters(), lr=lr), "binary_crossentropy")
    model.eval()
    eng = model._require_engine()
    X, y = c.X.to(DEV), c.y.to(DEV)
    tr = O.OracleTrainer(c.tensors("param"), c.spec(), lr=lr)
    for step in range(3):
        sd, opt = sd_to_cpu(model), model.optimizer_state_dict()
        for k, leaf in tr.leaves.items():
            leaf.data.copy_(sd[k])
            st = opt.get("state", {}).get(k)
            if st is not None:
                tr.optim.state[leaf] = dict(step=torch.tensor(float(step)), exp_avg=st["exp_avg"].clone(),
                                            exp_avg_sq=st["exp_avg_sq"].clone())
        tr.step(c.X, c.y)
        eng.train_step(X, y)
        got, gopt = sd_to_cpu(model), model.optimizer_state_dict()
        assert gopt["step"] == step + 1
        for k, leaf in tr.leaves.items():
            if leaf not in tr.optim.state or k not in gopt["state"]:
                continue
            ref_m, ref_v = tr.optim.state[leaf]["exp_avg"], tr.optim.state[leaf]["exp_avg_sq"]
            if float(ref_m.abs().max()) < 1e-8:
                continue                                  # mathematically-zero gradient: rounding noise
            m, v = gopt["state"][k]["exp_avg"], gopt["state"][k]["exp_avg_sq"]
            # (1e-4 / 2e-4 of the largest element is where the fp32 kernels' own rounding sits for the cancellation-heavy
            # tensors - the scenario embeddings: 128 numbers that sum every token of the batch)
            wide = 1.0
            np.testing.assert_allclose(m.numpy(), ref_m.numpy(), rtol=1e-5, atol=wide * 1e-4 * float(ref_m.abs().max()),
                                       err_msg=f"step {step} exp_avg/{k}")
            np.testing.assert_allclose(v.numpy(), ref_v.numpy(), rtol=1e-5, atol=wide * 2e-4 * float(ref_v.abs().max()),
                                       err_msg=f"step {step} exp_avg_sq/{k}")
            # the parameter itself: tight where |m_hat| / (sqrt(v_hat) + eps) is insensitive to 1e-4 relative changes of m
            # and v, i.e. where sqrt(v_hat) >> eps; elsewhere one step can differ by up to lr
            delta = (got[k] - leaf.detach()).abs()
            vhat = ref_v / (1 - 0.999 ** (step + 1))
            ok = vhat.sqrt() > 1e-4 * max(float(vhat.sqrt().max()), 1e-30)
            if bool(ok.any()):
                bound = 2e-2 * lr
                assert float(delta[ok].max()) <= bound, (step, k, float(delta[ok].max()))
            assert float(delta.max()) <= 2.0 * lr + 1e-6, (step, k)


@pytest.mark.parametrize("opt", ["adam", "adagrad", "rmsprop", "sgd"])
def test_optimizer_state_survives_a_device_move_and_a_resume(opt):
    """`.to()` in the middle of training keeps the optimizer state (torch's optimizer state follows its parameters), and
    optimizer_state_dict()/load_optimizer_state_dict() resume a run: both continue bit for bit like an uninterrupted run.
    Adam's moments, Adagrad's `sum` and RMSprop's `square_avg` alike (the accumulators of the non-Adam
    optimizers used to be dropped)."""
    c = Case("small_qkv")
    X, y = c.X.to(DEV), c.y.to(DEV)

    def fresh():
        m = build_model(c, DEV)
        m.compile(torch.optim.Adam(m.parameters(), lr=c.meta["lr"]) if opt == "adam" else opt, "binary_crossentropy")
        m.train()
        return m

    ref = fresh()
    for _ in range(4):
        ref._require_engine().train_step(X, y)
    want = sd_to_cpu(ref)

    moved = fresh()
    for _ in range(2):
        moved._require_engine().train_step(X, y)
    moved.to(DEV)                                   # rebuilds the arena and the engine
    assert moved._engine is None
    for _ in range(2):
        moved._require_engine().train_step(X, y)
    got = sd_to_cpu(moved)
    for k in want:
        assert torch.equal(got[k], want[k]), k

    first = fresh()
    for _ in range(2):
        first._require_engine().train_step(X, y)
    params, opt_sd = sd_to_cpu(first), first.optimizer_state_dict()
    assert opt_sd["kind"] == opt and opt_sd["step"] == 2
    key = {"adam": "exp_avg_sq", "adagrad": "sum", "rmsprop": "square_avg", "sgd": None}[opt]
    if key is not None:                         # the accumulators are really there (not a zero-filled stand-in)
        assert float(opt_sd["state"]["dnn_linear.weight"][key].abs().max()) > 0
        assert any(float(v[key].abs().max()) > 0 for k, v in opt_sd["state"].items() if k.startswith("embedding_dict."))
    resumed = fresh()
    resumed.load_state_dict(params)
    resumed.load_optimizer_state_dict(opt_sd)
    for _ in range(2):
        resumed._require_engine().train_step(X, y)
    got = sd_to_cpu(resumed)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_learning_rate_changes_take_effect():
    """param_groups edits (what an LR scheduler does) are read at every step; postponed lazy steps use the old value."""
    c = Case("small_qkv")
    X, y = c.X.to(DEV), c.y.to(DEV)
    m = build_model(c, DEV)
    opt = torch.optim.Adam(m.parameters(), lr=c.meta["lr"])
    m.compile(opt, "binary_crossentropy")
    m.eval()
    eng = m._require_engine()
    eng.train_step(X, y)
    opt.param_groups[0]["lr"] = 0.0                 # from now on nothing may move
    before = sd_to_cpu(m)
    eng.train_step(X, y)
    after = sd_to_cpu(m)
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_lr_schedule_needs_no_flush_and_stays_bitwise(monkeypatch):
    """An LR scheduler changes the rate before every step.  The lazy form must not flush for that (the replay of a postponed
    step reads the rate that step was taken with from the per-step table), and must leave exactly the tables and moments of
    the every-step streaming form under the same schedule - rows that wait several steps for their next gather included."""
    c = Case("aliccp_sota")
    rng = np.random.RandomState(5)
    B, steps = 16, 9
    Xs = [np.stack([rng.randint(1 if f == "301" else 0, v - 1, size=B) for f, v in zip(c.meta["fields"], c.meta["vocab"])],
                   axis=1).astype(np.float32) for _ in range(steps)]
    ys = [(rng.rand(B) < 0.3).astype(np.float32) for _ in range(steps)]
    results = {}
    for lazy in ("1", "0"):
        monkeypatch.setenv("SATRANS_LAZY_ADAM", lazy)
        monkeypatch.setenv("SATRANS_LAZY_FLUSH_EVERY", "0")
        m = build_model(c, DEV)
        opt = torch.optim.Adam(m.parameters(), lr=c.meta["lr"])
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 / (1.0 + 0.37 * e))
        m.compile(opt, "binary_crossentropy")
        m.train()
        eng = m._require_engine()
        flushes = getattr(eng, "flush_count", 0)
        for i in range(steps):
            eng.train_step(torch.from_numpy(Xs[i]).to(DEV), torch.from_numpy(ys[i]).to(DEV))
            import warnings
            with warnings.catch_warnings():       # (torch warns that optimizer.step() was not called: the step runs as HIP kernels)
                warnings.simplefilter("ignore")
                sched.step()                      # a new rate for the next step
        if lazy == "1":
            assert getattr(eng, "flush_count", 0) == flushes, "a learning-rate change must not flush the postponed steps"
            assert len(eng._lr_hist) == steps                  # one entry per rate change while the steps are postponed ...
        res = sd_to_cpu(m)
        if lazy == "1":
            assert len(eng._lr_hist) == 1, "... and only the rate in force once a flush (state_dict) made every row current"
        for k, st_ in m.optimizer_state_dict()["state"].items():
            res["exp_avg/" + k], res["exp_avg_sq/" + k] = st_["exp_avg"], st_["exp_avg_sq"]
        results[lazy] = res
    for k, v in results["1"].items():
        same = (v.view(torch.int32) == results["0"][k].view(torch.int32)) if v.dtype == torch.float32 else (v == results["0"][k])
        assert bool(same.all()), f"lazy and streaming forms differ under an LR schedule at {k}"


def _adam_reference(p, g, lr, steps_done, m, v):
    """torch.optim.Adam on CPU for one more step with explicit state (the reference's optimizer, main.py:343)."""
    p = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([p], lr=lr)
    opt.state[p] = dict(step=torch.tensor(float(steps_done)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    p.grad = g.clone()
    opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_optimizer_kernels_exact(arith):
    """Optimizer kernels in isolation, on gradients that are exact in any summation order (small integers times
    a power of two): flat Adam, touched-row Adam with heavy duplication across chunk boundaries, and the
    streaming Adam of untouched rows must reproduce torch.optim.Adam + L2 to the last few ulps - in the exact arithmetic and,
    inside the same bounds (its own is 3.2e-7 of the update), in the fast one; whichever path a row takes, the bits agree."""
    import ctypes as C
    import math
    from satrans_amd import native as N
    lib = N.lib()
    g = torch.Generator().manual_seed(5)
    st = torch.cuda.current_stream().cuda_stream
    lr, b1, b2, eps, l2, t = 0.005, 0.9, 0.999, 1e-8, 1e-5, 4

    def hp(l2v):
        h = N.AdamHParams()
        h.lr_over_bc1, h.bc2_sqrt = lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t)
        h.beta1, h.beta2, h.eps, h.l2 = b1, b2, eps, l2v
        h.arith = N.ADAM_FAST if arith == "fast" else N.ADAM_EXACT
        return h

    # ---- flat ----
    n = 10007
    p = torch.randn(n, generator=g) * 0.05
    gr = torch.randn(n, generator=g) * 1e-3
    m = torch.randn(n, generator=g) * 1e-3
    v = torch.rand(n, generator=g) * 1e-6
    pd, gd, md, vd = (x.to(DEV) for x in (p, gr, m, v))
    N.check(lib.satrans_adam_flat(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, C.byref(hp(0.0)), st), "flat")
    pr, mr, vr = _adam_reference(p, gr, lr, t - 1, m, v)
    # one ulp of the tensor scale: hipcc contracts m + w*(g-m) into an fma, torch's CPU lerp may not
    np.testing.assert_allclose(md.cpu().numpy(), mr.numpy(), rtol=3e-7, atol=2e-7 * float(mr.abs().max()))
    np.testing.assert_allclose(vd.cpu().numpy(), vr.numpy(), rtol=3e-7, atol=2e-7 * float(vr.abs().max()))
    np.testing.assert_allclose((pd.cpu() - p).numpy(), (pr - p).numpy(), rtol=2e-5, atol=1e-6 * lr)

    # ---- tables: 3000 rows, D = 32; row 5 gathered 4000 times (spans > 100 chunks), others a few times ----
    R, D = 3000, 32
    P = torch.randn(R, D, generator=g) * 1e-2
    M = torch.randn(R, D, generator=g) * 1e-4
    V = torch.rand(R, D, generator=g) * 1e-8
    rows = torch.cat([torch.full((4000,), 5), torch.randint(0, 1500, (6000,), generator=g),
                      torch.full((33,), 2999), torch.full((64,), 7)]).to(torch.int32)
    rows = rows[torch.randperm(rows.numel(), generator=g)]
    nrow = rows.numel()
    gemb = torch.randint(-8, 9, (nrow, D), generator=g).float() * 2.0 ** -20     # exact sums in any order
    dense_g = torch.zeros(R, D).index_add_(0, rows.long(), gemb) + (2 * l2) * P
    Pr, Mr, Vr = _adam_reference(P, dense_g, lr, t - 1, M, V)
    Pd, Md, Vd, rows_d, gemb_d = (x.to(DEV) for x in (P, M, V, rows, gemb))
    sorted_rows = torch.empty(nrow, dtype=torch.int32, device=DEV)
    src = torch.empty(nrow, dtype=torch.int32, device=DEV)
    touched = torch.empty((R + 31) // 32, dtype=torch.int32, device=DEV)
    sort_ws = torch.empty(int(lib.satrans_embed_sort_workspace_bytes(nrow, R)), dtype=torch.uint8, device=DEV)
    part = torch.empty(int(lib.satrans_embed_partial_ws_floats(nrow, D)), device=DEV)
    regp = torch.zeros(int(lib.satrans_embed_reg_partials(R, nrow, D)), dtype=torch.float64, device=DEV)
    N.check(lib.satrans_embed_sort(rows_d.data_ptr(), nrow, R, sorted_rows.data_ptr(), src.data_ptr(), touched.data_ptr(),
                                   sort_ws.data_ptr(), sort_ws.numel(), None, st), "sort")
    s2, c2 = torch.empty_like(sorted_rows), torch.empty_like(src)
    iota = torch.arange(nrow, dtype=torch.int32, device=DEV)
    N.check(lib.satrans_embed_sort(rows_d.data_ptr(), nrow, R, s2.data_ptr(), c2.data_ptr(), None, sort_ws.data_ptr(),
                                   sort_ws.numel(), iota.data_ptr(), st), "sort(positions given)")
    assert torch.equal(s2, sorted_rows) and torch.equal(c2, src)
    sr, sc = sorted_rows.cpu(), src.cpu().long()
    assert torch.equal(sr, torch.sort(rows, stable=True).values)
    assert torch.equal(rows[sc], sr) and bool((sc[1:][sr[1:] == sr[:-1]] > sc[:-1][sr[1:] == sr[:-1]]).all()), "stable"
    N.check(lib.satrans_embed_adam_touched(Pd.data_ptr(), Md.data_ptr(), Vd.data_ptr(), D, sorted_rows.data_ptr(),
                                           src.data_ptr(), nrow, gemb_d.data_ptr(), part.data_ptr(), C.byref(hp(l2)),
                                           regp.data_ptr(), None, 0, st), "touched")
    N.check(lib.satrans_embed_adam_untouched(Pd.data_ptr(), Md.data_ptr(), Vd.data_ptr(), 0, R, D, touched.data_ptr(),
                                             C.byref(hp(l2)), regp.data_ptr(), 0, st), "untouched")
    np.testing.assert_allclose(Md.cpu().numpy(), Mr.numpy(), rtol=1e-6, atol=2e-7 * float(Mr.abs().max()))
    np.testing.assert_allclose(Vd.cpu().numpy(), Vr.numpy(), rtol=1e-6, atol=2e-7 * float(Vr.abs().max()))
    # inputs are identical and exactly summed, so the only slack is ~1 ulp in m, v amplified by lr/(sqrt(v)+eps)
    np.testing.assert_allclose((Pd.cpu() - P).numpy(), (Pr - P).numpy(), rtol=2e-5, atol=1e-6 * lr)
    reg = torch.zeros(1, dtype=torch.float64, device=DEV)
    N.check(lib.satrans_sum_f64(regp.data_ptr(), regp.numel(), reg.data_ptr(), 0, st), "sum")
    # the reference multiplies fp32 tensors by the python float l2, i.e. by float32(l2)
    assert float(reg.item()) == pytest.approx(float(np.float32(l2)) * float((P.double() ** 2).sum()), rel=1e-12)

    # ---- the same step in the form the engine uses: rows < RS are "small tables" (ordered sums stored into a dense
    # gradient, dense step over ALL of them), the others go through the sorted list, whose gradient rows are first packed
    # in sorted order (what a rank contributes to the all-gather); untouched rows from RS on ----
    RS = 64
    n_s = int((sr < RS).sum())
    Pd2, Md2, Vd2 = (x.to(DEV) for x in (P, M, V))
    last = torch.zeros(R, dtype=torch.int32, device=DEV)
    G = torch.zeros(RS, D, device=DEV)
    regu = torch.zeros_like(regp)
    N.check(lib.satrans_embed_segment_sums(sorted_rows.data_ptr(), src.data_ptr(), n_s, gemb_d.data_ptr(), D, part.data_ptr(),
                                           regu.data_ptr(), G.data_ptr(), st), "segment_sums")
    assert torch.equal(G.cpu(), torch.zeros(R, D).index_add_(0, rows.long(), gemb)[:RS]), "dense gradient of the small rows"
    regr = torch.zeros(int(lib.satrans_embed_adam_rows_partials(RS, D)), dtype=torch.float64, device=DEV)
    N.check(lib.satrans_embed_adam_rows(Pd2.data_ptr(), Md2.data_ptr(), Vd2.data_ptr(), last.data_ptr(), 0, RS, D, G.data_ptr(),
                                        C.byref(hp(l2)), t, regr.data_ptr(), st), "adam_rows")
    n_b = nrow - n_s
    packed = torch.empty(n_b, D, device=DEV)
    N.check(lib.satrans_embed_pack_rows(src[n_s:].data_ptr(), n_b, gemb_d.data_ptr(), D, packed.data_ptr(), st), "pack")
    assert torch.equal(packed.cpu(), gemb[sc[n_s:]])
    ident = torch.arange(n_b, dtype=torch.int32, device=DEV)
    regp2 = torch.zeros_like(regp)
    N.check(lib.satrans_embed_adam_touched(Pd2.data_ptr(), Md2.data_ptr(), Vd2.data_ptr(), D, sorted_rows[n_s:].data_ptr(),
                                           ident.data_ptr(), n_b, packed.data_ptr(), part.data_ptr(), C.byref(hp(l2)),
                                           regp2.data_ptr(), last.data_ptr(), t, st), "touched(big)")
    N.check(lib.satrans_embed_mark_touched(sorted_rows[n_s:].data_ptr(), n_b, R, touched.data_ptr(), st), "mark")
    N.check(lib.satrans_embed_adam_untouched(Pd2.data_ptr(), Md2.data_ptr(), Vd2.data_ptr(), RS, R, D, touched.data_ptr(),
                                             C.byref(hp(l2)), regp2.data_ptr(), 0, st), "untouched(big)")
    # exact gradient sums => bit-identical tables, whichever path a row took
    assert torch.equal(Pd2, Pd) and torch.equal(Md2, Md) and torch.equal(Vd2, Vd)
    stepped = torch.zeros(R, dtype=torch.bool)
    stepped[sr[n_s:].long()] = True
    stepped[:RS] = True
    assert torch.equal(last.cpu() == t, stepped), "last[row] = t exactly for the rows that took their step"
    reg2 = torch.zeros(1, dtype=torch.float64, device=DEV)
    N.check(lib.satrans_sum_f64(regp2.data_ptr(), regp2.numel(), reg2.data_ptr(), 0, st), "sum")
    N.check(lib.satrans_sum_f64(regr.data_ptr(), regr.numel(), reg2.data_ptr(), 1, st), "sum")
    assert float(reg2.item()) == pytest.approx(float(reg.item()), rel=1e-12)


@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos"])
def test_fit_and_predict_match_reference_golden(name):
    c = Case(name)
    z = c.z
    model = build_model(c, DEV)
    model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy",
                  metrics=["binary_crossentropy", "auc"])
    model._require_engine().drop_p = 0.0           # the golden fit ran with every dropout p = 0
    feed = {n: z[f"fit/x/{n}"] for n in c.meta["feature_names"]}
    B = int(z["fit/batch_size"])
    hist = model.fit(x=dict(feed), y=z["fit/y"], batch_size=B, epochs=2, verbose=0, shuffle=False)
    np.testing.assert_allclose(hist.history["loss"], z["fit/loss"], rtol=2e-5)
    pred = model.predict(dict(feed), batch_size=2 * B)
    assert pred.dtype == np.float64 and pred.shape == z["fit/pred"].shape
    # 8 Adam steps on eps-scale gradients (see test_adam_steps_match_reference_golden) separate two correct fp32
    # runs by ~1e-4 in probability; the loss history above is the tight check
    np.testing.assert_allclose(pred, z["fit/pred"], rtol=0, atol=5e-4)


def test_training_mode_dropout_matches_oracle_with_same_masks():
    """Train-mode forward: the kernels' counter-based masks, replayed through the CPU oracle."""
    c = Case("aliccp_sota")
    model = build_model(c, DEV)
    model.train()
    prob = model(c.X.to(DEV))
    eng = model._engine
    m = c.meta
    masks = O.dropout_masks(eng.drop_seed, eng.drop_step, c.X.shape[0], len(m["fields"]), m["D"], m["H"], m["L"], 0.1)
    p_ref, logit_ref = O.forward(c.tensors("param"), c.X, c.spec(), O.Dropper("masks", 0.1, masks))
    np.testing.assert_allclose(eng.last_logit().cpu().numpy(), logit_ref.numpy(), rtol=0, atol=LOGIT_ATOL)
    # and dropout really is on: the eval logits differ
    model.eval()
    model(c.X.to(DEV))
    assert float((eng.last_logit().cpu() - logit_ref).abs().max()) > 1e-4


@pytest.mark.parametrize("name", ["small_qkv", "aliccp_sota"])
def test_training_mode_gradients_match_oracle_with_same_masks(name):
    """Training-mode step (four dropout sites per layer on) against the oracle with the kernels' masks replayed.  `small_qkv` is
    D = 16; `aliccp_sota` is the headline shape (D = 32, U = 64, H = 4, F = 19, meta_mode QK): the fused backward instantiation
    of the benchmark."""
    c = Case(name)
    model = build_model(c, DEV)
    model.compile("adam", "binary_crossentropy")
    model.train()
    eng = model._require_engine()
    bce, reg, grads = eng.loss_and_grads(c.X.to(DEV), c.y.to(DEV))
    m = c.meta
    masks = O.dropout_masks(eng.drop_seed, eng.drop_step, c.X.shape[0], len(m["fields"]), m["D"], m["H"], m["L"], 0.1)
    (bce_ref, reg_ref, g_ref), kinks = oracle_grads_probing_kinks(c.tensors("param"), c.X, c.y, c.spec(), O.Dropper("masks", 0.1, masks))
    assert bce == pytest.approx(bce_ref, rel=2e-6)
    assert set(grads) <= set(g_ref)
    for k, g in g_ref.items():
        if k not in grads:                           # alias keys of the oracle (K_/V_meta_mlp, domain_map_dnn_K/V)
            continue
        scale = max(1e-6, float(g.abs().max()))
        floor = 1e-9
        assert_grad_close_but_for_kinks(grads[k].cpu().numpy(), g.numpy(), 5e-5 * scale + floor, k, kinks=kinks)


@pytest.mark.parametrize("loss", ["binary_crossentropy", "mse", "mae"])
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos", "small_qkv", "small_pos_dense", "small_relu", "small_k", "small_gate",
                                  "small_bilinear"])
def test_fused_last_layer_and_head_equal_the_separate_calls(name, train, loss):
    """satrans_layer_bwd_head (last layer forward + head + loss + backward in one launch; the default of a training step) against
    satrans_layer_fwd + satrans_head_loss + satrans_layer_bwd on the same batch, weights and dropout counters: probabilities,
    loss and every gradient.  The two differ only in the order the logit's F x D terms are added (token dots summed per sample
    against a lane-strided sum), i.e. by fp32 rounding of the logit.  Covers dense columns (Alimama), D = 16, separate Q / K
    tables ('pos'), ReLU output, one modulated role, flags gate / bilinear, and the three losses of compile()."""
    c = Case(name)
    out = []
    for fuse in (True, False):
        model = build_model(c, DEV)
        model.compile("adam", loss)
        model.train(train)
        eng = model._require_engine()
        eng.fuse_head = fuse
        X, y = c.X.to(DEV), c.y.to(DEV)
        bce, reg, grads = eng.loss_and_grads(X, y)
        assert bool(eng._ws[X.shape[0]]["fuse_head"]) == fuse, "the fused last-layer step was expected to take every one of these cases"
        out.append((bce, eng.last_prob().clone().cpu(), {k: g.cpu() for k, g in grads.items()}))
    (b1, p1, g1), (b0, p0, g0) = out
    assert b1 == pytest.approx(b0, rel=2e-6)
    np.testing.assert_allclose(p1.numpy(), p0.numpy(), rtol=0, atol=3e-7)
    for k in g0:
        sc = max(1e-6, float(g0[k].abs().max()))
        # MAE: d|p - t| / dp = sign(p - t) is discontinuous where p == t; no golden label sits there
        np.testing.assert_allclose(g1[k].numpy(), g0[k].numpy(), rtol=0, atol=2e-5 * sc + 1e-9, err_msg=k)


def test_kernel_timing_brackets_every_fused_launch_and_changes_no_bit():
    """satrans_kernel_timing (bench.py's `roofline.launch_ms`): while armed, the fused layer kernels are launched with events that
    the dispatch itself signals; a training-mode loss_and_grads of a three-layer model reports two forwards, the fused last layer and
    two backwards, in launch order, with plausible durations - and the gradients are the bits of the unarmed run."""
    import ctypes as C
    from satrans_amd import native as N
    lib = N.lib()
    c = Case("aliccp_sota")
    X, y = c.X.to(DEV), c.y.to(DEV)
    outs = []
    for armed in (0, 1):
        model = build_model(c, DEV)
        model.compile("adam", "binary_crossentropy")
        model.train()
        eng = model._require_engine()
        assert lib.satrans_kernel_timing_read(None, None, 0) >= 0          # (forget whatever an earlier test left)
        assert lib.satrans_kernel_timing(armed) == 0
        try:
            bce, reg, grads = eng.loss_and_grads(X, y)
        finally:
            assert lib.satrans_kernel_timing(0) == armed
        kinds, ms = (C.c_int * 64)(), (C.c_float * 64)()
        n = lib.satrans_kernel_timing_read(kinds, ms, 64)
        if armed:
            fused = bool(eng._ws[X.shape[0]]["fuse_head"])          # (fuse_head off: three forwards, three plain backwards)
            assert [kinds[i] for i in range(n)] == ([0, 0, 2, 1, 1] if fused else [0, 0, 0, 1, 1, 1]), [kinds[i] for i in range(n)]
            assert all(0.0 < ms[i] < 50.0 for i in range(n)), [ms[i] for i in range(n)]
            assert lib.satrans_kernel_timing_read(kinds, ms, 64) == 0      # read forgets
        else:
            assert n == 0
        outs.append((bce, {k: g.cpu() for k, g in grads.items()}))
    assert outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize("S,B", [(1, 1), (3, 5), (4, 1000), (4, 8192), (16, 8192), (16, 65536), (17, 300), (4, 70000), (4096, 5000),
                                 (4, 32768), (3, 16000), (8, 40000), (7, 65536)])
def test_scenario_bucketing_is_a_stable_sort(S, B):
    """satrans_bucket_scenarios - one counting-sort launch for S <= 16 scenario rows (two launches of one workgroup per 1,024 samples
    from 16 rounds on, S <= 8: the prediction batch), the rocPRIM radix sort beyond - against a stable argsort: `order` groups the sample indices by scenario in their original order, seg[s] is where scenario s starts."""
    from satrans_amd import native as N
    lib = N.lib()
    rng = np.random.RandomState(S + B)
    ids = rng.randint(0, S, size=B)
    if S > 2:
        ids[ids == 1] = 2                                   # an empty scenario row
    X = torch.from_numpy(np.stack([rng.rand(B), ids.astype(np.float64)], axis=1).astype(np.float32)).to(DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    sid, order, seg, status = torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(S + 1, **i32), torch.zeros(1, **i32)
    wsb = torch.empty(int(lib.satrans_bucket_workspace_bytes(B, S)), dtype=torch.uint8, device=DEV)
    N.check(lib.satrans_bucket_scenarios(X.data_ptr(), N.ID_F32, X.stride(0), 1, B, S, sid.data_ptr(), order.data_ptr(),
                                         seg.data_ptr(), status.data_ptr(), wsb.data_ptr(), wsb.numel(),
                                         torch.cuda.current_stream().cuda_stream), "satrans_bucket_scenarios")
    want = np.argsort(ids, kind="stable")
    assert np.array_equal(sid.cpu().numpy(), ids)
    assert np.array_equal(order.cpu().numpy(), want)
    assert np.array_equal(seg.cpu().numpy(), np.searchsorted(ids[want], np.arange(S + 1)))
    assert int(status.item()) == 0
    X[B // 2, 1] = S                                        # an id outside the table: flagged, counted as row 0
    N.check(lib.satrans_bucket_scenarios(X.data_ptr(), N.ID_F32, X.stride(0), 1, B, S, sid.data_ptr(), order.data_ptr(),
                                         seg.data_ptr(), status.data_ptr(), wsb.data_ptr(), wsb.numel(),
                                         torch.cuda.current_stream().cuda_stream), "satrans_bucket_scenarios")
    assert int(status.item()) == 1 and int(sid[B // 2].item()) == 0
    assert sorted(order.cpu().tolist()) == list(range(B))


def test_next_batch_hint_changes_no_bit():
    """train_step(X, y, next_X=...) runs the next batch's ids -> rows, per-field sort and scenario bucketing on a side stream under
    the current step's tail, and the step's reduction + scenario-table backward run on a stream of their own beside the touched-row
    kernels.  Tables, moments and the logged sums after six steps are the same bits with everything in line on the launch stream,
    with the side streams, with the hint, without it, and with a hint that names the wrong batch (prepared work discarded)."""
    c = Case("aliccp_sota")
    rng = np.random.RandomState(4)
    n = c.X.shape[0]
    Xs = [c.X[rng.permutation(n)].to(DEV) for _ in range(6)]
    ys = [c.y[rng.permutation(n)].to(DEV) for _ in range(6)]

    def run(hint, side_tail=True, early=True):
        model = build_model(c, DEV)
        model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
        model.train()
        eng = model._require_engine()
        eng.side_tail = side_tail          # reduction + scenario-table backward on their own stream beside the touched-row kernels
        eng.prep_early = early             # the next batch forked in front of the last backward kernel (low-priority stream) / behind it
        eng.reset_epoch_sums()
        for i in range(6):
            nxt = None
            if hint == "right" and i + 1 < 6:
                nxt = Xs[i + 1]
            elif hint == "wrong":
                nxt = Xs[(i + 3) % 6]
            eng.train_step(Xs[i], ys[i], next_X=nxt)
        sums = eng.epoch_sums()
        return sd_to_cpu(model), model.optimizer_state_dict(), sums
    ref_sd, ref_opt, ref_sums = run(None, side_tail=False)      # everything in line on the launch stream
    for hint in ("right", "wrong", None, "late fork"):
        sd, opt, sums = run(hint) if hint != "late fork" else run("right", early=False)
        assert sums == ref_sums, hint
        for k in ref_sd:
            assert torch.equal(sd[k], ref_sd[k]), (hint, k)
        for k, st in ref_opt["state"].items():
            for kind in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt["state"][k][kind], st[kind]), (hint, k, kind)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos", "small_qkv", "small_gate", "small_bilinear"])
def test_one_reduction_launch_for_all_layers_is_bitwise_the_per_layer_reductions(name, train):
    """satrans_layer_bwd_launch x L + satrans_layer_bwd_reduce (one launch for all layers' slabs and the fused head's rows; the
    default) against satrans_layer_bwd per layer: the same arithmetic in the same order - the layers' generated-weight records,
    which without 'pos' all go to ONE table, are added layer after layer inside a block - so every gradient is the same bits."""
    c = Case(name)
    X, y = c.X.to(DEV), c.y.to(DEV)
    outs = []
    for defer in (True, False):
        model = build_model(c, DEV)
        model.compile("adam", "binary_crossentropy")
        model.train(train)
        eng = model._require_engine()
        eng.defer_reduce = defer
        bce, reg, grads = eng.loss_and_grads(X, y)
        assert bool(eng._ws[X.shape[0]]["defer"]) == defer
        outs.append((bce, {k: g.cpu() for k, g in grads.items()}))
    assert outs[0][0] == outs[1][0]
    for k in outs[1][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k

def test_gather_bit_exact_and_out_of_range_ids():
    c = Case("aliccp_sota")
    model = build_model(c, DEV)
    model.eval()
    rng = np.random.RandomState(3)
    B = 4099                                         # ragged: not a multiple of any tile
    X = np.stack([rng.randint(1 if f == "301" else 0, v - 1, size=B) for f, v in zip(c.meta["fields"], c.meta["vocab"])],
                 axis=1).astype(np.float32)
    model(torch.from_numpy(X).to(DEV))
    got = model._engine.layer_outputs(B)[0].cpu()
    want = O.gather_fields(sd_to_cpu(model), torch.from_numpy(X), c.spec())
    assert torch.equal(got, want)
    X[7, 3] = c.meta["vocab"][3]                     # one id past the end of its table
    with pytest.raises(IndexError):
        model(torch.from_numpy(X).to(DEV))
    model(torch.from_numpy(X[:7]).to(DEV))           # the error state does not stick


def test_single_sample_and_empty_scenarios():
    """B = 1, and batches in which some scenario rows are never seen."""
    c = Case("aliccp_sota")
    model = build_model(c, DEV)
    model.eval()
    X = c.X.clone()
    X[:, c.meta["feature_names"].index("301")] = 2.0
    for xb in (X[:1], X[:5], X):
        p = model(xb.to(DEV)).cpu()
        p_ref, _ = O.forward(c.tensors("param"), xb, c.spec())
        np.testing.assert_allclose(p.numpy(), p_ref.numpy(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("name", ["aliccp_sota", "small_pos_dense", "small_d64"])
def test_other_layer_implementations_match_golden_too(name, impl):
    """The LDS-resident layer kernels - scalar-FMA arm (1: fallback for any shape, the ablation arm) and MFMA arm (2) -
    against the same golden vectors; everything else in this file runs the automatic choice (fused kernels)."""
    from satrans_amd import native as N
    c = Case(name)
    N.check(N.lib().satrans_set_layer_impl(impl), "set_layer_impl")
    try:
        model = build_model(c, DEV)
        model.compile("adam", "binary_crossentropy")
        model.eval()
        model(c.X.to(DEV))
        eng = model._engine
        np.testing.assert_allclose(eng.last_logit().cpu().numpy(), c.arrays("out")["logit"], rtol=0, atol=LOGIT_ATOL)
        bce, reg, grads = eng.loss_and_grads(c.X.to(DEV), c.y.to(DEV))
        for k, g in c.arrays("grad").items():
            scale = max(1e-6, float(np.abs(g).max()))
            np.testing.assert_allclose(grads[k].cpu().numpy(), g, rtol=0, atol=5e-5 * scale + 1e-9, err_msg=k)
    finally:
        N.check(N.lib().satrans_set_layer_impl(0), "set_layer_impl")


@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos"])
def test_bf16_forward_stays_within_bf16_rounding_of_the_reference(name):
    """BASELINE.json configs[1] "bf16 forward, fp32 ref-parity check": evaluation forward with the dense products on the bf16
    matrix pipe (fp32 accumulation, fp32 LayerNorm / softmax) against the reference's fp32 golden logits.  Stated tolerance:
    5e-2 abs on logits (SURVEY.md §6 measured 8.1e-3 for an all-bf16 forward near init); the gather stays bit-exact and
    switching back restores the fp32 result bit for bit."""
    c = Case(name)
    model = build_model(c, DEV)
    model.eval()
    X = c.X.to(DEV)
    p32 = model(X).clone()
    l32 = model._engine.last_logit().clone()
    model.set_forward_precision("bf16")
    pb = model(X)
    lb = model._engine.last_logit()
    want = c.arrays("out")
    err = float(np.abs(lb.cpu().numpy() - want["logit"]).max())
    assert err < 5e-2, err
    assert err > 0.0 or float((lb - l32).abs().max()) > 0.0, "the bf16 path did not run"
    assert float((lb - l32).abs().max()) > 0.0, "bf16 and fp32 logits are identical: the bf16 kernel was not used"
    np.testing.assert_allclose(pb.cpu().numpy(), want["prob"], rtol=0, atol=1.5e-2)
    assert np.array_equal(model._engine.layer_outputs(X.shape[0])[0].cpu().numpy(), want["att_input"])
    pred = model.predict({n: c.z[f"fit/x/{n}"] for n in c.meta["feature_names"]}, batch_size=64)
    assert pred.dtype == np.float64 and pred.shape == (c.z["fit/y"].shape[0], 1)
    model.set_forward_precision("fp32")
    assert torch.equal(model(X), p32)
    print(f"[bf16] {name}: logit max-abs-err vs reference {err:.3e}, vs fp32 kernels {float((lb - l32).abs().max()):.3e}")


@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos"])
def test_bf16_stack_launch_is_the_layer_launches_bit_for_bit(name):
    """The bf16 evaluation forward runs the whole stack of layers as ONE launch (satrans_stack_fwd_bf16: a tile's rows stay in LDS
    between the layers).  Per layer it is the code of satrans_layer_fwd_bf16: logits and probabilities must be the bits of the
    layer-by-layer launches, on the golden batch, on a ragged one and on a batch larger than a workgroup's tile count."""
    c = Case(name)
    model = build_model(c, DEV)
    model.eval()
    model.set_forward_precision("bf16")
    eng = model._require_engine()
    rng = np.random.RandomState(3)
    big = torch.from_numpy(np.concatenate([c.X.numpy()[rng.randint(0, c.X.shape[0], size=3000)]], axis=0))
    for X in (c.X, c.X[:37], big):
        X = X.to(DEV)
        outs = {}
        for stack in (True, False):
            eng.bf16_stack = stack
            p = model(X).clone()
            outs[stack] = (p, eng.last_logit().clone())
        assert torch.equal(outs[True][1], outs[False][1]) and torch.equal(outs[True][0], outs[False][0]), X.shape
    # layer_outputs() behind a stacked forward hands out every layer's output (the layers run once more, one launch each)
    eng.bf16_stack = False
    model(c.X.to(DEV))
    want = eng.layer_outputs(c.X.shape[0])
    eng.bf16_stack = True
    model(c.X.to(DEV))
    got = eng.layer_outputs(c.X.shape[0])
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    model.set_forward_precision("fp32")


@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos"])
def test_streamed_input_pipeline_equals_the_resident_dataset(name, tmp_path):
    """fit / predict with the dataset kept on the host and streamed in double-buffered pinned batches (satrans_amd/pipeline.py;
    here from memory-mapped .npy columns, the loader for datasets that should not sit in HBM) against the resident-dataset
    path: same History, same predictions, same parameters, bit for bit - and both on the reference's golden History."""
    from satrans_amd.pipeline import load_npy_columns
    c = Case(name)
    names = c.meta["feature_names"]
    x = {n: c.z[f"fit/x/{n}"] for n in names}
    y, B = c.z["fit/y"], int(c.z["fit/batch_size"])
    for n in names:
        np.save(tmp_path / f"{n}.npy", x[n])
    x_mm = load_npy_columns(str(tmp_path), names)
    assert all(isinstance(v, np.memmap) for v in x_mm.values())
    res = {}
    for stream in (False, True):
        model = build_model(c, DEV)
        for mod in model.modules():
            pass
        model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy",
                      metrics=["binary_crossentropy", "auc"])
        model.stream_input = stream
        model._require_engine().drop_p = 0.0                    # the reference's fit was recorded with every dropout p = 0
        hist = model.fit(x=dict(x_mm if stream else x), y=y, batch_size=B, epochs=2, verbose=0, shuffle=False)
        pred = model.predict(dict(x_mm if stream else x), batch_size=2 * B)
        res[stream] = (hist.history["loss"], pred, sd_to_cpu(model))
    assert res[True][0] == res[False][0]
    assert np.array_equal(res[True][1], res[False][1])
    for k in res[True][2]:
        assert torch.equal(res[True][2][k], res[False][2][k]), k
    np.testing.assert_allclose(res[True][0], c.z["fit/loss"], rtol=2e-5)
    # shuffled epochs draw the same permutation either way
    out = []
    for stream in (False, True):
        model = build_model(c, DEV)
        model.compile("adam", "binary_crossentropy")
        model.stream_input = stream
        torch.manual_seed(5)
        out.append(model.fit(x=dict(x), y=y, batch_size=B, epochs=1, verbose=0, shuffle=True).history["loss"])
    assert out[0] == out[1]


def test_integer_ids_with_dense_features_travel_as_a_packed_input():
    """A vocabulary of 2**24 rows and more next to a DenseFeat: ids as int64, dense features as their own float block
    (inputs.PackedInput) - resident and streamed - must gather exactly the rows the ids name and use the dense values."""
    from satrans_amd import DenseFeat, SATrans, SparseFeat
    big = (1 << 24) + 1000
    cols = [SparseFeat("a", big, 16), SparseFeat("b", 50, 16), SparseFeat("dom", 4, 16), DenseFeat("price", 1)]
    model = SATrans(cols, cols, ["dom"], [3], att_layer_num=0, domain_att_layer_num=1, att_head_num=2, use_linear=False,
                    use_dnn=False, meta_mode="QK", meta_dnn_hidden_units=(32, 16), seed=3, device=DEV, flag="sota")
    rng = np.random.RandomState(0)
    N = 300
    x = {"a": np.concatenate([[big - 1, (1 << 24) + 1, (1 << 24) + 3], rng.randint(0, big, size=N - 3)]).astype(np.int64),
         "b": rng.randint(0, 50, size=N).astype(np.int64), "dom": rng.randint(1, 4, size=N).astype(np.int64),
         "price": rng.rand(N).astype(np.float32)}
    with torch.no_grad():
        model.dnn_linear.weight[0, -1] = 3.0                    # make the dense feature matter
    preds = {}
    for stream in (False, True):
        model.stream_input = stream
        preds[stream] = model.predict(dict(x), batch_size=128)
    assert np.array_equal(preds[True], preds[False])
    eng = model._engine
    rows = eng._ws[N % 128 or 128]["rows"].cpu().numpy()
    # the last batch's recorded arena rows of field "a" are exactly id + table offset
    off = model._table_rows["a"][0]
    last = x["a"][-(N % 128 or 128):]
    assert np.array_equal(rows[:, 0], (last + off).astype(np.int32))
    x2 = dict(x, price=np.zeros(N, dtype=np.float32))
    assert not np.array_equal(model.predict(x2, batch_size=128), preds[False])


@pytest.mark.parametrize("opt,loss", [("sgd", "binary_crossentropy"), ("adagrad", "mse"), ("rmsprop", "mae"), ("adam", "mse")])
def test_other_optimizers_and_losses_of_compile(opt, loss):
    """compile() accepts what the reference's does (models/meta_basemodel.py:612-653): sgd / adagrad / rmsprop next to adam,
    mse / mae next to binary_crossentropy.  Three steps against torch's own optimizers on the oracle's dense gradients."""
    c = Case("small_qkv")
    model = build_model(c, DEV)
    model.compile(opt, loss)
    model.eval()
    eng = model._require_engine()
    lr = model._adam_cfg["lr"]
    X, y = c.X.to(DEV), c.y.to(DEV)
    tr = O.OracleTrainer(c.tensors("param"), c.spec(), lr=lr, optimizer=opt, loss=loss)
    eng.reset_epoch_sums()
    loss_ref = reg_ref = 0.0
    for _ in range(3):
        eng.train_step(X, y)
        a, b = tr.step(c.X, c.y)
        loss_ref, reg_ref = loss_ref + a, reg_ref + b
    got_loss, got_reg = eng.epoch_sums()
    assert got_loss == pytest.approx(loss_ref, rel=2e-5)
    assert got_reg == pytest.approx(reg_ref, rel=2e-5)
    got, want = sd_to_cpu(model), tr.state()
    init = c.tensors("param")
    for k, w in want.items():
        moved = float((w - init[k]).abs().max())
        if moved == 0.0:
            assert torch.equal(got[k], w), k
            continue
        err = (got[k] - w).abs().flatten().double()
        if opt == "sgd":                     # well-conditioned: every element
            assert float(err.max()) <= 2e-4 * moved + 1e-9, (k, float(err.max()), moved)
        else:                                # g / sqrt(state): ill-conditioned where the gradient is ~0 (see the Adam tests)
            assert float(err.median()) <= 2e-3 * lr * 3, (k, float(err.median()))
            assert float(err.max()) <= 2.0 * lr * 3 + 1e-6, (k, float(err.max()))


def test_one_launch_batch_metrics_equal_sklearn():
    """csrc/metrics.hip (satrans_batch_metrics; what fit(verbose > 0) launches once per step): log loss and ROC AUC of a batch
    against sklearn on host copies - all scores distinct, 13 / 2 distinct levels (large tie groups), saturated and denormal
    probabilities, every batch-size class of the kernel, one class only (NaN, as sklearn raises), run-to-run bit identity -
    and fit()'s History through it against the reference's own per-step sklearn path."""
    from sklearn.metrics import log_loss, roc_auc_score
    from satrans_amd import device_metrics as DM
    rng = np.random.RandomState(9)
    for n, levels in ((8192, None), (8192, 13), (5000, 2), (4096, None), (2048, 5), (1500, None), (1024, 3), (257, 2), (2, None)):
        p = rng.rand(n).astype(np.float32)
        if levels:
            p = (np.floor(p * levels) / levels).astype(np.float32)
        if n >= 4:
            p[:4] = [0.0, 1.0, 1e-30, 1 - 1e-7]
        y = (rng.rand(n) < 0.2).astype(np.float32)
        y[0], y[1] = 1.0, 0.0                                        # both classes present
        yt, pt = torch.from_numpy(y).to(DEV), torch.from_numpy(p).to(DEV)
        assert DM.fused_supported(["binary_crossentropy", "auc"], n, yt, pt)
        out = torch.zeros(2, 2, dtype=torch.float64, device=DEV)
        DM.fused_logloss_auc(yt, pt, out[0])
        DM.fused_logloss_auc(yt.reshape(-1, 1), pt.reshape(-1, 1), out[1])
        got = out.cpu().numpy()
        assert np.array_equal(got[0], got[1]), "two launches on the same batch differ"
        p64 = p.astype("float64")
        assert got[0, 0] == pytest.approx(log_loss(y, p64), rel=1e-12), (n, levels)
        assert got[0, 1] == pytest.approx(roc_auc_score(y, p64), rel=1e-12, abs=1e-15), (n, levels)
    ones = torch.ones(100, device=DEV)
    DM.fused_logloss_auc(ones, torch.rand(100, device=DEV), out[0])
    assert bool(torch.isnan(out[0, 1])) and bool(torch.isfinite(out[0, 0]))
    assert not DM.fused_supported(["auc", "mse"], 100, ones, ones) and not DM.fused_supported(["auc"], 8193, ones, ones)
    # fit(): per-step metrics through the kernel == the reference's sklearn-on-host path (SATRANS_HOST_METRICS=1)
    c = Case("aliccp_sota")
    names = c.meta["feature_names"]
    x = {nm: c.z[f"fit/x/{nm}"] for nm in names}
    hist = []
    for host in ("0", "1"):
        os.environ["SATRANS_HOST_METRICS"] = host
        try:
            model = build_model(c, DEV)
            model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
            model.eval()                                                # (no dropout: both runs see the same steps)
            model.train = lambda mode=True: model                       # fit() switches to training mode: keep evaluation mode
            hist.append(model.fit(x=dict(x), y=c.z["fit/y"], batch_size=64, epochs=1, verbose=2, shuffle=False).history)
        finally:
            os.environ.pop("SATRANS_HOST_METRICS", None)
    for k in ("binary_crossentropy", "auc"):
        assert hist[0][k][0] == pytest.approx(hist[1][k][0], rel=1e-9), k


def test_device_metrics_and_the_per_scenario_report_equal_sklearn_on_the_gpu():
    """satrans_amd/device_metrics.py on device tensors (sort + searchsorted on the GPU) against sklearn on host copies - ties
    and saturated probabilities included - and `evaluate_domains`, the test report of reference main.py:353-374."""
    from sklearn.metrics import accuracy_score, log_loss, mean_squared_error, roc_auc_score
    from satrans_amd import device_metrics as DM
    rng = np.random.RandomState(5)
    for n, levels in ((32768, None), (8192, 13), (257, 2)):
        p = rng.rand(n).astype(np.float32)
        if levels:
            p = (np.floor(p * levels) / levels).astype(np.float32)
        p[:4] = [0.0, 1.0, 1e-30, 1 - 1e-7]
        y = (rng.rand(n) < 0.2).astype(np.float32)
        dom = rng.randint(0, 4, size=n)
        yt, pt, dt = torch.from_numpy(y).to(DEV), torch.from_numpy(p).to(DEV), torch.from_numpy(dom).to(DEV)
        p64 = p.astype("float64")
        assert float(DM.log_loss(yt, pt)) == pytest.approx(log_loss(y, p64), rel=1e-12)
        assert float(DM.roc_auc(yt, pt)) == pytest.approx(roc_auc_score(y, p64), rel=1e-12, abs=1e-15)
        assert float(DM.mse(yt, pt)) == pytest.approx(mean_squared_error(y, p64), rel=1e-12)
        assert float(DM.accuracy(yt, pt)) == pytest.approx(accuracy_score(y, np.where(p64 > 0.5, 1, 0)), rel=1e-12)
        auc, per, loss = DM.per_domain_auc(yt, pt, dt)
        assert auc == pytest.approx(roc_auc_score(y, p64), rel=1e-12)
        for i in range(4):
            assert per[i] == pytest.approx(roc_auc_score(y[dom == i], p64[dom == i]), rel=1e-12, abs=1e-15)
    c = Case("aliccp_sota")
    model = build_model(c, DEV)
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    names = c.meta["feature_names"]
    x = {nm: c.z[f"fit/x/{nm}"] for nm in names}
    y = c.z["fit/y"]
    rep = model.evaluate_domains(x, y, batch_size=64)
    pred = model.predict(x, 64)
    assert np.array_equal(rep["pred"], pred)
    assert rep["auc"] == pytest.approx(roc_auc_score(y, pred), rel=1e-12)
    ids = np.asarray(x[c.meta["domain"][0]])
    assert sorted(rep["domain_auc"]) == list(range(ids.min(), ids.max() + 1))
    for i, v in rep["domain_auc"].items():
        assert v == pytest.approx(roc_auc_score(y[ids == i], pred[ids == i]), rel=1e-12)
    want = torch.nn.functional.binary_cross_entropy(torch.tensor(pred).squeeze(), torch.tensor(y).double()).item()
    assert rep["loss"] == pytest.approx(want, rel=1e-10)


@pytest.mark.parametrize("name", ["small_d64_u128", "aliccp_sota", "alimama_sota_pos", "small_qkv", "small_k", "small_none",
                                  "small_pos_dense", "small_relu", "small_multidomain", "small_gate", "small_bilinear", "small_d64",
                                  "small_onlyemb"])
def test_general_layer_path_matches_golden_and_the_oracle(monkeypatch, name):
    """csrc/layer_generic.hip (grouped f32-MFMA GEMMs + LayerNorm + attention launches over token rows in HBM; the path of
    BASELINE configs[4]-class shapes), forced also on shapes the fused kernels cover: forward and every gradient against
    the reference's golden vectors, a ragged batch and a training-mode step with replayed dropout masks against the oracle."""
    monkeypatch.setenv("SATRANS_GENERIC", "1")
    c = Case(name)
    model = build_model(c, DEV)
    model.compile("adam", "binary_crossentropy")
    model.eval()
    model.capture_attention = True
    prob = model(c.X.to(DEV))
    eng = model._engine
    assert eng._ws[c.X.shape[0]]["generic"], "the general path was not selected"
    want = c.arrays("out")
    acts = eng.layer_outputs(c.X.shape[0])
    for l in range(c.meta["L"]):
        np.testing.assert_allclose(acts[l + 1].cpu().numpy(), want[f"layer{l}"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(model.domain_int_layers[l].normalized_att_scores.cpu().numpy(), want[f"att{l}"],
                                   rtol=0, atol=2e-6)
    np.testing.assert_allclose(eng.last_logit().cpu().numpy(), want["logit"], rtol=0, atol=LOGIT_ATOL)
    model.capture_attention = False
    if name != "small_relu":
        bce, reg, grads = eng.loss_and_grads(c.X.to(DEV), c.y.to(DEV))
        assert bce == pytest.approx(float(c.z["train/bce"]), rel=2e-6)
        rel, floor = (1e-4, 5e-9) if name == "small_d64_u128" else (5e-5, 1e-9)
        for k, g in c.arrays("grad").items():
            scale = max(1e-6, float(np.abs(g).max()))
            np.testing.assert_allclose(grads[k].cpu().numpy(), g, rtol=0, atol=rel * scale + floor, err_msg=k)
    for B, train in ((5, False), (c.X.shape[0], True)):
        model.train(train)
        X, y = c.X[:B], c.y[:B]
        bce, reg, grads = eng.loss_and_grads(X.to(DEV), y.to(DEV))
        m = c.meta
        drop = O.Dropper("masks", 0.1, O.dropout_masks(eng.drop_seed, eng.drop_step, B, len(m["fields"]), m["D"],
                                                        m["H"], m["L"], 0.1)) if train else None
        # (the oracle in fp64: W_Query / W_Key gradients are differences of nearly equal softmax terms, 1e-3 of the other tensors'
        # scale, and an fp32 oracle carries as much cancellation noise in them as the kernels do - which of the two a 1e-4 bound
        # then measures depends on the mask realisation)
        (bce_ref, reg_ref, g_ref), kinks = oracle_grads_probing_kinks(c.tensors("param", torch.float64), X, y, c.spec(), drop)
        assert bce == pytest.approx(bce_ref, rel=5e-6)
        for k, g in g_ref.items():
            if k in grads:
                scale = max(1e-6, float(g.abs().max()))
                if train:
                    assert_grad_close_but_for_kinks(grads[k].cpu().numpy(), g.numpy(), 1e-4 * scale + softmax_side_floor(k, g_ref, 5e-9),
                                                    f"{k} B={B} train={train} (oracle: {kinks} hidden units on the kink)", kinks=kinks)
                else:
                    np.testing.assert_allclose(grads[k].cpu().numpy().astype(np.float64), g.numpy(), rtol=0, atol=1e-4 * scale + 5e-9,
                                               err_msg=f"{k} B={B} train={train}")


@pytest.mark.parametrize("family", ["fused", "lds"])
@pytest.mark.parametrize("name", ["small_gate", "small_bilinear"])
def test_gate_and_bilinear_kernel_families(monkeypatch, name, family):
    """`gate` / `bilinear` (satrans.py:61-64,68-71,79-81) on the fused kernels - their default since round 3: the doubled gate
    vector / the block-diagonal per-head maps take the MetaNet's place in LDS - and on the LDS-resident kernels
    (csrc/layer_lds.hip, satrans_set_layer_impl(2)); the general path runs the same cases in
    test_general_layer_path_matches_golden_and_the_oracle.  Golden outputs and every gradient, then a ragged batch and a
    training-mode step with the kernels' dropout masks replayed through the oracle."""
    from satrans_amd import native as N
    monkeypatch.setenv("SATRANS_GENERIC", "0")
    c = Case(name)
    if family == "lds":
        N.check(N.lib().satrans_set_layer_impl(2), "set_layer_impl")
    try:
        model = build_model(c, DEV)
        model.compile("adam", "binary_crossentropy")
        model.eval()
        model(c.X.to(DEV))
        eng = model._engine
        assert not eng._ws[c.X.shape[0]]["generic"]
        want = c.arrays("out")
        acts = eng.layer_outputs(c.X.shape[0])
        for l in range(c.meta["L"]):
            np.testing.assert_allclose(acts[l + 1].cpu().numpy(), want[f"layer{l}"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(eng.last_logit().cpu().numpy(), want["logit"], rtol=0, atol=LOGIT_ATOL)
        bce, reg, grads = eng.loss_and_grads(c.X.to(DEV), c.y.to(DEV))
        assert bce == pytest.approx(float(c.z["train/bce"]), rel=2e-6)
        for k, g in c.arrays("grad").items():
            scale = max(1e-6, float(np.abs(g).max()))
            np.testing.assert_allclose(grads[k].cpu().numpy(), g, rtol=0, atol=5e-5 * scale + 1e-9, err_msg=k)
        m = c.meta
        for B, train in ((5, False), (c.X.shape[0], True)):
            model.train(train)
            X, y = c.X[:B], c.y[:B]
            bce, reg, grads = eng.loss_and_grads(X.to(DEV), y.to(DEV))
            drop = O.Dropper("masks", 0.1, O.dropout_masks(eng.drop_seed, eng.drop_step, B, len(m["fields"]), m["D"],
                                                            m["H"], m["L"], 0.1)) if train else None
            bce_ref, reg_ref, g_ref = O.loss_and_grads(c.tensors("param"), X, y, c.spec(), drop)
            assert bce == pytest.approx(bce_ref, rel=5e-6)
            for k, g in g_ref.items():
                if k in grads:
                    scale = max(1e-6, float(g.abs().max()))
                    np.testing.assert_allclose(grads[k].cpu().numpy(), g.numpy(), rtol=0, atol=1e-4 * scale + 5e-9,
                                               err_msg=f"{k} B={B} train={train}")
    finally:
        N.check(N.lib().satrans_set_layer_impl(0), "set_layer_impl")


def test_general_path_sorted_activations_are_the_same_bits():
    """A training step of the general path keeps the activations of a stack of layers - and their gradients on the way back - in
    scenario-sorted order between the layers (SATRANS_X_SORTED / SATRANS_Y_SORTED: no order change at the ends of the interior
    layers).  Same operations on the same values: loss, every gradient and the layer outputs `layer_outputs()` hands out must be
    the bits of the form that changes the order at both ends of every layer, in evaluation and in training mode."""
    c = Case("small_d64_u128")
    res = {}
    for sorted_acts in (True, False):
        model = build_model(c, DEV)
        model.compile("adam", "binary_crossentropy")
        eng = model._require_engine()
        eng.sorted_acts = sorted_acts
        for train in (False, True):
            model.train(train)
            eng.drop_step = 40
            bce, reg, grads = eng.loss_and_grads(c.X.to(DEV), c.y.to(DEV))
            ws = eng._ws[c.X.shape[0]]
            assert ws["generic"] and bool(ws.get("acts_sorted")) == (sorted_acts and c.meta["L"] > 1)
            res[(sorted_acts, train)] = (bce, {k: g.clone() for k, g in grads.items()},
                                         [a.clone() for a in eng.layer_outputs(c.X.shape[0])[1:]])
    assert c.meta["L"] > 1, "the case must stack layers for the flags to be exercised"
    for train in (False, True):
        (bce_a, g_a, acts_a), (bce_b, g_b, acts_b) = res[(True, train)], res[(False, train)]
        assert bce_a == bce_b
        for k in g_b:
            assert torch.equal(g_a[k], g_b[k]), (train, k)
        for l, (a, b) in enumerate(zip(acts_a, acts_b)):
            assert torch.equal(a, b), (train, l)


def test_general_path_attention_arms_agree():
    """The two attention arms of the general forward at a configs[4]-class shape (40 fields, head dimension 16): MFMA
    (transposed scores, softmax in the accumulators, P^T fed straight back as the B operand) and one lane per query row -
    the MFMA-vs-wavefront ablation - must give the same layer outputs to rounding, with and without dropout."""
    from satrans_amd import native as N
    c = Case("small_d64_u128")
    outs, grads = {}, {}
    for mode in (1, 2):
        N.check(N.lib().satrans_set_generic_attention(mode), "set_generic_attention")
        try:
            model = build_model(c, DEV)
            model.compile("adam", "binary_crossentropy")
            for train in (False, True):
                model.train(train)
                model(c.X.to(DEV))
                outs[(mode, train)] = [a.clone() for a in model._engine.layer_outputs(c.X.shape[0])[1:]]
                eng = model._require_engine()
                eng.drop_step = 40          # the same masks in both arms
                grads[(mode, train)] = {k: g.clone() for k, g in eng.loss_and_grads(c.X.to(DEV), c.y.to(DEV))[2].items()}
            assert model._engine._ws[c.X.shape[0]]["generic"]
        finally:
            N.check(N.lib().satrans_set_generic_attention(-1), "set_generic_attention")
    for train in (False, True):
        for a, b in zip(outs[(1, train)], outs[(2, train)]):
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=2e-6)
    assert not torch.equal(outs[(1, True)][0], outs[(1, False)][0])
    # ... and the two backward arms (one lane per row / transposed MFMA tiles with the dK, dV contraction through LDS)
    for train in (False, True):
        for k, g in grads[(1, train)].items():
            scale = max(1e-6, float(g.abs().max()))
            np.testing.assert_allclose(grads[(2, train)][k].cpu().numpy(), g.cpu().numpy(), rtol=0, atol=1e-4 * scale + 1e-8,
                                       err_msg=f"{k} train={train}")


def test_fit_predict_at_baseline_config_scale():
    """BASELINE configs[1] through the public API: 50,000 AliCCP-shaped rows (tables capped at 20k rows per field to
    keep the test light), batch 8192 with a partial last batch, shuffle on, verbose=2 (per-step sklearn metrics),
    then predict at batch 32768.  Checks History, shapes/dtypes, that the loss goes down, and that predict() agrees
    with the CPU oracle evaluated on the trained weights."""
    from satrans_amd import SATrans, SparseFeat
    import bench
    rng = np.random.RandomState(0)
    N = 50000
    vocab = {f: min(bench.ALICCP_MAX[f], 20000) + 2 for f in bench.ALICCP_FIELDS}
    cols = [SparseFeat(f, vocabulary_size=vocab[f], embedding_dim=32) for f in bench.ALICCP_FIELDS]
    x = {f: rng.randint(1 if f == '301' else 0, vocab[f] - 1, size=N) for f in bench.ALICCP_FIELDS}
    # labels depend on two fields so that there is something to learn
    y = ((x['121'] % 2 == 0) & (rng.rand(N) < 0.5) | (rng.rand(N) < 0.05)).astype(np.float32)
    model = SATrans(cols, cols, ['301'], [3], att_layer_num=0, domain_att_layer_num=3, att_head_num=4,
                    use_linear=False, use_dnn=False, meta_mode='QK', seed='1021', device=DEV, flag='sota')
    model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy",
                  metrics=["binary_crossentropy", "auc"])
    hist = model.fit(x=dict(x), y=y, batch_size=8192, epochs=3, verbose=2)
    assert list(hist.history) == ["loss", "binary_crossentropy", "auc"] and len(hist.history["loss"]) == 3
    assert hist.history["loss"][-1] < hist.history["loss"][0]
    assert hist.history["auc"][-1] > 0.6
    pred = model.predict(dict(x), 8192 * 4)
    assert pred.shape == (N, 1) and pred.dtype == np.float64 and np.isfinite(pred).all()
    # oracle on the trained weights, first 4096 rows
    spec = O.PathSpec(sparse=[(f, i) for i, f in enumerate(bench.ALICCP_FIELDS)], dense=[], domain_cols=[18],
                      embedding_dim=32, head_num=4, layer_num=3, flag='sota', meta_mode='QK', meta_units=[32, 64, 32])
    X = np.stack([x[f] for f in bench.ALICCP_FIELDS], axis=1).astype(np.float32)[:4096]
    p_ref, _ = O.forward(sd_to_cpu(model), torch.from_numpy(X), spec)
    # (predict is an evaluation forward: fp32 products in either product mode)
    np.testing.assert_allclose(pred[:4096], p_ref.numpy().astype(np.float64), rtol=0, atol=5e-6)
    ev = model.evaluate(dict(x), y, 8192 * 4)
    assert set(ev) == {"binary_crossentropy", "auc"}


def test_public_api_on_full_size_aliccp_tables_against_the_oracle():
    """BASELINE configs[1] with the FULL-SIZE tables (6,571,961 rows, 841 MB) through the public API: `fit` for two steps of
    1,024 samples (dropout off, as in the golden fit cases), then `predict` - against the CPU oracle taking the same two dense
    steps over every table row (torch.optim.Adam + dense L2, ~2 s per step on the host) from the same seeded parameters:
    logged loss, and predictions on fresh rows through both trained models.  (The 50,000-row test above caps the tables.)"""
    import bench
    B = 1024
    X, y = bench.synth_batches(3 * B, 17)
    model = bench.build_model("cpu", 0.005)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    by_ptr = {}
    for k, v in model.state_dict().items():                      # keep the reference's aliasing (K_/V_ share Q_'s tensors)
        state[k] = by_ptr.setdefault(v.data_ptr(), state[k])
    model.to(DEV)
    model.device = DEV
    model._require_engine().drop_p = 0.0
    x = {f: X[:2 * B, i] for i, f in enumerate(bench.ALICCP_FIELDS)}
    hist = model.fit(x=x, y=y[:2 * B], batch_size=B, epochs=1, verbose=0, shuffle=False)
    tr = O.OracleTrainer(state, bench.oracle_spec(), lr=0.005)
    total = 0.0
    for i in range(2):
        bce, reg = tr.step(torch.from_numpy(X[i * B:(i + 1) * B]), torch.from_numpy(y[i * B:(i + 1) * B]))
        total += bce + reg
    assert hist.history["loss"][0] == pytest.approx(total / (2 * B), rel=2e-5)
    x_new = {f: X[2 * B:, i] for i, f in enumerate(bench.ALICCP_FIELDS)}
    pred = model.predict(x_new, B)
    p_ref, _ = O.forward(tr.state(), torch.from_numpy(X[2 * B:]), bench.oracle_spec())
    # two Adam steps move every weight by ~lr; elements with near-zero gradients may differ by a step between any two fp32
    # implementations (see the Adam tests), which shows up as ~1e-4 on a probability
    np.testing.assert_allclose(pred, p_ref.numpy().astype(np.float64), rtol=0, atol=2e-3)
    assert float(np.abs(pred - p_ref.numpy()).mean()) < 2e-4
    # and the untouched rows took their regulariser-only steps (|g| = 2 l2 |p| ~ 2e-9 against eps = 1e-8: ~0.07 lr per step)
    sd = sd_to_cpu(model)
    name = "embedding_dict.205.weight"                           # 4.3 M rows, 2,048 of them gathered
    moved = (sd[name] - state[name]).abs()
    ref_moved = (tr.state()[name] - state[name]).abs()
    assert float((moved - ref_moved).abs().max()) < 2 * 0.005 + 1e-6
    assert float((moved - ref_moved).abs().median()) < 1e-6
    assert float(moved.median()) > 1e-4


def test_teacher_forced_step_at_the_baseline_batch_on_full_size_tables():
    """The optimizer at BASELINE configs[1] scale, pinned tightly: full-size tables (6,571,961 rows),
    B = 8,192.  Two free-running GPU steps first (so that the moments are non-trivial and the lazy form has postponed steps
    in flight), then the oracle - torch.optim.Adam over EVERY row with the dense L2 term, reference main.py:343 +
    meta_basemodel.py:577-593 - takes over the GPU's parameters and both moments bit for bit and both take ONE step on a
    fresh batch.  Moments element by element at 1e-4 / 2e-4 of the tensor's largest element, for gathered and for
    not-gathered rows of every table separately (the latter move by the regulariser-only gradient 2 l2 p: they are what the
    lazy replay / flush produces); parameters wherever Adam's quotient is well-conditioned."""
    import bench
    B, lr = 8192, 0.005
    X, y = bench.synth_batches(3 * B, 23)
    model = bench.build_model("cpu", lr)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    by_ptr = {}
    for k, v in model.state_dict().items():                      # keep the reference's aliasing
        state[k] = by_ptr.setdefault(v.data_ptr(), state[k])
    model.to(DEV)
    model.device = DEV
    model.eval()                                                 # dropout off: the oracle replays no masks here
    eng = model._require_engine()
    Xd, yd = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    for i in range(2):
        eng.train_step(Xd[i * B:(i + 1) * B], yd[i * B:(i + 1) * B])
    assert eng.lazy and eng._lazy_pending
    sd, opt = sd_to_cpu(model), model.optimizer_state_dict()     # (flushes the postponed steps)
    assert opt["step"] == 2
    tr = O.OracleTrainer(state, bench.oracle_spec(), lr=lr)
    for k, leaf in tr.leaves.items():
        leaf.data.copy_(sd[k])
        st = opt["state"].get(k)
        if st is not None:
            tr.optim.state[leaf] = dict(step=torch.tensor(2.0), exp_avg=st["exp_avg"].clone(), exp_avg_sq=st["exp_avg_sq"].clone())
    before = {k: leaf.detach().clone() for k, leaf in tr.leaves.items()}
    O.KINK_PROBE = {"eps": 2e-6, "near_zero": 0}      # hidden units of THIS step within fp32 rounding of the ReLU's kink
    try:
        bce_ref, reg_ref = tr.step(torch.from_numpy(X[2 * B:]), torch.from_numpy(y[2 * B:]))
        kinks = int(O.KINK_PROBE["near_zero"])
    finally:
        O.KINK_PROBE = None
    print(f"oracle step at B = {B}: {kinks} MetaNet hidden units within 2e-6 of the kink")
    eng.reset_epoch_sums()
    eng.train_step(Xd[2 * B:], yd[2 * B:])
    bce, reg = eng.epoch_sums()
    assert bce == pytest.approx(bce_ref, rel=2e-6)
    assert reg == pytest.approx(reg_ref, rel=2e-5)
    got, gopt = sd_to_cpu(model), model.optimizer_state_dict()
    assert gopt["step"] == 3
    Xl = torch.from_numpy(X[2 * B:]).long()
    checked_tables = 0
    for k, leaf in tr.leaves.items():
        if leaf not in tr.optim.state or k not in gopt["state"]:
            continue
        ref_m, ref_v = tr.optim.state[leaf]["exp_avg"], tr.optim.state[leaf]["exp_avg_sq"]
        if float(ref_m.abs().max()) < 1e-8:
            continue
        m, v = gopt["state"][k]["exp_avg"], gopt["state"][k]["exp_avg_sq"]
        groups = [("all", slice(None))]
        if k.startswith("embedding_dict."):
            col = bench.ALICCP_FIELDS.index(k.split(".")[1])
            hit = torch.zeros(leaf.shape[0], dtype=torch.bool)
            hit[Xl[:, col]] = True
            groups = [("gathered", hit), ("not gathered", ~hit)]
            checked_tables += 1
        for what, sel in groups:
            rm, rv, gm, gv = ref_m[sel], ref_v[sel], m[sel], v[sel]
            if rm.numel() == 0:
                continue
            assert_close_but_for_kinks(gm.numpy(), rm.numpy(), rtol=1e-5, atol=1e-4 * float(rm.abs().max()) + 1e-30,
                                       err_msg=f"exp_avg/{k} ({what} rows)", kinks=kinks)
            assert_close_but_for_kinks(gv.numpy(), rv.numpy(), rtol=1e-5, atol=2e-4 * float(rv.abs().max()) + 1e-30,
                                       err_msg=f"exp_avg_sq/{k} ({what} rows)", kinks=kinks)
            delta = (got[k][sel] - leaf.detach()[sel]).abs()
            vhat = rv / (1 - 0.999 ** 3)
            ok = vhat.sqrt() > 1e-4 * max(float(vhat.sqrt().max()), 1e-30)
            if bool(ok.any()):
                assert float(delta[ok].max()) <= 2e-2 * lr, (k, what, float(delta[ok].max()))
            assert float(delta.max()) <= 2.0 * lr + 1e-6, (k, what)
            if what == "not gathered":
                # regulariser-only step: the row moved, and it moved like the oracle's dense step moved it
                moved_ref = (leaf.detach()[sel] - before[k][sel]).abs()
                assert float(moved_ref.median()) > 0
                assert float(delta.median()) <= 1e-3 * float(moved_ref.median()), (k, float(delta.median()))
    assert checked_tables == len(bench.ALICCP_FIELDS)


@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_lazy_adam_is_bitwise_the_streaming_adam(arith):
    """The lazy-exact optimizer path (postponed regulariser-only steps, replayed before a row is gathered and by the
    flush) must leave EXACTLY the tables, moments and epoch sums of the every-step streaming kernel - in either arithmetic."""
    c = Case("aliccp_sota")
    rng = np.random.RandomState(11)
    B, steps = 64, 9
    Xs = [np.stack([rng.randint(1 if f == "301" else 0, v - 1, size=B) for f, v in zip(c.meta["fields"], c.meta["vocab"])],
                   axis=1).astype(np.float32) for _ in range(steps)]
    ys = [(rng.rand(B) < 0.3).astype(np.float32) for _ in range(steps)]
    results = []
    for lazy in (True, False):
        model = build_model(c, DEV)
        model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy")
        model.train()
        eng = model._require_engine()
        eng.lazy, eng.overlap, eng.adam_arith = lazy, False, arith
        eng.reset_epoch_sums()
        for i, (xb, yb) in enumerate(zip(Xs, ys)):
            eng.train_step(torch.from_numpy(xb).to(DEV), torch.from_numpy(yb).to(DEV))
            if i == 4:      # a mid-run evaluation forces a flush in lazy mode and must not change anything
                model.eval(); model(torch.from_numpy(xb).to(DEV)); model.train()
        bce, reg = eng.epoch_sums()
        results.append((sd_to_cpu(model), eng.adam_m.cpu(), eng.adam_v.cpu(), bce, reg))
    (sd_l, m_l, v_l, bce_l, reg_l), (sd_d, m_d, v_d, bce_d, reg_d) = results
    for k in sd_d:
        assert torch.equal(sd_l[k], sd_d[k]), k
    assert torch.equal(m_l, m_d) and torch.equal(v_l, v_d)
    assert bce_l == bce_d
    assert reg_l == pytest.approx(reg_d, rel=1e-6)      # lazy sums p^2 per element in fp32 before going to double


@pytest.mark.parametrize("mode", ["tail", "step"])
@pytest.mark.parametrize("pipelined", [False, True])
def test_rolling_flush_is_bitwise_the_streaming_adam(pipelined, mode):
    """The rolling form of the periodic flush (engine._roll_flush: a slice of the rows per step, on its own lowest-priority
    stream, forked behind the step's last backward kernel - "tail" - or behind its replay launch - "step") leaves EXACTLY the tables, moments and epoch sums of the every-step streaming
    kernel - 43 steps with a slice count of 8 (every row rolled five times), a mid-run evaluation, with and without the
    announced next batch."""
    c = Case("aliccp_sota")
    rng = np.random.RandomState(12)
    B, steps = 64, 43
    Xs = [torch.from_numpy(np.stack([rng.randint(1 if f == "301" else 0, v - 1, size=B)
                                     for f, v in zip(c.meta["fields"], c.meta["vocab"])], axis=1).astype(np.float32)).to(DEV)
          for _ in range(steps)]
    ys = [torch.from_numpy((rng.rand(B) < 0.3).astype(np.float32)).to(DEV) for _ in range(steps)]
    results = []
    for form in ("rolling", "streaming"):
        model = build_model(c, DEV)
        model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy")
        model.train()
        eng = model._require_engine()
        eng.lazy, eng.overlap = form == "rolling", False
        eng.rolling_flush, eng.flush_every = mode if form == "rolling" else "", 8
        eng.reset_epoch_sums()
        rolled = 0
        for i in range(steps):
            eng.train_step(Xs[i], ys[i], next_X=Xs[i + 1] if pipelined and i + 1 < steps else None)
            rolled += eng._roll_done is not None
            if i == 20:
                model.eval(); model(Xs[i]); model.train()
        if form == "rolling":
            assert rolled >= steps - 2 and getattr(eng, "flush_count", 0) <= 2, (rolled, getattr(eng, "flush_count", 0))
        bce, reg = eng.epoch_sums()
        results.append((sd_to_cpu(model), eng.adam_m.cpu(), eng.adam_v.cpu(), bce, reg))
    (sd_l, m_l, v_l, bce_l, reg_l), (sd_d, m_d, v_d, bce_d, reg_d) = results
    for k in sd_d:
        assert torch.equal(sd_l[k], sd_d[k]), k
    assert torch.equal(m_l, m_d) and torch.equal(v_l, v_d)
    assert bce_l == bce_d
    assert reg_l == pytest.approx(reg_d, rel=1e-6)


def test_lazy_adam_stays_bitwise_the_streaming_adam_while_rows_decay():
    """700 steps over two small batches: the rows they never gather decay under the regulariser out of the packed range of the
    replay (|lr * exp_avg| < 2^-80 after ~500 steps) and on towards the subnormals - the regime of most rows of a long run.
    Tables and moments of the lazy form (periodic flushes, replays before every gather) must stay EXACTLY those of the
    every-step streaming kernel, and the decayed regime must actually have been reached."""
    c = Case("aliccp_sota")
    rng = np.random.RandomState(23)
    B, steps = 8, 700
    Xs = [np.stack([rng.randint(1 if f == "301" else 0, v - 1, size=B) for f, v in zip(c.meta["fields"], c.meta["vocab"])],
                   axis=1).astype(np.float32) for _ in range(2)]
    ys = [(rng.rand(B) < 0.3).astype(np.float32) for _ in range(2)]
    Xd = [torch.from_numpy(x).to(DEV) for x in Xs]
    yd = [torch.from_numpy(v).to(DEV) for v in ys]
    results = []
    for lazy in (True, False):
        model = build_model(c, DEV)
        model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy")
        model.train()
        eng = model._require_engine()
        eng.lazy, eng.overlap = lazy, False
        for i in range(steps):
            eng.train_step(Xd[i % 2], yd[i % 2])
        eng.flush_lazy()
        results.append((model.embedding_arena.detach().cpu(), eng.adam_m.cpu(), eng.adam_v.cpu()))
    (p_l, m_l, v_l), (p_d, m_d, v_d) = results
    for a, b, what in ((p_l, p_d, "p"), (m_l, m_d, "m"), (v_l, v_d, "v")):
        same = a.view(torch.int32) == b.view(torch.int32)
        assert bool(same.all()), f"{what}: {int((~same).sum())} elements differ between the lazy and the streaming form"
    decayed = ((0.005 * m_d).abs() < 2.0 ** -80) & (m_d != 0)
    assert float(decayed.float().mean()) > 0.2, "the run did not reach the decayed regime it is meant to cover"


def test_packed_replay_arithmetic_is_the_ieee_arithmetic():
    """The replay / flush kernels run their square root and division as packed fma sequences (embed_adam.hip).  They must be
    the correctly rounded operations: the square root is compared with the fp32 rounding of the fp64 square root (correct, as
    53 >= 2*24 + 2) on EVERY float of the packed operand range [2^-100, 2^64], the division with the rounded fp64 quotient on
    2^33 pseudo-random pairs of its range (both signs); the scalar sqrtf / division of the streaming kernel are held against the
    same references in the same pass."""
    import ctypes as C
    from satrans_amd import native as N
    lib = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    bad = C.c_uint64(123)
    lo = int(np.float32(2.0 ** -100).view(np.uint32))
    hi = int(np.float32(2.0 ** 64).view(np.uint32))
    N.check(lib.satrans_debug_check_packed_math(0, lo - 1000, hi - lo + 2000, C.byref(bad), st), "packed sqrt")
    assert bad.value == 0, f"{bad.value} square roots are not correctly rounded"
    for seed in (0, 1 << 40):
        N.check(lib.satrans_debug_check_packed_math(1, seed, 1 << 32, C.byref(bad), st), "packed division")
        assert bad.value == 0, f"{bad.value} quotients are not correctly rounded"
    # below the packed range (rows that decay under the regulariser): the same sequences behind exact power-of-two scaling -
    # EVERY positive float under 2^-100, subnormals included, and 2^33 numerator / denominator pairs with numerators from the
    # smallest subnormal to 2^-80 and signed zeros
    N.check(lib.satrans_debug_check_packed_math(2, 0, lo + 1000, C.byref(bad), st), "scaled sqrt")
    assert bad.value == 0, f"{bad.value} scaled square roots are not correctly rounded"
    for seed in (0, 1 << 40):
        N.check(lib.satrans_debug_check_packed_math(3, seed, 1 << 32, C.byref(bad), st), "scaled division")
        assert bad.value == 0, f"{bad.value} scaled quotients are not correctly rounded"


@pytest.mark.parametrize("arith", ["exact", "fast"])
@pytest.mark.parametrize("state", ["edge", "decayed", "eps0"])
@pytest.mark.parametrize("D", [16, 32, 64])
def test_lazy_flush_equals_streaming_steps_on_edge_values(D, state, arith):
    """Kernel level: K regulariser-only steps through the streaming kernel (one launch per step) and one flush (and one
    replay of a row list) must leave identical bits - `edge`: on ordinary table values and on the values that take the scalar
    path of the packed replay (zeros, subnormals, 1e-30, 1e20, negative zero) mixed into the same lanes; `decayed`: on the state
    of rows nobody gathers (magnitudes log-uniform from 1e-8 down through the subnormals to exact zeros of both signs, second
    moments down to subnormals and zero, whole rows of zeros, a few ordinary rows in between), over enough steps for values to
    cross from the packed range into the scaled one, into the subnormals and to zero; `eps0`: the decayed state with eps = 0,
    where a zero second moment under a zero numerator is 0 / 0 = NaN in the streaming kernel (and in torch.optim.Adam): the
    shortcuts of the lazy kernels for zero numerators must not hide it."""
    import ctypes as C
    import math
    from satrans_amd import native as N
    lib = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(17 + D)
    R, K = (4099, 13) if state == "edge" else (4099, 61 if state == "decayed" else 9)
    lr, b1, b2, eps, l2 = 0.005, 0.9, 0.999, (0.0 if state == "eps0" else 1e-8), 1e-5
    P = torch.randn(R, D, generator=g) * 1e-4
    M = torch.randn(R, D, generator=g) * 1e-9
    V = torch.rand(R, D, generator=g) * 1e-17
    odd = torch.tensor([0.0, -0.0, 1e-45, 3e-39, 1e-30, -1e-30, 1e20, -3e18, 1.0, 1e-12], dtype=torch.float32)
    pick = torch.randint(0, odd.numel(), (R, D), generator=g)
    if state == "edge":
        where = torch.rand(R, D, generator=g) < 0.05
        P = torch.where(where, odd[pick], P)
        M = torch.where(torch.rand(R, D, generator=g) < 0.03, torch.zeros(()), M)
        V = torch.where(torch.rand(R, D, generator=g) < 0.03, odd[pick].abs() ** 2, V)
        V = torch.where(torch.isfinite(V), V, torch.full((), 1e30))
    else:
        def tiny(lo_exp, hi_exp):       # +-10^u, u uniform in [lo_exp, hi_exp]: float32 rounds what is below its range to subnormals / zero
            u = torch.rand(R, D, generator=g, dtype=torch.float64) * (hi_exp - lo_exp) + lo_exp
            sign = torch.where(torch.rand(R, D, generator=g) < 0.5, -1.0, 1.0).double()
            return (sign * torch.pow(torch.tensor(10.0, dtype=torch.float64), u)).to(torch.float32)
        ordinary = (torch.rand(R, 1, generator=g) < 0.1).expand(R, D)          # every tenth row stays an ordinary row
        zero_row = (torch.rand(R, 1, generator=g) < 0.2).expand(R, D) & ~ordinary
        zero_row = zero_row.clone()
        zero_row[1000:1400] = True              # (whole waves of rows that have decayed to zero)
        ordinary = ordinary.clone()
        ordinary[1000:1400] = False
        ordinary[2000:2200] = True              # (and whole waves of ordinary rows)
        P = torch.where(ordinary, P, tiny(-46.0, -8.0))
        M = torch.where(ordinary, M, tiny(-47.0, -13.0))
        V = torch.where(ordinary, V, tiny(-46.0, -17.0).abs())
        signed_zero = torch.where(torch.rand(R, D, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
        P = torch.where(zero_row, signed_zero, P)
        M = torch.where(zero_row, torch.where(torch.rand(R, D, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0)), M)
        M = torch.where(torch.rand(R, D, generator=g) < 0.05, signed_zero, M)
        # (a zero second moment under a non-zero first one sends its whole wave to the IEEE path: rare, so that most waves take
        #  the scaled sequences)
        V = torch.where(torch.rand(R, D, generator=g) < 1e-4, torch.zeros(()), V)
    f32 = lambda x: float(np.float32(x))
    table = torch.tensor([(0.0, 1.0)] + [(f32(lr / (1.0 - b1 ** s)), 1.0 / f32(math.sqrt(1.0 - b2 ** s))) for s in range(1, K + 1)],
                         dtype=torch.float64, device=DEV)

    def hp(t):
        h = N.AdamHParams()
        h.lr_over_bc1, h.bc2_sqrt = lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t)
        h.beta1, h.beta2, h.eps, h.l2 = b1, b2, eps, l2
        h.arith = N.ADAM_FAST if arith == "fast" else N.ADAM_EXACT       # (every form runs the same sequence in either arithmetic)
        return h

    Ps, Ms, Vs = (x.clone().to(DEV) for x in (P, M, V))
    touched = torch.zeros((R + 31) // 32, dtype=torch.int32, device=DEV)
    regs = torch.zeros(int(lib.satrans_embed_reg_partials(R, 64, D)), dtype=torch.float64, device=DEV)
    for t in range(1, K + 1):
        N.check(lib.satrans_embed_adam_untouched(Ps.data_ptr(), Ms.data_ptr(), Vs.data_ptr(), 0, R, D, touched.data_ptr(),
                                                 C.byref(hp(t)), regs.data_ptr(), 0, st), "untouched")
    # flush: everything from step 0 to K in one launch
    Pf, Mf, Vf = (x.clone().to(DEV) for x in (P, M, V))
    last = torch.zeros(R, dtype=torch.int32, device=DEV)
    n = 64
    regl = torch.zeros(int(lib.satrans_embed_lazy_reg_partials(n, D)), dtype=torch.float64, device=DEV)
    N.check(lib.satrans_embed_lazy_flush(Pf.data_ptr(), Mf.data_ptr(), Vf.data_ptr(), last.data_ptr(), R, D, K, table.data_ptr(),
                                         C.byref(hp(K)), n, regl.data_ptr(), st), "flush")
    assert int(last.min()) == K
    for a, b, what in ((Pf, Ps, "p"), (Mf, Ms, "m"), (Vf, Vs, "v")):
        same = (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
        assert bool(same.all()), f"{what}: {int((~same).sum())} elements differ between flush and streaming steps"
    # replay of a sorted row list with duplicates, in two stages (0 -> 5 for some rows, then everything listed -> K)
    Pr, Mr, Vr = (x.clone().to(DEV) for x in (P, M, V))
    last = torch.zeros(R, dtype=torch.int32, device=DEV)
    rows1 = torch.sort(torch.randint(0, R, (1000,), generator=g).to(torch.int32)).values.to(DEV)
    rows2 = torch.sort(torch.randint(0, R, (3000,), generator=g).to(torch.int32)).values.to(DEV)
    for rows, target in ((rows1, 5), (rows2, K)):
        regr = torch.full((int(lib.satrans_embed_lazy_reg_partials(rows.numel(), D)),), 7.0, dtype=torch.float64, device=DEV)
        N.check(lib.satrans_embed_lazy_replay(Pr.data_ptr(), Mr.data_ptr(), Vr.data_ptr(), last.data_ptr(), D, rows.data_ptr(),
                                              rows.numel(), target, table.data_ptr(), C.byref(hp(target)), regr.data_ptr(), st),
                "replay")
        slots = (rows.numel() * D + 255) // 256
        assert not bool((regr[:slots] == 7.0).any()), "every partial-sum slot of the replay must be written"
    done = (last == K).cpu()
    assert int(done.sum()) == int(torch.unique(rows2).numel())
    for a, b, what in ((Pr, Ps, "p"), (Mr, Ms, "m"), (Vr, Vs, "v")):
        same = (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
        assert bool(same[done.to(DEV)].all()), f"{what}: replayed rows differ from the streaming steps"
    untouched_rows = (last == 0).cpu()
    assert torch.equal(Pr.cpu()[untouched_rows], P[untouched_rows])


def _dp_worker(rank, world, port, name, steps, out_dir, small_rows, mode="owner"):
    """One data-parallel rank of the engine; both ranks share cuda:0 and talk over gloo (host-staged), which runs
    exactly the code path of an RCCL job: ids all-gathered before the forward, gradient rows after the backward."""
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["SATRANS_SMALL_TABLE_ROWS"] = str(small_rows)
    os.environ["SATRANS_DP_MODE"] = mode
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from satrans_amd import parallel
        c = Case(name)
        model = build_model(c, DEV)
        model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
        model.eval()
        eng = model._require_engine()
        n = c.X.shape[0] // world
        X, y = c.X[rank * n:(rank + 1) * n].to(DEV), c.y[rank * n:(rank + 1) * n].to(DEV)
        eng.reset_epoch_sums()
        for _ in range(steps):
            eng.train_step(X, y)
        sums = eng.epoch_sums()                                   # (collective in the owner form)
        res = sd_to_cpu(model)
        opt = model.optimizer_state_dict()
        for k, st_ in opt["state"].items():
            res["exp_avg/" + k], res["exp_avg_sq/" + k] = st_["exp_avg"], st_["exp_avg_sq"]
        res["__reg__"] = torch.tensor(sums[1], dtype=torch.float64)
        res["__owner__"] = torch.tensor(eng._owner_world)
        res["__calls__"] = torch.tensor(sorted(parallel.STATS).index("all_to_all_rows_f32") if "all_to_all_rows_f32" in parallel.STATS else -1)
        torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["owner", "replicated"])
@pytest.mark.parametrize("small_rows", [16384, 20, 0])
@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos"])
def test_two_data_parallel_ranks_reproduce_the_full_batch_step(name, small_rows, mode, tmp_path):
    """Reference semantics of several GPUs (meta_basemodel.py:272-275, 317): per-GPU batches, loss SUMMED over all
    samples, one optimizer step on the summed gradient.  Two ranks with half of the golden batch each must therefore
    land where the reference's single full-batch steps land, and the two replicas must be bit-identical.
    `small_rows` moves the boundary between the table classes of the exchange: 16384 = every golden table takes the dense
    all-reduced path, 0 = every table goes through the exchanged sorted (row, gradient) lists, 20 = a mix (the golden tables
    have 3 .. 42 rows).
    `mode`: "owner" = every rank steps only the slice of the large tables it owns (ids to the owners, current rows back,
    gradient rows to the owners; replicas brought together at the flush points), "replicated" = every rank applies every
    rank's updates.  Both must leave bit-identical replicas - parameters AND Adam moments - and the two forms must agree with
    each other to the rounding of a sum (same summation order: rank-major, then position)."""
    import socket
    import torch.multiprocessing as mp
    c = Case(name)
    if c.X.shape[0] % 2:
        pytest.skip("odd golden batch")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    steps = c.meta["adam_steps"]
    mp.spawn(_dp_worker, args=(2, port, name, steps, str(tmp_path), small_rows, mode), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    owner_ran = int(r0.pop("__owner__")) == 2
    r1.pop("__owner__"); r0.pop("__calls__"); r1.pop("__calls__")
    assert owner_ran == (mode == "owner" and small_rows < 42), "unexpected data-parallel form"
    for k in r0:
        assert torch.equal(r0[k], r1[k]), f"replicas diverged at {k}"
    reg = float(r0.pop("__reg__")); r1.pop("__reg__")
    moments = {k: r0.pop(k) for k in list(r0) if k.startswith("exp_avg")}
    # the logged regulariser sum covers ALL rows whichever rank stepped them (reference: l2 * sum(w^2) over every table,
    # meta_basemodel.py:577-593): against the oracle's dense steps on the full batch
    tr = O.OracleTrainer(c.tensors("param"), c.spec(), lr=c.meta["lr"])
    reg_ref = sum(tr.step(c.X, c.y)[1] for _ in range(steps))
    assert reg == pytest.approx(reg_ref, rel=5e-5), (reg, reg_ref)
    if mode == "owner":
        # The other form on the same inputs.  Both add a row's gradient rows in the same ORDER (rank-major, then position), but
        # the ordered segmented sums bracket by 32-position chunks of the list they run over - all ranks' rows there, one
        # owner's slice here - so the two forms may differ in the last bit of a sum: moments to 1e-5 of their largest element,
        # parameters wherever Adam's quotient does not amplify that (same criterion as the trajectory test).
        other = tmp_path / "replicated"
        other.mkdir()
        mp.spawn(_dp_worker, args=(2, port + 1 if port < 65000 else port - 1, name, steps, str(other), small_rows, "replicated"),
                 nprocs=2, join=True)
        q0 = torch.load(other / "rank0.pt")
        for k, v in moments.items():
            if float(q0[k].abs().max()) < 1e-8:
                continue                          # mathematically-zero gradient: its moments are rounding noise
            # (the scenario embeddings: 128 numbers that each sum every token of the batch with heavy cancellation - a last-bit
            # difference of the tables after step 1 shows up there at 3.5e-5 of the largest moment after step 3)
            wide = 10.0 if ("domain_embeddings" in k or k.endswith((".W_Query", ".W_Key"))) else 1.0      # (and the softmax-side weights)
            np.testing.assert_allclose(v.numpy(), q0[k].numpy(), rtol=1e-5, atol=wide * 1e-5 * float(q0[k].abs().max()) + 1e-30, err_msg=k)
        gold = c.arrays("grad")
        for k, v in r0.items():
            diff = (v - q0[k]).abs().flatten().double()
            assert float(diff.max()) <= 2.0 * c.meta["lr"] * steps + 1e-6, k
            if k in gold and float(np.abs(gold[k]).max()) >= 1e-7:     # (zero-gradient tensors: Adam on rounding noise)
                assert float(diff.median()) <= 2e-4 * c.meta["lr"] * steps, (k, float(diff.median()))
    want, grads, init, lr = c.tensors("adam"), c.arrays("grad"), c.tensors("param"), c.meta["lr"]
    for k, w in want.items():     # same bounds as test_adam_steps_match_reference_golden
        err = (r0[k] - w).abs().flatten().double()
        if k in grads and float(np.abs(grads[k]).max()) >= 1e-7 and float((w - init[k]).abs().max()) > 0:
            assert float(err.median()) <= 2e-3 * lr * steps, (k, float(err.median()))
            assert float(torch.quantile(err, 0.95)) <= 2e-2 * lr * steps, (k, float(torch.quantile(err, 0.95)))
        assert float(err.max()) <= 2.0 * lr * steps + 1e-6, (k, float(err.max()))


def _dp_dense_worker(rank, world, port, name, opt, steps, out_dir):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = Case(name)
        model = build_model(c, DEV)
        model.compile(opt, "binary_crossentropy")
        model.eval()
        eng = model._require_engine()
        n = c.X.shape[0] // world
        X, y = c.X[rank * n:(rank + 1) * n].to(DEV), c.y[rank * n:(rank + 1) * n].to(DEV)
        for _ in range(steps):
            eng.train_step(X, y)
        torch.save(sd_to_cpu(model), os.path.join(out_dir, f"dense{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_two_ranks_with_the_other_optimizers(opt, tmp_path):
    """Several ranks with SGD / Adagrad / RMSprop (`engine.py` used to raise): all-reduced dense gradient, the
    ranks' (row, gradient row) lists merged rank-major into the dense table gradient.  Two ranks with half the golden batch
    each: replicas identical and on torch's own optimizer applied to the oracle's full-batch gradients."""
    import socket
    import torch.multiprocessing as mp
    c = Case("small_qkv")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    steps = 3
    mp.spawn(_dp_dense_worker, args=(2, port, "small_qkv", opt, steps, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "dense0.pt"), torch.load(tmp_path / "dense1.pt")
    for k in r0:
        assert torch.equal(r0[k], r1[k]), f"replicas diverged at {k}"
    lr = {"sgd": 0.01, "adagrad": 0.01}[opt]
    tr = O.OracleTrainer(c.tensors("param"), c.spec(), lr=lr, optimizer=opt)
    n = (c.X.shape[0] // 2) * 2
    for _ in range(steps):
        tr.step(c.X[:n], c.y[:n])
    init = c.tensors("param")
    for k, w in tr.state().items():
        moved = float((w - init[k]).abs().max())
        if moved == 0.0:
            assert torch.equal(r0[k], w), k
            continue
        err = (r0[k] - w).abs().flatten().double()
        if opt == "sgd":
            assert float(err.max()) <= 2e-4 * moved + 1e-9, (k, float(err.max()), moved)
        else:
            gmax = float(tr.leaves[k].grad.abs().max()) if tr.leaves[k].grad is not None else 0.0
            if gmax >= 1e-5:
                assert float(err.median()) <= 2e-3 * lr * steps, (k, float(err.median()))
            assert float(err.max()) <= 2.0 * lr * steps + 1e-6, (k, float(err.max()))


def _dp_fit_worker(rank, world, port, name, out_dir, mode):
    """Two ranks through the public `fit` (shuffled epochs, a ragged last batch): the owner form sizes its exchanges from the
    epoch plan `fit` hands the engine (engine.plan_owner_counts), not from a per-step read-back."""
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["SATRANS_SMALL_TABLE_ROWS"] = "20"
    os.environ["SATRANS_DP_MODE"] = mode.split("+")[0]
    os.environ["SATRANS_OWNER_PREFETCH"] = "1" if mode.endswith("+prefetch") else "0"      # (the id exchange a step ahead, or in the step)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = Case(name)
        torch.manual_seed(77)                                       # the same shuffles in both forms
        model = build_model(c, DEV)
        model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
        model._require_engine().drop_p = 0.0
        n = c.X.shape[0] // world
        Xr, yr = c.X[rank * n:(rank + 1) * n].numpy(), c.y[rank * n:(rank + 1) * n].numpy()
        x = {f: Xr[:, i] for i, f in enumerate(c.meta["feature_names"])}
        eng = model._require_engine()
        seen = []
        orig = eng.plan_owner_counts

        def spy(*a, **k):
            orig(*a, **k)
            seen.append(None if eng._owner_plan is None else eng._owner_plan["counts"].shape)
        eng.plan_owner_counts = spy
        hist = model.fit(x=x, y=yr, batch_size=10, epochs=2, verbose=0, shuffle=True)
        plan = eng._owner_plan
        res = sd_to_cpu(model)
        res["__loss__"] = torch.tensor(hist.history["loss"], dtype=torch.float64)
        res["__plan__"] = torch.tensor([-1, -1] if plan is None else [plan["step"], plan["counts"].shape[0]])
        res["__plans__"] = torch.tensor(len([s_ for s_ in seen if s_ is not None]))
        torch.save(res, os.path.join(out_dir, f"fit{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_rank_fit_plans_the_owner_exchange_per_epoch(tmp_path):
    """`fit` on two ranks (golden rows split in halves, batch 10: 4 steps per epoch, the last one ragged, shuffle on): in the
    owner form every epoch's exchange sizes come from ONE plan (no per-step read-back) and every step of the epoch consumes its
    entry; replicas identical; loss history and parameters equal to the replicated form's to the rounding of a sum."""
    import socket
    import torch.multiprocessing as mp
    name = "aliccp_sota"
    c = Case(name)
    res = {}
    for mode in ("owner", "owner+prefetch", "replicated"):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        out = tmp_path / mode.replace("+", "_")
        out.mkdir()
        mp.spawn(_dp_fit_worker, args=(2, port, name, str(out), mode), nprocs=2, join=True)
        r0, r1 = torch.load(out / "fit0.pt"), torch.load(out / "fit1.pt")
        for k in r0:
            if not k.startswith("__"):
                assert torch.equal(r0[k], r1[k]), f"{mode}: replicas diverged at {k}"
        res[mode] = r0
    steps = (c.X.shape[0] // 2 - 1) // 10 + 1
    assert res["owner"]["__plan__"].tolist() == [steps, steps], "the epoch plan was not consumed step by step"
    assert res["owner+prefetch"]["__plan__"].tolist() == [steps, steps]
    for k, v in res["owner"].items():                            # where the id exchange runs changes nothing of the result
        assert torch.equal(v, res["owner+prefetch"][k]), f"the exchange a step ahead changed {k}"
    assert int(res["owner"]["__plans__"]) == 2 and res["replicated"]["__plan__"].tolist() == [-1, -1]
    np.testing.assert_allclose(res["owner"]["__loss__"].numpy(), res["replicated"]["__loss__"].numpy(), rtol=1e-6)
    gold = c.arrays("grad")
    lr = c.meta["lr"]
    for k, v in res["owner"].items():
        if k.startswith("__"):
            continue
        diff = (v - res["replicated"][k]).abs().flatten().double()
        assert float(diff.max()) <= 2.0 * lr * 2 * steps + 1e-6, k
        if k in gold and float(np.abs(gold[k]).max()) >= 1e-7:
            assert float(diff.median()) <= 2e-4 * lr * 2 * steps, (k, float(diff.median()))


def test_reference_main_flow_from_an_hdf5_file(tmp_path):
    """examples/aliccp_main.py - the SATrans branch of the reference's main.py on this package - end to end on a small
    `alicpp.h5`-shaped file (written byte by byte by tests/h5_fixture.py; read through satrans_amd/h5lite.py): train one epoch,
    per-scenario report, result line, state_dict dump with the reference's keys; the reported AUCs equal sklearn's on the
    predictions of the dumped weights."""
    import importlib.util
    import json
    from sklearn.metrics import roc_auc_score
    from tests.h5_fixture import write_h5
    spec = importlib.util.spec_from_file_location("aliccp_main", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "aliccp_main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.RandomState(1)
    small = {f: min(v, 500) for f, v in mod.DATA_MAX.items()}

    def split(n):
        d = {f: rng.randint(1 if f == '301' else 0, small[f] + 1, size=n).astype(np.int64) for f in mod.SPARSE}
        d['click'] = ((d['121'] % 2 == 0) & (rng.rand(n) < 0.6) | (rng.rand(n) < 0.05)).astype(np.int64)
        return d
    path = str(tmp_path / "alicpp.h5")
    write_h5(path, {"ctr_train": split(6000), "ctr_test": split(2500)})
    dump, results = str(tmp_path / "model.pt"), str(tmp_path / "res.csv")
    rep = mod.main(["--h5", path, "--batch_size", "1024", "--epochs", "2", "--data_max", json.dumps(small), "--dump", dump,
                    "--results", results])
    assert 0.5 < rep["auc"] <= 1.0 and set(rep["domain_auc"]) == {1, 2, 3}
    line = open(results).read().strip().split(",")
    assert len(line) == 1 + 1 + 3 + 1 and "SATrans_32_0.005_3_4_QK_1021_301_sota" in line[0]
    sd = torch.load(dump)
    assert "embedding_dict.101.weight" in sd and "domain_int_layers.2.W_Query" in sd and sd["embedding_dict.205.weight"].shape == (502, 32)
    from satrans_amd.pipeline import load_h5_columns
    test = load_h5_columns(path, "ctr_test", ["click", "301"])
    assert rep["auc"] == pytest.approx(roc_auc_score(np.asarray(test["click"]), rep["pred"].reshape(-1)), abs=1e-9)
    sel = np.asarray(test["301"]) == 2
    assert rep["domain_auc"][2] == pytest.approx(roc_auc_score(np.asarray(test["click"])[sel], rep["pred"].reshape(-1)[sel]), abs=1e-9)


@pytest.mark.parametrize("B", [1, 2])
def test_regulariser_sum_of_tiny_batches(monkeypatch, B):
    """A batch of one or two samples makes every partial-sum group of the touched-row kernels a single block (their slots
    must not overlap the replay's): the logged regulariser sum must agree between the lazy and the streaming form and with
    the oracle's dense sum(l2 * w^2) over the same steps."""
    c = Case("aliccp_sota")
    sums = {}
    for lazy in ("1", "0"):
        monkeypatch.setenv("SATRANS_LAZY_ADAM", lazy)
        model = build_model(c, DEV)
        model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
        model.eval()
        eng = model._require_engine()
        X, y = c.X[:B].to(DEV), c.y[:B].to(DEV)
        eng.reset_epoch_sums()
        for _ in range(3):
            eng.train_step(X, y)
        sums[lazy] = eng.epoch_sums()
    tr = O.OracleTrainer(c.tensors("param"), c.spec(), lr=c.meta["lr"])
    bce = reg = 0.0
    for _ in range(3):
        b_, r_ = tr.step(c.X[:B], c.y[:B])
        bce, reg = bce + b_, reg + r_
    for lazy in ("1", "0"):
        assert sums[lazy][0] == pytest.approx(bce, rel=1e-5), (lazy, sums[lazy], bce)
        assert sums[lazy][1] == pytest.approx(reg, rel=2e-5), (lazy, sums[lazy], reg)
    assert sums["1"][1] == pytest.approx(sums["0"][1], rel=1e-9)


@pytest.mark.parametrize("mode", ["owner", "replicated"])
@pytest.mark.parametrize("small_rows", ["20", "0"])
def test_rccl_single_rank_exchange_is_bitwise_the_local_step(tmp_path, small_rows, mode):
    """RCCL for real on a one-GPU box: a ONE-rank nccl process group, created before anything touches the GPU, with the
    training step forced through its multi-rank branch (SATRANS_FORCE_EXCHANGE=1): device-pointer int32 all-gather of the
    row ids, SUM all-reduce of the flat gradient, asynchronous fp32 all-gather of the gradient rows + wait(), global sort.
    (`mode` "replicated"; "owner": int64 all-gather of the per-owner counts, int32 all-to-all of the row ids, fp32 all-to-alls
    of the rows and of the gradient rows.)  With one rank every collective is an identity, so the result must equal the local
    step with the same table classes bit for bit - parameters, tables and both Adam moments.  small_rows = 0 makes every table a large one: the exchanged list
    is then as long as the rank's own [B, F] row matrix and must still go through the device-wide sort."""
    import socket
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_one_rank.py")
    outs = {}
    for how in ("nccl", "plain"):
        out = str(tmp_path / f"{how}.pt")
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SATRANS_DP_MODE=mode)
        env.pop("SATRANS_FORCE_EXCHANGE", None)
        r = subprocess.run([sys.executable, script, how, "aliccp_sota", "3", out, str(port), small_rows], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        outs[how] = torch.load(out)
    a, b = outs["nccl"], outs["plain"]
    assert a["__backend__"] == "nccl" and a["__exchange__"] and not b["__exchange__"]
    stats = a["__stats__"]
    names = ("all_gather_rows_i32", "all_reduce_flat_f32", "all_gather_grad_rows_f32") if mode == "replicated" else \
        ("all_gather_counts_i64", "all_to_all_row_ids_i32", "all_to_all_rows_f32", "all_reduce_flat_f32", "all_to_all_grad_rows_f32")
    for name in names:
        assert stats[name]["calls"] == 3 and stats[name]["bytes_in"] > 0, (name, stats)
    assert not b["__stats__"]
    for k in a:
        if not k.startswith("__"):
            assert torch.equal(a[k], b[k]), f"RCCL single-rank exchange changed {k}"


@pytest.mark.parametrize("small_rows", ["16384", "100"])
@pytest.mark.parametrize("lazy", ["1", "0"])
def test_table_classes_on_one_rank_match_reference_golden(monkeypatch, lazy, small_rows):
    """The small/large table classes of the multi-rank step (dense all-reduced gradient + dense step for small tables,
    sorted lists for large ones), forced on a single rank, in both forms of the dense step."""
    monkeypatch.setenv("SATRANS_SPLIT_TABLES", "1")
    monkeypatch.setenv("SATRANS_LAZY_ADAM", lazy)
    monkeypatch.setenv("SATRANS_SMALL_TABLE_ROWS", small_rows)      # 100: some golden tables small, some large
    c = Case("aliccp_sota")
    model = build_model(c, DEV)
    model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
    model.eval()
    eng = model._require_engine()
    assert eng.force_split and eng.small_rows > 0
    X, y = c.X.to(DEV), c.y.to(DEV)
    steps, lr = c.meta["adam_steps"], c.meta["lr"]
    for _ in range(steps):
        eng.train_step(X, y)
    got, want, grads, init = sd_to_cpu(model), c.tensors("adam"), c.arrays("grad"), c.tensors("param")
    for k, w in want.items():
        err = (got[k] - w).abs().flatten().double()
        if k in grads and float(np.abs(grads[k]).max()) >= 1e-7 and float((w - init[k]).abs().max()) > 0:
            assert float(err.median()) <= 2e-3 * lr * steps, (k, float(err.median()))
            assert float(torch.quantile(err, 0.95)) <= 2e-2 * lr * steps, (k, float(torch.quantile(err, 0.95)))
        assert float(err.max()) <= 2.0 * lr * steps + 1e-6, (k, float(err.max()))


@pytest.mark.parametrize("config", ["aliccp", "alimama"])
def test_size_independent_properties_at_the_baseline_batch(config):
    """BASELINE configs[1] shape at the full batch (8192 x 19 fields, D=32, 3 layers, 4 heads, full-size tables) and configs[3]
    (Alimama shape: 15 sparse fields + a dense column, flag sota-pos - separate Q / K generated tables per layer, the
    launch_bwd<32,64,4,false,...> instantiations with the saved-attention hand-over and the fused head), where
    the CPU oracle is too slow to be the checker: properties that hold at any size.
      * the gather is a copy: bit-exact against torch indexing of the arena;
      * a sample's output does not depend on its batch-mates (scenario bucketing, tiling, work distribution):
        forward(X[perm]) == forward(X)[perm] bit for bit, and a prefix of the batch gives the same bits;
      * fixed-order reductions: two training runs from the same seed on the same batches leave identical bits in every
        parameter, table and optimizer-visible quantity (dropout on)."""
    import bench
    B = 8192
    cfg = bench.make_config(config)
    X, y = bench.synth_batches(3 * B, 11, cfg=cfg)
    Xd, yd = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)

    def fresh():
        m = bench.build_model("cpu", cfg["lr"], cfg=cfg)
        m.to(DEV)
        m.device = DEV
        return m

    m1 = fresh()
    m1.eval()
    eng = m1._require_engine()
    p = m1(Xd[:B])
    # gather: layer input = arena rows
    rows = (Xd[:B, :len(cfg["fields"])].long() + eng.row_span[:, 0][None, :])
    assert torch.equal(eng.layer_outputs(B)[0], m1.embedding_arena[rows])
    assert not eng._ws[B]["generic"], "the fused kernels were expected to take this shape"
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(m1(Xd[:B][perm]), p[perm]), "a sample's output depends on the order of the batch"
    assert torch.equal(m1(Xd[:1000]), p[:1000]), "a sample's output depends on the batch size"

    def train(m):
        m.train()
        e = m._require_engine()
        for i in range(3):
            e.train_step(Xd[i * B:(i + 1) * B], yd[i * B:(i + 1) * B])
        assert e._ws[B]["fuse_head"] and all(t is not None for t in e._ws[B]["attn_save"][:-1]), \
            "the step was expected to run the fused last layer and the saved-attention hand-over"
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        return sd, float(e.epoch_sums()[0])

    # both engines were / are created right after construction seeded the generator (the dropout seed derives from it)
    sd1, loss1 = train(m1)
    m2 = fresh()
    sd2, loss2 = train(m2)
    assert loss1 == loss2
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), f"run-to-run difference in {k}"


def test_skewed_ids_at_the_baseline_batch_are_reproducible_and_lazy_equals_streaming():
    """The full batch (8192 x 19, full-size tables) with SKEWED ids - log-uniform ranks, P(id) ~ 1 / (id + 1): what real CTR ids
    look like - so that hot rows appear thousands of times in one batch: runs of thousands of positions through
    the ordered segmented sums (touched_chunks, the superchunk walk) and replays of rows gathered every step.  Properties:
      * the gather is a copy (bit-exact against torch indexing);
      * two training runs from one seed leave identical bits (fixed-order reductions over the long runs);
      * the lazy optimizer form leaves the bits of the every-step streaming kernel, tables and both moments."""
    import bench
    B, steps = 8192, 4
    cfg = bench.make_config("aliccp")
    X, y = bench.synth_batches(steps * B, 29, ids="skewed", cfg=cfg)
    Xd, yd = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    # the premise: hot rows - the most frequent row of the largest table fills hundreds of positions of ONE batch
    col = X[:B, cfg["fields"].index("205")].astype(np.int64)
    assert np.bincount(col).max() > 300, "the skewed batches are expected to repeat their hot rows hundreds of times"

    def run(lazy):
        m = bench.build_model("cpu", cfg["lr"], cfg=cfg)
        m.to(DEV)
        m.device = DEV
        e = m._require_engine()
        m.eval()
        m(Xd[:B])
        rows = (Xd[:B, :len(cfg["fields"])].long() + e.row_span[:, 0][None, :])
        assert torch.equal(e.layer_outputs(B)[0], m.embedding_arena[rows])
        m.train()
        e.lazy = lazy
        for i in range(steps):
            e.train_step(Xd[i * B:(i + 1) * B], yd[i * B:(i + 1) * B])
        e.flush_lazy()
        return ({k: v.detach().clone() for k, v in m.state_dict().items()}, e.adam_m.clone(), e.adam_v.clone(),
                float(e.epoch_sums()[0]))

    sd1, m1, v1, loss1 = run(True)
    sd2, m2, v2, loss2 = run(True)
    assert loss1 == loss2
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), f"run-to-run difference in {k}"
    assert torch.equal(m1, m2) and torch.equal(v1, v2)
    del sd2, m2, v2
    sd3, m3, v3, loss3 = run(False)
    assert loss1 == loss3
    for k in sd1:
        assert torch.equal(sd1[k].view(torch.int32) if sd1[k].dtype == torch.float32 else sd1[k],
                           sd3[k].view(torch.int32) if sd3[k].dtype == torch.float32 else sd3[k]), f"lazy and streaming differ in {k}"
    assert torch.equal(m1, m3) and torch.equal(v1, v3)


def test_vocabulary_above_2_pow_24_uses_integer_ids():
    """Ids of 2**24 and above do not survive the reference's fp32 id matrix (16777217 becomes 16777216).  The integer-id
    layout must gather exactly the addressed rows, and fit/predict must run on it."""
    from satrans_amd import SATrans, SparseFeat
    V = (1 << 24) + 8
    cols = [SparseFeat("big", vocabulary_size=V, embedding_dim=16), SparseFeat("small", vocabulary_size=10, embedding_dim=16),
            SparseFeat("dom", vocabulary_size=4, embedding_dim=16)]
    model = SATrans(cols, cols, ["dom"], [3], att_layer_num=0, domain_att_layer_num=2, att_head_num=2,
                    use_linear=False, use_dnn=False, meta_mode='QK', meta_dnn_hidden_units=(32, 16), seed=5,
                    device=DEV, flag='sota')
    model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy")
    rng = np.random.RandomState(1)
    n = 512
    x = {"big": np.concatenate([np.arange((1 << 24) - 4, (1 << 24) + 8), rng.randint(0, V, size=n - 12)]).astype(np.int64),
         "small": rng.randint(0, 10, size=n), "dom": rng.randint(1, 4, size=n)}
    y = (rng.rand(n) < 0.3).astype(np.float32)
    model.eval()
    X = model._to_device_matrix(model._pack(x))
    assert X.dtype == torch.int64
    model(X)
    eng = model._require_engine()
    want = torch.stack([model.embedding_dict[c].weight[torch.from_numpy(x[c]).to(DEV)] for c in ("big", "small", "dom")], dim=1)
    assert torch.equal(eng.layer_outputs(n)[0], want), "integer ids must address exactly their rows"
    with pytest.raises(ValueError):
        model._to_device_matrix(model._pack({k: v.astype(np.float32) for k, v in x.items()}))
    before = model.embedding_dict["big"].weight[(1 << 24) + 1].clone()
    hist = model.fit(x=x, y=y, batch_size=256, epochs=2, verbose=0)
    assert np.isfinite(hist.history["loss"]).all() and hist.history["loss"][1] < hist.history["loss"][0]
    assert not torch.equal(model.embedding_dict["big"].weight[(1 << 24) + 1], before)
    p = model.predict(x, 512)
    assert p.shape == (n, 1) and np.isfinite(p).all()


@pytest.mark.parametrize("B", [1, 5, 37])
@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos", "small_qkv"])
def test_ragged_batches_gradients_match_the_oracle(name, B):
    """Batches that fill no tile (one sample), one tile partly, or several tiles with a ragged last one; with scenario rows that
    receive no sample at all.  Loss and every gradient against the CPU oracle on the same rows."""
    c = Case(name)
    model = build_model(c, DEV)
    model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
    model.eval()
    eng = model._require_engine()
    X, y = c.X[:B], c.y[:B]
    bce, reg, grads = eng.loss_and_grads(X.to(DEV), y.to(DEV))
    bce_ref, reg_ref, g_ref = O.loss_and_grads(c.tensors("param"), X, y, c.spec())
    assert bce == pytest.approx(bce_ref, rel=5e-6)
    for k, g in g_ref.items():
        if k not in grads:                           # alias keys share a leaf
            continue
        # with a handful of samples some gradients (the key projections of the last layer: differences of nearly equal
        # softmax terms) are ~1e-5 and carry ~1e-9 of fp32 cancellation noise in ANY fp32 evaluation: absolute floor 5e-9
        scale = max(1e-6, float(g.abs().max()))
        np.testing.assert_allclose(grads[k].cpu().numpy(), g.numpy(), rtol=0, atol=1e-4 * scale + 5e-9, err_msg=k)


@pytest.mark.parametrize("D,H,U,F", [(128, 8, 64, 9), (64, 8, 32, 33), (32, 2, 64, 70), (64, 4, 48, 24), (16, 1, 16, 5)])
def test_general_layer_path_on_shapes_without_a_golden_case(monkeypatch, D, H, U, F):
    """Shapes no recorded case holds and no fused kernel covers - embedding_dim 128 (weight-gradient products in two passes,
    per-product dx), head dimension 8 with more than 32 fields (wavefront attention arms), more than 64 fields at head dimension
    16 (MFMA arms not applicable), a MetaNet width that is not a power of two - through the public API against the oracle:
    logits and every gradient, evaluation mode and training mode with replayed dropout masks, on a ragged batch."""
    monkeypatch.setenv("SATRANS_GENERIC", "1")             # (small batches of these shapes would otherwise go to the LDS kernels)
    _synthetic_shape_against_oracle(D, H, U, F, generic=True)


def test_configs4_shape_against_the_oracle():
    """BASELINE configs[4] at ITS shape - 64 fields, embedding_dim 64, MetaNet hidden 128, 4 heads, 6 layers, int64 ids - on a
    batch the CPU oracle finishes in seconds (B = 256): logits and every gradient, evaluation mode and training mode with the
    kernels' dropout masks replayed through the oracle (the general path picks itself at this shape).
    The oracle runs in fp64 here, so the comparison sees the kernels' fp32 rounding alone: every tensor but a handful agrees to
    1e-6 of its largest element (measured 2e-7 .. 2e-6 on the 64 embedding tables).  The bound is 5e-4 of the tensor's largest
    element - the key / query projections of the deeper layers are sums of 16 k cancelling terms whose result is 1e-3 of the
    terms (measured 4e-4 there) - with at most 1 % of a tensor's elements - the rows of tokens that sit on a ReLU kink of one
    of the 25 M MetaNet hidden units - held to 5e-3."""
    _synthetic_shape_against_oracle(64, 4, 128, 64, generic=True, B=256, L=6, int_ids=True, ref64=True, grad_tol=5e-4,
                                    kink_frac=0.01)


def test_size_independent_properties_at_the_configs4_batch():
    """configs[4] shape at the full batch (8192 samples x 64 int64 fields, D = 64, 6 layers; tables scaled to 2 M rows - their
    size plays no part in these properties), where the oracle is too slow to be the checker - the twin of
    test_size_independent_properties_at_the_baseline_batch on the general path: the gather is a copy, a sample's output does
    not depend on its batch-mates, and two training runs from one seed leave identical bits everywhere."""
    import bench
    cfg = bench.make_config("c5", 2_000_000)
    B = 8192
    X, y = bench.synth_batches(2 * B, 13, cfg=cfg)
    assert X.dtype == np.int64
    Xd, yd = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)

    def fresh():
        m = bench.build_model("cpu", cfg["lr"], cfg=cfg)
        m.to(DEV)
        m.device = DEV
        return m

    m1 = fresh()
    m1.eval()
    eng = m1._require_engine()
    p = m1(Xd[:B])
    assert eng._ws[B]["generic"], "configs[4] runs on the general path"
    rows = Xd[:B] + eng.row_span[:, 0][None, :]
    assert torch.equal(eng.layer_outputs(B)[0], m1.embedding_arena[rows])
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(m1(Xd[:B][perm]), p[perm]), "a sample's output depends on the order of the batch"
    assert torch.equal(m1(Xd[:1000]), p[:1000]), "a sample's output depends on the batch size"
    assert bool(torch.isfinite(p).all()) and float(p.min()) > 0 and float(p.max()) < 1

    def train(m):
        m.train()
        e = m._require_engine()
        for i in range(2):
            e.train_step(Xd[i * B:(i + 1) * B], yd[i * B:(i + 1) * B])
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        return sd, float(e.epoch_sums()[0])

    sd1, loss1 = train(m1)
    del m1, eng
    torch.cuda.empty_cache()
    m2 = fresh()
    sd2, loss2 = train(m2)
    assert loss1 == loss2
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), f"run-to-run difference in {k}"


@pytest.mark.parametrize("F,B", [(3, 50), (7, 21), (13, 64), (20, 21), (25, 33), (32, 21)])
def test_fused_kernels_on_field_counts_without_a_golden_case(F, B):
    """The fused kernels at the AliCCP dimensions (D = 32, 4 heads, hidden 64) for field counts no recorded case has: the tile
    geometry (samples per tile 64 / F: 21 ... 2), the task-to-lane maps of the attention phases and the generic (runtime field
    count) backward instantiation, against the oracle in evaluation and training mode."""
    _synthetic_shape_against_oracle(32, 4, 64, F, generic=False, B=B)


@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos"])
@pytest.mark.parametrize("train", [False, True])
def test_saved_attention_backward_equals_the_recomputing_one(train, name):
    """Saved attention (the default; engine.save_attention = False recomputes; include/satrans_hip.h: satrans_layer_desc.attn_save): the
    forward leaves softmax numerators, 1 / sum, dropout keep words and the attention output per sorted sample position, the
    backward copies them straight into LDS (global_load_lds) instead of running its attention-forward phase.  Same mathematics: every gradient
    within rounding of the recomputing backward (the saved numerators come from the forward kernel's q / k, the recomputed
    ones from the backward's - equal up to the last bit), on the golden batch and on a ragged one that leaves partial tiles.
    `alimama_sota_pos`: separate Q / K generated tables per layer (flag 'pos'), 15 fields (H F < 2 D: the staging area of the hand-over
    is larger than the dS cache it shares LDS with)."""
    c = Case(name)
    outs = []
    for save in (False, True):
        model = build_model(c, DEV)
        model.compile(torch.optim.Adam(model.parameters(), lr=c.meta["lr"]), "binary_crossentropy")
        model.train(train)
        eng = model._require_engine()
        eng.save_attention = save
        res = []
        for B in (c.X.shape[0], 37):
            bce, reg, grads = eng.loss_and_grads(c.X[:B].to(DEV), c.y[:B].to(DEV))
            held = [t is not None for t in eng._ws[B]["attn_save"]]
            # (the last layer runs with the head fused in: no forward launch, nothing saved for it)
            assert held == ([True] * (eng.L - 1) + [False] if save else [False] * eng.L), held
            res.append((bce, {k: g.cpu() for k, g in grads.items()}))
        outs.append(res)
    for (bce0, g0), (bce1, g1) in zip(*outs):
        assert bce0 == pytest.approx(bce1, rel=1e-6)
        for k in g0:
            scale = max(1e-6, float(g0[k].abs().max()))
            np.testing.assert_allclose(g1[k].numpy(), g0[k].numpy(), rtol=0,
                                       atol=2e-5 * scale + softmax_side_floor(k, g0, 1e-9),
                                       err_msg=f"{k} train={train}")


@pytest.mark.parametrize("meta_mode", ["Q", "K", "V"])
def test_fused_kernels_with_one_or_no_modulated_role(meta_mode):
    """The AliCCP layer shape with only the queries, only the keys or neither of them modulated (meta_mode 'Q' / 'K' / 'V': the
    golden cases of these modes are D = 16): one role's MetaNet chain, its weight-gradient products and the shared LayerNorm
    accumulators on the split-product kernels (no MetaNet at all: fp32 products), eval and replayed-mask training."""
    _synthetic_shape_against_oracle(32, 4, 64, 19, generic=False, B=23, meta_mode=meta_mode, ref64=True)


@pytest.mark.parametrize("B", [1, 37, 1024, 3000, 8192])
def test_per_field_sort_equals_the_device_wide_sort(B):
    """satrans_embed_sort_fields (one workgroup per field, LDS radix sort) against satrans_embed_sort and torch's stable sort on
    batches of [B, F] arena rows with heavy duplication, tables of very different sizes and fields out of arena order."""
    import ctypes as C
    from satrans_amd import native as N
    lib = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(B)
    sizes = [3, 70000, 17, 1 << 20, 5000, 2, 300000, 64]               # rows of each field's table
    order = [2, 0, 5, 7, 4, 1, 6, 3]                                   # arena order of the fields
    F = len(sizes)
    lo = [0] * F
    off = 0
    for f in order:
        lo[f] = off
        off += sizes[f]
    total = off
    ids = torch.stack([torch.randint(0, min(sizes[f], 50 if f % 2 else sizes[f]), (B,), generator=g) for f in range(F)], dim=1)
    rows = (ids + torch.tensor(lo)[None, :]).to(torch.int32).contiguous().to(DEV)
    n = B * F
    want_rows, want_src = torch.sort(rows.reshape(-1).cpu(), stable=True)
    Arr = C.c_int32 * F
    out_r, out_s = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    N.check(lib.satrans_embed_sort_fields(rows.data_ptr(), B, F, Arr(*order), Arr(*[lo[f] for f in order]),
                                          Arr(*[sizes[f] for f in order]), out_r.data_ptr(), out_s.data_ptr(), st), "sort_fields")
    assert torch.equal(out_r.cpu(), want_rows) and torch.equal(out_s.cpu().long(), want_src)
    ws = torch.empty(int(lib.satrans_embed_sort_workspace_bytes(n, total)), dtype=torch.uint8, device=DEV)
    ref_r, ref_s = torch.empty_like(out_r), torch.empty_like(out_s)
    N.check(lib.satrans_embed_sort(rows.data_ptr(), n, total, ref_r.data_ptr(), ref_s.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                   None, st), "sort")
    assert torch.equal(out_r, ref_r) and torch.equal(out_s, ref_s)
    # ... and from the id matrix itself (satrans_embed_rows_sort_fields: ids -> rows as satrans_gather_fwd translates them, written
    # on the way, one launch), in the three id dtypes, with the columns permuted and a few ids outside their tables
    cols = torch.randperm(F + 2, generator=g)[:F].to(torch.int32)
    span = torch.tensor([[lo[f], lo[f] + sizes[f]] for f in range(F)], dtype=torch.int64, device=DEV)
    for dt in (torch.int64, torch.int32, torch.float32):
        bad_ids = ids.clone()
        bad_ids[0, 1], bad_ids[B - 1, 3] = -1, sizes[3]                 # out of range: flagged, recorded as the table's first row
        X = torch.zeros(B, F + 2, dtype=dt)
        X[:, cols.long()] = bad_ids.to(dt)
        X = X.to(DEV)
        arena = torch.zeros(4, 16, device=DEV)                           # (rows-only mode never reads it)
        want_rows_m = torch.empty(B, F, dtype=torch.int32, device=DEV)
        status0 = torch.zeros(1, dtype=torch.int32, device=DEV)
        N.check(lib.satrans_gather_fwd(arena.data_ptr(), span.data_ptr(), cols.to(DEV).data_ptr(), X.data_ptr(), N.id_dtype_of(X),
                                       X.stride(0), B, F, 16, None, want_rows_m.data_ptr(), status0.data_ptr(), st), "gather_fwd(rows)")
        N.check(lib.satrans_embed_sort_fields(want_rows_m.data_ptr(), B, F, Arr(*order), Arr(*[lo[f] for f in order]),
                                              Arr(*[sizes[f] for f in order]), ref_r.data_ptr(), ref_s.data_ptr(), st), "sort_fields")
        got_rows_m = torch.full((B, F), -7, dtype=torch.int32, device=DEV)
        status1 = torch.zeros(1, dtype=torch.int32, device=DEV)
        N.check(lib.satrans_embed_rows_sort_fields(X.data_ptr(), N.id_dtype_of(X), X.stride(0), cols.to(DEV).data_ptr(), span.data_ptr(),
                                                   got_rows_m.data_ptr(), B, F, Arr(*order), Arr(*[lo[f] for f in order]),
                                                   Arr(*[sizes[f] for f in order]), out_r.data_ptr(), out_s.data_ptr(),
                                                   status1.data_ptr(), st), "rows_sort_fields")
        assert torch.equal(got_rows_m, want_rows_m) and int(status1.item()) == int(status0.item()) == 1, dt
        assert torch.equal(out_r, ref_r) and torch.equal(out_s, ref_s), dt


@pytest.mark.parametrize("W,n,vocab", [(1, 1000, 50), (2, 5, 3), (4, 70000, 1 << 20), (8, 65536, 400), (8, 65536, 1 << 22), (64, 3000, 97),
                                       (3, 1, 5)])
def test_merge_of_sorted_runs_equals_the_stable_sort(W, n, vocab):
    """satrans_embed_merge_runs (the owner form's sort of what W ranks sent an owner: W sorted runs, ONE ranking launch) against
    torch's stable sort and satrans_embed_sort of the same list: ascending rows, equal rows in position order (rank-major).  Empty
    runs, runs of one element, heavy duplication across runs.  And satrans_embed_inverse_positions against index_put."""
    import ctypes as C
    from satrans_amd import native as N
    lib = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(W * 1000 + n)
    cuts = torch.sort(torch.randint(0, n + 1, (W - 1,), generator=g))[0].tolist() if W > 1 else []
    starts = [0] + cuts + [n]
    if W > 2:
        starts[2] = starts[1]                                    # an empty run
    ids = torch.randint(0, vocab, (n,), generator=g, dtype=torch.int64)
    for q in range(W):
        ids[starts[q]:starts[q + 1]] = torch.sort(ids[starts[q]:starts[q + 1]])[0]
    ids_d = ids.to(torch.int32).to(DEV)
    want_rows, want_src = torch.sort(ids, stable=True)
    out_r, out_s = torch.full((n,), -1, dtype=torch.int32, device=DEV), torch.full((n,), -1, dtype=torch.int32, device=DEV)
    N.check(lib.satrans_embed_merge_runs(ids_d.data_ptr(), n, (C.c_int64 * (W + 1))(*starts), W, out_r.data_ptr(), out_s.data_ptr(), st),
            "merge_runs")
    assert torch.equal(out_r.cpu().long(), want_rows) and torch.equal(out_s.cpu().long(), want_src)
    ws = torch.empty(int(lib.satrans_embed_sort_workspace_bytes(n, vocab)), dtype=torch.uint8, device=DEV)
    ref_r, ref_s = torch.empty_like(out_r), torch.empty_like(out_s)
    N.check(lib.satrans_embed_sort(ids_d.data_ptr(), n, vocab, ref_r.data_ptr(), ref_s.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                   None, st), "sort")
    assert torch.equal(out_r, ref_r) and torch.equal(out_s, ref_s)
    inv = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    N.check(lib.satrans_embed_inverse_positions(out_s.data_ptr(), n, inv.data_ptr(), st), "inverse_positions")
    want_inv = torch.empty(n, dtype=torch.int64)
    want_inv[want_src] = torch.arange(n)
    assert torch.equal(inv.cpu().long(), want_inv)
    # boundaries that do not cover the list are refused
    bad = list(starts)
    bad[-1] = n + 1
    assert lib.satrans_embed_merge_runs(ids_d.data_ptr(), n, (C.c_int64 * (W + 1))(*bad), W, out_r.data_ptr(), out_s.data_ptr(), st) != 0


@pytest.mark.parametrize("F", [15, 19, 32])
@pytest.mark.parametrize("flag", ["sota-gate", "sota-bilinear", "sota-pos"])
def test_fused_variants_at_embedding_dim_32_against_the_oracle(flag, F):
    """flags gate / bilinear / pos at D = 32, H = 4 (the shape the fused kernels hand the attention state over at, and run the
    last layer with the head fused in): logits and every gradient against the oracle, evaluation and training mode (masks
    replayed).  The golden gate / bilinear cases are D = 16, which has neither."""
    _synthetic_shape_against_oracle(32, 4, 64, F, generic=False, B=33, L=3, flag=flag)
