"""VarLenSparseFeat against fixtures recorded from the reference's own SATrans (tests/golden/varlen/, tools/gen_varlen_golden.py):
construction (CPU), and the product's probabilities, gradients and Adam steps on the MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from tests import varlen_reference as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "varlen")
CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz"))
DEV = "cuda:0"
# Gradient tolerance, relative to a tensor's largest element.  5e-5 is the golden gradient bound of the existing cases.  A batch
# with an all-padding `max` list carries -1e9 tokens through the layers; the fp32 reference's own rounding noise there, measured
# as the worst fp32-vs-fp64 difference of tests/varlen_reference.py over five seeds (48 samples, every third list empty):
# 1.5e-4 (max), 8.2e-5 (max + dense), 6.7e-5 (sum beside a max field) - against 2.1e-5 .. 3.6e-5 without empty lists.
GRAD_REL, GRAD_REL_EMPTY_MAX = 5e-5, 5e-4


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def prefixed(z, prefix):
    return {k[len(prefix) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix + "/")}


def build(meta, device):
    from satrans_amd import SATrans
    from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    D = meta["D"]
    cols = [SparseFeat(f, v, embedding_dim=D) for f, v in zip(meta["sparse"], meta["vocab"])]
    cols += [VarLenSparseFeat(SparseFeat(v["name"], v["vocab"], embedding_dim=D), maxlen=v["maxlen"], combiner=v["combiner"],
                              length_name=v["length_name"]) for v in meta["varlen"]]
    cols += [DenseFeat(f, 1) for f in meta["dense"]]
    return SATrans(linear_feature_columns=cols, dnn_feature_columns=cols, domain_column_list=meta["domain"],
                   num_domains_list=meta["num_domains_list"], att_layer_num=0, domain_att_layer_num=meta["L"],
                   att_head_num=meta["H"], share_domain_dnn_across_layers=False, use_domain_dnn_linear=False, use_linear=False,
                   meta_mode=meta["mode"], use_dnn=False, meta_dnn_hidden_units=tuple(meta["units"]), seed=meta["seed"],
                   device=device, flag=meta["flag"])


def grad_rel(model, X):
    """GRAD_REL_EMPTY_MAX when the batch holds an all-padding `max` list, else GRAD_REL."""
    _, vs = V.spec_of(model)
    empty_max = any(bool((V.slot_mask(X, v).sum(1) == 0).any()) for v in vs if v.combiner == "max")
    return GRAD_REL_EMPTY_MAX if empty_max else GRAD_REL


def test_fixtures_are_present_and_small():
    assert set(CASES) == {"varlen_sum", "varlen_mean", "varlen_max", "varlen_length", "varlen_dense"}
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, c + ".npz")) < 400_000


@pytest.mark.parametrize("name", CASES)
def test_construction_is_bit_identical_to_the_reference(name):
    """Same seed, same generator draws: embedding_dict (sparse then varlen), linear_model, every layer - bit for bit, and the
    same keys and shapes (dnn_linear sized by len(embedding_dict), the varlen tables counted)."""
    z, meta = load(name)
    model = build(meta, "cpu")
    want = prefixed(z, "param")
    sd = model.state_dict()
    aliases = {k[6:] for k in z.files if k.startswith("alias/")}
    assert set(want) | aliases == set(sd), set(want) ^ set(sd)
    for k, w in want.items():
        assert torch.equal(sd[k], w), k


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    """tests/varlen_reference.py (fp32) on the recorded parameters gives the reference's probabilities, losses and gradients: the
    composition of the unchanged oracle with the pooling is the reference's model, regulariser over the varlen tables included."""
    z, meta = load(name)
    model = build(meta, "cpu")
    spec, vs = V.spec_of(model)
    P = V.params(model, torch.float32)                           # (aliased keys stay one tensor)
    X, y = torch.from_numpy(z["X"]), torch.from_numpy(z["y"])
    prob, _ = V.forward(P, X, spec, vs)
    np.testing.assert_allclose(prob.numpy(), z["out/prob"], rtol=0, atol=2e-6)
    bce, reg, grads = V.loss_and_grads(P, X, y, spec, vs)
    assert bce == pytest.approx(float(z["train/bce"]), rel=1e-6)
    assert reg == pytest.approx(float(z["train/reg"]), rel=1e-6)
    for k, g in prefixed(z, "grad").items():
        s = max(1e-6, float(g.abs().max()))
        np.testing.assert_allclose(grads[k].numpy(), g.numpy(), rtol=0, atol=1e-5 * s + 1e-9, err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_product_matches_the_reference(name):
    """Probabilities (2e-6, as the existing golden forward checks), BCE, regulariser, every gradient (GRAD_REL of its largest
    element, GRAD_REL_EMPTY_MAX with an all-padding max list: measured above) and two Adam steps (the bounds of
    test_adam_steps_match_reference_golden)."""
    z, meta = load(name)
    model = build(meta, DEV)
    model.eval()
    X, y = torch.from_numpy(z["X"]), torch.from_numpy(z["y"])
    prob = model(X.to(DEV)).cpu()
    np.testing.assert_allclose(prob.numpy(), z["out/prob"], rtol=0, atol=2e-6)
    model.compile(torch.optim.Adam(model.parameters(), lr=meta["lr"]), "binary_crossentropy")
    eng = model._require_engine()
    bce, reg, grads = eng.loss_and_grads(X.to(DEV), y.to(DEV))
    assert abs(bce - float(z["train/bce"])) <= 2e-6 * abs(float(z["train/bce"]))
    assert reg == pytest.approx(float(z["train/reg"]), rel=1e-5)
    rel = grad_rel(model, X)
    gold = prefixed(z, "grad")
    for k, g in gold.items():
        assert k in grads, k
        s = max(1e-6, float(g.abs().max()))
        np.testing.assert_allclose(grads[k].cpu().numpy(), g.numpy(), rtol=0, atol=rel * s + 1e-9, err_msg=k)
    steps, lr = meta["adam_steps"], meta["lr"]
    for _ in range(steps):
        eng.train_step(X.to(DEV), y.to(DEV))
    got = model.state_dict()
    init = prefixed(z, "param")
    for k, w in prefixed(z, "adam").items():
        err = (got[k].detach().cpu() - w).abs().flatten().double()
        assert float(err.max()) <= 2.0 * lr * steps + 1e-6, (k, float(err.max()))
        if k in gold and float(gold[k].abs().max()) >= 1e-7 and float((w - init[k]).abs().max()) > 0:
            assert float(err.median()) <= 2e-3 * lr * steps, (k, float(err.median()))
