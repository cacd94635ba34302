"""Sibling users of the attention-path kernels: reference SelfAttention_Layer and
BaseModel.meta_transformation.  CPU: the oracle restatements against vectors recorded from the reference's own classes
(oracle/gen_golden_siblings.py).  GPU: satrans_amd.layers (HIP launches behind torch.autograd.Function) against the same
vectors, forward and every gradient."""
import ast
import os

import numpy as np
import pytest
import torch

from oracle import satrans_oracle as O
from tests.helpers import GOLDEN, SIBLING_METANET, SIBLING_SELFATT


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = ast.literal_eval(str(z["meta"]))
    P = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}
    G = {k[5:]: z[k] for k in z.files if k.startswith("grad/")}
    return z, meta, P, G


def close(got, want, rel, msg):
    scale = max(1e-6, float(np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=rel * scale + 1e-9, err_msg=msg)


@pytest.mark.parametrize("name", SIBLING_SELFATT)
def test_oracle_selfattention_matches_reference(name):
    z, m, P, G = load(name)
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    y, att = O.selfattention_layer(leaves, x, m["H"], m["use_res"], m["scaling"])
    close(y.detach().numpy(), z["y"], 2e-6, "y")
    close(att.detach().numpy(), z["att"], 2e-6, "att")
    (y * torch.from_numpy(z["w"])).sum().backward()
    close(x.grad.numpy(), G["x"], 2e-5, "grad x")
    for k, g in G.items():
        if k != "x":
            close(leaves[k].grad.numpy(), g, 2e-5, k)
    assert "W_Out" not in G                       # a parameter the reference never uses


@pytest.mark.parametrize("name", SIBLING_METANET)
def test_oracle_meta_transformation_matches_reference(name):
    z, m, P, G = load(name)
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    y = O.meta_transformation(leaves, torch.from_numpy(z["ids"]), x, [m["D"], m["U"], m["D"]], m["use_norm"])
    close(y.detach().numpy(), z["y"], 2e-6, "y")
    (y * torch.from_numpy(z["w"])).sum().backward()
    close(x.grad.numpy(), G["x"], 2e-5, "grad x")
    for k, g in G.items():
        if k != "x":
            close(leaves[k].grad.numpy(), g, 2e-5, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SIBLING_SELFATT)
def test_selfattention_layer_on_the_gpu_matches_reference(name):
    from satrans_amd import SelfAttention_Layer
    z, m, P, G = load(name)
    torch.manual_seed(7)                          # the reference's creation order and init: same seed, same parameters
    layer = SelfAttention_Layer(m["D"], head_num=m["H"], use_res=m["use_res"], scaling=m["scaling"])
    for k, v in layer.state_dict().items():
        assert torch.equal(v, P[k]), f"seeded parameter {k} differs from the reference's"
    layer.to("cuda:0")
    x = torch.from_numpy(z["x"]).to("cuda:0")
    layer.eval()
    layer.capture_attention = True
    y = layer(x)
    close(y.detach().cpu().numpy(), z["y"], 1e-5, "y")
    close(layer.normalized_att_scores.cpu().numpy(), z["att"], 2e-6, "att")
    layer.capture_attention = False
    xg = x.clone().requires_grad_(True)
    (layer(xg) * torch.from_numpy(z["w"]).to("cuda:0")).sum().backward()      # eval mode = dropout off, like the recorded step
    close(xg.grad.cpu().numpy(), G["x"], 5e-5, "grad x")
    grads = {k: p.grad for k, p in layer.named_parameters()}
    for k, g in G.items():
        if k != "x":
            close(grads[k].cpu().numpy(), g, 5e-5, k)
    assert grads["W_Out"] is None
    # training mode: dropout on, deterministic for a (seed, step), different from eval
    layer.train()
    y1 = layer(x)
    assert not torch.equal(y1, y) and torch.isfinite(y1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SIBLING_METANET)
def test_meta_transformation_on_the_gpu_matches_reference(name):
    from satrans_amd import MetaTransformation
    z, m, P, G = load(name)
    mod = MetaTransformation(m["D"], m["S"] - 1, (m["D"], m["U"], m["D"]), use_norm=m["use_norm"])
    sd = {"domain_embeddings.weight": P["domain_embeddings.weight"], "domain_map_dnn.weight": P["domain_map_dnn.weight"],
          "domain_map_dnn.bias": P["domain_map_dnn.bias"]}
    if m["use_norm"]:
        sd["ffn_layer_norm.weight"], sd["ffn_layer_norm.bias"] = P["ffn_layer_norm.weight"], P["ffn_layer_norm.bias"]
    mod.load_state_dict(sd)
    mod.to("cuda:0")
    mod.eval()
    ids = torch.from_numpy(z["ids"]).to("cuda:0")
    x = torch.from_numpy(z["x"]).to("cuda:0")
    y = mod(ids, x)
    close(y.detach().cpu().numpy(), z["y"], 1e-5, "y")
    xg = x.clone().requires_grad_(True)
    (mod(ids, xg) * torch.from_numpy(z["w"]).to("cuda:0")).sum().backward()
    close(xg.grad.cpu().numpy(), G["x"], 5e-5, "grad x")
    grads = {k: p.grad for k, p in mod.named_parameters()}
    for k, g in G.items():
        if k != "x":
            close(grads[k].cpu().numpy(), g, 5e-5, k)


@pytest.mark.gpu
@pytest.mark.parametrize("D,U", [(16, 16), (16, 48), (32, 32), (32, 128), (64, 16), (64, 96), (64, 128), (128, 16), (128, 64)])
@pytest.mark.parametrize("use_norm", [True, False])
def test_meta_transformation_shape_sweep_against_the_oracle(D, U, use_norm):
    """The general-path products behind MetaTransformation (register-direct MFMA products for every K / 16, N / 16 in 1..8,
    weight-gradient products of the 1x1, 1x2 and 2x1 block forms) on shapes no golden case holds: forward and every gradient
    against the oracle's meta_transformation - itself pinned to the reference by the recorded vectors above - on a ragged
    batch with uneven, partly empty scenario segments."""
    from satrans_amd import MetaTransformation
    g = torch.Generator().manual_seed(1000 + 7 * D + U)
    S, B, F = 5, 37, 11
    mod = MetaTransformation(D, S - 1, (D, U, D), use_norm=use_norm)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.ndim > 1 else 0.1))
        if use_norm:
            mod.ffn_layer_norm.weight.copy_(1.0 + 0.2 * torch.randn(D, generator=g))
    P = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    ids = torch.tensor([0, 1, 3, 3, 1, 0, 3] * 6)[:B]                     # scenario 2 and 4 stay empty
    x = torch.randn(B, F, D, generator=g)
    w = torch.randn(B, F, D, generator=g)
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xr = x.clone().requires_grad_(True)
    y_ref = O.meta_transformation(leaves, ids, xr, [D, U, D], use_norm)
    (y_ref * w).sum().backward()
    mod.to("cuda:0")
    mod.eval()
    xg = x.to("cuda:0").requires_grad_(True)
    y = mod(ids.to("cuda:0"), xg)
    close(y.detach().cpu().numpy(), y_ref.detach().numpy(), 2e-5, "y")
    (y * w.to("cuda:0")).sum().backward()
    close(xg.grad.cpu().numpy(), xr.grad.numpy(), 1e-4, "grad x")
    for k, p in mod.named_parameters():
        want = leaves[k].grad
        assert want is not None, k
        close(p.grad.cpu().numpy(), want.numpy(), 1e-4, k)


# ---- the siblings' oracle in training mode and its kink probe (test infrastructure; no GPU) -------------------------------------
def _small_selfatt(seed=3, B=4, F=7, D=16):
    g = torch.Generator().manual_seed(seed)
    P = {k: torch.randn(D, D, generator=g, dtype=torch.float64) * 0.3 for k in ("W_Query", "W_Key", "W_Value", "W_Res")}
    P["layer_norm.weight"] = 1.0 + 0.2 * torch.randn(D, generator=g, dtype=torch.float64)
    P["layer_norm.bias"] = 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    return P, torch.randn(B, F, D, generator=g, dtype=torch.float64)


def _small_metanet(seed=4, B=6, F=5, D=16, U=32, S=3):
    g = torch.Generator().manual_seed(seed)
    P = {"domain_embeddings.weight": torch.randn(S, D, generator=g, dtype=torch.float64),
         "domain_map_dnn.weight": torch.randn(2 * D * U, D, generator=g, dtype=torch.float64) * 0.3,
         "domain_map_dnn.bias": torch.randn(2 * D * U, generator=g, dtype=torch.float64) * 0.1,
         "ffn_layer_norm.weight": torch.ones(D, dtype=torch.float64), "ffn_layer_norm.bias": torch.zeros(D, dtype=torch.float64)}
    return P, torch.tensor([0, 2, 2, 1, 0, 2])[:B], torch.randn(B, F, D, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("H", [1, 2])
def test_oracle_selfattention_replays_the_sibling_masks(H):
    P, x = _small_selfatt()
    B, F, D = x.shape
    y0, a0 = O.selfattention_layer(P, x, H)
    masks = O.sibling_dropout_masks(1234, 1, B, F, D, H)
    assert masks[(0, "attn")].shape == (H, B, F, F) and masks[(0, "out")].shape == (B, F, D)
    for m in masks.values():                          # keep -> 1 / (1 - p), drop -> 0, about one in ten dropped
        assert set(np.unique(m.numpy())) == {np.float32(0.0), np.float32(1.0 / 0.9)}
    y1, a1 = O.selfattention_layer(P, x, H, drop=O.Dropper("masks", 0.1, masks))
    assert not torch.equal(y1, y0) and torch.isfinite(y1).all()
    assert torch.equal(a1, a0 * masks[(0, "attn")].double())
    # the mask of head h, sample b is the layer's [b, h] one: element index (h F + i) * pad4(F) + j of sample b
    h, b, i, j = H - 1, 2, 3, 5
    keep = O.dropout_keep(1234, 1, 0, 2, np.uint32(b), np.uint32((h * F + i) * ((F + 3) & ~3) + j), 0.1)
    assert bool(keep) == bool(masks[(0, "attn")][h, b, i, j] > 0)
    y2, _ = O.selfattention_layer(P, x, H, drop=O.Dropper("masks", 0.1, O.sibling_dropout_masks(1234, 2, B, F, D, H)))
    assert not torch.equal(y2, y1)                    # the next step: other masks
    ones = {k: torch.ones_like(m) for k, m in masks.items()}
    y3, a3 = O.selfattention_layer(P, x, H, drop=O.Dropper("masks", 0.1, ones))
    assert torch.equal(y3, y0) and torch.equal(a3, a0)


@pytest.mark.parametrize("use_norm", [True, False])
def test_oracle_meta_transformation_replays_the_sibling_masks(use_norm):
    P, ids, x = _small_metanet()
    B, F, D = x.shape
    y0 = O.meta_transformation(P, ids, x, [D, 32, D], use_norm)
    masks = O.sibling_dropout_masks(99, 1, B, F, D)
    y1 = O.meta_transformation(P, ids, x, [D, 32, D], use_norm, drop=O.Dropper("masks", 0.1, masks))      # (raised KeyError 'meta_q')
    assert not torch.equal(y1, y0) and torch.isfinite(y1).all()
    if not use_norm:                                  # y - x = mask * (the MetaNet's output): zero exactly where dropped
        dropped = masks[(0, "metaQ")] == 0
        assert dropped.any() and torch.equal((y1 - x)[dropped], torch.zeros(int(dropped.sum()), dtype=torch.float64))
    ones = {k: torch.ones_like(m) for k, m in masks.items()}
    assert torch.equal(O.meta_transformation(P, ids, x, [D, 32, D], use_norm, drop=O.Dropper("masks", 0.1, ones)), y0)


def test_sibling_kink_probe_counts_planted_elements_and_changes_nothing():
    # self-attention with W_Value = 0 and W_Res = 1: t = x
    P, x = _small_selfatt()
    D = x.shape[-1]
    P["W_Value"] = torch.zeros(D, D, dtype=torch.float64)
    P["W_Res"] = torch.eye(D, dtype=torch.float64)
    x[0, 0, 0], x[1, 2, 3], x[2, 4, 5] = 1e-7, -2e-7, 0.0          # two within 2e-6 * max|t| of the kink; an exact zero is not one
    assert float(x.abs().max()) > 1.0 and int(((x.abs() < 1e-5) & (x != 0)).sum()) == 2
    assert O.SIBLING_KINK_PROBE is None
    off = O.selfattention_layer(P, x, 2)
    O.SIBLING_KINK_PROBE = {"eps": 2e-6, "near_zero": 0}
    try:
        on = O.selfattention_layer(P, x, 2)
        assert O.SIBLING_KINK_PROBE["near_zero"] == 2
        # MetaNet with W1 = 1 (bias of the scenario encoder, weight 0): hidden = x
        Pm, ids, xm = _small_metanet(D=16, U=16)
        Pm["domain_map_dnn.weight"] = torch.zeros_like(Pm["domain_map_dnn.weight"])
        Pm["domain_map_dnn.bias"][:256] = torch.eye(16, dtype=torch.float64).reshape(-1)
        xm[3, 1, 2] = 3e-7
        O.SIBLING_KINK_PROBE["near_zero"] = 0
        m_on = O.meta_transformation(Pm, ids, xm, [16, 16, 16], True)
        assert O.SIBLING_KINK_PROBE["near_zero"] == 1
    finally:
        O.SIBLING_KINK_PROBE = None
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert torch.equal(O.meta_transformation(Pm, ids, xm, [16, 16, 16], True), m_on)
