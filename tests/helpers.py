"""Fixture loading shared by the CPU and GPU tests (test infrastructure)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import satrans_oracle as O
from oracle.satrans_oracle import PathSpec

DEV = "cuda:0"

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and not f.startswith("sibling_"))
SIBLING_SELFATT = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("sibling_selfatt"))
SIBLING_METANET = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("sibling_metanet"))
TRAIN_CASES = [c for c in ALL_CASES if c != "small_relu"]


class Case:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        self.z = z
        self.meta = json.loads(str(z["meta"]))
        self.X = torch.from_numpy(z["X"])
        self.y = torch.from_numpy(z["y"])

    def tensors(self, prefix, dtype=torch.float32):
        """state_dict-shaped dict; aliased keys share ONE tensor object, as in the reference."""
        out = {k[len(prefix) + 1:]: torch.from_numpy(self.z[k]).to(dtype) for k in self.z.files
               if k.startswith(prefix + "/")}
        for k in self.z.files:
            if k.startswith("alias/"):
                out[k[6:]] = out[str(self.z[k])]
        return out

    def arrays(self, prefix):
        return {k[len(prefix) + 1:]: self.z[k] for k in self.z.files if k.startswith(prefix + "/")}

    def spec(self) -> PathSpec:
        m = self.meta
        col = {n: i for i, n in enumerate(m["feature_names"])}
        return PathSpec(
            sparse=[(f, col[f]) for f in m["fields"]],
            dense=[(col[f], col[f] + 1) for f in m["dense"]],
            domain_cols=[col[c] for c in m["domain"]],
            embedding_dim=m["D"], head_num=m["H"], layer_num=m["L"], flag=m["flag"], meta_mode=m["mode"],
            meta_units=[m["D"]] + list(m["units"]),
            multi_domain_sparse=[(f, col[f]) for f in m["fields"] if f in m["domain"]],
        )

    def columns(self):
        """Feature columns of the product package for this case (reference main.py:182-191)."""
        from satrans_amd.inputs import SparseFeat, DenseFeat
        m = self.meta
        return [SparseFeat(f, vocabulary_size=v, embedding_dim=m["D"]) for f, v in zip(m["fields"], m["vocab"])] + \
               [DenseFeat(f, 1) for f in m["dense"]]


def build_model(case: "Case", device: str):
    """The product model for a golden case, constructed the way reference main.py:292-306 does."""
    from satrans_amd import SATrans
    m = case.meta
    cols = case.columns()
    model = SATrans(linear_feature_columns=cols, dnn_feature_columns=cols, domain_column_list=list(m["domain"]),
                    num_domains_list=m["num_domains_list"], att_layer_num=0, domain_att_layer_num=m["L"],
                    att_head_num=m["H"], share_domain_dnn_across_layers=False, use_domain_dnn_linear=False,
                    use_linear=False, meta_mode=m["mode"], use_dnn=False, meta_dnn_hidden_units=tuple(m["units"]),
                    seed=m["seed"], device=device, flag=m["flag"])
    return model


def _adam_steps(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"]))["adam_steps"]


ADAM_CASES = [c for c in TRAIN_CASES if _adam_steps(c) > 0]     # cases that carry parameters / moments after Adam steps
NATIVE_CASES = list(ALL_CASES)
NATIVE_TRAIN_CASES = [c for c in NATIVE_CASES if c in TRAIN_CASES]
NATIVE_ADAM_CASES = [c for c in NATIVE_CASES if c in ADAM_CASES]


def softmax_side_floor(key, grads, floor):
    """Absolute floor of a gradient bound.  W_Query / W_Key sit upstream of the softmax: their gradients are differences of nearly
    equal terms (the softmax is shift-invariant) and come out ~1e-3 of their layer's W_Value gradient, while what perturbs them
    is NOT scaled down with them - the rounding of the cancelling terms, and above all a MetaNet ReLU whose pre-activation is
    within rounding of zero and takes the other branch than the oracle's, which changes one token's dq / dk by O(1) of that token's
    share and reaches every element of the 32 x 32 matrix (seen as "half of the elements off by 1e-7" whenever a mask
    realisation puts a unit on its kink; masks, forward outputs and all other tensors agree to 1e-7 then).  Their floor is
    therefore 2e-4 of the same layer's W_Value gradient; every other tensor keeps `floor`."""
    for side in ("W_Query", "W_Key"):             # "<layer>.W_Query" of the model, bare "W_Query" of SelfAttention_Layer
        if key == side or key.endswith("." + side):
            ref = grads.get(key[:-len(side)] + "W_Value")
            if ref is not None:
                return max(floor, 1e-3 * float(torch.as_tensor(ref).abs().max()))
    return floor


def assert_grad_close_but_for_kinks(got, want, atol, err_msg, frac=0.02, outlier=0.05, kinks=None):
    """Gradient comparison of a TRAINING-mode step against the oracle (replayed dropout masks).  Element by element within `atol`,
    except where a MetaNet ReLU on its kink may have taken the other branch than the oracle's: one hidden unit of one token then
    contributes - or does not - to the rows / columns of the generated-weight gradient it touches and to everything downstream
    of them (measured: 440 of 131,072 elements of the scenario encoder's weight gradient, the largest 1.5 % of the tensor's
    largest entry).  The exception - at most `frac` of a tensor's elements outside `atol`, none of them by more than `outlier`
    of the tensor's largest entry - is granted ONLY when the oracle itself saw a hidden unit within fp32 rounding of the kink on
    these very inputs (`kinks` = the count of oracle_grads_probing_kinks; None / 0: element-wise)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    bad = err > atol
    if not bad.any():
        return
    if not kinks:
        np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=0, atol=atol,
                                   err_msg=err_msg)
    assert float(bad.mean()) <= frac, (err_msg, "fraction outside the bound", float(bad.mean()))
    assert float(err.max()) <= outlier * float(np.abs(want).max()) + atol, (err_msg, float(err.max()), float(np.abs(want).max()))


WORST = {}      # largest err / bound-scale seen per (tag, quantity) in this process; printed as it grows


def check_close(tag, got, want, rel, msg, what="y", floor=0.0):
    """Element-wise: |got - want| <= rel * max|want| + floor; the largest ratio seen is printed under `tag`."""
    want = want.double()
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    key, ratio = (tag, f"{what} err / max"), err / max(scale, 1e-30)
    if ratio > WORST.get(key, -1.0):
        WORST[key] = ratio
        print(f"[{tag}] largest {key[1]} so far: {ratio:.3e} ({msg})")
    assert err <= rel * scale + floor, (msg, what, err, scale)


def note_worst(tag, what, ratio, msg):
    """Keep and print the largest `ratio` seen under (tag, what) in this process (the figures the module docstrings quote)."""
    if tag is not None and ratio > WORST.get((tag, what), -1.0):
        WORST[(tag, what)] = ratio
        print(f"[{tag}] largest {what} so far: {ratio:.3e} ({msg})")


def oracle_grads_probing_kinks(state, X, y, spec, drop=None, eps=2e-6):
    """O.loss_and_grads plus the number of MetaNet hidden units whose pre-activation the oracle saw within `eps` (relative to the
    largest pre-activation of its product) of the ReLU's kink: fp32 products of 32 / 64 terms differ by a few 1e-7 of that
    scale between two evaluation orders, so only such a unit can take one branch in the kernels and the other in the oracle."""
    O.KINK_PROBE = {"eps": eps, "near_zero": 0}
    try:
        out = O.loss_and_grads(state, X, y, spec, drop)
        return out, int(O.KINK_PROBE["near_zero"])
    finally:
        O.KINK_PROBE = None


class SyntheticModel:
    """A seeded synthetic model through the public API, built on the CPU, and the same parameters as a state_dict-shaped dict
    for the oracle (aliased keys one tensor): the construction of synthetic_shape_against_oracle - SATrans(..., seed='1021')
    behind torch.manual_seed(3), embedding parameters x `emb` - with three additions.  Every LayerNorm vector is redrawn
    (weight 1 + 0.2 n, bias 0.1 n: at their initial 1 / 0 the Q-side and K-side vectors are equal and a kernel that read the
    wrong one would go unnoticed), the scenario encoder's weight is scaled by `gen`, and `n_dense` DenseFeat columns may follow
    the sparse ones.  `scen_ids`: the scenario column (ids 1..3; id 0 stays unused); `seed`: of the other id columns;
    `vocab`: range the fields' vocabulary sizes are drawn from.  Nothing here needs a device;
    on_device() moves the model there and returns its engine."""

    def __init__(self, D, H, U, F, L=2, flag="sota", meta_mode="QK", scen_ids=None, B=21, n_dense=0, emb=300.0, gen=1.0, seed=0, vocab=(5, 60)):
        from satrans_amd import SATrans, SparseFeat, DenseFeat
        rng = np.random.RandomState(D + F)
        self.fields = [f"f{i}" for i in range(F)]
        vocab = {f: int(rng.randint(*vocab)) for f in self.fields}
        vocab[self.fields[0]] = 4                              # the scenario column: ids 1..3
        self.dense = [f"d{i}" for i in range(n_dense)]
        cols = [SparseFeat(f, vocabulary_size=vocab[f] + 1, embedding_dim=D) for f in self.fields] + \
               [DenseFeat(f, 1) for f in self.dense]
        torch.manual_seed(3)
        model = SATrans(cols, cols, [self.fields[0]], [3], att_layer_num=0, domain_att_layer_num=L, att_head_num=H,
                        use_linear=False, use_dnn=False, meta_mode=meta_mode, meta_dnn_hidden_units=(U, D), seed='1021',
                        device='cpu', flag=flag)
        gen_ = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for k, p in model.named_parameters():
                if "embedding" in k:
                    p.mul_(emb)
                elif k.endswith("layer_norm.weight"):
                    p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=gen_))
                elif k.endswith("layer_norm.bias"):
                    p.copy_(0.1 * torch.randn(p.shape, generator=gen_))
                elif k == "domain_map_dnn_Q.linears.0.weight":
                    p.mul_(gen)
        by_ptr = {}
        self.state = {k: by_ptr.setdefault(v.data_ptr(), v.detach().clone()) for k, v in model.state_dict().items()}
        if scen_ids is not None:
            B = len(scen_ids)
        rng = np.random.RandomState(1000 * seed + D + F)       # `seed`: another id matrix for the same model
        X = np.stack([rng.randint(1 if f == self.fields[0] else 0, vocab[f], size=B) for f in self.fields], axis=1).astype(np.float32)
        if scen_ids is not None:
            X[:, 0] = np.asarray(scen_ids, dtype=np.float32)
        if n_dense:
            X = np.concatenate([X, rng.rand(B, n_dense).astype(np.float32)], axis=1)
        self.X = torch.from_numpy(X)
        self.spec = O.PathSpec(sparse=[(f, i) for i, f in enumerate(self.fields)], dense=[(F + i, F + i + 1) for i in range(n_dense)],
                               domain_cols=[0], embedding_dim=D, head_num=H, layer_num=L, flag=flag, meta_mode=meta_mode,
                               meta_units=[D, U, D])
        self.model, self.eng = model, None

    def on_device(self):
        model = self.model
        model.to(DEV)
        model.device = DEV
        model.compile("adam", "binary_crossentropy")
        model.eval()
        self.eng = model._require_engine()
        return self.eng


def synthetic_shape_against_oracle(D, H, U, F, generic, B=21, L=2, int_ids=False, ref64=False, grad_tol=2e-4, kink_frac=0.0,
                                   meta_mode='QK', flag='sota', scen_ids=None, first_scen_ids=None, check_attention=False,
                                   route_check=None, tag=None):
    """A synthetic model of layer shape (D, H, U, F) through the public API against the oracle: logits, BCE and every gradient, in
    evaluation mode and in training mode with the kernels' dropout masks replayed through the oracle.
    `scen_ids` ([B] ids in 1..3): the scenario column, instead of the uniform draw.  `first_scen_ids`: before every compared step
    the same engine runs a step on ANOTHER batch of the same size with these scenario ids (what a step leaves behind in the
    workspace must not reach the next one).  `check_attention`: each layer's normalized_att_scores against the oracle's, in both
    modes.  `route_check(eng, B)`: called before the first kernel runs.  `tag`: print the largest errors under this name."""
    from satrans_amd import SATrans, SparseFeat
    rng = np.random.RandomState(D + F)
    fields = [f"f{i}" for i in range(F)]
    vocab = {f: int(rng.randint(5, 60)) for f in fields}
    vocab[fields[0]] = 4                                   # the scenario column: ids 1..3
    cols = [SparseFeat(f, vocabulary_size=vocab[f] + 1, embedding_dim=D) for f in fields]
    torch.manual_seed(3)
    model = SATrans(cols, cols, [fields[0]], [3], att_layer_num=0, domain_att_layer_num=L, att_head_num=H, use_linear=False,
                    use_dnn=False, meta_mode=meta_mode, meta_dnn_hidden_units=(U, D), seed='1021', device='cpu', flag=flag)
    with torch.no_grad():                                  # weights far enough from zero for every gradient to matter
        for k, p in model.named_parameters():
            if "embedding" in k:
                p.mul_(300.0)
    sd = model.state_dict()
    state, by_ptr = {}, {}
    for k, v in sd.items():                                # keep the reference's aliasing (K_meta_mlp is Q_meta_mlp without 'pos')
        state[k] = by_ptr.setdefault(v.data_ptr(), v.detach().clone())
    X = np.stack([rng.randint(1 if f == fields[0] else 0, vocab[f], size=B) for f in fields], axis=1).astype(np.float32)
    y = (rng.rand(B) < 0.4).astype(np.float32)
    if scen_ids is not None:
        X[:, 0] = np.asarray(scen_ids, dtype=np.float32)
    X_first = None
    if first_scen_ids is not None:                         # another batch of the same size (its own generator: X, y stay what they were)
        rng1 = np.random.RandomState(1000 + D + F)
        X_first = np.stack([rng1.randint(0, vocab[f], size=B) for f in fields], axis=1).astype(np.float32)
        X_first[:, 0] = np.asarray(first_scen_ids, dtype=np.float32)
        y_first = torch.from_numpy((rng1.rand(B) < 0.4).astype(np.float32))
        X_first = torch.from_numpy(X_first)
    spec = O.PathSpec(sparse=[(f, i) for i, f in enumerate(fields)], dense=[], domain_cols=[0], embedding_dim=D, head_num=H,
                      layer_num=L, flag=flag, meta_mode=meta_mode, meta_units=[D, U, D])
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    Xg = Xt.long() if int_ids else Xt                     # the id matrix as the kernels get it (int64: SATRANS_ID_I64)
    if ref64:                                             # the oracle in fp64: the difference is then the kernels' rounding alone
        conv = {}
        state = {k: conv.setdefault(id(v), v.double()) for k, v in state.items()}
    model.to(DEV); model.device = DEV
    model.compile("adam", "binary_crossentropy")
    if route_check is not None:
        route_check(model._require_engine(), B)
    for train in (False, True):
        model.train(train)
        eng = model._require_engine()
        if X_first is not None:
            eng.loss_and_grads((X_first.long() if int_ids else X_first).to(DEV), y_first.to(DEV))
        bce, reg, grads = eng.loss_and_grads(Xg.to(DEV), yt.to(DEV))
        assert bool(eng._ws[B]["generic"]) == generic, "unexpected layer path"
        drop = O.Dropper("masks", 0.1, O.dropout_masks(eng.drop_seed, eng.drop_step, B, F, D, H, L, 0.1)) if train else None
        (bce_ref, reg_ref, g_ref), kinks = oracle_grads_probing_kinks(state, Xt, yt, spec, drop)
        if not train:
            model(Xg.to(DEV))
            _, logit_ref = O.forward(state, Xt, spec)
            note_worst(tag, "logit err / max(1, |logit|)", float((eng.last_logit().cpu().double().reshape(-1) - logit_ref.double().reshape(-1))
                                                                 .abs().max()) / max(1.0, float(logit_ref.abs().max())), f"F={F} B={B}")
            np.testing.assert_allclose(eng.last_logit().cpu().numpy().reshape(-1), logit_ref.float().numpy().reshape(-1), rtol=0,
                                       atol=2e-5 * max(1.0, float(logit_ref.abs().max())))
        note_worst(tag, "BCE rel err", abs(bce - bce_ref) / abs(bce_ref), f"F={F} B={B} train={train}")
        assert bce == pytest.approx(bce_ref, rel=1e-5)
        for k, g in g_ref.items():
            if k in grads:
                scale = max(1e-6, float(g.abs().max()))
                got_g, want_g = grads[k].cpu().numpy().astype(np.float64), g.double().numpy()
                note_worst(tag, "gradient err / max|g|", float(np.abs(got_g - want_g).max()) / scale,
                           f"{k} F={F} B={B} train={train} kinks={kinks}")
                if kink_frac > 0:
                    # ReLU kinks: a MetaNet hidden unit whose pre-activation is within rounding of zero takes one branch here and
                    # the other in the oracle (any two evaluation orders do that to each other); its dh then reaches - or does not
                    # reach - the rows of ONE token.  With tens of millions of hidden units per step a few such tokens are certain,
                    # so a small fraction of a tensor's elements is held to 10x the bound only.
                    err = np.abs(got_g - want_g)
                    assert float((err > grad_tol * scale + 1e-8).mean()) <= kink_frac, (k, train, float((err > grad_tol * scale + 1e-8).mean()))
                    assert float(err.max()) <= 10 * grad_tol * scale + 1e-8, (k, train, float(err.max()), scale)
                    continue
                if train:
                    assert_grad_close_but_for_kinks(got_g, want_g, grad_tol * scale + softmax_side_floor(k, g_ref, 1e-8),
                                                    f"{k} train={train} (oracle: {kinks} hidden units on the kink)", kinks=kinks)
                else:
                    np.testing.assert_allclose(got_g, want_g, rtol=0, atol=grad_tol * scale + 1e-8, err_msg=f"{k} train={train}")
        if check_attention:
            # normalized_att_scores [H, B, F, F] (after dropout) of every layer; a training-mode forward is a step of its own for
            # the dropout counters: its masks are replayed from the counters it left
            model.capture_attention = True
            try:
                model(Xg.to(DEV))
            finally:
                model.capture_attention = False
            drop_a = O.Dropper("masks", 0.1, O.dropout_masks(eng.drop_seed, eng.drop_step, B, F, D, H, L, 0.1)) if train else None
            trace = {}
            O.forward(state, Xt, spec, drop_a, trace=trace)
            for l in range(L):
                got_a = model.domain_int_layers[l].normalized_att_scores.cpu().double().numpy()
                want_a = trace[f"att{l}"].double().numpy()
                note_worst(tag, "attention map abs err", float(np.abs(got_a - want_a).max()), f"layer {l} F={F} train={train}")
                np.testing.assert_allclose(got_a, want_a, rtol=0, atol=2e-6, err_msg=f"att{l} train={train}")
                if train:
                    assert (want_a == 0).any(), "no dropped attention element: the masks were not on"
    return model
