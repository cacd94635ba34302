"""AdaSparse's scenario-pruned DNN without a GPU: the fp64 restatement against the reference's recorded AdaSparse runs, its
explicit backward against autograd of the plain-torch form, the modules' state, the C ABI's new symbols and their argument
validation, and the premise of the GPU bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from satrans_amd import native
from tests import adasparse_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adasparse")
CASES = {"plain": dict(widths=(16, 8), consts=(1.0, 2.0, 0.25)), "one_layer": dict(widths=(8,), consts=(1.0, 2.0, 0.25)),
         "scaled": dict(widths=(16, 8), consts=(0.5, 1.5, 0.4))}
SYMBOLS = ("satrans_adasparse_saved_floats", "satrans_adasparse_workspace_floats", "satrans_adasparse_fwd", "satrans_adasparse_bwd",
           "satrans_adasparse_set_forward")
TILE, CHUNK = native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK
SWEEP_B = CHUNK + TILE + 1

# The recorded side is an fp32 run (unit roundoff u = 6e-8), the restatement fp64 on the same fp32 inputs.  A recorded element
# has passed at most 6 products (forward and backward) whose contractions are at most 24 long (C + E = 17, widths <= 16, B = 24
# rows in a weight gradient) and a sigmoid: its rounding error is bounded by about 6 * 24 * u = 9e-6 of the largest magnitude in
# the worst case.  The bound is that figure rounded up to the siblings' (tests/test_mmoe_cpu.py); the deviations seen are printed.
BOUND = 2e-5


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def state_of(fx):
    return {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}


def replay(fx, name):
    """Probabilities, loss, cache and every gradient (the table's through the gather), recomputed by the restatement in fp64."""
    L = len(CASES[name]["widths"])
    P = R.params_from_state(state_of(fx), L)
    consts = tuple(float(v) for v in fx["consts"])
    x, e = torch.from_numpy(fx["dnn_input"]).double(), torch.from_numpy(fx["domain_emb"]).double()
    labels = torch.from_numpy(fx["labels"]).double()
    logit, cache = R.forward(x, e, P, consts)
    y = torch.sigmoid(logit)
    loss = -(labels * torch.log(y.squeeze(1)) + (1 - labels) * torch.log(1 - y.squeeze(1))).sum()
    g = R.backward(y - labels.unsqueeze(1), cache)      # d(summed BCE) / d(logit)
    grads = R.state_from_params({k: v for k, v in g.items() if k not in ("x", "emb")})
    grads["dnn_input"] = g["x"]
    lo, hi = (int(v) for v in fx["dom_cols"])
    table = torch.zeros(fx["grad/domain_table"].shape, dtype=torch.float64)
    table.index_add_(0, torch.from_numpy(fx["dom_ids"]), g["x"][:, lo:hi] + g["emb"])      # both paths into the table
    grads["domain_table"] = table
    return y, loss, cache, grads


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_every_fixture(name):
    fx = load(name)
    y, loss, cache, grads = replay(fx, name)
    rec_y = torch.from_numpy(fx["y_pred"]).double()
    worst = float((y - rec_y).abs().max() / rec_y.abs().max())
    assert worst <= BOUND, ("y", worst)
    assert abs(float(loss) - float(fx["loss"])) <= BOUND * abs(float(fx["loss"]))
    for l, z in enumerate(cache.zs):
        rec = torch.from_numpy(fx[f"z/{l}"]).double()
        dev = float((z - rec).abs().max() / rec.abs().max())
        worst = max(worst, dev)
        assert dev <= BOUND, (f"z/{l}", dev)
    recorded = sorted(k[len("grad/"):] for k in fx if k.startswith("grad/"))
    assert recorded == sorted(grads)
    for k in recorded:
        rec = torch.from_numpy(fx[f"grad/{k}"]).double()
        scale = float(rec.abs().max())
        assert scale > 0.0, k
        dev = float((grads[k].reshape(rec.shape) - rec).abs().max() / scale)
        worst = max(worst, dev)
        assert dev <= BOUND, (k, dev)
    print(f"[adasparse] {name}: largest deviation {worst:.2e}")


@pytest.mark.parametrize("name", list(CASES))
def test_fixtures_hold_the_cases_they_claim(name):
    """Every layer prunes between 0.1 and 0.6 of its units, no unit sits within the bound of the threshold or of relu's kink, the
    recorded z give the same cut, and `scaled` uses its own constants."""
    fx = load(name)
    _, _, cache, _ = replay(fx, name)
    consts = tuple(float(v) for v in fx["consts"])
    assert consts == pytest.approx(CASES[name]["consts"])
    assert (consts != pytest.approx(R.DEFAULTS)) == (name == "scaled")
    shares = R.pruned_shares(cache)
    assert len(shares) == len(CASES[name]["widths"]) and all(0.1 <= s <= 0.6 for s in shares), shares
    relu, thr = R.margins(cache)
    print(f"[adasparse] {name}: pruned shares {shares}, relu margin {relu:.2e}, threshold margin {thr:.2e}")
    assert relu >= BOUND and thr >= BOUND
    alpha, beta, eps = consts
    for l, pi in enumerate(cache.pis):
        rec_pi = beta / (1 + np.exp(-alpha * fx[f"z/{l}"].astype(np.float64)))
        assert np.array_equal(rec_pi <= eps, (pi == 0).numpy())
    assert fx["dnn_input"].shape == (24, 13) and fx["domain_emb"].shape == (24, 4) and fx["y_pred"].shape == (24, 1)
    assert all(fx[k].dtype.kind in "fiU" for k in fx)


def test_explicit_backward_equals_autograd_of_the_plain_torch_form():
    """fp64 autograd through the reference's statement (R.torch_form, with its in-place cut) against R.backward, with and
    without the logit layer, at non-default constants too."""
    for consts, head in ((R.DEFAULTS, True), ((0.5, 1.5, 0.4), True), (R.DEFAULTS, False)):
        x, e, w, P = R.draw(40, 7, 3, (6, 5, 4), 1, consts=consts)
        P = {k: ([t.double().requires_grad_(True) for t in v] if isinstance(v, list) else v.double().requires_grad_(True))
             for k, v in P.items()}
        x, e = x.double().requires_grad_(True), e.double().requires_grad_(True)
        up = w.double() if head else torch.randn(40, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
        out = R.torch_form(x, e, P, consts, head=head)
        (out * up).sum().backward()
        with torch.no_grad():
            mine_out, cache = R.forward(x, e, P, consts, head=head)
            mine = R.flat(R.backward(up, cache, head=head))
        assert float((mine_out - out.detach()).abs().max()) <= 1e-12 * float(out.detach().abs().max())
        want = {k: t.grad for k, t in R.flat(P).items() if head or k not in R.SINGLES}
        want.update(x=x.grad, emb=e.grad)
        assert sorted(want) == sorted(mine)
        for k, t in want.items():
            assert float((mine[k] - t).abs().max()) <= 1e-12 * float(t.abs().max()), k


def test_a_pruned_unit_contributes_exactly_nothing():
    """A pruned unit's row of dW and dP, both bias entries, and its terms of dh and demb are exactly zero: the explicit
    backward with that unit's weights replaced by garbage gives bit-identical gradients everywhere else."""
    x, e, w, P = R.draw(50, 9, 4, (12, 6), 3)
    Pd = R.double(P)
    Pd["prn_b"][0][5] = -30.0      # unit 5 of layer 0: pruned for every row
    _, cache = R.forward(x.double(), e.double(), Pd)
    assert bool((cache.pis[0][:, 5] == 0).all()) and bool((cache.pis[0][:, 4] != 0).any())
    g = R.backward(w.double(), cache)
    for k in ("lin_w", "prn_w"):
        assert float(g[k][0][5].abs().max()) == 0.0 and float(g[k][0][4].abs().max()) > 0.0
    for k in ("lin_b", "prn_b"):
        assert float(g[k][0][5]) == 0.0 and float(g[k][0][4].abs()) > 0.0
    pruned = cache.pis[1] == 0
    assert bool(pruned.any())
    P2 = R.double(P)
    P2["prn_b"][0][5] = -30.0
    P2["lin_w"][0][5] = 1e3
    P2["prn_w"][0][5, :9] = 1e-3      # (small: the unit must stay pruned)
    _, cache2 = R.forward(x.double(), e.double(), P2)
    g2 = R.backward(w.double(), cache2)
    assert torch.equal(g2["x"], g["x"]) and torch.equal(g2["emb"], g["emb"])


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_matches_the_reference(name):
    """Keys, order and shapes of state_dict() equal the reference AdaSparse's head entries, and the recorded values load."""
    from satrans_amd import AdaSparseHead, PrunedDNN
    fx, c = load(name), CASES[name]
    keys, shapes = [str(k) for k in fx["keys"]], [str(s) for s in fx["shapes"]]
    assert keys == R.keys_of(len(c["widths"]))
    Cn, E = fx["dnn_input"].shape[1], fx["domain_emb"].shape[1]
    head = AdaSparseHead(Cn, c["widths"], domain_emb_dim=E)
    sd = head.state_dict()
    assert list(sd) == keys
    assert [str(tuple(sd[k].shape)) for k in keys] == shapes
    values = state_of(fx)
    head.load_state_dict(values)      # strict
    for k, v in values.items():
        assert torch.equal(head.state_dict()[k], v), k
    fresh = AdaSparseHead(Cn, c["widths"], domain_emb_dim=E)
    assert float(fresh.dnn.linears[0].weight.detach().abs().max()) < 1e-3      # N(0, 1e-4)
    assert float(fresh.dnn.pruners[0].weight.detach().abs().max()) > 1e-3      # torch's default
    assert float(fresh.dnn_linear.weight.detach().abs().max()) > 1e-3
    assert float(fresh.out.bias.detach().abs().max()) == 0.0
    assert (fresh.dnn.alpha, fresh.dnn.beta, fresh.dnn.epsilon) == (1, 2.0, 0.25)
    dnn = PrunedDNN(Cn, c["widths"], domain_emb_dim=E)
    assert list(dnn.state_dict()) == [k[len("dnn."):] for k in keys if k.startswith("dnn.")]


def test_modules_refuse_what_is_not_built():
    from satrans_amd import AdaSparseHead, PrunedDNN
    with pytest.raises(NotImplementedError, match="relu"):
        PrunedDNN(8, (4,), activation="prelu")
    with pytest.raises(NotImplementedError, match="dropout"):
        PrunedDNN(8, (4,), dropout_rate=0.1)
    with pytest.raises(NotImplementedError, match="batch-norm"):
        PrunedDNN(8, (4,), use_bn=True)
    with pytest.raises(NotImplementedError, match="hidden layers"):
        PrunedDNN(8, (4,) * 4)
    with pytest.raises(ValueError):
        PrunedDNN(8, ())
    with pytest.raises(ValueError):
        PrunedDNN(8, (4, 0))
    with pytest.raises(ValueError):
        PrunedDNN(8, (4, -2))
    with pytest.raises(NotImplementedError, match="relu"):
        AdaSparseHead(8, dnn_activation="prelu")
    with pytest.raises(NotImplementedError, match="dropout"):
        AdaSparseHead(8, dnn_dropout=0.1)
    with pytest.raises(NotImplementedError, match="batch-norm"):
        AdaSparseHead(8, dnn_use_bn=True)
    with pytest.raises(NotImplementedError, match="hidden layers"):
        AdaSparseHead(8, (4,) * 4)
    with pytest.raises(ValueError):
        AdaSparseHead(8, ())
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        AdaSparseHead(8, (4,), domain_emb_dim=3)(torch.zeros(3, 8), torch.zeros(3, 3))


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert "typedef struct satrans_adasparse_desc" in header and "typedef struct satrans_adasparse_grads" in header
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    H = native.MMOE_MAX_HIDDEN
    # B, C, E, n_layers, the widths, three float constants + x, emb + the parameter pointers
    assert ctypes.sizeof(native.AdaSparseDesc) == (4 + H + 3) * 4 + (2 + 4 * H + 2) * 8
    assert ctypes.sizeof(native.AdaSparseGrads) == (4 * H + 2) * 8
    for struct, cls in (("satrans_adasparse_desc", native.AdaSparseDesc), ("satrans_adasparse_grads", native.AdaSparseGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.split(None, 1)[1] if decl.split() else "")]
        names = [n for n in names if n not in ("float", "int32_t", "const")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def ada_desc(B, Cn, E, widths, consts=R.DEFAULTS):
    d = native.AdaSparseDesc()
    d.B, d.C, d.E, d.n_layers = B, Cn, E, len(widths)
    for l, n in enumerate(widths[:native.MMOE_MAX_HIDDEN]):
        d.width[l] = n
    d.alpha, d.beta, d.epsilon = consts
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    null = ctypes.POINTER(native.AdaSparseDesc)()
    assert lib.satrans_adasparse_saved_floats(null) == -1
    assert lib.satrans_adasparse_workspace_floats(null) == -1
    assert lib.satrans_adasparse_fwd(null, None, None, None) == -1
    assert b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_adasparse_bwd(null, None, None, None, None, None, None, None) == -1
    ok = (4, 8, 3, (16, 8))
    bad = [ok[:at] + (v,) + ok[at + 1:] for at, values in ((0, (0, -1)), (1, (0, -8)), (2, (0, -2)), (3, ((), (4,) * 4, (16, 0), (-4,))))
           for v in values]
    for args in bad:
        d = ada_desc(*args)
        assert lib.satrans_adasparse_saved_floats(ctypes.byref(d)) == -1, args
        assert lib.satrans_adasparse_workspace_floats(ctypes.byref(d)) == -1, args
        assert lib.satrans_adasparse_fwd(ctypes.byref(d), None, None, None) == -1, args
        assert b"bad sizes" in lib.satrans_last_error(), args
        assert lib.satrans_adasparse_bwd(ctypes.byref(d), None, None, None, None, None, None, None) == -1, args
    for consts in ((1.0, 0.0, 0.25), (1.0, -2.0, 0.25), (1.0, 2.0, -0.1), (float("nan"), 2.0, 0.25)):
        d = ada_desc(*ok, consts=consts)
        assert lib.satrans_adasparse_saved_floats(ctypes.byref(d)) == -1, consts
        assert b"bad constants" in lib.satrans_last_error(), consts
        assert lib.satrans_adasparse_fwd(ctypes.byref(d), None, None, None) == -1, consts
    assert lib.satrans_adasparse_saved_floats(ctypes.byref(ada_desc(*ok, consts=(1.0, 2.0, 0.0)))) > 0      # epsilon = 0 is allowed
    B, Cn, E = 300, 70, 5
    d = ada_desc(B, Cn, E, (48, 32))
    assert lib.satrans_adasparse_saved_floats(ctypes.byref(d)) == 3 * B * (48 + 32)
    chunks = -(-B // CHUNK)
    part = chunks * max(48 * (Cn + 1) + 48 * (Cn + E + 1), 32 * (48 + 1) + 32 * (48 + E + 1), 32 + 1)
    assert lib.satrans_adasparse_workspace_floats(ctypes.byref(d)) == 4 * B * 48 + part
    assert lib.satrans_adasparse_fwd(ctypes.byref(d), None, None, None) == -1      # sizes fine, pointers null
    assert b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_adasparse_bwd(ctypes.byref(d), None, None, None, None, None, None, None) == -1
    assert b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_adasparse_set_forward(2) == -1 and lib.satrans_adasparse_set_forward(0) == 0


@pytest.mark.parametrize("case", R.SWEEP, ids=lambda c: f"C{c[0]}-E{c[1]}")
def test_premise_of_the_gpu_bounds(case):
    """The GPU tests hold the kernels to 2e-5 max|.| on logits and saved factors and 1e-4 max|g| + 5e-9 on gradients
    (DESIGN.md §4).  On their seeded inputs the restatement run in fp32 stays inside those bounds against its fp64 run, every
    layer prunes between 0.1 and 0.6 of its units (asserted by the draw), and no unit of the fp64 forward lies within the output
    bound of relu's kink or of the pruning threshold (R.draw draws such rows again; decided by the fp64 forward alone)."""
    x, e, w, P = R.sweep_draw(case, SWEEP_B)
    want_y, cache = R.forward(x.double(), e.double(), R.double(P))
    want = R.flat(R.backward(w.double(), cache))
    relu, thr = R.margins(cache)
    assert relu >= 2e-5 and thr >= 2e-5
    y, c32 = R.forward(x, e, P)
    got = R.flat(R.backward(w, c32))
    dev_y = float((y.double() - want_y).abs().max() / want_y.abs().max())
    dev_pi = max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(c32.pis, cache.pis))
    worst = 0.0
    for k in want:
        scale = float(want[k].abs().max())
        err = float((got[k].double() - want[k]).abs().max())
        worst = max(worst, err / max(scale, 1e-30))
    print(f"[adasparse] premise {case}: y {dev_y:.2e}, pi {dev_pi:.2e}, worst gradient {worst:.2e}, relu margin {relu:.2e}, "
          f"threshold margin {thr:.2e}, pruned shares {R.pruned_shares(cache)}")
    assert dev_y <= 2e-5 and dev_pi <= 2e-5
    for k in want:
        scale = float(want[k].abs().max())
        assert float((got[k].double() - want[k]).abs().max()) <= 1e-4 * scale + 5e-9, k
