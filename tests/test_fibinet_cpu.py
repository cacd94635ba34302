"""CPU side of FiBiNET's SENet layer, bilinear interaction and head: the restatement tests/fibinet_reference.py against autograd of
deepctr's literal form and against the recorded runs of the reference's own FiBiNET.forward (tests/golden/fibinet, written by
tools/gen_fibinet_golden.py); the ABI mirror; the modules' parameters, state_dict order and construction errors; the premise of
the GPU bounds."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from satrans_amd import native
from tests import fibinet_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fibinet")
SYMBOLS = ("satrans_senet_saved_floats", "satrans_senet_workspace_floats", "satrans_senet_fwd", "satrans_senet_bwd",
           "satrans_bilinear_workspace_floats", "satrans_bilinear_fwd", "satrans_bilinear_bwd", "satrans_fibinet_saved_floats",
           "satrans_fibinet_workspace_floats", "satrans_fibinet_fwd", "satrans_fibinet_bwd")


def fixture(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def close(got, want, rel, msg, floor=0.0):
    want = torch.as_tensor(want)
    err, scale = float((torch.as_tensor(got) - want).abs().max()), float(want.abs().max())
    assert err <= rel * scale + floor, (msg, err, scale)


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_explicit_backward_equals_autograd_of_deepctrs_form(case):
    """fp64: the restatement's forward is deepctr's literal form (a Linear, a product and a cat per pair; the same Bilinear on
    the SENet output and on the raw embeddings), and its explicit backward is autograd's of that form."""
    B, Fn, D, kind, ratio, dnn, dense_dim = case
    emb, dense, up, P = R.sweep_draw(case)
    leaves = {k: v.double().requires_grad_(True) for k, v in R.flat(P).items()}
    e = emb.double().requires_grad_(True)
    dn = None if dense is None else dense.double().requires_grad_(True)
    # deepctr, literally
    A = torch.relu(F.linear(torch.relu(F.linear(torch.mean(e, dim=-1), leaves["w1"])), leaves["w2"]))
    V = torch.mul(e, torch.unsqueeze(A, dim=2))

    def bil(x):
        xs = torch.split(x, 1, dim=1)
        out = []
        for p, (i, j) in enumerate(itertools.combinations(range(Fn), 2)):
            out.append(torch.mul(F.linear(xs[i], leaves["bil"][R.weight_index(kind, i, p)]), xs[j]))
        return torch.cat(out, dim=1)

    h = torch.flatten(torch.cat((bil(V), bil(e)), dim=1), start_dim=1)
    if dn is not None:
        h = torch.cat([h, dn], dim=-1)
    for l in range(len(dnn)):
        h = torch.relu(F.linear(h, leaves[f"dnn_w.{l}"], leaves[f"dnn_b.{l}"]))
    want_y = F.linear(h, leaves["lin"]) + leaves["out_bias"]
    (want_y * up.double()).sum().backward()
    y, cache = R.forward(emb.double(), None if dense is None else dense.double(), R.double(P), kind)
    assert y.shape == (B, 1) and cache.X.shape == (B, Fn * (Fn - 1) * D + dense_dim)
    close(y, want_y.detach(), 1e-12, "forward")
    g = R.flat(R.backward(up.double(), cache))
    close(g.pop("emb"), e.grad, 1e-11, "demb")
    if dn is not None:
        close(g.pop("dense"), dn.grad, 1e-11, "ddense")
    assert sorted(g) == sorted(leaves)
    for k, v in g.items():
        close(v, leaves[k].grad, 1e-11, k)
    if kind == "each":
        assert float(g["bil"][Fn - 1].abs().max()) == 0.0      # the last weight is never used


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_every_draw_opens_and_shuts_gates(case):
    """Over the batch: at least one (row, field) with a = 0 and at least half with a > 0, and no pre-activation near a kink.
    A dead SENet block would hide its kernels.  (Printed too: the shut gates in rows that have open ones.)"""
    emb, dense, up, P = R.sweep_draw(case)
    _, c = R.forward(emb.double(), None if dense is None else dense.double(), R.double(P), case[3])
    a = R.gates(c)
    shut = a == 0
    print(f"[fibinet-gates] {R.case_id(case)}: a = 0 at {int(shut.sum())} of {a.numel()}, in mixed rows "
          f"{int((shut & (a > 0).any(1, keepdim=True)).sum())}")
    assert bool(shut.any())
    assert int((a > 0).sum()) * 2 >= a.numel()
    assert R.gates_ok(a)
    assert not bool(R.near_kink(c, 2e-5).any())


def run_fixture(fx, dtype=torch.float32):
    kind = str(fx["bilinear_type"])
    sd = {k[6:]: torch.from_numpy(v).to(dtype) for k, v in fx.items() if k.startswith("param/")}
    emb, dense, lin, labels = (torch.from_numpy(fx[k]).to(dtype) for k in ("emb", "dense", "linear_logit", "labels"))
    P = R.params_from_state(sd, emb.shape[1], kind, dtype)
    logit, cache = R.forward(emb, dense, P, kind)
    leaf = (lin + logit).clone().requires_grad_(True)
    y = torch.sigmoid(leaf)
    loss = F.binary_cross_entropy(y.squeeze(1), labels, reduction='sum')
    loss.backward()
    return kind, sd, y.detach(), loss.detach(), R.backward(leaf.grad, cache)


@pytest.mark.parametrize("name", R.TYPES)
def test_restatement_reproduces_every_fixture(name):
    """fp32 against the reference's fp32 run: y_pred, the loss, every parameter gradient, grad/emb and reg_loss within 2e-5
    max|.| (the DNN input is 49 wide).  The gradients come from the explicit backward, fed d loss / d logit."""
    fx = fixture(name)
    kind, sd, y, loss, g = run_fixture(fx)
    close(y, fx["y_pred"], 2e-5, "y_pred")
    assert abs(float(loss) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    grads = R.state_from_params(g, fx["emb"].shape[1], kind)
    assert list(grads) == list(fx["keys"])
    for k, v in grads.items():
        unused = kind == "each" and k == "Bilinear.bilinear.3.weight"
        assert (float(np.abs(fx[f"grad/{k}"]).max()) > 0.0) != unused, k
        close(v, fx[f"grad/{k}"], 2e-5, k)
    close(g["emb"], fx["grad/emb"], 2e-5, "grad/emb")
    assert fx["reg_loss"].shape == (1,)
    assert torch.equal(R.reg_loss(sd), torch.from_numpy(fx["reg_loss"]))


def test_fixtures_hold_the_cases_they_claim():
    for name in R.TYPES:
        fx = fixture(name)
        assert str(fx["bilinear_type"]) == name
        assert list(fx["keys"]) == R.keys_of(4, name, 2)
        B, Fn, D = fx["emb"].shape
        assert (B, Fn, D) == (24, 4, 4) and fx["dense"].shape == (B, 1) and fx["X"].shape == (B, 5)
        assert fx["param/SE.excitation.0.weight"].shape == (1, 4) and fx["param/SE.excitation.2.weight"].shape == (4, 1)
        n_w = {"all": 1, "each": 4, "interaction": 6}[name]
        assert sum(k.startswith("param/Bilinear.") for k in fx) == n_w
        assert fx["param/dnn.linears.0.weight"].shape == (16, 4 * 3 * 4 + 1) and fx["param/dnn.linears.1.weight"].shape == (8, 16)
        assert fx["param/dnn_linear.weight"].shape == (1, 8)
        # FiBiNET.__init__ registers nothing of its own for regularisation
        assert int(fx["n_own_reg"]) == 0 and float(fx["reg_loss"][0]) == 0.0
        # the recorded run has open and shut gates
        emb = torch.from_numpy(fx["emb"])
        a = torch.relu(R.senet(emb, torch.from_numpy(fx["param/SE.excitation.0.weight"]),
                               torch.from_numpy(fx["param/SE.excitation.2.weight"]))[1][2])
        assert bool((a == 0).any()) and bool((a > 0).any())


@pytest.mark.parametrize("name", R.TYPES)
def test_state_dict_matches_the_reference(name):
    """Keys, their order and the shapes of FiBiNETHead are the recorded ones, and the recorded values load."""
    from satrans_amd import FiBiNETHead
    fx = fixture(name)
    state = {k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    head = FiBiNETHead(4, 4, 1, name, 3, (16, 8))
    sd = head.state_dict()
    assert list(sd) == list(fx["keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(fx["shapes"])
    head.load_state_dict(state)
    for k, v in head.state_dict().items():
        assert torch.equal(v, state[k]), k
    reg = head.regularization_loss()      # plain torch: runs on the CPU too
    assert reg.shape == (1,) and torch.equal(reg.detach(), torch.from_numpy(fx["reg_loss"]))
    assert float(head.out.bias.detach().abs().max()) > 0.0
    assert torch.equal(FiBiNETHead(4, 4, 1, name).out.bias.detach(), torch.zeros(1))


def test_layers_have_deepctrs_initial_bits():
    from satrans_amd import BilinearInteraction, SENETLayer
    Fn, D = 7, 5
    torch.manual_seed(3)
    se = SENETLayer(Fn, 3, 1024, device='cpu')
    torch.manual_seed(3)      # deepctr's: Sequential(Linear(F, R, bias=False), ReLU, Linear(R, F, bias=False), ReLU)
    ref = nn.Sequential(nn.Linear(Fn, 2, bias=False), nn.ReLU(), nn.Linear(2, Fn, bias=False), nn.ReLU())
    assert [(k, tuple(v.shape)) for k, v in se.state_dict().items()] == [("excitation.0.weight", (2, Fn)), ("excitation.2.weight", (Fn, 2))]
    for k, v in ref.state_dict().items():
        assert torch.equal(v, se.state_dict()[f"excitation.{k}"]), k
    assert SENETLayer(2, 3).reduction_size == 1 and SENETLayer(5, 1).reduction_size == 5
    for kind, n in (("all", 1), ("each", Fn), ("interaction", Fn * (Fn - 1) // 2)):
        torch.manual_seed(4)
        mod = BilinearInteraction(Fn, D, kind, 1024, device='cpu')
        torch.manual_seed(4)
        want = [nn.Linear(D, D, bias=False).weight.detach() for _ in range(n)]
        assert list(mod.state_dict()) == R.bilinear_keys(Fn, kind, "")
        for v, w in zip(mod.state_dict().values(), want):
            assert torch.equal(v, w) and float(w.abs().max()) > 0.0


def test_modules_refuse_what_is_not_built():
    from satrans_amd import BilinearInteraction, FiBiNETHead, SENETLayer
    with pytest.raises(NotImplementedError):
        BilinearInteraction(4, 8, 'some')
    with pytest.raises(NotImplementedError):
        FiBiNETHead(4, 8, 0, 'some')
    with pytest.raises(ValueError):
        FiBiNETHead(1, 8)
    with pytest.raises(ValueError):
        BilinearInteraction(1, 8)
    with pytest.raises(NotImplementedError, match="FIBINET_MAX_FIELDS"):
        FiBiNETHead(native.FIBINET_MAX_FIELDS + 1, 4, 0, 'all')
    with pytest.raises(NotImplementedError, match="FIBINET_MAX_FIELDS"):
        SENETLayer(native.FIBINET_MAX_FIELDS + 1)
    with pytest.raises(NotImplementedError, match="FIBINET_MAX_DIM"):
        FiBiNETHead(4, native.FIBINET_MAX_DIM + 1)
    with pytest.raises(NotImplementedError, match="FIBINET_MAX_DIM"):
        BilinearInteraction(4, native.FIBINET_MAX_DIM + 1)
    with pytest.raises(NotImplementedError, match="MMOE_MAX_HIDDEN"):
        FiBiNETHead(4, 8, 0, 'all', 3, (8,) * (native.MMOE_MAX_HIDDEN + 1))
    for kw in (dict(dnn_dropout=0.5), dict(dnn_use_bn=True), dict(dnn_activation='prelu')):
        with pytest.raises(NotImplementedError, match="not built"):
            FiBiNETHead(4, 8, **kw)
    assert FiBiNETHead(native.FIBINET_MAX_FIELDS, 4, 0, 'all', 3, (8,)).dnn.linears[0].weight.shape == (8, 64 * 63 * 4)
    x = torch.randn(6, 4, 8)
    for mod in (SENETLayer(4), BilinearInteraction(4, 8), FiBiNETHead(4, 8, 0, 'each', 3, (16,))):
        with pytest.raises(native.NativeError, match="no CPU fallback"):
            mod(x)
    for mod in (SENETLayer(4), BilinearInteraction(4, 8)):
        with pytest.raises(ValueError, match="expect to be 3 dimensions"):
            mod(x[0])
        with pytest.raises(ValueError):
            mod(x[:, :3])
    with pytest.raises(ValueError):
        FiBiNETHead(4, 8, 2)(x)                       # dense columns missing
    with pytest.raises(ValueError):
        FiBiNETHead(4, 8)(x, torch.randn(6, 1))       # dense columns unexpected
    no_dnn = FiBiNETHead(4, 8, 3, 'all', 3, ())
    assert list(no_dnn.state_dict()) == R.keys_of(4, 'all', 0) and no_dnn.dnn_linear.weight.shape == (1, 4 * 3 * 8 + 3)


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    for name in ("MAX_FIELDS", "MAX_DIM", "DW_ROW_CHUNK", "SENET_ROW_CHUNK"):
        assert int(re.search(r"#define SATRANS_FIBINET_%s (\d+)" % name, header).group(1)) == getattr(native, f"FIBINET_{name}"), name
    for name, code in native.BILINEAR_TYPES.items():
        assert int(re.search(r"#define SATRANS_BILINEAR_%s (\d+)" % name.upper(), header).group(1)) == code
    assert native.FIBINET_MAX_FIELDS == 64 and native.FIBINET_MAX_DIM == 128
    H = native.MMOE_MAX_HIDDEN
    assert ctypes.sizeof(native.SENetDesc) == 4 * 4 + 3 * 8 and ctypes.sizeof(native.SENetGrads) == 2 * 8
    assert ctypes.sizeof(native.BilinearDesc) == 4 * 4 + 3 * 8
    assert ctypes.sizeof(native.FiBiNETGrads) == (5 + 2 * H) * 8
    assert ctypes.sizeof(native.FiBiNETDesc) == (8 + H + 1) * 4 + (2 + 5 + 2 * H) * 8
    for struct, cls in (("satrans_senet_desc", native.SENetDesc), ("satrans_senet_grads", native.SENetGrads),
                        ("satrans_bilinear_desc", native.BilinearDesc), ("satrans_fibinet_desc", native.FiBiNETDesc),
                        ("satrans_fibinet_grads", native.FiBiNETGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") if decl.split()
                 for n in re.findall(r"\*?\s*(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.split(None, 1)[1])]
        names = [n for n in names if n not in ("float", "int32_t", "const")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def head_desc(B, Fn, D, kind=2, R_=1, dense=0, dnn=()):
    d = native.FiBiNETDesc()
    d.B, d.F, d.D, d.type, d.R, d.dense_dim, d.n_dnn = B, Fn, D, kind, R_, dense, len(dnn)
    for l, w in enumerate(dnn[:native.MMOE_MAX_HIDDEN]):
        d.width[l] = w
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    by = ctypes.byref
    assert lib.satrans_fibinet_saved_floats(ctypes.POINTER(native.FiBiNETDesc)()) == -1 and b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_fibinet_workspace_floats(ctypes.POINTER(native.FiBiNETDesc)()) == -1
    assert lib.satrans_fibinet_fwd(ctypes.POINTER(native.FiBiNETDesc)(), None, None, None) == -1
    assert lib.satrans_fibinet_bwd(ctypes.POINTER(native.FiBiNETDesc)(), None, None, None, None, None, None, None) == -1
    assert lib.satrans_senet_saved_floats(ctypes.POINTER(native.SENetDesc)()) == -1
    assert lib.satrans_senet_fwd(ctypes.POINTER(native.SENetDesc)(), None, None, None) == -1
    assert lib.satrans_senet_bwd(ctypes.POINTER(native.SENetDesc)(), None, None, None, None, None, None, None) == -1
    assert lib.satrans_bilinear_workspace_floats(ctypes.POINTER(native.BilinearDesc)()) == -1
    assert lib.satrans_bilinear_fwd(ctypes.POINTER(native.BilinearDesc)(), None, None) == -1
    assert lib.satrans_bilinear_bwd(ctypes.POINTER(native.BilinearDesc)(), None, None, None, None, None, None, None) == -1
    bad = [dict(B=0, Fn=4, D=8), dict(B=8, Fn=1, D=8), dict(B=8, Fn=4, D=0), dict(B=8, Fn=4, D=8, kind=3), dict(B=8, Fn=4, D=8, kind=-1),
           dict(B=8, Fn=4, D=8, R_=0), dict(B=8, Fn=4, D=8, R_=5), dict(B=8, Fn=4, D=8, dense=-1), dict(B=8, Fn=4, D=8, dnn=(16, 0))]
    for kw in bad:
        d = head_desc(**kw)
        for rc in (lib.satrans_fibinet_saved_floats(by(d)), lib.satrans_fibinet_workspace_floats(by(d)),
                   lib.satrans_fibinet_fwd(by(d), None, None, None), lib.satrans_fibinet_bwd(by(d), None, None, None, None, None, None, None)):
            assert rc == -1, kw
    beyond = [dict(B=8, Fn=native.FIBINET_MAX_FIELDS + 1, D=8), dict(B=8, Fn=4, D=native.FIBINET_MAX_DIM + 1),
              dict(B=(1 << 31) - 1, Fn=64, D=128), dict(B=(1 << 31) - 1, Fn=4, D=8, dnn=(4096,))]      # (the last: the DNN's grid alone)
    for kw in beyond:
        d = head_desc(**kw)
        assert lib.satrans_fibinet_saved_floats(by(d)) == -2, kw
        assert lib.satrans_fibinet_fwd(by(d), None, None, None) == -2 and lib.satrans_last_error(), kw
    d = head_desc(8, 4, 8)
    d.n_dnn = native.MMOE_MAX_HIDDEN + 1
    assert lib.satrans_fibinet_saved_floats(by(d)) == -2 and b"hidden layers" in lib.satrans_last_error()
    # sizes, at the AliCCP shape with a ragged batch
    B, Fn, D, R_, dense, dnn = 131, 19, 32, 6, 2, (128, 64)
    n_pairs = Fn * (Fn - 1) // 2
    ld = 2 * n_pairs * D + dense
    d = head_desc(B, Fn, D, 2, R_, dense, dnn)
    head = -(-(B * (Fn + R_)) // 4) * 4      # a, hid, up to a multiple of 4 floats
    assert lib.satrans_fibinet_saved_floats(by(d)) == head + B * ld + B * sum(dnn)
    dw_chunks, se_chunks, mm_chunks = (-(-B // c) for c in (native.FIBINET_DW_ROW_CHUNK, native.FIBINET_SENET_ROW_CHUNK,
                                                            native.MMOE_DW_ROW_CHUNK))
    parts = max(mm_chunks * 128 * (ld + 1), dw_chunks * n_pairs * D * D, 2 * se_chunks * Fn * R_)
    assert lib.satrans_fibinet_workspace_floats(by(d)) == B * ld + 2 * B * max(dnn) + B * Fn + parts
    s = native.SENetDesc()
    s.B, s.F, s.D, s.R = B, Fn, D, R_
    assert lib.satrans_senet_saved_floats(by(s)) == B * (Fn + R_)
    assert lib.satrans_senet_workspace_floats(by(s)) == 2 * se_chunks * Fn * R_
    for kind, n_w in ((0, 1), (1, Fn), (2, n_pairs)):
        b = native.BilinearDesc()
        b.B, b.F, b.D, b.type = B, Fn, D, kind
        assert lib.satrans_bilinear_workspace_floats(by(b)) == dw_chunks * n_w * D * D
        assert lib.satrans_bilinear_fwd(by(b), None, None) == -1 and b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_bilinear_bwd(by(b), None, None, None, None, None, None, None) == -1
    assert lib.satrans_senet_fwd(by(s), None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_senet_bwd(by(s), None, None, None, None, None, None, None) == -1
    assert lib.satrans_fibinet_fwd(by(d), None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_fibinet_bwd(by(d), None, None, None, None, None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()


def factored_forward(emb, dense, P, kind):
    """The arithmetic of the kernels in torch: ONE product per pair, the SENet block a_i a_j times the raw one."""
    B, Fn, D = emb.shape
    a = torch.relu(torch.relu(torch.mean(emb, -1) @ P["w1"].T) @ P["w2"].T)
    raw = R.bilinear(emb, P["bil"], kind)
    idx = torch.tensor(R.pairs(Fn))
    scaled = (a[:, idx[:, 0]] * a[:, idx[:, 1]]).unsqueeze(2) * raw
    h = torch.cat((scaled, raw), 1).flatten(1)
    if dense is not None:
        h = torch.cat([h, dense], -1)
    for w, b in zip(P["dnn_w"], P["dnn_b"]):
        h = torch.relu(h @ w.T + b)
    return h @ P["lin"].T + P["out_bias"]


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_premise_of_the_gpu_bounds(case):
    """The GPU tests hold the kernels to 2e-5 max|.| on results and 1e-4 max|g| + 5e-9 on gradients.  On every
    swept shape torch's own fp32 run of the FACTORED form a_i a_j (W e_i * e_j) - the kernels' arithmetic, under autograd - stays
    within a quarter of those bounds against the fp64 literal form (measured: <= 4.8e-7 on the logit, <= 1.2e-6 on gradients,
    relative to max|.|)."""
    B, Fn, D, kind, ratio, dnn, dense_dim = case
    emb, dense, up, P = R.sweep_draw(case)
    want_y, cache = R.forward(emb.double(), None if dense is None else dense.double(), R.double(P), kind)
    want = R.flat(R.backward(up.double(), cache))
    leaves = {k: v.clone().requires_grad_(True) for k, v in R.flat(P).items()}
    leaves["emb"] = emb.clone().requires_grad_(True)
    if dense is not None:
        leaves["dense"] = dense.clone().requires_grad_(True)
    P32 = {k: leaves[k] for k in ("w1", "w2", "bil", "lin", "out_bias")}
    P32["dnn_w"], P32["dnn_b"] = ([leaves[f"{n}.{l}"] for l in range(len(dnn))] for n in ("dnn_w", "dnn_b"))
    y = factored_forward(leaves["emb"], leaves.get("dense"), P32, kind)
    (y * up).sum().backward()
    dev_y = float((y.detach().double() - want_y).abs().max() / want_y.abs().max())
    print(f"[fibinet-premise] {R.case_id(case)}: logit {dev_y:.2e}")
    assert dev_y <= 2e-5 / 4
    assert sorted(leaves) == sorted(want)
    for k in want:
        scale = float(want[k].abs().max())
        assert scale > 0.0, k
        dev = float((leaves[k].grad.double() - want[k]).abs().max())
        print(f"[fibinet-premise] {R.case_id(case)}: {k} {dev / scale:.2e}")
        assert dev <= (1e-4 * scale + 5e-9) / 4, k
