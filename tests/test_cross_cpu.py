"""CPU side of DCN's cross network: the restatement tests/cross_reference.py against autograd of deepctr's literal tensordot /
matmul form and against the recorded runs of the reference's own DCN.forward (tests/golden/dcn, written by
tools/gen_dcn_golden.py); the ABI mirror; the modules' parameters, state_dict order and construction errors; the premise of the
GPU bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from satrans_amd import native
from tests import cross_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dcn")
CASES = ("vector", "matrix", "cross_only")
SYMBOLS = ("satrans_cross_saved_floats", "satrans_cross_workspace_floats", "satrans_cross_fwd", "satrans_cross_bwd")


def fixture(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def close(got, want, rel, msg):
    want = torch.as_tensor(want)
    err, scale = float((torch.as_tensor(got) - want).abs().max()), float(want.abs().max())
    assert err <= rel * scale, (msg, err, scale)


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_explicit_backward_equals_autograd_of_deepctrs_form(case):
    """fp64: the restatement's forward is deepctr's unsqueeze + tensordot + matmul (vector) or matmul + Hadamard (matrix) form,
    and its explicit backward is autograd's of that form."""
    B, N, L, matrix = case
    x, up, P = R.sweep_draw(case)
    xl = x.double().requires_grad_(True)
    kernels = (P["kernels"] if matrix else P["kernels"].unsqueeze(-1)).double().requires_grad_(True)      # deepctr's shapes
    bias = P["bias"].unsqueeze(-1).double().requires_grad_(True)
    x_0 = xl.unsqueeze(2)
    x_l = x_0
    for i in range(L):
        if matrix:
            x_l = x_0 * (torch.matmul(kernels[i], x_l) + bias[i]) + x_l
        else:
            xl_w = torch.tensordot(x_l, kernels[i], dims=([1], [0]))
            x_l = torch.matmul(x_0, xl_w) + bias[i] + x_l
    want_y = torch.squeeze(x_l, dim=2)
    (want_y * up.double()).sum().backward()
    y, cache = R.forward(x.double(), R.double(P), matrix)
    assert y.shape == (B, N)
    close(y, want_y.detach(), 1e-12, "forward")
    g = R.backward(up.double(), cache)
    close(g["x"], xl.grad, 1e-11, "dx")
    close(g["kernels"], kernels.grad.reshape(g["kernels"].shape), 1e-11, "dkernels")
    close(g["bias"], bias.grad.squeeze(-1), 1e-11, "dbias")


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_every_fixture(name):
    """fp32 against the reference's fp32 run: y_pred, the loss, every parameter gradient, grad/emb and reg_loss within 2e-5
    max|.| (N = 17).  The cross network's own gradients come from the explicit backward, fed d loss / d result."""
    fx = fixture(name)
    matrix = bool(fx["matrix"])
    sd = {k[6:]: torch.from_numpy(v).requires_grad_(True) for k, v in fx.items() if k.startswith("param/")}
    emb = torch.from_numpy(fx["emb"]).requires_grad_(True)
    dense, lin, labels = (torch.from_numpy(fx[k]) for k in ("dense", "linear_logit", "labels"))
    P = R.params_from_state({k: v.detach() for k, v in sd.items()}, "crossnet.", torch.float32)
    assert (P["kernels"].dim() == 3) == matrix
    x = torch.cat([emb.detach().flatten(1), dense], -1)
    cross_out, cache = R.forward(x, P, matrix)
    leaf = cross_out.clone().requires_grad_(True)
    y = torch.sigmoid(R.head_forward(emb, dense, lin, sd, cross_out=leaf))
    loss = F.binary_cross_entropy(y.squeeze(1), labels, reduction='sum')
    loss.backward()
    close(y.detach(), fx["y_pred"], 2e-5, "y_pred")
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    g = R.backward(leaf.grad, cache)
    grads = {k: v.grad for k, v in sd.items() if not k.startswith("crossnet.")}
    grads.update(R.state_from_params(g, "crossnet."))
    assert sorted(grads) == sorted(sd)
    for k, v in grads.items():
        assert float(np.abs(fx[f"grad/{k}"]).max()) > 0.0, k
        close(v, fx[f"grad/{k}"], 2e-5, k)
    dflat = g["x"][:, :emb[0].numel()].reshape(emb.shape)
    demb = dflat + (emb.grad if emb.grad is not None else 0)
    close(demb, fx["grad/emb"], 2e-5, "grad/emb")
    assert fx["reg_loss"].shape == (1,) and float(fx["reg_loss"][0]) > 0.0
    close(R.reg_loss({k: v.detach() for k, v in sd.items()}), fx["reg_loss"], 2e-5, "reg_loss")


def test_fixtures_hold_the_cases_they_claim():
    want = {"vector": (2, 0, 2), "matrix": (3, 1, 2), "cross_only": (2, 0, 0)}
    for name, (cross, matrix, n_dnn) in want.items():
        fx = fixture(name)
        assert int(fx["matrix"]) == matrix
        assert list(fx["keys"]) == R.keys_of(n_dnn)
        B, Fn, D = fx["emb"].shape
        assert (B, Fn, D) == (24, 4, 4) and fx["dense"].shape == (B, 1) and fx["X"].shape == (B, 5)
        n = Fn * D + 1
        assert fx["param/crossnet.kernels"].shape == (cross, n, n if matrix else 1)
        assert fx["param/crossnet.bias"].shape == (cross, n, 1)
        assert fx["param/dnn_linear.weight"].shape == (1, n + (8 if n_dnn else 0))
        if n_dnn:
            assert fx["param/dnn.linears.0.weight"].shape == (16, n) and fx["param/dnn.linears.1.weight"].shape == (8, 16)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_matches_the_reference(name):
    """Keys, their order and the shapes of DCNHead are the recorded ones, and the recorded values load."""
    from satrans_amd import DCNHead
    fx = fixture(name)
    state = {k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    dnn = (16, 8) if name != "cross_only" else ()
    head = DCNHead(4, 4, 1, state["crossnet.kernels"].shape[0], "matrix" if int(fx["matrix"]) else "vector", dnn)
    sd = head.state_dict()
    assert list(sd) == list(fx["keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(fx["shapes"])
    head.load_state_dict(state)
    close(head.regularization_loss().detach(), fx["reg_loss"], 2e-5, "reg_loss")      # plain torch: runs on the CPU too


@pytest.mark.parametrize("form", ("vector", "matrix"))
def test_crossnet_parameters_are_deepctrs(form):
    from satrans_amd import CrossNet
    n, L = 37, 3
    torch.manual_seed(3)
    net = CrossNet(n, L, form, 1024, device='cpu')
    width = 1 if form == "vector" else n
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [("kernels", (L, n, width)), ("bias", (L, n, 1))]
    torch.manual_seed(3)      # deepctr's order: xavier_normal_ of each kernels[i], then zeros for the bias
    ref = torch.empty(L, n, width)
    for i in range(L):
        torch.nn.init.xavier_normal_(ref[i])
    assert torch.equal(ref, net.kernels.detach()) and float(ref.abs().max()) > 0.0
    assert torch.equal(net.bias.detach(), torch.zeros(L, n, 1))
    zero = CrossNet(n, 0, form)
    assert [tuple(v.shape) for v in zero.state_dict().values()] == [(0, n, width), (0, n, 1)]


def test_modules_refuse_what_is_not_built():
    from satrans_amd import CrossNet, DCNHead
    with pytest.raises(ValueError, match="parameterization should be 'vector' or 'matrix'"):
        CrossNet(8, 2, 'tensor')
    with pytest.raises(NotImplementedError, match="layers"):
        CrossNet(8, native.CROSS_MAX_LAYERS + 1)
    with pytest.raises(NotImplementedError, match="features"):
        CrossNet(native.CROSS_MAX_FEATURES + 1, 1)
    with pytest.raises(ValueError):
        CrossNet(0, 2)
    assert CrossNet(native.CROSS_MAX_FEATURES, native.CROSS_MAX_LAYERS).kernels.shape == (8, 4096, 1)
    x = torch.randn(6, 8)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        CrossNet(8, 2)(x)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        CrossNet(8, 0)(x)
    with pytest.raises(ValueError):
        CrossNet(8, 2)(x[:, :7])
    with pytest.raises(ValueError):
        CrossNet(8, 2)(x[0])
    emb = torch.randn(6, 4, 8)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        DCNHead(4, 8, 0, 2, 'vector', (16,))(emb)
    with pytest.raises(ValueError):
        DCNHead(4, 8, 2, 2, 'vector', (16,))(emb)
    with pytest.raises(ValueError, match="parameterization"):
        DCNHead(4, 8, 0, 2, 'tensor', (16,))
    with pytest.raises(ValueError):
        DCNHead(4, 8, 0, 0, 'vector', ())
    assert list(DCNHead(4, 8, 0, 2, 'matrix', ()).state_dict()) == R.keys_of(0)
    only_deep = DCNHead(4, 8, 0, 0, 'vector', (16,))
    assert list(only_deep.state_dict()) == R.keys_of(1) and only_deep.dnn_linear.weight.shape == (1, 16)
    assert DCNHead(4, 8, 3, 2, 'vector', (16, 8)).dnn_linear.weight.shape == (1, 35 + 8)


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    for name in ("MAX_LAYERS", "MAX_FEATURES", "VEC_ROW_CHUNK"):
        assert int(re.search(r"#define SATRANS_CROSS_%s (\d+)" % name, header).group(1)) == getattr(native, f"CROSS_{name}"), name
    assert native.CROSS_MAX_LAYERS >= 8 and native.CROSS_MAX_FEATURES >= 4096
    assert ctypes.sizeof(native.CrossDesc) == 4 * 4 + 3 * 8
    assert ctypes.sizeof(native.CrossGrads) == 2 * 8
    for struct, cls in (("satrans_cross_desc", native.CrossDesc), ("satrans_cross_grads", native.CrossGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") if decl.split()
                 for n in re.findall(r"\*?\s*(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.split(None, 1)[1])]
        names = [n for n in names if n not in ("float", "int32_t", "const")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def cross_desc(B, N, L, matrix):
    d = native.CrossDesc()
    d.B, d.N, d.L, d.matrix = B, N, L, matrix
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    null = ctypes.POINTER(native.CrossDesc)()
    assert lib.satrans_cross_saved_floats(null) == -1 and b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_cross_workspace_floats(null) == -1
    assert lib.satrans_cross_fwd(null, None, None, None) == -1
    assert lib.satrans_cross_bwd(null, None, None, None, None, None, None) == -1
    for args in [(0, 8, 2, 0), (8, 0, 2, 1), (8, 8, 0, 0), (-3, 8, 2, 1), (8, 8, 2, 2), (8, 8, 2, -1)]:
        d = cross_desc(*args)
        for rc in (lib.satrans_cross_saved_floats(ctypes.byref(d)), lib.satrans_cross_workspace_floats(ctypes.byref(d)),
                   lib.satrans_cross_fwd(ctypes.byref(d), None, None, None),
                   lib.satrans_cross_bwd(ctypes.byref(d), None, None, None, None, None, None)):
            assert rc == -1, args
    beyond = [(8, native.CROSS_MAX_FEATURES + 1, 2, 0), (8, 8, native.CROSS_MAX_LAYERS + 1, 1), (8, native.CROSS_MAX_FEATURES + 1, 2, 1),
              ((1 << 31) - 1, 4096, 1, 1)]
    for args in beyond:
        d = cross_desc(*args)
        assert lib.satrans_cross_saved_floats(ctypes.byref(d)) == -2, args
        assert lib.satrans_cross_fwd(ctypes.byref(d), None, None, None) == -2, args
    # sizes.  vector: saved = s [B, L]; workspace = the two partials of every row chunk.  matrix: saved = u_l of every layer
    # and x_1 .. x_{L-1}; workspace = du, g and one layer's partials [chunks][N (N + 1)]
    B, N, L = 131, 608, 3
    v, m = cross_desc(B, N, L, 0), cross_desc(B, N, L, 1)
    assert lib.satrans_cross_saved_floats(ctypes.byref(v)) == B * L
    assert lib.satrans_cross_workspace_floats(ctypes.byref(v)) == 2 * -(-B // native.CROSS_VEC_ROW_CHUNK) * L * N
    assert lib.satrans_cross_saved_floats(ctypes.byref(m)) == (2 * L - 1) * B * N
    assert lib.satrans_cross_workspace_floats(ctypes.byref(m)) == 2 * B * N + -(-B // native.MMOE_DW_ROW_CHUNK) * N * (N + 1)
    top = cross_desc((1 << 31) - 1, native.CROSS_MAX_FEATURES, native.CROSS_MAX_LAYERS, 0)      # the vector form's grids always fit
    assert lib.satrans_cross_saved_floats(ctypes.byref(top)) == ((1 << 31) - 1) * native.CROSS_MAX_LAYERS
    for dd in (v, m):
        assert lib.satrans_cross_fwd(ctypes.byref(dd), None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_cross_bwd(ctypes.byref(dd), None, None, None, None, None, None) == -1
        assert b"null pointer" in lib.satrans_last_error()


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_premise_of_the_gpu_bounds(case):
    """The GPU tests hold the kernels to 2e-5 max|.| on results and 1e-4 max|g| + 5e-9 on gradients.  On every
    swept shape torch's own fp32 run of the restatement stays within a quarter of those bounds against fp64 (measured:
    <= 4.4e-7 on results, <= 6.4e-7 on gradients, relative to max|.|)."""
    B, N, L, matrix = case
    x, up, P = R.sweep_draw(case)
    want_y, cache = R.forward(x.double(), R.double(P), matrix)
    want = R.backward(up.double(), cache)
    y, c32 = R.forward(x, P, matrix)
    got = R.backward(up, c32)
    dev_y = float((y.double() - want_y).abs().max() / want_y.abs().max())
    print(f"[cross-premise] {R.case_id(case)}: result {dev_y:.2e}")
    assert dev_y <= 2e-5 / 4
    assert sorted(got) == sorted(want)
    for k in want:
        scale = float(want[k].abs().max())
        assert scale > 0.0, k
        dev = float((got[k].double() - want[k]).abs().max())
        print(f"[cross-premise] {R.case_id(case)}: {k} {dev / scale:.2e}")
        assert dev <= (1e-4 * scale + 5e-9) / 4, k
