"""CPU side of the compressed interaction network: the restatement tests/cin_reference.py against autograd of the einsum form
and against the recorded runs of the reference's own xDeepFM.forward (tests/golden/cin, written by tools/gen_cin_golden.py);
the ABI mirror; the modules' parameters, state_dict order and construction errors; the premise of the GPU bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from satrans_amd import native
from tests import cin_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cin")
CASES = ("plain", "nosplit", "cin_only")
SYMBOLS = ("satrans_cin_saved_floats", "satrans_cin_workspace_floats", "satrans_cin_fwd", "satrans_cin_bwd")


def fixture(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def close(got, want, rel, msg):
    want = torch.as_tensor(want)
    err, scale = float((torch.as_tensor(got) - want).abs().max()), float(want.abs().max())
    assert err <= rel * scale, (msg, err, scale)


@pytest.mark.parametrize("case", R.SWEEP[:4] + R.SWEEP[6:], ids=R.case_id)
def test_explicit_backward_equals_autograd_of_the_einsum_form(case):
    """fp64: the restatement's forward is deepctr's einsum + reshape + conv1d + relu + split, and its explicit backward is
    autograd's of that form."""
    B, M, D, layers, split = case
    x, up, P = R.sweep_draw(case)
    xl = x.double().requires_grad_(True)
    Pl = {k: [t.double().requires_grad_(True) for t in v] for k, v in P.items()}
    hidden, final = xl, []
    for i, size in enumerate(layers):
        z = torch.einsum('bhd,bmd->bhmd', hidden, xl).reshape(B, hidden.shape[1] * M, D)
        z = torch.relu(F.conv1d(z, Pl["w"][i].unsqueeze(-1), Pl["b"][i]))
        if split and i != len(layers) - 1:
            hidden, direct = torch.split(z, 2 * [size // 2], 1)
        else:
            hidden = direct = z
        final.append(direct)
    want_y = torch.cat(final, dim=1).sum(-1)
    (want_y * up.double()).sum().backward()
    y, cache = R.forward(x.double(), R.double(P), split)
    assert y.shape == (B, R.featuremap_num(layers, split))
    close(y, want_y.detach(), 1e-12, "forward")
    g = R.backward(up.double(), cache)
    close(g["x"], xl.grad, 1e-11, "dx")
    for i in range(len(layers)):
        close(g["w"][i], Pl["w"][i].grad, 1e-11, f"dw[{i}]")
        close(g["b"][i], Pl["b"][i].grad, 1e-11, f"db[{i}]")


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_every_fixture(name):
    """fp32 against the reference's fp32 run: y_pred, the loss, every parameter gradient and grad/emb within 2e-5 max|.| (the
    contractions are at most 33 long).  The CIN's own gradients come from the explicit backward, fed d loss / d result."""
    fx = fixture(name)
    split = bool(fx["split_half"])
    sd = {k[6:]: torch.from_numpy(v).requires_grad_(True) for k, v in fx.items() if k.startswith("param/")}
    emb = torch.from_numpy(fx["emb"]).requires_grad_(True)
    dense, lin, labels = (torch.from_numpy(fx[k]) for k in ("dense", "linear_logit", "labels"))
    P = R.params_from_state({k: v.detach() for k, v in sd.items()}, "cin.", torch.float32)
    cin_out, cache = R.forward(emb.detach(), P, split)
    cin_leaf = cin_out.clone().requires_grad_(True)
    y = torch.sigmoid(R.head_forward(emb, dense, lin, sd, split, cin_out=cin_leaf))
    loss = F.binary_cross_entropy(y.squeeze(1), labels, reduction='sum')
    loss.backward()
    close(y.detach(), fx["y_pred"], 2e-5, "y_pred")
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    g = R.backward(cin_leaf.grad, cache)
    grads = {k: v.grad for k, v in sd.items() if not k.startswith("cin.")}
    grads.update(R.state_from_params(g, "cin."))
    assert sorted(grads) == sorted(sd)
    for k, v in grads.items():
        assert float(np.abs(fx[f"grad/{k}"]).max()) > 0.0, k
        close(v, fx[f"grad/{k}"], 2e-5, k)
    demb = g["x"] + (emb.grad if emb.grad is not None else 0)
    close(demb, fx["grad/emb"], 2e-5, "grad/emb")


def test_fixtures_hold_the_cases_they_claim():
    want = {"plain": ((8, 6), 1, 2), "nosplit": ((6, 5), 0, 2), "cin_only": ((8, 6), 1, 0)}
    for name, (cin, split, n_dnn) in want.items():
        fx = fixture(name)
        assert int(fx["split_half"]) == split
        assert tuple(fx[f"param/cin.conv1ds.{i}.weight"].shape[0] for i in range(2)) == cin
        assert list(fx["keys"]) == R.keys_of(n_dnn, 2)
        B, Fn, D = fx["emb"].shape
        assert (Fn, D) == (4, 4) and fx["dense"].shape == (B, 1) and fx["X"].shape == (B, 5)
        h1 = cin[0] // 2 if split else cin[0]
        assert fx["param/cin.conv1ds.1.weight"].shape == (cin[1], h1 * Fn, 1)
        assert fx["param/cin_linear.weight"].shape == (1, R.featuremap_num(cin, bool(split)))


@pytest.mark.parametrize("name", CASES)
def test_state_dict_matches_the_reference(name):
    """Keys, their order and the shapes of XDeepFMHead are the recorded ones, and the recorded values load."""
    from satrans_amd import XDeepFMHead
    fx = fixture(name)
    state = {k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    dnn = tuple(state[f"dnn.linears.{l}.weight"].shape[0] for l in range(2)) if name != "cin_only" else ()
    cin = tuple(state[f"cin.conv1ds.{i}.weight"].shape[0] for i in range(2))
    head = XDeepFMHead(4, 4, 1, dnn, cin, bool(fx["split_half"]))
    sd = head.state_dict()
    assert list(sd) == list(fx["keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(fx["shapes"])
    head.load_state_dict(state)
    assert head.featuremap_num == state["cin_linear.weight"].shape[1]


def test_cin_parameters_are_deepctrs():
    from satrans_amd import CIN
    torch.manual_seed(3)
    cin = CIN(19, (256, 128), 'relu', True, 1e-5, 1024, device='cpu')
    assert [(k, tuple(v.shape)) for k, v in cin.state_dict().items()] == [
        ("conv1ds.0.weight", (256, 361, 1)), ("conv1ds.0.bias", (256,)), ("conv1ds.1.weight", (128, 2432, 1)),
        ("conv1ds.1.bias", (128,))]
    assert cin.featuremap_num == 256 and cin.field_nums == [19, 128, 64]
    assert CIN(5, (6, 5), split_half=False).featuremap_num == 11
    torch.manual_seed(3)      # torch's Conv1d default initialisation, in layer order
    for i, (c_in, c_out) in enumerate(((361, 256), (2432, 128))):
        ref = torch.nn.Conv1d(c_in, c_out, 1)
        assert torch.equal(ref.weight, cin.conv1ds[i].weight) and torch.equal(ref.bias, cin.conv1ds[i].bias)


def test_modules_refuse_what_is_not_built():
    from satrans_amd import CIN, XDeepFMHead
    with pytest.raises(NotImplementedError, match="relu"):
        CIN(4, (8, 6), activation='sigmoid')
    with pytest.raises(ValueError, match="even"):
        CIN(4, (7, 6), split_half=True)
    assert CIN(4, (8, 7), split_half=True).featuremap_num == 11      # the last layer may be odd
    assert CIN(4, (7, 6), split_half=False).featuremap_num == 13
    with pytest.raises(NotImplementedError, match="layers"):
        CIN(4, (8,) * (native.CIN_MAX_LAYERS + 1))
    with pytest.raises(NotImplementedError, match="fields"):
        CIN(native.CIN_MAX_FIELDS + 1, (8, 6))
    with pytest.raises(NotImplementedError, match="sizes"):
        CIN(4, (native.CIN_MAX_WIDTH + 2, 6))
    with pytest.raises(ValueError):
        CIN(4, ())
    with pytest.raises(ValueError):
        CIN(0, (8, 6))
    assert CIN(native.CIN_MAX_FIELDS, (native.CIN_MAX_WIDTH,) * native.CIN_MAX_LAYERS, split_half=False).featuremap_num == 1024
    x = torch.randn(6, 4, 8)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        CIN(4, (8, 6))(x)
    with pytest.raises(ValueError):
        CIN(4, (8, 6))(x[:, :3])
    with pytest.raises(ValueError):
        CIN(4, (8, 6))(x[0])
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        XDeepFMHead(4, 8, 0, (16,), (8, 6))(x)
    with pytest.raises(ValueError):
        XDeepFMHead(4, 8, 2, (16,), (8, 6))(x)
    with pytest.raises(ValueError, match="even"):
        XDeepFMHead(4, 8, 0, (16,), (7, 6))
    assert list(XDeepFMHead(4, 8, 0, (), (8, 6)).state_dict()) == R.keys_of(0, 2)
    assert list(XDeepFMHead(4, 8, 0, (16,), ()).state_dict()) == R.keys_of(1, 0)


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    for name in ("MAX_LAYERS", "MAX_FIELDS", "MAX_WIDTH", "ROW_TILE", "DW_ROW_CHUNK"):
        assert int(re.search(r"#define SATRANS_CIN_%s (\d+)" % name, header).group(1)) == getattr(native, f"CIN_{name}"), name
    assert native.CIN_MAX_LAYERS >= 4 and native.CIN_MAX_FIELDS >= 64 and native.CIN_MAX_WIDTH >= 256
    L = native.CIN_MAX_LAYERS
    assert ctypes.sizeof(native.CINDesc) == (6 + L) * 4 + (1 + 2 * L) * 8
    assert ctypes.sizeof(native.CINGrads) == 2 * L * 8
    for struct, cls in (("satrans_cin_desc", native.CINDesc), ("satrans_cin_grads", native.CINGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") if decl.split()
                 for n in re.findall(r"\*?\s*(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.split(None, 1)[1])]
        names = [n for n in names if n not in ("float", "int32_t", "const")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def cin_desc(B, M, D, layers, split):
    d = native.CINDesc()
    d.B, d.M, d.D, d.L, d.split_half = B, M, D, len(layers), split
    for i, n in enumerate(layers[:native.CIN_MAX_LAYERS]):
        d.width[i] = n
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    null = ctypes.POINTER(native.CINDesc)()
    assert lib.satrans_cin_saved_floats(null) == -1 and b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_cin_workspace_floats(null) == -1
    assert lib.satrans_cin_fwd(null, None, None, None) == -1
    assert lib.satrans_cin_bwd(null, None, None, None, None, None, None) == -1
    ok = (8, 5, 4, (8, 6), 1)
    bad = [(0,) + ok[1:], (8, 0, 4, (8, 6), 1), (8, 5, -1, (8, 6), 1), (8, 5, 4, (), 1), (8, 5, 4, (8, 0), 1), (8, 5, 4, (7, 6), 1),
           (8, 5, 4, (8, 6), 2)]
    for args in bad:
        d = cin_desc(*args)
        for rc in (lib.satrans_cin_saved_floats(ctypes.byref(d)), lib.satrans_cin_workspace_floats(ctypes.byref(d)),
                   lib.satrans_cin_fwd(ctypes.byref(d), None, None, None),
                   lib.satrans_cin_bwd(ctypes.byref(d), None, None, None, None, None, None)):
            assert rc == -1, args
    beyond = [(8, native.CIN_MAX_FIELDS + 1, 4, (8, 6), 1), (8, 5, 4, (8,) * (native.CIN_MAX_LAYERS + 1), 0),
              (8, 5, 4, (native.CIN_MAX_WIDTH + 2, 6), 1), (1 << 20, 5, 1 << 12, (8, 6), 1)]
    for args in beyond:
        d = cin_desc(*args)
        assert lib.satrans_cin_saved_floats(ctypes.byref(d)) == -2, args
        assert lib.satrans_cin_fwd(ctypes.byref(d), None, None, None) == -2, args
    assert lib.satrans_cin_saved_floats(ctypes.byref(cin_desc(8, 5, 4, (7, 6), 0))) == 8 * 4 * 13      # odd is fine unsplit
    assert lib.satrans_cin_saved_floats(ctypes.byref(cin_desc(8, 5, 4, (8, 7), 1))) == 8 * 4 * 15      # and in the last layer
    # sizes: saved = every layer's activations; workspace = dz + dX of the layer above + the widest layer's chunk partials
    B, M, D, layers = 131, 19, 32, (16, 8)
    rows = B * D
    chunks = -(-rows // native.CIN_DW_ROW_CHUNK)
    d = cin_desc(B, M, D, layers, 1)
    assert lib.satrans_cin_saved_floats(ctypes.byref(d)) == rows * 24
    part = chunks * max(16 * (M * M + 1), 8 * (8 * M + 1))
    assert lib.satrans_cin_workspace_floats(ctypes.byref(d)) == rows * 16 + rows * 8 + part
    d1 = cin_desc(B, M, D, (65,), 0)
    assert lib.satrans_cin_workspace_floats(ctypes.byref(d1)) == rows * 65 + chunks * 65 * (M * M + 1)
    for dd in (d, d1):
        assert lib.satrans_cin_fwd(ctypes.byref(dd), None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_cin_bwd(ctypes.byref(dd), None, None, None, None, None, None) == -1
        assert b"null pointer" in lib.satrans_last_error()


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_premise_of_the_gpu_bounds(case):
    """The GPU tests hold the kernels to 2e-5 max|.| on results and 1e-4 max|g| + 5e-9 on gradients.  On every
    swept shape the seeded draw ends (no sample within the result bound of relu's kink is left; decided by the fp64 forward
    alone), and torch's own fp32 run of the restatement stays within a quarter of those bounds against fp64 (measured:
    <= 2.4e-7 on results, <= 6.0e-7 on gradients, relative to max|.|)."""
    B, M, D, layers, split = case
    x, up, P = R.sweep_draw(case)
    want_y, cache = R.forward(x.double(), R.double(P), split)
    assert R.kink_margin(cache) >= 2e-5
    want = R.flat(R.backward(up.double(), cache))
    y, c32 = R.forward(x, P, split)
    got = R.flat(R.backward(up, c32))
    dev_y = float((y.double() - want_y).abs().max() / want_y.abs().max())
    print(f"[cin-premise] {R.case_id(case)}: result {dev_y:.2e}")
    assert dev_y <= 2e-5 / 4
    assert sorted(got) == sorted(want)
    for k in want:
        scale = float(want[k].abs().max())
        assert scale > 0.0, k
        dev = float((got[k].double() - want[k]).abs().max())
        print(f"[cin-premise] {R.case_id(case)}: {k} {dev / scale:.2e}")
        assert dev <= (1e-4 * scale + 5e-9) / 4, k


def test_draw_refuses_to_go_on_forever():
    with pytest.raises(RuntimeError, match="rounds"):
        R.draw(64, 19, 32, (256, 128), True, 1, rel=0.5, rounds=2)
