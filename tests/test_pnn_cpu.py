"""CPU side of PNN's inner and outer product layers and head: the restatement tests/pnn_reference.py against autograd of deepctr's
literal form and against the recorded runs of the reference's own PNN.forward (tests/golden/pnn, written by
tools/gen_pnn_golden.py); the ABI mirror; the modules' parameters, state_dict order and construction errors; the premise of the
GPU bounds."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from satrans_amd import native
from tests import pnn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pnn")
SYMBOLS = ("satrans_inner_product_fwd", "satrans_inner_product_bwd", "satrans_outer_product_workspace_floats",
           "satrans_outer_product_fwd", "satrans_outer_product_bwd", "satrans_pnn_saved_floats", "satrans_pnn_workspace_floats",
           "satrans_pnn_fwd", "satrans_pnn_bwd")
STRUCTS = (("satrans_inner_product_desc", "InnerProductDesc"), ("satrans_outer_product_desc", "OuterProductDesc"),
           ("satrans_pnn_desc", "PNNDesc"), ("satrans_pnn_grads", "PNNGrads"))


def fixture(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def close(got, want, rel, msg, floor=0.0):
    want = torch.as_tensor(want)
    err, scale = float((torch.as_tensor(got) - want).abs().max()), float(want.abs().max())
    assert err <= rel * scale + floor, (msg, err, scale)


def literal_forward(e, dn, leaves, cfg, n_dnn):
    """deepctr and pnn.py:91-114, literally, on the list of [B, 1, D] pieces."""
    use_inner, use_outter, kind = cfg
    pieces = list(torch.split(e, 1, dim=1))
    row, col = zip(*R.pairs(e.shape[1]))
    parts = [torch.flatten(torch.cat(pieces, dim=-1), start_dim=1)]
    p = torch.cat([pieces[i] for i in row], dim=1)
    q = torch.cat([pieces[j] for j in col], dim=1)
    if use_inner:
        parts.append(torch.flatten(torch.sum(p * q, dim=2, keepdim=True), start_dim=1))
    if use_outter:
        if kind == "mat":
            parts.append(torch.sum(torch.mul(torch.transpose(torch.sum(torch.mul(p.unsqueeze(1), leaves["kernel"]), dim=-1), 2, 1), q),
                                   dim=-1))
        else:
            parts.append(torch.sum(p * q * torch.unsqueeze(leaves["kernel"], 0), dim=-1))
    h = torch.cat(parts, dim=1)
    if dn is not None:
        h = torch.cat([h, dn], dim=-1)
    for l in range(n_dnn):
        h = torch.relu(F.linear(h, leaves[f"dnn_w.{l}"], leaves[f"dnn_b.{l}"]))
    return F.linear(h, leaves["lin"]) + leaves["out_bias"]


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_explicit_backward_equals_autograd_of_deepctrs_form(case):
    """fp64: the restatement's forward is deepctr's literal form (the two gathers, the [B, D, P, D] product of 'mat'), and its
    explicit backward is autograd's of that form.  No sample of a draw sits near a kink, and no gradient is identically zero."""
    B, Fn, D, use_inner, use_outter, kind, dnn, dense_dim = case
    emb, dense, up, P = R.sweep_draw(case)
    leaves = {k: v.double().requires_grad_(True) for k, v in R.flat(P).items()}
    e = emb.double().requires_grad_(True)
    dn = None if dense is None else dense.double().requires_grad_(True)
    want_y = literal_forward(e, dn, leaves, case[3:6], len(dnn))
    (want_y * up.double()).sum().backward()
    y, cache = R.forward(emb.double(), None if dense is None else dense.double(), R.double(P), case[3:6])
    n_pairs = Fn * (Fn - 1) // 2
    assert y.shape == (B, 1) and cache.X.shape == (B, Fn * D + n_pairs * (int(use_inner) + int(use_outter)) + dense_dim)
    assert not bool(R.near_kink(cache, 2e-5).any())
    close(y, want_y.detach(), 1e-12, "forward")
    g = R.flat(R.backward(up.double(), cache))
    close(g.pop("emb"), e.grad, 1e-11, "demb")
    if dn is not None:
        close(g.pop("dense"), dn.grad, 1e-11, "ddense")
    assert sorted(g) == sorted(leaves) and ("kernel" in g) == bool(use_outter)
    for k, v in g.items():
        assert float(v.abs().max()) > 0.0, k
        close(v, leaves[k].grad, 1e-11, k)


def run_fixture(fx, dtype=torch.float32):
    cfg = (bool(fx["use_inner"]), bool(fx["use_outter"]), str(fx["kernel_type"]))
    sd = {k[6:]: torch.from_numpy(v).to(dtype) for k, v in fx.items() if k.startswith("param/")}
    emb, dense, labels = (torch.from_numpy(fx[k]).to(dtype) for k in ("emb", "dense", "labels"))
    logit, cache = R.forward(emb, dense, R.params_from_state(sd, dtype), cfg)
    leaf = logit.clone().requires_grad_(True)
    y = torch.sigmoid(leaf)
    loss = F.binary_cross_entropy(y.squeeze(1), labels, reduction='sum')
    loss.backward()
    return sd, y.detach(), loss.detach(), R.backward(leaf.grad, cache)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_reproduces_every_fixture(name):
    """fp32 against the reference's fp32 run: y_pred, the loss, every parameter gradient, grad/emb and reg_loss within 2e-5
    max|.| (the DNN input is at most 29 wide).  The gradients come from the explicit backward, fed d loss / d logit."""
    fx = fixture(name)
    sd, y, loss, g = run_fixture(fx)
    close(y, fx["y_pred"], 2e-5, "y_pred")
    assert abs(float(loss) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    grads = R.state_from_params(g)
    assert list(grads) == list(fx["keys"])
    for k, v in grads.items():
        assert float(np.abs(fx[f"grad/{k}"]).max()) > 0.0, k
        close(v, fx[f"grad/{k}"], 2e-5, k)
    close(g["emb"], fx["grad/emb"], 2e-5, "grad/emb")
    assert fx["reg_loss"].shape == (1,) and float(fx["reg_loss"][0]) > 0.0
    close(R.reg_loss(sd, float(fx["l2_reg_dnn"])), fx["reg_loss"], 2e-5, "reg_loss")


def test_fixtures_hold_the_cases_they_claim():
    assert sorted(R.FIXTURES) == sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz"))
    for name in R.FIXTURES:
        fx = fixture(name)
        use_inner, use_outter, kind = R.FIXTURE_CONFIG[name]
        assert (bool(fx["use_inner"]), bool(fx["use_outter"])) == (use_inner, use_outter)
        assert str(fx["kernel_type"]) == kind
        assert list(fx["keys"]) == R.keys_of(use_outter, 2)
        B, Fn, D = fx["emb"].shape
        assert (B, Fn, D) == (24, 4, 4) and fx["dense"].shape == (B, 1) and fx["X"].shape == (B, 5)
        assert ("param/outterproduct.kernel" in fx) == use_outter
        if use_outter:
            assert fx["param/outterproduct.kernel"].shape == R.kernel_shape(4, 4, kind)
        n = 16 + 6 * (int(use_inner) + int(use_outter)) + 1
        assert fx["param/dnn.linears.0.weight"].shape == (16, n) and fx["param/dnn.linears.1.weight"].shape == (8, 16)
        assert fx["param/dnn_linear.weight"].shape == (1, 8)
        # PNN.__init__ registers the DNN's weights and dnn_linear.weight, and l2_reg_dnn is not zero
        assert int(fx["n_own_reg"]) == 2 and float(fx["l2_reg_dnn"]) > 0.0 and float(fx["reg_loss"][0]) > 0.0
        assert os.path.getsize(os.path.join(GOLDEN, f"{name}.npz")) < 64 * 1024


@pytest.mark.parametrize("name", R.FIXTURES)
def test_state_dict_matches_the_reference(name):
    """Keys, their order and the shapes of PNNHead are the recorded ones, the recorded values load, and regularization_loss()
    is the recorded one."""
    from satrans_amd import PNNHead
    fx = fixture(name)
    use_inner, use_outter, kind = R.FIXTURE_CONFIG[name]
    state = {k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    head = PNNHead(4, 4, 1, (16, 8), use_inner, use_outter, kind, l2_reg_dnn=float(fx["l2_reg_dnn"]))
    sd = head.state_dict()
    assert list(sd) == list(fx["keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(fx["shapes"])
    head.load_state_dict(state)
    for k, v in head.state_dict().items():
        assert torch.equal(v, state[k]), k
    reg = head.regularization_loss()      # plain torch: runs on the CPU too
    assert reg.shape == (1,) and torch.equal(reg.detach(), torch.from_numpy(fx["reg_loss"]))
    assert float(PNNHead(4, 4, 1, (16, 8), use_inner, use_outter, kind).regularization_loss()) == 0.0      # l2_reg_dnn = 0
    assert float(head.out.bias.detach().abs().max()) > 0.0
    assert torch.equal(PNNHead(4, 4, 1).out.bias.detach(), torch.zeros(1))


def test_outer_product_layer_has_deepctrs_initial_bits():
    from satrans_amd import InnerProductLayer, OutterProductLayer
    Fn, D = 7, 5
    n_pairs = Fn * (Fn - 1) // 2
    for kind, shape in (("mat", (D, n_pairs, D)), ("vec", (n_pairs, D)), ("num", (n_pairs, 1))):
        torch.manual_seed(4)
        mod = OutterProductLayer(Fn, D, kind, 1024, device='cpu')
        torch.manual_seed(4)      # deepctr's: nn.Parameter(torch.Tensor(*shape)), then nn.init.xavier_uniform_
        want = nn.init.xavier_uniform_(nn.Parameter(torch.Tensor(*shape)))
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == [("kernel", shape)]
        assert torch.equal(mod.kernel.detach(), want.detach()) and float(want.detach().abs().max()) > 0.0
    assert OutterProductLayer(Fn, D).kernel_type == "mat"
    assert list(InnerProductLayer().state_dict()) == [] and list(InnerProductLayer(device='cpu').parameters()) == []


def test_modules_refuse_what_is_not_built():
    from satrans_amd import InnerProductLayer, OutterProductLayer, PNNHead
    with pytest.raises(ValueError, match="kernel_type must be mat,vec or num"):
        OutterProductLayer(4, 8, 'some')
    with pytest.raises(ValueError, match="kernel_type must be mat,vec or num"):
        PNNHead(4, 8, kernel_type='some')
    with pytest.raises(NotImplementedError, match="reduce_sum"):
        InnerProductLayer(reduce_sum=False)
    with pytest.raises(ValueError):
        PNNHead(1, 8)
    with pytest.raises(ValueError):
        OutterProductLayer(1, 8)
    with pytest.raises(NotImplementedError, match="PNN_MAX_FIELDS"):
        PNNHead(native.PNN_MAX_FIELDS + 1, 4)
    with pytest.raises(NotImplementedError, match="PNN_MAX_FIELDS"):
        OutterProductLayer(native.PNN_MAX_FIELDS + 1, 4)
    with pytest.raises(NotImplementedError, match="PNN_MAX_DIM"):
        PNNHead(4, native.PNN_MAX_DIM + 1)
    with pytest.raises(NotImplementedError, match="PNN_MAX_DIM"):
        OutterProductLayer(4, native.PNN_MAX_DIM + 1)
    with pytest.raises(NotImplementedError, match="MMOE_MAX_HIDDEN"):
        PNNHead(4, 8, 0, (8,) * (native.MMOE_MAX_HIDDEN + 1))
    for kw in (dict(dnn_dropout=0.5), dict(dnn_activation='prelu')):
        with pytest.raises(NotImplementedError, match="not built"):
            PNNHead(4, 8, **kw)
    wide = PNNHead(native.PNN_MAX_FIELDS, 4, 0, (8,), True, True, 'num')
    assert wide.dnn.linears[0].weight.shape == (8, 64 * 4 + 2 * 2016) and wide.outterproduct.kernel.shape == (2016, 1)
    x = torch.randn(6, 4, 8)
    for mod in (InnerProductLayer(), OutterProductLayer(4, 8), PNNHead(4, 8, 0, (16,), True, True)):
        with pytest.raises(native.NativeError, match="no CPU fallback"):
            mod(x)
    for mod in (InnerProductLayer(), OutterProductLayer(4, 8)):
        with pytest.raises(ValueError):
            mod(x[0])
    with pytest.raises(ValueError):
        PNNHead(4, 8, 2)(x)                       # dense columns missing
    with pytest.raises(ValueError):
        PNNHead(4, 8)(x, torch.randn(6, 1))       # dense columns unexpected
    # the defaults are the reference's: inner products only
    plain = PNNHead(4, 8, 3)
    assert plain.use_inner and not plain.use_outter and list(plain.state_dict()) == R.keys_of(False, 2)
    assert plain.dnn.linears[0].weight.shape == (128, 4 * 8 + 6 + 3)
    no_dnn = PNNHead(4, 8, 3, (), False, True, 'vec')
    assert list(no_dnn.state_dict()) == R.keys_of(True, 0) and no_dnn.dnn_linear.weight.shape == (1, 4 * 8 + 6 + 3)
    neither = PNNHead(4, 8, 0, (16,), False, False)
    assert list(neither.state_dict()) == R.keys_of(False, 1) and neither.dnn.linears[0].weight.shape == (16, 32)


def header_text():
    return open(os.path.join(ROOT, "include", "satrans_hip.h")).read()


def test_abi_carries_the_new_symbols(tmp_path):
    header = header_text()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    for name in ("MAX_FIELDS", "MAX_DIM", "DW_ROW_CHUNK"):
        assert int(re.search(r"#define SATRANS_PNN_%s (\d+)" % name, header).group(1)) == getattr(native, f"PNN_{name}"), name
    for name, code in native.PNN_KERNEL_TYPES.items():
        assert int(re.search(r"#define SATRANS_PNN_KERNEL_%s (\d+)" % name.upper(), header).group(1)) == code
    assert native.PNN_MAX_FIELDS == 64 and native.PNN_MAX_DIM == 128
    H = native.MMOE_MAX_HIDDEN
    assert ctypes.sizeof(native.InnerProductDesc) == 4 * 4 + 8 and ctypes.sizeof(native.OuterProductDesc) == 4 * 4 + 2 * 8
    assert ctypes.sizeof(native.PNNGrads) == (3 + 2 * H) * 8
    assert ctypes.sizeof(native.PNNDesc) == (8 + H + 1) * 4 + (2 + 3 + 2 * H) * 8
    for struct, cls in STRUCTS:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") if decl.split()
                 for n in re.findall(r"\*?\s*(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.split(None, 1)[1])]
        names = [n for n in names if n not in ("float", "int32_t", "const")]
        assert names == [f[0] for f in getattr(native, cls)._fields_], (struct, names)
    # the header's own sizes and offsets, from a tiny host program compiled against it
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler"
    fields = [(struct, cls, f[0]) for struct, cls in STRUCTS for f in getattr(native, cls)._fields_]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "satrans_hip.h"', "int main(void) {"]
    src += ['    printf("%%zu\\n", sizeof(%s));' % struct for struct, _ in STRUCTS]
    src += ['    printf("%%zu\\n", offsetof(%s, %s));' % (struct, f) for struct, _, f in fields]
    src += ["    return 0;", "}"]
    (tmp_path / "sizes.c").write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "sizes")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "sizes.c"), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(getattr(native, cls)) for _, cls in STRUCTS]
    want += [getattr(getattr(native, cls), f).offset for _, cls, f in fields]
    assert got == want


def head_desc(B, Fn, D, inner=1, outer=1, kind=0, dense=0, dnn=()):
    d = native.PNNDesc()
    d.B, d.F, d.D, d.use_inner, d.use_outer, d.kernel_type, d.dense_dim, d.n_dnn = B, Fn, D, inner, outer, kind, dense, len(dnn)
    for l, w in enumerate(dnn[:native.MMOE_MAX_HIDDEN]):
        d.width[l] = w
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    by = ctypes.byref
    null_head, null_in, null_out = (ctypes.POINTER(c)() for c in (native.PNNDesc, native.InnerProductDesc, native.OuterProductDesc))
    assert lib.satrans_pnn_saved_floats(null_head) == -1 and b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_pnn_workspace_floats(null_head) == -1
    assert lib.satrans_pnn_fwd(null_head, None, None, None) == -1
    assert lib.satrans_pnn_bwd(null_head, None, None, None, None, None, None, None) == -1
    assert lib.satrans_inner_product_fwd(null_in, None, None) == -1
    assert lib.satrans_inner_product_bwd(null_in, None, None, None) == -1
    assert lib.satrans_outer_product_workspace_floats(null_out) == -1
    assert lib.satrans_outer_product_fwd(null_out, None, None) == -1
    assert lib.satrans_outer_product_bwd(null_out, None, None, None, None, None) == -1
    bad = [dict(B=0, Fn=4, D=8), dict(B=8, Fn=1, D=8), dict(B=8, Fn=4, D=0), dict(B=8, Fn=4, D=8, kind=3), dict(B=8, Fn=4, D=8, kind=-1),
           dict(B=8, Fn=4, D=8, dense=-1), dict(B=8, Fn=4, D=8, dnn=(16, 0))]
    for kw in bad:
        d = head_desc(**kw)
        for rc in (lib.satrans_pnn_saved_floats(by(d)), lib.satrans_pnn_workspace_floats(by(d)), lib.satrans_pnn_fwd(by(d), None, None, None),
                   lib.satrans_pnn_bwd(by(d), None, None, None, None, None, None, None)):
            assert rc == -1, kw
    beyond = [dict(B=8, Fn=native.PNN_MAX_FIELDS + 1, D=8), dict(B=8, Fn=4, D=native.PNN_MAX_DIM + 1),
              dict(B=(1 << 31) - 1, Fn=64, D=128), dict(B=(1 << 31) - 1, Fn=4, D=8, dnn=(4096,))]      # (the last: the DNN's grid alone)
    for kw in beyond:
        d = head_desc(**kw)
        assert lib.satrans_pnn_saved_floats(by(d)) == -2, kw
        assert lib.satrans_pnn_fwd(by(d), None, None, None) == -2 and lib.satrans_last_error(), kw
    d = head_desc(8, 4, 8)
    d.n_dnn = native.MMOE_MAX_HIDDEN + 1
    assert lib.satrans_pnn_saved_floats(by(d)) == -2 and b"hidden layers" in lib.satrans_last_error()
    # sizes, at the AliCCP shape with a ragged batch
    B, Fn, D, dense, dnn = 131, 19, 32, 2, (128, 64)
    n_pairs = Fn * (Fn - 1) // 2
    chunks, mm_chunks = -(-B // native.PNN_DW_ROW_CHUNK), -(-B // native.MMOE_DW_ROW_CHUNK)
    for inner, outer, kind, kpart in ((1, 1, 0, n_pairs * D * D), (1, 0, 0, 0), (0, 1, 1, n_pairs * D), (1, 1, 2, n_pairs * D), (0, 0, 0, 0)):
        ld = Fn * D + n_pairs * (inner + outer) + dense
        d = head_desc(B, Fn, D, inner, outer, kind, dense, dnn)
        assert lib.satrans_pnn_saved_floats(by(d)) == B * ld + B * sum(dnn)
        parts = max(mm_chunks * 128 * (ld + 1), chunks * kpart)
        assert lib.satrans_pnn_workspace_floats(by(d)) == B * ld + 2 * B * max(dnn) + parts
        assert lib.satrans_pnn_fwd(by(d), None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_pnn_bwd(by(d), None, None, None, None, None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    for kind, kpart in ((0, n_pairs * D * D), (1, n_pairs * D), (2, n_pairs * D)):
        o = native.OuterProductDesc()
        o.B, o.F, o.D, o.kernel_type = B, Fn, D, kind
        assert lib.satrans_outer_product_workspace_floats(by(o)) == chunks * kpart
        assert lib.satrans_outer_product_fwd(by(o), None, None) == -1 and b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_outer_product_bwd(by(o), None, None, None, None, None) == -1
    o.kernel_type = 3
    assert lib.satrans_outer_product_workspace_floats(by(o)) == -1 and b"kernel_type" in lib.satrans_last_error()
    i = native.InnerProductDesc()
    i.B, i.F, i.D = B, Fn, D
    assert lib.satrans_inner_product_fwd(by(i), None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_inner_product_bwd(by(i), None, None, None) == -1
    i.F = native.PNN_MAX_FIELDS + 1
    assert lib.satrans_inner_product_fwd(by(i), None, None) == -2


def factored_forward(emb, dense, P, cfg):
    """The arithmetic of the kernels in torch: one product per pair, no gathered [B, P, D] tensors, no [B, D, P, D] product."""
    use_inner, use_outter, kind = cfg
    idx = torch.tensor(R.pairs(emb.shape[1]))
    ei, ej = emb[:, idx[:, 0]], emb[:, idx[:, 1]]
    parts = [emb.flatten(1)]
    if use_inner:
        parts.append((ei * ej).sum(-1))
    if use_outter:
        if kind == "mat":
            parts.append((torch.einsum("bpk,npk->bpn", ei, P["kernel"]) * ej).sum(-1))
        elif kind == "vec":
            parts.append((ei * ej * P["kernel"]).sum(-1))
        else:
            parts.append((ei * ej).sum(-1) * P["kernel"][:, 0])
    h = torch.cat(parts + ([] if dense is None else [dense]), -1)
    for w, b in zip(P["dnn_w"], P["dnn_b"]):
        h = torch.relu(h @ w.T + b)
    return h @ P["lin"].T + P["out_bias"]


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_premise_of_the_gpu_bounds(case):
    """The GPU tests hold the kernels to 2e-5 max|.| on results and 1e-4 max|g| + 5e-9 on gradients.  On every
    swept shape torch's own fp32 run of the FACTORED form - the kernels' arithmetic, under autograd - stays within a quarter of
    those bounds against the fp64 literal form (measured: <= 4.6e-7 on the logit, <= 5.5e-7 on gradients, relative to max|.|)."""
    B, Fn, D, use_inner, use_outter, kind, dnn, dense_dim = case
    emb, dense, up, P = R.sweep_draw(case)
    want_y, cache = R.forward(emb.double(), None if dense is None else dense.double(), R.double(P), case[3:6])
    want = R.flat(R.backward(up.double(), cache))
    leaves = {k: v.clone().requires_grad_(True) for k, v in R.flat(P).items()}
    leaves["emb"] = emb.clone().requires_grad_(True)
    if dense is not None:
        leaves["dense"] = dense.clone().requires_grad_(True)
    P32 = {k: leaves[k] for k in ("kernel", "lin", "out_bias") if k in leaves}
    P32["dnn_w"], P32["dnn_b"] = ([leaves[f"{n}.{l}"] for l in range(len(dnn))] for n in ("dnn_w", "dnn_b"))
    y = factored_forward(leaves["emb"], leaves.get("dense"), P32, case[3:6])
    (y * up).sum().backward()
    dev_y = float((y.detach().double() - want_y).abs().max() / want_y.abs().max())
    print(f"[pnn-premise] {R.case_id(case)}: logit {dev_y:.2e}")
    assert dev_y <= 2e-5 / 4
    assert sorted(leaves) == sorted(want)
    for k in want:
        scale = float(want[k].abs().max())
        assert scale > 0.0, k
        dev = float((leaves[k].grad.double() - want[k]).abs().max())
        print(f"[pnn-premise] {R.case_id(case)}: {k} {dev / scale:.2e}")
        assert dev <= (1e-4 * scale + 5e-9) / 4, k
