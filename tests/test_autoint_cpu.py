"""CPU side of InteractingLayer and AutoIntHead: the restatement tests/autoint_reference.py against autograd of deepctr's literal
form and against the recorded runs of the reference's own AutoInt.forward (tests/golden/autoint, written by
tools/gen_autoint_golden.py); the ABI mirror; the modules' parameters, state_dict order, initial statistics and construction
errors; the library's descriptor checks and sizes; the premise of the GPU bounds."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from satrans_amd import native
from tests import autoint_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "autoint")
SYMBOLS = ("satrans_interacting_saved_floats", "satrans_interacting_scratch_floats", "satrans_interacting_fwd",
           "satrans_interacting_bwd", "satrans_autoint_saved_floats", "satrans_autoint_workspace_floats", "satrans_autoint_fwd",
           "satrans_autoint_bwd")
STRUCTS = (("satrans_interacting_desc", "InteractingDesc"), ("satrans_autoint_desc", "AutoIntDesc"),
           ("satrans_autoint_grads", "AutoIntGrads"))
CASES = [(c, R.HEAD_EXTRAS[i]) for i, c in enumerate(R.SWEEP)] + [(R.WALK, ((), 0))]


def ids(cx):
    c, (dnn, dense_dim) = cx
    return f"{R.case_id(c)}-dnn{'x'.join(map(str, dnn)) or 'none'}-dense{dense_dim}"


def fixture(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def close(got, want, rel, msg, floor=0.0):
    want = torch.as_tensor(want)
    err, scale = float((torch.as_tensor(got) - want).abs().max()), float(want.abs().max())
    assert err <= rel * scale + floor, (msg, err, scale)


def literal_layer(x, W, head_num, scaling):
    """deepctr's InteractingLayer.forward, literally (in-place ops spelled out of place for autograd on leaves)."""
    dh = x.shape[2] // head_num
    querys = torch.tensordot(x, W["W_Query"], dims=([-1], [0]))
    keys = torch.tensordot(x, W["W_key"], dims=([-1], [0]))
    values = torch.tensordot(x, W["W_Value"], dims=([-1], [0]))
    querys = torch.stack(torch.split(querys, dh, dim=2))
    keys = torch.stack(torch.split(keys, dh, dim=2))
    values = torch.stack(torch.split(values, dh, dim=2))
    inner_product = torch.einsum('bnik,bnjk->bnij', querys, keys)
    if scaling:
        inner_product = inner_product / dh ** 0.5
    att = F.softmax(inner_product, dim=-1)
    result = torch.matmul(att, values)
    result = torch.cat(torch.split(result, 1, ), dim=-1)
    result = torch.squeeze(result, dim=0)
    if "W_Res" in W:
        result = result + torch.tensordot(x, W["W_Res"], dims=([-1], [0]))
    return F.relu(result), att


def literal_head(emb, dense, leaves, n_layers, n_dnn, head_num, scaling, use_res):
    """autoint.py:93-121, literally; -> logit, the last layer's normalized_att_scores."""
    att_input, att = emb, None
    for l in range(n_layers):
        W = {k: leaves[f"int.{l}.{k}"] for k in (R.LAYER_KEYS if use_res else R.LAYER_KEYS[:3])}
        att_input, att = literal_layer(att_input, W, head_num, scaling)
    att_output = torch.flatten(att_input, start_dim=1)
    if n_dnn:
        h = torch.flatten(emb, start_dim=1)
        if dense is not None:
            h = torch.cat([h, dense], dim=-1)
        for l in range(n_dnn):
            h = torch.relu(F.linear(h, leaves[f"dnn_w.{l}"], leaves[f"dnn_b.{l}"]))
        att_output = torch.cat([att_output, h], dim=-1)
    return F.linear(att_output, leaves["lin"]) + leaves["out_bias"], att


def autograd_of_the_literal_form(case, dnn, emb, dense, up, P, dtype):
    """(logit, last scores, gradients) of the literal form under autograd in `dtype`, gradients under R.flat's names."""
    B, F_, D, H, L, use_res, scaling = case
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)      # noqa: E731  (a copy: the draw is shared and stays as it is)
    leaves = {k: leaf(v) for k, v in R.flat(P).items()}
    leaves["emb"] = leaf(emb)
    if dense is not None and dnn:
        leaves["dense"] = leaf(dense)
    y, att = literal_head(leaves["emb"], leaves.get("dense"), leaves, L, len(dnn), H, scaling, use_res)
    (y * up.to(dtype)).sum().backward()
    return y.detach(), att.detach(), {k: v.grad for k, v in leaves.items()}


def fp64_of(case, dnn, emb, dense, up, P):
    _, _, _, H, _, _, scaling = case
    y, cache = R.forward(emb.double(), None if dense is None or not dnn else dense.double(), R.double(P), H, scaling)
    return y, cache, R.flat(R.backward(up.double(), cache))


@pytest.mark.parametrize("cx", CASES, ids=ids)
def test_explicit_backward_equals_autograd_of_deepctrs_form(cx):
    """fp64: the restatement's forward is deepctr's literal form and its explicit backward is autograd's of that form."""
    case, (dnn, dense_dim) = cx
    emb, dense, _, up, P, _ = R.draw(case, dnn, dense_dim)
    want_y, want_att, want = autograd_of_the_literal_form(case, dnn, emb, dense, up, P, torch.float64)
    y, cache, g = fp64_of(case, dnn, emb, dense, up, P)
    assert y.shape == (emb.shape[0], 1)
    close(y, want_y, 1e-12, "forward")
    close(cache.layers[-1].p, want_att, 1e-12, "normalized_att_scores")
    assert cache.layers[-1].p.shape == (case[3], case[0], case[1], case[1])
    assert sorted(g) == sorted(want)
    for k, v in g.items():
        assert float(v.abs().max()) > 0.0, k
        close(v, want[k], 1e-10, k)


def run_fixture(fx, dtype=torch.float32):
    sd = {k[6:]: torch.from_numpy(v).to(dtype) for k, v in fx.items() if k.startswith("param/")}
    emb, dense, labels = (torch.from_numpy(fx[k]).to(dtype) for k in ("emb", "dense", "labels"))
    P = R.params_from_state(sd, dtype)
    logit, cache = R.forward(emb, dense if P["dnn_w"] else None, P, int(fx["att_head_num"]))
    leaf = logit.clone().requires_grad_(True)
    y = torch.sigmoid(leaf)
    loss = F.binary_cross_entropy(y.squeeze(1), labels, reduction='sum')
    loss.backward()
    return sd, y.detach(), loss.detach(), R.backward(leaf.grad, cache), cache


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_reproduces_every_fixture(name):
    """fp32 against the reference's fp32 run: y_pred, the loss, every parameter gradient, grad/emb and the last layer's
    normalized_att_scores within 2e-5 max|.| (contractions at most 24 long)."""
    fx = fixture(name)
    sd, y, loss, g, cache = run_fixture(fx)
    close(y, fx["y_pred"], 2e-5, "y_pred")
    assert abs(float(loss) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    grads = R.state_from_params({k: v for k, v in g.items() if k not in ("emb", "dense")})
    assert list(grads) == list(fx["keys"])
    for k, v in grads.items():
        assert float(np.abs(fx[f"grad/{k}"]).max()) > 0.0, k
        close(v, fx[f"grad/{k}"], 2e-5, k)
    close(g["emb"], fx["grad/emb"], 2e-5, "grad/emb")
    close(cache.layers[-1].p, fx["normalized_att_scores"], 2e-5, "normalized_att_scores")


def fixture_config(name):
    return {"autoint": (3, 2, True, (16, 8)), "autoint_nodnn": (3, 2, True, ()), "autoint_nores": (1, 2, False, (16, 8))}[name]


def test_fixtures_hold_the_cases_they_claim():
    assert sorted(R.FIXTURES) == sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz"))
    for name in R.FIXTURES:
        fx = fixture(name)
        L, H, res, dnn = fixture_config(name)
        assert (int(fx["att_layer_num"]), int(fx["att_head_num"]), bool(fx["att_res"])) == (L, H, res)
        B, Fn, D = fx["emb"].shape
        assert (B, Fn, D) == (24, 4, 4) and fx["dense"].shape == (B, 1) and fx["X"].shape == (B, 5)
        assert list(fx["keys"]) == R.keys_of(L, len(dnn), res)
        assert "param/dnn_linear.bias" not in fx and "linear_logit" not in fx
        assert fx["param/dnn_linear.weight"].shape == (1, Fn * D + (dnn[-1] if dnn else 0))
        if dnn:
            assert fx["param/dnn.linears.0.weight"].shape == (16, Fn * D + 1) and fx["param/dnn.linears.1.weight"].shape == (8, 16)
        assert fx["normalized_att_scores"].shape == (H, B, Fn, Fn)
        np.testing.assert_allclose(fx["normalized_att_scores"].sum(-1), 1.0, rtol=1e-6)
        assert os.path.getsize(os.path.join(GOLDEN, f"{name}.npz")) < 64 * 1024


def make_head(name):
    from satrans_amd import AutoIntHead
    L, H, res, dnn = fixture_config(name)
    return AutoIntHead(4, 4, 1, L, H, res, dnn)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_state_dict_matches_the_reference(name):
    """Keys, their order and the shapes of the head are the recorded ones, and the recorded values load."""
    fx = fixture(name)
    state = {k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    head = make_head(name)
    sd = head.state_dict()
    assert list(sd) == list(fx["keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(fx["shapes"])
    head.load_state_dict(state)
    for k, v in head.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert torch.equal(make_head(name).out.bias.detach(), torch.zeros(1))


def test_interacting_layer_is_deepctrs():
    from satrans_amd import InteractingLayer, SelfAttention_Layer
    D = 64
    torch.manual_seed(4)
    mod = InteractingLayer(D, 4)
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == [(k, (D, D)) for k in R.LAYER_KEYS]
    assert [k for k, _ in mod.named_parameters()] == list(R.LAYER_KEYS)
    assert (mod.head_num, mod.use_res, mod.scaling, mod.seed, mod.att_embedding_size) == (4, True, False, 1024, 16)
    assert mod.normalized_att_scores is None and mod.capture_attention is False
    torch.manual_seed(4)      # deepctr's: the parameters in creation order, each N(0, 0.05)
    for k in R.LAYER_KEYS:
        want = torch.nn.init.normal_(torch.empty(D, D), mean=0.0, std=0.05)
        assert torch.equal(getattr(mod, k).detach(), want), k
        assert abs(float(want.mean())) < 0.005 and abs(float(want.std()) - 0.05) < 0.005
    assert list(InteractingLayer(D, 2, use_res=False).state_dict()) == list(R.LAYER_KEYS[:3])
    with pytest.raises(ValueError, match="head_num must be a int > 0"):
        InteractingLayer(D, 0)
    with pytest.raises(ValueError, match="not an integer multiple"):
        InteractingLayer(D, 3)
    # not SelfAttention_Layer: other names, other defaults, and its checkpoint does not load
    sibling = SelfAttention_Layer(D, 4)
    assert sibling.scaling is True and "W_Key" in sibling.state_dict() and "W_Out" in sibling.state_dict()
    with pytest.raises(RuntimeError):
        mod.load_state_dict(sibling.state_dict())
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        mod(torch.randn(3, 5, D))
    with pytest.raises(ValueError, match="3 dimensions"):
        mod(torch.randn(5, D))
    with pytest.raises(ValueError):
        mod(torch.randn(3, 5, D + 1))


def test_head_refuses_what_is_not_built():
    from satrans_amd import AutoIntHead
    with pytest.raises(ValueError, match="att_layer_num"):
        AutoIntHead(4, 16, att_layer_num=0)
    with pytest.raises(ValueError):
        AutoIntHead(1, 16)
    with pytest.raises(ValueError, match="integer multiple"):
        AutoIntHead(4, 16, att_head_num=3)
    for kw in (dict(dnn_dropout=0.5), dict(dnn_activation='prelu'), dict(dnn_use_bn=True)):
        with pytest.raises(NotImplementedError, match="not built"):
            AutoIntHead(4, 16, **kw)
    with pytest.raises(NotImplementedError, match="MMOE_MAX_HIDDEN"):
        AutoIntHead(4, 16, dnn_hidden_units=(8,) * (native.MMOE_MAX_HIDDEN + 1))
    with pytest.raises(NotImplementedError, match="AUTOINT_MAX_LAYERS"):
        AutoIntHead(4, 16, att_layer_num=native.AUTOINT_MAX_LAYERS + 1)
    x = torch.randn(6, 4, 16)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        AutoIntHead(4, 16)(x)
    with pytest.raises(ValueError):
        AutoIntHead(4, 16, 2)(x)                          # dense columns missing
    with pytest.raises(ValueError):
        AutoIntHead(4, 16)(x, torch.randn(6, 1))          # dense columns unexpected
    with pytest.raises(ValueError):
        AutoIntHead(5, 16)(x)
    # the defaults are the reference's
    head = AutoIntHead(19, 32, 3)
    assert [lin.weight.shape for lin in head.dnn.linears] == [(256, 19 * 32 + 3), (128, 256)]
    assert head.dnn_linear.weight.shape == (1, 19 * 32 + 128) and head.dnn_linear.bias is None
    assert len(head.int_layers) == 3 and all(l.head_num == 2 and l.use_res and not l.scaling for l in head.int_layers)
    assert list(AutoIntHead(4, 16, 0, 2, 2, False, ()).state_dict()) == R.keys_of(2, 0, False)
    assert AutoIntHead(4, 16, 0, 1, 2, True, ()).dnn_linear.weight.shape == (1, 64)


def header_text():
    return open(os.path.join(ROOT, "include", "satrans_hip.h")).read()


def test_abi_carries_the_new_symbols(tmp_path):
    header = header_text()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    for name in ("INTERACTING_MAX_WORKGROUPS", "AUTOINT_MAX_LAYERS"):
        assert int(re.search(r"#define SATRANS_%s (\d+)" % name, header).group(1)) == getattr(native, name), name
    H, L = native.MMOE_MAX_HIDDEN, native.AUTOINT_MAX_LAYERS
    assert ctypes.sizeof(native.InteractingDesc) == 6 * 4 + 5 * 8
    assert ctypes.sizeof(native.AutoIntDesc) == (8 + H + 1) * 4 + (2 + 4 * L + 2 * H + 2) * 8
    assert ctypes.sizeof(native.AutoIntGrads) == (L + 2 * H + 2) * 8
    for struct, cls in STRUCTS:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") if decl.split()
                 for n in re.findall(r"\*?\s*(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.split(None, 1)[1])]
        names = [n for n in names if n not in ("float", "int32_t", "uint32_t", "const")]
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


def layer_desc(B, Fn, D, H, flags=0):
    d = native.InteractingDesc()
    d.B, d.F, d.D, d.H, d.flags = B, Fn, D, H, flags
    return d


def head_desc(B, Fn, D, H, L=1, dense=0, dnn=(16,), flags=0):
    d = native.AutoIntDesc()
    d.B, d.F, d.D, d.H, d.flags, d.n_layers, d.dense_dim, d.n_dnn = B, Fn, D, H, flags, L, dense, len(dnn)
    for l, w in enumerate(dnn[:native.MMOE_MAX_HIDDEN]):
        d.width[l] = w
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    by = ctypes.byref
    null_layer, null_head = (ctypes.POINTER(c)() for c in (native.InteractingDesc, native.AutoIntDesc))
    assert lib.satrans_interacting_saved_floats(null_layer) == -1 and b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_interacting_scratch_floats(null_layer) == -1
    assert lib.satrans_interacting_fwd(null_layer, None, None, None, None) == -1
    assert lib.satrans_interacting_bwd(null_layer, None, None, None, None, None, None, None) == -1
    assert lib.satrans_autoint_saved_floats(null_head) == -1 and lib.satrans_autoint_workspace_floats(null_head) == -1
    assert lib.satrans_autoint_fwd(null_head, None, None, None, None) == -1
    assert lib.satrans_autoint_bwd(null_head, None, None, None, None, None, None, None) == -1
    # outside the shapes: the sizes say -1, the launches SATRANS_E_UNSUPPORTED, before any pointer is looked at
    for B, Fn, D, H in ((8, 4, 24, 2), (8, 4, 16, 4), (8, 65, 32, 2), (8, 1, 32, 2), (8, 4, 128, 4), (8, 4, 64, 1), (8, 4, 32, 3)):
        d = layer_desc(B, Fn, D, H)
        assert lib.satrans_interacting_saved_floats(by(d)) == -1 and lib.satrans_last_error(), (B, Fn, D, H)
        assert lib.satrans_interacting_scratch_floats(by(d)) == -1
        assert lib.satrans_interacting_fwd(by(d), None, None, None, None) == -2
        assert lib.satrans_interacting_bwd(by(d), None, None, None, None, None, None, None) == -2
        h = head_desc(B, Fn, D, H)
        assert lib.satrans_autoint_saved_floats(by(h)) == -1 and lib.satrans_autoint_fwd(by(h), None, None, None, None) == -2
    for B, Fn, D, H in ((0, 4, 16, 2), (8, 0, 16, 2), (8, 4, 0, 2), (8, 4, 16, 0)):
        d = layer_desc(B, Fn, D, H)
        assert lib.satrans_interacting_saved_floats(by(d)) == -1 and lib.satrans_interacting_fwd(by(d), None, None, None, None) == -1
    assert lib.satrans_interacting_fwd(by(layer_desc(8, 4, 16, 2, 1)), None, None, None, None) == -1      # a flag of another layer
    assert b"flags" in lib.satrans_last_error()
    # the sizes over the sweep: saved is exactly the statistics; the scratch is bounded by the grid, not by B F D
    for B, Fn, D, H, L, res, scaling in R.SWEEP + [R.WALK, (1 << 20, 19, 32, 2, 3, True, False)]:
        d = layer_desc(B, Fn, D, H, (0 if res else native.NO_RES) | (0 if scaling else 128))
        assert lib.satrans_interacting_saved_floats(by(d)) == 2 * B * H * Fn
        blk = (4 if res else 3) * D * D
        ws = lib.satrans_interacting_scratch_floats(by(d))
        assert 0 < ws <= min(B, native.INTERACTING_MAX_WORKGROUPS) * blk and ws % blk == 0
        assert lib.satrans_interacting_fwd(by(d), None, None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_interacting_bwd(by(d), None, None, None, None, None, None, None) == -1
    assert lib.satrans_interacting_scratch_floats(by(layer_desc(1 << 20, 19, 32, 2))) == native.INTERACTING_MAX_WORKGROUPS * 4 * 32 * 32
    # the head
    for kw in (dict(L=0), dict(dense=-1), dict(dnn=(16, 0))):
        h = head_desc(8, 4, 16, 2, **kw)
        for rc in (lib.satrans_autoint_saved_floats(by(h)), lib.satrans_autoint_workspace_floats(by(h)),
                   lib.satrans_autoint_fwd(by(h), None, None, None, None), lib.satrans_autoint_bwd(by(h), None, None, None, None, None, None, None)):
            assert rc == -1, kw
    h = head_desc(8, 4, 16, 2, L=native.AUTOINT_MAX_LAYERS + 1)
    assert lib.satrans_autoint_fwd(by(h), None, None, None, None) == -2 and b"interacting layers" in lib.satrans_last_error()
    h = head_desc(8, 4, 16, 2)
    h.n_dnn = native.MMOE_MAX_HIDDEN + 1
    assert lib.satrans_autoint_fwd(by(h), None, None, None, None) == -2
    B, Fn, D, H, L, dense, dnn = 131, 19, 32, 2, 3, 2, (128, 64)
    ld = Fn * D + dense
    h = head_desc(B, Fn, D, H, L, dense, dnn)
    assert lib.satrans_autoint_saved_floats(by(h)) == L * B * Fn * D + L * 2 * B * H * Fn + B * ld + B * sum(dnn)
    assert lib.satrans_autoint_workspace_floats(by(h)) > 0
    assert lib.satrans_autoint_fwd(by(h), None, None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_autoint_bwd(by(h), None, None, None, None, None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    h = head_desc(B, Fn, D, H, L, 0, ())
    assert lib.satrans_autoint_saved_floats(by(h)) == L * B * Fn * D + L * 2 * B * H * Fn


@pytest.mark.parametrize("cx", CASES, ids=ids)
def test_premise_of_the_gpu_bounds(cx):
    """The GPU tests hold the kernels to 2e-5 max|.| on results and 1e-4 max|g| + 5e-9 on gradients.  On every
    swept shape torch's own fp32 run of the literal form under autograd stays within a quarter of those bounds against the
    fp64 restatement, and every relu tensor's smallest |pre-activation| (each interacting layer's o + r, the DNN's) is at
    least 1e-4 of its largest: a differently ordered fp32 sum cannot flip a relu and change a gradient discretely."""
    case, (dnn, dense_dim) = cx
    emb, dense, _, up, P, used = R.draw(case, dnn, dense_dim)
    want_y, cache, want = fp64_of(case, dnn, emb, dense, up, P)
    margins = R.kink_margins(cache)
    print(f"[autoint-premise] {ids(cx)}: redraw rounds {used}, kink margins {' '.join(f'{m:.2e}' for m in margins)}")
    assert len(margins) == case[4] + len(dnn) and min(margins) >= 1e-4
    y, att, got = autograd_of_the_literal_form(case, dnn, emb, dense, up, P, torch.float32)
    dev_y = float((y.double() - want_y).abs().max() / want_y.abs().max())
    dev_a = float((att.double() - cache.layers[-1].p).abs().max() / cache.layers[-1].p.abs().max())
    print(f"[autoint-premise] {ids(cx)}: logit {dev_y:.2e} normalized_att_scores {dev_a:.2e}")
    assert dev_y <= 2e-5 / 4 and dev_a <= 2e-5 / 4
    assert sorted(got) == sorted(want)
    worst = 0.0
    for k in want:
        scale = float(want[k].abs().max())
        dev = float((got[k].double() - want[k]).abs().max())
        worst = max(worst, dev / (1e-4 * scale + 5e-9))
        assert dev <= (1e-4 * scale + 5e-9) / 4, k
    print(f"[autoint-premise] {ids(cx)}: worst gradient at {worst:.3f} of its bound")
