"""CPU side of FM, BiInteractionPooling, AFMLayer and the DeepFM / NFM / AFM heads: the restatement tests/fm_reference.py against
autograd of deepctr's literal form and against the recorded runs of the reference's own DeepFM.forward, NFM.forward and
AFM.forward (tests/golden/fm, written by tools/gen_fm_golden.py); the ABI mirror; the modules' parameters, state_dict order,
initial bits and construction errors; the library's descriptor checks and sizes; the premise of the GPU bounds."""
import ctypes
import itertools
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
from tests import fm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fm")
SYMBOLS = ("satrans_fm_fwd", "satrans_fm_bwd", "satrans_bipool_fwd", "satrans_bipool_bwd", "satrans_afm_saved_floats",
           "satrans_afm_workspace_floats", "satrans_afm_fwd", "satrans_afm_bwd", "satrans_fmhead_saved_floats",
           "satrans_fmhead_workspace_floats", "satrans_fmhead_fwd", "satrans_fmhead_bwd")
STRUCTS = (("satrans_fm_desc", "FMDesc"), ("satrans_afm_desc", "AFMDesc"), ("satrans_afm_grads", "AFMGrads"),
           ("satrans_fmhead_desc", "FMHeadDesc"), ("satrans_fmhead_grads", "FMHeadGrads"))


def fixture(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def close(got, want, rel, msg, floor=0.0):
    want = torch.as_tensor(want)
    err, scale = float((torch.as_tensor(got) - want).abs().max()), float(want.abs().max())
    assert err <= rel * scale + floor, (msg, err, scale)


def literal_afm(e, leaves):
    """deepctr's AFMLayer.forward, literally, on the list of [B, 1, D] pieces."""
    row, col = zip(*itertools.combinations(list(torch.split(e, 1, dim=1)), 2))
    bi = torch.cat(row, dim=1) * torch.cat(col, dim=1)
    temp = F.relu(torch.tensordot(bi, leaves["W"], dims=([-1], [0])) + leaves["b"])
    score = F.softmax(torch.tensordot(temp, leaves["h"], dims=([-1], [0])), dim=1)
    return torch.tensordot(torch.sum(score * bi, dim=1), leaves["p"], dims=([-1], [0])), score


def literal_head(kind, e, dn, lin, leaves, n_dnn, use_fm):
    """deepfm.py:87-113 / nfm.py:73-83 / afm.py:66-73, literally."""
    logit = lin
    if kind == "afm":
        return logit + literal_afm(e, leaves)[0] + leaves["out_bias"]
    sq = torch.pow(torch.sum(e, dim=1, keepdim=True), 2) - torch.sum(e * e, dim=1, keepdim=True)
    if kind == "deepfm" and use_fm:
        logit = logit + 0.5 * torch.sum(sq, dim=2, keepdim=False)
    if n_dnn:
        h = torch.flatten(0.5 * sq if kind == "nfm" else e, start_dim=1)
        if dn is not None:
            h = torch.cat([h, dn], dim=-1)
        for l in range(n_dnn):
            h = torch.relu(F.linear(h, leaves[f"dnn_w.{l}"], leaves[f"dnn_b.{l}"]))
        logit = logit + F.linear(h, leaves["lin"])
    return logit + leaves["out_bias"]


def autograd_against_explicit(kind, emb, dense, lin, up, P, n_dnn, use_fm, dtype):
    """(logit, gradients) of the literal form under autograd in `dtype`, gradients under R.flat's names."""
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in R.flat(P).items()}
    leaves["emb"] = emb.to(dtype).requires_grad_(True)
    leaves["lin_logit"] = lin.to(dtype).requires_grad_(True)
    if dense is not None:
        leaves["dense"] = dense.to(dtype).requires_grad_(True)
    y = literal_head(kind, leaves["emb"], leaves.get("dense"), leaves["lin_logit"], leaves, n_dnn, use_fm)
    (y * up.to(dtype)).sum().backward()
    return y.detach(), {k: v.grad for k, v in leaves.items()}


def all_cases():
    return [("afm",) + c for c in R.AFM_SWEEP] + list(R.HEAD_SWEEP)


def case_id(c):
    return "afm-" + R.afm_id(c[1:]) if c[0] == "afm" else R.head_id(c)


def draw_of(c):
    """kind, emb, dense, lin_logit, up, P, n_dnn, use_fm, rounds of any sweep case."""
    if c[0] == "afm":
        emb, lin, up, P, used = R.afm_draw(c[1:])
        return "afm", emb, None, lin, up, P, 0, True, used
    emb, dense, lin, up, P, used = R.head_draw(c)
    return c[0], emb, dense, lin, up, P, len(c[4]), c[6], used


@pytest.mark.parametrize("case", all_cases(), ids=case_id)
def test_explicit_backward_equals_autograd_of_deepctrs_form(case):
    """fp64: the restatement's forward is deepctr's literal form and its explicit backward is autograd's of that form.  No sample
    of a draw sits near a kink; the redraw needs at most 18 rounds."""
    kind, emb, dense, lin, up, P, n_dnn, use_fm, used = draw_of(case)
    assert used <= 18
    want_y, want = autograd_against_explicit(kind, emb, dense, lin, up, P, n_dnn, use_fm, torch.float64)
    y, cache = R.forward(kind, emb.double(), None if dense is None else dense.double(), lin.double(), R.double(P), use_fm)
    assert y.shape == (emb.shape[0], 1) and not bool(R.near_kink(cache, 2e-5).any())
    close(y, want_y, 1e-12, "forward")
    g = R.flat(R.backward(up.double(), cache))
    assert sorted(g) == sorted(want)
    one_pair = kind == "afm" and emb.shape[1] == 2
    for k, v in g.items():
        if one_pair and k in ("W", "b", "h"):      # the softmax over one pair is the constant 1
            assert float(v.abs().max()) == 0.0 and float(want[k].abs().max()) == 0.0, k
            continue
        assert float(v.abs().max()) > 0.0, k
        close(v, want[k], 1e-11, k)
    if kind == "afm":
        close(cache.afm.a, literal_afm(emb.double(), R.double(P))[1], 1e-12, "normalized_att_score")
        assert cache.afm.a.shape == (emb.shape[0], len(R.pairs(emb.shape[1])), 1)


def run_fixture(fx, dtype=torch.float32):
    kind = str(fx["kind"])
    sd = {k[6:]: torch.from_numpy(v).to(dtype) for k, v in fx.items() if k.startswith("param/")}
    emb, dense, lin, labels = (torch.from_numpy(fx[k]).to(dtype) for k in ("emb", "dense", "linear_logit", "labels"))
    P = R.params_from_state(sd, dtype)
    has_dnn = kind != "afm" and len(P["dnn_w"]) > 0
    logit, cache = R.forward(kind, emb, dense if has_dnn else None, lin, P)
    leaf = logit.clone().requires_grad_(True)
    y = torch.sigmoid(leaf)
    loss = F.binary_cross_entropy(y.squeeze(1), labels, reduction='sum')
    loss.backward()
    return sd, y.detach(), loss.detach(), R.backward(leaf.grad, cache), cache


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_reproduces_every_fixture(name):
    """fp32 against the reference's fp32 run: y_pred, the loss, every parameter gradient, grad/emb, reg_loss and AFM's
    normalized_att_score within 2e-5 max|.| (contractions at most 17 long)."""
    fx = fixture(name)
    sd, y, loss, g, cache = run_fixture(fx)
    close(y, fx["y_pred"], 2e-5, "y_pred")
    assert abs(float(loss) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    grads = R.state_from_params({k: v for k, v in g.items() if k not in ("emb", "dense", "lin_logit")})
    assert list(grads) == list(fx["keys"])
    for k, v in grads.items():
        assert float(np.abs(fx[f"grad/{k}"]).max()) > 0.0, k
        close(v, fx[f"grad/{k}"], 2e-5, k)
    close(g["emb"], fx["grad/emb"], 2e-5, "grad/emb")
    close(R.reg_loss(sd, float(fx["l2"])), fx["reg_loss"], 2e-5, "reg_loss")
    if str(fx["kind"]) == "afm":
        close(cache.afm.a, fx["normalized_att_score"], 2e-5, "normalized_att_score")


def test_fixtures_hold_the_cases_they_claim():
    assert sorted(R.FIXTURES) == sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz"))
    for name in R.FIXTURES:
        fx = fixture(name)
        kind = R.FIXTURE_KIND[name]
        assert str(fx["kind"]) == kind
        B, Fn, D = fx["emb"].shape
        assert (B, Fn, D) == (24, 4, 4) and fx["dense"].shape == (B, 1) and fx["X"].shape == (B, 5)
        assert fx["linear_logit"].shape == (B, 1) and float(np.abs(fx["linear_logit"]).max()) > 0.0
        n_dnn = 0 if name in ("deepfm_nodnn", "afm", "afm_wide") else 2
        assert list(fx["keys"]) == R.keys_of(kind, n_dnn)
        if kind == "afm":
            A = 5 if name == "afm_wide" else 3
            assert fx["param/fm.attention_W"].shape == (D, A) and fx["param/fm.attention_b"].shape == (A,)
            assert fx["param/fm.projection_h"].shape == (A, 1) and fx["param/fm.projection_p"].shape == (D, 1)
            assert fx["normalized_att_score"].shape == (B, 6, 1)
            np.testing.assert_allclose(fx["normalized_att_score"].sum(1), 1.0, rtol=1e-6)
            assert int(fx["n_own_reg"]) == 1
        elif n_dnn:
            n = (D if kind == "nfm" else Fn * D) + 1
            assert fx["param/dnn.linears.0.weight"].shape == (16, n) and fx["param/dnn.linears.1.weight"].shape == (8, 16)
            assert fx["param/dnn_linear.weight"].shape == (1, 8) and int(fx["n_own_reg"]) == 2
        else:
            assert int(fx["n_own_reg"]) == 0 and float(fx["reg_loss"][0]) == 0.0
        assert float(fx["l2"]) > 0.0 and (float(fx["reg_loss"][0]) > 0.0) == (name != "deepfm_nodnn")
        assert os.path.getsize(os.path.join(GOLDEN, f"{name}.npz")) < 64 * 1024


def make_head(name, fx, l2=None):
    from satrans_amd import AFMHead, DeepFMHead, NFMHead
    l2 = float(fx["l2"]) if l2 is None else l2
    if name == "deepfm":
        return DeepFMHead(4, 4, 1, True, (16, 8), l2_reg_dnn=l2)
    if name == "deepfm_nodnn":
        return DeepFMHead(4, 4, 1, True, (), l2_reg_dnn=l2)
    if name == "nfm":
        return NFMHead(4, 1, (16, 8), l2_reg_dnn=l2)
    return AFMHead(4, 5 if name == "afm_wide" else 3, l2_reg_att=l2)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_state_dict_matches_the_reference(name):
    """Keys, their order and the shapes of the three heads are the recorded ones, the recorded values load, and
    regularization_loss() is the recorded one."""
    fx = fixture(name)
    state = {k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    head = make_head(name, fx)
    sd = head.state_dict()
    assert list(sd) == list(fx["keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(fx["shapes"])
    head.load_state_dict(state)
    for k, v in head.state_dict().items():
        assert torch.equal(v, state[k]), k
    reg = head.regularization_loss()      # plain torch: runs on the CPU too
    assert reg.shape == (1,) and torch.equal(reg.detach(), torch.from_numpy(fx["reg_loss"]))
    assert float(make_head(name, fx, 0.0).regularization_loss()) == 0.0
    assert torch.equal(make_head(name, fx).out.bias.detach(), torch.zeros(1))


def test_afm_layer_has_deepctrs_initial_bits():
    from satrans_amd import FM, AFMLayer, BiInteractionPooling
    D, A = 6, 5
    torch.manual_seed(4)
    mod = AFMLayer(D, A, 0, 0, 1024, device='cpu')
    torch.manual_seed(4)      # deepctr's: four nn.Parameter(torch.Tensor(...)), then xavier_normal_ on W, h, p, zeros on b
    W, b, h, p = (nn.Parameter(torch.Tensor(*s)) for s in ((D, A), (A,), (A, 1), (D, 1)))
    for t in (W, h, p):
        nn.init.xavier_normal_(t)
    nn.init.zeros_(b)
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == [
        ("attention_W", (D, A)), ("attention_b", (A,)), ("projection_h", (A, 1)), ("projection_p", (D, 1))]
    for got, want in ((mod.attention_W, W), (mod.attention_b, b), (mod.projection_h, h), (mod.projection_p, p)):
        assert torch.equal(got.detach(), want.detach())
    assert float(W.detach().abs().max()) > 0.0 and AFMLayer(D).attention_factor == 4 and mod.normalized_att_score is None
    assert list(FM().state_dict()) == [] and list(BiInteractionPooling().parameters()) == []


def test_modules_refuse_what_is_not_built():
    from satrans_amd import FM, AFMHead, AFMLayer, BiInteractionPooling, DeepFMHead, NFMHead
    with pytest.raises(NotImplementedError, match="dropout"):
        AFMLayer(8, dropout_rate=0.5)
    with pytest.raises(NotImplementedError, match="dropout"):
        AFMHead(8, afm_dropout=0.5)
    with pytest.raises(NotImplementedError, match="AFM_MAX_FACTOR"):
        AFMLayer(8, native.AFM_MAX_FACTOR + 1)
    with pytest.raises(NotImplementedError, match="FM_MAX_DIM"):
        AFMLayer(native.FM_MAX_DIM + 1)
    with pytest.raises(NotImplementedError, match="FM_MAX_DIM"):
        AFMHead(native.FM_MAX_DIM + 1)
    with pytest.raises(NotImplementedError, match="FM_MAX_DIM"):
        DeepFMHead(4, native.FM_MAX_DIM + 1)
    with pytest.raises(NotImplementedError, match="FM_MAX_DIM"):
        NFMHead(native.FM_MAX_DIM + 1)
    with pytest.raises(NotImplementedError, match="FM_MAX_FIELDS"):
        DeepFMHead(native.FM_MAX_FIELDS + 1, 4)
    with pytest.raises(NotImplementedError, match="MMOE_MAX_HIDDEN"):
        DeepFMHead(4, 8, 0, True, (8,) * (native.MMOE_MAX_HIDDEN + 1))
    with pytest.raises(NotImplementedError, match="MMOE_MAX_HIDDEN"):
        NFMHead(8, 0, (8,) * (native.MMOE_MAX_HIDDEN + 1))
    for kw in (dict(dnn_dropout=0.5), dict(dnn_activation='prelu'), dict(dnn_use_bn=True)):
        with pytest.raises(NotImplementedError, match="not built"):
            DeepFMHead(4, 8, **kw)
    for kw in (dict(bi_dropout=0.5), dict(dnn_dropout=0.5), dict(dnn_activation='prelu')):
        with pytest.raises(NotImplementedError, match="not built"):
            NFMHead(8, **kw)
    with pytest.raises(ValueError, match="neither"):
        DeepFMHead(4, 8, use_fm=False, dnn_hidden_units=())
    with pytest.raises(ValueError):
        DeepFMHead(1, 8)
    with pytest.raises(ValueError):
        NFMHead(8, dnn_hidden_units=())
    x = torch.randn(6, 4, 8)
    for mod in (FM(), BiInteractionPooling(), AFMLayer(8), AFMHead(8), DeepFMHead(4, 8), NFMHead(8)):
        with pytest.raises(native.NativeError, match="no CPU fallback"):
            mod(x)
    for mod in (FM(), BiInteractionPooling(), AFMLayer(8)):
        with pytest.raises(ValueError):
            mod(x[0])
    with pytest.raises(ValueError):
        DeepFMHead(4, 8, 2)(x)                        # dense columns missing
    with pytest.raises(ValueError):
        NFMHead(8)(x, torch.randn(6, 1))              # dense columns unexpected
    # the defaults are the reference's
    assert [lin.weight.shape for lin in DeepFMHead(4, 8, 3).dnn.linears] == [(256, 35), (128, 256)]
    assert [lin.weight.shape for lin in NFMHead(8, 3).dnn.linears] == [(128, 11), (128, 128)]
    assert AFMHead(8).fm.attention_W.shape == (8, 8) and AFMHead(8).l2_reg_att == 1e-5
    assert list(DeepFMHead(4, 8, 0, True, ()).state_dict()) == ["out.bias"]
    assert list(DeepFMHead(4, 8, 0, False, (16,)).state_dict()) == R.keys_of("deepfm", 1)
    wide = AFMHead(native.FM_MAX_DIM, native.AFM_MAX_FACTOR)
    assert wide.fm.attention_W.shape == (128, 64)


def header_text():
    return open(os.path.join(ROOT, "include", "satrans_hip.h")).read()


def test_abi_carries_the_new_symbols(tmp_path):
    header = header_text()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    for name in ("FM_MAX_FIELDS", "FM_MAX_DIM", "AFM_MAX_FACTOR", "AFM_MAX_WORKGROUPS", "FMHEAD_DEEPFM", "FMHEAD_NFM"):
        assert int(re.search(r"#define SATRANS_%s (\d+)" % name, header).group(1)) == getattr(native, name), name
    assert (native.FM_MAX_FIELDS, native.FM_MAX_DIM, native.AFM_MAX_FACTOR) == (64, 128, 64)
    H = native.MMOE_MAX_HIDDEN
    assert ctypes.sizeof(native.FMDesc) == 4 * 4 + 8 and ctypes.sizeof(native.AFMDesc) == 4 * 4 + 7 * 8
    assert ctypes.sizeof(native.AFMGrads) == 5 * 8 and ctypes.sizeof(native.FMHeadGrads) == (2 + 2 * H) * 8
    assert ctypes.sizeof(native.FMHeadDesc) == (8 + H + 1) * 4 + (3 + 2 + 2 * H) * 8
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


def afm_desc(B, Fn, D, A):
    d = native.AFMDesc()
    d.B, d.F, d.D, d.A = B, Fn, D, A
    return d


def head_desc(B, Fn, D, kind=0, use_fm=1, dense=0, dnn=(16,)):
    d = native.FMHeadDesc()
    d.B, d.F, d.D, d.kind, d.use_fm, d.dense_dim, d.n_dnn = B, Fn, D, kind, use_fm, dense, len(dnn)
    for l, w in enumerate(dnn[:native.MMOE_MAX_HIDDEN]):
        d.width[l] = w
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    by = ctypes.byref
    null_fm, null_afm, null_head = (ctypes.POINTER(c)() for c in (native.FMDesc, native.AFMDesc, native.FMHeadDesc))
    for fn in (lib.satrans_fm_fwd, lib.satrans_bipool_fwd):
        assert fn(null_fm, None, None) == -1 and b"null descriptor" in lib.satrans_last_error()
    for fn in (lib.satrans_fm_bwd, lib.satrans_bipool_bwd):
        assert fn(null_fm, None, None, None) == -1
    assert lib.satrans_afm_saved_floats(null_afm) == -1 and b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_afm_workspace_floats(null_afm) == -1
    assert lib.satrans_afm_fwd(null_afm, None, None, None) == -1
    assert lib.satrans_afm_bwd(null_afm, None, None, None, None, None, None) == -1
    assert lib.satrans_fmhead_saved_floats(null_head) == -1 and b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_fmhead_workspace_floats(null_head) == -1
    assert lib.satrans_fmhead_fwd(null_head, None, None, None) == -1
    assert lib.satrans_fmhead_bwd(null_head, None, None, None, None, None, None, None) == -1
    for B, Fn, D, A in ((0, 4, 8, 4), (8, 1, 8, 4), (8, 4, 0, 4), (8, 4, 8, 0)):
        d = afm_desc(B, Fn, D, A)
        assert lib.satrans_afm_saved_floats(by(d)) == -1 and lib.satrans_afm_fwd(by(d), None, None, None) == -1, (B, Fn, D, A)
    for B, Fn, D, A in ((8, native.FM_MAX_FIELDS + 1, 8, 4), (8, 4, native.FM_MAX_DIM + 1, 4), (8, 4, 8, native.AFM_MAX_FACTOR + 1)):
        d = afm_desc(B, Fn, D, A)
        assert lib.satrans_afm_saved_floats(by(d)) == -2 and lib.satrans_last_error(), (B, Fn, D, A)
        assert lib.satrans_afm_workspace_floats(by(d)) == -2 and lib.satrans_afm_fwd(by(d), None, None, None) == -2
        assert lib.satrans_afm_bwd(by(d), None, None, None, None, None, None) == -2
    f = native.FMDesc()
    f.B, f.F, f.D = 8, native.FM_MAX_FIELDS + 1, 8
    assert lib.satrans_fm_fwd(by(f), None, None) == -2 and lib.satrans_bipool_bwd(by(f), None, None, None) == -2
    f.F = 4
    assert lib.satrans_fm_fwd(by(f), None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_bipool_fwd(by(f), None, None) == -1 and lib.satrans_fm_bwd(by(f), None, None, None) == -1
    # AFM's sizes over the sweep: saved is exactly B (P + D); the workspace does not grow with B P D
    for B, Fn, D, A in R.AFM_SWEEP + [(8192, 19, 32, 8), (1 << 20, 19, 32, 8)]:
        d = afm_desc(B, Fn, D, A)
        n_pairs = Fn * (Fn - 1) // 2
        assert lib.satrans_afm_saved_floats(by(d)) == B * (n_pairs + D)
        ws = lib.satrans_afm_workspace_floats(by(d))
        assert 0 < ws <= min(B, native.AFM_MAX_WORKGROUPS) * (D * A + 2 * A + D) and ws % (D * A + 2 * A + D) == 0
        assert lib.satrans_afm_fwd(by(d), None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_afm_bwd(by(d), None, None, None, None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    d = afm_desc(8192, 19, 32, 8)
    assert lib.satrans_afm_workspace_floats(by(d)) * 100 < 8192 * 171 * 32      # (745 workgroups of 304 floats)
    # the heads
    bad = [dict(B=0, Fn=4, D=8), dict(B=8, Fn=1, D=8), dict(B=8, Fn=4, D=0), dict(B=8, Fn=4, D=8, kind=2), dict(B=8, Fn=4, D=8, dense=-1),
           dict(B=8, Fn=4, D=8, dnn=(16, 0)), dict(B=8, Fn=4, D=8, kind=1, dnn=()), dict(B=8, Fn=4, D=8, use_fm=0, dnn=())]
    for kw in bad:
        d = head_desc(**kw)
        for rc in (lib.satrans_fmhead_saved_floats(by(d)), lib.satrans_fmhead_workspace_floats(by(d)),
                   lib.satrans_fmhead_fwd(by(d), None, None, None), lib.satrans_fmhead_bwd(by(d), None, None, None, None, None, None, None)):
            assert rc == -1, kw
    beyond = [dict(B=8, Fn=native.FM_MAX_FIELDS + 1, D=8), dict(B=8, Fn=4, D=native.FM_MAX_DIM + 1),
              dict(B=(1 << 31) - 1, Fn=4, D=8, dnn=(4096,))]      # (the last: the DNN's grid alone)
    for kw in beyond:
        d = head_desc(**kw)
        assert lib.satrans_fmhead_saved_floats(by(d)) == -2, kw
        assert lib.satrans_fmhead_fwd(by(d), None, None, None) == -2 and lib.satrans_last_error(), kw
    d = head_desc(8, 4, 8)
    d.n_dnn = native.MMOE_MAX_HIDDEN + 1
    assert lib.satrans_fmhead_saved_floats(by(d)) == -2 and b"hidden layers" in lib.satrans_last_error()
    B, Fn, D, dense, dnn = 131, 19, 32, 2, (128, 64)
    chunks = -(-B // native.MMOE_DW_ROW_CHUNK)
    for kind, first in ((native.FMHEAD_DEEPFM, Fn * D), (native.FMHEAD_NFM, D)):
        ld = first + dense
        d = head_desc(B, Fn, D, kind, 1, dense, dnn)
        assert lib.satrans_fmhead_saved_floats(by(d)) == B * ld + B * sum(dnn)
        parts = chunks * max(n * (k + 1) for n, k in zip(dnn + (1,), (ld,) + dnn))      # the largest layer's partials
        assert lib.satrans_fmhead_workspace_floats(by(d)) == B * ld + 2 * B * max(dnn) + parts
        assert lib.satrans_fmhead_fwd(by(d), None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_fmhead_bwd(by(d), None, None, None, None, None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    d = head_desc(B, Fn, D, native.FMHEAD_DEEPFM, 1, 0, ())
    assert lib.satrans_fmhead_saved_floats(by(d)) == 0 and lib.satrans_fmhead_workspace_floats(by(d)) == 0


@pytest.mark.parametrize("case", all_cases(), ids=case_id)
def test_premise_of_the_gpu_bounds(case):
    """The GPU tests hold the kernels to 2e-5 max|.| on results and 1e-4 max|g| + 5e-9 on gradients.  On every
    swept shape torch's own fp32 run of the literal form under autograd stays within a quarter of those bounds against the
    fp64 restatement."""
    kind, emb, dense, lin, up, P, n_dnn, use_fm, _ = draw_of(case)
    want_y, cache = R.forward(kind, emb.double(), None if dense is None else dense.double(), lin.double(), R.double(P), use_fm)
    want = R.flat(R.backward(up.double(), cache))
    y, got = autograd_against_explicit(kind, emb, dense, lin, up, P, n_dnn, use_fm, torch.float32)
    dev_y = float((y.double() - want_y).abs().max() / want_y.abs().max())
    print(f"[fm-premise] {case_id(case)}: logit {dev_y:.2e}")
    assert dev_y <= 2e-5 / 4
    if kind == "afm":
        a32 = literal_afm(emb, P)[1]
        dev_a = float((a32.double() - cache.afm.a).abs().max() / cache.afm.a.abs().max())
        print(f"[fm-premise] {case_id(case)}: normalized_att_score {dev_a:.2e}")
        assert dev_a <= 2e-5 / 4
    assert sorted(got) == sorted(want)
    for k in want:
        scale = float(want[k].abs().max())
        dev = float((got[k].double() - want[k]).abs().max())
        print(f"[fm-premise] {case_id(case)}: {k} {dev / max(scale, 1e-30):.2e}")
        assert dev <= (1e-4 * scale + 5e-9) / 4, k
