"""ESMMHead and WDLHead without a GPU: the fp64 restatement against the reference's recorded ESMM and WDL runs and against
autograd of the literal composition, the modules' state, the C ABI's new symbols and their argument validation, the dropout mask
contract on the host, and the premise of the GPU bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.satrans_oracle import dropout_keep
from satrans_amd import native
from tests import esmm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = {"esmm/two_layers": (2, (16, 8)), "esmm/one_layer": (2, (8,)), "wdl/two_layers": (1, (16, 8))}
SYMBOLS = ("satrans_esmm_saved_floats", "satrans_esmm_workspace_floats", "satrans_esmm_fwd", "satrans_esmm_bwd",
           "satrans_esmm_set_forward")
TILE, CHUNK = native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK
# the project's sibling bounds, element-wise
OUT_BOUND, GRAD_REL, GRAD_ABS = 2e-5, 1e-4, 5e-9
HEADS = ((2, "esmm"), (1, "wdl"))


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def state_of(fx):
    return {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}


def head_of(towers, C, hidden, **kw):
    from satrans_amd import ESMMHead, WDLHead
    return ESMMHead(C, hidden, **kw) if towers == 2 else WDLHead(C, hidden, **kw)


def literal(x, P, masks=None, p=0.0):
    """The reference's module composition (esmm.py:84-96 / wdl.py:75-79 with PredictionLayer's sigmoid(x + bias)) in torch ops,
    dropout as a mask times 1 / (1 - p) after each relu.  -> what the heads return: ESMM's probabilities, WDL's logit + bias."""
    towers = P["wf"].shape[0]
    outs = []
    for t in range(towers):
        h = x
        for l in range(len(P["w"])):
            h = F.relu(F.linear(h, P["w"][l][t], P["b"][l][t]))
            if masks is not None:
                h = h * masks[l][t].to(h.dtype) / (1.0 - p)
        outs.append(F.linear(h, P["wf"][t][None, :]))
    if towers == 1:
        return outs[0] + P["ob"]
    ctr_pred, cvr_pred = torch.sigmoid(outs[0] + P["ob"]), torch.sigmoid(outs[1] + P["ob"])
    return torch.cat([ctr_pred, ctr_pred * cvr_pred], -1)


def leaves(P, dtype):
    return {k: ([t.to(dtype).clone().requires_grad_(True) for t in v] if isinstance(v, list) else v.to(dtype).clone().requires_grad_(True))
            for k, v in P.items()}


def autograd_of_literal(x, dout, P, masks, p, dtype):
    L = leaves(P, dtype)
    xl = x.to(dtype).clone().requires_grad_(True)
    y = literal(xl, L, masks, p)
    (y * dout.to(dtype)).sum().backward()
    return y.detach(), R.flat({k: ([t.grad for t in v] if isinstance(v, list) else v.grad) for k, v in L.items()}, xl.grad)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_restatement_reproduces_every_fixture(name):
    """The recorded side is the reference's fp32 run, the restatement fp64 on the same fp32 inputs: within the sibling bounds."""
    towers, hidden = FIXTURES[name]
    fx = load(name)
    assert list(fx["keys"]) == list(R.state_from_params(R.params_from_state(state_of(fx), towers)))
    P = R.double(R.params_from_state(state_of(fx), towers))
    assert tuple(w.shape[1] for w in P["w"]) == hidden
    x, labels = torch.from_numpy(fx["dnn_input"]).double(), torch.from_numpy(fx["labels"]).double()
    out, cache = R.forward(x, P)
    y = out if towers == 2 else torch.sigmoid(out)
    loss = -(labels * torch.log(y) + (1 - labels) * torch.log(1 - y)).sum()
    dy = (y - labels) / (y * (1 - y))                              # d(summed BCE) / d(probability)
    dx, G = R.backward(dy if towers == 2 else dy * y * (1 - y), cache)
    assert float((y - torch.from_numpy(fx["y_pred"]).double()).abs().max()) <= OUT_BOUND * float(y.abs().max())
    assert abs(float(loss) - float(fx["loss"])) <= OUT_BOUND * abs(float(loss))
    got = R.state_from_params(G)
    got["dnn_input"] = dx
    for k, g in got.items():
        want = torch.from_numpy(fx[f"grad/{k}"]).double()
        assert want.shape == g.shape, k
        assert float((g - want).abs().max()) <= GRAD_REL * float(want.abs().max()) + GRAD_ABS, k


@pytest.mark.parametrize("towers,_", HEADS, ids=[h for _, h in HEADS])
@pytest.mark.parametrize("p", (0.0, 0.5, 0.1))
def test_explicit_backward_equals_autograd_of_the_literal_form(towers, _, p):
    case = R.SWEEP[2]
    x, dout, P, _used = R.draw(case, towers)
    masks = R.keep_masks(R.DROP_SEED, 1, case[0], case[2], towers, p) if p else None
    want_y, cache = R.forward(x.double(), R.double(P), masks, p)
    dx, G = R.backward(dout.double(), cache)
    want = R.flat(G, dx)
    y, got = autograd_of_literal(x, dout, P, masks, p, torch.float64)
    assert float((y - want_y).abs().max()) <= 1e-12
    assert sorted(got) == sorted(want)
    for k in want:
        assert float((got[k] - want[k]).abs().max()) <= 1e-11 * max(1.0, float(want[k].abs().max())), k
    if towers == 2:      # dout[:, 0] = 0 is the product rule alone, and it reaches both towers
        only = dout.double().clone()
        only[:, 0] = 0
        _, G1 = R.backward(only, cache)
        assert float(G1["wf"][0].abs().max()) > 0 and float(G1["wf"][1].abs().max()) > 0


@pytest.mark.parametrize("towers,head", HEADS, ids=[h for _, h in HEADS])
@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_premise_of_the_gpu_bounds(case, towers, head):
    """The GPU tests hold the kernels to 2e-5 max|.| on results and saved rows and 1e-4 max|g| + 5e-9 on gradients.
    On every SWEEP draw, without dropout and under the masks of both dropout runs, torch's own fp32 run of the literal form
    under autograd stays within a quarter of those bounds against the fp64 restatement (measured worst over the sweep: results
    1.8e-2 of their bound, gradients 2.1e-2 of theirs), and no pre-activation lies within 1e-4 of its kink."""
    B, C, hidden = case
    x, dout, P, _used = R.draw(case, towers)
    for p, step in ((0.0, 0),) + R.DROP_RUNS:
        masks = R.keep_masks(R.DROP_SEED, step, B, hidden, towers, p) if p else None
        assert float(R.min_margin(x, P, ((masks, p),) if p else ()).min()) >= R.KINK
        want_y, cache = R.forward(x.double(), R.double(P), masks, p)
        dx, G = R.backward(dout.double(), cache)
        want = R.flat(G, dx)
        y, got = autograd_of_literal(x, dout, P, masks, p, torch.float32)
        dev_y = float((y.double() - want_y).abs().max() / want_y.abs().max())
        worst = 0.0
        for k in want:
            scale = float(want[k].abs().max())
            dev = float((got[k].double() - want[k]).abs().max())
            worst = max(worst, dev / (GRAD_REL * scale + GRAD_ABS))
            assert dev <= (GRAD_REL * scale + GRAD_ABS) / 4, k
        print(f"[esmm-premise] {head} {R.case_id(case)} p={p}: result {dev_y / OUT_BOUND:.2e} of its bound, worst gradient "
              f"{worst:.2e} of its bound")
        assert dev_y <= OUT_BOUND / 4


def test_state_dict_is_the_references_and_loads_the_golden_entries():
    from satrans_amd import ESMMHead, WDLHead
    for name, (towers, hidden) in FIXTURES.items():
        fx = load(name)
        head = head_of(towers, fx["dnn_input"].shape[1], hidden)
        sd = head.state_dict()
        assert list(sd) == list(fx["keys"])
        assert [str(tuple(v.shape)) for v in sd.values()] == list(fx["shapes"])
        head.load_state_dict(state_of(fx))
        for k, v in state_of(fx).items():
            assert torch.equal(head.state_dict()[k], v), k
    fresh = ESMMHead(12, (16, 8), init_std=1e-4)
    assert float(fresh.ctr_dnn.linears[0].weight.detach().abs().max()) < 1e-3          # N(0, init_std)
    assert float(fresh.ctr_dnn.linears[0].bias.detach().abs().max()) > 1e-3            # nn.Linear's default
    assert float(fresh.cvr_dnn_final_layer.weight.detach().abs().max()) > 1e-3        # nn.Linear's default
    assert float(fresh.out.bias.detach().abs().max()) == 0.0
    assert not torch.equal(fresh.ctr_dnn.linears[0].weight, fresh.cvr_dnn.linears[0].weight)
    assert fresh.drop_row_offset == 0 and fresh.last_cvr is None and WDLHead(12).dnn_hidden_units == (256, 128)


@pytest.mark.parametrize("towers,head", HEADS, ids=[h for _, h in HEADS])
def test_module_refuses_what_is_not_built(towers, head):
    what = "ESMMHead" if towers == 2 else "WDLHead"
    with pytest.raises(NotImplementedError, match="relu"):
        head_of(towers, 8, (4,), dnn_activation="prelu")
    with pytest.raises(NotImplementedError, match="batch-norm"):
        head_of(towers, 8, (4,), dnn_use_bn=True)
    with pytest.raises(NotImplementedError, match="hidden layers"):
        head_of(towers, 8, (4,) * (native.MMOE_MAX_HIDDEN + 1))
    with pytest.raises(ValueError, match="empty"):
        head_of(towers, 8, ())
    for bad in (dict(C=0, hidden=(4,)), dict(C=8, hidden=(4, 0)), dict(C=8, hidden=(4,), dnn_dropout=1.0),
                dict(C=8, hidden=(4,), dnn_dropout=-0.1)):
        with pytest.raises(ValueError):
            head_of(towers, **bad)
    ok = head_of(towers, 8, (4,) * native.MMOE_MAX_HIDDEN, dnn_dropout=0.5)
    assert ok.dnn_dropout == 0.5
    with pytest.raises(ValueError, match="expected input"):
        ok(torch.zeros(3, 7))
    with pytest.raises(native.NativeError, match="no CPU fallback") as e:
        ok(torch.zeros(3, 8))
    assert what in str(e.value)
    assert ok._clock.step == 0      # refused before the clock moved


@pytest.mark.parametrize("towers,_", HEADS, ids=[h for _, h in HEADS])
def test_regularization_loss_is_the_restatements(towers, _):
    case = R.SWEEP[2]
    _x, _dout, P, _used = R.draw(case, towers)
    head = head_of(towers, case[1], case[2], l2_reg_dnn=0.03)
    head.load_state_dict(R.state_from_params(P))
    got, want = head.regularization_loss().detach(), R.l2_loss(R.double(P), 0.03)
    assert got.shape == (1,) and abs(float(got) - float(want)) <= 1e-6 * float(want)
    off = head_of(towers, case[1], case[2])
    assert float(off.regularization_loss()) == 0.0


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    H = native.MMOE_MAX_HIDDEN
    # B, C, towers, n_dnn, the widths, flags, drop_p, seed, step, row_offset + x + the parameter pointers
    assert ctypes.sizeof(native.ESMMDesc) == (4 + H + 5) * 4 + (1 + 2 * H + 2) * 8
    assert ctypes.sizeof(native.ESMMGrads) == (2 * H + 2) * 8
    # the field order of the two mirrors is the header's
    for struct, cls in (("satrans_esmm_desc", native.ESMMDesc), ("satrans_esmm_grads", native.ESMMGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in
                 re.findall(r"\*?\s*(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.split(None, 1)[1] if decl.split() else "")]
        names = [n for n in names if n not in ("float", "int32_t", "uint32_t", "const")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def esmm_desc(B, Cn, towers, hidden, flags=0, drop_p=0.0):
    d = native.ESMMDesc()
    d.B, d.C, d.towers, d.n_dnn, d.flags, d.drop_p = B, Cn, towers, len(hidden), flags, drop_p
    for l, n in enumerate(hidden[:native.MMOE_MAX_HIDDEN]):
        d.width[l] = n
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    by = ctypes.byref
    null = ctypes.POINTER(native.ESMMDesc)()
    assert lib.satrans_esmm_saved_floats(null) == -1 and lib.satrans_esmm_workspace_floats(null) == -1
    assert lib.satrans_esmm_fwd(null, None, None, None) == -1 and b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_esmm_bwd(null, None, None, None, None, None, None) == -1
    ok = (4, 8, 2, (16, 8))
    bad = []
    for at, values in ((0, (0, -1)), (1, (0, -8)), (3, ((), (4,) * 4, (16, 0), (-4,)))):
        for v in values:
            bad.append(ok[:at] + (v,) + ok[at + 1:])
    for args in bad:
        d = esmm_desc(*args)
        assert lib.satrans_esmm_saved_floats(by(d)) == -1, args
        assert lib.satrans_esmm_workspace_floats(by(d)) == -1, args
        assert lib.satrans_esmm_fwd(by(d), None, None, None) == -1 and b"bad sizes" in lib.satrans_last_error(), args
        assert lib.satrans_esmm_bwd(by(d), None, None, None, None, None, None) == -1, args
    for towers in (0, 3):
        assert lib.satrans_esmm_saved_floats(by(esmm_desc(4, 8, towers, (16,)))) == -1 and b"towers" in lib.satrans_last_error()
    for p in (-0.1, 1.0, float("nan")):
        assert lib.satrans_esmm_saved_floats(by(esmm_desc(4, 8, 2, (16,), native.TRAIN, p))) == -1
        assert b"drop_p" in lib.satrans_last_error()
    assert lib.satrans_esmm_saved_floats(by(esmm_desc(4, 8, 2, (16,), native.GATE))) == -1 and b"flags" in lib.satrans_last_error()
    # beyond 2^31 workgroups: decided from the sizes alone
    huge = esmm_desc(2 ** 31 - 1, 8, 2, (2 ** 20,))
    assert lib.satrans_esmm_saved_floats(by(huge)) == -2 and b"2^31 workgroups" in lib.satrans_last_error()
    assert lib.satrans_esmm_fwd(by(huge), None, None, None) == -2
    B, Cn = 300, 70
    chunks = -(-B // CHUNK)
    for towers in (1, 2):
        d = esmm_desc(B, Cn, towers, (48, 32, 8), native.TRAIN, 0.5)
        assert lib.satrans_esmm_saved_floats(by(d)) == B * towers * (48 + 32 + 8) + (2 * B if towers == 2 else 0)
        part = chunks * max(towers * 48 * (Cn + 1), towers * 32 * (48 + 1), towers * 8 * (32 + 1), towers * 8 + 1)
        assert lib.satrans_esmm_workspace_floats(by(d)) == 2 * B * towers * 48 + part
        assert lib.satrans_esmm_fwd(by(d), None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_esmm_bwd(by(d), None, None, None, None, None, None) == -1 and b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_esmm_set_forward(2) == -1 and b"mode 2" in lib.satrans_last_error()
    was = lib.satrans_esmm_set_forward(1)
    try:
        assert was in (0, 1) and lib.satrans_esmm_set_forward(0) == 1 and lib.satrans_esmm_set_forward(1) == 0
    finally:
        lib.satrans_esmm_set_forward(was)


def test_mask_contract_on_the_host():
    """The key of a mask bit is (seed, step, layer, site = tower, row, column): the two towers and successive steps get
    different masks, a row offset shifts the rows, and the keep rate over a 64 x 256 layer at p = 0.5 lies within 5 binomial
    standard deviations of 1 - p (5 * sqrt(0.25 / 16384) = 0.0195: [0.48, 0.52])."""
    rows, cols = np.arange(64)[:, None], np.arange(256)[None, :]
    m = {(step, t): dropout_keep(R.DROP_SEED, step, 0, t, rows, cols, 0.5) for step in (1, 2) for t in (0, 1)}
    for a in m:
        assert 0.48 <= m[a].mean() <= 0.52, a
        for b in m:
            if a < b:
                assert 0.4 <= (m[a] != m[b]).mean() <= 0.6, (a, b)
    assert (dropout_keep(R.DROP_SEED, 1, 1, 0, rows, cols, 0.5) != m[(1, 0)]).any()      # the layer is in the key
    masks = R.keep_masks(R.DROP_SEED, 1, 64, (256, 9), 2, 0.5)
    assert [tuple(t.shape) for t in masks] == [(2, 64, 256), (2, 64, 9)]
    assert np.array_equal(masks[0][1].numpy(), m[(1, 1)])
    shifted = R.keep_masks(R.DROP_SEED, 1, 8, (256,), 2, 0.5, row_offset=5)
    assert torch.equal(shifted[0][:, :8], masks[0][:, 5:13])
    assert dropout_keep(R.DROP_SEED, 1, 0, 0, rows, cols, 0.0).all()
    assert 0.88 <= dropout_keep(R.DROP_SEED, 2, 0, 0, rows, cols, 0.1).mean() <= 0.92      # 0.9 +- 5 * sqrt(0.09 / 16384)
