"""VarLenSparseFeat on the MI355X: the pooled gather and its backward (csrc/pool.hip) bit for bit against the fp32 restatement
of tests/varlen_reference.py, and the whole model - probabilities, gradients, Adam steps - against its fp64 composition of the
unchanged oracle, through the engine and the public API."""
import os

import numpy as np
import pytest
import torch

from tests import varlen_reference as V
from tests.test_varlen_golden import grad_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = [(c, ln) for c in ("sum", "mean", "max") for ln in (False, True)]


def _model(combiners, length=False, dense=False, **kw):
    m = V.build(DEV, combiners, length=length, dense=dense, **kw)
    m.eval()
    return m


def _tie(model):
    """Rows 1 and 2 of every varlen table equal: slots holding those ids tie under max."""
    with torch.no_grad():
        for n in ("h0", "h1", "h2"):
            if n in model.embedding_dict:
                w = model.embedding_dict[n].weight
                w[2] = w[1]


def layer_input_and_reference(model, X, ids):
    """(engine, its layer input [B, F, D] after a forward of X as float or int64 ids, the fp32 restatement's, the VarSpecs)"""
    spec, vs = V.spec_of(model)
    want = V.layer_input(V.params(model, torch.float32), X, spec, vs)
    Xd = X.to(DEV) if ids == "f32" else X.long().to(DEV)
    model(Xd)
    eng = model._engine
    return eng, eng.layer_outputs(X.shape[0])[0].cpu(), want, vs


@pytest.mark.parametrize("combiner,length", FORMS)
@pytest.mark.parametrize("ids", ["f32", "i64"])
def test_pooled_gather_is_bit_exact(combiner, length, ids):
    model = _model((combiner, combiner), length=length)
    _tie(model)
    X, _ = V.batch(model, 96, seed=1)
    eng, got, want, vs = layer_input_and_reference(model, X, ids)
    assert torch.equal(got, want)
    empty = V.slot_mask(X, vs[0]).sum(1) == 0
    assert bool(empty.any())
    if combiner == "max":                        # the reference's value of an all-padding list, kept
        assert bool((got[empty, 5] < -9e8).all())
    # slot rows: sparse ids, then every slot of every list (padding slots read their table's row 0)
    rows = eng._ws[96]["rows"].cpu().long()
    off = {n: lo for n, (lo, _) in model._table_rows.items()}
    assert torch.equal(rows[:, 5:8], X[:, vs[0].col:vs[0].col + 3].long() + off["h0"])


@pytest.mark.parametrize("where", ["valid", "padding"])
def test_out_of_range_id_raises(where):
    model = _model(("max",), length=True)
    X, _ = V.batch(model, 32, seed=2)
    _, vs = V.spec_of(model)
    lengths = X[:, vs[0].len_col].long()
    b = int(torch.nonzero(lengths == 1)[0]) if where == "valid" else int(torch.nonzero(lengths < 3)[0])
    X[b, vs[0].col + (0 if where == "valid" else 2)] = 23          # vocabulary_size of h0
    with pytest.raises(IndexError):
        model(X.to(DEV))
    X[b, vs[0].col + (0 if where == "valid" else 2)] = 1
    model(X.to(DEV))                                              # the status word was cleared


def check_slot_gradients(model, X):
    """The pooling backward of a random dx after a forward of X: every slot's row gradient equals torch autograd through
    `pool_rows` on an fp32 leaf of the gathered rows, bit for bit (5 sparse slots first: V.build's columns)."""
    B = X.shape[0]
    spec, vs = V.spec_of(model)
    model(X.to(DEV))
    eng = model._engine
    ws = eng.train_workspace(B, 1, False)
    g = torch.randn(B, eng.F, eng.D, generator=torch.Generator().manual_seed(5))
    gemb = eng._pool_backward(g.to(DEV), ws, B).cpu().view(B, eng.R, eng.D)
    assert torch.equal(gemb[:, :5], g[:, :5])                      # sparse slots: the row gradient is dx
    P = V.params(model, torch.float32)
    slot = 5
    for i, v in enumerate(vs):
        table = P[f"embedding_dict.{v.name}.weight"]
        E = table[X[:, v.col:v.col + v.maxlen].long()].clone().requires_grad_(True)
        V.pool_rows(E, V.slot_mask(X, v), v).backward(g[:, 5 + i])
        assert torch.equal(gemb[:, slot:slot + v.maxlen], E.grad), v.name
        slot += v.maxlen
    assert slot == eng.R


@pytest.mark.parametrize("combiner,length", FORMS)
def test_pool_backward_is_bit_exact_per_slot(combiner, length):
    model = _model((combiner, combiner), length=length)
    _tie(model)
    X, _ = V.batch(model, 64, seed=4)
    check_slot_gradients(model, X)


CASES = [("sum", False, False), ("mean", False, False), ("max", False, False), ("mean", True, False), ("max", False, True)]


def _grads_and_ref(combiner, length, dense, seed=7, B=48):
    """A model with a `combiner` field and a second one; the batch has padding, duplicates and empty lists (every fifth sample)."""
    model = _model((combiner, "sum" if combiner != "sum" else "max"), length=length, dense=dense)
    X, y = V.batch(model, B, seed=seed)
    spec, vs = V.spec_of(model)
    model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy")
    eng = model._require_engine()
    return model, eng, X, y, spec, vs


@pytest.mark.parametrize("combiner,length,dense", CASES)
def test_probabilities_and_gradients_match_fp64_composition(combiner, length, dense):
    """Same tolerances as smoke() / the golden gradient checks: logits 1e-5, BCE 2e-6 relative, every gradient to 5e-5 of its
    largest element - or, with an all-padding `max` list in the batch, to the wider bound whose measured fp32 noise figure
    tests/test_varlen_golden.py records (GRAD_REL_EMPTY_MAX)."""
    model, eng, X, y, spec, vs = _grads_and_ref(combiner, length, dense)
    P64 = V.params(model, torch.float64)
    prob = model(X.to(DEV)).cpu()
    p_ref, logit_ref = V.forward(P64, X.double(), spec, vs)
    scale = max(1.0, float(logit_ref.abs().max()))
    assert float((eng.last_logit().cpu().double() - logit_ref).abs().max()) < 1e-5 * scale
    assert float((prob.double() - p_ref).abs().max()) < 1e-5
    bce, reg, grads = eng.loss_and_grads(X.to(DEV), y.to(DEV))
    bce_ref, reg_ref, g_ref = V.loss_and_grads(P64, X.double(), y.double(), spec, vs)
    rel = grad_rel(model, X)
    assert abs(bce - bce_ref) <= 2e-6 * abs(bce_ref), (bce, bce_ref)
    assert reg == pytest.approx(reg_ref, rel=1e-5)
    for k, g in g_ref.items():
        if k not in grads:
            continue
        s = max(1e-6, float(g.abs().max()))
        np.testing.assert_allclose(grads[k].cpu().double().numpy(), g.numpy(), rtol=0, atol=rel * s + 1e-9, err_msg=k)
    for v in vs:                                                   # the varlen tables are trained
        assert f"embedding_dict.{v.name}.weight" in grads


@pytest.mark.parametrize("combiner,length,dense", CASES)
def test_adam_steps_match_fp64_composition(combiner, length, dense):
    """Two training steps (dropout off: eval mode) against two dense torch.optim.Adam steps in fp64 - the bounds of
    test_adam_steps_match_reference_golden: every element within 2 lr steps, the median of tensors with a real gradient within
    2e-3 lr steps."""
    model, eng, X, y, spec, vs = _grads_and_ref(combiner, length, dense, seed=11)
    P64 = V.params(model, torch.float64)
    _, _, g_ref = V.loss_and_grads(P64, X.double(), y.double(), spec, vs)
    steps, lr = 2, 0.005
    for _ in range(steps):
        eng.train_step(X.to(DEV), y.to(DEV))
    want = V.adam_steps(P64, X.double(), y.double(), spec, vs, lr, steps)
    got = V.params(model, torch.float64)
    for k, g in g_ref.items():
        diff = (got[k] - want[k]).abs().flatten()
        assert float(diff.max()) <= 2.0 * lr * steps + 1e-6, k
        if float(g.abs().max()) >= 1e-7:
            assert float(diff.median()) <= 2e-3 * lr * steps, (k, float(diff.median()))


def test_gradients_repeat_bitwise_and_lazy_adam_equals_streaming(monkeypatch):
    model, eng, X, y, _, _ = _grads_and_ref("max", False, False)
    _, _, g1 = eng.loss_and_grads(X.to(DEV), y.to(DEV))
    _, _, g2 = eng.loss_and_grads(X.to(DEV), y.to(DEV))
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    sds = []
    for lazy in ("1", "0"):
        monkeypatch.setenv("SATRANS_LAZY_ADAM", lazy)
        m, e, X, y, _, _ = _grads_and_ref("mean", False, False, seed=13)
        m.train()
        for s in range(4):
            Xs, ys = V.batch(m, 48, seed=20 + s)
            e.train_step(Xs.to(DEV), ys.to(DEV))
        sds.append({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    for k in sds[0]:
        assert torch.equal(sds[0][k], sds[1][k]), k


def test_all_padding_max_lists_run():
    model = _model(("max",))
    X, y = V.batch(model, 64, seed=8, empty_every=2)
    prob = model(X.to(DEV)).cpu()
    assert bool(torch.isfinite(prob).all())
    model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy")
    bce, _, grads = model._require_engine().loss_and_grads(X.to(DEV), y.to(DEV))
    assert np.isfinite(bce) and all(bool(torch.isfinite(g).all()) for g in grads.values())


def _dict_input(model, X):
    """Per-feature arrays as a user passes them: [N] ids, [N, maxlen] id lists."""
    out = {}
    for n, (lo, hi) in model.feature_index.items():
        block = X[:, lo:hi].numpy().astype(np.int64)
        out[n] = block[:, 0] if hi - lo == 1 else block
    return out


def test_public_api_fit_predict_evaluate_stream_bf16_and_attention():
    outs = []
    for stream in (False, True):
        model = V.build(DEV, ("max", "mean", "sum"), seed=5)
        X, y = V.batch(model, 700, seed=6)
        x = _dict_input(model, X)
        assert x["h0"].shape == (700, 3)
        model.stream_input = stream
        model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy")
        hist = model.fit(x, y.numpy(), batch_size=128, epochs=2, verbose=0)
        assert np.isfinite(hist.history["loss"]).all()
        outs.append((model, x, y, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    for k in outs[0][3]:
        assert torch.equal(outs[0][3][k], outs[1][3][k]), k           # streamed input == resident input, bit for bit
    model, x, y, _ = outs[0]
    p32 = model.predict(x, batch_size=256)
    assert p32.shape == (700, 1) and np.isfinite(p32).all()
    res = model.evaluate_domains(x, y.numpy(), batch_size=256)
    assert res
    model.set_forward_precision("bf16")
    p16 = model.predict(x, batch_size=256)
    assert float(np.abs(p16 - p32).max()) < 1e-2                     # bf16 products, fp32 accumulation
    model.set_forward_precision("fp32")
    st = model.attention_statistics(x, y.numpy(), batch_size=256)
    F = 5 + 3
    shape = st["sum"].shape
    assert shape[0] == model.domain_att_layer_num and shape[2:] == (3, model.att_head_num, F, F), shape
    model.capture_attention = True
    model.eval()
    model(torch.from_numpy(model._pack(x)[:64].astype(np.float32)).to(DEV))
    assert tuple(model.domain_int_layers[0].normalized_att_scores.shape) == (model.att_head_num, 64, F, F)


def _dp_worker(rank, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["SATRANS_FORCE_EXCHANGE"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=1)
    try:
        model = V.build(DEV, ("max",))
        model.compile(torch.optim.Adam(model.parameters(), lr=0.005), "binary_crossentropy")
        X, y = V.batch(model, 32)
        msg = ""
        try:
            model._require_engine().train_step(X.to(DEV), y.to(DEV))
        except NotImplementedError as e:
            msg = str(e)
        with open(os.path.join(out_dir, "msg.txt"), "w") as f:
            f.write(msg)
    finally:
        dist.destroy_process_group()


def test_data_parallel_forms_refuse_varlen_models(tmp_path):
    """The row-ownership and replicated forms exchange one row per field; a varlen model is refused there."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_dp_worker, args=(port, str(tmp_path)), nprocs=1, join=True)
    msg = (tmp_path / "msg.txt").read_text()
    assert "data-parallel" in msg and "VarLenSparseFeat" in msg, msg


def test_rows_through_an_indirection_read_the_same_values():
    """satrans_pool_gather_fwd with (src, src_rows): slot (b, r) read from src + src_rows[b * R + r] * D - here a permuted copy
    of the arena addressed through the permutation - gives the arena gather's layer input bit for bit, and the same rows."""
    import ctypes as C
    from satrans_amd import native as N
    model = _model(("max", "mean"), length=True)
    X, _ = V.batch(model, 80, seed=12)
    Xd = X.to(DEV)
    model(Xd)
    eng = model._engine
    ws = eng._ws[80]
    want, rows = ws["acts"][0].clone(), ws["rows"].clone()
    arena = model.embedding_arena
    perm = torch.randperm(arena.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    src = torch.empty_like(arena)
    src[perm] = arena                                             # arena row i lives at src row perm[i]
    src_rows = perm[rows.long()].to(torch.int32).contiguous()
    out = torch.empty_like(want)
    rows2 = torch.empty_like(rows)
    N.check(eng.lib.satrans_pool_gather_fwd(
        arena.data_ptr(), arena.shape[0], src.data_ptr(), src_rows.data_ptr(), eng._pool_fields, eng.F, eng.R, eng.Fv,
        Xd.data_ptr(), N.ID_F32, Xd.stride(0), 80, eng.D, out.data_ptr(), rows2.data_ptr(), ws["vmask"].data_ptr(),
        ws["argmax"].data_ptr(), eng.status.data_ptr(), eng._stream()), "satrans_pool_gather_fwd(src_rows)")
    assert torch.equal(out, want) and torch.equal(rows2, rows)
    eng.raise_if_bad_ids()
    assert eng.lib.satrans_pool_gather_fwd(arena.data_ptr(), arena.shape[0], None, src_rows.data_ptr(), eng._pool_fields, eng.F,
                                           eng.R, eng.Fv, Xd.data_ptr(), N.ID_F32, Xd.stride(0), 80, eng.D, out.data_ptr(),
                                           None, ws["vmask"].data_ptr(), ws["argmax"].data_ptr(), eng.status.data_ptr(),
                                           eng._stream()) == -1                # src_rows without src: refused
    del C


@pytest.mark.parametrize("combiner", ["max", "mean"])
def test_general_layer_path_matches_fp64_composition(monkeypatch, combiner):
    """The general layer path (csrc/layer_generic.hip) hands interior activations on in scenario-sorted order; layer 0's input and
    dx stay in the caller's order, which the pooling backward relies on.  Gradients and two Adam steps as on the fused path."""
    monkeypatch.setenv("SATRANS_GENERIC", "1")
    model, eng, X, y, spec, vs = _grads_and_ref(combiner, False, False, seed=17)
    assert eng.workspace(48)["generic"]
    P64 = V.params(model, torch.float64)
    bce, _, grads = eng.loss_and_grads(X.to(DEV), y.to(DEV))
    bce_ref, _, g_ref = V.loss_and_grads(P64, X.double(), y.double(), spec, vs)
    assert abs(bce - bce_ref) <= 2e-6 * abs(bce_ref)
    rel = grad_rel(model, X)
    for k, g in g_ref.items():
        if k in grads:
            s = max(1e-6, float(g.abs().max()))
            np.testing.assert_allclose(grads[k].cpu().double().numpy(), g.numpy(), rtol=0, atol=rel * s + 1e-9, err_msg=k)
    for _ in range(2):
        eng.train_step(X.to(DEV), y.to(DEV))
    want = V.adam_steps(P64, X.double(), y.double(), spec, vs, 0.005, 2)
    got = V.params(model, torch.float64)
    for k, g in g_ref.items():
        diff = (got[k] - want[k]).abs().flatten()
        assert float(diff.max()) <= 2.0 * 0.005 * 2 + 1e-6, k
        if float(g.abs().max()) >= 1e-7:
            assert float(diff.median()) <= 2e-3 * 0.005 * 2, (k, float(diff.median()))
