"""TableAdam on the MI355X: the lazy forms against the every-row streaming step bit for bit (FeatureEmbedding's tables and, with
`linear_lazy`, LinearModel's 1-wide tables against the dense sweep), the result against the fp64 torch twin of
tests/table_adam_reference.py, resume, an out-of-range id, and the four guards.  No head is in the loop: the loss is linear
(table_adam_reference's docstring says why)."""
import pytest
import torch

from tests import table_adam_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(cols, fi, Pl, Pe, **kw):
    from satrans_amd import FeatureEmbedding, LinearModel, TableAdam
    fe, lin = FeatureEmbedding(cols, fi, device=DEV), LinearModel(cols, fi, device=DEV)
    fe.load_state_dict(Pe)
    lin.load_state_dict(Pl)
    kw.setdefault("lr", T.LR)
    return fe, lin, TableAdam([fe, lin], betas=T.BETAS, eps=T.EPS, **kw)


def one_step(fe, lin, opt, batch):
    X, W, c = (t.to(DEV) for t in batch)
    emb, _dense = fe(X)
    logit = lin(X)
    ((emb * W).sum() + (logit.squeeze(1) * c).sum()).backward()
    opt.step()
    assert all(p.grad is None for p in opt.param_groups[0]["params"])      # no dense gradient was built


def everything(fe, lin, opt):
    """After a flush: every table, weight and moment, on the host."""
    opt.flush()
    out = {f"fe.{k}": v.detach().cpu().clone() for k, v in fe.state_dict().items()}
    out.update({f"lin.{k}": v.detach().cpu().clone() for k, v in lin.state_dict().items()})
    sd = opt.state_dict()
    out["step"] = torch.tensor(sd["step"])
    for k, st in sd["state"].items():
        out[f"{k}.exp_avg"], out[f"{k}.exp_avg_sq"] = st["exp_avg"], st["exp_avg_sq"]
    return out


def run(D, batches_of, *, steps=T.STEPS, schedule=True, interrupt=False, **kw):
    cols, fi, _spec, Pl, Pe, batches = batches_of
    fe, lin, opt = build(cols, fi, Pl, Pe, **kw)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=T.HALVE_AFTER, gamma=0.5) if schedule else None
    for i, batch in enumerate(batches[:steps]):
        one_step(fe, lin, opt, batch)
        if sched is not None:
            sched.step()
        if interrupt and i + 1 == T.HALVE_AFTER:      # a forward without a backward, and a read of the tables, between two steps
            with torch.no_grad():
                fe.eval()
                fe(batches[-1][0].to(DEV))
                lin(batches[-1][0].to(DEV))
                fe.train()
            fe.state_dict()
    return everything(fe, lin, opt), (fe, lin, opt)


def assert_same_bits(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k, float((got[k].double() - want[k].double()).abs().max()))


_streaming = {}


def streaming(D, arith, l2, B=64, constant_a=False):
    """The oracle: lazy=False, linear_lazy=False; computed once per configuration and left unchanged."""
    key = (D, arith, l2, B, constant_a)
    if key not in _streaming:
        _streaming[key] = run(D, T.draw(D, B, constant_a), arith=arith, l2_reg_embedding=l2, l2_reg_linear=l2, lazy=False,
                              linear_lazy=False, flush_every=None)[0]
    return _streaming[key]


@pytest.mark.parametrize("flush_every", [4, None])
@pytest.mark.parametrize("l2", [0.0, 1e-5])
@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("D", [16, 32])
def test_lazy_is_the_streaming_step_bit_for_bit(D, arith, l2, flush_every):
    want = streaming(D, arith, l2)
    for linear_lazy in (False, True):
        got, _ = run(D, T.draw(D), interrupt=True, arith=arith, l2_reg_embedding=l2, l2_reg_linear=l2, lazy=True,
                     linear_lazy=linear_lazy, flush_every=flush_every)
        assert_same_bits(got, want, f"linear_lazy={linear_lazy}")
    assert int(want["step"]) == T.STEPS


@pytest.mark.parametrize("D, B, constant_a", [(128, 64, False), (16, 300, True)], ids=["d128", "b300_run_of_300"])
def test_lazy_is_the_streaming_step_at_d128_and_over_a_long_run(D, B, constant_a):
    want = streaming(D, "fast", 1e-5, B, constant_a)
    got, _ = run(D, T.draw(D, B, constant_a), interrupt=True, arith="fast", l2_reg_embedding=1e-5, l2_reg_linear=1e-5, lazy=True,
                 linear_lazy=True, flush_every=4)
    assert_same_bits(got, want, "lazy")


@pytest.mark.parametrize("l2", [0.0, 1e-5])
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_nine_steps_against_the_fp64_torch_twin(arith, l2):
    """Within 1e-4 max|p| + 5e-9 of torch.optim.Adam over the fp64 restatement (GRAD_REL / GRAD_ABS of test_input_gpu.py)."""
    L64, E64 = T.twin(16, l2, torch.float64)
    L32, E32 = T.twin(16, l2, torch.float32)
    got, _ = run(16, T.draw(16), arith=arith, l2_reg_embedding=l2, l2_reg_linear=l2, lazy=True, linear_lazy=True, flush_every=4)
    ours_e = {k: got[f"fe.{k}"] for k in E64}
    ours_l = {k: got[f"lin.{k}"] for k in L64}
    ratio = max(T.worst_ratio(ours_e, E64), T.worst_ratio(ours_l, L64))
    own = max(T.worst_ratio(E32, E64), T.worst_ratio(L32, L64))
    print(f"[table_adam] {arith}, l2 = {l2}: worst parameter {ratio:.2e} of its bound (torch's own fp32 run: {own:.2e})")
    assert ratio <= 1.0


def test_resume_from_the_three_state_dicts():
    D, kw = 16, dict(arith="fast", l2_reg_embedding=1e-5, l2_reg_linear=1e-5, lazy=True, linear_lazy=True, flush_every=4)
    drawn = T.draw(D)
    cols, fi, _spec, _Pl, _Pe, batches = drawn
    want, _ = run(D, drawn, steps=6, schedule=False, **kw)
    _, (fe, lin, opt) = run(D, drawn, steps=3, schedule=False, **kw)
    fe2, lin2, opt2 = build(cols, fi, lin.state_dict(), fe.state_dict(), **kw)
    opt2.load_state_dict(opt.state_dict())
    for batch in batches[3:6]:
        one_step(fe2, lin2, opt2, batch)
    assert_same_bits(everything(fe2, lin2, opt2), want, "resumed")


def test_out_of_range_id_raises_and_leaves_the_optimizer_consistent():
    D, l2 = 16, 1e-5
    cols, fi, _spec, Pl, Pe, batches = T.draw(D)
    want = streaming(D, "fast", l2)
    fe, lin, opt = build(cols, fi, Pl, Pe, arith="fast", l2_reg_embedding=l2, l2_reg_linear=l2, lazy=True, linear_lazy=True,
                         flush_every=None)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=T.HALVE_AFTER, gamma=0.5)
    for i, batch in enumerate(batches):
        if i == 3:      # rows are postponed by now: the replay in front of the failing gather is a real one
            bad = batch[0].clone()
            bad[5, fi["b"][0]] = 50.0
            with pytest.raises(IndexError):
                fe(bad.to(DEV))
            with pytest.raises(IndexError):
                lin(bad.to(DEV))
        one_step(fe, lin, opt, batch)
        sched.step()
    assert_same_bits(everything(fe, lin, opt), want, "after the IndexError")


def test_guards_fire_and_leave_the_state_usable():
    D, l2 = 16, 1e-5
    cols, fi, _spec, Pl, Pe, batches = T.draw(D)
    kw = dict(arith="fast", l2_reg_embedding=l2, l2_reg_linear=l2)
    want, _ = run(D, T.draw(D), steps=4, schedule=False, lazy=False, linear_lazy=False, flush_every=None, **kw)
    fe, lin, opt = build(cols, fi, Pl, Pe, lazy=True, linear_lazy=True, flush_every=None, **kw)

    def loss_of(batch):
        X, W, c = (t.to(DEV) for t in batch)
        return (fe(X)[0] * W).sum() + (lin(X).squeeze(1) * c).sum()

    with pytest.raises(RuntimeError, match="no pending gradient"):
        opt.step()
    one_step(fe, lin, opt, batches[0])
    loss_of(batches[1]).backward()                       # a second backward before step()
    with pytest.raises(RuntimeError, match="second backward"):
        loss_of(batches[1]).backward()
    with pytest.raises(RuntimeError, match="no pending gradient"):      # (both gradients were dropped)
        opt.step()
    early = loss_of(batches[3])                          # a forward made under t = 1 ...
    one_step(fe, lin, opt, batches[1])
    early.backward()                                     # ... whose backward arrives under t = 2
    with pytest.raises(RuntimeError, match="another step count"):
        opt.step()
    loss_of(batches[2]).backward()
    fe.to("cpu")                                         # a move after adoption
    with pytest.raises(RuntimeError, match="adopted on"):
        opt.step()
    fe.to(DEV)
    opt.step()
    one_step(fe, lin, opt, batches[3])
    assert opt.t == 4
    assert_same_bits(everything(fe, lin, opt), want, "after the guards")
