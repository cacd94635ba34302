"""What tests/test_embed_adam_gpu.py stands on, checked without a GPU: the fp64 restatements of tests/embed_adam_reference.py
against torch.optim, the run layouts against the boundary classes they are meant to place, and the premises of the GPU bounds."""
import numpy as np
import pytest
import torch

from tests import embed_adam_reference as E


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


@pytest.mark.parametrize("l2", [0.0, 1e-5])
def test_adam_step_is_torch_adam_in_fp64(l2):
    """Three steps of E.adam_step with unrounded constants against torch.optim.Adam in float64 (the regulariser's gradient 2 l2 p as
    its weight_decay): 1e-14 on p, m and v, relative to the element or, where exp_avg's lerp cancels, to the tensor's largest entry -
    the two differ by the order of a few float64 operations only."""
    lr, b1, b2, eps = 0.005, 0.9, 0.999, 1e-8
    p = torch.nn.Parameter(_randn(300, 7, seed=1, scale=0.05))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=2 * l2)
    q, m, v = p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)
    for t in (1, 2, 3):
        g = _randn(300, 7, seed=10 + t, scale=1e-3)
        p.grad = g.clone()
        opt.step()
        q, m, v = E.adam_step(q, m, v, g, E.hparams(lr, b1, b2, eps, l2, t, fp32=False))
        st = opt.state[p]
        for got, want in ((q, p.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-14, atol=1e-14 * float(want.abs().max()))


def test_hparams_round_where_the_host_rounds():
    """The float32 form: every constant is a float32 number, formed as engine._hparams and make_adamk form them - the weights 1 - beta
    from the float32 betas, which is not what torch applies to a float32 tensor."""
    lr, b1, b2, eps, l2, t = 0.005, 0.9, 0.999, 1e-8, 1e-5, 4
    h = E.hparams(lr, b1, b2, eps, l2, t)
    f = np.float32
    assert h.lr_over_bc1 == float(f(lr / (1 - b1 ** t))) and h.bc2_sqrt == float(f(np.sqrt(1 - b2 ** t)))
    assert h.w1 == float(f(1.0 - float(f(b1)))) and h.w2 == float(f(1.0 - float(f(b2)))) and h.beta2 == float(f(b2))
    ht = E.hparams(lr, b1, b2, eps, l2, t, weights="torch")
    assert ht.w1 == float(f(0.1)) and ht.w2 == float(f(0.001)) and ht._replace(w1=h.w1, w2=h.w2) == h
    assert 1.2e-5 < 1 - h.w2 / ht.w2 < 1.4e-5 and 2e-7 < h.w1 / ht.w1 - 1 < 3e-7
    assert h.l2 == float(f(l2)) and h.l2x2 == float(f(2) * f(l2)) and h.eps == float(f(eps))
    assert all(float(f(x)) == x for x in h)


@pytest.mark.parametrize("kind,make", [
    (E.SGD, lambda p, lr, a, eps: torch.optim.SGD([p], lr=lr)),
    (E.ADAGRAD, lambda p, lr, a, eps: torch.optim.Adagrad([p], lr=lr, eps=eps)),
    (E.RMSPROP, lambda p, lr, a, eps: torch.optim.RMSprop([p], lr=lr, alpha=a, eps=eps)),
])
def test_other_step_is_torch_in_fp64(kind, make):
    """Three steps of E.other_step with unrounded constants against torch.optim.SGD / Adagrad / RMSprop in float64: 1e-14 relative
    (to the element, or to the tensor's largest entry)."""
    lr, alpha, eps = 0.01, 0.99, 1e-8
    p = torch.nn.Parameter(_randn(300, 7, seed=2, scale=0.05))
    opt = make(p, lr, alpha, eps)
    q, s = p.detach().clone(), torch.zeros_like(p)
    for t in (1, 2, 3):
        g = _randn(300, 7, seed=20 + t, scale=1e-3)
        p.grad = g.clone()
        opt.step()
        q, s = E.other_step(kind, q, s, g, lr, alpha, eps, fp32=False)
        np.testing.assert_allclose(q.numpy(), p.detach().numpy(), rtol=1e-14, atol=1e-14 * float(p.detach().abs().max()))
        if kind != E.SGD:
            want = opt.state[p]["sum" if kind == E.ADAGRAD else "square_avg"]
            np.testing.assert_allclose(s.numpy(), want.numpy(), rtol=1e-14, atol=1e-14 * float(want.abs().max()))


def test_dense_grad_and_reg():
    rows = torch.tensor([2, 0, 2, 2], dtype=torch.int32)
    gemb = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]])
    assert E.dense_grad(rows, gemb, 4).tolist() == [[3.0, 4.0], [0.0, 0.0], [13.0, 16.0], [0.0, 0.0]]
    assert E.reg(torch.tensor([[1.0, 2.0], [3.0, 0.5]]), 1e-5) == float(np.float32(1e-5)) * 14.25


# ---- the layouts -------------------------------------------------------------------------------------------------------------------
def _classes(start, end):
    """The boundary classes of the run [start, end): which boundaries it crosses, starts before and ends on."""
    last = end - 1
    crossed = lambda unit: min(last // unit - start // unit, 2)
    out = {f"chunks_crossed_{crossed(E.K)}", f"supers_crossed_{crossed(E.S)}"}
    if start % E.K == E.K - 1: out.add("starts_on_last_of_chunk")
    if start % E.S == E.S - 1: out.add("starts_on_last_of_super")
    if end % E.K == 0: out.add("ends_on_chunk_end")
    if end % E.S == 0: out.add("ends_on_super_end")
    if end - start == E.K and start % E.K == 0: out.add("is_one_chunk")
    if end - start == E.S and start % E.S == 0: out.add("is_one_super")
    if end - start == 1 and start % E.S == 0: out.add("single_at_super_start")
    if end - start == 1 and start % E.S == E.S - 1: out.add("single_on_last_of_super")
    if end - start == 2 and start % E.S == E.S - 1: out.add("pair_straddles_super")
    return out


ALL_CLASSES = {f"{u}_crossed_{k}" for u in ("chunks", "supers") for k in (0, 1, 2)} | {
    "starts_on_last_of_chunk", "starts_on_last_of_super", "ends_on_chunk_end", "ends_on_super_end", "is_one_chunk", "is_one_super",
    "single_at_super_start", "single_on_last_of_super", "pair_straddles_super"}


def test_layouts_place_every_boundary_class():
    seen = {name: set().union(*(_classes(s, e) for s, e in E.run_bounds(name))) for name in E.LAYOUTS}
    assert set().union(*seen.values()) == ALL_CLASSES
    # ... and where the issue's table says they are
    assert {"is_one_chunk", "is_one_super", "ends_on_super_end", "supers_crossed_1"} <= seen["aligned"]
    assert (512, 1024) in E.run_bounds("aligned"), "a run of exactly two superchunks"
    assert {"starts_on_last_of_chunk", "single_at_super_start", "chunks_crossed_1", "supers_crossed_2"} <= seen["off_by_one"]
    assert any(e % E.K == 1 for _, e in E.run_bounds("off_by_one")) and any(e % E.S == 1 for _, e in E.run_bounds("off_by_one"))
    assert {"pair_straddles_super", "single_on_last_of_super"} <= seen["edge_of_super"]
    assert any((e - 1) // E.S - s // E.S == 3 for s, e in E.run_bounds("edge_of_super"))
    assert sum(E.LAYOUTS["one"]) == 1 and sum(E.LAYOUTS["short"]) < E.K and sum(E.LAYOUTS["distinct"]) % E.K != 0
    assert max(E.LAYOUTS["distinct"]) == 1
    (s, e), = E.run_bounds("one_row")
    assert (e - 1) // E.S - s // E.S == 19 and e % E.K != 0
    (_, mid), _ = E.run_bounds("two_giants")
    assert mid % E.K != 0


def test_layout_rows_are_sorted_runs_of_distinct_rows():
    with_ends, without = 0, 0
    for name, runs in E.LAYOUTS.items():
        rows, src = E.layout_rows(name)
        r = rows.numpy()
        assert r.size == sum(runs) and r.min() >= 0 and r.max() < E.R and bool((np.diff(r) >= 0).all())
        starts = np.flatnonzero(np.r_[True, np.diff(r) != 0])
        assert np.diff(np.r_[starts, r.size]).tolist() == list(runs), "one distinct row per run"
        assert sorted(src.tolist()) == list(range(r.size))
        assert r.size < 3 or src.tolist() != list(range(r.size))
        ends = (r[0] == 0, r[-1] == E.R - 1)
        assert ends in ((True, True), (False, False)) and ends[0] == (name in E.WITH_END_ROWS)
        with_ends += ends[0]
        without += not ends[0]
        again, again_src = E.layout_rows(name)
        assert torch.equal(again, rows) and torch.equal(again_src, src), "seeded"
    assert with_ends >= 1 and without >= 1 and E.R % 32 != 0


@pytest.mark.parametrize("D", E.DIMS)
def test_mixture_gives_every_stepping_body_two_workgroups(D):
    runs = E.LAYOUTS["mixture"]
    n = sum(runs)
    assert n >= 20000 and 2400 <= len(runs) <= 2600 and {33, 64, 700, 1500} <= set(runs)
    assert min(E.step_blocks(n, D)) >= 2, E.step_blocks(n, D)
    # the kernels' counts, spelled out
    assert E.step_blocks(20001, 16) == (2, 20, 313) and E.step_blocks(16384, 16) == (1, 16, 256)


# ---- premises of the GPU bounds ----------------------------------------------------------------------------------------------------
def _optim_flat_emulated(kind, p, s, g, lr, alpha, eps, contract):
    """optim_flat_kernel op by op in numpy float32.  contract: the state's multiply-add as one fma (emulated through float64, where
    the product of two float32 numbers is exact), otherwise as two rounded operations."""
    f = np.float32
    lr, alpha, eps = f(lr), f(alpha), f(eps)
    fma = (lambda a, b, c: (a.astype(np.float64) * b + c).astype(f)) if contract else (lambda a, b, c: a * b + c)
    s = fma(g, g, s) if kind == E.ADAGRAD else fma((f(1) - alpha) * g, g, s * alpha)
    return p + (-lr) * (g / (np.sqrt(s) + eps)), s


@pytest.mark.parametrize("contract", [True, False])
@pytest.mark.parametrize("kind", [E.ADAGRAD, E.RMSPROP])
def test_optim_flat_bounds_hold_for_a_float32_step(kind, contract):
    """The bounds tests/test_embed_adam_gpu.py sets on satrans_optim_flat are counted from the kernel's roundings (state: two roundings
    of positive terms, 1.01 * 2^-23 relative; parameter: 2^-21 |update| + 2^-23 |p|).  A float32 step taken op by op must sit inside
    them with room: measured here 0.47 of the parameter bound and 0.93 of 2^-23 on the state."""
    rng = np.random.RandomState(3)
    n = 20000
    p = (rng.randn(n) * 0.05).astype(np.float32)
    g = (rng.randn(n) * 1e-3).astype(np.float32)
    s = (rng.rand(n) * 1e-5).astype(np.float32)
    g[::7], s[::14] = 0.0, 0.0
    lr, alpha, eps = 0.01, 0.99, 1e-8
    got_p, got_s = _optim_flat_emulated(kind, p, s, g, lr, alpha, eps, contract)
    want_p, want_s = (x.numpy() for x in E.other_step(kind, *(torch.from_numpy(x) for x in (p, s, g)), lr, alpha, eps))
    state_ratio = float(np.max(np.abs(got_s - want_s) / np.maximum(2.0 ** -23 * want_s, 1e-300)))
    upd = np.abs(want_p - p.astype(np.float64))
    param_ratio = float(np.max(np.abs(got_p - want_p) / (2.0 ** -21 * upd + 2.0 ** -23 * np.abs(p))))
    print(f"kind {kind} contract {contract}: state {state_ratio:.3f} of 2^-23, parameter {param_ratio:.3f} of its bound")
    assert 0.0 < state_ratio <= 1.01 and 0.0 < param_ratio <= 1.0
    assert np.array_equal(got_p[(g == 0)], p[g == 0]) and not np.isnan(got_p).any()


@pytest.mark.parametrize("l2", [0.0, 1e-5])
def test_e32_of_the_many_step_bound(l2):
    """E.E32[l2] is what float32 arithmetic in torch's own operation order loses over the sequence: torch.optim.Adam in float32 on the
    CPU against the fp64 restatement of the same step (torch's weights), largest difference of any element after any step.  The pinned
    constant must be an upper bound of the measurement and within a factor two of it (torch builds differ in how they vectorise the
    step).  The GPU test's many-step bound is built from this constant, never from what the kernels give."""
    p0, grads = E.many_step_problem()
    assert 0.27 < float((grads == 0).float().mean()) < 0.33
    M = E.MANY
    p32 = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p32], lr=M["lr"], betas=(M["b1"], M["b2"]), eps=M["eps"], weight_decay=2 * l2)
    p, m, v = p0.double(), torch.zeros(M["n"], dtype=torch.float64), torch.zeros(M["n"], dtype=torch.float64)
    e32, at_T = 0.0, 0.0
    for t in range(1, M["T"] + 1):
        p32.grad = grads[t - 1].clone()
        opt.step()
        p, m, v = E.adam_step(p, m, v, grads[t - 1], E.hparams(M["lr"], M["b1"], M["b2"], M["eps"], l2, t, weights="torch"))
        at_T = float((p32.detach().double() - p).abs().max())
        e32 = max(e32, at_T)
    assert torch.equal(p, E.many_step_reference(l2, weights="torch"))
    print(f"l2 {l2}: e32 {e32:.3e} over all steps, {at_T:.3e} after the last; mean |p_T - p_0| {float((p - p0.double()).abs().mean()):.3e}")
    assert 0.5 * E.E32[l2] <= e32 <= E.E32[l2]


@pytest.mark.parametrize("l2", [0.0, 1e-5])
def test_what_the_weights_from_float32_betas_cost(l2):
    """A known deviation, measured: make_adamk forms the weights 1 - beta from the float32 betas of satrans_adam_hparams; torch forms
    them from the optimizer's doubles and rounds them where they meet a float32 tensor.  For beta2 = 0.999 the kernels' weight is
    1.3e-5 below torch's, so a second moment that the gradients have filled is 1.3e-5 low and an update 6.4e-6 large.  In fp64, over
    the many-step sequence, the two sets of weights end 1.8e-6 apart (3e-5 of the mean movement), ten times E32.  The GPU test holds
    the kernels to the restatement with their own weights, inside a bound made of E32 alone."""
    apart = float((E.many_step_reference(l2) - E.many_step_reference(l2, weights="torch")).abs().max())
    print(f"l2 {l2}: kernel weights against torch's weights after {E.MANY['T']} steps, in fp64: {apart:.3e}")
    assert 8 * E.E32[l2] < apart < 12 * E.E32[l2]


def test_what_the_rmsprop_weight_costs():
    """A known deviation, measured: optim_flat_kernel forms RMSprop's weight as 1.0f - alpha from the float32 alpha, torch applies
    float32(1 - alpha) from the double.  For alpha = 0.99 the kernel's weight is 9.3e-7 smaller, so the g^2 share of the state is
    9.3e-7 low (eight times the rounding bound of the state) and an update at most 4.7e-7 large.  E.other_step restates the kernel's
    weight, so the GPU bounds hold the kernel to its own weight."""
    f = np.float32
    kernel, as_torch = float(f(1) - f(0.99)), float(f(1.0 - 0.99))
    assert 9.2e-7 < 1 - kernel / as_torch < 9.4e-7
    g, s = torch.tensor([1e-3], dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    _, s_kernel = E.other_step(E.RMSPROP, s, s, g, 0.01, 0.99, 1e-8)
    assert float(s_kernel / (as_torch * g * g)) == pytest.approx(kernel / as_torch, rel=1e-12)
