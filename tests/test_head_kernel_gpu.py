"""csrc/head.hip called straight through the C ABI against the fp64 restatement of tests/scenario_head_reference.py, in the two
stages its docstring describes: logit and probability against the fp64 forward inside a bound computed from the inputs; loss,
dlogit, da, g_w, g_b against the kernel's own formulas evaluated in fp64 on the probability THE KERNEL STORED.  w[0] = 1 in
every draw, so da[:, 0] is the kernel's dlogit itself.  B on both sides of the 8 samples of a block and of kReduceGroups
blocks, FD on both sides of one 256-column pass, dense columns above one wave, a padded dense matrix with unsorted columns,
all three losses; the evaluation forms; satrans_head; saturated logits; the reduction alone; refusals; reproducibility.

`prob`, `logit`, `da` and the scratch start as NaN; the scratch is exactly satrans_head_scratch_floats floats with a NaN guard
band behind it."""
import ctypes as C
import functools
from collections import namedtuple

import pytest
import torch

from satrans_amd import native as N
from tests import scenario_head_reference as R
from tests.test_scenario_kernels_gpu import DEV, GUARD, NAN, check, nan, stream

pytestmark = pytest.mark.gpu
U = R.U
Out = namedtuple("Out", "rc prob logit da g_w g_b loss_sum scratch n_scratch")


def run(d, train=True, want_logit=True, entry="loss", priors=None, kind=None, with_scratch=True):
    """One satrans_head_loss (or satrans_head) on a draw; outputs as CPU tensors.  `priors` = (g_w, g_b, loss_sum) to
    accumulate onto (None: zeros).  Without `train`, y is NULL and the training outputs are handed over all the same."""
    lib = N.lib()
    B, FD, nd, ncol = d["B"], d["FD"], d["n_dense"], d["ncol"]
    a, w, bias, y = (d[k].to(DEV) for k in ("a", "w", "bias", "y"))
    dense = d["dense"].to(DEV) if nd else None
    cols = d["cols"].to(DEV) if nd else None
    prob, logit, da = nan(B), nan(B) if want_logit else None, nan(B, FD)
    n_s = int(lib.satrans_head_scratch_floats(B, FD, nd))
    assert n_s == R.ceil_div(B, R.SAMPLES_PER_BLOCK) * (ncol + 2)
    scratch = nan(n_s + GUARD)
    pw, pb, pl = priors if priors is not None else (torch.zeros(ncol), torch.zeros(1), torch.zeros(1, dtype=torch.float64))
    g_w, g_b, loss_sum = pw.clone().to(DEV), pb.clone().to(DEV), pl.clone().to(DEV)
    args = [a.data_ptr(), N.ptr(dense), d["stride"], N.ptr(cols), nd, B, FD, w.data_ptr(), bias.data_ptr(), prob.data_ptr(), N.ptr(logit),
            y.data_ptr() if train else None, loss_sum.data_ptr(), da.data_ptr(), g_w.data_ptr(), g_b.data_ptr(),
            scratch.data_ptr() if with_scratch else None]
    if entry == "loss":
        rc = lib.satrans_head_loss(*args, d["kind"] if kind is None else kind, stream())
    else:
        rc = lib.satrans_head(*args, stream())
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()      # noqa: E731
    return Out(rc, cpu(prob), cpu(logit), cpu(da), cpu(g_w), cpu(g_b), cpu(loss_sum), cpu(scratch), n_s)


def check_scratch(o, written=True):
    assert bool(torch.isnan(o.scratch[o.n_scratch:]).all())
    assert bool(torch.isnan(o.scratch[:o.n_scratch]).any()) != written and (written or bool(torch.isnan(o.scratch).all()))


def fp64_forward(d):
    return R.head_forward(d["a"].double(), d["dense"].double() if d["n_dense"] else None, d["cols"], d["w"].double(), d["bias"].double())


def check_two_stages(tag, d, o, msg):
    """Stage 1: logit, prob against the fp64 forward.  Stage 2: everything behind `prob` against the formulas on the stored prob."""
    w64 = d["w"].double()
    p64, z64, flat64 = fp64_forward(d)
    lb = R.logit_bound(flat64, w64, d["bias"].double(), d["FD"], d["n_dense"])
    check(tag, "logit", o.logit, z64, lb, msg)
    check(tag, "prob", o.prob, p64, R.prob_bound(lb), msg)
    want, bound = R.head_stage2(o.prob, d["y"], flat64, w64, d["kind"])
    name = R.LOSS_NAMES[d["kind"]]
    dlogit = o.da[:, 0]                                                  # w[0] = 1
    check(tag, f"{name} dlogit", dlogit, want["dlogit"], bound["dlogit"], msg)
    da64 = dlogit.double().unsqueeze(1) * w64[:d["FD"]]
    check(tag, "da", o.da, da64, 8 * U * da64.abs() + 1e-45, msg)
    check(tag, f"{name} loss_sum", o.loss_sum, want["loss_sum"].reshape(1), bound["loss_sum"].reshape(1), msg)
    check(tag, "g_w", o.g_w, want["g_w"], bound["g_w"], msg)
    check(tag, "g_b", o.g_b, want["g_b"].reshape(1), bound["g_b"].reshape(1), msg)
    check_scratch(o)
    return want, bound


@functools.lru_cache(maxsize=None)
def head_case(case):
    return R.draw_head(case)


def case_id(c):
    return "B%d-FD%d-nd%d-%s" % (c[0], c[1], c[2], R.LOSS_NAMES[c[3]])


# ---- 1. the sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=case_id)
def test_head_sweep(case):
    d = head_case(case)
    o = run(d)
    assert o.rc == 0, N.lib().satrans_last_error()
    check_two_stages("head", d, o, case_id(case))


# ---- 2., 3., 7. evaluation forms, satrans_head, the ADD contract, reproducibility -------------------------------------------
FORMS = [(9, 260, 65, R.MAE), (131, 256, 2, R.MAE), (269, 736, 2, R.BCE), (7, 252, 2, R.BCE), (8, 256, 1, R.MSE)]


@pytest.mark.parametrize("case", FORMS, ids=case_id)
def test_evaluation_forms_add_contract_and_reproducibility(case):
    d = head_case(case)
    first = run(d)
    assert first.rc == 0
    g = torch.Generator().manual_seed(5)
    priors = (torch.randn(d["ncol"], generator=g), torch.randn(1, generator=g), torch.randn(1, generator=g, dtype=torch.float64) * 100)
    # y = NULL: the same prob / logit bits, every training output untouched
    ev = run(d, train=False, priors=priors)
    assert ev.rc == 0
    assert torch.equal(ev.prob, first.prob) and torch.equal(ev.logit, first.logit)
    assert bool(torch.isnan(ev.da).all())
    check_scratch(ev, written=False)
    assert torch.equal(ev.g_w, priors[0]) and torch.equal(ev.g_b, priors[1]) and torch.equal(ev.loss_sum, priors[2])
    # logit = NULL, in both forms
    for train in (False, True):
        nl = run(d, train=train, want_logit=False)
        assert nl.rc == 0 and nl.logit is None and torch.equal(nl.prob, first.prob)
    # onto random contents: one += per element (loss_sum in fp64); twice from the same state: the same bits
    once, again = run(d, priors=priors), run(d, priors=priors)
    for name in ("g_w", "g_b", "loss_sum"):
        p, f, a, b = priors[("g_w", "g_b", "loss_sum").index(name)], getattr(first, name), getattr(once, name), getattr(again, name)
        assert torch.equal(a, p + f), name
        assert torch.equal(a, b), name
    for name in ("prob", "logit", "da"):
        assert torch.equal(getattr(once, name), getattr(first, name)) and torch.equal(getattr(once, name), getattr(again, name)), name
    assert torch.equal(once.scratch[:once.n_scratch], first.scratch[:first.n_scratch])
    if d["kind"] == R.BCE:                                               # satrans_head IS satrans_head_loss(..., SATRANS_LOSS_BCE)
        h = run(d, entry="head", priors=priors)
        assert h.rc == 0
        for name in ("prob", "logit", "da", "g_w", "g_b", "loss_sum", "scratch"):
            a, b = getattr(h, name), getattr(once, name)
            assert torch.equal(a[:h.n_scratch], b[:h.n_scratch]) if name == "scratch" else torch.equal(a, b), name
    else:                                                                # ... whatever loss the draw was made for
        h, bce = run(d, entry="head"), run(d, kind=R.BCE)
        assert h.rc == 0 and bce.rc == 0
        for name in ("prob", "logit", "da", "g_w", "g_b", "loss_sum"):
            assert torch.equal(getattr(h, name), getattr(bce, name)), name
        assert not torch.equal(bce.da, first.da)


# ---- 4. saturated rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=["alone", "mixed"])
def test_saturated_rows(mixed):
    """z in {+-20, +-90, +-104} x t in {0, 1}: torch's fp32 behaviour is the contract - p rounds to 1.0 from z = 17 on, the logs
    clamp at -100, (p - t) / max(pq, 1e-12) pq is 0 once pq is.  Against torch's fp32 CPU BCE and its backward fed the kernel's
    prob, both sides being within the stage-2 bound of the fp64 formulas on that prob (so within twice it of each other)."""
    d, rows = R.draw_saturated(mixed)
    o = run(d)
    assert o.rc == 0
    want, bound = check_two_stages("head saturated", d, o, "mixed" if mixed else "alone")
    for b, (z, t) in rows.items():
        assert float(o.logit[b]) == z
        if abs(z) >= 90:
            assert float(o.prob[b]) == (1.0 if z > 0 else 0.0), (z, float(o.prob[b]))
        if z > 0 or abs(z) >= 90:                                        # pq = 0: no gradient at all
            assert float(o.prob[b]) in (0.0, 1.0) and bool((o.da[b] == 0).all()), (z, t)
    loss_t, dl_t = R.torch_loss_and_dlogit(o.prob, d["y"])
    assert abs(float(o.loss_sum) - float(loss_t)) <= 2 * float(bound["loss_sum"])
    assert abs(float(o.g_b) - float(dl_t.double().sum())) <= 2 * float(bound["g_b"])
    assert float((o.da[:, 0].double() - dl_t.double()).abs().max()) <= 2 * R.DLOGIT_BOUND
    flat32 = R.head_forward(d["a"], d["dense"], d["cols"], d["w"], d["bias"])[2]
    assert bool(((o.g_w.double() - dl_t.double() @ flat32.double()).abs() <= 2 * bound["g_w"]).all())
    # every row with |z| >= 90 as a batch of its own: the loss exactly 100.0 or 0.0, every gradient exactly 0
    for b, (z, t) in rows.items():
        if abs(z) < 90:
            continue
        one = dict(d, a=d["a"][b:b + 1], dense=d["dense"][b:b + 1], y=d["y"][b:b + 1], B=1)
        o1 = run(one)
        assert o1.rc == 0
        assert float(o1.loss_sum) == (100.0 if (z > 0) != (t > 0) else 0.0), (z, t, float(o1.loss_sum))
        assert float(o1.g_b) == 0.0 and bool((o1.g_w == 0).all()) and bool((o1.da == 0).all()), (z, t)
        per, _ = R.torch_loss_and_dlogit(o1.prob, one["y"])
        assert float(per) == float(o1.loss_sum)


# ---- 5. the reduction alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 15, 16, 17, 1025])
def test_reduce_partials_alone(nblk):
    """Partial rows of small integers times 2^-10: every order of addition gives the same sum, so g_w, g_b (fp32) and loss_sum
    (fp64) must equal prior + the fp64 column sums exactly.  (The fused last-layer step feeds this reduction its own rows.)"""
    fn = N.lib().satrans_head_reduce_partials                            # internal: exported, not in native.SIGNATURES
    vp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for ncol in (1, 30, 31, 62):
        g = torch.Generator().manual_seed(1000 * nblk + ncol)
        ints = lambda *shape: torch.randint(-8, 9, shape, generator=g).double() * 2.0 ** -10      # noqa: E731
        partial, pw, pb, pl = ints(nblk, ncol + 2), ints(ncol), ints(1), ints(1)
        want = partial.sum(0)
        part = torch.cat([partial.float().reshape(-1), torch.full((GUARD,), NAN)]).to(DEV)
        g_w = torch.cat([pw.float(), torch.full((GUARD,), NAN)]).to(DEV)
        g_b, loss_sum = pb.float().to(DEV), pl.to(DEV)
        rc = fn(vp(part), C.c_int(nblk), C.c_int(ncol), vp(g_w), vp(g_b), vp(loss_sum), C.c_void_p(stream()))
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.equal(g_w[:ncol].cpu().double(), pw + want[:ncol]), (nblk, ncol)
        assert bool(torch.isnan(g_w[ncol:]).all())
        assert torch.equal(g_b.cpu().double(), pb + want[ncol]), (nblk, ncol)
        assert torch.equal(loss_sum.cpu(), pl + want[ncol + 1]), (nblk, ncol)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = N.lib()
    d = head_case((9, 260, 65, R.MAE))

    def refused(o, what):
        assert o.rc == -1, what
        assert bool(torch.isnan(o.prob).all()) and bool(torch.isnan(o.logit).all()) and bool(torch.isnan(o.da).all()), what
        assert bool(torch.isnan(o.scratch).all()) and not bool(o.g_w.any()) and float(o.g_b) == 0.0 and float(o.loss_sum) == 0.0, what

    odd = dict(d, FD=258, ncol=258 + 65, a=d["a"][:, :258].contiguous(), w=d["w"][:258 + 65].contiguous())
    refused(run(odd), "FD % 4 != 0")
    assert b"bad sizes" in lib.satrans_last_error()
    refused(run(d, kind=3), "loss kind 3")
    assert b"loss kind 3" in lib.satrans_last_error()
    refused(run(d, kind=-1), "loss kind -1")
    refused(run_without_dense(d), "dense columns without a matrix")
    assert b"dense columns" in lib.satrans_last_error()
    refused(run(d, with_scratch=False), "y without scratch")
    assert b"training outputs" in lib.satrans_last_error()
    # B = 0: nothing to size the buffers by, so the call is made by hand
    a, w, bias, prob = d["a"].to(DEV), d["w"].to(DEV), d["bias"].to(DEV), nan(4)
    dense, cols = d["dense"].to(DEV), d["cols"].to(DEV)
    assert lib.satrans_head_loss(a.data_ptr(), dense.data_ptr(), d["stride"], cols.data_ptr(), d["n_dense"], 0, d["FD"], w.data_ptr(),
                                 bias.data_ptr(), prob.data_ptr(), None, None, None, None, None, None, None, R.BCE, stream()) == -1
    assert lib.satrans_head_scratch_floats(0, d["FD"], d["n_dense"]) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(prob).all())


def run_without_dense(d):
    """n_dense > 0 with dense = NULL (the column list is still given)."""
    lib = N.lib()
    B, FD, nd, ncol = d["B"], d["FD"], d["n_dense"], d["ncol"]
    a, w, bias, y, cols = (d[k].to(DEV) for k in ("a", "w", "bias", "y", "cols"))
    prob, logit, da = nan(B), nan(B), nan(B, FD)
    n_s = int(lib.satrans_head_scratch_floats(B, FD, nd))
    scratch = nan(n_s + GUARD)
    g_w, g_b, loss_sum = torch.zeros(ncol, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
    rc = lib.satrans_head_loss(a.data_ptr(), None, d["stride"], cols.data_ptr(), nd, B, FD, w.data_ptr(), bias.data_ptr(), prob.data_ptr(),
                               logit.data_ptr(), y.data_ptr(), loss_sum.data_ptr(), da.data_ptr(), g_w.data_ptr(), g_b.data_ptr(),
                               scratch.data_ptr(), d["kind"], stream())
    torch.cuda.synchronize()
    return Out(rc, prob.cpu(), logit.cpu(), da.cpu(), g_w.cpu(), g_b.cpu(), loss_sum.cpu(), scratch.cpu(), n_s)
