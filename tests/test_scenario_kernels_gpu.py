"""csrc/scenario.hip called straight through the C ABI against the fp64 restatements of tests/scenario_head_reference.py, inside
per-element bounds computed from the inputs (the module's docstring; tests/test_scenario_head_cpu.py proves torch's own fp32
stays within half of them on these very inputs): the table kernels over S / De / P on both sides of the 32 slices, the 8
sub-slices and the 32-column pass; the encoder-input kernels alone and as the chain inputs_fwd -> table_fwd -> table_bwd ->
inputs_bwd against autograd of the whole composition; relu; the ADD contract of every backward; reproducibility; refusals.

Pure outputs and the workspace start as NaN, accumulated outputs as zeros (bound check) or random values (ADD contract: the
result must be bit for bit prior + first result in fp32, since each kernel makes one `+=` per element)."""
import ctypes as C
import functools

import pytest
import torch

from satrans_amd import native as N
from tests import helpers as H
from tests import scenario_head_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                  # floats of NaN behind the workspace
NAN = float("nan")


def nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def stream():
    return N.stream_handle(torch.device(DEV))


def check(tag, what, got, want, bound, msg):
    """|got - want| <= bound element by element (bound 0: exact); the largest err / bound seen is printed under `tag`."""
    r = R.ratio(got.cpu(), want, bound)
    key = (tag, f"{what} err / bound")
    if r > H.WORST.get(key, -1.0):
        H.WORST[key] = r
        print(f"[{tag}] largest {key[1]} so far: {r:.3f} ({msg})")
    assert r <= 1.0, (msg, what, r)


def prior_like(t, seed):
    return torch.randn(t.shape, generator=torch.Generator().manual_seed(seed))


# ---- the table kernels ------------------------------------------------------------------------------------------------------
def table_fwd(emb, W, bias):
    S, De = emb.shape
    tab = nan(S, W.shape[0])
    rc = N.lib().satrans_scenario_table_fwd(emb.data_ptr(), W.data_ptr(), bias.data_ptr(), S, De, W.shape[0], tab.data_ptr(), stream())
    assert rc == 0, N.lib().satrans_last_error()
    return tab


def table_bwd(emb, W, g_tab, priors=None):
    """(g_emb, g_W, g_bias) on the device, accumulated onto `priors` (CPU tensors; None: zeros).  The workspace is exactly
    satrans_scenario_table_bwd_ws_floats floats of NaN with a guard band behind it that must stay NaN."""
    lib = N.lib()
    S, De = emb.shape
    P = W.shape[0]
    n_ws = int(lib.satrans_scenario_table_bwd_ws_floats(S, De))
    assert n_ws == S * R.K_SLICES * De
    ws = nan(n_ws + GUARD)
    outs = [torch.zeros(S, De), torch.zeros(P, De), torch.zeros(P)] if priors is None else priors
    g_emb, g_W, g_bias = (t.clone().to(DEV) for t in outs)
    rc = lib.satrans_scenario_table_bwd(emb.data_ptr(), W.data_ptr(), g_tab.data_ptr(), S, De, P, g_emb.data_ptr(), g_W.data_ptr(),
                                        g_bias.data_ptr(), ws.data_ptr(), stream())
    assert rc == 0, lib.satrans_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[n_ws:]).all()) and not bool(torch.isnan(ws[:n_ws]).any())
    return g_emb, g_W, g_bias


@functools.lru_cache(maxsize=None)
def table_case(case):
    """The draw and its fp64 reference, computed once and never written to."""
    ops = R.draw_table(case)
    return ops, R.table_reference(*ops)


@pytest.mark.parametrize("case", R.TABLE_CASES, ids=lambda c: "S%d-De%d-P%d" % c)
def test_table_forward_and_backward(case):
    (emb, W, bias, g_tab), (want, bound) = table_case(case)
    assert bool((emb == 0).any()) or emb.numel() < 3
    e, w, b, g = (t.to(DEV) for t in (emb, W, bias, g_tab))
    msg = "S=%d De=%d P=%d" % case
    tab = table_fwd(e, w, b)
    torch.cuda.synchronize()
    check("scenario", "tab", tab, want["tab"], bound["tab"], msg)
    g_emb, g_W, g_bias = table_bwd(e, w, g)
    check("scenario", "g_emb", g_emb, want["g_emb"], bound["g_emb"], msg)
    check("scenario", "g_W", g_W, want["g_W"], bound["g_W"], msg)
    check("scenario", "g_bias", g_bias, want["g_bias"], bound["g_bias"], msg)
    assert bool((g_emb.cpu()[emb <= 0] == 0).all())              # negatives, 0.0 and -0.0: exactly no gradient
    if emb.numel() >= 3:                                         # tab does not see them: the same bits with those entries at -1
        e2 = torch.where(emb <= 0, torch.full_like(emb, -1.0), emb).to(DEV)
        assert torch.equal(table_fwd(e2, w, b), tab)


REQUIRED = [(1, 1, 1), (240, 256, 33), (3, 32, 2080), (37, 20, 257)]


@pytest.mark.parametrize("case", REQUIRED, ids=lambda c: "S%d-De%d-P%d" % c)
def test_table_backward_adds_and_is_reproducible(case):
    (emb, W, bias, g_tab), _ = table_case(case)
    e, w, g = (t.to(DEV) for t in (emb, W, g_tab))
    first = [t.cpu() for t in table_bwd(e, w, g)]
    priors = [prior_like(t, 31 + i) for i, t in enumerate(first)]
    once = [t.cpu() for t in table_bwd(e, w, g, priors)]
    again = [t.cpu() for t in table_bwd(e, w, g, priors)]
    for name, f, p, a, b in zip(("g_emb", "g_W", "g_bias"), first, priors, once, again):
        assert torch.equal(a, p + f), name
        assert torch.equal(a, b), name
    assert torch.equal(once[0][emb <= 0], priors[0][emb <= 0])
    assert all(torch.equal(a, b.cpu()) for a, b in zip(first, table_bwd(e, w, g)))


# ---- the encoder's input rows, alone and as the chain -----------------------------------------------------------------------
class Chain:
    """One CHAIN_CASES draw on the device, with the pointer arrays of the C ABI."""

    def __init__(self, name):
        self.d = d = R.draw_chain(name)
        self.name = name
        self.tables = [t.to(DEV) for t in d["tables"]]
        self.index = d["index"].to(DEV) if d["index"] is not None else None
        self.lay = d["lay"].to(DEV) if d["pos"] else None
        self.role = d["role"].to(DEV) if d["pos"] else None          # [3, D]: the V row is never read
        self.ptrs = (C.c_void_p * d["C"])(*[t.data_ptr() for t in self.tables])
        self.rows = (C.c_int32 * d["C"])(*d["rows"])

    def inputs_fwd(self):
        d = self.d
        E = nan(d["LR"] * d["S"], d["De"])
        rc = N.lib().satrans_scenario_inputs_fwd(self.ptrs, N.ptr(self.index), d["C"], d["S"], d["D"], N.ptr(self.lay), N.ptr(self.role),
                                                 d["L"], E.data_ptr(), stream())
        assert rc == 0, N.lib().satrans_last_error()
        torch.cuda.synchronize()
        return E

    def priors(self, seed=None):
        """CPU priors of (g_tables..., g_lay [L,D], g_role [3,D]): zeros, or random with `seed`."""
        d = self.d
        shapes = [t.shape for t in d["tables"]] + ([(d["L"], d["D"]), (3, d["D"])] if d["pos"] else [])
        if seed is None:
            return [torch.zeros(s) for s in shapes]
        g = torch.Generator().manual_seed(seed)
        return [torch.randn(s, generator=g) for s in shapes]

    def inputs_bwd(self, g_E, priors):
        """(g_tables list, g_lay, g_role) as CPU tensors, accumulated onto `priors`."""
        d = self.d
        outs = [t.clone().to(DEV) for t in priors]
        g_ptrs = (C.c_void_p * d["C"])(*[t.data_ptr() for t in outs[:d["C"]]])
        g_lay, g_role = (outs[d["C"]], outs[d["C"] + 1]) if d["pos"] else (None, None)
        rc = N.lib().satrans_scenario_inputs_bwd(g_ptrs, self.rows, N.ptr(self.index), d["C"], d["S"], d["D"], g_E.data_ptr(), N.ptr(g_lay),
                                                 N.ptr(g_role), d["L"], stream())
        assert rc == 0, N.lib().satrans_last_error()
        torch.cuda.synchronize()
        outs = [t.cpu() for t in outs]
        return outs[:d["C"]], (outs[d["C"]] if d["pos"] else None), (outs[d["C"] + 1] if d["pos"] else None)


@functools.lru_cache(maxsize=None)
def chain_case(name):
    c = Chain(name)
    d = c.d
    role = d["role"][:2] if d["pos"] else None
    whole = R.chain_reference(d["tables"], d["index"], d["S"], d["lay"], role, d["W"], d["bias"], d["g_tab"])
    alone = R.inputs_bwd_reference(d["g_E"], d["index"], d["C"], d["S"], d["D"], d["L"], d["pos"], d["rows"])
    return c, whole, alone


def check_inputs_bwd(tag, c, got, want, bound, priors, msg):
    """g_tables, g_lay and the Q / K rows of g_role within their bounds of prior + want; the V row of g_role and every table
    row that no scenario names (bound 0) exactly the prior."""
    d = c.d
    g_tables, g_lay, g_role = got
    for i in range(d["C"]):
        check(tag, "g_tables", g_tables[i], priors[i].double() + want["g_tables"][i], bound["g_tables"][i], f"{msg} table {i}")
    named = [set(range(d["S"])) if d["index"] is None else set(d["index"][i].tolist()) for i in range(d["C"])]
    for i in range(d["C"]):
        for r in set(range(d["rows"][i])) - named[i]:
            assert torch.equal(g_tables[i][r], priors[i][r]), (msg, i, r)
    if d["pos"]:
        check(tag, "g_lay", g_lay, priors[d["C"]].double() + want["g_lay"], bound["g_lay"], msg)
        check(tag, "g_role", g_role[:2], priors[d["C"] + 1][:2].double() + want["g_role"], bound["g_role"], msg)
        assert torch.equal(g_role[2], priors[d["C"] + 1][2]), msg


@pytest.mark.parametrize("name", list(R.CHAIN_CASES))
def test_inputs_forward_and_backward_alone(name):
    c, (want, bound), (want1, bound1) = chain_case(name)
    d = c.d
    E = c.inputs_fwd()
    check("scenario", "E", E, want["E"], bound["E"], name)
    if d["C"] == 1:                                                     # one column: the row itself
        assert torch.equal(E.cpu()[:d["S"], :d["D"]], R.inputs_fwd(d["tables"], d["index"], d["S"], None, None))
    assert bool((E.cpu()[want["E"] == 0] == 0).all())
    g_E = d["g_E"].to(DEV)
    zeros = c.priors()
    first = c.inputs_bwd(g_E, zeros)
    check_inputs_bwd("scenario", c, first, want1, bound1, zeros, name + " alone")
    # the ADD contract and reproducibility
    priors = c.priors(seed=77)
    once, again = c.inputs_bwd(g_E, priors), c.inputs_bwd(g_E, priors)
    flat = lambda o: o[0] + ([o[1], o[2]] if d["pos"] else [])      # noqa: E731
    for f, p, a, b in zip(flat(first), priors, flat(once), flat(again)):
        assert torch.equal(a, p + f) and torch.equal(a, b), name


@pytest.mark.parametrize("name", list(R.CHAIN_CASES))
def test_chain_against_autograd_of_the_whole_composition(name):
    c, (want, bound), _ = chain_case(name)
    d = c.d
    assert R.kink_free(want["E"], bound["E"])
    W, bias, g_tab = (d[k].to(DEV) for k in ("W", "bias", "g_tab"))
    E = c.inputs_fwd()
    tab = table_fwd(E, W, bias)
    torch.cuda.synchronize()
    check("scenario chain", "tab", tab, want["tab"], bound["tab"], name)
    rows = d["LR"] * d["S"]
    g_E, g_W, g_bias = table_bwd(E, W, g_tab, [torch.zeros(rows, d["De"]), torch.zeros(d["P"], d["De"]), torch.zeros(d["P"])])
    check("scenario chain", "g_E", g_E, want["g_E"], bound["g_E"], name)
    check("scenario chain", "g_W", g_W, want["g_W"], bound["g_W"], name)
    check("scenario chain", "g_bias", g_bias, want["g_bias"], bound["g_bias"], name)
    zeros = c.priors()
    got = c.inputs_bwd(g_E, zeros)
    check_inputs_bwd("scenario chain", c, got, want, bound, zeros, name)
    priors = c.priors(seed=78)                                          # onto random contents: one += per element
    flat = lambda o: o[0] + ([o[1], o[2]] if d["pos"] else [])      # noqa: E731
    for f, p, a in zip(flat(got), priors, flat(c.inputs_bwd(g_E, priors))):
        assert torch.equal(a, p + f), name


def test_inputs_refusals():
    lib = N.lib()
    c = Chain("c2_pos_l3_d4")
    d = c.d
    nine = [torch.zeros(2, 4, device=DEV) for _ in range(9)]
    ptrs9 = (C.c_void_p * 9)(*[t.data_ptr() for t in nine])
    rows9 = (C.c_int32 * 9)(*([2] * 9))
    index9 = torch.zeros(9, 2, dtype=torch.int32, device=DEV)
    E, g_E = nan(2, 4), torch.zeros(2, 4, device=DEV)
    assert lib.satrans_scenario_inputs_fwd(ptrs9, index9.data_ptr(), 9, 2, 4, None, None, 1, E.data_ptr(), stream()) == -2
    assert b"9 scenario columns" in lib.satrans_last_error()
    assert lib.satrans_scenario_inputs_bwd(ptrs9, rows9, index9.data_ptr(), 9, 2, 4, g_E.data_ptr(), None, None, 1, stream()) == -2
    E2 = nan(d["LR"] * d["S"], d["De"])
    assert lib.satrans_scenario_inputs_fwd(c.ptrs, c.index.data_ptr(), d["C"], d["S"], d["D"], c.lay.data_ptr(), None, d["L"],
                                           E2.data_ptr(), stream()) == -1
    assert b"positions" in lib.satrans_last_error()
    g_lay = torch.zeros(d["L"], d["D"], device=DEV)
    g_ptrs = (C.c_void_p * d["C"])(*[t.data_ptr() for t in nine[:d["C"]]])
    assert lib.satrans_scenario_inputs_bwd(g_ptrs, c.rows, c.index.data_ptr(), d["C"], d["S"], d["D"], E2.data_ptr(), g_lay.data_ptr(),
                                           None, d["L"], stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(E).all()) and bool(torch.isnan(E2).all()) and not any(bool(t.any()) for t in nine) and not bool(g_lay.any())


# ---- 'onlyemb' --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_relu_forward_and_backward(n):
    lib = N.lib()
    g = torch.Generator().manual_seed(n)
    emb = torch.randn(n, generator=g)
    emb[::5] = 0.0
    emb[2::7] = -0.0
    g_tab, prior = torch.randn(n, generator=g), torch.randn(n, generator=g)
    e, gt = emb.to(DEV), g_tab.to(DEV)
    tab = nan(n + GUARD)
    assert lib.satrans_scenario_relu_fwd(e.data_ptr(), n, tab.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(tab[:n].cpu(), torch.relu(emb)) and bool(torch.isnan(tab[n:]).all())
    mask = emb > 0
    outs = []
    for p in (torch.zeros(n), prior, prior):
        buf = torch.cat([p, torch.full((GUARD,), NAN)]).to(DEV)
        assert lib.satrans_scenario_relu_bwd(e.data_ptr(), gt.data_ptr(), n, buf.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[n:]).all())
        outs.append(buf[:n].cpu())
    assert torch.equal(outs[0], torch.where(mask, g_tab, torch.zeros(n)))
    assert torch.equal(outs[1], torch.where(mask, prior + g_tab, prior)) and torch.equal(outs[1], prior + outs[0])
    assert torch.equal(outs[1], outs[2])
