"""The rounding model of the bf16 forward kernels (tests/bf16_reference.py) on its own, without a device: with every rounding
point off it is the oracle; rbf16 is round-to-nearest-even; on every case of tests/test_bf16_model_gpu.py, at that module's
sizes, the model alone meets the conditions the shared criterion puts on a reference (fp32 against fp64 model inside the tight
tier, the exact oracle far enough outside it); and the criterion tells four subtle faults from the unmutated model.
-s prints the figures per case (the CPU columns of the table in tests/test_bf16_model_gpu.py)."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import satrans_oracle as O
from tests import bf16_reference as R
from tests.helpers import Case, SyntheticModel, note_worst


@functools.lru_cache(maxsize=None)
def built(name):
    """(state fp32, X, spec, Triple, the model's own fp32 layer outputs) of a case of R.CASES / R.GOLDEN"""
    if name in R.GOLDEN:
        c = Case(name)
        state, X, spec = c.tensors("param"), c.X, c.spec()
    else:
        s = R.case_by_name(name)
        sm = SyntheticModel(s.D, s.H, s.U, s.F, L=s.L, flag=s.flag, meta_mode=s.mode, scen_ids=s.scenario_ids(), n_dense=s.n_dense,
                            emb=s.emb, gen=s.gen, seed=s.seed, vocab=s.vocab)
        state, X, spec = sm.state, sm.X, sm.spec
    tri = R.Triple(state, X, spec)
    return state, X, spec, tri, R.forward(state, X, spec)[0]


def group_of(name):
    return "golden" if name in R.GOLDEN else name.split("-")[0] + ("-gate/bilinear" if R.case_by_name(name).mod else "")


# ---- the model with every switch off is the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["QK", "Q", "K", ""])
@pytest.mark.parametrize("flag", ["sota", "sota-pos", "sota-gate", "sota-bilinear", "relu"])
def test_all_switches_off_is_the_oracle(flag, mode):
    sm = SyntheticModel(32, 4, 64, 7, L=2, flag=flag, meta_mode=mode, B=9, n_dense=1)
    P = R.as_double(sm.state)
    trace = {}
    _, logit = O.forward(P, sm.X, sm.spec, trace=trace)
    outs, got = R.forward(P, sm.X, sm.spec, R.ALL_OFF)
    assert torch.equal(outs[0], trace["att_input"])
    for l in range(2):
        assert float((outs[l + 1] - trace[f"out{l}"]).abs().max()) <= 1e-12
    assert float((got - logit.reshape(-1)).abs().max()) <= 1e-12
    # ... and with them on it is not (every flag has at least one rounding point)
    assert float((R.forward(P, sm.X, sm.spec)[0][1] - outs[1]).abs().max()) > 1e-7


def test_each_switch_is_a_rounding_point_of_its_own():
    """Each switch alone moves the oracle's output: the MetaNet's six, and the two that bilinear adds.  (Alone, because a later
    rounding point can swallow the whole effect of an earlier one.)"""
    for flag, names in (("sota", ["weights", "generated", "x", "meta_in", "hidden", "attn_out"]), ("sota-bilinear", ["generated", "bilinear_q"])):
        sm = SyntheticModel(32, 4, 64, 7, L=1, flag=flag, B=9)
        P = R.as_double(sm.state)
        base = R.forward(P, sm.X, sm.spec, R.ALL_OFF)[0][1]
        for n in names:
            on = R.forward(P, sm.X, sm.spec, dataclasses.replace(R.ALL_OFF, **{n: True}))[0][1]
            assert float((on - base).abs().max()) > 0.0, (flag, n)


# ---- rbf16 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rbf16_is_round_to_nearest_even(dtype):
    u = 2.0 ** -7                                    # spacing of bf16 in [1, 2)
    cases = [
        (1.0, 1.0), (1.0 + u, 1.0 + u), (-3.140625, -3.140625), (0.0, 0.0),                       # representable: unchanged
        (1.0 + u / 2, 1.0), (1.0 + 3 * u / 2, 1.0 + 2 * u), (1.0 + 5 * u / 2, 1.0 + 2 * u),       # ties go to the even mantissa
        (-(1.0 + u / 2), -1.0), (-(1.0 + 3 * u / 2), -(1.0 + 2 * u)),
        (1.0 + u / 2 + 2.0 ** -20, 1.0 + u), (1.0 + 3 * u / 2 - 2.0 ** -20, 1.0 + u), (-(1.0 + u / 2 + 2.0 ** -20), -(1.0 + u)),
        (2.0 - u / 2, 2.0),                                                                        # a tie that carries into the exponent
        (2.0 ** -133, 2.0 ** -133), (3 * 2.0 ** -133, 3 * 2.0 ** -133),                           # subnormals of bf16 (quantum 2^-133)
        (1.5 * 2.0 ** -133, 2 * 2.0 ** -133), (2.5 * 2.0 ** -133, 2 * 2.0 ** -133), (0.5 * 2.0 ** -133, 0.0),
        (-1.5 * 2.0 ** -133, -2 * 2.0 ** -133), (1.25 * 2.0 ** -133, 2.0 ** -133), (1.75 * 2.0 ** -133, 2 * 2.0 ** -133),
        (2.0 ** -126 - 2.0 ** -134, 2.0 ** -126),                                                  # the largest subnormal's tie
    ]
    x = torch.tensor([c[0] for c in cases], dtype=dtype)
    want = torch.tensor([c[1] for c in cases], dtype=dtype)
    got = R.rbf16(x)
    assert got.dtype == dtype and torch.equal(got, want), [(c, float(g)) for c, g in zip(cases, got) if c[1] != float(g)]


def test_rbf16_from_fp64_rounds_once():
    """A double just beside a bf16 tie rounds to the tie in fp32; rounding that again would go to the even neighbour whichever
    side the double was on."""
    u = 2.0 ** -7
    x = torch.tensor([1.0 + u / 2 + 2.0 ** -40, 1.0 + u / 2 - 2.0 ** -40, 1.0 + 3 * u / 2 + 2.0 ** -40, 1.0 + 3 * u / 2 - 2.0 ** -40,
                      -(1.0 + u / 2 + 2.0 ** -40)], dtype=torch.float64)
    want = torch.tensor([1.0 + u, 1.0, 1.0 + 2 * u, 1.0 + u, -(1.0 + u)], dtype=torch.float64)
    assert torch.equal(R.rbf16(x), want)
    g = torch.Generator().manual_seed(1)
    r = torch.randn(200000, generator=g, dtype=torch.float64)
    got = R.rbf16(r)
    assert torch.equal(got, got.bfloat16().double()) and float(((got - r).abs() / r.abs()).max()) <= 2.0 ** -8


# ---- the conditions on the reference alone, for every GPU case ---------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in R.CASES] + R.GOLDEN)
def test_the_reference_alone_meets_the_criterion(name):
    """Per layer, fed the fp32 model's own output of the layer before (the stand-in for the kernel's): the fp32 model leaves at
    most 2e-3 of its elements outside T and none outside E, and at least 5 % of the exact oracle's elements are outside T.
    A case marked tight=False is held to the loose tier only and says why in R.CASES."""
    state, X, spec, tri, outs = built(name)
    tight = name in R.GOLDEN or R.case_by_name(name).tight
    ex_last = None
    for l in range(spec.layer_num):
        m64, m32, ex = tri.layer(l, outs[l])
        c = R.criterion(None, m64, m32, ex)
        tag = f"bf16-model cpu {group_of(name)}"
        note_worst(tag, "m32 share outside T", c["m32_share"], f"{name} layer {l}")
        note_worst(tag, "m32 err / E", c["m32_loose"], f"{name} layer {l}")
        note_worst(tag, "1 - resolution", 1.0 - c["resolution"], f"{name} layer {l}: T {c['T']:.2e} E {c['E']:.2e}")
        R.check_reference(c, (name, l), resolution=tight)
        ex_last = ex
    c = R.criterion(None, *tri.logits(outs[-1], ex_last))
    note_worst(f"bf16-model cpu {group_of(name)}", "logits: m32 err / E", c["m32_loose"], f"{name}: T {c['T']:.2e} E {c['E']:.2e}")
    note_worst(f"bf16-model cpu {group_of(name)}", "logits: 1 - resolution", 1.0 - c["resolution"], name)
    assert c["m32_share"] == 0.0 and c["m32_loose"] <= 1.0, (name, c)
    if X.shape[0] >= 20 and tight:
        assert c["resolution"] >= R.RESOLUTION, (name, c)


@pytest.mark.parametrize("s", R.CASES, ids=lambda s: s.name)
def test_every_case_has_a_full_tile_followed_by_a_partial_one(s):
    """The tile sizes restated from the launchers' choosers; ids 1..3 with id 0 unused (an empty scenario)."""
    ids = s.scenario_ids()
    assert ids.min() >= 1 and ids.max() == 3 or len(ids) == 1
    Tl, Ts = s.tiles()
    assert Tl >= 1 and (Ts >= 1) == s.stack
    if len(ids) > 1:
        counts = np.bincount(ids, minlength=4)
        assert counts[0] == 0 and len(ids) in (400, 3000), len(ids)
        for T in (Tl, Ts or Tl):
            assert any(c > T and (T == 1 or c % T) for c in counts), (T, counts)
    if s.name.endswith("B3000"):
        assert -(-3000 // Ts) > 256 and -(-3000 // Tl) > 256      # more tiles than workgroups (one per CU)


# ---- the criterion catches subtle faults -------------------------------------------------------------------------------------
MUTATIONS = [
    ("relu(h) into W2 not rounded", dict(R=dataclasses.replace(R.ALL_ON, hidden=False)), ["d32-F19-QK", "d64-F13"]),
    ("two contraction indices of W2 swapped in the last K-step", dict(fault=R.FAULT_W2_SWAP), ["d32-F11", "d64-F13"]),
    ("K-side MetaNet LayerNorm from the Q-side vectors", dict(fault=R.FAULT_K_LN_FROM_Q), ["d32-F19-pos", "d64-F13-pos"]),
    ("padded keys counted into the softmax sum", dict(fault=R.FAULT_PAD_KEYS), ["d32-F11", "d32-F19-QK", "d64-F13"]),
]


@pytest.mark.parametrize("what,kw,names", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_the_criterion_tells_a_mutated_model_from_the_model(what, kw, names):
    """The mutated model, evaluated in fp32 as a kernel would, is put through the criterion in the kernel's place: it must fail
    at every layer, where the unmutated fp32 model passes."""
    for name in names:
        state, X, spec, tri, outs = built(name)
        for l in range(spec.layer_num):
            m64, m32, ex = tri.layer(l, outs[l])
            assert not R.fails(R.criterion(m32, m64, m32, ex)), (what, name, l)
            mutant = R.layer(state, l, outs[l], tri.v32[l], spec, kw.get("R", R.ALL_ON), kw.get("fault", ""))
            c = R.criterion(mutant, m64, m32, ex)
            print(f"[bf16-model cpu] {what}: {name} layer {l}: share outside T {c['share']:.3f}, err / E {c['loose']:.2f}")
            assert R.fails(c), (what, name, l, c)


# ---- what the layer query answers for a shape whose images do not fit LDS ------------------------------------------------------
def test_the_layer_query_refuses_what_the_launch_cannot_hold():
    """(64, 128, 4) with two generated tables ('pos'): the images of both roles leave room for 48 token rows, so F = 49..64 has no
    tile.  The query must say so (the engine then runs the fp32 kernels) instead of leaving it to the launch to fail."""
    from satrans_amd import native as N
    lib = N.lib()

    def desc(F_, two, D=64, U=128):
        d = N.LayerDesc()
        d.B, d.F, d.D, d.H, d.U, d.S, d.flags = 21, F_, D, 4, U, 4, N.META_Q | N.META_K
        d.order, d.seg, d.tab_q, d.tab_k, d.tab_stride = 0x1000, 0x2000, 0x3000, 0x4000 if two else 0x3000, 2 * D * U
        return d

    for F_ in (5, 48, 49, 64, 65):
        for two in (False, True):
            fits = R.tile_samples(F_, 64, not two, 0) > 0 and F_ <= 64
            assert fits == (F_ <= (48 if two else 64))
            assert lib.satrans_layer_fwd_bf16_supported(C.byref(desc(F_, two))) == int(fits), (F_, two)
    for F_ in (288, 289, 320, 321):                                # D = 32: the same rule (one table: 320 fields, two: 288)
        for two in (False, True):
            want = int(R.tile_samples(F_, 32, not two, 0) > 0)
            assert want == int(F_ <= (288 if two else 320))
            assert lib.satrans_layer_fwd_bf16_supported(C.byref(desc(F_, two, 32, 64))) == want, (F_, two)
