"""The bf16 evaluation forward kernels (csrc/layer_fwd_bf16.hip: the single layer and the 1-4-layer stack with the head) against
the rounding model of tests/bf16_reference.py: the same operation in fp64 with the operands of every product rounded to bf16
exactly where the kernels round them.  Every layer is compared on its own - layer l of the model is applied to the kernel's
output of layer l - 1 and to the generated rows the kernel read - by the criterion tests/test_bf16_reference_cpu.py checks on
the model alone:
  tight tier   at most 0.5 % of the elements further than T = max(8 q99|m32 - m64|, 2e-6 max|m64|) from the fp64 model
  loose tier   every element within E = max|m64 - exact oracle|, the largest effect of the rounding on that tensor
  resolution   at least 5 % of the exact oracle's elements are outside T (else the case cannot tell bf16 from fp32)
Per case: the library's answers for the engine's descriptors before any layer kernel runs; the layer launches per layer and
on the logits; the stacked launch bit for bit the layer launches where it is built; the fp32 kernels FAIL the tight tier (the
bf16 kernels ran); back under "fp32" the earlier bits.  Cases (tests/bf16_reference.py, CASES): MOD 0 at D = 32 with F = 19 / 15
as constants under meta_mode QK / Q / K / none, two tables ('pos'), 'relu', run-time F = 11, 5, 6, 8, 33, 37, nothing modulated at
U = 48; (D, U, H) = (64, 128, 4) at F = 5, 13, 33, 64; gate and bilinear; the golden cases; stacks of 1 - 5 layers; one and two dense
columns behind the stacked head; B = 1; B = 3000 (more tiles than workgroups) with 37 of its rows forwarded alone; and the
refusals (D = 64 at F = 65, D = 64 with two tables at F = 49, (32, 8, 64)), which run the fp32 kernels' bits.
Run on an MI355X:  python -m pytest tests/test_bf16_model_gpu.py -m gpu -s   (-s prints the figures per group)

Batches hold 400 samples and the fields' vocabularies are larger than the batch (tests/bf16_reference.py, Shape.scenario_ids and
Shape.vocab say why: about one token in 300 carries a bf16 flip between two evaluation orders, a key-side flip moves its whole
sample by about T, the shares count elements, and a flip on an embedding row that many samples share counts once per sample).
No case is held on the loose tier only: resolution is 35 % or more on the CPU for every case, (64, 128, 4) at F = 64 included
(44 %), at the embedding scale of 300 every other synthetic test here uses; it took feeding every layer on its own.

Measured on the MI355X, all 42 cases passing (worst over a group's layers: share outside T, cap 0.5 % | err / T inside the tight
tier | err / E; beside it the fp32 model's share on the same inputs; logits: share | err / T | err / E):
  D = 32, F = 19 / 15 (QK / Q / K / none, pos, relu, 1 - 5 layers, dense, B = 1, B = 3000)
                            0.38 % | 1.00 | 0.49    fp32 model 0.20 %    logits 0 | 0.07 | 0.002
  D = 32, run-time F        0.18 % | 1.00 | 0.21    fp32 model 0.19 %    logits 0 | 0.06 | 0.002
  (64, 128, 4)              0.13 % | 1.00 | 0.22    fp32 model 0.12 %    logits 0 | 0.07 | 0.001
  gate / bilinear           0.04 % | 1.00 | 0.22    fp32 model 0.06 %    logits 0 | 0.07 | 0.002
  golden cases              0.05 % | 0.97 | 0.07    fp32 model 0.05 %    logits 0 | 0.07 | 0.002
  (the largest share, 0.38 %, is d32-F19-dense2 layer 0; every other layer is at 0.2 % or less.  CPU, model alone,
  tests/test_bf16_reference_cpu.py: the fp32 model's share 0.20 % / 0.19 % / 0.12 % / 0.05 % / 0.07 %, its err / E at most 0.35.)
With vocabularies of 5 - 60 ids per field, the other synthetic models' range, two layer-0 comparisons missed the cap at the same
B = 400: d32-F37-pos (1.46 %) and d32-F15-L1 (0.503 %), both within 0.29 E.  The first was traced to ONE operand: an element of
k0 = r(x) r(W_Key) of one embedding row lies 3.8e-6 of a bf16 step from a tie, the kernel rounds it the other way than fp64, and
every sample that holds the row moves by ~4e-6 in all its tokens; with that operand put on the other side in the model the
kernel's output of those samples is back within 6e-7.  No defect was found in the kernels' arithmetic.
One host-side defect was found and fixed: satrans_layer_fwd_bf16_supported accepted shapes whose images leave no room for one
sample's rows (REFUSED: d64-F49-pos), and the launch then refused them.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import satrans_oracle as O
from tests import bf16_reference as R
from tests.helpers import DEV, Case, SyntheticModel, build_model, note_worst

pytestmark = pytest.mark.gpu


class Built:
    """A case's model on the device, its parameters for the CPU model, and one batch."""

    def __init__(self, name):
        self.name = name
        if name in R.GOLDEN:
            c = Case(name)
            model = build_model(c, "cpu")
            by_ptr = {}
            self.state = {k: by_ptr.setdefault(v.data_ptr(), v.detach().clone()) for k, v in model.state_dict().items()}
            self.X, self.spec, self.shape = c.X, c.spec(), None
            model.to(DEV)
            model.device = DEV
            model.compile("adam", "binary_crossentropy")
            model.eval()
            self.model, self.eng = model, model._require_engine()
        else:
            s = self.shape = R.case_by_name(name)
            sm = SyntheticModel(s.D, s.H, s.U, s.F, L=s.L, flag=s.flag, meta_mode=s.mode, scen_ids=s.scenario_ids(),
                                n_dense=s.n_dense, emb=s.emb, gen=s.gen, seed=s.seed, vocab=s.vocab)
            self.state, self.X, self.spec = sm.state, sm.X, sm.spec
            self.eng = sm.on_device()
            self.model = sm.model
        self.L, self.B = self.spec.layer_num, self.X.shape[0]

    def descs(self, B):
        """(descriptors the engine hands the bf16 entry points, the scenario tables they point into)"""
        eng = self.eng
        ws, tabs = eng.workspace(B), eng.scenario_tables(grad=False)
        fuse = eng.fuse_gather or eng._x_src is not None
        return [eng._layer_desc(ws, l, B, None, tabs, False, fuse) for l in range(self.L)], tabs

    def forward(self, X, precision, stack=True, layers=False):
        """-> (probabilities, logits [B], every layer's output or None, whether the stacked launch ran, whether it ran the head)"""
        eng, model = self.eng, self.model
        model.set_forward_precision(precision)
        eng.bf16_stack = stack
        ran_head = []
        inner = eng._run_forward
        eng._run_forward = lambda *a, **k: ran_head.append(inner(*a, **k)) or ran_head[-1]
        try:
            prob = model(X.to(DEV)).clone().cpu()
        finally:
            del eng._run_forward
        try:
            logit = eng.last_logit().reshape(-1).clone().cpu()
            stacked = bool(eng._ws[X.shape[0]]["acts_stacked"])
            outs = [t.clone().cpu() for t in eng.layer_outputs(X.shape[0])] if layers else None
        finally:
            eng.bf16_stack = True
            model.set_forward_precision("fp32")
        return prob, logit, outs, stacked, bool(ran_head[0])

    def vectors(self, tabs, X):
        """per layer [vec_Q, vec_K, vec_V] [B, P]: the rows of the engine's tables the kernels read for these samples"""
        sid = X[:, self.spec.domain_cols[0]].long()
        tabs = tabs.cpu()
        pos = tabs.shape[0] > 1
        return [[tabs[l if pos else 0, 0][sid], tabs[l if pos else 0, 1 if pos else 0][sid], tabs[l if pos else 0, 0][sid]]
                for l in range(self.L)]


def desc_array(descs):
    return (C.POINTER(type(descs[0])) * len(descs))(*[C.pointer(d) for d in descs])


def group_of(name):
    if name in R.GOLDEN:
        return "golden"
    s = R.case_by_name(name)
    return "gate / bilinear" if s.mod else ("D = 64" if s.D == 64 else ("D = 32, F = 19 / 15" if s.F in (15, 19) else "D = 32, run-time F"))


def compare(name, what, got, m64, m32, ex, tight=True, resolution=True):
    c = R.criterion(got, m64, m32, ex)
    tag = f"bf16-model {group_of(name)}"
    kind = "logits" if what == "logits" else "layers"
    note_worst(tag, f"{kind}: share outside T", c["share"], f"{name} {what}")
    note_worst(tag, f"{kind}: err / T inside the tight tier", c["tight"], f"{name} {what}")
    note_worst(tag, f"{kind}: err / E", c["loose"], f"{name} {what}: T {c['T']:.2e} E {c['E']:.2e}")
    note_worst(tag, f"{kind}: m32 share outside T", c["m32_share"], f"{name} {what}")
    note_worst(tag, f"{kind}: m32 err / E", c["m32_loose"], f"{name} {what}")
    R.check_reference(c, (name, what), resolution=resolution and tight, m32=False)
    R.check_got(c, (name, what), tight=tight)
    return c


@pytest.mark.parametrize("name", [c.name for c in R.CASES] + R.GOLDEN)
def test_bf16_kernels_against_the_rounding_model(name):
    b = Built(name)
    eng, lib, s, L, B, X = b.eng, b.eng.lib, b.shape, b.L, b.B, b.X
    tight = s is None or s.tight
    want_stack = s is None or s.stack
    # 1. the route, before any layer kernel runs
    descs, tabs = b.descs(B)
    assert all(lib.satrans_layer_fwd_bf16_supported(C.byref(d)) == 1 for d in descs)
    assert lib.satrans_stack_fwd_bf16_supported(L, desc_array(descs)) == int(want_stack)
    if s is not None:
        assert (eng.D, eng.H, eng.F, eng.L) == (s.D, s.H, s.F, s.L) and (s.mod != 0 or eng.U == s.U)
        assert bool(descs[0].tab_q == descs[0].tab_k) == s.same_tab
        Tl, Ts = s.tiles()
        ids = X[:, 0].long().numpy()
        if B > 1:
            assert (ids >= 1).all() and R.full_then_partial(ids, Tl) and (not Ts or R.full_then_partial(ids, Ts)), (Tl, Ts)
        if name.endswith("B3000"):
            assert -(-B // Tl) > 256 and -(-B // Ts) > 256         # more tiles than workgroups: a workgroup walks several
    vecs = b.vectors(tabs, X)
    tri = R.Triple(b.state, X, b.spec, vecs)
    # the fp32 kernels
    p32, l32, outs32, _, _ = b.forward(X, "fp32", layers=True)
    # 2. layer launches: every layer against the model applied to the kernel's own output of the layer before
    _, lb, outs, stacked, _ = b.forward(X, "bf16", stack=False, layers=True)
    assert not stacked and len(outs) == L + 1
    assert torch.equal(outs[0], O.gather_fields(b.state, X, b.spec)), "the gathered rows are not the oracle's bit for bit"
    ex = None
    for l in range(L):
        m64, m32, ex = tri.layer(l, outs[l])
        compare(name, f"layer {l}", outs[l + 1], m64, m32, ex, tight)
        # 4. ... and the fp32 kernels' output of this layer is NOT within the tight tier of the model for its input
        c32 = R.criterion(outs32[l + 1], *tri.layer(l, outs32[l]))
        assert c32["share"] > 10 * R.TIGHT_SHARE, ("the fp32 kernels pass for the bf16 model", name, l, c32)
    lm64, lm32, lex = tri.logits(outs[L], ex)
    compare(name, "logits", lb, lm64, lm32, lex, tight, resolution=B >= 20)
    assert float((lb - l32).abs().max()) > 0.0, "bf16 and fp32 logits are identical: the bf16 kernels were not used"
    # 3. the stacked launch (with the head behind it): the layer launches bit for bit
    pb, ls, _, stacked, ran_head = b.forward(X, "bf16", stack=True)
    ran_stack = want_stack and L > 1 and not eng._ws[B]["generic"]
    assert stacked == ran_stack and ran_head == ran_stack, (stacked, ran_head)
    assert torch.equal(ls, lb), "stacked launch and layer launches differ"
    compare(name, "logits", ls, lm64, lm32, lex, tight, resolution=B >= 20)
    assert float((pb.reshape(-1).double() - torch.sigmoid(ls.double())).abs().max()) <= 1e-6
    if want_stack:
        # the stack entry point itself (the engine keeps one layer on the layer launch): rows out, bit for bit the layer launches'
        from satrans_amd import native as N
        b.forward(X, "fp32")                               # (the workspace's rows are the fp32 kernels' again)
        y = torch.zeros(B, eng.F, eng.D, device=DEV)
        descs, _ = b.descs(B)
        rc = lib.satrans_stack_fwd_bf16(L, desc_array(descs), y.data_ptr(), N.stream_handle(torch.device(DEV)))
        assert rc == 0, lib.satrans_last_error()
        assert torch.equal(y.cpu(), outs[L]), "satrans_stack_fwd_bf16 differs from the layer launches"
    # 5. back under fp32: the earlier bits
    p_again, l_again, _, _, _ = b.forward(X, "fp32")
    assert torch.equal(p_again, p32) and torch.equal(l_again, l32)
    if name.endswith("B3000"):
        # a sample's result does not depend on the tile it falls into: 37 of the rows forwarded alone, bit for bit per sample
        idx = torch.from_numpy(np.random.RandomState(5).choice(B, size=37, replace=False))
        for stack in (False, True):
            _, l37, outs37, _, _ = b.forward(X[idx], "bf16", stack=stack, layers=not stack)
            assert torch.equal(l37, lb[idx]), stack
            if outs37 is not None:
                assert all(torch.equal(a, w[idx]) for a, w in zip(outs37, outs))


@pytest.mark.parametrize("name", [c.name for c in R.REFUSED])
def test_what_the_bf16_kernels_refuse_runs_the_fp32_kernels(name):
    """The layer query answers 0 for the engine's descriptors, and the forward under "bf16" is the fp32 kernels' bits - with
    the stack switched on and off."""
    b = Built(name)
    eng, lib = b.eng, b.eng.lib
    descs, _ = b.descs(b.B)
    assert all(lib.satrans_layer_fwd_bf16_supported(C.byref(d)) == 0 for d in descs)
    assert lib.satrans_stack_fwd_bf16_supported(b.L, desc_array(descs)) == 0
    p32, l32, outs32, _, _ = b.forward(b.X, "fp32", layers=True)
    for stack in (True, False):
        pb, lb, outs, stacked, ran_head = b.forward(b.X, "bf16", stack=stack, layers=True)
        assert not stacked and not ran_head
        assert torch.equal(pb, p32) and torch.equal(lb, l32) and all(torch.equal(a, w) for a, w in zip(outs, outs32))
    # ... and they are the oracle's forward (the fp32 bound of tests/helpers.py: 2e-5 max(1, |logit|))
    ref = O.forward(b.state, b.X, b.spec)[1].reshape(-1)
    assert float((l32 - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
